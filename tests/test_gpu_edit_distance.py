"""Token edit distance on the GPU (acai_edit_distance / ops.edit_distance) against the CPU dynamic program of tests/edit_distance_reference.py,
and what is built on it: the GRPO token reward (train/grpo.py) and the symbol error rate (utils.symbol_error_rate).  Distances are integers:
every comparison is exact."""
import numpy as np
import pytest
import torch

from conftest import VOCAB, load_golden
from decode_support import _models
from edit_distance_reference import edit_distance

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 767, 1536]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from acai_omr_amd import _lib
    _lib.lib()
    return "cuda"


def _vocab():
    toks = [ln.strip() for ln in open(VOCAB) if ln.strip()]
    return len(toks), toks.index("<pad>")


def _pack(rows, width=None, fill=0):
    """list of 1-D integer sequences -> (int64 (N, width) padded with `fill`, int32 (N,) lengths), on the CPU"""
    lens = [len(r) for r in rows]
    out = torch.full((len(rows), width if width is not None else max(lens + [1])), fill, dtype=torch.int64)
    for i, r in enumerate(rows):
        out[i, :lens[i]] = torch.as_tensor(np.asarray(r, dtype=np.int64))
    return out, torch.tensor(lens, dtype=torch.int32)


def _gpu(dev, preds, tgts, group=1):
    from acai_omr_amd import ops
    p, pl = _pack(preds)
    t, tl = _pack(tgts)
    out = ops.edit_distance(p.to(dev), pl.to(dev), t.to(dev), tl.to(dev), group=group)
    assert out.dtype == torch.int32 and out.shape == (len(preds),)
    return out.cpu().tolist()


@pytest.mark.parametrize("vocab", [2, 4, 227])
def test_random_pairs_over_the_length_grid(dev, vocab):
    """Every (pred length, target length) of LENGTHS x LENGTHS in one launch."""
    rng = np.random.default_rng(100 + vocab)
    preds, tgts = [], []
    for lp in LENGTHS:
        for lt in LENGTHS:
            preds.append(rng.integers(0, vocab, size=lp))
            tgts.append(rng.integers(0, vocab, size=lt))
    got = _gpu(dev, preds, tgts)
    want = [edit_distance(a, b) for a, b in zip(preds, tgts)]
    bad = [(len(a), len(b), g, w) for a, b, g, w in zip(preds, tgts, got, want) if g != w]
    print(f"vocab {vocab}: {len(got)} pairs, {len(bad)} differ")
    assert not bad, bad[:10]


@pytest.mark.parametrize("lp,lt", [(4096, 4096), (4096, 1), (1, 4096)])
def test_longest_rows(dev, lp, lt):
    rng = np.random.default_rng(lp + lt)
    a, b = rng.integers(0, 4, size=lp), rng.integers(0, 4, size=lt)
    got = _gpu(dev, [a], [b])
    want = edit_distance(a, b)
    print(f"{lp} x {lt}: {got[0]} vs {want}")
    assert got == [want]


def test_structured_pairs(dev):
    rng = np.random.default_rng(5)
    preds, tgts, known = [], [], []
    for n in (1, 64, 300, 1000):
        row = rng.integers(0, 227, size=n)
        preds.append(row), tgts.append(row.copy()), known.append(0)                       # identical
        cut = n // 3
        preds.append(row[:cut]), tgts.append(row), known.append(n - cut)                  # a prefix of the other
        preds.append(row), tgts.append(row[:cut]), known.append(n - cut)
        preds.append(row), tgts.append(row[::-1].copy()), known.append(None)              # reversed
        for k in (1, 5, 63):
            preds.append(row), tgts.append(np.roll(row, k)), known.append(None)           # rotated by k
    # a block of 100 tokens deleted in the middle; the block's tokens (1000 ... 1099) occur nowhere else, so nothing shorter than deleting
    # each of them turns the long row into the short one, and 100 deletions do
    left, right = rng.integers(0, 227, size=400), rng.integers(0, 227, size=350)
    full = np.concatenate([left, np.arange(1000, 1100), right])
    preds.append(full), tgts.append(np.concatenate([left, right])), known.append(100)
    preds.append(np.concatenate([left, right])), tgts.append(full), known.append(100)
    got = _gpu(dev, preds, tgts)
    want = [edit_distance(a, b) for a, b in zip(preds, tgts)]
    assert got == want, (got, want)
    for g, k in zip(got, known):
        assert k is None or g == k


def test_group_equals_repeated_targets(dev):
    rng = np.random.default_rng(8)
    G, B = 8, 5
    tgts = [rng.integers(0, 227, size=int(rng.integers(0, 700))) for _ in range(B)]
    preds = [rng.integers(0, 227, size=int(rng.integers(0, 768))) for _ in range(B * G)]
    grouped = _gpu(dev, preds, tgts, group=G)
    repeated = _gpu(dev, preds, [t for t in tgts for _ in range(G)])
    assert grouped == repeated
    assert grouped == [edit_distance(p, tgts[i // G]) for i, p in enumerate(preds)]


def test_padding_is_ignored_and_masks_equal_lengths(dev):
    from acai_omr_amd import ops
    rng = np.random.default_rng(9)
    preds = [rng.integers(0, 227, size=n) for n in (0, 3, 64, 65, 200, 511)]
    tgts = [rng.integers(0, 227, size=n) for n in (5, 0, 64, 300, 199, 512)]
    want = [edit_distance(a, b) for a, b in zip(preds, tgts)]
    outs = []
    for fill_p, fill_t in ((0, 0), (1, 1), (7, 200), (2 ** 31 - 1, -1), (-5, 2 ** 40)):
        p, pl = _pack(preds, width=600, fill=fill_p)
        t, tl = _pack(tgts, width=520, fill=fill_t)
        outs.append(ops.edit_distance(p.to(dev), pl.to(dev), t.to(dev), tl.to(dev)).cpu().tolist())
    # random valid token ids past the lengths
    p, pl = _pack(preds, width=600)
    t, tl = _pack(tgts, width=520)
    junk_p, junk_t = torch.from_numpy(rng.integers(0, 227, size=tuple(p.shape))), torch.from_numpy(rng.integers(0, 227, size=tuple(t.shape)))
    pm = torch.arange(p.shape[1])[None, :] < pl[:, None]
    tm = torch.arange(t.shape[1])[None, :] < tl[:, None]
    p, t = torch.where(pm, p, junk_p), torch.where(tm, t, junk_t)
    outs.append(ops.edit_distance(p.to(dev), pl.to(dev), t.to(dev), tl.to(dev)).cpu().tolist())
    # the same rows with bool prefix masks in the place of the lengths, on either side and on both
    outs.append(ops.edit_distance(p.to(dev), pm.to(dev), t.to(dev), tm.to(dev)).cpu().tolist())
    outs.append(ops.edit_distance(p.to(dev), pm.to(dev), t.to(dev), tl.to(dev)).cpu().tolist())
    outs.append(ops.edit_distance(p.to(dev), pl.to(dev), t.to(dev), tm.to(dev)).cpu().tolist())
    for o in outs:
        assert o == want, (o, want)


def test_token_ids_near_int32_max(dev):
    top = 2 ** 31 - 1
    rng = np.random.default_rng(10)
    a = top - rng.integers(0, 3, size=300)            # ids in {2^31 - 3, 2^31 - 2, 2^31 - 1}
    b = top - rng.integers(0, 3, size=280)
    c = a.copy()
    c[17] = top if a[17] != top else top - 1          # one substitution between neighbouring ids
    d = np.where(a == top, 0, a)                      # 2^31 - 1 against 0: ids that differ in every bit but the sign
    preds, tgts = [a, a, a, np.array([top]), np.array([top])], [b, c, d, np.array([top]), np.array([top - 1])]
    got = _gpu(dev, preds, tgts)
    want = [edit_distance(x, y) for x, y in zip(preds, tgts)]
    assert got == want and got[1] == 1 and got[3] == 0 and got[4] == 1 and got[2] == int((a == top).sum())


def test_operand_checks(dev):
    from acai_omr_amd import ops
    ok = torch.zeros(2, 8, dtype=torch.int64, device=dev)
    ln = torch.full((2,), 8, dtype=torch.int32, device=dev)
    wide = torch.zeros(2, 4097, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError):
        ops.edit_distance(wide, ln, ok, ln)
    with pytest.raises(ValueError):
        ops.edit_distance(ok, ln, wide, ln)
    full = torch.zeros(2, 4096, dtype=torch.int64, device=dev)   # 4096 itself is accepted
    assert ops.edit_distance(full, ln, ok, ln).cpu().tolist() == [0, 0]
    with pytest.raises(ValueError):
        ops.edit_distance(ok, ln, ok[:1], ln[:1], group=3)       # R != Rt * group
    with pytest.raises(TypeError):
        ops.edit_distance(ok.int(), ln, ok, ln)
    with pytest.raises(TypeError):
        ops.edit_distance(ok, ln.long(), ok, ln)
    with pytest.raises(RuntimeError):
        ops.edit_distance(ok.cpu(), ln, ok, ln)
    # lengths beyond the row are clamped to it on the device, negative ones to 0
    over = torch.tensor([100, -3], dtype=torch.int32, device=dev)
    assert ops.edit_distance(ok, over, ok, ln).cpu().tolist() == [0, 8]


def test_repeatable_and_graph_replay(dev):
    from acai_omr_amd import ops
    rng = np.random.default_rng(11)
    preds = [rng.integers(0, 4, size=int(rng.integers(0, 768))) for _ in range(48)]
    tgts = [rng.integers(0, 4, size=int(rng.integers(300, 700))) for _ in range(6)]
    p, pl = (x.to(dev) for x in _pack(preds))
    t, tl = (x.to(dev) for x in _pack(tgts))
    want = torch.tensor([edit_distance(a, tgts[i // 8]) for i, a in enumerate(preds)], dtype=torch.int32)
    first = ops.edit_distance(p, pl, t, tl, group=8)
    second = ops.edit_distance(p, pl, t, tl, group=8)
    assert torch.equal(first.cpu(), want) and torch.equal(first, second)
    out = torch.full((48,), -1, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ops.edit_distance(p, pl, t, tl, group=8, out=out)   # (the code object is loaded: nothing but the launch is left to capture)
        s.synchronize()
        g = ops.Graph()
        g.begin()
        try:
            ops.edit_distance(p, pl, t, tl, group=8, out=out)
        finally:
            g.end()
        out.fill_(-1)
        g.launch()
        s.synchronize()
        assert torch.equal(out, first)
        # the lengths are read by the replayed launch, not baked in: shorten every rollout and replay
        pl.copy_(torch.clamp(pl - 5, min=0))
        g.launch()
        s.synchronize()
    want2 = torch.tensor([edit_distance(a[:max(len(a) - 5, 0)], tgts[i // 8]) for i, a in enumerate(preds)], dtype=torch.int32)
    assert torch.equal(out.cpu(), want2)


# ---- the GRPO reward ---------------------------------------------------------------------------------------------------------------------
def _reward_batch(dev, B=4, G=3, seed=21):
    """Seeded rollouts as mask_and_clip_seqs leaves them (<bos> first, <pad> past the mask) and ragged targets."""
    from acai_omr_amd.train import grpo as GR
    _, pad = _vocab()
    g = torch.Generator().manual_seed(seed)
    targets = [torch.randint(3, 227, (int(n),), generator=g) for n in torch.randint(20, 90, (B,), generator=g)]
    R, T = B * G, 100
    lens = torch.randint(2, T + 1, (R,), generator=g)
    lens[0] = T
    rollouts = torch.randint(3, 227, (R, T), generator=g)
    for r in range(R):   # half of the rollouts are noisy copies of their target, so that the distances spread
        if r % 2 == 0:
            t = targets[r // G]
            n = min(int(lens[r]), len(t))
            keep = torch.rand(n, generator=g) < 0.8
            rollouts[r, :n] = torch.where(keep, t[:n], rollouts[r, :n])
    rollouts[:, 0] = 0
    mask = torch.arange(T)[None, :] < lens[:, None]
    rollouts = rollouts.masked_fill(~mask, pad).to(dev)
    mask = mask.to(dev)
    expanded = GR.expand_target_lmx_seqs([t.to(dev) for t in targets], G, pad, dev)
    return targets, rollouts, mask, expanded, pad


def _reference_costs(rollouts, mask, targets, G):
    ro, ln = rollouts.cpu().numpy(), mask.sum(-1).cpu().tolist()
    return [edit_distance(ro[r, :ln[r]], targets[r // G].numpy()) for r in range(ro.shape[0])]


def test_token_edit_costs_expanded_and_grouped_targets(dev):
    from acai_omr_amd.train import grpo as GR
    B, G = 4, 3
    targets, rollouts, mask, expanded, pad = _reward_batch(dev, B, G)
    unexpanded, _ = _pack([t.numpy() for t in targets], fill=pad)
    a = GR.calc_token_edit_costs(rollouts, mask, expanded, pad)
    b = GR.calc_token_edit_costs(rollouts, mask, unexpanded.to(dev), pad, group_size=G)
    assert a.dtype == torch.float32 and a.shape == (B * G,)
    assert torch.equal(a, b)
    assert a.cpu().tolist() == [float(c) for c in _reference_costs(rollouts, mask, targets, G)]


def test_token_reward_rollouts_components(dev):
    from acai_omr_amd.train import grpo as GR
    B, G = 4, 3
    targets, rollouts, mask, expanded, pad = _reward_batch(dev, B, G)
    rc = GR.INITIAL_REWARD_CONFIG
    rewards, comp = GR.token_reward_rollouts(rc, rollouts, mask, expanded, B, G, pad)
    costs = torch.tensor(_reference_costs(rollouts, mask, targets, G), dtype=torch.int32)
    # the same torch ops on equal integers: equal bits
    assert torch.equal(comp.tedn_scores, torch.exp(-rc.alpha_tedn * costs.to(dev).float()))
    assert torch.equal(comp.tedn_scores, GR.calc_tedn_scores(costs.to(dev).float(), rc.alpha_tedn))
    assert comp.wellformedness_scores.shape == (B * G,) and not bool(comp.wellformedness_scores.any())
    assert torch.equal(comp.f1_scores, GR.calc_token_f1(rollouts, expanded, pad))
    assert torch.equal(comp.repeat_penalty, GR.calc_repeat_penalty(rollouts, pad))
    assert torch.equal(comp.len_penalty, GR.calc_len_penalty(mask, expanded, pad, delta=rc.delta, tau=rc.tau))
    assert rewards.shape == (B, G) and torch.equal(rewards, GR.calc_group_rewards(rc, comp, B, G))
    assert float(comp.tedn_scores.max()) < 1.0 and float(comp.tedn_scores.std()) > 0   # (the costs are neither zero nor all alike)
    got = GR.make_token_reward_fn(rc, pad)(rollouts, mask, expanded, [None] * B)
    assert torch.equal(got[0], rewards) and torch.equal(got[1].tedn_scores, comp.tedn_scores)


def test_grpo_update_with_the_token_reward(dev):
    """grpo_update runs on a reward from the package alone: the average reward it returns is the mean of token_reward_rollouts on the rollouts it
    drew, and the step moves the parameters."""
    from acai_omr_amd.models.models import OMRCELoss
    from acai_omr_amd.train import grpo as GR
    fx, old, theta, Gs, cfg = _models(dev)
    _, pad = _vocab()
    g = torch.Generator().manual_seed(60)
    max_actions = cfg["max_len"] - 2
    R = len(fx["imgs"]) * Gs
    uniforms = torch.rand(R, max_actions, generator=g).to(dev)
    targets = [torch.randint(3, 227, (n,), generator=g) for n in (9, 5, 12)]
    batch = [(img, t, "") for img, t in zip(fx["imgs"], targets)]
    conf = GR.GRPOConfig(GR.RolloutConfig(Gs, max_actions, 20, 1.1), GR.INITIAL_REWARD_CONFIG, GR.LossConfig(0.05, 0.1), GR.UpdateConfig(0.2, 1, 1.0),
                         100, 100)
    opt = torch.optim.SGD(theta.parameters(), lr=1e-2)
    before = {n: p.detach().clone() for n, p in theta.decoder.named_parameters()}
    seen = []
    inner = GR.make_token_reward_fn(conf.reward_config, pad)

    def recording(rollouts, rollout_mask, target_lmx_seqs, batch_):
        seen.append((rollouts.clone(), rollout_mask.clone(), target_lmx_seqs.clone()))
        return inner(rollouts, rollout_mask, target_lmx_seqs, batch_)
    loss, ce, rew, comps = GR.grpo_update(old, theta, opt, batch, conf, OMRCELoss(pad), "cuda", reward_fn=recording, uniforms=uniforms)
    assert len(seen) == 1
    ro, rmask, tx = seen[0]
    # the same rollouts again (same old policy, same draws), rewarded from scratch
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        lat, lmask = old.encoder([i.to(dev) for i in fx["imgs"]])
        lat = old.transition_head(lat)
        ro2, _, rmask2 = GR._rollouts_grouped(old, lat, lmask, Gs, conf.rollout_config, uniforms)
    assert torch.equal(ro2, ro) and torch.equal(rmask2, rmask)
    tx2 = GR.expand_target_lmx_seqs([t.to(dev) for t in targets], Gs, pad, dev)
    rewards, comp = GR.token_reward_rollouts(conf.reward_config, ro2, rmask2, tx2, len(batch), Gs, pad)
    costs = _reference_costs(ro2, rmask2, targets, Gs)
    assert torch.equal(comp.tedn_scores, torch.exp(-conf.reward_config.alpha_tedn * torch.tensor(costs, dtype=torch.float32, device=dev)))
    print(f"grpo_update with the token reward: loss {loss:.6f}, ce {ce:.5f}, reward {rew:.6f}; token edit costs {costs}")
    assert rew == rewards.float().mean().item()
    assert comps.tedn_scores == comp.tedn_scores.mean().item() and comps.wellformedness_scores == 0.0
    assert loss == loss and ce == ce   # (finite: not NaN)
    moved = [n for n, p in theta.decoder.named_parameters() if not torch.equal(before[n], p.detach())]
    assert "unembed.weight" in moved and "vocab_embedding.weight" in moved, moved


# ---- symbol error rate on decoded rows ---------------------------------------------------------------------------------------------------
def test_symbol_error_rate_on_inference_output(dev):
    from acai_omr_amd.inference.vitomr_inference import inference
    from acai_omr_amd.models.models import FineTuneOMREncoder, OMRDecoder, TeacherForcedViTOMR
    from acai_omr_amd.utils import symbol_error_rate
    fx = load_golden("vitomr_dh64b")
    cfg, sd = fx["cfg"], fx["state_dict"]
    enc = FineTuneOMREncoder(cfg["P"], cfg["pe_h"], cfg["pe_w"], cfg["ft_depth"], num_layers=cfg["enc_layers"], hidden_dim=cfg["enc_dim"],
                             num_heads=cfg["enc_heads"], mlp_dim=cfg["enc_mlp"])
    dec = OMRDecoder(cfg["max_len"], VOCAB, num_layers=cfg["dec_layers"], hidden_dim=cfg["dec_dim"], num_heads=cfg["dec_heads"], mlp_dim=cfg["dec_mlp"])
    m = TeacherForcedViTOMR(enc, None, dec, transition_head_dim=cfg["head_dim"])
    m.load_state_dict(sd)
    cached = m.decoder.to_cached_version(8, torch.bfloat16)
    cached.load_state_dict(m.decoder.state_dict())
    m.decoder = cached
    m = m.to(dev).eval()
    seqs, _, mask = inference(m, fx["imgs"], "cuda", max_inference_len=cfg["gen_len"])
    rows = [seqs[i, :int(mask[i].sum())].cpu() for i in range(seqs.shape[0])]
    assert all(len(r) >= 3 for r in rows)
    ser, dist, lens = symbol_error_rate(seqs, mask, rows)
    assert ser == 0.0 and dist.cpu().tolist() == [0] * len(rows) and lens.cpu().tolist() == [len(r) for r in rows]
    _, pad = _vocab()
    ser, _, _ = symbol_error_rate(seqs, mask, seqs.masked_fill(~mask, pad), pad_idx=pad)   # (greedy rows hold no <pad> inside the mask)
    assert ser == 0.0
    # k substitutions per row at distinct positions, by an id that the row does not hold: the distance is exactly k
    g = torch.Generator().manual_seed(3)
    edited, counts = [], []
    for i, r in enumerate(rows):
        k = min(i + 1, len(r))
        pos = torch.randperm(len(r), generator=g)[:k]
        e = r.clone()
        e[pos] = 100000 + i
        edited.append(e), counts.append(k)
    ser, dist, lens = symbol_error_rate(seqs, mask, edited)
    assert dist.cpu().tolist() == counts
    assert ser == sum(counts) / sum(len(r) for r in rows)


def test_ser_validation(dev):
    """The corpus rate of a two-batch loader equals symbol_error_rate over all of its rows."""
    from acai_omr_amd.inference.vitomr_inference import inference
    from acai_omr_amd.models.models import FineTuneOMREncoder, OMRDecoder, TeacherForcedViTOMR
    from acai_omr_amd.train.loops import ser_validation
    from acai_omr_amd.utils import symbol_error_rate
    fx = load_golden("vitomr_dh64b")
    cfg, sd = fx["cfg"], fx["state_dict"]
    enc = FineTuneOMREncoder(cfg["P"], cfg["pe_h"], cfg["pe_w"], cfg["ft_depth"], num_layers=cfg["enc_layers"], hidden_dim=cfg["enc_dim"],
                             num_heads=cfg["enc_heads"], mlp_dim=cfg["enc_mlp"])
    dec = OMRDecoder(cfg["max_len"], VOCAB, num_layers=cfg["dec_layers"], hidden_dim=cfg["dec_dim"], num_heads=cfg["dec_heads"], mlp_dim=cfg["dec_mlp"])
    m = TeacherForcedViTOMR(enc, None, dec, transition_head_dim=cfg["head_dim"])
    m.load_state_dict(sd)
    cached = m.decoder.to_cached_version(8, torch.bfloat16)
    cached.load_state_dict(m.decoder.state_dict())
    m.decoder = cached
    m = m.to(dev).eval()
    g = torch.Generator().manual_seed(4)
    targets = [torch.randint(0, 227, (n,), generator=g) for n in (10, 4, 12)]
    loader = [[(fx["imgs"][0], targets[0]), (fx["imgs"][1], targets[1])], [(fx["imgs"][2], targets[2])]]
    got = ser_validation(m, loader, "cuda", max_inference_len=cfg["gen_len"])
    seqs, _, mask = inference(m, fx["imgs"], "cuda", max_inference_len=cfg["gen_len"])
    want, dist, _ = symbol_error_rate(seqs, mask, targets)
    rows = [seqs[i, :int(mask[i].sum())].cpu().numpy() for i in range(3)]
    assert dist.cpu().tolist() == [edit_distance(r, t.numpy()) for r, t in zip(rows, targets)]
    assert got == want and got > 0
    assert ser_validation(m, [[(fx["imgs"][i], torch.from_numpy(rows[i])) for i in range(3)]], "cuda", max_inference_len=cfg["gen_len"]) == 0.0
