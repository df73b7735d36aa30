"""Continuous-batching SAMPLED decode on the GPU (acai_decode_slot_sample_step through DecodeEngine.continuous(sample=...),
GRPOViTOMR.cached_continuous_rollout_policy, grpo_update(rollout_slots=...) and validation_loop).

The yardstick of every comparison is the STATIC sampling path (DecodeEngine.sample / cached_forward_rollout_policy) and the stepwise
`logits_step`; the continuous sampler is never compared with itself except for the bitwise agreement of its own forms.

Bars:
  * full width (E = 1024, 16 heads), fp32, 16 ragged memories, per-sequence caps around the 8-step graph and 16-step poll boundaries, one
    seeded uniforms table: every sequence equals static sampling of its memory alone with its uniforms row (ids and mask equal, log-probs
    within 1e-4, the bar of test_full_width_each_image_as_alone), at (top_k, temperature) = (50, 1.1) and (3, 1.1), slots 4 and 8;
  * top_k = 1 returns greedy continuous decoding's ids for any uniforms (fp32, equal);
  * bf16 and the FP8 memory cache: by REPLAY (see _replay_check);
  * graph / eager, poll 1 / 5 / 16, slots > N and N = 1 are bitwise equal;
  * a sampled continuous run leaves greedy continuous, static sampling, greedy and beam bitwise as they were and does not rebuild the
    greedy slot graphs;
  * the model and training surfaces against the static path, and the C ABI's argument checks (argument errors only)."""
import copy
import ctypes
import math

import pytest
import torch
from torch.amp import autocast

from conftest import load_golden
from decode_support import build_vitomr, _decoder, dev, _md, _memory, _models, ref_objective_and_bonus, _reward_fn, _same, _vit, _vocab

pytestmark = pytest.mark.gpu


# ---- the set-up of tests/test_gpu_continuous.py -------------------------------------------------------------------------------------------
LENS = [256, 4096, 700, 1300, 3000, 512, 2048, 999, 4096, 300, 1500, 2600, 777, 3500, 1024, 2222]
CAPS = [2, 8, 9, 16, 17, 96, 33, 50, 64, 5, 12, 24, 70, 96, 40, 3]
OFFS = [sum(LENS[:i]) for i in range(len(LENS) + 1)]


def _full_width(cdt, dev, seed=5, memory_cache_dtype=None):
    dec = _decoder(128, seed=seed, scale=16.0)
    m = _vit(dec, 8, cdt, dev, memory_cache_dtype)
    mem = torch.randn(sum(LENS), 1024, generator=torch.Generator().manual_seed(seed + 100))
    return m, (mem.to(torch.bfloat16) if cdt == torch.bfloat16 else mem).to(dev)


def _uniforms(seed, dev, n=len(LENS), w=max(CAPS)):
    return torch.rand(n, w, generator=torch.Generator().manual_seed(seed)).to(dev)


def _mems(mem, bf):
    return (None, mem) if bf else (mem, None)


def _static_alone(m, mem, bf, U, top_k, temperature, dev):
    """Static sampling (DecodeEngine.sample) of each memory alone at its cap with its own uniforms row."""
    out = []
    blocks = m.decoder.decoder_blocks
    for i, (l, c) in enumerate(zip(LENS, CAPS)):
        x = mem[OFFS[i]:OFFS[i + 1]]
        with torch.no_grad():
            blocks.prepare_caches_packed(*_mems(x, bf), [l])
            seqs, lps, _ = blocks.engine(dev).sample(c, top_k, temperature, uniforms=U[i:i + 1, :c])
            out.append(m.mask_and_clip_seqs(seqs.clone(), lps.clone()))
    return out


def _sampled(m, mem, bf, U, top_k, temperature, slots, lens=LENS, caps=CAPS, **kw):
    with torch.no_grad():
        return m._continuous_packed(*_mems(mem, bf), lens, caps, slots, sample=(top_k, temperature), uniforms=U, **kw)


# ---- 1. fp32: each sequence as alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_k", [50, 3])
def test_fp32_each_sequence_as_alone(dev, top_k):
    m, mem = _full_width(torch.float32, dev)
    U = _uniforms(11, dev)
    ref = _static_alone(m, mem, False, U, top_k, 1.1, dev)
    for slots in (4, 8):
        seqs, lps, smask = _sampled(m, mem, False, U, top_k, 1.1, slots)
        worst = 0.0
        for i, (rs, rl, rk) in enumerate(ref):
            n = rs.shape[1]
            worst = max(worst, _md(lps[i, :n], rl[0]))
            assert torch.equal(seqs[i, :n], rs[0]) and torch.equal(smask[i, :n], rk[0]), (slots, i)
            assert not bool(smask[i, n:].any()), (slots, i)
            assert _md(lps[i, :n], rl[0]) < 1e-4, (slots, i)
        print(f"fp32 top_k {top_k} slots {slots}: ids equal, max log-prob difference {worst:.3g}")
    assert sum(int(r[2].sum()) for r in ref) > 300   # (the rows run: random weights rarely draw <eos>)


# ---- 2. top_k = 1 is greedy ---------------------------------------------------------------------------------------------------------------
def test_top_k_1_is_greedy(dev):
    m, mem = _full_width(torch.float32, dev)
    with torch.no_grad():
        greedy = m._continuous_packed(mem, None, LENS, CAPS, 4)
    for seed in (1, 2):
        got = _sampled(m, mem, False, _uniforms(seed, dev), 1, 1.1, 4)
        assert torch.equal(got[0], greedy[0]) and torch.equal(got[2], greedy[2]), seed
        assert not bool(got[1].any())   # log_softmax over the one kept logit


# ---- 3 / 6. bf16 and the FP8 memory cache: replay against the stepwise logits ----------------------------------------------------------------
TEMPERATURE = 1.1
BF16_ULP = 0.125            # of a logit at the |logit| of 16 .. 32 this decoder gives (tests/test_gpu_continuous.py)
KTH_GAP = 2 * BF16_ULP      # the k-th and (k+1)-th logits within two ulps: which of them is kept may differ
# The largest move of a CDF boundary when ONE logit moves by one bf16 ulp: the mass c on one side of the boundary becomes
# c e / (c e + 1 - c) with e = exp(ulp / temperature); the change c (1 - c) (e - 1) / (1 + c (e - 1)) is below (e - 1) / 4.
CDF_SHIFT_ONE_ULP = 0.25 * (math.exp(BF16_ULP / TEMPERATURE) - 1.0)
# What excuses the STATIC bf16 sampler's own replay mismatches on these inputs (parent-commit code; measured by the first half of
# _replay_check and printed on every run: it has none, see _replay_check's docstring): the fp32 rounding of a CDF of up to 64 terms.
STATIC_OWN_MARGIN = 64 * 2.0 ** -24
CDF_MARGIN = STATIC_OWN_MARGIN + CDF_SHIFT_ONE_ULP
EXCUSED_CAP = 0.01


def _replay(eng, blocks, mem_i, l, toks, n, urow, top_k):
    """Teacher-forces toks[:n] of one sequence through logits_step on its memory alone; per drawn position t the token the inverse-CDF
    rule picks from those logits and urow[t] (float64), the distance of urow[t] to the nearest CDF boundary, and the k-th / (k+1)-th gap."""
    blocks.prepare_caches_packed(None, mem_i, [l])
    out = []
    with torch.no_grad():
        for t in range(1, n):
            lg = eng.logits_step(toks[t - 1:t], t).view(-1).double().cpu()
            val, idx = torch.sort(lg, descending=True, stable=True)   # ties: lower index first
            k = min(top_k, lg.numel())
            p = torch.exp((val[:k] - val[0]) / TEMPERATURE)
            cdf = torch.cumsum(p, 0) / p.sum()
            u = float(urow[t])
            hit = (cdf > u).nonzero()
            r = int(hit[0]) if hit.numel() else k - 1
            gap = float(val[k - 1] - val[k]) if k < lg.numel() else float("inf")
            out.append((t, int(idx[r]), float((cdf[:-1] - u).abs().min()) if k > 1 else float("inf"), gap))
    return out


def _replay_check(m, mem, U, top_k, slots_list, dev, what):
    """bf16 logits are rounded, and a slot run's cross split differs from the sequence-alone run's, so a draw whose uniform sits next to a
    CDF boundary (or whose top-k set is decided by a near tie) may go the other way and the trajectories then part for good.  Each sampled
    sequence is therefore checked by replay: its own tokens teacher-forced through logits_step on its memory alone must, position by
    position, be what the inverse-CDF rule picks from those logits and the same uniform, unless the position is excusable (uniform within
    CDF_MARGIN of a boundary, or k-th / (k+1)-th logit within KTH_GAP).  Excused positions are capped at EXCUSED_CAP of all drawn positions,
    for the static sampler alone (checked first) as for the continuous one, and everything before a sequence's first excused position
    equals static sampling of that sequence alone exactly.

    CDF_MARGIN = what excuses the static sampler's own replay mismatches + the shift one bf16 ulp of a logit makes in the CDF
    (0.25 (exp(0.125 / 1.1) - 1) = 0.0301).  Measured on the MI355X (uniforms seed 11, top_k 50, temperature 1.1, 529 drawn positions): the
    static sampler's own replay has NO mismatch, bf16 or FP8 memory (its chained step and logits_step give the same logits, and the
    float64 replay of its fp32 CDF never lands on the other side of a uniform), so its share of the margin is only the fp32 rounding of a
    CDF of up to 64 terms, 64 * 2^-24 = 3.8e-6: CDF_MARGIN = 0.03009.  The continuous sampler: 0 mismatches at 4 slots (bf16 and FP8), 2
    at 8 slots (0.38 %; CDF distances 0.0127 and 0.0045, and the k-th / (k+1)-th logits 0.031 apart in both)."""
    blocks = m.decoder.decoder_blocks
    eng = blocks.engine(dev)
    static = _static_alone(m, mem, True, U, top_k, TEMPERATURE, dev)

    def audit(rows, tag):
        """rows[i] = (tokens, n).  Asserts every replay mismatch is excusable and their share; returns each sequence's first excused
        position (None: none)."""
        drawn = excused = 0
        first, worst_cdf = [], 0.0
        for i, (toks, n) in enumerate(rows):
            rep = _replay(eng, blocks, mem[OFFS[i]:OFFS[i + 1]], LENS[i], toks, n, U[i].cpu(), top_k)
            f = None
            for t, want, dist, gap in rep:
                drawn += 1
                if int(toks[t]) != want:
                    excused += 1
                    f = t if f is None else f
                    print(f"  {tag}: sequence {i} position {t}: drew {int(toks[t])}, replay picks {want}; CDF distance {dist:.3g}, "
                          f"k-th gap {gap:.3g}")
                    if gap > KTH_GAP:
                        worst_cdf = max(worst_cdf, dist)
                    assert dist <= CDF_MARGIN or gap <= KTH_GAP, (tag, i, t, dist, gap)
            first.append(f)
        print(f"{what} {tag}: {excused} excused of {drawn} drawn positions; largest CDF distance that had to be excused {worst_cdf:.3g} "
              f"(margin {CDF_MARGIN:.4g})")
        assert excused <= EXCUSED_CAP * drawn, (tag, excused, drawn)
        return first

    audit([(rs[0], int(rk.sum())) for rs, _, rk in static], "static sampler alone")
    for slots in slots_list:
        seqs, lps, smask = _sampled(m, mem, True, U, top_k, TEMPERATURE, slots)
        rows = [(seqs[i], int(smask[i].sum())) for i in range(len(LENS))]
        first = audit(rows, f"continuous, {slots} slots")
        for i, (rs, rl, rk) in enumerate(static):
            n = rs.shape[1]
            p = min(n, seqs.shape[1]) if first[i] is None else first[i]
            assert torch.equal(seqs[i, :p], rs[0, :p]), (slots, i, p)
            assert _md(lps[i, :p], rl[0, :p]) < 0.25, (slots, i)
            if first[i] is None:
                assert torch.equal(smask[i, :n], rk[0]) and not bool(smask[i, n:].any()), (slots, i)


def test_bf16_replay_against_stepwise_logits(dev):
    m, mem = _full_width(torch.bfloat16, dev)
    _replay_check(m, mem, _uniforms(11, dev), 50, (4, 8), dev, "bf16")


def test_fp8_memory_cache_replay(dev):
    m, mem = _full_width(torch.bfloat16, dev, memory_cache_dtype=torch.float8_e4m3fn)
    assert m.decoder.decoder_blocks.engine(dev).cross_fp8
    _replay_check(m, mem, _uniforms(11, dev), 50, (4,), dev, "fp8 memory")


# ---- 4. forms agree -----------------------------------------------------------------------------------------------------------------------
def test_forms_agree_bitwise(dev):
    m, mem = _full_width(torch.bfloat16, dev, seed=7)
    U = _uniforms(12, dev)
    base = _sampled(m, mem, True, U, 50, 1.1, 4)
    for kw in (dict(use_graph=False), dict(poll=1), dict(poll=1, use_graph=False), dict(poll=5)):
        _same(base, _sampled(m, mem, True, U, 50, 1.1, 4, **kw))
    for lo, hi, caps, slots in ((0, 3, CAPS[3:6], 8), (5, 6, CAPS[5:6], 1), (5, 6, CAPS[5:6], 4)):   # slots > N and N = 1
        x, lens = mem[OFFS[lo]:OFFS[hi]], LENS[lo:hi]
        u = U[lo:hi, :max(caps)].contiguous()
        base = _sampled(m, x, True, u, 50, 1.1, slots, lens=lens, caps=caps)
        _same(base, _sampled(m, x, True, u, 50, 1.1, slots, lens=lens, caps=caps, poll=1, use_graph=False))
        assert base[0].shape[0] == len(lens) and bool((base[0][:, 0] == m.decoder.bos_idx).all())
    # the default uniforms come from torch's generator: a seed reproduces a run
    runs = []
    for _ in range(2):
        torch.manual_seed(99)
        with torch.no_grad():
            runs.append(m._continuous_packed(None, mem, LENS, CAPS, 4, sample=(50, 1.1)))
    _same(runs[0], runs[1])


# ---- 5. isolation -------------------------------------------------------------------------------------------------------------------------
def test_sampled_slot_mode_leaves_other_modes_alone(dev):
    from acai_omr_amd import engine as EG
    from acai_omr_amd.inference.vitomr_inference import inference
    fx = load_golden("vitomr_dh64b")
    cfg = fx["cfg"]
    T = cfg["gen_len"]
    u = torch.rand(len(fx["imgs"]) * 2, T, generator=torch.Generator().manual_seed(3)).to(dev)
    caps = [T, T - 3, 5]

    def setup():
        m = build_vitomr(cfg, fx["state_dict"], dev, torch.bfloat16, max_batch=16, transformer_dropout=0.0)
        mem, mask = _memory(m, fx["imgs"], True)
        return m, mem, mask

    def others(m, mem, mask):
        with torch.no_grad():
            c = m.cached_continuous_generate(mem, mask, max_len=caps, slots=2)
        g = inference(m, fx["imgs"], "cuda", max_inference_len=T)
        with torch.no_grad(), autocast(device_type="cuda", dtype=torch.bfloat16):
            b = m.cached_beam_generate(mem, mask, beam_width=4, max_len=T)
        blocks = m.decoder.decoder_blocks
        mem32, lens = EG.unpad_rows(mem, mask)
        blocks.prepare_caches_packed(mem32, None, lens, group_size=2)
        s = tuple(x.clone() for x in blocks.engine(dev).sample(T, 5, 1.3, uniforms=u)[:2])
        return c + g + b + s

    def sampled(m, mem, mask):
        mem32, lens = EG.unpad_rows(mem, mask)
        with torch.no_grad():
            return m._continuous_packed(mem32, None, lens, caps, 2, sample=(5, 1.3), uniforms=u[:3])

    m0, mem0, mask0 = setup()
    fresh_others = others(m0, mem0, mask0)
    m1, mem1, mask1 = setup()
    fresh_sampled = sampled(m1, mem1, mask1)
    _same(fresh_others, others(m1, mem1, mask1))          # sampled slot mode, then everything else
    _same(fresh_sampled, sampled(m1, mem1, mask1))        # everything else, then sampled slot mode
    # the greedy slot graphs survive a sampled run between two greedy slot runs, and the sampled run has graphs of its own
    eng = m1.decoder.decoder_blocks.engine(dev)
    with torch.no_grad():
        c0 = m1.cached_continuous_generate(mem1, mask1, max_len=caps, slots=2)
    greedy_graphs = {k: id(g) for k, g in eng.graphs.items() if k[4] == ("slot",)}
    assert greedy_graphs
    _same(fresh_sampled, sampled(m1, mem1, mask1))
    assert {k: id(g) for k, g in eng.graphs.items() if k[4] == ("slot",)} == greedy_graphs
    assert any(k[4] == ("slot_sample", 5, 1.3) for k in eng.graphs)
    with torch.no_grad():
        _same(c0, m1.cached_continuous_generate(mem1, mask1, max_len=caps, slots=2))
    assert {k: id(g) for k, g in eng.graphs.items() if k[4] == ("slot",)} == greedy_graphs
    assert eng._mode == ("greedy",)


# ---- 7. model surface ---------------------------------------------------------------------------------------------------------------------
def test_cached_continuous_rollout_policy_vs_static(dev):
    fx = load_golden("vitomr_dh64b")
    cfg = fx["cfg"]
    N, T = len(fx["imgs"]), cfg["max_len"] - 2
    big = build_vitomr(cfg, fx["state_dict"], dev, torch.float32, max_batch=16, grpo=True, transformer_dropout=0.0).eval()
    mem, mask = _memory(big, fx["imgs"], False)
    g = torch.Generator().manual_seed(21)
    U = torch.rand(N, T, generator=g).to(dev)
    with torch.no_grad():
        ref = big.cached_forward_rollout_policy(mem, mask, T, 20, 1.1, uniforms=U)
        for slots in (1, 2, None):
            got = big.cached_continuous_rollout_policy(mem, mask, T, 20, 1.1, slots=slots, uniforms=U)
            print(f"rollout policy, slots {slots}: max log-prob difference {_md(got[1], ref[1]):.3g}")
            _same(ref, got)
        # per-rollout caps
        caps = [T, 5, 9]
        got = big.cached_continuous_rollout_policy(mem, mask, caps, 20, 1.1, slots=2, uniforms=U)
        for i, c in enumerate(caps):
            one = big.cached_forward_rollout_policy(mem[i:i + 1], mask[i:i + 1], c, 20, 1.1, uniforms=U[i:i + 1, :c])
            n = one[0].shape[1]
            assert torch.equal(got[0][i, :n], one[0][0]) and torch.equal(got[2][i, :n], one[2][0]) and not bool(got[2][i, n:].any())
        # group_size = 4 against the grouped static path (one stored cross K/V per image there, one per rollout here)
        G = 4
        U4 = torch.rand(N * G, T, generator=g).to(dev)
        mem_x, mask_x = big.expand_img_latent_for_rollout(mem, mask, G)
        ref4 = big.cached_forward_rollout_policy(mem_x, mask_x, T, 20, 1.1, group_size=G, uniforms=U4)
        got4 = big.cached_continuous_rollout_policy(mem, mask, T, 20, 1.1, slots=5, group_size=G, uniforms=U4)
        print(f"rollout policy, group_size 4: max log-prob difference {_md(got4[1], ref4[1]):.3g}")
        assert got4[0].shape[0] == N * G and got4[1].dtype == torch.float32 and got4[2].dtype == torch.bool
        assert torch.equal(got4[0], ref4[0]) and torch.equal(got4[2], ref4[2])
        assert _md(got4[1], ref4[1]) < 1e-4
        # more rollouts than the cache's max batch size
        small = build_vitomr(cfg, fx["state_dict"], dev, torch.float32, max_batch=2, grpo=True, transformer_dropout=0.0).eval()
        with pytest.raises(ValueError, match="max batch size"):
            small.cached_forward_rollout_policy(mem, mask, T, 20, 1.1, uniforms=U)
        _same(ref, small.cached_continuous_rollout_policy(mem, mask, T, 20, 1.1, uniforms=U))
        _same(ref, small.cached_continuous_rollout_policy(mem, mask, T, 20, 1.1, slots=1, uniforms=U))
        assert torch.equal(small.cached_continuous_rollout_policy(mem, mask, T, 20, 1.1, group_size=G, uniforms=U4)[0], ref4[0])
        with pytest.raises(ValueError, match="uniforms must be"):
            big.cached_continuous_rollout_policy(mem, mask, T, 20, 1.1, uniforms=U4)
        with pytest.raises(ValueError, match="top_k"):
            big.cached_continuous_rollout_policy(mem, mask, T, 65, 1.1, uniforms=U)


# ---- 8. training surface ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lambda_ce", [0.1, 0.0])
def test_grpo_update_with_rollout_slots_matches_a_reference_step(dev, lambda_ce):
    """test_grpo_update_matches_a_reference_step (tests/test_gpu_grpo.py) with rollout_slots set: the reference step is built on the
    rollouts cached_continuous_rollout_policy returns for the same uniforms, within that test's bars."""
    from acai_omr_amd.models.models import OMRCELoss
    from acai_omr_amd.train import grpo as G
    fx, old, theta, Gs, cfg = _models(dev)
    V, pad, _ = _vocab()
    g = torch.Generator().manual_seed(60)
    max_actions = cfg["max_len"] - 2
    R = len(fx["imgs"]) * Gs
    uniforms = torch.rand(R, max_actions, generator=g).to(dev)
    targets = [torch.randint(3, 227, (n,), generator=g) for n in (9, 5, 12)]
    batch = [(img, t, "") for img, t in zip(fx["imgs"], targets)]
    conf = G.GRPOConfig(G.RolloutConfig(Gs, max_actions, 20, 1.1), G.INITIAL_REWARD_CONFIG, G.LossConfig(0.05, lambda_ce),
                        G.UpdateConfig(0.2, 1, 1.0), 100, 100)
    ref_theta = copy.deepcopy(theta)
    ce_fn = OMRCELoss(pad)
    lr = 1e-2
    opt = torch.optim.SGD(theta.parameters(), lr=lr)
    before = {n: p.detach().clone() for n, p in theta.decoder.named_parameters()}
    SLOTS = 4
    loss, ce, rew, _ = G.grpo_update(old, theta, opt, batch, conf, ce_fn, "cuda", reward_fn=_reward_fn, uniforms=uniforms, rollout_slots=SLOTS)

    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        lat, lmask = old.encoder([i.to(dev) for i in fx["imgs"]])
        lat = old.transition_head(lat)
        lat_x, lmask_x = old.expand_img_latent_for_rollout(lat, lmask, Gs)
        ro, olp, rmask = old.cached_continuous_rollout_policy(lat, lmask, max_actions, 20, 1.1, slots=SLOTS, group_size=Gs, uniforms=uniforms)
        st = old.cached_forward_rollout_policy(lat_x, lmask_x, max_actions, 20, 1.1, group_size=Gs, uniforms=uniforms)
    print(f"continuous rollouts equal the static ones: ids {st[0].shape == ro.shape and torch.equal(st[0], ro)}")
    assert ro.shape[0] == R
    tx = G.expand_target_lmx_seqs([t.to(dev) for t in targets], Gs, pad, dev)
    rg = _reward_fn(ro, rmask, tx, batch).float()
    assert abs(rew - float(rg.mean())) <= 1e-6 * max(1.0, abs(float(rg.mean())))
    adv = ((rg - rg.mean(-1, keepdim=True)) / (rg.std(-1, keepdim=True) + 1e-8)).view(-1)
    rs, am = old.prepare_rollouts_for_policy_theta(ro, rmask)
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        logits_x = ref_theta.decoder(rs, lat_x.float(), am, lmask_x, checkpoint_grads=True)
        logits = ref_theta.decoder(rs, lat.float(), am, lmask, checkpoint_grads=True, memory_group_size=Gs)
        if lambda_ce:
            ref_ce = G.calc_teacher_forced_ce_loss(ref_theta, lat.float(), lmask, [t.to(dev) for t in targets], ce_fn)
        else:
            ref_ce = torch.zeros((), device=dev)
    xobj, xbon = ref_objective_and_bonus(logits_x.detach().double().cpu(), ro.cpu(), am.cpu(), olp.cpu(), adv.cpu(), 0.2, len(batch))
    xloss = float(-(xobj + 0.05 * xbon) + lambda_ce * ref_ce.detach().double().cpu())
    l64 = logits.detach().double().cpu().requires_grad_(True)
    robj, rbon = ref_objective_and_bonus(l64, ro.cpu(), am.cpu(), olp.cpu(), adv.cpu(), 0.2, len(batch))
    rloss64 = -(robj + 0.05 * rbon) + lambda_ce * ref_ce.detach().double().cpu()
    rloss64.backward()
    ((logits.float() * l64.grad.to(dev).float()).sum() + lambda_ce * ref_ce).backward()
    torch.nn.utils.clip_grad_norm_(ref_theta.parameters(), max_norm=1.0)
    print(f"grpo_update rollout_slots={SLOTS} lambda_ce={lambda_ce}: loss {loss:.6f} vs {float(rloss64):.6f} (materialised expansion "
          f"{xloss:.6f}), ce {ce:.5f} vs {float(ref_ce):.5f}")
    assert abs(loss - xloss) <= 2e-3 * max(1.0, abs(xloss))
    assert abs(loss - float(rloss64)) <= 1e-5 * max(1.0, abs(float(rloss64)))
    assert abs(ce - float(ref_ce)) <= 1e-3 * max(1.0, abs(float(ref_ce)))
    names = ["unembed.weight", "unembed.bias", "decoder_blocks.layers.0.multihead_attn.in_proj_weight", "decoder_blocks.layers.1.linear1.weight",
             "decoder_blocks.layers.1.self_attn.out_proj.weight", "decoder_blocks.norm.weight", "vocab_embedding.weight", "pos_embedding"]
    rp = dict(ref_theta.decoder.named_parameters())
    for n, p in theta.decoder.named_parameters():
        if n in names:
            rg_ = rp[n].grad
            err = float(((before[n] - p.detach()) / lr - rg_).abs().max()) / max(1e-6, float(rg_.abs().max()))
            print(f"  {n}: gradient rel {err:.2e}")
            assert err <= 5e-2, n


def test_grpo_update_rollout_slots_lift_the_batch_limit(dev):
    from acai_omr_amd.models.models import OMRCELoss
    from acai_omr_amd.train import grpo as G
    fx, old, theta, Gs, cfg = _models(dev)
    _, pad, _ = _vocab()
    g = torch.Generator().manual_seed(61)
    max_actions = cfg["max_len"] - 2
    Gbig = Gs + 2                                   # B * G = 15 rollouts on a cache of 9 rows
    R = len(fx["imgs"]) * Gbig
    assert R > old.decoder.decoder_blocks.max_batch_size
    uniforms = torch.rand(R, max_actions, generator=g).to(dev)
    targets = [torch.randint(3, 227, (n,), generator=g) for n in (9, 5, 12)]
    batch = [(img, t, "") for img, t in zip(fx["imgs"], targets)]
    conf = G.GRPOConfig(G.RolloutConfig(Gbig, max_actions, 20, 1.1), G.INITIAL_REWARD_CONFIG, G.LossConfig(0.05, 0.1), G.UpdateConfig(0.2, 1, 1.0),
                        100, 100)
    opt = torch.optim.SGD(theta.parameters(), lr=1e-3)
    with pytest.raises(ValueError, match="max batch size"):
        G.grpo_update(old, theta, opt, batch, conf, OMRCELoss(pad), "cuda", reward_fn=_reward_fn, uniforms=uniforms)
    loss, ce, rew, _ = G.grpo_update(old, theta, opt, batch, conf, OMRCELoss(pad), "cuda", reward_fn=_reward_fn, uniforms=uniforms, rollout_slots=4)
    assert all(math.isfinite(v) for v in (loss, ce, rew))


def test_validation_loop_vs_hand_rolled(dev):
    """validation_loop over a two-batch list dataloader with fixed draws, fp32 without autocast, against a hand-rolled loop over
    cached_forward_rollout_policy + token_reward_rollouts + the teacher-forced CE (the two rollout routes agree exactly in fp32)."""
    from acai_omr_amd.models.models import OMRCELoss
    from acai_omr_amd.train import grpo as G
    fx = load_golden("vitomr_dh64b")
    cfg = fx["cfg"]
    _, pad, _ = _vocab()
    policy = build_vitomr(cfg, fx["state_dict"], dev, torch.float32, max_batch=4, grpo=True, transformer_dropout=0.0).eval()
    g = torch.Generator().manual_seed(80)
    max_actions = cfg["max_len"] - 2
    imgs = fx["imgs"]
    targets = [torch.randint(3, 227, (n,), generator=g) for n in (9, 5, 12, 7, 10)]
    order = [0, 1, 2, 1, 0]
    data = [(imgs[i], t, "") for i, t in zip(order, targets)]
    loader = [data[:3], data[3:]]
    U = [torch.rand(len(b), max_actions, generator=g).to(dev) for b in loader]
    rconf = G.RolloutConfig(1, max_actions, 20, 1.1)
    ce_fn = OMRCELoss(pad)
    calls = []

    def uniforms_fn(i, R, T):
        calls.append((i, R, T))
        return U[i]

    rew, comps, ce = G.validation_loop(loader, policy, G.INITIAL_REWARD_CONFIG, rconf, ce_fn, pad, "cuda", slots=2, uniforms_fn=uniforms_fn,
                                       autocast_dtype=None)
    assert calls == [(0, 3, max_actions), (1, 2, max_actions)]
    xr, xc, xce = 0.0, G.RewardComponents(0, 0, 0, 0, 0), 0.0
    with torch.no_grad():
        for i, b in enumerate(loader):
            ims, tg, _ = zip(*b)
            tg = [t.to(dev) for t in tg]
            lat, lmask = policy.encoder([im.to(dev) for im in ims])
            lat = policy.transition_head(lat)
            ro, _, rmask = policy.cached_forward_rollout_policy(lat, lmask, max_actions, 20, 1.1, uniforms=U[i])
            tx = G.expand_target_lmx_seqs(tg, 1, pad, dev)
            raw, c = G.token_reward_rollouts(G.INITIAL_REWARD_CONFIG, ro, rmask, tx, len(b), 1, pad)
            xr += raw.mean().item()
            xc += c.avg_over_rollouts()
            xce += G.calc_teacher_forced_ce_loss(policy, lat, lmask, tg, ce_fn).item()
    n = len(loader)
    print(f"validation_loop: reward {rew} vs {xr / n}, ce {ce} vs {xce / n}, components {comps} vs {xc / n}")
    assert rew == xr / n and comps == xc / n        # the rollouts are the same integers: the rewards agree exactly
    # the CE is a float32 mean over the same logits, but its reduction order is not pinned across calls (measured: 8.104257822 against
    # 8.104258299, 5.9e-8 relative); the bar is 8 roundings of 2^-24
    assert abs(ce - xce / n) <= 8 * 2.0 ** -24 * abs(xce / n)
    # the reference's own configuration: bf16 autocast, torch's generator for the draws, the default reward - it runs and is finite
    torch.manual_seed(5)
    r2, c2, ce2 = G.validation_loop(loader, policy, G.INITIAL_REWARD_CONFIG, rconf, ce_fn, pad, "cuda")
    assert all(math.isfinite(v) for v in (r2, ce2) + c2._vals())


# ---- 9. the C ABI's argument checks ---------------------------------------------------------------------------------------------------------
def test_c_abi_argument_checks(dev):
    from acai_omr_amd import _lib
    m, mem = _full_width(torch.float32, dev)
    U = _uniforms(11, dev, n=3, w=max(CAPS[:3]))
    _sampled(m, mem[:OFFS[3]], False, U, 50, 1.1, 2, lens=LENS[:3], caps=CAPS[:3])
    eng = m.decoder.decoder_blocks.engine(dev)
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    d, sl = ctypes.byref(eng._desc), ctypes.byref(eng._slot_desc)
    u, ur, ld = eng.slot_uniforms.data_ptr(), eng.slot_urow.data_ptr(), eng.Tmax

    def bad(msg, *args):
        assert L.acai_decode_slot_sample_step(*args) < 0
        assert msg in L.acai_last_error(), (msg, L.acai_last_error())

    bad(b"uniforms", d, sl, None, ld, ur, 50, 1.1, st)
    bad(b"urow", d, sl, u, ld, None, 50, 1.1, st)
    bad(b"ld_uniforms", d, sl, u, eng.Tmax - 1, ur, 50, 1.1, st)
    bad(b"top_k", d, sl, u, ld, ur, 0, 1.1, st)
    bad(b"top_k", d, sl, u, ld, ur, 65, 1.1, st)
    bad(b"temperature", d, sl, u, ld, ur, 50, 0.0, st)
    bad(b"slot state", d, None, u, ld, ur, 50, 1.1, st)
    eng._desc.cross_group = 2
    try:
        bad(b"cross_group", d, sl, u, ld, ur, 50, 1.1, st)
    finally:
        eng._desc.cross_group = 1
    eng._desc.max_len = eng.Tmax + 1
    try:
        bad(b"max_len", d, sl, u, ld + 1, ur, 50, 1.1, st)
    finally:
        eng._desc.max_len = eng.Tmax
    eng.logits_step(torch.zeros(eng.B, dtype=torch.int64, device=dev), 1)   # overwrites x
    bad(b"x does not hold", d, sl, u, ld, ur, 50, 1.1, st)
    torch.cuda.synchronize()
