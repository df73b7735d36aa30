"""GRPO policy update on the GPU: the fused objective / entropy kernels against the reference's KATs and float64 autograd of the reference
formulas (omr_grpo_train.py:240-283), the group-shared memory of OMRDecoder.forward(memory_group_size=G) against the materialised expansion,
and one grpo_update against a step built from the materialised expansion, the float64 formulas and stock torch ops."""
import copy

import pytest
import torch

from conftest import VOCAB, load_golden
from decode_support import _models, ref_objective_and_bonus, _reward_fn, _vocab

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from acai_omr_amd import _lib
    _lib.lib()
    return "cuda"


def _fused(logits, rollouts, mask, old_lp, adv, eps, num_groups):
    from acai_omr_amd.train import grpo as G
    return G.calc_grpo_objective_and_entropy_bonus(logits, rollouts, mask, old_lp, adv, eps, num_groups)


# ---- kernel: the reference's KATs ----------------------------------------------------------------------------------------------------------
def test_calc_grpo_reference_kat(dev):
    """tests/test_omr_grpo_train.py::test_calc_grpo restated: -inf logits, four classes at 1/4 each, eps = 100, ragged masks."""
    from acai_omr_amd.train import grpo as G
    V, pad, eos = _vocab()
    lg = torch.full([4, 3, V], float("-inf"))
    for c in (0, eos, 5, 200):
        lg[:, :, c] = 25
    ro = torch.tensor([[0, 0, 0, eos], [5, 5, 5, eos], [0, 0, eos, pad], [0, eos, pad, pad]])
    mask = torch.tensor([[False, False, False], [False, False, False], [False, False, True], [False, True, True]])
    old = torch.full(ro.shape, float(torch.log(torch.tensor([0.25]))))
    old[1, :] = float(torch.log(torch.tensor([0.1])))
    adv = torch.tensor([2.0, 2.0, 1.0, 1.0])
    lgd = lg.to(dev).requires_grad_(True)
    obj = G.calc_grpo_objective(lgd, ro.to(dev), mask.to(dev), old.to(dev), adv.to(dev), 100, 2)
    exp_r = torch.ones(4, 3)
    exp_r[1, :] = 0.25 / 0.1
    exp_r[2, -1] = 0
    exp_r[3, 1:] = 0
    expected = ((adv.unsqueeze(1) * exp_r).sum(-1) / torch.tensor([3, 3, 2, 1])).sum() / 2
    assert torch.isfinite(obj)
    assert abs(float(obj) - float(expected)) <= 1e-6 * float(expected)
    obj.backward()
    g = lgd.grad.cpu()
    assert torch.isfinite(g).all()
    assert (g[lg == float("-inf")] == 0).all()        # -inf logits: zero gradient


def test_calc_entropy_reference_kat(dev):
    """tests/test_omr_grpo_train.py::test_calc_entropy restated."""
    from acai_omr_amd.train import grpo as G
    V, _, _ = _vocab()
    lg = torch.zeros(4, 4, V)
    lg[1] = 100
    lg[3, :, 0] = 100
    mask = torch.zeros(4, 4, dtype=torch.bool)
    mask[0, 1] = True
    mask[3, 2:] = True
    ent = G.calc_policy_theta_entropy(lg.to(dev), mask.to(dev)).cpu()
    hmax = float(torch.log(torch.tensor([V])))
    assert torch.allclose(ent, torch.tensor([hmax, hmax, hmax, 0.0]), atol=1e-5)
    bonus = G.calc_entropy_bonus(lg.to(dev), mask.to(dev), V)
    assert abs(float(bonus) - float(ent.mean()) / hmax) <= 1e-6


# ---- kernel: random cases against float64 autograd ---------------------------------------------------------------------------------------
def _case(R, T, dtype, seed, eps=0.2):
    V, pad, _ = _vocab()
    g = torch.Generator().manual_seed(seed)
    lg = (torch.randn(R, T, V, generator=g) * 2.5).to(dtype)
    lens = torch.randint(1, T + 1, (R,), generator=g)
    lens[0] = T
    mask = torch.arange(T).unsqueeze(0) >= lens.unsqueeze(1)
    if R > 3:
        mask[3] = True                       # a fully masked rollout row: len 0 -> NaN objective, as the reference; left out below
    ro = torch.randint(0, V, (R, T + 1), generator=g)
    lp_own = torch.gather(torch.log_softmax(lg.float(), -1), -1, ro[:, 1:].unsqueeze(-1)).squeeze(-1)   # theta's own fp32 log-probs
    kind = torch.randint(0, 5, (R, T), generator=g)
    off = torch.tensor([0.0, 0.1, -0.1, 0.6, -0.6])[kind]               # ratio 1, inside the band, outside on both sides
    old = torch.zeros(R, T + 1)
    old[:, 1:] = lp_own - off
    old[:, 1:][kind == 0] = lp_own[kind == 0]                           # exactly theta's fp32 log-prob: ratio 1
    adv = torch.randn(R, generator=g)
    adv[1] = 0.0
    adv[2] = -abs(float(adv[2])) - 0.5
    return lg, ro, mask, old, adv, eps


@pytest.mark.parametrize("R,T,dtype", [(8, 40, torch.float32), (8, 40, torch.bfloat16), (37, 129, torch.float32), (128, 767, torch.bfloat16),
                                       (5, 1, torch.float32)])
def test_fused_objective_vs_float64_autograd(dev, R, T, dtype):
    lg, ro, mask, old, adv, eps = _case(R, T, dtype, seed=R * 1000 + T)
    live_rows = (~mask).any(-1)
    if R > 3:   # (a len-0 rollout makes the objective NaN, as in the reference: checked separately, then dropped)
        o, _ = _fused(lg.to(dev), ro.to(dev), mask.to(dev), old.to(dev), adv.to(dev), eps, 2)
        assert torch.isnan(o)
    lg, ro, mask, old, adv = lg[live_rows], ro[live_rows], mask[live_rows], old[live_rows], adv[live_rows]
    ng = 3
    lgd = lg.to(dev).requires_grad_(True)
    obj, bonus = _fused(lgd, ro.to(dev), mask.to(dev), old.to(dev), adv.to(dev), eps, ng)
    go, gb = 0.7, -1.3
    (go * obj + gb * bonus).backward()
    l64 = lg.double().requires_grad_(True)
    robj, rbonus = ref_objective_and_bonus(l64, ro, mask, old, adv, eps, ng)
    (go * robj + gb * rbonus).backward()
    e_obj = abs(float(obj) - float(robj)) / max(1e-3, abs(float(robj)))
    e_bon = abs(float(bonus) - float(rbonus)) / abs(float(rbonus))
    # positions whose fp32 ratio sits within a few ulps of 1 +- eps may land on the other side of the band: left out of the dlogits comparison
    lp = torch.gather(torch.log_softmax(lg.double(), -1), -1, ro[:, 1:T + 1].unsqueeze(-1)).squeeze(-1)
    ratio = torch.exp(lp - old[:, 1:T + 1].double())
    edge = ((ratio - (1 - eps)).abs() < 1e-5) | ((ratio - (1 + eps)).abs() < 1e-5)
    keep = (~edge).unsqueeze(-1).expand_as(l64)
    got, ref = lgd.grad.double().cpu(), l64.grad
    scale = float(ref.abs().max())
    e_d = float((got - ref).abs()[keep].max()) / scale
    print(f"grpo fused R={R} T={T} {dtype}: objective rel {e_obj:.2e}, bonus rel {e_bon:.2e}, dlogits max/|max| {e_d:.2e}, "
          f"{int(edge.sum())} band-edge positions left out, masked grads zero {bool((got[mask] == 0).all())}")
    assert e_obj <= 2e-5 and e_bon <= 2e-5      # measured <= 2.9e-6 / 2.7e-7 (the R = 5, T = 1 case is the largest)
    # fp32 dlogits: fp32 rounding of the formula; bf16: one bf16 rounding of each element (2^-9 relative to the element, below 4e-3 of the max)
    assert e_d <= (1e-5 if dtype == torch.float32 else 4e-3)     # measured 6.2e-7 fp32, 2.1e-3 bf16; no band-edge position was left out
    assert (got[mask] == 0).all()
    # the reductions are deterministic: a second backward gives the same bits
    lgd.grad = None
    obj2, bonus2 = _fused(lgd, ro.to(dev), mask.to(dev), old.to(dev), adv.to(dev), eps, ng)
    assert torch.equal(obj2, obj) and torch.equal(bonus2, bonus)
    (go * obj2 + gb * bonus2).backward()
    assert torch.equal(lgd.grad.cpu().double(), got)


def test_fused_objective_tie_gradient_is_autograds(dev):
    """Every in-band ratio is a torch.minimum tie (unclipped == clipped): the whole gradient flows there (0.5 + 0.5 through the clamp), and A = 0
    gives 0.  Out of band with A > 0 and ratio > 1 + eps only the clipped branch is the minimum: no gradient."""
    V, _, _ = _vocab()
    T = 3
    lg = torch.zeros(1, T, V)
    lg[0, :, 7] = 2.0
    ro = torch.tensor([[0, 7, 7, 7]])
    mask = torch.zeros(1, T, dtype=torch.bool)
    lp = float(torch.log_softmax(lg[0, 0], -1)[7])
    old = torch.tensor([[0.0, lp, lp - 0.5, lp + 0.5]])        # ratios 1 (tie), e^0.5 (above the band), e^-0.5 (below)
    adv = torch.tensor([1.0])
    lgd = lg.to(dev).requires_grad_(True)
    obj, _ = _fused(lgd, ro.to(dev), mask.to(dev), old.to(dev), adv.to(dev), 0.2, 1)
    obj.backward()
    g = lgd.grad.cpu()[0]
    l64 = lg.double().requires_grad_(True)
    ref, _ = ref_objective_and_bonus(l64, ro, mask, old, adv, 0.2, 1)
    ref.backward()
    assert torch.allclose(g.double(), l64.grad[0], atol=1e-7)
    assert float(g[0, 7]) > 0 and float(g[1].abs().max()) == 0 and float(g[2, 7]) > 0


# ---- decoder: group-shared memory ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 2, 8])
@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("ck", [False, True])
def test_decoder_memory_group_size_equals_materialised_expansion(dev, G, bf, ck):
    from acai_omr_amd.models.models import OMRDecoder
    torch.manual_seed(40 + G)
    dec = OMRDecoder(64, VOCAB, num_layers=2, hidden_dim=128, num_heads=4, mlp_dim=256, transformer_dropout=0.0).to(dev).train()
    g = torch.Generator().manual_seed(41 + G)
    B, T, S = 3, 23, 37
    R = B * G
    seqs = torch.randint(3, 227, (R, T), generator=g).to(dev)
    lens = torch.randint(1, T + 1, (R,), generator=g)
    lens[0], lens[-1] = T, 1
    lmx_mask = (torch.arange(T).unsqueeze(0) >= lens.unsqueeze(1)).to(dev)
    mem = torch.randn(B, S, 128, generator=g).to(dev)
    mem_mask = torch.zeros(B, S, dtype=torch.bool)
    mem_mask[1, 20:] = True
    mem_mask[2, 5:] = True
    mem_mask = mem_mask.to(dev)
    w = torch.randn(R, T, 227, generator=g).to(dev) * (~lmx_mask).unsqueeze(-1)
    outs = []
    for grouped in (True, False):
        dec.zero_grad(set_to_none=True)
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16, enabled=bf):
            if grouped:
                logits = dec(seqs, mem, lmx_mask, mem_mask, checkpoint_grads=ck, memory_group_size=G)
            else:
                logits = dec(seqs, mem.repeat_interleave(G, 0), lmx_mask, mem_mask.repeat_interleave(G, 0), checkpoint_grads=ck)
        (logits.float() * w).sum().backward()
        outs.append((logits.detach().float().clone(), {n: p.grad.clone() for n, p in dec.named_parameters() if p.grad is not None}))
    (l0, g0), (l1, g1) = outs
    el = float((l0 - l1).abs().max()) / max(1.0, float(l1.abs().max()))
    worst = max(float((g0[n] - g1[n]).abs().max()) / max(1.0, float(g1[n].abs().max())) for n in g1)
    print(f"memory_group_size G={G} bf16={bf} ckpt={ck}: logits {el:.2e}, worst parameter gradient {worst:.2e}")
    assert set(g0) == set(g1) and len(g0) > 20
    assert el <= (1e-5 if not bf else 1e-2)     # measured 0 (bit-equal) in every case
    for n in g1:   # measured worst 2.9e-7 fp32, 2.9e-3 bf16.  Split-K float atomics and the group's dK / dV summation order (bf16: the rounding of the bf16 operands on top)
        assert float((g0[n] - g1[n]).abs().max()) <= (2e-5 if not bf else 2e-2) * max(1.0, float(g1[n].abs().max())), n


def test_decoder_memory_group_size_vs_float64_oracle(dev):
    """fp32 grouped logits against oracle.decoder_forward_tf in float64 on the expanded memory."""
    from acai_omr_amd.models.models import OMRDecoder
    from oracle import vitomr_oracle as O
    torch.manual_seed(50)
    dec = OMRDecoder(64, VOCAB, num_layers=2, hidden_dim=128, num_heads=4, mlp_dim=256, transformer_dropout=0.0).to(dev).eval()
    g = torch.Generator().manual_seed(51)
    B, G, T, S = 2, 3, 11, 19
    seqs = torch.randint(3, 227, (B * G, T), generator=g)
    lens = [11, 4, 1, 9, 11, 6]
    lmx_mask = torch.arange(T).unsqueeze(0) >= torch.tensor(lens).unsqueeze(1)
    mem = torch.randn(B, S, 128, generator=g)
    mem_mask = torch.zeros(B, S, dtype=torch.bool)
    mem_mask[1, 12:] = True
    with torch.no_grad():
        got = dec(seqs.to(dev), mem.to(dev), lmx_mask.to(dev), mem_mask.to(dev), memory_group_size=G).cpu()
    sd = {"decoder." + k: v.detach().cpu().double() for k, v in dec.state_dict().items()}
    lens_s = [int((~mem_mask[b]).sum()) for b in range(B)]
    mem_x = torch.cat([mem[b, :lens_s[b]] for b in range(B) for _ in range(G)]).double()
    inp = torch.cat([seqs[r, :lens[r]] for r in range(B * G)])
    ref = O.decoder_forward_tf(inp, mem_x, lens, [lens_s[r // G] for r in range(B * G)], sd, 4, "fp64")
    o = 0
    for r in range(B * G):
        d = float((got[r, :lens[r]].double() - ref[o:o + lens[r]]).abs().max())
        assert d <= 1e-4 * max(1.0, float(ref.abs().max())), (r, d)
        o += lens[r]


# ---- the full step -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lambda_ce", [0.1, 0.0])
def test_grpo_update_matches_a_reference_step(dev, lambda_ce):
    """One grpo_update (update_epochs = 1, plain SGD so that the parameter change IS the clipped gradient) against the same step built from
    unshared decoder passes, the float64 formulas, OMRCELoss and torch's clip_grad_norm_; the loss also against the materialised expansion."""
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
    loss, ce, rew, _ = G.grpo_update(old, theta, opt, batch, conf, ce_fn, "cuda", reward_fn=_reward_fn, uniforms=uniforms)

    # the reference step on the materialised expansion (same rollouts: same old policy, same uniforms)
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        lat, lmask = old.encoder([i.to(dev) for i in fx["imgs"]])
        lat = old.transition_head(lat)
        lat_x, lmask_x = old.expand_img_latent_for_rollout(lat, lmask, Gs)
        ro, olp, rmask = old.cached_forward_rollout_policy(lat_x, lmask_x, max_actions, 20, 1.1, group_size=Gs, uniforms=uniforms)
    tx = G.expand_target_lmx_seqs([t.to(dev) for t in targets], Gs, pad, dev)
    rg = _reward_fn(ro, rmask, tx, batch).float()
    adv = ((rg - rg.mean(-1, keepdim=True)) / (rg.std(-1, keepdim=True) + 1e-8)).view(-1)
    rs, am = old.prepare_rollouts_for_policy_theta(ro, rmask)
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        # the materialised expansion: its logits differ from the group-shared pass's by bf16 rounding of the K / V projection (a GEMM over
        # G times the rows); the ratios of a rollout taken under the cached decode's position quirk are far from 1 and amplify that, so the loss
        # is held to it and the gradients to the group-shared pass WITHOUT the shared-K/V context (no fused dK / dV accumulation, its own CE pass)
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
    # (one backward through both passes: they share the weight casts)
    ((logits.float() * l64.grad.to(dev).float()).sum() + lambda_ce * ref_ce).backward()
    torch.nn.utils.clip_grad_norm_(ref_theta.parameters(), max_norm=1.0)
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        ro_g = G._rollouts_grouped(old, lat, lmask, Gs, conf.rollout_config, uniforms)
    fobj, fbon = G.calc_grpo_objective_and_entropy_bonus(logits.detach(), ro, am, olp, adv, 0.2, len(batch))
    print(f"grpo_update lambda_ce={lambda_ce}: loss {loss:.6f} vs {float(rloss64):.6f}, ce {ce:.5f} vs {float(ref_ce):.5f}; "
          f"rollouts equal {torch.equal(ro_g[0], ro)}, log-probs equal {torch.equal(ro_g[1], olp)}; fused on the reference logits "
          f"{float(fobj):.6f} / {float(fbon):.6f} vs {float(robj):.6f} / {float(rbon):.6f}")
    print(f"  materialised expansion: loss {xloss:.6f}")
    assert abs(loss - xloss) <= 2e-3 * max(1.0, abs(xloss))    # measured 8.5e-4 relative
    assert abs(loss - float(rloss64)) <= 1e-5 * max(1.0, abs(float(rloss64)))
    assert abs(ce - float(ref_ce)) <= 1e-3 * max(1.0, abs(float(ref_ce)))
    names = ["unembed.weight", "unembed.bias", "decoder_blocks.layers.0.multihead_attn.in_proj_weight", "decoder_blocks.layers.1.linear1.weight",
             "decoder_blocks.layers.1.self_attn.out_proj.weight", "decoder_blocks.norm.weight", "vocab_embedding.weight", "pos_embedding"]
    rp = dict(ref_theta.decoder.named_parameters())
    for n, p in theta.decoder.named_parameters():
        if n in names:
            rg_ = rp[n].grad                                           # SGD: the parameter change is the clipped gradient
            err = float(((before[n] - p.detach()) / lr - rg_).abs().max()) / max(1e-6, float(rg_.abs().max()))
            print(f"  {n}: gradient rel {err:.2e}")
            assert err <= 5e-2, n    # measured 2e-5 ... 2.7e-3 (vocab_embedding)


def test_refresh_old_policy_refreshes_the_decode_engine(dev):
    """After grpo_update + refresh_old_policy the old policy (its decode engine live since the rollouts) samples what a fresh deep copy of it
    samples with the same uniforms: the engine's weight copies followed the in-place refresh."""
    from acai_omr_amd.models.models import OMRCELoss
    from acai_omr_amd.train import grpo as G
    fx, old, theta, Gs, cfg = _models(dev)
    _, pad, _ = _vocab()
    g = torch.Generator().manual_seed(70)
    max_actions = cfg["max_len"] - 2
    R = len(fx["imgs"]) * Gs
    uniforms = torch.rand(R, max_actions, generator=g).to(dev)
    targets = [torch.randint(3, 227, (n,), generator=g) for n in (9, 5, 12)]
    batch = [(img, t, "") for img, t in zip(fx["imgs"], targets)]
    conf = G.GRPOConfig(G.RolloutConfig(Gs, max_actions, 20, 1.1), G.INITIAL_REWARD_CONFIG, G.LossConfig(0.05, 0.1), G.UpdateConfig(0.2, 2, 1.0), 100, 100)
    opt = torch.optim.AdamW(theta.parameters(), lr=3e-2)
    G.grpo_update(old, theta, opt, batch, conf, OMRCELoss(pad), "cuda", reward_fn=_reward_fn, uniforms=uniforms)
    G.refresh_old_policy(old, theta)
    for n, p in theta.decoder.state_dict().items():
        assert torch.equal(old.decoder.state_dict()[n], p), n
    fresh = copy.deepcopy(old)

    def roll(m):
        with torch.no_grad(), torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            lat, lmask = m.encoder([i.to(dev) for i in fx["imgs"]])
            lat = m.transition_head(lat)
            lx, mx = m.expand_img_latent_for_rollout(lat, lmask, Gs)
            return m.cached_forward_rollout_policy(lx, mx, max_actions, 20, 1.1, group_size=Gs, uniforms=uniforms)
    a, b = roll(old), roll(fresh)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    assert torch.equal(a[1], b[1])
