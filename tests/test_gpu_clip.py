"""Clipping by the global gradient norm inside the fused AdamW step, on the GPU: `ops.grad_norm` (acai_grad_norm) against float64 sums at
the edges of its launch geometry, `FusedAdamW(max_grad_norm=...)` (acai_adamw_step_clipped) against the float64 restatement of
tests/clip_reference.py and against torch's own clip + AdamW on the device, the non-finite guard, the untouched default step, and the
`grpo_update(fused_clip=True)` glue."""
import ctypes
import functools
import math

import pytest
import torch

import clip_reference as C
import row_reference as R
from decode_support import _models, _reward_fn, _vocab
from test_gpu_row_kernels import P_BAR, V_BAR, offset_view, within

pytestmark = pytest.mark.gpu

CHUNK = 16384


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from acai_omr_amd import _lib
    _lib.lib()
    return "cuda"


def ulps(got, ref):
    """|got - ref| in units of one fp32 ulp of ref (relative 2^-23); 0 where both are 0.  <= 1 passes: an fp64 sum of at most 2^27 non-negative
    terms errs by at most 2^-26 relative, so the fp32 rounding of the result (half an ulp) dominates."""
    got, ref = got.detach().double().cpu().reshape(-1), torch.as_tensor(ref, dtype=torch.float64).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(((got - ref).abs() / (C.ULP32 * ref.abs()).clamp_min(1e-300)).max())


# ---- the norm ----------------------------------------------------------------------------------------------------------------------------------
def _norm_case(dev, tensors, offset):
    from acai_omr_amd import ops
    on_dev = [offset_view(t, dev, offset) for t in tensors]
    for t in on_dev:
        assert t.is_contiguous() and (t.data_ptr() % 16 == 0) == (offset == 0)
    total, per = ops.grad_norm(on_dev, per_tensor=True)
    assert total.dim() == 0 and total.dtype == torch.float32 and total.is_cuda and per.shape == (len(tensors),) and per.dtype == torch.float32
    assert ulps(per, C.tensor_norms(tensors)) <= 1.0
    assert ulps(total, C.global_norm(tensors)) <= 1.0
    total2, per2 = ops.grad_norm(on_dev, per_tensor=True)
    assert torch.equal(total, total2) and torch.equal(per, per2)          # fixed summation order: bitwise repeatable
    alone = ops.grad_norm(on_dev)
    assert torch.equal(alone, total)
    half = ops.grad_norm(on_dev, grad_scale=-0.5)
    assert ulps(half, 0.5 * C.global_norm(tensors)) <= 1.0
    return total, per


@pytest.mark.parametrize("offset", [0, 3], ids=["aligned", "unaligned"])
def test_grad_norm_chunk_edges(dev, offset):
    """Sizes around the 16384-element chunk, 16-byte aligned (vector loads) and as views three elements into a buffer (scalar loads).
    All-ones tensors give sqrt(n): a lost or doubled element moves the norm by 1 / (2 n) relative, more than the bar for every n here."""
    g = torch.Generator().manual_seed(5)
    _norm_case(dev, [torch.randn(n, generator=g) for n in R.ADAMW_SIZES], offset)
    assert 1.0 / (2 * sum(R.ADAMW_SIZES)) > C.ULP32
    total, per = _norm_case(dev, [torch.ones(n) for n in R.ADAMW_SIZES], offset)
    assert ulps(per, [math.sqrt(n) for n in R.ADAMW_SIZES]) <= 1.0 and ulps(total, math.sqrt(sum(R.ADAMW_SIZES))) <= 1.0
    total, per = _norm_case(dev, [torch.zeros(n) for n in R.ADAMW_SIZES], offset)
    assert float(total) == 0.0 and not bool(per.any())


def test_grad_norm_many_tensors(dev):
    """300 tensors of 1 to 7 elements: more tensors than the reducing workgroup has waves or threads."""
    g = torch.Generator().manual_seed(6)
    _norm_case(dev, [torch.randn(1 + i % 7, generator=g) for i in range(300)], 0)
    total, per = _norm_case(dev, [torch.ones(1 + i % 7) for i in range(300)], 3)
    assert ulps(per, [math.sqrt(1 + i % 7) for i in range(300)]) <= 1.0


def test_grad_norm_many_chunks(dev):
    """One tensor of 257 chunks and 5 elements (more chunks than a wave of the reducing workgroup has lanes, four times over) between two small
    ones.  What can go wrong here and not at the chunk-edge sizes is a chunk's partial sum that is lost or counted twice: on all-ones data it
    moves the norm by CHUNK / (2 n) = 1.9e-3 relative, and the 5-element last chunk by 5 / (2 n) = 5.9e-7, five times the bar."""
    n = CHUNK * 257 + 5
    assert 5.0 / (2 * (n + 4)) > 4 * C.ULP32
    g = torch.Generator().manual_seed(7)
    _norm_case(dev, [torch.randn(3, generator=g), torch.randn(n, generator=g), torch.randn(1, generator=g)], 0)
    total, per = _norm_case(dev, [torch.ones(3), torch.ones(n), torch.ones(1)], 3)
    assert ulps(per, [math.sqrt(3), math.sqrt(n), 1.0]) <= 1.0 and ulps(total, math.sqrt(n + 4)) <= 1.0


def test_grad_norm_refuses_what_it_cannot_run(dev):
    from acai_omr_amd import ops
    for bad in ([torch.zeros(4)], [torch.zeros(4, device=dev, dtype=torch.bfloat16)], [torch.zeros(4, 4, device=dev)[:, 1]], []):
        with pytest.raises(RuntimeError):
            ops.grad_norm(bad)


# ---- the clipped step --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(case, max_norm, grad_scale=1.0):
    params, grads, hyper = R.adamw_case(case)
    return (params, grads, hyper) + C.clipped_adamw_run(params, grads, hyper, max_norm, grad_scale)


def _run_clipped(dev, case, max_norm, aligned, grad_scale=1.0, against_torch=True):
    from acai_omr_amd.optim import FusedAdamW
    params, grads, hyper, p64, m64, v64, steps, norms, coefs = _reference(case, max_norm, grad_scale)
    off_p, off_g = (0, 0) if aligned else (1, 3)
    mine = [torch.nn.Parameter(offset_view(p, dev, off_p)) for p in params]
    theirs = [torch.nn.Parameter(p.clone().to(dev)) for p in params]
    of = FusedAdamW(R.adamw_groups(mine, hyper), max_grad_norm=max_norm)
    ot = torch.optim.AdamW(R.adamw_groups(theirs, hyper), foreach=False)
    for it, gs in enumerate(grads):
        for a, b, g in zip(mine, theirs, gs):
            a.grad = None if g is None else offset_view(g, dev, off_g)
            b.grad = None if g is None else (g * grad_scale).to(dev)
            if g is not None:
                assert a.grad.is_contiguous() and (a.grad.data_ptr() % 16 == 0) == aligned
        of.step(grad_scale=grad_scale)
        torch.nn.utils.clip_grad_norm_(theirs, max_norm=max_norm, foreach=False)
        ot.step()
        tag = (case, max_norm, aligned, it)
        assert of.grad_norm.dim() == 0 and of.grad_norm.is_cuda and of.clip_coef.is_cuda
        assert ulps(of.grad_norm, norms[it]) <= 1.0, tag
        assert torch.equal(of.clip_coef.cpu(), C.clip_coef_fp32(of.grad_norm.cpu(), max_norm)), tag      # the fp32 formula on the kernel's own norm
        per = of.grad_norms()
        present = [(a, g) for a, g in zip(mine, gs) if g is not None]
        assert len(per) == len(present), tag
        assert ulps(torch.stack([per[a] for a, _ in present]), C.tensor_norms([g for _, g in present], grad_scale)) <= 1.0, tag
    assert int(of.skipped_steps) == 0
    for i, (a, b) in enumerate(zip(mine, theirs)):
        tag = (case, max_norm, aligned, R.ADAMW_SIZES[i])
        st = of.state[a]
        assert float(st["step"]) == float(ot.state[b]["step"]) == steps[i], tag
        if against_torch:
            assert torch.allclose(a, b, **P_BAR), (tag, float((a - b).abs().max()))
            assert torch.allclose(st["exp_avg"], ot.state[b]["exp_avg"], **P_BAR), tag
            assert torch.allclose(st["exp_avg_sq"], ot.state[b]["exp_avg_sq"], **V_BAR), tag
        assert within(a, p64[i], atol=2 * P_BAR["atol"], rtol=2 * P_BAR["rtol"]) <= 1.0, tag
        assert within(st["exp_avg"], m64[i], atol=2 * P_BAR["atol"], rtol=2 * P_BAR["rtol"]) <= 1.0, tag
        assert within(st["exp_avg_sq"], v64[i], atol=2 * V_BAR["atol"], rtol=2 * V_BAR["rtol"]) <= 1.0, tag
    return of, norms, coefs


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("max_norm", C.MAX_NORMS)
@pytest.mark.parametrize("case", R.ADAMW_CASES)
def test_clipped_adamw(dev, case, max_norm, aligned):
    """Six steps of FusedAdamW(max_grad_norm=...) over the sizes and cases of test_fused_adamw: parameters, both moments and step counts against
    the float64 restatement at twice P_BAR / V_BAR (the factor test_fused_adamw allows against float64) and against torch's clip_grad_norm_ +
    AdamW on the device at once those bars; every step's norm, coefficient and per-parameter norms.  exp_avg_sq at max_norm = 1 is ~1e-5 of its
    unclipped value, so a clip that was not applied fails V_BAR outright."""
    of, norms, coefs = _run_clipped(dev, case, max_norm, aligned)
    if case == "zero_grad":
        assert float(of.grad_norm) == 0.0 and float(of.clip_coef) == 1.0


def test_clipped_adamw_with_grad_scale(dev):
    """grad_scale = 0.5 halves the norm that max_norm = 300 is compared with: step 3 (norm ~1435) still clips, the others do not."""
    of, norms, coefs = _run_clipped(dev, "default", 300.0, True, grad_scale=0.5)
    full = _reference("default", 300.0)[7]
    assert all(abs(h - 0.5 * f) <= 1e-12 * f for h, f in zip(norms, full))
    assert [c < 1.0 for c in coefs] == [False, False, True, False, False, False]


def test_step_argument_overrides_the_constructor(dev):
    """step(max_grad_norm=None) on an optimizer built with a max_grad_norm takes the plain step; step(max_grad_norm=x) on a plain one clips."""
    from acai_omr_amd.optim import FusedAdamW
    g = torch.Generator().manual_seed(3)
    w0, gr = torch.randn(1000, generator=g), torch.randn(1000, generator=g) * 5
    outs = []
    for ctor, arg in ((dict(max_grad_norm=1.0), dict(max_grad_norm=None)), (dict(), dict()), (dict(), dict(max_grad_norm=1.0)), (dict(max_grad_norm=1.0), dict())):
        p = torch.nn.Parameter(w0.clone().to(dev))
        p.grad = gr.clone().to(dev)
        o = FusedAdamW([p], lr=1e-2, **ctor)
        o.step(**arg)
        outs.append((o.state[p]["exp_avg_sq"].clone(), o.grad_norm))
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] is None and outs[1][1] is None
    assert torch.equal(outs[2][0], outs[3][0]) and outs[2][1] is not None and torch.equal(outs[2][1], outs[3][1])
    assert float(outs[2][0].sum()) < 1e-3 * float(outs[0][0].sum())


# ---- the non-finite guard ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["inf_tail", "nan_mid_chunk"])
def test_nonfinite_norm_skips_the_step(dev, where):
    """One inf in the last element of the 32769-element gradient (the scalar tail after the vector loop) or one NaN in the middle of the
    16384-element one: no parameter and no moment of ANY tensor changes, the counter moves, the next finite step updates as usual."""
    from acai_omr_amd.optim import FusedAdamW
    params, grads, hyper = R.adamw_case("default")
    idx, pos, val = (R.ADAMW_SIZES.index(32769), 32768, float("inf")) if where == "inf_tail" else (R.ADAMW_SIZES.index(16384), 8191, float("nan"))
    bad = [g.clone() for g in grads[1]]
    bad[idx][pos] = val

    def run(skip_nonfinite):
        ps = [torch.nn.Parameter(p.clone().to(dev)) for p in params]
        o = FusedAdamW(R.adamw_groups(ps, hyper), max_grad_norm=1.0, skip_nonfinite=skip_nonfinite)
        for p, g in zip(ps, grads[0]):
            p.grad = g.to(dev)
        o.step()
        before = [(p.detach().clone(), o.state[p]["exp_avg"].clone(), o.state[p]["exp_avg_sq"].clone()) for p in ps]
        for p, g in zip(ps, bad):
            p.grad = g.to(dev)
        o.step()
        return ps, o, before

    ps, o, before = run(True)
    assert not math.isfinite(float(o.grad_norm)) and int(o.skipped_steps) == 1
    for p, (w, m, v) in zip(ps, before):
        assert torch.equal(p.detach(), w) and torch.equal(o.state[p]["exp_avg"], m) and torch.equal(o.state[p]["exp_avg_sq"], v)
    assert all(float(o.state[p]["step"]) == 2 for p in ps)      # the documented wart: the host-side counts advance all the same
    for p, g in zip(ps, grads[2]):
        p.grad = g.to(dev)
    o.step()
    assert int(o.skipped_steps) == 1 and math.isfinite(float(o.grad_norm)) and float(o.clip_coef) < 1.0
    for p, (w, m, v) in zip(ps, before):
        assert not torch.equal(p.detach(), w) and bool(torch.isfinite(p).all()) and not torch.equal(o.state[p]["exp_avg_sq"], v)

    # skip_nonfinite=False is torch: clip_grad_norm_ scales by max_norm / (inf + 1e-6) = 0 (inf * 0 = NaN in that element) or by NaN (everywhere)
    ps, o, before = run(False)
    theirs = [torch.nn.Parameter(p.clone().to(dev)) for p in params]
    ot = torch.optim.AdamW(R.adamw_groups(theirs, hyper), foreach=False)
    for gs in (grads[0], bad):
        for b, g in zip(theirs, gs):
            b.grad = g.to(dev)
        torch.nn.utils.clip_grad_norm_(theirs, max_norm=1.0, foreach=False)
        ot.step()
    assert int(o.skipped_steps) == 0
    assert bool(torch.isnan(ps[idx][pos]))
    for a, b in zip(ps, theirs):
        assert torch.equal(torch.isnan(a), torch.isnan(b))
    if where == "nan_mid_chunk":
        assert all(bool(torch.isnan(a).all()) for a in ps)


# ---- the default step is untouched ---------------------------------------------------------------------------------------------------------------
def test_default_step_is_the_plain_launch(dev):
    """FusedAdamW(...).step() without a max_grad_norm equals, bit for bit, the same steps through a direct acai_adamw_step call on clones."""
    from acai_omr_amd import _lib
    from acai_omr_amd.optim import FusedAdamW
    params, grads, hyper = R.adamw_case("default")
    h = hyper[0]
    ps = [torch.nn.Parameter(p.clone().to(dev)) for p in params]
    o = FusedAdamW(ps, **h)
    w = [p.clone().to(dev) for p in params]
    m, v = [torch.zeros_like(t) for t in w], [torch.zeros_like(t) for t in w]
    ct = torch.tensor([i for i, n in enumerate(R.ADAMW_SIZES) for _ in range(0, n, CHUNK)], dtype=torch.int32, device=dev)
    co = torch.tensor([off for n in R.ADAMW_SIZES for off in range(0, n, CHUNK)], dtype=torch.int64, device=dev)
    garr = (_lib.AcaiAdamWGroup * 1)()
    garr[0].lr, garr[0].beta1, garr[0].beta2, garr[0].eps, garr[0].weight_decay = h["lr"], h["betas"][0], h["betas"][1], h["eps"], h["weight_decay"]
    gdev = torch.frombuffer(bytearray(bytes(garr)), dtype=torch.uint8).to(dev)
    for it in range(3):
        gd = [g.to(dev) for g in grads[it]]
        for p, g in zip(ps, gd):
            p.grad = g
        o.step()
        arr = (_lib.AcaiAdamWTensor * len(w))()
        for i in range(len(w)):
            arr[i].p, arr[i].g, arr[i].m, arr[i].v, arr[i].n, arr[i].group = w[i].data_ptr(), gd[i].data_ptr(), m[i].data_ptr(), v[i].data_ptr(), w[i].numel(), 0
            arr[i].bias_c1, arr[i].bias_c2_sqrt = 1.0 - h["betas"][0] ** (it + 1.0), math.sqrt(1.0 - h["betas"][1] ** (it + 1.0))
        tdev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
        _lib.check(_lib.lib().acai_adamw_step(tdev.data_ptr(), gdev.data_ptr(), ct.data_ptr(), co.data_ptr(), ct.numel(), CHUNK, 1.0,
                                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "acai_adamw_step")
        torch.cuda.synchronize()
    assert o.grad_norm is None and o.clip_coef is None and o.skipped_steps is None and o.grad_norms() is None
    for i, p in enumerate(ps):
        assert torch.equal(p.detach(), w[i]) and torch.equal(o.state[p]["exp_avg"], m[i]) and torch.equal(o.state[p]["exp_avg_sq"], v[i]), R.ADAMW_SIZES[i]


# ---- grpo_update(fused_clip=True) --------------------------------------------------------------------------------------------------------------
def _grpo_setup(dev, seed):
    from acai_omr_amd.models.models import OMRCELoss
    from acai_omr_amd.train import grpo as G
    fx, old, theta, Gs, cfg = _models(dev)
    _, pad, _ = _vocab()
    g = torch.Generator().manual_seed(seed)
    max_actions = cfg["max_len"] - 2
    uniforms = torch.rand(len(fx["imgs"]) * Gs, max_actions, generator=g).to(dev)
    targets = [torch.randint(3, 227, (n,), generator=g) for n in (9, 5, 12)]
    batch = [(img, t, "") for img, t in zip(fx["imgs"], targets)]
    conf = G.GRPOConfig(G.RolloutConfig(Gs, max_actions, 20, 1.1), G.INITIAL_REWARD_CONFIG, G.LossConfig(0.05, 0.1), G.UpdateConfig(0.2, 1, 1.0), 100, 100)
    return old, theta, batch, conf, OMRCELoss(pad), uniforms


def test_grpo_update_fused_clip(dev):
    """After one fused-clip update from zero moments, sum(exp_avg_sq) / (1 - beta2) IS the squared clipped norm: Adam's update is invariant to
    the gradients' scale, so the parameters cannot tell whether the clip happened, the second moment can.  (fp32 rounding of each v is at
    most 3 * 2^-24 relative and survives a sum of non-negative terms: 1e-6 holds.)"""
    from acai_omr_amd.optim import FusedAdamW
    from acai_omr_amd.train import grpo as G
    old, theta, batch, conf, ce_fn, uniforms = _grpo_setup(dev, 61)
    opt = FusedAdamW(theta.parameters(), lr=1e-4, betas=(0.9, 0.95))
    G.grpo_update(old, theta, opt, batch, conf, ce_fn, "cuda", reward_fn=_reward_fn, uniforms=uniforms, fused_clip=True)
    norm, coef = opt.grad_norm.cpu(), opt.clip_coef.cpu()
    assert math.isfinite(float(norm)) and float(norm) > 0.0 and int(opt.skipped_steps) == 0
    assert torch.equal(coef, C.clip_coef_fp32(norm, 1.0))
    total = sum(float(st["exp_avg_sq"].double().sum()) for st in opt.state.values())
    clipped = math.sqrt(total / float(torch.tensor(1.0) - torch.tensor(0.95)))       # 1 - beta2 as the kernel forms it, in fp32
    print(f"grpo fused clip: norm {float(norm):.6g}, coefficient {float(coef):.6g}, clipped norm from the second moments {clipped:.8g}")
    assert abs(clipped - float(coef) * float(norm)) <= 1e-6 * float(coef) * float(norm)
    assert len(opt.grad_norms()) == len(opt.state) > 0


def test_grpo_update_default_still_clips_through_torch(dev):
    from acai_omr_amd.optim import FusedAdamW
    from acai_omr_amd.train import grpo as G
    old, theta, batch, conf, ce_fn, uniforms = _grpo_setup(dev, 62)
    with pytest.raises(ValueError):
        G.grpo_update(old, theta, torch.optim.SGD(theta.parameters(), lr=1e-2), batch, conf, ce_fn, "cuda", reward_fn=_reward_fn, uniforms=uniforms,
                      fused_clip=True)
    opt = FusedAdamW(theta.parameters(), lr=1e-4)
    G.grpo_update(old, theta, opt, batch, conf, ce_fn, "cuda", reward_fn=_reward_fn, uniforms=uniforms)
    assert opt.grad_norm is None and opt.clip_coef is None and opt.skipped_steps is None and len(opt.state) > 0
