"""tests/row_reference.py on the CPU: the hand-written float64 references equal torch's float64 autograd, the probe inputs have the exactness
the GPU tests (tests/test_gpu_row_kernels.py) rely on, a plain fp32 evaluation of each formula stays inside each bar, and every defect the
GPU tests are meant to catch moves the reference by at least four times the bar of the case that catches it."""
import math

import pytest
import torch
import torch.nn.functional as F

import row_reference as R

EPS = 1e-5
DX_BAR = dict(atol=2e-5, rtol=1e-4)
DW_BAR = dict(atol=2e-3, rtol=1e-4)
P_BAR = dict(rtol=2e-6, atol=2e-7)
V_BAR = dict(rtol=1e-5, atol=1e-12)
MAE_CASES = [(1, 2), (5, 12), (4095, 64), (4096, 256), (4100, 65), (65539, 12)]


def excess(got, ref, atol, rtol=0.0):
    return float(((got.double() - ref.double()).abs() / (atol + rtol * ref.double().abs())).max())


# ---- the references equal torch's float64 autograd -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,dim", [(1, 10), (5, 96), (130, 256), (37, 1280)])
def test_layernorm_reference_is_autograd(rows, dim):
    x, w, b, dy = (t.double() for t in R.ln_inputs(rows, dim, seed=rows + dim))
    xr, wr, br = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    y = F.layer_norm(xr, (dim,), wr, br, EPS)
    y.backward(dy)
    dx, dw, db = R.layernorm_bwd(x, w, dy, EPS)
    assert torch.allclose(R.layernorm_fwd(x, w, b, EPS), y.detach(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(dx, xr.grad, rtol=1e-10, atol=1e-12) and torch.allclose(dw, wr.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(db, br.grad, rtol=1e-12, atol=1e-12)


def test_gelu_reference_is_autograd():
    x = torch.linspace(-8, 8, 4001, dtype=torch.float64).requires_grad_()
    y = F.gelu(x)
    y.sum().backward()
    assert torch.allclose(R.gelu(x.detach()), y.detach(), rtol=0, atol=1e-15)
    assert torch.allclose(R.gelu_grad(x.detach()), x.grad, rtol=0, atol=1e-15)
    # the left tail keeps its relative accuracy (1 + erf would return 0 below -8.3): x Phi(x) ~ -phi(x) (1 - 1 / x^2)
    t = torch.tensor([-10.0, -13.0], dtype=torch.float64)
    asym = -torch.exp(-0.5 * t * t) / math.sqrt(2 * math.pi) * (1 - 1 / t ** 2 + 3 / t ** 4)
    assert torch.allclose(R.gelu(t), asym, rtol=2e-3, atol=0)


@pytest.mark.parametrize("smoothing", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("mode", R.CE_IGNORE_MODES)
def test_ce_reference_is_torch(smoothing, mode):
    for rows, V, s, c in [(1, 5, 1.0, 0.0), (5, 63, 1.0, 80.0), (131, 65, 30.0, 0.0), (4, 300, 1.0, -80.0)]:
        logits, target, ignore, count = R.ce_inputs(rows, V, s, c, mode, seed=rows + V)
        lg = logits.double().requires_grad_()
        ref = F.cross_entropy(lg, target, ignore_index=ignore, label_smoothing=smoothing, reduction="sum") / count
        ref.backward()
        loss, dl = R.ce_loss(logits, target, ignore, count, smoothing)
        assert abs(float(loss) - float(ref.detach())) <= 1e-12 * max(1.0, abs(float(ref.detach())))
        assert torch.allclose(dl, lg.grad, rtol=1e-10, atol=1e-14)
        if count == int((target != ignore).sum()):
            mean = F.cross_entropy(logits.double(), target, ignore_index=ignore, label_smoothing=smoothing)
            assert abs(float(loss) - float(mean)) <= 1e-12 * max(1.0, abs(float(mean)))


@pytest.mark.parametrize("rows,dim", [(1, 2), (5, 12), (130, 65)])
def test_mae_reference_is_autograd(rows, dim):
    pred, target = (t.double() for t in R.mae_inputs(rows, dim, seed=rows))
    mask = R.mae_mask(rows, "random", seed=rows)
    count = int(mask.sum())
    p = pred.clone().requires_grad_()
    that = (target - target.mean(-1, keepdim=True)) / (target.var(-1, keepdim=True) + 1e-6) ** 0.5       # Tensor.var: unbiased
    ref = (((p - that) ** 2).mean(-1) * mask.double()).sum() / count
    ref.backward()
    loss, dp = R.mae_loss(pred, target, mask, count)
    assert abs(float(loss) - float(ref.detach())) <= 1e-12 * max(1.0, float(ref.detach())) and torch.allclose(dp, p.grad, rtol=1e-10, atol=1e-14)


@pytest.mark.parametrize("mode", ["absent", "quarter", "all", "free"])
def test_scatter_reference_is_index_add(mode):
    for rows, dim in [(1, 4), (65, 10), (300, 24)]:
        src, idx, dst, shared = R.scatter_inputs(rows, dim, mode, seed=rows)
        assert R.scatter_precondition_ok(idx, shared, dst.shape[0])
        ref = dst.double().index_add_(0, idx.long(), src.double())
        assert torch.equal(R.scatter_add_rows(src, idx, dst), ref)
        if mode in ("absent", "quarter") and rows >= 3:
            assert 0 in idx.tolist() and dst.shape[0] - 1 in idx.tolist()
        n_shared = int((idx == shared).sum())
        assert n_shared == {"absent": 0, "quarter": max(1, rows // 4), "all": rows, "free": 0}[mode]
    assert not R.scatter_precondition_ok(torch.tensor([0, 2, 2, 1]), 1, 3) and not R.scatter_precondition_ok(torch.tensor([0, 3]), -1, 3)


@pytest.mark.parametrize("case", R.ADAMW_CASES)
def test_adamw_reference_is_torch(case):
    """The hand-written float64 AdamW equals torch.optim.AdamW in float64, and torch's own fp32 AdamW stays within ONE times the bars the GPU
    test holds FusedAdamW to against torch (it holds it to the float64 reference at twice those bars)."""
    params, grads, hyper = R.adamw_case(case)
    p64, m64, v64, steps = R.adamw_run(params, grads, hyper)
    for dtype in (torch.float64, torch.float32):
        ps = [torch.nn.Parameter(p.to(dtype)) for p in params]
        opt = torch.optim.AdamW(R.adamw_groups(ps, hyper), foreach=False)
        for gs in grads:
            for p, g in zip(ps, gs):
                p.grad = None if g is None else g.to(dtype)
            opt.step()
        for i, p in enumerate(ps):
            assert float(opt.state[p]["step"]) == steps[i]
            if dtype == torch.float64:
                assert torch.allclose(p.detach(), p64[i], rtol=1e-12, atol=1e-14)
                assert torch.allclose(opt.state[p]["exp_avg"], m64[i], rtol=1e-12, atol=1e-14)
                assert torch.allclose(opt.state[p]["exp_avg_sq"], v64[i], rtol=1e-12, atol=1e-16)
            else:
                assert excess(p.detach(), p64[i], **P_BAR) <= 1.0, (case, i, excess(p.detach(), p64[i], **P_BAR))
                assert excess(opt.state[p]["exp_avg_sq"], v64[i], **V_BAR) <= 1.0, (case, i)
                if hyper[i]["lr"] == 0.0:
                    assert torch.equal(p.detach(), params[i]) and bool(opt.state[p]["exp_avg"].any())
    if case == "skip":
        assert steps == [6, 6, 4, 6, 6, 6, 6]
    if case == "lr0":
        assert [h["lr"] == 0.0 for h in hyper] == [False, True] * 3 + [False] and len(R.adamw_groups(params, hyper)) == 2


# ---- the probe inputs are as exact as the GPU tests need them ----------------------------------------------------------------------------------
def test_integer_inputs_sum_exactly_in_fp32():
    """At the largest exact-integer shape every order of fp32 additions gives the float64 sum, and bf16 holds the values."""
    x = R.int_tensor((R.INT_ROWS_MAX, 260), seed=1)
    assert float(x.min()) == -8 and float(x.max()) == 8 and torch.equal(x, x.round())
    assert torch.equal(x.to(torch.bfloat16).float(), x)
    ref = R.colsum(x)
    assert R.INT_ROWS_MAX * 8 + 8 < 2 ** 24 and float(x.abs().sum(0).max()) + 8 < 2 ** 24
    g = torch.Generator().manual_seed(2)
    for order in (torch.arange(x.shape[0]), torch.randperm(x.shape[0], generator=g), torch.argsort(x[:, 0])):
        xs = x[order]
        assert torch.equal(xs.sum(0).double(), ref)                          # torch's blocked fp32 sum
        assert torch.equal(xs.cumsum(0)[-1].double(), ref)                    # strictly sequential
        assert torch.equal(xs.view(-1, 16, 260).sum(1).sum(0).double(), ref)  # chunked
    pre = R.int_tensor((260,), seed=3)
    assert torch.equal((pre + x.sum(0)).double(), R.colsum(x, out=pre))


@pytest.mark.parametrize("rows,dim", [(5, 10), (1037, 256), (8200, 1024)])
def test_loud_row_zeroes_every_other_row(rows, dim):
    """One loud row in dy: in a plain fp32 evaluation every other row's dx is +-0 and db is dy[r] bit for bit, dw one product."""
    x, w, b, dy = R.ln_inputs(rows, dim, seed=rows)
    rpb = R.ln_rows_per_block(rows, dim)
    rows_l = R.loud_rows(rows, rpb)
    assert rows_l[0] == 0 and rows_l[-1] == rows - 1 and all(r in rows_l for r in (3, 4, rpb - 1, rpb) if r < rows)
    dx_full, _, _ = R.layernorm_bwd(x, w, dy, EPS, dtype=torch.float32)
    for r in rows_l[:2] + rows_l[-1:]:
        dx, dw, db = R.layernorm_bwd(x, w, R.one_row(dy, r), EPS, dtype=torch.float32)
        quiet = torch.ones(rows, dtype=torch.bool)
        quiet[r] = False
        assert not bool(dx[quiet].any()) and torch.equal(dx[r], dx_full[r]) and torch.equal(db, dy[r])
        assert int((dw != 0).sum()) == dim


def test_launch_geometry():
    assert [R.ln_rows_per_block(r, 256) for r in (1, 5, 1037, 8192, 8193, 8200)] == [4, 4, 4, 4, 8, 8]
    assert R.ln_rows_per_block(5, 96) == 2048 and R.ln_rows_per_block(5, 1280) == 2048 and R.ln_rows_per_block(5, 512, aligned=False) == 2048
    assert [R.mae_rows_per_wave(r) for r in (1, 4095, 4096, 65535, 65536)] == [1, 1, 4, 4, 16]
    assert R.colsum_rows_per_block(8208, 256, 256, 4) == 64 and R.colsum_rows_per_block(77, 256, 256, 4) == 64
    assert R.colsum_rows_per_block(8208, 70, 70, 4) == 2048
    assert R.colsum_vec(256, 260, 4) and not R.colsum_vec(70, 70, 4) and not R.colsum_vec(64, 69, 4) and R.colsum_vec(504, 520, 2)
    assert R.mae_onehot_rows(65539) == [0, 3, 4, 15, 16, 63, 64, 65538] and R.mae_onehot_rows(1) == [0]
    assert R.all_finite_bf16().numel() == 65280 and R.gelu_points().numel() == 400009


@pytest.mark.parametrize("rows,dim", MAE_CASES)
def test_mae_inputs(rows, dim):
    """The constant row's deviations are exact zeros and the near-constant row's are exactly +-2^-10 (or 0) in fp32, whatever the order of the
    sum; the near-constant row's variance is the size of the 1e-6 it is added to."""
    pred, target = R.mae_inputs(rows, dim, seed=rows + dim)
    if rows > 1:
        assert torch.equal(target[1], torch.full((dim,), 0.75))
    if rows > 2:
        g = torch.Generator().manual_seed(0)
        for row in (target[2], target[2][torch.randperm(dim, generator=g)], target[2].flip(0)):
            assert float(row.cumsum(0)[-1]) == 0.75 * dim and float(row.sum() / dim) == 0.75
        dev = target[2] - 0.75
        assert set(dev.abs().tolist()) <= {0.0, R.MAE_NEAR} and float(dev.sum()) == 0.0
        var = float((dev.double() ** 2).sum() / (dim - 1))
        assert 0.5e-6 < var < 2e-6
    m = R.mae_mask(rows, "random", seed=rows)
    assert bool(m[:3].all()) and (rows < 100 or 0.7 < float(m.float().mean()) < 0.8)


# ---- a plain fp32 evaluation stays inside each bar ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,dim", [(5, 10), (130, 96), (1037, 256), (1037, 1024), (130, 1280)])
def test_layernorm_fp32_inside_bars(rows, dim):
    x, w, b, dy = R.ln_inputs(rows, dim, seed=rows * 4099 + dim)
    ref, got = R.layernorm_bwd(x, w, dy, EPS), R.layernorm_bwd(x, w, dy, EPS, dtype=torch.float32)
    assert excess(got[0], ref[0], **DX_BAR) <= 0.5 and excess(got[1], ref[1], **DW_BAR) <= 0.5 and excess(got[2], ref[2], **DW_BAR) <= 0.5
    dyi = R.int_tensor((rows, dim), seed=rows + dim)
    ref, got = R.layernorm_bwd(x, w, dyi, EPS), R.layernorm_bwd(x, w, dyi, EPS, dtype=torch.float32)
    assert excess(got[1], ref[1], **DW_BAR) <= 0.5 and torch.equal(got[2].double(), ref[2])


@pytest.mark.parametrize("rows,dim", MAE_CASES)
def test_mae_fp32_inside_bars(rows, dim):
    """Below 0.05 of the loss bar and 0.2 of the gradient bar on these inputs."""
    pred, target = R.mae_inputs(rows, dim, seed=rows + dim)
    kinds = ["random", "ones"] + [("onehot", r) for r in R.mae_onehot_rows(rows)]
    for kind in kinds:
        mask = R.mae_mask(rows, kind, seed=rows)
        count = max(1, int(mask.sum()))
        (l64, d64), (l32, d32) = R.mae_loss(pred, target, mask, count), R.mae_loss(pred, target, mask, count, dtype=torch.float32)
        assert abs(float(l32) - float(l64)) <= 0.05 * 1e-5 * max(1.0, abs(float(l64))), kind
        assert excess(d32, d64, atol=1e-5 * float(d64.abs().max())) <= 0.2, kind
        assert not bool(d64[mask == 0].any())
    l0, d0 = R.mae_loss(pred, target, R.mae_mask(rows, "zeros"), 1)
    assert float(l0) == 0.0 and not bool(d0.any())


@pytest.mark.parametrize("V", [5, 63, 64, 65, 227, 300])
def test_ce_fp32_inside_bars(V):
    """Below 0.2 of both bars over the whole grid of the GPU test."""
    worst_l = worst_g = 0.0
    for rows in (1, 3, 4, 5, 131):
        for si, (s, c) in enumerate(((1.0, 0.0), (1.0, 80.0), (1.0, -80.0), (30.0, 0.0))):
            for mode in R.CE_IGNORE_MODES:
                logits, target, ignore, count = R.ce_inputs(rows, V, s, c, mode, seed=V * 1000 + rows * 10 + si)
                assert count == int((target != ignore).sum()) >= 1 and bool(((target >= 0) & (target < V) | (target == ignore)).all())
                assert (mode == "none") == (ignore == -100) and (mode != "all_but_one" or count == 1)
                for e in (0.0, 0.1, 1.0):
                    (l64, d64), (l32, d32) = R.ce_loss(logits, target, ignore, count, e), R.ce_loss(logits, target, ignore, count, e, dtype=torch.float32)
                    l_bar, g_bar = R.ce_bars(logits, l64, count)
                    worst_l, worst_g = max(worst_l, abs(float(l32) - float(l64)) / l_bar), max(worst_g, excess(d32, d64, atol=g_bar))
                    assert not bool(d64[target == ignore].any())
    assert worst_l <= 0.2 and worst_g <= 0.2, (worst_l, worst_g)


def test_ce_bars_reduce_to_the_project_bars():
    l_bar, g_bar = R.ce_bars(torch.tensor([[1.0, -1.0]]), 0.5, 1)
    assert abs(l_bar - 1e-5) < 1e-6 and abs(g_bar - 1e-6) < 3e-7


def test_gelu_fp32_inside_bars():
    x = R.gelu_points()
    assert bool(torch.isfinite(x).all()) and float(x[:400001].min()) == -20 and float(x[:400001].max()) == 20
    assert excess(R.gelu(x, dtype=torch.float32), R.gelu(x), atol=1e-6, rtol=2 * R.EPS32) <= 0.5
    assert excess(R.gelu_grad(x, dtype=torch.float32), R.gelu_grad(x), atol=1e-5, rtol=1e-6) <= 0.5


def test_gelu_bf16_bar():
    """Why the bf16 bar has an absolute floor.  The plain fp32 evaluation in the shape of the backward kernel, Phi(x) = 0.5 (1 + erf(x / sqrt 2)),
    misses one bf16 ulp of the reference only below x = -4.375, where the cancellation leaves an absolute error of about eps32 in a value below
    1e-5, and stays inside one ulp + GELU_BF16_FLOOR everywhere."""
    xb = R.all_finite_bf16()
    x32, x64 = xb.float(), xb.double()
    got = (0.5 * (1.0 + torch.erf(x32 * 0.70710678118654752440)) + x32 * 0.39894228040143267794 * torch.exp(-0.5 * x32 * x32)).to(torch.bfloat16)
    rb = R.round_bf16(R.gelu_grad(x64))
    over = (got.double() - rb).abs() > R.bf16_ulp(rb)
    assert bool(over.any()) and float(x64[over].max()) < -4.375 and not bool(over[R.bf16_ulp(rb) >= R.GELU_BF16_FLOOR].any())
    assert R.gelu_bf16_excess(got, R.gelu_grad(x64)) <= 1.0
    assert R.gelu_bf16_excess(R.gelu(x64, dtype=torch.float32).to(torch.bfloat16), R.gelu(x64)) <= 1.0
    assert float(R.bf16_ulp(torch.tensor([1.0, 1.5, 0.0, 3e-5], dtype=torch.float64))[0]) == 2.0 ** -7
    live = (R.gelu(x64).abs() > 1e-4)
    assert bool((R.bf16_ulp(R.round_bf16(R.gelu(x64)))[live] > 0.3 * R.GELU_BF16_FLOOR).all())


# ---- every defect moves the reference by at least four bars of the case meant to catch it --------------------------------------------------------
@pytest.mark.parametrize("defect", ["drop_last_row", "double_first_row"])
def test_row_defects_show(defect):
    # column sums and db on integer data: the comparison is exact, a lost or doubled row moves some column by a whole number
    for rows, cols, es in [(64, 256, 4), (65, 70, 4), (8208, 256, 4), (2049, 70, 4), (17, 512, 2)]:
        x = R.int_tensor((rows, cols), seed=rows)
        chunk = R.colsum_rows_per_block(rows, cols, cols, es)
        assert float((R.colsum(x, chunk=chunk, defect=defect) - R.colsum(x)).abs().max()) >= 1.0
    for rows, dim in [(5, 256), (1037, 512), (8200, 1024), (2049, 96), (130, 10)]:
        x, w, b, dy = R.ln_inputs(rows, dim, seed=rows)
        rpb = R.ln_rows_per_block(rows, dim)
        dyi = R.int_tensor((rows, dim), seed=rows + dim)
        assert float((R.layernorm_bwd(x, w, dyi, EPS, chunk=rpb, defect=defect)[2] - R.layernorm_bwd(x, w, dyi, EPS)[2]).abs().max()) >= 1.0
        # the loud row that sits on the defect: db is dy[r] against 0 or 2 dy[r]; dw moves by a whole product against a bar of 2e-5 + 1e-4 |dw|
        r = min(rpb, rows) - 1 if defect == "drop_last_row" else (rpb if rpb < rows else 0)
        assert r in R.loud_rows(rows, rpb)
        dyl = R.one_row(dy, r)
        _, dw, db = R.layernorm_bwd(x, w, dyl, EPS)
        _, dwd, dbd = R.layernorm_bwd(x, w, dyl, EPS, chunk=rpb, defect=defect)
        assert not torch.equal(db, dbd) and torch.equal((db - dbd).abs(), dy[r].double().abs())
        moved = (dw - dwd).abs() >= 4 * (DX_BAR["atol"] + DX_BAR["rtol"] * dw.abs())
        assert float(moved.double().mean()) > 0.99
    for rows, dim, mode in [(65, 24, "quarter"), (3000, 1028, "all"), (64, 4, "absent"), (300, 10, "free")]:
        src, idx, dst, shared = R.scatter_inputs(rows, dim, mode, seed=rows)
        assert float((R.scatter_add_rows(src, idx, dst, chunk=16, defect=defect) - R.scatter_add_rows(src, idx, dst)).abs().max()) >= 1.0
    # MAE: the one-hot mask on the row the defect touches takes the whole loss away (or doubles it)
    for rows, dim in MAE_CASES:
        pred, target = R.mae_inputs(rows, dim, seed=rows + dim)
        rpw = R.mae_rows_per_wave(rows)
        r = min(rpw, rows) - 1 if defect == "drop_last_row" else (rpw if rpw < rows else 0)
        assert r in R.mae_onehot_rows(rows)
        mask = R.mae_mask(rows, ("onehot", r))
        (l, d), (ld, dd) = R.mae_loss(pred, target, mask, 1), R.mae_loss(pred, target, mask, 1, chunk=rpw, defect=defect)
        assert abs(float(l) - float(ld)) >= 4 * 1e-5 * max(1.0, float(l))
        if defect == "drop_last_row":
            assert float((d - dd).abs().max()) >= 4 * 1e-5 * float(d.abs().max())


@pytest.mark.parametrize("rows,dim", MAE_CASES)
def test_mae_variance_defects_show(rows, dim):
    pred, target = R.mae_inputs(rows, dim, seed=rows + dim)
    mask = R.mae_mask(rows, "random", seed=rows)
    count = int(mask.sum())
    l, d = R.mae_loss(pred, target, mask, count)
    for defect in ("biased_var", "eps_outside_sqrt"):
        if defect == "eps_outside_sqrt" and rows < 3:
            continue        # no near-constant row to catch it
        ld, dd = R.mae_loss(pred, target, mask, count, defect=defect)
        assert float((d - dd).abs().max()) >= 4 * 1e-5 * float(d.abs().max()), defect
        if defect == "biased_var" or rows <= 5:
            assert abs(float(l) - float(ld)) >= 4 * 1e-5 * max(1.0, float(l)), defect
        if defect == "eps_outside_sqrt":     # and only the near-constant row moves by that much: on ordinary rows the 1e-6 is lost in var ~ 9
            moved = (d - dd).abs().amax(1) >= 4 * 1e-5 * float(d.abs().max())
            assert moved.nonzero().flatten().tolist() == [2]


@pytest.mark.parametrize("V", [5, 63, 64, 65, 227, 300])
def test_ce_smoothing_defect_shows(V):
    for rows in (1, 5, 131):
        for s, c in ((1.0, 0.0), (1.0, 80.0), (30.0, 0.0)):
            for mode in R.CE_IGNORE_MODES:
                logits, target, ignore, count = R.ce_inputs(rows, V, s, c, mode, seed=V + rows)
                for e in (0.1, 1.0):
                    _, d = R.ce_loss(logits, target, ignore, count, e)
                    _, dd = R.ce_loss(logits, target, ignore, count, e, defect="no_smoothing_grad")
                    assert float((d - dd).abs().max()) >= 4 * R.ce_bars(logits, 0.0, count)[1], (rows, V, s, c, mode, e)


def test_adamw_shared_bias_correction_shows():
    params, grads, hyper = R.adamw_case("skip")
    p, _, v, _ = R.adamw_run(params, grads, hyper)
    pd, _, vd, _ = R.adamw_run(params, grads, hyper, defect="shared_bias_corr")
    assert excess(pd[2], p[2], atol=2 * P_BAR["atol"], rtol=2 * P_BAR["rtol"]) >= 4.0
    for i in (0, 1, 3, 4, 5, 6):
        assert torch.equal(pd[i], p[i]) and torch.equal(vd[i], v[i])
