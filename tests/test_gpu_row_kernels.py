"""The training row kernels of train.hip (LayerNorm backward, column sums, row scatter-add, MAE and cross-entropy loss, GELU) and the fused
AdamW, each alone, against the float64 references of tests/row_reference.py at the edges of their launch geometry.

Where a kernel sums over rows through float atomics the inputs are exact integers or have one loud row (see row_reference.py), so that a
lost or doubled row fails an exact comparison instead of hiding inside a bar sized for thousands of rows.  Random data is used for the
arithmetic itself, under the bars the project's existing tests already hold for the same quantities.
tests/test_row_reference_cpu.py checks the references, the inputs' exactness, and that each defect these tests are meant to catch moves the
reference by at least four times the bar."""
import pytest
import torch

import row_reference as R

pytestmark = pytest.mark.gpu

EPS = 1e-5
DX_BAR = dict(atol=2e-5, rtol=1e-4)       # test_layernorm_bwd_fused_and_colsum_vec
DW_BAR = dict(atol=2e-3, rtol=1e-4)       # the same test, rows <= 1037


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from acai_omr_amd import _lib
    _lib.lib()
    return "cuda"


def within(got, ref, atol, rtol=0.0):
    """max over elements of |got - ref| / (atol + rtol |ref|), in float64 on the CPU: <= 1 passes."""
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.numel() == 0:
        return 0.0
    return float(((got - ref).abs() / (atol + rtol * ref.abs())).max())


def same(got, ref):
    """Bit-for-bit as numbers: got (fp32 on the device) equals the float64 reference exactly."""
    return torch.equal(got.detach().double().cpu(), ref.double())


def offset_view(t, dev, offset):
    """`t` on the device as a contiguous view `offset` elements into a larger buffer (offset 0: its own allocation)."""
    if offset == 0:
        return t.clone().to(dev)
    buf = torch.zeros(t.numel() + offset, dtype=t.dtype, device=dev)
    v = buf[offset:].view(t.shape)
    v.copy_(t)
    return v


# ---- LayerNorm backward ------------------------------------------------------------------------------------------------------------------------
LN_FUSED = [(r, d) for d in (256, 512, 768, 1024) for r in (1, 3, 4, 5, 1037)] + [(r, d) for d in (256, 1024) for r in (8192, 8193, 8200)]
LN_GENERIC = [(r, d) for d in (10, 64, 96, 260, 1280) for r in (1, 5, 130)] + [(r, 96) for r in (2048, 2049, 2052)]


def _ln_case(dev, rows, dim, fused, x_offset=0):
    from acai_omr_amd import ops
    x, w, b, dy = R.ln_inputs(rows, dim, seed=rows * 4099 + dim)
    dx_ref, dw_ref, db_ref = R.layernorm_bwd(x, w, dy, EPS)
    xd, wd, dyd = offset_view(x, dev, x_offset), w.to(dev), dy.to(dev)
    assert (xd.data_ptr() % 16 == 0) == (x_offset == 0)
    rpb = R.ln_rows_per_block(rows, dim, aligned=x_offset == 0)

    # random data: the arithmetic
    dx, dw, db = ops.layernorm_bwd(xd, wd, dyd, EPS)
    assert within(dx, dx_ref, **DX_BAR) <= 1.0
    if rows <= 1037:
        assert within(dw, dw_ref, **DW_BAR) <= 1.0 and within(db, db_ref, **DW_BAR) <= 1.0
    dx1, dw1, db1 = ops.layernorm_bwd(xd, wd, dyd, EPS, want_param_grads=False)
    assert dw1 is None and db1 is None and torch.equal(dx1, dx)
    if fused:
        dx2, _, _, dxb, cs = ops.layernorm_bwd(xd, wd, dyd, EPS, want_bf16=True, want_colsum=True)
        assert torch.equal(dx2, dx) and torch.equal(dxb, dx.to(torch.bfloat16)) and cs.shape == (dim,)
    else:   # the error return: the generic form serves neither the bf16 copy nor the column sums, and says so before it launches anything
        with pytest.raises(RuntimeError, match="acai_layernorm_bwd"):
            ops.layernorm_bwd(xd, wd, dyd, EPS, want_bf16=True)
        with pytest.raises(RuntimeError, match="acai_layernorm_bwd"):
            ops.layernorm_bwd(xd, wd, dyd, EPS, want_colsum=True)

    # integer dy: db is exact in any order of the atomics, alone and on top of an integer pre-fill
    dyi = R.int_tensor((rows, dim), seed=rows + dim)
    _, dwi_ref, dbi_ref = R.layernorm_bwd(x, w, dyi, EPS)
    dyid = dyi.to(dev)
    _, dwi, dbi = ops.layernorm_bwd(xd, wd, dyid, EPS)
    assert same(dbi, dbi_ref)
    pw, pb = R.int_tensor((dim,), seed=dim + 1), R.int_tensor((dim,), seed=dim + 2)
    dw0, db0 = pw.clone().to(dev), pb.clone().to(dev)
    _, dwn, dbn = ops.layernorm_bwd(xd, wd, dyid, EPS, accum_into=(dw0, db0))
    assert dwn is None and dbn is None
    assert same(db0, pb.double() + dbi_ref)
    if rows <= 1037:
        assert within(dwi, dwi_ref, **DW_BAR) <= 1.0
        assert within(dw0 - pw.to(dev), dwi_ref, **DW_BAR) <= 1.0

    # one loud row at each edge of the launch geometry: every other row adds exact zeros, so db is dy[r] and dw one product, bit for bit
    xhat = (x.double() - x.double().mean(1, keepdim=True))
    xhat = xhat / torch.sqrt((xhat * xhat).mean(1, keepdim=True) + EPS)
    quiet = torch.ones(rows, dtype=torch.bool, device=dev)
    for r in R.loud_rows(rows, rpb):
        dyl = torch.zeros_like(dyd)
        dyl[r] = dyd[r]
        quiet.fill_(True)
        quiet[r] = False
        for bf16 in ((False, True) if fused else (False,)):
            out = ops.layernorm_bwd(xd, wd, dyl, EPS, want_bf16=bf16, want_colsum=fused)
            dxl, dwl, dbl = out[:3]
            tag = (rows, dim, r, bf16)
            assert torch.equal(dxl[r], dx[r]), tag
            assert not bool(dxl[quiet].any()), tag                  # +-0 everywhere else
            assert torch.equal(dbl, dyd[r]), tag
            assert within(dwl, dy[r].double() * xhat[r], **DX_BAR) <= 1.0, tag
            if fused:
                assert torch.equal(out[-1], out[3][r].float() if bf16 else dxl[r]), tag
                if bf16:
                    assert torch.equal(out[3], dxl.to(torch.bfloat16)), tag


@pytest.mark.parametrize("rows,dim", LN_FUSED)
def test_layernorm_bwd_fused(dev, rows, dim):
    """The one-pass form (dim a multiple of 256 up to 1024): 1 - 5 rows (idle waves, a workgroup with one busy wave), 1037 rows (4 rows per
    workgroup, a ragged last one), 8192 / 8193 / 8200 rows (4, 8 and 8 rows per workgroup: a wave walks more than one row)."""
    assert R.ln_fused_dim(dim) and R.ln_rows_per_block(rows, dim) == (8 if rows > 8192 else 4)
    _ln_case(dev, rows, dim, fused=True)


@pytest.mark.parametrize("rows,dim", LN_GENERIC)
def test_layernorm_bwd_generic(dev, rows, dim):
    """The two-kernel form: dims that are no multiple of 256 or lie above 1024 (1280 is both a multiple and above), and a second 2048-row chunk of
    the parameter-gradient kernel."""
    assert not R.ln_fused_dim(dim)
    _ln_case(dev, rows, dim, fused=False)


@pytest.mark.parametrize("rows", [5, 130])
def test_layernorm_bwd_generic_by_alignment(dev, rows):
    """dim 512 with x one element into a larger buffer: not 16-byte aligned, so the generic form serves a dim the fused form would take.
    That it did is asserted inside: want_bf16 raises."""
    _ln_case(dev, rows, 512, fused=False, x_offset=1)


# ---- column sums (integer data: exact throughout) ------------------------------------------------------------------------------------------------
COLSUM_ROWS = (1, 4, 5, 13, 16, 17, 63, 64, 65, 77, 8208)


def _colsum_case(dev, rows, cols, dtype, ld=None, col0=0, prefill=False):
    from acai_omr_amd import ops
    ld = ld or cols + col0
    full = R.int_tensor((rows, ld), seed=rows * 131 + ld)
    xd = full.to(dev).to(dtype)[:, col0:col0 + cols]
    ref = R.colsum(full[:, col0:col0 + cols])
    if prefill:
        pre = R.int_tensor((cols,), seed=cols)
        out = pre.clone().to(dev)
        ret = ops.colsum(xd, out=out)
        assert ret.data_ptr() == out.data_ptr()
        ref = R.colsum(full[:, col0:col0 + cols], out=pre)
    else:
        out = ops.colsum(xd)
    assert out.shape == (cols,) and same(out, ref), (rows, cols, dtype, ld, col0, prefill)
    return xd


@pytest.mark.parametrize("rows", COLSUM_ROWS)
def test_colsum_vector_form(dev, rows):
    """The 16-byte form: fp32 cols {4, 252, 256, 260}, bf16 cols {8, 504, 512, 520} (one lane, one short of / exactly / one over a 64-lane
    column tile); rows walk the 16-unrolled loop's tails, the 64-row chunk edge, and 8208 rows (chunks of 16 k)."""
    for dtype, es, colss in ((torch.float32, 4, (4, 252, 256, 260)), (torch.bfloat16, 2, (8, 504, 512, 520))):
        for cols in colss:
            xd = _colsum_case(dev, rows, cols, dtype)
            assert R.colsum_vec(cols, xd.stride(0), es, xd.data_ptr() % 16 == 0)
        xd = _colsum_case(dev, rows, colss[1], dtype, ld=colss[3])       # a wider buffer whose rows stay 16-byte aligned
        assert R.colsum_vec(colss[1], xd.stride(0), es, xd.data_ptr() % 16 == 0)
    _colsum_case(dev, rows, 256, torch.float32, prefill=True)
    _colsum_case(dev, rows, 512, torch.bfloat16, prefill=True)


@pytest.mark.parametrize("rows", COLSUM_ROWS + (2047, 2048, 2049))
def test_colsum_generic_form(dev, rows):
    """The one-column-per-lane form: cols that are no multiple of a 16-byte vector, a column-offset view, a row stride that is no multiple of
    16 bytes; 2047 / 2048 / 2049 rows sit on its 2048-row chunk edge."""
    edge = rows in (2047, 2048, 2049)
    for dtype, es, colss in ((torch.float32, 4, (70,) if edge else (1, 63, 65, 70)), (torch.bfloat16, 2, (70,) if edge else (4, 70))):
        for cols in colss:
            xd = _colsum_case(dev, rows, cols, dtype)
            assert not R.colsum_vec(cols, xd.stride(0), es, xd.data_ptr() % 16 == 0)
        xd = _colsum_case(dev, rows, 64, dtype, ld=65, col0=1)           # x[:, 1:]: the data pointer leaves the 16-byte grid
        assert xd.data_ptr() % 16 != 0
        xd = _colsum_case(dev, rows, 64, dtype, ld=64 + 16 // es + 1)    # ld * elem_size % 16 != 0
        assert not R.colsum_vec(64, xd.stride(0), es, True)
    _colsum_case(dev, rows, 70, torch.float32, prefill=True)
    _colsum_case(dev, rows, 70, torch.bfloat16, prefill=True)


def test_colsum_refuses_strided_columns(dev):
    from acai_omr_amd import ops
    x = torch.zeros(8, 8, device=dev)
    with pytest.raises((AssertionError, ValueError)):
        ops.colsum(x[:, ::2])
    with pytest.raises((AssertionError, ValueError)):
        ops.ce_loss(x[:, ::2], torch.zeros(8, dtype=torch.int64, device=dev), -100, 8, False)


# ---- row scatter-add (integer src and dst: exact) ---------------------------------------------------------------------------------------------------
SCATTER_ROWS = (1, 63, 64, 65, 3000)


def _scatter_case(dev, rows, dim, mode, give_shared=True):
    from acai_omr_amd import ops
    src, idx, dst, shared = R.scatter_inputs(rows, dim, mode, seed=rows * 7 + dim)
    assert R.scatter_precondition_ok(idx, shared, dst.shape[0])
    ref = R.scatter_add_rows(src, idx, dst)
    dd = dst.clone().to(dev)
    out = ops.scatter_add_rows(src.to(dev), idx.to(dev), dd, shared_row=shared if give_shared else -1)
    assert out.data_ptr() == dd.data_ptr() and same(dd, ref), (rows, dim, mode, give_shared)


@pytest.mark.parametrize("dim", [4, 24, 512, 1024, 1028, 2048])
def test_scatter_add_rows_shared_form(dev, dim):
    """The shared-row form (dim % 4 == 0): plain read-modify-write for the unique rows, a workgroup column sum for the shared one, whose image
    in LDS holds 1024 columns (1028 and 2048 go past it, into per-element atomics).  Rows: one, one short of / exactly / one over a 64-row
    workgroup, many.  The shared row is absent from idx, a quarter of it, or all of it; dst is not zero."""
    for rows in SCATTER_ROWS:
        for mode in ("absent", "quarter", "all"):
            _scatter_case(dev, rows, dim, mode)


@pytest.mark.parametrize("dim", [10, 30])
def test_scatter_add_rows_shared_row_on_unaligned_dim(dev, dim):
    """dim % 4 != 0 with a shared row given: the atomic form serves it."""
    for rows in SCATTER_ROWS:
        for mode in ("absent", "quarter", "all"):
            _scatter_case(dev, rows, dim, mode)


@pytest.mark.parametrize("dim", [10, 24])
def test_scatter_add_rows_atomic_form(dev, dim):
    """shared_row = -1: indices repeat freely over a 17-row table (and the shared-form inputs are served just as well)."""
    for rows in SCATTER_ROWS:
        _scatter_case(dev, rows, dim, "free")
        _scatter_case(dev, rows, dim, "quarter", give_shared=False)


# ---- MAE loss ---------------------------------------------------------------------------------------------------------------------------------------
MAE_CASES = [(1, 2), (5, 12), (4095, 64), (4096, 256), (4100, 65), (65539, 12)]


@pytest.mark.parametrize("rows,dim", MAE_CASES)
def test_mae_loss(dev, rows, dim):
    """Loss within 1e-5 max(1, |ref|) and dpred within 1e-5 max|dpred_ref| of float64 (the project's 1e-5 of the MAE KAT), masked-out rows of
    dpred exactly zero, for a random 75 % mask, all ones, all zeros, and one-hot masks at the edges of a wave's row chunk (1, 4 or 16 rows per
    wave).  dim 2 pins the unbiased variance, target row 1 is constant, row 2 nearly so (row_reference.mae_inputs).
    want_grad=False gives a bit-equal loss where one atomic forms it: up to 4 rows (one workgroup) and the one-hot masks."""
    from acai_omr_amd import ops
    assert R.mae_rows_per_wave(rows) == (16 if rows == 65539 else (4 if rows >= 4096 else 1))
    pred, target = R.mae_inputs(rows, dim, seed=rows + dim)
    pd, td = pred.to(dev), target.to(dev)
    masks = [("random", R.mae_mask(rows, "random", seed=rows)), ("ones", R.mae_mask(rows, "ones")), ("zeros", R.mae_mask(rows, "zeros"))]
    masks += [(("onehot", r), R.mae_mask(rows, ("onehot", r))) for r in R.mae_onehot_rows(rows)]
    for kind, mask in masks:
        count = max(1, int(mask.sum()))
        loss_ref, dp_ref = R.mae_loss(pred, target, mask, count)
        md = mask.to(dev)
        loss, dp = ops.mae_loss(pd, td, md, count, True)
        l_err = abs(float(loss) - float(loss_ref)) / (1e-5 * max(1.0, abs(float(loss_ref))))
        g_err = within(dp, dp_ref, atol=1e-5 * max(float(dp_ref.abs().max()), 1e-300))
        print(f"mae rows={rows} dim={dim} mask={kind}: loss error {l_err:.3f} of its bar, dpred error {g_err:.3f} of its bar")
        assert l_err <= 1.0 and g_err <= 1.0, (kind, l_err, g_err)
        assert not bool(dp[md == 0].any()), kind
        if kind == "zeros":
            assert float(loss) == 0.0
        loss2, none = ops.mae_loss(pd, td, md, count, False)
        assert none is None
        if rows <= 4 or kind == "zeros" or isinstance(kind, tuple):
            assert torch.equal(loss2, loss), kind
        else:
            assert abs(float(loss2) - float(loss_ref)) <= 1e-5 * max(1.0, abs(float(loss_ref))), kind


# ---- cross-entropy loss ----------------------------------------------------------------------------------------------------------------------------
CE_ROWS = (1, 3, 4, 5, 131)
CE_LOGITS = ((1.0, 0.0), (1.0, 80.0), (1.0, -80.0), (30.0, 0.0))
CE_SMOOTHING = (0.0, 0.1, 1.0)


@pytest.mark.parametrize("V", [5, 63, 64, 65, 227, 300])
def test_ce_loss(dev, V):
    """rows {1, 3, 4, 5, 131} x logits randn * s + c for (s, c) in {(1, 0), (1, 80), (1, -80), (30, 0)} x label smoothing {0, 0.1, 1} x
    (ignore_index 1 with some rows ignored / with all but one ignored / -100 with none ignored) x (ld = V, ld = V + 5), against a float64
    log-softmax.  Bars (row_reference.ce_bars): loss 1e-5 max(1, |ref|) + 4 eps32 max|logit|, gradient (1e-6 + 2 eps32 max|logit|) / count.
    Ignored rows of dlogits are exactly zero.
    want_grad=False: the loss is bit-equal where ONE atomic forms it, i.e. where one row is kept.  (Every kept row's wave issues its own
    atomic on the loss, so with 3 or 4 kept rows in one workgroup the order of the additions is still free: those cases are held to the
    loss bar instead.)"""
    from acai_omr_amd import ops
    worst_l = worst_g = 0.0
    for rows in CE_ROWS:
        for si, (s, c) in enumerate(CE_LOGITS):
            for mode in R.CE_IGNORE_MODES:
                logits, target, ignore, count = R.ce_inputs(rows, V, s, c, mode, seed=V * 1000 + rows * 10 + si)
                assert bool(((target >= 0) & (target < V) | (target == ignore)).all()) and count == int((target != ignore).sum()) >= 1
                wide = torch.full((rows, V + 5), 1e4)      # what lies past V must not be read: it would win every maximum
                wide[:, :V] = logits
                ld_v, ld_w, td = logits.to(dev), wide.to(dev)[:, :V], target.to(dev)
                assert ld_w.stride(0) == V + 5
                for e in CE_SMOOTHING:
                    loss_ref, dl_ref = R.ce_loss(logits, target, ignore, count, e)
                    l_bar, g_bar = R.ce_bars(logits, loss_ref, count)
                    for lg in (ld_v, ld_w):
                        tag = (rows, V, s, c, mode, e, lg.stride(0))
                        loss, dl = ops.ce_loss(lg, td, ignore, count, True, label_smoothing=e)
                        l_err, g_err = abs(float(loss) - float(loss_ref)) / l_bar, within(dl, dl_ref, atol=g_bar)
                        worst_l, worst_g = max(worst_l, l_err), max(worst_g, g_err)
                        assert l_err <= 1.0 and g_err <= 1.0, (tag, l_err, g_err)
                        assert dl.shape == (rows, V) and not bool(dl[td == ignore].any()), tag
                        loss2, none = ops.ce_loss(lg, td, ignore, count, False, label_smoothing=e)
                        assert none is None
                        if count == 1:
                            assert torch.equal(loss2, loss), tag
                        else:
                            assert abs(float(loss2) - float(loss_ref)) <= l_bar, tag
    print(f"ce V={V}: worst loss error {worst_l:.3f} of its bar, worst gradient error {worst_g:.3f} of its bar")


# ---- GELU -------------------------------------------------------------------------------------------------------------------------------------------
def test_gelu_fp32(dev):
    """400 001 points on [-20, 20] and +-0, +-1e-30, +-88, +-1e30 (the clamp at t = 12 is |x| = 17; the polynomial is fitted up to |x| = 6.1).
    Forward within 1e-6 + 2 eps32 |ref| of float64 (1e-6: the project's bar, common.h documents 5.0e-7 for the approximation; the relative term
    is the final rounding where gelu(x) = x); backward with dh = randn within 1e-5 + 1e-6 |ref| (project bar 1e-5)."""
    from acai_omr_amd import ops
    x = R.gelu_points()
    g = torch.Generator().manual_seed(3)
    dh = torch.randn(x.shape, generator=g)
    xd = x.to(dev)
    fwd = within(ops.gelu_fwd(xd), R.gelu(x), atol=1e-6, rtol=2 * R.EPS32)
    bwd = within(ops.gelu_bwd(xd, dh.to(dev)), dh.double() * R.gelu_grad(x), atol=1e-5, rtol=1e-6)
    print(f"gelu fp32: forward error {fwd:.3f} of its bar, backward error {bwd:.3f} of its bar")
    assert fwd <= 1.0 and bwd <= 1.0


def test_gelu_grid_stride_second_trip(dev):
    """n = 8192 * 256 + 257: the grid is capped at 8192 workgroups, so 257 threads make a second trip of the grid-stride loop."""
    from acai_omr_amd import ops
    n = 8192 * 256 + 257
    g = torch.Generator().manual_seed(4)
    x, dh = torch.randn(n, generator=g) * 3, torch.randn(n, generator=g)
    xd = x.to(dev)
    assert within(ops.gelu_fwd(xd), R.gelu(x), atol=1e-6, rtol=2 * R.EPS32) <= 1.0
    assert within(ops.gelu_bwd(xd, dh.to(dev)), dh.double() * R.gelu_grad(x), atol=1e-5, rtol=1e-6) <= 1.0
    xb = x.to(torch.bfloat16)
    assert R.gelu_bf16_excess(ops.gelu_fwd(xb.to(dev)).cpu(), R.gelu(xb.double())) <= 1.0


def test_gelu_bf16_every_input(dev):
    """Every finite bf16 bit pattern (65 280 values), forward and backward with dh = 1, against the correctly rounded bf16 of the float64 value.

    The bar first set for this test was one bf16 ulp of the reference and nothing else.  A correct kernel misses that in the far left tail, and
    the CPU module shows it without a GPU: the forward is a polynomial fit whose error is bounded in ABSOLUTE terms (5.0e-7 over [-8, 8],
    common.h), and the backward forms Phi(x) as 0.5 (1 + erff(x / sqrt 2)), which cancels to an absolute error of about eps32 for x < -5.
    From x = -4.375 down, where |gelu(x)| < 3e-5 and one bf16 ulp of it is below 1.2e-7, the relative bar asks for more than either promises: an
    fp32 emulation of the forward (tools/check_erf.py) is off by more than one ulp for 198 inputs in [-13.44, -4.375], by up to 248 ulps at
    x = -12.5 where gelu(x) = -4.7e-35; the plain fp32 evaluation of the backward for 141 inputs in [-13.2, -5.3], by up to 8 ulps.
    Measured on the MI355X: forward 198 inputs over one ulp, all in [-13.4375, -4.375], largest absolute error 2.4e-7; backward 140 inputs, all
    in [-13.1875, -5.34375], largest absolute error 1.5e-8.
    The corrected bar is therefore one bf16 ulp of the reference PLUS the absolute 1e-6 that the fp32 forward test holds
    (row_reference.GELU_BF16_FLOOR); and no input may miss the one-ulp bar wherever one ulp of the reference is as large as that floor
    (|gelu| or |gelu'| from 2.4e-4 up), where an absolute error below half the floor cannot cost more than one ulp."""
    from acai_omr_amd import ops
    xb = R.all_finite_bf16()
    assert xb.numel() == 65280
    xd = xb.to(dev)
    x64 = xb.double()
    for name, got, ref in (("forward", ops.gelu_fwd(xd), R.gelu(x64)), ("backward", ops.gelu_bwd(xd, torch.ones_like(xd)), R.gelu_grad(x64))):
        assert got.dtype == torch.bfloat16
        rb = R.round_bf16(ref)
        err = (got.double().cpu() - rb).abs()
        ulps = err / R.bf16_ulp(rb)
        over = ulps > 1.0
        print(f"gelu bf16 {name}: {int(over.sum())} inputs over one ulp" + (f", all in [{float(x64[over].min())}, {float(x64[over].max())}], "
              f"largest absolute error {float(err[over].max()):.3e}" if bool(over.any()) else ""))
        assert R.gelu_bf16_excess(got.cpu(), ref) <= 1.0, name
        assert not bool(over[R.bf16_ulp(rb) >= R.GELU_BF16_FLOOR].any()), name     # the floor is idle wherever an ulp is as large


# ---- fused AdamW -----------------------------------------------------------------------------------------------------------------------------------
P_BAR = dict(rtol=2e-6, atol=2e-7)       # test_fused_adamw_matches_torch
V_BAR = dict(rtol=1e-5, atol=1e-12)


@pytest.mark.parametrize("case", R.ADAMW_CASES)
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "unaligned"])
def test_fused_adamw(dev, case, aligned):
    """Six steps of FusedAdamW over sizes {1, 3, 17, 16383, 16384, 16385, 32769} (the kernel's chunk is 16384 elements) against
    torch.optim.AdamW(foreach=False) on the device under the bars of test_fused_adamw_matches_torch, and against the hand-written float64 AdamW
    at twice those bars.  unaligned: every parameter is a contiguous view one element into a larger buffer and every gradient a view three
    elements into its own, so no pointer is 16-byte aligned and the kernel's scalar branch runs.
    Cases (row_reference.adamw_case): "skip" - a parameter without a gradient on steps 2 and 3 keeps its own step count and bias corrections
    (the chunk table is rebuilt for the shorter list and again when the parameter returns); "lr0" - a group with lr = 0 leaves its parameters
    bit-unchanged while the moments move; "wd0"; "zero_grad" - pure decay; "beta1_0" - betas (0.0, 0.9)."""
    from acai_omr_amd.optim import FusedAdamW
    params, grads, hyper = R.adamw_case(case)
    off_p, off_g = (0, 0) if aligned else (1, 3)
    mine = [torch.nn.Parameter(offset_view(p, dev, off_p)) for p in params]
    theirs = [torch.nn.Parameter(p.clone().to(dev)) for p in params]
    for p in mine:
        assert p.is_contiguous() and (p.data_ptr() % 16 == 0) == aligned
    of = FusedAdamW(R.adamw_groups(mine, hyper))
    ot = torch.optim.AdamW(R.adamw_groups(theirs, hyper), foreach=False)
    for gs in grads:
        for a, b, g in zip(mine, theirs, gs):
            a.grad = None if g is None else offset_view(g, dev, off_g)
            b.grad = None if g is None else g.to(dev)
            if g is not None:
                assert a.grad.is_contiguous() and (a.grad.data_ptr() % 16 == 0) == aligned
        of.step(), ot.step()
    p64, m64, v64, steps = R.adamw_run(params, grads, hyper)
    for i, (a, b) in enumerate(zip(mine, theirs)):
        tag = (case, aligned, R.ADAMW_SIZES[i])
        assert float(of.state[a]["step"]) == float(ot.state[b]["step"]) == steps[i], tag
        assert torch.allclose(a, b, **P_BAR), (tag, float((a - b).abs().max()))
        assert torch.allclose(of.state[a]["exp_avg_sq"], ot.state[b]["exp_avg_sq"], **V_BAR), tag
        assert within(a, p64[i], atol=2 * P_BAR["atol"], rtol=2 * P_BAR["rtol"]) <= 1.0, tag
        assert within(of.state[a]["exp_avg_sq"], v64[i], atol=2 * V_BAR["atol"], rtol=2 * V_BAR["rtol"]) <= 1.0, tag
        if hyper[i]["lr"] == 0.0:
            assert torch.equal(a.detach().cpu(), params[i]), tag
            assert bool(of.state[a]["exp_avg"].any()) and bool(of.state[a]["exp_avg_sq"].any()), tag
        if case == "zero_grad":
            assert not bool(of.state[a]["exp_avg"].any()) and not bool(of.state[a]["exp_avg_sq"].any()), tag
    if case == "skip":
        assert steps[2] == R.ADAMW_STEPS - 2 and all(s == R.ADAMW_STEPS for i, s in enumerate(steps) if i != 2)
