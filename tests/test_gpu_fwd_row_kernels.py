"""The forward row kernels of elementwise.hip (LayerNorm forward, patchify, the row gather, the fp32 -> bf16 cast, the positional-embedding
interpolation and its transpose), each alone through acai_omr_amd.ops, against the float64 references of tests/fwd_row_reference.py at every
dispatch form (float4 or scalar, one grid sweep or several) and at the edges of their launch geometry.

Wherever the operation allows it the inputs are exact in fp32 (distinct pixels, small integers, power-of-two interpolation ratios, the bf16
edge set), so a misplaced, dropped, doubled or unwritten element fails a `torch.equal`; caller-given outputs are views into buffers filled
with POISON whose guard elements must keep it.  Random data is used for the arithmetic itself, under the bars the project already holds or,
for the two new LayerNorm input families, four times the error of a plain fp32 evaluation as measured in
tests/test_fwd_row_reference_cpu.py, which also checks the references, the inputs' exactness, and that each defect these tests are meant to
catch clears the bar of the case that catches it."""
import pytest
import torch

import fwd_row_reference as R

pytestmark = pytest.mark.gpu

GUARD = 4       # floats before and after a caller-given output: the view stays 16-byte aligned


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
    """Bit-for-bit as numbers: got (on the device) equals the float64 reference exactly."""
    return torch.equal(got.detach().double().cpu(), ref.double())


def offset_view(t, dev, offset):
    """`t` on the device as a contiguous view `offset` elements into a larger buffer (offset 0: its own allocation)."""
    if offset == 0:
        return t.clone().to(dev)
    buf = torch.zeros(t.numel() + offset, dtype=t.dtype, device=dev)
    v = buf[offset:].view(t.shape)
    v.copy_(t)
    return v


def poisoned(shape, dev, guard=GUARD, dtype=torch.float32):
    """(buffer, contiguous view of `shape` that starts `guard` elements into it); the buffer holds POISON and ends `guard` elements after the view."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * guard,), R.POISON, dtype=dtype, device=dev)
    return buf, buf[guard:guard + n].view(shape)


def guards_intact(buf, guard=GUARD):
    return bool((buf[:guard] == R.POISON).all()) and bool((buf[buf.numel() - guard:] == R.POISON).all())


# ---- LayerNorm forward ---------------------------------------------------------------------------------------------------------------------------
def _ln_case(dev, kind, rows, dim, x_off=0, w_off=0):
    from acai_omr_amd import ops
    x, w, b = R.ln_inputs(kind, rows, dim, seed=R.ln_seed(rows, dim))
    xd, wd, bd = offset_view(x, dev, x_off), offset_view(w, dev, w_off), b.to(dev)
    assert (xd.data_ptr() % 16 == 0) == (x_off == 0) and (wd.data_ptr() % 16 == 0) == (w_off == 0) and bd.data_ptr() % 16 == 0
    tag = (kind, rows, dim, x_off, w_off)

    y32, y16 = ops.layernorm(xd, wd, bd, R.LN_EPS, want_bf16=True)
    assert y32.dtype == torch.float32 and y16.dtype == torch.bfloat16 and y32.shape == y16.shape == (rows, dim)
    if kind == "const":
        assert torch.equal(y32.cpu(), b.expand(rows, dim)), tag
    else:
        err = within(y32, R.layernorm(x, w, b, R.LN_EPS), atol=R.LN_BAR[kind])
        print(f"layernorm {tag}: error {err:.3f} of its bar {R.LN_BAR[kind]:.1e}")
        assert err <= 1.0, (tag, err)
    assert torch.equal(R.bf16_to_bits(y16.cpu()), R.bf16_bits(y32.cpu())), tag          # the bf16 copy is the fp32 output, rounded to nearest even

    none, y16b = ops.layernorm(xd, wd, bd, R.LN_EPS, want_f32=False, want_bf16=True)
    assert none is None and torch.equal(y16b, y16), tag

    buf, view = poisoned((rows, dim), dev)
    assert view.data_ptr() % 16 == 0
    r32, r16 = ops.layernorm(xd, wd, bd, R.LN_EPS, want_bf16=True, out_f32=view)
    assert r32.data_ptr() == view.data_ptr() and torch.equal(view, y32) and torch.equal(r16, y16) and guards_intact(buf), tag
    return y32


@pytest.mark.parametrize("dim", R.LN_VEC_DIMS)
def test_layernorm_vector_form(dev, dim):
    """dim % 4 == 0 and every pointer 16-byte aligned: the float4 kernel; dims of one lane, one short of / on / one over its 256-float
    stride, several trips with and without a ragged last one; rows {1, 3, 4, 5, 130} (idle waves, a full workgroup, one row into the next)."""
    assert R.ln_vec(dim)
    for rows in R.LN_ROWS:
        _ln_case(dev, "randn3p1", rows, dim)


@pytest.mark.parametrize("dim", R.LN_SCALAR_DIMS)
def test_layernorm_scalar_form(dev, dim):
    """dim % 4 != 0: the one-float-per-lane kernel, on both sides of its 64-float stride."""
    assert not R.ln_vec(dim)
    for rows in R.LN_ROWS:
        _ln_case(dev, "randn3p1", rows, dim)


@pytest.mark.parametrize("which", ["x", "w"])
@pytest.mark.parametrize("dim", R.LN_VEC_DIMS)
def test_layernorm_scalar_form_by_alignment(dev, dim, which):
    """The vector dims with x, then w, a view one float into a larger buffer: the pointer is off the 16-byte grid (asserted inside), so the
    scalar kernel serves a dim % 4 == 0 row; the result is held to the same bar, not to equality with the vector form (another summation order)."""
    assert R.ln_vec(dim) and not R.ln_vec(dim, aligned=False)
    for rows in R.LN_ROWS:
        _ln_case(dev, "randn3p1", rows, dim, x_off=1 if which == "x" else 0, w_off=1 if which == "w" else 0)


@pytest.mark.parametrize("kind", R.LN_FAMILIES)
@pytest.mark.parametrize("dim", R.LN_FAMILY_DIMS)
def test_layernorm_input_families(dev, dim, kind):
    """Rows with a large mean (randn + 100: a one-pass variance cancels), rows whose variance is the size of eps (0.75 + randn 2^-10: eps
    outside the square root changes the result by a factor), the project's randn * 3 + 1, and constant rows, whose output is exactly b.
    Bars: fwd_row_reference.LN_BAR."""
    for rows in R.LN_FAMILY_ROWS:
        _ln_case(dev, kind, rows, dim)
    if dim % 4 == 0 and kind != "randn3p1":
        _ln_case(dev, kind, R.LN_FAMILY_ROWS[0], dim, x_off=1)


# ---- patchify ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,P", R.PATCHIFY_CASES + (R.PATCHIFY_ONE_SWEEP, R.PATCHIFY_TWO_SWEEPS))
def test_patchify(dev, H, W, P):
    """Distinct pixels (img[y, x] = y W + x), fp32 and bf16 output, into rows 2.. of a poisoned buffer whose rows are five elements wider than
    a patch: the whole buffer is compared, so the columns beyond P * P, the rows before and after, and every pixel's place are all held
    exactly.  The small sizes write a second (mirrored) image behind the first (row0 = 2 + n).  P in {16, 4, 2, 3, 5, 1}, H or W not a
    multiple of P; (512, 2048, 16) is exactly one sweep of the grid, (1040, 1024, 16) goes 16 384 elements into the second."""
    from acai_omr_amd import ops
    small = H * W < 2 ** 16
    assert R.patchify_sweeps(H, W, P) == (2 if (H, W, P) == R.PATCHIFY_TWO_SWEEPS else 1)
    n, PP = (H // P) * (W // P), P * P
    imgs = [R.distinct_pixels(H, W)] + ([R.distinct_pixels(H, W).flip(1, 2).contiguous()] if small else [])
    rows, ld = 2 + n * len(imgs) + 3, PP + 5
    ref = torch.full((rows, ld), R.POISON, dtype=torch.float64)
    for k, img in enumerate(imgs):
        part = R.patchify(img, P, rows=rows, row0=2 + k * n, ld=ld)
        ref = torch.where(part != R.POISON, part, ref)
    for dtype in (torch.float32, torch.bfloat16):
        buf = torch.full((rows, ld), R.POISON, dtype=dtype, device=dev)
        out = buf[:, :PP]
        assert out.stride(0) == ld
        for k, img in enumerate(imgs):
            assert ops.patchify(img.to(dev), P, out, 2 + k * n) == n
        got = buf.cpu()
        want = ref.float().to(dtype)
        if not torch.equal(got, want):
            bad = (got != want).nonzero()
            assert False, (H, W, P, dtype, f"{bad.shape[0]} elements differ, first (row, column) {bad[0].tolist()}, last {bad[-1].tolist()}")


# ---- row gather (integer table and add: exact) -------------------------------------------------------------------------------------------------------------
def _gather_rows_case(dev, rows, dim, t_off=0, patterns=R.GATHER_PATTERNS, out_guard=GUARD):
    from acai_omr_amd import ops
    table, add = R.int_tensor((rows + 1, dim), seed=dim * 31 + rows), R.int_tensor((rows, dim), seed=dim * 31 + rows + 1)
    td, ad = offset_view(table, dev, t_off), add.to(dev)
    assert (td.data_ptr() % 16 == 0) == (t_off == 0) and td.is_contiguous()
    for pattern in patterns:
        idx = R.gather_index(pattern, rows, rows + 1, seed=rows)
        idxd = idx.to(dev)
        for a, a_dev in ((add, ad), (None, None)):
            tag = (rows, dim, t_off, pattern, a is not None)
            ref = R.gather_rows(table, idx, a)
            out = ops.gather_rows(td, idxd, a_dev)
            assert out.shape == (rows, dim) and out.dtype == torch.float32 and same(out, ref), tag
            buf, view = poisoned((rows, dim), dev, guard=out_guard)
            ret = ops.gather_rows(td, idxd, a_dev, out=view)
            assert ret.data_ptr() == view.data_ptr() and same(view, ref) and guards_intact(buf, out_guard), tag


@pytest.mark.parametrize("dim", R.GATHER_VEC_DIMS)
def test_gather_rows_vector_form(dev, dim):
    """dim % 4 == 0, aligned: the float4 kernel at one lane, six lanes, one trip exactly, one lane into the second trip, three and four trips;
    rows {1, 3, 4, 5, 33}; identity, reversed, one row for all, the pad_rows pattern (a valid prefix, then the fill row repeated) and random
    indices with duplicates; add given and None; out fresh and as a guarded view of a poisoned buffer."""
    assert R.gather_vec(dim)
    for rows in R.GATHER_ROWS:
        _gather_rows_case(dev, rows, dim)


@pytest.mark.parametrize("dim", R.GATHER_SCALAR_DIMS)
def test_gather_rows_scalar_form(dev, dim):
    """dim % 4 != 0: the one-float-per-lane kernel on both sides of its 64-float stride and beyond 256."""
    assert not R.gather_vec(dim)
    for rows in R.GATHER_ROWS:
        _gather_rows_case(dev, rows, dim)


@pytest.mark.parametrize("dim", R.GATHER_VEC_DIMS)
def test_gather_rows_scalar_form_by_alignment(dev, dim):
    """A dim % 4 == 0 table as a view one float into a buffer, and, with an aligned table, an out view five floats into its buffer: either
    pointer off the 16-byte grid sends the row to the scalar kernel."""
    for rows in R.GATHER_ROWS:
        _gather_rows_case(dev, rows, dim, t_off=1)
    _gather_rows_case(dev, 5, dim, out_guard=5, patterns=("pad", "random"))


@pytest.mark.parametrize("dim", R.GATHER_MANY_DIMS)
def test_gather_rows_many_rows(dev, dim):
    """8200 rows: 2050 workgroups, the last one full."""
    _gather_rows_case(dev, R.GATHER_MANY_ROWS, dim, patterns=("pad", "random"))


# ---- fp32 -> bf16 ---------------------------------------------------------------------------------------------------------------------------------------------
def test_cast_bf16_every_rounding_edge(dev):
    """The whole edge set (fwd_row_reference.bf16_edge_set: 391 680 values) in one call: NaN stays NaN, everything else has the bits of round
    to nearest even - ties up and down, the carry into the exponent, overflow to inf, +-inf.  +-0 next to it, through the vector loop (n = 4)
    and through the tail (n = 2)."""
    from acai_omr_amd import ops
    x = R.bf16_edge_set()
    got = R.bf16_to_bits(ops.cast_bf16(x.to(dev)).cpu())
    ref, nan = R.bf16_bits(x), torch.isnan(x)
    assert bool(R.bf16_is_nan(got)[nan].all()), "a NaN came out as a number"
    bad = ((got != ref) & ~nan).nonzero().flatten()
    assert bad.numel() == 0, (f"{bad.numel()} values rounded wrongly, first: fp32 bits {int(R.f32_to_bits(x)[bad[0]]):#010x} -> "
                              f"{int(got[bad[0]]):#06x}, expected {int(ref[bad[0]]):#06x}")
    for z in (torch.tensor([0.0, -0.0, -0.0, 0.0]), torch.tensor([0.0, -0.0])):
        assert torch.equal(R.bf16_to_bits(ops.cast_bf16(z.to(dev)).cpu()), R.bf16_bits(z))


@pytest.mark.parametrize("n", R.CAST_SMALL)
def test_cast_bf16_small(dev, n):
    """n below one float4, one float4 exactly, a float4 and a tail, 1003 and 1024 elements, on random data: the bits of round to nearest even."""
    from acai_omr_amd import ops
    x = torch.randn(n, generator=torch.Generator().manual_seed(n))
    y = ops.cast_bf16(x.to(dev))
    assert y.shape == (n,) and y.dtype == torch.bfloat16 and torch.equal(R.bf16_to_bits(y.cpu()), R.bf16_bits(x))


@pytest.mark.parametrize("n", R.CAST_LARGE)
def test_cast_bf16_grid_sweeps(dev, n):
    """4096 * 1024 elements is exactly one trip of the grid-stride loop; four more elements make one thread take a second trip, 1027 more a
    second trip and a three-element tail, and 2 * 4096 * 1024 + 3 two whole trips and a tail.  The source is the integers -8 .. 8 in turn, which
    bf16 holds exactly.  The destination is allocated inside the wrapper; a buffer of the same size is filled with POISON and freed just
    before, so that the allocator hands back poisoned memory and not the result of an earlier call."""
    from acai_omr_amd import ops
    x = R.int_cycle(n)
    xd = x.to(dev)
    p = torch.full((n,), R.POISON, dtype=torch.bfloat16, device=dev)
    del p
    got = ops.cast_bf16(xd).float().cpu()
    first, body = R.cast_first_sweep(n), n & ~3
    assert torch.equal(got[:first], x[:first]), f"n={n}: first sweep, elements [0, {first})"
    assert torch.equal(got[first:body], x[first:body]), f"n={n}: later sweeps, elements [{first}, {body}): got {got[first:first + 8].tolist()}"
    assert torch.equal(got[body:], x[body:]), f"n={n}: tail, elements [{body}, {n}): got {got[body:].tolist()}"


def test_cast_bf16_refuses_unaligned_source(dev):
    """The kernel reads float4s: a source off the 16-byte grid is refused before any launch, and nothing already written changes."""
    from acai_omr_amd import ops
    x = torch.randn(1024, generator=torch.Generator().manual_seed(1))
    good = ops.cast_bf16(x.to(dev))
    keep = good.clone()
    xv = offset_view(x, dev, 1)
    assert xv.is_contiguous() and xv.data_ptr() % 16 != 0
    with pytest.raises(RuntimeError, match="acai_cast_f32_bf16"):
        ops.cast_bf16(xv)
    torch.cuda.synchronize()
    assert torch.equal(good, keep) and torch.equal(R.bf16_to_bits(good.cpu()), R.bf16_bits(x))


# ---- positional-embedding interpolation -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", R.PE_DYADIC, ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_pe_interp_dyadic_exact(dev, sizes):
    """Power-of-two ratios (x2, x4, x1, /2 on a 4 x 6 and an 8 x 12 table, x2 on a one-row table) on integer table and dout: every weight is
    a multiple of 1/64, so forward and backward are exact in fp32 in any order of the atomics and are compared with torch.equal.
    E in {1, 10, 64, 65, 70, 130}: one lane, one trip short of / exactly / one over the 64 lanes, three trips.  The backward is called twice:
    each call returns a freshly zeroed table.  At the identity size the forward copies a random table bit for bit."""
    from acai_omr_amd import ops
    (Hin, Win), (Ho, Wo) = sizes
    for E in R.PE_DYADIC_E:
        table, dout = R.pe_inputs(Hin, Win, E, Ho, Wo, seed=E, integers=True)
        td, dd = table.to(dev), dout.to(dev)
        out = ops.pe_interp(td, Ho, Wo)
        assert out.shape == (Ho * Wo, E) and same(out, R.pe_interp(table, Ho, Wo)), (sizes, E)
        ref = R.pe_interp_bwd(dout, Ho, Wo, (Hin, Win, E))
        for call in (1, 2):
            dt = ops.pe_interp_bwd(dd, Ho, Wo, (Hin, Win, E))
            assert dt.shape == (Hin, Win, E) and same(dt, ref), (sizes, E, call)
        if (Hin, Win) == (Ho, Wo):
            rnd, _ = R.pe_inputs(Hin, Win, E, Ho, Wo, seed=E, integers=False)
            assert torch.equal(ops.pe_interp(rnd.to(dev), Ho, Wo).cpu(), rnd.view(-1, E)), (sizes, E)


@pytest.mark.parametrize("sizes", R.PE_OTHER + R.PE_OTHER_EXTRA, ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_pe_interp_other_ratios(dev, sizes):
    """Up, down and mixed scaling, one-cell and one-column tables, a one-cell output; Ho * Wo % 4 takes 0, 1, 2 and 3.  Random data under the
    project's bars (1e-5 forward, 1e-4 backward) against float64.  Then one loud cell: dout is zero except in cell c in {0, 3, 4, last}, so the
    result is that cell's four products alone - a cell the backward loses or adds twice is the whole result, not a part of a sum the bar was
    sized for - and every table cell it does not touch is exactly zero."""
    from acai_omr_amd import ops
    (Hin, Win), (Ho, Wo) = sizes
    for E in R.PE_OTHER_E:
        table, dout = R.pe_inputs(Hin, Win, E, Ho, Wo, seed=E, integers=False)
        shape = (Hin, Win, E)
        fwd = within(ops.pe_interp(table.to(dev), Ho, Wo), R.pe_interp(table, Ho, Wo), atol=R.PE_FWD_BAR)
        ref = R.pe_interp_bwd(dout, Ho, Wo, shape)
        dd = dout.to(dev)
        first = ops.pe_interp_bwd(dd, Ho, Wo, shape)
        bwd = within(first, ref, atol=R.PE_BWD_BAR)
        print(f"pe_interp {sizes} E={E}: forward error {fwd:.3f} of its bar, backward error {bwd:.3f} of its bar")
        assert fwd <= 1.0 and bwd <= 1.0, (sizes, E, fwd, bwd)
        assert within(ops.pe_interp_bwd(dd, Ho, Wo, shape), ref, atol=R.PE_BWD_BAR) <= 1.0, (sizes, E)       # a second call starts from zero again
        for c in R.edge_cells(Ho * Wo):
            one = R.one_cell(dout, c)
            ref1 = R.pe_interp_bwd(one, Ho, Wo, shape)
            got1 = ops.pe_interp_bwd(one.to(dev), Ho, Wo, shape)
            assert within(got1, ref1, atol=R.PE_BWD_BAR) <= 1.0, (sizes, E, c)
            assert not bool(got1.cpu()[ref1 == 0].any()), (sizes, E, c)


# ---- zero rows ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_zero_rows(dev):
    """An empty input gives an empty result of the right shape and dtype, without an error and without a launch."""
    from acai_omr_amd import ops
    w, b = torch.ones(8, device=dev), torch.zeros(8, device=dev)
    y32, y16 = ops.layernorm(torch.empty(0, 8, device=dev), w, b, R.LN_EPS, want_bf16=True)
    assert y32.shape == y16.shape == (0, 8) and y32.dtype == torch.float32 and y16.dtype == torch.bfloat16
    none, y16 = ops.layernorm(torch.empty(0, 8, device=dev), w, b, R.LN_EPS, want_f32=False, want_bf16=True)
    assert none is None and y16.shape == (0, 8)
    table = torch.ones(3, 8, device=dev)
    out = ops.gather_rows(table, torch.empty(0, dtype=torch.int32, device=dev))
    assert out.shape == (0, 8) and out.dtype == torch.float32 and out.is_cuda
    out = ops.gather_rows(table, torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, 8, device=dev))
    assert out.shape == (0, 8)
    y = ops.cast_bf16(torch.empty(0, device=dev))
    assert y.shape == (0,) and y.dtype == torch.bfloat16 and y.is_cuda
    y = ops.cast_bf16(torch.empty(0, 8, device=dev))
    assert y.shape == (0, 8) and y.dtype == torch.bfloat16
