"""tests/fwd_row_reference.py on the CPU: the hand-written references equal aten in float64, the probe inputs have the exactness the GPU
tests (tests/test_gpu_fwd_row_kernels.py) rely on, the LayerNorm bars are measured here, and every defect the GPU tests are meant to catch
moves the reference by at least four times the bar of the case that catches it, or breaks that case's exact comparison."""
import pytest
import torch
import torch.nn.functional as F

import fwd_row_reference as R


def maxabs(got, ref):
    """max |got - ref| in float64; a NaN or inf in got counts as infinitely far."""
    d = (got.double() - ref.double()).abs()
    return float("inf") if not bool(torch.isfinite(d).all()) else (float(d.max()) if d.numel() else 0.0)


def aten_interp(table, Ho, Wo):
    """(out, function dout -> dtable) of F.interpolate on the (Hin, Win, E) table in its own dtype."""
    t = table.clone().requires_grad_()
    out = F.interpolate(t.permute(2, 0, 1).unsqueeze(0), size=(Ho, Wo), mode="bilinear", align_corners=False).squeeze(0).permute(1, 2, 0)
    out = out.reshape(Ho * Wo, table.shape[2])

    def bwd(dout):
        return torch.autograd.grad(out, t, dout.to(table.dtype), retain_graph=True)[0]
    return out.detach(), bwd


# ---- launch geometry ---------------------------------------------------------------------------------------------------------------------------
def test_launch_geometry():
    assert all(R.ln_vec(d) and not R.ln_vec(d, aligned=False) for d in R.LN_VEC_DIMS) and not any(R.ln_vec(d) for d in R.LN_SCALAR_DIMS)
    assert all(R.gather_vec(d) and not R.gather_vec(d, aligned=False) for d in R.GATHER_VEC_DIMS) and not any(R.gather_vec(d) for d in R.GATHER_SCALAR_DIMS)
    # both lane strides have dims one short of, on and one over them, and dims with and without a ragged last trip
    assert {252, 256, 260} <= set(R.LN_VEC_DIMS) and {63, 65} <= set(R.LN_SCALAR_DIMS) and 64 in R.LN_VEC_DIMS      # 64: scalar form by alignment
    assert [d % R.VEC_STRIDE for d in R.LN_VEC_DIMS] == [4, 64, 252, 0, 4, 0, 0, 4, 0]
    assert [d % R.SCALAR_STRIDE for d in R.LN_SCALAR_DIMS] == [1, 10, 63, 1, 2, 2]
    assert sorted(r % R.ROWS_PER_BLOCK for r in R.LN_ROWS) == [0, 1, 1, 2, 3]
    assert sorted({r % R.ROWS_PER_BLOCK for r in R.GATHER_ROWS + (R.GATHER_MANY_ROWS,)}) == [0, 1, 3] and R.GATHER_MANY_ROWS > 4 * 2048
    assert [R.patchify_sweeps(*c) for c in R.PATCHIFY_CASES] == [1] * len(R.PATCHIFY_CASES)
    H, W, P = R.PATCHIFY_ONE_SWEEP
    assert (H // P) * (W // P) * P * P == R.PATCHIFY_SWEEP and R.patchify_sweeps(H, W, P) == 1
    H, W, P = R.PATCHIFY_TWO_SWEEPS
    assert (H // P) * (W // P) * P * P == R.PATCHIFY_SWEEP + 16384 and R.patchify_sweeps(H, W, P) == 2
    assert any(H % P or W % P for H, W, P in R.PATCHIFY_CASES) and any(P % 4 for _, _, P in R.PATCHIFY_CASES) and any(P == 1 for _, _, P in R.PATCHIFY_CASES)
    assert [R.cast_first_sweep(n) for n in R.CAST_SMALL] == [0, 0, 0, 4, 4, 4, 1000, 1024]
    assert [R.cast_first_sweep(n) for n in R.CAST_LARGE] == [R.CAST_SWEEP] * 4
    assert [n - R.cast_first_sweep(n) for n in R.CAST_LARGE] == [0, 4, 1027, R.CAST_SWEEP + 3] and [n % 4 for n in R.CAST_LARGE] == [0, 0, 3, 3]
    cells = sorted({(Ho * Wo) % 4 for _, (Ho, Wo) in R.PE_OTHER + R.PE_OTHER_EXTRA})
    assert cells == [0, 1, 2, 3]
    assert R.edge_cells(77) == [0, 3, 4, 76] and R.edge_cells(1) == [0] and R.edge_cells(4) == [0, 3]
    assert {e < 64 for e in R.PE_DYADIC_E} == {True, False} and 64 in R.PE_DYADIC_E and 65 in R.PE_DYADIC_E


# ---- the references equal aten --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.LN_FAMILIES)
def test_layernorm_reference_is_aten(kind):
    for rows, dim in [(1, 1), (3, 10), (5, 96), (130, 260), (5, 4100)]:
        x, w, b = (t.double() for t in R.ln_inputs(kind, rows, dim, seed=R.ln_seed(rows, dim)))
        ref = F.layer_norm(x, (dim,), w, b, R.LN_EPS)
        assert torch.allclose(R.layernorm(x, w, b, R.LN_EPS), ref, rtol=1e-9, atol=1e-9), (kind, rows, dim)
    x, w, b = R.ln_inputs("const", 5, 260, seed=1)
    for dtype in (torch.float64, torch.float32):
        assert torch.equal(R.layernorm(x, w, b, R.LN_EPS, dtype=dtype), b.to(dtype).expand(5, 260))


@pytest.mark.parametrize("H,W,P", R.PATCHIFY_CASES + (R.PATCHIFY_TWO_SWEEPS,))
def test_patchify_reference_is_unfold(H, W, P):
    img = R.distinct_pixels(H, W)
    ref = torch.nn.Unfold(P, stride=P)(img.double().unsqueeze(0))[0].transpose(0, 1)
    n = (H // P) * (W // P)
    assert ref.shape == (n, P * P) and torch.equal(R.patchify(img, P), ref)
    wide = R.patchify(img, P, rows=n + 5, row0=2, ld=P * P + 3)
    assert torch.equal(wide[2:2 + n, :P * P], ref)
    wide[2:2 + n, :P * P] = R.POISON
    assert bool((wide == R.POISON).all())


def test_gather_reference_is_indexing():
    for rows, dim in [(1, 4), (5, 10), (33, 260)]:
        table, add = R.int_tensor((rows + 1, dim), seed=rows), R.int_tensor((rows, dim), seed=rows + 1)
        for pattern in R.GATHER_PATTERNS:
            idx = R.gather_index(pattern, rows, rows + 1, seed=dim)
            assert idx.dtype == torch.int32 and int(idx.min()) >= 0 and int(idx.max()) <= rows
            assert torch.equal(R.gather_rows(table, idx, add), table.double()[idx.long()] + add.double())
            assert torch.equal(R.gather_rows(table, idx), torch.index_select(table.double(), 0, idx.long()))
    idx = R.gather_index("pad", 33, 34)
    assert idx.tolist() == list(range(22)) + [33] * 11
    idx = R.gather_index("random", 33, 34, seed=3)
    assert idx.unique().numel() < 33


def test_bf16_reference_is_aten():
    x = R.bf16_edge_set()
    assert x.numel() == 391680 and int(torch.isnan(x).sum()) == 1534 and int(torch.isinf(x).sum()) == 2
    u = R.f32_to_bits(x)
    assert bool(((u >> 23) & 0xFF != 0).all()) and torch.equal(R.f32_to_bits(R.bits_to_f32(u)), u)
    ok = ~torch.isnan(x)
    assert torch.equal(R.bf16_bits(x)[ok], R.bf16_to_bits(x.to(torch.bfloat16))[ok])
    assert R.same_bf16(R.bf16_to_bits(x.to(torch.bfloat16)), x)
    z = torch.tensor([0.0, -0.0])
    assert R.bf16_bits(z).tolist() == [0, 0x8000] == R.bf16_to_bits(z.to(torch.bfloat16)).tolist()
    # what the set holds: ties that go up and ties that go down, overflow to inf from the largest finite exponent, both infinities
    bits = R.bf16_bits(x)
    tie = (u & 0xFFFF) == 0x8000
    assert bool((bits[tie & ok] == (u[tie & ok] >> 16) + 1).any()) and bool((bits[tie & ok] == (u[tie & ok] >> 16)).any())
    assert bool(((bits == 0x7F80) & torch.isfinite(x)).any()) and bool(((bits == 0xFF80) & torch.isfinite(x)).any())
    assert bool(R.bf16_is_nan(R.bf16_to_bits(x.to(torch.bfloat16)))[~ok].all()) and not bool(R.bf16_is_nan(bits)[ok].any())
    for n in R.CAST_SMALL:
        y = torch.randn(n, generator=torch.Generator().manual_seed(n))
        assert torch.equal(R.bf16_bits(y), R.bf16_to_bits(y.to(torch.bfloat16)))
    c = R.int_cycle(40)
    assert c[:18].tolist() == list(range(-8, 9)) + [-8] and torch.equal(c.to(torch.bfloat16).float(), c)


@pytest.mark.parametrize("sizes", R.PE_DYADIC + R.PE_OTHER + R.PE_OTHER_EXTRA)
def test_pe_interp_reference_is_aten(sizes):
    """float64 reference against float64 aten (which forms the source index in float64: 1e-5 covers the float32 index of the reference, the
    dyadic sizes are equal), float32 reference against float32 aten (the same index arithmetic: 2e-6 for the order of the blend)."""
    (Hin, Win), (Ho, Wo) = sizes
    dyadic = sizes in R.PE_DYADIC
    for E in (1, 10, 65):
        table, dout = R.pe_inputs(Hin, Win, E, Ho, Wo, seed=E, integers=False)
        for dtype in (torch.float64, torch.float32):
            ref, bwd = aten_interp(table.to(dtype), Ho, Wo)
            out = R.pe_interp(table, Ho, Wo, dtype=dtype)
            dt = R.pe_interp_bwd(dout, Ho, Wo, (Hin, Win, E), dtype=dtype)
            assert out.dtype == dt.dtype == dtype and out.shape == (Ho * Wo, E) and dt.shape == (Hin, Win, E)
            loose = 1.0 if dtype == torch.float32 else 5.0      # an ulp of a float32 source index near 10, times a neighbour difference of a few
            assert maxabs(out, ref) <= (1e-12 if dyadic and dtype == torch.float64 else loose * 2e-6), (sizes, E, dtype)
            assert maxabs(dt, bwd(dout)) <= (1e-11 if dyadic and dtype == torch.float64 else loose * 2e-5), (sizes, E, dtype)


# ---- the exactness the GPU tests rely on ------------------------------------------------------------------------------------------------------------
def test_distinct_pixels_are_exact():
    H, W, _ = max((R.PATCHIFY_ONE_SWEEP, R.PATCHIFY_TWO_SWEEPS) + R.PATCHIFY_CASES, key=lambda c: c[0] * c[1])
    assert (H, W) == (1040, 1024) and H * W < 2 ** 24
    img = R.distinct_pixels(H, W)
    assert torch.equal(img.double().view(-1), torch.arange(H * W, dtype=torch.float64)) and float(img.min()) >= 0 > R.POISON
    assert torch.equal(torch.tensor(R.POISON).to(torch.bfloat16).float(), torch.tensor(R.POISON))


@pytest.mark.parametrize("sizes", R.PE_DYADIC)
def test_dyadic_interpolation_is_exact_in_fp32(sizes):
    """Integer table and dout at power-of-two ratios: float32 equals float64 bit for bit, in the reference and in aten, forward and backward, and
    the reference equals aten; the identity size copies a random table."""
    (Hin, Win), (Ho, Wo) = sizes
    for E in R.PE_DYADIC_E:
        table, dout = R.pe_inputs(Hin, Win, E, Ho, Wo, seed=E, integers=True)
        out64, out32 = R.pe_interp(table, Ho, Wo), R.pe_interp(table, Ho, Wo, dtype=torch.float32)
        dt64, dt32 = R.pe_interp_bwd(dout, Ho, Wo, (Hin, Win, E)), R.pe_interp_bwd(dout, Ho, Wo, (Hin, Win, E), dtype=torch.float32)
        assert torch.equal(out32.double(), out64) and torch.equal(dt32.double(), dt64)
        assert float(out64.min()) > R.POISON
        for dtype in (torch.float64, torch.float32):
            ref, bwd = aten_interp(table.to(dtype), Ho, Wo)
            assert torch.equal(ref.double(), out64) and torch.equal(bwd(dout).double(), dt64)
        # a backward that walks the cells in another order gives the same sums
        perm = torch.randperm(Ho * Wo, generator=torch.Generator().manual_seed(E))
        acc = torch.zeros(Hin, Win, E)
        for c in perm.tolist():
            acc += R.pe_interp_bwd(R.one_cell(dout, c), Ho, Wo, (Hin, Win, E), dtype=torch.float32)
        assert torch.equal(acc.double(), dt64)
    if (Hin, Win) == (Ho, Wo):
        table, _ = R.pe_inputs(Hin, Win, 65, Ho, Wo, seed=1, integers=False)
        assert torch.equal(R.pe_interp(table, Ho, Wo, dtype=torch.float32), table.view(-1, 65))


@pytest.mark.parametrize("sizes", [((1, 1), (3, 4)), ((6, 10), (7, 11))])
def test_other_ratios_are_not_exact(sizes):
    """Why the other sizes get a bar: float32 and float64 differ there."""
    (Hin, Win), (Ho, Wo) = sizes
    table, dout = R.pe_inputs(Hin, Win, 10, Ho, Wo, seed=1, integers=True)
    fwd = torch.equal(R.pe_interp(table, Ho, Wo, dtype=torch.float32).double(), R.pe_interp(table, Ho, Wo))
    bwd = torch.equal(R.pe_interp_bwd(dout, Ho, Wo, (Hin, Win, 10), dtype=torch.float32).double(), R.pe_interp_bwd(dout, Ho, Wo, (Hin, Win, 10)))
    assert not (fwd and bwd)


@pytest.mark.parametrize("sizes", R.PE_OTHER + R.PE_OTHER_EXTRA)
def test_other_ratios_fp32_inside_bars(sizes):
    (Hin, Win), (Ho, Wo) = sizes
    for E in R.PE_OTHER_E:
        table, dout = R.pe_inputs(Hin, Win, E, Ho, Wo, seed=E, integers=False)
        assert maxabs(R.pe_interp(table, Ho, Wo, dtype=torch.float32), R.pe_interp(table, Ho, Wo)) <= 0.25 * R.PE_FWD_BAR
        assert maxabs(R.pe_interp_bwd(dout, Ho, Wo, (Hin, Win, E), dtype=torch.float32), R.pe_interp_bwd(dout, Ho, Wo, (Hin, Win, E))) <= 0.25 * R.PE_BWD_BAR
        for c in R.edge_cells(Ho * Wo):      # one loud cell: at most four table cells are touched, each by one product
            d1 = R.pe_interp_bwd(R.one_cell(dout, c), Ho, Wo, (Hin, Win, E))
            assert 1 <= int(d1.abs().sum(2).ne(0).sum()) <= 4
            assert maxabs(R.pe_interp_bwd(R.one_cell(dout, c), Ho, Wo, (Hin, Win, E), dtype=torch.float32), d1) <= 0.25 * R.PE_BWD_BAR


# ---- the LayerNorm bars are measured here --------------------------------------------------------------------------------------------------------------
def ln_err32(kind):
    worst = 0.0
    for rows, dim in R.ln_cases(kind):
        x, w, b = R.ln_inputs(kind, rows, dim, seed=R.ln_seed(rows, dim))
        worst = max(worst, maxabs(R.layernorm(x, w, b, R.LN_EPS, dtype=torch.float32), R.layernorm(x, w, b, R.LN_EPS)))
    return worst


@pytest.mark.parametrize("kind", ["randn3p1", "mean100", "tiny_var"])
def test_layernorm_fp32_error_is_the_recorded_constant(kind):
    """The plain fp32 evaluation's largest error over the family's case shapes is what fwd_row_reference.LN_ERR32 records: not above it, and
    not below a quarter of it (torch's fp32 row sum changes its order with the host's vector width, the constant should not be stale by more)."""
    got = ln_err32(kind)
    print(f"layernorm fp32 plain evaluation, {kind}: max error {got:.3e} against float64 (recorded {R.LN_ERR32[kind]:.3e})")
    assert 0.25 * R.LN_ERR32[kind] <= got <= R.LN_ERR32[kind]
    assert R.LN_BAR[kind] == (2e-5 if kind == "randn3p1" else 4 * R.LN_ERR32[kind]) and got <= 0.25 * R.LN_BAR[kind]


# ---- every defect moves the reference by at least four bars of the case meant to catch it, or breaks its exact comparison ------------------------------
def test_every_defect_is_covered():
    covered = {"one_pass_var", "eps_outside_sqrt", "drop_row_tail", "drop_last_row", "truncate_bf16", "align_corners", "no_index_clamp",
               "neighbour_past_edge", "patch_transposed", "single_sweep"}
    assert covered == set(R.DEFECTS)


def test_layernorm_statistics_defects_show():
    """"one_pass_var" (in fp32, where it cancels) on every large-mean case, "eps_outside_sqrt" on every tiny-variance case."""
    for rows, dim in R.ln_cases("mean100"):
        x, w, b = R.ln_inputs("mean100", rows, dim, seed=R.ln_seed(rows, dim))
        moved = maxabs(R.layernorm(x, w, b, R.LN_EPS, dtype=torch.float32, defect="one_pass_var"), R.layernorm(x, w, b, R.LN_EPS))
        assert moved >= 4 * R.LN_BAR["mean100"], (rows, dim, moved)
    for rows, dim in R.ln_cases("tiny_var"):
        x, w, b = R.ln_inputs("tiny_var", rows, dim, seed=R.ln_seed(rows, dim))
        moved = maxabs(R.layernorm(x, w, b, R.LN_EPS, defect="eps_outside_sqrt"), R.layernorm(x, w, b, R.LN_EPS))
        assert moved >= 4 * R.LN_BAR["tiny_var"], (rows, dim, moved)
        var = float(x.double().var(1, unbiased=False).mean())
        assert 0.5e-6 < var < 2e-6 < R.LN_EPS


def test_layernorm_launch_defects_show():
    """"drop_row_tail" at every dim with a ragged last trip of the form that serves it (the unaligned views put the vector dims on the scalar
    form's stride of 64), "drop_last_row" at every row count from four up."""
    forms = [(d, True) for d in R.LN_VEC_DIMS] + [(d, False) for d in R.LN_SCALAR_DIMS + R.LN_VEC_DIMS]
    ragged = {True: 0, False: 0}
    for dim, vec in forms:
        stride = R.lane_stride(vec)
        for rows in R.LN_ROWS:
            x, w, b = R.ln_inputs("randn3p1", rows, dim, seed=R.ln_seed(rows, dim))
            ref = R.layernorm(x, w, b, R.LN_EPS)
            tail = R.layernorm(x, w, b, R.LN_EPS, defect="drop_row_tail", stride=stride)
            if dim % stride:
                ragged[vec] += 1
                assert maxabs(tail, ref) >= 4 * R.LN_BAR["randn3p1"], (rows, dim, vec)
            else:
                assert torch.equal(tail, ref)
            last = R.layernorm(x, w, b, R.LN_EPS, defect="drop_last_row")
            assert (maxabs(last, ref) >= 4 * R.LN_BAR["randn3p1"]) == (rows >= 4), (rows, dim)
    assert ragged[True] >= 4 * len(R.LN_ROWS) and ragged[False] >= 10 * len(R.LN_ROWS)
    assert sum(r >= 4 for r in R.LN_ROWS) >= 3


def test_patchify_defects_show():
    for H, W, P in R.PATCHIFY_CASES + (R.PATCHIFY_ONE_SWEEP, R.PATCHIFY_TWO_SWEEPS):
        img = R.distinct_pixels(H, W)
        ref = R.patchify(img, P)
        assert torch.equal(R.patchify(img, P, defect="patch_transposed"), ref) == (P == 1), (H, W, P)
        assert torch.equal(R.patchify(img, P, defect="single_sweep"), ref) == ((H, W, P) != R.PATCHIFY_TWO_SWEEPS), (H, W, P)
        assert torch.equal(ref.to(torch.bfloat16).double(), ref) == (H * W <= 257)      # bf16 output: the comparison is against the rounded reference
        if P > 1:
            assert not torch.equal(R.patchify(img, P, defect="patch_transposed").to(torch.bfloat16), ref.to(torch.bfloat16)), (H, W, P)
    H, W, P = R.PATCHIFY_TWO_SWEEPS
    left = R.patchify(R.distinct_pixels(H, W), P, defect="single_sweep") == R.POISON
    assert int(left.sum()) == 16384 and bool(left[-64:].any(1).all()) and not bool(left[:-64].any())      # the last patch row of the image
    assert not torch.equal(R.patchify(R.distinct_pixels(H, W), P, defect="single_sweep").to(torch.bfloat16), R.patchify(R.distinct_pixels(H, W), P).to(torch.bfloat16))


def test_gather_defects_show():
    forms = [(d, True) for d in R.GATHER_VEC_DIMS] + [(d, False) for d in R.GATHER_SCALAR_DIMS + R.GATHER_VEC_DIMS]
    ragged = {True: 0, False: 0}
    for dim, vec in forms:
        for rows in R.GATHER_ROWS:
            table, add = R.int_tensor((rows + 1, dim), seed=dim), R.int_tensor((rows, dim), seed=dim + 1)
            assert float(table.min()) >= -8 > R.POISON and float(add.min()) >= -8
            for pattern in R.GATHER_PATTERNS:
                idx = R.gather_index(pattern, rows, rows + 1, seed=rows)
                for a in (add, None):
                    ref = R.gather_rows(table, idx, a)
                    assert torch.equal(ref.float().double(), ref)
                    tail = R.gather_rows(table, idx, a, defect="drop_row_tail", stride=R.lane_stride(vec))
                    assert torch.equal(tail, ref) == (dim % R.lane_stride(vec) == 0)
                    ragged[vec] += dim % R.lane_stride(vec) != 0
                    assert torch.equal(R.gather_rows(table, idx, a, defect="drop_last_row"), ref) == (rows < 4)
    assert ragged[True] and ragged[False]
    assert R.GATHER_MANY_ROWS % 4 == 0      # the many-row case ends on a full workgroup: its last row is one that "drop_last_row" skips


def test_cast_defects_show():
    x = R.bf16_edge_set()
    good = R.bf16_bits(x)
    ok = ~torch.isnan(x)
    aten = R.bf16_to_bits(x.to(torch.bfloat16))
    assert R.same_bf16(aten, x) and not R.same_bf16(torch.where(ok, R.bf16_bits(x, defect="truncate_bf16"), aten), x)
    differs = (R.bf16_bits(x, defect="truncate_bf16") != good) & ok
    lows = R.f32_to_bits(x) & 0xFFFF
    assert sorted(set(lows[differs].tolist())) == [0x8000, 0x8001, 0xFFFF] and not bool(differs[lows < 0x8000].any())
    up = differs & (lows == 0x8000)
    assert bool((((R.f32_to_bits(x) >> 16) & 1)[up] == 1).all())             # only the odd ties go up
    # "single_sweep": the elements beyond the first trip hold integers whose bf16 differs from a poisoned destination's
    for n in R.CAST_LARGE[1:]:
        first = R.cast_first_sweep(n)
        rest = R.int_cycle(n)[first:]
        assert rest.numel() >= 4 and bool((R.bf16_bits(rest) != int(R.bf16_bits(torch.tensor([R.POISON]))[0])).all())
    assert R.cast_first_sweep(R.CAST_LARGE[0]) == R.CAST_LARGE[0]


PE_CATCHES = {      # the sizes that must catch each defect (others may: the assertion is "at least these")
    "align_corners": R.PE_DYADIC[:2] + R.PE_DYADIC[3:] + R.PE_OTHER[:3] + (R.PE_OTHER[5],) + R.PE_OTHER_EXTRA,
    "no_index_clamp": R.PE_DYADIC[:2] + (R.PE_DYADIC[5],) + R.PE_OTHER[:3] + R.PE_OTHER_EXTRA,           # upscaling along an axis with more than one cell
    # upscaling along an axis, in a table of more than one cell (in a 1 x 1 table every neighbour is the cell itself)
    "neighbour_past_edge": R.PE_DYADIC[:2] + (R.PE_DYADIC[5],) + R.PE_OTHER[:3] + (R.PE_OTHER[4],) + R.PE_OTHER_EXTRA,
    "drop_last_row": R.PE_DYADIC + R.PE_OTHER[:5] + R.PE_OTHER_EXTRA,                                      # four cells or more
}


@pytest.mark.parametrize("defect", sorted(PE_CATCHES))
def test_interpolation_defects_show(defect):
    for sizes in PE_CATCHES[defect]:
        (Hin, Win), (Ho, Wo) = sizes
        if sizes in R.PE_DYADIC:
            for E in R.PE_DYADIC_E:
                table, dout = R.pe_inputs(Hin, Win, E, Ho, Wo, seed=E, integers=True)
                assert not torch.equal(R.pe_interp(table, Ho, Wo, defect=defect), R.pe_interp(table, Ho, Wo)), (sizes, E)
                assert not torch.equal(R.pe_interp_bwd(dout, Ho, Wo, (Hin, Win, E), defect=defect), R.pe_interp_bwd(dout, Ho, Wo, (Hin, Win, E))), (sizes, E)
        else:
            for E in R.PE_OTHER_E:
                table, dout = R.pe_inputs(Hin, Win, E, Ho, Wo, seed=E, integers=False)
                assert maxabs(R.pe_interp(table, Ho, Wo, defect=defect), R.pe_interp(table, Ho, Wo)) >= 4 * R.PE_FWD_BAR, (sizes, E)
                shape = (Hin, Win, E)
                assert maxabs(R.pe_interp_bwd(dout, Ho, Wo, shape, defect=defect), R.pe_interp_bwd(dout, Ho, Wo, shape)) >= 4 * R.PE_BWD_BAR, (sizes, E)
                if defect == "drop_last_row":      # the loud cell that sits on it: the whole result is gone
                    assert 3 in R.edge_cells(Ho * Wo)
                    assert maxabs(R.pe_interp_bwd(R.one_cell(dout, 3), Ho, Wo, shape, defect=defect), R.pe_interp_bwd(R.one_cell(dout, 3), Ho, Wo, shape)) >= 4 * R.PE_BWD_BAR


def test_lost_or_doubled_cell_shows_under_the_loud_cell_bar():
    """A cell the backward loses (or adds twice) moves the table by that cell's whole contribution: with one loud cell that is the whole
    result and clears four times the backward bar at every loud cell of every size, whatever the cell's weights and values."""
    for (Hin, Win), (Ho, Wo) in R.PE_OTHER + R.PE_OTHER_EXTRA:
        table, dout = R.pe_inputs(Hin, Win, 10, Ho, Wo, seed=10, integers=False)
        for c in R.edge_cells(Ho * Wo):
            whole = R.pe_interp_bwd(R.one_cell(dout, c), Ho, Wo, (Hin, Win, 10))
            assert float(whole.abs().max()) >= 4 * R.PE_BWD_BAR, ((Hin, Win), (Ho, Wo), c)
