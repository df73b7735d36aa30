"""Plain references for the forward row kernels of `acai_omr_amd/csrc/elementwise.hip` (LayerNorm forward, patchify, the row gather, the
fp32 -> bf16 cast, the positional-embedding bilinear interpolation and its transpose), the probe inputs the tests feed them, and the launch
geometry those inputs are built around.

Every formula is written out by hand and evaluated in the dtype that is asked for: float64 gives the reference the GPU tests compare
against, float32 the "plain evaluation" whose own error shows how much of a bar a correct fp32 kernel may use up.

Wherever the operation allows it the inputs make the comparison exact, so that one misplaced, dropped or unwritten element fails it:

  distinct pixels   img[y, x] = y * W + x, exact in fp32 below 2^24: any misplaced element of patchify shows.
  exact integers    values in [-8, 8] for the gather (table and add) and for the interpolation at power-of-two ratios, where every weight is
                    a multiple of 1/64, so forward and backward are exact in fp32 in any summation order.
  one loud cell     the interpolation backward at other ratios: dout is zero except in cell c, and c walks the edges of a workgroup.
  the bf16 edge set every 16-bit high half with the low halves that sit on and next to a rounding tie (`bf16_edge_set`).

Outputs that a defective kernel would leave unwritten are modelled by `POISON`, the value the GPU tests fill caller-given buffers with.

The references can be broken on purpose (`defect=`, as tests/row_reference.py and tests/attn_probe.py do);
tests/test_fwd_row_reference_cpu.py holds every defect to at least four times the bar of the case that is meant to catch it, or to a broken
exact comparison.

  "one_pass_var"        LayerNorm variance as E[x^2] - mean^2 (a defect of fp32 arithmetic: evaluate it with dtype=torch.float32)
  "eps_outside_sqrt"    1 / (sqrt(var) + eps) instead of 1 / sqrt(var + eps)
  "drop_row_tail"       the last dim % stride elements of a row are not summed (LayerNorm) or not written (gather)
  "drop_last_row"       the last row or cell of every group of four is skipped
  "truncate_bf16"       fp32 -> bf16 by dropping the low half (round toward zero)
  "align_corners"       the interpolation's source index as o * (in - 1) / (out - 1)
  "no_index_clamp"      a negative source index is not clamped to 0
  "neighbour_past_edge" the +1 neighbour is taken at the last index too (the flat table index is clamped so that it stays inside the table)
  "patch_transposed"    kh and kw swapped inside a patch
  "single_sweep"        elements beyond the first grid sweep are left at their initial value

Everything is CPU torch."""
import torch

DEFECTS = ("one_pass_var", "eps_outside_sqrt", "drop_row_tail", "drop_last_row", "truncate_bf16", "align_corners", "no_index_clamp",
           "neighbour_past_edge", "patch_transposed", "single_sweep")
POISON = -512.0         # exact in bf16; no probe input and no correct output of an exact-comparison case takes this value


def cdiv(a, b):
    return (a + b - 1) // b


# ---- launch geometry (restated from the dispatch code of elementwise.hip: the cases sit on its edges) -------------------------------------
ROWS_PER_BLOCK = 4                  # LayerNorm, gather, interpolation: one wave per row / cell, four waves per workgroup
VEC_STRIDE, SCALAR_STRIDE = 256, 64  # elements a wave covers per trip: 64 lanes x float4, or 64 lanes x one float
PATCHIFY_SWEEP = 4096 * 256         # patchify: at most 4096 workgroups of 256 threads, one element per thread and trip
CAST_SWEEP = 4096 * 1024            # cast: at most 4096 workgroups of 256 threads, four elements per thread and trip


def ln_vec(dim, aligned=True):
    """LayerNorm takes the float4 kernel when dim % 4 == 0 and x, w, b and both outputs are 16-byte aligned."""
    return dim % 4 == 0 and aligned


def gather_vec(dim, aligned=True):
    """The gather takes the float4 kernel when dim % 4 == 0 and table, out and add are 16-byte aligned."""
    return dim % 4 == 0 and aligned


def lane_stride(vec):
    return VEC_STRIDE if vec else SCALAR_STRIDE


def patchify_sweeps(H, W, P):
    total = (H // P) * (W // P) * P * P
    return cdiv(total, min(4096, cdiv(total, 256)) * 256)


def cast_first_sweep(n):
    """Elements the first trip of the cast's grid-stride loop covers (the n % 4 tail is written by workgroup 0 outside the loop)."""
    grid = min(4096, max(1, cdiv(n // 4, 256)))
    return min(n & ~3, grid * 1024)


def edge_cells(cells):
    """First cell, last wave of the first workgroup, first wave of the second, the last cell."""
    return sorted({c for c in (0, 3, 4, cells - 1) if 0 <= c < cells})


# ---- the cases (shared by the CPU and the GPU module) -----------------------------------------------------------------------------------------
# dim 64 is a multiple of four, so an aligned row of it takes the vector form (one trip, 16 busy lanes); the scalar form meets it, exactly
# one trip of its 64-lane stride, through the unaligned views that every vector dim is also run as
LN_VEC_DIMS = (4, 64, 252, 256, 260, 768, 1024, 1028, 1280)
LN_SCALAR_DIMS = (1, 10, 63, 65, 130, 258)
LN_ROWS = (1, 3, 4, 5, 130)
LN_FAMILY_DIMS = (96, 768, 1280, 4100, 130)    # large-mean and tiny-variance rows: vector dims below, on and above a 256 stride, one scalar dim
LN_FAMILY_ROWS = (5, 130)
LN_EPS = 1e-5

PATCHIFY_CASES = ((16, 16, 16), (32, 64, 16), (37, 53, 16), (12, 20, 4), (6, 10, 2), (9, 15, 3), (10, 5, 5), (3, 7, 1))
PATCHIFY_ONE_SWEEP = (512, 2048, 16)
PATCHIFY_TWO_SWEEPS = (1040, 1024, 16)

GATHER_VEC_DIMS = (4, 24, 256, 260, 768, 1024)
GATHER_SCALAR_DIMS = (1, 10, 65, 130, 258)
GATHER_ROWS = (1, 3, 4, 5, 33)
GATHER_MANY_ROWS = 8200             # 2050 workgroups; the row count enters the kernel apart from dim, so a few dims carry it
GATHER_MANY_DIMS = (4, 24, 256, 10, 65)
GATHER_PATTERNS = ("identity", "reversed", "one_row", "pad", "random")

CAST_SMALL = (1, 2, 3, 4, 5, 7, 1003, 1024)
CAST_LARGE = (CAST_SWEEP, CAST_SWEEP + 4, CAST_SWEEP + 1027, 2 * CAST_SWEEP + 3)

PE_DYADIC = (((3, 5), (6, 10)), ((3, 5), (12, 20)), ((3, 5), (3, 5)), ((4, 6), (2, 3)), ((8, 12), (4, 6)), ((1, 7), (2, 14)))
PE_DYADIC_E = (1, 10, 64, 65, 70, 130)
PE_OTHER = (((6, 10), (7, 11)), ((6, 10), (7, 5)), ((4, 8), (9, 3)), ((1, 1), (3, 4)), ((5, 1), (5, 3)), ((5, 5), (1, 1)))    # cells % 4: 1 3 3 0 3 1
PE_OTHER_EXTRA = (((6, 10), (7, 6)),)      # 42 cells: cells % 4 == 2, which the six sizes above do not take
PE_OTHER_E = (10, 65)
PE_FWD_BAR, PE_BWD_BAR = 1e-5, 1e-4         # the project's bars (test_pe_interpolation_kernel_vs_aten)

# Largest error of the plain fp32 evaluation (`layernorm(..., dtype=torch.float32)`) against float64, per input family, as measured by
# tests/test_fwd_row_reference_cpu.py::test_layernorm_fp32_error_is_the_recorded_constant over every case shape of the family:
#   randn3p1  LN_VEC_DIMS + LN_SCALAR_DIMS x LN_ROWS, and LN_FAMILY_DIMS x LN_FAMILY_ROWS
#   mean100, tiny_var   LN_FAMILY_DIMS x LN_FAMILY_ROWS
#   measured: randn3p1 1.744e-6, mean100 6.348e-5, tiny_var 1.242e-4
# The constants are the measured maxima plus a tenth, rounded up to two digits: torch's fp32 row sum takes its order from the host's vector
# width, and the tenth keeps the constant an upper bound on another host.  The test holds the measurement between a quarter of the constant and
# the constant.
LN_ERR32 = {"randn3p1": 2.0e-6, "mean100": 7.0e-5, "tiny_var": 1.4e-4}
# The GPU bar of a family is four times its constant: the device reduces in another order and contracts to FMAs.  randn * 3 + 1 stays at the
# 2e-5 the project already holds (test_gpu_kernels.py::test_layernorm).
LN_BAR = {"randn3p1": 2e-5, "mean100": 4 * LN_ERR32["mean100"], "tiny_var": 4 * LN_ERR32["tiny_var"]}


def ln_cases(kind):
    """(rows, dim) of every LayerNorm case of an input family."""
    family = [(r, d) for d in LN_FAMILY_DIMS for r in LN_FAMILY_ROWS]
    if kind == "randn3p1":
        return [(r, d) for d in LN_VEC_DIMS + LN_SCALAR_DIMS for r in LN_ROWS] + family
    return family


def ln_seed(rows, dim):
    return rows * 4099 + dim


# ---- probe inputs ------------------------------------------------------------------------------------------------------------------------------
def int_tensor(shape, seed):
    """Integers in [-8, 8] as float32."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, tuple(shape), generator=g).float()


def int_cycle(n):
    """The integers -8 .. 8 in turn, as float32: element i holds i % 17 - 8."""
    return (torch.arange(n, dtype=torch.int64) % 17 - 8).float()


def distinct_pixels(H, W):
    """(1, H, W) image with img[y, x] = y * W + x."""
    return torch.arange(H * W, dtype=torch.float32).view(1, H, W)


LN_FAMILIES = ("randn3p1", "mean100", "tiny_var", "const")
LN_CONST = 0.75     # dyadic: the sum of up to 2^22 of them, and so the mean, is exact in fp32 in any order


def ln_inputs(kind, rows, dim, seed):
    """(x, w, b).  "randn3p1": randn * 3 + 1, the project's LayerNorm input; "mean100": randn + 100; "tiny_var": 0.75 + randn * 2^-10, a row
    whose variance (~1e-6) is the size of eps; "const": every element 0.75, whose output is exactly b.  w, b = randn."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(rows, dim, generator=g)
    w, b = torch.randn(dim, generator=g), torch.randn(dim, generator=g)
    if kind == "randn3p1":
        x = r * 3 + 1
    elif kind == "mean100":
        x = r + 100
    elif kind == "tiny_var":
        x = LN_CONST + r * 2.0 ** -10
    else:
        assert kind == "const", kind
        x = torch.full((rows, dim), LN_CONST)
    return x, w, b


def gather_index(pattern, rows, table_rows, seed=0):
    """int32 index of `rows` entries into a table of `table_rows` >= rows + 1 rows.  "pad" is the pad_rows pattern: a valid prefix, then the
    fill row (the table's last) repeated."""
    assert table_rows >= rows + 1
    if pattern == "identity":
        idx = torch.arange(rows)
    elif pattern == "reversed":
        idx = table_rows - 1 - torch.arange(rows)
    elif pattern == "one_row":
        idx = torch.full((rows,), table_rows // 2)
    elif pattern == "pad":
        idx = torch.arange(rows)
        idx[(2 * rows + 2) // 3:] = table_rows - 1
    else:
        assert pattern == "random", pattern
        g = torch.Generator().manual_seed(seed)
        idx = torch.randint(0, table_rows, (rows,), generator=g)
        idx[-1] = idx[0]            # a duplicate from two rows up
    return idx.to(torch.int32)


BF16_EDGE_LOWS = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)


def bf16_edge_set():
    """For every 16-bit high half h whose exponent field is not zero, and for the low halves 0x0000 (exact), 0x0001 / 0x7FFF (just above a
    bf16 value / just below a tie), 0x8000 (the tie: up when h is odd, down when it is even), 0x8001 / 0xFFFF (just above the tie / just below the
    next value), the float with the pattern (h << 16) | low: 391 680 values, 1 534 of them NaN.  Ties in both directions and their neighbours,
    the carry into the exponent, overflow to inf (0x7F7F8000 and up), +-inf and the NaNs are all in it.  The fp32 subnormals (exponent field
    zero) are left out, because whether the device flushes them is not for this test to pin; that rule leaves out +-0 as well, which the GPU
    test casts next to the set."""
    h = torch.arange(65536, dtype=torch.int64)
    h = h[(h & 0x7F80) != 0]
    u = ((h[:, None] << 16) | torch.tensor(BF16_EDGE_LOWS, dtype=torch.int64)[None, :]).reshape(-1)
    return bits_to_f32(u)


def bits_to_f32(u):
    """int64 holding 32-bit patterns -> float32."""
    return torch.where(u >= 2 ** 31, u - 2 ** 32, u).to(torch.int32).view(torch.float32)


def f32_to_bits(x):
    return x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def bf16_to_bits(y):
    return y.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


# ---- LayerNorm forward -------------------------------------------------------------------------------------------------------------------------
def layernorm(x, w, b, eps, dtype=torch.float64, defect=None, stride=None):
    """y = (x - mean) / sqrt(var + eps) * w + b per row: two passes, biased variance, eps inside the square root.
    stride: the lane stride of the kernel form the case reaches; "drop_row_tail" leaves the last dim % stride elements out of both sums."""
    x, w, b = x.to(dtype), w.to(dtype), b.to(dtype)
    dim = x.shape[1]
    keep = dim - dim % stride if defect == "drop_row_tail" else dim
    mean = x[:, :keep].sum(1, keepdim=True) / dim
    xc = x - mean
    if defect == "one_pass_var":
        var = (x * x)[:, :keep].sum(1, keepdim=True) / dim - mean * mean
    else:
        var = (xc * xc)[:, :keep].sum(1, keepdim=True) / dim
    rstd = 1.0 / (torch.sqrt(var) + eps) if defect == "eps_outside_sqrt" else 1.0 / torch.sqrt(var + eps)
    y = xc * rstd * w + b
    if defect == "drop_last_row":
        y[ROWS_PER_BLOCK - 1::ROWS_PER_BLOCK] = POISON
    return y


# ---- patchify --------------------------------------------------------------------------------------------------------------------------------------
def patchify(img, P, rows=None, row0=0, ld=None, dtype=torch.float64, defect=None):
    """img (1, H, W) -> a [rows, ld] buffer of POISON whose rows row0 .. row0 + n hold, in columns [0, P * P), the n = (H // P) * (W // P)
    patches: patch (i, j) in row row0 + i * wp + j, pixel (kh, kw) in column kh * P + kw.  H and W are floored to multiples of P."""
    H, W = img.shape[-2:]
    hp, wp = H // P, W // P
    n = hp * wp
    out = torch.full((row0 + n if rows is None else rows, P * P if ld is None else ld), POISON, dtype=dtype)
    i, kh, j, kw = torch.meshgrid(torch.arange(hp), torch.arange(P), torch.arange(wp), torch.arange(P), indexing="ij")
    v = img[0][i * P + kh, j * P + kw].to(dtype)
    row, col = row0 + i * wp + j, (kw * P + kh if defect == "patch_transposed" else kh * P + kw)
    if defect == "single_sweep":        # the kernel's element order: kw fastest, then j, kh, i
        first = (((i * P + kh) * wp + j) * P + kw) < PATCHIFY_SWEEP
        row, col, v = row[first], col[first], v[first]
    out[row, col] = v
    return out


# ---- row gather ------------------------------------------------------------------------------------------------------------------------------------
def gather_rows(table, idx, add=None, dtype=torch.float64, defect=None, stride=None):
    """out[r] = table[idx[r]] (+ add[r])."""
    out = table.to(dtype)[idx.long()]
    if add is not None:
        out = out + add.to(dtype)
    dim = out.shape[1]
    if defect == "drop_row_tail":
        out[:, dim - dim % stride:] = POISON
    elif defect == "drop_last_row":
        out[ROWS_PER_BLOCK - 1::ROWS_PER_BLOCK] = POISON
    return out


# ---- fp32 -> bf16 ----------------------------------------------------------------------------------------------------------------------------------
def bf16_bits(x, defect=None):
    """The bf16 bit pattern (int64 in [0, 65535]) of each fp32 element: round to nearest, ties to even, on the integer pattern.  Not meaningful
    for NaN (the carry can run out of the payload): NaNs are compared by NaN-ness."""
    u = f32_to_bits(x)
    if defect == "truncate_bf16":
        return u >> 16
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF


def bf16_is_nan(bits):
    return (bits & 0x7FFF) > 0x7F80


def same_bf16(got_bits, x, defect=None):
    """got_bits against bf16_bits(x): NaN wherever x is NaN, the same bits everywhere else."""
    ref, nan = bf16_bits(x, defect), torch.isnan(x)
    return bool(bf16_is_nan(got_bits)[nan].all()) and torch.equal(got_bits[~nan], ref[~nan])


# ---- positional-embedding interpolation: aten's upsample_bilinear2d, align_corners = False, on a (Hin, Win, E) table -----------------------------
def _source_index(n_in, n_out, defect):
    """(i0, i1, lambda1) per output index, in float32 exactly as aten computes them: scale = float(in) / float(out),
    src = max(scale * (o + 0.5) - 0.5, 0), i0 = trunc(src), i1 = i0 + 1 only below the last index, lambda1 = src - i0."""
    o = torch.arange(n_out, dtype=torch.float32)
    if defect == "align_corners":
        src = o * (torch.tensor(float(n_in - 1)) / torch.tensor(float(n_out - 1)) if n_out > 1 else torch.tensor(0.0))
    else:
        src = (torch.tensor(float(n_in)) / torch.tensor(float(n_out))) * (o + 0.5) - 0.5
        if defect != "no_index_clamp":
            src = src.clamp_min(0.0)
    i0 = torch.trunc(src).to(torch.int64).clamp_max(n_in - 1)
    lam = src - i0.to(torch.float32)
    i1 = i0 + 1 if defect == "neighbour_past_edge" else i0 + (i0 < n_in - 1).to(torch.int64)
    assert src.dtype == lam.dtype == torch.float32
    return i0, i1, lam


def _stencil(Hin, Win, Ho, Wo, defect, dtype):
    """Flat table rows of the four neighbours of every output cell and their weights' factors (hy, ly, hx, lx) as [cells, 1] columns."""
    y0, y1, ly = _source_index(Hin, Ho, defect)
    x0, x1, lx = _source_index(Win, Wo, defect)
    hy, hx = 1.0 - ly, 1.0 - lx        # float32, as the kernel forms them

    def flat(y, x):
        return (y[:, None] * Win + x[None, :]).clamp_max(Hin * Win - 1).reshape(-1)

    def col(v, axis):
        return (v[:, None].expand(Ho, Wo) if axis == 0 else v[None, :].expand(Ho, Wo)).reshape(-1, 1).to(dtype)

    return (flat(y0, x0), flat(y0, x1), flat(y1, x0), flat(y1, x1)), (col(hy, 0), col(ly, 0), col(hx, 1), col(lx, 1))


def pe_interp(table, Ho, Wo, dtype=torch.float64, defect=None):
    """table (Hin, Win, E) -> (Ho * Wo, E); the blend h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11) in `dtype`."""
    Hin, Win, E = table.shape
    (f00, f01, f10, f11), (hy, ly, hx, lx) = _stencil(Hin, Win, Ho, Wo, defect, dtype)
    t = table.to(dtype).reshape(Hin * Win, E)
    out = hy * (hx * t[f00] + lx * t[f01]) + ly * (hx * t[f10] + lx * t[f11])
    if defect == "drop_last_row":
        out[ROWS_PER_BLOCK - 1::ROWS_PER_BLOCK] = POISON
    return out


def pe_interp_bwd(dout, Ho, Wo, table_shape, dtype=torch.float64, defect=None):
    """The transpose: dtable (Hin, Win, E) of dout (Ho * Wo, E), cell after cell into a zeroed table."""
    Hin, Win, E = table_shape
    (f00, f01, f10, f11), (hy, ly, hx, lx) = _stencil(Hin, Win, Ho, Wo, defect, dtype)
    g = dout.to(dtype).clone()
    if defect == "drop_last_row":
        g[ROWS_PER_BLOCK - 1::ROWS_PER_BLOCK] = 0
    dt = torch.zeros(Hin * Win, E, dtype=dtype)
    for f, wgt in ((f00, hy * hx), (f01, hy * lx), (f10, ly * hx), (f11, ly * lx)):
        dt.index_add_(0, f, wgt * g)
    return dt.view(Hin, Win, E)


def one_cell(dout, c):
    """dout with every cell but c zeroed."""
    out = torch.zeros_like(dout)
    out[c] = dout[c]
    return out


def pe_inputs(Hin, Win, E, Ho, Wo, seed, integers):
    """(table, dout): exact integers in [-8, 8] or randn."""
    if integers:
        return int_tensor((Hin, Win, E), seed), int_tensor((Ho * Wo, E), seed + 1)
    g = torch.Generator().manual_seed(seed)
    return torch.randn(Hin, Win, E, generator=g), torch.randn(Ho * Wo, E, generator=g)
