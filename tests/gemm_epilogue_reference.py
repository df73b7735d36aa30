"""The float64 model of one `acai_gemm_nt_ex` call: C = epilogue(A . W^T), and the tensor the epilogue keeps beside it.

The epilogue's arithmetic stands in three hand-written copies (gemm_epilogue and gemm_vec_epilogue in csrc/gemm_device.h, gemm_pp_epilogue in
csrc/gemm_pp.hip) that nine kernel forms call.  This module is a fourth statement of it that shares no code with them: plain torch, elementwise,
in float64, on whatever device its inputs live on.  It follows DESIGN.md's contract, quoted here (test_gemm_epilogue_reference_cpu.py asserts that
the two texts are the same):
"""
import collections
import math
import os

import torch

import row_reference as R

CONTRACT = """\
1. v = (acc + bias[col]) * cs          cs = col_scale for col < scale_cols, else 1; bias = 0 without a bias
2. if ROUND_BF16: v = bf16(v)
3. aux_mode 1: aux[row][col] = v       aux_mode 3: aux[row][col] = gelu'(v)      (stored in C's dtype)
4. aux_mode 2: v = v * gelu'(aux[row][col])      aux_mode 4: v = v * aux[row][col]
5. if GELU: v = gelu(v); if ROUND_BF16: v = bf16(v)
6. if residual: v = v + residual[row][col]
7. C[row][col] = v                     (stored in C's dtype: a bf16 C rounds once more)
"""

__doc__ += "\n" + CONTRACT + """
Every single fp32 operation of the device is reproduced exactly: the multiply by cs, the multiply by the aux-4 tensor and the add of the residual
are formed in float64 from fp32 operands (exact: 48 bits), rounded once to fp32 and then to bf16 where the kernel rounds.  gelu and gelu' are
row_reference's float64 forms; what a kernel may differ from them is the bar of the stand-alone GELU kernels (tests/test_gpu_row_kernels.py).

Inputs that make the accumulator exact (`gemm_inputs`): A in multiples of 1/8 on [-1, 1], W in multiples of 1/32 on [-1/8, 1/8] (both bf16
numbers), bias in multiples of 2^-12 inside (-1, 1).  Every product is a multiple of 2^-8, every partial sum of sum_k a w + bias a multiple of 2^-12
below 2^12: an fp32 number in any summation order, so each kernel's accumulator equals float64's bit for bit and the comparison needs no allowance
for "differs here and there".  The fine bias grid is what makes the first rounding matter: without it 70-95 % of the sums are bf16 numbers already.

The model can be broken on purpose (`defect=`, as row_reference.DEFECTS): the CPU test holds every defect to missing the GPU test's bars.

  "scale_after_round"         the column scale is applied after the first bf16 rounding
  "no_pre_round_before_gelu"  step 2 is skipped when a GELU follows
  "no_round_after_gelu"       the rounding of step 5 is skipped
  "residual_before_gelu"      step 6 runs before step 5
  "bias_of_next_column"       bias[col + 1] (wrapping) instead of bias[col]
  "aux_row_stride_off"        aux rows advance by ldc where ldaux belongs
  "scale_cols_off_by_one"     col <= scale_cols is scaled
  "drop_last_k_tile"          the last K-tile is left out of the accumulator
  "gelu_grad_of_output"       aux_mode 3 keeps gelu'(gelu(v)): the derivative taken after the GELU
"""

DEFECTS = ("scale_after_round", "no_pre_round_before_gelu", "no_round_after_gelu", "residual_before_gelu", "bias_of_next_column",
           "aux_row_stride_off", "scale_cols_off_by_one", "drop_last_k_tile", "gelu_grad_of_output")
GELU, ROUND_BF16 = 1, 2      # ACAI_GEMM_GELU, ACAI_GEMM_ROUND_BF16
QSCALE64 = math.log2(math.e) / 8.0      # ops.QSCALE(64), restated so that the CPU test needs no device module


def design_contract():
    """The contract as DESIGN.md states it (the text between its two marks, without the code fence)."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "DESIGN.md")) as f:
        text = f.read()
    body = text.split("<!-- gemm-epilogue-contract -->")[1].split("<!-- /gemm-epilogue-contract -->")[0]
    return "".join(line + "\n" for line in body.strip().splitlines() if not line.startswith("```"))


# ---- number formats ------------------------------------------------------------------------------------------------------------------------------
def f32(v):
    """float64 -> the nearest fp32 (RNE), as float64."""
    return v.float().double()


def ulp32(r):
    """Spacing of fp32 at |r|."""
    return torch.exp2(torch.floor(torch.log2(r.abs().clamp_min(2.0 ** -126))) - 23)


def is_bf16(v):
    return bool((R.round_bf16(v.double()) == v.double()).all())


def store(v, out):
    return R.round_bf16(v) if out == "bf16" else f32(v)


# ---- the forms of a call and the input sets the GPU test runs ------------------------------------------------------------------------------------
# out: dtype of C and of the aux tensor; aux: aux_mode; views: C and aux are column views of wider buffers
Form = collections.namedtuple("Form", "name out bias round gelu aux res scale views")


def _form(base, out, rnd, bias=True, gelu=False, aux=0, res=False, scale=False, views=False):
    return Form(f"{base}_{out}" + ("_r" if rnd else ""), out, bias, rnd, gelu, aux, res, scale, views)


def forms(dtype):
    """The forms of an input dtype, in the order the GPU test runs them."""
    if dtype == "bf16":
        return [_form("plain", "bf16", True), _form("plain", "f32", False), _form("nobias", "f32", False, bias=False),
                _form("res", "f32", True, res=True), _form("gelu_res", "f32", True, gelu=True, res=True),
                _form("gelu_aux1", "bf16", True, gelu=True, aux=1), _form("gelu_aux1", "f32", True, gelu=True, aux=1),
                _form("aux2", "bf16", True, aux=2), _form("gelu_aux3", "bf16", True, gelu=True, aux=3), _form("aux4", "bf16", True, aux=4),
                _form("scale", "bf16", True, scale=True), _form("scale", "f32", False, scale=True),
                _form("views_aux4", "bf16", True, aux=4, views=True), _form("views_gelu_aux1", "bf16", True, gelu=True, aux=1, views=True),
                _form("aux4_res", "f32", True, aux=4, res=True)]
    out = []
    for rnd in (False, True):
        out += [_form("plain", "f32", rnd), _form("nobias", "f32", rnd, bias=False), _form("res", "f32", rnd, res=True),
                _form("gelu_res", "f32", rnd, gelu=True, res=True), _form("gelu_aux1", "f32", rnd, gelu=True, aux=1), _form("aux2", "f32", rnd, aux=2),
                _form("gelu_aux3", "f32", rnd, gelu=True, aux=3), _form("aux4", "f32", rnd, aux=4), _form("scale", "f32", rnd, scale=True),
                _form("views_aux4", "f32", rnd, aux=4, views=True), _form("views_gelu_aux1", "f32", rnd, gelu=True, aux=1, views=True)]
    return out + [_form("gelu_aux1", "bf16", True, gelu=True, aux=1)]


def form_named(dtype, name):
    return next(f for f in forms(dtype) if f.name == name)


SPLIT_FORMS = ("plain_bf16_r", "res_f32_r", "gelu_aux3_bf16_r", "aux4_bf16_r", "scale_bf16_r")       # the auto rule's two-launch shape
SPLIT_SHAPE = (8208, 2048, 64)


def persistent_forms(dtype):
    """The forms of the shape with more tiles than CUs: plain, residual, GELU + aux 3, aux 4."""
    names = SPLIT_FORMS[:4] if dtype == "bf16" else ("plain_f32", "res_f32_r", "gelu_aux3_f32_r", "aux4_f32_r")
    return [form_named(dtype, n) for n in names]


def persistent_rows(n_cu):
    """Rows of the persistent kernels' second shape (N = 536: three column tiles of 256, five of 128): more tiles than CUs, a ragged last one."""
    return (n_cu // 3 + 1) * 256 + 5


def ktile(dtype):
    return 64 if dtype == "bf16" else 32     # a K-tile is 128 bytes


def small_input_sets(dtype):
    """(M, N, K) of every test of the pinned kernels and of the register-staged kernel."""
    kt = ktile(dtype)
    return [(1797, n, k) for n in (264, 262) for k in (kt, 3 * kt)] + [(300, 130, 72), (37, 19, 10)]


def scale_cols(N):
    n = N // 3
    return n + 1 if n % 4 == 0 else n       # never a multiple of 4: the boundary falls inside a lane's four (eight) columns


PATHS = ("vec", "n262", "ldc", "c_off8", "ldr", "ldaux")      # the LDS-transposed epilogue, and each single cause of the scalar one


def geometry(form, path, N):
    """Where C, the aux tensor and the residual sit inside their buffers: per tensor (first column, row stride), in elements.  Every buffer is
    wider than N and one row above and two rows below the tensor belong to it too (sentinels).  By default everything allows 16-byte row
    accesses (N % 8 == 0 given) and the three strides differ; a path breaks exactly one condition."""
    esz = 2 if form.out == "bf16" else 4
    wN = R.cdiv(N, 8) * 8
    c, x, r = [0, wN + 8], [0, wN + 16], [0, wN + 4]
    if form.views:
        c, x = [8, wN + 40], [8, wN + 24]
    if path == "ldc":
        c[1] = wN + 9
    elif path == "c_off8":
        c[0] += 8 // esz
    elif path == "ldr":
        r[1] = wN + 6
    elif path == "ldaux":
        x[1] = wN + 9
    return dict(c=tuple(c), aux=tuple(x), res=tuple(r))


def path_forms(dtype, path):
    """The forms a path runs: a residual / aux stride can only matter to the forms that have one."""
    fs = forms(dtype)
    return [f for f in fs if (path != "ldr" or f.res) and (path != "ldaux" or f.aux)]


# ---- which kernel a cell must run (restated from the issue of the kernels, not read from the planner) -------------------------------------------
PINNED = {"v1": "gemm_nt_glds_kernel<wm=2>", "v2": "gemm_nt_glds_kernel<wm=4>", "v3": "gemm_nt_glds3_kernel", "v4": "gemm_nt_pers_kernel",
          "v5": "gemm_nt_256_kernel", "v6": "gemm_nt_pers256_kernel"}
PERSISTENT = ("v4", "v6", "v7")
# the register-staged kernel: its 16-byte chunk loads (fast = 1) need K % 8 == 0 (bf16; fp32: % 4), such row strides and aligned operands
REG_KERNELS = {"reg_fast1": "gemm_nt_kernel<fast=1>", "reg_fast0_lda": "gemm_nt_kernel<fast=0>", "reg_fast0_k10": "gemm_nt_kernel<fast=0>",
               "reg_fast0_off1": "gemm_nt_kernel<fast=0>"}
PP_OBF, PP_GELU, PP_AUX1, PP_AUX2, PP_RES, PP_SCALE, PP_AUX3, PP_AUX4 = 1, 2, 4, 8, 16, 32, 128, 256      # ACAI_PP_*


def pp_mode(form):
    return ((PP_OBF if form.out == "bf16" else 0) | (PP_GELU if form.gelu else 0) | {0: 0, 1: PP_AUX1, 2: PP_AUX2, 3: PP_AUX3, 4: PP_AUX4}[form.aux] |
            (PP_RES if form.res else 0) | (PP_SCALE if form.scale else 0))


# the forms gemm_nt_pp_kernel is instantiated for; every other form, and every launch of the scalar epilogue, keeps the persistent 256x256 ring
PP_MODES = (0, PP_OBF, PP_RES, PP_OBF | PP_SCALE, PP_OBF | PP_GELU | PP_AUX1, PP_OBF | PP_AUX2, PP_OBF | PP_GELU | PP_AUX3, PP_OBF | PP_AUX4)


def kernels_of(dtype):
    """The kernels an input dtype runs on: fp32 has no persistent 256x256 ring and no ping-pong ring (6 and 7 fall back to 5)."""
    return [f"v{i}" for i in range(1, 8 if dtype == "bf16" else 6)] + list(REG_KERNELS)


def expected_kernel(kern, form, vec):
    if kern in REG_KERNELS:
        return REG_KERNELS[kern]
    if kern == "v7":
        return f"gemm_nt_pp_kernel<mode={pp_mode(form)}>" if vec and pp_mode(form) in PP_MODES else PINNED["v6"]
    return PINNED[kern]


def expected_vec(form, N, ptr_c, ldc, ptr_aux, ldaux, ptr_res, ldr):
    """Whether a call allows the LDS-transposed epilogue: 16-byte accesses along the rows of C, of the aux tensor and of the residual."""
    return int(N % 8 == 0 and ldc % 8 == 0 and ptr_c % 16 == 0 and (not form.res or (ldr % 4 == 0 and ptr_res % 16 == 0)) and
               (not form.aux or (ldaux % 8 == 0 and ptr_aux % 16 == 0)))


def gemm_inputs(M, N, K):
    """a [M, K], w [N, K], bias [N], res [M, N], saved [M, N] as fp32 on the CPU (a and w are bf16 numbers); res and saved are random normals
    (the fp32 residual, and the aux tensor of modes 2 / 4, used as it stands for an fp32 C and rounded to bf16 for a bf16 C)."""
    g = torch.Generator().manual_seed(M * 1000003 + N * 1009 + K)
    a = torch.randint(-8, 9, (M, K), generator=g).float() / 8
    w = torch.randint(-4, 5, (N, K), generator=g).float() / 32
    bias = torch.randint(-4095, 4096, (N,), generator=g).float() / 4096
    res = torch.randn(M, N, generator=g)
    saved = torch.randn(M, N, generator=g)
    return dict(a=a, w=w, bias=bias, res=res, saved=saved)


def exact_span(a, w, bias):
    """max over outputs of sum_k |a||w| + |bias|: below 2^12 every partial sum, a multiple of 2^-12, is an fp32 number."""
    return float((a.abs().double() @ w.abs().double().t() + bias.abs().double()).max())


def first_rounding_share(acc, bias):
    v = f32(acc + bias.double())
    return float((R.round_bf16(v) != v).double().mean())


def accumulator(a, w, dtype="bf16", defect=None):
    """sum_k a w in float64."""
    K = a.shape[1]
    if defect == "drop_last_k_tile":
        K = (R.cdiv(K, ktile(dtype)) - 1) * ktile(dtype)
    return a[:, :K].double() @ w[:, :K].double().t()


# ---- the model -----------------------------------------------------------------------------------------------------------------------------------
# c / kept: what the call stores (float64 holding numbers of the out dtype); c_kind / kept_kind: which bar holds them; g: the float64 value of the
# GELU-bearing term before any rounding after it (gelu(v), v gelu'(aux), gelu'(v) for kept); res: the residual added after it
Model = collections.namedtuple("Model", "c kept c_kind kept_kind g kept_g res out round")


def _misplaced_read(aux, ldc):
    """aux[row][col] read with rows ldc apart (inside the buffer aux is a view of)."""
    base = aux._base if aux._base is not None else aux
    flat = base.reshape(-1)
    M, N = aux.shape
    rows = torch.arange(M, device=aux.device)[:, None]
    cols = torch.arange(N, device=aux.device)[None, :]
    return flat[(aux.storage_offset() - base.storage_offset() + rows * ldc + cols) % flat.numel()]


def _misplaced_write(keep, ldc, ldaux):
    """What a view with rows ldaux apart shows of values written with rows ldc apart (NaN where nothing landed)."""
    M, N = keep.shape
    rows = torch.arange(M, device=keep.device)[:, None]
    cols = torch.arange(N, device=keep.device)[None, :]
    img = torch.full((M * max(ldc, ldaux) + N,), float("nan"), dtype=keep.dtype, device=keep.device)
    img[(rows * ldc + cols).reshape(-1)] = keep.reshape(-1)
    return img[rows * ldaux + cols]


def model(a, w, bias, flags, out, aux_mode=0, aux=None, residual=None, col_scale=None, acc=None, defect=None, dtype="bf16", ldc=None, ldaux=None):
    """One call.  a [M, K], w [N, K]; bias [N] fp32 or None; flags GELU | ROUND_BF16; out "bf16" / "f32"; aux: the [M, N] tensor of aux modes
    2 / 4 in C's dtype; residual [M, N] fp32 or None; col_scale (scale_cols, s) or None; acc: the float64 product if the caller has it already."""
    assert defect is None or defect in DEFECTS, defect
    do_gelu, do_round = bool(flags & GELU), bool(flags & ROUND_BF16)
    assert (aux_mode in (1, 3)) == (do_gelu and aux_mode != 0) and not (aux_mode in (2, 4) and do_gelu)
    if acc is None or defect == "drop_last_k_tile":
        acc = accumulator(a, w, dtype, defect).to(a.device)
    M, N = acc.shape
    dev = acc.device
    b = torch.zeros(N, dtype=torch.float64, device=dev) if bias is None else bias.double()
    if defect == "bias_of_next_column":
        b = torch.roll(b, -1)
    cs = torch.ones(N, dtype=torch.float64, device=dev)
    if col_scale is not None:
        n, s = col_scale
        cs[:n + (1 if defect == "scale_cols_off_by_one" else 0)] = float(torch.tensor(s, dtype=torch.float32))
    rnd1 = do_round and not (defect == "no_pre_round_before_gelu" and do_gelu)
    # 1, 2
    v = f32(acc + b)
    if defect == "scale_after_round":
        v = f32((R.round_bf16(v) if rnd1 else v) * cs)
    else:
        v = f32(v * cs)
        if rnd1:
            v = R.round_bf16(v)
    # 3
    kept = kept_kind = kept_g = None
    if aux_mode == 1:
        kept, kept_kind = store(v, out), "exact"
    elif aux_mode == 3:
        kept_g = R.gelu_grad(R.gelu(v)) if defect == "gelu_grad_of_output" else R.gelu_grad(v)
        kept, kept_kind = store(kept_g, out), "dgelu_bf16" if out == "bf16" else "dgelu32"
    if kept is not None and defect == "aux_row_stride_off":
        kept = _misplaced_write(kept, ldc, ldaux)
    # 4
    c_kind, g = "exact", None
    if aux_mode in (2, 4):
        x = (_misplaced_read(aux, ldc) if defect == "aux_row_stride_off" else aux).double()
        if aux_mode == 2:
            assert residual is None
            g = v * R.gelu_grad(x)
            v, c_kind = g, "dgelu_bf16" if out == "bf16" else "dgelu32"
        else:
            v = f32(v * x)
            if residual is not None:
                c_kind = "ulp32"       # the multiply and the add may be one fused operation
    r = None if residual is None else residual.double()
    if r is not None and defect == "residual_before_gelu":
        v = f32(v + r)
    # 5
    if do_gelu:
        g = R.gelu(v)
        v = R.round_bf16(g) if do_round and defect != "no_round_after_gelu" else g
        c_kind = "gelu_res" if r is not None else ("gelu_bf16" if do_round or out == "bf16" else "gelu32")
    # 6
    if r is not None and defect != "residual_before_gelu":
        v = f32(v + r)
    # 7
    return Model(store(v, out), kept, c_kind, kept_kind, g, kept_g, r, out, do_round)


# ---- the bars -------------------------------------------------------------------------------------------------------------------------------------
def _ratio(err, bar):
    q = err / bar
    return float("inf") if bool(torch.isnan(q).any()) else float(q.max())


def _excess(kind, got, want, g, m):
    got = got.double()
    if kind == "exact":                 # no GELU, no gelu': every operation is modelled bit for bit
        return 0.0 if torch.equal(got, want) else float("inf")
    if kind == "ulp32":                 # aux 4 + residual: one fp32 ulp of the result
        return _ratio((got - want).abs(), ulp32(want))
    if kind == "gelu32":                # test_gelu_fp32's forward bar
        return _ratio((got - g).abs(), 1e-6 + 2 * R.EPS32 * g.abs())
    if kind == "dgelu32":               # test_gelu_fp32's backward bar (aux 2: dh = v)
        return _ratio((got - g).abs(), 1e-5 + 1e-6 * g.abs())
    if kind in ("gelu_bf16", "dgelu_bf16"):     # test_gelu_bf16_every_input's bar, and the result is a bf16 number
        if torch.isnan(got).any() or not is_bf16(got):
            return float("inf")
        return R.gelu_bf16_excess(got, g)
    assert kind == "gelu_res"           # the GELU's bar plus one fp32 ulp of the sum
    if m.round:
        rb = R.round_bf16(g)
        target, bar = rb + m.res, R.bf16_ulp(rb) + R.GELU_BF16_FLOOR
    else:
        target, bar = g + m.res, 1e-6 + 2 * R.EPS32 * g.abs()
    return _ratio((got - target).abs(), bar + ulp32(target))


def excess(m, got_c, got_kept=None):
    """The largest error of C and of the kept tensor as a fraction of their bars: (C, aux), <= 1 passes; 0 / inf for the bit-equal kinds."""
    ec = _excess(m.c_kind, got_c, m.c, m.g, m)
    ek = 0.0 if m.kept is None else _excess(m.kept_kind, got_kept, m.kept, m.kept_g, m)
    return ec, ek


def form_call(form, inp, N):
    """The model's arguments of a form on an input set: (bias, flags, aux tensor of modes 2 / 4, residual, col_scale)."""
    flags = (GELU if form.gelu else 0) | (ROUND_BF16 if form.round else 0)
    aux = None
    if form.aux in (2, 4):
        aux = inp["saved"].bfloat16().float() if form.out == "bf16" else inp["saved"]
    return (inp["bias"] if form.bias else None, flags, aux, inp["res"] if form.res else None, (scale_cols(N), QSCALE64) if form.scale else None)
