"""Plain references for the training row kernels of `acai_omr_amd/csrc/train.hip` (LayerNorm backward, column sums, row scatter-add, the MAE
and cross-entropy losses, GELU, AdamW), the probe inputs the tests feed them, and the launch geometry those inputs are built around.

Every formula is written out by hand and evaluated in the dtype that is asked for: float64 gives the reference the GPU tests compare
against, float32 the "plain evaluation" whose own error shows how much of a bar a correct fp32 kernel may use up.

Sums that leave a kernel through float atomics arrive in any order.  On random data the bar that tolerates this is wider than one lost row
out of thousands, so two input families make the bar independent of the row count:

  exact integers   values in [-8, 8] (bf16 holds them exactly); with at most 8208 rows every partial sum stays below 2^24, so every summation
                   order gives the same fp32 result and the comparison is `torch.equal`.
  one loud row     dy (or the loss mask) is zero except in row r, so every other row adds exact zeros to every accumulator, and r walks the
                   edges of the launch geometry (`loud_rows`).

The references can be broken on purpose (`defect=`, as tests/attn_probe.py does for attention): tests/test_row_reference_cpu.py holds every
defect to at least four times the bar of the case that is meant to catch it.

  "drop_last_row"     the last row of every row chunk (and the last row of all) is left out of the sums over rows
  "double_first_row"  the first row of every row chunk is counted twice
  "biased_var"        MAE target normalisation with the biased variance (/ D instead of / (D - 1))
  "eps_outside_sqrt"  1 / (sqrt(var) + eps) instead of 1 / sqrt(var + eps)
  "no_smoothing_grad" the label-smoothing term - eps / V left out of dlogits
  "shared_bias_corr"  AdamW: every parameter uses the bias corrections of the first one

Everything is CPU torch."""
import math

import torch

EPS32 = 2.0 ** -23
DEFECTS = ("drop_last_row", "double_first_row", "biased_var", "eps_outside_sqrt", "no_smoothing_grad", "shared_bias_corr")
INT_ROWS_MAX = 8208     # the largest row count of an exact-integer case: |partial sum| <= 8208 * 8 + 8 < 2^24


def cdiv(a, b):
    return (a + b - 1) // b


# ---- launch geometry (restated from the dispatch code of train.hip: the probes sit on its edges) -------------------------------------------
def ln_fused_dim(dim):
    return dim % 256 == 0 and dim <= 1024


def ln_rows_per_block(rows, dim, aligned=True):
    """Rows per workgroup of the kernel that forms dw / db: the fused form's chunk (whole groups of four rows, ~2048 workgroups) or the 2048-row
    chunk of the generic parameter-gradient kernel."""
    if ln_fused_dim(dim) and aligned:
        return max(4, cdiv(cdiv(rows, 2048), 4) * 4)
    return 2048


def colsum_vec(cols, ld, elem_size, aligned=True):
    epc = 16 // elem_size
    return cols % epc == 0 and ld % epc == 0 and aligned


def colsum_rows_per_block(rows, cols, ld, elem_size, aligned=True):
    if colsum_vec(cols, ld, elem_size, aligned):
        gx = cdiv(cols, 64 * (16 // elem_size))
        return max(64, cdiv(cdiv(rows, max(1, 2048 // gx)), 16) * 16)
    return 2048


def mae_rows_per_wave(rows):
    return 16 if rows >= 65536 else (4 if rows >= 4096 else 1)


def loud_rows(rows, rpb):
    """The rows at the edges of the launch geometry: first, the last wave of the first group of four, the first row of the second group, both
    sides of the first workgroup's end, the last row."""
    return sorted({r for r in (0, 3, 4, rpb - 1, rpb, rows - 1) if 0 <= r < rows})


def row_weights(rows, chunk, defect, dtype=torch.float64):
    """How often each row enters a sum over rows: 1, unless a defect says otherwise."""
    w = torch.ones(rows, dtype=dtype)
    if defect == "drop_last_row":
        w[chunk - 1::chunk] = 0
        w[rows - 1] = 0
    elif defect == "double_first_row":
        w[0::chunk] = 2
    return w


# ---- probe inputs ----------------------------------------------------------------------------------------------------------------------------
def int_tensor(shape, seed):
    """Integers in [-8, 8] as float32."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, tuple(shape), generator=g).float()


def ln_inputs(rows, dim, seed):
    """x = randn * 2 + 0.5; w, b, dy = randn (the inputs of the project's LayerNorm backward tests)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, dim, generator=g) * 2 + 0.5
    return x, torch.randn(dim, generator=g), torch.randn(dim, generator=g), torch.randn(rows, dim, generator=g)


def one_row(dy, r):
    """dy with every row but r zeroed."""
    out = torch.zeros_like(dy)
    out[r] = dy[r]
    return out


MAE_CONST = 0.75        # dyadic: the constant row's mean is exact in fp32, so its deviations are exact zeros
MAE_NEAR = 2.0 ** -10   # the near-constant row's deviations: var ~ 2^-20 ~ 0.95e-6, the size of the 1e-6 it is added to


def mae_inputs(rows, dim, seed):
    """pred = randn, target = randn * 3 + 1.  Row 1 of the target (when there is one) is constant 0.75: a constant row has deviations of exact
    zero, so it pins that the 1e-6 is there at all (without it 0 * inf = NaN) but not where it sits.  Row 2 (when there is one) is 0.75 +- 2^-10
    in alternation, with the odd element out left at 0.75: sum, mean and deviations are exact in fp32 in any summation order, and its variance is
    as large as the 1e-6, so moving the 1e-6 out of the square root changes that row's normalised target by 40 %."""
    g = torch.Generator().manual_seed(seed)
    pred, target = torch.randn(rows, dim, generator=g), torch.randn(rows, dim, generator=g) * 3 + 1
    if rows > 1:
        target[1] = MAE_CONST
    if rows > 2:
        target[2] = MAE_CONST
        half = dim // 2
        target[2, 0:2 * half:2] += MAE_NEAR
        target[2, 1:2 * half:2] -= MAE_NEAR
    return pred, target


def mae_mask(rows, kind, seed=0):
    """"random": 75 % ones with the constant and the near-constant row kept; "ones"; "zeros"; ("onehot", r)."""
    if kind == "ones":
        return torch.ones(rows, dtype=torch.uint8)
    if kind == "zeros":
        return torch.zeros(rows, dtype=torch.uint8)
    if kind == "random":
        g = torch.Generator().manual_seed(seed)
        m = (torch.rand(rows, generator=g) < 0.75).to(torch.uint8)
        m[:3] = 1
        return m
    m = torch.zeros(rows, dtype=torch.uint8)
    m[kind[1]] = 1
    return m


def mae_onehot_rows(rows):
    """Edges of a wave's row chunk and of a workgroup's (4 waves): first and last row of the first wave, first row of the second wave, both
    sides of the first workgroup's end, the last row of all."""
    rpw = mae_rows_per_wave(rows)
    return sorted({r for r in (0, 3, 4, rpw - 1, rpw, 4 * rpw - 1, 4 * rpw, rows - 1) if 0 <= r < rows})


CE_IGNORE_MODES = ("some", "all_but_one", "none")


def ce_inputs(rows, V, scale, shift, ignore_mode, seed):
    """logits = randn * scale + shift; targets inside [0, V) or equal to ignore_index.  Returns (logits, target, ignore_index, count).
    "some": ignore_index 1, about a third of the rows ignored (at least one row kept); "all_but_one": ignore_index 1, one row kept;
    "none": ignore_index -100."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(rows, V, generator=g) * scale + shift
    target = torch.randint(0, V, (rows,), generator=g)
    if ignore_mode == "none":
        return logits, target, -100, rows
    target[target == 1] = 0                       # kept rows do not carry the ignore index by accident
    keep = int(torch.randint(0, rows, (1,), generator=g))
    if ignore_mode == "some":
        drop = torch.rand(rows, generator=g) < 1.0 / 3.0
    else:
        drop = torch.ones(rows, dtype=torch.bool)
    drop[keep] = False
    target[drop] = 1
    return logits, target, 1, int((~drop).sum())


def scatter_inputs(rows, dim, shared_mode, seed):
    """Integer src [rows, dim], an integer pre-filled table dst, int32 idx.  shared_mode "absent" / "quarter" / "all": the shared row holds none,
    a quarter or all of idx and every other index occurs at most once (the precondition of the shared-row form); "free": indices repeat freely
    over a small table.  Index 0 and the last table row occur wherever the mode leaves room for them.  Returns (src, idx, dst, shared_row)."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(-8, 9, (rows, dim), generator=g).float()
    if shared_mode == "free":
        table = 17
        idx = torch.randint(0, table, (rows,), generator=g)
        idx[0], idx[-1] = table - 1, 0
        shared = -1
    else:
        table = rows + 3
        shared = 1 + int(torch.randint(0, table - 2, (1,), generator=g))     # neither 0 nor the last row: those stay ordinary rows
        rest = [j for j in range(1, table - 1) if j != shared]
        vals = [0, table - 1] + [rest[i] for i in torch.randperm(len(rest), generator=g).tolist()]
        idx = torch.tensor(vals[:rows])
        if shared_mode == "all":
            idx[:] = shared
        elif shared_mode == "quarter":
            idx[rows - max(1, rows // 4):] = shared
        idx = idx[torch.randperm(rows, generator=g)]
    dst = torch.randint(-8, 9, (table, dim), generator=g).float()
    return src, idx.to(torch.int32), dst, shared


def scatter_precondition_ok(idx, shared, table):
    """Every index inside the table; with a shared row, every other index at most once."""
    idx = idx.long()
    if int(idx.min()) < 0 or int(idx.max()) >= table:
        return False
    if shared < 0:
        return True
    other = idx[idx != shared]
    return other.unique().numel() == other.numel()


# ---- LayerNorm backward ------------------------------------------------------------------------------------------------------------------------
def layernorm_bwd(x, w, dy, eps, chunk=None, defect=None, dtype=torch.float64):
    """(dx, dw, db) of y = (x - mean) / sqrt(var + eps) * w + b for the upstream gradient dy; var is the biased variance over the row."""
    x, w, dy = x.to(dtype), w.to(dtype), dy.to(dtype)
    rows, dim = x.shape
    mean = x.sum(1, keepdim=True) / dim
    xc = x - mean
    var = (xc * xc).sum(1, keepdim=True) / dim
    rstd = 1.0 / (torch.sqrt(var) + eps) if defect == "eps_outside_sqrt" else 1.0 / torch.sqrt(var + eps)
    xhat = xc * rstd
    g = dy * w
    dx = rstd * (g - g.sum(1, keepdim=True) / dim - xhat * ((g * xhat).sum(1, keepdim=True) / dim))
    wt = row_weights(rows, chunk or rows, defect, dtype)[:, None]
    return dx, (wt * dy * xhat).sum(0), (wt * dy).sum(0)


def layernorm_fwd(x, w, b, eps, dtype=torch.float64):
    x = x.to(dtype)
    dim = x.shape[1]
    xc = x - x.sum(1, keepdim=True) / dim
    return xc / torch.sqrt((xc * xc).sum(1, keepdim=True) / dim + eps) * w.to(dtype) + b.to(dtype)


# ---- column sums and row scatter-add -----------------------------------------------------------------------------------------------------------
def colsum(x, out=None, chunk=None, defect=None, dtype=torch.float64):
    x = x.to(dtype)
    s = (row_weights(x.shape[0], chunk or x.shape[0], defect, dtype)[:, None] * x).sum(0)
    return s if out is None else out.to(dtype) + s


def scatter_add_rows(src, idx, dst, chunk=None, defect=None, dtype=torch.float64):
    """dst[idx[r]] += src[r], one row after the other."""
    out, src = dst.to(dtype).clone(), src.to(dtype)
    wt = row_weights(src.shape[0], chunk or src.shape[0], defect, dtype)
    for r, j in enumerate(idx.tolist()):
        out[j] += wt[r] * src[r]
    return out


# ---- MAELoss: masked mean over rows of mean_d (pred - normalised target)^2 -------------------------------------------------------------------
def mae_loss(pred, target, mask, count, chunk=None, defect=None, dtype=torch.float64):
    """(loss, dpred).  The target row is normalised by its mean and its UNBIASED variance, 1e-6 inside the square root."""
    pred, target, m = pred.to(dtype), target.to(dtype), mask.to(dtype)
    rows, dim = pred.shape
    mean = target.sum(1, keepdim=True) / dim
    tc = target - mean
    var = (tc * tc).sum(1, keepdim=True) / (dim if defect == "biased_var" else dim - 1)
    rs = 1.0 / (torch.sqrt(var) + 1e-6) if defect == "eps_outside_sqrt" else 1.0 / torch.sqrt(var + 1e-6)
    d = pred - tc * rs
    wt = row_weights(rows, chunk or rows, defect, dtype)
    loss = (wt * m * ((d * d).sum(1) / dim)).sum() / count
    seen = (wt != 0).to(dtype) if defect == "drop_last_row" else torch.ones(rows, dtype=dtype)     # a dropped row's gradient is not written either
    return loss, 2.0 * d / dim * (m * seen)[:, None] / count


# ---- cross entropy with label smoothing and an ignore index ------------------------------------------------------------------------------------
def log_softmax(logits):
    z = logits - logits.max(1, keepdim=True).values
    return z - torch.log(torch.exp(z).sum(1, keepdim=True))


def ce_loss(logits, target, ignore_index, count, label_smoothing=0.0, defect=None, dtype=torch.float64):
    """(loss, dlogits): row loss (1 - eps) * -log p[t] + eps / V * sum_c -log p[c], summed over the rows with t != ignore_index, over count."""
    lg = logits.to(dtype)
    rows, V = lg.shape
    keep = target != ignore_index
    t = torch.where(keep, target, torch.zeros_like(target))
    lp = log_softmax(lg)
    onehot = torch.zeros(rows, V, dtype=dtype)
    onehot[torch.arange(rows), t] = 1.0
    e = label_smoothing
    row = (1.0 - e) * -(lp * onehot).sum(1) + e * -(lp.sum(1) / V)
    k = keep.to(dtype)
    uni = 0.0 if defect == "no_smoothing_grad" else e / V
    return (row * k).sum() / count, (torch.exp(lp) - (1.0 - e) * onehot - uni) * k[:, None] / count


def ce_bars(logits, ref_loss, count):
    """(loss bar, gradient bar).  lse = m + log(sum exp(x - m)) is rounded to an ulp of |m| and x - lse adds half an ulp more, so p carries a
    relative error of about 2 eps32 |m|; at |logit| ~ 1 the bars are the project's 1e-5 (loss) and 1e-6 (gradient)."""
    mx = float(logits.abs().max())
    return 1e-5 * max(1.0, abs(float(ref_loss))) + 4 * EPS32 * mx, (1e-6 + 2 * EPS32 * mx) / count


# ---- GELU (exact-erf form) ---------------------------------------------------------------------------------------------------------------------
def _phi_cdf(x):
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0))      # erfc, not 1 + erf: the left tail keeps its relative accuracy


def gelu(x, dtype=torch.float64):
    x = x.to(dtype)
    return x * _phi_cdf(x)


def gelu_grad(x, dtype=torch.float64):
    x = x.to(dtype)
    return _phi_cdf(x) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu_points():
    """fp32 probe: 400 001 points on [-20, 20] and the values at the ends of the format the path can meet (no inf, no NaN)."""
    grid = torch.linspace(-20.0, 20.0, 400001, dtype=torch.float64).float()
    edge = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 88.0, -88.0, 1e30, -1e30])
    return torch.cat([grid, edge])


def all_finite_bf16():
    """Every finite bf16 bit pattern (65 280 values)."""
    v = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    return v[torch.isfinite(v.float())]


def bf16_ulp(r):
    """Spacing of bf16 at |r| (r float64 holding bf16 values): 2^(e - 7), e the exponent, not below the smallest normal's."""
    e = torch.floor(torch.log2(r.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 7)


def round_bf16(v):
    """float64 -> the nearest bf16 (through fp32: the double rounding cannot matter at the 1-ulp bars this feeds), as float64."""
    return v.float().to(torch.bfloat16).double()


# What the bf16 GELU bars allow on top of one bf16 ulp of the reference: the absolute 1e-6 of the fp32 forward bar.  Both the polynomial of the
# forward and the 1 + erf of the backward are accurate in absolute, not relative, terms; see test_gelu_bf16_every_input.
GELU_BF16_FLOOR = 1e-6


def gelu_bf16_excess(got, ref):
    """max of |got - round_bf16(ref)| / (one bf16 ulp of it + GELU_BF16_FLOOR): <= 1 passes."""
    rb = round_bf16(ref)
    return float(((got.double() - rb).abs() / (bf16_ulp(rb) + GELU_BF16_FLOOR)).max())


# ---- AdamW ---------------------------------------------------------------------------------------------------------------------------------------
def adamw_run(params, grads, hyper, defect=None, dtype=torch.float64):
    """Decoupled-weight-decay Adam over a schedule.  params: list of tensors; grads: per step, a list with one gradient (or None: the parameter
    sits the step out and its own step count stands still) per parameter; hyper: per parameter, a dict lr / betas / eps / weight_decay.
    Returns (params, exp_avg, exp_avg_sq, steps)."""
    p = [t.to(dtype).clone() for t in params]
    m = [torch.zeros_like(t) for t in p]
    v = [torch.zeros_like(t) for t in p]
    steps = [0] * len(p)
    for gs in grads:
        for i, g in enumerate(gs):
            if g is not None:
                steps[i] += 1
        first = next((i for i, g in enumerate(gs) if g is not None), None)
        for i, g in enumerate(gs):
            if g is None:
                continue
            h = hyper[i]
            b1, b2 = h["betas"]
            g = g.to(dtype)
            k = steps[first] if defect == "shared_bias_corr" else steps[i]
            p[i] = p[i] * (1.0 - h["lr"] * h["weight_decay"])
            m[i] = m[i] + (g - m[i]) * (1.0 - b1)
            v[i] = v[i] * b2 + (1.0 - b2) * g * g
            bc1, bc2 = 1.0 - b1 ** k, 1.0 - b2 ** k
            p[i] = p[i] - (h["lr"] / bc1) * (m[i] / (torch.sqrt(v[i]) / math.sqrt(bc2) + h["eps"]))
    return p, m, v, steps


ADAMW_SIZES = (1, 3, 17, 16383, 16384, 16385, 32769)      # the kernel's chunk is 16384 elements: one short, exact, one over, two chunks and one
ADAMW_STEPS = 6
ADAMW_CASES = ("default", "skip", "lr0", "wd0", "zero_grad", "beta1_0")


def adamw_case(case, seed=11):
    """(params, grads per step, hyper per parameter) of a named case.  "skip": parameter 2 has no gradient on steps 2 and 3 and returns on step
    4; "lr0": the parameters of odd index sit in a group with lr = 0; "wd0": no weight decay; "zero_grad": all gradients zero (pure decay);
    "beta1_0": betas (0.0, 0.9).  The third step's gradients are ten times louder, as in the project's AdamW test."""
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(n, generator=g) for n in ADAMW_SIZES]
    base = dict(lr=3e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05)
    hyper = [dict(base) for _ in params]
    if case == "lr0":
        for i in range(1, len(params), 2):
            hyper[i]["lr"] = 0.0
    elif case == "wd0":
        for h in hyper:
            h["weight_decay"] = 0.0
    elif case == "beta1_0":
        for h in hyper:
            h["betas"] = (0.0, 0.9)
    grads = []
    for it in range(ADAMW_STEPS):
        gs = [torch.randn(n, generator=g) * (10.0 if it == 2 else 1.0) for n in ADAMW_SIZES]
        if case == "zero_grad":
            gs = [torch.zeros(n) for n in ADAMW_SIZES]
        if case == "skip" and it in (1, 2):
            gs[2] = None
        grads.append(gs)
    return params, grads, hyper


def adamw_groups(params, hyper):
    """Optimizer param groups for a case: parameters that share their hyper-parameters share a group, in order of first appearance."""
    groups = []
    for p, h in zip(params, hyper):
        for grp in groups:
            if all(grp[k] == h[k] for k in h):
                grp["params"].append(p)
                break
        else:
            groups.append(dict(h, params=[p]))
    return groups
