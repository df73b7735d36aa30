"""Every epilogue form of `acai_gemm_nt_ex` on every GEMM kernel against the float64 model of tests/gemm_epilogue_reference.py.

The epilogue's arithmetic exists in three hand-written copies (scalar, LDS-transposed, register) behind nine kernel forms; the other GEMM tests
compare them with each other.  Here each kernel is pinned (or reached through the shape that selects it), each call asserts the kernel that ran
and the epilogue path the plan chose, and the result is held to DESIGN.md's contract:

  * The inputs make every accumulator exact in fp32 in any summation order (test_gemm_epilogue_reference_cpu.py), so the forms without GELU or
    gelu' - plain, no bias, column scale, residual, aux 4, the kept pre-activation of aux 1, strided outputs - must equal the model BIT FOR BIT.
    aux 4 + residual alone may fuse its multiply and add: one fp32 ulp.
  * The GELU argument is then known bit for bit, so the GELU forms take the bars of the stand-alone GELU kernels (test_gpu_row_kernels.py):
    1e-6 + 2 eps32 |ref| in unrounded fp32; a bf16 number within one bf16 ulp (+ 1e-6) of the rounded reference where the result is rounded;
    1e-5 + 1e-6 |ref| (fp32) or the bf16 bar for gelu' kept by aux 3 and for the product of aux 2; GELU + residual: the GELU's bar plus one fp32
    ulp of the sum.  No share of the elements is exempt.
  * C and the aux tensor are views inside larger buffers filled with a sentinel: nothing outside [M, N] may change.

Each test prints the largest error of every form as a fraction of its bar (0 for the bit-equal forms)."""
import pytest
import torch

import gemm_epilogue_reference as E
import row_reference as R

pytestmark = pytest.mark.gpu

SENTINEL = -768.0       # a bf16 number no result comes near
AUX_KW = {1: "pre_act", 2: "gelu_grad_of", 3: "gelu_grad_out", 4: "times"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from acai_omr_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


_INPUTS = {}


def _inputs(dev, dtype, M, N, K, keep=True):
    """The input set on the device: the fp32 tensors of gemm_inputs, the operands in the kernel's dtype and the float64 product (torch's own
    matmul: independent of these kernels, and exact on these inputs in any order)."""
    key = (dtype, M, N, K)
    if key in _INPUTS:
        return _INPUTS[key]
    d = {k: v.to(dev) for k, v in E.gemm_inputs(M, N, K).items()}
    dt = torch.bfloat16 if dtype == "bf16" else torch.float32
    d["a_in"], d["w_in"] = d["a"].to(dt), d["w"].to(dt)
    d["acc"] = d["a"].double() @ d["w"].double().t()
    assert E.exact_span(d["a"], d["w"], d["bias"]) < 2.0 ** 12
    if keep:
        _INPUTS[key] = d
    return d


def _buffer(dev, M, c0, ld, N, dt, fill=None):
    """A [M + 3, ld] buffer of sentinels and the [M, N] tensor inside it: one row down, c0 columns in."""
    buf = torch.full((M + 3, ld), SENTINEL, dtype=dt, device=dev)
    view = buf[1:M + 1, c0:c0 + N]
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _untouched(buf, M, c0, N):
    chk = buf.clone()
    chk[1:M + 1, c0:c0 + N] = SENTINEL
    return bool((chk == SENTINEL).all())


def _call(dev, dtype, form, path, d, M, N, a_in=None):
    """One call of a form.  Returns (largest error over its bars, kernels that ran, vec_epi of each launch, the vec_epi the call allows)."""
    from acai_omr_amd import _lib, ops
    assert float(torch.tensor(ops.QSCALE(64), dtype=torch.float32)) == float(torch.tensor(E.QSCALE64, dtype=torch.float32))
    geo = E.geometry(form, path, N)
    odt = torch.bfloat16 if form.out == "bf16" else torch.float32
    bias, flags, aux, res, scale = E.form_call(form, d, N)
    cbuf, c = _buffer(dev, M, *geo["c"], N, odt)
    xbuf = x = rbuf = r = None
    if form.aux:
        xbuf, x = _buffer(dev, M, *geo["aux"], N, odt, fill=aux)
    if form.res:
        rbuf, r = _buffer(dev, M, *geo["res"], N, torch.float32, fill=res)
    kw = {AUX_KW[form.aux]: x} if form.aux else {}
    ops.gemm_nt(d["a_in"] if a_in is None else a_in, d["w_in"], bias, residual=r, out=c, gelu=form.gelu, round_bf16=form.round, col_scale=scale, **kw)
    names, vecs = _lib.gemm_last_kernels(), [l.vec_epi for l in _lib.gemm_last_plan()]
    vec = E.expected_vec(form, N, c.data_ptr(), c.stride(0), x.data_ptr() if form.aux else 0, x.stride(0) if form.aux else 0,
                         r.data_ptr() if form.res else 0, r.stride(0) if form.res else 0)
    m = E.model(d["a"], d["w"], bias, flags, form.out, form.aux, aux, res, scale, acc=d["acc"], dtype=dtype)
    ec, ek = E.excess(m, c, x if form.aux in (1, 3) else None)
    assert _untouched(cbuf, M, geo["c"][0], N), (form.name, "C written outside [M, N]")
    if form.aux:
        assert _untouched(xbuf, M, geo["aux"][0], N), (form.name, "aux written outside [M, N]")
        if form.aux in (2, 4):
            assert torch.equal(x, aux.to(odt)), (form.name, "the aux operand was written")
    if form.res:
        assert torch.equal(r, res) and _untouched(rbuf, M, geo["res"][0], N), (form.name, "the residual was written")
    return max(ec, ek), names, vecs, vec


def _report(tag, worst):
    print(f"{tag}: " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (tag, bad)


def _pinned(kern):
    from acai_omr_amd import _lib
    _lib.check(_lib.lib().acai_gemm_set_variant(int(kern[1])), "acai_gemm_set_variant")


def _unpin():
    from acai_omr_amd import _lib
    _lib.lib().acai_gemm_set_variant(0)


PINNED_CELLS = [(k, dt, p) for dt in ("bf16", "fp32") for k in E.kernels_of(dt) if k not in E.REG_KERNELS for p in E.PATHS]


@pytest.mark.parametrize("kern,dtype,path", PINNED_CELLS)
def test_pinned_kernel_epilogues(dev, kern, dtype, path):
    """Variants 1-7 (fp32: 1-5), 1797 x 264 (seven tiles of 256 rows and five rows; a ragged last column tile) at one and at three K-tiles.
    path "vec": everything allows 16-byte row accesses, the LDS-transposed epilogue (7: the register epilogue in the forms it has).  The other
    paths each break ONE condition - N = 262, ldc % 8 != 0, C eight bytes in, ldr % 4 != 0, ldaux % 8 != 0 - and must run the scalar epilogue
    (7: on the persistent 256x256 ring) in the forms the condition concerns."""
    M, N, kt = 1797, 262 if path == "n262" else 264, E.ktile(dtype)
    worst = {}
    _pinned(kern)
    try:
        for K in (kt, 3 * kt):
            d = _inputs(dev, dtype, M, N, K)
            for form in E.path_forms(dtype, path):
                err, names, vecs, vec = _call(dev, dtype, form, path, d, M, N)
                assert names == [E.expected_kernel(kern, form, vec)] and vecs == [vec], (form.name, K, names, vecs, vec)
                concerned = path in ("n262", "ldc", "c_off8") or (path == "ldr" and form.res) or (path == "ldaux" and bool(form.aux))
                assert vec == (0 if concerned else 1), (form.name, path, vec)
                worst[form.name] = max(worst.get(form.name, 0.0), err)
    finally:
        _unpin()
    _report(f"{kern} {dtype} {path}", worst)


@pytest.mark.parametrize("kern,dtype", [(k, dt) for dt in ("bf16", "fp32") for k in E.REG_KERNELS])
def test_register_staged_kernel_epilogues(dev, kern, dtype):
    """gemm_nt_kernel: <fast=1> at K = 72 (no whole K-tiles, whole 16-byte chunks); <fast=0> through an odd lda, through K = 10 and through
    an A that starts one element into its buffer.  Its epilogue is the scalar one at every shape."""
    M, N, K = (37, 19, 10) if kern == "reg_fast0_k10" else (300, 130, 72)
    d = _inputs(dev, dtype, M, N, K)
    a_in = d["a_in"]
    if kern == "reg_fast0_lda":
        a_in = torch.zeros(M, K + 1, dtype=a_in.dtype, device=dev)[:, :K].copy_(d["a_in"])
    elif kern == "reg_fast0_off1":
        a_in = torch.zeros(M, K + 8, dtype=a_in.dtype, device=dev)[:, 1:K + 1].copy_(d["a_in"])
    worst = {}
    for form in E.forms(dtype):
        err, names, vecs, vec = _call(dev, dtype, form, "vec", d, M, N, a_in=a_in)
        assert names == [E.expected_kernel(kern, form, vec)] and vecs == [vec] and vec == 0, (form.name, names, vecs, vec)
        worst[form.name] = err
    _report(f"{kern} {dtype}", worst)


@pytest.mark.parametrize("kern,dtype", [("v4", "bf16"), ("v6", "bf16"), ("v7", "bf16"), ("v4", "fp32")])
def test_persistent_kernels_second_round(dev, kern, dtype):
    """pers, pers256 and pp with more tiles than the device has CUs (N = 536, one K-tile): a workgroup runs a second tile, the last row of tiles
    and the last column of tiles are ragged."""
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    M, N, K = E.persistent_rows(n_cu), 536, E.ktile(dtype)
    assert R.cdiv(M, 256) * R.cdiv(N, 256) > n_cu
    d = _inputs(dev, dtype, M, N, K, keep=False)
    worst = {}
    _pinned(kern)
    try:
        for form in E.persistent_forms(dtype):
            err, names, vecs, vec = _call(dev, dtype, form, "vec", d, M, N)
            assert names == [E.expected_kernel(kern, form, vec)] and vecs == [1] and vec == 1, (form.name, names, vecs, vec)
            worst[form.name] = err
    finally:
        _unpin()
    _report(f"{kern} {dtype} second round, {M} rows", worst)


def test_auto_rule_remainder_rows(dev):
    """8208 x 2048 x 64 under the auto rule: on 256 CUs the ping-pong ring over 8192 rows and the 128x128 two-stage kernel over the last 16, whose
    C, residual and aux pointers are advanced for the second launch.  (The plan is asserted on 256 CUs only; the results everywhere.)"""
    from acai_omr_amd import _lib
    M, N, K = E.SPLIT_SHAPE
    d = _inputs(dev, "bf16", M, N, K, keep=False)
    on_256_cus = torch.cuda.get_device_properties(dev).multi_processor_count == 256
    worst = {}
    for name in E.SPLIT_FORMS:
        form = E.form_named("bf16", name)
        err, names, vecs, vec = _call(dev, "bf16", form, "vec", d, M, N)
        assert vec == 1
        if on_256_cus:
            assert names == [f"gemm_nt_pp_kernel<mode={E.pp_mode(form)}>", "gemm_nt_glds_kernel<wm=2>"] and vecs == [1, 1], (name, names, vecs)
            assert [(l.row0, l.rows) for l in _lib.gemm_last_plan()] == [(0, 8192), (8192, 16)], name
        worst[name] = err
    _report("auto 8208 x 2048 x 64", worst)
