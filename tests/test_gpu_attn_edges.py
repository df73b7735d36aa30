"""The attention kernels on probe inputs (tests/attn_probe.py) that turn an addressing defect at an edge - a zero-filled key past the ragged
end that is not masked, a neighbouring sequence's key read in, a key or a query row skipped - into an error of many times the tolerance,
where randn inputs leave it at or below the tolerance (tests/test_attn_probe_cpu.py shows both).  Every operand and every output is a
view into the middle of a larger allocation whose guard rows are finite and hostile (operands) or hold a fill value (outputs): nothing
outside the range may be written, every row inside it must be.  Tolerances are the existing tests': forward 2e-5 (fp32) / 1.2e-2 (bf16),
backward 3e-5 / 6e-2, each times max(1, max |ref|) and taken separately over the ordinary and the reserved columns; the log-sum-exp to
1e-4 / 2e-2.  The shapes are the smallest that reach each kernel form.

Worst error / tolerance seen on an MI355X, per form - the margin the kernels leave under those tolerances (no defect found):
  forward, generic kernel        fp32 out 0.49, lse 0.29 (causal, d_h 64, [300]); bf16 out 0.27, lse 0.08
  forward, two blocks per wave   out 0.27, lse 0.08
  forward, attn_fwd64            out 0.23, lse 0.26 (the single-key sequence; 0.08 otherwise)
  backward, one-block kernels    fp32 dq 0.32, dk 0.19, dv 0.26; bf16 dq 0.15, dk 0.08, dv 0.09
  backward, two blocks per wave  dq 0.06, dk 0.06, dv 0.08
  backward, one pass             dq 0.07, dk 0.08, dv 0.07
  backward, attn_bwd64w          dq 0.06, dk 0.06, dv 0.07, with the wide dK / dV form as without it
  backward, accumulating         dq 0.06, dk 0.07, dv 0.07

Every test also asserts, through acai_attn_last_plan, the kernels and forms that its forward and its backward call ran."""
import contextlib

import pytest
import torch

import attn_probe as P

pytestmark = pytest.mark.gpu

ROWS = 64     # guard rows on either side
BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from acai_omr_amd import _lib
    _lib.lib()  # fails loudly if the HIP library is not built
    return torch.device("cuda:0")


def _operands(case, dtype, prescaled):
    """The probe inputs as the kernel gets them (q prescaled and rounded to dtype if asked for) and the q it thereby effectively sees."""
    from acai_omr_amd import ops
    H, dh, lens_q, lens_k, causal = case
    q, k, v, dout, res = P.build(lens_q, lens_k or lens_q, H, dh, dtype, causal, P.case_seed(case))
    qk = (q * ops.QSCALE(dh)).to(dtype) if prescaled else q.to(dtype)
    q_ref = qk.double() / ops.QSCALE(dh) if prescaled else q.double()
    return qk, q_ref, k, v, dout, res


_REFERENCES = {}


def _reference(case, dtype, prescaled, backward):
    """float64 out, lse (and dq, dk, dv), computed once per input set and shared by the forms that run on it."""
    key = (P.case_id(case), dtype, prescaled)
    have = _REFERENCES.get(key)
    if have is None or (backward and len(have) == 2):
        H, dh, lens_q, lens_k, causal = case
        qk, q_ref, k, v, dout, res = _operands(case, dtype, prescaled)
        shape = (lens_q, lens_k or lens_q, H, dh, causal)
        have = _REFERENCES[key] = P.gradients(q_ref, k, v, dout, *shape) if backward else P.reference(q_ref, k, v, *shape)
    return have


def launch(dev, case, dtype, prescaled, backward=False, lend_workspace=True, calls=1, accumulate=None, overrides=()):
    """Runs the forward (and the backward, `calls` times into the same outputs) on guarded views, under the given (override, value) pairs.
    Returns the WHOLE allocations of the outputs, guards included, on the CPU, and what ran: {"fwd": [AcaiAttnLaunch, ...], "bwd": ...}.
    accumulate = (dk0, dv0): what dk / dv hold before a backward call that adds to them."""
    from acai_omr_amd import _lib, engine, ops
    with contextlib.ExitStack() as stack:
        for which, value in overrides:
            stack.enter_context(ops.attn_override(which, value))
        return _launch(_lib, engine, ops, dev, case, dtype, prescaled, backward, lend_workspace, calls, accumulate)


def _launch(_lib, engine, ops, dev, case, dtype, prescaled, backward, lend_workspace, calls, accumulate):
    H, dh, lens_q, lens_k, causal = case
    lens_k = lens_k or lens_q
    E = H * dh
    qk, q_ref, k, v, dout, res = _operands(case, dtype, prescaled)
    qd = P.guarded(qk.to(dev), ROWS, kind="q")
    kd, vd = P.guarded(k.to(dev).to(dtype), ROWS, kind="k", dh=dh), P.guarded(v.to(dev).to(dtype), ROWS, kind="v")
    cu_q, cu_k = engine.cu_from_lens(lens_q, dev), engine.cu_from_lens(lens_k, dev)
    out = P.guarded(torch.empty(sum(lens_q), E, dtype=dtype, device=dev), ROWS)
    lse = P.guarded(torch.empty(H * sum(lens_q), device=dev), ROWS)
    o = ops.attn_varlen(qd, kd, vd, cu_q, cu_k, H, dh, max(lens_q), causal=causal, out=out, lse=lse, q_prescaled=prescaled)
    assert o.data_ptr() == out.data_ptr()
    got, ran = {"out": out, "lse": lse}, {"fwd": _lib.attn_last_plan()}
    if backward:
        dd = P.guarded(dout.to(dev).to(dtype), ROWS, kind="dout")
        dq, dk, dv = P.guarded(torch.empty_like(qd), ROWS), P.guarded(torch.empty_like(kd), ROWS), P.guarded(torch.empty_like(vd), ROWS)
        if accumulate is not None:
            dk.copy_(accumulate[0].to(dev))
            dv.copy_(accumulate[1].to(dev))
        for _ in range(calls):
            ops.attn_varlen_bwd(qd, kd, vd, out, dd, lse, cu_q, cu_k, H, dh, max(lens_q), max(lens_k), causal, dq, dk, dv, q_prescaled=prescaled,
                                accumulate_dkv=accumulate is not None, lend_workspace=lend_workspace)
            ran["bwd"] = _lib.attn_last_plan()
        got.update(dq=dq, dk=dk, dv=dv)
    torch.cuda.synchronize()
    return {n: t._base.cpu() for n, t in got.items()}, ran


def kernels(launches):
    from acai_omr_amd import _lib
    return [_lib.attn_kernel_name(l) for l in launches]


def _form(kernel, case, dtype, prescaled):
    """The name of an instantiated kernel in the form a case reaches: 16-byte loads where the head size allows them, no dropout."""
    dh = case[1]
    fast = int(dh % (8 if dtype == BF else 4) == 0)
    return (f"{kernel}<{'bf16' if dtype == BF else 'fp32'},{32 if dh <= 32 else 64},fast={fast},drop=0,pre={int(prescaled)}"
            + (",nq=1>" if kernel == "attn_fwd_kernel" else ">"))


def _ragged(lens):
    return len(set(lens)) > 1


def _dq_past_full_blocks(case):
    """The one-block dQ launch over the rows past each sequence's last full 256-row block (tail256 = 1): present unless the host can tell
    from equal lengths that there are no such rows."""
    return _ragged(case[2]) or max(case[2]) % 256 != 0


def check(form, case, dtype, prescaled, whole, accumulate=None):
    """(a) error / tolerance < 1 per output and column group, (b) the log-sum-exp, (c) guards untouched and every row written, (d) all
    finite.  Prints the figures first."""
    H, dh = case[0], case[1]
    backward = "dq" in whole
    ref = dict(zip(("out", "lse", "dq", "dk", "dv"), _reference(case, dtype, prescaled, backward)))
    res = P.reserved_columns(H, dh)
    bf = dtype == BF
    tols = {"out": 1.2e-2 if bf else 2e-5, "dq": 6e-2 if bf else 3e-5}
    tols["dk"] = tols["dv"] = tols["dq"]
    got = {n: w[ROWS:w.shape[0] - ROWS] for n, w in whole.items()}
    if accumulate is not None:
        for n, before in zip(("dk", "dv"), accumulate):
            got[n] = got[n].double() - before.double()
    fig = {n: P.compare(got[n], ref[n], tols[n], res) for n in got if n != "lse"}
    fig["lse"] = float((got["lse"].double().view(H, -1) - ref["lse"]).abs().max()) / (2e-2 if bf else 1e-4)
    print(f"\nPROBE {form} {P.case_id(case)} {'bf16' if bf else 'fp32'}{' prescaled' if prescaled else ''}: "
          + " ".join(f"{n}={fig[n]:.3f}" for n in ("out", "lse", "dq", "dk", "dv") if n in fig))
    for n, w in whole.items():
        assert bool(torch.isfinite(w.float()).all()), (n, "not finite")
    for n in whole:
        view = whole[n][ROWS:whole[n].shape[0] - ROWS]
        assert P.guards_hold(view, ROWS), (n, "a guard row was written")
        if accumulate is None or n not in ("dk", "dv"):
            assert P.all_written(view.reshape(view.shape[0], -1)), (n, "a row in range still holds the fill")
    for n, f in fig.items():
        assert f < 1.0, (n, f)
    return fig


def _typed(cases):
    """case x dtype x prescaled, without the combinations the prescaled form does not exist for (heads that are not 16-byte aligned)."""
    out = []
    for c in cases:
        for dtype in (F32, BF):
            for prescaled in (False, True):
                if not (prescaled and c[1] % (8 if dtype == BF else 4)):
                    out.append(pytest.param(c, dtype, prescaled, id=f"{P.case_id(c)}-{'bf16' if dtype == BF else 'fp32'}{'-prescaled' if prescaled else ''}"))
    return out


@pytest.mark.parametrize("case,dtype,prescaled", _typed(P.FWD_GENERIC))
def test_forward_generic(dev, case, dtype, prescaled):
    """attn_fwd_kernel, one query block per wave: fast and unaligned (bf16 d_h = 12) loads, prescaled or not, causal or not.  (bf16 prescaled
    d_h = 64 without a mask is attn_fwd64.hip's.)"""
    whole, ran = launch(dev, case, dtype, prescaled)
    assert kernels(ran["fwd"]) == [_form("attn_fwd_kernel", case, dtype, prescaled)]
    check("fwd generic", case, dtype, prescaled, whole)


@pytest.mark.parametrize("case", P.FWD_TWO_BLOCK, ids=P.case_id)
def test_forward_two_blocks_per_wave(dev, case):
    """bf16, prescaled, d_h <= 32, >= 512 queries: two query blocks per wave against a zero reference."""
    whole, ran = launch(dev, case, BF, True)
    assert kernels(ran["fwd"]) == ["attn_fwd_kernel<bf16,32,fast=1,drop=0,pre=1,nq=2>"]
    check("fwd two-block", case, BF, True, whole)


@pytest.mark.parametrize("case", P.FWD_64, ids=P.case_id)
def test_forward_dh64_pipelined(dev, case):
    """attn_fwd64.hip (bf16, prescaled, d_h = 64, no mask): the wide kernel, which leaves a sequence's last 256-row block to the tail kernel
    when it holds <= 32 rows.  The tail kernel is launched for every ragged batch (in [40, 129, 192] it finds no such block and exits) and
    for an equal-length one with such a block; [256] runs the wide kernel alone."""
    whole, ran = launch(dev, case, BF, True)
    lens_q = case[2]
    tail = _ragged(lens_q) or 0 < max(lens_q) % 256 <= 32
    assert kernels(ran["fwd"]) == ["attn_fwd64w_kernel"] + (["attn_fwd64_tail_kernel"] if tail else [])
    assert [l.tail for l in ran["fwd"]] == [32 if tail else 0] * len(ran["fwd"])
    check("fwd64", case, BF, True, whole)


@pytest.mark.parametrize("waves,form", [(4, 1), (8, 2)], ids=["four-wave", "eight-wave"])
@pytest.mark.parametrize("case", P.FWD_64, ids=P.case_id)
def test_forward_dh64_narrow_forms(dev, case, waves, form):
    """attn_fwd64_kernel<4> and <8> (32 queries per wave; the override ACAI_ATTN_OV_FWD64 is the only way to them): one launch covers
    every row, tails included."""
    from acai_omr_amd import _lib
    assert form == (_lib.ATTN_FWD64_NW4 if waves == 4 else _lib.ATTN_FWD64_NW8)
    whole, ran = launch(dev, case, BF, True, overrides=[(_lib.ATTN_OV_FWD64, form)])
    assert kernels(ran["fwd"]) == [f"attn_fwd64_kernel<{waves}>"]
    assert ran["fwd"][0].grid_x == -(-max(case[2]) // (32 * waves)) and ran["fwd"][0].block == 64 * waves
    check(f"fwd64 {waves} waves", case, BF, True, whole)


@pytest.mark.parametrize("case,dtype,prescaled", _typed(P.BWD_GENERIC))
def test_backward_one_block(dev, case, dtype, prescaled):
    """attn_bwd.hip's one-block dQ and dK / dV kernels.  (bf16 prescaled d_h = 64 with 256 queries: the wide dQ form of attn_bwd64w.hip.)"""
    whole, ran = launch(dev, case, dtype, prescaled, backward=True)
    dq, dkv = _form("attn_bwd_dq_kernel", case, dtype, prescaled), _form("attn_bwd_dkv_kernel", case, dtype, prescaled)
    wide_dq = dtype == BF and prescaled and case[1] == 64 and not case[4] and max(case[2]) >= 256   # [256] x [400]: no rows past the full block
    assert kernels(ran["bwd"]) == (["attn_bwd64w_dq_kernel", dkv] if wide_dq else [dq, dkv])
    assert [l.tail256 for l in ran["bwd"]] == [0, 0]
    check("bwd one-block", case, dtype, prescaled, whole)


@pytest.mark.parametrize("case", P.BWD_TWO_BLOCK, ids=P.case_id)
def test_backward_two_blocks_per_wave(dev, case):
    """bf16, prescaled, d_h <= 32, >= 512 queries and keys, no workspace lent: the two-blocks-per-wave dQ and dK / dV kernels."""
    whole, ran = launch(dev, case, BF, True, backward=True, lend_workspace=False)
    assert kernels(ran["bwd"]) == ["attn_bwd_dq2_kernel", "attn_bwd_dkv2_kernel"]
    check("bwd two-block", case, BF, True, whole)


@pytest.mark.parametrize("case", P.BWD_TWO_BLOCK + P.BWD_ONE_PASS_EQUAL, ids=P.case_id)
def test_backward_one_pass(dev, case):
    """attn_bwd1p.hip (d_h = 32, a workspace lent; d_h = 24 stays with the two-block kernels): ragged and equal-length launches, called twice
    over the same workspace, which the call itself must zero again."""
    whole, ran = launch(dev, case, BF, True, backward=True, lend_workspace=True, calls=2)
    if case[1] == 32:
        equal = case in P.BWD_ONE_PASS_EQUAL   # (their key counts are multiples of 512: no slot for partial key blocks)
        assert kernels(ran["bwd"]) == ["attn_bwd1p_kernel"]
        assert (ran["bwd"][0].equal_len, ran["bwd"][0].partial_blocks, ran["bwd"][0].tail256) == ((1, 0, 1) if equal else (0, 1, 0))
    else:
        assert kernels(ran["bwd"]) == ["attn_bwd_dq2_kernel", "attn_bwd_dkv2_kernel"]
    check("bwd one-pass", case, BF, True, whole)


@pytest.mark.parametrize("case", P.BWD_64, ids=P.case_id)
def test_backward_dh64_wide_dq(dev, case):
    """bf16, prescaled, d_h = 64, >= 256 queries, as dispatched by default: attn_bwd64w.hip's wide dQ over the full 256-row blocks, the
    one-block kernels over the rows past them (none in [768], an equal-length multiple of 256) and over dK / dV."""
    whole, ran = launch(dev, case, BF, True, backward=True)
    dq, dkv = _form("attn_bwd_dq_kernel", case, BF, True), _form("attn_bwd_dkv_kernel", case, BF, True)
    assert kernels(ran["bwd"]) == ["attn_bwd64w_dq_kernel"] + ([dq] if _dq_past_full_blocks(case) else []) + [dkv]
    assert [l.tail256 for l in ran["bwd"]] == [0] + ([1] if _dq_past_full_blocks(case) else []) + [0]
    check("bwd64w dQ", case, BF, True, whole)


def test_backward_dh64_wide_dkv(dev):
    """attn_bwd64w.hip's wide dK / dV form next to its wide dQ (ACAI_ATTN_OV_BWD64_WIDE = 3; by default only sequences of >= 2048 queries
    take it): the wide kernel over the full 256-key blocks, the one-block kernel over the keys past them.  [768] x [129] has no full key
    block and keeps the one-block dK / dV kernel alone: two of the three cases reach the wide form."""
    from acai_omr_amd import _lib
    for case in P.BWD_64:
        whole, ran = launch(dev, case, BF, True, backward=True, overrides=[(_lib.ATTN_OV_BWD64_WIDE, 3)])
        dq, dkv = _form("attn_bwd_dq_kernel", case, BF, True), _form("attn_bwd_dkv_kernel", case, BF, True)
        wide = max(case[3] or case[2]) >= 256
        assert wide == (case != P.BWD_64[2])
        assert kernels(ran["bwd"]) == ["attn_bwd64w_dq_kernel"] + ([dq] if _dq_past_full_blocks(case) else []) + (["attn_bwd64w_dkv_kernel"] if wide else []) + [dkv]
        assert ran["bwd"][-1].tail256 == (2 if wide else 0)
        check("bwd64w dQ + dK/dV", case, BF, True, whole)


@pytest.mark.parametrize("case", P.BWD_ACCUMULATE, ids=P.case_id)
def test_backward_accumulates_into_dk_dv(dev, case):
    """accumulate_dkv: dk, dv end as what they held plus the gradient (one bf16 rounding of the sum, far inside the tolerance); dq is written."""
    g = torch.Generator().manual_seed(9)
    H, dh, lens_q, lens_k, causal = case
    before = tuple(torch.randn(sum(lens_k), H * dh, generator=g).to(BF) for _ in range(2))
    whole, ran = launch(dev, case, BF, True, backward=True, accumulate=before)
    # (d_h = 64 with 300 queries: the wide dQ and the one-block dQ over the 44 rows past its block; accumulation keeps the one-block dK / dV)
    assert kernels(ran["bwd"]) == ["attn_bwd64w_dq_kernel", _form("attn_bwd_dq_kernel", case, BF, True), _form("attn_bwd_dkv_kernel", case, BF, True)]
    assert [l.tail256 for l in ran["bwd"]] == [0, 1, 0]
    check("bwd accumulate", case, BF, True, whole, accumulate=before)
