"""The self-attention forms of decode_attn_kernel - plain, ancestor table (beam), ring (slots), key table (speculative verify) - and the
matrix-core rollout-group kernel, each launched alone through acai_debug_decode_self_attn / acai_debug_decode_attn_group (the step's own
dispatch on given operands) and held to the float64 reference of tests/decode_attn_reference.py.

Shapes: H = 2, Tmax = 130, at most 13 rows (the bit-for-bit plain launches: 32); (dtype, dh) giving 8, 4, 2, 16 and 4 lanes per key; lengths
at the edges of keys per wave, per workgroup pass, per unrolled iteration and per split, and len == Tmax; one split (chunk 256) and three
(chunk 64: full, partial, one-key and empty splits), merged by the separate combine launch and inside the launch (tickets).  Inputs q = 2
randn, k, v = randn rounded to the cache type, for which the project's bar is 2e-5 absolute.  The caches hold NaN wherever no logical key
lives, so a key read from a wrong place or past a length poisons the row; outputs start as a sentinel between guard rows.

The group kernel rounds its probabilities to bf16, so its inputs make them exact: q = 0 (the mean of V over exactly the image's keys) and
one-hot queries (row g of an image gets the V row of key (7 g + 3) % len: pins the row-to-column mapping of the MFMA tile)."""
import pytest
import torch

import decode_attn_reference as R
from decode_support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

FORM_NO = {"plain": 0, "ancestor": 1, "ring": 2, "spec": 3}
MERGES = [(256, 1, "one_split"), (64, 3, "combine"), (64, 3, "tickets")]
MERGE_IDS = [m[2] for m in MERGES]
_REFS = {}


def _dev(case, dev):  # noqa: F811
    if not hasattr(case, "_d"):
        tdt = torch.bfloat16 if case.dtype == "bf16" else torch.float32
        case._d = {k: (getattr(case, k).to(dev) if getattr(case, k) is not None else None) for k in ("q", "step", "row_len", "table", "seq_off", "seq_len")}
        case._d["kc"], case._d["vc"] = case.kc.to(dev).to(tdt), case.vc.to(dev).to(tdt)
    return case._d


def _run(case, dev, merge, round_out=False, out_dtype=torch.float32, q=None):  # noqa: F811
    """One launch of a self form: the guarded output, after the checks every launch must pass."""
    from acai_omr_amd import ops
    chunk, nsplit, how = merge
    d = _dev(case, dev)
    q = d["q"] if q is None else q
    B = q.shape[0]
    out = R.guarded_out(B, R.H * case.dh, out_dtype, dev)
    tickets = torch.zeros(B * R.H, dtype=torch.int32, device=dev) if how == "tickets" else None
    ops.debug_decode_self_attn(FORM_NO[case.form], q, d["kc"], d["vc"], R.H, case.dh, chunk, nsplit, step=d["step"], row_len=d["row_len"],
                               table=d["table"], table_pitch=case.pitch, table_stride=case.stride, out=out, round_out=round_out, tickets=tickets)
    assert R.intact(out), "NaN in the result, a row not written, or a guard row written"
    assert tickets is None or int(tickets.abs().sum()) == 0, "arrival counters must re-arm to zero"
    return out


def _reference(key, case):
    if key not in _REFS:
        _REFS[key] = R.reference(case)
    return _REFS[key]


def _cases(kind, form, cover):
    return [(n, c) for n, c in R.self_cases(*form, cover) if c.form == kind]


@pytest.mark.parametrize("merge", MERGES, ids=MERGE_IDS)
@pytest.mark.parametrize("form", R.FORMS, ids=R.form_id)
@pytest.mark.parametrize("kind", list(FORM_NO))
def test_form_vs_float64(dev, kind, form, merge):  # noqa: F811
    cover = merge[0] * merge[1]
    worst = (0.0, "")
    for name, case in _cases(kind, form, cover):
        ref = _reference((form, name, cover if kind == "spec" else 0), case)
        err = float((_run(case, dev, merge).double().cpu() - ref).abs().max())
        worst = max(worst, (err, name))
        assert err < R.BAR, (name, err)
    print(f"vs float64: {kind} {R.form_id(form)} {merge[2]}: worst |error| {worst[0]:.3g} ({worst[1]}), bar {R.BAR:g}")


_PLAIN = {}


def _plain_rows(dev, form, merge, L):  # noqa: F811
    """The plain form at length L on every (sequence, query) pair: [SEQS, 8, H * dh]."""
    key = (form, merge[2], L)
    if key not in _PLAIN:
        rows = [(s, j) for s in range(R.SEQS) for j in range(8)]
        _PLAIN[key] = _run(R.build_plain(*form, L, rows=rows), dev, merge).clone().view(R.SEQS, 8, -1)
    return _PLAIN[key]


@pytest.mark.parametrize("merge", MERGES, ids=MERGE_IDS)
@pytest.mark.parametrize("form", R.FORMS, ids=R.form_id)
def test_table_forms_equal_plain_bit_for_bit(dev, form, merge):  # noqa: F811
    """The same logical keys through an ancestor table, a ring or a key table - identity or scattered - give the plain form's bits: what
    makes beam width 1, slots and speculation equal greedy."""
    cover = merge[0] * merge[1]
    cases = [(n, c) for n, c in R.self_cases(*form, cover) if c.form != "plain"]
    cases += [("ring_identity", R.build_ring(*form, identity=True))]
    cases += [(f"ancestor_identity_L{L}", R.build_ancestor(*form, L, L & 1, identity=True)) for L in R.LENGTHS]
    compared = 0
    for name, case in cases:
        out = _run(case, dev, merge)
        for b, ((s, j), L) in enumerate(zip(case.rows, case.lens)):
            if L <= R.TMAX:   # (a verify row may be longer than the cache; the plain form has no such row)
                assert torch.equal(out[b], _plain_rows(dev, form, merge, L)[s, j]), (name, b, L)
                compared += 1
    assert compared > 200


KIND_CASE = {"plain": lambda f, c: R.build_plain(*f, 65), "ancestor": lambda f, c: R.build_ancestor(*f, 65, 1),
             "ring": lambda f, c: R.build_ring(*f, 0), "spec": lambda f, c: R.spec_cases(*f, c)[0][1]}


@pytest.mark.parametrize("merge", [MERGES[0], MERGES[2]], ids=[MERGE_IDS[0], MERGE_IDS[2]])
@pytest.mark.parametrize("form", R.FORMS, ids=R.form_id)
@pytest.mark.parametrize("kind", list(FORM_NO))
def test_output_forms(dev, kind, form, merge):  # noqa: F811
    """round_out rounds the unrounded result to bf16; the bf16 output form stores the same values as bf16."""
    case = KIND_CASE[kind](form, merge[0] * merge[1])
    plain = _run(case, dev, merge)
    rounded = _run(case, dev, merge, round_out=True)
    assert torch.equal(rounded, plain.to(torch.bfloat16).float())
    assert torch.equal(_run(case, dev, merge, round_out=True, out_dtype=torch.bfloat16), rounded.to(torch.bfloat16))
    assert torch.equal(_run(case, dev, merge, out_dtype=torch.bfloat16), plain.to(torch.bfloat16))


@pytest.mark.parametrize("merge", [MERGES[0], MERGES[2]], ids=[MERGE_IDS[0], MERGE_IDS[2]])
@pytest.mark.parametrize("form", [f for f in R.FORMS if f[1] in (12, 64)], ids=R.form_id)
@pytest.mark.parametrize("kind", list(FORM_NO))
def test_q_load_paths(dev, kind, form, merge):  # noqa: F811
    """q one float off 16-byte alignment, q with a row stride that is no multiple of 4, and both: the dword loads give the 16-byte path's bits."""
    case = KIND_CASE[kind](form, merge[0] * merge[1])
    q = _dev(case, dev)["q"]
    B, E = q.shape
    assert q.data_ptr() % 16 == 0 and q.stride(0) % 4 == 0
    want = _run(case, dev, merge)
    for shift, ld in ((1, E), (0, E + 3), (1, E + 1)):
        buf = torch.full((4 + shift + B * ld,), float("nan"), device=dev)
        view = buf[4 + shift:].view(B, ld)[:, :E]
        view.copy_(q)
        assert (view.data_ptr() % 16 != 0) == (shift != 0) and view.stride(0) == ld
        assert torch.equal(_run(case, dev, merge, q=view), want), (shift, ld)


def test_self_entry_refuses_without_launching(dev):  # noqa: F811
    from acai_omr_amd import ops
    case = R.build_ancestor("bf16", 64, 65, 0)
    d = _dev(case, dev)

    def call(form=1, chunk=64, nsplit=3, out_dtype=torch.float32, tickets=False, kc=None, table=d["table"], step=d["step"], stride=case.stride):
        out = R.guarded_out(3, R.H * 64, out_dtype, dev)
        tk = torch.zeros(3 * R.H, dtype=torch.int32, device=dev) if tickets else None
        with pytest.raises(RuntimeError, match="acai_debug_decode_self_attn"):
            ops.debug_decode_self_attn(form, d["q"], d["kc"] if kc is None else kc, d["vc"] if kc is None else kc, R.H, 64, chunk, nsplit, step=step,
                                       row_len=None, table=table, table_pitch=case.pitch, table_stride=stride, out=out, tickets=tk)
        torch.cuda.synchronize()
        assert bool((out._base == 7.0).all()), "a refused call must launch nothing"

    call(chunk=64, nsplit=2)                       # the splits do not cover the cache
    call(chunk=32768, nsplit=1)                    # the LDS-staged table bounds the chunk
    call(out_dtype=torch.bfloat16)                 # bf16 rows from the combine launch
    call(table=None)                               # a table form without its table
    call(step=None)
    call(form=4)
    call(form=2)                                   # the ring form without row_len
    call(kc=torch.zeros(6, R.H, R.TMAX, 48, dtype=torch.bfloat16, device=dev))   # dhp no power of two
    call(form=3, stride=4)                         # rows per image must divide B (and spec needs row_len)


# ---- the rollout-group kernel ---------------------------------------------------------------------------------------------------------------
def _run_group(case, dev, chunk, nsplit):  # noqa: F811
    from acai_omr_amd import ops
    d = _dev(case, dev)
    B = d["q"].shape[0]
    out = R.guarded_out(B, R.H * case.dh, torch.float32, dev)
    tickets = torch.zeros(B * R.H, dtype=torch.int32, device=dev) if nsplit > 1 else None
    ops.debug_decode_attn_group(d["q"], d["kc"], d["vc"], d["seq_off"], d["seq_len"], R.H, case.dh, 64, case.group, chunk, nsplit, out=out,
                                tickets=tickets)
    assert R.intact(out), "NaN in the result, a row not written, or a guard row written"
    assert tickets is None or int(tickets.abs().sum()) == 0, "arrival counters must re-arm to zero"
    return out


@pytest.mark.parametrize("split", R.GROUP_SPLITS, ids=["chunk64_tickets", "one_split"])
@pytest.mark.parametrize("kind", ["mean", "onehot"])
@pytest.mark.parametrize("dh", [64, 48])
@pytest.mark.parametrize("group", list(R.GROUP_MEMS))
def test_group_kernel_vs_float64(dev, group, dh, kind, split):  # noqa: F811
    case = R.build_group(dh, group, kind)
    ref = _reference(("group", group, dh, kind), case)
    if kind == "onehot":
        assert float((ref - R.one_hot_targets(case)).abs().max()) < 1e-9
    err = (_run_group(case, dev, *split).double().cpu() - ref).abs().max(1).values
    print(f"vs float64: group {group} dh{dh} {kind} chunk {split[0]} x {split[1]}: worst |error| {float(err.max()):.3g}, bar {R.BAR:g}")
    assert float(err.max()) < R.BAR, (float(err.max()), int(err.argmax()))


def test_group_entry_refuses_without_launching(dev):  # noqa: F811
    from acai_omr_amd import ops
    case = R.build_group(64, 2, "mean")
    d = _dev(case, dev)
    B = d["q"].shape[0]

    def call(group=2, nsplit=5, tickets=True, kc=d["kc"], dhp=64):
        out = R.guarded_out(B, R.H * 64, torch.float32, dev)
        tk = torch.zeros(B * R.H, dtype=torch.int32, device=dev) if tickets else None
        with pytest.raises(RuntimeError, match="acai_debug_decode_attn_group"):
            ops.debug_decode_attn_group(d["q"], kc, kc, d["seq_off"], d["seq_len"], R.H, 64 if dhp == 64 else 32, dhp, group, 64, nsplit, out=out,
                                        tickets=tk)
        torch.cuda.synchronize()
        assert bool((out._base == 7.0).all()), "a refused call must launch nothing"

    call(group=4)             # B = 14 rows
    call(tickets=False)       # several splits merge inside the launch only
    call(dhp=32)
