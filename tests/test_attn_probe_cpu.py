"""The probe inputs of tests/attn_probe.py are decisive: on every shape tests/test_gpu_attn_edges.py runs, each addressing defect an
attention kernel is likely to have, injected into the float64 reference, moves the result by at least FOUR times the tolerance the GPU test
allows a bf16 kernel (1.2e-2 forward, 6e-2 backward, each times max(1, max |ref|)).  A kernel's own rounding error is bounded by the
tolerance, so it is a factor of three short of hiding such a defect.  No GPU."""
import math

import pytest
import torch

import attn_probe as P

BF = torch.bfloat16
DECISIVE = 4.0


def key_defects(case):
    """Per sequence: the last key, key 64, key 0 dropped; the neighbours' adjacent keys leaked in; a zero phantom key.  Causal: the mask off by one."""
    H, dh, lens_q, lens_k, causal = case
    lens_k = lens_k or lens_q
    out = []
    for s, lk in enumerate(lens_k):
        out.append(("drop_key", s, lk - 1))
        if lk > 64:
            out.append(("drop_key", s, 64))
        if lk > 1:
            out.append(("drop_key", s, 0))
        if s + 1 < len(lens_k):
            out.append(("leak_key_after", s))
        if s > 0:
            out.append(("leak_key_before", s))
        out.append(("phantom_zero_key", s))
    if causal:
        out += [("causal_offset", 1), ("causal_offset", -1)]
    return out


def row_defects(case):
    """Per sequence: the last query row and the first row of the second 256-row block lost."""
    out = []
    for s, lq in enumerate(case[2]):
        out.append(("lose_query_row", s, lq - 1))
        if lq > 256:
            out.append(("lose_query_row", s, 256))
    return out


def _inputs(case):
    H, dh, lens_q, lens_k, causal = case
    lens_k = lens_k or lens_q
    return (lens_q, lens_k, H, dh, causal), P.build(lens_q, lens_k, H, dh, BF, causal, P.case_seed(case))


@pytest.mark.parametrize("case", P.FWD_CASES, ids=P.case_id)
def test_forward_defects_are_decisive(case):
    shape, (q, k, v, dout, res) = _inputs(case)
    base = P.reference(q, k, v, *shape)[0]
    for d in key_defects(case):
        r = P.compare(P.reference(q, k, v, *shape, defect=d)[0], base, 1.2e-2, res)
        assert r >= DECISIVE, (d, r)


@pytest.mark.parametrize("case", P.BWD_CASES, ids=P.case_id)
def test_backward_defects_are_decisive(case):
    """A key defect must show in at least one of dq, dk, dv (the GPU test holds all three to the tolerance); a lost query row in dk or dv."""
    shape, (q, k, v, dout, res) = _inputs(case)
    base = P.gradients(q, k, v, dout, *shape)
    for d in key_defects(case) + row_defects(case):
        got = P.gradients(q, k, v, dout, *shape, defect=d)
        r = max(P.compare(got[i], base[i], 6e-2, res) for i in ((3, 4) if d[0] == "lose_query_row" else (2, 3, 4)))
        assert r >= DECISIVE, (d, r)


def test_randn_inputs_do_not_show_a_phantom_key():
    """The gap the probe closes: on plain randn inputs a kernel that attends to a zero-filled key past the ragged end stays far inside the
    tolerance, forward and backward."""
    H, dh, lens_q, lens_k = 2, 32, [600, 513], [1000, 577]
    g = torch.Generator().manual_seed(5)
    q, dout = (torch.randn(sum(lens_q), H * dh, generator=g).to(BF).float() for _ in range(2))
    k, v = (torch.randn(sum(lens_k), H * dh, generator=g).to(BF).float() for _ in range(2))
    res = P.reserved_columns(H, dh)
    shape = (lens_q, lens_k, H, dh, False)
    base = P.gradients(q, k, v, dout, *shape)
    for s in range(2):
        got = P.gradients(q, k, v, dout, *shape, defect=("phantom_zero_key", s))
        assert P.compare(got[0], base[0], 1.2e-2, res) < 0.1
        assert max(P.compare(got[i], base[i], 6e-2, res) for i in (2, 3, 4)) < 0.1


@pytest.mark.parametrize("causal", [False, True])
def test_reference_without_a_defect_is_softmax_attention(causal):
    """Against torch's own scaled_dot_product_attention in float64, per sequence and head; the log-sum-exp in the log2 domain."""
    H, dh, lens_q, lens_k = 2, 8, [5, 9], [7, 9]
    q, k, v, dout, res = P.build(lens_q, lens_k, H, dh, torch.float32, causal, 3)
    out, lse = P.reference(q, k, v, lens_q, lens_k, H, dh, causal)
    oq = ok = 0
    for lq, lk in zip(lens_q, lens_k):
        for h in range(H):
            sl = slice(h * dh, (h + 1) * dh)
            qs, ks, vs = q[oq:oq + lq, sl].double(), k[ok:ok + lk, sl].double(), v[ok:ok + lk, sl].double()
            mask = torch.ones(lq, lk, dtype=torch.bool).tril() if causal else None
            want = torch.nn.functional.scaled_dot_product_attention(qs[None], ks[None], vs[None], attn_mask=mask)[0]
            assert float((out[oq:oq + lq, sl] - want).abs().max()) < 1e-12
            sc = qs @ ks.t() / math.sqrt(dh)
            if causal:
                sc = sc.masked_fill(~mask, float("-inf"))
            assert float((lse[h, oq:oq + lq] - torch.log2(torch.exp(sc).sum(-1))).abs().max()) < 1e-9
        oq += lq
        ok += lk


def test_probe_columns_leave_the_scores_inside_a_sequence_alone():
    """Parity and shift change every score of a row by the same amount: the output equals the one with those three columns zeroed."""
    H, dh, lens_q, lens_k = 2, 16, [9, 6, 4], [11, 5, 8]
    q, k, v, dout, res = P.build(lens_q, lens_k, H, dh, BF, False, 1)
    out = P.reference(q, k, v, lens_q, lens_k, H, dh, False)[0]
    q0 = q.clone()
    q0.view(-1, H, dh)[:, :, :3] = 0.0
    assert float((P.reference(q0, k, v, lens_q, lens_k, H, dh, False)[0] - out).abs().max()) < 1e-9
    Aq, Ak = P.amplitude(dh)
    assert abs(Aq * Ak / math.sqrt(dh) - 30.0) < 1.0 and torch.equal(q, q.to(BF).float()) and torch.equal(k, k.to(BF).float())


def test_guarded_views():
    H, dh = 2, 8
    t = torch.randn(10, H * dh).to(BF)
    for kind in ("q", "k", "v", "dout"):
        g = P.guarded(t, 4, kind=kind, dh=dh)
        assert torch.equal(g, t) and g._base.shape[0] == 18 and bool(torch.isfinite(g._base.float()).all())
        assert g.data_ptr() == g._base.data_ptr() + 4 * H * dh * 2
    gk = P.guarded(t, 4, kind="k", dh=dh)._base.float().view(18, H, dh)
    for rows in (slice(0, 4), slice(14, 18)):
        assert bool((gk[rows, :, :2] == P.amplitude(dh)[1]).all()) and bool((gk[rows, :, 2] == 0).all())
    o = P.guarded(torch.empty(10, H * dh), 4)
    assert P.guards_hold(o, 4) and not P.all_written(o)
    o[:9] = 1.0
    assert P.guards_hold(o, 4) and not P.all_written(o)
    o[9] = 2.0
    assert P.all_written(o)
    o._base[3, 0] = 0.0
    assert not P.guards_hold(o, 4)
    assert P.compare(torch.full((2, 16), float("nan")), torch.zeros(2, 16), 1.0, P.reserved_columns(H, dh)) == float("inf")
