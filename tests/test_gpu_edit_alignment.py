"""Edit alignment on the GPU (acai_edit_align / ops.edit_alignment) against the CPU table and canonical traceback of
tests/edit_alignment_reference.py, and what is built on it: the S/I/D breakdown, the ground-truth error maps (ViTOMR.error_maps,
diagnosed_inference) and ser_validation's breakdown.  Every output is an integer array: every comparison is exact."""
import numpy as np
import pytest
import torch
from torch.amp import autocast

from conftest import load_golden
from decode_support import _same, build_vitomr, dev  # noqa: F401
from edit_alignment_reference import INS, MATCH, SUB, edit_alignment
from edit_distance_reference import edit_distance

pytestmark = pytest.mark.gpu

NAMES = ("counts", "pred_op", "pred_to_tgt", "tgt_to_pred", "tgt_slot")
# longer-row lengths: both edges of every strip width (64 W for W in 1 2 4 8 12 16 24 32 48 64) and of every direction-word count (W = 16 | 24, 32 | 48 | 64)
EDGES = [1, 63, 64, 65, 128, 129, 256, 257, 512, 513, 768, 769, 1024, 1025, 1536, 1537, 2048, 2049, 3072, 3073, 4096]


def _pack(rows, width=None, fill=0):
    """list of 1-D integer sequences -> (int64 (N, width) padded with `fill`, int32 (N,) lengths), on the CPU"""
    lens = [len(r) for r in rows]
    out = torch.full((len(rows), width if width is not None else max(lens + [1])), fill, dtype=torch.int64)
    for i, r in enumerate(rows):
        out[i, :lens[i]] = torch.as_tensor(np.asarray(r, dtype=np.int64))
    return out, torch.tensor(lens, dtype=torch.int32)


def _want(preds, tgts, Lp, Lt, group=1):
    """The reference's five arrays for pred row r against target row r // group, padded to the widths."""
    cols = [[], [], [], [], []]
    for r, p in enumerate(preds):
        for c, x in zip(cols, edit_alignment(p, tgts[r // group], Lp, Lt)):
            c.append(x)
    return [np.stack(c) for c in cols]


def _check(got, want, what, preds=None, tgts=None, group=1):
    assert [t.dtype for t in got] == [torch.int32, torch.int8, torch.int32, torch.int32, torch.int32]
    for name, g, w in zip(NAMES, got, want):
        g = g.cpu().numpy()
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            rows = np.nonzero((g != w).reshape(g.shape[0], -1).any(1))[0]
            r = int(rows[0])
            lens = (len(preds[r]), len(tgts[r // group])) if preds is not None else None
            cols = np.nonzero(g[r] != w[r])[0]
            raise AssertionError(f"{what}: {name} differs in rows {rows.tolist()[:8]}; row {r} (lp, lt) = {lens} first at {cols[:5].tolist()}: "
                                 f"got {g[r][cols[:5]].tolist()} want {w[r][cols[:5]].tolist()}")


def _run(dev, preds, tgts, what, group=1, width_p=None, width_t=None, fill=0, **kw):
    """ops.edit_alignment on the packed rows against the reference, plus the cross-check against ops.edit_distance; returns the result."""
    from acai_omr_amd import ops
    p, pl = _pack(preds, width_p, fill)
    t, tl = _pack(tgts, width_t, fill)
    p, pl, t, tl = p.to(dev), pl.to(dev), t.to(dev), tl.to(dev)
    al = ops.edit_alignment(p, pl, t, tl, group=group, **kw)
    assert isinstance(al, ops.EditAlignment)
    _check(al, _want(preds, tgts, p.shape[1], t.shape[1], group), what, preds, tgts, group)
    assert torch.equal(al.counts[:, 1:].sum(1, dtype=torch.int32), ops.edit_distance(p, pl, t, tl, group=group)), what
    return al


def _shorter(k, m):
    """A few shorter-side lengths for the k-th longer length m out of {1, 7, 64, 65, m - 1, m}."""
    picks = [(1, 64), (7, 65)][k % 2] + (m - 1, m)
    return sorted({n for n in picks if 1 <= n <= m})


def test_strip_widths_and_direction_words_at_their_edges(dev):
    """Every strip width and direction-word count at both edges, pred the longer side and target the longer side; alphabets of 2 and 3 ids, so
    that nearly every cell has co-optimal neighbours.  One launch per longer length; 4096 x 4096 once."""
    rng = np.random.default_rng(2024)
    pairs = 0
    for k, m in enumerate(EDGES):
        preds, tgts = [], []
        for n in _shorter(k, m):
            vocab = 2 + (len(preds) + k) % 2
            a, b = rng.integers(0, vocab, size=m), rng.integers(0, vocab, size=n)
            preds.append(a), tgts.append(b)                  # pred the longer side (or equal)
            if n < m:
                preds.append(b.copy()), tgts.append(a.copy())    # target the longer side
        pairs += len(preds)
        _run(dev, preds, tgts, f"m = {m}")
    print(f"{pairs} pairs")
    assert pairs <= 200


@pytest.mark.parametrize("vocab", [2, 3])
def test_ties_across_two_strip_widths(dev, vocab):
    """Tiny alphabets: many co-optimal paths, where a wrong tie-break shows.  Lengths on both sides of the W = 1 | 2 and 2 | 4 edges, every
    pair of them in both orientations, in one launch."""
    rng = np.random.default_rng(50 + vocab)
    lens = [2, 3, 5, 17, 40, 64, 65, 100, 128, 129, 200]
    preds, tgts = [], []
    for lp in lens:
        for lt in lens:
            preds.append(rng.integers(0, vocab, size=lp)), tgts.append(rng.integers(0, vocab, size=lt))
    _run(dev, preds, tgts, f"ties, alphabet {vocab}")


def test_structured_rows_and_empty_sides(dev):
    rng = np.random.default_rng(5)
    preds, tgts = [], []
    for n in (1, 64, 65, 300, 1000):
        row = rng.permutation(5000)[:n]                                              # distinct ids: the optimal alignment is unique
        preds.append(row), tgts.append(row.copy())                                   # identical
        preds.append(row), tgts.append(row[:n // 3].copy())                          # the target a prefix of pred: insertions at the end
        preds.append(row[:n // 3].copy()), tgts.append(row)                          # pred a prefix of the target: deletions at the end
        preds.append(row), tgts.append(row[n - n // 3:].copy())                      # the target a suffix of pred: insertions at the start
        preds.append(row[n - n // 3:].copy()), tgts.append(row)                      # pred a suffix of the target: deletions at the start
        preds.append(row), tgts.append(10000 + rng.permutation(5000)[:n - n // 4])     # no id in common: substitutions + a length difference
        preds.append(10000 + rng.permutation(5000)[:n - n // 4]), tgts.append(row)
    for n in (0, 1, 5, 64, 700):                                                     # an empty side, and both
        preds.append(np.zeros(0, np.int64)), tgts.append(rng.integers(0, 4, size=n))
        preds.append(rng.integers(0, 4, size=n)), tgts.append(np.zeros(0, np.int64))
    al = _run(dev, preds, tgts, "structured rows")
    counts = al.counts.cpu().tolist()
    assert counts[0] == [1, 0, 0, 0] and counts[7 * 3] == [300, 0, 0, 0]
    assert counts[7 * 3 + 1] == [100, 0, 200, 0] and counts[7 * 3 + 2] == [100, 0, 0, 200] and counts[7 * 3 + 3] == [100, 0, 200, 0]
    assert counts[7 * 3 + 5] == [0, 225, 75, 0] and counts[7 * 3 + 6] == [0, 225, 0, 75]
    assert counts[-2] == [0, 0, 0, 700] and counts[-1] == [0, 0, 700, 0] and counts[35] == [0, 0, 0, 0]
    op = al.pred_op.cpu()
    assert op[7 * 3 + 1, :100].eq(MATCH).all() and op[7 * 3 + 1, 100:300].eq(INS).all()        # the run of insertions lies at the end ...
    assert op[7 * 3 + 3, :200].eq(INS).all() and op[7 * 3 + 3, 200:300].eq(MATCH).all()        # ... or at the start
    assert al.tgt_slot[7 * 3 + 2, 100:300].eq(100).all() and al.tgt_slot[7 * 3 + 4, :200].eq(0).all()


def test_group_shares_the_target_row(dev):
    rng = np.random.default_rng(8)
    G, B = 4, 5
    tgts = [rng.integers(0, 3, size=int(rng.integers(0, 300))) for _ in range(B)]
    preds = [rng.integers(0, 3, size=int(rng.integers(0, 330))) for _ in range(B * G)]
    grouped = _run(dev, preds, tgts, "group 4", group=G)
    repeated = _run(dev, preds, [t for t in tgts for _ in range(G)], "repeated targets")
    _same(grouped, repeated)


def test_padding_masks_clamped_lengths_and_large_ids(dev):
    from acai_omr_amd import ops
    rng = np.random.default_rng(9)
    preds = [rng.integers(0, 5, size=n) for n in (0, 3, 64, 65, 200, 511)]
    tgts = [rng.integers(0, 5, size=n) for n in (5, 0, 64, 300, 199, 512)]
    want = _want(preds, tgts, 600, 520)
    for fill_p, fill_t in ((0, 0), (7, 200), (2 ** 31 - 1, -1), (-5, 2 ** 40)):
        p, pl = _pack(preds, width=600, fill=fill_p)
        t, tl = _pack(tgts, width=520, fill=fill_t)
        _check(ops.edit_alignment(p.to(dev), pl.to(dev), t.to(dev), tl.to(dev)), want, f"fill {fill_p} / {fill_t}", preds, tgts)
    # random valid ids past the lengths; lengths as int32 and as bool prefix masks, on either side and on both
    p, pl = _pack(preds, width=600)
    t, tl = _pack(tgts, width=520)
    pm = torch.arange(p.shape[1])[None, :] < pl[:, None]
    tm = torch.arange(t.shape[1])[None, :] < tl[:, None]
    p = torch.where(pm, p, torch.from_numpy(rng.integers(0, 5, size=tuple(p.shape))))
    t = torch.where(tm, t, torch.from_numpy(rng.integers(0, 5, size=tuple(t.shape))))
    p, pl, pm, t, tl, tm = (x.to(dev) for x in (p, pl, pm, t, tl, tm))
    for a, b in ((pl, tl), (pm, tm), (pm, tl), (pl, tm)):
        al = ops.edit_alignment(p, a, t, b)
        _check(al, want, f"lengths {a.dtype} / {b.dtype}", preds, tgts)
    assert bool((al.pred_op[4, 200:] == -1).all()) and bool((al.tgt_slot[4, 199:] == -1).all()) and bool((al.pred_op[4, :200] >= 0).all())
    # a length above the width is clamped to it, a negative one to 0
    over = ops.edit_alignment(p, torch.tensor([700, 3, 64, -4, 100000, 511], dtype=torch.int32, device=dev), t, tl)
    rows = p.cpu().numpy()
    clamped = [rows[0], preds[1], preds[2], preds[3][:0], rows[4], preds[5]]
    _check(over, _want(clamped, tgts, 600, 520), "clamped lengths", clamped, tgts)
    # ids at and next to 2^31 - 1, as edit_distance's test has them
    top = 2 ** 31 - 1
    a = top - rng.integers(0, 3, size=300)
    b = top - rng.integers(0, 3, size=280)
    c = a.copy()
    c[17] = top if a[17] != top else top - 1
    d = np.where(a == top, 0, a)
    al = _run(dev, [a, a, a, np.array([top]), np.array([top])], [b, c, d, np.array([top]), np.array([top - 1])], "ids near 2^31")
    counts = al.counts.cpu().tolist()
    assert counts[1] == [299, 1, 0, 0] and int(al.pred_op[1, 17]) == SUB and counts[3] == [1, 0, 0, 0] and counts[4] == [0, 1, 0, 0]
    assert sum(counts[2][1:]) == int((a == top).sum())


def _rollouts(dev, seed=11):
    rng = np.random.default_rng(seed)
    preds = [rng.integers(0, 4, size=int(rng.integers(0, 768))) for _ in range(24)]
    tgts = [rng.integers(0, 4, size=int(rng.integers(300, 700))) for _ in range(6)]
    p, pl = (x.to(dev) for x in _pack(preds, width=768))
    t, tl = (x.to(dev) for x in _pack(tgts, width=700))
    return preds, tgts, p, pl, t, tl


def test_repeatable_chunked_and_given_buffers(dev):
    """Two calls give the same bits; a small workspace= forces chunks of whole groups, with the same results; out= is written in place."""
    from acai_omr_amd import ops
    preds, tgts, p, pl, t, tl = _rollouts(dev)
    want = _want(preds, tgts, 768, 700, group=4)
    first = ops.edit_alignment(p, pl, t, tl, group=4)
    second = ops.edit_alignment(p, pl, t, tl, group=4)
    _check(first, want, "first call", preds, tgts, 4)
    _same(first, second)
    per_pair = ops.edit_alignment_workspace_bytes(768, 700)
    assert per_pair == (700 + 63) * 1 * 256 and ops.edit_alignment_workspace_bytes(768, 700, 24) == 24 * per_pair
    assert ops.edit_alignment_workspace_bytes(4096, 4096) == (4096 + 63) * 4 * 256 and ops.edit_alignment_workspace_bytes(1536, 1536) == (1536 + 63) * 2 * 256
    for groups in (1, 2, 5, 6):   # chunks of 1, 2 and 5 (+ 1 left over) groups, and the single launch in a given buffer
        ws = torch.empty(groups * 4 * per_pair + 100, dtype=torch.uint8, device=dev)
        out = ops.EditAlignment(*(torch.full_like(x, -7) for x in first))
        got = ops.edit_alignment(p, pl, t, tl, group=4, out=out, workspace=ws)
        assert all(a is b for a, b in zip(got, out))
        _same(got, first)


def test_graph_replay_reads_new_inputs(dev):
    from acai_omr_amd import ops
    preds, tgts, p, pl, t, tl = _rollouts(dev, seed=12)
    first = ops.edit_alignment(p, pl, t, tl, group=4)
    out = ops.EditAlignment(*(torch.full_like(x, -7) for x in first))
    ws = torch.empty(ops.edit_alignment_workspace_bytes(768, 700, 24), dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ops.edit_alignment(p, pl, t, tl, group=4, out=out, workspace=ws)   # (the code object is loaded: nothing but the launch is left to capture)
        s.synchronize()
        g = ops.Graph()
        g.begin()
        try:
            ops.edit_alignment(p, pl, t, tl, group=4, out=out, workspace=ws)
        finally:
            g.end()
        for x in out:
            x.fill_(-7)
        g.launch()
        s.synchronize()
        _same(out, first)
        # lengths and tokens are read by the replayed launch: shorten every rollout, rewrite one target row in place, and replay
        pl.copy_(torch.clamp(pl - 5, min=0))
        t[1].copy_(torch.flip(t[1], dims=[0]))
        g.launch()
        s.synchronize()
    preds2 = [a[:max(len(a) - 5, 0)] for a in preds]
    trow = t[1].cpu().numpy()
    tgts2 = [x if i != 1 else trow[:len(x)] for i, x in enumerate(tgts)]
    _check(out, _want(preds2, tgts2, 768, 700, group=4), "replay after the inputs changed", preds2, tgts2, 4)


def test_operand_checks(dev):
    from acai_omr_amd import ops
    ok = torch.zeros(2, 8, dtype=torch.int64, device=dev)
    ln = torch.full((2,), 8, dtype=torch.int32, device=dev)
    wide = torch.zeros(2, 4097, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError):
        ops.edit_alignment(wide, ln, ok, ln)
    with pytest.raises(ValueError):
        ops.edit_alignment(ok, ln, wide, ln)
    with pytest.raises(ValueError):
        ops.edit_alignment(ok, ln, ok[:1], ln[:1], group=3)       # R != Rt * group
    with pytest.raises(TypeError):
        ops.edit_alignment(ok.int(), ln, ok, ln)
    with pytest.raises(TypeError):
        ops.edit_alignment(ok, ln.long(), ok, ln)
    with pytest.raises(RuntimeError):
        ops.edit_alignment(ok.cpu(), ln, ok, ln)
    need = ops.edit_alignment_workspace_bytes(8, 8)
    with pytest.raises(ValueError):
        ops.edit_alignment(ok, ln, ok, ln, workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev))     # not even one pair
    with pytest.raises(ValueError):
        ops.edit_alignment(ok, ln, ok, ln, group=2, workspace=torch.empty(need, dtype=torch.uint8, device=dev))   # not even one group
    with pytest.raises(RuntimeError):
        ops.edit_alignment(ok, ln, ok, ln, workspace=torch.empty(2 * need, dtype=torch.uint8))                   # a CPU buffer
    good = ops.edit_alignment(ok, ln, ok, ln)
    with pytest.raises(TypeError):
        ops.edit_alignment(ok, ln, ok, ln, out=good._replace(pred_op=good.pred_op.int()))
    with pytest.raises(ValueError):
        ops.edit_alignment(ok, ln, ok, ln, out=good._replace(tgt_slot=good.tgt_slot[:, :7]))
    # the C entry point refuses a short workspace and a missing pointer before it launches anything
    from acai_omr_amd import _lib
    L = _lib.lib()
    ws = torch.empty(2 * need, dtype=torch.uint8, device=dev)
    args = lambda nbytes, counts: (ok.data_ptr(), 8, ln.data_ptr(), ok.data_ptr(), 8, ln.data_ptr(), 2, 1, counts, good.pred_op.data_ptr(),   # noqa: E731
                                   good.pred_to_tgt.data_ptr(), good.tgt_to_pred.data_ptr(), good.tgt_slot.data_ptr(), ws.data_ptr(), nbytes, 0)
    assert L.acai_edit_align(*args(2 * need - 1, good.counts.data_ptr())) != 0 and b"workspace" in L.acai_last_error()
    assert L.acai_edit_align(*args(2 * need, None)) != 0
    assert L.acai_edit_align_workspace_bytes(4097, 8, 1) == 0
    # R == 0: empty outputs, nothing launched; 4096 itself is accepted
    empty = ops.edit_alignment(ok[:0], ln[:0], ok[:0], ln[:0])
    assert [tuple(x.shape) for x in empty] == [(0, 4), (0, 8), (0, 8), (0, 8), (0, 8)]
    full = torch.zeros(2, 4096, dtype=torch.int64, device=dev)
    assert ops.edit_alignment(full, ln, ok, ln).counts.cpu().tolist() == [[8, 0, 0, 0]] * 2


# ---- end to end on the tiny golden model ---------------------------------------------------------------------------------------------------
BF = torch.bfloat16
_MODEL = {}


def _decoded(dev):
    """(fixture, model, greedy seqs, log_probs, seq_mask, rows as CPU tensors) of the tiny golden model, built and decoded once."""
    from acai_omr_amd.inference.vitomr_inference import inference
    if not _MODEL:
        fx = load_golden("vitomr_small")
        m = build_vitomr(fx["cfg"], fx["state_dict"], dev, BF, 12)
        seqs, lps, mask = inference(m, fx["imgs"], "cuda", max_inference_len=fx["cfg"]["gen_len"])
        _MODEL["x"] = (fx, m, seqs, lps, mask, [seqs[i, :int(mask[i].sum())].cpu() for i in range(seqs.shape[0])])
    return _MODEL["x"]


def _grids(fx):
    P = fx["cfg"]["P"]
    return [(int(t.shape[-2]) // P, int(t.shape[-1]) // P) for t in fx["imgs"]]


def _padded_memory(m, imgs):
    """The packed memory of the inference entry points (encoder outside autocast, transition head inside), padded to (B, S_max, E) with its
    mask: the same rows, bit for bit, that diagnosed_inference's pass reads."""
    from acai_omr_amd.inference.vitomr_inference import _encode
    with torch.no_grad():
        lat32, _, lens = _encode(m, imgs)
        with autocast(device_type="cuda", dtype=BF):
            mem = m.transition_head.forward_packed(lat32)
    out = torch.zeros(len(lens), max(lens), mem.shape[-1], dtype=mem.dtype, device=mem.device)
    mask = torch.ones(len(lens), max(lens), dtype=torch.bool, device=mem.device)
    o = 0
    for i, s in enumerate(lens):
        out[i, :s] = mem[o:o + s]
        mask[i, :s] = False
        o += s
    return out, mask


def test_diagnosed_inference_of_the_models_own_output(dev):
    """Targets equal to the decode's rows: every op is a match, the error map is all zero, and the decode is inference()'s."""
    from acai_omr_amd.inference.vitomr_inference import diagnosed_inference, inference
    fx, m, seqs, lps, mask, rows = _decoded(dev)
    n = fx["cfg"]["gen_len"]
    got = diagnosed_inference(m, fx["imgs"], rows, "cuda", max_inference_len=n)
    _same(got[:3], (seqs, lps, mask))
    conf, al = got[3], got[4]
    assert al.counts.cpu().tolist() == [[len(r), 0, 0, 0] for r in rows]
    for i, r in enumerate(rows):
        assert bool((al.pred_op[i, :len(r)] == MATCH).all()) and al.pred_to_tgt[i, :len(r)].cpu().tolist() == list(range(len(r)))
    assert [tuple(u.shape) for u in conf.uncertainty] == _grids(fx) and all(float(u.abs().max()) == 0.0 for u in conf.uncertainty)
    assert conf.alignment is not None and conf.alignment.grids == _grids(fx) and not bool(torch.isnan(conf.log_prob[:, 1:len(rows[0])]).any())
    _same(inference(m, fx["imgs"], "cuda", max_inference_len=n), (seqs, lps, mask))   # engine state is untouched


def test_diagnosed_inference_names_the_edits(dev):
    """In rows whose tokens are all distinct - so that the optimal alignment is unique - the target gets one token substituted, one removed
    and one added at known indices: the ops name exactly those, the breakdown is one of each, and the heat map is uncertainty_maps' map of
    the hand-built weight, bit for bit; a token added after <eos> is charged to the last output position (the slot clamp)."""
    from acai_omr_amd.inference.vitomr_inference import diagnosed_inference
    from acai_omr_amd.utils import confidence_error_auroc, symbol_error_breakdown, token_confusions
    fx, m, seqs, lps, mask, rows = _decoded(dev)
    n = fx["cfg"]["gen_len"]
    distinct = [i for i, r in enumerate(rows) if len(set(r.tolist())) == len(r) and len(r) >= 10]
    assert len(distinct) >= 2, [r.tolist() for r in rows]
    # (substituted pred index, pred index whose token the target lacks, pred index in front of which the target has one more token)
    plans = {distinct[0]: (2, 5, 9), distinct[1]: (3, 6, None)}     # None: the extra token comes after the row's last token
    targets, hand = [], torch.zeros(seqs.shape, dtype=torch.float32)
    for i, r in enumerate(rows):
        if i not in plans:
            targets.append(r.clone())
            continue
        a, b, c = plans[i]
        L = len(r)
        t = r.tolist()
        t[a] = 250 + i                                     # an id no row holds (the vocabulary ends below it)
        c_at = L if c is None else c
        t = t[:b] + t[b + 1:c_at] + [260 + i] + t[c_at:]
        targets.append(torch.tensor(t))
        hand[i, a] += 1
        hand[i, b] += 1
        hand[i, min(c_at, L - 1)] += 1
    got = diagnosed_inference(m, fx["imgs"], targets, "cuda", max_inference_len=n)
    _same(got[:3], (seqs, lps, mask))
    conf, al = got[3], got[4]
    _check(al, _want([r.numpy() for r in rows], [t.numpy() for t in targets], seqs.shape[1], max(len(t) for t in targets)), "edited targets")
    for i, (a, b, c) in plans.items():
        L = len(rows[i])
        op = al.pred_op[i, :L].cpu().tolist()
        assert [k for k, x in enumerate(op) if x == SUB] == [a] and [k for k, x in enumerate(op) if x == INS] == [b]
        assert al.counts[i].cpu().tolist() == [L - 2, 1, 1, 1]
        j = (L if c is None else c) - 1                    # the added token's index in the target: one token was removed in front of it
        t2p = al.tgt_to_pred[i, :len(targets[i])].cpu().tolist()
        assert [k for k, x in enumerate(t2p) if x < 0] == [j] and int(al.tgt_slot[i, j]) == (L if c is None else c)
    bd = symbol_error_breakdown(seqs, mask, targets)
    _same(bd.alignment, al)
    total = sum(len(t) for t in targets)
    assert (bd.sub_rate, bd.ins_rate, bd.del_rate) == (2 / total, 2 / total, 2 / total) and bd.ser == 6 / total
    cf = token_confusions(al, seqs, targets, vocab_size=300)
    assert sorted(cf.insertions) == sorted((int(rows[i][b]), 1) for i, (a, b, c) in plans.items())
    assert sorted(cf.deletions) == sorted((260 + i, 1) for i in plans)
    assert sorted(cf.substitutions) == sorted((250 + i, int(rows[i][a]), 1) for i, (a, b, c) in plans.items())
    # the heat map: uncertainty_maps on the same memory rows with the hand-built weight
    mem, lmask = _padded_memory(m, fx["imgs"])
    with torch.no_grad(), autocast(device_type="cuda", dtype=BF):
        want = m.uncertainty_maps(mem, lmask, seqs, mask, weight=hand.to(dev), grids=_grids(fx), return_alignment=True)
        maps, al2 = m.error_maps(mem, lmask, seqs, mask, targets, grids=_grids(fx), return_alignment=True)
    _same(al2, al)
    for u, v, w in zip(conf.uncertainty, maps.uncertainty, want.uncertainty):
        assert torch.equal(v, w) and torch.equal(u, w)
    assert torch.equal(conf.alignment.patch, want.alignment.patch)
    assert torch.equal(torch.nan_to_num(conf.log_prob, nan=7.0), torch.nan_to_num(want.log_prob, nan=7.0))
    for i in plans:       # the maps' rows sum to 1: an image's heat adds up to its three errors; an untouched row stays dark
        assert abs(float(conf.uncertainty[i].double().sum()) - 3.0) <= 0.02 * 3.0
    for i in set(range(len(rows))) - set(plans):
        assert float(conf.uncertainty[i].abs().max()) == 0.0
    # the statistic runs on the pass's own scores and labels (its value on an untrained toy model means nothing: only that it is one)
    auc = confidence_error_auroc(1.0 - torch.exp(conf.log_prob), al.pred_op != 0, mask & ~torch.isnan(conf.log_prob))
    assert 0.0 <= auc <= 1.0


def test_ser_validation_breakdown(dev):
    from acai_omr_amd.train.loops import ser_validation
    from acai_omr_amd.utils import symbol_error_breakdown
    fx, m, seqs, lps, mask, rows = _decoded(dev)
    n = fx["cfg"]["gen_len"]
    g = torch.Generator().manual_seed(4)
    targets = [torch.randint(0, 227, (k,), generator=g) for k in (10, 4, 12)]
    targets[1] = torch.cat([rows[1][:6], targets[1]])      # (something to match, so that all three kinds occur)
    loader = [[(fx["imgs"][0], targets[0]), (fx["imgs"][1], targets[1])], [(fx["imgs"][2], targets[2])]]
    plain = ser_validation(m, loader, "cuda", max_inference_len=n)
    bd = ser_validation(m, loader, "cuda", max_inference_len=n, breakdown=True)
    assert set(bd) == {"ser", "sub_rate", "ins_rate", "del_rate"} and bd["ser"] == plain and plain > 0
    whole = symbol_error_breakdown(seqs, mask, targets)
    assert (bd["ser"], bd["sub_rate"], bd["ins_rate"], bd["del_rate"]) == whole[:4]
    want = sum(edit_distance(r.numpy(), t.numpy()) for r, t in zip(rows, targets)) / sum(len(t) for t in targets)
    assert plain == want
