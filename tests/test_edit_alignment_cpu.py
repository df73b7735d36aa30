"""CPU checks of the canonical edit alignment reference (tests/edit_alignment_reference.py) that the GPU tests compare against, and of the host
arithmetic built on ops.edit_alignment - utils.symbol_error_breakdown, utils.token_confusions, the error-map weight, ser_validation's breakdown -
with the device op replaced by that reference; and utils.confidence_error_auroc against a count over all (error, match) pairs."""
import math
import types

import numpy as np
import pytest
import torch

from edit_alignment_reference import INS, MATCH, SUB, edit_alignment, edit_alignment_transposed_rule, edit_alignments, replay
from edit_distance_reference import edit_distance, edit_distances


def _s(word):
    return [ord(c) for c in word]


def _lists(al):
    return [x.tolist() for x in al]


def test_hand_known_cases():
    # kitten -> sitting: s/k, i/e substituted, g added at the end of the target (a deletion in front of pred index 6 = past the end)
    counts, op, p2t, t2p, slot = _lists(edit_alignment(_s("kitten"), _s("sitting")))
    assert counts == [4, 2, 0, 1]
    assert op == [SUB, MATCH, MATCH, MATCH, SUB, MATCH] and p2t == [0, 1, 2, 3, 4, 5]
    assert t2p == [0, 1, 2, 3, 4, 5, -1] and slot == [0, 1, 2, 3, 4, 5, 6]
    # the other way round the g is an extra pred token
    counts, op, p2t, t2p, slot = _lists(edit_alignment(_s("sitting"), _s("kitten")))
    assert counts == [4, 2, 1, 0] and op == [SUB, MATCH, MATCH, MATCH, SUB, MATCH, INS] and p2t == [0, 1, 2, 3, 4, 5, -1]
    assert t2p == [0, 1, 2, 3, 4, 5] and slot == [0, 1, 2, 3, 4, 5]
    # an empty row on either side, and on both
    counts, op, p2t, t2p, slot = _lists(edit_alignment([], [4, 5, 6]))
    assert counts == [0, 0, 0, 3] and op == [] and p2t == [] and t2p == [-1, -1, -1] and slot == [0, 0, 0]
    counts, op, p2t, t2p, slot = _lists(edit_alignment([4, 5, 6], []))
    assert counts == [0, 0, 3, 0] and op == [INS] * 3 and p2t == [-1] * 3 and t2p == [] and slot == []
    assert _lists(edit_alignment([], [])) == [[0, 0, 0, 0], [], [], [], []]
    # identical rows
    row = [5, 3, 3, 9, 1, 200, 7]
    counts, op, p2t, t2p, slot = _lists(edit_alignment(row, row))
    assert counts == [7, 0, 0, 0] and op == [MATCH] * 7 and p2t == list(range(7)) and t2p == list(range(7)) and slot == list(range(7))
    # one pure insertion (pred index 3 is extra), one pure deletion (target index 3 is missing in front of pred index 3), one pure substitution
    counts, op, p2t, t2p, slot = _lists(edit_alignment([1, 2, 3, 99, 4, 5], [1, 2, 3, 4, 5]))
    assert counts == [5, 0, 1, 0] and op == [0, 0, 0, INS, 0, 0] and p2t == [0, 1, 2, -1, 3, 4] and t2p == [0, 1, 2, 4, 5] and slot == [0, 1, 2, 4, 5]
    counts, op, p2t, t2p, slot = _lists(edit_alignment([1, 2, 3, 4, 5], [1, 2, 3, 99, 4, 5]))
    assert counts == [5, 0, 0, 1] and op == [0] * 5 and p2t == [0, 1, 2, 4, 5] and t2p == [0, 1, 2, -1, 3, 4] and slot == [0, 1, 2, 3, 3, 4]
    counts, op, p2t, t2p, slot = _lists(edit_alignment([1, 2, 3, 4, 5], [1, 2, 99, 4, 5]))
    assert counts == [4, 1, 0, 0] and op == [0, 0, SUB, 0, 0] and p2t == list(range(5)) and t2p == list(range(5))
    # padded widths hold -1 past the lengths ((2, 1): the diagonal would cost 2, dropping pred token 1 costs 1)
    counts, op, p2t, t2p, slot = _lists(edit_alignment([1, 2], [1], ld_pred=4, ld_tgt=3))
    assert op == [MATCH, INS, -1, -1] and p2t == [0, -1, -1, -1] and t2p == [0, -1, -1] and slot == [0, -1, -1]


def test_ties_follow_the_stated_priority():
    """Co-optimal paths: the diagonal first, then the insertion, then the deletion, walking back from the ends."""
    # x x x x against x x x: every pred token could be the extra one; walking back, the matches are taken first, so it is the FIRST
    counts, op, p2t, t2p, slot = _lists(edit_alignment([7, 7, 7, 7], [7, 7, 7]))
    assert op == [INS, MATCH, MATCH, MATCH] and t2p == [1, 2, 3]
    counts, op, p2t, t2p, slot = _lists(edit_alignment([7, 7, 7], [7, 7, 7, 7]))
    assert op == [MATCH] * 3 and t2p == [-1, 0, 1, 2] and slot == [0, 0, 1, 2]
    # a b against b a: two substitutions (diagonal) rather than an insertion and a deletion of equal cost
    counts, op, p2t, t2p, slot = _lists(edit_alignment([1, 2], [2, 1]))
    assert counts == [0, 2, 0, 0] and op == [SUB, SUB]
    # a b against c a: two substitutions tie with deleting c and dropping b; the diagonal wins at (2, 2) and again at (1, 1)
    counts, op, p2t, t2p, slot = _lists(edit_alignment([1, 2], [3, 1]))
    assert counts == [0, 2, 0, 0]
    # where the diagonal does not attain the minimum, an insertion is preferred to a deletion: a b c against c: D = 2 = drop a, b
    counts, op, p2t, t2p, slot = _lists(edit_alignment([1, 2, 3], [3]))
    assert op == [INS, INS, MATCH] and t2p == [2]


def _random_pair(rng, hi=60):
    vocab = int(rng.choice([2, 3, 5, 227]))
    return rng.integers(0, vocab, size=int(rng.integers(0, hi))), rng.integers(0, vocab, size=int(rng.integers(0, hi)))


def test_transposed_rule_gives_the_mirrored_alignment():
    """The table transposed (rows over the target) with the rule transposed with it - diagonal, then the LEFT neighbour (one pred token fewer),
    then the upper one - names the same alignment: the device kernel runs in whichever orientation puts the longer row along its lanes, and
    what the contract fixes is a path, not a table layout.  The two sides of the result mirror each other: pred_to_tgt and tgt_to_pred pair
    the same tokens."""
    rng = np.random.default_rng(4321)
    for _ in range(200):
        a, b = _random_pair(rng)
        want = _lists(edit_alignment(a, b))
        assert _lists(edit_alignment_transposed_rule(b, a)) == want
        # the mirror: matches / substitutions pair the same tokens from the other side
        counts, op, p2t, t2p, slot = want
        for i, j in enumerate(p2t):
            assert (j == -1) == (op[i] == INS)
            if j >= 0:
                assert t2p[j] == i
        assert sum(1 for i in t2p if i >= 0) == counts[0] + counts[1]


def test_invariants_on_random_pairs():
    rng = np.random.default_rng(99)
    for _ in range(300):
        a, b = _random_pair(rng)
        lp, lt = len(a), len(b)
        counts, op, p2t, t2p, slot = edit_alignment(a, b)
        m, s, i, d = counts.tolist()
        assert m + s + i == lp and m + s + d == lt
        assert s + i + d == edit_distance(a, b)
        assert (op == MATCH).sum() == m and (op == SUB).sum() == s and (op == INS).sum() == i and (t2p < 0).sum() == d
        assert replay(a, op, p2t, t2p, b, lt) == b.tolist()
        for x in range(lp):
            if op[x] == MATCH:
                assert a[x] == b[p2t[x]]
            elif op[x] == SUB:
                assert a[x] != b[p2t[x]]
        aligned = p2t[p2t >= 0]
        assert np.all(np.diff(aligned) > 0)                       # the pairs keep both orders
        assert np.all(np.diff(slot) >= 0) and (lt == 0 or (slot.min() >= 0 and slot.max() <= lp))
        for j in range(lt):
            if t2p[j] >= 0:
                assert slot[j] == t2p[j]
    # the batched form: groups, padded widths, clamped lengths
    pred = rng.integers(0, 3, size=(6, 20))
    tgt = rng.integers(0, 3, size=(2, 17))
    pl, tl = [0, 5, 20, 33, 7, -2], [17, 9]
    counts, op, p2t, t2p, slot = edit_alignments(pred, pl, tgt, tl, group=3)
    assert counts[:, 1:].sum(1).tolist() == edit_distances(pred, [0, 5, 20, 20, 7, 0], tgt, tl, group=3)
    assert op.shape == (6, 20) and t2p.shape == (6, 17) and (op[1, 5:] == -1).all() and (t2p[3:, 9:] == -1).all() and (slot[3:, 9:] == -1).all()


# ---- what is built on the op, with the op replaced by the reference ------------------------------------------------------------------------
def _fake_alignment(pred, pred_len, tgt, tgt_len, group=1, out=None, workspace=None):
    from acai_omr_amd import ops
    pl = pred_len.sum(-1) if pred_len.dtype == torch.bool else pred_len
    tl = tgt_len.sum(-1) if tgt_len.dtype == torch.bool else tgt_len
    return ops.EditAlignment(*(torch.from_numpy(x) for x in edit_alignments(pred.numpy(), pl.tolist(), tgt.numpy(), tl.tolist(), group)))


@pytest.fixture
def reference_op(monkeypatch):
    """ops.edit_alignment and ops.edit_distance replaced by the CPU references (bool masks summed as the ops sum them)."""
    from acai_omr_amd import ops

    def fake_distance(pred, pred_len, tgt, tgt_len, group=1, out=None):
        pl = pred_len.sum(-1) if pred_len.dtype == torch.bool else pred_len
        tl = tgt_len.sum(-1) if tgt_len.dtype == torch.bool else tgt_len
        return torch.tensor(edit_distances(pred.numpy(), pl.tolist(), tgt.numpy(), tl.tolist(), group), dtype=torch.int32)
    monkeypatch.setattr(ops, "edit_alignment", _fake_alignment)
    monkeypatch.setattr(ops, "edit_distance", fake_distance)


def _decoded():
    pad = 1
    rows = [[0, 7, 8, 9, 2], [0, 7, 7, 2], [0, 5, 6, 4, 3, 2]]
    T = max(len(r) for r in rows)
    seqs = torch.full((len(rows), T), pad, dtype=torch.int64)
    mask = torch.zeros(len(rows), T, dtype=torch.bool)
    for i, r in enumerate(rows):
        seqs[i, :len(r)] = torch.tensor(r)
        mask[i, :len(r)] = True
    return rows, seqs, mask, pad


TARGETS = [[0, 7, 8, 9, 2], [0, 7, 9, 9, 9, 2], [0, 5, 4, 3, 2]]   # row 0 exact; row 1: one substitution, two deletions; row 2: one insertion


def test_symbol_error_breakdown(reference_op):
    from acai_omr_amd.utils import symbol_error_breakdown, symbol_error_rate
    rows, seqs, mask, pad = _decoded()
    bd = symbol_error_breakdown(seqs, mask, [torch.tensor(t) for t in TARGETS])
    assert bd.counts.tolist() == [[5, 0, 0, 0], [3, 1, 0, 2], [5, 0, 1, 0]] and bd.target_lens.tolist() == [5, 6, 5]
    assert (bd.sub_rate, bd.ins_rate, bd.del_rate) == (1 / 16, 1 / 16, 2 / 16) and bd.ser == 4 / 16
    assert bd.ser == symbol_error_rate(seqs, mask, [torch.tensor(t) for t in TARGETS])[0]
    assert bd.alignment.pred_op.tolist()[2] == [0, 0, INS, 0, 0, 0] and bd.alignment.counts is bd.counts
    padded = torch.full((3, 8), pad, dtype=torch.int64)
    for i, t in enumerate(TARGETS):
        padded[i, :len(t)] = torch.tensor(t)
    bd2 = symbol_error_breakdown(seqs, mask, padded, pad_idx=pad)
    assert bd2[:4] == bd[:4] and torch.equal(bd2.counts, bd.counts) and bd2.alignment.tgt_slot.shape == (3, 8)
    with pytest.raises(ValueError):
        symbol_error_breakdown(seqs, mask, padded)
    with pytest.raises(ValueError):
        symbol_error_breakdown(seqs, mask, [torch.tensor(TARGETS[0])])
    # every target empty: the rates are undefined, the counts are all insertions
    bd = symbol_error_breakdown(seqs, mask, torch.full((3, 4), pad, dtype=torch.int64), pad_idx=pad)
    assert all(math.isnan(x) for x in bd[:4]) and bd.counts.tolist() == [[0, 0, 5, 0], [0, 0, 4, 0], [0, 0, 6, 0]]
    # seeded random rows: ser is symbol_error_rate's value, bit for bit
    rng = np.random.default_rng(3)
    p = torch.from_numpy(rng.integers(0, 4, size=(9, 30)))
    t = torch.from_numpy(rng.integers(0, 4, size=(9, 26)))
    pm = torch.arange(30)[None, :] < torch.from_numpy(rng.integers(0, 31, size=9))[:, None]
    tl = rng.integers(0, 27, size=9)
    tl[0] = 26
    tlist = [t[i, :tl[i]] for i in range(9)]
    bd = symbol_error_breakdown(p, pm, tlist)
    assert bd.ser == symbol_error_rate(p, pm, tlist)[0] and abs(bd.ser - (bd.sub_rate + bd.ins_rate + bd.del_rate)) < 1e-12


def test_token_confusions(reference_op):
    from acai_omr_amd import ops
    from acai_omr_amd.utils import token_confusions
    rows, seqs, mask, pad = _decoded()
    targets = [torch.tensor(t) for t in TARGETS]
    tgt = torch.zeros(3, 6, dtype=torch.int64)
    for i, t in enumerate(TARGETS):
        tgt[i, :len(t)] = torch.tensor(t)
    al = ops.edit_alignment(seqs, mask, tgt, torch.tensor([5, 6, 5], dtype=torch.int32))
    conf = token_confusions(al, seqs, targets, vocab_size=10)
    # row 1, [0 7 7 2] against [0 7 9 9 9 2]: one 7 is substituted by a 9 and two 9s are missing; row 2: the 6 is extra
    want = edit_alignment(rows[1], TARGETS[1])
    subs = [(TARGETS[1][want[2][i]], rows[1][i], 1) for i in range(4) if want[1][i] == SUB]
    assert conf.substitutions == subs and len(subs) == 1
    assert conf.deletions == [(9, 2)] and conf.insertions == [(6, 1)]
    assert token_confusions(al, seqs, tgt, vocab_size=10) == conf      # the padded tensor in the place of the list
    # counts add up and the order is by falling count, then rising id, cut at `top`
    rng = np.random.default_rng(17)
    V = 5
    p = torch.from_numpy(rng.integers(0, V, size=(12, 40)))
    t = torch.from_numpy(rng.integers(0, V, size=(12, 37)))
    pl = torch.from_numpy(rng.integers(0, 41, size=12).astype(np.int32))
    tl = torch.from_numpy(rng.integers(0, 38, size=12).astype(np.int32))
    al = ops.edit_alignment(p, pl, t, tl)
    conf = token_confusions(al, p, t, vocab_size=V, top=V * V)
    sub, dele, ins = {}, {}, {}
    for r in range(12):
        for i in range(int(pl[r])):
            if al.pred_op[r, i] == SUB:
                k = (int(t[r, al.pred_to_tgt[r, i]]), int(p[r, i]))
                sub[k] = sub.get(k, 0) + 1
            elif al.pred_op[r, i] == INS:
                ins[int(p[r, i])] = ins.get(int(p[r, i]), 0) + 1
        for j in range(int(tl[r])):
            if al.tgt_to_pred[r, j] < 0:
                dele[int(t[r, j])] = dele.get(int(t[r, j]), 0) + 1
    assert conf.substitutions == sorted(((a, b, c) for (a, b), c in sub.items()), key=lambda x: (-x[2], x[0], x[1]))
    assert conf.deletions == sorted(dele.items(), key=lambda x: (-x[1], x[0])) and conf.insertions == sorted(ins.items(), key=lambda x: (-x[1], x[0]))
    assert sum(c for *_, c in conf.substitutions) == int(al.counts[:, 1].sum()) and sum(c for _, c in conf.deletions) == int(al.counts[:, 3].sum())
    assert token_confusions(al, p, t, vocab_size=V, top=3).substitutions == conf.substitutions[:3]
    with pytest.raises(ValueError):
        token_confusions(al, p, t, vocab_size=V - 1, top=3)     # an id outside the vocabulary takes part in an error
    with pytest.raises(ValueError):
        token_confusions(al, p[:, :-1], t, vocab_size=V)


def test_error_token_weights_and_the_slot_clamp(reference_op):
    """w[i] = [pred_op[i] != 0] + deleted target tokens whose slot, clamped to [1, L - 1], is i - through ViTOMR._error_weights, which is what
    error_maps and diagnosed_inference hand to uncertainty_maps."""
    from acai_omr_amd.models.models import ViTOMR
    stub = types.SimpleNamespace(decoder=types.SimpleNamespace(pos_embedding=torch.zeros(1)))
    pad = 1
    #        index:  0  1  2  3  4  5
    rows = [[0, 7, 8, 9, 2],            # target drops nothing, adds 50 51 in front of <bos> (slot 0 -> 1) and 60 after <eos> (slot 5 -> 4)
            [0, 7, 8, 9, 4, 2],         # 8 substituted, 4 inserted, 70 missing in front of index 3
            [0, 2],                     # everything between is missing: slot 1 three times
            [0, 7, 8, 2]]               # exact
    targets = [[50, 51, 0, 7, 8, 9, 2, 60], [0, 7, 33, 70, 9, 2], [0, 11, 12, 13, 2], [0, 7, 8, 2]]
    seqs = torch.full((4, 7), pad, dtype=torch.int64)
    mask = torch.zeros(4, 7, dtype=torch.bool)
    for i, r in enumerate(rows):
        seqs[i, :len(r)] = torch.tensor(r)
        mask[i, :len(r)] = True
    al, w = ViTOMR._error_weights(stub, seqs, mask, [torch.tensor(t) for t in targets], None)
    assert w.dtype == torch.float32 and w.shape == seqs.shape
    assert al.tgt_slot[0].tolist() == [0, 0, 0, 1, 2, 3, 4, 5] and al.tgt_to_pred[0].tolist() == [-1, -1, 0, 1, 2, 3, 4, -1]
    assert w.tolist() == [[0, 2, 0, 0, 1, 0, 0],
                          [0, 0, 1, 1, 1, 0, 0],
                          [0, 3, 0, 0, 0, 0, 0],
                          [0, 0, 0, 0, 0, 0, 0]]
    assert float(w.sum()) == float(al.counts[:, 1:].sum())     # every error is charged exactly once
    # the padded-tensor form of the targets and the mask-free form (rows end at their first <eos>) give the same weights
    padded = torch.full((4, 9), pad, dtype=torch.int64)
    for i, t in enumerate(targets):
        padded[i, :len(t)] = torch.tensor(t)
    stub.create_inference_mask = lambda s: mask
    al2, w2 = ViTOMR._error_weights(stub, seqs, None, padded, pad)
    assert torch.equal(w2, w) and torch.equal(al2.counts, al.counts)
    with pytest.raises(ValueError):
        ViTOMR._error_weights(stub, seqs, mask, [torch.tensor(targets[0])], None)


def test_ser_validation_breakdown_arithmetic(reference_op, monkeypatch):
    from acai_omr_amd.inference import vitomr_inference
    from acai_omr_amd.train.loops import ser_validation
    from acai_omr_amd.utils import symbol_error_breakdown
    rows, seqs, mask, pad = _decoded()
    targets = [torch.tensor(t) for t in TARGETS]
    batches = {2: (seqs[:2], None, mask[:2]), 1: (seqs[2:], None, mask[2:])}
    monkeypatch.setattr(vitomr_inference, "inference", lambda vitomr, imgs, device, **kw: batches[len(imgs)])
    model = types.SimpleNamespace(eval=lambda: None)
    img = torch.zeros(1, 4, 4)
    loader = [[(img, targets[0]), (img, targets[1])], [(img, targets[2])]]
    plain = ser_validation(model, loader, "cpu")
    bd = ser_validation(model, loader, "cpu", breakdown=True)
    assert isinstance(plain, float) and plain == 4 / 16
    assert bd == {"ser": 4 / 16, "sub_rate": 1 / 16, "ins_rate": 1 / 16, "del_rate": 2 / 16} and bd["ser"] == plain
    whole = symbol_error_breakdown(seqs, mask, targets)
    assert (bd["ser"], bd["sub_rate"], bd["ins_rate"], bd["del_rate"]) == whole[:4]
    empty = [[(img, torch.zeros(0, dtype=torch.int64)), (img, torch.zeros(0, dtype=torch.int64))]]
    assert all(math.isnan(v) for v in ser_validation(model, empty, "cpu", breakdown=True).values()) and math.isnan(ser_validation(model, empty, "cpu"))


def _auroc_brute(score, is_error, mask):
    s, e, k = score.reshape(-1).tolist(), is_error.reshape(-1).tolist(), mask.reshape(-1).tolist()
    pos = [x for x, y, z in zip(s, e, k) if z and y and not math.isnan(x)]
    neg = [x for x, y, z in zip(s, e, k) if z and not y and not math.isnan(x)]
    if not pos or not neg:
        return float("nan")
    return sum(1.0 if a > b else 0.5 if a == b else 0.0 for a in pos for b in neg) / (len(pos) * len(neg))


def test_confidence_error_auroc_against_the_pair_count():
    from acai_omr_amd.utils import confidence_error_auroc
    g = torch.Generator().manual_seed(12)
    for levels in (0, 2, 5):   # 0: continuous scores; otherwise heavily tied ones
        for _ in range(5):
            score = torch.rand(6, 17, generator=g)
            if levels:
                score = torch.floor(score * levels) / levels
            is_error = torch.rand(6, 17, generator=g) < 0.3
            mask = torch.rand(6, 17, generator=g) < 0.8
            score[0, 0] = float("nan")                      # an unscored entry inside the mask is left out
            got, want = confidence_error_auroc(score, is_error, mask), _auroc_brute(score, is_error, mask)
            assert abs(got - want) < 1e-12, (levels, got, want)
    score = torch.tensor([0.1, 0.2, 0.8, 0.9])
    every = torch.ones(4, dtype=torch.bool)
    assert confidence_error_auroc(score, torch.tensor([False, False, True, True]), every) == 1.0
    assert confidence_error_auroc(score, torch.tensor([True, True, False, False]), every) == 0.0
    assert confidence_error_auroc(torch.full((4,), 0.5), torch.tensor([True, False, True, False]), every) == 0.5      # all tied
    assert confidence_error_auroc(torch.tensor([0.0, float("inf"), 1.0]), torch.tensor([False, True, False]), torch.ones(3, dtype=torch.bool)) == 1.0
    # an empty class, by the labels or by the mask
    assert math.isnan(confidence_error_auroc(score, torch.zeros(4, dtype=torch.bool), every))
    assert math.isnan(confidence_error_auroc(score, torch.ones(4, dtype=torch.bool), every))
    assert math.isnan(confidence_error_auroc(score, torch.tensor([True, False, False, False]), torch.tensor([False, True, True, True])))
    assert math.isnan(confidence_error_auroc(score, torch.tensor([True, False, False, False]), torch.zeros(4, dtype=torch.bool)))
