"""CPU checks of the Levenshtein reference (tests/edit_distance_reference.py) that the GPU tests compare against, and of the host arithmetic of
utils.symbol_error_rate with the device op replaced by that reference."""
import math

import numpy as np
import pytest
import torch

from edit_distance_reference import edit_distance, edit_distances


def _s(word):
    return [ord(c) for c in word]


def test_hand_known_cases():
    assert edit_distance(_s("kitten"), _s("sitting")) == 3
    for n in (0, 1, 7, 100):
        assert edit_distance([], list(range(n))) == n
        assert edit_distance(list(range(n)), []) == n
    row = [5, 3, 3, 9, 1, 200, 7]
    assert edit_distance(row, row) == 0
    sub = list(row)
    sub[3] = 10
    assert edit_distance(row, sub) == 1
    # a pure shift by one: drop the first token, append a new last one
    base = list(range(10, 40))
    assert edit_distance(base, base[1:] + [999]) == 2


def test_reference_is_symmetric():
    rng = np.random.default_rng(1234)
    for _ in range(50):
        vocab = int(rng.choice([2, 4, 227]))
        a = rng.integers(0, vocab, size=int(rng.integers(0, 90)))
        b = rng.integers(0, vocab, size=int(rng.integers(0, 90)))
        assert edit_distance(a, b) == edit_distance(b, a)


def test_reference_matches_the_full_table():
    """The vectorised insertion chain against the recurrence written out cell by cell."""
    rng = np.random.default_rng(7)
    for _ in range(30):
        vocab = int(rng.choice([2, 3, 227]))
        a = rng.integers(0, vocab, size=int(rng.integers(0, 40))).tolist()
        b = rng.integers(0, vocab, size=int(rng.integers(0, 40))).tolist()
        D = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
        for i in range(len(a) + 1):
            for j in range(len(b) + 1):
                if i == 0 or j == 0:
                    D[i][j] = i + j
                else:
                    D[i][j] = min(D[i - 1][j] + 1, D[i][j - 1] + 1, D[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
        assert edit_distance(a, b) == D[len(a)][len(b)]


@pytest.fixture
def reference_op(monkeypatch):
    """ops.edit_distance replaced by the CPU reference (bool masks summed as the op sums them), so symbol_error_rate runs without a GPU."""
    from acai_omr_amd import ops

    def fake(pred, pred_len, tgt, tgt_len, group=1, out=None):
        pl = pred_len.sum(-1) if pred_len.dtype == torch.bool else pred_len
        tl = tgt_len.sum(-1) if tgt_len.dtype == torch.bool else tgt_len
        return torch.tensor(edit_distances(pred.numpy(), pl.tolist(), tgt.numpy(), tl.tolist(), group), dtype=torch.int32)
    monkeypatch.setattr(ops, "edit_distance", fake)


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


def test_symbol_error_rate_list_and_padded_targets(reference_op):
    from acai_omr_amd.utils import symbol_error_rate
    rows, seqs, mask, pad = _decoded()
    targets = [[0, 7, 8, 9, 2], [0, 7, 9, 9, 9, 2], [0, 5, 4, 3, 2]]   # distances 0, 3, 1
    want = [edit_distance(r, t) for r, t in zip(rows, targets)]
    assert want == [0, 3, 1]
    ser, dist, lens = symbol_error_rate(seqs, mask, [torch.tensor(t) for t in targets])
    assert dist.tolist() == want and lens.tolist() == [5, 6, 5]
    assert isinstance(ser, float) and ser == sum(want) / 16
    padded = torch.full((3, 8), pad, dtype=torch.int64)
    for i, t in enumerate(targets):
        padded[i, :len(t)] = torch.tensor(t)
    ser2, dist2, lens2 = symbol_error_rate(seqs, mask, padded, pad_idx=pad)
    assert ser2 == ser and torch.equal(dist2, dist) and torch.equal(lens2, lens)
    assert ser2 == float(dist2.sum()) / float(lens2.sum())
    with pytest.raises(ValueError):
        symbol_error_rate(seqs, mask, padded)   # a padded tensor needs its pad_idx


def test_symbol_error_rate_zero_length_targets(reference_op):
    from acai_omr_amd.utils import symbol_error_rate
    rows, seqs, mask, pad = _decoded()
    # one empty target among the rows: it adds its decoded row's length to the distances and nothing to the lengths
    ser, dist, lens = symbol_error_rate(seqs, mask, [torch.tensor(rows[0]), torch.zeros(0, dtype=torch.int64), torch.tensor(rows[2])])
    assert dist.tolist() == [0, 4, 0] and lens.tolist() == [5, 0, 6]
    assert ser == 4 / 11
    # every target empty: no division error, the rate is undefined
    ser, dist, lens = symbol_error_rate(seqs, mask, torch.full((3, 4), pad, dtype=torch.int64), pad_idx=pad)
    assert math.isnan(ser) and dist.tolist() == [5, 4, 6] and lens.tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        symbol_error_rate(seqs, mask, [torch.tensor(rows[0])])   # row counts differ
