"""Unit-cost Levenshtein distance on the CPU: the yardstick of the edit-distance tests (tests/test_edit_distance_cpu.py,
tests/test_gpu_edit_distance.py) and the CPU side of tools/bench_edit_distance.py.

The textbook two-row dynamic program, D[i][j] = min(D[i-1][j] + 1, D[i][j-1] + 1, D[i-1][j-1] + [a_i != b_j]) with D[i][0] = i and
D[0][j] = j, one numpy row at a time.  The substitution and deletion terms of a row are elementwise in the row above; the insertion term chains
along the row, D[i][j] = min_k<=j (c[k] + j - k) for the elementwise candidates c, which is a running minimum of c[k] - k with j added back:
np.minimum.accumulate(c - arange) + arange.  Nothing here is shared with the device kernel (no diagonal offsets, no strips, no skew)."""
import numpy as np


def edit_distance(a, b):
    """Levenshtein distance between two 1-D integer sequences (lists, numpy arrays or CPU tensors)."""
    a = np.asarray(a, dtype=np.int64).reshape(-1)
    b = np.asarray(b, dtype=np.int64).reshape(-1)
    ar = np.arange(b.shape[0] + 1, dtype=np.int64)
    row = ar.copy()   # D[0][j] = j
    for i in range(a.shape[0]):
        cand = np.empty_like(row)
        cand[0] = i + 1
        cand[1:] = np.minimum(row[1:] + 1, row[:-1] + (b != a[i]))
        row = np.minimum.accumulate(cand - ar) + ar
    return int(row[-1])


def edit_distances(pred, pred_len, tgt, tgt_len, group=1):
    """Row-wise distances of pred[r, :pred_len[r]] to tgt[r // group, :tgt_len[r // group]] as a list of ints (the device op's contract)."""
    pred, tgt = np.asarray(pred), np.asarray(tgt)
    return [edit_distance(pred[r, :int(pred_len[r])], tgt[r // group, :int(tgt_len[r // group])]) for r in range(pred.shape[0])]
