"""Canonical edit alignment on the CPU: the yardstick of tests/test_edit_alignment_cpu.py and tests/test_gpu_edit_alignment.py and the CPU side of
tools/bench_edit_alignment.py.

The FULL Levenshtein table D[i][j] (pred prefix i, target prefix j; numpy, one row at a time as in edit_distance_reference.py, every row kept)
and the traceback of the contract, word for word.  Start at (lp, lt); at (i, j):
  1. if i > 0, j > 0 and D[i-1][j-1] + [pred[i-1] != tgt[j-1]] == D[i][j]: step diagonally (match or substitution);
  2. otherwise, if i > 0 and D[i-1][j] + 1 == D[i][j]: insertion (pred token i-1 is extra);
  3. otherwise: deletion (target token j-1 is missing).
Nothing here is shared with the device kernel (no direction bits, no strips, no skew, no orientation swap)."""
import numpy as np

MATCH, SUB, INS = 0, 1, 2


def edit_table(pred, tgt):
    """D as an int32 (lp + 1, lt + 1) array."""
    pred = np.asarray(pred, dtype=np.int64).reshape(-1)
    tgt = np.asarray(tgt, dtype=np.int64).reshape(-1)
    ar = np.arange(tgt.shape[0] + 1, dtype=np.int32)
    D = np.empty((pred.shape[0] + 1, tgt.shape[0] + 1), dtype=np.int32)
    D[0] = ar
    for i in range(pred.shape[0]):
        cand = np.empty_like(ar)
        cand[0] = i + 1
        cand[1:] = np.minimum(D[i, 1:] + 1, D[i, :-1] + (tgt != pred[i]))
        D[i + 1] = np.minimum.accumulate(cand - ar) + ar
    return D


def edit_alignment(pred, tgt, ld_pred=None, ld_tgt=None):
    """(counts (4,) = matches, substitutions, insertions, deletions; pred_op (ld_pred,) int8; pred_to_tgt (ld_pred,); tgt_to_pred (ld_tgt,);
    tgt_slot (ld_tgt,)) int32 of one pair, padded with -1 to the given widths (default: the rows' lengths)."""
    pred = np.asarray(pred, dtype=np.int64).reshape(-1)
    tgt = np.asarray(tgt, dtype=np.int64).reshape(-1)
    lp, lt = pred.shape[0], tgt.shape[0]
    D = edit_table(pred, tgt)
    op = np.full(lp if ld_pred is None else ld_pred, -1, dtype=np.int8)
    p2t = np.full(op.shape[0], -1, dtype=np.int32)
    t2p = np.full(lt if ld_tgt is None else ld_tgt, -1, dtype=np.int32)
    slot = np.full(t2p.shape[0], -1, dtype=np.int32)
    counts = np.zeros(4, dtype=np.int32)
    i, j = lp, lt
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i - 1, j - 1] + (pred[i - 1] != tgt[j - 1]) == D[i, j]:
            kind = SUB if pred[i - 1] != tgt[j - 1] else MATCH
            op[i - 1], p2t[i - 1], t2p[j - 1], slot[j - 1] = kind, j - 1, i - 1, i - 1
            counts[kind] += 1
            i, j = i - 1, j - 1
        elif i > 0 and D[i - 1, j] + 1 == D[i, j]:
            op[i - 1], p2t[i - 1] = INS, -1
            counts[2] += 1
            i -= 1
        else:
            t2p[j - 1], slot[j - 1] = -1, i
            counts[3] += 1
            j -= 1
    return counts, op, p2t, t2p, slot


def edit_alignment_transposed_rule(tgt, pred):
    """The same alignment computed on the TRANSPOSED table E[j][i] = D[i][j] (rows over the target) with the rule transposed with it: diagonal
    first, then the LEFT neighbour E[j][i-1] (pred token extra), then the upper one.  Returns what edit_alignment(pred, tgt) returns."""
    pred = np.asarray(pred, dtype=np.int64).reshape(-1)
    tgt = np.asarray(tgt, dtype=np.int64).reshape(-1)
    lp, lt = pred.shape[0], tgt.shape[0]
    E = edit_table(tgt, pred)
    op, p2t = np.full(lp, -1, dtype=np.int8), np.full(lp, -1, dtype=np.int32)
    t2p, slot = np.full(lt, -1, dtype=np.int32), np.full(lt, -1, dtype=np.int32)
    counts = np.zeros(4, dtype=np.int32)
    j, i = lt, lp
    while i > 0 or j > 0:
        if i > 0 and j > 0 and E[j - 1, i - 1] + (pred[i - 1] != tgt[j - 1]) == E[j, i]:
            kind = SUB if pred[i - 1] != tgt[j - 1] else MATCH
            op[i - 1], p2t[i - 1], t2p[j - 1], slot[j - 1] = kind, j - 1, i - 1, i - 1
            counts[kind] += 1
            i, j = i - 1, j - 1
        elif i > 0 and E[j, i - 1] + 1 == E[j, i]:
            op[i - 1] = INS
            counts[2] += 1
            i -= 1
        else:
            slot[j - 1] = i
            counts[3] += 1
            j -= 1
    return counts, op, p2t, t2p, slot


def edit_alignments(pred, pred_len, tgt, tgt_len, group=1):
    """The device op's contract on padded arrays: (counts (R, 4), pred_op (R, Lp) int8, pred_to_tgt (R, Lp), tgt_to_pred (R, Lt), tgt_slot (R, Lt))
    for pred[r, :pred_len[r]] against tgt[r // group, :tgt_len[r // group]], lengths clamped to the widths."""
    pred, tgt = np.asarray(pred), np.asarray(tgt)
    R, Lp, Lt = pred.shape[0], pred.shape[1], tgt.shape[1]
    out = (np.zeros((R, 4), np.int32), np.full((R, Lp), -1, np.int8), np.full((R, Lp), -1, np.int32), np.full((R, Lt), -1, np.int32),
           np.full((R, Lt), -1, np.int32))
    for r in range(R):
        lp, lt = min(max(int(pred_len[r]), 0), Lp), min(max(int(tgt_len[r // group]), 0), Lt)
        for dst, src in zip(out, edit_alignment(pred[r, :lp], tgt[r // group, :lt], Lp, Lt)):
            dst[r] = src
    return out


def replay(pred, pred_op, pred_to_tgt, tgt_to_pred, tgt, lt):
    """Apply the alignment's edits to pred: keep matched tokens, replace substituted ones by their target token, drop inserted ones and put the
    deleted target tokens where they belong - target order is the order of the result.  Returns the rebuilt target as a list."""
    out = []
    for j in range(lt):
        i = int(tgt_to_pred[j])
        if i < 0:
            out.append(int(tgt[j]))                       # deleted: re-inserted
        elif pred_op[i] == MATCH:
            out.append(int(pred[i]))                      # kept as it is
        else:
            assert pred_op[i] == SUB and pred_to_tgt[i] == j
            out.append(int(tgt[j]))                       # substituted
    return out
