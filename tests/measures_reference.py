"""numpy / float64 restatement of the per-measure results (measures.hip, acai_omr_amd/measures.py, utils.measure_accuracy), written from the
statements in include/acai_omr_hip.h and the docstrings, not from the kernels: plain loops over rows, spans and cells.

THE RULES, in one place.

token_segments: a row of clamped length L ends at E, its first `stop` token (L without one).  c(p) counts the delimiter tokens at indices
<= p.  seg[p] = c(p) - 1 for p < E, -1 from E on; count = c(E - 1); bounds[m] = (index of the m-th delimiter, index of the next or E).

measure report, error assignment (PRED side): a substituted or inserted pred token i counts in seg[i]; a deleted target token with
tgt_slot = s counts in seg[max(s - 1, 0)], the last pred token consumed before it; what lands on -1 goes to outside_errors.

measure_accuracy (TARGET side): the target rows are segmented (no stop token: a row ends at its length).  With tseg the target's segment
index per token: a substitution at pred index i counts in tseg[pred_to_tgt[i]]; a deleted target token j counts in tseg[j]; an inserted pred
token i counts in tseg[j'] with j' = pred_to_tgt of the nearest earlier pred token that is aligned (match or substitution), and nowhere
when there is none.  Errors that land on -1 (before the first delimiter) count in no measure.  A target measure is reproduced when no error
counts in it; the accuracy is reproduced measures / target measures over all rows (NaN without a target measure)."""
import math

import numpy as np


def token_segments(tokens, lens, delims, stop, cap):
    tokens = np.asarray(tokens, dtype=np.int64)
    R, ld = tokens.shape
    seg = np.full((R, ld), -1, dtype=np.int32)
    count = np.zeros(R, dtype=np.int32)
    bounds = np.full((R, cap, 2), -1, dtype=np.int32)
    dset = set(int(d) for d in delims)
    for r in range(R):
        L = min(max(int(lens[r]), 0), ld)
        E = L
        if stop >= 0:
            for p in range(L):
                if int(tokens[r, p]) == stop:
                    E = p
                    break
        starts = [p for p in range(E) if int(tokens[r, p]) in dset]
        c = 0
        for p in range(E):
            if int(tokens[r, p]) in dset:
                c += 1
            seg[r, p] = c - 1
        count[r] = len(starts)
        for m, s in enumerate(starts[:cap]):
            bounds[r, m] = (s, starts[m + 1] if m + 1 < len(starts) else E)
    return seg, count, bounds


def segment_reduce(values, bounds, count):
    """-> (sum float64, min float64, max float64, argmin int32, argmax int32), each (K, R, cap); 0 / -1 past min(count, cap)."""
    values = np.asarray(values, dtype=np.float64)
    K, R, ld = values.shape
    cap = bounds.shape[1]
    s, lo, hi = (np.zeros((K, R, cap), dtype=np.float64) for _ in range(3))
    alo, ahi = (np.full((K, R, cap), -1, dtype=np.int32) for _ in range(2))
    for k in range(K):
        for r in range(R):
            for m in range(min(int(count[r]), cap)):
                a, b = max(int(bounds[r, m, 0]), 0), min(int(bounds[r, m, 1]), ld)
                if a >= b:
                    continue
                span = values[k, r, a:b]
                s[k, r, m] = math.fsum(span.tolist())
                lo[k, r, m], hi[k, r, m] = span.min(), span.max()
                alo[k, r, m], ahi[k, r, m] = a + int(np.argmin(span)), a + int(np.argmax(span))   # numpy: the first of equal values
    return s, lo, hi, alo, ahi


def segment_abs_sums(values, bounds, count):
    """sum |x| and the length per span, (K, R, cap): what the sum's error bar is made of."""
    s = segment_reduce(np.abs(np.asarray(values, dtype=np.float64)), bounds, count)[0]
    n = np.zeros(bounds.shape[:2], dtype=np.int64)
    for r in range(bounds.shape[0]):
        for m in range(min(int(count[r]), bounds.shape[1])):
            n[r, m] = max(min(int(bounds[r, m, 1]), values.shape[2]) - max(int(bounds[r, m, 0]), 0), 0)
    return s, n


def attn_map_segment_sum(maps, weights, ranges):
    """maps: per image a (T, S) array; weights: per image a (T,) array or None; ranges: per image a list of (t0, t1) -> per image (n, S) float64
    and, for the error bar, sum |w p| of the same spans."""
    out, mag = [], []
    for b, (mp, rg) in enumerate(zip(maps, ranges)):
        mp = np.asarray(mp, dtype=np.float64)
        w = np.ones(mp.shape[0]) if weights is None else np.asarray(weights[b], dtype=np.float64)
        o, g = np.zeros((len(rg), mp.shape[1])), np.zeros((len(rg), mp.shape[1]))
        for m, (t0, t1) in enumerate(rg):
            for t in range(t0, t1):
                o[m] += w[t] * mp[t]
                g[m] += np.abs(w[t] * mp[t])
        out.append(o)
        mag.append(g)
    return out, mag


def _pos(a, target):
    c_prev = 0.0
    for i, ai in enumerate(a):
        c = c_prev + ai
        if c >= target and ai > 0:
            return i + (target - c_prev) / ai
        c_prev = c
    return float(len(a))


def marginals(p, gw):
    p = np.asarray(p, dtype=np.float64)
    S = p.shape[0]
    nx, ny = min(gw, S), -(-S // gw)
    full = np.zeros(ny * gw)
    full[:S] = p
    full = full.reshape(ny, gw)
    return full.sum(0)[:nx], full.sum(1)


def extent(p, gw, q):
    """One map row over S patches in rows of gw -> (x0, y0, x1, y1) float64 in patch units."""
    ax, ay = marginals(p, gw)
    out = []
    for a in (ax, ay):
        m = float(a.sum())
        out.append((0.0, 0.0) if not m > 0 else (_pos(a, q * m), _pos(a, (1 - q) * m)))
    return np.array([out[0][0], out[1][0], out[0][1], out[1][1]])


def attn_map_extent(maps, grid_w, q):
    """per image a (T, S) array -> (sum T, 4) float64."""
    rows = [extent(row, gw, q) for mp, gw in zip(maps, grid_w) for row in np.asarray(mp, dtype=np.float64)]
    return np.stack(rows) if rows else np.zeros((0, 4))


def locate(p, gw):
    """acai_attn_map_locate's centroid and spread of one map row: (cx, cy, sx, sy) float64 in patch units."""
    p = np.asarray(p, dtype=np.float64)
    s = np.arange(p.shape[0])
    x, y = s % gw + 0.5, s // gw + 0.5
    m = p.sum()
    if not m > 0:
        return np.zeros(4)
    cx, cy = (p * x).sum() / m, (p * y).sum() / m
    return np.array([cx, cy, math.sqrt((p * (x - cx) ** 2).sum() / m), math.sqrt((p * (y - cy) ** 2).sum() / m)])


def report_errors(seg, pred_op, tgt_to_pred, tgt_slot, cap_count):
    """The report's error assignment for one batch: seg (B, T) as token_segments gives it, the alignment's arrays, cap_count (B,) =
    min(count, cap) -> (errors (B, M, 3) with M = max cap_count, outside (B, 3)): S, I, D."""
    B, T = seg.shape
    M = int(max(cap_count.max(), 0)) if B else 0
    errors, outside = np.zeros((B, M, 3), dtype=np.int64), np.zeros((B, 3), dtype=np.int64)

    def charge(r, where, kind):
        if 0 <= where < cap_count[r]:
            errors[r, where, kind] += 1
        elif where < 0:
            outside[r, kind] += 1

    for r in range(B):
        for i in range(T):
            if pred_op[r, i] in (1, 2):
                charge(r, int(seg[r, i]), int(pred_op[r, i]) - 1)
        for j in range(tgt_slot.shape[1]):
            if tgt_to_pred[r, j] < 0 and tgt_slot[r, j] >= 0:
                charge(r, int(seg[r, min(max(int(tgt_slot[r, j]) - 1, 0), T - 1)]) if T else -1, 2)
    return errors, outside


def measure_accuracy(tseg, tcount, pred_op, pred_to_tgt, tgt_to_pred, tgt_slot):
    """The target-side rule of the module docstring: tseg (N, Lt) / tcount (N,) from token_segments of the targets (cap >= every count) and
    the alignment's arrays -> (accuracy float, reproduced (N,), tcount (N,))."""
    N = tseg.shape[0]
    good = np.zeros(N, dtype=np.int64)
    for r in range(N):
        bad = set()
        last = -1
        for i in range(pred_op.shape[1]):
            op = int(pred_op[r, i])
            if op < 0:
                break
            if op in (0, 1):
                last = int(pred_to_tgt[r, i])
                if op == 1:
                    bad.add(int(tseg[r, last]))
            elif last >= 0:
                bad.add(int(tseg[r, last]))
        for j in range(tseg.shape[1]):
            if tgt_to_pred[r, j] < 0 and tgt_slot[r, j] >= 0:
                bad.add(int(tseg[r, j]))
        good[r] = int(tcount[r]) - len([m for m in bad if m >= 0])
    total = int(np.sum(tcount))
    return (float(good.sum()) / total if total else float("nan")), good, np.asarray(tcount, dtype=np.int64)
