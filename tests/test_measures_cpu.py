"""The float64 restatement of the per-measure results (tests/measures_reference.py) against brute-force loops written a second way, its
invariants, and the host-side argument checks that need no GPU."""
import math

import numpy as np
import pytest
import torch

import edit_alignment_reference as EA
import measures_reference as R


def _rows(rng, R_, ld, delims, stop, p_delim=0.25, p_stop=0.05):
    t = rng.integers(20, 40, size=(R_, ld)).astype(np.int64)
    t[rng.random((R_, ld)) < p_delim] = rng.choice(delims)
    if stop >= 0:
        t[rng.random((R_, ld)) < p_stop] = stop
    return t


@pytest.mark.parametrize("seed", range(6))
def test_token_segments_against_a_second_statement(seed):
    rng = np.random.default_rng(seed)
    delims, stop, cap = [3, 7], (2 if seed % 2 else -1), 5
    ld = int(rng.integers(1, 40))
    t = _rows(rng, 9, ld, delims, stop)
    lens = rng.integers(-2, ld + 4, size=9)
    seg, count, bounds = R.token_segments(t, lens, delims, stop, cap)
    for r in range(9):
        row = t[r, :min(max(int(lens[r]), 0), ld)].tolist()
        if stop in row:
            row = row[:row.index(stop)]
        E = len(row)
        is_d = np.isin(np.array(row, dtype=np.int64), delims)
        want = np.full(ld, -1)
        want[:E] = np.cumsum(is_d) - 1
        assert seg[r].tolist() == want.tolist()
        assert count[r] == int(is_d.sum())
        # the segments partition [first delimiter, E)
        n = min(int(count[r]), cap)
        if count[r]:
            assert bounds[r, 0, 0] == int(np.argmax(is_d))
        for m in range(n):
            a, b = bounds[r, m]
            assert a < b and bool((seg[r, a:b] == m).all()) and is_d[a] and not is_d[a + 1:b].any()
            assert b == (bounds[r, m + 1, 0] if m + 1 < n else (E if count[r] <= cap else int(np.flatnonzero(is_d)[cap])))
        assert bool((bounds[r, n:] == -1).all())


def test_segment_reduce_against_loops():
    rng = np.random.default_rng(3)
    t = _rows(rng, 5, 70, [3], -1)
    _, count, bounds = R.token_segments(t, [70, 0, 33, 70, 1], [3], -1, 6)
    v = rng.integers(-8, 9, size=(2, 5, 70)) / 4.0      # ties are common
    s, lo, hi, alo, ahi = R.segment_reduce(v, bounds, count)
    for k in range(2):
        for r in range(5):
            for m in range(6):
                if m >= min(count[r], 6):
                    assert s[k, r, m] == 0 and alo[k, r, m] == -1 and ahi[k, r, m] == -1
                    continue
                a, b = bounds[r, m]
                best = min(range(a, b), key=lambda p: (v[k, r, p], p))
                top = min(range(a, b), key=lambda p: (-v[k, r, p], p))
                assert (alo[k, r, m], ahi[k, r, m]) == (best, top) and lo[k, r, m] == v[k, r, best] and hi[k, r, m] == v[k, r, top]
                assert s[k, r, m] == sum(v[k, r, a:b])


def test_extent_of_a_uniform_map_and_edges():
    for h, w, q in ((4, 8, 0.05), (16, 32, 0.25), (1, 7, 0.0), (5, 1, 0.1)):
        e = R.extent(np.full(h * w, 0.5), w, q)
        assert np.allclose(e, [q * w, q * h, (1 - q) * w, (1 - q) * h], atol=1e-12), (h, w, q, e)
    p = np.zeros(6 * 5)
    p[2 * 5 + 1] = p[3 * 5 + 3] = 1.0
    assert R.extent(p, 5, 0.0).tolist() == [1.0, 2.0, 4.0, 4.0]        # q = 0: the outer edges of the non-zero cells
    assert R.extent(np.zeros(12), 4, 0.1).tolist() == [0, 0, 0, 0]
    e = R.extent(np.ones(10), 4, 0.0)                                   # a last partial grid row: 4 + 4 + 2
    assert e.tolist() == [0.0, 0.0, 4.0, 3.0]
    assert np.allclose(R.extent(np.ones(10), 4, 0.25), [2.5 / 3, 0.625, 2.75, 1.875])   # columns hold 3, 3, 2, 2


def test_segment_sum_is_a_weighted_sum_over_the_range():
    rng = np.random.default_rng(5)
    maps = [rng.random((7, 9)), rng.random((3, 4))]
    w = [rng.random(7), rng.random(3)]
    out, mag = R.attn_map_segment_sum(maps, w, [[(0, 7), (2, 3)], []])
    assert np.allclose(out[0][0], w[0] @ maps[0]) and np.allclose(out[0][1], w[0][2] * maps[0][2]) and out[1].shape == (0, 4)
    assert np.allclose(mag[0][0], out[0][0])


def _edit(rng, row, V):
    out = []
    for t in row:
        u = rng.random()
        if u < 0.1:
            continue
        out.append(int(rng.integers(0, V)) if u < 0.2 else int(t))
        if u > 0.9:
            out.append(int(rng.integers(0, V)))
    return out


@pytest.mark.parametrize("seed", range(5))
def test_error_sums_equal_the_alignments_counts(seed):
    """errors.sum(1) + outside_errors == counts[:, 1:] for the report's rule, and measure_accuracy's rule charges every error at most once."""
    rng = np.random.default_rng(seed)
    V, B = 6, 4
    tg = [rng.integers(0, V, size=int(rng.integers(1, 30))).tolist() for _ in range(B)]
    pr = [_edit(rng, t, V) or [0] for t in tg]
    Lp, Lt = max(map(len, pr)), max(map(len, tg))
    pred, tgt = np.zeros((B, Lp), dtype=np.int64), np.zeros((B, Lt), dtype=np.int64)
    for i in range(B):
        pred[i, :len(pr[i])], tgt[i, :len(tg[i])] = pr[i], tg[i]
    al = EA.edit_alignments(pred, [len(p) for p in pr], tgt, [len(t) for t in tg])
    counts, pred_op, pred_to_tgt, tgt_to_pred, tgt_slot = (np.asarray(a) for a in al)
    seg, count, _ = R.token_segments(pred, [len(p) for p in pr], [0, 1], -1, 64)
    errors, outside = R.report_errors(seg, pred_op, tgt_to_pred, tgt_slot, np.minimum(count, 64))
    assert (errors.sum(1) + outside == counts[:, 1:]).all()
    tseg, tcount, _ = R.token_segments(tgt, [len(t) for t in tg], [0, 1], -1, 64)
    acc, good, total = R.measure_accuracy(tseg, tcount, pred_op, pred_to_tgt, tgt_to_pred, tgt_slot)
    assert (good >= np.maximum(total - counts[:, 1:].sum(1), 0)).all() and (good <= total).all()
    own = [np.asarray(a) for a in EA.edit_alignments(tgt, [len(t) for t in tg], tgt, [len(t) for t in tg])]
    same = R.measure_accuracy(tseg, tcount, *own[1:])
    assert (same[1] == total).all() and (same[0] == 1.0 or total.sum() == 0)


def test_measure_accuracy_hand_made_rows():
    M, a, b, c = 3, 10, 11, 12
    cases = [([M, a, b, M, c], [M, a, b, M, c], 2, 2),       # perfect
             ([M, a, c, M, c], [M, a, b, M, c], 1, 2),       # an error in one measure
             ([M, a, b, c], [M, a, b, M, c], 1, 2),          # a missing delimiter: the measure it would have opened is wrong
             ([M, a, M, b, M, c], [M, a, b, M, c], 1, 2),    # an extra measure: charged to the measure before it
             ([a, M, b], [c, M, b], 1, 1)]                   # an error before the first delimiter counts in no measure
    for pred, tgt, good, total in cases:
        al = EA.edit_alignments(np.array([pred]), [len(pred)], np.array([tgt]), [len(tgt)])
        tseg, tcount, _ = R.token_segments(np.array([tgt]), [len(tgt)], [M], -1, 8)
        acc, g, t = R.measure_accuracy(tseg, tcount, *(np.asarray(x) for x in al[1:]))
        assert (int(g[0]), int(t[0])) == (good, total) and acc == good / total, (pred, tgt, g, t)


def test_config_and_host_checks():
    from acai_omr_amd import ops
    from acai_omr_amd.measures import MeasureConfig
    cfg = MeasureConfig()
    assert cfg.delimiters == ("measure",) and cfg.quantile == 0.05 and cfg.weight is None and cfg.max_measures == 256 and not cfg.return_maps
    for bad in (dict(delimiters=()), dict(delimiters=list(range(9))), dict(delimiters=(1.5,)), dict(quantile=0.5), dict(quantile=-0.1),
                dict(weight="error"), dict(weight=torch.zeros(3)), dict(max_measures=0), dict(max_measures=True)):
        with pytest.raises(ValueError):
            MeasureConfig(**bad)

    class Dec:
        tokens_to_idxs = {"measure": 3}
        vocab_size = 10
    assert cfg.resolve(Dec) == [3] and MeasureConfig(delimiters=(4, "measure")).resolve(Dec) == [4, 3]
    for bad in (("bar",), (10,), (-1,)):
        with pytest.raises(ValueError):
            MeasureConfig(delimiters=bad).resolve(Dec)
    with pytest.raises(ValueError):
        MeasureConfig(weight=torch.zeros(2, 3)).resolve(Dec, (2, 4))
    # no CPU fallback
    t = torch.zeros(2, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError):
        ops.token_segments(t, torch.zeros(2, dtype=torch.int32), [3])
    with pytest.raises(RuntimeError):
        ops.segment_reduce(torch.zeros(1, 2, 4), torch.zeros(2, 3, 2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        ops.attn_map_extent(torch.zeros(8), torch.zeros(1, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), [2], 0.1)
    with pytest.raises(RuntimeError):
        ops.attn_map_segment_sum(torch.zeros(8), torch.zeros(1, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32),
                                 None, torch.zeros(1, 2, dtype=torch.int32), [1])


def test_measure_boxes_are_the_report_boxes_taken_to_the_page():
    """page.measure_boxes against PageResult.to_page_xy on a hand-made result (a turned page, a shifted window) and a stub report: four
    corners per measure, rows past `count` cut, a NaN box gives None, a report of another size is refused."""
    from types import SimpleNamespace
    from acai_omr_amd import page as pg
    boxes = [[(10, 20, 110, 60), (10, 100, 210, 140)], [(0, 0, 64, 32)]]
    res = pg.PageResult(boxes, None, None, None, [0, 0, 1], [(32, 128)] * 3, [(0, 0, 32, 128), (0, 8, 32, 112), (0, 0, 32, 128)],
                        angles=[2.0, 0.0], page_sizes=[(200, 300), (40, 80)])
    nan = float("nan")
    box_px = torch.tensor([[[1.0, 2.0, 30.5, 16.0], [31.0, 0.0, 127.0, 32.0], [5.0, 5.0, 6.0, 6.0]],       # the third lies past count = 2
                           [[0.0, 0.0, 112.0, 32.0], [nan] * 4, [8.0, 4.0, 16.0, 12.0]],
                           [[nan] * 4] * 3])
    report = SimpleNamespace(box_px=box_px, count=torch.tensor([2, 3, 0]))
    got = pg.measure_boxes(res, report)
    assert [len(g) for g in got] == [2, 3, 0] and got[1][1] is None
    for s, m in ((0, 0), (0, 1), (1, 0), (1, 2)):
        x0, y0, x1, y1 = box_px[s, m].tolist()
        assert got[s][m] == [res.to_page_xy(s, x, y) for x, y in ((x0, y0), (x1, y0), (x1, y1), (x0, y1))]
    # page 0 was turned by 2 degrees: its quads are not axis-parallel, and the turn (quantised as the kernel's) keeps lengths
    (ax, ay), (bx, by) = got[0][0][0], got[0][0][1]
    assert ay != by and abs(math.hypot(bx - ax, by - ay) - (30.5 - 1.0) * (110 - 10) / 128) < 1e-3
    with pytest.raises(ValueError, match="measure_boxes"):
        pg.measure_boxes(res, SimpleNamespace(box_px=box_px[:2], count=torch.tensor([2, 3])))
