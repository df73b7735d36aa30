"""A numpy restatement of the page assessment (csrc/assess.hip, page.choose_staff_scale / assess_pages), written from the definitions in
include/acai_omr_hip.h and the docstrings with plain loops.  Integer results: the tests use equality."""
from fractions import Fraction

import numpy as np

from page_reference import ink_mask


def column_runs(col):
    """The maximal runs of one column of booleans, top to bottom: [(value, length), ...]."""
    out = []
    for v in col:
        v = bool(v)
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return [(v, n) for v, n in out]


def runs(page, ink_threshold=0.5):
    """int64 [3, 256]: closed ink runs, closed paper runs, and closed ink runs with the closed paper run directly under them, by length
    (clamped to 255).  The first and the last run of a column touch row 0 and row H - 1: they are open and not counted."""
    m = ink_mask(page, ink_threshold)
    hist = np.zeros((3, 256), dtype=np.int64)
    for x in range(m.shape[1]):
        r = column_runs(m[:, x])
        for i in range(1, len(r) - 1):
            ink, n = r[i]
            hist[0 if ink else 1, min(n, 255)] += 1
            if ink and i + 1 < len(r) - 1:
                hist[2, min(n + r[i + 1][1], 255)] += 1
    return hist


def levels_of(page):
    """int64 [H, W]: a uint8 value as it is, a float value v as floor(v * 255 + 0.5) in float32, one rounding per operation, clamped."""
    page = np.asarray(page)
    if page.dtype == np.uint8:
        return page.astype(np.int64)
    v = page.astype(np.float32) * np.float32(255.0)
    v = np.floor(v + np.float32(0.5))
    return np.clip(v, 0, 255).astype(np.int64)


def sharpness(page):
    """(stats int64 [3], levels int64 [256]): (sum L, sum L * L, count) of L = 4 p - up - down - left - right over the interior pixels, and
    the histogram of all levels."""
    lv = levels_of(page)
    H, W = lv.shape
    hist = np.zeros(256, dtype=np.int64)
    for v in lv.ravel():
        hist[v] += 1
    s1 = s2 = count = 0
    for y in range(1, H - 1):
        for x in range(1, W - 1):
            L = 4 * int(lv[y, x]) - int(lv[y - 1, x]) - int(lv[y + 1, x]) - int(lv[y, x - 1]) - int(lv[y, x + 1])
            s1 += L
            s2 += L * L
            count += 1
    return np.array([s1, s2, count], dtype=np.int64), hist


def choose_staff_scale(hists):
    """dict(line, space, pitch_bin, pitch, confidence) or None, from the three histograms."""
    ink, pair = [int(v) for v in hists[0]], [int(v) for v in hists[2]]
    pitch_bin, best = 0, 0
    for b in range(2, 255):
        if pair[b] > best:
            pitch_bin, best = b, pair[b]
    if best == 0:
        return None
    line, best = 0, -1
    for b in range(1, pitch_bin):
        if ink[b] > best:
            line, best = b, ink[b]
    near = [(b, pair[b]) for b in (pitch_bin - 1, pitch_bin, pitch_bin + 1)]
    n = sum(c for _, c in near)
    return dict(line=line, space=pitch_bin - line, pitch_bin=pitch_bin, pitch=sum(b * c for b, c in near) / n, confidence=n / sum(pair))


def level_at(hist, percent):
    """The smallest level at or below which at least max(1, ceil(n * percent / 100)) of the n pixels lie."""
    n = int(sum(int(v) for v in hist))
    rank, acc = max(1, -(-n * percent // 100)), 0
    for level in range(256):
        acc += int(hist[level])
        if acc >= rank:
            return level
    return 255


def quality(page, ink_threshold=0.5, paper_percent=50, ink_percent=2):
    """The fields of page.PageQuality that are measured, as a dict."""
    stats, hist = sharpness(page)
    s1, s2, n = (int(v) for v in stats)
    var = float(Fraction(n * s2 - s1 * s1, n * n)) if n else 0.0
    paper, ink = level_at(hist, paper_percent), level_at(hist, ink_percent)
    total = int(hist.sum())
    inked = sum(int(hist[v]) for v in range(256) if np.float32(v) / np.float32(255.0) < np.float32(ink_threshold))
    return dict(scale=choose_staff_scale(runs(page, ink_threshold)), sharpness=var, paper_level=paper, ink_level=ink, contrast=paper - ink,
                ink_share=inked / total, focus=var / max(paper - ink, 1) ** 2)


def boundary_page(H, W, C, seed=0):
    """A uint8 page (paper 255, ink 0) whose columns hold the runs a kernel that walks chunks of C rows can get wrong, repeated across the
    width: runs that start or end exactly on a chunk boundary, runs that span three chunks, runs of exactly 254, 255, 256 and 300 rows,
    all-ink and all-paper columns, a pair whose paper run is open, one-row runs either side of a boundary, and random columns."""
    rng = np.random.RandomState(seed)
    cols = []

    def col(*ink_spans):
        c = np.full(H, 255, dtype=np.uint8)
        for a, b in ink_spans:
            c[max(a, 0):max(min(b, H), 0)] = 0
        cols.append(c)

    col()                                            # all paper
    col((0, H))                                      # all ink
    col((H // 2, H))                                 # ink open at the bottom
    col((0, H // 2))                                 # ink open at the top, paper open at the bottom
    col((1, H - 1))                                  # one closed ink run between two one-row open paper runs
    col((2, 5))                                      # a closed ink run over an OPEN paper run: no pair
    col((2, 5), (H - 1, H))                          # the same with the paper run closed by the last row
    for b in range(C, H, C):
        col((b, b + 3), (b + 5, b + 6))              # starts on the boundary
        col((b - 3, b), (b + 2, b + 4))              # ends on it
        col((b - 1, b + 1))                          # across it
        col((b - 1, b), (b + 1, b + 2))              # one-row runs either side of it
        col((b - 2, b - 1), (b, b + 1))
        col((b - C, b), (b + C, b + C + 1))          # fills a chunk exactly; the paper under it fills the next
        col((b - C + 1, b + C + 1))                  # spans three chunks
        col((1, b), (b + 1, b + 2 * C + 3))
    for n in (254, 255, 256, 300):
        for y in (1, C - 1, C, C + 1):
            col((y, y + n))                          # the clamp bin, alone ...
            col((y, y + n), (y + n + 2, y + n + 3))  # ... and as half of a pair
            col((y - 1 if y > 1 else 1, y), (y + n, y + n + 1))   # a paper run of n rows
    for p in (0.5, 0.1, 0.9, 0.02):
        for _ in range(6):
            cols.append(np.where(rng.rand(H) < p, 0, 255).astype(np.uint8))
    page = np.stack([cols[i % len(cols)] for i in range(W)], axis=1) if W >= len(cols) else np.stack(cols[:W], axis=1)
    return np.ascontiguousarray(page), len(cols)
