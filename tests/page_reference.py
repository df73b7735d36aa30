"""A numpy restatement of the page kernels (csrc/page.hip) and of the host's box rounding, written from their definitions in
include/acai_omr_hip.h with plain loops, plus a seeded synthetic page whose systems are known.  Integer results: the tests use equality."""
import math

import numpy as np


def as_float(page):
    """A page as the kernels read it: uint8 -> float32(p) / float32(255), float -> float32."""
    page = np.asarray(page)
    if page.dtype == np.uint8:
        return page.astype(np.float32) / np.float32(255.0)
    return page.astype(np.float32)


def ink_mask(page, ink_threshold):
    return as_float(page) < np.float32(ink_threshold)


def longest_run(row):
    best = cur = 0
    for v in row:
        cur = cur + 1 if v else 0
        best = max(best, cur)
    return best


def profile(page, ink_threshold=0.5):
    """(ink, run) int32 [H]: ink pixels per row, and the longest run of consecutive ink pixels per row."""
    m = ink_mask(page, ink_threshold)
    return m.sum(1).astype(np.int32), np.array([longest_run(r) for r in m], dtype=np.int32)


def bands(ink, run, min_ink, merge_gap, min_height, line_len, min_line_rows):
    """(all bands, kept bands) as lists of (y0, y1): a band is a maximal set of inked rows (ink >= min_ink) whose consecutive inked rows are
    at most merge_gap other rows apart; kept if y1 - y0 >= min_height and at least min_line_rows of rows [y0, y1) have run >= line_len."""
    inked = [y for y in range(len(ink)) if ink[y] >= min_ink]
    found = []
    for y in inked:
        if found and y - found[-1][1] <= merge_gap:     # found[-1][1] is one past the previous inked row: y - that = rows in between
            found[-1][1] = y + 1
        else:
            found.append([y, y + 1])
    found = [(a, b) for a, b in found]
    kept = [(a, b) for a, b in found if b - a >= min_height and int((np.asarray(run[a:b]) >= line_len).sum()) >= min_line_rows]
    return found, kept


def systems(page, ink_threshold, min_ink, merge_gap, min_height, line_len, min_line_rows, margin, max_systems):
    """(count, boxes): the number of kept bands and the first max_systems boxes (x0, y0, x1, y1), top to bottom."""
    H, W = np.asarray(page).shape
    m = ink_mask(page, ink_threshold)
    ink, run = profile(page, ink_threshold)
    _, kept = bands(ink, run, min_ink, merge_gap, min_height, line_len, min_line_rows)
    boxes = []
    for y0, y1 in kept[:max_systems]:
        cols = np.nonzero(m[y0:y1].any(0))[0]
        x0, x1 = int(cols[0]), int(cols[-1]) + 1
        boxes.append((max(x0 - margin, 0), max(y0 - margin, 0), min(x1 + margin, W), min(y1 + margin, H)))
    return len(kept), boxes


def boxes_from_fractions(boxes, H, W):
    """routes.py:122,126: sorted by y0, cropped by PIL with the float box (x0 W, y0 H, x1 W, y1 H), which `Image.crop` rounds with
    int(round(.)) (Python's rounding)."""
    rows = [tuple(b[k] for k in ("x0", "y0", "x1", "y1")) if isinstance(b, dict) else tuple(b) for b in boxes]
    return [(int(round(x0 * W)), int(round(y0 * H)), int(round(x1 * W)), int(round(y1 * H))) for x0, y0, x1, y1 in sorted(rows, key=lambda r: r[1])]


LINE_GAP, STAFF_GAP, HEAD = 3, 21, 3   # rows from staff line to staff line, from staff to staff of a system, rows a note head sticks out


def synthetic_page(seed=0, H=240, W=200, systems_at=((40, 2), (110, 1), (170, 2)), x0=14, x1=191):
    """A uint8 page and its truth boxes (margin 0).  Paper is noise in 200..255, ink is noise in 0..90, so no pixel lies in [100, 160] and
    no comparison with a threshold of 0.5 is close.  Every system (first row, staves) has five one-row staff lines per staff from column x0
    to x1 - 1, LINE_GAP rows apart, staves STAFF_GAP rows apart and joined by barlines at both ends, and a note head HEAD rows above its
    first line.  A "title" of short dashes fills rows 8..15 (a band of its own, tall enough, without a line row) and a 3 x 3 "page number"
    sits near the bottom (a band that is too short)."""
    rng = np.random.RandomState(seed)
    page = rng.randint(200, 256, size=(H, W)).astype(np.uint8)

    def ink(ys, xs):
        page[ys, xs] = rng.randint(0, 91, size=page[ys, xs].shape).astype(np.uint8)

    for x in range(W // 5, W - W // 5 - 6, 10):          # the title: 6-pixel dashes
        ink(slice(8, 16), slice(x, x + 6))
    truth = []
    for y, staves in systems_at:
        last = y + (staves - 1) * STAFF_GAP + 4 * LINE_GAP
        for s in range(staves):
            for k in range(5):
                r = y + s * STAFF_GAP + k * LINE_GAP
                ink(slice(r, r + 1), slice(x0, x1))
        ink(slice(y, last + 1), slice(x0, x0 + 1))        # barlines
        ink(slice(y, last + 1), slice(x1 - 1, x1))
        ink(slice(y - HEAD, y), slice(x0 + 46, x0 + 51))  # a note head above the first line
        truth.append((x0, y - HEAD, x1, last + 1))
    ink(slice(H - 10, H - 7), slice(W // 2 - 2, W // 2 + 1))   # the page number
    assert not ((page >= 100) & (page <= 160)).any()
    return page, truth


def truth_boxes_with_margin(truth, margin, H, W):
    return [(max(a - margin, 0), max(b - margin, 0), min(c + margin, W), min(d + margin, H)) for a, b, c, d in truth]
