"""A numpy restatement of page ingest (csrc/ingest.hip, the host side in acai_omr_amd/page.py), written from the definitions in
include/acai_omr_hip.h and the rule of `page.estimate_orientation` with plain index arithmetic: the grey value, the eight EXIF index
maps, the column profile, the box ink counts, the two decisions of the orientation estimate and the coordinate map through an
orientation - plus a synthetic page with a "clef" at the start of every staff, grey and in colour.  Integer results: the tests use
equality."""
import math

import numpy as np

import page_reference as P

INVERSE = {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 8, 7: 7, 8: 6}     # a quarter turn is undone by the opposite quarter turn, the rest by themselves


def grey(img):
    """(H, W, C >= 3) uint8 -> (H, W) uint8: PIL's convert("L"), (19595 R + 38470 G + 7471 B + 32768) >> 16; further channels are ignored."""
    img = np.asarray(img).astype(np.int64)
    return ((19595 * img[..., 0] + 38470 * img[..., 1] + 7471 * img[..., 2] + 32768) >> 16).astype(np.uint8)


def source_index(code, H, W):
    """The (rows, columns) index arrays of the output of orientation `code` into an H x W input: output pixel (y, x) reads input
    [rows[y, x], columns[y, x]].  The table of the header, line by line."""
    OH, OW = (W, H) if code >= 5 else (H, W)
    y, x = np.indices((OH, OW))
    return {1: (y, x), 2: (y, W - 1 - x), 3: (H - 1 - y, W - 1 - x), 4: (H - 1 - y, x),
            5: (x, y), 6: (H - 1 - x, y), 7: (H - 1 - x, W - 1 - y), 8: (x, W - 1 - y)}[code]


def orient(img, code):
    """A (H, W) or (H, W, C) array with orientation `code` applied (what ImageOps.exif_transpose makes of an image tagged with it)."""
    img = np.asarray(img)
    r, c = source_index(code, img.shape[0], img.shape[1])
    return np.ascontiguousarray(img[r, c])


def ingest(img, code=1):
    """A (H, W), (H, W, 1), (H, W, 3) or (H, W, 4) array -> the grey, upright page."""
    img = np.asarray(img)
    if img.ndim == 3:
        img = img[..., 0] if img.shape[2] == 1 else grey(img)
    return orient(img, code)


def col_profile(page, ink_threshold=0.5):
    """(ink, run) int32 [W]: the row profile of the transposed page."""
    return P.profile(np.asarray(page).T, ink_threshold)


def box_ink(page, boxes, ink_threshold=0.5):
    """int32 [n]: the ink pixels in rows [y0, y1), columns [x0, x1) of every box (x0, y0, x1, y1), clipped to the page."""
    m = P.ink_mask(page, ink_threshold)
    H, W = m.shape
    out = []
    for x0, y0, x1, y1 in boxes:
        x0, y0, x1, y1 = max(int(x0), 0), max(int(y0), 0), min(int(x1), W), min(int(y1), H)
        out.append(int(m[y0:y1, x0:x1].sum()) if x1 > x0 and y1 > y0 else 0)
    return np.array(out, dtype=np.int32)


def detect(page, ink_threshold=0.5, line_frac=0.5, min_line_rows=5):
    """The system boxes of `page.detect_systems` with the defaults of `page.DetectConfig`, sized from the page."""
    H, W = np.asarray(page).shape
    count, boxes = P.systems(page, ink_threshold, max(1, W // 500), max(1, H // 200), max(1, H // 90), int(math.ceil(line_frac * W)), min_line_rows,
                             max(1, H // 100), 64)
    assert count <= 64
    return boxes


def is_sideways(page, ink_threshold=0.5, line_frac=0.5, min_line_rows=5):
    H, W = np.asarray(page).shape
    rows = int((P.profile(page, ink_threshold)[1] >= int(math.ceil(line_frac * W))).sum())
    cols = int((col_profile(page, ink_threshold)[1] >= int(math.ceil(line_frac * H))).sum())
    return cols >= min_line_rows and cols > rows


def end_boxes(boxes, end_frac=0.12):
    out = []
    for x0, y0, x1, y1 in boxes:
        e = max(1, int(round(end_frac * (x1 - x0))))
        out += [(x0, y0, x0 + e, y1), (x1 - e, y0, x1, y1)]
    return out


def estimate(page, ink_threshold=0.5, line_frac=0.5, min_line_rows=5, end_frac=0.12):
    """A grey page as it lies -> (code, confidence): sideways if it has at least min_line_rows line columns and more line columns than line
    rows, then turned by code 6; on the level page the systems' left ends against their right ends: upside down iff the right ends hold
    more ink.  1 / 3 level, 6 / 8 sideways."""
    page = np.asarray(page)
    sideways = is_sideways(page, ink_threshold, line_frac, min_line_rows)
    level = orient(page, 6) if sideways else page
    counts = box_ink(level, end_boxes(detect(level, ink_threshold), end_frac), ink_threshold)
    left, right = int(counts[0::2].sum()), int(counts[1::2].sum())
    down = right > left
    return ((8 if down else 6) if sideways else (3 if down else 1)), abs(left - right) / max(left + right, 1)


def to_photo_xy(code, H, W, x, y):
    """Pixel (x, y) of the upright page -> pixel (px, py) of the H x W photo it was read from: (column, row) of the header's table."""
    r, c = {1: (y, x), 2: (y, W - 1 - x), 3: (H - 1 - y, W - 1 - x), 4: (H - 1 - y, x),
            5: (x, y), 6: (H - 1 - x, y), 7: (H - 1 - x, W - 1 - y), 8: (x, W - 1 - y)}[code]
    return c, r


# ---- the synthetic pages -----------------------------------------------------------------------------------------------------------------
CLEF_X, CLEF_W = 4, 6      # the clef: columns x0 + 4 .. x0 + 9 of every staff, within the leftmost round(0.12 * 181) = 22 columns of a box


def clef_page(seed=0, **kw):
    """`page_reference.synthetic_page` (whose systems end alike: staff lines and one barline) with a solid block of ink over every staff's
    height a few columns right of its start, as clef, key and time signature weigh on a real system -> (uint8 page, truth boxes)."""
    page, truth = P.synthetic_page(seed, **kw)
    page = page.copy()
    rng = np.random.RandomState(seed + 1000)
    systems_at, x0 = kw.get("systems_at", ((40, 2), (110, 1), (170, 2))), kw.get("x0", 14)
    for y, staves in systems_at:
        for s in range(staves):
            r = y + s * P.STAFF_GAP
            page[r:r + 4 * P.LINE_GAP + 1, x0 + CLEF_X:x0 + CLEF_X + CLEF_W] = rng.randint(0, 91, size=(4 * P.LINE_GAP + 1, CLEF_W))
    assert not ((page >= 100) & (page <= 160)).any()
    return page, truth


def colour_page(page):
    """A grey uint8 page -> (H, W, 3) uint8: yellowish paper and blue-black ink, chosen so that the grey value of paper stays above 160 and
    that of ink below 100 (no comparison with a threshold of 0.5 is close, as in the original)."""
    g = np.asarray(page).astype(np.int64)
    paper = g >= 128
    rgb = np.where(paper[..., None], np.stack([g, g - 5, g - 40], -1), np.stack([g // 2, g // 2, g + 60], -1)).astype(np.uint8)
    lum = grey(rgb)
    assert (lum[paper] > 160).all() and (lum[~paper] < 100).all()
    return rgb
