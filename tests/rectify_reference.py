"""A numpy restatement of page rectification (csrc/rectify.hip and the host fit of acai_omr_amd/page.py), written from the definitions in
include/acai_omr_hip.h and the fit rule of `page.fit_page_quad`: plain loops over runs, whole-array int64 floor division over the pixels,
the taps and the blend of deskew_reference - plus `embed`, which photographs a page: puts it into a frame of dark noise through a
homography.  Integer results: the tests use equality."""
import math

import numpy as np

import deskew_reference as D
import page_reference as R


# ---- extents ----------------------------------------------------------------------------------------------------------------------------
def _line_extents(paper, run, none_lo):
    """(lo, hi) of one row or column: the start of the first and the end of the last maximal paper run of at least `run` pixels."""
    lo, hi, n, k = none_lo, -1, len(paper), 0
    while k < n:
        if not paper[k]:
            k += 1
            continue
        s = k
        while k < n and paper[k]:
            k += 1
        if k - s >= run:                      # the run [s, k)
            lo, hi = min(lo, s), k - 1
    return lo, hi


def extents(page, run, paper_threshold=0.5):
    """int32 [2 H + 2 W] = row_lo, row_hi, col_lo, col_hi; paper = not ink at paper_threshold."""
    paper = ~R.ink_mask(page, paper_threshold)
    H, W = paper.shape
    rows = [_line_extents(paper[y], run, W) for y in range(H)]
    cols = [_line_extents(paper[:, x], run, H) for x in range(W)]
    return np.array([r[0] for r in rows] + [r[1] for r in rows] + [c[0] for c in cols] + [c[1] for c in cols], dtype=np.int32)


def default_min_run(H, W):
    return max(4, min(H, W) // 100)


# ---- the fit ----------------------------------------------------------------------------------------------------------------------------
def fit_edge(t, v, tol, min_points):
    """v = a t + b through the points in the order given: the central half by index first, then three times all points within tol."""
    t, v = np.asarray(t, dtype=np.float64), np.asarray(v, dtype=np.float64)
    n = len(t)
    keep = np.zeros(n, dtype=bool)
    keep[n // 4:n - n // 4] = True
    for rounds_left in (3, 2, 1, 0):
        if keep.sum() < 2 or (rounds_left == 0 and keep.sum() < min_points):
            return None
        if np.ptp(t[keep]) == 0:
            return None
        a, b = np.polyfit(t[keep] - t[keep].mean(), v[keep], 1)
        b -= a * t[keep].mean()
        if rounds_left:
            keep = np.abs(v - (a * t + b)) <= tol
    return float(a), float(b)


def fit_quad(ext, H, W, tol=1.5, min_points=16, min_area=0.25):
    """[TL, TR, BR, BL] or None, by the rule of page.fit_page_quad."""
    ext = np.asarray(ext, dtype=np.float64)
    row_lo, row_hi, col_lo, col_hi = ext[:H], ext[H:2 * H], ext[2 * H:2 * H + W], ext[2 * H + W:]
    ys, xs = np.nonzero(row_hi >= 0)[0], np.nonzero(col_hi >= 0)[0]
    lines = [fit_edge(t, v, tol, min_points) for t, v in ((ys, row_lo[ys]), (ys, row_hi[ys]), (xs, col_lo[xs]), (xs, col_hi[xs]))]
    if any(ln is None for ln in lines):
        return None
    left, right, top, bottom = lines
    quad = []
    for (a1, b1), (a2, b2) in ((left, top), (right, top), (right, bottom), (left, bottom)):
        if 1.0 - a1 * a2 == 0.0:
            return None
        x = (a1 * b2 + b1) / (1.0 - a1 * a2)
        quad.append((x, a2 * x + b2))
    q = np.array(quad)
    nxt, nn = np.roll(q, -1, axis=0), np.roll(q, -2, axis=0)
    cross = (nxt[:, 0] - q[:, 0]) * (nn[:, 1] - nxt[:, 1]) - (nxt[:, 1] - q[:, 1]) * (nn[:, 0] - nxt[:, 0])
    ordered = q[0, 0] < q[1, 0] and q[3, 0] < q[2, 0] and q[0, 1] < q[3, 1] and q[1, 1] < q[2, 1]
    if not ((cross > 0).all() and ordered):
        return None
    area = 0.5 * abs(np.sum(q[:, 0] * nxt[:, 1] - nxt[:, 0] * q[:, 1]))
    if area < min_area * H * W:
        return None
    frame = np.array([(0, 0), (W - 1, 0), (W - 1, H - 1), (0, H - 1)], dtype=np.float64)
    if (np.abs(q - frame) <= 1).all():
        return None
    return quad


# ---- the homography ---------------------------------------------------------------------------------------------------------------------
def square_to_quad(quad):
    """(a .. h) of x = (a u + b v + c) / (g u + h v + 1), y = (d u + e v + f) / (g u + h v + 1) taking (0, 0), (1, 0), (1, 1), (0, 1) to the
    quad's TL, TR, BR, BL: Heckbert's closed form in Python floats, in the order of operations ops.homography_q30 documents."""
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = ((float(x), float(y)) for x, y in quad)
    dx1, dx2, sx = x1 - x2, x3 - x2, (x0 - x1) + (x2 - x3)
    dy1, dy2, sy = y1 - y2, y3 - y2, (y0 - y1) + (y2 - y3)
    det = dx1 * dy2 - dx2 * dy1
    g, h = (sx * dy2 - dx2 * sy) / det, (dx1 * sy - sx * dy1) / det
    return (x1 - x0) + g * x1, (x3 - x0) + h * x3, x0, (y1 - y0) + g * y1, (y3 - y0) + h * y3, y0, g, h


def homography_q30(quad, out_size, inset=0):
    OH, OW = out_size
    inset = float(inset)
    lx, ly = OW - 1 + 2.0 * inset, OH - 1 + 2.0 * inset
    a, b, c, d, e, f, g, h = square_to_quad(quad)
    m = [a / lx, b / ly, c + (a * inset) / lx + (b * inset) / ly,
         d / lx, e / ly, f + (d * inset) / lx + (e * inset) / ly,
         g / lx, h / ly, 1.0 + (g * inset) / lx + (h * inset) / ly]
    top = max(m[6] * x + m[7] * y + m[8] for x, y in ((0, 0), (OW - 1, 0), (OW - 1, OH - 1), (0, OH - 1)))
    return [int(round(v / top * 2.0 ** 30)) for v in m]


def solve_homography(src, dst):
    """The 3 x 3 matrix (h33 = 1) taking the four points src to dst, by the 8 x 8 linear system (numpy): what the closed form is checked by."""
    rows, rhs = [], []
    for (x, y), (u, v) in zip(src, dst):
        rows += [[x, y, 1, 0, 0, 0, -u * x, -u * y], [0, 0, 0, x, y, 1, -v * x, -v * y]]
        rhs += [u, v]
    return np.append(np.linalg.solve(np.array(rows, dtype=np.float64), np.array(rhs, dtype=np.float64)), 1.0).reshape(3, 3)


IDENTITY = [1 << 30, 0, 0, 0, 1 << 30, 0, 0, 0, 1 << 30]


# ---- the warp ---------------------------------------------------------------------------------------------------------------------------
def _source(coef, OH, OW):
    A, B, C, D_, E, F, G, H_, I = (int(v) for v in coef)   # noqa: E741
    x = np.arange(OW, dtype=np.int64)[None, :]
    y = np.arange(OH, dtype=np.int64)[:, None]
    den = G * x + H_ * y + I
    assert (den > 0).all()
    sxq = np.floor_divide((A * x + B * y + C) * 256, den)
    syq = np.floor_divide((D_ * x + E * y + F) * 256, den)
    return sxq >> 8, syq >> 8, sxq & 255, syq & 255


def warp_u8(page, coef, out_size, fill=255):
    page = np.asarray(page)
    assert page.dtype == np.uint8
    ix, iy, fx, fy = _source(coef, *out_size)
    t00, t01, t10, t11 = D._taps(page.astype(np.int64), iy, ix, int(fill))
    out = ((256 - fy) * ((256 - fx) * t00 + fx * t01) + fy * ((256 - fx) * t10 + fx * t11) + 32768) >> 16
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def warp_f64(page, coef, out_size, fill=1.0):
    """The fp32 kernel's definition evaluated in float64 (the weights f / 256 are exact in both)."""
    page = np.asarray(page, dtype=np.float64)
    ix, iy, fx, fy = _source(coef, *out_size)
    t00, t01, t10, t11 = D._taps(page, iy, ix, float(fill))
    wx, wy = fx / 256.0, fy / 256.0
    return (1.0 - wy) * ((1.0 - wx) * t00 + wx * t01) + wy * ((1.0 - wx) * t10 + wx * t11)


def apply(coef, x, y):
    """The homography itself, in float64."""
    A, B, C, D_, E, F, G, H_, I = (float(v) for v in coef)   # noqa: E741
    den = G * x + H_ * y + I
    return (A * x + B * y + C) / den, (D_ * x + E * y + F) / den


# ---- a photographed page ----------------------------------------------------------------------------------------------------------------
def embed(page, quad, FH, FW, seed=0):
    """The page as a camera sees it lying on a table: a uint8 FH x FW frame of noise in 20 .. 70 in which the page's corner pixels (0, 0),
    (W - 1, 0), (W - 1, H - 1), (0, H - 1) land on quad = [TL, TR, BR, BL], the sheet's outline.  A frame pixel is the page sampled
    bilinearly at its preimage (clamped to the page, float64) where the sheet covers it, the table where it does not, and on the outline
    the two weighed by the share of the pixel the sheet covers, as a sensor weighs them: clip(0.5 + d, 0, 1) with d the distance, in frame
    pixels, from the pixel's centre to the nearest side of the quad, positive inside.  Rounded to nearest."""
    page = np.asarray(page)
    H, W = page.shape
    table = np.random.RandomState(seed).randint(20, 71, size=(FH, FW)).astype(np.float64)
    inv = np.linalg.inv(solve_homography([(0, 0), (W - 1, 0), (W - 1, H - 1), (0, H - 1)], quad))
    x, y = np.meshgrid(np.arange(FW, dtype=np.float64), np.arange(FH, dtype=np.float64))
    d = np.full((FH, FW), np.inf)
    for k in range(4):                                   # TL, TR, BR, BL runs clockwise as displayed (y down): inside is to the right
        (ax, ay), (bx, by) = quad[k], quad[(k + 1) % 4]
        d = np.minimum(d, ((bx - ax) * (y - ay) - (by - ay) * (x - ax)) / math.hypot(bx - ax, by - ay))
    cover = np.clip(0.5 + d, 0.0, 1.0)
    den = np.where(cover > 0, inv[2, 0] * x + inv[2, 1] * y + inv[2, 2], 1.0)
    u = np.clip((inv[0, 0] * x + inv[0, 1] * y + inv[0, 2]) / den, 0, W - 1)
    v = np.clip((inv[1, 0] * x + inv[1, 1] * y + inv[1, 2]) / den, 0, H - 1)
    iu, iv = np.clip(np.floor(u).astype(np.int64), 0, W - 2), np.clip(np.floor(v).astype(np.int64), 0, H - 2)
    fu, fv = u - iu, v - iv
    p = page.astype(np.float64)
    val = (1 - fv) * ((1 - fu) * p[iv, iu] + fu * p[iv, iu + 1]) + fv * ((1 - fu) * p[iv + 1, iu] + fu * p[iv + 1, iu + 1])
    return np.clip(np.floor(cover * val + (1.0 - cover) * table + 0.5), 0, 255).astype(np.uint8)


FRAME = (440, 480)                                      # (FH, FW) of the end-to-end case
QUADS = [[(60, 40), (400, 55), (430, 420), (35, 400)],
         [(50, 50), (380, 30), (420, 400), (70, 430)],
         [(90, 30), (390, 60), (360, 410), (40, 380)],
         [(70, 25), (395, 25), (440, 415), (25, 415)]]
LEVEL_BOXES = [(27, 53, 293, 129), (27, 163, 293, 199), (27, 243, 293, 319)]   # of deskew_reference.synthetic_page() at its DetectConfig


def rectify(frame, out_size=(360, 320), inset=2, run=None, tol=1.5, min_points=16, min_area=0.25):
    """(the rectified frame, the fitted quad) by the reference chain: extents -> fit -> homography -> warp; (frame, None) without a quad."""
    frame = np.asarray(frame)
    H, W = frame.shape
    quad = fit_quad(extents(frame, default_min_run(H, W) if run is None else run), H, W, tol, min_points, min_area)
    if quad is None:
        return frame, None
    return warp_u8(frame, homography_q30(quad, out_size, inset), out_size), quad


def corner_error(quad, truth):
    return max(math.hypot(x - tx, y - ty) for (x, y), (tx, ty) in zip(quad, truth))
