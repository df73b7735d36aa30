"""A numpy restatement of the deskew kernels (csrc/deskew.hip), written from their definitions in include/acai_omr_hip.h - loops over strips,
slopes and taps, whole-array integer arithmetic over the pixels - plus the host's choice of the angle and a seeded synthetic page whose
systems survive two bilinear resamplings.  Integer results: the tests use equality."""
import math

import numpy as np

import page_reference as R

MAX_SLOPE = 17560   # round(tan(15 deg) * 65536)


def strips(page, S, ink_threshold=0.5):
    """uint8 [nS][H]: ink pixels of row y in columns [s S, min((s + 1) S, W))."""
    m = R.ink_mask(page, ink_threshold)
    H, W = m.shape
    nS = -(-W // S)
    out = np.zeros((nS, H), dtype=np.uint8)
    for s in range(nS):
        out[s] = m[:, s * S:min((s + 1) * S, W)].sum(1)
    return out


def sheared_profile(P, W, S, m):
    """Q[y] = sum over s of P[s][y + off(s)], off(s) = (m (s S + S // 2 - W // 2) + 32768) >> 16, rows outside [0, H) counting 0.  int64 [H]."""
    nS, H = P.shape
    Q = np.zeros(H, dtype=np.int64)
    for s in range(nS):
        off = (int(m) * (s * S + S // 2 - W // 2) + 32768) >> 16      # (Python's >> on ints is arithmetic)
        lo, hi = max(0, -off), min(H, H - off)                        # the rows y with 0 <= y + off < H
        if lo < hi:
            Q[lo:hi] += P[s, lo + off:hi + off]
    return Q


def skew_scores(P, W, S, slopes):
    """Per slope, sum over y in [0, H - 2] of (Q[y + 1] - Q[y])^2 as Python ints."""
    out = []
    for m in slopes:
        d = np.diff(sheared_profile(P, W, S, m))
        out.append(int((d * d).sum()))
    return out


def candidates(max_angle, step):
    n = int(round(max_angle / step))
    return [(k - n) * step for k in range(2 * n + 1)]


def slope_table(max_angle, step):
    return [int(round(math.tan(math.radians(a)) * 65536.0)) for a in candidates(max_angle, step)]


def choose(scores, max_angle, step):
    """The maximum; among equal maxima the candidate nearest to 0, the negative one first; an interior winner with a negative second
    difference moves to the vertex of the parabola through its neighbours."""
    s = [int(v) for v in scores]
    cand = candidates(max_angle, step)
    n = len(s) // 2
    best = max(s)
    ties = [i for i in range(len(s)) if s[i] == best]
    k = sorted(ties, key=lambda i: (abs(i - n), i))[0]
    angle = cand[k]
    if 0 < k < len(s) - 1:
        den = s[k - 1] - 2 * s[k] + s[k + 1]
        if den < 0:
            angle += step * 0.5 * (s[k - 1] - s[k + 1]) / den
    return float(angle)


def estimate(page, S=16, max_angle=10.0, step=0.125, ink_threshold=0.5):
    """(angle, scores) of one page."""
    W = np.asarray(page).shape[1]
    sc = skew_scores(strips(page, S, ink_threshold), W, S, slope_table(max_angle, step))
    return choose(sc, max_angle, step), sc


def rotation_q16(angle_deg):
    a = math.radians(float(angle_deg))
    return int(round(math.cos(a) * 65536.0)), int(round(math.sin(a) * 65536.0))


def _source(H, W, cos_q, sin_q):
    x = np.arange(W, dtype=np.int64)[None, :]
    y = np.arange(H, dtype=np.int64)[:, None]
    dx2, dy2 = 2 * x - (W - 1), 2 * y - (H - 1)
    sx = (cos_q * dx2 - sin_q * dy2 + (W - 1) * 65536) >> 1
    sy = (sin_q * dx2 + cos_q * dy2 + (H - 1) * 65536) >> 1
    return sx >> 16, sy >> 16, (sx >> 8) & 255, (sy >> 8) & 255


def _taps(page, iy, ix, fill):
    H, W = page.shape
    out = []
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        yy, xx = iy + dy, ix + dx
        inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        out.append(np.where(inside, page[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], fill))
    return out


def rotate_u8(page, cos_q, sin_q, fill=255):
    page = np.asarray(page)
    assert page.dtype == np.uint8
    ix, iy, fx, fy = _source(*page.shape, int(cos_q), int(sin_q))
    t00, t01, t10, t11 = _taps(page.astype(np.int64), iy, ix, int(fill))
    out = ((256 - fy) * ((256 - fx) * t00 + fx * t01) + fy * ((256 - fx) * t10 + fx * t11) + 32768) >> 16
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def rotate_f64(page, cos_q, sin_q, fill=1.0):
    """The fp32 kernel's definition evaluated in float64 (the weights f / 256 are exact in both)."""
    page = np.asarray(page, dtype=np.float64)
    ix, iy, fx, fy = _source(*page.shape, int(cos_q), int(sin_q))
    t00, t01, t10, t11 = _taps(page, iy, ix, float(fill))
    wx, wy = fx / 256.0, fy / 256.0
    return (1.0 - wy) * ((1.0 - wx) * t00 + wx * t01) + wy * ((1.0 - wx) * t10 + wx * t11)


def rotate_deg(page, angle_deg, fill=255):
    return rotate_u8(page, *rotation_q16(angle_deg), fill)


LINE_GAP, STAFF_GAP, HEAD, THICK = 6, 40, 4, 2


def synthetic_page(seed=0, H=360, W=320, systems_at=((60, 2), (170, 1), (250, 2)), x0=30, x1=290):
    """`page_reference.synthetic_page` with strokes a bilinear resampling cannot take above the ink threshold: staff lines THICK = 2 rows
    and barlines 2 columns thick (between two ink pixels every interpolated value is ink).  Paper is noise in 200..255, ink noise in 0..90.
    Systems (first row, staves): five lines per staff LINE_GAP rows apart, staves STAFF_GAP apart, columns x0 .. x1 - 1, joined by barlines
    at both ends, a note head above the first line.  Returns (page, truth boxes at margin 0)."""
    rng = np.random.RandomState(seed)
    page = rng.randint(200, 256, size=(H, W)).astype(np.uint8)

    def ink(ys, xs):
        page[ys, xs] = rng.randint(0, 91, size=page[ys, xs].shape).astype(np.uint8)

    truth = []
    for y, staves in systems_at:
        last = y + (staves - 1) * STAFF_GAP + 4 * LINE_GAP + THICK - 1
        for s in range(staves):
            for k in range(5):
                r = y + s * STAFF_GAP + k * LINE_GAP
                ink(slice(r, r + THICK), slice(x0, x1))
        ink(slice(y, last + 1), slice(x0, x0 + 2))
        ink(slice(y, last + 1), slice(x1 - 2, x1))
        ink(slice(y - HEAD, y), slice(x0 + 46, x0 + 52))
        truth.append((x0, y - HEAD, x1, last + 1))
    return page, truth


def detect(page, cfg_resolved, ink_threshold=0.5, min_line_rows=5, max_systems=64):
    """`page_reference.systems` with a DetectConfig's resolved (min_ink, merge_gap, min_height, line_len, margin) -> the boxes."""
    min_ink, merge_gap, min_height, line_len, margin = cfg_resolved
    return R.systems(page, ink_threshold, min_ink, merge_gap, min_height, line_len, min_line_rows, margin, max_systems)[1]
