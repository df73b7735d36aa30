"""A numpy restatement of page illumination flattening (csrc/flatten.hip), written from its definition in include/acai_omr_hip.h: loops over
the tiles and the grid, whole-array integer arithmetic over the pixels.  Every result is defined in integers (the fp32 output is ONE
correctly rounded fp32 multiply), so the tests use equality.  Plus the shading helpers: a brightness ramp, a vignette and a hard shadow
across a straight edge, each floor(page * gain + 0.5) as uint8."""
import numpy as np

TILES = (16, 32, 64, 128)


def default_tile(H):
    """The largest of 16, 32, 64, 128 that is <= max(16, H // 40)."""
    return max(t for t in TILES if t <= max(16, H // 40))


def levels(page):
    """int64 [H][W]: a uint8 pixel is its own level, an fp32 pixel v is min(255, max(0, floor(v * 255 + 0.5))) with the product and the sum
    each rounded to fp32."""
    page = np.asarray(page)
    if page.dtype == np.uint8:
        return page.astype(np.int64)
    v = page.astype(np.float32)
    t = (v * np.float32(255.0)).astype(np.float32)
    t = (t + np.float32(0.5)).astype(np.float32)
    return np.clip(np.floor(t), 0, 255).astype(np.int64)


def tile_levels(page, T, percent=50):
    """uint8 [GH][GW]: per tile the rank-th smallest level of its n pixels, rank = max(1, (n percent + 99) // 100)."""
    lv = levels(page)
    H, W = lv.shape
    GH, GW = -(-H // T), -(-W // T)
    g = np.zeros((GH, GW), dtype=np.uint8)
    for i in range(GH):
        for j in range(GW):
            px = lv[i * T:min((i + 1) * T, H), j * T:min((j + 1) * T, W)].ravel()
            rank = max(1, (px.size * percent + 99) // 100)
            below = np.cumsum(np.bincount(px, minlength=256))          # below[L] = pixels with level <= L
            g[i, j] = next(L for L in range(256) if below[L] >= rank)
    return g


def smooth(g, rq=85, floor=32):
    """(s, rescued): s = max(floor, g * 256 < m * rq ? m : g), m the maximum of g over the 3 x 3 neighbourhood clipped at the border."""
    g = np.asarray(g).astype(np.int64)
    GH, GW = g.shape
    s = np.zeros_like(g)
    rescued = np.zeros(g.shape, dtype=bool)
    for i in range(GH):
        for j in range(GW):
            m = int(g[max(i - 1, 0):i + 2, max(j - 1, 0):j + 2].max())
            rescued[i, j] = int(g[i, j]) * 256 < m * rq
            s[i, j] = max(floor, m if rescued[i, j] else int(g[i, j]))
    return s, rescued


def _axis(n, T, G):
    """Per coordinate c of an axis: (first grid index, second grid index, weight w of the second in [1, 2 T), odd)."""
    u = 2 * np.arange(n, dtype=np.int64) + 1 - T
    j0 = u // (2 * T)                                                  # (numpy's // on integers is a floor division)
    w = u - j0 * 2 * T
    assert ((w >= 1) & (w < 2 * T) & (w % 2 == 1)).all()
    return np.clip(j0, 0, G - 1), np.clip(j0 + 1, 0, G - 1), w


def background(s, H, W, T):
    """int64 [H][W]: s interpolated bilinearly between the tile centres, rounded to nearest."""
    GH, GW = s.shape
    assert (GH, GW) == (-(-H // T), -(-W // T))
    D = 2 * T
    y0, y1, wy = _axis(H, T, GH)
    x0, x1, wx = _axis(W, T, GW)
    wy, wx = wy[:, None], wx[None, :]
    s00, s01 = s[y0][:, x0], s[y0][:, x1]
    s10, s11 = s[y1][:, x0], s[y1][:, x1]
    acc = (D - wy) * ((D - wx) * s00 + wx * s01) + wy * ((D - wx) * s10 + wx * s11) + D * D // 2
    assert acc.max() < 1 << 24
    return acc >> (2 * (D.bit_length() - 1))


RECIP = np.array([0] + [(255 * 65536 + b // 2) // b for b in range(1, 256)], dtype=np.int64)


def flatten_with_grid(page, g, T, rq=85, floor=32):
    """The page divided by its background: uint8 min(255, (p recip[bg] + 32768) >> 16); fp32 min(1, v * (recip[bg] * 2^-16)) in fp32."""
    page = np.asarray(page)
    H, W = page.shape
    s, _ = smooth(g, rq, floor)
    bg = background(s, H, W, T)
    assert bg.min() >= floor and bg.max() <= 255
    r = RECIP[bg]
    if page.dtype == np.uint8:
        return np.minimum(255, (page.astype(np.int64) * r + 32768) >> 16).astype(np.uint8)
    gain = r.astype(np.float32) * np.float32(2.0 ** -16)               # exact: recip < 2^24
    return np.minimum(np.float32(1.0), (page.astype(np.float32) * gain).astype(np.float32)).astype(np.float32)


def flatten(page, T=None, percent=50, rq=85, floor=32):
    page = np.asarray(page)
    T = default_tile(page.shape[0]) if T is None else T
    return flatten_with_grid(page, tile_levels(page, T, percent), T, rq, floor)


# ---- shading: what a phone does to a page ---------------------------------------------------------------------------------------------
def shade(page, gain):
    """floor(page * gain + 0.5) as uint8, gain a float64 [H][W] (or broadcastable) in [0, 1]."""
    return np.floor(np.asarray(page).astype(np.float64) * gain + 0.5).astype(np.uint8)


def ramp_gain(H, W, lo=0.35, vertical=0.0):
    """Brightness falling linearly from 1.0 at the left edge to `lo` at the right one; vertical > 0 lets it also fall from 1.0 at the top to
    1 - vertical at the bottom (the two multiply)."""
    gx = 1.0 + (lo - 1.0) * np.arange(W) / max(W - 1, 1)
    gy = 1.0 - vertical * np.arange(H) / max(H - 1, 1)
    return gy[:, None] * gx[None, :]


def vignette_gain(H, W, corner=0.4):
    """1.0 at the centre, falling with the squared distance to `corner` in the corners."""
    y = (np.arange(H) - (H - 1) / 2.0) / ((H - 1) / 2.0)
    x = (np.arange(W) - (W - 1) / 2.0) / ((W - 1) / 2.0)
    return 1.0 - (1.0 - corner) * (y[:, None] ** 2 + x[None, :] ** 2) / 2.0


def shadow_gain(H, W, dark=0.45, slope=0.5, at=0.5):
    """A hard shadow: `dark` on the right of the straight edge x = at W + slope (y - H / 2), 1.0 on its left."""
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    return np.where(x >= at * W + slope * (y - H / 2.0), dark, 1.0)
