"""Page illumination flattening, the parts that need no GPU: the numpy restatement (tests/flatten_reference.py) on the synthetic page under
synthetic shading - the detection rule loses systems of the shaded page and finds the unshaded page's boxes on the flattened one - the
rescue of mostly-ink tiles, and the host side of acai_omr_amd/page.py: FlattenConfig and its default tile, the refusals, the signature of
page_inference, the declarations."""
import inspect
import os
import re

import numpy as np
import pytest

import deskew_reference as D
import flatten_reference as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _resolved(H=360, W=320):
    from acai_omr_amd.page import DetectConfig
    return DetectConfig().resolved(H, W)


@pytest.fixture(scope="module")
def page():
    """The synthetic page (360 x 320, 3 systems) and its boxes."""
    p = D.synthetic_page(0)[0]
    boxes = D.detect(p, _resolved())
    assert len(boxes) == 3
    return p, boxes


# ---- 1. FlattenConfig, the surface -------------------------------------------------------------------------------------------------------
def test_flatten_config_defaults_and_default_tile():
    from acai_omr_amd.page import FlattenConfig
    cfg = FlattenConfig()
    assert (cfg.tile, cfg.percent, cfg.floor) == (None, 50, 32) and cfg.ink_ratio == 1 / 3
    assert cfg.resolved(360) == (16, 50, 85, 32)                       # rq = round(256 / 3)
    assert cfg.resolved(3508) == (64, 50, 85, 32)                      # A4 at 300 dpi
    for H, tile in ((1, 16), (639, 16), (1279, 16), (1280, 32), (2559, 32), (2560, 64), (5119, 64), (5120, 128), (65535, 128)):
        assert cfg.resolved(H)[0] == tile == F.default_tile(H), H
    assert FlattenConfig(tile=128, percent=100, ink_ratio=0, floor=255).resolved(10) == (128, 100, 0, 255)
    assert FlattenConfig(percent=1, ink_ratio=1.0, floor=1).resolved(10) == (16, 1, 256, 1)


@pytest.mark.parametrize("kw", [dict(tile=24), dict(tile=8), dict(tile=256), dict(tile=16.0), dict(tile=True), dict(percent=0), dict(percent=101),
                                dict(percent=50.0), dict(ink_ratio=-0.01), dict(ink_ratio=1.01), dict(ink_ratio=None), dict(floor=0), dict(floor=256),
                                dict(floor=32.0)])
def test_flatten_config_refuses(kw):
    from acai_omr_amd.page import FlattenConfig
    with pytest.raises(ValueError):
        FlattenConfig(**kw)
    cfg = FlattenConfig()
    for k, v in kw.items():
        setattr(cfg, k, v)                                             # a config changed after it was made is checked when it is used
    with pytest.raises(ValueError):
        cfg.resolved(360)


def test_page_inference_takes_flatten_keyword_only():
    from acai_omr_amd.inference.vitomr_inference import page_inference
    p = inspect.signature(page_inference).parameters["flatten"]
    assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    d = inspect.signature(page_inference).parameters["deskew"]
    assert d.default is None and d.kind is inspect.Parameter.KEYWORD_ONLY


def test_page_result_flattened_defaults_to_false():
    from acai_omr_amd.page import PageResult
    r = PageResult([[], []], None, None, None, [], [], [])
    assert r.flattened == [False, False]
    assert PageResult([[], []], None, None, None, [], [], [], flattened=[True, 0]).flattened == [True, False]
    with pytest.raises(ValueError):
        PageResult([[], []], None, None, None, [], [], [], flattened=[True])


def test_surface_is_unchanged():
    import test_surface
    test_surface.test_mirror_surface_matches_reference()


def test_declared_built_and_documented():
    from acai_omr_amd import _lib, page
    hdr = open(os.path.join(ROOT, "include", "acai_omr_hip.h")).read()
    for name in ("acai_page_tile_levels", "acai_page_flatten"):
        assert re.search(r"\bint " + name + r"\s*\(", hdr) and name in _lib._SIGNATURES
    assert "flatten.hip" in _lib.SOURCES and _lib.FLATTEN_TILES == page.FLATTEN_TILES == F.TILES
    doc = " ".join(page.__doc__.split())
    for words in ("binarisation", "colour input", "dark table", "two tiles wide", "real photographs"):
        assert words in doc, words


# ---- 2. the restatement itself -----------------------------------------------------------------------------------------------------------
def test_reference_small_cases_by_hand():
    # one tile of 4 pixels 10, 20, 30, 40: rank = max(1, (4 percent + 99) // 100)
    px = np.array([[10, 20], [30, 40]], dtype=np.uint8)
    assert [int(F.tile_levels(px, 16, pc)[0, 0]) for pc in (1, 25, 26, 50, 51, 75, 76, 100)] == [10, 10, 20, 20, 30, 30, 40, 40]
    # fp32 levels: floor(v * 255 + 0.5) in fp32, clipped
    v = np.array([[0.0, 1.0, 0.5, 0.001, 0.00196, 0.00197, 1.5, -0.2]], dtype=np.float32)
    assert F.levels(v).tolist() == [[0, 255, 128, 0, 0, 1, 255, 0]]
    # recip: 255 / b in Q16, rounded to nearest; a pixel at its background becomes 255 (b >= 2)
    assert F.RECIP[255] == 65536 and F.RECIP[1] == 255 * 65536 and F.RECIP[3] == 85 * 65536
    for b in range(2, 256):
        assert (b * F.RECIP[b] + 32768) >> 16 == 255, b
    # rescue and floor on a 3 x 3 grid: the centre is ink (its level is below a third of its brightest neighbour's)
    g = np.array([[200, 210, 220], [200, 60, 220], [20, 210, 10]], dtype=np.uint8)
    s, resc = F.smooth(g, 85, 32)
    assert resc.tolist() == [[False] * 3, [False, True, False], [True, False, True]]
    assert s.tolist() == [[200, 210, 220], [200, 220, 220], [210, 210, 220]]
    s0, resc0 = F.smooth(g, 0, 32)
    assert not resc0.any() and s0.tolist() == [[200, 210, 220], [200, 60, 220], [32, 210, 32]]
    # the interpolation reproduces a constant grid, and at a tile centre's two pixels weighs the tile 2 T - 1 : 1 against its neighbour
    assert (F.background(np.full((3, 2), 77, dtype=np.int64), 40, 20, 16) == 77).all()
    bg = F.background(np.array([[100, 200]], dtype=np.int64), 1, 32, 16)[0]
    assert bg[:8].tolist() == [100] * 8 and bg[24:].tolist() == [200] * 8 and bg[8] == (31 * 100 + 200 + 16) >> 5 and (np.diff(bg) >= 0).all()


def test_reference_leaves_an_even_page_alone(page):
    p, boxes = page
    for T in (16, 32):
        flat = F.flatten(p, T)
        assert np.array_equal(flat < 128, p < 128)
        assert D.detect(flat, _resolved()) == boxes
    white = np.full((40, 50), 255, dtype=np.uint8)
    assert np.array_equal(F.flatten(white, 16), white)
    ones = np.ones((40, 50), dtype=np.float32)
    assert np.array_equal(F.flatten(ones, 16), ones) and F.flatten(ones, 16).dtype == np.float32


# ---- 3. what flattening is for -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [16, 32])
def test_ramp_loses_systems_and_flattening_restores_them(page, T):
    p, boxes = page
    shaded = F.shade(p, F.ramp_gain(360, 320, 0.35))                   # brightness 1.0 at the left edge, 0.35 at the right one
    assert len(D.detect(shaded, _resolved())) < 3
    flat = F.flatten(shaded, T)
    assert D.detect(flat, _resolved()) == boxes
    assert np.array_equal(flat < 128, p < 128)                         # the ink mask of the unshaded page, pixel for pixel


@pytest.mark.parametrize("T", [16, 32])
@pytest.mark.parametrize("gain", ["xy ramp", "vignette"])
def test_smooth_shading_keeps_the_ink_mask(page, gain, T):
    p, boxes = page
    shaded = F.shade(p, F.ramp_gain(360, 320, 0.35, 0.3) if gain == "xy ramp" else F.vignette_gain(360, 320, 0.4))
    flat = F.flatten(shaded, T)
    assert D.detect(flat, _resolved()) == boxes and np.array_equal(flat < 128, p < 128)


@pytest.mark.parametrize("dark", [0.45, 0.6])
def test_hard_shadow_keeps_the_boxes(page, dark):
    """A hard shadow across a diagonal edge, at the page's default tile (16).  No claim about the ink mask: it differs in a thin band along
    the edge, where the interpolated background is between the two levels."""
    p, boxes = page
    shaded = F.shade(p, F.shadow_gain(360, 320, dark))
    assert len(D.detect(shaded, _resolved())) < 3
    flat = F.flatten(shaded)
    assert D.detect(flat, _resolved()) == boxes
    print(f"shadow {dark}: ink mask differs in {int(((flat < 128) != (p < 128)).sum())} of {p.size} pixels")


@pytest.mark.parametrize("shaded", [False, True])
def test_rescue_of_a_filled_block(page, shaded):
    """A 32 x 32 ink block on tile boundaries (tile 16: four tiles that are all ink).  Rescued, they take the paper around them and stay
    ink; not rescued, their own median passes for paper and about half the block turns white."""
    p, _ = page
    blk = p.copy()
    blk[208:240, 112:144] = np.random.RandomState(1).randint(0, 91, size=(32, 32))
    src = F.shade(blk, F.ramp_gain(360, 320, 0.35)) if shaded else blk
    g = F.tile_levels(src, 16)
    _, rescued = F.smooth(g, 85, 32)
    assert np.argwhere(rescued).tolist() == [[13, 7], [13, 8], [14, 7], [14, 8]]
    assert np.array_equal(F.flatten_with_grid(src, g, 16, 85, 32) < 128, blk < 128)
    _, none = F.smooth(g, 0, 32)
    assert not none.any()
    off = F.flatten_with_grid(src, g, 16, 0, 32) < 128
    assert not np.array_equal(off, blk < 128)
    lost = int((~off[208:240, 112:144]).sum())
    assert 1024 // 4 < lost < 3 * 1024 // 4, lost                      # about half of the block
