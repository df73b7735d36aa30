"""Page ingest, the parts that need no GPU: the numpy restatement (tests/ingest_reference.py) against PIL where PIL is installed and
against itself by hand, the rule of the orientation estimate on the synthetic clef page, the host side of acai_omr_amd/page.py (the two
decisions, the coordinate maps of PageResult through an orientation), the signature of page_inference, the declarations and documents,
and the refusals."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ingest_reference as G
import page_reference as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

try:
    from PIL import Image, ImageOps
except ImportError:                                              # the comparison is optional: the GPU tests stand on the restatement
    Image = None

needs_pil = pytest.mark.skipif(Image is None, reason="PIL is not installed")


# ---- 1. the restatement ------------------------------------------------------------------------------------------------------------------
@needs_pil
def test_grey_is_pil_convert_l():
    rng = np.random.RandomState(0)
    rgb = rng.randint(0, 256, size=(97, 131, 3)).astype(np.uint8)
    rgb[0, :6] = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 1, 1]]
    assert np.array_equal(G.grey(rgb), np.asarray(Image.fromarray(rgb, "RGB").convert("L")))
    rgba = rng.randint(0, 256, size=(97, 131, 4)).astype(np.uint8)
    assert np.array_equal(G.grey(rgba), np.asarray(Image.fromarray(rgba, "RGBA").convert("L")))


@needs_pil
@pytest.mark.parametrize("code", range(1, 9))
def test_orient_is_pil_exif_transpose(code):
    rng = np.random.RandomState(code)
    for arr in (rng.randint(0, 256, size=(37, 53)).astype(np.uint8), rng.randint(0, 256, size=(37, 53, 3)).astype(np.uint8)):
        im = Image.fromarray(arr)
        im.getexif()[0x0112] = code
        want = np.asarray(ImageOps.exif_transpose(im))
        assert np.array_equal(G.orient(arr, code), want)


def test_orientations_by_hand():
    a = np.array([[1, 2, 3], [4, 5, 6]], dtype=np.uint8)
    assert G.orient(a, 1).tolist() == [[1, 2, 3], [4, 5, 6]]
    assert G.orient(a, 2).tolist() == [[3, 2, 1], [6, 5, 4]]
    assert G.orient(a, 3).tolist() == [[6, 5, 4], [3, 2, 1]]
    assert G.orient(a, 4).tolist() == [[4, 5, 6], [1, 2, 3]]
    assert G.orient(a, 5).tolist() == [[1, 4], [2, 5], [3, 6]]
    assert G.orient(a, 6).tolist() == [[4, 1], [5, 2], [6, 3]]              # a quarter turn clockwise
    assert G.orient(a, 7).tolist() == [[6, 3], [5, 2], [4, 1]]
    assert G.orient(a, 8).tolist() == [[3, 6], [2, 5], [1, 4]]              # a quarter turn counter-clockwise
    for code in range(1, 9):
        assert np.array_equal(G.orient(G.orient(a, code), G.INVERSE[code]), a)
    assert np.array_equal(G.orient(G.orient(a, 6), 6), G.orient(a, 3))
    assert int(G.grey(np.array([[[255, 255, 255]]]))[0, 0]) == 255 and int(G.grey(np.array([[[77, 77, 77, 9]]]))[0, 0]) == 77
    assert int(G.grey(np.array([[[255, 0, 0]]]))[0, 0]) == 76 and int(G.grey(np.array([[[0, 0, 255]]]))[0, 0]) == 29


def test_col_profile_and_box_ink_by_hand():
    page = np.full((5, 4), 255, dtype=np.uint8)
    page[0:3, 0] = 0
    page[4, 0] = 0
    page[1:5, 2] = 0
    ink, run = G.col_profile(page)
    assert ink.tolist() == [4, 0, 4, 0] and run.tolist() == [3, 0, 4, 0]
    assert G.box_ink(page, [(0, 0, 4, 5), (0, 0, 1, 1), (1, 0, 2, 5), (2, 3, 9, 9), (-3, -3, 1, 2), (2, 2, 2, 5)]).tolist() == [8, 1, 0, 2, 2, 0]


# ---- 2. the rule of the estimate ---------------------------------------------------------------------------------------------------------
def test_estimate_on_the_clef_page():
    upright = G.clef_page(0)[0]
    for page in (upright, G.grey(G.colour_page(upright))):
        for code in (1, 3, 6, 8):
            photo = G.orient(page, G.INVERSE[code])                          # the photo that `code` turns upright
            got, conf = G.estimate(photo)
            assert got == code and 0.0 < conf <= 1.0, (code, got, conf)
            assert np.array_equal(G.orient(photo, got), page)
    assert G.is_sideways(G.orient(upright, 8)) and not G.is_sideways(upright)


def test_estimate_without_evidence():
    sym = P.synthetic_page(0)[0]                                             # its systems end alike: a tie
    assert G.estimate(sym) == (1, 0.0) and G.estimate(G.orient(sym, 3)) == (1, 0.0) and G.estimate(G.orient(sym, 8)) == (6, 0.0)
    blank = np.full((120, 90), 230, dtype=np.uint8)
    assert G.estimate(blank) == (1, 0.0)


def test_host_decisions_equal_the_restatement():
    from acai_omr_amd import page as pg
    cfg = pg.OrientConfig()
    assert (cfg.ink_threshold, cfg.line_frac, cfg.min_line_rows, cfg.end_frac, cfg.detect) == (0.5, 0.5, 5, 0.12, None)
    upright = G.clef_page(0)[0]
    for code in (1, 3, 6, 8):
        photo = G.orient(upright, G.INVERSE[code])
        H, W = photo.shape
        side = pg.orientation_is_sideways(P.profile(photo)[1], G.col_profile(photo)[1], H, W)
        assert side == G.is_sideways(photo) == (code in (6, 8))
        level = G.orient(photo, 6) if side else photo
        boxes = G.detect(level)
        rects = pg.orientation_end_boxes(boxes)
        assert rects == G.end_boxes(boxes) and len(rects) == 6
        down, conf = pg.orientation_up_down(G.box_ink(level, rects).tolist())
        assert ((8 if down else 6) if side else (3 if down else 1), conf) == G.estimate(photo)
    assert pg.orientation_up_down([]) == (False, 0.0) and pg.orientation_up_down([5, 5]) == (False, 0.0) and pg.orientation_up_down([1, 3]) == (True, 0.5)
    assert pg.orientation_end_boxes([(10, 0, 15, 9)], pg.OrientConfig(end_frac=0.01)) == [(10, 0, 11, 9), (14, 0, 15, 9)]     # at least one column
    for kw in (dict(end_frac=0), dict(end_frac=0.6), dict(line_frac=0), dict(min_line_rows=0), dict(min_line_rows=2.0), dict(detect=5), dict(ink_threshold=None)):
        with pytest.raises(ValueError):
            pg.OrientConfig(**kw)


# ---- 3. PageResult through an orientation -------------------------------------------------------------------------------------------------
H_SRC, W_SRC = 50, 70                                                        # the photo; the upright page of a quarter turn is 70 x 50


def _result(code, angle=0.0, quad=None):
    from acai_omr_amd import ops
    from acai_omr_amd.page import PageResult
    size = ops.oriented_size(H_SRC, W_SRC, code)
    return PageResult([[(5, 8, 37, 24)]], None, None, None, [0], [(16, 32)], [(0, 0, 16, 32)], angles=[angle], page_sizes=[size], quads=[quad],
                      source_sizes=[(H_SRC, W_SRC)], orientations=[code])


@pytest.mark.parametrize("code", range(1, 9))
def test_page_result_maps_through_an_orientation(code):
    from acai_omr_amd import ops
    from acai_omr_amd.page import PageResult
    res = _result(code)
    assert res.orientations == [code] and res.source_sizes == [(H_SRC, W_SRC)]
    OH, OW = ops.oriented_size(H_SRC, W_SRC, code)
    assert (OH, OW) == ((W_SRC, H_SRC) if code >= 5 else (H_SRC, W_SRC))
    # the pixels of the photo the index map names: photo[py, px] is upright[y, x]
    photo = np.arange(H_SRC * W_SRC).reshape(H_SRC, W_SRC)
    upright = G.orient(photo, code)
    x0, y0, x1, y1 = res.boxes[0][0]
    corners = [(x0, y0), (x1 - 1, y0), (x1 - 1, y1 - 1), (x0, y1 - 1)]       # the four corner PIXELS of the box
    for x, y in corners:
        px, py = res.to_source_xy(0, x, y)
        assert (px, py) == G.to_photo_xy(code, H_SRC, W_SRC, x, y) and photo[py, px] == upright[y, x]
    # the model's pixel grid: the box is resized by 1 (32 x 16 from 32 x 16), so model pixel (x, y) is box pixel (x, y)
    for x, y in ((0, 0), (31, 15), (7, 3)):
        assert res.to_page_xy(0, x, y) == pytest.approx(G.to_photo_xy(code, H_SRC, W_SRC, x0 + x, y0 + y), abs=1e-12)
        assert res.from_page_xy(0, *res.to_page_xy(0, x, y)) == pytest.approx((x, y), abs=1e-12)
    assert res.from_page_xy(0, *res.to_page_xy(0, 3.25, 9.5)) == pytest.approx((3.25, 9.5), abs=1e-12)
    assert res.box_corners(0) == [G.to_photo_xy(code, H_SRC, W_SRC, float(x), float(y)) for x, y in ((x0, y0), (x1, y0), (x1, y1), (x0, y1))]
    # composed with an angle and a quad: the orientation is the last step back, applied to what the map without it gives
    quad = [(3.0, 2.0), (OW - 4.0, 4.0), (OW - 2.0, OH - 3.0), (1.0, OH - 5.0)]
    both, plain = _result(code, 2.5, quad), PageResult([[(5, 8, 37, 24)]], None, None, None, [0], [(16, 32)], [(0, 0, 16, 32)], angles=[2.5],
                                                        page_sizes=[(OH, OW)], quads=[quad], source_sizes=[(OH, OW)])
    for xy in ((0.0, 0.0), (17.25, 9.5), (31.0, 15.0)):
        ux, uy = plain.to_page_xy(0, *xy)
        assert both.to_page_xy(0, *xy) == pytest.approx(G.to_photo_xy(code, H_SRC, W_SRC, ux, uy), abs=1e-9)
        assert both.from_page_xy(0, *both.to_page_xy(0, *xy)) == pytest.approx(xy, abs=1e-6)


def test_page_result_defaults_and_refusals():
    from acai_omr_amd.page import PageResult
    old = PageResult([[(10, 20, 110, 60)]], None, None, None, [0], [(32, 64)], [(0, 0, 32, 64)])
    assert old.orientations == [1] and old.to_page_xy(0, -0.5, -0.5) == pytest.approx((9.5, 19.5))
    with pytest.raises(ValueError):
        PageResult([[]], None, None, None, [], [], [], orientations=[6])                 # a turn needs the photo's size
    with pytest.raises(ValueError):
        PageResult([[]], None, None, None, [], [], [], orientations=[1, 1])
    with pytest.raises(ValueError):
        PageResult([[]], None, None, None, [], [], [], source_sizes=[(4, 5)], orientations=[9])
    with pytest.raises(TypeError):
        PageResult([[]], None, None, None, [], [], [], source_sizes=[(4, 5)], orientations=[6.0])


# ---- 4. signature, declarations, documents ------------------------------------------------------------------------------------------------
def test_page_inference_takes_orient_keyword_only():
    from acai_omr_amd.inference.vitomr_inference import page_inference
    params = inspect.signature(page_inference).parameters
    assert params["orient"].default is None and params["orient"].kind is inspect.Parameter.KEYWORD_ONLY
    names = list(params)
    assert names.index("orient") < names.index("rectify") and names[-1] == "rectify"
    from acai_omr_amd.page import PageResult
    assert inspect.signature(PageResult.__init__).parameters["orientations"].default is None


def test_declared_built_and_documented():
    from acai_omr_amd import _lib, ops, page
    hdr = open(os.path.join(ROOT, "include", "acai_omr_hip.h")).read()
    for name in ("acai_page_ingest", "acai_page_col_profile", "acai_page_box_ink"):
        assert re.search(r"\bint " + name + r"\s*\(", hdr) and name in _lib._SIGNATURES
    for cite in ("routes.py:98,115", "datasets.py:32,122", "routes.py:118"):                 # the reference call sites the launch replaces
        assert cite in hdr
    assert "ingest.hip" in _lib.SOURCES and os.path.exists(os.path.join(_lib.CSRC, "ingest.hip"))
    for fn in ("page_ingest", "page_col_profile", "page_box_ink"):
        assert callable(getattr(ops, fn))
    for fn in ("ingest_pages", "estimate_orientation", "OrientConfig"):
        assert hasattr(page, fn)
    assert _lib.col_chunks(1) == (64, 1) and _lib.col_chunks(64) == (64, 1) and _lib.col_chunks(65) == (64, 2) and _lib.col_chunks(4096) == (64, 64)
    assert _lib.col_chunks(4097) == (65, 64) and _lib.col_chunks(_lib.PAGE_MAX_H) == (1024, 64)
    doc = " ".join(page.__doc__.split())
    for words in ("colour input", "quarter-turn", "that is `ingest_pages`", "exif_transpose", "19595", "float colour input", "mirrored photos without a tag",
                  "reading the EXIF tag out of a file", "JPEG decoding", "folding the quarter turn into the rectification warp", "HEURISTIC",
                  "real photographs"):
        assert words in doc, words
    from acai_omr_amd.inference.vitomr_inference import page_inference
    pdoc = " ".join(page_inference.__doc__.split())
    for words in ("orient", "ingest -> rectify -> flatten -> deskew -> detect", "UPRIGHT", "not measured on real photographs", "float colour input"):
        assert words in pdoc, words
    for name in ("README.md", "DESIGN.md"):
        text = " ".join(open(os.path.join(ROOT, name)).read().split())
        for words in ("page_ingest", "estimate_orientation", "real photographs", "ingest_bench.json"):
            assert words in text, (name, words)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_without_a_gpu():
    from acai_omr_amd import ops
    from acai_omr_amd import page as pg
    from acai_omr_amd.inference.vitomr_inference import page_inference
    from types import SimpleNamespace
    grey, rgb = torch.from_numpy(G.clef_page(0)[0]), torch.from_numpy(G.colour_page(G.clef_page(0)[0]))
    tr = SimpleNamespace(device=torch.device("cuda"))            # (all page_inference asks of `resize` before it refuses)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.page_ingest(rgb, 6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.page_col_profile(grey)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.page_box_ink(grey, torch.zeros(1, 4, dtype=torch.int32))
    if not torch.cuda.is_available():                            # the host entry points refuse as well when there is no GPU to upload to
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pg.ingest_pages(rgb, 6)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pg.ingest_pages(grey)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pg.estimate_orientation(grey)
        for orient in (None, 6, True):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                page_inference(None, rgb, "cuda", tr, orient=orient)
    # what is wrong with the arguments is said before anything is uploaded
    for bad in ("upright", 1.5, 6.0, {6}, [1.5], ["6"]):
        with pytest.raises(TypeError):
            page_inference(None, grey, "cuda", tr, orient=bad)
    for bad in (0, 9, -1, [0], [9]):
        with pytest.raises(ValueError):
            page_inference(None, grey, "cuda", tr, orient=bad)
    with pytest.raises(ValueError):
        page_inference(None, [grey, grey], "cuda", tr, orient=[6])                     # one code per page
    for bad in (0, 9):
        with pytest.raises(ValueError):
            ops.exif_code(bad)
        with pytest.raises(ValueError):
            pg.orientation_codes(bad, 1)
    for bad in (True, 1.0, "1", None):
        with pytest.raises(TypeError):
            ops.exif_code(bad)
    assert pg.orientation_codes(None, 2) == [1, 1] and pg.orientation_codes(6, 2) == [6, 6] and pg.orientation_codes((3, 8), 2) == [3, 8]
    assert [ops.EXIF_INVERSE[c] for c in range(1, 9)] == [G.INVERSE[c] for c in range(1, 9)]
    with pytest.raises(TypeError):
        pg.ingest_pages("not a tensor")
    with pytest.raises(TypeError):
        pg.detect_systems("not a tensor")
    with pytest.raises(TypeError):
        pg.estimate_orientation("not a tensor")
