"""Page rectification, the parts that need no GPU: the numpy restatement (tests/rectify_reference.py) checked against itself and by hand,
the host side of acai_omr_amd/page.py and ops.py against it (the edge fit, the integer homography, RectifyConfig, the refusals, the
signature of page_inference, PageResult's maps through quad and angle), the declarations - and the claim itself on the CPU: a page
photographed on a dark table has ONE band for the detection rule, and its three systems after the reference chain has rectified it."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import deskew_reference as D
import rectify_reference as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Corner error of the fit against the quad `embed` was given, in pixels: twice the worst of the four quads, measured with the restatement
# (test_photographed_page_* prints them): 0.7053, 0.6758, 0.6698, 0.5514.  The first paper pixel of a row lies between 0 and 1 pixel inside
# the outline, half a pixel on average, on every side: about 0.5 * sqrt(2) at a corner, which `inset` is there to absorb.
MEASURED_WORST_CORNER_ERROR = 0.7053
CORNER_TOL = 2 * MEASURED_WORST_CORNER_ERROR             # 1.4106
assert CORNER_TOL < 1.5                                  # below RectifyConfig.tol: were it not, the fit rule would be inadequate

# What rounding the nine entries to 2^-30 can move a mapped point by: each entry is off by at most 2^-31, so a numerator and the
# denominator (at least about 0.5 after the scaling, here) by (320 + 360 + 1) * 2^-31, and the quotient, a coordinate of up to 480, by
# about (1 + 480) * 681 * 2^-31 / 0.5 = 3.1e-4.
Q_TOL = 3.1e-4


def _resolved(H, W):
    from acai_omr_amd.page import DetectConfig
    return DetectConfig().resolved(H, W)


@pytest.fixture(scope="module")
def page():
    p = D.synthetic_page(0)[0]
    assert D.detect(p, _resolved(360, 320)) == Q.LEVEL_BOXES
    return p


@pytest.fixture(scope="module")
def frames(page):
    """Per quad: (the photographed page, its reference extents at the default run, the fitted quad, the rectified page), computed once."""
    out = []
    for i, quad in enumerate(Q.QUADS):
        frame = Q.embed(page, quad, *Q.FRAME, seed=i)
        ext = Q.extents(frame, Q.default_min_run(*Q.FRAME))
        rect, fitted = Q.rectify(frame)
        out.append((frame, ext, fitted, rect))
    return out


# ---- 1. the restatement itself ----------------------------------------------------------------------------------------------------------
def test_reference_extents_by_hand():
    row = lambda s: np.array([[255 if c == "p" else 0 for c in s]], dtype=np.uint8)   # noqa: E731
    ext = lambda s, r: Q.extents(row(s), r).tolist()[:2]                              # noqa: E731  (row_lo, row_hi of the one row)
    assert ext("..ppp.pppp", 3) == [2, 9]                    # a run ending at the last column
    assert ext("..ppp.pppp", 4) == [6, 9]
    assert ext("..ppp.pppp", 5) == [10, -1]
    assert ext("pppp", 5) == [4, -1]                         # R > W
    assert ext("......", 1) == [6, -1]                       # no paper
    assert ext("p....p", 1) == [0, 5]
    e = Q.extents(row("..ppp.pppp"), 1).tolist()
    assert e[2:12] == [1, 1, 0, 0, 0, 1, 0, 0, 0, 0] and e[12:] == [-1, -1, 0, 0, 0, -1, 0, 0, 0, 0]   # columns of a one-row page
    col = np.array([[0], [255], [255], [0], [255]], dtype=np.uint8)
    assert Q.extents(col, 2).tolist() == [1, 1, 1, 1, 1, -1, -1, -1, -1, -1, 1, 2]
    f32 = np.array([[0.49999, 0.5, 1.0, np.nan]], dtype=np.float32)                    # paper is NOT (v < threshold): 0.5 and NaN are paper
    assert Q.extents(f32, 1).tolist()[:2] == [1, 3]


def test_reference_identity_and_shift(page):
    assert np.array_equal(Q.warp_u8(page, Q.IDENTITY, page.shape), page)
    f = page.astype(np.float64) / 255.0
    assert np.array_equal(Q.warp_f64(f, Q.IDENTITY, page.shape), f)
    one = 1 << 30
    got = Q.warp_u8(page, [one, 0, 3 * one, 0, one, -2 * one, 0, 0, one], (50, 60), fill=7)     # out(x, y) = page(x + 3, y - 2)
    assert np.array_equal(got[2:, :], page[:48, 3:63]) and (got[:2] == 7).all()
    # a scaled matrix is the same map: the quotient does not change
    assert np.array_equal(Q.warp_u8(page, [3 * v for v in Q.IDENTITY], page.shape), page)


@pytest.mark.parametrize("inset", [0, 1, 2.5])
def test_closed_form_is_the_homography_of_the_four_corners(inset):
    """The closed form against the 8 x 8 linear system, and the integers against both: the corners of the grown rectangle land on the quad."""
    OH, OW = 360, 320
    for quad in Q.QUADS:
        coef = Q.homography_q30(quad, (OH, OW), inset)
        rect = [(-inset, -inset), (OW - 1 + inset, -inset), (OW - 1 + inset, OH - 1 + inset), (-inset, OH - 1 + inset)]
        for (x, y), (qx, qy) in zip(rect, quad):
            assert Q.apply(coef, x, y) == pytest.approx((qx, qy), abs=Q_TOL)
        M = Q.solve_homography(rect, quad)
        dens = [M[2, 0] * x + M[2, 1] * y + 1.0 for x, y in ((0, 0), (OW - 1, 0), (OW - 1, OH - 1), (0, OH - 1))]
        want = M.flatten() / max(dens) * 2.0 ** 30
        assert np.abs(np.array(coef, dtype=np.float64) - want).max() <= 1.0 + 1e-6 * np.abs(want).max()
        assert max(coef[6] * x + coef[7] * y + coef[8] for x, y in ((0, 0), (OW - 1, 0), (OW - 1, OH - 1), (0, OH - 1))) == pytest.approx(2 ** 30, abs=2 * (OH + OW))


# ---- 2. the host side against the restatement -------------------------------------------------------------------------------------------
def test_fit_agrees_with_the_restatement(frames):
    from acai_omr_amd.page import RectifyConfig, fit_page_quad
    for (frame, ext, fitted, _), truth in zip(frames, Q.QUADS):
        for src in (ext, torch.from_numpy(ext), ext.tolist()):
            mine = fit_page_quad(src, *Q.FRAME)
            assert mine is not None and np.abs(np.array(mine) - np.array(fitted)).max() <= 1e-6
        loose = fit_page_quad(ext, *Q.FRAME, RectifyConfig(tol=3.0, min_points=50))
        assert np.abs(np.array(loose) - np.array(Q.fit_quad(ext, *Q.FRAME, tol=3.0, min_points=50))).max() <= 1e-6
    with pytest.raises(ValueError):
        fit_page_quad(frames[0][1][:-1], *Q.FRAME)


def test_homography_q30_equals_the_restatement():
    from acai_omr_amd import ops
    for quad in Q.QUADS + [[(0, 0), (99, 0), (99, 49), (0, 49)], [(10.25, 3.5), (700.125, 40.0), (650.5, 900.75), (-20.0, 880.0)]]:
        for size in ((360, 320), (50, 100), (1, 2), (2, 1)):
            for inset in (0, 1, 2, 0.5):
                if size[0] - 1 + 2 * inset > 0 and size[1] - 1 + 2 * inset > 0:
                    got = ops.homography_q30(quad, size, inset)
                    assert got == Q.homography_q30(quad, size, inset) and all(type(v) is int for v in got) and len(got) == 9
    assert ops.homography_q30([(0, 0), (99, 0), (99, 49), (0, 49)], (50, 100), 0) == Q.IDENTITY       # the rectangle itself


def test_homography_q30_refuses():
    from acai_omr_amd import ops
    with pytest.raises(ValueError):
        ops.homography_q30([(0, 0), (10, 0), (20, 0), (0, 10)], (10, 10), 0)           # three corners on a line
    with pytest.raises(ValueError):
        ops.homography_q30(Q.QUADS[0], (1, 10), 0)                                     # a rectangle without height
    with pytest.raises(ValueError):
        ops.homography_q30([(0, 0), (100, 0), (40, 30), (0, 100)], (100, 100), 0)      # not convex: the horizon crosses the output


def test_rectify_config():
    from acai_omr_amd.page import RectifyConfig
    cfg = RectifyConfig()
    assert (cfg.paper_threshold, cfg.min_run, cfg.tol, cfg.min_points, cfg.min_area, cfg.inset, cfg.out_size) == (0.5, None, 1.5, 16, 0.25, 2, None)
    assert cfg.resolved(440, 480) == 4 == Q.default_min_run(440, 480) and cfg.resolved(4000, 3000) == 30 and cfg.resolved(10, 10) == 4
    assert RectifyConfig(min_run=256).resolved(10, 10) == 256


@pytest.mark.parametrize("kw", [dict(min_run=0), dict(min_run=257), dict(min_run=4.0), dict(min_run=True), dict(tol=0), dict(tol=-1.0), dict(tol=None),
                                dict(min_points=1), dict(min_points=16.0), dict(min_area=-0.1), dict(min_area=1.5), dict(inset=-1), dict(inset=None),
                                dict(out_size=(0, 10)), dict(out_size=(10,)), dict(out_size=(10.0, 10)), dict(out_size=(65536, 10)), dict(out_size=(10, 16385)),
                                dict(paper_threshold=None)])
def test_rectify_config_refuses(kw):
    from acai_omr_amd.page import RectifyConfig, fit_page_quad
    with pytest.raises(ValueError):
        RectifyConfig(**kw)
    cfg = RectifyConfig()
    for k, v in kw.items():
        setattr(cfg, k, v)                                   # a config changed after it was made is checked when it is used
    with pytest.raises(ValueError):
        cfg.resolved(440, 480)
    with pytest.raises(ValueError):
        fit_page_quad(np.zeros(2 * 440 + 2 * 480), 440, 480, cfg)


def test_page_inference_takes_rectify_keyword_only():
    from acai_omr_amd.inference.vitomr_inference import page_inference
    params = inspect.signature(page_inference).parameters
    for name in ("rectify", "flatten", "deskew", "grammar"):
        assert params[name].default is None and params[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(params)[-1] == "rectify"


def test_surface_is_unchanged():
    import test_surface
    test_surface.test_mirror_surface_matches_reference()


def test_declared_built_and_documented():
    from acai_omr_amd import _lib, page
    hdr = open(os.path.join(ROOT, "include", "acai_omr_hip.h")).read()
    for name in ("acai_page_extents", "acai_page_warp"):
        assert re.search(r"\bint " + name + r"\s*\(", hdr) and name in _lib._SIGNATURES
    assert "rectify.hip" in _lib.SOURCES and os.path.exists(os.path.join(_lib.CSRC, "rectify.hip"))
    doc = " ".join(page.__doc__.split())
    for words in ("page curl", "lighter than", "cut off by the frame", "colour input", "quarter-turn", "one resampling", "batching the stage", "real photographs"):
        assert words in doc, words


def test_ops_refuse_cpu_tensors_and_bad_arguments(page):
    from acai_omr_amd import ops
    t = torch.from_numpy(page)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.page_extents(t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.page_warp(t, Q.IDENTITY, (10, 10))
    if not torch.cuda.is_available():                        # the host entry points refuse as well when there is no GPU to upload to
        from acai_omr_amd.page import find_page_quad, rectify_pages
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            find_page_quad(t)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            rectify_pages([t], Q.QUADS[0])


# ---- 3. PageResult ----------------------------------------------------------------------------------------------------------------------
def _result(quad, angle, **kw):
    from acai_omr_amd.page import PageResult
    seqs = torch.tensor([[1, 5, 2], [1, 6, 2]])
    mask = torch.ones(2, 3, dtype=torch.bool)
    boxes = [[(10, 20, 110, 60)], [(0, 0, 177, 16)]]
    return PageResult(boxes, seqs, torch.zeros(2, 3), mask, [0, 1], [(32, 64), (16, 176)], [(0, 0, 32, 64), (0, 24, 16, 128)], (1, 2, 0),
                      angles=[angle, 0.0], page_sizes=[(360, 320), (50, 300)], quads=[quad, None], source_sizes=[Q.FRAME, (50, 300)], **kw)


@pytest.mark.parametrize("angle", [0.0, 3.5])
def test_page_result_maps_through_quad_and_angle(angle):
    from acai_omr_amd.page import PageResult
    quad = Q.QUADS[3]
    level, res = _result(None, angle), _result(quad, angle)
    assert res.quads == [[(float(x), float(y)) for x, y in quad], None] and res.source_sizes == [Q.FRAME, (50, 300)] and res.inset == 2
    assert level.quads == [None, None]
    coef = Q.homography_q30(quad, (360, 320), 2)
    for xy in [(0.0, 0.0), (17.25, 9.5), (63.0, 31.0)]:
        rx, ry = level.to_page_xy(0, *xy)                        # the point in the rectified page: the map without a quad
        assert res.to_page_xy(0, *xy) == pytest.approx(Q.apply(coef, rx, ry), abs=1e-9)     # where the kernel's homography leads from there
        assert res.from_page_xy(0, *res.to_page_xy(0, *xy)) == pytest.approx(xy, abs=1e-6)
        assert res.to_page_xy(1, *xy) == level.to_page_xy(1, *xy)                            # the other page was not rectified
    assert res.box_corners(0) == [pytest.approx(Q.apply(coef, *p), abs=1e-9) for p in level.box_corners(0)]
    # the rectangle grown by the inset is the quad
    plain = _result(quad, 0.0)
    for (x, y), corner in zip([(-2, -2), (321, -2), (321, 361), (-2, 361)], quad):
        assert plain.to_source_xy(0, x, y) == pytest.approx(corner, abs=Q_TOL)
        assert plain.from_source_xy(0, *corner) == pytest.approx((x, y), abs=Q_TOL)
    assert _result(quad, 0.0, inset=0).to_source_xy(0, 0, 0) == pytest.approx(quad[0], abs=Q_TOL)
    # every construction the tests had keeps working, and a quad needs the page sizes
    old = PageResult([[(10, 20, 110, 60)]], None, None, None, [0], [(32, 64)], [(0, 0, 32, 64)])
    assert old.quads == [None] and old.source_sizes is None and old.to_page_xy(0, -0.5, -0.5) == pytest.approx((9.5, 19.5))
    assert PageResult([[]], None, None, None, [], [], [], page_sizes=[(5, 6)]).source_sizes == [(5, 6)]
    with pytest.raises(ValueError):
        PageResult([[(10, 20, 110, 60)]], None, None, None, [0], [(32, 64)], [(0, 0, 32, 64)], quads=[quad])
    with pytest.raises(ValueError):
        PageResult([[], []], None, None, None, [], [], [], quads=[None])


# ---- 4. what rectification is for -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(4))
def test_photographed_page_has_one_band_and_three_systems_once_rectified(frames, k):
    frame, _, fitted, rect = frames[k]
    assert len(D.detect(frame, _resolved(*Q.FRAME))) == 1        # the present path: the table is ink in every row, the bands merge
    err = Q.corner_error(fitted, Q.QUADS[k])
    print(f"quad {k}: corner error {err:.4f} px")
    assert err <= CORNER_TOL
    boxes = D.detect(rect, _resolved(360, 320))
    assert len(boxes) == 3
    dev = max(abs(a - b) for box, want in zip(boxes, Q.LEVEL_BOXES) for a, b in zip(box, want))
    print(f"quad {k}: boxes deviate by {dev} px from the level page's")
    assert dev <= 2 + 1                                          # inset + 1


def test_measured_constant_is_the_worst_of_the_four(frames):
    worst = max(Q.corner_error(fitted, quad) for (_, _, fitted, _), quad in zip(frames, Q.QUADS))
    assert worst == pytest.approx(MEASURED_WORST_CORNER_ERROR, abs=5e-4)


def test_nothing_to_rectify(page):
    from acai_omr_amd.page import fit_page_quad
    H, W = page.shape
    ext = Q.extents(page, Q.default_min_run(H, W))               # the sheet fills the frame
    assert Q.fit_quad(ext, H, W) is None and fit_page_quad(ext, H, W) is None
    dark = np.random.RandomState(3).randint(20, 71, size=Q.FRAME).astype(np.uint8)
    ext = Q.extents(dark, 4)                                     # a blank dark frame: no points at all
    assert (ext[:440] == 480).all() and (ext[440:880] == -1).all()
    assert Q.fit_quad(ext, *Q.FRAME) is None and fit_page_quad(ext, *Q.FRAME) is None
    small = Q.embed(page[:60, :60], [(200, 200), (259, 200), (259, 259), (200, 259)], *Q.FRAME)   # 1.7 % of the frame: below min_area
    ext = Q.extents(small, 4)
    assert Q.fit_quad(ext, *Q.FRAME) is None and fit_page_quad(ext, *Q.FRAME) is None
    assert Q.fit_quad(ext, *Q.FRAME, min_area=0.01) is not None
