"""Page deskew, the parts that need no GPU: the numpy restatement (tests/deskew_reference.py) on a synthetic page tilted by known angles - the
estimate finds the angle, the detection rule loses the systems of the tilted page and finds them again on the levelled one - and the host
arithmetic of acai_omr_amd/page.py: the choice of the angle, the slope table, PageResult's map through the rotation, the refusals."""
import math

import numpy as np
import pytest
import torch

import deskew_reference as D

ANGLES = (0, 0.6, -1.3, 2.0, -3.7, 5.0, -8.0)
MAX_ANGLE, STEP = 10.0, 0.25
_cache = {}


def _resolved():
    from acai_omr_amd.page import DetectConfig
    return DetectConfig().resolved(360, 320)


def _tilted(seed, angle):
    """The synthetic page turned so that its staff lines run down to the right by `angle` degrees (computed once per seed and angle)."""
    key = (seed, angle)
    if key not in _cache:
        page = D.synthetic_page(seed)[0]
        _cache[key] = D.rotate_deg(page, -angle) if angle else page
    return _cache[key]


@pytest.mark.parametrize("S", [8, 16])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_levels_the_tilted_synthetic_page(seed, S):
    res = _resolved()
    base = D.detect(_tilted(seed, 0), res)
    assert len(base) == 3
    for a in ANGLES:
        tilted = _tilted(seed, a)
        est, _ = D.estimate(tilted, S, MAX_ANGLE, STEP)
        found = D.detect(tilted, res)
        levelled = D.rotate_deg(tilted, est) if est != 0.0 else tilted
        boxes = D.detect(levelled, res)
        print(f"seed {seed} S {S} angle {a}: estimate {est:.4f}, {len(found)} systems tilted, {len(boxes)} levelled")
        assert abs(est - a) <= STEP, (a, est)
        if abs(a) >= 1.3:
            assert len(found) < 3, (a, found)            # the rule as it stands loses systems of such a page
        assert len(boxes) == 3, (a, boxes)
        assert max(abs(p - q) for b, c in zip(boxes, base) for p, q in zip(b, c)) <= 3, (a, boxes, base)
    if seed == 0:
        assert D.estimate(_tilted(0, 0), S, MAX_ANGLE, STEP)[0] == 0.0


@pytest.mark.parametrize("S", [8, 16, 32, 64])
def test_reference_blank_page_is_level(S):
    for blank in (np.full((50, 60), 255, dtype=np.uint8), np.ones((7, 130), dtype=np.float32)):
        est, scores = D.estimate(blank, S)
        assert est == 0.0 and not any(scores)


def test_reference_rotation_exact_cases():
    rng = np.random.RandomState(5)
    page = rng.randint(0, 256, size=(9, 9)).astype(np.uint8)
    assert np.array_equal(D.rotate_u8(page, 65536, 0), page)
    assert np.array_equal(D.rotate_u8(page, 0, 65536), np.rot90(page, 1))            # + 90 degrees: counter-clockwise as displayed
    wide = rng.randint(0, 256, size=(5, 12)).astype(np.uint8)
    assert np.array_equal(D.rotate_u8(wide, 65536, 0), wide)
    assert D.rotation_q16(90) == (0, 65536) and D.rotation_q16(0) == (65536, 0)
    f = D.rotate_f64(page / 255.0, *D.rotation_q16(3.0), fill=1.0)
    assert abs(f * 255.0 - D.rotate_u8(page, *D.rotation_q16(3.0), fill=255)).max() <= 0.5 + 1e-9     # the uint8 result is its rounding


def test_reference_strips_and_scores_by_hand():
    page = np.full((4, 20), 255, dtype=np.uint8)
    page[1, 3:19] = 0
    page[2, 7:9] = 0
    P = D.strips(page, 8)
    assert P.shape == (3, 4) and P[:, 1].tolist() == [5, 8, 3] and P[:, 2].tolist() == [1, 1, 0] and P[:, 0].tolist() == [0, 0, 0]
    assert D.sheared_profile(P, 20, 8, 0).tolist() == [0, 16, 2, 0]
    assert D.skew_scores(P, 20, 8, [0]) == [16 * 16 + 14 * 14 + 2 * 2]
    # slope 1/8 per column: strips at dx = -6, 2, 10 shift by round(-0.75), round(0.25), round(1.25) = -1, 0, 1 rows
    assert D.sheared_profile(P, 20, 8, 8192).tolist() == [0 + 0 + 3, 0 + 8 + 0, 5 + 1 + 0, 1 + 0 + 0]
    assert D.skew_scores(np.zeros((3, 1), dtype=np.uint8), 20, 8, [0, 5]) == [0, 0]                    # H = 1


# ---- host arithmetic ---------------------------------------------------------------------------------------------------------------------
def test_choose_skew_tie_break_and_parabola():
    from acai_omr_amd.page import SkewConfig, choose_skew
    cfg = SkewConfig(max_angle=1.0, step=0.25)                   # candidates -1 .. 1 in steps of 0.25: 9 of them, 0 at index 4
    assert cfg.candidates() == [-1.0, -0.75, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75, 1.0]
    assert choose_skew([0] * 9, cfg) == 0.0                      # a blank page
    assert choose_skew([7] * 9, cfg) == 0.0
    assert choose_skew([0, 0, 1, 5, 1, 5, 1, 0, 0], cfg) == -0.25   # equally near: the negative one (its neighbours are equal: no shift)
    assert choose_skew([0, 0, 0, 5, 1, 5, 0, 0, 0], cfg) == D.choose([0, 0, 0, 5, 1, 5, 0, 0, 0], 1.0, 0.25) == -0.25 + 0.125 / 9
    assert choose_skew([0, 9, 0, 0, 0, 0, 9, 0, 0], cfg) == 0.5     # the nearer of two maxima, symmetric neighbours: no shift
    # the parabola through (-1, 4), (0, 10), (1, 8) peaks at 0.5 (4 - 8) / (4 - 20 + 8) = 0.25 of a step
    assert choose_skew([0, 0, 0, 0, 0, 4, 10, 8, 0], cfg) == pytest.approx(0.5 + 0.25 * 0.25, abs=1e-15)
    assert choose_skew([0, 0, 0, 0, 0, 4, 10, 8, 0], cfg) == D.choose([0, 0, 0, 0, 0, 4, 10, 8, 0], 1.0, 0.25)
    assert choose_skew([10, 0, 0, 0, 0, 0, 0, 0, 3], cfg) == -1.0   # a winner at the end is taken as it is
    assert choose_skew([0, 0, 0, 0, 0, 0, 0, 3, 10], cfg) == 1.0
    big = 1 << 40                                                # scores pass 2^32: Python integers all the way
    assert choose_skew([0, 0, big, big + 8, big, 0, 0, 0, 0], cfg) == -0.25
    with pytest.raises(ValueError):
        choose_skew([1, 2, 3], cfg)


def test_slope_table():
    from acai_omr_amd import _lib
    from acai_omr_amd.page import SkewConfig
    cfg = SkewConfig()
    cand, slopes = cfg.candidates(), cfg.slopes()
    assert len(cand) == 161 and cand[0] == -10.0 and cand[80] == 0.0 and cand[-1] == 10.0 and cand[81] == 0.125
    assert slopes == D.slope_table(10.0, 0.125) and slopes[80] == 0 and slopes[-1] == 11556 == -slopes[0]      # tan(10 deg) * 65536 = 11555.8
    assert slopes == sorted(slopes) and len(set(slopes)) == len(slopes)
    widest = SkewConfig(max_angle=15.0, step=0.5).slopes()
    assert widest[-1] == _lib.SKEW_MAX_SLOPE == D.MAX_SLOPE == int(round(math.tan(math.radians(15.0)) * 65536)) and widest[0] == -widest[-1]
    for bad in (SkewConfig(max_angle=15.5), SkewConfig(step=0.0), SkewConfig(max_angle=10.0, step=0.01), SkewConfig(max_angle=-1.0)):
        with pytest.raises(ValueError):
            bad.slopes()
    assert _lib.SKEW_CHUNK == 1023 and _lib.STRIP_WIDTHS == (8, 16, 32, 64)


def _result(angle):
    from acai_omr_amd.page import PageResult
    seqs = torch.tensor([[1, 5, 2], [1, 6, 2]])
    mask = torch.ones(2, 3, dtype=torch.bool)
    boxes = [[(10, 20, 110, 60)], [(0, 0, 177, 16)]]
    return PageResult(boxes, seqs, torch.zeros(2, 3), mask, [0, 1], [(32, 64), (16, 176)], [(0, 0, 32, 64), (0, 24, 16, 128)], (1, 2, 0),
                      angles=[angle, 0.0], page_sizes=[(240, 200), (50, 300)])


def test_page_result_maps_through_the_rotation():
    flat, res = _result(0.0), _result(3.5)
    assert flat.angles == [0.0, 0.0] and res.angles == [3.5, 0.0]
    cos_q, sin_q = D.rotation_q16(3.5)
    c, s, cx, cy = cos_q / 65536.0, sin_q / 65536.0, 199 / 2.0, 239 / 2.0
    for xy in [(0.0, 0.0), (17.25, 9.5), (63.0, 31.0)]:
        lx, ly = flat.to_page_xy(0, *xy)                         # the point in the levelled page: today's map
        want = (cx + c * (lx - cx) - s * (ly - cy), cy + s * (lx - cx) + c * (ly - cy))     # where the kernel sampled that pixel
        assert res.to_page_xy(0, *xy) == pytest.approx(want, abs=1e-9)
        assert res.from_page_xy(0, *res.to_page_xy(0, *xy)) == pytest.approx(xy, abs=1e-9)
        assert res.to_page_xy(1, *xy) == flat.to_page_xy(1, *xy)                            # the other page was not turned
    # the centre of the page is the fixed point: the same system pixel leads to it at any angle
    at_centre = flat.from_page_xy(0, cx, cy)
    assert res.from_page_xy(0, cx, cy) == pytest.approx(at_centre, abs=1e-9)
    assert res.to_page_xy(0, *at_centre) == pytest.approx((cx, cy), abs=1e-9)
    # a positive angle levels lines that run down to the right: a point right of the centre on the levelled page lies lower on the original
    px, py = res.to_page_xy(0, *flat.from_page_xy(0, cx + 50.0, cy))
    assert py > cy + 2.0 and px < cx + 50.0


def test_box_corners():
    flat, res = _result(0.0), _result(3.5)
    assert flat.box_corners(0) == [(10.0, 20.0), (110.0, 20.0), (110.0, 60.0), (10.0, 60.0)]     # angle 0: the box
    assert res.box_corners(1) == [(0.0, 0.0), (177.0, 0.0), (177.0, 16.0), (0.0, 16.0)]
    q = res.box_corners(0)
    side = lambda a, b: math.hypot(b[0] - a[0], b[1] - a[1])   # noqa: E731
    assert [side(q[i], q[(i + 1) % 4]) for i in range(4)] == pytest.approx([100.0, 40.0, 100.0, 40.0], rel=1e-4)     # a rigid turn
    assert q[1][1] - q[0][1] == pytest.approx(100.0 * math.sin(math.radians(3.5)), abs=1e-2)


def test_page_result_without_angles_is_unchanged():
    from acai_omr_amd.page import PageResult
    res = PageResult([[(10, 20, 110, 60)]], None, None, None, [0], [(32, 64)], [(0, 0, 32, 64)])
    assert res.angles == [0.0] and res.to_page_xy(0, -0.5, -0.5) == pytest.approx((9.5, 19.5))
    with pytest.raises(ValueError):
        PageResult([[(10, 20, 110, 60)]], None, None, None, [0], [(32, 64)], [(0, 0, 32, 64)], angles=[1.0])      # a turn needs the page size


def test_deskew_ops_refuse_cpu_tensors():
    from acai_omr_amd import ops
    page = torch.from_numpy(D.synthetic_page()[0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.page_strips(page, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.page_skew_scores(torch.zeros(20, 360, dtype=torch.uint8), 320, 16, [0, 100])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.page_rotate(page, 1.0)
    with pytest.raises(ValueError):
        ops.page_strips(page, 12)
    if not torch.cuda.is_available():                            # the host entry points refuse as well when there is no GPU to upload to
        from acai_omr_amd.page import deskew_pages, estimate_skew
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            estimate_skew(page)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            deskew_pages([page], 1.0)
