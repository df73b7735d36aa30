"""The host code that strings the page stages together, without a GPU: the geometry of `page.PageResult` held, with `==`, to what the
commit before the stage table computed (tests/golden/page_geometry.json, recorded by tools/record_page_geometry.py: 8 orientation codes x
3 angles x quad or none x 2 insets, two systems each), and the one rule for stage keywords (`page.resolve_stage`) tabled for the five
stages - every accepted form, and the rejected ones, which must be refused before anything is uploaded or launched."""
import json
import os
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. frozen geometry -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "page_geometry.json")) as f:
        return json.load(f)


def _result(case):
    from acai_omr_amd.page import PageResult
    n = len(case["boxes"])
    return PageResult([[tuple(b) for b in case["boxes"]]], None, None, None, [0] * n, [tuple(s) for s in case["sizes"]],
                      [tuple(w) for w in case["windows"]], angles=[case["angle"]], page_sizes=[tuple(case["page_size"])], quads=[case["quad"]],
                      source_sizes=[tuple(case["source_size"])], inset=case["inset"], orientations=[case["code"]])


def _typed(v):
    """Nested sequences as lists, every number with the name of its type: 1 == 1.0, and an int must stay an int."""
    return [_typed(x) for x in v] if isinstance(v, (list, tuple)) else (type(v).__name__, v)


def test_golden_covers_every_combination(golden):
    seen = {(c["inputs"]["code"], c["inputs"]["angle"], c["inputs"]["quad"] is not None, c["inputs"]["inset"]) for c in golden["cases"]}
    assert seen == {(code, a, q, i) for code in range(1, 9) for a in (0.0, 2.5, -7.25) for q in (False, True) for i in (0, 2)} and len(golden["cases"]) == 96
    assert golden["points"] == [[0, 0], [5.0, 3.0], [31.5, 15.25]]
    for c in golden["cases"]:
        inp = c["inputs"]
        assert len(inp["boxes"]) == 2 and inp["boxes"][0] != inp["boxes"][1] and inp["sizes"][0] != inp["sizes"][1]
        assert all(w[0] > 0 or w[1] > 0 for w in inp["windows"]) and inp["source_size"] == (inp["page_size"] if inp["code"] <= 4 else inp["page_size"][::-1])


def test_page_result_geometry_is_what_it_was(golden):
    """No tolerance: each map is the same operations in the same order as before the maps became a list."""
    for c in golden["cases"]:
        res, inp = _result(c["inputs"]), {k: c["inputs"][k] for k in ("code", "angle", "inset")}
        for s in range(2):
            assert _typed(res.box_corners(s)) == _typed(c["box_corners"][s]), (inp, s)
            for p, want, back in zip(golden["points"], c["to_page_xy"][s], c["from_page_xy"][s]):
                got = res.to_page_xy(s, *p)
                assert _typed(got) == _typed(want), (inp, s, p)
                assert _typed(res.from_page_xy(s, *got)) == _typed(back), (inp, s, p)


def test_page_result_chain_has_a_map_per_stage_that_did_something(golden):
    """turn, homography, orientation, in that order; to_source_xy applies them one after the other and from_source_xy undoes them."""
    from acai_omr_amd.page import homography_map, orientation_map, turn_map
    for c in golden["cases"]:
        inp = c["inputs"]
        res = _result(inp)
        want = [m for on, m in ((inp["angle"] != 0.0, turn_map(inp["angle"], inp["page_size"])),
                                (inp["quad"] is not None, homography_map(inp["quad"], inp["page_size"], inp["inset"])),
                                (inp["code"] != 1, orientation_map(inp["code"], inp["source_size"]))) if on]
        x, y = 17, 40
        for m in want:
            x, y = m.back(x, y)
        assert _typed(res.to_source_xy(0, 17, 40)) == _typed((x, y))
        if inp["angle"] == 0.0 and inp["quad"] is None:          # nothing but the orientation: a pixel for a pixel, Python ints
            assert all(type(v) is int for v in (x, y)) and res.from_source_xy(0, x, y) == (17, 40)
        else:
            assert res.from_source_xy(0, x, y) == pytest.approx((17, 40), abs=1e-6)


# ---- 2. the stage rule --------------------------------------------------------------------------------------------------------------------
QUAD = [(20.5, 15.0), (180.0, 22.25), (172.5, 220.0), (12.0, 210.5)]
MALFORMED_QUAD = [(20.5, 15.0), (180.0, 22.25), (172.5, 220.0)]
MESSAGES = {
    "orient": "orient: expected None, a bool, a page.OrientConfig, one EXIF orientation code 1 .. 8 or a list with one per page",
    "rectify": "rectify: expected None, a bool, a page.RectifyConfig, one quad [TL, TR, BR, BL] or a list of quads (or None) per page",
    "flatten": "flatten: expected None, a bool or a page.FlattenConfig",
    "deskew": "deskew: expected None, a bool, a page.SkewConfig, one angle in degrees or a list with one per page",
    "assess": "assess: expected None, a bool or a page.AssessConfig",
}
EXPLICIT = {"orient": [1, 6, [6, 1], (3,)], "rectify": [QUAD, [list(c) for c in QUAD], [QUAD, None], [None]], "flatten": [], "deskew": [2.5, 0, 0.0, -7, [1.0, -2], (0.5,)],
            "assess": []}
TYPE_ERRORS = {"orient": ["upright", 1.5, {}], "rectify": [MALFORMED_QUAD, [MALFORMED_QUAD], "yes", 4], "flatten": [16, "yes", 0.5], "deskew": ["yes", [1.0, "x"], [True], {}],
               "assess": ["yes", 3]}


def _configs():
    from acai_omr_amd import page
    return {"orient": page.OrientConfig, "rectify": page.RectifyConfig, "flatten": page.FlattenConfig, "deskew": page.SkewConfig, "assess": page.AssessConfig}


@pytest.mark.parametrize("name", ["orient", "rectify", "flatten", "deskew", "assess"])
def test_resolve_stage(name):
    from acai_omr_amd.page import resolve_stage
    Config = _configs()[name]
    for off in (None, False):
        assert resolve_stage(name, off) == (None, None)
    assert resolve_stage(name, True) == (Config(), None)                     # estimate with the defaults
    cfg = Config()
    got = resolve_stage(name, cfg)
    assert got[0] is cfg and got[1] is None                                  # estimate with the caller's config
    for value in EXPLICIT[name]:
        got = resolve_stage(name, value)
        assert got[0] == Config() and got[1] is value, value                 # the caller's values, as given
    for bad in TYPE_ERRORS[name]:
        with pytest.raises(TypeError) as e:
            resolve_stage(name, bad)
        assert str(e.value) == MESSAGES[name], bad


def test_bad_stage_keywords_are_refused_before_anything_is_uploaded(monkeypatch):
    """Both entry points, every rejected form: the exception of before, and no call that reaches the device - also when a stage ahead of
    the bad one is on and would have launched (orient=6 in front of a bad flatten)."""
    from acai_omr_amd import page as pg
    from acai_omr_amd.inference.vitomr_inference import page_inference

    def refuse(*a, **k):
        raise AssertionError("the device was reached before the stage keywords were checked")

    for name in ("_device_page", "_device_photo", "ingest_pages", "rectify_pages", "flatten_pages", "deskew_pages", "estimate_orientation", "assess_counts", "detect_systems"):
        monkeypatch.setattr(pg, name, refuse)
    monkeypatch.setattr(torch.cuda, "is_available", refuse)
    page = torch.full((60, 40), 255, dtype=torch.uint8)
    resize = types.SimpleNamespace(device=None)
    bad = [(TypeError, {k: v}) for k, values in TYPE_ERRORS.items() for v in values]
    bad += [(TypeError, dict(orient=[1.5])), (ValueError, dict(orient=0)), (ValueError, dict(orient=9)), (ValueError, dict(orient=[1, 1]))]
    bad += [(TypeError, dict(orient=6, flatten=16)), (TypeError, dict(orient=True, rectify=True, deskew="yes")), (TypeError, dict(rectify=QUAD, orient="upright"))]
    for exc, kw in bad:
        with pytest.raises(exc):
            page_inference(None, page, "cuda", resize, max_inference_len=4, **kw)
        if "assess" not in kw:
            with pytest.raises(exc):
                pg.prepare_pages(page, None, **kw)
    with pytest.raises(AssertionError):                                      # the guard itself: a good call does reach the device
        pg.prepare_pages(page, None, orient=6)
