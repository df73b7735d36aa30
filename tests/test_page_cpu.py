"""Whole-page input, the parts that need no GPU: the numpy restatement of the detection rule on a page whose systems are known, and the host
edge (acai_omr_amd/page.py): the UI's fraction boxes, PageResult's joins and confidence figures against the formulas of the reference's
service (acai_omr/ui/routes.py), the map back to page pixels, and the refusals without a GPU."""
import math

import numpy as np
import pytest
import torch

import page_reference as R

DETECT = dict(min_ink=1, merge_gap=4, min_height=8, line_len=100, min_line_rows=5, margin=0)
TRUTH = [(14, 37, 191, 74), (14, 107, 191, 123), (14, 167, 191, 204)]


def test_reference_finds_the_systems_of_the_synthetic_page():
    page, truth = R.synthetic_page()
    assert page.shape == (240, 200) and truth == TRUTH
    ink, run = R.profile(page)
    found, kept = R.bands(ink, run, 1, 4, 8, 100, 5)
    assert (8, 16) in found and (8, 16) not in kept              # the title: tall enough, but no row with a 100-pixel run
    assert any(b - a < 8 for a, b in found)                      # the page number: a band that is too short
    assert kept == [(y0, y1) for _, y0, _, y1 in TRUTH]
    assert R.systems(page, 0.5, max_systems=64, **DETECT) == (3, TRUTH)
    assert R.systems(page, 0.5, max_systems=2, **DETECT) == (3, TRUTH[:2])
    assert R.systems((page.astype(np.float32) / 255.0), 0.5, max_systems=64, **DETECT) == (3, TRUTH)
    m = dict(DETECT, margin=20)
    assert R.systems(page, 0.5, max_systems=64, **m)[1] == R.truth_boxes_with_margin(TRUTH, 20, 240, 200)


def test_reference_profile_by_hand():
    row = np.full((3, 12), 255, dtype=np.uint8)
    row[0, [0, 1, 2, 5, 6, 7, 11]] = 0        # two runs of three and one at the last pixel
    row[1, :] = 10                            # a full-width run
    ink, run = R.profile(row)
    assert ink.tolist() == [7, 12, 0] and run.tolist() == [3, 12, 0]
    assert R.profile(np.array([[127, 128]], dtype=np.uint8))[0].tolist() == [1]   # 127 / 255 < 0.5 <= 128 / 255


def test_boxes_from_fractions():
    from acai_omr_amd.page import boxes_from_fractions
    assert boxes_from_fractions([(0.0725, 0.1625, 0.9575, 0.4375)], 240, 200) == [(14, 39, 192, 105)]
    ui = [{"x0": 0.1, "y0": 0.7, "x1": 0.9, "y1": 0.8}, {"x0": 0.0725, "y0": 0.1625, "x1": 0.9575, "y1": 0.4375}, (0.0, 0.5, 1.0, 0.6)]
    got = boxes_from_fractions(ui, 240, 200)
    assert got == [(14, 39, 192, 105), (0, 120, 200, 144), (20, 168, 180, 192)]   # sorted by y0
    assert got == R.boxes_from_fractions(ui, 240, 200)
    assert boxes_from_fractions([(0.0125, 0.0, 0.0375, 1.0)], 10, 200) == [(2, 0, 8, 10)]   # 2.5 -> 2, 7.5 -> 8: ties go to even
    assert boxes_from_fractions([], 240, 200) == []


@pytest.mark.parametrize("box", [(0.5, 0.2, 0.5, 0.4), (0.2, 0.401, 0.8, 0.4), (-0.1, 0.1, 0.5, 0.5), (0.1, 0.1, 1.1, 0.5), (0.1, 0.1, 0.5, 1.01),
                                 (0.6, 0.1, 0.4, 0.5)])
def test_boxes_from_fractions_refuses_empty_and_outside(box):
    from acai_omr_amd.page import boxes_from_fractions
    with pytest.raises(ValueError):
        boxes_from_fractions([box], 240, 200)


def _result():
    from acai_omr_amd.page import PageResult
    BOS, EOS, PAD = 1, 2, 0
    seqs = torch.tensor([[BOS, 5, 6, EOS, PAD], [BOS, 7, EOS, PAD, PAD], [BOS, 8, 9, 10, 11]])
    mask = torch.tensor([[1, 1, 1, 1, 0], [1, 1, 1, 0, 0], [1, 1, 1, 1, 1]], dtype=torch.bool)
    lps = torch.tensor([[0.0, -0.5, -0.25, -0.125, 0.0], [0.0, -1.0, -2.0, 0.0, 0.0], [0.0, -0.1, -0.2, -0.3, -0.4]])
    boxes = [[(10, 20, 110, 60), (10, 80, 110, 120)], [], [(0, 0, 177, 16)]]
    sizes, windows = [(32, 64), (32, 64), (16, 176)], [(0, 0, 32, 64), (0, 0, 32, 64), (0, 24, 16, 128)]
    return PageResult(boxes, seqs, lps, mask, [0, 0, 2], sizes, windows, (BOS, EOS, PAD)), seqs, mask, lps


def test_page_result_joins_and_confidence():
    res, seqs, mask, lps = _result()
    assert len(res) == 3
    assert [t.tolist() for t in res.tokens()] == [[5, 6, 7], [], [8, 9, 10, 11]]
    names = {0: "<pad>", 1: "<bos>", 2: "<eos>", 5: "a", 6: "b", 7: "c", 8: "d", 9: "e", 10: "f", 11: "g"}
    from acai_omr_amd.utils import stringify_lmx_seq
    assert res.lmx(names) == ["a b c", "", "d e f g"]
    assert res.lmx(names)[0] == " ".join(stringify_lmx_seq(seqs[i][mask[i]], names) for i in (0, 1))      # routes.py:74-80, :179
    want = [float(lps[i][mask[i]].sum() / mask[i].sum()) for i in range(3)]                                 # routes.py:83
    assert res.avg_log_probs.tolist() == pytest.approx(want, abs=1e-7)
    conf = res.avg_confidence
    assert conf[0] == pytest.approx(torch.exp(torch.tensor(sum(want[:2]) / 2)).item(), rel=1e-6)           # routes.py:190
    assert math.isnan(conf[1]) and conf[2] == pytest.approx(math.exp(want[2]), rel=1e-6)


def test_empty_page_result():
    from acai_omr_amd.page import PageResult
    res = PageResult([[], []], None, None, None, [], [], [])
    assert len(res) == 0 and [t.numel() for t in res.tokens()] == [0, 0] and res.lmx({}) == ["", ""]
    assert res.avg_log_probs.numel() == 0 and all(math.isnan(c) for c in res.avg_confidence)


def test_to_page_xy():
    res, *_ = _result()
    # system 0: a 100 x 40 box at (10, 20) resized to 64 x 32, no crop: output pixel centres map onto the box, corner to corner
    assert res.to_page_xy(0, -0.5, -0.5) == pytest.approx((9.5, 19.5))
    assert res.to_page_xy(0, 63.5, 31.5) == pytest.approx((109.5, 59.5))
    assert res.to_page_xy(0, 0, 0) == pytest.approx((10 + 0.5 * 100 / 64 - 0.5, 20 + 0.5 * 40 / 32 - 0.5))
    # system 2: 177 x 16 at the origin resized to 176 x 16, columns 24 .. 151 kept: window pixel 0 is resized pixel 24
    assert res.to_page_xy(2, 0, 0) == pytest.approx((24.5 * 177 / 176 - 0.5, 0.0))
    for s in range(3):
        for xy in [(0.0, 0.0), (17.25, 9.5), (63.0, 15.0)]:
            assert res.from_page_xy(s, *res.to_page_xy(s, *xy)) == pytest.approx(xy, abs=1e-9)


def test_plan_matches_dynamic_resize():
    from acai_omr_amd.page import plan_systems
    from acai_omr_amd.utils import DynamicResize
    tr = DynamicResize(16, 32, 4, 8, True)
    plans = plan_systems([(240, 200), (50, 300)], [[(14, 37, 191, 74)], [(0, 0, 177, 16), (1, 2, 21, 11)]], tr)
    assert [p for p, *_ in plans] == [0, 1, 1]
    assert plans[1][2:] == ((16, 176), (0, 24, 16, 128)) and plans[1][2:] == tr._plan(16, 177)
    assert plans[2][2:] == tr._plan(9, 20)
    with pytest.raises(ValueError):
        plan_systems([(240, 200)], [[(14, 37, 201, 74)]], tr)


def test_packed_patches_slice():
    from acai_omr_amd.utils import PackedPatches
    pk = PackedPatches(torch.arange(9 * 4).view(9, 4), [(1, 2), (2, 2), (3, 1)], 2)
    a, b = pk.slice(0, 2), pk.slice(2, 5)
    assert a.dims == [(1, 2), (2, 2)] and torch.equal(a.patches, pk.patches[:6]) and a.patch_size == 2
    assert b.dims == [(3, 1)] and torch.equal(b.patches, pk.patches[6:]) and len(pk.slice(1, 1)) == 0
    assert a.patches.data_ptr() == pk.patches.data_ptr()     # a view, not a copy


def test_page_entry_points_refuse_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from acai_omr_amd import ops
    from acai_omr_amd.inference.vitomr_inference import page_inference
    from acai_omr_amd.page import detect_systems, split_pages
    from acai_omr_amd.utils import DynamicResize
    page = torch.from_numpy(R.synthetic_page()[0])
    tr = DynamicResize(16, 32, 4, 8, True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        split_pages(page, TRUTH, tr)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        detect_systems(page)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        page_inference(None, page, "cuda", tr, boxes=TRUTH)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.page_profile(page)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.page_systems(page, torch.zeros(240, dtype=torch.int32), torch.zeros(240, dtype=torch.int32), 0.5, 1, 4, 8, 100, 5, 0, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.crop_resize_to_patches([], torch.empty(4, 256), 16)
    with pytest.raises(TypeError):
        detect_systems("not a tensor")
