"""Page illumination flattening on the GPU (csrc/flatten.hip through ops.page_tile_levels / page_flatten, page.flatten_pages and
page_inference(flatten=...)).

Bars: every step is defined in integers and the fp32 output is one correctly rounded fp32 multiply, so tile levels and flattened pages -
uint8 AND fp32 - are torch.equal to the numpy restatement (tests/flatten_reference.py); page_inference(flatten=True) returns seqs, seq_mask
and log_probs torch.equal to page_inference of the page flattened beforehand."""
import numpy as np
import pytest
import torch

import deskew_reference as D
import flatten_reference as F

pytestmark = pytest.mark.gpu

H = 70            # more than one tile row at 16, 32 and 64 and a partial last one; less than one tile at 128
WIDTHS = [1, 15, 16, 17, 255, 257, 1000]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from acai_omr_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _pages(W, seed):
    """A uint8 page with paper, ink and a brightness ramp (so that neighbouring tiles differ), and an fp32 page of values that are no
    multiples of 1 / 255."""
    rng = np.random.RandomState(seed)
    mask = rng.rand(H, W) < 0.3
    u8 = np.where(mask, rng.randint(0, 91, mask.shape), rng.randint(200, 256, mask.shape)).astype(np.uint8)
    u8 = F.shade(u8, F.ramp_gain(H, W, 0.35, 0.3))
    f32 = (u8.astype(np.float32) / np.float32(255.0) * rng.uniform(0.9, 1.0, size=u8.shape).astype(np.float32)).astype(np.float32)
    return u8, f32


def _views(arr, dev):
    """name -> the same page as a GPU tensor: contiguous, in rows 16 bytes apart with INK in the padding, shifted by one column (on no
    16-byte boundary), and (1, H, W)."""
    h, W = arr.shape
    t = torch.from_numpy(arr)
    pitch = -(-(W + 5) // 16) * 16
    wide = torch.zeros(h, pitch, dtype=t.dtype)
    wide[:, :W] = t
    shifted = torch.zeros(h, W + 2, dtype=t.dtype)
    shifted[:, 1:W + 1] = t
    return {"contiguous": t.to(dev), "wide pitch": wide.to(dev)[:, :W], "shifted": shifted.to(dev)[:, 1:W + 1], "(1,H,W)": t.to(dev)[None]}


# ---- 1. tile levels ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", WIDTHS)
def test_tile_levels_match_reference(dev, W):
    from acai_omr_amd import ops
    for arr in _pages(W, 100 + W):
        views = _views(arr, dev)
        for T in F.TILES:
            for percent in (1, 50, 100):
                want = torch.from_numpy(F.tile_levels(arr, T, percent))
                assert want.shape == (-(-H // T), -(-W // T))
                for name, page in views.items():
                    got = ops.page_tile_levels(page, T, percent)
                    assert got.dtype == torch.uint8 and got.is_contiguous() and torch.equal(got.cpu(), want), (W, str(arr.dtype), T, percent, name)


def test_tile_levels_every_value_and_constant(dev):
    from acai_omr_amd import ops
    every = np.arange(256, dtype=np.uint8).reshape(16, 16)             # one tile of 16 holding every level once: rank r is level r - 1
    for percent in (1, 2, 50, 99, 100):
        got = ops.page_tile_levels(torch.from_numpy(every).to(dev), 16, percent)
        assert got.cpu().tolist() == [[max(1, (256 * percent + 99) // 100) - 1]] == F.tile_levels(every, 16, percent).tolist()
    rng = np.random.RandomState(7)
    spread = rng.permutation(np.arange(256 * 35, dtype=np.int64) % 256).astype(np.uint8).reshape(70, 128)   # every value 35 times
    f32 = rng.rand(70, 128).astype(np.float32)                          # every level of fp32 values, and what rounds to them
    f32[0, :8] = [0.0, 1.0, 0.5 / 255, np.nextafter(np.float32(0.5 / 255), np.float32(0)), 254.5 / 255, 0.5, 127.5 / 255, 1e-9]
    for arr in (spread, f32):
        for T in F.TILES:
            for percent in (1, 50, 100):
                assert torch.equal(ops.page_tile_levels(torch.from_numpy(arr).to(dev), T, percent).cpu(), torch.from_numpy(F.tile_levels(arr, T, percent))), (T, percent)
    for value in (0, 37, 255):                                         # a constant page: one bin takes every add
        const = np.full((70, 100), value, dtype=np.uint8)
        for T in (16, 64):
            got = ops.page_tile_levels(torch.from_numpy(const).to(dev), T, 50).cpu()
            assert got.shape == (-(-70 // T), -(-100 // T)) and (got == value).all()
        got = ops.page_tile_levels(torch.from_numpy(const).to(dev).float() / 255.0, 32, 50).cpu()
        assert (got == value).all()


# ---- 2. flatten --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", WIDTHS)
def test_flatten_matches_reference(dev, W):
    from acai_omr_amd import ops
    rng = np.random.RandomState(200 + W)
    for arr in _pages(W, 300 + W):
        views = _views(arr, dev)
        for T in F.TILES:
            shape = (-(-H // T), -(-W // T))
            grids = {"random": rng.randint(0, 256, size=shape).astype(np.uint8), "of the page": F.tile_levels(arr, T, 50)}
            for gname, g in grids.items():
                gd = torch.from_numpy(g).to(dev)
                for rq in (0, 85, 256):
                    for floor in (1, 32, 255):
                        want = torch.from_numpy(F.flatten_with_grid(arr, g, T, rq, floor))
                        some = views if (rq, floor) == (85, 32) else {"contiguous": views["contiguous"]}   # every view at the defaults
                        for name, page in some.items():
                            got = ops.page_flatten(page, gd, T, rq, floor)
                            assert got.dtype == page.dtype and got.shape == (H, W) and got.is_contiguous()
                            assert torch.equal(got.cpu(), want), (W, str(arr.dtype), T, gname, rq, floor, name)   # bitwise, fp32 too


@pytest.mark.parametrize("W", [1, 17, 257, 1000])
def test_flatten_out_view_and_input_untouched(dev, W):
    from acai_omr_amd import ops
    for arr in _pages(W, 400 + W):
        T = 16
        g = F.tile_levels(arr, T, 50)
        gd = torch.from_numpy(g).to(dev)
        want = torch.from_numpy(F.flatten_with_grid(arr, g, T, 85, 32))
        page = torch.from_numpy(arr).to(dev)
        keep = page.clone()
        sentinel = 7 if arr.dtype == np.uint8 else 0.25
        pitch = -(-(W + 5) // 16) * 16
        for left in (0, 1):                                            # rows on 16-byte boundaries, and a view on none
            buf = torch.full((H, pitch), sentinel, dtype=page.dtype, device=dev)
            view = buf[:, left:left + W]
            assert ops.page_flatten(page, gd, T, 85, 32, out=view) is view
            assert torch.equal(view.cpu(), want), (W, left)
            pad = torch.ones(H, pitch, dtype=torch.bool)
            pad[:, left:left + W] = False
            assert (buf.cpu()[pad] == sentinel).all(), (W, left)       # nothing written outside the view
        assert torch.equal(page, keep)                                 # the input is not modified
        with pytest.raises(ValueError):
            ops.page_flatten(page, gd, T, 85, 32, out=page)            # not in place
        with pytest.raises(ValueError):
            ops.page_flatten(page, gd, T, 85, 32, out=torch.empty(H, W + 1, dtype=page.dtype, device=dev))


def test_refusals(dev):
    from acai_omr_amd import ops
    page = torch.full((70, 100), 200, dtype=torch.uint8, device=dev)
    g = ops.page_tile_levels(page, 16, 50)
    assert g.shape == (5, 7)
    for bad in (g[:4], g[:, :6], g.float(), g.to(torch.int32), g.cpu(), g.t().contiguous().t()):
        with pytest.raises(ValueError):
            ops.page_flatten(page, bad, 16, 85, 32)
    with pytest.raises(ValueError):
        ops.page_flatten(page, g, 32, 85, 32)                          # the grid of another tile
    for tile in (24, 8, 256):
        with pytest.raises(ValueError):
            ops.page_tile_levels(page, tile, 50)
        with pytest.raises(ValueError):
            ops.page_flatten(page, g, tile, 85, 32)
    for percent in (0, 101, 50.5):
        with pytest.raises(ValueError):
            ops.page_tile_levels(page, 16, percent)
    for rq, floor in ((-1, 32), (257, 32), (85, 0), (85, 256)):
        with pytest.raises(ValueError):
            ops.page_flatten(page, g, 16, rq, floor)


# ---- 3. flatten, then detect -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shaded():
    """The synthetic page, its boxes, and the page under the 1.0 -> 0.35 ramp with its restatement's flattening (tile 16, the default at 360
    rows), computed once."""
    from acai_omr_amd.page import DetectConfig
    page = D.synthetic_page(0)[0]
    boxes = D.detect(page, DetectConfig().resolved(360, 320))
    ramp = F.shade(page, F.ramp_gain(360, 320, 0.35))
    return page, boxes, ramp, F.flatten(ramp)


def test_flatten_then_detect(dev, shaded):
    from acai_omr_amd.page import FlattenConfig, detect_systems, flatten_pages
    page, boxes, ramp, want = shaded
    assert len(boxes) == 3 and len(detect_systems(torch.from_numpy(ramp).to(dev))) < 3     # what flattening is for
    (flat,) = flatten_pages(torch.from_numpy(ramp).to(dev))
    assert torch.equal(flat.cpu(), torch.from_numpy(want))
    assert detect_systems(flat) == boxes
    assert torch.equal(flat.cpu() < 128, torch.from_numpy(page) < 128)
    # a list, from the host, fp32, and a config
    f32 = torch.from_numpy(ramp).float() / 255.0
    out = flatten_pages([torch.from_numpy(ramp), f32[None]], FlattenConfig(tile=32, ink_ratio=0.25, floor=40))
    assert [o.dtype for o in out] == [torch.uint8, torch.float32] and all(o.is_cuda and o.shape == (360, 320) for o in out)
    assert torch.equal(out[0].cpu(), torch.from_numpy(F.flatten(ramp, 32, 50, 64, 40)))
    assert torch.equal(out[1].cpu(), torch.from_numpy(F.flatten(f32.numpy(), 32, 50, 64, 40)))
    assert detect_systems(out[1]) == boxes


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e(dev):
    from conftest import load_golden
    from decode_support import build_vitomr
    from acai_omr_amd.utils import DynamicResize
    fx = load_golden("vitomr_dh64b")
    cfg = fx["cfg"]
    m = build_vitomr(cfg, fx["state_dict"], dev, torch.bfloat16, max_batch=2)
    return m, DynamicResize(16, 32, 4, 8, True)


def _same(a, b):
    return torch.equal(a.seqs, b.seqs) and torch.equal(a.log_probs, b.log_probs) and torch.equal(a.seq_mask, b.seq_mask) and a.boxes == b.boxes


def test_page_inference_flatten(dev, e2e, shaded):
    from acai_omr_amd.inference.vitomr_inference import page_inference
    from acai_omr_amd.page import FlattenConfig, flatten_pages
    m, tr = e2e
    page, boxes, ramp, _ = shaded
    ramp_d, level = torch.from_numpy(ramp).to(dev), torch.from_numpy(page).to(dev)
    off_before = page_inference(m, level, "cuda", tr, max_inference_len=12, flatten=None)
    assert len(off_before) == 3 and off_before.flattened == [False]
    (flat,) = flatten_pages(ramp_d)
    want = page_inference(m, flat, "cuda", tr, max_inference_len=12)                                   # flattened beforehand
    assert len(want) == 3 and want.boxes == [boxes]
    res = page_inference(m, ramp_d, "cuda", tr, max_inference_len=12, flatten=True)
    assert _same(res, want) and res.flattened == [True] and res.angles == [0.0] and res.page_sizes == [(360, 320)]
    assert _same(page_inference(m, ramp_d, "cuda", tr, max_inference_len=12, flatten=FlattenConfig()), want)
    assert len(page_inference(m, ramp_d, "cuda", tr, max_inference_len=12)) < 3                        # without it the shaded page loses systems
    # off: None and False are the present path, before and after a flatten call in the same process
    for off in (None, False):
        again = page_inference(m, level, "cuda", tr, max_inference_len=12, flatten=off)
        assert _same(again, off_before) and again.flattened == [False]
    with pytest.raises(TypeError):
        page_inference(m, level, "cuda", tr, max_inference_len=12, flatten=16)


def test_page_inference_flatten_and_deskew(dev, e2e, shaded):
    """Tilted by 2 degrees, then shaded.  By hand: flatten, estimate the skew of the flattened page, level it, run the plain call.  At tile 32
    the levelled page has its 3 systems (restated on the CPU); at the default tile of this small page (16) the gain of the flattening
    lifts the grey rims that the resampling left on the 2-row staff lines over the threshold and the rule finds none - equal on both
    paths all the same."""
    from acai_omr_amd import ops
    from acai_omr_amd.inference.vitomr_inference import page_inference
    from acai_omr_amd.page import FlattenConfig, estimate_skew, flatten_pages
    m, tr = e2e
    page = shaded[0]
    both = torch.from_numpy(F.shade(D.rotate_deg(page, -2.0), F.ramp_gain(360, 320, 0.35))).to(dev)
    for flatten, systems in ((FlattenConfig(tile=32), 3), (True, None)):
        (flat,) = flatten_pages(both, None if flatten is True else flatten)
        angle = estimate_skew(flat)[0]
        assert abs(angle - 2.0) <= 0.125
        want = page_inference(m, ops.page_rotate(flat, angle), "cuda", tr, max_inference_len=12)
        res = page_inference(m, both, "cuda", tr, max_inference_len=12, flatten=flatten, deskew=True)
        assert res.boxes == want.boxes and len(res) == len(want) and res.flattened == [True] and res.angles == [angle]
        if systems is not None:
            assert len(want) == systems
        if len(want):
            assert _same(res, want)
