"""Page ingest on the GPU (csrc/ingest.hip through ops.page_ingest / page_col_profile / page_box_ink, page.ingest_pages /
estimate_orientation and page_inference(orient=...)).

Bars: everything is defined in integers (or moves bits), so every comparison is torch.equal to the numpy restatement
(tests/ingest_reference.py); page_inference(orient=code) on the turned colour photo returns the rows of page_inference on the grey upright
page, and orient=True those of orient=<the estimated codes>."""
import numpy as np
import pytest
import torch

import deskew_reference as D
import ingest_reference as G
import page_reference as P
import rectify_reference as Q

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from acai_omr_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ---- 1. acai_page_ingest: shapes, layouts, strides, bounds -------------------------------------------------------------------------------
# name -> (layout argument, what of the (H, W, 4) base array it holds, how the tensor is made of that).  The last two are views whose pixels
# are not adjacent (a channel slice of a wider pixel): the kernel's byte-by-byte form.
LAYOUTS = {
    "(H,W)": (None, lambda a: a[..., 0], lambda t: t),
    "(1,H,W)": ("chw", lambda a: a[..., :1], lambda t: t.permute(2, 0, 1)),
    "(H,W,3)": ("hwc", lambda a: a[..., :3], lambda t: t),
    "(3,H,W)": ("chw", lambda a: a[..., :3], lambda t: t.permute(2, 0, 1)),
    "(H,W,4)": ("hwc", lambda a: a, lambda t: t),
    "(H,W,3) of RGBA": ("hwc", lambda a: a[..., :3], None),
    "(H,W) of RGB": (None, lambda a: a[..., 1], None),
}
SIZES = [(1, 1), (1, 7), (5, 1), (3, 4), (63, 65), (64, 64), (65, 63), (67, 130), (130, 67), (1, 300), (300, 1)]


def _tensor(name, base, padded, dev):
    """The layout `name` of the (H, W, 4) array `base` on the device: contiguous, or (padded) a slice of a larger tensor - rows further apart
    than they are long and a first element at an odd offset."""
    layout, pick, make = LAYOUTS[name]
    H, W = base.shape[:2]
    if make is None:                                             # a channel slice of the interleaved base
        big = torch.from_numpy(np.ascontiguousarray(base if name.endswith("RGBA") else base[..., :3])).to(dev)
        if padded:
            wide = torch.full((H + 2, W + 3, big.shape[2]), 7, dtype=torch.uint8, device=dev)
            wide[1:H + 1, 2:W + 2] = big
            big = wide[1:H + 1, 2:W + 2]
        return (big[..., :3] if name.endswith("RGBA") else big[..., 1]), layout
    src = torch.from_numpy(np.ascontiguousarray(pick(base)))
    src = src if src.dim() == 2 else make(src).contiguous()
    if not padded:
        return src.to(dev), layout
    shape = list(src.shape)
    hd, wd = (0, 1) if src.dim() == 2 or layout == "hwc" else (1, 2)
    shape[hd] += 2
    shape[wd] += 3
    wide = torch.full(shape, 7, dtype=torch.uint8, device=dev)
    view = wide.narrow(hd, 1, H).narrow(wd, 2, W)
    view.copy_(src)
    return view, layout


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ingest_every_code_layout_and_stride(dev, size):
    from acai_omr_amd import ops
    H, W = size
    base = np.random.RandomState(H * 1000 + W).randint(0, 256, size=(H, W, 4)).astype(np.uint8)
    for name, (_, pick, _) in LAYOUTS.items():
        want = {code: torch.from_numpy(G.ingest(pick(base), code)) for code in range(1, 9)}
        for padded in (False, True):
            src, layout = _tensor(name, base, padded, dev)
            for code in range(1, 9):
                OH, OW = want[code].shape
                got = ops.page_ingest(src, code, layout)
                assert got.dtype == torch.uint8 and got.shape == (OH, OW) and got.is_contiguous()
                assert torch.equal(got.cpu(), want[code]), (name, padded, code)
                # into a view of a larger buffer, on no word boundary: the bytes around it stay as they were
                buf = torch.full((OH + 2, OW + 5), SENTINEL, dtype=torch.uint8, device=dev)
                view = buf[1:OH + 1, 3:3 + OW]
                assert ops.page_ingest(src, code, layout, out=view) is view
                host = buf.cpu()
                assert torch.equal(host[1:OH + 1, 3:3 + OW], want[code]), (name, padded, code)
                host[1:OH + 1, 3:3 + OW] = SENTINEL
                assert (host == SENTINEL).all(), (name, padded, code)


def test_ingest_reads_shapes_as_documented(dev):
    from acai_omr_amd import ops
    from acai_omr_amd.page import ingest_pages
    rng = np.random.RandomState(3)
    rgb = rng.randint(0, 256, size=(20, 30, 3)).astype(np.uint8)
    want = torch.from_numpy(G.ingest(rgb, 6))
    for t in (torch.from_numpy(rgb), torch.from_numpy(rgb).permute(2, 0, 1).contiguous(), torch.from_numpy(rgb).permute(2, 0, 1)):
        assert torch.equal(ops.page_ingest(t.to(dev), 6).cpu(), want)                     # (H,W,3), (3,H,W) and a permuted view of either
        assert torch.equal(ingest_pages(t, 6)[0].cpu(), want)                             # a CPU tensor is uploaded as it is
    rgba = np.concatenate([rgb, rng.randint(0, 256, size=(20, 30, 1)).astype(np.uint8)], -1)
    assert torch.equal(ops.page_ingest(torch.from_numpy(rgba).to(dev), 6).cpu(), want)    # the fourth channel is ignored
    grey = torch.from_numpy(rgb[..., 0].copy()).to(dev)
    out = ingest_pages([grey, grey[None], torch.from_numpy(rgb)], [1, 1, 3])
    assert out[0] is grey and out[1].data_ptr() == grey.data_ptr() and torch.equal(out[2].cpu(), torch.from_numpy(G.ingest(rgb, 3)))   # code 1, one channel: no copy
    assert torch.equal(ingest_pages(grey, 8)[0].cpu(), torch.from_numpy(G.orient(rgb[..., 0], 8)))
    for bad in (torch.zeros(20, 30, 3, device=dev), torch.zeros(3, 20, 30, device=dev), torch.zeros(2, 20, 30, dtype=torch.uint8, device=dev),
                torch.zeros(20, 30, dtype=torch.int32, device=dev), torch.zeros(4, 20, 30, dtype=torch.uint8, device=dev)[:, :, :29]):
        with pytest.raises(TypeError):
            ops.page_ingest(bad, 1)
    with pytest.raises(ValueError):
        ops.page_ingest(grey, 9)
    with pytest.raises(ValueError):
        ops.page_ingest(grey[:1].expand(20, 30), 1)                                       # rows on top of each other
    with pytest.raises(ValueError):
        ops.page_ingest(grey, 6, out=torch.empty(20, 30, dtype=torch.uint8, device=dev))  # code 6 gives 30 x 20
    with pytest.raises(RuntimeError, match="acai_page_ingest"):
        ops.page_ingest(torch.zeros(2, 16385, dtype=torch.uint8, device=dev), 1)          # wider than a page may be
    assert ops.page_ingest(torch.zeros(2, 16385, dtype=torch.uint8, device=dev), 6).shape == (16385, 2)     # the limits are the OUTPUT's


def test_grey_formula_exhaustive(dev):
    """Every one of the 2^24 colours once, as one 4096 x 4096 x 3 image: no rounding case of the grey formula is left out; with code 1 (the
    row kernel) and code 6 (the tile kernel)."""
    from acai_omr_amd import ops
    idx = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([idx & 255, (idx >> 8) & 255, idx >> 16], -1).astype(np.uint8).reshape(4096, 4096, 3)
    want = G.grey(rgb)
    src = torch.from_numpy(rgb).to(dev)
    assert torch.equal(ops.page_ingest(src, 1), torch.from_numpy(want).to(dev))
    assert torch.equal(ops.page_ingest(src, 6), torch.from_numpy(G.orient(want, 6)).to(dev))


def test_ingest_fp32_moves_bits(dev):
    from acai_omr_amd import ops
    rng = np.random.RandomState(5)
    for H, W in ((1, 1), (5, 7), (65, 130), (130, 63)):
        bits = rng.randint(-2 ** 31, 2 ** 31, size=(H, W), dtype=np.int64).astype(np.int32)        # NaNs with payloads, infinities, subnormals among them
        bits.flat[:4] = np.array([0x7FC00001, -0x003FFFFF, -0x80000000, 0x7F800001][:bits.size], dtype=np.int64).astype(np.int32)   # quiet / signalling NaN, -0.0
        host = torch.from_numpy(bits).view(torch.float32)
        wide = torch.zeros(H + 1, W + 3, dtype=torch.float32)
        wide[1:, 2:W + 2] = host
        for src in (host.to(dev), wide.to(dev)[1:, 2:W + 2], host.to(dev)[None]):
            for code in range(1, 9):
                got = ops.page_ingest(src, code)
                assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32).cpu(), torch.from_numpy(G.orient(bits, code))), (H, W, code)


def test_codes_compose(dev):
    from acai_omr_amd import ops
    rgb = torch.from_numpy(G.colour_page(G.clef_page(0)[0])).to(dev)
    grey = ops.page_ingest(rgb, 1)
    assert torch.equal(grey.cpu(), torch.from_numpy(G.grey(rgb.cpu().numpy())))
    for code in range(1, 9):
        turned = ops.page_ingest(rgb, code)
        assert torch.equal(ops.page_ingest(turned, G.INVERSE[code]), grey) and ops.EXIF_INVERSE[code] == G.INVERSE[code]
        assert torch.equal(ops.page_ingest(grey, code), turned)                               # grey first, or in the same launch
    assert torch.equal(ops.page_ingest(ops.page_ingest(rgb, 6), 6), ops.page_ingest(rgb, 3))


# ---- 2. column profile --------------------------------------------------------------------------------------------------------------------
def _as_f32(u8, rng):
    """An fp32 page with the uint8 page's ink mask at 0.5, the threshold itself among the paper."""
    f = np.where(u8 >= 128, rng.uniform(0.5, 1.0, u8.shape), rng.uniform(0.0, 0.4999, u8.shape)).astype(np.float32)
    f[u8 == 255] = 0.5
    return f


def _check_col_profile(arr, dev, what):
    from acai_omr_amd import ops
    want_ink, want_run = (torch.from_numpy(v) for v in P.profile(np.asarray(arr).T))
    H, W = arr.shape
    t = torch.from_numpy(arr)
    wide = torch.full((H, W + 5), 0, dtype=t.dtype)              # ink in the padding: it must not be read
    wide[:, 3:W + 3] = t
    for name, page in (("contiguous", t.to(dev)), ("slice", wide.to(dev)[:, 3:W + 3])):
        ink, run = ops.page_col_profile(page)
        assert ink.dtype == run.dtype == torch.int32 and ink.shape == run.shape == (W,)
        assert torch.equal(ink.cpu(), want_ink) and torch.equal(run.cpu(), want_run), (what, name)


def test_col_profile_matches_reference(dev):
    from acai_omr_amd import _lib
    rng = np.random.RandomState(9)
    page = G.clef_page(0)[0]
    assert _lib.col_chunks(page.shape[0])[1] == 4
    for arr in (page, G.orient(page, 8), _as_f32(page, rng)):
        _check_col_profile(arr, dev, "synthetic")
    for H, W in ((1, 1), (1, 70), (70, 1), (257, 65), (513, 130)):          # 257 rows are 5 chunks, 513 rows 9
        for density in (0.5, 0.95):
            u8 = np.where(rng.rand(H, W) < density, rng.randint(0, 91, (H, W)), rng.randint(200, 256, (H, W))).astype(np.uint8)
            _check_col_profile(u8, dev, (H, W, density, "u8"))
            _check_col_profile(_as_f32(u8, rng), dev, (H, W, density, "f32"))
    for value in (0, 255):                                                   # all ink: one run through every chunk; no ink
        u8 = np.full((200, 67), value, dtype=np.uint8)
        _check_col_profile(u8, dev, ("flat", value))
        _check_col_profile(u8.astype(np.float32) / np.float32(255.0), dev, ("flat f32", value))
    runs = np.full((300, 9), 255, dtype=np.uint8)                            # runs that begin, end and meet at the chunk boundaries 64, 128, 192, 256
    runs[0:64, 0] = 0
    runs[64:128, 1] = 0
    runs[63:65, 2] = 0
    runs[10:291, 3] = 0
    runs[0:300, 4] = 0
    runs[128:192, 5] = 0
    runs[200:256, 5] = 0
    runs[64:300, 6] = 0
    runs[299, 7] = 0
    _check_col_profile(runs, dev, "boundaries")


def test_col_profile_at_the_tallest_page(dev):
    """H = 65535, one column wide: 64 chunks of 1024 rows, the most and the longest the kernel makes."""
    from acai_omr_amd import _lib, ops
    H = _lib.PAGE_MAX_H
    assert _lib.col_chunks(H) == (1024, 64)
    rng = np.random.RandomState(13)
    col = np.where(rng.rand(H, 1) < 0.95, 20, 240).astype(np.uint8)
    col[3000:9000] = 10                                                      # a run over five chunk boundaries
    want_ink, want_run = P.profile(col.T)
    assert want_run[0] >= 6000
    ink, run = ops.page_col_profile(torch.from_numpy(col).to(dev))
    assert ink.cpu().tolist() == want_ink.tolist() and run.cpu().tolist() == want_run.tolist()
    with pytest.raises(RuntimeError, match="acai_page_col_profile"):
        L = _lib.lib()
        t, o = torch.zeros(70, 100, dtype=torch.uint8, device=dev), torch.zeros(2, 100, dtype=torch.int32, device=dev)
        work = torch.zeros(4 * 2 * 100 - 1, dtype=torch.int32, device=dev)
        _lib.check(L.acai_page_col_profile(t.data_ptr(), 1, 70, 100, 100, 0.5, o[0].data_ptr(), o[1].data_ptr(), work.data_ptr(), work.numel(), None),
                   "acai_page_col_profile")                                  # work one element short of 4 * 2 chunks * 100


# ---- 3. box ink ---------------------------------------------------------------------------------------------------------------------------
def test_box_ink_matches_reference(dev):
    from acai_omr_amd import ops
    rng = np.random.RandomState(17)
    page = G.clef_page(0)[0]
    H, W = page.shape
    noise = np.where(rng.rand(H, W) < 0.4, rng.randint(0, 91, (H, W)), rng.randint(200, 256, (H, W))).astype(np.uint8)
    fixed = [(0, 0, W, H), (0, 0, 1, 1), (W - 1, H - 1, W, H), (0, 0, W, 1), (0, H - 1, W, H), (0, 0, 1, H), (W - 1, 0, W, H), (18, 40, 24, 53),
             (-5, -5, 3, 3), (W - 3, H - 3, W + 9, H + 9), (10, 10, 10, 50), (50, 30, 40, 60), (-10, 5, -2, 9)]       # the last four: clipped, empty, empty, outside
    for arr in (page, noise, _as_f32(noise, rng)):
        t = torch.from_numpy(arr).to(dev)
        for n in (0, 1, 65):
            rects = fixed[:n] if n <= len(fixed) else fixed + [tuple(int(v) for v in (x, y, x + w, y + h)) for x, y, w, h in
                                                               zip(rng.randint(0, W, n), rng.randint(0, H, n), rng.randint(1, W, n), rng.randint(1, H, n))][:n - len(fixed)]
            assert len(rects) == n
            table = torch.tensor(rects, dtype=torch.int32).reshape(n, 4).to(dev)
            got = ops.page_box_ink(t, table)
            assert got.dtype == torch.int32 and got.shape == (n,) and got.cpu().tolist() == G.box_ink(arr, rects).tolist(), (str(arr.dtype), n)
    with pytest.raises(ValueError):
        ops.page_box_ink(torch.from_numpy(page).to(dev), torch.zeros(3, 3, dtype=torch.int32, device=dev))
    with pytest.raises(TypeError):
        ops.page_box_ink(torch.from_numpy(page).to(dev), torch.zeros(3, 4, dtype=torch.int64, device=dev))


# ---- 4. the estimate ----------------------------------------------------------------------------------------------------------------------
def test_estimate_orientation(dev):
    from acai_omr_amd.page import estimate_orientation
    upright = G.clef_page(0)[0]
    colour = G.colour_page(upright)
    for code in (1, 3, 6, 8):
        photo = G.orient(upright, G.INVERSE[code])
        want = G.estimate(photo)
        assert want[0] == code and want[1] > 0
        assert estimate_orientation(torch.from_numpy(photo).to(dev)) == want
        cphoto = G.orient(colour, G.INVERSE[code])
        cwant = G.estimate(G.grey(cphoto))
        assert cwant[0] == code
        assert estimate_orientation(torch.from_numpy(cphoto).to(dev)) == cwant
        assert estimate_orientation(torch.from_numpy(cphoto).permute(2, 0, 1).contiguous()) == cwant          # planar, from the host
    sym = P.synthetic_page(0)[0]
    assert estimate_orientation(torch.from_numpy(sym).to(dev)) == (1, 0.0)
    assert estimate_orientation(torch.full((120, 90), 230, dtype=torch.uint8, device=dev)) == (1, 0.0)


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e(dev):
    from conftest import load_golden
    from decode_support import build_vitomr
    from acai_omr_amd.inference.vitomr_inference import page_inference
    from acai_omr_amd.utils import DynamicResize
    fx = load_golden("vitomr_dh64b")
    m = build_vitomr(fx["cfg"], fx["state_dict"], dev, torch.bfloat16, max_batch=2)
    tr = DynamicResize(16, 32, 4, 8, True)
    colour = G.colour_page(G.clef_page(0)[0])
    grey = torch.from_numpy(G.grey(colour)).to(dev)
    base = page_inference(m, grey, "cuda", tr, max_inference_len=12)          # the grey upright page on the path as it was: computed once
    assert len(base) == 3
    return m, tr, colour, grey, base


def _same(a, b):
    return torch.equal(a.seqs, b.seqs) and torch.equal(a.log_probs, b.log_probs) and torch.equal(a.seq_mask, b.seq_mask) and a.boxes == b.boxes


def test_page_inference_orient_off_is_the_present_path(dev, e2e, monkeypatch):
    from acai_omr_amd import ops
    from acai_omr_amd.inference.vitomr_inference import page_inference
    m, tr, colour, grey, base = e2e
    assert base.orientations == [1] and base.source_sizes == [(240, 200)] and base.page_sizes == [(240, 200)]
    def no_launch(*a, **k):
        raise AssertionError("ops.page_ingest was launched for a single-channel page that needs no turn")
    monkeypatch.setattr(ops, "page_ingest", no_launch)
    for orient in (None, False, 1, [1]):
        res = page_inference(m, grey, "cuda", tr, max_inference_len=12, orient=orient)
        assert _same(res, base) and res.orientations == [1] and res.source_sizes == base.source_sizes and res.page_sizes == base.page_sizes
        assert (res.angles, res.flattened, res.quads, res.system_page, res.sizes, res.windows, res.specials) == (
            base.angles, base.flattened, base.quads, base.system_page, base.sizes, base.windows, base.specials)
        assert res.box_corners(0) == base.box_corners(0) and res.to_page_xy(1, 3.0, 2.0) == base.to_page_xy(1, 3.0, 2.0)
    monkeypatch.undo()
    res = page_inference(m, torch.from_numpy(colour), "cuda", tr, max_inference_len=12)                  # a colour page with orient=None: made grey
    assert _same(res, base) and res.orientations == [1] and res.source_sizes == [(240, 200)]
    for bad in ("upright", 1.5, [1.5]):
        with pytest.raises(TypeError):
            page_inference(m, grey, "cuda", tr, max_inference_len=12, orient=bad)
    with pytest.raises(ValueError):
        page_inference(m, grey, "cuda", tr, max_inference_len=12, orient=0)


@pytest.mark.parametrize("code", [3, 6, 8])
def test_page_inference_orient(dev, e2e, code):
    from acai_omr_amd.inference.vitomr_inference import page_inference
    m, tr, colour, grey, base = e2e
    photo_np = G.orient(colour, G.INVERSE[code])                              # the photo that `code` turns upright
    Hs, Ws = photo_np.shape[:2]
    photo = torch.from_numpy(photo_np)
    res = page_inference(m, photo, "cuda", tr, max_inference_len=12, orient=code)
    assert _same(res, base)                                                   # boxes, rows, log-probs and mask of the grey upright page
    assert res.orientations == [code] and res.source_sizes == [(Hs, Ws)] and res.page_sizes == [(240, 200)] and res.quads == [None] and res.angles == [0.0]
    # the corners of the first system lead to its pixels in the photo as it lay
    x0, y0, x1, y1 = res.boxes[0][0]
    assert res.box_corners(0) == [G.to_photo_xy(code, Hs, Ws, float(x), float(y)) for x, y in ((x0, y0), (x1, y0), (x1, y1), (x0, y1))]
    lum = G.grey(photo_np)
    upright = G.grey(colour)
    for x, y in ((x0, y0), (x1 - 1, y0), (x1 - 1, y1 - 1), (x0, y1 - 1), (14 + G.CLEF_X, 40), (14 + G.CLEF_X + 2, 44)):      # the last two: in the first clef
        px, py = res.to_source_xy(0, x, y)
        assert lum[py, px] == upright[y, x]
    cx, cy = res.to_source_xy(0, 14 + G.CLEF_X, 40)
    assert lum[cy, cx] < 100 and res.from_page_xy(0, *res.to_page_xy(0, 5.0, 3.0)) == pytest.approx((5.0, 3.0), abs=1e-9)
    # the estimate: a pure function photo -> code, so orient=True is orient=<the estimated codes>, bit for bit
    est = page_inference(m, [photo, torch.from_numpy(colour)], "cuda", tr, max_inference_len=12, orient=True)
    assert est.orientations == [code, 1] and est.source_sizes == [(Hs, Ws), (240, 200)]
    given = page_inference(m, [photo, torch.from_numpy(colour)], "cuda", tr, max_inference_len=12, orient=[code, 1])
    assert _same(est, given) and est.boxes == [base.boxes[0]] * 2 and est.system_page == given.system_page
    flat = page_inference(m, photo, "cuda", tr, max_inference_len=12, orient=True, flatten=True)
    assert flat.orientations == [code] and flat.flattened == [True]
    assert _same(flat, page_inference(m, photo, "cuda", tr, max_inference_len=12, orient=flat.orientations, flatten=True))


def _framed_clef_frame():
    """`deskew_reference.synthetic_page` - strokes two pixels thick, which a bilinear resampling cannot take above the ink threshold (the
    one-pixel lines of the clef page do not survive being photographed) - with a clef stamped on every staff, photographed on the table of
    the rectification tests."""
    page = D.synthetic_page(0)[0].copy()
    rng = np.random.RandomState(7)
    for y, staves in ((60, 2), (170, 1), (250, 2)):
        for s in range(staves):
            r = y + s * D.STAFF_GAP
            page[r:r + 4 * D.LINE_GAP + D.THICK, 36:46] = rng.randint(0, 91, size=(4 * D.LINE_GAP + D.THICK, 10))
    return Q.embed(page, Q.QUADS[0], *Q.FRAME, seed=0)


@pytest.mark.parametrize("code", [6, 3])
def test_page_inference_orient_with_rectify(dev, e2e, code):
    """A photo of the sheet on a table, lying on its side or on its head: the estimate is made on a rectified temporary, then the call is
    orient=<that code> with rectify."""
    from acai_omr_amd.inference.vitomr_inference import page_inference
    from acai_omr_amd.page import OrientConfig
    m, tr = e2e[:2]
    frame = _framed_clef_frame()
    photo = torch.from_numpy(G.orient(frame, G.INVERSE[code]))
    upright = page_inference(m, torch.from_numpy(frame), "cuda", tr, max_inference_len=12, rectify=True)          # the present path on the frame as it stands
    assert len(upright) == 3
    for orient in (True, OrientConfig(end_frac=0.1)):
        est = page_inference(m, photo, "cuda", tr, max_inference_len=12, orient=orient, rectify=True)
        assert est.orientations == [code] and est.source_sizes == [tuple(photo.shape)] and est.quads[0] is not None
        given = page_inference(m, photo, "cuda", tr, max_inference_len=12, orient=code, rectify=True)
        assert _same(est, given) and est.quads == given.quads and est.page_sizes == given.page_sizes
        assert _same(est, upright) and est.quads == upright.quads                                                 # the turn is exact: the same page is rectified
