"""Page assessment on the GPU (csrc/assess.hip through ops.page_runs / page_sharpness, page.estimate_staff_scale / assess_pages and
page_inference(assess=)).

Bars: every device result is integers, so torch.equal to the numpy restatement (tests/assess_reference.py); the floats of `PageQuality`
are formed on the host from those integers by the same exact rational, so they are equal too; page_inference's rows are torch.equal
where the boxes are.  Shapes: the kernels walk chunks of C = _lib.RUNS_CHUNK_ROWS rows and 256 columns (64 lanes x 4), so heights around C
and 2 C and widths around 64 lanes and one wave's 256 columns, and a page of 12 C + 1 rows whose columns hold every way a run can meet a
chunk's edge, are where they can go wrong."""
import numpy as np
import pytest
import torch

import assess_reference as A
import page_reference as R

pytestmark = pytest.mark.gpu

DENSE = dict(seed=1, H=1600, W=200, systems_at=tuple((60 + 60 * i, 1) for i in range(24)))
WIDTHS = (1, 3, 63, 64, 65, 200, 257)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from acai_omr_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _heights():
    from acai_omr_amd import _lib
    C = _lib.RUNS_CHUNK_ROWS
    assert C == _lib.SHARP_CHUNK_ROWS
    return C, (1, 2, 3, C - 1, C, C + 1, 2 * C + 1)


def _as(page_u8, dtype):
    """A uint8 page in the dtype under test: fp32 pages hold p / 255 formed in float32, which is what the kernels make of a uint8 pixel."""
    return page_u8 if dtype == "uint8" else R.as_float(page_u8)


def _check(dev, page_np, thr=0.5, view=None):
    """Both kernels on `page_np` (or on the device view of it that is given) against the restatement."""
    from acai_omr_amd import ops
    t = torch.from_numpy(np.ascontiguousarray(page_np)).to(dev) if view is None else view
    hist = ops.page_runs(t, thr)
    stats, levels = ops.page_sharpness(t)
    assert hist.dtype == torch.int64 and tuple(hist.shape) == (3, 256) and stats.dtype == torch.int64 and tuple(stats.shape) == (3,)
    assert levels.dtype == torch.int64 and tuple(levels.shape) == (256,)
    want_stats, want_levels = A.sharpness(page_np)
    where = (page_np.shape, str(page_np.dtype))
    assert torch.equal(hist.cpu(), torch.from_numpy(A.runs(page_np, thr))), where
    assert torch.equal(stats.cpu(), torch.from_numpy(want_stats)), where
    assert torch.equal(levels.cpu(), torch.from_numpy(want_levels)), where
    return hist


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_every_height_and_width_around_the_chunk_and_the_wave(dev, dtype):
    C, heights = _heights()
    for H in heights:
        for W in WIDTHS:
            rng = np.random.RandomState(1000 * H + W)
            noise = np.where(rng.rand(H, W) < 0.35, rng.randint(0, 91, size=(H, W)), rng.randint(200, 256, size=(H, W))).astype(np.uint8)
            _check(dev, _as(noise, dtype))
            _check(dev, _as(A.boundary_page(H, W, C, seed=H + W)[0], dtype))


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_runs_that_meet_a_chunk_edge_every_way(dev, dtype):
    C, _ = _heights()
    H, W = 12 * C + 1, 200
    page, n_cols = A.boundary_page(H, W, C)
    assert n_cols <= W                                   # every column kind is on the page
    want = A.runs(page)
    assert want[0, 254] and want[0, 255] >= 3 and want[1, 254] and want[1, 255] and want[2, 255]   # 254, and 255 / 256 / 300 in the clamp bin
    assert not page[:, 0].min() < 128 and not page[:, 1].max() >= 128                              # an all-paper and an all-ink column
    hist = _check(dev, _as(page, dtype))
    assert hist[:, 0].tolist() == [0, 0, 0]
    # grey levels on the same ink: the Laplacian and the level histogram on something that is not two-valued
    rng = np.random.RandomState(5)
    grey = np.where(page < 128, rng.randint(0, 91, size=page.shape), rng.randint(200, 256, size=page.shape)).astype(np.uint8)
    _check(dev, _as(grey, dtype))


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_a_strided_slice_of_a_larger_tensor(dev, dtype):
    C, _ = _heights()
    H, W = 2 * C + 3, 203
    rng = np.random.RandomState(11)
    big = np.where(rng.rand(2 * H, W + 13) < 0.4, rng.randint(0, 91, size=(2 * H, W + 13)), rng.randint(200, 256, size=(2 * H, W + 13))).astype(np.uint8)
    big = _as(big, dtype)
    t = torch.from_numpy(big).to(dev)
    for rows, x0 in ((slice(0, H), 5), (slice(1, 2 * H, 2), 3), (slice(H - 1, 2 * H - 1), 0)):
        view = t[rows, x0:x0 + W]
        assert not view.is_contiguous() and view.stride(1) == 1
        _check(dev, np.ascontiguousarray(big[rows, x0:x0 + W]), view=view)


def test_float_values_at_the_threshold_and_at_level_boundaries(dev):
    C, _ = _heights()
    f32 = np.float32
    edges = []
    for k in list(range(0, 255, 7)) + [126, 127, 128, 253, 254]:
        v = f32(f32(k + 0.5) / f32(255.0))
        edges += [v, np.nextafter(v, f32(0)), np.nextafter(v, f32(1))]
    for thr in (0.5, 0.25, 1.0 / 3.0):
        edges += [f32(thr), np.nextafter(f32(thr), f32(0)), np.nextafter(f32(thr), f32(1))]
    edges += [f32(0), f32(1), f32(-0.25), f32(1.5), f32(0.5 / 255), f32(254.5 / 255)]
    edges = np.array(edges, dtype=f32)
    rng = np.random.RandomState(3)
    page = edges[rng.randint(0, len(edges), size=(2 * C + 1, 130))]
    lv = A.levels_of(page)
    assert lv.min() == 0 and lv.max() == 255
    for thr in (0.5, 0.25, 1.0 / 3.0):
        _check(dev, page, thr)
    half = np.full((C + 2, 70), f32(0.5))                 # exactly the threshold: paper, everywhere
    assert _check(dev, half).sum() == 0
    half[3:9] = np.nextafter(f32(0.5), f32(0))            # just below: ink
    assert int(_check(dev, half)[0, 6]) == 70


def test_two_calls_give_the_same_bits_and_out_is_added_to(dev):
    from acai_omr_amd import _lib, ops
    page = torch.from_numpy(R.synthetic_page(**DENSE)[0]).to(dev)
    a, b = ops.page_runs(page), ops.page_runs(page)
    assert torch.equal(a, b) and int(a.sum()) > 0
    (s1, l1), (s2, l2) = ops.page_sharpness(page), ops.page_sharpness(page)
    assert torch.equal(s1, s2) and torch.equal(l1, l2) and int(l1.sum()) == page.numel()
    acc = torch.zeros(_lib.RUNS_WORDS, dtype=torch.int64, device=dev)
    ops.page_runs(page, out=acc)
    assert torch.equal(ops.page_runs(page, out=acc), 2 * a) and acc.data_ptr() == ops.page_runs(page, out=acc).data_ptr()
    sh = torch.zeros(_lib.SHARP_WORDS, dtype=torch.int64, device=dev)
    ops.page_sharpness(page, out=sh)
    st, lv = ops.page_sharpness(page, out=sh)
    assert torch.equal(st, 2 * s1) and torch.equal(lv, 2 * l1)


def test_bad_pages_and_outputs_are_refused_before_any_launch(dev):
    from acai_omr_amd import _lib, ops
    good = torch.zeros(8, 8, dtype=torch.uint8, device=dev)
    for fn in (ops.page_runs, ops.page_sharpness):
        for bad in (torch.zeros(8, 8, dtype=torch.int32, device=dev), torch.zeros(8, 8, dtype=torch.float16, device=dev), "page"):
            with pytest.raises(TypeError):
                fn(bad)
        for bad in (torch.zeros(2, 8, 8, dtype=torch.uint8, device=dev), torch.zeros(8, dtype=torch.uint8, device=dev),
                    torch.zeros(0, 8, dtype=torch.uint8, device=dev), torch.zeros(8, 16, dtype=torch.uint8, device=dev)[:, ::2],
                    torch.zeros(1, 8, dtype=torch.uint8, device=dev).expand(4, 8)):
            with pytest.raises(ValueError):
                fn(bad)
        words = _lib.RUNS_WORDS if fn is ops.page_runs else _lib.SHARP_WORDS
        with pytest.raises(TypeError):
            fn(good, out=torch.zeros(words, dtype=torch.int32, device=dev))
        with pytest.raises(TypeError):
            fn(good, out=[0] * words)
        for bad in (torch.zeros(words - 1, dtype=torch.int64, device=dev), torch.zeros(2 * words, dtype=torch.int64, device=dev)[::2]):
            with pytest.raises(ValueError):
                fn(good, out=bad)
        with pytest.raises(RuntimeError):
            fn(good, out=torch.zeros(words, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="acai_page_runs"):                 # the C entry's own check, also before any launch
        ops.page_runs(torch.zeros(1, _lib.PAGE_MAX_W + 1, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match="acai_page_sharpness"):
        ops.page_sharpness(torch.zeros(1, _lib.PAGE_MAX_W + 1, dtype=torch.uint8, device=dev))


def _fields(q):
    s = q.scale
    scale = None if s is None else dict(line=s.line, space=s.space, pitch_bin=s.pitch_bin, pitch=s.pitch, confidence=s.confidence)
    return dict(scale=scale, sharpness=q.sharpness, paper_level=q.paper_level, ink_level=q.ink_level, contrast=q.contrast, ink_share=q.ink_share, focus=q.focus)


def test_assess_pages_equals_the_restatement(dev):
    from acai_omr_amd.page import AssessConfig, assess_pages, estimate_staff_scale
    syn = R.synthetic_page()[0]
    dense = R.synthetic_page(**DENSE)[0][:400]
    rng = np.random.RandomState(9)
    soft = rng.rand(70, 90).astype(np.float32)
    blank = np.full((40, 50), 255, dtype=np.uint8)
    pages = [syn, R.as_float(dense), soft, blank]
    got = assess_pages([torch.from_numpy(p) for p in pages])
    assert [_fields(q) for q in got] == [A.quality(p) for p in pages]
    assert all(q.ok and q.reasons == () for q in got) and got[3].scale is None and got[0].scale.staff_space == 2
    assert [None if s is None else s.pitch_bin for s in estimate_staff_scale([torch.from_numpy(p).to(dev) for p in pages])] == [3, 3, got[2].scale.pitch_bin, None]
    one = assess_pages(torch.from_numpy(syn).to(dev), AssessConfig(ink_threshold=0.3, paper_percent=90, ink_percent=10, min_contrast=250))
    assert len(one) == 1 and _fields(one[0]) == A.quality(syn, 0.3, 90, 10)
    assert not one[0].ok and len(one[0].reasons) == 1 and "min_contrast" in one[0].reasons[0]


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e(dev):
    from conftest import load_golden
    from decode_support import build_vitomr
    from acai_omr_amd.utils import DynamicResize
    fx = load_golden("vitomr_dh64b")
    m = build_vitomr(fx["cfg"], fx["state_dict"], dev, torch.bfloat16, max_batch=8)
    return m, DynamicResize(16, 32, 4, 8, True)


def _same(a, b):
    return torch.equal(a.seqs, b.seqs) and torch.equal(a.log_probs, b.log_probs) and torch.equal(a.seq_mask, b.seq_mask)


def test_page_inference_finds_the_dense_page_only_when_it_assesses(dev, e2e):
    from acai_omr_amd.inference.vitomr_inference import page_inference
    from acai_omr_amd.page import AssessConfig, plan_systems
    m, tr = e2e
    page_np, truth = R.synthetic_page(**DENSE)
    H, W = page_np.shape
    page = torch.from_numpy(page_np)
    res = page_inference(m, page, "cuda", tr, max_inference_len=4, assess=True)
    want = R.truth_boxes_with_margin(truth, 5, H, W)
    assert len(res) == 24 and res.boxes == [want]
    q = res.quality[0]
    assert q.scale.staff_space == 2 and (q.scale.line, q.scale.pitch_bin) == (1, 3) and q.ok and q.reasons == ()
    assert _fields(q) == A.quality(page_np)
    plans = plan_systems([(H, W)], [want], tr)
    assert res.system_staff_space == [q.scale.pitch * size[0] / (y1 - y0) for _, (_, y0, _, y1), size, _ in plans]
    assert all(v > 0 for v in res.system_staff_space)
    # the parent's behaviour: sized from the canvas, every band is under min_height
    none = page_inference(m, page, "cuda", tr, max_inference_len=4, assess=None)
    assert len(none) == 0 and none.boxes == [[]] and none.quality == [None] and none.system_staff_space == []
    assert len(page_inference(m, page, "cuda", tr, max_inference_len=4, assess=False)) == 0
    # a gate the page fails is reported, and the page is decoded all the same
    smallest = min(res.system_staff_space)
    gated = page_inference(m, page, "cuda", tr, max_inference_len=4, assess=AssessConfig(min_model_staff_space=smallest + 1.0, min_staff_space=3))
    assert _same(gated, res) and gated.boxes == res.boxes
    assert not gated.quality[0].ok and len(gated.quality[0].reasons) == 1 and "min_model_staff_space" in gated.quality[0].reasons[0]
    with pytest.raises(TypeError):
        page_inference(m, page, "cuda", tr, max_inference_len=4, assess="yes")


def test_page_inference_without_assess_issues_none_of_the_new_launches(dev, e2e, monkeypatch):
    from acai_omr_amd import ops
    from acai_omr_amd.inference.vitomr_inference import page_inference
    from acai_omr_amd.page import DetectConfig
    m, tr = e2e
    page = torch.from_numpy(R.synthetic_page()[0])
    cfg = DetectConfig(0.5, 1, 4, 8, 0.5, 5, 0, 64)
    want = page_inference(m, page, "cuda", tr, max_inference_len=12, detect=cfg)

    def refuse(*a, **k):
        raise AssertionError("an assessment launch on a path that did not ask for one")

    monkeypatch.setattr(ops, "page_runs", refuse)
    monkeypatch.setattr(ops, "page_sharpness", refuse)
    for off in (None, False):
        assert _same(page_inference(m, page, "cuda", tr, max_inference_len=12, detect=cfg, assess=off), want)
    assert _same(page_inference(m, page, "cuda", tr, max_inference_len=12, detect=cfg), want)
    with pytest.raises(AssertionError):
        page_inference(m, page, "cuda", tr, max_inference_len=12, detect=cfg, assess=True)


def test_page_inference_leaves_a_page_in_a4_proportion_as_it_was(dev, e2e):
    """`synthetic_page()` itself (240 rows, 3 rows from line to line) is NOT in A4 proportion - 180 staff spaces are 540 rows - and the
    default `DetectConfig` finds none of its systems, which is why every test on it sets the detector's fields.  Two cases then: that page
    with the fields its other tests set (fields the caller set win, so assessing changes nothing), and the same music on a canvas of 560
    rows, which is in proportion, with the default config (the sizes from the canvas and from the music are the same numbers)."""
    from acai_omr_amd.inference.vitomr_inference import page_inference
    from acai_omr_amd.page import DetectConfig
    m, tr = e2e
    cfg = DetectConfig(0.5, 1, 4, 8, 0.5, 5, 0, 64)
    page = torch.from_numpy(R.synthetic_page()[0])
    off, on = (page_inference(m, page, "cuda", tr, max_inference_len=12, detect=cfg, assess=a) for a in (None, True))
    assert len(off) == 3 and on.boxes == off.boxes == [[(14, 37, 191, 74), (14, 107, 191, 123), (14, 167, 191, 204)]] and _same(on, off)
    assert off.quality == [None] and on.quality[0].scale.staff_space == 2 and len(on.system_staff_space) == 3
    a4_np, truth = R.synthetic_page(H=560)
    assert DetectConfig().resolved(560, 200) == DetectConfig().resolved(560, 200, staff_space=3)
    a4 = torch.from_numpy(a4_np).float() / 255.0
    off, on = (page_inference(m, a4, "cuda", tr, max_inference_len=12, assess=a) for a in (None, True))
    assert on.boxes == off.boxes == [R.truth_boxes_with_margin(truth, 5, 560, 200)] and _same(on, off)
    assert on.quality[0].scale.pitch_bin == 3 and off.quality == [None]
    # explicit boxes: assessed and reported, the boxes are the caller's
    boxed = page_inference(m, a4, "cuda", tr, boxes=truth, max_inference_len=12, assess=True)
    assert boxed.boxes == [truth] and boxed.quality[0].scale.pitch_bin == 3 and len(boxed.system_staff_space) == 3
