"""Whole-page input on the GPU (csrc/page.hip through ops.page_profile / page_systems / crop_resize_to_patches, page.detect_systems /
split_pages and page_inference).

Bars:
  * profile and systems: integer outputs, torch.equal to the numpy restatement (tests/page_reference.py);
  * crop-resize, fp32: torch.equal to DynamicResize.to_patches of the contiguous crops (the same arithmetic) and within 2e-6 of aten's
    antialiased bicubic on the crop (the bar tests/test_resize.py holds the resize to); bf16: torch.equal to the fp32 rows cast to bf16;
    rows of the patch tensor that belong to no entry keep their sentinel;
  * page_inference: seqs, seq_mask and log_probs torch.equal to continuous_inference over the resized crops."""
import numpy as np
import pytest
import torch

import page_reference as R

pytestmark = pytest.mark.gpu

DETECT = dict(min_ink=1, merge_gap=4, min_height=8, line_len=100, min_line_rows=5, margin=0)
TRUTH = [(14, 37, 191, 74), (14, 107, 191, 123), (14, 167, 191, 204)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from acai_omr_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ---- 1. profile --------------------------------------------------------------------------------------------------------------------------
def _profile_rows(W):
    """Ink masks [rows, W] built around the kernel's own layout: a lane holds PAGE_LANE_PIXELS pixels, a wave step 64 lanes, and each of a
    row's PAGE_WAVES waves one span."""
    from acai_omr_amd import _lib
    lane, step = _lib.PAGE_LANE_PIXELS, 64 * _lib.PAGE_LANE_PIXELS
    span = -(-(-(-W // _lib.PAGE_WAVES)) // step) * step
    rows = []

    def row(*runs):
        m = np.zeros(W, dtype=bool)
        for a, b in runs:
            m[max(a, 0):max(min(b, W), 0)] = True
        rows.append(m)

    row()                                        # empty
    row((0, W))                                  # full width
    row((W - 3, W))                              # ends at the last pixel
    row((0, 1))
    row((1, W - 1))                              # one run across every boundary there is
    row((0, W // 3), (W // 3 + 1, 2 * (W // 3) + 1))          # two equal runs
    row((2, 7), (W - 7, W - 2))                               # two equal runs far apart
    edges = {lane, 2 * lane, step - lane, step, step + lane, 2 * step, span - step, span, span + step, 2 * span, 3 * span, W - 1}
    for b in sorted(e for e in edges if 0 < e < W):
        row((b - 2, b + 3))                      # a short run across the boundary
        row((b - 5, b), (b + 1, b + 7))          # the longer run starts right behind it
        row((0, b))                              # ends at the boundary
        row((b, W))                              # starts at it
    rng = np.random.RandomState(W)
    for p in (0.5, 0.9, 0.99):
        rows.append(rng.rand(W) < p)
    return np.stack(rows)


@pytest.mark.parametrize("W", [1, 63, 64, 65, 255, 257, 1000, 4099])
def test_profile_matches_reference(dev, W):
    from acai_omr_amd import ops
    mask = _profile_rows(W)
    rng = np.random.RandomState(7 + W)
    u8 = np.where(mask, rng.randint(0, 91, mask.shape), rng.randint(200, 256, mask.shape)).astype(np.uint8)
    ink, run = R.profile(u8)
    assert ink.tolist() == mask.sum(1).tolist() and run[1] == W and run[0] == 0
    want_ink, want_run = torch.from_numpy(ink), torch.from_numpy(run)
    f32 = torch.from_numpy(u8).float() / 255.0
    wide = torch.zeros(mask.shape[0], W + 5, dtype=torch.uint8)       # pitch > W: the columns behind the page are all ink
    wide[:, :W] = torch.from_numpy(u8)
    for page in (torch.from_numpy(u8).to(dev), f32.to(dev), wide.to(dev)[:, :W], f32.to(dev)[None]):
        got_ink, got_run = ops.page_profile(page, 0.5)
        assert got_ink.dtype == torch.int32 and torch.equal(got_ink.cpu(), want_ink), W
        assert torch.equal(got_run.cpu(), want_run), (W, (got_run.cpu() != want_run).nonzero().flatten().tolist())
    # the threshold is the kernel's comparison: value < threshold
    got_ink, _ = ops.page_profile(torch.from_numpy(u8).to(dev), 0.25)
    assert torch.equal(got_ink.cpu(), torch.from_numpy(R.profile(u8, 0.25)[0]))


# ---- 2. systems --------------------------------------------------------------------------------------------------------------------------
def _page(H, W, rows):
    """A white uint8 page with ink in rows: {y: (x_start, x_end)} or {y: [(x_start, x_end), ...]}."""
    page = np.full((H, W), 255, dtype=np.uint8)
    for y, spans in rows.items():
        for a, b in ([spans] if isinstance(spans[0], int) else spans):
            page[y, a:b] = 0
    return page


def _block(y0, y1, a, b):
    return {y: (a, b) for y in range(y0, y1)}


def _systems_cases():
    W = 40
    P = dict(min_ink=1, merge_gap=2, min_height=4, line_len=20, min_line_rows=2, margin=0)
    cases = {}
    syn = R.synthetic_page()[0]
    cases["synthetic"] = (syn, DETECT, 64, 3)
    cases["synthetic_margin"] = (syn, dict(DETECT, margin=20), 64, 3)
    cases["touch_first_and_last_row"] = (_page(30, W, {**_block(0, 5, 3, 30), **_block(25, 30, 5, 38)}), P, 8, 2)
    gap = {**_block(2, 6, 3, 30), **_block(6 + 2, 12, 3, 30), **_block(20, 24, 3, 30), **_block(24 + 3, 31, 3, 30)}
    cases["gap_merge_gap_and_one_more"] = (_page(40, W, gap), P, 8, 3)           # rows 2..11 merge; 20..23 and 27..30 do not
    cases["one_row_short"] = (_page(30, W, {**_block(2, 5, 3, 30), **_block(10, 14, 3, 30)}), P, 8, 1)
    lines = {2: (3, 30), 3: (3, 10), 4: (3, 10), 5: (3, 10), 10: (3, 30), 11: (3, 10), 12: (3, 30), 13: (3, 10)}
    cases["one_line_row_short"] = (_page(30, W, lines), P, 8, 1)
    cases["split_run_is_no_line"] = (_page(30, W, {y: [(0, 19), (20, 39)] for y in range(4, 10)}), P, 8, 0)
    cases["column_0_only"] = (_page(30, W, _block(5, 12, 0, 1)), dict(P, line_len=1), 8, 1)
    cases["column_last_only"] = (_page(30, W, _block(5, 12, W - 1, W)), dict(P, line_len=1, margin=1), 8, 1)
    cases["margin_clamps_everywhere"] = (_page(12, W, _block(2, 10, 3, 37)), dict(P, margin=5), 8, 1)
    cases["min_ink_3"] = (_page(30, W, {**_block(2, 8, 3, 30), 9: (3, 5), 10: (3, 5), **_block(11, 17, 3, 30)}), dict(P, min_ink=3, merge_gap=1), 8, 2)
    cases["H_1"] = (_page(1, W, {0: (2, 30)}), dict(P, min_height=1, min_line_rows=1), 8, 1)
    cases["H_1_blank"] = (_page(1, W, {}), dict(P, min_height=1, min_line_rows=1), 8, 0)
    cases["zero_bands"] = (_page(30, W, {}), P, 8, 0)
    # widths of whole 16-byte rows (uint8: 48, 80; fp32: every width above that is a multiple of 4): the extent's wide loads
    cases["rows_16B_column_0_only"] = (_page(30, 48, _block(5, 12, 0, 1)), dict(P, line_len=1), 8, 1)
    cases["rows_16B_column_last_only"] = (_page(30, 48, _block(5, 12, 47, 48)), dict(P, line_len=1), 8, 1)
    cases["rows_16B_inside_and_tail"] = (_page(30, 80, {**_block(3, 9, 17, 46), **_block(15, 21, 31, 33), 16: (5, 79), 17: (20, 60)}), P, 8, 2)
    cases["rows_16B_plus_tail_columns"] = (_page(30, 83, {**_block(3, 9, 17, 46), 5: (15, 82), **_block(15, 21, 33, 82), 16: (40, 83)}), P, 8, 2)
    rng = np.random.RandomState(3)
    tall, y, n = {}, 0, 0
    while True:                                   # H = 3001: three rows per thread, bands of every height across the thread boundaries
        y += int(rng.randint(1, 9))
        h = int(rng.randint(1, 12))
        if y + h > 3001:
            break
        a = int(rng.randint(0, 10))
        for r in range(y, y + h):
            tall[r] = (a, a + (int(rng.randint(20, 30)) if rng.rand() < 0.5 else int(rng.randint(1, 19))))
        y += h
        n += 1
    tall[3000] = (0, 40)
    cases["H_3001"] = (_page(3001, W, tall), P, 512, None)
    cases["more_than_max_systems"] = (_page(3001, W, tall), P, 5, None)
    return cases


SYSTEMS = _systems_cases()


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_systems_match_reference(dev, name):
    from acai_omr_amd import ops
    page, prm, max_systems, expect = SYSTEMS[name]
    count, boxes = R.systems(page, 0.5, max_systems=max_systems, **prm)
    if expect is not None:
        assert count == expect, (name, count)      # the case is the one its name says
    else:
        assert count > 100
    H, W = page.shape
    if name == "margin_clamps_everywhere":
        assert boxes == [(0, 0, W, H)]
    GUARD = -77
    for t in (torch.from_numpy(page), torch.from_numpy(page).float() / 255.0):
        t = t.to(dev)
        ink, run = ops.page_profile(t, 0.5)
        out = torch.full((4 + 4 * max_systems + 8,), GUARD, dtype=torch.int32, device=dev)
        c, b = ops.page_systems(t, ink, run, 0.5, max_systems=max_systems, out=out, **prm)
        n = min(count, max_systems)
        assert torch.equal(c.cpu(), torch.tensor([count], dtype=torch.int32)), (name, int(c))
        assert torch.equal(b[:n].cpu(), torch.tensor(boxes, dtype=torch.int32).view(n, 4)), name
        host = out.cpu()
        assert bool((host[1:4] == GUARD).all()) and bool((host[4 + 4 * n:] == GUARD).all()), name    # nothing behind the last box is written


def test_detect_systems(dev):
    from acai_omr_amd.page import DetectConfig, detect_systems
    page = torch.from_numpy(R.synthetic_page()[0])
    cfg = DetectConfig(ink_threshold=0.5, line_frac=0.5, max_systems=64, **{k: v for k, v in DETECT.items() if k != "line_len"})
    assert cfg.resolved(240, 200)[3] == DETECT["line_len"]
    assert detect_systems(page, cfg) == TRUTH
    assert detect_systems(page[None].to(dev), cfg) == TRUTH
    assert detect_systems(torch.full((50, 60), 255, dtype=torch.uint8), cfg) == []
    many, prm, _, _ = SYSTEMS["more_than_max_systems"]
    small = DetectConfig(0.5, prm["min_ink"], prm["merge_gap"], prm["min_height"], 0.5, prm["min_line_rows"], prm["margin"], max_systems=5)
    with pytest.raises(ValueError, match="max_systems"):
        detect_systems(torch.from_numpy(many), small)
    # the defaults, sized from the page: the same page four times as large in both directions has the same systems
    big = torch.from_numpy(np.kron(R.synthetic_page()[0], np.ones((4, 4), dtype=np.uint8)))
    found = detect_systems(big)
    assert [(y0, y1) for _, y0, _, y1 in found] == [(4 * a - 9, 4 * b + 9) for _, a, _, b in TRUTH]      # margin 960 // 100 = 9


# ---- 3. crop-resize ----------------------------------------------------------------------------------------------------------------------
P = 16


def _aten_rows(crop, size, window):
    x = torch.nn.functional.interpolate(crop[None, None], size=size, mode="bicubic", align_corners=False, antialias=True)[0, 0].clamp(0.0, 1.0)
    top, left, ch, cw = window
    x = x[top:top + ch, left:left + cw]
    return x.reshape(ch // P, P, cw // P, P).permute(0, 2, 1, 3).reshape(-1, P * P)


@pytest.fixture(scope="module")
def crop_setup(dev):
    from acai_omr_amd.utils import DynamicResize
    tr32, tr8 = DynamicResize(P, 32, 4, 8, True), DynamicResize(P, 8, 4, 8, True)
    g = torch.Generator().manual_seed(11)
    HA, WA, HB, WB = 120, 400, 90, 301
    pa = torch.randint(0, 256, (HA, WA), generator=g, dtype=torch.uint8)
    pb = torch.rand(HB, WB, generator=g)
    # (page, (x0, y0, x1, y1), transform)
    items = [(0, (0, 0, 50, 20), tr32), (0, (WA - 50, 0, WA, 20), tr32), (0, (0, HA - 20, 50, HA), tr32), (0, (WA - 50, HA - 20, WA, HA), tr32),
             (1, (0, 0, 31, 17), tr8), (1, (WB - 31, HB - 17, WB, HB), tr8),
             (1, (150, 40, 151, 41), tr8),                   # 1 x 1
             (0, (100, 30, 277, 67), tr32),                  # 37 x 177 -> 32 x 128
             (1, (60, 30, 80, 39), tr8),                     # 9 x 20 -> 32 x 64
             (0, (200, 70, 328, 102), tr32),                 # 32 x 128: identity
             (1, (100, 60, 277, 76), tr32)]                  # 16 x 177 -> 16 x 176, columns 24 .. 151 kept
    for p, (x0, y0, x1, y1), _ in items:                     # 0 / 1 stripes directly outside every box
        page = pa if p == 0 else pb
        H, W = page.shape
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        frame = (yy >= y0 - 3) & (yy < y1 + 3) & (xx >= x0 - 3) & (xx < x1 + 3) & ~((yy >= y0) & (yy < y1) & (xx >= x0) & (xx < x1))
        stripes = (xx + yy) % 2
        page[frame] = (stripes[frame] * (255 if p == 0 else 1)).to(page.dtype)
    assert tr32._plan(37, 177) == ((32, 128), (0, 0, 32, 128)) and tr8._plan(9, 20) == ((32, 64), (0, 0, 32, 64))
    assert tr32._plan(32, 128)[0] == (32, 128) and tr32._plan(16, 177) == ((16, 176), (0, 24, 16, 128))
    pages = [pa.to(dev), pb.to(dev)]
    crops = [(pa if p == 0 else pb)[y0:y1, x0:x1].contiguous() for p, (x0, y0, x1, y1), _ in items]
    want = [tr.to_patches([c.to(dev)]).patches for c, (_, _, tr) in zip(crops, items)]      # the reference, computed once
    return items, pages, crops, want


def _entries(items, pages, gap):
    from acai_omr_amd import ops
    entries, spans, row0, tmp_off = [], [], gap, 0
    for p, (x0, y0, x1, y1), tr in items:
        size, window = tr._plan(y1 - y0, x1 - x0)
        entries.append(ops.crop_resize_entry(pages[p], (x0, y0, x1 - x0, y1 - y0), size, window, row0, tmp_off))
        n = (window[2] // P) * (window[3] // P)
        spans.append((row0, row0 + n))
        row0 += n + gap
        tmp_off += (y1 - y0) * size[1]
    return entries, spans, row0


def test_crop_resize_one_launch_pair(dev, crop_setup):
    from acai_omr_amd import ops
    from acai_omr_amd.page import split_pages
    items, pages, crops, want = crop_setup
    entries, spans, rows = _entries(items, pages, gap=3)
    SENT = -123.0
    out = torch.full((rows, P * P), SENT, device=dev)
    ops.crop_resize_to_patches(entries, out, P, clamp01=True)
    used = torch.zeros(rows, dtype=torch.bool)
    for (a, b), w, c, (_, box, tr) in zip(spans, want, crops, items):
        used[a:b] = True
        assert w.shape[0] == b - a
        assert torch.equal(out[a:b], w), box                                        # the same bits as resize.to_patches of the crop
        cf = c.float() / 255.0 if c.dtype == torch.uint8 else c
        size, window = tr._plan(*c.shape)
        assert float((out[a:b].cpu() - _aten_rows(cf, size, window)).abs().max()) < 2e-6, box
    assert bool((out[~used.to(dev)] == SENT).all())                                 # rows of no entry are untouched
    out16 = torch.full((rows, P * P), SENT, device=dev, dtype=torch.bfloat16)
    ops.crop_resize_to_patches(entries, out16, P, clamp01=True)
    assert torch.equal(out16[used.to(dev)], out[used.to(dev)].to(torch.bfloat16)) and bool((out16[~used.to(dev)] == SENT).all())
    # split_pages: the same rows packed back to back, the grids of the plans
    tr32 = items[0][2]
    sel = [i for p in (0, 1) for i, (q, _, tr) in enumerate(items) if q == p and tr is tr32]      # page order, then the order given
    boxes = [[items[i][1] for i in sel if items[i][0] == p] for p in (0, 1)]
    pk = split_pages(pages, boxes, tr32)
    assert torch.equal(pk.patches, torch.cat([want[i] for i in sel])) and len(pk) == len(sel)
    assert pk.dims == [(w[2] // P, w[3] // P) for w in (tr32._plan(*crops[i].shape)[1] for i in sel)]
    pk16 = split_pages(pages, boxes, tr32, dtype=torch.bfloat16)
    assert torch.equal(pk16.patches, pk.patches.to(torch.bfloat16))
    one = split_pages(pages[0], boxes[0], tr32)                               # one page, its boxes given bare
    assert torch.equal(one.patches, pk.patches[:one.patches.shape[0]])


def test_crop_resize_refusals(dev, crop_setup):
    from acai_omr_amd import ops
    items, pages, _, _ = crop_setup
    out = torch.zeros(64, P * P, device=dev)
    H, W = pages[0].shape
    bad = [ops.crop_resize_entry(pages[0], (W - 49, 0, 50, 20), (64, 128), (0, 0, 64, 128), 0, 0),      # one column outside the page
           ops.crop_resize_entry(pages[0], (0, H - 19, 50, 20), (64, 128), (0, 0, 64, 128), 0, 0),      # one row outside
           ops.crop_resize_entry(pages[0], (-1, 0, 50, 20), (64, 128), (0, 0, 64, 128), 0, 0),
           ops.crop_resize_entry(pages[0], (0, 0, 50, 20), (64, 128), (0, 0, 64, 120), 0, 0),           # window not a multiple of P
           ops.crop_resize_entry(pages[0], (0, 0, 50, 20), (64, 128), (8, 0, 64, 128), 0, 0),           # window outside the result
           ops.crop_resize_entry(pages[0], (0, 0, 50, 20), (64, 128), (0, 0, 64, 128), 40, 0)]          # rows outside the patch stream
    good = ops.crop_resize_entry(pages[0], (0, 0, 50, 20), (64, 128), (0, 0, 64, 128), 0, 0)
    for e in bad:
        with pytest.raises(RuntimeError, match="acai_crop_resize_to_patches"):
            ops.crop_resize_to_patches([good, e], out, P)
    assert float(out.abs().max()) == 0.0                                            # a refused call launches nothing
    with pytest.raises(ValueError):
        ops.crop_resize_to_patches([], out, P)


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e(dev):
    from conftest import load_golden
    from decode_support import build_vitomr
    from acai_omr_amd.inference.vitomr_inference import continuous_inference
    from acai_omr_amd.utils import DynamicResize
    fx = load_golden("vitomr_dh64b")
    cfg = fx["cfg"]
    assert (cfg["P"], cfg["pe_h"], cfg["pe_w"]) == (16, 4, 8)
    m = build_vitomr(cfg, fx["state_dict"], dev, torch.bfloat16, max_batch=2)      # a cache of 2 rows: 3 systems = two encode chunks, a refill
    tr = DynamicResize(16, 32, 4, 8, True)
    page = torch.from_numpy(R.synthetic_page()[0]).float() / 255.0
    crops = [page[y0:y1, x0:x1][None] for x0, y0, x1, y1 in TRUTH]
    want = continuous_inference(m, [tr(c) for c in crops], "cuda", max_inference_len=12)
    return m, tr, page, want


def _same(res, want):
    return torch.equal(res.seqs, want[0]) and torch.equal(res.log_probs, want[1]) and torch.equal(res.seq_mask, want[2])


def test_page_inference_with_boxes(dev, e2e):
    from acai_omr_amd.inference.vitomr_inference import page_inference
    m, tr, page, want = e2e
    assert want[0].shape[0] == 3
    res = page_inference(m, page, "cuda", tr, boxes=TRUTH, max_inference_len=12)
    assert _same(res, want)
    assert res.boxes == [TRUTH] and res.system_page == [0, 0, 0] and len(res) == 3
    assert res.sizes == [(32, 128), (16, 176), (32, 128)] and res.windows[1] == (0, 24, 16, 128)
    # the joins, on the real rows
    toks = res.tokens()[0]
    dec = m.decoder
    assert not any(int(s) in (dec.bos_idx, dec.eos_idx, dec.pad_idx) for s in toks) and toks.numel() > 0
    assert res.lmx(dec.idxs_to_tokens)[0].split(" ") == [dec.idxs_to_tokens[int(t)] for t in toks]
    a = res.avg_log_probs
    assert a.shape == (3,) and float((a - torch.stack([want[1][i][want[2][i]].sum() / want[2][i].sum() for i in range(3)])).abs().max()) < 1e-6
    assert res.avg_confidence[0] == pytest.approx(float(torch.exp(a.mean())), rel=1e-5)
    # fraction boxes that round to the truth boxes, out of order as a UI may send them
    fr = [{"x0": x0 / 200, "y0": y0 / 240, "x1": x1 / 200, "y1": y1 / 240} for x0, y0, x1, y1 in TRUTH]
    res_f = page_inference(m, page, "cuda", tr, boxes=[fr[2], fr[0], fr[1]], max_inference_len=12)
    assert res_f.boxes == [TRUTH] and _same(res_f, want)
    # a uint8 page: the same pixels after the 1 / 255 on load
    res_u8 = page_inference(m, torch.from_numpy(R.synthetic_page()[0]), "cuda", tr, boxes=TRUTH, max_inference_len=12)
    assert _same(res_u8, want)


def test_page_inference_detects(dev, e2e):
    from acai_omr_amd.inference.vitomr_inference import page_inference
    from acai_omr_amd.page import DetectConfig
    m, tr, page, want = e2e
    cfg = DetectConfig(0.5, DETECT["min_ink"], DETECT["merge_gap"], DETECT["min_height"], 0.5, DETECT["min_line_rows"], DETECT["margin"], 64)
    res = page_inference(m, page, "cuda", tr, boxes=None, max_inference_len=12, detect=cfg)
    assert res.boxes == [TRUTH] and _same(res, want)
    # two pages, the second blank: the first page's rows and an empty second page
    blank = torch.ones(100, 120)
    res2 = page_inference(m, [page, blank], "cuda", tr, max_inference_len=12, detect=cfg)
    assert res2.boxes == [TRUTH, []] and res2.system_page == [0, 0, 0] and _same(res2, want)
    assert res2.tokens()[1].numel() == 0 and res2.lmx(m.decoder.idxs_to_tokens)[1] == ""
    # no system at all: an empty result
    res0 = page_inference(m, [blank, blank], "cuda", tr, max_inference_len=12, detect=cfg)
    assert len(res0) == 0 and res0.boxes == [[], []] and res0.seqs is None
    assert len(page_inference(m, blank, "cuda", tr, boxes=[], max_inference_len=12)) == 0


def test_page_inference_prepares_pages_in_the_order_of_the_stages_run_by_hand(dev, e2e):
    """Every stage on, on a photo of the sheet on a table that lies on its side: ingest -> rectify -> flatten -> deskew, then assess and
    detect, is what the public stage functions give when they are called one after the other in that order."""
    import ingest_reference as G
    from test_gpu_ingest import _framed_clef_frame
    from acai_omr_amd.inference.vitomr_inference import page_inference
    from acai_omr_amd.page import deskew_pages, flatten_pages, ingest_pages, rectify_pages
    m, tr = e2e[:2]
    photo = torch.from_numpy(G.orient(_framed_clef_frame(), G.INVERSE[6]))        # the photo that code 6 turns upright
    want = page_inference(m, photo, "cuda", tr, max_inference_len=12, orient=6, rectify=True, flatten=True, deskew=True, assess=True)
    rect, quads = rectify_pages(ingest_pages(photo, 6))
    level, angles = deskew_pages(flatten_pages(rect))
    hand = page_inference(m, level[0], "cuda", tr, max_inference_len=12, assess=True)
    print(f"{len(want)} systems, quad {quads[0]}, angle {angles[0]}")
    assert len(want) > 0 and quads[0] is not None                                  # rows to compare, and a sheet that was found
    assert torch.equal(want.seqs, hand.seqs) and torch.equal(want.log_probs, hand.log_probs) and torch.equal(want.seq_mask, hand.seq_mask)
    assert want.boxes == hand.boxes and want.quality == hand.quality and want.system_staff_space == hand.system_staff_space
    assert want.quads == quads and want.angles == angles and want.page_sizes == [tuple(level[0].shape)] and want.flattened == [True]
    assert want.source_sizes == [tuple(photo.shape)] and want.orientations == [6]


def test_page_inference_with_a_permissive_grammar(dev, e2e):
    from acai_omr_amd.grammar import TokenAutomaton
    from acai_omr_amd.inference.vitomr_inference import page_inference
    m, tr, page, want = e2e
    dec = m.decoder
    V = dec.vocab_size
    everything = TokenAutomaton(torch.zeros(1, V, dtype=torch.int16), 0, torch.zeros(V, dtype=torch.int16), pad_idx=dec.pad_idx, bos_idx=dec.bos_idx,
                                eos_idx=dec.eos_idx)
    res = page_inference(m, page, "cuda", tr, boxes=TRUTH, max_inference_len=12, grammar=everything)
    assert torch.equal(res.seqs, want[0]) and torch.equal(res.seq_mask, want[2])
