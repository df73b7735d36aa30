"""Page deskew on the GPU (csrc/deskew.hip through ops.page_strips / page_skew_scores / page_rotate, page.estimate_skew / deskew_pages and
page_inference(deskew=...)).

Bars:
  * strips, scores and the uint8 rotation are defined in integers: torch.equal to the numpy restatement (tests/deskew_reference.py);
  * fp32 rotation: within 1e-6 absolute of the float64 restatement on values in [0, 1] - three fp32 interpolations with weights that are
    exact in fp32, each result in [0, 1], so a few ulp of 1 (6e-8 each): a bound, not a measurement;
  * estimate_skew: the scores equal the restatement's, and the angles too (the same float64 formula on the same integers);
  * page_inference(deskew=True): seqs, seq_mask and log_probs torch.equal to page_inference of the page levelled beforehand."""
import numpy as np
import pytest
import torch

import deskew_reference as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from acai_omr_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _ink_page(H, W, seed, p=0.5):
    rng = np.random.RandomState(seed)
    mask = rng.rand(H, W) < p
    return np.where(mask, rng.randint(0, 91, mask.shape), rng.randint(200, 256, mask.shape)).astype(np.uint8)


# ---- 1. strips ---------------------------------------------------------------------------------------------------------------------------
STRIP_H = 70      # more than one tile of 64 rows, and not a multiple of it


@pytest.mark.parametrize("W", [1, 15, 16, 17, 255, 257, 1000, 4099])
def test_strips_match_reference(dev, W):
    from acai_omr_amd import _lib, ops
    assert STRIP_H > _lib.STRIP_TILE_ROWS and STRIP_H % _lib.STRIP_TILE_ROWS
    u8 = _ink_page(STRIP_H, W, 100 + W)
    f32 = torch.from_numpy(u8).float() / 255.0
    pitch = -(-(W + 5) // 16) * 16                                    # rows on 16-byte boundaries whatever W is: the wide loads, then a tail
    wide = torch.zeros(STRIP_H, pitch, dtype=torch.uint8)             # ... with ink in the padding
    wide[:, :W] = torch.from_numpy(u8)
    wide32 = torch.zeros(STRIP_H, pitch)
    wide32[:, :W] = f32
    shifted = torch.zeros(STRIP_H, W + 2, dtype=torch.uint8)          # a view that starts one column in: on no 16-byte boundary
    shifted[:, 1:W + 1] = torch.from_numpy(u8)
    shifted32 = torch.zeros(STRIP_H, W + 2)
    shifted32[:, 1:W + 1] = f32
    pages = {"u8": torch.from_numpy(u8).to(dev), "f32": f32.to(dev), "u8 wide pitch": wide.to(dev)[:, :W], "f32 wide pitch": wide32.to(dev)[:, :W],
             "u8 shifted": shifted.to(dev)[:, 1:W + 1], "f32 shifted": shifted32.to(dev)[:, 1:W + 1], "f32 (1,H,W)": f32.to(dev)[None]}
    for S in _lib.STRIP_WIDTHS:
        want = torch.from_numpy(D.strips(u8, S))
        assert want.shape == (-(-W // S), STRIP_H) and int(want.sum()) == int((u8 < 128).sum())
        for name, page in pages.items():
            got = ops.page_strips(page, S, 0.5)
            assert got.dtype == torch.uint8 and got.is_contiguous() and torch.equal(got.cpu(), want), (W, S, name)


def test_strips_threshold_is_the_profiles_comparison(dev):
    from acai_omr_amd import ops
    rng = np.random.RandomState(3)
    u8 = rng.randint(0, 256, size=(33, 96)).astype(np.uint8)          # every value: the uint8 limit of the wide loads against value / 255 < thr
    f32 = u8.astype(np.float32) / np.float32(255.0)
    for thr in (0.5, 0.25, 0.0, 1.0, 1.5, 127 / 255):
        for S in (8, 16):
            want = torch.from_numpy(D.strips(u8, S, thr))
            assert torch.equal(ops.page_strips(torch.from_numpy(u8).to(dev), S, thr).cpu(), want), (thr, S)              # 16-byte loads
            assert torch.equal(ops.page_strips(torch.from_numpy(u8).to(dev)[:, 1:], S, thr).cpu(), torch.from_numpy(D.strips(u8[:, 1:], S, thr)))
            assert torch.equal(ops.page_strips(torch.from_numpy(f32).to(dev), S, thr).cpu(), torch.from_numpy(D.strips(f32, S, thr))), (thr, S)
    ink, _ = ops.page_profile(torch.from_numpy(u8).to(dev), 0.5)
    assert torch.equal(ops.page_strips(torch.from_numpy(u8).to(dev), 32, 0.5).sum(0, dtype=torch.int32), ink)            # the strips of a row add up to its profile


# ---- 2. scores ---------------------------------------------------------------------------------------------------------------------------
def _scores_case(dev, H, W, S, slopes, seed):
    from acai_omr_amd import ops
    rng = np.random.RandomState(seed)
    nS = -(-W // S)
    P = rng.randint(0, S + 1, size=(nS, H)).astype(np.uint8)
    want = torch.tensor(D.skew_scores(P, W, S, slopes), dtype=torch.int64)
    got = ops.page_skew_scores(torch.from_numpy(P).to(dev), W, S, slopes)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), want), (H, W, S, (got.cpu() - want).tolist())
    return want


SLOPES = [0, 1, -1, 700, -700, 4099, -5000, D.MAX_SLOPE, -D.MAX_SLOPE]


def _chunk_heights():
    from acai_omr_amd import _lib
    c = _lib.SKEW_CHUNK
    return [1, 2, 3, c - 1, c, c + 1, 2 * c + 1]


@pytest.mark.parametrize("i", range(7))
def test_scores_match_reference_at_every_chunk_edge(dev, i):
    H = _chunk_heights()[i]
    want = _scores_case(dev, H, 203, 16, SLOPES, seed=H)
    assert (H == 1) == (not any(want.tolist()))
    _scores_case(dev, H, 203, 16, [SLOPES[(i + 1) % len(SLOPES)]], seed=H + 1)         # K = 1
    _scores_case(dev, H, 64, 8 << (i % 4), [0, -300, D.MAX_SLOPE], seed=H + 2)         # every strip width over the seven cases


def test_scores_random_and_degenerate(dev):
    from acai_omr_amd import ops
    _scores_case(dev, 301, 1000, 32, list(range(-9000, 9001, 750)), seed=1)
    _scores_case(dev, 40, 17, 64, [0, 3], seed=2)                                      # one strip
    _scores_case(dev, 77, 130, 8, [0], seed=3)                                         # slope 0 alone
    # the two extreme slopes on a page so low that every row of the outer strips is shifted out: only the strips about the middle count
    want = _scores_case(dev, 3, 4099, 16, [D.MAX_SLOPE, -D.MAX_SLOPE, 0], seed=4)
    assert want[0] < want[2] and want[1] < want[2]
    # refusals: a slope beyond tan(15 deg), too many slopes, a strips tensor of another width
    P = torch.zeros(13, 5, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        ops.page_skew_scores(P, 203, 16, [D.MAX_SLOPE + 1])
    with pytest.raises(ValueError):
        ops.page_skew_scores(P, 203, 16, [0] * 1025)
    with pytest.raises(ValueError):
        ops.page_skew_scores(P, 300, 16, [0])


def test_score_passes_32_bits(dev):
    from acai_omr_amd import ops
    H, W, S = 1025, 4099, 16
    page = torch.full((H, W), 255, dtype=torch.uint8, device=dev)
    page[::2] = 0                                                                      # alternate rows are all ink
    P = ops.page_strips(page, S)
    widths = torch.tensor([min(S, W - s * S) for s in range(-(-W // S))], dtype=torch.uint8)
    want_P = torch.zeros(-(-W // S), H, dtype=torch.uint8)
    want_P[:, ::2] = widths[:, None]
    assert torch.equal(P.cpu(), want_P)
    slopes = [0, 40, -D.MAX_SLOPE]
    got = ops.page_skew_scores(P, W, S, slopes).cpu()
    assert int(got[0]) == (H - 1) * W * W and int(got[0]) > 1 << 32                    # 1.7e10
    assert got.tolist() == D.skew_scores(want_P.numpy(), W, S, slopes)


# ---- 3. rotate ---------------------------------------------------------------------------------------------------------------------------
ROT_ANGLES = [0.0, 0.7, -0.7, 9.0, -9.0, 90.0]


@pytest.mark.parametrize("H,W", [(1, 1), (7, 5), (64, 64), (65, 257)])
def test_rotate_u8_matches_reference(dev, H, W):
    from acai_omr_amd import ops
    rng = np.random.RandomState(H * 1000 + W)
    u8 = rng.randint(0, 256, size=(H, W)).astype(np.uint8)
    wide = torch.from_numpy(rng.randint(0, 256, size=(H, W + 7)).astype(np.uint8))     # pitch > W: what lies behind the page is not paper
    wide[:, :W] = torch.from_numpy(u8)
    for page in (torch.from_numpy(u8).to(dev), wide.to(dev)[:, :W]):
        for angle in ROT_ANGLES:
            cos_q, sin_q = D.rotation_q16(angle)
            assert ops.rotation_q16(angle) == (cos_q, sin_q)
            for fill in (255, 0):
                want = torch.from_numpy(D.rotate_u8(u8, cos_q, sin_q, fill))
                got = ops.page_rotate(page, angle, fill)
                assert got.dtype == torch.uint8 and got.is_contiguous() and torch.equal(got.cpu(), want), (H, W, angle, fill)
        assert torch.equal(ops.page_rotate(page, 0.0).cpu(), torch.from_numpy(u8))                     # angle 0: the page, bit for bit
        assert torch.equal(ops.page_rotate(page, cos_sin_q=(65536, 0)).cpu(), torch.from_numpy(u8))
        if H == W:
            assert torch.equal(ops.page_rotate(page, 90.0).cpu(), torch.from_numpy(np.rot90(u8, 1).copy()))   # counter-clockwise as displayed
    assert torch.equal(ops.page_rotate(torch.from_numpy(u8).to(dev), 3.0).cpu(), torch.from_numpy(D.rotate_u8(u8, *D.rotation_q16(3.0), 255)))    # default fill: paper


@pytest.mark.parametrize("H,W", [(1, 1), (7, 5), (64, 64), (65, 257)])
def test_rotate_f32_within_bound(dev, H, W):
    from acai_omr_amd import ops
    rng = np.random.RandomState(H * 1000 + W + 1)
    f32 = rng.rand(H, W).astype(np.float32)
    wide = torch.from_numpy(rng.rand(H, W + 3).astype(np.float32))
    wide[:, :W] = torch.from_numpy(f32)
    for page in (torch.from_numpy(f32).to(dev), wide.to(dev)[:, :W]):
        for angle in ROT_ANGLES:
            for fill in (1.0, 0.0):
                want = D.rotate_f64(f32, *D.rotation_q16(angle), fill)
                got = ops.page_rotate(page, angle, fill)
                assert got.dtype == torch.float32
                err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
                assert err < 1e-6, (H, W, angle, fill, err)
        assert torch.equal(ops.page_rotate(page, 0.0).cpu(), torch.from_numpy(f32))                    # weights 1 and 0: exact
    with pytest.raises(RuntimeError, match="acai_page_rotate"):
        ops.page_rotate(torch.from_numpy(f32).to(dev), cos_sin_q=(70000, 0))
    with pytest.raises(RuntimeError, match="acai_page_rotate"):
        ops.page_rotate((torch.from_numpy(f32) * 255).to(torch.uint8).to(dev), 1.0, fill=0.5)


# ---- 4. estimate, level, detect ----------------------------------------------------------------------------------------------------------
TILTS = [0.0, -1.3, 5.0]


@pytest.fixture(scope="module")
def tilted():
    """The synthetic page tilted by TILTS (the staff lines run down to the right by that angle) and a blank page, with the restatement's
    scores and angles at step 0.25, computed once."""
    from acai_omr_amd.page import SkewConfig
    cfg = SkewConfig(max_angle=10.0, step=0.25, strip=16)
    page = D.synthetic_page(0)[0]
    pages = [D.rotate_deg(page, -a) if a else page for a in TILTS] + [np.full((90, 130), 255, dtype=np.uint8)]
    ref = [D.estimate(p, cfg.strip, cfg.max_angle, cfg.step, cfg.ink_threshold) for p in pages]
    return cfg, pages, [a for a, _ in ref], [s for _, s in ref]


def test_estimate_skew_matches_reference(dev, tilted):
    from acai_omr_amd.page import estimate_skew, skew_scores
    cfg, pages, want_angles, want_scores = tilted
    same = [torch.from_numpy(p) for p in pages[:3]]                                   # one call, a list of pages (of one size here: one tensor of scores)
    scores = skew_scores(same, cfg)
    assert scores.dtype == torch.int64 and scores.shape == (3, 81) and scores.cpu().tolist() == want_scores[:3]
    got = estimate_skew([torch.from_numpy(p).to(dev) for p in pages], cfg)
    assert got == want_angles                                                          # exactly: the same float64 formula on the same integers
    assert got[0] == 0.0 and got[3] == 0.0 and abs(got[1] + 1.3) <= cfg.step and abs(got[2] - 5.0) <= cfg.step
    assert estimate_skew(torch.from_numpy(pages[1]), cfg) == [want_angles[1]]          # one page, from the host
    assert estimate_skew(torch.from_numpy(pages[2]).float() / 255.0, cfg) == [want_angles[2]]      # fp32: the same ink, the same scores


def test_deskew_then_detect_matches_reference(dev, tilted):
    from acai_omr_amd.page import DetectConfig, deskew_pages, detect_systems
    cfg, pages, want_angles, _ = tilted
    resolved = DetectConfig().resolved(360, 320)
    levelled, angles = deskew_pages([torch.from_numpy(p).to(dev) for p in pages], cfg=cfg)
    assert angles == want_angles
    base = D.detect(pages[0], resolved)
    for p, lev, a in zip(pages[:3], levelled, angles):
        want = D.rotate_deg(p, a) if a != 0.0 else p
        assert torch.equal(lev.cpu(), torch.from_numpy(want))
        boxes = detect_systems(lev)
        assert boxes == D.detect(want, resolved) and len(boxes) == 3
        assert max(abs(u - v) for b, c in zip(boxes, base) for u, v in zip(b, c)) <= 3
    assert len(detect_systems(torch.from_numpy(pages[2]).to(dev))) < 3                 # what deskew is for: the tilted page loses its systems
    # an angle of exactly 0.0 hands the page back, given angles are taken as they are
    dev_pages = [torch.from_numpy(p).to(dev) for p in pages[:2]]
    out, ang = deskew_pages(dev_pages, [0.0, 2.5])
    assert out[0] is dev_pages[0] and ang == [0.0, 2.5] and torch.equal(out[1].cpu(), torch.from_numpy(D.rotate_deg(pages[1], 2.5)))
    out, ang = deskew_pages(dev_pages[1], -1.0, fill=0)
    assert ang == [-1.0] and torch.equal(out[0].cpu(), torch.from_numpy(D.rotate_deg(pages[1], -1.0, fill=0)))


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------------
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


def test_page_inference_deskew(dev, e2e):
    from acai_omr_amd import ops
    from acai_omr_amd.inference.vitomr_inference import page_inference
    from acai_omr_amd.page import SkewConfig, estimate_skew
    m, tr = e2e
    page = D.synthetic_page(0)[0]
    tilted = torch.from_numpy(D.rotate_deg(page, -2.0)).to(dev)
    blank = torch.full((90, 130), 255, dtype=torch.uint8, device=dev)
    angle = estimate_skew(tilted)[0]
    assert abs(angle - 2.0) <= 0.125
    want = page_inference(m, ops.page_rotate(tilted, angle), "cuda", tr, max_inference_len=12)          # levelled beforehand, no deskew
    assert len(want) == 3 and want.angles == [0.0]
    res = page_inference(m, [tilted, blank], "cuda", tr, max_inference_len=12, deskew=True)
    assert res.angles == [angle, 0.0] and res.boxes == [want.boxes[0], []] and res.system_page == [0, 0, 0]
    assert torch.equal(res.seqs, want.seqs) and torch.equal(res.log_probs, want.log_probs) and torch.equal(res.seq_mask, want.seq_mask)
    assert res.page_sizes == [(360, 320), (90, 130)]
    # the box comes back as a tilted quadrilateral of the page that was passed in: its top edge runs down to the right by the angle
    q = res.box_corners(0)
    x0, y0, x1, y1 = res.boxes[0][0]
    assert (q[1][1] - q[0][1]) / (q[1][0] - q[0][0]) == pytest.approx(np.tan(np.radians(angle)), abs=1e-4)
    assert res.from_page_xy(0, *res.to_page_xy(0, 5.0, 7.0)) == pytest.approx((5.0, 7.0), abs=1e-9)
    # a SkewConfig, a given angle, and boxes of the caller's (they refer to the levelled page)
    assert _same(page_inference(m, tilted, "cuda", tr, max_inference_len=12, deskew=SkewConfig()), want)
    given = page_inference(m, tilted, "cuda", tr, max_inference_len=12, deskew=angle)
    assert _same(given, want) and given.angles == [angle]
    boxed = page_inference(m, tilted, "cuda", tr, boxes=want.boxes[0], max_inference_len=12, deskew=[angle])
    assert _same(boxed, want)
    # off: 0.0 and None are the present path
    level = torch.from_numpy(page).to(dev)
    off, zero = page_inference(m, level, "cuda", tr, max_inference_len=12), page_inference(m, level, "cuda", tr, max_inference_len=12, deskew=0.0)
    assert _same(off, zero) and off.angles == zero.angles == [0.0] and len(off) == 3
    # a blank page: no rows, no failure
    none = page_inference(m, blank, "cuda", tr, max_inference_len=12, deskew=True)
    assert len(none) == 0 and none.angles == [0.0] and none.boxes == [[]] and none.seqs is None
