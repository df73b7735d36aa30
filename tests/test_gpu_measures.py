"""Per-measure results on the GPU (measures.hip, acai_omr_amd/measures.py) against the float64 restatement in tests/measures_reference.py:
the four kernels alone, their refusals, the report end to end and measure_accuracy.
Seen on an MI355X, as shares of the bars the tests state: segment sums at most 0.10; measure maps 0.58 .. 0.98 (a span of one row is a single
rounding, which n * 2^-24 * sum|w p| just covers); extents 0.0013 on the well-conditioned maps and at most 0.10 on the report's own maps; centres
and variances at most 0.10.  Every integer output exact."""
import ctypes
import math

import numpy as np
import pytest
import torch

import measures_reference as R
from conftest import load_golden
from decode_support import _memory, _same, build_vitomr, dev  # noqa: F401

pytestmark = pytest.mark.gpu

BF, F32, I32, I64 = torch.bfloat16, torch.float32, torch.int32, torch.int64
E24 = 2.0 ** -24
GUARD, SENT = 64, -77
DELIMS8 = [3, 5, 7, 9, 11, 13, 15, 17]
STOP, CAP = 2, 4


# ---- 1. token_segments and segment_reduce -------------------------------------------------------------------------------------------------
def _segment_rows(ld, delims, rng):
    """Rows of width ld that cover the issue's cases; ordinary tokens are 20 .. 39, so neither delimiters nor STOP."""
    rows, lens = [], []

    def add(L, at=(), stop_at=None):
        t = rng.integers(20, 40, size=ld)
        for p in at:
            if 0 <= p < ld:
                t[p] = delims[int(rng.integers(len(delims)))]
        if stop_at is not None and 0 <= stop_at < ld:
            t[stop_at] = STOP
        rows.append(t)
        lens.append(L)

    for L in (0, 1, ld - 1, ld, ld + 3, -2):
        Lc = min(max(L, 0), ld)
        add(L, (0, 63, 64, Lc - 1))
        add(L, (63, 64, Lc - 1, Lc))          # (a delimiter AT the length is not the row's)
    add(ld, range(1, 7))                       # a run of consecutive delimiters
    add(ld, range(max(ld - 5, 0), ld))
    add(ld)                                    # no delimiter
    add(ld, (1, 3), stop_at=0)                 # stop before the first delimiter
    add(ld, (0, 3), stop_at=1)                 # right after one
    add(ld, (0, 2, 70), stop_at=64)
    add(ld, (0, 62, 63), stop_at=ld - 1)
    for n in (CAP - 1, CAP, CAP + 1):          # count = cap - 1, cap, cap + 1
        add(ld, sorted(rng.choice(ld, size=min(n, ld), replace=False).tolist()))
    for dens in (0.1, 0.5):
        add(int(rng.integers(0, ld + 1)), np.flatnonzero(rng.random(ld) < dens).tolist(), stop_at=int(rng.integers(0, 2 * ld)))
    return np.stack(rows).astype(np.int64), np.array(lens, dtype=np.int32)


def _guarded(shape, dtype, dev, fill=SENT):
    """(a contiguous view of `shape` inside a buffer filled with a sentinel, the buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf[GUARD:GUARD + n].view(*shape), buf


def _guards_intact(buf, fill=SENT):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


@pytest.mark.parametrize("ld", [1, 5, 63, 64, 65, 127, 128, 129, 200])
def test_segments_and_reductions_exact(dev, ld):
    """seg / count / bounds and every output of segment_reduce on dyadic values: torch.equal to the reference, 1 and 8 delimiter ids, with and
    without a stop token, bool masks as lengths, and sentinel-filled buffers around and inside the outputs."""
    from acai_omr_amd import ops
    rng = np.random.default_rng(ld)
    for delims, stop in ((DELIMS8[:1], STOP), (DELIMS8, STOP), (DELIMS8, -1)):
        tok, lens = _segment_rows(ld, delims, rng)
        Rn = tok.shape[0]
        want = R.token_segments(tok, lens, delims, stop, CAP)
        outs = [_guarded(s, I32, dev) for s in ((Rn, ld), (Rn,), (Rn, CAP, 2))]
        t_dev = torch.from_numpy(tok).to(dev)
        got = ops.token_segments(t_dev, torch.from_numpy(lens).to(dev), delims, stop=stop, cap=CAP, out=[o for o, _ in outs])
        for g, w, (o, buf), name in zip(got, want, outs, ("seg", "count", "bounds")):
            assert g.data_ptr() == o.data_ptr() and _guards_intact(buf), name
            assert torch.equal(g.cpu(), torch.from_numpy(w)), (name, ld, len(delims), stop)     # (no sentinel survives: every element is written)
        mask = torch.arange(ld)[None, :] < torch.from_numpy(lens)[:, None]
        for g, w in zip(ops.token_segments(t_dev, mask.to(dev), delims, stop=stop, cap=CAP), want):
            assert torch.equal(g.cpu(), torch.from_numpy(w))
        # segment_reduce on multiples of 2^-6: sums are exact, so all five outputs are the reference's
        K = 3
        vals = rng.integers(-64, 65, size=(K, Rn, ld)).astype(np.float32) / 64.0
        rw = R.segment_reduce(vals, want[2], want[1])
        routs = [_guarded((K, Rn, CAP), d, dev) for d in (F32, F32, F32, I32, I32)]
        rg = ops.segment_reduce(torch.from_numpy(vals).to(dev), got[2], got[1], out=[o for o, _ in routs])
        for g, w, (o, buf), name in zip(rg, rw, routs, rg._fields):
            assert _guards_intact(buf), name
            assert torch.equal(g.cpu(), torch.from_numpy(w).to(g.dtype)), (name, ld)


def test_segment_reduce_sums_within_the_depth_bar(dev):
    """General fp32 values: |sum - float64| <= (ceil(len / 64) + 6) * 2^-24 * sum|x| per span - the depth of the stated addition order -, min / max
    are the spans' own elements and the indices exact; 0/1 planes give exact counts; K = 1 and K = 8."""
    from acai_omr_amd import ops
    rng = np.random.default_rng(11)
    ld, Rn, cap = 700, 6, 7
    tok = rng.integers(20, 40, size=(Rn, ld)).astype(np.int64)
    for r, starts in enumerate(([0], [5, 6, 300], [1, 65, 129, 193, 257, 321, 385, 449], [10, 699], [], [0, 64, 128])):
        tok[r, starts] = 3
    lens = np.array([ld, ld, ld, ld, ld, 130], dtype=np.int32)
    _, count, bounds = R.token_segments(tok, lens, [3], -1, cap)
    seg_d = ops.token_segments(torch.from_numpy(tok).to(dev), torch.from_numpy(lens).to(dev), [3], cap=cap)
    worst = 0.0
    for K in (1, 8):
        vals = (rng.standard_normal((K, Rn, ld)) * 10 ** rng.uniform(-2, 2, size=(K, Rn, 1))).astype(np.float32)
        vals[K - 1] = (rng.random((Rn, ld)) < 0.3).astype(np.float32)       # a 0/1 plane
        got = ops.segment_reduce(torch.from_numpy(vals).to(dev), seg_d[2], seg_d[1])
        s, lo, hi, alo, ahi = R.segment_reduce(vals, bounds, count)
        mag, n = R.segment_abs_sums(vals, bounds, count)
        tol = (np.ceil(n / 64.0) + 6)[None] * E24 * mag
        err = np.abs(got.sum.cpu().double().numpy() - s)
        worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
        assert (err <= tol).all()
        assert torch.equal(got.sum[K - 1].cpu(), torch.from_numpy(s[K - 1]).float())
        for g, w in ((got.min, lo), (got.max, hi), (got.argmin, alo), (got.argmax, ahi)):
            assert torch.equal(g.cpu(), torch.from_numpy(w).to(g.dtype))
    print(f"\nsegment_reduce: worst |sum - f64| / bar = {worst:.3f}")


# ---- 2. attn_map_segment_sum --------------------------------------------------------------------------------------------------------------
def _map_buffer(maps, dev):
    from acai_omr_amd import ops
    lens_q, lens_k = [m.shape[0] for m in maps], [m.shape[1] for m in maps]
    offs, total = ops.attn_map_layout(lens_q, lens_k, guard=GUARD)
    buf = torch.full((total,), float("nan"), dtype=F32)
    for o, m in zip(offs, maps):
        buf[o:o + m.size] = torch.from_numpy(m.reshape(-1))
    cu = lambda ls: torch.tensor([0] + np.cumsum(ls).tolist(), dtype=I32, device=dev)   # noqa: E731
    return buf.to(dev), torch.tensor(offs, dtype=I64, device=dev), cu(lens_q), cu(lens_k), (lens_q, lens_k, offs)


@pytest.mark.parametrize("S", [1, 255, 256, 257, 600])
def test_segment_sum(dev, S):
    """Spans of 1, 2 and 33 rows and the whole block; an image without segments; weights None = a tensor of ones, bit for bit; two runs bitwise
    equal; dyadic inputs exact; general inputs within n * 2^-24 * sum|w p|; the whole-block span against attn_map_weighted_sum within the
    same bar; the layout is attn_map_layout(counts, lens_k)."""
    from acai_omr_amd import ops
    rng = np.random.default_rng(S)
    shapes = [(40, S), (6, 9), (5, 7)]
    ranges = [[(3, 4), (4, 6), (6, 39), (0, 40), (39, 40)], [], [(0, 5), (2, 3)]]
    counts = [len(r) for r in ranges]
    rt = torch.tensor([p for r in ranges for p in r], dtype=I32, device=dev).view(-1, 2)
    worst = 0.0
    for dyadic in (True, False):
        if dyadic:
            maps = [rng.integers(0, 65, size=s).astype(np.float32) / 64.0 for s in shapes]
            w = [rng.integers(-8, 9, size=s[0]).astype(np.float32) / 8.0 for s in shapes]
        else:
            maps = [rng.random(s).astype(np.float32) for s in shapes]
            w = [rng.standard_normal(s[0]).astype(np.float32) for s in shapes]
        buf, off, cu_q, cu_k, layout = _map_buffer(maps, dev)
        wt = torch.from_numpy(np.concatenate(w)).to(dev)
        out, offs, seg_off, cu_seg = ops.attn_map_segment_sum(buf, off, cu_q, cu_k, wt, rt, counts, layout=layout)
        again = ops.attn_map_segment_sum(buf, off, cu_q, cu_k, wt, rt, counts)[0]           # (layout read back from the device)
        assert torch.equal(out, again)
        assert (offs, out.numel()) == ops.attn_map_layout(counts, [s[1] for s in shapes]) and seg_off.tolist() == offs
        assert cu_seg.tolist() == [0] + np.cumsum(counts).tolist()
        want, mag = R.attn_map_segment_sum(maps, w, ranges)
        for b, (o, c, (_, s)) in enumerate(zip(offs, counts, shapes)):
            got = out[o:o + c * s].view(c, s).cpu()
            if dyadic:
                assert torch.equal(got, torch.from_numpy(want[b]).float()), (S, b)
            else:
                n = np.array([t1 - t0 for t0, t1 in ranges[b]], dtype=np.float64).reshape(-1, 1)
                err, tol = np.abs(got.double().numpy() - want[b]), n * E24 * mag[b]
                assert (err <= tol).all(), (S, b, float((err / tol).max()))
                if c:
                    worst = max(worst, float((err / tol).max()))
        ones = ops.attn_map_segment_sum(buf, off, cu_q, cu_k, torch.ones_like(wt), rt, counts, layout=layout)[0]
        none = ops.attn_map_segment_sum(buf, off, cu_q, cu_k, None, rt, counts, layout=layout)[0]
        assert torch.equal(ones, none)
        if not dyadic:   # one span over every row = the weighted sum, within the same bar
            full = [[(0, s[0])] for s in shapes]
            ft = torch.tensor([p for r in full for p in r], dtype=I32, device=dev).view(-1, 2)
            fo = ops.attn_map_segment_sum(buf, off, cu_q, cu_k, wt, ft, [1, 1, 1], layout=layout)[0]
            heat = ops.attn_map_weighted_sum(buf, off, cu_q, cu_k, wt, 40, layout=layout)
            _, fmag = R.attn_map_segment_sum(maps, w, full)
            tol = np.concatenate([s[0] * E24 * g[0] for s, g in zip(shapes, fmag)])
            assert (np.abs(fo.cpu().double().numpy() - heat.cpu().double().numpy()) <= tol).all()
    print(f"\nsegment_sum S={S}: worst err / bar = {worst:.3f}")
    for bad in ([(3, 3)], [(-1, 2)], [(39, 41)]):
        r = torch.tensor(bad + [(0, 1)] * 6, dtype=I32, device=dev)
        with pytest.raises(ValueError, match="attn_map_segment_sum: image 0 has the range"):
            ops.attn_map_segment_sum(buf, off, cu_q, cu_k, wt, r, counts, layout=layout)
    with pytest.raises(ValueError, match="ranges must be"):
        ops.attn_map_segment_sum(buf, off, cu_q, cu_k, wt, rt[:-1].contiguous(), counts, layout=layout)
    with pytest.raises(ValueError, match="weights"):
        ops.attn_map_segment_sum(buf, off, cu_q, cu_k, wt[:-1].contiguous(), rt, counts, layout=layout)


# ---- 3. attn_map_extent -------------------------------------------------------------------------------------------------------------------
def _extents(maps, gws, q, dev):
    from acai_omr_amd import ops
    buf, off, cu_q, cu_k, layout = _map_buffer(maps, dev)
    return ops.attn_map_extent(buf, off, cu_q, cu_k, gws, q, layout=layout).cpu().double().numpy()


def test_extent_exact_cases(dev):
    """Maps of multiples of 1/64 whose quotients are dyadic (p[y][x] = c[x] r[y] with powers of two): q = 0.25 within 2^-22 relative; q = 0 gives
    the outer edges of the non-zero cells; a map without mass gives zeros; a last partial grid row; grid_w of 1 and of S."""
    rng = np.random.default_rng(2)
    maps, gws = [], []
    for h, w in ((4, 8), (16, 32), (1, 16), (8, 1), (64, 64)):
        c, r = 2.0 ** rng.integers(0, 3, size=w) / 8, 2.0 ** rng.integers(0, 3, size=h) / 8
        maps.append(np.stack([np.outer(r, c).reshape(-1), np.outer(r[::-1], c[::-1]).reshape(-1)]).astype(np.float32))
        gws.append(w)
    got, want = _extents(maps, gws, 0.25, dev), R.attn_map_extent(maps, gws, 0.25)
    assert (np.abs(got - want) <= 2.0 ** -22 * np.abs(want)).all(), np.abs(got - want).max()
    # q = 0, no mass, a partial last row, grid_w 1 and S
    p = np.zeros((3, 30), dtype=np.float32)
    p[0, [2 * 5 + 1, 3 * 5 + 3]] = 0.5
    p[2, 7] = 0.25
    got0 = _extents([p, np.ones((1, 10), dtype=np.float32), np.ones((2, 6), dtype=np.float32), np.ones((2, 6), dtype=np.float32)], [5, 4, 1, 6], 0.0, dev)
    assert got0.tolist() == [[1, 2, 4, 4], [0, 0, 0, 0], [2, 1, 3, 2], [0, 0, 4, 3], [0, 0, 1, 6], [0, 0, 1, 6], [0, 0, 6, 1], [0, 0, 6, 1]]
    part = _extents([np.ones((1, 10), dtype=np.float32)], [4], 0.25, dev)
    assert np.allclose(part, R.attn_map_extent([np.ones((1, 10))], [4], 0.25), rtol=2.0 ** -22, atol=0)


def test_extent_general_case(dev):
    """Strictly positive maps whose every marginal cell is at least m / (8 n) (asserted with the float64 reference).  A running sum is off by at
    most S * 2^-24 * m, hence |pos - reference| <= 2 * S * 2^-24 * m / a_min <= 16 * n * S * 2^-24 cells: for the largest grid here, 16 x 32
    (S = 512), that is 2^-6 = 0.0156 cells along x (n = 32) and 2^-7 along y."""
    rng = np.random.default_rng(4)
    grids = [(16, 32), (7, 13), (3, 32), (16, 5)]
    maps = [(0.25 + rng.random((9, h * w)) ** 3).astype(np.float32) for h, w in grids]
    gws = [w for _, w in grids]
    worst = 0.0
    for q in (0.05, 0.25, 0.499):
        got, want = _extents(maps, gws, q, dev), R.attn_map_extent(maps, gws, q)
        row = 0
        for mp, (h, w) in zip(maps, grids):
            for p in mp:
                ax, ay = R.marginals(p, w)
                assert ax.min() >= ax.sum() / (8 * w) and ay.min() >= ay.sum() / (8 * h)
                bar = np.array([w, h, w, h]) * 16.0 * h * w * E24
                err = np.abs(got[row] - want[row])
                assert (err <= bar).all(), (h, w, q, err, bar)
                worst = max(worst, float((err / bar).max()))
                row += 1
    print(f"\nextent: worst err / bar = {worst:.4f}")


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
def _refusal_state(dev):
    tok = torch.full((3, 10), 3, dtype=I64, device=dev)
    s = dict(tok=tok, lens=torch.full((3,), 10, dtype=I32, device=dev), seg=torch.full((3, 10), SENT, dtype=I32, device=dev),
             count=torch.full((3,), SENT, dtype=I32, device=dev), bounds=torch.full((3, 4, 2), SENT, dtype=I32, device=dev),
             vals=torch.ones(2, 3, 10, device=dev), fout=torch.full((3, 2, 3, 4), float(SENT), device=dev),
             iout=torch.full((2, 2, 3, 4), SENT, dtype=I32, device=dev), map=torch.ones(3 * 4 * 6, device=dev),
             off=torch.tensor([0, 24, 48], dtype=I64, device=dev), cu_q=torch.tensor([0, 4, 8, 12], dtype=I32, device=dev),
             cu_k=torch.tensor([0, 6, 12, 18], dtype=I32, device=dev), rng=torch.tensor([[0, 2]] * 3, dtype=I32, device=dev),
             cu_seg=torch.tensor([0, 1, 2, 3], dtype=I32, device=dev), seg_off=torch.tensor([0, 6, 12], dtype=I64, device=dev),
             sums=torch.full((18,), float(SENT), device=dev), ext=torch.full((12, 4), float(SENT), device=dev))
    return s


def _untouched(s):
    torch.cuda.synchronize()
    return all(bool((s[k] == SENT).all()) for k in ("seg", "count", "bounds", "fout", "iout", "sums", "ext"))


REFUSALS = [
    ("acai_token_segments", dict(ld=0)), ("acai_token_segments", dict(R=-1)), ("acai_token_segments", dict(nd=0)), ("acai_token_segments", dict(nd=9)),
    ("acai_token_segments", dict(delims=None)), ("acai_token_segments", dict(cap=0)), ("acai_token_segments", dict(stop=-2)),
    ("acai_token_segments", dict(tok=None)), ("acai_token_segments", dict(lens=None)), ("acai_token_segments", dict(seg=None)),
    ("acai_token_segments", dict(count=None)), ("acai_token_segments", dict(bounds=None)),
    ("acai_segment_reduce", dict(K=0)), ("acai_segment_reduce", dict(K=9)), ("acai_segment_reduce", dict(R=-1)), ("acai_segment_reduce", dict(ld=0)),
    ("acai_segment_reduce", dict(cap=0)), ("acai_segment_reduce", dict(vals=None)), ("acai_segment_reduce", dict(bounds=None)),
    ("acai_segment_reduce", dict(count=None)), ("acai_segment_reduce", dict(argmax=None)), ("acai_segment_reduce", dict(K=8, R=1 << 20, cap=1 << 10)),
    ("acai_attn_map_segment_sum", dict(B=-1)), ("acai_attn_map_segment_sum", dict(B=65536)), ("acai_attn_map_segment_sum", dict(max_seg=65536)),
    ("acai_attn_map_segment_sum", dict(max_k=-1)), ("acai_attn_map_segment_sum", dict(map=None)), ("acai_attn_map_segment_sum", dict(rng=None)),
    ("acai_attn_map_segment_sum", dict(cu_seg=None)), ("acai_attn_map_segment_sum", dict(seg_off=None)), ("acai_attn_map_segment_sum", dict(sums=None)),
    ("acai_attn_map_extent", dict(B=513)), ("acai_attn_map_extent", dict(B=-1)), ("acai_attn_map_extent", dict(max_q=-1)), ("acai_attn_map_extent", dict(q=0.5)),
    ("acai_attn_map_extent", dict(q=-0.01)), ("acai_attn_map_extent", dict(q=float("nan"))), ("acai_attn_map_extent", dict(gw=[6, 0, 6])),
    ("acai_attn_map_extent", dict(gw=[6, 6, 4097])), ("acai_attn_map_extent", dict(map=None)), ("acai_attn_map_extent", dict(ext=None)),
    ("acai_attn_map_extent", dict(gw=None)),
]


@pytest.mark.parametrize("entry,change", REFUSALS, ids=[f"{e[5:]}-{'-'.join(f'{k}={v}' for k, v in c.items())}" for e, c in REFUSALS])
def test_f_refusals(dev, entry, change):
    """Every condition an entry validates raises with the entry's name, and nothing is launched: every output buffer keeps its sentinel."""
    from acai_omr_amd import _lib
    L, s = _lib.lib(), _refusal_state(dev)
    a = dict(ld=10, R=3, nd=1, cap=4, stop=2, K=2, B=3, max_k=6, max_seg=1, max_q=4, q=0.1, gw=[6, 6, 6], delims=[3], argmax=s["iout"][1])
    a.update({k: s[k] for k in ("tok", "lens", "seg", "count", "bounds", "vals", "map", "rng", "cu_seg", "seg_off", "sums", "ext")})
    a.update(change)
    p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    with pytest.raises(RuntimeError, match=rf"\): {entry}: "):
        if entry == "acai_token_segments":
            d = None if a["delims"] is None else (ctypes.c_int64 * 8)(*a["delims"])
            rc = L.acai_token_segments(p(a["tok"]), a["ld"], p(a["lens"]), a["R"], d, a["nd"], a["stop"], a["cap"], p(a["seg"]), p(a["count"]),
                                       p(a["bounds"]), st)
        elif entry == "acai_segment_reduce":
            f = s["fout"]
            rc = L.acai_segment_reduce(p(a["vals"]), a["K"], a["R"], a["ld"], p(a["bounds"]), p(a["count"]), a["cap"], p(f[0]), p(f[1]), p(f[2]),
                                       p(s["iout"][0]), p(a["argmax"]), st)
        elif entry == "acai_attn_map_segment_sum":
            rc = L.acai_attn_map_segment_sum(p(a["map"]), p(s["off"]), p(s["cu_q"]), p(s["cu_k"]), None, p(a["rng"]), p(a["cu_seg"]), p(a["seg_off"]),
                                             a["B"], a["max_k"], a["max_seg"], p(a["sums"]), st)
        else:
            g = None if a["gw"] is None else (ctypes.c_int32 * 3)(*a["gw"])
            rc = L.acai_attn_map_extent(p(a["map"]), p(s["off"]), p(s["cu_q"]), p(s["cu_k"]), g, a["B"], a["max_q"], a["q"], p(a["ext"]), st)
        _lib.check(rc, entry)
    assert _untouched(s)


def test_wrappers_refuse_on_the_host_and_zero_rows_return_at_once(dev):
    from acai_omr_amd import ops
    tok, lens = torch.zeros(2, 5, dtype=I64, device=dev), torch.zeros(2, dtype=I32, device=dev)
    for kw in (dict(delims=[]), dict(delims=list(range(9))), dict(delims=[-1]), dict(delims=[3], cap=0), dict(delims=[3], stop=-2)):
        with pytest.raises(ValueError, match="token_segments"):
            ops.token_segments(tok, lens, **kw)
    with pytest.raises(ValueError, match="token_segments"):
        ops.token_segments(tok, lens[:1], [3])
    with pytest.raises(ValueError, match="token_segments"):
        ops.token_segments(tok[0], lens, [3])
    with pytest.raises(TypeError):
        ops.token_segments(tok, lens.long(), [3])
    seg, count, bounds = ops.token_segments(tok[:0], lens[:0], [3], cap=3)
    assert seg.shape == (0, 5) and count.shape == (0,) and bounds.shape == (0, 3, 2)
    assert ops.segment_reduce(torch.zeros(2, 0, 5, device=dev), bounds, count).sum.shape == (2, 0, 3)
    _, count, bounds = ops.token_segments(tok, lens, [3], cap=3)
    for vals in (torch.zeros(2, 5, device=dev), torch.zeros(9, 2, 5, device=dev), torch.zeros(1, 3, 5, device=dev)):
        with pytest.raises(ValueError, match="segment_reduce"):
            ops.segment_reduce(vals, bounds, count)
    buf, off, cu_q, cu_k, layout = _map_buffer([np.ones((2, 6), dtype=np.float32)], dev)
    for gw, q in (([0], 0.1), ([4097], 0.1), ([6], 0.5), ([6], -0.1), ([6, 6], 0.1)):
        with pytest.raises(ValueError, match="attn_map_extent"):
            ops.attn_map_extent(buf, off, cu_q, cu_k, gw, q, layout=layout)
    big = torch.zeros(5000, device=dev)
    with pytest.raises(ValueError, match="grid sides"):
        ops.attn_map_extent(big, off, torch.tensor([0, 1], dtype=I32, device=dev), torch.tensor([0, 4097], dtype=I32, device=dev), [1], 0.1)


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------------------
FIXTURE, DELIMS = "vitomr_dh64b", (68, 86)
_MODELS = {}


def _model(dev, bf16):
    if bf16 not in _MODELS:
        fx = load_golden(FIXTURE)
        _MODELS[bf16] = (fx, build_vitomr(fx["cfg"], fx["state_dict"], dev, BF if bf16 else torch.float, 9))
    return _MODELS[bf16]


def _nan_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(torch.nan_to_num(a.double(), nan=-5.0), torch.nan_to_num(b.double(), nan=-5.0))


def _same_confidence(a, b):
    for f in ("log_prob", "entropy", "rank", "top_tokens", "top_log_probs"):
        assert _nan_equal(getattr(a, f), getattr(b, f)), f
    assert len(a.uncertainty) == len(b.uncertainty) and all(torch.equal(x, y) for x, y in zip(a.uncertainty, b.uncertainty))
    for f in ("patch", "center_px", "spread_px", "peak"):
        assert _nan_equal(getattr(a.alignment, f), getattr(b.alignment, f)), f
    assert a.alignment.grids == b.alignment.grids


def _check_report(rep, seqs, Ls, lp, ent, rank, maps, grids, P, delims, eos, cap, q, weight=None, what=""):
    """rep against the reference applied to the pass's own per-token outputs: lp / ent / rank (B, T') and maps, per image (L - 1, S)."""
    B = seqs.shape[0]
    tok = seqs.cpu().numpy()
    seg, count, bounds = R.token_segments(tok, Ls, delims, eos, cap)
    n = np.minimum(count, cap)
    M = int(n.max())
    assert rep.count.tolist() == count.tolist() and rep.overflowed.tolist() == (count > cap).tolist() and rep.bounds.shape == (B, M, 2)
    valid = np.arange(M)[None, :] < n[:, None]
    wb = np.where(valid[..., None], bounds[:, :M], -1)
    assert torch.equal(rep.bounds.cpu(), torch.from_numpy(wb).long())
    assert torch.equal(rep.n_tokens.cpu(), torch.from_numpy(np.where(valid, wb[..., 1] - wb[..., 0], -1)).long())
    planes = np.stack([np.nan_to_num(lp.cpu().numpy(), nan=0.0), np.nan_to_num(ent.cpu().numpy(), nan=0.0), (rank.cpu().numpy() > 0).astype(np.float32)])
    s, lo, hi, alo, ahi = R.segment_reduce(planes, bounds, count)
    mag, ln = R.segment_abs_sums(planes, bounds, count)
    for got, k, name in ((rep.mean_log_prob, 0, "mean_log_prob"), (rep.mean_entropy, 1, "mean_entropy")):
        g = got.cpu().double().numpy()
        assert np.array_equal(np.isnan(g), ~valid), name
        want = s[k, :, :M] / np.maximum(ln[:, :M], 1)
        tol = ((np.ceil(ln[:, :M] / 64.0) + 6) * E24 * mag[k, :, :M]) / np.maximum(ln[:, :M], 1) + E24 * np.abs(want)
        assert (np.abs(g - want)[valid] <= tol[valid]).all(), (name, what)
    for got, w, name in ((rep.min_log_prob, lo[0], "min_log_prob"), (rep.max_entropy, hi[1], "max_entropy")):
        assert _nan_equal(got.cpu(), torch.from_numpy(np.where(valid, w[:, :M], np.nan)).float()), name
    assert torch.equal(rep.weakest_token.cpu(), torch.from_numpy(np.where(valid, alo[0][:, :M], -1)).long())
    assert torch.equal(rep.forced.cpu(), torch.from_numpy(np.where(valid, s[2][:, :M], -1)).long())
    # the measure maps and what is read off them
    worst_box = worst_c = 0.0
    for i, (h, w) in enumerate(grids):
        S = h * w
        rg = [(int(a) - 1, int(b) - 1) for a, b in bounds[i, :n[i]]]
        wt = None if weight is None else [weight[i]]
        want, mag_m = R.attn_map_segment_sum([maps[i].cpu().double().numpy()], wt, [rg])
        got = rep.maps[i].cpu().double().numpy()
        assert got.shape == (n[i], S)
        rows = np.array([b - a for a, b in rg], dtype=np.float64).reshape(-1, 1)
        assert (np.abs(got - want[0]) <= rows * E24 * mag_m[0]).all(), (what, i)
        for m in range(n[i]):
            # the map above is checked against float64; box, centre and spread are checked on the kernels' exact input, the map the report
            # holds.  The extent bar before its premise is used: a running sum is off by at most S 2^-24 m, so a position by at most twice
            # that over the smallest marginal cell that has mass
            amin = np.array([x[x > 0].min() for x in R.marginals(got[m], w)] * 2)
            bar = 2.0 * S * E24 * got[m].sum() / amin * P
            err = np.abs(rep.box_px[i, m].cpu().double().numpy() - R.extent(got[m], w, q) * P)
            assert (err <= bar).all(), (what, i, m, err, bar)
            worst_box = max(worst_box, float((err / bar).max()))
            c = R.locate(got[m], w)
            side = max(h, w)
            cbar = (S / 64.0 + 8) * 2.0 ** -23 * side * P
            cerr = np.abs(rep.center_px[i, m].cpu().double().numpy() - c[:2] * P).max()
            verr = np.abs(rep.spread_px[i, m].cpu().double().numpy() ** 2 - (c[2:] * P) ** 2).max()
            assert cerr <= cbar and verr <= 2 * cbar * side * P, (what, i, m, cerr, verr, cbar)
            worst_c = max(worst_c, cerr / cbar, verr / (2 * cbar * side * P))
        for t in (rep.box_px, rep.center_px, rep.spread_px):
            assert bool(torch.isnan(t[i, n[i]:]).all()) and not bool(torch.isnan(t[i, :n[i]]).any())
    print(f"\n{what}: counts {count.tolist()}, worst box err / bar {worst_box:.4f}, worst centre or variance err / bar {worst_c:.4f}")
    return seg, count, n


def _targets(seqs, Ls):
    """The decode's own rows with one token substituted, one removed and one inserted (ordinary ids 20 / 21: neither a delimiter nor special)."""
    out = []
    for i, L in enumerate(Ls):
        t = seqs[i, :L].tolist()
        t[3] = 20 if t[3] != 20 else 21
        del t[L // 2]
        t.insert(L - 3, 21 if t[L - 3] != 21 else 20)
        out.append(torch.tensor(t, dtype=I64))
    return out


def _check_errors(rep, al, seg, n, what):
    errors, outside = R.report_errors(seg, *(t.cpu().numpy() for t in (al.pred_op, al.tgt_to_pred, al.tgt_slot)), n)
    M = errors.shape[1]
    valid = np.arange(M)[None, :] < n[:, None]
    assert torch.equal(rep.errors.cpu(), torch.from_numpy(np.where(valid[..., None], errors, -1)))
    assert torch.equal(rep.correct.cpu(), torch.from_numpy((errors.sum(-1) == 0) & valid))
    assert torch.equal(rep.outside_errors.cpu(), torch.from_numpy(outside))
    total = rep.errors.clamp(min=0).sum(1) + rep.outside_errors
    assert torch.equal(total.cpu(), al.counts[:, 1:].long().cpu()), what
    assert int(al.counts[:, 1:].sum()) >= seg.shape[0]                # the edits are real errors
    assert not bool(rep.correct.all()) or int(rep.outside_errors.sum()) > 0


def test_measured_inference_end_to_end_bf16(dev, monkeypatch):
    from acai_omr_amd import ops
    from acai_omr_amd.inference.vitomr_inference import confident_inference, inference, measured_inference
    from acai_omr_amd.measures import MeasureConfig
    fx, m = _model(dev, True)
    T, P = fx["cfg"]["gen_len"], fx["cfg"]["P"]
    eos = m.decoder.eos_idx
    before = inference(m, fx["imgs"], "cuda", max_inference_len=T)
    Ls = m._alignment_lengths(*before[::2])
    seg, count, _ = R.token_segments(before[0].cpu().numpy(), Ls, DELIMS, eos, 256)
    assert (count >= 3).all(), count                                  # the random-weight model never emits `measure`: these ids do occur
    # unused, the hook is not taken: confident_inference runs none of the four ops (what else _confidence_packed does with measure=None is the
    # parent's code: its results are compared bit for bit with inference() and with measured_inference's below)
    calls = {k: 0 for k in ("token_segments", "segment_reduce", "attn_map_segment_sum", "attn_map_extent")}
    for k in calls:
        def counted(*a, _k=k, _f=getattr(ops, k), **kw):
            calls[_k] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(ops, k, counted)
    plain = confident_inference(m, fx["imgs"], "cuda", max_inference_len=T, uncertainty="entropy")
    assert not any(calls.values()), calls
    cfg = MeasureConfig(delimiters=DELIMS, return_maps=True)
    seqs, lps, mask, conf, rep = measured_inference(m, fx["imgs"], "cuda", max_inference_len=T, measures=cfg)
    assert calls == {"token_segments": 1, "segment_reduce": 1, "attn_map_segment_sum": 1, "attn_map_extent": 1}
    _same((seqs, lps, mask), plain[:3])
    _same((seqs, lps, mask), before)
    _same_confidence(conf, plain[3])
    grids = conf.alignment.grids
    seg, count, n = _check_report(rep, seqs, Ls, conf.log_prob, conf.entropy, conf.rank, conf.alignment.maps, grids, P, DELIMS, eos, 256, 0.05,
                                  what="bf16")
    assert rep.errors is None and rep.correct is None and rep.outside_errors is None and rep.delimiters == DELIMS
    # with targets; a surprisal-weighted map; a cap below the count
    tg = _targets(seqs, Ls)
    cfg_w = MeasureConfig(delimiters=DELIMS, return_maps=True, weight="surprisal", quantile=0.25, max_measures=4)
    *_, conf_w, rep_w = measured_inference(m, fx["imgs"], "cuda", max_inference_len=T, measures=cfg_w, target_lmx_seqs=tg)
    _same_confidence(conf_w, plain[3])
    wts = [(-conf_w.log_prob[i, 1:L]).cpu().double().numpy() for i, L in enumerate(Ls)]
    seg_w, _, n_w = _check_report(rep_w, seqs, Ls, conf_w.log_prob, conf_w.entropy, conf_w.rank, conf_w.alignment.maps, grids, P, DELIMS, eos, 4, 0.25,
                                  weight=wts, what="bf16 surprisal cap 4")
    assert rep_w.overflowed.tolist() == [True] * len(Ls) and rep_w.bounds.shape[1] == 4
    *_, rep_t = measured_inference(m, fx["imgs"], "cuda", max_inference_len=T, measures=cfg, target_lmx_seqs=tg)
    al = m._error_weights(seqs, mask, tg, None)[0]
    _check_errors(rep_t, al, seg, n, "bf16")
    # a decode after the reports is bitwise the decode before them
    _same(inference(m, fx["imgs"], "cuda", max_inference_len=T), before)
    # the default configuration cuts at `measure`, id 3 in the vocabulary
    assert MeasureConfig().resolve(m.decoder) == [3]
    *_, rep_d = measured_inference(m, fx["imgs"], "cuda", max_inference_len=T)
    want = R.token_segments(seqs.cpu().numpy(), Ls, [3], eos, 256)[1]
    assert rep_d.delimiters == (3,) and rep_d.count.tolist() == want.tolist() and rep_d.maps is None
    with pytest.raises(TypeError):
        measured_inference(m, fx["imgs"], "cuda", max_inference_len=T, measures=cfg, beam=2)
    with pytest.raises(ValueError):
        measured_inference(m, fx["imgs"], "cuda", max_inference_len=T, measures=MeasureConfig(delimiters=("no such token",)))


def test_measure_report_end_to_end_fp32(dev):
    """The model method on fp32 memories, outside autocast: the report against the reference on uncertainty_maps' / locate_tokens' own outputs."""
    from acai_omr_amd.measures import MeasureConfig
    fx, m = _model(dev, False)
    T, P = fx["cfg"]["gen_len"], fx["cfg"]["P"]
    mem, lmask = _memory(m, fx["imgs"], False)
    with torch.no_grad():
        seqs, lps, smask = m.cached_greedy_generate(mem, lmask, max_len=T)
        grids = [(int(t.shape[-2]) // P, int(t.shape[-1]) // P) for t in fx["imgs"]]
        Ls = m._alignment_lengths(seqs, smask)
        assert (R.token_segments(seqs.cpu().numpy(), Ls, DELIMS, m.decoder.eos_idx, 256)[1] >= 3).all()
        conf = m.uncertainty_maps(mem, lmask, seqs, smask, grids=grids)
        loc = m.locate_tokens(mem, lmask, seqs, smask, grids=grids, return_maps=True)
        tg = _targets(seqs, Ls)
        cfg = MeasureConfig(delimiters=DELIMS, return_maps=True)
        rep = m.measure_report(mem, lmask, seqs, smask, config=cfg, target_lmx_seqs=tg, grids=grids)
        again = m.measure_report(mem, lmask, seqs, smask, config=cfg, target_lmx_seqs=tg, grids=grids)
        al = m._error_weights(seqs, smask, tg, None)[0]
        after = m.cached_greedy_generate(mem, lmask, max_len=T)
    seg, count, n = _check_report(rep, seqs, Ls, conf.log_prob, conf.entropy, conf.rank, loc.maps, grids, P, DELIMS, m.decoder.eos_idx, 256, 0.05,
                                  what="fp32")
    _check_errors(rep, al, seg, n, "fp32")
    for f in ("bounds", "mean_log_prob", "max_entropy", "center_px", "spread_px", "box_px", "errors"):
        assert _nan_equal(getattr(rep, f), getattr(again, f)), f          # the same bits on every run
    _same(after, (seqs, lps, smask))
    with pytest.raises(ValueError, match="grids"):
        m.measure_report(mem, lmask, seqs, smask, config=cfg)
    with pytest.raises(TypeError):
        m.measure_report(mem, lmask, seqs, smask, config="measure", grids=grids)


def test_measured_inference_pruned(dev):
    """prune=True on images where pruning drops patches: the report still equals the reference on that call's own per-token outputs, whose maps
    speak of the FULL grid - the measure maps were summed over the kept patches and expanded afterwards."""
    import prune_reference as PR
    from acai_omr_amd.inference.vitomr_inference import confident_inference, measured_inference
    from acai_omr_amd.measures import MeasureConfig
    fx, m = _model(dev, True)
    T, P = fx["cfg"]["gen_len"], fx["cfg"]["P"]
    imgs = PR.model_images()
    plain = confident_inference(m, imgs, "cuda", max_inference_len=T, uncertainty="entropy", prune=True)
    seqs = plain[0]
    Ls = m._alignment_lengths(seqs, plain[2])
    ids, freq = torch.unique(seqs[:, 1:], return_counts=True)
    ids = ids[torch.argsort(freq, descending=True, stable=True)].tolist()
    delims = tuple(i for i in ids if i not in (m.decoder.bos_idx, m.decoder.eos_idx, m.decoder.pad_idx))[:2]
    cfg = MeasureConfig(delimiters=delims, return_maps=True)
    s2, l2, m2, conf, rep = measured_inference(m, imgs, "cuda", max_inference_len=T, measures=cfg, prune=True)
    _same((s2, l2, m2), plain[:3])
    _same_confidence(conf, plain[3])
    grids = conf.alignment.grids
    assert grids == [(t.shape[-2] // P, t.shape[-1] // P) for t in imgs]
    dropped = [int((mp == 0).all(0).sum()) for mp in conf.alignment.maps]
    assert sum(dropped) > 0, "pruning dropped nothing: the test would show nothing"
    seg, count, _ = _check_report(rep, seqs, Ls, conf.log_prob, conf.entropy, conf.rank, conf.alignment.maps, grids, P, delims, m.decoder.eos_idx, 256,
                                  0.05, what="bf16 pruned")
    bounds = R.token_segments(seqs.cpu().numpy(), Ls, delims, m.decoder.eos_idx, 256)[2]
    assert int(count.sum()) >= 3
    assert rep.count.tolist() == count.tolist()
    for i, (h, w) in enumerate(grids):
        rg = [(int(a) - 1, int(b) - 1) for a, b in bounds[i, :count[i]]]
        want, mag = R.attn_map_segment_sum([conf.alignment.maps[i].cpu().double().numpy()], None, [rg])
        got = rep.maps[i].cpu().double().numpy()
        rows = np.array([b - a for a, b in rg], dtype=np.float64).reshape(-1, 1)
        assert got.shape == (count[i], h * w) and (np.abs(got - want[0]) <= rows * E24 * mag[0]).all()
        zero = (conf.alignment.maps[i] == 0).all(0).cpu().numpy()
        assert (got[:, zero] == 0).all()
        for mi in range(count[i]):      # the boxes are the extents of the full-grid maps the report itself holds (exactly the kernel's input)
            box = R.extent(got[mi], w, 0.05) * P
            err = np.abs(rep.box_px[i, mi].cpu().double().numpy() - box)
            a = [x[x > 0].min() for x in R.marginals(got[mi], w)]
            bar = 2.0 * h * w * E24 * got[mi].sum() / min(a) * P        # 2 S 2^-24 m / a_min: the general bound before its premise is used
            assert (err <= bar).all(), (i, mi, err, bar)
            assert 0 <= box[0] <= box[2] <= w * P and 0 <= box[1] <= box[3] <= h * P


# ---- 6. measure_accuracy -------------------------------------------------------------------------------------------------------------------
def test_measure_accuracy_against_the_reference(dev):
    import edit_alignment_reference as EA
    from acai_omr_amd import utils
    M, a, b, c = 3, 10, 11, 12
    pairs = [([0, M, a, b, M, c, 1], [0, M, a, b, M, c, 1]),          # perfect
             ([0, M, a, c, M, c, 1], [0, M, a, b, M, c, 1]),          # an error in one measure
             ([0, M, a, b, c, 1], [0, M, a, b, M, c, 1]),             # a missing delimiter
             ([0, M, a, M, b, M, c, 1], [0, M, a, b, M, c, 1]),       # an extra measure
             ([0, a, M, b], [0, c, M, b, M, a, a, M]),                # an error outside every measure; the end is missing
             ([0, 1], [0, 1]), ([5], [M])]                            # no measure at all; a lone delimiter that was missed
    rng = np.random.default_rng(8)
    for _ in range(6):
        t = rng.integers(3, 8, size=int(rng.integers(1, 90))).tolist()
        p = [int(rng.integers(3, 8)) if rng.random() < 0.15 else x for x in t if rng.random() > 0.1]
        pairs.append((p or [4], t))
    Lp = max(len(p) for p, _ in pairs)
    pred = torch.zeros(len(pairs), Lp, dtype=I64)
    pmask = torch.zeros(len(pairs), Lp, dtype=torch.bool)
    for i, (p, _) in enumerate(pairs):
        pred[i, :len(p)], pmask[i, :len(p)] = torch.tensor(p), True
    tg = [torch.tensor(t, dtype=I64) for _, t in pairs]
    acc, good, total = utils.measure_accuracy(pred.to(dev), pmask.to(dev), tg, [M])
    Lt = max(len(t) for _, t in pairs)
    tgt = np.zeros((len(pairs), Lt), dtype=np.int64)
    for i, (_, t) in enumerate(pairs):
        tgt[i, :len(t)] = t
    tl = [len(t) for _, t in pairs]
    al = EA.edit_alignments(pred.numpy(), [len(p) for p, _ in pairs], tgt, tl)
    tseg, tcount, _ = R.token_segments(tgt, tl, [M], -1, Lt)
    w_acc, w_good, w_total = R.measure_accuracy(tseg, tcount, *(np.asarray(x) for x in al[1:]))
    assert good.tolist() == w_good.tolist() and total.tolist() == w_total.tolist() and math.isclose(acc, w_acc, rel_tol=0, abs_tol=1e-15)
    assert good.tolist()[:7] == [2, 1, 1, 1, 1, 0, 0] and total.tolist()[:7] == [2, 2, 2, 2, 3, 0, 1]
    padded = torch.full((len(pairs), Lt), 99, dtype=I64)
    for i, t in enumerate(tg):
        padded[i, :len(t)] = t
    assert utils.measure_accuracy(pred.to(dev), pmask.to(dev), padded.to(dev), [M], pad_idx=99)[1].tolist() == w_good.tolist()
    acc0, good0, total0 = utils.measure_accuracy(pred.to(dev), pmask.to(dev), padded[:, :0].to(dev), [M], pad_idx=99)     # targets without a column
    assert math.isnan(acc0) and good0.tolist() == [0] * len(pairs) and total0.tolist() == [0] * len(pairs)
