"""Per-token confidence on the GPU: acai_token_confidence and acai_attn_map_weighted_sum against the float64 references of
tests/confidence_reference.py, the pass against the decode it scores, and its independence of every decode mode.

Tolerances.  Kernel 1: the integer outputs (rank, top ids) must match exactly - every comparison is on the raw fp32 logits.  For the float
outputs each case measures what a float32 torch CPU restatement of the same formula (log_softmax, -(p * logp).sum) loses against float64 on
the same inputs (`e32`) and allows the kernel MARGIN = 4 times max(e32, 2^-23 x max(1, max |log-prob| among the outputs)): the kernel's
reduction order differs from torch's, and one rounding per stage on top of that is the most it should cost.  -inf must be exactly -inf.
Kernel 2: every term is non-negative, so (T_i + 2) x 2^-23 x heat_ref[s] plus the float32 rounding of the result bounds a float32 sum in any
order.  The figures seen on an MI355X are in the docstrings of the tests."""
import math

import pytest
import torch
from torch.amp import autocast

import confidence_reference as R
from conftest import load_golden
from decode_support import _memory, _same, build_vitomr, dev  # noqa: F401

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
MARGIN = 4.0
EPS = 2.0 ** -23
INF = float("inf")
FILL, GUARD = 7.0, 97


# ---- kernel 1 ----------------------------------------------------------------------------------------------------------------------------
def _logits(N, V, scale, seed):
    """Normal logits at `scale`; every seventh column rounded (exact ties); with enough rows: row 1 all equal, row 2 with its maximum at the
    first and the last index, row 3 (row 0 of a short batch) with -inf entries next to finite ones, row 4 with a planted tie that `chosen`
    falls on.  chosen: 0, V - 1, V - 1 (the later of the tied maxima), a -inf entry, the later of the planted tie, then random."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, V, generator=g) * scale
    x[:, ::7] = torch.round(x[:, ::7])
    chosen = torch.randint(0, V, (N,), generator=g)
    chosen[0] = 0
    if N > 1:
        x[1] = x[1, 0]
        chosen[1] = V - 1
    if N > 2:
        x[2, 0] = x[2, V - 1] = float(x[2].max()) + 1.0
        chosen[2] = V - 1
    r = 3 if N > 3 else 0
    if V >= 4:
        dead = torch.rand(V, generator=g) < 0.2
        dead[[1, V - 2]] = True
        dead[0] = dead[V - 1] = False
        x[r, dead] = -INF
        if N > 3:
            chosen[3] = V - 2
    if N > 4 and V > 7:
        x[4, 7] = x[4, 0]
        chosen[4] = 7
    return x, chosen


K1_CASES = [(1, 5, 5, 1.0, 4.0), (3, 64, 5, 1.0, 4.0), (17, 65, 5, 1.0, 4.0), (40, 230, 5, 1.0, 4.0), (1000, 230, 5, 1.0, 4.0),
            (33, 1000, 5, 1.0, 4.0), (5, 4099, 5, 1.0, 4.0)]
K1_CASES += [(40, 230, K, tau, 4.0) for K in (1, 2, 8) for tau in (1.0, 0.5, 2.0)]
K1_CASES += [(40, 230, 5, 1.0, 30.0), (17, 65, 8, 2.0, 30.0), (5, 4099, 8, 0.5, 30.0)]


def _err(got, ref):
    """Largest |got - ref| over the finite reference entries; where the reference is -inf the result must be exactly -inf."""
    fin = torch.isfinite(ref)
    assert bool((got[~fin] == -INF).all()), "a -inf log-probability is not exactly -inf"
    assert bool(torch.isfinite(got[fin]).all())
    return float((got[fin].double() - ref[fin]).abs().max()) if bool(fin.any()) else 0.0


def _check_kernel1(got, x, chosen, K, tau, what):
    """got: the kernel's five outputs on the CPU.  Returns the largest err / tolerance."""
    lp, ent, rank, ids, tlp = got
    rlp, rent, rrank, rids, rtlp = R.token_confidence(x.double(), chosen, K, tau)
    flp, fent, _, fids, ftlp = R.token_confidence_f32(x, chosen, K, tau)
    assert torch.equal(fids, rids)
    assert rank.dtype == torch.int32 and ids.dtype == torch.int32 and lp.dtype == torch.float32
    assert torch.equal(rank.long(), rrank), (what, "rank")
    assert torch.equal(ids.long(), rids), (what, "top ids")
    outs = torch.cat([rlp, rtlp.reshape(-1)])
    big = max(1.0, float(outs[torch.isfinite(outs)].abs().max()))
    e32_lp = max(_err(flp, rlp), _err(ftlp, rtlp))
    e32_ent = _err(fent, rent)
    tol_lp, tol_ent = MARGIN * max(e32_lp, EPS * big), MARGIN * max(e32_ent, EPS * big)
    err_lp, err_ent = max(_err(lp, rlp), _err(tlp, rtlp)), _err(ent, rent)
    print(f"\nCONF {what}: log-prob e32={e32_lp:.2e} kernel err={err_lp:.2e} (x{err_lp / max(e32_lp, 1e-30):.2f}, {err_lp / tol_lp:.3f} of the "
          f"tolerance {tol_lp:.2e}); entropy e32={e32_ent:.2e} kernel err={err_ent:.2e} (x{err_ent / max(e32_ent, 1e-30):.2f}, "
          f"{err_ent / tol_ent:.3f} of the tolerance {tol_ent:.2e}); max |log-prob| {big:.1f}")
    assert err_lp <= tol_lp, (what, err_lp, tol_lp)
    assert err_ent <= tol_ent, (what, err_ent, tol_ent)
    return max(err_lp / tol_lp, err_ent / tol_ent)


@pytest.mark.parametrize("case", K1_CASES, ids=lambda c: f"N{c[0]}-V{c[1]}-K{c[2]}-tau{c[3]}-scale{c[4]:g}")
def test_token_confidence_against_float64(dev, case):
    """Both kernel forms (row in registers up to V = 256, re-read beyond) at V = 5 = K, 64, 65, 230, 1000, 4099, one and many workgroups,
    K in {1, 2, 5, 8}, temperature in {1, 0.5, 2}, logits at scale 4 and 30, planted ties, an all-equal row, a duplicated maximum, -inf
    entries with `chosen` on one of them.  Integers exact; floats within MARGIN x max(e32, 2^-23 max(1, max |log-prob|)); two launches give
    the same bits.
    Seen on an MI355X (e32 8.4e-8 .. 7.2e-6 for log-probabilities, 3.1e-8 .. 2.6e-6 for entropy): log-probability error 0.81 .. 1.18 x e32 (up
    to 7.2e-6 absolute at scale 30, |log-prob| up to 203), entropy error 0.13 .. 2.8 x e32 (up to 6.6e-7); at most 0.16 of the tolerance."""
    from acai_omr_amd import ops
    N, V, K, tau, scale = case
    x, chosen = _logits(N, V, scale, 100 * N + V)
    xd, cd = x.to(dev), chosen.to(dev)
    a = ops.token_confidence(xd, cd, K, tau)
    b = ops.token_confidence(xd, cd.to(torch.int32), K, tau)
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32)), "two launches differ"
    got = [t.cpu() for t in a]
    assert got[3].shape == (N, K) and got[4].shape == (N, K)
    _check_kernel1(got, x, chosen, K, tau, f"N={N} V={V} K={K} tau={tau} scale={scale:g}")
    if N > 3 and V >= 4:
        assert float(got[0][3]) == -INF and int(got[2][3]) >= 1     # chosen on a -inf entry
    if N > 2:
        assert got[3][1].tolist() == list(range(K)) and int(got[2][1]) == V - 1    # the all-equal row
        assert abs(float(got[1][1]) - math.log(V)) <= MARGIN * EPS * math.log(V)   # se = V exactly; its logarithm, a few ulp
        assert int(got[3][2, 0]) == 0 and int(got[2][2]) == 1                      # the duplicated maximum: first index wins
        if K > 1:
            assert int(got[3][2, 1]) == V - 1


def test_token_confidence_refuses_bad_arguments(dev):
    """Every refusal is raised on the host before any launch; N = 0 gives empty tensors."""
    from acai_omr_amd import ops
    x = torch.randn(6, 10, device=dev)
    c = torch.zeros(6, dtype=torch.long, device=dev)
    for bad in (torch.tensor([0, 0, 0, 0, 0, 10]), torch.tensor([0, -1, 0, 0, 0, 0])):
        with pytest.raises(ValueError, match="outside"):
            ops.token_confidence(x, bad.to(dev))
    for kw in (dict(top_k=0), dict(top_k=9), dict(top_k=2.0), dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan"))):
        with pytest.raises(ValueError):
            ops.token_confidence(x, c, **kw)
    with pytest.raises(ValueError, match="top_k"):
        ops.token_confidence(x[:, :3].contiguous(), c, top_k=4)      # K > V
    with pytest.raises(ValueError, match="contiguous"):
        ops.token_confidence(torch.randn(6, 20, device=dev)[:, :10], c)
    with pytest.raises(ValueError, match="float32"):
        ops.token_confidence(x.to(BF), c)
    with pytest.raises(ValueError, match="chosen"):
        ops.token_confidence(x, c[:5])
    with pytest.raises(ValueError, match="chosen"):
        ops.token_confidence(x, c.float())
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.token_confidence(x, c.cpu())
    out = ops.token_confidence(x[:0], c[:0], 3)
    assert [tuple(t.shape) for t in out] == [(0,), (0,), (0,), (0, 3), (0, 3)]
    from acai_omr_amd import _lib
    L = _lib.lib()
    p = x.data_ptr()
    assert L.acai_token_confidence(p, c.data_ptr(), 6, 10, 11, 1.0, p, p, p, p, p, None) != 0 and b"top_k" in L.acai_last_error()
    assert L.acai_token_confidence(p, c.data_ptr(), 6, 10, 2, 0.0, p, p, p, p, p, None) != 0 and b"temperature" in L.acai_last_error()
    assert L.acai_token_confidence(None, c.data_ptr(), 6, 10, 2, 1.0, p, p, p, p, p, None) != 0 and b"null" in L.acai_last_error()


# ---- kernel 2 ----------------------------------------------------------------------------------------------------------------------------
K2_BATCHES = [[(1, 1000), (300, 63), (3, 257), (130, 1)], [(300, 1000), (1, 1), (130, 63), (3, 257), (130, 1000)], [(3, 63)], [(300, 257)]]


@pytest.mark.parametrize("shapes", K2_BATCHES, ids=lambda b: "_".join(f"{t}x{s}" for t, s in b))
def test_weighted_sum_against_float64(dev, shapes):
    """Ragged batches with T_i in {1, 3, 130, 300} (one split, and up to ten with a ragged last one) and S_i in {1, 63, 257, 1000} mixed in
    one call, 7.0-filled guard margins around the blocks, every image's weights at another scale (1, 1e3, 1e-3) and, in the batches of
    several, image 1's all zero.  Per entry within (T_i + 2) 2^-23 heat_ref[s] + the float32 rounding; the sums within the summed
    bound; two launches the same bits; the zero-weight image exact zeros.
    Seen on an MI355X: per entry at most 0.20 of the bound, the sums at most 0.005 of theirs."""
    from acai_omr_amd import engine, ops
    g = torch.Generator().manual_seed(31 + len(shapes) + shapes[0][0])
    lens_q, lens_k = [t for t, _ in shapes], [s for _, s in shapes]
    maps, ws = [], []
    for i, (t, s) in enumerate(shapes):
        m = torch.rand(t, s, generator=g, dtype=torch.float64) ** 3 + 1e-3
        maps.append((m / m.sum(-1, keepdim=True)).float())
        w = torch.rand(t, generator=g) * (1.0, 1e3, 1e-3)[i % 3]
        if i == 1:
            w.zero_()
        ws.append(w)
    offs, total = ops.attn_map_layout(lens_q, lens_k, guard=GUARD)
    flat = torch.full((total,), FILL)
    for o, m in zip(offs, maps):
        flat[o:o + m.numel()] = m.reshape(-1)
    args = (flat.to(dev), torch.tensor(offs, device=dev), engine.cu_from_lens(lens_q, dev), engine.cu_from_lens(lens_k, dev),
            torch.cat(ws).to(dev), max(lens_q))
    a = ops.attn_map_weighted_sum(*args)
    b = ops.attn_map_weighted_sum(*args)
    torch.cuda.synchronize()
    assert a.shape == (sum(lens_k),) and a.dtype == torch.float32
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "two launches differ"
    c = ops.attn_map_weighted_sum(*args, layout=(lens_q, lens_k, offs))   # the layout from the host instead of read back: the same launches
    assert torch.equal(a.view(torch.int32), c.view(torch.int32))
    with pytest.raises(ValueError, match="layout"):
        ops.attn_map_weighted_sum(*args, layout=(lens_q, lens_k, offs[:-1]))
    ref = R.weighted_sum([m.double() for m in maps], [w.double() for w in ws])
    got, o, worst, worst_sum = a.cpu().double(), 0, 0.0, 0.0
    for i, ((t, s), rf, w) in enumerate(zip(shapes, ref, ws)):
        h = got[o:o + s]
        tol = ((t + 2) * EPS + 2.0 ** -24) * rf
        if float(w.abs().max()) == 0.0:
            assert bool((h == 0).all()), "the zero-weight image is not exactly zero"
        else:
            worst = max(worst, float(((h - rf).abs() / tol).max()))
            assert bool(((h - rf).abs() <= tol).all()), (i, t, s, float(((h - rf).abs() / tol).max()))
            sum_tol = s * float(tol.max())
            d = abs(float(h.sum()) - float(w.double().sum()))
            worst_sum = max(worst_sum, d / sum_tol)
            assert d <= sum_tol, (i, t, s, d, sum_tol)
        o += s
    print(f"\nWSUM {shapes}: worst err/tolerance per entry {worst:.3f}, of the sums {worst_sum:.3f}")
    if len(shapes) > 1:
        with pytest.raises(ValueError, match="weights"):
            ops.attn_map_weighted_sum(args[0], args[1], args[2], args[3], args[4][:-1].contiguous(), args[5])
        with pytest.raises(ValueError, match="max_q"):
            ops.attn_map_weighted_sum(*args[:5], max(lens_q) - 1)
        with pytest.raises(ValueError, match="outside"):
            ops.attn_map_weighted_sum(args[0][:-(GUARD + 1)].contiguous(), *args[1:])


# ---- the pass ----------------------------------------------------------------------------------------------------------------------------
_DECODED = {}


def _decoded(dev, name, bf16, memory_cache_dtype=None, max_batch=12):
    """(fixture, model, memory, mask, greedy seqs, log_probs, seq_mask), built and decoded once per module."""
    key = (name, bf16, memory_cache_dtype)
    if key not in _DECODED:
        fx = load_golden(name)
        m = build_vitomr(fx["cfg"], fx["state_dict"], dev, BF if bf16 else torch.float, max_batch, memory_cache_dtype=memory_cache_dtype)
        mem, mask = _memory(m, fx["imgs"], bf16)
        with torch.no_grad(), autocast(device_type="cuda", dtype=BF, enabled=bf16):
            seqs, lps, smask = m.cached_greedy_generate(mem, mask, max_len=fx["cfg"]["gen_len"])
        _DECODED[key] = (fx, m, mem, mask, seqs, lps, smask)
    return _DECODED[key]


def _ctx(bf16):
    return autocast(device_type="cuda", dtype=BF, enabled=bf16)


def _scored(m, seqs, smask):
    Ls = m._alignment_lengths(seqs, smask)
    has = torch.zeros(seqs.shape, dtype=torch.bool)
    for i, L in enumerate(Ls):
        has[i, 1:L] = True
    return Ls, has


def _grids(fx):
    P = fx["cfg"]["P"]
    return [(int(t.shape[-2]) // P, int(t.shape[-1]) // P) for t in fx["imgs"]]


def _unscored_is_blank(conf, has):
    lp, ent, rank, ids, tlp = (t.cpu() for t in (conf.log_prob, conf.entropy, conf.rank, conf.top_tokens, conf.top_log_probs))
    assert rank.dtype == torch.int64 and ids.dtype == torch.int64 and lp.dtype == torch.float32 and lp.shape == has.shape
    assert torch.equal(~torch.isnan(lp), has) and torch.equal(~torch.isnan(ent), has) and torch.equal(~torch.isnan(tlp).any(-1), has)
    assert torch.equal(rank >= 0, has) and bool((rank[~has] == -1).all())
    assert torch.equal((ids >= 0).all(-1), has) and bool((ids[~has] == -1).all())
    return lp, ent, rank, ids, tlp


def _against_reference(conf, logits, seqs, Ls, has, K, what, tau=1.0):
    """conf's scored entries against kernel 1's reference on the packed logits they were computed from."""
    chosen = torch.cat([seqs[i, 1:L] for i, L in enumerate(Ls)]).cpu()
    got = [t.cpu()[has] for t in (conf.log_prob, conf.entropy, conf.rank, conf.top_tokens, conf.top_log_probs)]
    got[2], got[3] = got[2].to(torch.int32), got[3].to(torch.int32)
    return _check_kernel1(got, logits.float().cpu(), chosen, K, tau, what)


@pytest.mark.parametrize("name", ["vitomr_small", "vitomr_dh64", "vitomr_odd"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_the_pass_scores_the_decodes_own_choices(dev, name, bf16):
    """Greedy decode, then token_confidence: every scored token is the arg-max (rank 0, top_tokens[..., 0] == seqs) with the decode's
    log-probability (1e-4 in fp32, 0.07 in bf16: the project's bars); NaN / -1 exactly where nothing is scored; entropy, rank and top-k
    equal kernel 1's reference on the pass's own logits, for the logits-only pass and for the combined pass of uncertainty_maps; the heat
    maps equal the float64 weighted sum of cross_attention_maps' maps within kernel 2's bound; with return_alignment the TokenAlignment is
    locate_tokens' bit for bit; a caller's weight tensor is honoured (NaN at the entries that are not scored); temperature 2 moves
    log_prob and leaves rank and top_tokens alone.
    Seen on an MI355X: log_prob within 9.5e-7 .. 2.0e-6 (fp32) / 2.4e-2 .. 3.0e-2 (bf16) of the decode's; against the reference on the pass's
    own logits log-probabilities 0.68 .. 3.8 x e32 (at most 4.5e-7), entropy 0.34 .. 0.77 x e32 (at most 7.3e-7), at most 0.26 of the tolerance; heat maps at
    most 0.10 of kernel 2's bound."""
    from acai_omr_amd import engine
    fx, m, mem, mask, seqs, lps, smask = _decoded(dev, name, bf16)
    Ls, has = _scored(m, seqs, smask)
    bar = 0.07 if bf16 else 1e-4
    K = 5
    with torch.no_grad(), _ctx(bf16):
        conf = m.token_confidence(mem, mask, seqs, smask)
        warm = m.token_confidence(mem, mask, seqs, smask, temperature=2.0)
    lp, ent, rank, ids, tlp = _unscored_is_blank(conf, has)
    assert bool((rank[has] == 0).all()) and torch.equal(ids[..., 0][has], seqs.cpu()[has])
    d = float((lp[has] - lps.cpu()[has]).abs().max())
    print(f"\n{name} {'bf16' if bf16 else 'fp32'}: max |log_prob - decode's log_probs| = {d:.2e} (bar {bar})")
    assert d < bar
    mean = conf.mean_log_prob.cpu()
    for i, L in enumerate(Ls):
        assert abs(float(mean[i]) - float(lps[i, 1:L].sum()) / (L - 1)) < bar
    assert torch.equal(conf.margin.cpu()[has], (tlp[..., 0] - tlp[..., 1])[has]) and bool((conf.margin.cpu()[has] >= 0).all())
    # the logits-only pass against the reference on its own logits
    tokens = torch.cat([seqs[i, :L - 1] for i, L in enumerate(Ls)])
    lens_t = [L - 1 for L in Ls]
    with torch.no_grad(), _ctx(bf16):
        mem32, lens_s = engine.unpad_rows(mem, mask)
        logits = m.decoder.logits_packed(tokens, lens_t, mem32, None, lens_s, position_offset=1)
        maps, logits_c = m.decoder.cross_attention_maps_packed(tokens, lens_t, mem32, None, lens_s, position_offset=1, return_logits=True)
    _against_reference(conf, logits, seqs, Ls, has, K, f"{name} logits-only pass")
    _against_reference(warm, logits, seqs, Ls, has, K, f"{name} logits-only pass, temperature 2", tau=2.0)
    wlp = warm.log_prob.cpu()
    assert torch.equal(warm.rank.cpu(), rank) and torch.equal(warm.top_tokens.cpu(), ids)
    assert float((wlp[has] - lp[has]).abs().max()) > 1e-3
    # the combined pass
    grids = _grids(fx)
    custom = torch.full(seqs.shape, float("nan"))
    custom[has] = torch.rand(int(has.sum()), generator=torch.Generator().manual_seed(9))
    with torch.no_grad(), _ctx(bf16):
        un = m.uncertainty_maps(mem, mask, seqs, smask, grids=grids, return_alignment=True)
        plain = m.uncertainty_maps(mem, mask, seqs, smask, weight="surprisal", grids=grids)
        err = m.uncertainty_maps(mem, mask, seqs, smask, weight="error", grids=grids)
        own = m.uncertainty_maps(mem, mask, seqs, smask, weight=custom, grids=grids)
        api_maps = m.cross_attention_maps(mem, mask, seqs, smask)
        loc = m.locate_tokens(mem, mask, seqs, smask, grids=grids)
    _unscored_is_blank(un, has)
    _against_reference(un, logits_c, seqs, Ls, has, K, f"{name} combined pass")
    for a, b in zip(api_maps, maps):
        assert torch.equal(a, b)
    assert plain.alignment is None and un.alignment is not None and un.alignment.maps is None and un.alignment.grids == loc.grids
    for f in ("patch", "center_px", "spread_px", "peak"):
        a, b = getattr(un.alignment, f).cpu(), getattr(loc, f).cpu()
        assert a.dtype == b.dtype and torch.equal(torch.nan_to_num(a.double(), nan=-5.0), torch.nan_to_num(b.double(), nan=-5.0)), f
    worst = 0.0
    for res, wname in ((un, "entropy"), (plain, "surprisal"), (err, "error"), (own, None)):
        for i, (L, (h, w)) in enumerate(zip(Ls, grids)):
            if wname is None:
                wt = custom[i, 1:L].double()
            else:
                wt = R.weight_of(wname, res.log_prob[i, 1:L].cpu().double(), res.entropy[i, 1:L].cpu().double())
            rf = R.weighted_sum([api_maps[i].cpu().double()], [wt])[0]
            heat = res.uncertainty[i].cpu()
            assert heat.shape == (h, w) and heat.dtype == torch.float32
            tol = ((L - 1 + 2) * EPS + 2.0 ** -24) * rf + 1e-30   # kernel 2's bound (entropy, -log_prob and the caller's weights are exact)
            if wname == "error":   # 1 - exp(log_prob) is formed in float32 on the device: exp and the difference round, 2^-23 per weight
                tol = tol + EPS * api_maps[i].cpu().double().sum(0)
            e = float(((heat.double().reshape(-1) - rf).abs() / tol).max())
            worst = max(worst, e)
            assert e <= 1.0, (wname, i, e)
    print(f"{name}: heat maps, worst err/tolerance {worst:.3f}")
    assert not torch.equal(own.uncertainty[0], un.uncertainty[0])


def test_a_decode_after_the_pass_is_the_decode_before_it(dev):
    """greedy decode, token_confidence and uncertainty_maps, greedy decode: bitwise the same, with and without the FP8 memory cache; and
    the pass reads the memory, not the caches: both models give the same confidence bit for bit."""
    res = []
    first = _decoded(dev, "vitomr_small", True)
    for mcd in (None, torch.float8_e4m3fn):
        fx, m, mem, mask, seqs, lps, smask = _decoded(dev, "vitomr_small", True, memory_cache_dtype=mcd)
        assert torch.equal(mem, first[2])
        with torch.no_grad(), _ctx(True):
            m.token_confidence(mem, mask, seqs, smask)
            m.uncertainty_maps(mem, mask, seqs, smask, grids=_grids(fx))
            again = m.cached_greedy_generate(mem, mask, max_len=fx["cfg"]["gen_len"])
            res.append(m.token_confidence(mem, mask, first[4], first[6]))   # the bf16-cache model's tokens, scored by both models
        _same(again, (seqs, lps, smask))
    for f in ("log_prob", "entropy", "rank", "top_tokens", "top_log_probs"):
        x, y = getattr(res[0], f), getattr(res[1], f)
        assert torch.equal(torch.nan_to_num(x.double(), nan=-5.0), torch.nan_to_num(y.double(), nan=-5.0)), f


def _forbidding_grammar(m, plain):
    """One state that allows every token but <bos>, <pad> and the token greedy put first in row 0: the constraint binds at index 1."""
    from acai_omr_amd.grammar import TokenAutomaton
    dec = m.decoder
    nxt = torch.zeros(1, dec.vocab_size, dtype=torch.long)
    nxt[0, [dec.bos_idx, dec.pad_idx, int(plain[0][0, 1])]] = -1
    return TokenAutomaton.from_transitions(nxt, 0, pad_idx=dec.pad_idx, bos_idx=dec.bos_idx, eos_idx=dec.eos_idx)


@pytest.mark.parametrize("mode", ["greedy", "beam2", "speculative2", "grammar"])
def test_confident_inference_decodes_as_inference_does(dev, mode):
    """Tokens, log-probs and mask are inference()'s; the scores follow the decode's log_probs within the bars (beam: some rank may exceed
    0; grammar: the unconstrained model's log_prob <= the renormalised log_probs + bar, and the forced token has rank > 0); with
    uncertainty="entropy" the heat maps and the alignment are filled."""
    from acai_omr_amd.inference.vitomr_inference import aligned_inference, confident_inference, inference
    fx, m, *_ = _decoded(dev, "vitomr_small", True)
    n = fx["cfg"]["gen_len"]
    kw = {"greedy": {}, "beam2": {"beam_width": 2}, "speculative2": {"speculative": 2}}.get(mode)
    if kw is None:
        kw = {"grammar": _forbidding_grammar(m, inference(m, fx["imgs"], "cuda", max_inference_len=n))}
    plain = inference(m, fx["imgs"], "cuda", max_inference_len=n, **kw)
    seqs, lps, mask, conf = confident_inference(m, fx["imgs"], "cuda", max_inference_len=n, **kw)
    _same((seqs, lps, mask), plain)
    assert conf.uncertainty is None and conf.alignment is None
    Ls, has = _scored(m, seqs, mask)
    lp, ent, rank, ids, tlp = _unscored_is_blank(conf, has)
    d = lp[has] - lps.cpu()[has]
    print(f"\n{mode}: log_prob - log_probs in [{float(d.min()):.2e}, {float(d.max()):.2e}], largest rank {int(rank.max())}")
    if mode == "grammar":
        assert float(d.max()) <= 0.07
        assert int(rank[0, 1]) >= 1 and int(seqs[0, 1]) != int(ids[0, 1, 0])
    else:
        assert float(d.abs().max()) < 0.07
    if mode in ("greedy", "speculative2"):
        assert bool((rank[has] == 0).all())
    full = confident_inference(m, fx["imgs"], "cuda", max_inference_len=n, uncertainty="entropy", top_k=3, **kw)
    _same(full[:3], plain)
    c3 = full[3]
    assert c3.top_tokens.shape == seqs.shape + (3,) and torch.equal(~torch.isnan(c3.log_prob.cpu()), has)
    if mode in ("greedy", "speculative2"):
        assert bool((c3.rank.cpu()[has] == 0).all())
    assert [tuple(u.shape) for u in c3.uncertainty] == _grids(fx) and c3.alignment.grids == _grids(fx)
    al = aligned_inference(m, fx["imgs"], "cuda", max_inference_len=n, **kw)[3]
    assert torch.equal(c3.alignment.patch, al.patch)
    for i, L in enumerate(Ls):   # the maps' rows sum to 1: the heat map's sum is the sum of the weights
        s, want = float(c3.uncertainty[i].double().sum()), float(c3.entropy[i, 1:L].double().sum())
        assert abs(s - want) <= 0.02 * max(want, 1e-3), (i, s, want)   # (bf16 map rows sum to 1 within 2e-2: tests/test_gpu_alignment.py)
    _same(inference(m, fx["imgs"], "cuda", max_inference_len=n, **kw), plain)
