"""Token-to-image alignment on the GPU: acai_attn_probs_mean and acai_attn_map_locate at every dispatch edge against float64 references
(tests/alignment_reference.py), the decoder pass against the decode it explains, and its independence of every decode mode.

Tolerances.  Each comparison measures, on its own inputs, what a float32 torch restatement of the same formula loses against float64
(`e32`) and allows the kernel MARGIN times that, never more than 1e-3 absolute on a probability (beyond that the probe no longer separates
a defect from rounding: with queries randn / 2 and keys 4 randn the scores spread over ~2 nats, and a key read from the neighbouring
sequence or a dropped last key moves its own map entry by its whole value, 1e-3 .. 1 here).  The kernel is allowed more than the restatement
because it exponentiates score * log2(e) / sqrt(dh) - lse directly: the argument is up to ~2^4 where softmax's max-subtracted one is ~1, so
its float32 rounding is ~2^4 times coarser, and lse itself carries the forward kernel's rounding.  e32 is floored at one float32 ulp of the
weights' sum.  The figures seen on an MI355X are in the docstrings of the tests."""
import pytest
import torch
from torch.amp import autocast

import alignment_reference as R
from conftest import load_golden
from decode_support import _memory, _same, build_vitomr, dev  # noqa: F401

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
FILL, GUARD = 7.0, 97
CAP = 1e-3
MARGIN = 32.0          # kernel / float32-restatement error allowed (see the module docstring and test_probs_mean_edges)
# bf16 operands: the forward kernel's log-sum-exp is that of its bf16-ROUNDED probabilities (attn_varlen.hip, MFSUM: the sum of exactly what
# multiplies V), so it carries up to one bf16 unit roundoff, 2^-8 relative, and every entry of the row inherits it: an entry p may be off by
# MARGIN e32 + REL_BF16 p.  The probe's head weights sum to 1/4, so that this stays below CAP for every entry and every row sum (2^-8 / 4 =
# 9.8e-4) and the 1e-3 cap keeps its meaning for bf16 too.
REL_BF16 = 2.0 ** -8
MARGIN_LOCATE = 16.0
CAP_BF16 = 2e-2        # model level, bf16: a few bf16 unit roundoffs (2^-8) of a probability near 1


def _tol(e32, wsum, margin=MARGIN, cap=CAP):
    return min(cap, margin * max(e32, 2.0 ** -23 * wsum))


# (H, dh, dtype, query lengths, key lengths, q layout, accumulate): every query length of {1, 15, 17, 64, 65, 130} and key length of
# {1, 63, 64, 65, 127, 129, 257} occurs with each kernel form; neighbours in a batch are unequal.
CASES = [
    (16, 64, BF, (1, 65, 130), (257, 1, 127), "aligned", False),
    (3, 32, BF, (15, 17, 64), (63, 64, 65), "aligned", True),
    (1, 64, BF, (130, 1, 17), (129, 257, 1), "aligned", False),
    (16, 32, BF, (64, 65, 15), (65, 129, 63), "aligned", True),
    (3, 64, BF, (17, 130, 1), (64, 63, 257), "aligned", True),
    (3, 8, F32, (1, 15, 17), (1, 63, 64), "aligned", False),
    (16, 24, F32, (64, 65, 130), (65, 127, 129), "aligned", True),
    (1, 64, F32, (17, 130, 1), (257, 1, 65), "aligned", False),
    (3, 24, BF, (15, 64, 65), (127, 129, 257), "aligned", False),
    (3, 64, BF, (17, 65, 1), (64, 63, 257), "unaligned", False),
    (16, 32, BF, (130, 15, 64), (1, 257, 127), "unaligned", True),
]


def _case_id(c):
    H, dh, dt, lq, lk, layout, acc = c
    return f"H{H}-dh{dh}-{'bf16' if dt == BF else 'fp32'}-q{'_'.join(map(str, lq))}-k{'_'.join(map(str, lk))}-{layout}{'-acc' if acc else ''}"


def _inputs(case):
    H, dh, dtype, lens_q, lens_k, layout, acc = case
    E = H * dh
    g = torch.Generator().manual_seed(1000 * H + dh + sum(lens_q) + 7 * sum(lens_k))
    q = (torch.randn(sum(lens_q), E, generator=g) / 2).to(dtype)
    kv = torch.cat([torch.randn(sum(lens_k), E, generator=g) * 4, torch.randn(sum(lens_k), E, generator=g)], 1).to(dtype)
    w = torch.rand(H, generator=g) + 0.1
    if H >= 3:
        w[1] = 0.0
    w = w * (0.25 / float(w.sum()))   # (not 1: the rows must sum to whatever the weights sum to; why 1/4: REL_BF16)
    before = torch.rand(sum(a * b for a, b in zip(lens_q, lens_k)), generator=g) if acc else None
    return q, kv, w, before


def _run_probs(dev, case, layout=None):
    """The kernel's whole output buffer (guards included) on the CPU, and the offsets of the blocks."""
    from acai_omr_amd import engine, ops
    H, dh, dtype, lens_q, lens_k, lay, acc = case
    layout = layout or lay
    E = H * dh
    q, kv, w, before = _inputs(case)
    if layout == "unaligned":   # rows start 2 bytes past a 16-byte boundary and their pitch is odd
        base = torch.zeros(q.shape[0], E + 3, dtype=dtype, device=dev)
        qd = base[:, 1:1 + E]
        qd.copy_(q)
        assert qd.data_ptr() % 16 != 0
    else:
        qd = q.to(dev)
    kvd = kv.to(dev)
    kd, vd = kvd[:, :E], kvd[:, E:]
    cu_q, cu_k = engine.cu_from_lens(lens_q, dev), engine.cu_from_lens(lens_k, dev)
    lse = torch.empty(H * q.shape[0], device=dev)
    ops.attn_varlen(qd, kd, vd, cu_q, cu_k, H, dh, max(lens_q), lse=lse)
    offs, total = ops.attn_map_layout(lens_q, lens_k, guard=GUARD)
    out = torch.full((total,), FILL, device=dev)
    if acc:
        o = 0
        for off, a, b in zip(offs, lens_q, lens_k):
            out[off:off + a * b] = before[o:o + a * b].to(dev)
            o += a * b
    got = ops.attn_probs_mean(qd, kd, cu_q, cu_k, H, dh, max(lens_q), max(lens_k), lse, w.to(dev), torch.tensor(offs, device=dev), out,
                              accumulate=acc)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    return out.cpu(), offs


def _check_probs(case, whole, offs):
    H, dh, dtype, lens_q, lens_k, _, acc = case
    q, kv, w, before = _inputs(case)
    E = H * dh
    ref = R.probs_mean(q.double(), kv[:, :E].double(), lens_q, lens_k, H, dh, w.double())
    r32 = R.probs_mean(q.float(), kv[:, :E].float(), lens_q, lens_k, H, dh, w)
    e32 = max(float((a.double() - b).abs().max()) for a, b in zip(r32, ref))
    wsum = float(w.double().sum())
    tol = _tol(e32, wsum)
    rel = REL_BF16 if dtype == BF else 0.0
    inside = torch.zeros(whole.numel(), dtype=torch.bool)
    err = rows = worst = relerr = 0.0
    o = 0
    for off, a, b, rf in zip(offs, lens_q, lens_k, ref):
        inside[off:off + a * b] = True
        got = whole[off:off + a * b].double().view(a, b)
        if acc:
            got = got - before[o:o + a * b].double().view(a, b)
            o += a * b
        d = (got - rf).abs()
        err = max(err, float(d.max()))
        relerr = max(relerr, float((d / rf.clamp_min(1e-3)).max()))
        worst = max(worst, float((d / torch.clamp(tol + rel * rf, max=CAP)).max()))
        rows = max(rows, float((got.sum(-1) - wsum).abs().max()))
    # (accumulate: the float32 sum with the buffer's old value, up to 1 + wsum, adds half an ulp of it)
    slack = 2.0 ** -23 * (1.0 + wsum) if acc else 0.0
    row_tol = min(CAP, tol + rel * wsum) + 4 * slack + 257 * 2.0 ** -24 * wsum   # (+ up to 257 float32 roundings of the entries)
    print(f"\nPROBS {_case_id(case)}: e32={e32:.2e} tol={tol:.2e} kernel err={err:.2e} (x{err / max(e32, 1e-30):.1f}, relative {relerr:.2e}) "
          f"worst err/tolerance={worst:.3f} row sums off by {rows:.2e} (tolerance {row_tol:.2e})")
    assert bool(torch.isfinite(whole).all())
    assert bool((whole[~inside] == FILL).all()), "a guard element was written"
    assert worst <= 1.0 + slack / tol, (worst, err, tol)
    assert rows <= row_tol, (rows, row_tol)
    return err, tol


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_probs_mean_edges(dev, case):
    """Both kernel forms on ragged batches of three, k as the [:, :E] view of a [Mk, 2E] tensor, non-uniform head weights with a zero,
    writing and accumulating, 7.0-filled guard margins before, between and after the blocks.
    Seen on an MI355X (e32 = the float32 torch restatement's error, 6e-9 .. 1e-7 here): fp32 operands - kernel error 2.8 .. 5.9 x e32
    (5.9e-8 .. 2.8e-7), row sums off by at most 5.2e-7; bf16 operands - error up to 2.0e-4 absolute and 2.2e-3 relative (that is 460 ..
    8400 x e32: the forward's log-sum-exp of bf16-rounded probabilities, REL_BF16), at most 0.55 of the tolerance, row sums off by at most
    4.0e-4.  MARGIN = 32 was set from the fp32 figures: the exponent's argument is ~2^4 coarser than softmax's, times two."""
    whole, offs = _run_probs(dev, case)
    _check_probs(case, whole, offs)


def test_unaligned_q_takes_the_fallback_and_agrees(dev):
    """The same values through an unaligned q view (plain FMA form) and an aligned one (matrix cores): both within tolerance of the
    reference, hence within two tolerances of each other."""
    case = CASES[9]
    a, offs = _run_probs(dev, case, "unaligned")
    b, _ = _run_probs(dev, case, "aligned")
    _, tol = _check_probs(case, a, offs)
    _check_probs(case, b, offs)
    d = float((a.double() - b.double()).abs().max())
    print(f"\nfallback vs matrix cores: max difference {d:.2e} (tolerance {tol:.2e})")
    assert d <= 2 * tol   # (both read the same lse: its rounding cancels between them)


def test_probs_mean_is_deterministic_and_refuses_bad_arguments(dev):
    from acai_omr_amd import _lib
    a, _ = _run_probs(dev, CASES[0])
    b, _ = _run_probs(dev, CASES[0])
    assert torch.equal(a, b)
    L = _lib.lib()
    x = torch.zeros(64, device=dev)
    i32, i64 = torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    p = x.data_ptr()
    good = dict(q=p, ldq=8, k=p, ldk=8, cu_q=i32.data_ptr(), cu_k=i32.data_ptr(), B=1, H=1, dh=8, max_q=1, max_k=1, dtype=0, lse=p, total_q=1,
                head_w=p, map_off=i64.data_ptr(), out=p, accumulate=0, stream=None)
    for bad in (dict(q=None), dict(out=None), dict(lse=None), dict(dh=65, ldq=65, ldk=65), dict(H=0), dict(dtype=7)):
        args = dict(good, **bad)
        assert L.acai_attn_probs_mean(*args.values()) != 0, bad
        assert b"acai_attn_probs_mean" in L.acai_last_error()
    gw = (__import__("ctypes").c_int32 * 1)(0)
    assert L.acai_attn_map_locate(p, i64.data_ptr(), i32.data_ptr(), i32.data_ptr(), gw, 1, 1, i32.data_ptr(), p, None) != 0
    assert b"grid_w" in L.acai_last_error()


# ---- locate ----------------------------------------------------------------------------------------------------------------------------
def test_locate_against_the_reference(dev):
    """Widths 1, 7 and 64 with S = h w up to 257 x 1, planted exact ties (the lower index wins), an all-zero row.  Patch indices equal;
    moments within MARGIN_LOCATE times what float32 torch loses on the same maps, relative to the grid's sides.
    Seen on an MI355X: float32 torch 7.2e-8 .. 1.4e-7, the kernel 5.0e-8 .. 6.8e-8 (it sums the second moments around the centroid)."""
    from acai_omr_amd import engine, ops
    g = torch.Generator().manual_seed(5)
    shapes = [(5, 257, 1), (4, 9, 7), (6, 3, 64)]   # (rows, h, w)
    maps = []
    for T, h, w in shapes:
        m = torch.rand(T, h * w, generator=g) ** 6
        m = m / m.sum(-1, keepdim=True)
        m[1] = 0.0                                     # a dead row
        m[2, [h * w - 1, 3]] = float(m[2].max()) * 2   # an exact tie, the later one first in no order the kernel walks
        m[3] = 1.0 / (h * w)                           # every patch ties
        maps.append(m)
    lens_q, lens_k = [s[0] for s in shapes], [s[1] * s[2] for s in shapes]
    offs, total = ops.attn_map_layout(lens_q, lens_k, guard=GUARD)
    flat = torch.full((total,), FILL)
    for o, m in zip(offs, maps):
        flat[o:o + m.numel()] = m.reshape(-1)
    patch, loc = ops.attn_map_locate(flat.to(dev), torch.tensor(offs, device=dev), engine.cu_from_lens(lens_q, dev), engine.cu_from_lens(lens_k, dev),
                                     [s[2] for s in shapes], max(lens_q), sum(lens_q))
    patch, loc = patch.cpu(), loc.cpu().double()
    o = 0
    for (T, h, w), m in zip(shapes, maps):
        rp, rl = R.locate(m.double(), w)
        _, l32 = R.locate(m, w)
        scale = torch.tensor([1.0, 1.0, w, h, w, h], dtype=torch.float64)     # the moments are in patch units: compare relative to the grid
        e32 = float(((l32.double() - rl).abs() / scale).max())
        err = float(((loc[o:o + T] - rl).abs() / scale).max())
        tol = MARGIN_LOCATE * max(e32, 2.0 ** -23)
        print(f"\nLOCATE {h}x{w}: e32={e32:.2e} kernel err={err:.2e} tol={tol:.2e}")
        assert torch.equal(patch[o:o + T].long(), rp), (patch[o:o + T], rp)
        assert int(patch[o + 1]) == 0 and float(loc[o + 1].abs().max()) == 0.0
        assert int(patch[o + 2]) == 3 and int(patch[o + 3]) == 0
        assert err <= tol, (err, tol)
        o += T
    with pytest.raises(RuntimeError, match="grid_w"):
        ops.attn_map_locate(flat.to(dev), torch.tensor(offs, device=dev), engine.cu_from_lens(lens_q, dev), engine.cu_from_lens(lens_k, dev), [1, 0, 64],
                            max(lens_q), sum(lens_q))


# ---- the decoder pass --------------------------------------------------------------------------------------------------------------------
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


def _packed_pass(m, mem, mask, seqs, smask, bf16, **kw):
    from acai_omr_amd import engine
    Ls = m._alignment_lengths(seqs, smask)
    tokens = torch.cat([seqs[i, :L - 1] for i, L in enumerate(Ls)])
    lens_t = [L - 1 for L in Ls]
    with torch.no_grad(), autocast(device_type="cuda", dtype=BF, enabled=bf16):
        mem32, lens_s = engine.unpad_rows(mem, mask)
        res = m.decoder.cross_attention_maps_packed(tokens, lens_t, mem32, None, lens_s, **kw)
    return Ls, tokens, lens_t, mem32, lens_s, res


def _f64(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


@pytest.mark.parametrize("name", ["vitomr_small", "vitomr_dh64", "vitomr_odd"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_the_map_is_the_decodes_own_attention(dev, name, bf16):
    """Greedy decode, then the pass with position_offset=1 over its tokens: the pass's logits choose the decoded tokens with the decode's
    log-probabilities (1e-4 in fp32, the project's fp32 bar; bf16: the existing bf16 bar of 0.07), so its cross-attention is the decode's;
    the maps equal the float64 restatement (bf16: with the bf16 rounding points) within MARGIN x its float32 error, capped.  fp32 only:
    as_decoded=False (positions from 0) gives different maps - a pass that ignored quirk Q1 would fail here.
    Seen on an MI355X: log-probabilities within 2.0e-6 (fp32) / 3.0e-2 (bf16) of the decode's; maps fp32 - e32 1.6e-8 .. 2.0e-8, the pass
    2.5e-8 .. 3.9e-8; bf16 - the pass 1.4e-5 .. 3.0e-5 from the restatement; as_decoded=False moves the maps by 5.7e-4 .. 9.5e-4."""
    fx, m, mem, mask, seqs, lps, smask = _decoded(dev, name, bf16)
    cfg = fx["cfg"]
    Ls, tokens, lens_t, mem32, lens_s, (maps, logits) = _packed_pass(m, mem, mask, seqs, smask, bf16, position_offset=1, return_logits=True)
    L, H = cfg["dec_layers"], cfg["dec_heads"]
    lsm = torch.log_softmax(logits.float(), -1)
    o = 0
    for i, Li in enumerate(Ls):
        want = seqs[i, 1:Li]
        rows = lsm[o:o + Li - 1]
        assert torch.equal(rows.argmax(-1), want), (name, i)
        d = float((rows.gather(-1, want[:, None]).squeeze(1) - lps[i, 1:Li]).abs().max())
        print(f"\n{name} image {i}: max |log-prob(pass) - log-prob(decode)| = {d:.2e}")
        assert d < (0.07 if bf16 else 1e-4)
        o += Li - 1
    sd = _f64(fx["state_dict"])
    w = torch.full((L, H), 1.0 / (L * H), dtype=torch.float64)
    memc = mem32.cpu()
    prec = "bf16" if bf16 else "fp32"
    ref, _ = R.decoder_maps(sd, tokens.cpu(), memc.double(), (lens_t, lens_s), H, list(range(L)), w, 1, prec=prec)
    r32, _ = R.decoder_maps(fx["state_dict"], tokens.cpu(), memc.float(), (lens_t, lens_s), H, list(range(L)), w.float(), 1, prec=prec)
    e32 = max(float((a.double() - b).abs().max()) for a, b in zip(r32, ref))
    err = max(float((a.cpu().double() - b).abs().max()) for a, b in zip(maps, ref))
    tol = _tol(e32, 1.0)
    if bf16:
        # bf16: the float32 and float64 restatements differ only where a bf16 rounding flips, which may be nowhere, while the pass differs from
        # both by the roundings themselves: per entry p allow, on top of the fp32 term, a few bf16 unit roundoffs of p (the log-sum-exp, q, k
        # and what feeds them: 4 x 2^-8), at most CAP_BF16
        worst = max(float(((a.cpu().double() - b).abs() / torch.clamp(tol + 4 * REL_BF16 * b, max=CAP_BF16)).max()) for a, b in zip(maps, ref))
    else:
        worst = err / tol
    print(f"{name} {prec}: e32={e32:.2e} pass err={err:.2e} fp32 tol={tol:.2e} worst err/tolerance={worst:.3f}")
    assert worst <= 1.0, (worst, err, tol)
    tol = CAP_BF16 if bf16 else tol
    for mp, t, s in zip(maps, lens_t, lens_s):
        assert mp.shape == (t, s) and float((mp.sum(-1) - 1).abs().max()) <= tol + s * 2.0 ** -24
    with torch.no_grad(), autocast(device_type="cuda", dtype=BF, enabled=bf16):
        api = m.cross_attention_maps(mem, mask, seqs, smask)
        tf = m.cross_attention_maps(mem, mask, seqs, smask, as_decoded=False)
    for a, b in zip(api, maps):
        assert torch.equal(a, b)
    if not bf16:
        d0 = max(float((a - b).abs().max()) for a, b in zip(tf, maps))
        print(f"{name}: max |map(as_decoded=False) - map| = {d0:.2e}")
        assert d0 > 10 * tol


def test_selection_of_layers_and_heads(dev):
    """layers=[-1] is the last layer's map alone, a one-hot head_weights that head's softmax, the default the mean over everything: each
    against the float64 restatement with those weights, and the default against the mean of the one-hot maps."""
    fx, m, mem, mask, seqs, lps, smask = _decoded(dev, "vitomr_small", False)
    cfg = fx["cfg"]
    L, H = cfg["dec_layers"], cfg["dec_heads"]
    sd = _f64(fx["state_dict"])
    Ls, tokens, lens_t, mem32, lens_s, default = _packed_pass(m, mem, mask, seqs, smask, False, position_offset=1)
    memc = mem32.cpu().double()

    def ref(layers, w, dtype=torch.float64):
        sdx = sd if dtype == torch.float64 else fx["state_dict"]
        return R.decoder_maps(sdx, tokens.cpu(), memc.to(dtype), (lens_t, lens_s), H, layers, torch.as_tensor(w, dtype=dtype), 1)[0]

    def close(got, want, what, e32=0.0):
        err = max(float((a.cpu().double() - b).abs().max()) for a, b in zip(got, want))
        tol = _tol(e32, 1.0)
        print(f"\n{what}: e32={e32:.2e} err={err:.2e} tol={tol:.2e}")
        assert err <= tol, (what, err, tol)

    def against_reference(got, layers, w, what):
        want = ref(layers, w)
        e32 = max(float((a.double() - b).abs().max()) for a, b in zip(ref(layers, w, torch.float32), want))
        close(got, want, what, e32)

    last = _packed_pass(m, mem, mask, seqs, smask, False, position_offset=1, layers=[-1])[-1]
    against_reference(last, [L - 1], [[1.0 / H] * H], "layers=[-1]")
    onehot = [0.0] * H
    onehot[2] = 5.0
    one = _packed_pass(m, mem, mask, seqs, smask, False, position_offset=1, layers=[0], head_weights=onehot)[-1]
    against_reference(one, [0], [[0.0, 0.0, 1.0, 0.0]], "one-hot head")
    against_reference(default, list(range(L)), [[1.0 / (L * H)] * H] * L, "default")
    mean = [torch.zeros_like(d) for d in default]
    for l in range(L):
        for h in range(H):
            w = [0.0] * H
            w[h] = 1.0
            part = _packed_pass(m, mem, mask, seqs, smask, False, position_offset=1, layers=[l], head_weights=w)[-1]
            mean = [a + p / (L * H) for a, p in zip(mean, part)]
    close(default, [x.cpu().double() for x in mean], "default vs mean of one-hot maps", 2.0 ** -23)


# ---- orthogonality -----------------------------------------------------------------------------------------------------------------------
def _grids(fx):
    P = fx["cfg"]["P"]
    return [(int(t.shape[-2]) // P, int(t.shape[-1]) // P) for t in fx["imgs"]]


def test_locating_between_two_decodes_changes_nothing(dev):
    """greedy decode, locate_tokens, greedy decode: the second decode (graph replays included) is bitwise the first; and where the result
    has no map - index 0 and everything after a row's end - patch is -1 and center_px NaN, nowhere else."""
    fx, m, mem, mask, seqs, lps, smask = _decoded(dev, "vitomr_small", True)
    with torch.no_grad(), autocast(device_type="cuda", dtype=BF):
        al = m.locate_tokens(mem, mask, seqs, smask, grids=_grids(fx), return_maps=True)
        again = m.cached_greedy_generate(mem, mask, max_len=fx["cfg"]["gen_len"])
    _same(again, (seqs, lps, smask))
    Ls = m._alignment_lengths(seqs, smask)
    B, T = seqs.shape
    has = torch.zeros(B, T, dtype=torch.bool)
    for i, Li in enumerate(Ls):
        has[i, 1:Li] = True
    patch, center, spread, peak = al.patch.cpu(), al.center_px.cpu(), al.spread_px.cpu(), al.peak.cpu()
    assert patch.dtype == torch.int64 and patch.shape == (B, T) and center.shape == (B, T, 2) and spread.shape == (B, T, 2)
    assert torch.equal(patch >= 0, has) and bool((patch[~has] == -1).all())
    assert torch.equal(~torch.isnan(center).any(-1), has) and torch.equal(~torch.isnan(spread).any(-1), has) and torch.equal(~torch.isnan(peak), has)
    P = fx["cfg"]["P"]
    for i, ((h, w), mp) in enumerate(zip(al.grids, al.maps)):
        assert mp.shape == (Ls[i] - 1, h * w)
        rp, rl = R.locate(mp.cpu().double(), w)
        assert torch.equal(patch[i, 1:Ls[i]], rp)
        assert float((center[i, 1:Ls[i]].double() - rl[:, 2:4] * P).abs().max()) < 1e-3 * P
        assert bool((patch[i, 1:Ls[i]] < h * w).all())
        assert bool((center[i, 1:Ls[i], 0] <= w * P).all()) and bool((center[i, 1:Ls[i], 1] <= h * P).all())


def test_fp8_memory_cache_gives_the_same_maps(dev):
    """The pass reads the memory, not the KV caches: a model whose cross K/V cache is FP8 returns the bf16-cache model's maps bit for bit."""
    fx, m, mem, mask, seqs, lps, smask = _decoded(dev, "vitomr_small", True)
    _, m8, mem8, mask8, *_ = _decoded(dev, "vitomr_small", True, memory_cache_dtype=torch.float8_e4m3fn)
    assert torch.equal(mem, mem8)
    with torch.no_grad(), autocast(device_type="cuda", dtype=BF):
        a = m.cross_attention_maps(mem, mask, seqs, smask)
        b = m8.cross_attention_maps(mem8, mask8, seqs, smask)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("kw", [{}, {"beam_width": 2}, {"speculative": 2}], ids=["greedy", "beam2", "speculative2"])
def test_aligned_inference_decodes_as_inference_does(dev, kw):
    from acai_omr_amd.inference.vitomr_inference import aligned_inference, inference
    fx, m, *_ = _decoded(dev, "vitomr_small", True)
    n = fx["cfg"]["gen_len"]
    plain = inference(m, fx["imgs"], "cuda", max_inference_len=n, **kw)
    seqs, lps, mask, al = aligned_inference(m, fx["imgs"], "cuda", max_inference_len=n, **kw)
    _same((seqs, lps, mask), plain)
    assert al.grids == _grids(fx) and al.maps is None and al.patch.shape == seqs.shape
    Ls = m._alignment_lengths(seqs, mask)
    for i, Li in enumerate(Ls):
        assert bool((al.patch[i, 1:Li] >= 0).all()) and bool((al.patch[i, Li:] == -1).all()) and int(al.patch[i, 0]) == -1
    with pytest.raises(ValueError):
        aligned_inference(m, fx["imgs"], "cuda", max_inference_len=n, beam_width=2, speculative=2)
    with pytest.raises(TypeError):
        aligned_inference(m, fx["imgs"], "cuda", max_inference_len=n, top_k=3)
