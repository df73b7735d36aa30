"""FP8 (e4m3fn) memory cache on the GPU: OMRDecoder.to_cached_version(B, torch.bfloat16, memory_cache_dtype=torch.float8_e4m3fn).

  1. the quantiser (acai_cross_kv_quantize_fp8): the FP8 engine's K/V bytes and scales equal acai_omr_amd.fp8.quantize_rows of the bf16
     engine's cross K/V, bit for bit, padding included; and on crafted rows with subnormal outputs;
  2. the FP8 form of the cross-attention kernel (ops.decode_attn on an e4m3fn cache) against float64 attention over the dequantised K/V:
     max|dev - R64| <= 2e-5 max|R64| (fp32 accumulation), arrival counters back at zero;
  3. full-width decoder steps against the oracle's bf16 restatement whose cross K/V is the engine's dequantised FP8 cache, at the bar of
     test_full_width_decoder_steps_vs_float64 (bf16); the deviation from the plain bf16 engine is printed;
  4. the entry points agree with each other on an FP8 memory cache, its allocation is at most (dhp8 + 4) / (2 dhp) of the bf16 one, and
     grouped cross K/V raises ValueError;
  5. a bf16 engine built after an FP8 one computes what a bf16 engine computed before it, bit for bit.
Token ids are NOT compared with the bf16 memory cache's: the fixtures' random weights have argmax margins well inside FP8's rounding."""
import pytest
import torch
from torch.amp import autocast

from conftest import VOCAB, load_golden
from decode_support import build_vitomr, dev

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn
F64 = torch.float64


def _small_decoder(E, H, L=2, T=32, seed=1):
    from acai_omr_amd.models.models import OMRDecoder
    torch.manual_seed(seed)
    return OMRDecoder(T, VOCAB, num_layers=L, hidden_dim=E, num_heads=H, mlp_dim=2 * E)


def _cached(dec, B, dev, mdt=None):
    c = dec.to_cached_version(B, torch.bfloat16, mdt)
    c.load_state_dict(dec.state_dict())
    return c.to(dev).eval()


# ---- 1. quantiser ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,H", [(256, 4), (48, 4)], ids=["dh64", "dh12"])
def test_quantiser_bit_exact_against_torch(dev, E, H):
    from acai_omr_amd.fp8 import quantize_rows
    lens = [4096, 1300, 64, 1]
    dec = _small_decoder(E, H)
    mem = torch.randn(sum(lens), E, generator=torch.Generator().manual_seed(4)).to(dev).to(torch.bfloat16)
    cb, c8 = _cached(dec, 4, dev), _cached(dec, 4, dev, F8)
    with torch.no_grad():
        for c in (cb, c8):
            c.decoder_blocks.prepare_caches_packed(None, mem, lens)
    eb, e8 = cb.decoder_blocks.engine(dev), c8.decoder_blocks.engine(dev)
    assert e8.cdhp == eb.dhp and e8.cross_fp8 and not eb.cross_fp8
    d = e8.cdhp
    n = sum(lens) * H
    for l in range(eb.L):
        for xb, x8, s8 in ((eb.k_cross[l], e8.k_cross[l], e8.k_cross_scale[l]), (eb.v_cross[l], e8.v_cross[l], e8.v_cross_scale[l])):
            q, s = quantize_rows(xb[:n * d].view(n, d).cpu())
            assert torch.equal(x8[:n * d].view(torch.uint8).cpu(), q.view(torch.uint8).view(-1)), l
            assert torch.equal(s8[:n].cpu().view(torch.int32), s.view(torch.int32)), l
    # the padding columns (d_h 12 -> rows of 16) are zero bytes
    if E // H < d:
        assert int(e8.k_cross[0][:n * d].view(n, d)[:, E // H:].view(torch.uint8).abs().sum()) == 0


def test_quantiser_subnormals_and_wide_rows(dev):
    """Rows spanning 2^-40 .. 2^20 of their maximum: many outputs are e4m3fn subnormals or round to (signed) zero."""
    from acai_omr_amd import ops
    from acai_omr_amd.fp8 import quantize_rows
    g = torch.Generator().manual_seed(9)
    for dhp in (16, 32, 64):
        rows = 3001
        x = torch.randn(rows, dhp, generator=g) * torch.exp2(torch.randint(-40, 20, (rows, dhp), generator=g).float())
        x[7] = 0.0
        x[8, :] = -0.0
        x = x.to(torch.bfloat16)
        xd = x.view(-1).to(dev)
        k8 = torch.empty(rows * dhp, dtype=F8, device=dev)
        v8 = torch.empty_like(k8)
        ks = torch.empty(rows, device=dev)
        vs = torch.empty_like(ks)
        ops.cross_kv_quantize_fp8(xd, xd.neg(), k8, v8, ks, vs, 0, rows, dhp)
        for got, gs, src in ((k8, ks, x), (v8, vs, -x)):
            q, s = quantize_rows(src)
            assert torch.equal(got.view(torch.uint8).cpu(), q.view(torch.uint8).view(-1)), dhp
            assert torch.equal(gs.cpu(), s), dhp
        sub = ((q.view(torch.uint8) & 0x78) == 0) & ((q.view(torch.uint8) & 0x07) != 0)
        assert int(sub.sum()) > 100, "the case must reach subnormal outputs"
        # a row range at an offset leaves the other rows alone
        k8.zero_()
        ops.cross_kv_quantize_fp8(xd, xd, k8, v8, ks, vs, 100, 50, dhp)
        kb = k8.view(torch.uint8).view(rows, dhp).cpu()
        assert int(kb[:100].sum()) == 0 and int(kb[150:].sum()) == 0
        assert torch.equal(kb[100:150], quantize_rows(x[100:150])[0].view(torch.uint8))


# ---- 2. kernel against float64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dh,dhp", [(64, 64), (12, 16), (32, 32)])
@pytest.mark.parametrize("chunk", [4096, 256])
@pytest.mark.parametrize("fused", [True, False])
def test_fp8_decode_attn_vs_float64(dev, dh, dhp, chunk, fused):
    from acai_omr_amd import ops
    from acai_omr_amd.fp8 import dequantize_rows, quantize_rows
    lens, H = [1, 15, 16, 17, 1000, 4096], 4
    g = torch.Generator().manual_seed(dh + chunk)
    offs, o = [], 0
    for l in lens:
        offs.append(o)
        o += l * H * dhp
    rows = o // dhp
    kv = []
    for _ in range(2):
        x = torch.zeros(rows, dhp)
        x[:, :dh] = torch.randn(rows, dh, generator=g) * torch.exp2(torch.randint(-3, 4, (rows, 1), generator=g).float())
        kv.append(quantize_rows(x.to(torch.bfloat16)))
    (kq, ksc), (vq, vsc) = kv
    q = torch.randn(len(lens), H * dh, generator=g) * 2
    out = ops.decode_attn(q.to(dev), kq.view(-1).to(dev), vq.view(-1).to(dev), torch.tensor(offs, dtype=torch.int64, device=dev),
                          torch.tensor(lens, dtype=torch.int32, device=dev), H, dh, dhp, max(lens), chunk=chunk, fused_merge=fused,
                          k_scale=ksc.to(dev), v_scale=vsc.to(dev))   # (the wrapper asserts the arrival counters are back at zero)
    K, V = dequantize_rows(kq, ksc).double(), dequantize_rows(vq, vsc).double()
    worst = 0.0
    for b, (l, off) in enumerate(zip(lens, offs)):
        r0 = off // dhp
        kb = K[r0:r0 + H * l].view(H, l, dhp)[..., :dh]
        vb = V[r0:r0 + H * l].view(H, l, dhp)[..., :dh]
        qb = q[b].double().view(H, 1, dh)
        p = torch.softmax((qb @ kb.transpose(1, 2)) / dh ** 0.5, dim=-1)
        r64 = (p @ vb).view(-1)
        err = float((out[b].cpu().double() - r64).abs().max())
        assert err <= 2e-5 * float(r64.abs().max()), (b, l, err)
        worst = max(worst, err / float(r64.abs().max()))
    print(f"dh {dh} chunk {chunk} fused {fused}: worst max|dev - R64| / max|R64| {worst:.3g}")


# ---- 3. full-width decoder steps ---------------------------------------------------------------------------------------------------------
def test_full_width_decoder_steps_fp8_memory(dev):
    """E 1024, 16 heads, F 4096, 2 layers, memories [4096, 1300, 64], 70 teacher-forced logits_step calls."""
    from oracle import vitomr_oracle as O
    from test_gpu_decode_forms import _decoder, _oracle_states, _ragged_mem, ulp_bf16
    T, S, lens, H = 80, 70, [4096, 1300, 64], 16
    dec = _decoder(T)
    mem = _ragged_mem(lens, 1024, 11)
    st_bf, st64 = _oracle_states(dec, mem, lens, H)
    memb = mem.to(dev).to(torch.bfloat16)
    c8, cb = _cached(dec, 4, dev, F8), _cached(dec, 4, dev)
    with torch.no_grad():
        for c in (c8, cb):
            c.decoder_blocks.prepare_caches_packed(None, memb, lens)
    e8, eb = c8.decoder_blocks.engine(dev), cb.decoder_blocks.engine(dev)
    for l in range(e8.L):   # R_bf with the engine's dequantised FP8 cross K/V
        K, V = e8.cross_kv_values(l)
        o = 0
        for b, n in enumerate(lens):
            st_bf.k_cross[l][b] = K[o:o + H * n * e8.cdhp].view(H, n, e8.cdhp)[..., :64].double().cpu()
            st_bf.v_cross[l][b] = V[o:o + H * n * e8.cdhp].view(H, n, e8.cdhp)[..., :64].double().cpu()
            o += H * n * e8.cdhp
    toks = torch.randint(3, 227, (S, len(lens)), generator=torch.Generator().manual_seed(12))
    worst, vs_bf16 = (0.0, 0.0), 0.0
    with torch.no_grad():
        for t in range(S):
            lg = e8.logits_step(toks[t].to(dev), t).double().cpu()
            lb = eb.logits_step(toks[t].to(dev), t).double().cpu()
            r64 = O.decode_step(st64, toks[t], t)
            rbf = O.decode_step(st_bf, toks[t], t)
            e, gap = float(((lg - rbf).abs() - 2 * ulp_bf16(rbf)).max()), float((rbf - r64).abs().max())
            assert e <= 0.5 * gap, (t, e, gap)
            worst = max(worst, (e / gap, e))
            vs_bf16 = max(vs_bf16, float((lg - lb).abs().max()) / float(lb.abs().max()))
    print(f"fp8 memory: worst step error / bar scale {worst}; max|fp8 - bf16 engine| / max|logit| {vs_bf16:.3g}")


# ---- 4. entry points ---------------------------------------------------------------------------------------------------------------------
def _rows_equal(a, b):
    return a.shape == b.shape and torch.equal(a, b)


@pytest.mark.parametrize("name", ["vitomr_small", "vitomr_dh64", "vitomr_odd"])
def test_entry_points_agree_on_fp8_memory(dev, name):
    """Token ids are not compared with the bf16 memory cache's (random weights: small argmax margins).  Within the FP8 cache: inference()
    with and without graph replay, streamed_inference, a stepwise argmax loop over cached_generate and continuous_inference(slots=2) -
    whose every image equals its own solo greedy run bit for bit - agree."""
    from acai_omr_amd.inference.vitomr_inference import continuous_inference, inference, streamed_inference
    fx = load_golden(name)
    cfg, sd, imgs, T = fx["cfg"], fx["state_dict"], fx["imgs"], fx["cfg"]["gen_len"]
    m = build_vitomr(cfg, sd, dev, torch.bfloat16, max_batch=8, memory_cache_dtype=F8)
    blocks = m.decoder.decoder_blocks
    seqs, lps, mask = inference(m, imgs, "cuda", max_inference_len=T)
    eng = blocks.engine(dev)
    assert eng.cross_fp8 and eng.k_cross[0].dtype == F8
    with torch.no_grad():   # the same prepared caches, eager steps instead of graph replays
        s2, l2, _ = eng.greedy(T, use_graph=False)
        s2, l2, m2 = m.mask_and_clip_seqs(s2.clone(), l2.clone())
    assert _rows_equal(s2, seqs) and torch.equal(l2, lps) and torch.equal(m2, mask)
    # per image: streamed and a stepwise cached_generate loop against inference() of the image alone
    for i, img in enumerate(imgs):
        si, li, mi = inference(m, [img], "cuda", max_inference_len=T)
        n = si.shape[1]
        ev = list(streamed_inference([img], m, "cuda", max_inference_len=T, flush_interval=5))
        assert torch.equal(ev[-1]["payload"]["sequence"], si), i
        with torch.no_grad():
            lat, lmask = m.encoder([img])
            with autocast(device_type="cuda", dtype=torch.bfloat16):
                memi = m.transition_head(lat)
            seq, _, _ = m.cached_set_up_inference(memi, T)
            for t in range(1, T):
                idx, _ = m.cached_get_next_token(seq, t, lmask)
                seq[:, t] = idx
        assert torch.equal(seq[0, :n], si[0]), (i, seq, si)
    # continuous batching through 2 slots, the images twice: every image bit for bit its own greedy run on the same packed memory
    from acai_omr_amd.inference.vitomr_inference import _encode_chunks
    order = list(range(len(imgs))) * 2
    cs, cl, cm = continuous_inference(m, [imgs[i] for i in order], "cuda", max_inference_len=T, slots=2)
    with torch.no_grad():
        pm, plens = _encode_chunks(m, [imgs[i] for i in order], "cuda")
        o = 0
        for r, l in enumerate(plens):
            si, li, _ = m._greedy_packed(None, pm[o:o + l], [l], T)
            o += l
            n = si.shape[1]
            assert torch.equal(cs[r, :n], si[0]) and torch.equal(cl[r, :n], li[0]), r
            assert bool((cs[r, n:] == m.decoder.pad_idx).all()), r
    # allocation: at most (dhp8 + 4) / (2 dhp) of the bf16 engine's, prepared on the same memories
    mb, m8 = (build_vitomr(cfg, sd, dev, torch.bfloat16, max_batch=8, memory_cache_dtype=mdt) for mdt in (None, F8))
    inference(mb, imgs, "cuda", max_inference_len=T)
    inference(m8, imgs, "cuda", max_inference_len=T)
    eb, eng = mb.decoder.decoder_blocks.engine(dev), m8.decoder.decoder_blocks.engine(dev)
    ratio = eng.cross_kv_bytes() / eb.cross_kv_bytes()
    assert ratio <= (eng.cdhp + 4) / (2 * eb.dhp) + 1e-9, ratio
    print(f"{name}: d_h {eng.dh} dhp8 {eng.cdhp}: FP8 / bf16 cross K/V bytes {ratio:.4f}")
    # grouped cross K/V (beam search, grouped rollouts) is out of scope: a ValueError, no silent fallback
    with pytest.raises(ValueError, match="FP8 memory cache"):
        inference(m, imgs, "cuda", max_inference_len=T, beam_width=2)
    with pytest.raises(ValueError, match="FP8 memory cache"):
        with torch.no_grad():
            lat, lmask = m.encoder(imgs)
            blocks.prepare_caches_packed(*_packed(m, lat, lmask), group_size=2)


def _packed(m, lat, lmask):
    from acai_omr_amd import engine as EG
    with autocast(device_type="cuda", dtype=torch.bfloat16):
        mem = m.transition_head(lat)
    mem32, lens = EG.unpad_rows(mem, lmask)
    return mem32, None, lens


# ---- 5. isolation ------------------------------------------------------------------------------------------------------------------------
def test_bf16_engine_unchanged_after_fp8_engine(dev):
    from test_gpu_decode_forms import _decoder, _ragged_mem
    lens = [4096, 1300, 64]
    dec = _decoder(40)
    memb = _ragged_mem(lens, 1024, 11).to(dev).to(torch.bfloat16)
    toks = torch.randint(3, 227, (30, len(lens)), generator=torch.Generator().manual_seed(2))

    def run(mdt):
        c = _cached(dec, 4, dev, mdt)
        with torch.no_grad():
            c.decoder_blocks.prepare_caches_packed(None, memb, lens)
            eng = c.decoder_blocks.engine(dev)
            out = [eng.logits_step(toks[t].to(dev), t).clone() for t in range(30)]
            seqs, _, _ = eng.greedy(24)
        return torch.stack(out), seqs.clone()

    before, sb = run(None)
    run(F8)
    after, sa = run(None)
    assert torch.equal(before, after) and torch.equal(sb, sa)
