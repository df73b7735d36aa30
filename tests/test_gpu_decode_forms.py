"""Every form of the bf16 decode step's kernels against float64 references (the fused path bench.py measures).

Two references per case, both in float64 arithmetic:
  R64  - no rounding anywhere (fp32 operands taken exactly, bf16 weights replaced by their fp32 originals);
  R_bf - the operands the kernel sees (bf16-rounded W, activations rounded where the kernel rounds them: LayerNorm in float64,
         then bf16) and the kernel's output rounding points.
Bars:
  * GEMV forms: per element |dev - R_bf| <= 2 K 2^-24 (|x^| |W^|^T + |bias|) (fp32 accumulation) + one bf16 ulp of the value at each
    rounding point the form has + 2^-21 of the residual term; LayerNorm-on-load forms may further exceed that by 0.2 max|R_bf - R64|
    (an fp32 LayerNorm may round an element to the neighbouring bf16 value where float64 does not).
  * Full decoder steps: max(|dev - R_bf| - two bf16 ulps of the logit) <= 0.5 max|R_bf - R64| per step (bf16; 1.0 x for the grouped
    matrix-core cross attention, which rounds P to bf16),
    max|dev - R64| <= 2e-5 max|R64| (fp32).
Measured on one MI355X (printed by each test with -s): GEMV forms max|dev - R_bf| <= 0.023 against max|R_bf - R64| of 0.005-0.04 (most
fp32-output cases 1e-7..3e-5); published (mean, rstd) within 0.25 x 2^-22 max|x| and 5e-7 relative, offset/spread 3000 rows included;
full-width decoder (bf16) at most 0.45 of its bar, fp32 6e-7 relative; self caches layer 0 inside one ulp, layer 1 at 0.67 of its bar;
grouped cross attention at most 0.6 of its bar.  The module runs in about 15 s on the device."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import VOCAB
from decode_support import dev

pytestmark = pytest.mark.gpu

F64 = torch.float64


def ulp_bf16(a):
    """One bf16 ulp of |a| (float64), the subnormal floor ignored (values here are far above it)."""
    a = a.abs().clamp_min(1e-30)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def rb(x):
    return x.to(torch.bfloat16).to(F64)


def ln64(x, w, b, eps):
    x = x.to(F64)
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + eps) * w.to(F64) + b.to(F64), m[:, 0], 1 / torch.sqrt(v[:, 0] + eps)


# ---------------------------------------------------------------------------------------------------------------------------------------
# A / B: GEMV forms through ops.skinny_gemm_ex

def _rows(B, K, kind, g):
    """fp32 activation rows.  kind: 'unit' O(1) rows; 'edges' cycles offset/spread 30, 300, 3000, rows scaled by 1e-3 (variance near eps)
    and a constant row - every row with its own offset, so a statistic taken from the wrong row shows."""
    x = torch.randn(B, K, generator=g)
    if kind == "unit":
        return x + torch.randn(B, 1, generator=g)
    out = []
    for b in range(B):
        c = b % 5
        if c == 0:
            out.append(x[b] + 30.0 * (1 + 0.1 * b))
        elif c == 1:
            out.append(0.5 * x[b] + 150.0 * (1 + 0.01 * b))
        elif c == 2:
            out.append(0.01 * x[b] - 30.0 * (1 + 0.01 * b))        # offset / spread 3000
        elif c == 3:
            out.append(1e-3 * x[b] + 0.002 * b)                   # variance 1e-6, eps 1e-5
        else:
            out.append(torch.full((K,), 1234.567 + b))            # constant row
    return torch.stack(out)


def _gemv(dev, B, N, K, *, xbf=False, ln=False, res=False, rln=None, gelu=False, rnd=False, ybf=False, ldx_pad=0, rows="unit",
          seed=0, form=None):
    """One skinny_gemm_ex call and its two references; returns (excess over the bar, stats error) and checks both."""
    from acai_omr_amd import ops
    g = torch.Generator().manual_seed(seed * 7919 + B * 31 + N + K)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    Wb = W.to(torch.bfloat16)
    bias = 0.1 * torch.randn(N, generator=g)
    xs = _rows(B, K + ldx_pad, rows, g)[:, :K]
    lnw, lnb = 1 + 0.2 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g)
    # operands as the kernel sees them (R_bf) and unrounded (R64)
    if xbf:
        xbuf = torch.randn(B, K + ldx_pad, generator=g).to(torch.bfloat16)
        xk, x64 = xbuf[:, :K].to(F64), xbuf[:, :K].to(F64)
        xd = xbuf.to(dev)[:, :K]
    else:
        xbuf = torch.zeros(B, K + ldx_pad)
        xbuf[:, :K] = xs
        xd = xbuf.to(dev)[:, :K]
        if ln:
            xl, m64, r64 = ln64(xs, lnw, lnb, 1e-5)
            xk, x64 = rb(xl), xl
        else:
            xk, x64 = rb(xs), xs.to(F64)
    resid = rterm = None
    if res:
        resid = torch.randn(B, N, generator=g) if rln is None else rln["z"]
        rterm = resid.to(F64) if rln is None else ln64(resid, rln["w"], rln["b"], 1e-5)[0]
        if rln is not None:   # the published mean is an fp32 value: ~2^-24 |mean| off, times rstd |w| in the rebuilt row
            zm, zr = ln64(resid, rln["w"], rln["b"], 1e-5)[1:]
            rln_tol = 2.0 ** -22 * (zm.abs() * zr)[:, None] * rln["w"].abs().to(F64)[None, :]

    def ref(xop, Wop, rounded):
        y = xop @ Wop.to(F64).T + bias.to(F64)
        if rounded and rnd:
            y = rb(y)
        if gelu:
            y = F.gelu(y)
            if rounded and rnd:
                y = rb(y)
        pre = y
        if res:
            y = y + rterm
        if rounded and ybf:
            y = rb(y)
        return y, pre
    Rbf, pre = ref(xk, Wb, True)
    R64, _ = ref(x64, W, False)
    stats = torch.full((B, 2), float("nan"), device=dev) if ln else None
    kw = dict(bias=bias.to(dev), gelu=gelu, round_bf16=rnd, out_dtype=torch.bfloat16 if ybf else torch.float32)
    if ln:
        kw.update(ln=(lnw.to(dev), lnb.to(dev)), stats_out=stats)
    if res:
        kw["residual"] = resid.to(dev)
        if rln is not None:
            kw.update(rln=(rln["w"].to(dev), rln["b"].to(dev)), rstats=rln["stats"])
    y = ops.skinny_gemm_ex(xd, Wb.to(dev), **kw)
    torch.cuda.synchronize()
    yd = y.double().cpu()
    tol = 2 * K * 2.0 ** -24 * (xk.abs() @ Wb.to(F64).abs().T + bias.abs().to(F64))
    if rnd:
        tol = tol + ulp_bf16(pre) * (2 if gelu else 1)
    elif gelu:
        tol = tol + 2.0 ** -21 * pre.abs()
    if res:
        tol = tol + 2.0 ** -21 * rterm.abs() + (rln_tol if rln is not None else 0)
    if ybf:
        tol = tol + ulp_bf16(Rbf)
    err = (yd - Rbf).abs()
    gap = float((Rbf - R64).abs().max())
    excess = float((err - tol).max())
    allow = 0.2 * gap if ln else 0.0
    assert torch.isfinite(yd).all(), form
    assert excess <= allow, (form, B, N, K, excess, allow, float(err.max()), gap)
    st_err = None
    if ln:
        s = stats.cpu().double()
        # mean: an fp32 value of the row's scale; rstd: relative
        em = float(((s[:, 0] - m64).abs() / (xs.double().abs().max(1).values * 2.0 ** -22 + 1e-12)).max())
        er = float(((s[:, 1] - r64) / r64).abs().max())
        assert em <= 1.0 and er <= 2e-5, (form, em, er)
        st_err = (em, er)
    return dict(err=float(err.max()), gap=gap, excess=excess, stats=st_err, y=y, stats_t=stats, xs=xs, lnw=lnw, lnb=lnb)


# (form the launcher selects, cases).  The selection (decode_gemv.hip launch_skinny, bf16 weights, K % 256 == 0, 16-byte aligned operands):
#   fp32 x, K = 1024                  -> skinny_chain_kernel<false, LN, 4>        (LN = 1 with ln, 0 without)
#   bf16 x, K = 4096, no ln           -> skinny_chain_kernel<true, 0, 16>
#   fp32 x, K <= 1024 (not 1024)      -> skinny_mfma_kernel<false, 4, 4>
#   fp32 x, 1024 < K <= 4096          -> skinny_mfma_kernel<false, 16, 4>
#   bf16 x, K != 4096                 -> skinny_mfma_kernel<true, 1, 4>
# rows per workgroup: N >= 2560 -> 16, N >= 1600 -> 8, else 4; batch tiles of 16 rows.
FORMS = [
    ("chain<false,0,4>", dict(K=1024), [(1, 1024, {}), (5, 3072, dict(rnd=True, ldx_pad=2048)), (17, 227, dict(res=True)),
                                         (40, 1600, dict(rnd=True, res=True)), (64, 1000, dict(rnd=True, gelu=True, ybf=True))]),
    ("chain<false,1,4>", dict(K=1024, ln=True), [(1, 227, {}), (3, 4096, dict(rnd=True, gelu=True, ybf=True)), (4, 2560, dict(rnd=True)),
                                                 (13, 3072, dict(rnd=True, ldx_pad=2048)), (16, 1024, dict(res=True)),
                                                 (17, 1600, dict(rnd=True, res=True)), (64, 1004, dict(rnd=True))]),
    ("chain<true,0,16>", dict(K=4096, xbf=True), [(1, 1024, dict(rnd=True, res=True)), (5, 227, {}), (16, 2560, dict(ldx_pad=64)),
                                                   (17, 1024, dict(rnd=True)), (40, 3000, dict(rnd=True, gelu=True, ybf=True))]),
    ("mfma<false,4,4>", dict(K=512), [(1, 227, dict(ln=True)), (5, 1600, dict(rnd=True)), (17, 2560, dict(ln=True, rnd=True, res=True)),
                                      (40, 1000, dict(ln=True, rnd=True, gelu=True, ybf=True))]),
    ("mfma<false,4,4>", dict(K=768), [(3, 4096, dict(ln=True, rnd=True)), (13, 1024, dict(ldx_pad=256)), (64, 227, dict(ln=True))]),
    ("mfma<false,16,4>", dict(K=2048), [(1, 1024, dict(ln=True)), (5, 1000, dict(ln=True, rnd=True, ldx_pad=64)),
                                        (17, 2560, dict(rnd=True, res=True)), (40, 227, dict(ln=True, gelu=True, rnd=True, ybf=True))]),
    ("mfma<true,1,4>", dict(K=2048, xbf=True), [(1, 227, {}), (13, 3072, dict(rnd=True, res=True)), (17, 1600, dict(ldx_pad=64)),
                                                (64, 1000, dict(rnd=True, gelu=True, ybf=True))]),
]


@pytest.mark.parametrize("form,base,cases", FORMS, ids=[f[0] + f"_K{f[1]['K']}" for f in FORMS])
def test_gemv_forms_vs_float64(dev, form, base, cases):
    for B, N, kw in cases:
        r = _gemv(dev, B, N, form=form, **base, **kw)
        print(f"{form} B={B} N={N} {kw}: max|dev-R_bf| {r['err']:.3g}  max|R_bf-R64| {r['gap']:.3g}  stats {r['stats']}")


@pytest.mark.parametrize("K,N1,K2,xbf2", [(1024, 1024, 1024, False), (1024, 1024, 4096, True), (1024, 1024, 2048, False),
                                          (768, 2560, 512, False)])
@pytest.mark.parametrize("B", [3, 17, 40])
def test_residual_layernorm_from_published_stats(dev, K, N1, K2, xbf2, B):
    """Call 1 applies LN(z) on load and publishes (mean, rstd) (checked against float64); call 2 adds LN(z) rebuilt from those statistics
    to its output - the decode step's self_out / cross_out / linear2 pattern.  z rows carry large per-row offsets (LayerNorm edges), so
    statistics taken from another row would be far off."""
    r1 = _gemv(dev, B, N1, K=K, ln=True, rnd=True, rows="edges", seed=1, form="publish")
    rln = dict(z=r1["xs"], w=r1["lnw"], b=r1["lnb"], stats=r1["stats_t"])
    r2 = _gemv(dev, B, K, K=K2, xbf=xbf2, res=True, rln=rln, rnd=True, seed=2, form="rln")
    print(f"publish K={K} B={B}: stats (mean err in 2^-22 |x|max, rstd rel) {r1['stats']};  rln K2={K2}: max|dev-R_bf| {r2['err']:.3g} "
          f"gap {r2['gap']:.3g}")


@pytest.mark.parametrize("K,form", [(1024, "chain<false,1,4>"), (512, "mfma<false,4,4>"), (2048, "mfma<false,16,4>")])
def test_layernorm_statistics_edges(dev, K, form):
    """Rows whose offset is 30, 300 and 3000 times their spread, rows with variance near eps and constant rows, through every
    LayerNorm-on-load form: the outputs against R_bf and the published (mean, rstd) against float64."""
    for B in (5, 16, 17):
        r = _gemv(dev, B, 1024, K=K, ln=True, rnd=True, rows="edges", seed=3, form=form)
        print(f"{form} edges B={B}: max|dev-R_bf| {r['err']:.3g} gap {r['gap']:.3g} stats {r['stats']}")


@pytest.mark.parametrize("wdt,K", [(torch.float32, 1000), (torch.float32, 999), (torch.bfloat16, 520), (torch.bfloat16, 517)])
def test_valu_skinny_gemm_forms(dev, wdt, K):
    """skinny_gemm_kernel, the VALU GEMV: fp32 weights, or bf16 weights whose K the MFMA kernels cannot take; the fast (16-byte rows)
    and slow (element) weight loads; B over one 8-row pass; bias, residual, GELU, the round flag."""
    from acai_omr_amd import ops
    for B, N, gelu, rnd in [(1, 227, False, False), (9, 1000, True, wdt == torch.bfloat16), (17, 333, False, True)]:
        g = torch.Generator().manual_seed(B + K)
        W = torch.randn(N, K, generator=g) / math.sqrt(K)
        Wk = W.to(wdt)
        x = torch.randn(B, K, generator=g)
        bias, resid = 0.1 * torch.randn(N, generator=g), torch.randn(B, N, generator=g)
        y = ops.skinny_gemm_ex(x.to(dev), Wk.to(dev), bias=bias.to(dev), residual=resid.to(dev), gelu=gelu, round_bf16=rnd).double().cpu()
        xk = rb(x) if wdt == torch.bfloat16 else x.double()
        pre = xk @ Wk.double().T + bias.double()
        if rnd:
            pre = rb(pre)
        if gelu:
            pre = F.gelu(pre)
            if rnd:
                pre = rb(pre)
        ref = pre + resid.double()
        tol = 2 * K * 2.0 ** -24 * (xk.abs() @ Wk.double().abs().T + bias.abs().double()) + 2.0 ** -21 * (ref.abs() + pre.abs())
        if rnd:
            tol = tol + 2 * ulp_bf16(pre)
        assert float(((y - ref).abs() - tol).max()) <= 0, (wdt, K, B, float((y - ref).abs().max()))


def test_layernorm_refused_where_it_cannot_run(dev):
    from acai_omr_amd import ops
    K = 520
    x = torch.randn(2, K, device=dev)
    w = torch.randn(64, K, device=dev).to(torch.bfloat16)
    ln = (torch.ones(K, device=dev), torch.zeros(K, device=dev))
    with pytest.raises(RuntimeError, match="LayerNorm"):
        ops.skinny_gemm_ex(x, w, ln=ln)          # K % 256 != 0: the VALU kernel has no LayerNorm
    for K in (2048, 4096):                        # bf16 activations: LayerNorm on load needs the fp32 rows
        xb = torch.randn(2, K, device=dev).to(torch.bfloat16)
        with pytest.raises(RuntimeError, match="LayerNorm"):
            ops.skinny_gemm_ex(xb, torch.randn(64, K, device=dev).to(torch.bfloat16), ln=(torch.ones(K, device=dev), torch.zeros(K, device=dev)))
    with pytest.raises(RuntimeError, match="LayerNorm"):
        ops.skinny_gemm_ex(torch.randn(2, 1024, device=dev), torch.randn(64, 1024, device=dev), ln=(torch.ones(1024, device=dev),
                                                                                                 torch.zeros(1024, device=dev)))  # fp32 W


# ---------------------------------------------------------------------------------------------------------------------------------------
# C / D / E: the full-width decoder, step by step, against the oracle in float64

def _decoder(T, L=2, E=1024, H=16, Fd=4096, seed=5, edges=True):
    from acai_omr_amd.models.models import OMRDecoder
    torch.manual_seed(seed)
    dec = OMRDecoder(T, VOCAB, num_layers=L, hidden_dim=E, num_heads=H, mlp_dim=Fd)
    with torch.no_grad():
        for n, p in dec.named_parameters():
            if "norm" in n:
                p.add_(0.1 * torch.randn_like(p))
        dec.unembed.weight.mul_(4.0)
        if edges:
            lay = dec.decoder_blocks.layers
            lay[L - 1].norm3.weight.mul_(1e-3)     # the final norm's input variance ~1e-6: its eps 1e-6 against norm3's 1e-5 matters
            lay[L - 1].norm3.bias.mul_(1e-3)
            lay[0].norm2.bias.add_(40.0)           # z rows after layer 0's MLP carry an offset of ~40 spreads
    return dec


def _cached(dec, B, cdt, dev):
    c = dec.to_cached_version(B, cdt)
    c.load_state_dict(dec.state_dict())
    return c.to(dev).eval()


def _oracle_states(dec, mem, lens, H, group=1):
    """(R_bf state, R64 state) on float64 weights; group > 1: every memory's cross K/V serves `group` materialised rows."""
    from oracle import vitomr_oracle as O
    sd = {"decoder." + k: v.detach().double() for k, v in dec.state_dict().items()}
    out = []
    for prec, m in (("bf16", rb(mem)), ("fp32", mem.double())):
        st = O.DecodeState(m, lens, sd, H, prec)
        if group > 1:
            st.k_cross = [[k for k in ks for _ in range(group)] for ks in st.k_cross]
            st.v_cross = [[v for v in vs for _ in range(group)] for vs in st.v_cross]
            st.B = len(lens) * group
            st.k_self = [torch.zeros(st.B, *c.shape[1:], dtype=F64) for c in st.k_self]
            st.v_self = [torch.zeros(st.B, *c.shape[1:], dtype=F64) for c in st.v_self]
        out.append(st)
    return out


def _ragged_mem(lens, E, seed):
    return torch.randn(sum(lens), E, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_full_width_decoder_steps_vs_float64(dev, prec):
    """OMRDecoder(E 1024, 16 heads, F 4096, V 227, 2 layers), ragged memories [4096, 1300, 64] (several cross splits, a partial one and a
    one-split row), 70 teacher-forced steps (the self cache crosses a 64-key boundary): logits at every step, then the self K/V caches and
    the cross K/V of the prefill, against the float64 oracle.  Then: prepare again after a longer run; the logits equal a fresh engine's."""
    from oracle import vitomr_oracle as O
    T, S, lens, H = 80, 70, [4096, 1300, 64], 16
    dec = _decoder(T)
    bf = prec == "bf16"
    cdt = torch.bfloat16 if bf else torch.float32
    mem = _ragged_mem(lens, 1024, 11)
    st_bf, st64 = _oracle_states(dec, mem, lens, H)
    cached = _cached(dec, 4, cdt, dev)
    blocks = cached.decoder_blocks
    mem32 = mem.to(dev)
    prep = lambda c: c.decoder_blocks.prepare_caches_packed(None if bf else mem32, mem32.to(torch.bfloat16) if bf else None, lens)  # noqa: E731
    prep(cached)
    eng = blocks.engine(dev)
    toks = torch.randint(3, 227, (S, len(lens)), generator=torch.Generator().manual_seed(12))
    worst = (0.0, 0.0)
    with torch.no_grad():
        for t in range(S):
            lg = eng.logits_step(toks[t].to(dev), t).double().cpu()
            r64 = O.decode_step(st64, toks[t], t)
            if bf:
                rbf = O.decode_step(st_bf, toks[t], t)
                # the logits are bf16: two output ulps (a flip at the output and one carried in from an upstream rounding point) on top of
                # the rounding-difference bar
                e, gap = float(((lg - rbf).abs() - 2 * ulp_bf16(rbf)).max()), float((rbf - r64).abs().max())
                assert e <= 0.5 * gap, (t, e, gap)
            else:
                e, gap = float((lg - r64).abs().max()), float(r64.abs().max())
                assert e <= 2e-5 * gap, (t, e, gap)
            worst = max(worst, (e / gap, e))
        print(f"{prec}: worst step error / bar scale {worst}")
        # self K/V caches.  bf16, layer 0 (its input is the embedding, identical on both sides): within one ulp of the oracle's rounded k/v,
        # plus 2^-16 of the cache's scale for entries near zero, where the fp32 accumulation error of the projection exceeds their ulp.
        # Deeper layers read activations that went through rounding points already: one ulp plus 0.5 max|R_bf - R64| of that cache.
        # fp32: 1e-5 of the cache's scale.
        ref_st = st_bf if bf else st64
        for l in range(len(blocks.layers)):
            for dc, rc, r64 in ((eng.k_self[l], ref_st.k_self[l], st64.k_self[l]), (eng.v_self[l], ref_st.v_self[l], st64.v_self[l])):
                d = dc[:len(lens), :, :S, :64].double().cpu()
                r = rc[:, :, :S]
                if bf:
                    ex = float(((d - r).abs() - ulp_bf16(r) - 2.0 ** -16 * r.abs().max()).max())
                    allow = 0.0 if l == 0 else 0.5 * float((r - r64[:, :, :S]).abs().max())
                    print(f"self cache layer {l}: excess over one ulp {ex:.3g}, allowed {allow:.3g}")
                    assert ex <= allow, (l, ex, allow)
                else:
                    assert float((d - r).abs().max()) <= 1e-5 * float(r.abs().max()), l
            # cross K/V of the prefill: [offset of sequence b + (h * len_b + s) * dhp + d]
            o = 0
            for b, n in enumerate(lens):
                for dc, rc in ((eng.k_cross[l], ref_st.k_cross[l][b]), (eng.v_cross[l], ref_st.v_cross[l][b])):
                    d = dc[o:o + H * n * eng.dhp].view(H, n, eng.dhp)[..., :64].double().cpu()
                    if bf:
                        assert float(((d - rc).abs() - ulp_bf16(rc) - 2.0 ** -16 * rc.abs().max()).max()) <= 0, (l, b)
                    else:
                        assert float((d - rc).abs().max()) <= 1e-5 * float(rc.abs().max()), (l, b)
                o += H * n * eng.dhp
        # stale entries are never read: run further (78 steps), prepare, decode again; bit for bit a fresh engine's logits
        for t in range(S, T - 2):
            eng.logits_step(toks[t % S].to(dev), t)
        prep(cached)
        fresh = _cached(dec, 4, cdt, dev)
        prep(fresh)
        eng2 = fresh.decoder_blocks.engine(dev)
        for t in range(66):
            a = eng.logits_step(toks[(t + 5) % S].to(dev), t).clone()
            b = eng2.logits_step(toks[(t + 5) % S].to(dev), t)
            assert torch.equal(a, b), t


@pytest.mark.parametrize("G,dh", [(2, 64), (16, 64), (17, 64), (20, 64), (33, 64), (17, 48)])
def test_grouped_cross_attention_vs_float64(dev, G, dh):
    """Rollout groups (bf16, stored d_h padded to 64): prepare_caches_packed(group_size=G) on three ragged images [4096, 1500, 40]
    (several splits, a partial split, one split), G rows per image (a second 16-row tile from G = 17, a third at 33), every row's logits
    against the float64 oracle on the materialised rows.  d_h = 48: E = 768, 16 heads, padded to 64."""
    from oracle import vitomr_oracle as O
    E = 64 * 16 if dh == 64 else 768
    T, S, lens, H = 16, 4, [4096, 1500, 40], 16
    dec = _decoder(T, E=E, Fd=4 * E, seed=6 + G)
    B = len(lens) * G
    mem = _ragged_mem(lens, E, 13)
    st_bf, st64 = _oracle_states(dec, mem, lens, H, group=G)
    cached = _cached(dec, B, torch.bfloat16, dev)
    blocks = cached.decoder_blocks
    blocks.prepare_caches_packed(None, mem.to(dev).to(torch.bfloat16), lens, group_size=G)
    eng = blocks.engine(dev)
    assert eng.group == G and eng.dhp == 64
    toks = torch.randint(3, 227, (S, B), generator=torch.Generator().manual_seed(G))
    with torch.no_grad():
        for t in range(S):
            lg = eng.logits_step(toks[t].to(dev), t).double().cpu()
            rbf, r64 = O.decode_step(st_bf, toks[t], t), O.decode_step(st64, toks[t], t)
            e, gap = ((lg - rbf).abs() - 2 * ulp_bf16(rbf)).amax(1), (rbf - r64).abs().amax(1)   # bf16 logits: two output ulps, as above
            print(f"G={G} dh={dh} t={t}: max|dev-R_bf| {float(e.max()):.3g}  max|R_bf-R64| {float(gap.max()):.3g}")
            # bar 1.0 x (not 0.5 x) the rounding gap: the matrix-core kernel rounds P to bf16 for its PV product, a rounding point R_bf lacks
            assert float(e.max()) <= float(gap.max()), (t, int(e.argmax()), float(e.max()), float(gap.max()))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [3, 6, 10])
def test_greedy_argmax_ties_pick_the_lower_index(dev, prec, B):
    """Unembed rows 3, 67 and 200 identical (weights and bias), and far above the rest: the decode step's argmax must pick 3 (torch.argmax:
    the first index) - 3 and 67 fall to one lane's strided scan, 200 to another lane.  B <= 4, B <= 8 and B > 8 use different block sizes."""
    from acai_omr_amd.models.models import ViTOMR
    dec = _decoder(16, L=1, edges=False)
    with torch.no_grad():
        for i in (67, 200):
            dec.unembed.weight[i] = dec.unembed.weight[3]
        dec.unembed.bias[3] = 60.0
        dec.unembed.bias[67] = dec.unembed.bias[200] = 60.0
    bf = prec == "bf16"
    model = ViTOMR(None, None, _cached(dec, 16, torch.bfloat16 if bf else torch.float32, dev))
    lens = [40 + 7 * b for b in range(B)]
    mem = _ragged_mem(lens, 1024, 14).to(dev)
    with torch.no_grad():
        seqs, _, _ = model._greedy_packed(None if bf else mem, mem.to(torch.bfloat16) if bf else None, lens, 6)
    seqs = seqs.cpu()
    assert seqs.shape[1] == 6 and bool((seqs[:, 1:] == 3).all()), seqs
