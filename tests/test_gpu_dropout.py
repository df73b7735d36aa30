"""Train-mode dropout on the GPU against float64 references under the SAME keep masks.

The kernels' masks are a counter hash of (seed, row, col) (csrc/common.h drop_hash); oracle/dropout_mirror.py restates it on the host, so
every check here is exact about WHICH elements are dropped and float64 about the arithmetic around them:
  - acai_dropout_add bit-exact against the mirror (all four dtype instantiations, with and without a residual, the grid-stride loop);
  - the attention forward / backward with probability dropout against float64 autograd with the mirror's mask on P in front of P V;
  - whole train-mode steps (TeacherForcedViTOMR, ScheduledSamplingViTOMR) against the CPU oracle fed, site by site, with the masks the HIP
    path drew - the sites' order, kinds, probabilities and shapes are part of the check.
"""
import math
import os

import pytest
import torch

from conftest import VOCAB, load_golden
from oracle import dropout_mirror as DM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from acai_omr_amd import _lib
    _lib.lib()
    return "cuda"


def _threads():
    try:
        n = len(os.sched_getaffinity(0))
    except Exception:
        n = os.cpu_count() or 8
    torch.set_num_threads(max(1, min(n, 16)))


def md(a, b):
    return float((a.detach().float().cpu() - b.detach().float().cpu()).abs().max())


def relerr(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def cosine(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a @ b) / (a.norm() * b.norm()).clamp(min=1e-300))


# ---- acai_dropout_add --------------------------------------------------------------------------------------------------------------------
_DT = {"fp32": torch.float32, "bf16": torch.bfloat16}


@pytest.mark.parametrize("rows,cols", [(1037, 77), (513, 1), (4104, 1024)])      # ragged rows; one column; > 8192 x 256: the grid-stride loop
@pytest.mark.parametrize("xdt,odt", [("fp32", "fp32"), ("fp32", "bf16"), ("bf16", "fp32"), ("bf16", "bf16")])
@pytest.mark.parametrize("residual", [False, True])
def test_dropout_add_bit_exact_against_the_mirror(dev, rows, cols, xdt, odt, residual):
    """Kept set = the mirror's, exactly; kept values = fp32(x * scale) (+ res) rounded once to the output dtype (the product and the sum may be
    one fused multiply-add: either rounding is accepted, element by element); dropped values = res (or 0).  DropoutAddFn's backward drops
    exactly the same elements and passes the residual's gradient through."""
    from acai_omr_amd import ops
    from acai_omr_amd.train.autograd_path import DropoutAddFn
    p = 0.1 if rows != 513 else 0.5
    seed = 2 ** 31 - 3 if cols == 1024 else rows * 7 + cols
    g = torch.Generator().manual_seed(rows + cols)
    x = torch.randn(rows, cols, generator=g)
    x = torch.where(x == 0, torch.ones_like(x), x).to(_DT[xdt])
    res = torch.randn(rows, cols, generator=g) if residual else None
    out = ops.dropout_add(x.to(dev), None if res is None else res.to(dev), p, seed, out_dtype=_DT[odt]).cpu()
    assert out.dtype == _DT[odt]
    keep = DM.dropout_keep(seed, rows, cols, p)
    scale = torch.tensor(DM.drop_scale(p), dtype=torch.float32)
    xs = x.float() * scale                                                   # fp32 product
    base = torch.zeros(rows, cols) if res is None else res
    two = torch.where(keep, xs + base, base).to(_DT[odt])                     # rounded product, then the sum
    fused = torch.where(keep, (x.double() * scale.double() + base.double()).float(), base).to(_DT[odt])
    ok = (out == two) | (out == fused)
    assert bool(ok.all()), (int((~ok).sum()), float((out.float() - two.float()).abs().max()))
    if res is None:
        assert torch.equal(out != 0, keep)
    else:
        assert torch.equal(out[~keep], res.to(_DT[odt])[~keep])
    assert abs(float(keep.float().mean()) - (1 - p)) < 6 * (p * (1 - p) / keep.numel()) ** 0.5
    # the autograd node: same elements dropped in the backward, scale applied, residual gradient passed through
    xg = x.to(dev).requires_grad_(True)
    rg = None if res is None else res.to(dev).requires_grad_(True)
    y = DropoutAddFn.apply(xg, rg, p, seed)
    dy = torch.randn(rows, cols, generator=g)
    y.backward(dy.to(dev).to(y.dtype))
    dyy = dy.to(y.dtype).float()
    dx_ref = torch.where(keep, dyy * scale, torch.zeros(())).to(x.dtype)
    assert xg.grad.dtype == x.dtype and torch.equal(xg.grad.cpu(), dx_ref)
    if rg is not None:
        assert torch.equal(rg.grad.cpu(), dyy)


# ---- attention with probability dropout --------------------------------------------------------------------------------------------------
def ref_attn_dropout(q, k, v, dout, lens_q, lens_k, H, dh, causal, p, seed):
    """float64 autograd: O = (softmax(q k^T / sqrt(dh)) * keep / (1 - p)) V per (sequence, head) with the mirror's mask (the placement of
    F.multi_head_attention_forward); lse = log2 sum exp of the UNDROPPED scores, as the kernels store it (log2 domain).  Returns o, lse, dq,
    dk, dv."""
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    total_q = sum(lens_q)
    o = torch.zeros(total_q, H * dh, dtype=torch.float64)
    lse = torch.zeros(H * total_q, dtype=torch.float64)
    parts = []
    oq = ok = 0
    for lq, lk in zip(lens_q, lens_k):
        for h in range(H):
            sl = slice(h * dh, (h + 1) * dh)
            s = qr[oq:oq + lq, sl] @ kr[ok:ok + lk, sl].t() / math.sqrt(dh)
            if causal:
                s = s.masked_fill(~torch.ones(lq, lk, dtype=torch.bool).tril(), float("-inf"))
            mult = DM.multiplier(DM.attn_keep(seed, p, h, total_q, oq, lq, lk), p)
            ob = (torch.softmax(s, -1) * mult) @ vr[ok:ok + lk, sl]
            parts.append((oq, lq, sl, ob))
            lse[h * total_q + oq:h * total_q + oq + lq] = torch.logsumexp(s.detach(), -1) / math.log(2.0)
            o[oq:oq + lq, sl] = ob.detach()
        oq += lq
        ok += lk
    loss = sum((ob * dout[a:a + l, sl].double()).sum() for a, l, sl, ob in parts)
    loss.backward()
    return o, lse, qr.grad, kr.grad, vr.grad


# The dropout instantiations (attn_varlen.hip launch_form<>: attn_fwd_kernel<T, DHP, FAST, DROP = true, PRE>; attn_bwd.hip launch_form<>:
# attn_bwd_dq_kernel / attn_bwd_dkv_kernel<T, DHP, F, D = true, P>).  "slow": d_h not a multiple of 16 bytes' elements (fp32 4, bf16 8);
# "fast": aligned, q unscaled; "pre": aligned, q prescaled (the training path).  Each instantiation is reached by the cases marked:
#
#   T     DHP | slow                     | fast                            | pre
#   fp32  32  | fp32_s32 (d_h 6)         | fp32_f32 (d_h 16)               | fp32_p32 (d_h 32)
#   bf16  32  | bf16_s32a (6), _s32b (12)| bf16_f32 (d_h 32, >= 512 rows)  | bf16_p32 (d_h 16, p = 0.5)
#   fp32  64  | fp32_s64 (d_h 34)        | fp32_f64 (d_h 48)               | fp32_p64 (d_h 64, 1025 x 512)
#   bf16  64  | bf16_s64 (d_h 36)        | bf16_f64 (d_h 64)               | bf16_p64 (d_h 48), enc4096, dec513, cross513x4096
#
# With dropout the dispatch takes none of the no-dropout fast forms (attn_fwd64, two-block forward, one-pass / wide / two-block backward), so
# the long bf16 prescaled cases run the one-block kernels at the training lengths.
ATTN_CASES = [
    # id,           H, dh, lens_q,            lens_k,             causal, dtype,  pre,   p,    seed
    ("fp32_s32",    2, 6,  [37, 1, 20],        None,               False,  "fp32", False, 0.1,  7),
    ("fp32_f32",    2, 16, [130, 1, 77],       None,               True,   "fp32", False, 0.1,  2 ** 31 - 3),
    ("fp32_p32",    2, 32, [333, 128],         [200, 513],         False,  "fp32", True,  0.05, 91),
    ("bf16_s32a",   2, 6,  [65, 64],           None,               True,   "bf16", False, 0.05, 2 ** 31 - 3),
    ("bf16_s32b",   3, 12, [7, 12],            [20, 13],           False,  "bf16", False, 0.1,  5),
    ("bf16_f32",    2, 32, [600, 513],         [1000, 577],        False,  "bf16", False, 0.05, 123),
    ("bf16_p32",    2, 16, [700, 130, 1],      None,               True,   "bf16", True,  0.5,  4294967290),
    ("fp32_s64",    2, 34, [8, 32, 200],       None,               False,  "fp32", False, 0.1,  3),
    ("fp32_f64",    2, 48, [513, 1],           [256, 40],          False,  "fp32", False, 0.1,  17),
    ("fp32_p64",    1, 64, [1025],             [512],              False,  "fp32", True,  0.05, 2 ** 31 - 1),
    ("bf16_s64",    1, 36, [300, 1],           None,               True,   "bf16", False, 0.05, 11),
    ("bf16_f64",    2, 64, [256, 1],           [400, 77],          False,  "bf16", False, 0.1,  29),
    ("bf16_p64",    2, 48, [37, 20],           None,               True,   "bf16", True,  0.1,  31),
    # the training shapes: bf16, prescaled, d_h 64 - fine-tune encoder self attention, causal decoder self attention, the decoder's cross
    # attention into the shared memory K / V (accumulate_dkv: dk / dv are pre-filled and the kernel adds to them)
    ("enc4096",     2, 64, [4096],             None,               False,  "bf16", True,  0.05, 2 ** 31 - 3),
    ("dec513",      2, 64, [513, 300],         None,               True,   "bf16", True,  0.1,  1234567),
    ("cross513x4096", 2, 64, [513, 300],       [4096, 1100],       False,  "bf16", True,  0.1,  2 ** 31 - 2),
]


@pytest.mark.parametrize("case", ATTN_CASES, ids=[c[0] for c in ATTN_CASES])
def test_attn_dropout_vs_float64(dev, case):
    """o, lse, dq, dk, dv of the attention kernels with probability dropout against float64 autograd under the mirror's mask.  Bars: those of
    test_attn_varlen (o: fp32 2e-5, bf16 1.2e-2 x max(1, |o|)) and test_attn_backward (gradients: fp32 3e-5, bf16 6e-2 relative to max(1, |g|));
    lse: 1e-5 relative to max(1, |lse|) (fp32 score arithmetic in both dtypes); relative Frobenius errors: fp32 1e-5, bf16 1e-2, and o's under a
    quarter of the dropout's own effect on it."""
    from acai_omr_amd import engine, ops
    name, H, dh, lens_q, lens_k, causal, dtype, pre, p, seed = case
    _threads()
    lens_k = lens_k or lens_q
    accum = name.startswith("cross")
    tdt = _DT[dtype]
    E = H * dh
    g = torch.Generator().manual_seed(H * dh + sum(lens_q) + sum(lens_k))
    q = (torch.randn(sum(lens_q), E, generator=g) * 1.5).to(tdt).float()
    k = torch.randn(sum(lens_k), E, generator=g).to(tdt).float()
    v = torch.randn(sum(lens_k), E, generator=g).to(tdt).float()
    dout = torch.randn(sum(lens_q), E, generator=g).to(tdt).float()
    qp = (q * ops.QSCALE(dh)).to(tdt)
    if pre:
        q = qp.double() / ops.QSCALE(dh)          # the q the kernel effectively sees
    o_r, lse_r, dq_r, dk_r, dv_r = ref_attn_dropout(q, k, v, dout, lens_q, lens_k, H, dh, causal, p, seed)
    qd = qp.to(dev) if pre else q.to(dev).to(tdt)
    kd, vd, dd = (t.to(dev).to(tdt) for t in (k, v, dout))
    cu_q, cu_k = engine.cu_from_lens(lens_q, dev), engine.cu_from_lens(lens_k, dev)
    lse = torch.empty(H * sum(lens_q), device=dev)
    o = ops.attn_varlen(qd, kd, vd, cu_q, cu_k, H, dh, max(lens_q), causal=causal, lse=lse, dropout_p=p, seed=seed, q_prescaled=pre)
    dq = torch.empty_like(qd)
    if accum:
        k0 = (0.1 * torch.randn(k.shape, generator=g)).to(tdt)
        v0 = (0.1 * torch.randn(v.shape, generator=g)).to(tdt)
        dk, dv = k0.to(dev), v0.to(dev)
        dk_r, dv_r = dk_r + k0.double(), dv_r + v0.double()
    else:
        dk, dv = torch.empty_like(kd), torch.empty_like(vd)
    ops.attn_varlen_bwd(qd, kd, vd, o, dd, lse, cu_q, cu_k, H, dh, max(lens_q), max(lens_k), causal, dq, dk, dv, dropout_p=p, seed=seed,
                        q_prescaled=pre, accumulate_dkv=accum)
    bf = dtype == "bf16"
    e_o = md(o, o_r)
    e_lse = md(lse, lse_r) / max(1.0, float(lse_r.abs().max()))
    outs = (("o", o, o_r), ("dq", dq, dq_r), ("dk", dk, dk_r), ("dv", dv, dv_r))
    errs = {n: md(a, r) / max(1.0, float(r.abs().max())) for n, a, r in outs[1:]}
    fro = {n: float((a.cpu().double() - r).norm() / r.norm()) for n, a, r in outs}
    # the size of the dropout's own effect on o: the kernel's output without dropout against the dropped reference
    o0 = ops.attn_varlen(qd, kd, vd, cu_q, cu_k, H, dh, max(lens_q), causal=causal, q_prescaled=pre)
    d_drop = float((o0.cpu().double() - o_r).norm() / o_r.norm())
    print(f"{name}: o {e_o:.3e}  lse {e_lse:.3e}  " + "  ".join(f"{n} {e:.3e}" for n, e in errs.items()) +
          "  | rel. Frobenius " + "  ".join(f"{n} {e:.3e}" for n, e in fro.items()) + f"  | dropout's effect on o {d_drop:.3e}")
    assert e_o < (1.2e-2 * max(1.0, float(o_r.abs().max())) if bf else 2e-5), e_o   # measured: fp32 <= 1.2e-6, bf16 <= 1.3e-2 (|o| up to 6)
    assert e_lse < 1e-5, e_lse                                           # measured <= 1.3e-7
    for n, e in errs.items():
        assert e < (6e-2 if bf else 3e-5), (n, e)                          # measured: fp32 <= 2.4e-6, bf16 <= 7.6e-3
    # the max-abs bars above are bf16 resolution of the largest element; the mask's own effect can be smaller than that on long rows, so
    # the whole tensors are held to a bar well under that effect as well
    assert fro["o"] < 0.25 * d_drop, (fro["o"], d_drop)
    for n, e in fro.items():
        assert e < (1e-2 if bf else 1e-5), (n, e)                          # measured: fp32 <= 1.4e-6, bf16 <= 3.9e-3


# ---- whole train-mode steps against the oracle under the same masks ----------------------------------------------------------------------
class _Recorder:
    """Wraps ops.attn_varlen / ops.dropout_add for the forward: every call with p > 0, in call order, as (kind, p, seed, geometry)."""

    def __init__(self):
        self.recs = []

    def __enter__(self):
        from acai_omr_amd import ops
        self._ops, self._attn, self._add = ops, ops.attn_varlen, ops.dropout_add
        attn, add, recs = self._attn, self._add, self.recs

        def attn_rec(q, k, v, cu_q, cu_k, H, dh, max_q, causal=False, out=None, lse=None, dropout_p=0.0, seed=0, q_prescaled=False):
            if dropout_p > 0:
                recs.append(dict(kind="attn", p=dropout_p, seed=int(seed) & 0xFFFFFFFF, total_q=q.shape[0], H=H,
                                 cu_q=cu_q.cpu().tolist(), cu_k=cu_k.cpu().tolist()))
            return attn(q, k, v, cu_q, cu_k, H, dh, max_q, causal=causal, out=out, lse=lse, dropout_p=dropout_p, seed=seed, q_prescaled=q_prescaled)

        def add_rec(x, residual, p, seed, out_dtype=None):
            if p > 0:
                recs.append(dict(kind="add", p=p, seed=int(seed) & 0xFFFFFFFF, shape=tuple(x.shape)))
            return add(x, residual, p, seed, out_dtype=out_dtype)

        ops.attn_varlen, ops.dropout_add = attn_rec, add_rec
        return self

    def __exit__(self, *exc):
        self._ops.attn_varlen, self._ops.dropout_add = self._attn, self._add
        return False


class _Replay:
    """The oracle's `drop` hook fed from a _Recorder's record.  A site's probability is that of the HIP model's module of the same path; at
    every site with p > 0 the next record must have the site's kind, p and shape.  Rows of the oracle's packings are mapped onto the HIP
    path's: the encoder packs the same real lengths (checked: its cu_seqlens are the oracle's); the transition head runs on the padded
    (B, L_max) latent; the decoder packs the real LMX lengths where the oracle packs T rows per sequence (pad rows: any mask)."""

    def __init__(self, model, recs, lens_s, real_t):
        self.model, self.recs, self.i = model, recs, 0
        self.lens_s, self.real_t = list(lens_s), list(real_t)
        self.sites = []

    def _p(self, site):
        from acai_omr_amd.train.autograd_path import _p_of
        return _p_of(self.model.get_submodule(site), True)

    def _hip_rows(self, site, lens):
        """For each oracle row: (HIP row or -1 for a pad row)."""
        out = []
        if site.startswith("encoder."):
            assert list(lens) == self.lens_s
            return torch.arange(sum(lens))
        if site.startswith("transition_head."):
            lm = max(self.lens_s)
            for b, l in enumerate(lens):
                out.append(b * lm + torch.arange(l))
            return torch.cat(out)
        cu = [0]
        for l in self.real_t:
            cu.append(cu[-1] + l)
        for b, l in enumerate(lens):
            r = cu[b] + torch.arange(l)
            r[self.real_t[b]:] = -1
            out.append(r)
        return torch.cat(out)

    def __call__(self, site, kind, **geom):
        p = self._p(site)
        if p <= 0.0:
            return None
        assert self.i < len(self.recs), f"the HIP forward drew fewer masks than the oracle has sites (at {site})"
        rec = self.recs[self.i]
        self.i += 1
        self.sites.append(site)
        assert rec["kind"] == kind and DM.p_f32(rec["p"]) == DM.p_f32(p), (site, kind, p, rec)
        seed = rec["seed"]
        if kind == "add":
            rows = self._hip_rows(site, geom["lens"])
            if site.startswith("decoder."):
                n_hip = sum(self.real_t)
            elif site.startswith("transition_head."):
                n_hip = len(self.lens_s) * max(self.lens_s)
            else:
                n_hip = sum(geom["lens"])
            assert rec["shape"] == (n_hip, geom["cols"]), (site, rec["shape"], n_hip, geom["cols"])
            m = DM.multiplier(DM.dropout_keep(seed, rows.clamp(min=0), geom["cols"], p), p)
            m[rows < 0] = 1.0
            return m
        lens_q, lens_k, H = geom["lens_q"], geom["lens_k"], geom["heads"]
        assert rec["H"] == H
        hq = self.lens_s if site.startswith("encoder.") else self.real_t
        hk = self.lens_s if (site.startswith("encoder.") or site.endswith("multihead_attn")) else self.real_t
        cq, ck = [0], [0]
        for a, b in zip(hq, hk):
            cq.append(cq[-1] + a)
            ck.append(ck[-1] + b)
        assert rec["cu_q"] == cq and rec["cu_k"] == ck and rec["total_q"] == cq[-1], (site, rec["cu_q"], cq, rec["cu_k"], ck)

        def blk(i, h):
            m = torch.ones(lens_q[i], lens_k[i], dtype=torch.float64)
            lq, lk = min(lens_q[i], hq[i]), min(lens_k[i], hk[i])
            m[:lq, :lk] = DM.multiplier(DM.attn_keep(seed, p, h, cq[-1], cq[i], lq, lk), p)
            return m
        return blk


P_ENC, P_DEC, P_HEAD = 0.05, 0.1, 0.05     # the reference's fine-tune schedule (transformer_dropout / transition_head_dropout)


def _model(cls, cfg, sd, dev):
    from acai_omr_amd.models.models import FineTuneOMREncoder, OMRDecoder
    enc = FineTuneOMREncoder(cfg["P"], cfg["pe_h"], cfg["pe_w"], cfg["ft_depth"], num_layers=cfg["enc_layers"], hidden_dim=cfg["enc_dim"],
                             num_heads=cfg["enc_heads"], mlp_dim=cfg["enc_mlp"], transformer_dropout=P_ENC)
    dec = OMRDecoder(cfg["max_len"], VOCAB, num_layers=cfg["dec_layers"], hidden_dim=cfg["dec_dim"], num_heads=cfg["dec_heads"], mlp_dim=cfg["dec_mlp"],
                     transformer_dropout=P_DEC)
    m = cls(enc, None, dec, transition_head_dim=cfg["head_dim"], transition_head_dropout=P_HEAD)
    m.load_state_dict(sd)
    return m.to(dev).train()


def _expected_count(cfg, passes):
    return cfg["ft_depth"] * 4 + 1 + cfg["dec_layers"] * 6 * passes


def _run_case(dev, name, prec, ss, fuse=True, step_seed=5):
    """HIP train-mode step (records the masks) and the oracle's step under them; returns both sides' pred, loss, gradients."""
    from torch.amp import autocast
    import oracle.vitomr_oracle as O
    from acai_omr_amd.models.models import OMRCELoss, ScheduledSamplingViTOMR, TeacherForcedViTOMR
    from acai_omr_amd.train import autograd_path as AP
    _threads()
    fx = load_golden(name)
    base = load_golden(fx["base"]) if ss else fx
    cfg = base["cfg"]
    batch = list(zip(base["imgs"], base["lmx"]))
    m = _model(ScheduledSamplingViTOMR if ss else TeacherForcedViTOMR, cfg, base["state_dict"], dev)
    bf = prec == "bf16"
    AP.PGRAD_FUSE, AP._KV_GRAD_FUSE = fuse, fuse
    try:
        torch.manual_seed(step_seed)
        with _Recorder() as rec, autocast(device_type="cuda", dtype=torch.bfloat16, enabled=bf):
            if ss:
                pred, tgt = m.forward_train(batch, fx["tf_prob"], fx["tau"], fx["hard"], noise=fx["noise"])
            else:
                pred, tgt = m(batch)
            loss = OMRCELoss(m.decoder.pad_idx)(pred, tgt)
        loss.backward()
    finally:
        AP.PGRAD_FUSE, AP._KV_GRAD_FUSE = True, True
    recs = rec.recs
    assert len(recs) == _expected_count(cfg, 2 if ss else 1), len(recs)
    assert len({r["seed"] for r in recs}) == len(recs)                        # a fresh seed per site (and per pass)
    # the oracle under the recorded masks: float64 for the fp32 step, the bf16 restatement (fp32 weights) for the autocast one
    dt = torch.float32 if bf else torch.float64
    sd = {k: (v.to(dt) if v.is_floating_point() else v).clone().requires_grad_(v.is_floating_point()) for k, v in base["state_dict"].items()}
    imgs = [t.to(dt) for t in base["imgs"]]
    P = cfg["P"]
    lens_s = [(t.shape[-2] // P) * (t.shape[-1] // P) for t in imgs]
    T = max(len(s) for s in base["lmx"]) - 1
    real_t = [min(len(s), T) for s in base["lmx"]]        # the decoder's input is the padded batch minus its last column: non-pad tokens
    replay = _Replay(m, recs, lens_s, real_t)
    ob = list(zip(imgs, base["lmx"]))
    if ss:
        pred_o, tgt_o = O.scheduled_sampling_forward(ob, sd, cfg["enc_heads"], cfg["dec_heads"], P, prec, fx["tf_prob"], fx["tau"], fx["hard"],
                                                     fx["noise"], drop=replay)
    else:
        pred_o, tgt_o = O.teacher_forced_forward(ob, sd, cfg["enc_heads"], cfg["dec_heads"], P, prec, drop=replay)
    assert replay.i == len(recs), (replay.i, len(recs))                       # every mask the HIP path drew has its oracle site
    loss_o = O.ce_loss(pred_o, tgt_o, 1)
    loss_o.backward()
    assert torch.equal(tgt.cpu(), tgt_o)
    params = dict(m.named_parameters())
    grads = {n: (params[n].grad, sd[n].grad) for n in params if params[n].grad is not None}
    assert len(grads) > 20 and all(go is not None for _, go in grads.values())
    return pred, loss, pred_o, loss_o, grads, replay.sites


def _check_fp32(label, pred, loss, pred_o, loss_o, grads, tgt_valid):
    e_pred, e_loss = md(pred.float().cpu()[tgt_valid], pred_o.detach()[tgt_valid]), abs(float(loss.detach()) - float(loss_o.detach()))
    print(f"{label}: pred max|d| {e_pred:.3e}  loss d {e_loss:.3e} (loss {float(loss_o):.4f})")
    assert e_pred < 1e-3                                                     # measured <= 8.4e-7
    assert e_loss < 1e-4                                                     # measured 4.8e-7
    worst = 0.0
    for n, (g, go) in grads.items():
        e = md(g, go)
        worst = max(worst, e / max(1.0, float(go.abs().max())))
        assert e < 3e-4 * max(1.0, float(go.abs().max())), (n, e)          # measured <= 8.2e-8 relative
    print(f"  grads: max |d| / max(1, |g|) {worst:.3e} over {len(grads)} tensors")


def test_teacher_forced_train_step_with_dropout_vs_oracle(dev):
    """TeacherForcedViTOMR.train() with the reference's dropout (encoder fine-tune blocks 0.05, decoder 0.1, head 0.05) on the tf_small weights:
    pred, loss and every gradient against the float64 oracle under the masks the HIP step drew, with the bars of
    test_teacher_forced_train_step_vs_reference.  Also: the sites come in torch's order and number."""
    pred, loss, pred_o, loss_o, grads, sites = _run_case(dev, "tf_small", "fp32", ss=False)
    cfg = load_golden("tf_small")["cfg"]
    d0 = "decoder.decoder_blocks.layers.0."
    i_head = 4 * cfg["ft_depth"]
    assert sites[:4] == ["encoder.fine_tune_blocks.layers.0." + s for s in ("self_attn", "dropout1", "dropout", "dropout2")]
    assert sites[i_head] == "transition_head.2"
    assert sites[i_head + 1:i_head + 7] == [d0 + s for s in ("self_attn", "dropout1", "multihead_attn", "dropout2", "dropout", "dropout3")]
    valid = load_golden("tf_small")["target"] != 1
    _check_fp32("tf_small train mode", pred, loss, pred_o, loss_o, grads, valid)
    # the masks matter: the eval-mode (p = 0) oracle is far from this step
    assert abs(float(loss_o) - float(load_golden("tf_small")["loss"])) > 1e-3


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "plain"])
def test_scheduled_sampling_train_step_with_dropout_vs_oracle(dev, fuse):
    """ScheduledSamplingViTOMR.forward_train at tf_prob 0.7 with the tf_ss_small draws and the reference's dropout: two decoder passes, fresh
    masks in each (the shared memory K / V gathers both passes' gradients), against the float64 oracle under the same masks; with the gradient
    fusions on and off, as test_scheduled_sampling_train_step_vs_reference."""
    pred, loss, pred_o, loss_o, grads, sites = _run_case(dev, "tf_ss_small", "fp32", ss=True, fuse=fuse)
    assert sites.count("decoder.decoder_blocks.layers.1.dropout3") == 2
    valid = load_golden("tf_ss_small")["target"] != 1
    _check_fp32(f"tf_ss_small train mode {'fused' if fuse else 'plain'}", pred, loss, pred_o, loss_o, grads, valid)


@pytest.mark.parametrize("name", ["tf_small", "tf_dh64"])
def test_teacher_forced_bf16_train_step_with_dropout_vs_oracle(dev, name):
    """The same step under autocast(bf16) against the oracle's bf16 restatement under the same masks, with the bars of
    test_config3_teacher_forced_bf16_golden_sizes_vs_oracle.  tf_dh64 (d_h 64 everywhere): the prescaled-q dropout kernels inside a real step."""
    pred, loss, pred_o, loss_o, grads, _ = _run_case(dev, name, "bf16", ss=False)
    valid = load_golden(name)["target"] != 1
    e_pred = md(pred.float().cpu()[valid], pred_o.detach()[valid])
    print(f"{name} bf16 train mode: pred max|d| {e_pred:.3e} (|pred| max {float(pred_o.abs().max()):.2f})  loss d {abs(float(loss) - float(loss_o)):.3e}")
    assert e_pred < 0.05 * max(1.0, float(pred_o.abs().max()))             # measured 7.8e-3 (|pred| max 2.1)
    assert abs(float(loss) - float(loss_o)) < 2e-2                          # measured <= 3.4e-4
    worst_r, worst_c = 0.0, 1.0
    for n, (g, go) in grads.items():
        r, c = relerr(g, go), cosine(g, go)
        worst_r, worst_c = max(worst_r, r), min(worst_c, c)
        assert r < 0.08 and c > 0.995, (n, r, c)                            # measured <= 9.7e-3, cosine >= 0.99997
    print(f"  grads: rel max err <= {worst_r:.3e}, cosine >= {worst_c:.6f} over {len(grads)} tensors")
