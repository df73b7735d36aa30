"""decode_attn_kernel after its prologue was rebuilt for latency: one argument fetch, q read as clamped 16-byte loads, the self form's first
key groups requested before the length is known, cross-lane sums on the DPP network.  None of that may change a result; these tests hold
the two forms of the greedy step to float64 references on inputs where a key read past a length would show.

Cross form (ops.decode_attn, RAGGED): float64 softmax reference, the bar of tests/test_gpu_kernels.py::test_decode_attn (2e-5 absolute, q =
2 randn, k, v = randn), lengths around every edge of the key loop at chunk 64 - 8 keys per wave and 32 per workgroup pass (bf16 d_h 64;
16 / 64 and 4 / 16 for the narrower rows), 64 per unrolled iteration, 64 per split - so that a launch has full, partial, one-key and
empty splits, merged in the launch and by the separate combine.  Every sequence's K / V block sits between rows of NaN: a key of the last
head read past the length, or before the offset, poisons the row.

Self form (acai_decode_hidden, plain self attention): a one-layer decoder, E 1024, 16 heads, cache of Tmax = 130 positions, stepped from
one key to the full cache (lengths 1 .. 130: the group edges 8, 32, 64, 128, and len == Tmax where the early request's clamp to Tmax - 1
is the last row).  The cache is NaN wherever no step has written yet, so a key past the length - which the early request does read, and the
key loop must discard - poisons the step.  Reference: the float64 oracle step of tests/test_gpu_decode_forms.py with an identity unembed, so
that it returns the hidden state; that file's bars (fp32: 2e-5 of the largest value; bf16: two ulps over half the distance between the
bf16-rounding oracle and the float64 one)."""
import math

import pytest
import torch

from decode_support import dev  # noqa: F401
from test_gpu_decode_forms import _cached, _decoder, _ragged_mem, rb, ulp_bf16

pytestmark = pytest.mark.gpu

NAN_ROWS = 64
LENS = [[1, 64, 129], [7, 65, 127], [8, 9, 63]]
FORMS = [("bf16", 64), ("bf16", 32), ("fp32", 64)]
_CASES = {}


def _cross_case(dtype, dh, lens):
    """Inputs and the float64 reference of one case, built once and shared by the two merge forms."""
    key = (dtype, dh, tuple(lens))
    if key not in _CASES:
        H, B = 2, len(lens)
        g = torch.Generator().manual_seed(H + dh + sum(lens))
        q = torch.randn(B, H * dh, generator=g) * 2
        ks = [torch.randn(H, l, dh, generator=g) for l in lens]
        vs = [torch.randn(H, l, dh, generator=g) for l in lens]
        if dtype == "bf16":
            ks, vs = [rb(k).float() for k in ks], [rb(v).float() for v in vs]
        dhp = dh                      # 64 and 32: powers of two, no padded columns
        gap = NAN_ROWS * dhp
        total = gap + sum(H * l * dhp + gap for l in lens)
        kc, vc = torch.full((total,), float("nan")), torch.full((total,), float("nan"))
        offs, o = [], gap
        for k, v, l in zip(ks, vs, lens):
            offs.append(o)
            kc[o:o + H * l * dhp].view(H, l, dhp)[:] = k
            vc[o:o + H * l * dhp].view(H, l, dhp)[:] = v
            o += H * l * dhp + gap
        ref = torch.empty(B, H * dh, dtype=torch.float64)
        for b in range(B):
            for h in range(H):
                s = (q[b, h * dh:(h + 1) * dh].double() @ ks[b][h].double().t()) / math.sqrt(dh)
                ref[b, h * dh:(h + 1) * dh] = torch.softmax(s, -1) @ vs[b][h].double()
        _CASES[key] = (q, kc, vc, offs, dhp, ref)
    return _CASES[key]


@pytest.mark.parametrize("fused_merge", [False, True], ids=["combine", "in_launch"])
@pytest.mark.parametrize("lens", LENS, ids=lambda l: "_".join(map(str, l)))
@pytest.mark.parametrize("dtype,dh", FORMS, ids=[f"{d}_dh{n}" for d, n in FORMS])
def test_cross_form_vs_float64(dev, dtype, dh, lens, fused_merge):  # noqa: F811
    from acai_omr_amd import ops
    q, kc, vc, offs, dhp, ref = _cross_case(dtype, dh, lens)
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    out = ops.decode_attn(q.to(dev), kc.to(dev).to(tdt), vc.to(dev).to(tdt), torch.tensor(offs, dtype=torch.int64, device=dev),
                          torch.tensor(lens, dtype=torch.int32, device=dev), 2, dh, dhp, max(lens), chunk=64, fused_merge=fused_merge)
    err = float((out.cpu().double() - ref).abs().max())
    print(f"{dtype} dh{dh} lens {lens} fused_merge {fused_merge}: max |error| {err:.3g}")
    assert err < 2e-5, err


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_self_form_from_one_key_to_the_full_cache(dev, prec):  # noqa: F811
    from oracle import vitomr_oracle as O
    T, H, E, lens = 130, 16, 1024, [65, 9, 128]
    dec = _decoder(T, L=1, edges=False)
    bf = prec == "bf16"
    mem = _ragged_mem(lens, E, 21)
    sd = {"decoder." + k: v.detach().double() for k, v in dec.state_dict().items()}
    sd["decoder.unembed.weight"], sd["decoder.unembed.bias"] = torch.eye(E, dtype=torch.float64), torch.zeros(E, dtype=torch.float64)
    st_bf, st64 = O.DecodeState(rb(mem), lens, sd, H, "bf16"), O.DecodeState(mem.double(), lens, sd, H, "fp32")
    cached = _cached(dec, 4, torch.bfloat16 if bf else torch.float32, dev)
    mem32 = mem.to(dev)
    cached.decoder_blocks.prepare_caches_packed(None if bf else mem32, mem32.to(torch.bfloat16) if bf else None, lens)
    eng = cached.decoder_blocks.engine(dev)
    assert eng.Tmax == T
    eng.reset_self_cache()
    for c in eng.k_self + eng.v_self:
        c.fill_(float("nan"))
    toks = torch.randint(3, 227, (T, len(lens)), generator=torch.Generator().manual_seed(22))
    emb, pos = dec.vocab_embedding.weight.detach(), dec.pos_embedding.detach()
    worst = (0.0, 0.0, 0)
    with torch.no_grad():
        for t in range(T):
            hid = eng.hidden_step((emb[toks[t]] + pos[t]).to(dev)).double().cpu()
            r64 = O.decode_step(st64, toks[t], t)
            if bf:
                rbf = O.decode_step(st_bf, toks[t], t)
                e, gap = float(((rb(hid) - rbf).abs() - 2 * ulp_bf16(rbf)).max()), float((rbf - r64).abs().max())
                assert e <= 0.5 * gap, (t, e, gap)
            else:
                e, gap = float((hid - r64).abs().max()), float(r64.abs().max())
                assert e <= 2e-5 * gap, (t, e, gap)
            worst = max(worst, (e / gap, e, t))
    print(f"{prec}: worst step error / bar scale {worst}")
    # the whole cache was written, by the steps alone
    for c in eng.k_self + eng.v_self:
        assert bool(torch.isfinite(c[:len(lens)].float()).all())
