"""The FP8 memory-cache format, restated in torch (no GPU needed).

A cross K/V row of dhp elements is stored as OCP e4m3fn values q and one fp32 scale 2^e, the value being q * 2^e.  e is the smallest integer
with amax(row) * 2^-e <= 448 (the e4m3fn maximum), but at least -126 so that 2^e and 2^-e are normal floats; an all-zero row has e = 0.
Because the scale is a power of two, quantising (x * 2^-e, then one round-to-nearest-even cast) and dequantising (q * 2^e) round nothing
beyond the cast itself.  `acai_cross_kv_quantize_fp8` computes exactly this, bit for bit.
"""
import torch

E4M3_MAX = 448.0
E_MIN = -126


def pow2(e):
    """2^e as fp32, exactly, for integer tensors e in [-126, 127] (built from the exponent bits)."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def scale_exponents(amax):
    """Per-row exponent e (int32) for row maxima amax (fp32, >= 0)."""
    m, k = torch.frexp(amax.to(torch.float32))   # amax = m 2^k, m in [0.5, 1)
    e = (k - 9 + (m > 0.875).to(k.dtype)).clamp_min(E_MIN)
    return torch.where(amax > 0, e, torch.zeros_like(e)).to(torch.int32)


def quantize_rows(x):
    """x (..., dhp) -> (q (..., dhp) torch.float8_e4m3fn, scale (...) fp32)."""
    xf = x.to(torch.float32)
    e = scale_exponents(xf.abs().amax(dim=-1))
    q = (xf * pow2(-e).unsqueeze(-1)).to(torch.float8_e4m3fn)
    return q, pow2(e)


def dequantize_rows(q, scale):
    """q (..., dhp) e4m3fn, scale (...) -> fp32 values q * scale (exact)."""
    return q.to(torch.float32) * scale.unsqueeze(-1)
