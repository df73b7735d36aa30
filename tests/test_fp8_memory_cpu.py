"""FP8 memory cache, host side (no GPU): which (cache_dtype, memory_cache_dtype) pairs construct, and the format's torch restatement
(acai_omr_amd/fp8.py) - power-of-two row scales, one round-to-nearest-even cast - against its defining properties."""
import inspect

import pytest
import torch

from conftest import VOCAB


def _omr(**kw):
    from acai_omr_amd.models.models import OMRDecoder
    return OMRDecoder(16, VOCAB, num_layers=1, hidden_dim=16, num_heads=2, mlp_dim=8, **kw)


@pytest.mark.parametrize("mdt", [torch.float8_e4m3fn, None, torch.bfloat16])
def test_supported_pairs_construct(mdt):
    from acai_omr_amd.models.kv_caching import CachedTransformerDecoder, CachedTransformerDecoderLayer
    c = _omr().to_cached_version(4, torch.bfloat16, mdt)
    assert c.decoder_blocks.memory_cache_dtype is mdt
    assert c.decoder_blocks.__dict__["_memory_fp8"] == (mdt == torch.float8_e4m3fn)
    assert set(c.state_dict()) == set(_omr().state_dict())   # the FP8 cache is runtime state, as the bf16 one
    _omr(use_caching=True, max_batch_size=2, cache_dtype=torch.bfloat16, memory_cache_dtype=mdt)
    CachedTransformerDecoder(CachedTransformerDecoderLayer(16, 2, 8, batch_first=True), 1, 2, 16, torch.bfloat16, memory_cache_dtype=mdt)
    assert _omr().to_cached_version(4, torch.bfloat16).decoder_blocks.__dict__["_memory_fp8"] is False


@pytest.mark.parametrize("cdt,mdt", [(torch.float32, torch.float8_e4m3fn), (torch.bfloat16, torch.float8_e5m2),
                                     (torch.bfloat16, torch.float8_e4m3fnuz), (torch.bfloat16, torch.float8_e5m2fnuz),
                                     (torch.bfloat16, torch.float16), (torch.float32, torch.bfloat16)])
def test_unsupported_pairs_raise_type_error(cdt, mdt):
    from acai_omr_amd.models.kv_caching import CachedTransformerDecoder, CachedTransformerDecoderLayer
    with pytest.raises(TypeError, match="float8_e4m3fn with cache_dtype=torch.bfloat16"):
        _omr().to_cached_version(4, cdt, mdt)
    with pytest.raises(TypeError):
        CachedTransformerDecoder(CachedTransformerDecoderLayer(16, 2, 8, batch_first=True), 1, 2, 16, cdt, memory_cache_dtype=mdt)


def test_keyword_defaults_on_every_entry_point():
    from acai_omr_amd.inference.vitomr_inference import set_up_omr_inference
    from acai_omr_amd.models.kv_caching import CachedTransformerDecoder
    from acai_omr_amd.models.models import OMRDecoder
    for fn in (OMRDecoder.__init__, OMRDecoder.to_cached_version, CachedTransformerDecoder.__init__, set_up_omr_inference):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "memory_cache_dtype" and p["memory_cache_dtype"].default is None, fn


def _e4m3_values(n, g):
    """n finite e4m3fn values drawn over every bit pattern (NaN excluded), as float32."""
    b = torch.randint(0, 256, (n,), generator=g, dtype=torch.int32).to(torch.uint8)
    b = torch.where((b & 0x7F) == 0x7F, b & 0xFE, b)   # 0x7F / 0xFF are NaN
    return b.view(torch.float8_e4m3fn).float()


def test_round_trip_on_representable_values():
    from acai_omr_amd.fp8 import dequantize_rows, pow2, quantize_rows
    g = torch.Generator().manual_seed(3)
    for e0 in (-20, -9, -1, 0, 3, 17):
        v = _e4m3_values(64 * 64, g).view(64, 64)
        v[:, 5] = 448.0 * torch.where(torch.rand(64, generator=g) < 0.5, -1.0, 1.0)   # amax 448 2^e0: the scale is 2^e0 exactly
        x = v * 2.0 ** e0
        q, s = quantize_rows(x.to(torch.bfloat16))   # every value is bf16-representable (3 mantissa bits)
        assert torch.equal(s, pow2(torch.full((64,), e0)))
        assert torch.equal(q.view(torch.uint8)[:, :5], v.to(torch.float8_e4m3fn).view(torch.uint8)[:, :5])
        assert torch.equal(dequantize_rows(q, s), x)
    # rows whose maximum is below 448 2^e0 get a smaller scale; their values still come back exactly
    v = _e4m3_values(32 * 64, g).view(32, 64) * 2.0 ** -4
    q, s = quantize_rows(v)
    assert torch.equal(dequantize_rows(q, s), v)


def test_all_zero_row_has_unit_scale():
    from acai_omr_amd.fp8 import quantize_rows
    x = torch.zeros(3, 16, dtype=torch.bfloat16)
    x[1, 7] = 1.0
    q, s = quantize_rows(x)
    assert s[0] == 1.0 and s[2] == 1.0 and torch.all(q.view(torch.uint8)[0] == 0)
    assert s[1] == 2.0 ** -8   # 1 * 2^8 = 256 <= 448 < 512


@pytest.mark.parametrize("k", [-30, -9, -1, 0, 1, 8, 40])
def test_amax_at_448_times_power_of_two(k):
    from acai_omr_amd.fp8 import quantize_rows
    amax = 448.0 * 2.0 ** k
    up = torch.nextafter(torch.tensor(amax), torch.tensor(float("inf"))).item()
    x = torch.tensor([[amax, -amax / 3, 0.0, amax / 7], [-amax, 0.5 * amax, 0.0, 0.0], [up, 0.0, 0.0, 0.0]], dtype=torch.float32)
    q, s = quantize_rows(x)
    assert s[0] == 2.0 ** k and s[1] == 2.0 ** k   # amax 2^-e = 448 exactly, the e4m3fn maximum
    assert s[2] == 2.0 ** (k + 1)                  # just above: the next power
    assert q[0, 0].float() == 448.0 and q[1, 0].float() == -448.0
    assert torch.isfinite(q.float()).all()


def test_scale_exponent_floor_and_subnormal_outputs():
    """e stays >= -126 (normal fp32 scales); values far below the row maximum land on e4m3fn subnormals, rounded to nearest even."""
    from acai_omr_amd.fp8 import quantize_rows, scale_exponents
    assert int(scale_exponents(torch.tensor([2.0 ** -130]))[0]) == -126
    x = torch.tensor([[448.0, 2.0 ** -9, 3 * 2.0 ** -10, 2.0 ** -10, 5 * 2.0 ** -11]])
    q, s = quantize_rows(x)
    assert s[0] == 1.0
    # 2^-9 is the smallest subnormal; 1.5 2^-9 is a tie (-> 2^-8, even); 2^-10 is a tie (-> 0, even); 1.25 2^-9 -> 2^-9
    assert q.float()[0, 1:].tolist() == [2.0 ** -9, 2.0 ** -8, 0.0, 2.0 ** -9]
