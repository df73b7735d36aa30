"""The sampled continuous-batching surface, as far as it can be checked without a device: the C ABI declaration (header, ctypes signature),
and the Python entry points' parameters and defaults (every parameter the feature adds has a default, so existing callers are untouched)."""
import ctypes
import inspect
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))


def test_header_and_ctypes_signature_agree():
    from acai_omr_amd import _lib
    hdr = open(os.path.join(HERE, "..", "include", "acai_omr_hip.h")).read()
    m = re.search(r"int acai_decode_slot_sample_step\(([^;]*)\);", hdr)
    assert m, "acai_decode_slot_sample_step is not declared in the header"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["d", "sl", "uniforms", "ld_uniforms", "urow", "top_k", "temperature", "stream"]
    res, args = _lib._SIGNATURES["acai_decode_slot_sample_step"]
    assert res is ctypes.c_int and len(args) == len(params)
    assert args[3] is ctypes.c_int and args[5] is ctypes.c_int and args[6] is ctypes.c_float
    # AcaiSlots keeps its layout: urow and the uniforms travel as arguments
    assert [f for f, _ in _lib.AcaiSlots._fields_] == ["t", "first", "cap", "rows", "pad_"]


def _defaults(fn):
    return {n: p.default for n, p in inspect.signature(fn).parameters.items()}


def test_python_entry_points():
    from acai_omr_amd.engine import DecodeEngine
    from acai_omr_amd.models.models import GRPOViTOMR
    from acai_omr_amd.train import grpo as G
    d = _defaults(DecodeEngine.continuous)
    assert d["sample"] is None and d["uniforms"] is None and d["group"] == 1
    assert list(d)[:8] == ["self", "mem32", "memb", "lens", "caps", "slots", "poll", "use_graph"] and d["poll"] == 16 and d["use_graph"] is True
    d = _defaults(GRPOViTOMR.cached_continuous_rollout_policy)
    assert list(d) == ["self", "img_latent", "latent_attention_mask", "max_actions", "top_k", "temperature", "slots", "group_size", "uniforms"]
    assert (d["max_actions"], d["top_k"], d["temperature"], d["slots"], d["group_size"], d["uniforms"]) == (768, 50, 1.2, None, 1, None)
    d = _defaults(G.grpo_update)
    assert d["rollout_slots"] is None and d["uniforms"] is None
    sig = inspect.signature(G.validation_loop)
    assert list(sig.parameters)[:7] == ["dataloader", "policy_theta", "reward_config", "rollout_config", "ce_loss_fn", "pad_idx", "device"]
    for n in ("reward_fn", "slots", "uniforms_fn"):
        assert sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[n].default is None
