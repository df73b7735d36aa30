"""Set-up shared by the decode GPU tests (beam, continuous, continuous-sample, speculative, FP8 memory, decode forms, GRPO, edit distance):
the device fixture, the fixture-model and random-decoder builders, the comparison helpers and the GRPO reference step's pieces.  A plain
module: import what a test file uses by name.  Nothing here has a default that changes the model built: call sites pass their sizes."""
import pytest
import torch
from torch.amp import autocast

from conftest import VOCAB, load_golden


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from acai_omr_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def build_vitomr(cfg, sd, dev, cache_dtype, max_batch, memory_cache_dtype=None, grpo=False, transformer_dropout=None):
    """The fixture's model (conftest.load_golden) with its decoder in the cached form (cache_dtype None: uncached); grpo: as a GRPOViTOMR.
    transformer_dropout None keeps OMRDecoder's default."""
    from acai_omr_amd.models.models import FineTuneOMREncoder, GRPOViTOMR, OMRDecoder, TeacherForcedViTOMR
    enc = FineTuneOMREncoder(cfg["P"], cfg["pe_h"], cfg["pe_w"], cfg["ft_depth"], num_layers=cfg["enc_layers"], hidden_dim=cfg["enc_dim"],
                             num_heads=cfg["enc_heads"], mlp_dim=cfg["enc_mlp"])
    drop = {} if transformer_dropout is None else {"transformer_dropout": transformer_dropout}
    dec = OMRDecoder(cfg["max_len"], VOCAB, num_layers=cfg["dec_layers"], hidden_dim=cfg["dec_dim"], num_heads=cfg["dec_heads"], mlp_dim=cfg["dec_mlp"],
                     **drop)
    m = TeacherForcedViTOMR(enc, None, dec, transition_head_dim=cfg["head_dim"])
    m.load_state_dict(sd)
    if grpo:
        d = dec.to_cached_version(max_batch, cache_dtype, memory_cache_dtype) if cache_dtype is not None else dec
        return GRPOViTOMR(m.encoder, m.transition_head, d, m.state_dict()).to(dev)
    if cache_dtype is not None:
        cached = m.decoder.to_cached_version(max_batch, cache_dtype, memory_cache_dtype)
        cached.load_state_dict(m.decoder.state_dict())
        m.decoder = cached
    return m.to(dev).eval()


def _decoder(T, L=2, E=1024, H=16, Fd=4096, seed=5, scale=4.0):
    """Random-init OMRDecoder with perturbed norms and the unembed scaled up (well separated decisions)."""
    from acai_omr_amd.models.models import OMRDecoder
    torch.manual_seed(seed)
    dec = OMRDecoder(T, VOCAB, num_layers=L, hidden_dim=E, num_heads=H, mlp_dim=Fd)
    with torch.no_grad():
        for n, p in dec.named_parameters():
            if "norm" in n:
                p.add_(0.1 * torch.randn_like(p))
        dec.unembed.weight.mul_(scale)
    return dec


def _vit(dec, max_batch, cdt, dev, memory_cache_dtype=None):
    from acai_omr_amd.models.models import ViTOMR
    c = dec.to_cached_version(max_batch, cdt, memory_cache_dtype=memory_cache_dtype)
    c.load_state_dict(dec.state_dict())
    return ViTOMR(None, None, c.to(dev).eval())


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)


def _md(a, b):
    return float((a.cpu().double() - b.cpu().double()).abs().max())


def _memory(m, imgs, bf16):
    with torch.no_grad():
        lat, mask = m.encoder(imgs)
        with autocast(device_type="cuda", dtype=torch.bfloat16, enabled=bf16):
            return m.transition_head(lat), mask


def _vocab():
    toks = [ln.strip() for ln in open(VOCAB) if ln.strip()]
    return len(toks), toks.index("<pad>"), toks.index("<eos>")


# ---- float64 reference formulas (written from the issue's statement of omr_grpo_train.py:240-283) -----------------------------------------
def ref_objective_and_bonus(logits, rollouts, mask, old_lp, adv, eps, num_groups):
    """logits float64 [R, T, V] (requires_grad allowed); entropy terms with p == 0 count 0."""
    V = logits.shape[-1]
    lsm = torch.log_softmax(logits, dim=-1)
    lp = torch.gather(lsm, -1, rollouts[:, 1:logits.shape[1] + 1].unsqueeze(-1)).squeeze(-1)
    ratios = torch.exp(lp - old_lp[:, 1:logits.shape[1] + 1].double())
    a = adv.double().unsqueeze(1)
    unclipped = (ratios * a).masked_fill(mask, 0)
    clipped = (torch.clip(ratios, min=1 - eps, max=1 + eps) * a).masked_fill(mask, 0)
    lens = (~mask).sum(dim=-1)
    obj = (torch.minimum(unclipped, clipped).sum(-1) / lens).sum() / num_groups
    p = torch.softmax(logits, dim=-1)
    ent = torch.where(p > 0, -p * lsm, torch.zeros_like(p)).sum(-1).masked_fill(mask, 0)
    bonus = (ent.sum(-1) / lens).mean() / float(torch.log(torch.tensor(V)))
    return obj, bonus


def _models(dev):
    """The old (bf16 cache, one row per rollout) / theta (uncached, training) policy pair on the vitomr_dh64b fixture, three rollouts per image."""
    fx = load_golden("vitomr_dh64b")
    cfg, sd = fx["cfg"], fx["state_dict"]
    G = 3
    old = build_vitomr(cfg, sd, dev, torch.bfloat16, len(fx["imgs"]) * G, grpo=True, transformer_dropout=0.0).eval()
    theta = build_vitomr(cfg, sd, dev, None, None, grpo=True, transformer_dropout=0.0).train()
    return fx, old, theta, G, cfg


def _reward_fn(rollouts, rollout_mask, target_lmx_seqs, batch):
    from acai_omr_amd.train import grpo as G
    _, pad, _ = _vocab()
    r = G.calc_token_f1(rollouts, target_lmx_seqs.to(rollouts.device), pad) + 0.05 * rollout_mask.sum(-1).float()
    return r.view(len(batch), -1)
