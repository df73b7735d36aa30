"""BASELINE.json configurations AT SIZE on the GPU, in their stated arithmetic, against the CPU oracle (`-m gpu`):

  config 2  MAE forward + MAELoss + backward under autocast(bf16), full-size model, a 512 x 2048 image       (pre_train.py:54-62 step shape)
  config 3  ScheduledSamplingViTOMR.forward_train + OMRCELoss + backward under autocast(bf16), T = 512        (omr_teacher_force_train.py:113-138)
  config 4  inference() on the ragged batch of 8 systems 256 x 1024 ... 768 x 3072 (N = 1024 ... 9216)        (models.py:600-615)

plus the reference-pinned fixtures added in round 2 (GRPO rollouts, PE interpolation in the training path, label-smoothed CE) and the
host-side behaviours the advisor flagged (deep copies after a decode, STEP events on a flush boundary, per-tensor AdamW step counts).

bf16 bars: the HIP path rounds where autocast rounds, so forward values agree with the oracle's autocast restatement to bf16 resolution;
gradients of a 20-layer bf16 network differ by accumulated bf16 rounding of the backward GEMMs (the oracle's backward is fp32 through
straight-through casts), so they are held to a relative max-norm error and a cosine, both stated per test."""
import copy
import math
import os

import pytest
import torch
from torch.amp import autocast

from conftest import VOCAB, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from acai_omr_amd import _lib
    _lib.lib()
    return "cuda"


def md(a, b):
    return float((a.detach().float().cpu() - b.detach().float().cpu()).abs().max())


def relerr(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def cosine(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a @ b) / (a.norm() * b.norm()).clamp(min=1e-300))


def _threads():
    try:
        n = len(os.sched_getaffinity(0))
    except Exception:
        n = os.cpu_count() or 8
    torch.set_num_threads(max(1, min(n, 16)))


def _perturb(model, unembed_scale=None):
    """Default init leaves LayerNorm at identity and logits tiny: perturb so that parity is not vacuous."""
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "norm" in n:
                p.add_(0.1 * torch.randn_like(p))
        if unembed_scale is not None:
            model.decoder.unembed.weight.mul_(unembed_scale)


# ---- config 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mae_small", "mae_debug_ckpt"])
def test_config2_mae_bf16_step_golden_sizes_vs_oracle(dev, name):
    """MAE fwd + loss + bwd under autocast(bf16) on the golden fixtures' weights / images / injected noise against autograd through the
    oracle's bf16 restatement: pred, loss and EVERY gradient the fp32 golden test checks."""
    import oracle.vitomr_oracle as O
    from acai_omr_amd.models.models import MAE, MAELoss
    fx = load_golden(name)
    cfg = fx["cfg"]
    sd = {k: v.clone().requires_grad_(True) for k, v in fx["state_dict"].items()}
    batch = list(zip(fx["imgs"], fx["tgts"]))
    eh, dh = cfg["enc_kwargs"]["num_heads"], cfg["dec_kwargs"]["num_heads"]
    pred_o, lm_o, tgt_o, lens = O.mae_forward(batch, fx["noises"], sd, cfg["P"], cfg["mask_ratio"], eh, dh, prec="bf16")
    loss_o = O.mae_loss(pred_o, lm_o, tgt_o)
    loss_o.backward()
    mae = MAE(cfg["mask_ratio"], cfg["P"], cfg["pe_h"], cfg["pe_w"], encoder_hidden_dim=cfg["enc_dim"], decoder_hidden_dim=cfg["dec_dim"],
              encoder_kwargs=cfg["enc_kwargs"], decoder_kwargs=cfg["dec_kwargs"])
    mae.load_state_dict(fx["state_dict"])
    mae = mae.to(dev).train()
    with autocast(device_type="cuda", dtype=torch.bfloat16):
        pred, loss_mask, target, lens_h = mae.forward_packed(batch, noises=fx["noises"])
    assert lens_h == lens and torch.equal(loss_mask.cpu(), lm_o)
    assert md(pred, pred_o) < 0.05 * max(1.0, float(pred_o.abs().max()))        # bf16 resolution of O(1) values through 4 layers
    loss = MAELoss()(pred, loss_mask, target)
    assert abs(float(loss) - float(loss_o)) < 2e-2 * max(1.0, abs(float(loss_o)))
    loss.backward()
    params = dict(mae.named_parameters())
    for n in fx["grads"]:
        g, go = params[n].grad, sd[n].grad
        assert relerr(g, go) < 0.08 and cosine(g, go) > 0.995, (n, relerr(g, go), cosine(g, go))


def test_config2_mae_bf16_step_at_size_vs_oracle(dev):
    """BASELINE config 2 in its stated arithmetic at the stated image size: the FULL-SIZE MAE on one 512 x 2048 image (N = 4096, 1024 kept;
    every GEMM / attention shape of the benchmarked step, d_h = 64 encoder and d_h = 32 decoder) under autocast(bf16): loss and three named
    gradients against autograd through the CPU oracle's bf16 restatement."""
    import oracle.vitomr_oracle as O
    from acai_omr_amd.config import MASK_RATIO, PATCH_SIZE, PE_MAX_HEIGHT, PE_MAX_WIDTH
    from acai_omr_amd.models.models import MAE, MAELoss
    _threads()
    torch.manual_seed(2)
    mae = MAE(MASK_RATIO, PATCH_SIZE, PE_MAX_HEIGHT, PE_MAX_WIDTH)
    _perturb(mae)
    g = torch.Generator().manual_seed(3)
    img = torch.rand(1, 512, 2048, generator=g)
    noise = [torch.rand(4096, generator=g)]
    names = ("decoder_unembed.weight", "decoder.decoder_blocks.layers.7.linear1.weight", "encoder.encoder_blocks.layers.0.self_attn.in_proj_weight",
             "mask_token", "encoder.projection.weight")
    sd = {k: v.detach().clone().requires_grad_(k in names) for k, v in mae.state_dict().items()}
    pred_o, lm_o, tgt_o, lens = O.mae_forward([(img, img)], noise, sd, PATCH_SIZE, MASK_RATIO, 12, 16, prec="bf16")
    loss_o = O.mae_loss(pred_o, lm_o, tgt_o)
    loss_o.backward()
    mae = mae.to(dev).train()
    with autocast(device_type="cuda", dtype=torch.bfloat16):
        pred, loss_mask, target, _ = mae.forward_packed([(img.to(dev), img.to(dev))], noises=noise)
    loss = MAELoss()(pred, loss_mask, target)
    loss.backward()
    assert torch.equal(loss_mask.cpu(), lm_o)
    e_pred = md(pred, pred_o)
    print(f"config2 at size: loss {float(loss):.5f} oracle {float(loss_o):.5f}  pred max|d| {e_pred:.3e}")
    assert abs(float(loss) - float(loss_o)) < 2e-3 * max(1.0, abs(float(loss_o)))     # measured 1e-5
    assert e_pred < 0.06 * max(1.0, float(pred_o.abs().max()))
    params = dict(mae.named_parameters())
    for n in names:
        r, c = relerr(params[n].grad, sd[n].grad), cosine(params[n].grad, sd[n].grad)
        print(f"  grad {n}: rel max err {r:.3e} cosine {c:.6f}")
        assert r < 2e-2 and c > 0.9999, (n, r, c)            # measured 6e-4 ... 3e-3, cosine 0.999998


# ---- config 3 ------------------------------------------------------------------------------------------------------------------------
def test_config3_teacher_forced_bf16_step_at_size_vs_oracle(dev):
    """BASELINE config 3's step in its arithmetic (bf16 autocast forward + CE, backward outside autocast) at its sequence sizes: the FULL-SIZE
    ScheduledSamplingViTOMR.forward_train with tf_prob = 1 (two decoder passes, the second on the gold embeddings = the teacher-forced
    step) on a 512 x 2048 system (N = 4096) and a 256 x 1024 one (ragged memory), T = 512 LMX tokens each: loss and named gradients of
    encoder, head and decoder against autograd through the oracle's bf16 restatement."""
    import oracle.vitomr_oracle as O
    from acai_omr_amd.config import ENCODER_FINE_TUNE_DEPTH, MAX_LMX_SEQ_LEN, NUM_DECODER_LAYERS, PATCH_SIZE, PE_MAX_HEIGHT, PE_MAX_WIDTH
    from acai_omr_amd.models.models import FineTuneOMREncoder, OMRCELoss, OMRDecoder, ScheduledSamplingViTOMR
    _threads()
    torch.manual_seed(4)
    enc = FineTuneOMREncoder(PATCH_SIZE, PE_MAX_HEIGHT, PE_MAX_WIDTH, ENCODER_FINE_TUNE_DEPTH, transformer_dropout=0.0)
    dec = OMRDecoder(MAX_LMX_SEQ_LEN, VOCAB, num_layers=NUM_DECODER_LAYERS, transformer_dropout=0.0)
    m = ScheduledSamplingViTOMR(enc, None, dec, transition_head_dropout=0.0)
    _perturb(m, unembed_scale=3.0)
    g = torch.Generator().manual_seed(5)
    imgs = [torch.rand(1, 512, 2048, generator=g), torch.rand(1, 256, 1024, generator=g)]
    T = 512
    lmx = [torch.cat([torch.tensor([0]), torch.randint(3, 227, (T - 1,), generator=g), torch.tensor([2])]),
           torch.cat([torch.tensor([0]), torch.randint(3, 227, (T - 140,), generator=g), torch.tensor([2])])]
    names = ("decoder.unembed.weight", "decoder.decoder_blocks.layers.0.multihead_attn.in_proj_weight", "decoder.decoder_blocks.layers.11.linear2.weight",
             "transition_head.0.weight", "encoder.fine_tune_blocks.layers.11.linear1.weight", "encoder.fine_tune_blocks.layers.0.self_attn.in_proj_weight")
    sd = {k: v.detach().clone().requires_grad_(k in names) for k, v in m.state_dict().items()}
    pred_o, tgt_o = O.teacher_forced_forward(list(zip(imgs, lmx)), sd, 12, 16, PATCH_SIZE, "bf16")
    loss_o = O.ce_loss(pred_o, tgt_o, 1)
    loss_o.backward()
    m = m.to(dev).train()
    batch = [(im.to(dev), sq.to(dev)) for im, sq in zip(imgs, lmx)]
    with autocast(device_type="cuda", dtype=torch.bfloat16):
        pred, tgt = m.forward_train(batch, 1.0, 0.5, False)
        loss = OMRCELoss(m.decoder.pad_idx)(pred, tgt)
    loss.backward()
    assert torch.equal(tgt.cpu(), tgt_o) and pred.shape == (2, T, 227)
    valid = tgt_o != 1
    e_pred = md(pred.float().cpu()[valid], pred_o.detach()[valid])
    print(f"config3 at size: loss {float(loss):.5f} oracle {float(loss_o):.5f}  logits max|d| {e_pred:.3e} (|logit| max {float(pred_o.abs().max()):.2f})")
    assert abs(float(loss) - float(loss_o)) < 2e-3 * max(1.0, abs(float(loss_o)))     # measured 3e-4
    assert e_pred < 0.05 * max(1.0, float(pred_o.abs().max()))
    params = dict(m.named_parameters())
    for n in names:
        r, c = relerr(params[n].grad, sd[n].grad), cosine(params[n].grad, sd[n].grad)
        print(f"  grad {n}: rel max err {r:.3e} cosine {c:.6f}")
        assert r < 2e-2 and c > 0.9999, (n, r, c)            # measured 3e-3 ... 5e-3, cosine 0.999996


def test_config3_scheduled_sampling_bf16_step_at_size_vs_oracle(dev):
    """Config 3's step as the reference trains it for 35 of its 40 fine-tune epochs and as bench.py's tf_step times it: the FULL-SIZE
    ScheduledSamplingViTOMR.forward_train at tf_prob = 0.7, tau = 0.5 (soft) under autocast(bf16), one 256 x 1024 system, T = 371, with
    injected draws - so the expected-embedding branch carries gradient: MatmulKNFn's dW and d(distr) at E = 1024, V = 227, and the second
    contributions of every decoder parameter.  Against autograd through the oracle's bf16 scheduled_sampling_forward on the same weights and
    draws, with the bars and gradient names of test_config3_teacher_forced_bf16_step_at_size_vs_oracle plus the embedding table.  The bf16
    target is the CPU-autocast restatement (Gumbel-softmax rounded to bf16 where CPU autocast rounds it), not CUDA autocast's fp32 softmax."""
    import oracle.vitomr_oracle as O
    from acai_omr_amd.config import ENCODER_FINE_TUNE_DEPTH, MAX_LMX_SEQ_LEN, NUM_DECODER_LAYERS, PATCH_SIZE, PE_MAX_HEIGHT, PE_MAX_WIDTH
    from acai_omr_amd.models.models import FineTuneOMREncoder, OMRCELoss, OMRDecoder, ScheduledSamplingViTOMR
    _threads()
    torch.manual_seed(4)
    enc = FineTuneOMREncoder(PATCH_SIZE, PE_MAX_HEIGHT, PE_MAX_WIDTH, ENCODER_FINE_TUNE_DEPTH, transformer_dropout=0.0)
    dec = OMRDecoder(MAX_LMX_SEQ_LEN, VOCAB, num_layers=NUM_DECODER_LAYERS, transformer_dropout=0.0)
    m = ScheduledSamplingViTOMR(enc, None, dec, transition_head_dropout=0.0)
    _perturb(m, unembed_scale=3.0)
    g = torch.Generator().manual_seed(6)
    imgs = [torch.rand(1, 256, 1024, generator=g)]
    lmx = [torch.cat([torch.tensor([0]), torch.randint(3, 227, (370,), generator=g), torch.tensor([2])])]
    T = 371
    noise = dict(uniform=torch.rand(1, T, generator=g), exponential=torch.empty(1, T, 227, dtype=torch.bfloat16).exponential_(generator=g))
    names = ("decoder.unembed.weight", "decoder.decoder_blocks.layers.0.multihead_attn.in_proj_weight", "decoder.decoder_blocks.layers.11.linear2.weight",
             "transition_head.0.weight", "encoder.fine_tune_blocks.layers.11.linear1.weight", "encoder.fine_tune_blocks.layers.0.self_attn.in_proj_weight",
             "decoder.vocab_embedding.weight")
    sd = {k: v.detach().clone().requires_grad_(k in names) for k, v in m.state_dict().items()}
    pred_o, tgt_o = O.scheduled_sampling_forward(list(zip(imgs, lmx)), sd, 12, 16, PATCH_SIZE, "bf16", 0.7, 0.5, False, noise)
    loss_o = O.ce_loss(pred_o, tgt_o, 1)
    loss_o.backward()
    m = m.to(dev).train()
    batch = [(im.to(dev), sq.to(dev)) for im, sq in zip(imgs, lmx)]
    with autocast(device_type="cuda", dtype=torch.bfloat16):
        pred, tgt = m.forward_train(batch, 0.7, 0.5, False, noise=noise)
        loss = OMRCELoss(m.decoder.pad_idx)(pred, tgt)
    loss.backward()
    assert torch.equal(tgt.cpu(), tgt_o) and pred.shape == (1, T, 227)
    assert 0 < int((noise["uniform"][0, 1:] < 0.3).sum()) < T - 1
    valid = tgt_o != 1
    e_pred = md(pred.float().cpu()[valid], pred_o.detach()[valid])
    print(f"config3 scheduled sampling at size: loss {float(loss):.5f} oracle {float(loss_o):.5f}  logits max|d| {e_pred:.3e} "
          f"(|logit| max {float(pred_o.abs().max()):.2f})")
    assert abs(float(loss) - float(loss_o)) < 2e-3 * max(1.0, abs(float(loss_o)))     # measured 1.2e-4 (loss 6.66)
    assert e_pred < 0.05 * max(1.0, float(pred_o.abs().max()))                        # measured 5.1e-2 (|logit| max 5.6)
    params = dict(m.named_parameters())
    for n in names:
        r, c = relerr(params[n].grad, sd[n].grad), cosine(params[n].grad, sd[n].grad)
        print(f"  grad {n}: rel max err {r:.3e} cosine {c:.6f}")
        assert r < 2e-2 and c > 0.9999, (n, r, c)            # measured 3.9e-3 ... 5.7e-3, cosine >= 0.999983 (CPU oracle ~10 s)

# ---- configs 2 and 3 at their BATCH sizes: a size-independent property instead of the (too slow) CPU oracle ---------------------------------
def _grads(model, names):
    ps = dict(model.named_parameters())
    return {n: ps[n].grad.detach().float().clone() for n in names}


def test_config2_full_batch_of_32_equals_its_two_halves(dev):
    """BASELINE config 2 at its batch size (32 x 512 x 2048, bf16 autocast, full-size MAE): the at-size test above runs ONE image against the
    oracle; the batch-level mechanisms (131072-row decoder GEMMs in their persistent ping-pong forms, 32-sequence attention grids, the loss's
    batch-global denominator) are pinned here by linearity - the gradient of the batch-of-32 loss equals the mean of the two half-batch
    gradients (every image masks the same number of patches, so the halves weigh equally), and the loss likewise."""
    from acai_omr_amd.config import MASK_RATIO, PATCH_SIZE, PE_MAX_HEIGHT, PE_MAX_WIDTH
    from acai_omr_amd.models.models import MAE, MAELoss
    torch.manual_seed(12)
    mae = MAE(MASK_RATIO, PATCH_SIZE, PE_MAX_HEIGHT, PE_MAX_WIDTH)
    _perturb(mae)
    mae = mae.to(dev).train()
    g = torch.Generator().manual_seed(13)
    imgs = [torch.rand(1, 512, 2048, generator=g).to(dev) for _ in range(32)]
    noise = [torch.rand(4096, generator=g) for _ in range(32)]
    names = ("decoder_unembed.weight", "decoder.decoder_blocks.layers.7.linear1.weight", "decoder.decoder_blocks.layers.0.self_attn.in_proj_weight",
             "encoder.encoder_blocks.layers.0.self_attn.in_proj_weight", "mask_token", "encoder.projection.weight")

    def step(lo, hi):
        mae.zero_grad(set_to_none=True)
        with autocast(device_type="cuda", dtype=torch.bfloat16):
            pred, loss_mask, target, _ = mae.forward_packed([(im, im) for im in imgs[lo:hi]], noises=noise[lo:hi])
        loss = MAELoss()(pred, loss_mask, target)
        loss.backward()
        return float(loss.detach()), _grads(mae, names)

    l_full, g_full = step(0, 32)
    l_a, g_a = step(0, 16)
    l_b, g_b = step(16, 32)
    assert abs(l_full - 0.5 * (l_a + l_b)) < 2e-4 * max(1.0, abs(l_full)), (l_full, l_a, l_b)
    for n in names:
        ref = 0.5 * (g_a[n] + g_b[n])
        r, c = relerr(g_full[n], ref), cosine(g_full[n], ref)
        print(f"config2 batch 32 vs 2 x 16: grad {n}: rel max err {r:.3e} cosine {c:.6f}")
        assert r < 1e-2 and c > 0.99995, (n, r, c)           # measured 3e-7 ... 2e-6 (an image's rows never meet another image's)


def test_config3_full_batch_of_16_equals_its_two_halves(dev):
    """BASELINE config 3 at its batch size (16 systems of 512 x 2048 with 512 LMX tokens + <bos>: the 16 x 513 = 8208-row decoder stream with
    its one-row tails - GEMM tiles of 8208 rows, the 513th token's attention tail kernels, the 65536-token encoder stream), full-size
    ScheduledSamplingViTOMR.forward_train(tf_prob = 1) under autocast(bf16): the gradient of the batch loss equals the token-count-weighted
    mean of the two half-batch gradients (4104-row streams: different tile counts, ragged tails and split-K factors for the same arithmetic)."""
    from acai_omr_amd.config import ENCODER_FINE_TUNE_DEPTH, MAX_LMX_SEQ_LEN, NUM_DECODER_LAYERS, PATCH_SIZE, PE_MAX_HEIGHT, PE_MAX_WIDTH
    from acai_omr_amd.models.models import FineTuneOMREncoder, OMRCELoss, OMRDecoder, ScheduledSamplingViTOMR
    torch.manual_seed(14)
    enc = FineTuneOMREncoder(PATCH_SIZE, PE_MAX_HEIGHT, PE_MAX_WIDTH, ENCODER_FINE_TUNE_DEPTH, transformer_dropout=0.0)
    dec = OMRDecoder(MAX_LMX_SEQ_LEN, VOCAB, num_layers=NUM_DECODER_LAYERS, transformer_dropout=0.0)
    m = ScheduledSamplingViTOMR(enc, None, dec, transition_head_dropout=0.0)
    _perturb(m, unembed_scale=3.0)
    m = m.to(dev).train()
    g = torch.Generator().manual_seed(15)
    T = 512
    batch = []
    for i in range(16):
        n_tok = T - 1 if i % 5 else T - 1 - 37 * (i // 5 + 1)        # mostly full-length sequences, a few shorter ones (pad columns in the batch)
        batch.append((torch.rand(1, 512, 2048, generator=g).to(dev),
                      torch.cat([torch.tensor([0]), torch.randint(3, 227, (n_tok,), generator=g), torch.tensor([2])]).to(dev)))
    names = ("decoder.unembed.weight", "decoder.decoder_blocks.layers.0.multihead_attn.in_proj_weight", "decoder.decoder_blocks.layers.11.linear2.weight",
             "decoder.decoder_blocks.layers.5.self_attn.in_proj_weight", "transition_head.0.weight", "encoder.fine_tune_blocks.layers.11.linear1.weight",
             "encoder.fine_tune_blocks.layers.0.self_attn.in_proj_weight")

    def step(lo, hi):
        m.zero_grad(set_to_none=True)
        with autocast(device_type="cuda", dtype=torch.bfloat16):
            pred, tgt = m.forward_train(batch[lo:hi], 1.0, 0.5, False)
            loss = OMRCELoss(m.decoder.pad_idx)(pred, tgt)
        loss.backward()
        return float(loss.detach()), int((tgt != m.decoder.pad_idx).sum()), _grads(m, names)

    l_full, n_full, g_full = step(0, 16)
    l_a, n_a, g_a = step(0, 8)
    l_b, n_b, g_b = step(8, 16)
    assert n_full == n_a + n_b
    wa, wb = n_a / n_full, n_b / n_full
    assert abs(l_full - (wa * l_a + wb * l_b)) < 5e-4 * max(1.0, abs(l_full)), (l_full, l_a, l_b)
    for n in names:
        ref = wa * g_a[n] + wb * g_b[n]
        r, c = relerr(g_full[n], ref), cosine(g_full[n], ref)
        print(f"config3 batch 16 vs 2 x 8: grad {n}: rel max err {r:.3e} cosine {c:.6f}")
        assert r < 1e-2 and c > 0.99995, (n, r, c)           # measured 1e-4 ... 9e-4 (bf16 roundings of differently split sums), cosine 1.000000


# ---- config 5: the single-rank arithmetic of its largest ragged shard shapes ------------------------------------------------------------
def test_config5_shard_shapes_mae_bf16_step_vs_oracle(dev):
    """BASELINE config 5 deals 768 x 3072 images (N = 9216 patches) to every rank; no other test ran a training BACKWARD beyond N = 4096.
    Full WIDTHS of the MAE (768-wide d_h = 64 encoder on the 2304 / 256 kept tokens, 512-wide d_h = 32 decoder over all 9216 / 1024 tokens,
    i.e. the two-blocks-per-wave backward over 9216 keys), a ragged pair 768 x 3072 + 256 x 1024, two layers per stack (the oracle's autograd
    keeps every N x N probability tensor: 5.4 GB per decoder layer at N = 9216): loss and named gradients against autograd through the CPU
    oracle's bf16 restatement, the bars of the config-2 test."""
    import oracle.vitomr_oracle as O
    from acai_omr_amd.config import MASK_RATIO, PATCH_SIZE, PE_MAX_HEIGHT, PE_MAX_WIDTH
    from acai_omr_amd.models.models import MAE, MAELoss
    _threads()
    torch.manual_seed(12)
    mae = MAE(MASK_RATIO, PATCH_SIZE, PE_MAX_HEIGHT, PE_MAX_WIDTH, encoder_kwargs=dict(num_layers=2), decoder_kwargs=dict(num_layers=2))
    _perturb(mae)
    g = torch.Generator().manual_seed(13)
    imgs = [torch.rand(1, 768, 3072, generator=g), torch.rand(1, 256, 1024, generator=g)]
    noise = [torch.rand(9216, generator=g), torch.rand(1024, generator=g)]
    names = ("decoder_unembed.weight", "decoder.decoder_blocks.layers.0.self_attn.in_proj_weight", "decoder.decoder_blocks.layers.1.linear1.weight",
             "encoder.encoder_blocks.layers.0.self_attn.in_proj_weight", "mask_token", "encoder.projection.weight")
    sd = {k: v.detach().clone().requires_grad_(k in names) for k, v in mae.state_dict().items()}
    pred_o, lm_o, tgt_o, lens = O.mae_forward([(im, im) for im in imgs], noise, sd, PATCH_SIZE, MASK_RATIO, 12, 16, prec="bf16")
    loss_o = O.mae_loss(pred_o, lm_o, tgt_o)
    loss_o.backward()
    mae = mae.to(dev).train()
    with autocast(device_type="cuda", dtype=torch.bfloat16):
        pred, loss_mask, target, _ = mae.forward_packed([(im.to(dev), im.to(dev)) for im in imgs], noises=noise)
    loss = MAELoss()(pred, loss_mask, target)
    loss.backward()
    assert torch.equal(loss_mask.cpu(), lm_o)
    e_pred = md(pred, pred_o)
    print(f"config5 shard shapes (MAE): loss {float(loss):.5f} oracle {float(loss_o):.5f}  pred max|d| {e_pred:.3e}")
    assert abs(float(loss) - float(loss_o)) < 2e-3 * max(1.0, abs(float(loss_o)))
    assert e_pred < 0.06 * max(1.0, float(pred_o.abs().max()))
    params = dict(mae.named_parameters())
    for n in names:
        r, c = relerr(params[n].grad, sd[n].grad), cosine(params[n].grad, sd[n].grad)
        print(f"  grad {n}: rel max err {r:.3e} cosine {c:.6f}")
        assert r < 2e-2 and c > 0.9999, (n, r, c)


def test_config5_shard_shapes_teacher_forced_bf16_step_vs_oracle(dev):
    """The teacher-forced half of config 5 at the same ragged pair: forward_train(tf_prob = 1) under autocast(bf16) with the encoder's d_h = 64
    self-attention over 9216 tokens (forward: the one-wave-per-SIMD kernel with its 128-query tail launch for the 1024-token image; backward:
    9216 keys) and the decoder's cross attention 513 queries x 9216 / 1024 keys; full widths, two encoder and two decoder layers."""
    import oracle.vitomr_oracle as O
    from acai_omr_amd.config import MAX_LMX_SEQ_LEN, PATCH_SIZE, PE_MAX_HEIGHT, PE_MAX_WIDTH
    from acai_omr_amd.models.models import FineTuneOMREncoder, OMRCELoss, OMRDecoder, ScheduledSamplingViTOMR
    _threads()
    torch.manual_seed(14)
    enc = FineTuneOMREncoder(PATCH_SIZE, PE_MAX_HEIGHT, PE_MAX_WIDTH, 2, num_layers=2, transformer_dropout=0.0)
    dec = OMRDecoder(MAX_LMX_SEQ_LEN, VOCAB, num_layers=2, transformer_dropout=0.0)
    m = ScheduledSamplingViTOMR(enc, None, dec, transition_head_dropout=0.0)
    _perturb(m, unembed_scale=3.0)
    g = torch.Generator().manual_seed(15)
    imgs = [torch.rand(1, 768, 3072, generator=g), torch.rand(1, 256, 1024, generator=g)]
    T = 512
    lmx = [torch.cat([torch.tensor([0]), torch.randint(3, 227, (T - 1,), generator=g), torch.tensor([2])]),
           torch.cat([torch.tensor([0]), torch.randint(3, 227, (T - 200,), generator=g), torch.tensor([2])])]
    names = ("decoder.unembed.weight", "decoder.decoder_blocks.layers.0.multihead_attn.in_proj_weight", "decoder.decoder_blocks.layers.1.linear2.weight",
             "transition_head.0.weight", "encoder.fine_tune_blocks.layers.1.linear1.weight", "encoder.fine_tune_blocks.layers.0.self_attn.in_proj_weight")
    sd = {k: v.detach().clone().requires_grad_(k in names) for k, v in m.state_dict().items()}
    pred_o, tgt_o = O.teacher_forced_forward(list(zip(imgs, lmx)), sd, 12, 16, PATCH_SIZE, "bf16")
    loss_o = O.ce_loss(pred_o, tgt_o, 1)
    loss_o.backward()
    m = m.to(dev).train()
    batch = [(im.to(dev), sq.to(dev)) for im, sq in zip(imgs, lmx)]
    with autocast(device_type="cuda", dtype=torch.bfloat16):
        pred, tgt = m.forward_train(batch, 1.0, 0.5, False)
        loss = OMRCELoss(m.decoder.pad_idx)(pred, tgt)
    loss.backward()
    assert torch.equal(tgt.cpu(), tgt_o)
    valid = tgt_o != 1
    e_pred = md(pred.float().cpu()[valid], pred_o.detach()[valid])
    print(f"config5 shard shapes (TF): loss {float(loss):.5f} oracle {float(loss_o):.5f}  logits max|d| {e_pred:.3e}")
    assert abs(float(loss) - float(loss_o)) < 2e-3 * max(1.0, abs(float(loss_o)))
    assert e_pred < 0.05 * max(1.0, float(pred_o.abs().max()))
    params = dict(m.named_parameters())
    for n in names:
        r, c = relerr(params[n].grad, sd[n].grad), cosine(params[n].grad, sd[n].grad)
        print(f"  grad {n}: rel max err {r:.3e} cosine {c:.6f}")
        assert r < 2e-2 and c > 0.9999, (n, r, c)


@pytest.mark.parametrize("name", ["tf_small", "tf_dh64"])
def test_config3_teacher_forced_bf16_golden_sizes_vs_oracle(dev, name):
    """The same step on the golden fixtures' weights under autocast(bf16): logits, loss and every gradient the fp32 golden test checks."""
    import oracle.vitomr_oracle as O
    from acai_omr_amd.models.models import FineTuneOMREncoder, OMRCELoss, OMRDecoder, ScheduledSamplingViTOMR
    fx = load_golden(name)
    cfg = fx["cfg"]
    sd = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in fx["state_dict"].items()}
    batch = list(zip(fx["imgs"], fx["lmx"]))
    pred_o, tgt_o = O.teacher_forced_forward(batch, sd, cfg["enc_heads"], cfg["dec_heads"], cfg["P"], "bf16")
    loss_o = O.ce_loss(pred_o, tgt_o, 1)
    loss_o.backward()
    enc = FineTuneOMREncoder(cfg["P"], cfg["pe_h"], cfg["pe_w"], cfg["ft_depth"], num_layers=cfg["enc_layers"], hidden_dim=cfg["enc_dim"],
                             num_heads=cfg["enc_heads"], mlp_dim=cfg["enc_mlp"], transformer_dropout=0.0)
    dec = OMRDecoder(cfg["max_len"], VOCAB, num_layers=cfg["dec_layers"], hidden_dim=cfg["dec_dim"], num_heads=cfg["dec_heads"], mlp_dim=cfg["dec_mlp"],
                     transformer_dropout=0.0)
    m = ScheduledSamplingViTOMR(enc, None, dec, transition_head_dim=cfg["head_dim"], transition_head_dropout=0.0)
    m.load_state_dict(fx["state_dict"])
    m = m.to(dev).train()
    with autocast(device_type="cuda", dtype=torch.bfloat16):
        pred, tgt = m.forward_train(batch, 1.0, 0.5, False)
        loss = OMRCELoss(1)(pred, tgt)
    loss.backward()
    valid = tgt_o != 1
    assert md(pred.float().cpu()[valid], pred_o.detach()[valid]) < 0.05 * max(1.0, float(pred_o.abs().max()))
    assert abs(float(loss) - float(loss_o)) < 2e-2
    params = dict(m.named_parameters())
    for n in fx["grads"]:
        g, go = params[n].grad, sd[n].grad
        assert relerr(g, go) < 0.08 and cosine(g, go) > 0.995, (n, relerr(g, go), cosine(g, go))


# ---- config 4 ------------------------------------------------------------------------------------------------------------------------
CONFIG4_SHAPES = [(256, 1024), (256, 2048), (384, 1536), (512, 2048), (512, 3072), (640, 2560), (768, 2304), (768, 3072)]


def _config4_model(dev, cache_dtype):
    from acai_omr_amd.inference.vitomr_inference import set_up_omr_inference
    torch.manual_seed(6)
    vitomr, _ = set_up_omr_inference(VOCAB, max_batch_size=8, cache_dtype=cache_dtype, device="cpu")
    _perturb(vitomr, unembed_scale=6.0)
    with torch.no_grad():
        vitomr.decoder.unembed.bias[2] = -1.0e4      # never <eos>: every row decodes the full length
    sd = {k: v.detach().clone() for k, v in vitomr.state_dict().items()}
    g = torch.Generator().manual_seed(0)
    imgs = [torch.rand(1, h, w, generator=g) for h, w in CONFIG4_SHAPES]
    return vitomr.to(dev).eval(), sd, imgs


def test_config4_ragged_batch_of_8_vs_oracle_on_the_extremes(dev):
    """BASELINE config 4 through `inference()` (encoder fp32, head + hipGraph decode bf16): the ragged batch of 8 systems 256 x 1024 ...
    768 x 3072.  The two extreme images (N = 1024 and N = 9216 - the largest encoder attention and cross-attention memory of the config,
    never run under pytest before) are checked against the CPU oracle: fp32 latent within 1e-3; greedy ids of 36 steps equal to the
    oracle's autocast restatement, a differing token tolerated only where the oracle's own top-2 margin is within bf16 resolution."""
    import oracle.vitomr_oracle as O
    from acai_omr_amd.inference.vitomr_inference import inference
    _threads()
    vitomr, sd, imgs = _config4_model(dev, torch.bfloat16)
    steps = 37
    seqs, lps, mask = inference(vitomr, [im.to(dev) for im in imgs], dev, max_inference_len=steps)
    assert seqs.shape == (8, steps) and bool(mask.all())
    with torch.no_grad():
        lat32, _, lens = vitomr.encoder.forward_packed([im.to(dev) for im in imgs])
    assert lens == [h * w // 256 for h, w in CONFIG4_SHAPES] and sum(lens) == 38144
    offs = [0]
    for l in lens:
        offs.append(offs[-1] + l)
    for b in (0, 7):
        lat_o, l_o = O.encoder_forward([imgs[b]], sd, "encoder.", 16, 12, "omr_ft", "fp32")
        assert l_o == [lens[b]]
        e_lat = md(lat32[offs[b]:offs[b + 1]], lat_o)
        mem_o = O.transition_head(lat_o, sd, "bf16")
        oseqs, olps, omask, ologits = O.greedy_generate(mem_o, l_o, sd, 16, "bf16", steps, return_logits=True)
        same = seqs[b].cpu() == oseqs[0]
        top2 = ologits[0].topk(2, dim=-1).values
        margin = top2[:, 0] - top2[:, 1]
        bad = (~same).nonzero()
        first = int(bad[0]) if len(bad) else steps
        print(f"config4 image {b} (N={lens[b]}): latent max|d| {e_lat:.3e}; tokens equal up to step {first} of {steps}; min top-2 margin {float(margin.min()):.3f}")
        assert e_lat < 1e-3
        if len(bad):
            assert float(margin[first - 1]) <= 0.13, (b, first, float(margin[first - 1]))
        assert first >= 8                                             # a tie that early would make the check vacuous: reseed
        eq = slice(1, first)
        assert md(lps[b, eq], olps[0, eq]) < 0.07


def test_config4_batch_independence_of_all_8(dev):
    """Size-independent property on the same ragged batch (fp32 cache: no rounding freedom): every system decoded inside the batch of 8 -
    different cross-attention split counts, packed encoder stream, GEMV batch tiles - gets the tokens and log-probs it gets alone."""
    from acai_omr_amd.inference.vitomr_inference import inference
    vitomr, sd, imgs = _config4_model(dev, torch.float)
    steps = 20
    with torch.no_grad():
        lat32, _, lens = vitomr.encoder.forward_packed([im.to(dev) for im in imgs])
        mem = vitomr.transition_head.forward_packed(lat32)
        seqs, lps, mask = vitomr._greedy_packed(mem, None, lens, steps)
        o = 0
        for b, l in enumerate(lens):
            lat1, _, l1 = vitomr.encoder.forward_packed([imgs[b].to(dev)])
            assert md(lat1, lat32[o:o + l]) < 1e-4, b
            s1, p1, m1 = vitomr._greedy_packed(vitomr.transition_head.forward_packed(lat1), None, l1, steps)
            assert torch.equal(s1[0], seqs[b]), b
            assert md(p1[0], lps[b]) < 1e-3, b
            o += l


# ---- GRPO rollouts pinned on the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grpo_small", "grpo_dh64"])
@pytest.mark.parametrize("tag", ["fp32", "bf16"])
@pytest.mark.parametrize("grouped", [False, True])
def test_grpo_rollouts_replay_the_reference(dev, name, tag, grouped):
    """`GRPOViTOMR.cached_forward_rollout_policy` as the imported reference ran it under torch.manual_seed (tests/golden/grpo_*.pt): fed the
    fixture's uniforms (the inverse-CDF arguments of the reference's own multinomial draws) the graph-replayed HIP sampling step lands on the
    reference's rollouts, mask and log-probs; with `group_size` the rows of an image share one stored cross K/V (bf16 / d_h = 64: the
    matrix-core group kernel)."""
    from acai_omr_amd.models.models import FineTuneOMREncoder, GRPOViTOMR, OMRDecoder, TeacherForcedViTOMR
    fx = load_golden(name)
    cfg, ref = fx["cfg"], fx[tag]
    bf = tag == "bf16"
    enc = FineTuneOMREncoder(cfg["P"], cfg["pe_h"], cfg["pe_w"], cfg["ft_depth"], num_layers=cfg["enc_layers"], hidden_dim=cfg["enc_dim"],
                             num_heads=cfg["enc_heads"], mlp_dim=cfg["enc_mlp"])
    dec = OMRDecoder(cfg["max_len"], VOCAB, num_layers=cfg["dec_layers"], hidden_dim=cfg["dec_dim"], num_heads=cfg["dec_heads"], mlp_dim=cfg["dec_mlp"])
    tf = TeacherForcedViTOMR(enc, None, dec, transition_head_dim=cfg["head_dim"])
    tf.load_state_dict(fx["state_dict"])
    G = fx["group"]
    R = len(fx["lat_lens"]) * G
    cached = dec.to_cached_version(R, torch.bfloat16 if bf else torch.float)
    g = GRPOViTOMR(tf.encoder, tf.transition_head, cached, fx["state_dict"]).to(dev).eval()
    mem_x, mask_x = g.expand_img_latent_for_rollout(fx["mem"].to(dev), fx["mask"].to(dev), G)
    with torch.no_grad(), autocast(device_type="cuda", dtype=torch.bfloat16, enabled=bf):
        ro, lp, mk = g.cached_forward_rollout_policy(mem_x, mask_x, max_actions=fx["max_actions"], top_k=fx["top_k"], temperature=fx["temperature"],
                                                     uniforms=ref["uniforms"], group_size=G if grouped else None)
    rro, rlp, rmk = ref["rollouts"], ref["log_probs"], ref["mask"]
    if not bf:
        assert torch.equal(ro.cpu(), rro) and torch.equal(mk.cpu(), rmk)
        assert md(lp, rlp) < 1e-4
    else:
        # bf16 logits differ from the reference's by accumulation order (one bf16 ulp at |logit| ~ 4-8 is 0.03): a draw may fall on the other
        # side of a CDF step.  Rows must agree up to such a step, and the log-probs of agreeing live positions to that logit resolution (the
        # sampling formula itself is held to the oracle on the path's OWN logits in test_gpu_parity.py::test_grpo_rollout_policy_sampling)
        n = min(ro.shape[1], rro.shape[1])
        same = ro.cpu()[:, :n] == rro[:, :n]
        agree = same.int().cumprod(dim=1).bool()
        print(f"grpo bf16 replay {name} grouped={grouped}: prefix agreement {float(agree.float().mean()):.3f}, rows identical {int(same.all(dim=1).sum())}/{same.shape[0]}")
        assert float(agree.float().mean()) > 0.9     # measured 1.000 on every fixture (all rows identical); the slack is for a draw that lands on a CDF step
        live = agree & rmk[:, :n] & mk.cpu()[:, :n]
        d = (lp.cpu()[:, :n] - rlp[:, :n]).abs()[live]
        assert float(d.max()) < 0.07, float(d.max())


# ---- small holes: PE interpolation in the training path, label smoothing, the reference's micro-config --------------------------------------
def test_pe_interpolation_kernel_vs_aten(dev):
    from acai_omr_amd import ops
    g = torch.Generator().manual_seed(8)
    for (Hin, Win, E, Ho, Wo) in [(6, 10, 32, 7, 11), (60, 200, 768, 64, 208), (4, 8, 10, 9, 3), (5, 5, 16, 5, 12)]:
        t = torch.randn(Hin, Win, E, generator=g).to(dev).requires_grad_(True)
        ref = torch.nn.functional.interpolate(t.permute(2, 0, 1).unsqueeze(0), size=(Ho, Wo), mode="bilinear", align_corners=False).squeeze(0).permute(1, 2, 0)
        out = ops.pe_interp(t.detach(), Ho, Wo)
        assert md(out.view(Ho, Wo, E), ref) < 1e-5
        dy = torch.randn(Ho * Wo, E, generator=g).to(dev)
        ref.reshape(-1, E).backward(dy)
        assert md(ops.pe_interp_bwd(dy, Ho, Wo, (Hin, Win, E)), t.grad) < 1e-4


def test_teacher_forced_train_step_with_pe_interpolation_vs_reference(dev):
    """tests/golden/tf_interp.pt: images beyond the PE grid in TRAIN mode (the reference interpolates in batchify in every mode,
    models.py:304-332): logits, loss and gradients - incl. pos_embedding's, which flows through the bilinear interpolation."""
    from acai_omr_amd.models.models import FineTuneOMREncoder, OMRCELoss, OMRDecoder, TeacherForcedViTOMR
    fx = load_golden("tf_interp")
    cfg = fx["cfg"]
    enc = FineTuneOMREncoder(cfg["P"], cfg["pe_h"], cfg["pe_w"], cfg["ft_depth"], num_layers=cfg["enc_layers"], hidden_dim=cfg["enc_dim"],
                             num_heads=cfg["enc_heads"], mlp_dim=cfg["enc_mlp"], transformer_dropout=0.0)
    dec = OMRDecoder(cfg["max_len"], VOCAB, num_layers=cfg["dec_layers"], hidden_dim=cfg["dec_dim"], num_heads=cfg["dec_heads"], mlp_dim=cfg["dec_mlp"],
                     transformer_dropout=0.0)
    m = TeacherForcedViTOMR(enc, None, dec, transition_head_dim=cfg["head_dim"], transition_head_dropout=0.0)
    m.load_state_dict(fx["state_dict"])
    m = m.to(dev).train()
    assert any(im.shape[-2] // cfg["P"] > cfg["pe_h"] or im.shape[-1] // cfg["P"] > cfg["pe_w"] for im in fx["imgs"])
    pred, tgt = m(list(zip(fx["imgs"], fx["lmx"])))
    valid = fx["target"] != 1
    assert torch.equal(tgt.cpu(), fx["target"]) and md(pred.cpu()[valid], fx["pred"][valid]) < 1e-3
    loss = OMRCELoss(m.decoder.pad_idx)(pred, tgt)
    assert abs(float(loss) - float(fx["loss"])) < 1e-4
    loss.backward()
    params = dict(m.named_parameters())
    assert "encoder.pos_embedding" in fx["grads"]
    for n, gref in fx["grads"].items():
        assert md(params[n].grad, gref) < 3e-4 * max(1.0, float(gref.abs().max())), n
    # a non-interpolating encoder still refuses, with the reference's message, in the training path too
    from acai_omr_amd.models.models import Encoder
    base = Encoder(4, 6, 10, num_layers=1, hidden_dim=32, num_heads=2, mlp_dim=64).to(dev).train()
    with pytest.raises(ValueError) as e:
        base([torch.rand(1, 28, 44)])
    assert str(e.value) == load_golden("omr_encoder_interp")["too_large_msg"]


def test_ce_loss_label_smoothing_vs_reference(dev):
    from acai_omr_amd.models.models import OMRCELoss
    fx = load_golden("ce_label_smoothing")
    for eps in (0.0, 0.1):
        lg = fx["logits"].to(dev).requires_grad_(True)
        loss = OMRCELoss(fx["pad_idx"], label_smoothing=eps)(lg, fx["target"].to(dev))
        assert abs(float(loss) - float(fx[f"loss_{eps}"])) < 1e-5
        loss.backward()
        assert md(lg.grad, fx[f"grad_{eps}"]) < 1e-6


def test_reference_micro_config_through_fine_tune_epoch(dev):
    """The literal configuration of the reference's tests/test_omr_teacher_force_train.py:10-38: 64 examples of a (1, 32, 32) image and 10
    tokens in [10, 100), the debug-width model (hidden 10, 2 layers, 1 head, mlp 1, patch 16, fine-tune depth 1) initialised from the
    reference's own debug MAE checkpoint, batch 8, accumulation 8 - one epoch of `fine_tune_epoch` (bf16 autocast, LLRD param groups, fused
    AdamW, schedulers) against the same loop over the oracle's bf16 restatement + torch.optim.AdamW (tf_prob pinned to 1)."""
    import oracle.vitomr_oracle as O
    from acai_omr_amd.models.models import FineTuneOMREncoder, OMRCELoss, OMRDecoder, ScheduledSamplingViTOMR
    from acai_omr_amd.optim import FusedAdamW
    from acai_omr_amd.train import loops
    from acai_omr_amd.utils import cosine_anneal_with_warmup
    dbg = load_golden("mae_debug_ckpt")["state_dict"]
    kw = dict(num_layers=2, num_heads=1, mlp_dim=1)
    torch.manual_seed(7)
    enc = FineTuneOMREncoder(16, 60, 200, 1, hidden_dim=10, **kw)
    dec = OMRDecoder(1536, VOCAB, hidden_dim=10, **kw)
    m = ScheduledSamplingViTOMR(enc, dbg, dec)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = 0.0
    g = torch.Generator().manual_seed(8)
    data = [(torch.rand(1, 32, 32, generator=g), torch.randint(10, 100, (10,), generator=g)) for _ in range(64)]
    batches = [data[i:i + 8] for i in range(0, 64, 8)]

    class L(list):
        pass

    ACC = loops.FINE_TUNE["grad_accumulation_steps"]
    trainable = {n for n, p in m.named_parameters() if p.requires_grad}      # frozen blocks / projection / PE (models.py:667-677) stay put
    assert "encoder.pos_embedding" not in trainable and "encoder.fine_tune_blocks.layers.0.linear1.weight" in trainable
    sd = {k: v.detach().clone().requires_grad_(k in trainable) for k, v in m.state_dict().items()}

    def groups_for(model, params_of):
        gs, _ = model.create_fine_tune_param_groups(1e-2, 5e-3, 0.9)
        ids = {id(p): n for n, p in model.named_parameters()}
        return [{"params": [params_of(ids[id(p)]) for p in list(gr["params"])], "lr": gr["lr"]} for gr in gs]

    opt_o = torch.optim.AdamW(groups_for(m, lambda n: sd[n]), betas=(0.9, 0.95), weight_decay=0.01)
    sch_o = cosine_anneal_with_warmup(opt_o, 1, 3, 1e-6, num_train_batches=1)
    tot = 0.0
    for i, b in enumerate(batches):
        pred, tgt = O.teacher_forced_forward(b, sd, 1, 1, 16, "bf16")
        loss = O.ce_loss(pred, tgt, 1)
        tot += loss.item()
        loss.backward()
        if (i + 1) % ACC == 0 or i + 1 == len(batches):
            opt_o.step()
            opt_o.zero_grad()
            sch_o.step()
    m = m.to(dev)
    named = dict(m.named_parameters())
    opt = FusedAdamW(groups_for(m, lambda n: named[n]), betas=(0.9, 0.95), weight_decay=0.01)
    sch = cosine_anneal_with_warmup(opt, 1, 3, 1e-6, num_train_batches=1)
    tfc = loops.TFConfig(1.0, 5.0, False)
    tfs = loops.TFScheduler(tfc, 1.0, 1.0, 5.0, 0.1, 1, 2, 1)
    counter = loops.StepCounter()
    avg = loops.fine_tune_epoch(m, L(batches), OMRCELoss(m.decoder.pad_idx), opt, sch, "cuda", ACC, tfc, tfs, None, counter)
    assert counter.global_step == 1 and abs(avg - tot / len(batches)) < 2e-2, (avg, tot / len(batches))
    assert [gr["lr"] for gr in opt.param_groups] == [gr["lr"] for gr in opt_o.param_groups]
    moved = 0
    for n, p in m.named_parameters():
        d = float((p.detach().cpu() - sd[n].detach()).abs().max())
        assert d < 2.5e-2, (n, d)                     # one AdamW step of lr 1e-2: a flipped sign of a ~0 gradient moves 2 lr
        moved += int(p.requires_grad)
    assert moved > 10


# ---- advisor items ------------------------------------------------------------------------------------------------------------------------
def test_deepcopy_and_save_after_a_decode(dev):
    """The reference's GRPO loop deep-copies its policy (omr_grpo_train.py): a model that has decoded (live DecodeEngine: ctypes descriptors,
    stream, graphs) must deep-copy and pickle, and the copy must decode to the same tokens."""
    import io
    from acai_omr_amd.inference.vitomr_inference import inference
    from test_gpu_parity import build_vitomr
    fx = load_golden("vitomr_dh64")
    cfg = fx["cfg"]
    m = build_vitomr(cfg, fx["state_dict"], dev, torch.bfloat16)
    seqs, lps, mask = inference(m, fx["imgs"], dev, max_inference_len=cfg["gen_len"])
    m2 = copy.deepcopy(m)
    assert m2.decoder.decoder_blocks.__dict__["_engine"] is None and m.decoder.decoder_blocks.__dict__["_engine"] is not None
    s2, l2, k2 = inference(m2, fx["imgs"], dev, max_inference_len=cfg["gen_len"])
    assert torch.equal(s2, seqs) and torch.equal(k2, mask) and torch.equal(l2, lps)
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    m3 = torch.load(buf, weights_only=False)
    s3, _, _ = inference(m3, fx["imgs"], dev, max_inference_len=cfg["gen_len"])
    assert torch.equal(s3, seqs)
    # WeightCache.invalidate(): a write through .data does not move the version counter
    from acai_omr_amd.engine import WeightCache
    p = torch.nn.Parameter(torch.randn(4, 8, device=dev))
    wc = WeightCache()
    w0 = wc.w(p, "bf16").clone()
    p.data.mul_(2.0)
    assert torch.equal(wc.w(p, "bf16"), w0)            # stale, as documented
    wc.invalidate()
    assert torch.equal(wc.w(p, "bf16"), p.detach().to(torch.bfloat16))


def test_streamed_step_event_on_the_last_flush_boundary(dev):
    """models.py:641-645: STEP is yielded at every t % flush_interval == 0 that did not finish the sequence - also when t == max_len - 1."""
    from acai_omr_amd.config import InferenceEvent
    from test_gpu_parity import build_vitomr
    fx = load_golden("vitomr_small")
    cfg = fx["cfg"]
    m = build_vitomr(cfg, fx["state_dict"], dev, torch.float)
    with torch.no_grad():
        m.decoder.unembed.bias[2] = -1.0e4       # never <eos>
        lat, mask = m.encoder(fx["imgs"][:1])
        mem = m.transition_head(lat)
        ev = list(m.streamed_cached_greedy_generate(mem, mask, max_len=13, flush_interval=4))    # t = 1..12: boundaries 4, 8, 12 = max_len - 1
        steps = [e for e in ev if e["type"] == InferenceEvent.STEP.value]
        assert len(steps) == 3 and ev[-1]["type"] == InferenceEvent.INFERENCE_FINISH.value
        seq = ev[-1]["payload"]["sequence"]
        assert torch.equal(torch.cat([s["payload"]["tokens"] for s in steps], 1).long()[0], seq[0, 1:13])
        ev = list(m.streamed_cached_greedy_generate(mem, mask, max_len=12, flush_interval=4))    # t = 1..11: boundaries 4, 8
        assert len([e for e in ev if e["type"] == InferenceEvent.STEP.value]) == 2


def test_fused_adamw_per_tensor_step_counts(dev):
    """torch.optim.AdamW keeps `step` per parameter: one that skips steps (no gradient for a while) carries its own bias correction."""
    from acai_omr_amd.optim import FusedAdamW
    g = torch.Generator().manual_seed(10)
    base = [torch.randn(33, 7, generator=g), torch.randn(50, generator=g)]
    pa = [torch.nn.Parameter(b.clone().to(dev)) for b in base]
    pb = [torch.nn.Parameter(b.clone().to(dev)) for b in base]
    oa, ob = torch.optim.AdamW(pa, lr=1e-2, betas=(0.9, 0.95)), FusedAdamW(pb, lr=1e-2, betas=(0.9, 0.95))
    for it in range(5):
        for i, (x, y) in enumerate(zip(pa, pb)):
            if i == 1 and it in (1, 2):
                x.grad = y.grad = None            # the second tensor skips two steps
                continue
            gr = torch.randn(x.shape, generator=g).to(dev)
            x.grad, y.grad = gr.clone(), gr.clone()
        oa.step(), ob.step()
    assert float(ob.state[pb[0]]["step"]) == 5 and float(ob.state[pb[1]]["step"]) == 3
    for x, y in zip(pa, pb):
        assert torch.allclose(x, y, rtol=2e-6, atol=2e-7)


def test_ops_follow_the_operands_device(dev):
    """ADVICE: a model on cuda:N while another device is current must launch on ITS device.  Needs two GPUs (the wrappers switch the device
    for the launch); on a one-GPU box only the mixed-device refusal path is checked."""
    from acai_omr_amd import ops
    if torch.cuda.device_count() >= 2:
        x = torch.randn(64, 256, device="cuda:1")
        w, b = torch.ones(256, device="cuda:1"), torch.zeros(256, device="cuda:1")
        with torch.cuda.device(0):
            y, _ = ops.layernorm(x, w, b, 1e-5)
        torch.cuda.synchronize("cuda:1")
        assert y.device == x.device and md(y, torch.nn.functional.layer_norm(x, (256,))) < 1e-5
        with pytest.raises(RuntimeError):
            ops.layernorm(x, w.to("cuda:0"), b, 1e-5)
    else:
        x = torch.randn(8, 256, device=dev)
        y, _ = ops.layernorm(x, torch.ones(256, device=dev), torch.zeros(256, device=dev), 1e-5)
        assert md(y, torch.nn.functional.layer_norm(x, (256,))) < 1e-5


def test_data_parallel_step_on_the_hip_path_two_ranks(dev):
    """`GradAllReduce` + global-count loss scaling + `no_sync` accumulation + fused AdamW on the REAL path (HIP autograd Functions) under two
    ranks with ragged shards == the single-process global-batch step (gradients and updated parameters).  Two processes started by
    torch.distributed.run (before anything of theirs touches the GPU) share this box's one card over gloo; on the 8-GPU node the same
    function runs over RCCL inside `bench.py --gpus N` (`dp_parity_max_abs_diff`)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    port = 29700 + os.getpid() % 200
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(root, "tools", "dp_parity.py"), "--backend", "gloo"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["world"] == 2 and out["dp_parity_max_abs_diff"] < 1e-4, out


def test_data_parallel_scheduled_sampling_step_two_ranks(dev):
    """The same two-rank check with its scheduled-sampling leg (tools/dp_parity.py --scheduled-sampling): forward_train at tf_prob = 0.4 with
    per-item injected draws, sharded over two gloo ranks on this card, == the single-process global-batch step.  The decoder's parameters
    get their second gradient contribution written in place (autograd_path._PGRAD) while GradAllReduce's hooks hand bucket views to the
    all-reduce."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    port = 29500 + os.getpid() % 200
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(root, "tools", "dp_parity.py"), "--backend", "gloo", "--scheduled-sampling"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["world"] == 2 and out["scheduled_sampling"] and out["dp_parity_max_abs_diff"] < 1e-4, out


def test_benchmarked_decode_shape_bf16_vs_oracle(dev):
    """The BENCHMARKED configuration itself (BASELINE north star: batch 8, 4096-patch memories, full-size decoder, bf16 plumbing, hipGraph
    replay - what `bench.py` times): greedy ids and log-probs of two of the eight rows against the CPU oracle's autocast restatement run on
    that row alone; a differing token is tolerated only where the oracle's own top-2 margin is within bf16 resolution."""
    from acai_omr_amd.models.models import OMRDecoder, ViTOMR
    from oracle import vitomr_oracle as O
    _threads()
    torch.manual_seed(31)
    dec = OMRDecoder(64, VOCAB, num_layers=12)
    with torch.no_grad():
        for n, p in dec.named_parameters():
            if "norm" in n:
                p.add_(0.1 * torch.randn_like(p))
        dec.unembed.weight.mul_(6.0)
        dec.unembed.bias[2] = -1.0e4
    cached = dec.to_cached_version(8, torch.bfloat16)
    cached.load_state_dict(dec.state_dict())
    model = ViTOMR(None, None, cached.to(dev).eval())
    S, steps = 4096, 33
    mem = O.rbf16(torch.randn(8 * S, 1024, generator=torch.Generator().manual_seed(32)))
    with torch.no_grad():
        seqs, lps, mask = model._greedy_packed(None, mem.to(dev).to(torch.bfloat16), [S] * 8, steps)
    assert seqs.shape == (8, steps)
    sd = {"decoder." + k: v for k, v in dec.state_dict().items()}
    for b in (1, 6):
        oseqs, olps, omask, ologits = O.greedy_generate(mem[b * S:(b + 1) * S], [S], sd, 16, "bf16", steps, return_logits=True)
        same = seqs[b].cpu() == oseqs[0]
        top2 = ologits[0].topk(2, dim=-1).values
        margin = top2[:, 0] - top2[:, 1]
        bad = (~same).nonzero()
        first = int(bad[0]) if len(bad) else steps
        if len(bad):
            assert float(margin[first - 1]) <= 0.13, (b, first, float(margin[first - 1]))
        assert first >= 8, (b, first)
        assert md(lps[b, 1:first], olps[0, 1:first]) < 0.07


def test_bench_dump_outputs_of_the_timed_decode(dev, tmp_path):
    """`bench.py --dump-outputs DIR` (headline only): the decode state the last timed step left - ids and log-probs up to the current position,
    that step's logits - as float .npy files; `--steps` sets the timed steps, and two runs with the same arguments write the same arrays."""
    import json
    import subprocess
    import sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = []
    for i in range(2):
        out = tmp_path / f"run{i}"
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--legs", "", "--no-cpu-baseline",
                            "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        runs.append({n: np.load(out / f"{n}.npy") for n in ("seqs", "logprobs", "logits")})
    seqs, lps, logits = runs[0]["seqs"], runs[0]["logprobs"], runs[0]["logits"]
    assert seqs.dtype == np.float64 and lps.dtype == np.float32 and logits.dtype == np.float32
    assert seqs.shape == (8, 1 + 2 + 3) and lps.shape == seqs.shape and logits.shape == (8, 227)
    assert (seqs == np.round(seqs)).all() and seqs.min() >= 0 and seqs.max() < 227
    assert np.isfinite(lps).all() and np.isfinite(logits).all()
    for n in ("seqs", "logprobs", "logits"):
        assert np.array_equal(runs[1][n], runs[0][n]), n
