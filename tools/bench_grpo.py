"""Time one GRPO update epoch at the reference's shape (omr_grpo_train.py: 16 images x 8 rollouts, decoder 10 x 1024, bf16 autocast,
checkpoint_grads=True): the policy forward + fused objective / bonus + backward with the group-shared memory (memory_group_size) against the
materialised expansion the reference makes (expand_img_latent_for_rollout), and the fused objective pass against the ATen formulas.
Seeded weights, fixed rollout length.  Prints one JSON line.

    python tools/bench_grpo.py [--images 16] [--group 8] [--tokens 500] [--mem 4096] [--iters 3]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BF16_TFLOPS = 2500.0   # MI355X dense bf16 matrix peak (public spec)
PEAK_HBM_TBS = 8.0          # MI355X HBM3E peak (public spec)


def aten_objective_and_bonus(logits, rollouts, mask, old_lp, adv, eps, num_groups):
    lsm = torch.log_softmax(logits.float(), -1)
    lp = torch.gather(lsm, -1, rollouts[:, 1:].unsqueeze(-1)).squeeze(-1)
    ratios = torch.exp(lp - old_lp[:, 1:])
    u = (ratios * adv.unsqueeze(1)).masked_fill(mask, 0)
    c = (torch.clip(ratios, 1 - eps, 1 + eps) * adv.unsqueeze(1)).masked_fill(mask, 0)
    lens = (~mask).sum(-1)
    obj = (torch.min(u, c).sum(-1) / lens).sum() / num_groups
    ent = (-torch.softmax(logits.float(), -1) * lsm).sum(-1).masked_fill(mask, 0)
    bonus = (ent.sum(-1) / lens).mean() / torch.log(torch.tensor(logits.shape[-1]))
    return obj, bonus


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(iters):
        s = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - s) * 1e3)
    return min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--group", type=int, default=8)
    ap.add_argument("--tokens", type=int, default=500)
    ap.add_argument("--mem", type=int, default=4096)
    ap.add_argument("--layers", type=int, default=10)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=3)
    a = ap.parse_args()
    from acai_omr_amd.models.models import OMRDecoder
    from acai_omr_amd.train import grpo as G
    dev = "cuda"
    vocab = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lmx_vocab.txt")
    torch.manual_seed(0)
    dec = OMRDecoder(a.tokens + 1, vocab, num_layers=a.layers, hidden_dim=a.dim, num_heads=a.dim // 64, mlp_dim=4 * a.dim,
                     transformer_dropout=0.0).to(dev).train()
    B, Gs, T, S, E, V = a.images, a.group, a.tokens, a.mem, a.dim, dec.vocab_size
    R = B * Gs
    g = torch.Generator().manual_seed(1)
    ro = torch.randint(3, V, (R, T + 1), generator=g).to(dev)
    mask = torch.zeros(R, T, dtype=torch.bool, device=dev)
    old = (torch.randn(R, T + 1, generator=g) * 0.1 - 5.4).to(dev)
    adv = torch.randn(R, generator=g).to(dev)
    mem = torch.randn(B, S, E, generator=g).to(dev)
    mmask = torch.zeros(B, S, dtype=torch.bool, device=dev)

    def epoch(grouped):
        def run():
            with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
                if grouped:
                    lg = dec(ro[:, :-1], mem, mask, mmask, checkpoint_grads=True, memory_group_size=Gs)
                else:
                    mx, mmx = mem.unsqueeze(1).expand(-1, Gs, -1, -1).flatten(0, 1), mmask.unsqueeze(1).expand(-1, Gs, -1).flatten(0, 1)
                    lg = dec(ro[:, :-1], mx, mask, mmx, checkpoint_grads=True)
                obj, bonus = G.calc_grpo_objective_and_entropy_bonus(lg, ro, mask, old, adv, 0.2, B)
            (-(obj + 0.05 * bonus)).backward()
            dec.zero_grad(set_to_none=True)
        return run

    ms_grouped = timed(epoch(True), a.iters)
    ms_expanded = timed(epoch(False), a.iters)
    lg = (torch.randn(R, T, V, generator=g) * 2).to(dev).to(torch.bfloat16).requires_grad_(True)

    def fused():
        o, b = G.calc_grpo_objective_and_entropy_bonus(lg, ro, mask, old, adv, 0.2, B)
        (o + b).backward()

    def aten():
        o, b = aten_objective_and_bonus(lg, ro, mask, old, adv, 0.2, B)
        (o + b).backward()
    ms_fused, ms_aten = timed(fused, 10), timed(aten, 10)
    lg.grad = None
    with torch.no_grad():
        ms_fused_fwd = timed(lambda: G.calc_grpo_objective_and_entropy_bonus(lg, ro, mask, old, adv, 0.2, B), 10)
    # FLOPs of one epoch (forward + recompute + backward = 4x the forward's matmuls), grouped form: per layer, token-side GEMMs
    # (self in/out, cross q/out, MLP) 2 * Nt * (4E^2 + 2E^2 + 8E^2), memory K/V 2 * B*S * 2E^2, attention 4 * Nt * (T/2 + S) * E
    Nt = R * T
    fwd = a.layers * (2 * Nt * 14 * E * E + 2 * B * S * 2 * E * E + 4 * Nt * (T / 2 + S) * E) + 2 * Nt * E * V
    fwd_x = fwd + a.layers * 2 * (R - B) * S * 2 * E * E
    tflop_g, tflop_x = 4 * fwd / 1e12, 4 * fwd_x / 1e12
    bytes_fwd = R * T * V * 2
    print(json.dumps({
        "shape": {"images": B, "group": Gs, "tokens": T, "mem": S, "layers": a.layers, "dim": E},
        "epoch_ms_grouped": round(ms_grouped, 2), "epoch_ms_expanded": round(ms_expanded, 2), "speedup": round(ms_expanded / ms_grouped, 3),
        "tflop_counted_grouped": round(tflop_g, 2), "tflop_counted_expanded": round(tflop_x, 2),
        "frac_bf16_peak_grouped": round(tflop_g / (ms_grouped / 1e3) / PEAK_BF16_TFLOPS, 3),
        "objective_fwd_bwd_ms_fused": round(ms_fused, 3), "objective_fwd_bwd_ms_aten": round(ms_aten, 3),
        "objective_fwd_ms_fused": round(ms_fused_fwd, 3),
        "objective_fwd_frac_hbm_peak": round(bytes_fwd / (ms_fused_fwd / 1e3) / (PEAK_HBM_TBS * 1e12), 3),
    }))


if __name__ == "__main__":
    main()
