"""Per-token confidence: what the passes after decoding cost.  Workload: 8 images of 512x2048 (4096 patches each), 512 tokens per image,
bf16, bench.py's random-init full-size model, all 12 decoder layers and 16 heads, one process.  The tokens are the model's own greedy
output with <eos> suppressed.  Reported, each as median / min / max over --rounds (device events around the work, warmed up first,
variants interleaved):

  logits_pass_ms    the logits-only pass as confident_inference runs it after the decode: the teacher-forced pass over the 8 x 512 tokens
                    and acai_token_confidence;
  combined_pass_ms  the combined pass (uncertainty="entropy"): the pass with acai_attn_probs_mean in every layer, acai_token_confidence,
                    acai_attn_map_weighted_sum and acai_attn_map_locate;
  align_pass_ms     aligned_inference's pass on the same inputs (maps and acai_attn_map_locate, no logits) - what the combined pass adds to;
  conf_ms           ops.token_confidence alone on the pass's logits (4096 x 230), per call, --reps calls per timed window;
  conf_torch_ms     the same five results from torch on the same GPU: log_softmax, gather, topk, entropy, rank by comparison;
  wsum_ms           ops.attn_map_weighted_sum alone on the pass's maps (both launches; the layout given on the host, as the pass does), per call;
  wsum_torch_ms     torch.einsum over the same maps as one padded (B, T, S) tensor;
  decode_ms         the greedy decode of the same batch to 513 indices (replayed graphs, captured in an untimed cold run);
and from them the passes as shares of the decode, the kernels' speed-ups over torch, and the map-read rate of the weighted sum (bytes of
map read per second of wsum_ms) against the HBM copy rate of 6.29 TB/s (MI355X_MICROARCH.md: float4 copy).  Also the largest differences
between the kernels' results and torch's.  One JSON line on stdout, the same written to --out.

  python tools/bench_confidence.py --rounds 7 --out profiles/confidence_bench.json
"""
import argparse
import json
import os
import sys

import torch
from torch.amp import autocast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_BYTES_PER_S = 6.29e12


def stats(xs):
    s = sorted(xs)
    return dict(median=s[len(s) // 2], min=s[0], max=s[-1])


def event_ms(fn, reps=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, out


def torch_confidence(logits, chosen, top_k):
    """The baseline: the kernel's five results from torch ops (torch.topk orders equal logits as it likes, the kernel by index)."""
    lsm = torch.log_softmax(logits, dim=-1)
    lp = lsm.gather(-1, chosen[:, None]).squeeze(1)
    p = torch.exp(lsm)
    ent = -(p * lsm).sum(-1)
    vc = logits.gather(-1, chosen[:, None])
    idx = torch.arange(logits.shape[1], device=logits.device)
    rank = ((logits > vc) | ((logits == vc) & (idx < chosen[:, None]))).sum(-1)
    top_lp, top_ids = lsm.topk(top_k, dim=-1)
    return lp, ent, rank, top_ids, top_lp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--top-k", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    from acai_omr_amd import engine, ops
    from acai_omr_amd.inference.vitomr_inference import set_up_omr_inference
    torch.manual_seed(0)   # bench.py's weights
    vitomr, _ = set_up_omr_inference(os.path.join(ROOT, "lmx_vocab.txt"), max_batch_size=a.images, cache_dtype=torch.bfloat16, device="cuda")
    vitomr = vitomr.eval()
    dec = vitomr.decoder
    with torch.no_grad():
        dec.unembed.bias[dec.eos_idx] = -1e4   # <eos> suppressed: every row runs to the cap
    g = torch.Generator().manual_seed(1000)
    imgs = [torch.rand(1, a.height, a.width, generator=g).to(dev) for _ in range(a.images)]
    P = vitomr.encoder.patch_size
    grids = [(a.height // P, a.width // P)] * a.images
    T = a.tokens + 1
    with torch.no_grad():
        lat32, _, lens = vitomr.encoder.forward_packed(imgs)
        with autocast(device_type="cuda", dtype=torch.bfloat16):
            mem = vitomr.transition_head.forward_packed(lat32)

    def ctx():
        return autocast(device_type="cuda", dtype=torch.bfloat16)

    def decode():
        with torch.no_grad(), ctx():
            return vitomr._greedy_packed(None, mem, lens, T)

    seqs, lps, mask = decode()   # cold: code objects, graph capture
    assert seqs.shape[1] == T and bool(mask.all()), "the rows did not run to the cap"

    def logits_pass():
        with torch.no_grad(), ctx():
            return vitomr._confidence_packed(None, mem, lens, seqs, mask, a.top_k, 1.0, True)

    def combined_pass():
        with torch.no_grad(), ctx():
            return vitomr._confidence_packed(None, mem, lens, seqs, mask, a.top_k, 1.0, True, "entropy", None, None, grids, P, True)

    def align_pass():
        with torch.no_grad(), ctx():
            return vitomr._align_packed(None, mem, lens, seqs, mask, None, None, True, grids, P, False)

    # the kernels' own inputs, from one combined pass
    lens_t = [a.tokens] * a.images
    tokens = seqs[:, :a.tokens].reshape(-1)
    chosen = seqs[:, 1:T].reshape(-1).contiguous()
    with torch.no_grad(), ctx():
        maps, offs, map_off, logits = dec._cross_attention_maps_flat(tokens, lens_t, None, mem, lens, None, None, 1, None, True)
    cu_t, cu_s = engine.cu_from_lens(lens_t, dev), engine.cu_from_lens(lens, dev)
    conf = ops.token_confidence(logits, chosen, a.top_k, 1.0)
    weights = conf[1].contiguous()
    base = torch_confidence(logits, chosen, a.top_k)
    conf_diff = dict(log_prob=float((conf[0] - base[0]).abs().max()), entropy=float((conf[1] - base[1]).abs().max()),
                     rank_mismatches=int((conf[2].long() != base[2]).sum()), top_id_mismatches=int((conf[3].long() != base[3]).sum()),
                     # (torch.topk orders equal logits as it likes; the kernel by index: ids may differ where values tie, values may not)
                     top_value_mismatches=int((logits.gather(-1, conf[3].long()) != logits.gather(-1, base[3])).sum()),
                     top_log_probs=float((conf[4] - base[4]).abs().max()))
    equal = len(set(lens)) == 1 and offs == [i * a.tokens * lens[0] for i in range(a.images)]
    assert equal, "the einsum baseline wants equal image sizes"
    padded = maps.view(a.images, a.tokens, lens[0])
    wpad = weights.view(a.images, a.tokens)

    def conf_only():
        return ops.token_confidence(logits, chosen, a.top_k, 1.0)

    def conf_torch():
        return torch_confidence(logits, chosen, a.top_k)

    def wsum_only():
        return ops.attn_map_weighted_sum(maps, map_off, cu_t, cu_s, weights, a.tokens, layout=(lens_t, lens, offs))

    def wsum_torch():
        return torch.einsum("bts,bt->bs", padded, wpad)

    heat, heat_t = wsum_only(), wsum_torch().reshape(-1)
    wsum_diff = float((heat - heat_t).abs().max() / heat_t.abs().max())
    del base, heat, heat_t

    variants = [("logits_pass_ms", logits_pass, 1), ("combined_pass_ms", combined_pass, 1), ("align_pass_ms", align_pass, 1),
                ("conf_ms", conf_only, a.reps), ("conf_torch_ms", conf_torch, a.reps), ("wsum_ms", wsum_only, a.reps),
                ("wsum_torch_ms", wsum_torch, a.reps), ("decode_ms", decode, 1)]
    for _, fn, _ in variants:   # warm-up
        fn()
    torch.cuda.synchronize()
    times = {n: [] for n, _, _ in variants}
    for _ in range(a.rounds):
        for n, fn, reps in variants:
            times[n].append(event_ms(fn, reps)[0])
    res = {n: stats(v) for n, v in times.items()}
    med = lambda n: res[n]["median"]   # noqa: E731
    map_bytes = sum(t * s for t, s in zip(lens_t, lens)) * 4
    out = dict(workload=f"{a.images} images of {a.height}x{a.width} ({lens[0]} patches each), {a.tokens} tokens per image, bf16, random-init full-size "
                        f"model, {len(dec.decoder_blocks.layers)} layers x {dec.num_heads} heads, top_k {a.top_k}; device events, warmed up, variants "
                        f"interleaved, median / min / max of rounds; kernel variants per call over {a.reps} calls per window",
               rounds=a.rounds, reps=a.reps, device=torch.cuda.get_device_name(dev), **res,
               logits_pass_over_decode=med("logits_pass_ms") / med("decode_ms"), combined_pass_over_decode=med("combined_pass_ms") / med("decode_ms"),
               combined_minus_align_ms=med("combined_pass_ms") - med("align_pass_ms"),
               conf_torch_over_kernel=med("conf_torch_ms") / med("conf_ms"), wsum_torch_over_kernel=med("wsum_torch_ms") / med("wsum_ms"),
               map_bytes=map_bytes, wsum_map_read_bytes_per_s=map_bytes / (med("wsum_ms") * 1e-3), hbm_copy_bytes_per_s=HBM_COPY_BYTES_PER_S,
               wsum_read_rate_over_hbm_copy=map_bytes / (med("wsum_ms") * 1e-3) / HBM_COPY_BYTES_PER_S,
               max_abs_diff_conf_kernel_vs_torch=conf_diff, max_rel_diff_wsum_kernel_vs_torch=wsum_diff)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
