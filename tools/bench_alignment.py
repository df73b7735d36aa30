"""Token-to-image alignment: what the pass after decoding costs.  Workload: 8 images of 512x2048 (4096 patches each), 512 tokens per image,
bf16, bench.py's random-init full-size model, all 12 decoder layers and 16 heads, one process.  The tokens are the model's own greedy
output with <eos> suppressed.  Reported, each as median / min / max over --rounds (device events around the work, warmed up first):

  pass_ms          ViTOMR's alignment pass as aligned_inference runs it after the decode: the teacher-forced pass over the 8 x 512 tokens
                   with acai_attn_probs_mean in every layer, and acai_attn_map_locate;
  probs_ms         acai_attn_probs_mean alone, the layers' launches on the pass's own q / k / lse (captured from one pass);
  locate_ms        acai_attn_map_locate alone;
  torch_ms         the same maps from a torch restatement on the same GPU and the same q / k: per image and layer a batched matmul over the
                   heads, a float32 softmax, the weighted mean over heads, added up over the layers - the baseline;
  decode_ms        the greedy decode of the same batch to 513 indices (replayed graphs, captured in an untimed cold run);
and from them: the map-write rate of acai_attn_probs_mean (bytes of map written per second over its kernel time; the first layer writes
the map, the others read and write it - both counts are given) against the HBM copy rate of 6.29 TB/s (MI355X_MICROARCH.md: float4
copy, 79 % of the 8 TB/s spec), the kernel's speed-up over torch, and the pass as a share of the decode.  Also the largest difference
between the kernel's maps and torch's.  One JSON line on stdout, the same written to --out.

  python tools/bench_alignment.py --rounds 7 --out profiles/alignment_bench.json
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


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def torch_maps(calls, lens_t, lens_s, H, dh):
    """The baseline: matmul, softmax, weighted mean, summed over the layers.  calls: (q, k, head_w) per layer."""
    out = [torch.zeros(t, s, dtype=torch.float32, device=calls[0][0].device) for t, s in zip(lens_t, lens_s)]
    scale = 1.0 / dh ** 0.5
    for q, k, w in calls:
        oq = ok = 0
        for b, (t, s) in enumerate(zip(lens_t, lens_s)):
            qb = q[oq:oq + t].view(t, H, dh).transpose(0, 1)
            kb = k[ok:ok + s].view(s, H, dh).permute(1, 2, 0)
            p = torch.softmax(torch.matmul(qb, kb).float() * scale, dim=-1)
            out[b] += (w.view(H, 1, 1) * p).sum(0)
            oq += t
            ok += s
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
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

    def decode():
        with torch.no_grad(), autocast(device_type="cuda", dtype=torch.bfloat16):
            return vitomr._greedy_packed(None, mem, lens, T)

    def align(return_maps=False):
        with torch.no_grad(), autocast(device_type="cuda", dtype=torch.bfloat16):
            return vitomr._align_packed(None, mem, lens, seqs, mask, None, None, True, grids, P, return_maps)

    seqs, lps, mask = decode()   # cold: code objects, graph capture
    assert seqs.shape[1] == T and bool(mask.all()), "the rows did not run to the cap"
    lens_t = [a.tokens] * a.images
    H, dh = dec.num_heads, dec.hidden_dim // dec.num_heads

    # one pass with the kernel's arguments captured, layer by layer
    calls, real = [], ops.attn_probs_mean

    def recorder(q, k, cu_q, cu_k, H_, dh_, max_q, max_k, lse, head_w, map_off, out, accumulate=False):
        calls.append((q, k, cu_q, cu_k, max_q, max_k, lse.clone(), head_w, map_off, out, accumulate))
        return real(q, k, cu_q, cu_k, H_, dh_, max_q, max_k, lse, head_w, map_off, out, accumulate=accumulate)
    ops.attn_probs_mean = recorder
    try:
        al = align(return_maps=True)
    finally:
        ops.attn_probs_mean = real
    torch.cuda.synchronize()
    L = len(calls)
    assert L == len(dec.decoder_blocks.layers)
    kernel_maps = [m.clone() for m in al.maps]
    base = torch_maps([(c[0], c[1], c[7]) for c in calls], lens_t, lens, H, dh)
    max_diff = max(float((x - y).abs().max()) for x, y in zip(kernel_maps, base))
    row_sum_err = max(float((x.sum(-1) - 1).abs().max()) for x in kernel_maps)
    del base, al

    def probs_only():
        for q, k, cu_q, cu_k, max_q, max_k, lse, w, map_off, out, acc in calls:
            real(q, k, cu_q, cu_k, H, dh, max_q, max_k, lse, w, map_off, out, accumulate=acc)

    out0, map_off0 = calls[0][9], calls[0][8]
    cu_t, cu_s = engine.cu_from_lens(lens_t, dev), engine.cu_from_lens(lens, dev)

    def locate_only():
        return ops.attn_map_locate(out0, map_off0, cu_t, cu_s, [w for _, w in grids], max(lens_t), sum(lens_t))

    def torch_only():
        return torch_maps([(c[0], c[1], c[7]) for c in calls], lens_t, lens, H, dh)

    variants = [("pass_ms", align), ("probs_ms", probs_only), ("locate_ms", locate_only), ("torch_ms", torch_only), ("decode_ms", decode)]
    for _, fn in variants:   # warm-up
        fn()
    torch.cuda.synchronize()
    times = {n: [] for n, _ in variants}
    for _ in range(a.rounds):
        for n, fn in variants:
            times[n].append(event_ms(fn)[0])
    res = {n: stats(v) for n, v in times.items()}
    map_bytes = sum(t * s for t, s in zip(lens_t, lens)) * 4
    probs_s = res["probs_ms"]["median"] * 1e-3
    written, moved = map_bytes * L, map_bytes * (2 * L - 1)
    out = dict(workload=f"{a.images} images of {a.height}x{a.width} ({lens[0]} patches each), {a.tokens} tokens per image, bf16, random-init full-size "
                        f"model, {L} layers x {H} heads; device events, warmed up, variants interleaved, median / min / max of rounds",
               rounds=a.rounds, device=torch.cuda.get_device_name(dev), **res,
               map_bytes_per_layer=map_bytes, probs_map_write_bytes_per_s=written / probs_s, probs_map_read_write_bytes_per_s=moved / probs_s,
               hbm_copy_bytes_per_s=HBM_COPY_BYTES_PER_S, probs_write_rate_over_hbm_copy=written / probs_s / HBM_COPY_BYTES_PER_S,
               probs_read_write_rate_over_hbm_copy=moved / probs_s / HBM_COPY_BYTES_PER_S,
               torch_over_probs=res["torch_ms"]["median"] / res["probs_ms"]["median"],
               pass_over_decode=res["pass_ms"]["median"] / res["decode_ms"]["median"],
               max_abs_diff_kernel_vs_torch=max_diff, max_row_sum_error=row_sum_err)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
