"""Per-measure results: what they cost.  Workload: 8 images of 512x2048 (4096 patches each), 512 tokens per image, bf16, bench.py's
random-init full-size model, all 12 decoder layers and 16 heads, one process.  The tokens are the model's own greedy output with <eos>
suppressed; a random-init model never emits `measure`, so for the kernel and pass timings every --every-th token (default 16) is
overwritten with it - the passes are teacher-forced, any row will do - and for the end-to-end calls the delimiters are the decode's two
most frequent tokens.  Reported, each as median / min / max over --rounds (device events around the work, warmed up first, variants
interleaved):

  *_kernel_ms                the four C entries ALONE - acai_token_segments, acai_segment_reduce, acai_attn_map_segment_sum (and
                             acai_attn_map_weighted_sum, both launches, next to it), acai_attn_map_extent on the measure maps and on the
                             per-token maps - called through the library with outputs, tables and workspaces allocated beforehand: no
                             allocation, no upload, no host list work inside the timed window;
  segments_ms, reduce_ms     the wrappers, with their host work: ops.token_segments on the 8 x 513 tokens; ops.segment_reduce of 6 planes;
  ssum_ms, wsum_ms           ops.attn_map_segment_sum over the pass's 64 MB of maps (uniform weight, the layout given on the host) and
                             ops.attn_map_weighted_sum over the same buffer, per call: both read every map element once;
  extent_ms, extent_tok_ms   ops.attn_map_extent on the measure maps, and on all 4096 per-token maps;
  ssum_torch_ms              a torch restatement on the same GPU: index_add_ of the padded (B, T, S) maps along T (not bit-identical);
  reduce_torch_ms            the sums and extrema of the same planes with torch scatter_reduce_;
  combined_pass_ms           the combined confidence + alignment pass as confident_inference(uncertainty="entropy") runs it;
  report_pass_ms             the same pass with the measure report formed inside it (what measured_inference runs);
  measure_report_ms          ViTOMR.measure_report end to end on the padded memory (unpad, the pass without heat maps, the report);
  confident_ms, measured_ms  confident_inference(uncertainty="entropy") and measured_inference end to end (encode, decode, pass).
One JSON line on stdout, the same written to --out.  NOT measured here, and not measurable on random weights: whether cross-attention
localises measures on trained checkpoints, which layers, heads or weight do it best, any threshold on measure confidence.

  python tools/bench_measures.py --rounds 7 --out profiles/measures_bench.json
"""
import argparse
import ctypes
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--every", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    from acai_omr_amd import _lib, engine, ops
    from acai_omr_amd.inference.vitomr_inference import confident_inference, measured_inference, set_up_omr_inference
    from acai_omr_amd.measures import MeasureConfig, report_hook
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
    T, B = a.tokens + 1, a.images
    with torch.no_grad():
        lat32, _, lens = vitomr.encoder.forward_packed(imgs)
        with autocast(device_type="cuda", dtype=torch.bfloat16):
            mem = vitomr.transition_head.forward_packed(lat32)

    def ctx():
        return autocast(device_type="cuda", dtype=torch.bfloat16)

    with torch.no_grad(), ctx():
        seqs, lps, mask = vitomr._greedy_packed(None, mem, lens, T)   # cold: code objects, graph capture
    assert seqs.shape[1] == T and bool(mask.all()), "the rows did not run to the cap"
    ids, freq = torch.unique(seqs[:, 1:], return_counts=True)
    frequent = tuple(ids[torch.argsort(freq, descending=True)][:2].tolist())
    measure = dec.tokens_to_idxs["measure"]
    marked = seqs.clone()
    marked[:, 1::a.every] = measure
    cfg = MeasureConfig()

    def combined_pass():
        with torch.no_grad(), ctx():
            return vitomr._confidence_packed(None, mem, lens, marked, mask, 5, 1.0, True, "entropy", None, None, grids, P, True)

    def report_pass():
        with torch.no_grad(), ctx():
            hook = report_hook(cfg)
            vitomr._confidence_packed(None, mem, lens, marked, mask, 5, 1.0, True, "entropy", None, None, grids, P, True, measure=hook)
            return hook.report

    e2e_cfg = MeasureConfig(delimiters=frequent)

    def confident():
        return confident_inference(vitomr, imgs, "cuda", max_inference_len=T, uncertainty="entropy")

    def measured():
        return measured_inference(vitomr, imgs, "cuda", max_inference_len=T, measures=e2e_cfg)

    # the kernels' own inputs, from one combined pass
    lens_t = [a.tokens] * B
    tokens = marked[:, :a.tokens].reshape(-1)
    with torch.no_grad(), ctx():
        maps, offs, map_off, logits = dec._cross_attention_maps_flat(tokens, lens_t, None, mem, lens, None, None, 1, None, True)
    cu_t, cu_s = engine.cu_from_lens(lens_t, dev), engine.cu_from_lens(lens, dev)
    row_lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    seg, count, bounds = ops.token_segments(marked, row_lens, [measure], stop=dec.eos_idx, cap=cfg.max_measures)
    counts = count.tolist()
    planes = torch.rand(6, B, T, device=dev)
    ranges = torch.cat([bounds[i, :c] for i, c in enumerate(counts)]).contiguous() - 1
    layout = (lens_t, lens, offs)
    mout, moffs, mseg_off, cu_seg = ops.attn_map_segment_sum(maps, map_off, cu_t, cu_s, None, ranges, counts, layout=layout, check_ranges=False)
    gw = [w for _, w in grids]
    weights = torch.ones(B * a.tokens, device=dev)
    assert len(set(lens)) == 1 and offs == [i * a.tokens * lens[0] for i in range(B)], "the torch baseline wants equal image sizes"
    padded = maps.view(B, a.tokens, lens[0])
    seg_t = seg[:, 1:T].long().clamp(min=0)                  # map row t belongs to token index t + 1
    M = max(counts)

    def ssum_torch():
        out = torch.zeros(B, M, lens[0], device=dev)
        for b in range(B):
            out[b].index_add_(0, seg_t[b], padded[b])
        return out

    def reduce_torch():
        idx = seg.long().clamp(min=0)[None].expand(6, B, T)
        s = torch.zeros(6, B, M, device=dev).scatter_reduce_(2, idx, planes, "sum")
        lo = torch.full((6, B, M), float("inf"), device=dev).scatter_reduce_(2, idx, planes, "amin")
        hi = torch.full((6, B, M), float("-inf"), device=dev).scatter_reduce_(2, idx, planes, "amax")
        return s, lo, hi

    ref = ssum_torch()
    got = torch.stack([mout[o:o + c * lens[0]].view(c, lens[0]) for o, c in zip(moffs, counts)]) if len(set(counts)) == 1 else None
    ssum_diff = None if got is None else float((got - ref[:, :counts[0]]).abs().max() / ref.abs().max())
    del ref, got

    # the C entries alone: everything they write, and the weighted sum's workspace, exists before the timed window
    L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    f32, i32 = torch.float32, torch.int32
    k_seg, k_count, k_bounds = torch.empty_like(seg), torch.empty_like(count), torch.empty_like(bounds)
    k_red = [torch.empty(6, B, cfg.max_measures, dtype=d, device=dev) for d in (f32, f32, f32, i32, i32)]
    k_mout, k_ext, k_ext_tok = torch.empty_like(mout), torch.empty(sum(counts), 4, device=dev), torch.empty(B * a.tokens, 4, device=dev)
    k_heat, k_part = torch.empty(sum(lens), device=dev), torch.empty(-(-a.tokens // 32) * sum(lens), device=dev)
    delim_arr, gw_arr = (ctypes.c_int64 * 1)(measure), (ctypes.c_int32 * B)(*gw)
    ck = _lib.check

    def k_segments():
        ck(L.acai_token_segments(marked.data_ptr(), T, row_lens.data_ptr(), B, delim_arr, 1, dec.eos_idx, cfg.max_measures, k_seg.data_ptr(),
                                 k_count.data_ptr(), k_bounds.data_ptr(), st), "acai_token_segments")

    def k_reduce():
        ck(L.acai_segment_reduce(planes.data_ptr(), 6, B, T, bounds.data_ptr(), count.data_ptr(), cfg.max_measures, *(t.data_ptr() for t in k_red), st),
           "acai_segment_reduce")

    def k_ssum():
        ck(L.acai_attn_map_segment_sum(maps.data_ptr(), map_off.data_ptr(), cu_t.data_ptr(), cu_s.data_ptr(), None, ranges.data_ptr(), cu_seg.data_ptr(),
                                       mseg_off.data_ptr(), B, max(lens), max(counts), k_mout.data_ptr(), st), "acai_attn_map_segment_sum")

    def k_wsum():
        ck(L.acai_attn_map_weighted_sum(maps.data_ptr(), map_off.data_ptr(), cu_t.data_ptr(), cu_s.data_ptr(), weights.data_ptr(), B, a.tokens,
                                        max(lens), sum(lens), k_part.data_ptr(), k_heat.data_ptr(), st), "acai_attn_map_weighted_sum")

    def k_extent():
        ck(L.acai_attn_map_extent(mout.data_ptr(), mseg_off.data_ptr(), cu_seg.data_ptr(), cu_s.data_ptr(), gw_arr, B, max(counts), cfg.quantile,
                                  k_ext.data_ptr(), st), "acai_attn_map_extent")

    def k_extent_tok():
        ck(L.acai_attn_map_extent(maps.data_ptr(), map_off.data_ptr(), cu_t.data_ptr(), cu_s.data_ptr(), gw_arr, B, a.tokens, cfg.quantile,
                                  k_ext_tok.data_ptr(), st), "acai_attn_map_extent")

    k_ssum(), k_extent()
    assert torch.equal(k_mout, mout) and torch.equal(k_ext, ops.attn_map_extent(mout, mseg_off, cu_seg, cu_s, gw, cfg.quantile, layout=(counts, lens, moffs)))
    padded_mem = mem.view(B, lens[0], -1)

    def measure_report():
        with ctx():
            return vitomr.measure_report(padded_mem, None, marked, mask, config=cfg, grids=grids)

    variants = [
        ("segments_kernel_ms", k_segments, a.reps), ("reduce_kernel_ms", k_reduce, a.reps), ("ssum_kernel_ms", k_ssum, a.reps),
        ("wsum_kernel_ms", k_wsum, a.reps), ("extent_kernel_ms", k_extent, a.reps), ("extent_tok_kernel_ms", k_extent_tok, a.reps),
        ("measure_report_ms", measure_report, 1),
        ("segments_ms", lambda: ops.token_segments(marked, row_lens, [measure], stop=dec.eos_idx, cap=cfg.max_measures), a.reps),
        ("reduce_ms", lambda: ops.segment_reduce(planes, bounds, count), a.reps),
        ("reduce_torch_ms", reduce_torch, a.reps),
        ("ssum_ms", lambda: ops.attn_map_segment_sum(maps, map_off, cu_t, cu_s, None, ranges, counts, layout=layout, check_ranges=False), a.reps),
        ("wsum_ms", lambda: ops.attn_map_weighted_sum(maps, map_off, cu_t, cu_s, weights, a.tokens, layout=layout), a.reps),
        ("ssum_torch_ms", ssum_torch, a.reps),
        ("extent_ms", lambda: ops.attn_map_extent(mout, mseg_off, cu_seg, cu_s, gw, cfg.quantile, layout=(counts, lens, moffs)), a.reps),
        ("extent_tok_ms", lambda: ops.attn_map_extent(maps, map_off, cu_t, cu_s, gw, cfg.quantile, layout=layout), a.reps),
        ("combined_pass_ms", combined_pass, 1), ("report_pass_ms", report_pass, 1), ("confident_ms", confident, 1), ("measured_ms", measured, 1)]
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
    e2e_counts = measured()[4].count.tolist()
    out = dict(workload=f"{B} images of {a.height}x{a.width} ({lens[0]} patches each), {a.tokens} tokens per image, bf16, random-init full-size model, "
                        f"{len(dec.decoder_blocks.layers)} layers x {dec.num_heads} heads; `measure` written at every {a.every}th token for the kernels "
                        f"and the passes ({counts[0]} measures per row), the decode's two most frequent tokens {list(frequent)} as delimiters end to "
                        f"end (measures per row {e2e_counts}); device events, warmed up, variants interleaved, median / min / max of rounds; kernel "
                        f"variants per call over {a.reps} calls per window",
               rounds=a.rounds, reps=a.reps, device=torch.cuda.get_device_name(dev), **res,
               report_minus_combined_ms=med("report_pass_ms") - med("combined_pass_ms"),
               combined_pass_spread_ms=res["combined_pass_ms"]["max"] - res["combined_pass_ms"]["min"],
               measured_minus_confident_ms=med("measured_ms") - med("confident_ms"),
               confident_spread_ms=res["confident_ms"]["max"] - res["confident_ms"]["min"],
               ssum_torch_over_kernel=med("ssum_torch_ms") / med("ssum_ms"), reduce_torch_over_kernel=med("reduce_torch_ms") / med("reduce_ms"),
               map_bytes=map_bytes, ssum_map_read_bytes_per_s=map_bytes / (med("ssum_ms") * 1e-3),
               wsum_map_read_bytes_per_s=map_bytes / (med("wsum_ms") * 1e-3), hbm_copy_bytes_per_s=HBM_COPY_BYTES_PER_S,
               ssum_rate_over_wsum_rate=med("wsum_ms") / med("ssum_ms"),
               ssum_kernel_map_read_bytes_per_s=map_bytes / (med("ssum_kernel_ms") * 1e-3),
               wsum_kernel_map_read_bytes_per_s=map_bytes / (med("wsum_kernel_ms") * 1e-3),
               extent_tok_kernel_map_read_bytes_per_s=map_bytes / (med("extent_tok_kernel_ms") * 1e-3),
               ssum_kernel_rate_over_wsum_kernel_rate=med("wsum_kernel_ms") / med("ssum_kernel_ms"), max_rel_diff_ssum_kernel_vs_torch=ssum_diff,
               not_measured="whether cross-attention localises measures on trained checkpoints; which layers, heads or weight do it best; any "
                            "threshold on measure confidence (random-init weights)")
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
