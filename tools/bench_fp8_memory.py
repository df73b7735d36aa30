"""bf16 against FP8 (e4m3fn) memory cache on the headline workload (bench.py's decode: 8 x 512x2048 images, 4096 patches each, greedy steps
replayed from captured hipGraphs), in ONE process with the same weights and images, the variants interleaved round by round.

Reports per variant: median tokens/s and ms per step over the rounds, the warm prefill time (encoder + transition head + cross-K/V prefill,
and for FP8 the quantise pass), the time of one cross-attention launch as a step issues it (HIP events, cycling over the 12 layers) and its
achieved bytes per second on the bytes the launch must read, the time of one quantise launch (one layer), and the logit deviation of the FP8
engine from the bf16 one over teacher-forced steps.  One JSON line on stdout, the same written to --out.

  python tools/bench_fp8_memory.py --rounds 7 --steps 256 --out bench_outputs/fp8_memory.json
  python tools/bench_fp8_memory.py --only fp8 --rounds 1 --steps 64     (one variant: for a rocprofv3 --kernel-trace --stats run)
"""
import argparse
import json
import os
import sys
import time

import torch
from torch.amp import autocast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(dev, batch, mdt):
    from acai_omr_amd.inference.vitomr_inference import set_up_omr_inference
    torch.manual_seed(0)   # bench.py's weights
    vitomr, _ = set_up_omr_inference(os.path.join(ROOT, "lmx_vocab.txt"), max_batch_size=batch, cache_dtype=torch.bfloat16, device=dev,
                                     memory_cache_dtype=mdt)
    return vitomr.eval()


def prefill(vitomr, imgs):
    with torch.no_grad():
        lat32, _, lens = vitomr.encoder.forward_packed(imgs)
        with autocast(device_type="cuda", dtype=torch.bfloat16):
            mem = vitomr.transition_head.forward_packed(lat32)
        vitomr.decoder.decoder_blocks.prepare_caches_packed(None, mem, lens)
    return lens


def event_time(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn(0)
    torch.cuda.synchronize()
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e-3


def cross_attn_launch_s(eng, iters=48):
    """One cross-attention launch exactly as a step issues it (split over the memory, in-launch merge), cycling over the layers."""
    from acai_omr_amd import _lib, ops
    L = _lib.lib()
    q = torch.randn(eng.B, 3 * eng.E, device=eng.device)
    out = eng.ws["attn"]
    tk = eng.tickets.data_ptr() if L.acai_decode_merge_in_launch(_lib.ACAI_FP8_E4M3 if eng.cross_fp8 else _lib.ACAI_BF16, eng.cdhp) == 1 else None
    if eng.cross_fp8:
        f = lambda i: _lib.check(L.acai_decode_attn_fp8(  # noqa: E731
            q.data_ptr(), q.stride(0), eng.k_cross[i % eng.L].data_ptr(), eng.v_cross[i % eng.L].data_ptr(), eng.k_cross_scale[i % eng.L].data_ptr(),
            eng.v_cross_scale[i % eng.L].data_ptr(), eng.cross_off.data_ptr(), eng.cross_len.data_ptr(), eng.partial.data_ptr(), out.data_ptr(),
            out.stride(0), eng.B, eng.H, eng.dh, eng.cdhp, eng.cross_chunk, eng.cross_nsplit, 1, tk, ops._st()), "acai_decode_attn_fp8")
    else:
        f = lambda i: _lib.check(L.acai_decode_attn(  # noqa: E731
            q.data_ptr(), q.stride(0), eng.k_cross[i % eng.L].data_ptr(), eng.v_cross[i % eng.L].data_ptr(), eng.cross_off.data_ptr(),
            eng.cross_len.data_ptr(), eng.partial.data_ptr(), out.data_ptr(), out.stride(0), eng.B, eng.H, eng.dh, eng.dhp, eng.cross_chunk,
            eng.cross_nsplit, _lib.ACAI_BF16, 1, tk, ops._st()), "acai_decode_attn")
    return event_time(f, iters), tk is not None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--fp8-chunks", default="1024", help="keys per cross-attention workgroup of the FP8 variants (comma separated)")
    ap.add_argument("--only", choices=["bf16", "fp8"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1000)   # bench.py's rank-0 images
    imgs = [torch.rand(1, a.height, a.width, generator=g).to(dev) for _ in range(a.batch)]
    variants = []
    if a.only != "fp8":
        variants.append(("bf16", None, None))
    if a.only != "bf16":
        variants += [(f"fp8_chunk{c}", torch.float8_e4m3fn, int(c)) for c in a.fp8_chunks.split(",")]
    models, res = {}, {}
    for name, mdt, chunk in variants:
        if chunk is not None:
            os.environ["ACAI_CROSS_CHUNK_FP8"] = str(chunk)
        m = build(dev, a.batch, mdt)
        lens = prefill(m, imgs)   # cold: code objects, allocator
        torch.cuda.synchronize()
        pf = []
        for _ in range(3):
            t0 = time.perf_counter()
            prefill(m, imgs)
            torch.cuda.synchronize()
            pf.append(time.perf_counter() - t0)
        eng = m.decoder.decoder_blocks.engine(dev)
        models[name] = (m, eng)
        res[name] = dict(prefill_ms=sorted(pf)[1] * 1e3, cross_chunk=eng.cross_chunk, cross_nsplit=eng.cross_nsplit, tokens_per_s=[],
                         cross_kv_bytes=eng.cross_kv_bytes())
    os.environ.pop("ACAI_CROSS_CHUNK_FP8", None)
    H, S = models[variants[0][0]][1].H, lens[0]
    dh = models[variants[0][0]][1].dh

    # logit deviation FP8 - bf16 over teacher-forced steps (before the timing: logits_step leaves the stepwise state behind)
    if "bf16" in models and len(models) > 1:
        toks = torch.randint(3, 200, (48, a.batch), generator=torch.Generator().manual_seed(7)).to(dev)
        dev_max, dev_rel = 0.0, 0.0
        with torch.no_grad():
            eb = models["bf16"][1]
            for t in range(48):
                lb = eb.logits_step(toks[t], t).clone()
                for name, (m, e) in models.items():
                    if name != "bf16":
                        lf = e.logits_step(toks[t], t)
                        dev_max = max(dev_max, float((lf - lb).abs().max()))
                        dev_rel = max(dev_rel, float((lf - lb).abs().max() / lb.abs().max()))
        res["logit_deviation_vs_bf16"] = dict(max_abs=dev_max, max_rel_to_max_logit=dev_rel, steps=48, note="random-init weights (bench.py's)")

    # kernel-level: one cross-attention launch, one quantise launch
    from acai_omr_amd import ops
    for name, (m, eng) in models.items():
        t, fused = cross_attn_launch_s(eng)
        nbytes = res[name]["cross_kv_bytes"] / eng.L   # the bytes one launch must read: one layer's K/V (+ scales)
        res[name].update(cross_attn_launch_us=t * 1e6, cross_attn_bytes=nbytes, cross_attn_TBps=nbytes / t / 1e12, in_launch_merge=fused)
        if eng.cross_fp8:
            rows = sum(lens) * eng.H
            tq = event_time(lambda i: ops.cross_kv_quantize_fp8(eng.k_stage, eng.v_stage, eng.k_cross[i % eng.L], eng.v_cross[i % eng.L],
                                                                eng.k_cross_scale[i % eng.L], eng.v_cross_scale[i % eng.L], 0, rows, eng.cdhp), 24)
            qb = rows * eng.cdhp * (2 * 2 + 2 * 1) + rows * 8
            res[name].update(quantise_launch_us=tq * 1e6, quantise_bytes=qb, quantise_TBps=qb / tq / 1e12, quantise_ms_per_prefill=tq * eng.L * 1e3)

    # decode steps, interleaved
    cap = {}
    for name, (m, eng) in models.items():
        eng.stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(eng.stream):
            eng.arm(eng.B)
            eng.ensure_graph(1)
            eng.ensure_graph(eng.STEPS_PER_GRAPH)
            eng.arm(eng.B)
            eng.launch_steps(a.warmup)
        cap[name] = a.warmup
        torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, (m, eng) in models.items():
            with torch.cuda.stream(eng.stream):
                if cap[name] + a.steps > eng.Tmax - 2:
                    eng.arm(eng.B)
                    cap[name] = 0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.launch_steps(a.steps)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                cap[name] += a.steps
            res[name]["tokens_per_s"].append(a.batch * a.steps / dt)
    for name in models:
        tp = sorted(res[name]["tokens_per_s"])
        res[name]["median_tokens_per_s"] = tp[len(tp) // 2]
        res[name]["ms_per_step"] = a.batch / tp[len(tp) // 2] * 1e3
    if "bf16" in models:
        for name in models:
            if name != "bf16":
                res[name]["speedup_vs_bf16"] = res[name]["median_tokens_per_s"] / res["bf16"]["median_tokens_per_s"]
                res[name]["cross_attn_time_vs_bf16"] = res[name]["cross_attn_launch_us"] / res["bf16"]["cross_attn_launch_us"]
    out = dict(workload=f"{a.batch} x {a.height}x{a.width} images ({S} patches each), H {H}, d_h {dh}, greedy decode steps from hipGraphs",
               steps_per_round=a.steps, rounds=a.rounds, device=torch.cuda.get_device_name(dev), results=res)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
