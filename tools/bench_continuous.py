"""Continuous batching against static batching on the full-size model (random weights, <eos> suppressed as in bench.py), 512x2048 systems
(4096 patches), per-image caps drawn from a seeded uniform distribution.
python tools/bench_continuous.py [--images 64] [--slots 8 32] [--cap-lo 128] [--cap-hi 1024] [--repeats 3] [--single 4] [--seed 0]
Reports, per slot count: wall time and generated tokens/s of static batching (inference() over consecutive chunks of `slots` images, each
chunk run to its own largest cap) and of continuous batching; one image at a time for the first --single images; the ideal step ratio from
the caps; the slot step against the greedy step at the same rows and patches (graph replays, device events); encode and prefill times."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def wall(fn, repeats):
    fn()   # warm-up (graph capture, first-use code loads)
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def step_time(eng, rows, slot, steps=64, repeats=5):
    """Milliseconds per decode step, graph-replayed, device events: the greedy step, or the slot step with every row busy (the engine
    prepared with `rows` copies of one memory, which is also the slot layout: region s at offset s * Scap * H * dhp)."""
    import ctypes
    from acai_omr_amd import _lib, ops
    res = []
    cur = torch.cuda.current_stream()
    eng.stream.wait_stream(cur)
    with torch.cuda.stream(eng.stream):
        eng._mode = ("slot",) if slot else ("greedy",)
        eng.arm(rows)
        eng.ensure_graph(eng.STEPS_PER_GRAPH)
        rl = torch.tensor([list(range(rows)), [eng.Tmax] * rows], dtype=torch.int32).to(eng.device)
        for r in range(repeats + 1):
            eng.arm(rows)
            if slot:
                eng.cross_len[:rows].fill_(eng.lens[0])
                _lib.check(_lib.lib().acai_decode_slot_arm(ctypes.byref(eng._desc), ctypes.byref(eng._slot_desc), rl.data_ptr(), rows,
                                                           ops._st()), "acai_decode_slot_arm")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.launch_steps(steps)
            e1.record()
            e1.synchronize()
            if r:
                res.append(e0.elapsed_time(e1) / steps)
        eng._mode = ("greedy",)
    cur.wait_stream(eng.stream)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--slots", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--cap-lo", type=int, default=128)
    ap.add_argument("--cap-hi", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--single", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from acai_omr_amd.inference.vitomr_inference import _encode_chunks, continuous_inference, inference
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(a.seed)
    caps = torch.randint(a.cap_lo, a.cap_hi + 1, (a.images,), generator=g).tolist()
    imgs = [torch.rand(1, 512, 2048, generator=g) for _ in range(a.images)]
    tokens = sum(c - 1 for c in caps)
    for S in a.slots:
        vit = bench.build_model(dev, max(S, 8))
        bench._suppress_eos(vit)
        chunks = [list(range(c, min(c + S, a.images))) for c in range(0, a.images, S)]
        ideal_static = sum(max(caps[i] - 1 for i in ch) for ch in chunks)
        ideal_cont = -(-tokens // S)

        def static():
            for ch in chunks:
                inference(vit, [imgs[i] for i in ch], "cuda", max_inference_len=max(caps[i] for i in ch))

        def cont():
            continuous_inference(vit, imgs, "cuda", max_inference_len=caps, slots=S)

        def encode():
            with torch.no_grad():
                _encode_chunks(vit, imgs, "cuda")
        ts, tc, te = wall(static, a.repeats), wall(cont, a.repeats), wall(encode, a.repeats)
        eng = vit.decoder.decoder_blocks.engine(dev)
        cont_steps = eng.slot_steps
        # prefill of one image's cross K/V (every layer), as a refill does it
        with torch.no_grad():
            mem, lens = _encode_chunks(vit, imgs[:1], "cuda")
        blocks = vit.decoder.decoder_blocks
        tp = wall(lambda: blocks.prepare_caches_packed(None, mem, lens), a.repeats)
        # step times at S rows x 4096 patches
        rows = min(S, blocks.max_batch_size)
        memS = mem.repeat(rows, 1)
        blocks.prepare_caches_packed(None, memS, lens * rows)
        greedy_step = step_time(eng, rows, False)
        eng._slot_setup(lens[0], rows)
        slot_step = step_time(eng, rows, True)
        out = {"slots": S, "images": a.images, "caps": {"lo": a.cap_lo, "hi": a.cap_hi, "mean": tokens / a.images + 1, "seed": a.seed},
               "generated_tokens": tokens,
               "static": {"wall_s": spread(ts), "tokens_per_s": tokens / statistics.median(ts), "ideal_steps": ideal_static},
               "continuous": {"wall_s": spread(tc), "tokens_per_s": tokens / statistics.median(tc), "steps_run": cont_steps,
                              "ideal_steps": ideal_cont},
               "ideal_step_ratio": ideal_static / ideal_cont,
               "measured_speedup": statistics.median(ts) / statistics.median(tc),
               "fraction_of_ideal": (statistics.median(ts) / statistics.median(tc)) / (ideal_static / ideal_cont),
               "encode_s": spread(te), "prefill_one_image_s": spread(tp),
               "greedy_step_ms": spread(greedy_step), "slot_step_ms": spread(slot_step),
               "slot_over_greedy_step": statistics.median(slot_step) / statistics.median(greedy_step)}
        if a.single:
            sub = list(range(min(a.single, a.images)))

            def single():
                for i in sub:
                    inference(vit, [imgs[i]], "cuda", max_inference_len=caps[i])
            t1 = wall(single, max(1, a.repeats - 1))
            out["one_at_a_time"] = {"images": len(sub), "wall_s": spread(t1), "tokens_per_s": sum(caps[i] - 1 for i in sub) / statistics.median(t1)}
        print(json.dumps(out), flush=True)
        del vit, eng, blocks
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
