"""Sampled rollouts: static batches against continuous batching on the headline decoder (random weights, <eos> suppressed as in bench.py),
group size 1, top_k 50, temperature 1.1, per-sequence caps drawn once from a seeded spread to stand in for rows that end at different times.
python tools/bench_continuous_sample.py [--sequences 128] [--slots 16 64] [--cap-lo 100] [--cap-hi 768] [--repeats 5] [--patches 4096]
       [--out profiles/continuous_sample_bench.json]
(a) static sampling (DecodeEngine.sample) over consecutive batches of `slots` sequences, each batch run to its largest cap - the only way
    before the sampled slot step; (b) DecodeEngine.continuous(sample=...) with the same `slots`.  Both start from the encoded memories (the
    encoder is common to both), are warmed up at every shape, alternate a, b, a, b ... in one process, and every timing ends in a device
    synchronise.  Reports wall time (median, min, max), sequences/s, tokens/s (tokens a rollout keeps: cap - 1 per sequence), decode steps
    and the mean occupied slots per step (static: rows still below their own cap, averaged over the steps run)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=128)
    ap.add_argument("--slots", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--cap-lo", type=int, default=100)
    ap.add_argument("--cap-hi", type=int, default=768)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--patches", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    N, top_k, temperature = a.sequences, 50, 1.1
    g = torch.Generator().manual_seed(a.seed)
    caps = torch.randint(a.cap_lo, a.cap_hi + 1, (N,), generator=g).tolist()
    U = torch.rand(N, max(caps), generator=g).to(dev)
    tokens = sum(c - 1 for c in caps)
    results = []
    for S in a.slots:
        vit = bench.build_model(dev, S)
        bench._suppress_eos(vit)
        blocks = vit.decoder.decoder_blocks
        eng = blocks.engine(dev)
        E = vit.decoder.pos_embedding.shape[-1]
        lens = [a.patches] * N
        mem = torch.randn(N * a.patches, E, generator=torch.Generator().manual_seed(a.seed + 1)).to(torch.bfloat16).to(dev)
        chunks = [list(range(c, min(c + S, N))) for c in range(0, N, S)]
        static_steps = sum(max(caps[i] for i in ch) - 1 for ch in chunks)
        static_busy = sum(caps[i] - 1 for i in range(N))

        def static():
            for ch in chunks:
                w = max(caps[i] for i in ch)
                blocks.prepare_caches_packed(None, mem[ch[0] * a.patches:(ch[-1] + 1) * a.patches], [a.patches] * len(ch))
                seqs, lps, _ = eng.sample(w, top_k, temperature, uniforms=U[ch[0]:ch[-1] + 1, :w])
                vit.mask_and_clip_seqs(seqs.clone(), lps.clone())

        def cont():
            vit._continuous_packed(None, mem, lens, caps, S, sample=(top_k, temperature), uniforms=U)

        ta, tb = [], []
        with torch.no_grad():
            static()
            cont()   # warm-up of every shape: graph capture, first-use code loads
            for _ in range(a.repeats):
                for fn, out in ((static, ta), (cont, tb)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    out.append(time.perf_counter() - t0)
        ma, mb = statistics.median(ta), statistics.median(tb)
        res = {"slots": S, "sequences": N, "patches": a.patches, "top_k": top_k, "temperature": temperature,
               "caps": {"lo": a.cap_lo, "hi": a.cap_hi, "mean": sum(caps) / N, "max": max(caps), "seed": a.seed}, "kept_tokens": tokens,
               "static": {"wall_s": spread(ta), "sequences_per_s": N / ma, "tokens_per_s": tokens / ma, "steps": static_steps,
                          "mean_occupied_slots": static_busy / static_steps, "spread_rel": (max(ta) - min(ta)) / ma},
               "continuous": {"wall_s": spread(tb), "sequences_per_s": N / mb, "tokens_per_s": tokens / mb, "steps": eng.slot_steps,
                              "mean_occupied_slots": eng.slot_busy / max(1, eng.slot_steps), "spread_rel": (max(tb) - min(tb)) / mb},
               "speedup": ma / mb}
        print(json.dumps(res), flush=True)
        results.append(res)
        del vit, eng, blocks, mem
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
