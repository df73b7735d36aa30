"""Blank-patch pruning (acai_omr_amd/prune.py) against the unpruned path, in one process on one GPU, on SYNTHETIC systems only:
  a4        the A4 page of tools/bench_page.py (ten two-staff systems), through page_inference with its own detection;
  headline  the headline batch of 8 x 512 x 2048 (8 x 4096 patches), every image a synthetic two-staff system (synthetic_system below).
For halo 0 and 1 (the other thresholds at PruneConfig's defaults) it reports
  kept share      kept / total patches of these synthetic inputs - NOT a measurement of real scores;
  stage           prune_patches on the headline stream, and its parts one by one: the ink launch, the keep launch, the copy of the kept counts
                  to the host (which waits for the two launches before it) and the compact launch - host clock around --calls calls that
                  end in a device synchronise, median (min .. max) of --reps windows;
  encode          inference._encode_chunks (encoder + transition head) of the headline batch, pruned against unpruned, alternated;
  decode step     the graph-replayed greedy step on the prepared memories (as bench.py's config 4 times it), alternated, and
                  engine.cross_kv_bytes() after the FIRST prepare of each on a fresh engine, pruned first (the allocation grows with
                  sum(lens) and is kept, so later prepares report the larger one), next to the memory rows a step streams;
  page_inference  the whole call on the A4 page with prune= against prune=None, alternated, --repeats times after a warm-up.
Nothing here says what pruning does to the output of a trained checkpoint (the benchmark model has random weights), and no speed-up on real
data follows from it: the blank share of real systems has not been measured.
Kernel times come from a trace run of their own: `rocprofv3 --kernel-trace --stats -- python tools/bench_prune.py --trace-only` replays the
stage --calls times and times nothing itself.  Writes one JSON line to profiles/prune_bench.json and prints it.  Needs a GPU: no fallback.

    python tools/bench_prune.py [--calls 50] [--reps 5] [--repeats 3] [--steps 64] [--max-len 128] [--slots 16] [--trace-only] [--out ...]
"""
import argparse
import datetime
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HEADLINE = (8, 512, 2048)


def synthetic_system(seed, H, W):
    """A (1, H, W) float32 system: paper noise in 0.8 .. 1, ink in 0 .. 0.35; two staves of five 3-pixel lines 20 rows apart in the middle of
    the image, joined by barlines every 400 columns, and 40 note heads of 14 x 18 pixels scattered around the staves."""
    rng = np.random.RandomState(seed)
    img = (0.8 + 0.2 * rng.rand(H, W)).astype(np.float32)

    def ink(y0, y1, x0, x1):
        y0, y1, x0, x1 = max(y0, 0), min(y1, H), max(x0, 0), min(x1, W)
        img[y0:y1, x0:x1] = (0.35 * rng.rand(y1 - y0, x1 - x0)).astype(np.float32)

    top = H // 2 - 120
    bottom = top + 150 + 4 * 20 + 3
    for staff in (top, top + 150):
        for k in range(5):
            ink(staff + 20 * k, staff + 20 * k + 3, 40, W - 40)
    for x in list(range(40, W - 40, 400)) + [W - 44]:
        ink(top, bottom, x, x + 4)
    for x in rng.randint(80, W - 100, size=40):
        y = int(rng.randint(top - 30, bottom + 10))
        ink(y, y + 14, int(x), int(x) + 18)
    return torch.from_numpy(np.minimum(img, np.float32(0.999))).unsqueeze(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--max-len", type=int, default=128)
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--trace-only", action="store_true", help="replay the stage --calls times for a kernel trace; time and write nothing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prune_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_prune: needs a GPU (a CPU run says nothing about these kernels)")
    import bench
    from bench_page import a4_page, stat, windows
    from torch.amp import autocast

    from acai_omr_amd import ops
    from acai_omr_amd.config import PE_MAX_HEIGHT, PE_MAX_WIDTH
    from acai_omr_amd.inference.vitomr_inference import _encode_chunks, page_inference
    from acai_omr_amd.page import DetectConfig
    from acai_omr_amd.prune import PruneConfig, prune_patches
    from acai_omr_amd.utils import DynamicResize, PackedPatches
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    B, IH, IW = HEADLINE
    P = 16
    imgs = [synthetic_system(i, IH, IW).to(dev) for i in range(B)]
    dims = [(IH // P, IW // P)] * B
    patches = torch.empty(sum(h * w for h, w in dims), P * P, dtype=torch.float32, device=dev)
    r0 = 0
    for t in imgs:
        r0 += ops.patchify(t, P, patches, r0)
    stream = PackedPatches(patches, dims, P)
    pe_grid = (PE_MAX_HEIGHT, PE_MAX_WIDTH)
    cfgs = {0: PruneConfig(halo=0), 1: PruneConfig(halo=1)}
    if args.trace_only:
        for _ in range(args.calls):
            for cfg in cfgs.values():
                prune_patches(stream, cfg, pe_grid)
        torch.cuda.synchronize()
        return

    res = {"when": datetime.datetime.now().isoformat(timespec="seconds"), "device": torch.cuda.get_device_name(0), "inputs": "synthetic systems only",
           "headline": list(HEADLINE), "calls": args.calls, "reps": args.reps, "repeats": args.repeats, "halo": {}}
    vit = bench.build_model(dev, args.slots)
    bench._suppress_eos(vit)
    eng_blocks = vit.decoder.decoder_blocks

    def encode(x):
        with torch.no_grad():
            return _encode_chunks(vit, x, "cuda")

    def decode_ms(x):
        """(ms per greedy step on the memories of x, cross K/V bytes)"""
        mem, lens = encode(x)
        with torch.no_grad(), autocast(device_type="cuda", dtype=torch.bfloat16):
            eng_blocks.prepare_caches_packed(None, mem, lens)
        eng = eng_blocks.engine(dev)
        cur = torch.cuda.current_stream(dev)
        eng.stream.wait_stream(cur)
        with torch.cuda.stream(eng.stream):
            eng.arm(eng.B)
            eng.ensure_graph(1)
            eng.ensure_graph(eng.STEPS_PER_GRAPH)
            eng.arm(eng.B)
            eng.launch_steps(16)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.launch_steps(args.steps)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / args.steps * 1e3
        cur.wait_stream(eng.stream)
        return dt, eng.cross_kv_bytes(), lens

    resize = DynamicResize(16, 1024, PE_MAX_HEIGHT, PE_MAX_WIDTH, False)
    page_np, _ = a4_page()
    page = torch.from_numpy(page_np).to(dev)
    dcfg = DetectConfig()

    def whole(prune):
        return page_inference(vit, page, "cuda", resize, boxes=None, max_inference_len=args.max_len, slots=args.slots, detect=dcfg, prune=prune)

    for halo, cfg in cfgs.items():
        pruned = prune_patches(stream, cfg, pe_grid)
        out = {"config": {"ink_level": cfg.ink_level, "max_ink": cfg.max_ink, "halo": cfg.halo},
               "headline_kept": sum(pruned.kept_lens), "headline_total": patches.shape[0], "headline_kept_share": sum(pruned.kept_lens) / patches.shape[0]}
        # the stage and its parts
        table, rows, max_grid = ops.prune_table(dims, pe_grid, dev)
        ink = ops.patch_ink(patches, cfg.ink_level)
        kept_local, count = ops.patch_keep(ink, table, max_grid, cfg.max_ink, cfg.halo)
        counts = count.tolist()
        out["stage"] = {"prune_patches": stat(windows(lambda: prune_patches(stream, cfg, pe_grid), args.calls, args.reps)),
                        "patch_ink": stat(windows(lambda: ops.patch_ink(patches, cfg.ink_level), args.calls, args.reps)),
                        "patch_keep": stat(windows(lambda: ops.patch_keep(ink, table, max_grid, cfg.max_ink, cfg.halo), args.calls, args.reps)),
                        "counts_to_host": stat(windows(lambda: count.tolist(), args.calls, args.reps)),
                        "patch_compact": stat(windows(lambda: ops.patch_compact(patches, table, kept_local, counts), args.calls, args.reps)),
                        "launches": 3, "d2h_copies": 1,
                        "bytes_needed": patches.numel() * 4 + 2 * sum(counts) * P * P * 4}     # the stream read once, the kept rows read and written
        # encode and decode, alternated with the unpruned path
        t_enc = {"pruned": [], "unpruned": []}
        t_dec = {"pruned": [], "unpruned": []}
        kv = {}
        eng_blocks.__dict__["_engine"] = None      # a fresh engine: its cross K/V allocation starts from nothing
        encode(pruned), encode(stream)
        torch.cuda.synchronize()
        for _ in range(args.repeats):
            for name, x in (("pruned", pruned), ("unpruned", stream)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                encode(x)
                torch.cuda.synchronize()
                t_enc[name].append((time.perf_counter() - t0) * 1e3)
                ms, nbytes, lens = decode_ms(x)
                kv.setdefault(name, nbytes)
                t_dec[name].append(ms)
        out["encode_chunks"] = {k: stat(v, "ms") for k, v in t_enc.items()}
        out["decode_step"] = {k: stat(v, "ms") for k, v in t_dec.items()}
        out["cross_kv_bytes"] = kv
        out["memory_rows"] = {"pruned": sum(pruned.kept_lens), "unpruned": patches.shape[0]}
        # the page call
        r, p = whole(cfg), whole(None)
        torch.cuda.synchronize()
        out["a4_kept"], out["a4_total"] = sum(r.patches_kept), sum(r.patches_total)
        out["a4_kept_share"] = out["a4_kept"] / out["a4_total"]
        out["a4_systems"] = len(r)
        t_page = {"pruned": [], "unpruned": []}
        for _ in range(args.repeats):
            for name, pr in (("pruned", cfg), ("unpruned", None)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                whole(pr)
                torch.cuda.synchronize()
                t_page[name].append((time.perf_counter() - t0) * 1e3)
        out["page_inference"] = {**{k: stat(v, "ms") for k, v in t_page.items()}, "max_len": args.max_len, "slots": args.slots}
        res["halo"][str(halo)] = out
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
