"""Page illumination flattening on the A4 page of tools/bench_page.py (3508 x 2480 uint8, ten synthetic two-staff systems) under a horizontal
brightness ramp from 1.0 to --lo (0.35).  Before anything is timed the tool checks that the detector loses systems of the shaded page and
that the flattened page gives the unshaded page's boxes again.  On the same GPU, in one process, it then measures
  tile_levels, flatten     one call of ops.page_tile_levels / ops.page_flatten each (the default tile of the page, 64), uint8 and fp32;
  flatten_pages            both, end to end (two launches, nothing comes back to the host);
  torch_flatten            a plain torch restatement on the same GPU, alternated with ours window by window: the tiles by a view and
                           `kthvalue` (whole tiles only - the partial last tile row and column take their neighbours' level), the rescue
                           by `max_pool2d`, the background by `F.interpolate` (bilinear, float weights) and a divide, rounded to uint8.
                           The same work, not the same bits: the share of pixels that differ is reported;
  page_inference           `flatten=True` on the shaded page against `flatten=None` on the unshaded page - the present path, which this
                           feature leaves as the parent commit has it - alternated (benchmark model of bench.build_model, <eos> suppressed,
                           --max-len tokens per system), and flatten_pages' share of the former.
Per-call figures: host clock around --calls calls that end in a device synchronise, median (min .. max) of --reps windows; the inference
calls: wall clock around one call each, --repeats times after a warm-up.  Bytes: what each kernel has to read and write, from the shapes;
`bound_us` is that over --bandwidth (6.3 TB/s, the achievable HBM rate), and `fraction_of_bound` needs the KERNEL time, which a separate
`rocprofv3 --kernel-trace --stats` run of this tool gives (--kernel-stats CSV: read if present).  Synthetic shading on a synthetic page:
nothing here says how the defaults do on real photographs.
Writes one JSON line to --out and prints it.  Needs a GPU: there is no fallback.

    python tools/bench_flatten.py [--calls 50] [--reps 5] [--repeats 3] [--max-len 128] [--slots 16] [--no-model] [--out profiles/flatten_bench.json]
"""
import argparse
import csv
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

from bench_page import H, MAX_IMG_SEQ_LEN, SYSTEMS, W, a4_page, stat, windows   # noqa: E402


def torch_flatten(page, T, percent, rq, floor):
    """Flattening as plain torch offers it (uint8 in and out)."""
    GH, GW = page.shape[0] // T, page.shape[1] // T
    tiles = page[:GH * T, :GW * T].view(GH, T, GW, T).permute(0, 2, 1, 3).reshape(GH, GW, T * T)
    g = tiles.kthvalue(max(1, (T * T * percent + 99) // 100), dim=2).values.float()[None, None]
    m = torch.nn.functional.max_pool2d(g, 3, 1, 1)
    s = torch.where(g * 256 < m * rq, m, g).clamp_(min=floor)
    bg = torch.nn.functional.interpolate(s, size=(GH * T, GW * T), mode="bilinear", align_corners=False)
    bg = torch.nn.functional.pad(bg, (0, page.shape[1] - GW * T, 0, page.shape[0] - GH * T), mode="replicate")[0, 0]
    return (page.float() * 255.0 / bg).add_(0.5).clamp_(max=255.0).to(torch.uint8)


def kernel_times(path):
    """Kernel name -> average microseconds, from a rocprofv3 --stats CSV (kernel_stats): {} when there is none."""
    if not path or not os.path.exists(path):
        return {}
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            for key in ("page_tile_levels_kernel<unsigned char>", "page_tile_levels_kernel<float>", "page_flatten_kernel<unsigned char>", "page_flatten_kernel<float>"):
                if key in name:
                    out[key] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-len", type=int, default=128)
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--lo", type=float, default=0.35, help="brightness at the right edge (1.0 at the left one)")
    ap.add_argument("--bandwidth", type=float, default=6.3e12, help="achievable HBM bytes / s the bytes-moved bound is taken against")
    ap.add_argument("--kernel-stats", default=os.path.join(ROOT, "profiles", "flatten_bench_kernel_stats.csv"))
    ap.add_argument("--no-model", action="store_true", help="skip the two inference calls (no model is built)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flatten_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_flatten: needs a GPU (a CPU run says nothing about these kernels)")
    from acai_omr_amd import ops
    from acai_omr_amd.config import PE_MAX_HEIGHT, PE_MAX_WIDTH
    from acai_omr_amd.page import DetectConfig, FlattenConfig, detect_systems, flatten_pages
    from acai_omr_amd.utils import DynamicResize
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    cfg, det = FlattenConfig(), DetectConfig()
    T, percent, rq, floor = cfg.resolved(H)
    page_np, _ = a4_page()
    gain = 1.0 + (args.lo - 1.0) * np.arange(W) / (W - 1)
    shaded_np = np.floor(page_np.astype(np.float64) * gain[None, :] + 0.5).astype(np.uint8)
    level, shaded = torch.from_numpy(page_np).to(dev), torch.from_numpy(shaded_np).to(dev)
    (flat,) = flatten_pages(shaded, cfg)
    found_level, found_shaded, found = detect_systems(level, det), detect_systems(shaded, det), detect_systems(flat, det)
    assert len(found_level) == SYSTEMS and len(found_shaded) < SYSTEMS and found == found_level, (len(found_level), len(found_shaded), len(found))
    mask_diff = int(((flat < 128) != (level < 128)).sum())

    GH, GW = -(-H // T), -(-W // T)
    shaded_f = shaded.float() / 255.0
    g = ops.page_tile_levels(shaded, T, percent)
    out_u8, out_f32 = torch.empty_like(shaded), torch.empty_like(shaded_f)
    t_pages = windows(lambda: flatten_pages(shaded, cfg), args.calls, args.reps)
    theirs = torch_flatten(shaded, T, percent, rq, floor)
    differ = float((theirs != flat).float().mean())
    t_levels, t_levels_f32, t_flatten, t_flatten_f32, t_torch = [], [], [], [], []
    few = max(1, args.calls // 10)                               # the torch restatement takes milliseconds a call
    for _ in range(args.reps):
        t_levels += windows(lambda: ops.page_tile_levels(shaded, T, percent), args.calls, 1)
        t_levels_f32 += windows(lambda: ops.page_tile_levels(shaded_f, T, percent), args.calls, 1)
        t_flatten += windows(lambda: ops.page_flatten(shaded, g, T, rq, floor, out=out_u8), args.calls, 1)
        t_flatten_f32 += windows(lambda: ops.page_flatten(shaded_f, g, T, rq, floor, out=out_f32), args.calls, 1)
        t_torch += windows(lambda: torch_flatten(shaded, T, percent, rq, floor), few, 1)

    kt = kernel_times(args.kernel_stats)

    def kernel(name, nbytes):
        d = {"bytes_needed": nbytes, "bound_us": nbytes / args.bandwidth * 1e6}
        if name in kt:
            d.update(kernel_us=kt[name]["avg_us"], kernel_min_us=kt[name]["min_us"], fraction_of_bound=d["bound_us"] / kt[name]["avg_us"])
        return d

    res = {"when": datetime.datetime.now().isoformat(timespec="seconds"), "device": torch.cuda.get_device_name(0), "page": [H, W], "ramp_to": args.lo,
           "tile": T, "percent": percent, "rq": rq, "floor": floor, "grid": [GH, GW], "calls": args.calls, "reps": args.reps,
           "bandwidth_for_bound": args.bandwidth,
           "systems_found": {"unshaded": len(found_level), "shaded": len(found_shaded), "flattened": len(found)},
           "flattened_boxes_equal_unshaded": found == found_level, "ink_mask_pixels_differing_from_unshaded": mask_diff,
           "tile_levels_u8": {**stat(t_levels), "launches": 1, **kernel("page_tile_levels_kernel<unsigned char>", H * W + GH * GW)},
           "tile_levels_f32": {**stat(t_levels_f32), "launches": 1, **kernel("page_tile_levels_kernel<float>", 4 * H * W + GH * GW)},
           "flatten_u8": {**stat(t_flatten), "launches": 1, **kernel("page_flatten_kernel<unsigned char>", 2 * H * W)},
           "flatten_f32": {**stat(t_flatten_f32), "launches": 1, **kernel("page_flatten_kernel<float>", 8 * H * W)},
           "flatten_pages": {**stat(t_pages), "launches": 2, "d2h_copies": 0},
           "torch_flatten_u8": {**stat(t_torch), "calls": few, "share_of_pixels_differing_from_ours": differ}}
    res["torch_over_ours"] = res["torch_flatten_u8"]["median_us"] / res["flatten_pages"]["median_us"]
    if not args.no_model:
        import bench
        from acai_omr_amd.inference.vitomr_inference import page_inference
        resize = DynamicResize(16, MAX_IMG_SEQ_LEN, PE_MAX_HEIGHT, PE_MAX_WIDTH, False)
        vit = bench.build_model(dev, args.slots)
        bench._suppress_eos(vit)

        def with_flatten():
            return page_inference(vit, shaded, "cuda", resize, max_inference_len=args.max_len, slots=args.slots, detect=det, flatten=cfg)

        def without():
            return page_inference(vit, level, "cuda", resize, max_inference_len=args.max_len, slots=args.slots, detect=det)

        r, p = with_flatten(), without()
        before = page_inference(vit, flat, "cuda", resize, max_inference_len=args.max_len, slots=args.slots, detect=det)
        torch.cuda.synchronize()
        res["rows_equal_flattened_beforehand"] = bool(torch.equal(r.seqs, before.seqs) and torch.equal(r.seq_mask, before.seq_mask) and r.boxes == before.boxes)
        res["boxes_equal_unshaded"] = r.boxes == p.boxes
        t_with, t_without = [], []
        for _ in range(args.repeats):
            for fn, acc in ((with_flatten, t_with), (without, t_without)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                acc.append((time.perf_counter() - t0) * 1e3)
        res["page_inference_flatten_shaded"] = {**stat(t_with, "ms"), "max_len": args.max_len, "slots": args.slots, "tokens": int(r.seq_mask.sum())}
        res["page_inference_unshaded_present_path"] = stat(t_without, "ms")
        res["flatten_share_of_page_inference"] = res["flatten_pages"]["median_us"] / 1e3 / res["page_inference_flatten_shaded"]["median_ms"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
