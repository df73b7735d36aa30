"""Time one `CameraAugment` call (acai_omr_amd/augment.py: blur + noise + rotation + perspective + jitter, every image applied, the fine-tune
recipe at its widest parameters, noise drawn by torch.randn on the device) on the two batches a training step feeds it:
  flat    32 images of 512 x 2048 (the benchmarked MAE batch);
  ragged  config 5's shard of 32: the eight shapes of SURVEY section 8(d), 256 x 1024 ... 768 x 3072, four times;
in the image form (fp32 images out) and the bf16 patch form (rows of the packed patch stream out).  Reports milliseconds per call (host
clock around `--calls` calls that end in a device synchronise, median of `--reps` windows), the kernel launches per call (counted from the
stage list; `rocprofv3 --kernel-trace --stats -- python tools/bench_augment.py --images 8` against `--images 32` shows the same count in
the trace), and the bytes the algorithm has to move (each stage reads and writes every pixel once, the noise is written and read once)
over that time.  `--cpu-reference` also times the CPU restatement of the tests (tests/augment_reference.py, float32) on one 512 x 2048 image
with the threads the process has.  Writes one JSON line to profiles/augment_bench.json and prints it.  Needs a GPU: there is no fallback.

    python tools/bench_augment.py [--images 32] [--calls 50] [--reps 5] [--cpu-reference] [--mae-step-ms MS] [--out profiles/augment_bench.json]
"""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIG4_SHAPES = [(256, 1024), (256, 2048), (384, 1536), (512, 2048), (512, 3072), (640, 2560), (768, 2304), (768, 3072)]
P = 16


def widest_params(aug, sizes):
    from acai_omr_amd.augment import ImageParams
    out = []
    for i, (h, w) in enumerate(sizes):
        bh, bw = int(0.2 * (h // 2)) + 1, int(0.2 * (w // 2)) + 1
        out.append(ImageParams(sigma=0.7, noise_sigma=0.03, angle=2.0 if i % 2 else -2.0, endpoints=[(bw - 1, bh - 1), (w - bw, bh - 1), (w - bw, h - bh), (bw - 1, h - bh)],
                               brightness=1.15, contrast=0.8, brightness_first=bool(i % 2)))
    return out


def bytes_moved(sizes, patch_bf16):
    """What the algorithm needs: blur rows, blur columns (+ the noise), rotation, perspective: read + write fp32 each; the mean: one read; the
    last stage: one read and one write (2 bytes a pixel in the bf16 patch form); torch.randn's write of the noise."""
    px = sum(h * w for h, w in sizes)
    return px * (4 * (2 + 3 + 2 + 2 + 1 + 1) + (2 if patch_bf16 else 4) + 4)


def time_calls(fn, calls, reps):
    fn()
    torch.cuda.synchronize()
    windows = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t0) / calls * 1e3)
    return statistics.median(windows), min(windows), max(windows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-reference", action="store_true")
    ap.add_argument("--mae-step-ms", type=float, default=None, help="MAE step time of 32 images of 512 x 2048 measured in the same session (bench.py --full, "
                    "tools/prof_leg.py mae): recorded, with the augmentation's share of it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment: needs a GPU (a CPU run says nothing about this kernel)")
    from acai_omr_amd import augment as A
    dev = torch.device("cuda", 0)
    aug = A.fine_tune_camera_augment(p=1.0)
    launches = {"hip": 2 + 1 + 1 + 2, "torch_randn": 1, "h2d_copies": 1}
    res = {"when": datetime.datetime.now().isoformat(timespec="seconds"), "device": torch.cuda.get_device_name(0), "images": args.images, "calls": args.calls, "reps": args.reps,
           "recipe": "fine-tune (blur 15 taps sigma 0.7, noise 0.03, rotation +-2, perspective 0.2, brightness 1.15 / contrast 0.8), every image applied",
           "launches_per_call": launches, "workloads": {}}
    g = torch.Generator().manual_seed(0)
    for name, sizes in (("flat", [(512, 2048)] * args.images), ("ragged", [CONFIG4_SHAPES[i % 8] for i in range(args.images)])):
        imgs = [torch.rand(1, h, w, generator=g).to(dev) for h, w in sizes]
        params = widest_params(aug, sizes)
        # the two forms agree before anything is timed
        outs = aug(imgs, params=[A.ImageParams(**{**p.__dict__, "noise": torch.zeros(h, w, device=dev)}) for p, (h, w) in zip(params, sizes)])
        assert all(o.shape == im.shape and bool(torch.isfinite(o).all()) for o, im in zip(outs, imgs))
        for form, fn, bf16 in (("image_fp32", lambda: aug(imgs, params=params), False),
                               ("patches_bf16", lambda: aug.to_patches(imgs, P, dtype=torch.bfloat16, params=params), True)):
            med, lo, hi = time_calls(fn, args.calls, args.reps)
            nbytes = bytes_moved(sizes, bf16)
            res["workloads"][f"{name}/{form}"] = {"ms_per_call": med, "ms_min": lo, "ms_max": hi, "pixels": sum(h * w for h, w in sizes), "bytes_needed": nbytes,
                                                   "GBps_needed_bytes_over_call_time": nbytes / med / 1e6, "images_per_s": args.images / med * 1e3}
    if args.mae_step_ms:
        ms = res["workloads"]["flat/patches_bf16"]["ms_per_call"] * 32 / args.images
        res["mae_step_ms_same_session"] = args.mae_step_ms
        res["share_of_mae_step_32_images"] = ms / args.mae_step_ms
    if args.cpu_reference:
        import augment_reference as R
        img = R.staff_image(512, 2048)
        p = widest_params(aug, [(512, 2048)])[0]
        p.noise = torch.randn(512, 2048, generator=g)
        R.augment(img, p, dtype=torch.float32)
        t0 = time.perf_counter()
        for _ in range(3):
            R.augment(img, p, dtype=torch.float32)
        res["cpu_restatement"] = {"ms_per_image_512x2048_fp32": (time.perf_counter() - t0) / 3 * 1e3, "torch_threads": torch.get_num_threads()}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
