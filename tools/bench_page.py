"""Whole-page input on one A4 page at 300 dpi (3508 x 2480, uint8) with ten synthetic two-staff systems, through
`DynamicResize(16, 1024, PE_MAX_HEIGHT, PE_MAX_WIDTH, False)` (the reference's inference transform, omr_teacher_force_train.py:24,281).
On the same GPU, in one process, it measures
  detect     page.detect_systems: the profile launch, the two systems launches and the one device-to-host copy (default DetectConfig);
  split      page.split_pages: every system cut out, resized and packed by one launch pair (one table upload, one scratch allocation);
  per_system the only path the parent commit offers for the same PackedPatches: a `.contiguous()` copy of every box and
             `DynamicResize.to_patches` over the copies (two launches and one scratch allocation per system) - alternated with `split`,
             after checking that the two write the same bits;
  page_inference and continuous_inference over `[resize(crop) ...]` on the benchmark model (bench.build_model: full size, random weights,
             <eos> suppressed) at --max-len tokens per system, alternated, and the share of detect + split in the former.
detect / split / per_system: host clock around --calls calls that end in a device synchronise, median (min .. max) of --reps windows;
the two inference calls: wall clock around one call each, --repeats times after a warm-up.  The launch counts are those of the code paths,
not traced.  Bytes: what each step has to read and write, from the shapes.  Writes one JSON line to profiles/page_bench.json and prints it.
Needs a GPU: there is no fallback.

    python tools/bench_page.py [--calls 50] [--reps 5] [--repeats 3] [--max-len 128] [--slots 16] [--no-model] [--out profiles/page_bench.json]
"""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, SYSTEMS = 3508, 2480, 10
MAX_IMG_SEQ_LEN = 1024


def a4_page(seed=0):
    """The page and the ink extents of its systems.  Paper 200..255, ink 0..90; per system two staves of five 3-pixel lines 20 rows apart,
    the staves 150 rows apart and joined by 4-pixel barlines every 400 columns, a few note heads between and around the lines; a title of
    short words at the top and a page number at the bottom."""
    rng = np.random.RandomState(seed)
    page = rng.randint(200, 256, size=(H, W)).astype(np.uint8)

    def ink(y0, y1, x0, x1):
        page[y0:y1, x0:x1] = rng.randint(0, 91, size=(y1 - y0, x1 - x0)).astype(np.uint8)

    for x in range(700, 1700, 90):
        ink(90, 150, x, x + 60)
    truth = []
    for s in range(SYSTEMS):
        top = 260 + s * 320
        bottom = top + 150 + 4 * 20 + 3
        for staff in (top, top + 150):
            for k in range(5):
                ink(staff + 20 * k, staff + 20 * k + 3, 200, 2280)
        for x in list(range(200, 2280, 400)) + [2276]:
            ink(top, bottom, x, x + 4)
        for x in rng.randint(260, 2200, size=40):
            y = int(rng.randint(top - 30, bottom + 10))
            ink(y, y + 14, int(x), int(x) + 18)
        ys = np.nonzero((page[top - 40:bottom + 40, :] < 100).any(1))[0]
        truth.append((200, top - 40 + int(ys[0]), 2280, top - 40 + int(ys[-1]) + 1))
    ink(3460, 3490, 1220, 1260)
    return page, truth


def windows(fn, calls, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / calls * 1e6)
    return out


def stat(xs, unit="us"):
    return {f"median_{unit}": statistics.median(xs), f"min_{unit}": min(xs), f"max_{unit}": max(xs), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-len", type=int, default=128)
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--no-model", action="store_true", help="skip the two inference calls (no model is built)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "page_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_page: needs a GPU (a CPU run says nothing about these kernels)")
    from acai_omr_amd.config import PE_MAX_HEIGHT, PE_MAX_WIDTH
    from acai_omr_amd.page import DetectConfig, detect_systems, plan_systems, split_pages
    from acai_omr_amd.utils import DynamicResize
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    resize = DynamicResize(16, MAX_IMG_SEQ_LEN, PE_MAX_HEIGHT, PE_MAX_WIDTH, False)
    page_np, truth = a4_page()
    page = torch.from_numpy(page_np).to(dev)
    cfg = DetectConfig()
    margin = cfg.resolved(H, W)[4]
    boxes = detect_systems(page, cfg)
    want = [(max(a - margin, 0), max(b - margin, 0), min(c + margin, W), min(d + margin, H)) for a, b, c, d in truth]
    assert boxes == want, (boxes, want)      # the detector finds the ten systems, and only them, before anything is timed
    plans = plan_systems([(H, W)], [boxes], resize)

    def split():
        return split_pages(page, boxes, resize, dtype=torch.bfloat16)

    def per_system():
        return resize.to_patches([page[y0:y1, x0:x1].contiguous() for x0, y0, x1, y1 in boxes], dtype=torch.bfloat16)

    a, b = split(), per_system()
    assert a.dims == b.dims and torch.equal(a.patches, b.patches)
    t_detect = windows(lambda: detect_systems(page, cfg), args.calls, args.reps)
    t_split, t_per = [], []
    for _ in range(args.reps):               # alternated: one window of each per round
        t_split += windows(split, args.calls, 1)
        t_per += windows(per_system, args.calls, 1)
    box_px = sum((y1 - y0) * (x1 - x0) for x0, y0, x1, y1 in boxes)
    tmp_px = sum((y1 - y0) * size[1] for _, (x0, y0, x1, y1), size, _ in plans)
    out_px = sum(c[2] * c[3] for *_, c in plans)
    res = {"when": datetime.datetime.now().isoformat(timespec="seconds"), "device": torch.cuda.get_device_name(0), "page": [H, W], "systems": len(boxes),
           "boxes": boxes, "targets": [list(s) for _, _, s, _ in plans], "calls": args.calls, "reps": args.reps,
           "detect": {**stat(t_detect), "launches": 3, "d2h_copies": 1,
                      "bytes_needed": H * W + box_px + 4 * 4 * H},        # the page once, the kept bands once more, the two profiles written and read
           "split": {**stat(t_split), "launches": 2, "h2d_copies": 1, "bytes_needed": box_px + 2 * 4 * tmp_px + 2 * out_px},
           "per_system": {**stat(t_per), "launches": 3 * len(boxes), "bytes_needed": 3 * box_px + 2 * 4 * tmp_px + 2 * out_px}}
    res["split_over_per_system"] = res["split"]["median_us"] / res["per_system"]["median_us"]
    if not args.no_model:
        import bench
        from acai_omr_amd.inference.vitomr_inference import continuous_inference, page_inference
        vit = bench.build_model(dev, args.slots)
        bench._suppress_eos(vit)
        pagef = (torch.from_numpy(page_np).float() / 255.0).to(dev)   # divided on the host: torch's device kernel multiplies by 1 / 255 instead

        def whole():
            return page_inference(vit, page, "cuda", resize, boxes=None, max_inference_len=args.max_len, slots=args.slots, detect=cfg)

        def parent():
            crops = [resize(pagef[None, y0:y1, x0:x1]) for x0, y0, x1, y1 in boxes]
            return continuous_inference(vit, crops, "cuda", max_inference_len=args.max_len, slots=args.slots)

        r, p = whole(), parent()
        torch.cuda.synchronize()
        res["rows_equal_parent_path"] = bool(torch.equal(r.seqs, p[0]) and torch.equal(r.seq_mask, p[2]))
        t_whole, t_parent = [], []
        for _ in range(args.repeats):
            for fn, acc in ((whole, t_whole), (parent, t_parent)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                acc.append((time.perf_counter() - t0) * 1e3)
        res["page_inference"] = {**stat(t_whole, "ms"), "max_len": args.max_len, "slots": args.slots, "tokens": int(r.seq_mask.sum())}
        res["continuous_inference_on_given_boxes"] = stat(t_parent, "ms")
        res["detect_plus_split_share_of_page_inference"] = (res["detect"]["median_us"] + res["split"]["median_us"]) / 1e3 / res["page_inference"]["median_ms"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
