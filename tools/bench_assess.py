"""Page assessment (acai_omr_amd/page.py: estimate_staff_scale / assess_pages; csrc/assess.hip) on the A4 page of tools/bench_page.py
(3508 x 2480 uint8, ten synthetic two-staff systems), in one process on one GPU.  It reports
  page_runs, page_sharpness   ops.page_runs (two launches) and ops.page_sharpness (one launch) into zeroed words that are reused, and with
                   the allocation and fill of their own that a bare call makes;
  page_col_profile, page_profile   the nearest existing one-read kernels, on the same page, for scale;
  torch            a torch restatement of each on the same GPU (run lengths from the positions where a column changes colour and
                   bincount; the Laplacian from five shifted slices and bincount of the levels), after checking that it gives the same
                   integers;
  assess_pages     the whole call: one fill, three launches, ONE copy to the host, and the host's integers and float64;
  page_inference   assess=True against assess=None on that page, alternated, --repeats times after a warm-up, with the spread of the
                   assess=None path next to the difference (both find the page's ten systems; its lines are 20 rows apart, H / 175, so
                   sized from the music the margin is 36 rows where the canvas gives 35, and the boxes and rows are compared and reported).
Host clock around --calls calls that end in a device synchronise, median (min .. max) of --reps windows.  Kernel times come from a trace
run of their own: `rocprofv3 --kernel-trace --stats -- python tools/bench_assess.py --trace-only` replays the four ops --calls times and
times nothing itself.  The page is SYNTHETIC: nothing here says what the numbers of `PageQuality` are on a real photograph, and no gate
threshold follows from it.  Writes one JSON line to profiles/assess_bench.json and prints it.  Needs a GPU: no fallback.

    python tools/bench_assess.py [--calls 50] [--reps 5] [--repeats 3] [--max-len 128] [--slots 16] [--no-model] [--trace-only] [--out ...]
"""
import argparse
import datetime
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def torch_runs(page, ink_threshold=0.5):
    """ops.page_runs restated with torch ops on the page's device (uint8 pages)."""
    H, W = page.shape
    m = (page.float() / 255.0 < ink_threshold).t().contiguous()                   # [W, H]: a column is a row
    start = torch.ones(W, H, dtype=torch.bool, device=page.device)
    start[:, 1:] = m[:, 1:] != m[:, :-1]
    pos = torch.nonzero(start.flatten()).flatten()                                 # every run's first pixel, column after column
    length = torch.diff(pos, append=torch.tensor([W * H], device=page.device))
    ink = m.flatten()[pos]
    first = pos % H == 0
    last = (pos + length) % H == 0
    closed = ~first & ~last
    n = length.clamp(max=255)
    hist = torch.zeros(3, 256, dtype=torch.int64, device=page.device)
    hist[0] = torch.bincount(n[closed & ink], minlength=256)
    hist[1] = torch.bincount(n[closed & ~ink], minlength=256)
    pair = closed[:-1] & ink[:-1] & closed[1:] & ~first[1:]                        # the run after it is in the same column, and closed
    hist[2] = torch.bincount((length[:-1] + length[1:])[pair].clamp(max=255), minlength=256)
    return hist


def torch_sharpness(page):
    """ops.page_sharpness restated with torch ops (uint8 pages)."""
    lv = page.to(torch.int64)
    L = 4 * lv[1:-1, 1:-1] - lv[:-2, 1:-1] - lv[2:, 1:-1] - lv[1:-1, :-2] - lv[1:-1, 2:]
    stats = torch.stack([L.sum(), (L * L).sum(), torch.tensor(L.numel(), device=page.device)])
    return stats, torch.bincount(lv.flatten(), minlength=256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-len", type=int, default=128)
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--no-model", action="store_true", help="skip the two page_inference calls (no model is built)")
    ap.add_argument("--trace-only", action="store_true", help="replay the four ops --calls times for a kernel trace; time and write nothing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assess_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_assess: needs a GPU (a CPU run says nothing about these kernels)")
    from bench_page import H, W, MAX_IMG_SEQ_LEN, a4_page, stat, windows

    from acai_omr_amd import _lib, ops
    from acai_omr_amd.config import PE_MAX_HEIGHT, PE_MAX_WIDTH
    from acai_omr_amd.page import DetectConfig, assess_pages
    from acai_omr_amd.utils import DynamicResize
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    page_np, _ = a4_page()
    page = torch.from_numpy(page_np).to(dev)
    runs_words = torch.zeros(_lib.RUNS_WORDS, dtype=torch.int64, device=dev)
    sharp_words = torch.zeros(_lib.SHARP_WORDS, dtype=torch.int64, device=dev)
    if args.trace_only:
        for _ in range(args.calls):
            ops.page_runs(page, out=runs_words)
            ops.page_sharpness(page, out=sharp_words)
            ops.page_col_profile(page)
            ops.page_profile(page)
        torch.cuda.synchronize()
        return

    hist = ops.page_runs(page)
    stats, levels = ops.page_sharpness(page)
    t_stats, t_levels = torch_sharpness(page)
    same = bool(torch.equal(hist, torch_runs(page)) and torch.equal(stats, t_stats) and torch.equal(levels, t_levels))
    assert same, "the torch restatement and the kernels disagree"
    quality = assess_pages(page)[0]
    cases = {
        "page_runs": lambda: ops.page_runs(page, out=runs_words),
        "page_sharpness": lambda: ops.page_sharpness(page, out=sharp_words),
        "page_runs_with_its_fill": lambda: ops.page_runs(page),
        "page_sharpness_with_its_fill": lambda: ops.page_sharpness(page),
        "page_col_profile": lambda: ops.page_col_profile(page),
        "page_profile": lambda: ops.page_profile(page),
        "torch_runs": lambda: torch_runs(page),
        "torch_sharpness": lambda: torch_sharpness(page),
        "assess_pages": lambda: assess_pages(page),
    }
    launches = {"page_runs": 2, "page_sharpness": 1, "page_runs_with_its_fill": 3, "page_sharpness_with_its_fill": 2, "page_col_profile": 2, "page_profile": 1,
                "assess_pages": 4}
    res = {"when": datetime.datetime.now().isoformat(timespec="seconds"), "device": torch.cuda.get_device_name(0), "inputs": "one synthetic A4 page",
           "page": [H, W], "calls": args.calls, "reps": args.reps, "repeats": args.repeats, "page_bytes": H * W,
           "chunk_rows": _lib.RUNS_CHUNK_ROWS, "torch_restatement_equal": same,
           "scale": None if quality.scale is None else vars(quality.scale).copy(),
           "quality": {k: getattr(quality, k) for k in ("sharpness", "paper_level", "ink_level", "contrast", "ink_share", "focus")}}
    for name, fn in cases.items():
        res[name] = {**stat(windows(fn, args.calls, args.reps)), **({"launches": launches[name]} if name in launches else {})}
    res["assess_pages"]["d2h_copies"] = 1
    for a, b in (("page_runs", "page_col_profile"), ("page_sharpness", "page_col_profile"), ("page_runs", "torch_runs"), ("page_sharpness", "torch_sharpness")):
        res[f"{a}_over_{b}"] = res[a]["median_us"] / res[b]["median_us"]
    if not args.no_model:
        import bench
        from acai_omr_amd.inference.vitomr_inference import page_inference
        vit = bench.build_model(dev, args.slots)
        bench._suppress_eos(vit)
        resize = DynamicResize(16, MAX_IMG_SEQ_LEN, PE_MAX_HEIGHT, PE_MAX_WIDTH, False)
        cfg = DetectConfig()

        def call(assess):
            return page_inference(vit, page, "cuda", resize, max_inference_len=args.max_len, slots=args.slots, detect=cfg, assess=assess)

        on, off = call(True), call(None)
        torch.cuda.synchronize()
        res["systems"], res["systems_parent"] = len(on), len(off)
        res["resolved_by_canvas"] = list(cfg.resolved(H, W))
        res["resolved_by_music"] = list(cfg.resolved(H, W, on.quality[0].scale.pitch_bin))
        res["boxes_equal"] = on.boxes == off.boxes
        res["rows_equal"] = bool(torch.equal(on.seqs, off.seqs) and torch.equal(on.seq_mask, off.seq_mask)) if res["boxes_equal"] else False
        res["system_staff_space_model_px"] = [min(on.system_staff_space), max(on.system_staff_space)]
        t_on, t_off = [], []
        for _ in range(args.repeats):
            for assess, acc in ((True, t_on), (None, t_off)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(assess)
                torch.cuda.synchronize()
                acc.append((time.perf_counter() - t0) * 1e3)
        res["page_inference_assess"] = {**stat(t_on, "ms"), "max_len": args.max_len, "slots": args.slots}
        res["page_inference_parent"] = stat(t_off, "ms")
        res["page_inference_difference_ms"] = res["page_inference_assess"]["median_ms"] - res["page_inference_parent"]["median_ms"]
        res["page_inference_parent_spread_ms"] = res["page_inference_parent"]["max_ms"] - res["page_inference_parent"]["min_ms"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
