"""Page rectification on the A4 page of tools/bench_page.py (3508 x 2480 uint8, ten synthetic two-staff systems) photographed: embedded by
a keystone quadrilateral into a 4000 x 3000 frame of dark noise (tests/rectify_reference.py::embed).  Before anything is timed the tool
checks that the detector finds fewer systems in the frame than the page has and all of them in the rectified page.  On the same GPU, in
one process, it then measures
  extents, warp            one call of ops.page_extents (two launches) / ops.page_warp each, uint8 and fp32;
  find_page_quad           extents, the copy to the host and the fit there;  rectify_pages  all of it, end to end;
  page_rotate              the parent commit's resampling kernel on a page of the warp's output size, alternated with the warp window by
                           window: the same bytes written, the same taps and blend, Q16 increments instead of two exact 64-bit floor
                           divisions per pixel - what the exact division costs;
  torch_warp               a plain torch restatement on the same GPU, alternated likewise: the float32 homography over a pixel grid and
                           `grid_sample` (bilinear, align_corners), rounded to uint8; with the grid built per call, and with it given.
                           The same work, not the same bits: the share of pixels that differ is reported;
  page_inference           `rectify=True` on the frame against `rectify=None` on the page itself - the present path, which this feature
                           leaves as the parent commit has it - alternated (benchmark model of bench.build_model, <eos> suppressed,
                           --max-len tokens per system), and rectify_pages' share of the former.
Per-call figures: host clock around --calls calls that end in a device synchronise, median (min .. max) of --reps windows; the inference
calls: wall clock around one call each, --repeats times after a warm-up.  Bytes: what each kernel has to read and write, from the shapes
(the warp reads the pixels inside the quadrilateral; the column pass of the extents also re-reads min_run - 1 rows per 64, which is counted
as overhead, not as need); `bound_us` is that over --bandwidth (6.3 TB/s, the achievable HBM rate), and `fraction_of_bound` needs the
KERNEL time, which a separate `rocprofv3 --kernel-trace --stats` run of this tool gives (--kernel-stats CSV: read if present).  A
synthetic page on synthetic noise: nothing here says how the defaults do on real photographs.
Writes one JSON line to --out and prints it.  Needs a GPU: there is no fallback.

    python tools/bench_rectify.py [--calls 50] [--reps 5] [--repeats 3] [--max-len 128] [--slots 16] [--no-model] [--out profiles/rectify_bench.json]
"""
import argparse
import csv
import datetime
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_page import H, MAX_IMG_SEQ_LEN, SYSTEMS, W, a4_page, stat, windows   # noqa: E402

FH, FW = 4000, 3000
QUAD = [(330.0, 260.0), (2700.0, 200.0), (2890.0, 3760.0), (130.0, 3700.0)]     # top 2371 px wide, bottom 2761: keystone
KERNELS = ("page_row_extents_kernel<unsigned char>", "page_col_extents_kernel<unsigned char>", "page_row_extents_kernel<float>",
           "page_col_extents_kernel<float>", "page_warp_kernel<unsigned char>", "page_warp_kernel<float>", "page_rotate_kernel<unsigned char>")


def torch_grid(coef, OH, OW, FH, FW, dev):
    """The sampling grid of `grid_sample` (align_corners=True) for the homography, in float32."""
    A, B, C, D, E, F, G, H_, I = (float(v) / 2.0 ** 30 for v in coef)   # noqa: E741
    y, x = torch.meshgrid(torch.arange(OH, device=dev, dtype=torch.float32), torch.arange(OW, device=dev, dtype=torch.float32), indexing="ij")
    den = G * x + H_ * y + I
    sx, sy = (A * x + B * y + C) / den, (D * x + E * y + F) / den
    return torch.stack((sx * (2.0 / (FW - 1)) - 1.0, sy * (2.0 / (FH - 1)) - 1.0), dim=-1)[None]


def torch_warp(frame, grid):
    return torch.nn.functional.grid_sample(frame.float()[None, None], grid, mode="bilinear", padding_mode="border", align_corners=True)[0, 0].add_(0.5).to(torch.uint8)


def kernel_times(path):
    """Kernel name -> average microseconds, from a rocprofv3 --stats CSV (kernel_stats): {} when there is none."""
    if not path or not os.path.exists(path):
        return {}
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            for key in KERNELS:
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
    ap.add_argument("--bandwidth", type=float, default=6.3e12, help="achievable HBM bytes / s the bytes-moved bound is taken against")
    ap.add_argument("--kernel-stats", default=os.path.join(ROOT, "profiles", "rectify_bench_kernel_stats.csv"))
    ap.add_argument("--no-model", action="store_true", help="skip the two inference calls (no model is built)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rectify_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rectify: needs a GPU (a CPU run says nothing about these kernels)")
    import rectify_reference as Q
    from acai_omr_amd import ops
    from acai_omr_amd.config import PE_MAX_HEIGHT, PE_MAX_WIDTH
    from acai_omr_amd.page import DetectConfig, RectifyConfig, detect_systems, find_page_quad, rectified_size, rectify_pages
    from acai_omr_amd.utils import DynamicResize
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    cfg, det = RectifyConfig(), DetectConfig()
    R = cfg.resolved(FH, FW)
    page_np, _ = a4_page()
    frame_np = Q.embed(page_np, QUAD, FH, FW, seed=0)
    level, frame = torch.from_numpy(page_np).to(dev), torch.from_numpy(frame_np).to(dev)
    (rect,), (quad,) = rectify_pages(frame, None, cfg)
    assert quad is not None
    corner_err = Q.corner_error(quad, QUAD)
    OH, OW = rect.shape
    assert (OH, OW) == rectified_size(quad, cfg)
    found_level, found_frame, found = detect_systems(level, det), detect_systems(frame, det), detect_systems(rect, det)
    assert len(found_level) == SYSTEMS and len(found_frame) < SYSTEMS and len(found) == SYSTEMS, (len(found_level), len(found_frame), len(found))
    coef = ops.homography_q30(quad, (OH, OW), cfg.inset)

    frame_f = frame.float() / 255.0
    out_u8, out_f32 = torch.empty_like(rect), torch.empty(OH, OW, dtype=torch.float32, device=dev)
    same_size = torch.empty_like(rect).copy_(rect)                  # what page_rotate turns: a page of the warp's output size
    t_find = windows(lambda: find_page_quad(frame, cfg), args.calls, args.reps)
    t_pages = windows(lambda: rectify_pages(frame, None, cfg), args.calls, args.reps)
    grid = torch_grid(coef, OH, OW, FH, FW, dev)
    differ = float((torch_warp(frame, grid) != rect).float().mean())
    t_ext, t_ext_f32, t_warp, t_warp_f32, t_rot, t_torch, t_torch_grid = [], [], [], [], [], [], []
    few = max(1, args.calls // 5)
    for _ in range(args.reps):
        t_ext += windows(lambda: ops.page_extents(frame, cfg.paper_threshold, R), args.calls, 1)
        t_ext_f32 += windows(lambda: ops.page_extents(frame_f, cfg.paper_threshold, R), args.calls, 1)
        t_warp += windows(lambda: ops.page_warp(frame, coef, (OH, OW), out=out_u8), args.calls, 1)
        t_rot += windows(lambda: ops.page_rotate(same_size, 2.0), args.calls, 1)
        t_warp_f32 += windows(lambda: ops.page_warp(frame_f, coef, (OH, OW), out=out_f32), args.calls, 1)
        t_torch += windows(lambda: torch_warp(frame, grid), few, 1)
        t_torch_grid += windows(lambda: torch_warp(frame, torch_grid(coef, OH, OW, FH, FW, dev)), few, 1)

    kt = kernel_times(args.kernel_stats)

    def kernel(name, nbytes, **more):
        d = {"bytes_needed": nbytes, "bound_us": nbytes / args.bandwidth * 1e6, **more}
        if name in kt:
            d.update(kernel_us=kt[name]["avg_us"], kernel_min_us=kt[name]["min_us"], fraction_of_bound=d["bound_us"] / kt[name]["avg_us"])
        return d

    area = 0.5 * abs(sum(quad[i][0] * quad[(i + 1) % 4][1] - quad[(i + 1) % 4][0] * quad[i][1] for i in range(4)))
    halo = (R - 1) / 64.0
    res = {"when": datetime.datetime.now().isoformat(timespec="seconds"), "device": torch.cuda.get_device_name(0), "page": [H, W], "frame": [FH, FW],
           "quad": QUAD, "quad_found": quad, "corner_error_px": corner_err, "min_run": R, "inset": cfg.inset, "rectified_size": [OH, OW],
           "calls": args.calls, "reps": args.reps, "bandwidth_for_bound": args.bandwidth,
           "systems_found": {"page_itself": len(found_level), "frame": len(found_frame), "rectified": len(found)},
           "extents_u8": {**stat(t_ext), "launches": 2},
           "extents_rows_u8": kernel("page_row_extents_kernel<unsigned char>", FH * FW + 8 * FH + 8 * FW),
           "extents_cols_u8": kernel("page_col_extents_kernel<unsigned char>", FH * FW + 8 * FW, halo_rows_reread_share=halo),
           "extents_f32": {**stat(t_ext_f32), "launches": 2},
           "extents_rows_f32": kernel("page_row_extents_kernel<float>", 4 * FH * FW + 8 * FH + 8 * FW),
           "extents_cols_f32": kernel("page_col_extents_kernel<float>", 4 * FH * FW + 8 * FW, halo_rows_reread_share=halo),
           "warp_u8": {**stat(t_warp), "launches": 1, **kernel("page_warp_kernel<unsigned char>", int(area) + OH * OW)},
           "warp_f32": {**stat(t_warp_f32), "launches": 1, **kernel("page_warp_kernel<float>", 4 * (int(area) + OH * OW))},
           "page_rotate_u8_same_output_size": {**stat(t_rot), "launches": 1, **kernel("page_rotate_kernel<unsigned char>", 2 * OH * OW)},
           "find_page_quad": {**stat(t_find), "launches": 2, "d2h_copies": 1},
           "rectify_pages": {**stat(t_pages), "launches": 3, "d2h_copies": 1},
           "torch_warp_u8_grid_given": {**stat(t_torch), "calls": few, "share_of_pixels_differing_from_ours": differ},
           "torch_warp_u8_grid_built": {**stat(t_torch_grid), "calls": few}}
    res["warp_over_page_rotate"] = res["warp_u8"]["median_us"] / res["page_rotate_u8_same_output_size"]["median_us"]
    res["torch_grid_given_over_warp"] = res["torch_warp_u8_grid_given"]["median_us"] / res["warp_u8"]["median_us"]
    res["torch_grid_built_over_warp"] = res["torch_warp_u8_grid_built"]["median_us"] / res["warp_u8"]["median_us"]
    if not args.no_model:
        import bench
        from acai_omr_amd.inference.vitomr_inference import page_inference
        resize = DynamicResize(16, MAX_IMG_SEQ_LEN, PE_MAX_HEIGHT, PE_MAX_WIDTH, False)
        vit = bench.build_model(dev, args.slots)
        bench._suppress_eos(vit)

        def with_rectify():
            return page_inference(vit, frame, "cuda", resize, max_inference_len=args.max_len, slots=args.slots, detect=det, rectify=cfg)

        def without():
            return page_inference(vit, level, "cuda", resize, max_inference_len=args.max_len, slots=args.slots, detect=det)

        r, p = with_rectify(), without()
        before = page_inference(vit, rect, "cuda", resize, max_inference_len=args.max_len, slots=args.slots, detect=det)
        torch.cuda.synchronize()
        res["rows_equal_rectified_beforehand"] = bool(torch.equal(r.seqs, before.seqs) and torch.equal(r.seq_mask, before.seq_mask) and r.boxes == before.boxes)
        res["systems_decoded"] = {"frame_rectified": len(r), "page_itself": len(p)}
        t_with, t_without = [], []
        for _ in range(args.repeats):
            for fn, acc in ((with_rectify, t_with), (without, t_without)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                acc.append((time.perf_counter() - t0) * 1e3)
        res["page_inference_rectify_frame"] = {**stat(t_with, "ms"), "max_len": args.max_len, "slots": args.slots, "tokens": int(r.seq_mask.sum())}
        res["page_inference_page_itself_present_path"] = stat(t_without, "ms")
        res["rectify_share_of_page_inference"] = res["rectify_pages"]["median_us"] / 1e3 / res["page_inference_rectify_frame"]["median_ms"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
