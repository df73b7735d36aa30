"""Page deskew on the A4 page of tools/bench_page.py (3508 x 2480 uint8, ten synthetic two-staff systems), tilted by --tilt degrees (2) so
that its staff lines run down to the right.  Before anything is timed the tool checks that the detector loses the tilted page's systems,
that `estimate_skew` finds the tilt to within a step and that the levelled page gives all ten systems again.  On the same GPU, in one
process, it then measures
  strips, scores, rotate   one call of ops.page_strips / ops.page_skew_scores (161 slopes, strip 16) / ops.page_rotate each;
  estimate_skew            strips + scores + the one device-to-host copy + the choice of the angle on the host;
  deskew_pages             estimate_skew + the rotation;
  torch_rotate, torch_scores   a plain torch restatement on the same GPU: `affine_grid` + `grid_sample` (bilinear, fp32 in and out, the uint8
                           page converted outside the timed window) for the rotation, an index tensor + `gather` + sum over the strips +
                           squared differences for the scores (checked to give the same integers), each alternated with ours window by window;
  page_inference           `deskew=True` on the tilted page against `deskew=None` on the page levelled beforehand (benchmark model of
                           bench.build_model, <eos> suppressed, --max-len tokens per system), alternated, and deskew's share of the former.
Per-call figures: host clock around --calls calls that end in a device synchronise, median (min .. max) of --reps windows; the inference
calls: wall clock around one call each, --repeats times after a warm-up.  Bytes: what each step has to read and write, from the shapes.
Writes one JSON line to --out and prints it.  Needs a GPU: there is no fallback.

    python tools/bench_deskew.py [--calls 50] [--reps 5] [--repeats 3] [--max-len 128] [--slots 16] [--no-model] [--out profiles/deskew_bench.json]
"""
import argparse
import datetime
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_page import H, MAX_IMG_SEQ_LEN, SYSTEMS, W, a4_page, stat, windows   # noqa: E402


def torch_rotate(page_f, angle_deg):
    """The rotation of ops.page_rotate as torch offers it: an affine sampling grid about the centre and bilinear `grid_sample` (float
    coordinates and weights, zeros outside - not the same bits, the same work)."""
    a = math.radians(angle_deg)
    h, w = page_f.shape[-2:]
    # normalised coordinates (align_corners: x_n = dx / ((w - 1) / 2)): x_src = cos x - sin y (h - 1) / (w - 1), y_src = sin x (w - 1) / (h - 1) + cos y
    r = (h - 1) / (w - 1)
    theta = torch.tensor([[[math.cos(a), -math.sin(a) * r, 0.0], [math.sin(a) / r, math.cos(a), 0.0]]], device=page_f.device)
    grid = torch.nn.functional.affine_grid(theta, (1, 1, h, w), align_corners=True)
    return torch.nn.functional.grid_sample(page_f, grid, mode="bilinear", padding_mode="zeros", align_corners=True)


def torch_scores(P, off):
    """The scores of ops.page_skew_scores in plain torch: P int32 [nS, H], off int64 [K, nS] -> int64 [K]."""
    K, nS = off.shape
    Hh = P.shape[1]
    idx = torch.arange(Hh, device=P.device)[None, None, :] + off[:, :, None]
    inside = (idx >= 0) & (idx < Hh)
    vals = torch.gather(P[None].expand(K, nS, Hh), 2, idx.clamp_(0, Hh - 1)) * inside
    d = vals.sum(1, dtype=torch.int64).diff(dim=1)
    return (d * d).sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-len", type=int, default=128)
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--tilt", type=float, default=2.0)
    ap.add_argument("--no-model", action="store_true", help="skip the two inference calls (no model is built)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deskew_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_deskew: needs a GPU (a CPU run says nothing about these kernels)")
    from acai_omr_amd import ops
    from acai_omr_amd.config import PE_MAX_HEIGHT, PE_MAX_WIDTH
    from acai_omr_amd.page import DetectConfig, SkewConfig, deskew_pages, detect_systems, estimate_skew
    from acai_omr_amd.utils import DynamicResize
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    cfg, det = SkewConfig(), DetectConfig()
    page_np, _ = a4_page()
    level = torch.from_numpy(page_np).to(dev)
    tilted = ops.page_rotate(level, -args.tilt)                  # the staff lines now run down to the right by `tilt`
    found_level, found_tilted = detect_systems(level, det), detect_systems(tilted, det)
    angle = estimate_skew(tilted, cfg)[0]
    (levelled,), _ = deskew_pages(tilted, angle)
    found = detect_systems(levelled, det)
    assert len(found_level) == SYSTEMS and len(found_tilted) < SYSTEMS and abs(angle - args.tilt) <= cfg.step and len(found) == SYSTEMS, \
        (len(found_level), len(found_tilted), angle, len(found))
    box_shift = max(abs(p - q) for b, c in zip(found, found_level) for p, q in zip(b, c))

    S, slopes = cfg.strip, cfg.slopes()
    K, nS = len(slopes), -(-W // cfg.strip)
    table = ops.skew_slope_table(slopes, dev)
    P = ops.page_strips(tilted, S)
    scores = torch.empty(K, dtype=torch.int64, device=dev)
    t_strips = windows(lambda: ops.page_strips(tilted, S), args.calls, args.reps)
    t_estimate = windows(lambda: estimate_skew(tilted, cfg), args.calls, args.reps)
    t_deskew = windows(lambda: deskew_pages(tilted, None, cfg), args.calls, args.reps)

    # the torch restatements, checked, then alternated with ours
    off = torch.tensor([[(m * (s * S + S // 2 - W // 2) + 32768) >> 16 for s in range(nS)] for m in slopes], device=dev)
    P32 = P.to(torch.int32)
    assert torch.equal(torch_scores(P32, off), ops.page_skew_scores(P, W, S, table))
    tilted_f = (tilted.float() / 255.0)[None, None]
    mean_diff = float((torch_rotate(tilted_f, angle)[0, 0] - ops.page_rotate(tilted_f[0, 0], angle, 0.0)).abs().mean())
    t_scores, t_tscores, t_rotate, t_trotate, t_rotate_f32 = [], [], [], [], []
    few = max(1, args.calls // 10)                               # the torch scores take milliseconds a call
    for _ in range(args.reps):
        t_scores += windows(lambda: ops.page_skew_scores(P, W, S, table, out=scores), args.calls, 1)
        t_tscores += windows(lambda: torch_scores(P32, off), few, 1)
        t_rotate += windows(lambda: ops.page_rotate(tilted, angle), args.calls, 1)
        t_rotate_f32 += windows(lambda: ops.page_rotate(tilted_f[0, 0], angle), args.calls, 1)
        t_trotate += windows(lambda: torch_rotate(tilted_f, angle), args.calls, 1)

    res = {"when": datetime.datetime.now().isoformat(timespec="seconds"), "device": torch.cuda.get_device_name(0), "page": [H, W], "tilt": args.tilt,
           "estimated_angle": angle, "systems_found": {"level": len(found_level), "tilted": len(found_tilted), "deskewed": len(found)},
           "max_box_shift_vs_level_px": box_shift, "candidates": K, "strip": S, "calls": args.calls, "reps": args.reps,
           "strips": {**stat(t_strips), "launches": 1, "bytes_needed": H * W + nS * H},
           "scores": {**stat(t_scores), "launches": 1, "memsets": 1, "bytes_read_through_l2": K * nS * H, "bytes_unique": nS * H},
           "rotate_u8": {**stat(t_rotate), "launches": 1, "bytes_needed": 2 * H * W},
           "rotate_f32": {**stat(t_rotate_f32), "launches": 1, "bytes_needed": 8 * H * W},
           "estimate_skew": {**stat(t_estimate), "launches": 2, "d2h_copies": 1, "h2d_copies": 1},
           "deskew_pages": {**stat(t_deskew), "launches": 3},
           "torch_scores": {**stat(t_tscores), "calls": few}, "torch_rotate_f32": {**stat(t_trotate), "mean_abs_diff_to_ours": mean_diff}}
    res["torch_scores_over_ours"] = res["torch_scores"]["median_us"] / res["scores"]["median_us"]
    res["torch_rotate_over_ours_f32"] = res["torch_rotate_f32"]["median_us"] / res["rotate_f32"]["median_us"]
    res["torch_rotate_over_ours_u8"] = res["torch_rotate_f32"]["median_us"] / res["rotate_u8"]["median_us"]
    if not args.no_model:
        import bench
        from acai_omr_amd.inference.vitomr_inference import page_inference
        resize = DynamicResize(16, MAX_IMG_SEQ_LEN, PE_MAX_HEIGHT, PE_MAX_WIDTH, False)
        vit = bench.build_model(dev, args.slots)
        bench._suppress_eos(vit)

        def with_deskew():
            return page_inference(vit, tilted, "cuda", resize, max_inference_len=args.max_len, slots=args.slots, detect=det, deskew=cfg)

        def without():
            return page_inference(vit, levelled, "cuda", resize, max_inference_len=args.max_len, slots=args.slots, detect=det)

        r, p = with_deskew(), without()
        torch.cuda.synchronize()
        res["rows_equal_levelled_beforehand"] = bool(torch.equal(r.seqs, p.seqs) and torch.equal(r.seq_mask, p.seq_mask) and r.boxes == p.boxes)
        t_with, t_without = [], []
        for _ in range(args.repeats):
            for fn, acc in ((with_deskew, t_with), (without, t_without)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                acc.append((time.perf_counter() - t0) * 1e3)
        res["page_inference_deskew"] = {**stat(t_with, "ms"), "max_len": args.max_len, "slots": args.slots, "tokens": int(r.seq_mask.sum())}
        res["page_inference_levelled_beforehand"] = stat(t_without, "ms")
        res["deskew_share_of_page_inference"] = res["deskew_pages"]["median_us"] / 1e3 / res["page_inference_deskew"]["median_ms"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
