"""Page ingest on a phone-sized photo: 4000 x 3000 x 3 uint8 (the frame of tools/bench_rectify.py), the A4 page of tools/bench_page.py
(3508 x 2480, ten synthetic two-staff systems) on tinted paper in coloured ink (tests/ingest_reference.py::colour_page).  Before anything
is timed every one of the eight orientation codes is checked against the numpy restatement.  On the same GPU, in one process, it measures
  page_ingest              one launch per code 1 .. 8 on the interleaved photo (and code 1 and 6 on the planar one), with the effective
                           bandwidth over bytes read plus bytes written; the transposing codes are judged against code 1 of the same kernel;
  page_rotate              the project's existing one-read-one-write page kernel on a grey page of the same output size, alternated with
                           the ingest window by window;
  torch_ingest             a plain torch restatement on the same GPU: integer weighted sum, shift, `rot90(...).contiguous()`;
  col_profile, row_profile ops.page_col_profile against ops.page_profile on the same grey page;
  box_ink                  the 20 end rectangles of the ten systems, one launch;
  estimate_orientation     end to end (launches and copies to the host), on the photo upright and lying on its side;
  pil_on_host              what the reference does: PIL convert("L") + exif_transpose on the CPU, then the upload - when PIL is installed;
  page_inference           `orient=6` on the colour photo lying on its side against the present path on the grey upright page, alternated
                           (benchmark model of bench.build_model, <eos> suppressed, --max-len tokens per system), and the ingest's share.
Per-call figures: host clock around --calls calls that end in a device synchronise, median (min .. max) of --reps windows; the inference
calls: wall clock around one call each, --repeats times after a warm-up.  A synthetic page: nothing here says how the orientation
estimate does on real photographs.  Writes one JSON line to --out and prints it.  Needs a GPU: there is no fallback.

    python tools/bench_ingest.py [--calls 50] [--reps 5] [--repeats 3] [--max-len 128] [--slots 16] [--no-model] [--out profiles/ingest_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_page import H, MAX_IMG_SEQ_LEN, SYSTEMS, W, a4_page, stat, windows   # noqa: E402

FH, FW = 4000, 3000


def torch_ingest(photo, code):
    """The same work in plain torch: PIL's integer grey value, then the turn as a strided view made contiguous."""
    p = photo.to(torch.int32)
    g = ((p[..., 0] * 19595 + p[..., 1] * 38470 + p[..., 2] * 7471 + 32768) >> 16).to(torch.uint8)
    return {1: g, 3: torch.rot90(g, 2), 6: torch.rot90(g, -1), 8: torch.rot90(g, 1)}[code].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-len", type=int, default=128)
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--no-model", action="store_true", help="skip the two inference calls (no model is built)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ingest: needs a GPU (a CPU run says nothing about these kernels)")
    import ingest_reference as G
    from acai_omr_amd import ops
    from acai_omr_amd.config import PE_MAX_HEIGHT, PE_MAX_WIDTH
    from acai_omr_amd.page import DetectConfig, detect_systems, estimate_orientation, ingest_pages, orientation_end_boxes
    from acai_omr_amd.utils import DynamicResize
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    det = DetectConfig()
    page_np, _ = a4_page()
    sheet = np.random.RandomState(1).randint(200, 256, size=(FH, FW)).astype(np.uint8)      # the page on a sheet that fills the frame
    sheet[(FH - H) // 2:(FH - H) // 2 + H, (FW - W) // 2:(FW - W) // 2 + W] = page_np
    rgb_np = G.colour_page(sheet)
    grey_np = G.grey(rgb_np)
    photo, grey = torch.from_numpy(rgb_np).to(dev), torch.from_numpy(grey_np).to(dev)
    planar = photo.permute(2, 0, 1).contiguous()
    side_np = G.orient(rgb_np, G.INVERSE[6])                                                 # the photo that code 6 turns upright
    side = torch.from_numpy(side_np).to(dev)
    for code in range(1, 9):
        want = torch.from_numpy(G.orient(grey_np, code)).to(dev)
        assert torch.equal(ops.page_ingest(photo, code), want) and torch.equal(ops.page_ingest(planar, code), want), code
    assert torch.equal(ops.page_ingest(side, 6), grey)
    for code in (1, 3, 6, 8):
        assert torch.equal(torch_ingest(photo, code), ops.page_ingest(photo, code)), code
    boxes = detect_systems(grey, det)
    assert len(boxes) == SYSTEMS, len(boxes)
    rects = torch.tensor(orientation_end_boxes(boxes), dtype=torch.int32).to(dev)

    outs = {c: torch.empty(ops.oriented_size(FH, FW, c), dtype=torch.uint8, device=dev) for c in range(1, 9)}
    turned = torch.empty(FW, FH, dtype=torch.uint8, device=dev).copy_(ops.page_ingest(grey, 6))    # what page_rotate turns for the codes 5 .. 8
    few = max(1, args.calls // 5)
    t_ing, t_planar = {c: [] for c in range(1, 9)}, {1: [], 6: []}
    t_rot, t_rot_t, t_torch = [], [], {c: [] for c in (1, 3, 6, 8)}
    t_col, t_row, t_box, t_grey_turn = [], [], [], []
    for _ in range(args.reps):
        for c in range(1, 9):
            t_ing[c] += windows(lambda: ops.page_ingest(photo, c, out=outs[c]), args.calls, 1)
        t_rot += windows(lambda: ops.page_rotate(grey, 2.0), args.calls, 1)
        t_rot_t += windows(lambda: ops.page_rotate(turned, 2.0), args.calls, 1)
        for c in t_planar:
            t_planar[c] += windows(lambda: ops.page_ingest(planar, c, out=outs[c]), args.calls, 1)
        for c in t_torch:
            t_torch[c] += windows(lambda: torch_ingest(photo, c), few, 1)
        t_grey_turn += windows(lambda: ops.page_ingest(grey, 6, out=outs[6]), args.calls, 1)
        t_col += windows(lambda: ops.page_col_profile(grey), args.calls, 1)
        t_row += windows(lambda: ops.page_profile(grey), args.calls, 1)
        t_box += windows(lambda: ops.page_box_ink(grey, rects), args.calls, 1)
    est_up, est_side = estimate_orientation(photo), estimate_orientation(side)
    t_est_up = windows(lambda: estimate_orientation(photo), few, args.reps)
    t_est_side = windows(lambda: estimate_orientation(side), few, args.reps)

    def moved(us, nbytes):
        return {**stat(us), "bytes_read_plus_written": nbytes, "effective_GBps": nbytes / (stat(us)["median_us"] * 1e-6) / 1e9}

    colour_bytes, grey_bytes = 4 * FH * FW, 2 * FH * FW
    res = {"when": datetime.datetime.now().isoformat(timespec="seconds"), "device": torch.cuda.get_device_name(0), "photo": [FH, FW, 3], "page": [H, W],
           "calls": args.calls, "reps": args.reps,
           "page_ingest_hwc": {str(c): moved(t_ing[c], colour_bytes) for c in range(1, 9)},
           "page_ingest_chw": {str(c): moved(t_planar[c], colour_bytes) for c in t_planar},
           "page_ingest_grey_code6": moved(t_grey_turn, grey_bytes),
           "page_rotate_u8_same_output_size": {"4000x3000": moved(t_rot, grey_bytes), "3000x4000": moved(t_rot_t, grey_bytes)},
           "torch_ingest": {str(c): {**stat(t_torch[c]), "calls": few} for c in t_torch},
           "col_profile_u8": {**moved(t_col, FH * FW), "launches": 2}, "row_profile_u8": {**moved(t_row, FH * FW), "launches": 1},
           "box_ink": {**stat(t_box), "rectangles": int(rects.shape[0]), "launches": 1},
           "estimate_orientation_upright": {**stat(t_est_up), "calls": few, "result": list(est_up)},
           "estimate_orientation_sideways": {**stat(t_est_side), "calls": few, "result": list(est_side)}}
    med = lambda d: d["median_us"]   # noqa: E731
    res["ingest_code_over_code1"] = {str(c): med(res["page_ingest_hwc"][str(c)]) / med(res["page_ingest_hwc"]["1"]) for c in range(2, 9)}
    res["ingest_code1_over_page_rotate"] = med(res["page_ingest_hwc"]["1"]) / med(res["page_rotate_u8_same_output_size"]["4000x3000"])
    res["ingest_code6_over_page_rotate"] = med(res["page_ingest_hwc"]["6"]) / med(res["page_rotate_u8_same_output_size"]["3000x4000"])
    res["torch_over_ingest"] = {str(c): med(res["torch_ingest"][str(c)]) / med(res["page_ingest_hwc"][str(c)]) for c in t_torch}
    res["col_profile_over_row_profile"] = med(res["col_profile_u8"]) / med(res["row_profile_u8"])
    try:
        from PIL import Image, ImageOps
    except ImportError:
        res["pil_on_host"] = "not measured: PIL is not installed here"
    else:
        def pil_path():
            im = Image.fromarray(side_np, "RGB")
            im.getexif()[0x0112] = 6
            return torch.from_numpy(np.asarray(ImageOps.exif_transpose(im).convert("L"))).to(dev)   # (the tag does not survive convert: turn first)
        assert torch.equal(pil_path(), grey)
        res["pil_on_host"] = {**stat(windows(pil_path, max(1, few // 5), args.reps)), "what": "convert('L') + exif_transpose(6) on the CPU, then the upload"}
        res["upload_then_ingest"] = stat(windows(lambda: ingest_pages(torch.from_numpy(side_np), 6), few, args.reps))
    if not args.no_model:
        import bench
        from acai_omr_amd.inference.vitomr_inference import page_inference
        resize = DynamicResize(16, MAX_IMG_SEQ_LEN, PE_MAX_HEIGHT, PE_MAX_WIDTH, False)
        vit = bench.build_model(dev, args.slots)
        bench._suppress_eos(vit)

        def with_orient():
            return page_inference(vit, side, "cuda", resize, max_inference_len=args.max_len, slots=args.slots, detect=det, orient=6)

        def without():
            return page_inference(vit, grey, "cuda", resize, max_inference_len=args.max_len, slots=args.slots, detect=det)

        r, p = with_orient(), without()
        torch.cuda.synchronize()
        res["rows_equal_grey_upright_page"] = bool(torch.equal(r.seqs, p.seqs) and torch.equal(r.seq_mask, p.seq_mask) and r.boxes == p.boxes)
        res["systems_decoded"] = {"photo_ingested": len(r), "grey_upright_page": len(p)}
        t_with, t_without = [], []
        for _ in range(args.repeats):
            for fn, acc in ((with_orient, t_with), (without, t_without)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                acc.append((time.perf_counter() - t0) * 1e3)
        res["page_inference_orient6_colour_photo"] = {**stat(t_with, "ms"), "max_len": args.max_len, "slots": args.slots, "tokens": int(r.seq_mask.sum())}
        res["page_inference_grey_upright_present_path"] = stat(t_without, "ms")
        res["ingest_share_of_page_inference"] = med(res["page_ingest_hwc"]["6"]) / 1e3 / res["page_inference_orient6_colour_photo"]["median_ms"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
