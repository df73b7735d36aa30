"""Record what `page.PageResult` maps where, for tests/golden/page_geometry.json (tests/test_page_geometry_cpu.py holds the code to it with
`==`).  No GPU: the maps are host arithmetic.  Every combination of orientation code 1 .. 8 (a 240 x 200 upright page, so a sideways code
has a 200 x 240 photo), angle in {0, 2.5, -7.25}, quad in {None, one convex quad well inside} and inset in {0, 2}; two systems per result.
Every case carries its own inputs, so the test builds the result from the file alone.

    python tools/record_page_geometry.py [--out tests/golden/page_geometry.json]      # write
    python tools/record_page_geometry.py --check                                      # this tree still reproduces the file
"""
import argparse
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "page_geometry.json")

PAGE = (240, 200)                                                            # (H, W) of the upright page, and of the page that was cropped
QUAD = [[20.5, 15.0], [180.0, 22.25], [172.5, 220.0], [12.0, 210.5]]        # TL, TR, BR, BL in the upright page
BOXES = [[10, 20, 150, 70], [31, 101, 190, 139]]
SIZES = [[32, 96], [48, 200]]                                                # (OH, OW) the boxes were resized to
WINDOWS = [[0, 16, 32, 64], [16, 8, 32, 176]]                                # (top, left, ch, cw)
POINTS = [[0, 0], [5.0, 3.0], [31.5, 15.25]]


def build(case):
    """The `PageResult` of a case's inputs (no sequences: geometry only)."""
    from acai_omr_amd.page import PageResult
    return PageResult([[tuple(b) for b in case["boxes"]]], None, None, None, [0] * len(case["boxes"]), [tuple(s) for s in case["sizes"]],
                      [tuple(w) for w in case["windows"]], angles=[case["angle"]], page_sizes=[tuple(case["page_size"])],
                      quads=[case["quad"]], source_sizes=[tuple(case["source_size"])], inset=case["inset"], orientations=[case["code"]])


def measure(case):
    res = build(case)
    fwd = [[list(res.to_page_xy(s, *p)) for p in POINTS] for s in range(len(case["boxes"]))]
    return dict(box_corners=[[list(c) for c in res.box_corners(s)] for s in range(len(case["boxes"]))], to_page_xy=fwd,
                from_page_xy=[[list(res.from_page_xy(s, *q)) for q in row] for s, row in enumerate(fwd)])


def cases():
    for code, angle, quad, inset in itertools.product(range(1, 9), (0.0, 2.5, -7.25), (None, QUAD), (0, 2)):
        yield dict(code=code, angle=angle, quad=quad, inset=inset, page_size=list(PAGE), source_size=list(PAGE if code <= 4 else PAGE[::-1]),
                   boxes=BOXES, sizes=SIZES, windows=WINDOWS)


def typed(v):
    """Nested lists with every number paired with its type's name: 1 and 1.0 compare equal, and must not."""
    return [typed(x) for x in v] if isinstance(v, list) else (type(v).__name__, v)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--check", action="store_true", help="compare with the file, exactly, and write nothing")
    args = ap.parse_args()
    if args.check:
        with open(args.out) as f:
            rows = json.load(f)["cases"]
        bad = [i for i, row in enumerate(rows) if any(typed(measure(row["inputs"])[k]) != typed(row[k]) for k in ("box_corners", "to_page_xy", "from_page_xy"))]
        print(f"{len(rows)} cases, {len(bad)} differ" + (f": {bad[:10]}" if bad else ""))
        return 1 if bad else 0
    rows = [dict(inputs=c, **measure(c)) for c in cases()]
    with open(args.out, "w") as f:
        json.dump(dict(points=POINTS, cases=rows), f, indent=0)
        f.write("\n")
    print(f"wrote {len(rows)} cases to {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
