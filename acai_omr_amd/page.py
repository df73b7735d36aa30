"""Whole-page input (an extension): from a photographed or scanned page to the staff systems the model reads.

The reference's service has its user draw a box around every system of an uploaded page, crops each box with PIL, runs
`base_img_transform` on each crop, decodes the crops one after another at batch size 1, joins the sequences with " " and reports one
average confidence (acai_omr/ui/routes.py: `setup_inference` :108-129, `multiple_img_stream_inference_wrapper` :93-104, `prepare_results`
:172-192).  This module is the host edge of doing the same on the device for all systems of all pages at once:

  * `boxes_from_fractions`  the UI's payload (fractions of the page) -> pixel boxes, rounded as PIL's `Image.crop` rounds them;
  * `detect_systems`        no boxes drawn: row profiles -> bands of inked rows -> the bands that hold staff lines (ops.page_profile,
                            ops.page_systems; the reference has no detector);
  * `estimate_skew`, `deskew_pages`   opt-in, in front of the detection: the skew of a page estimated on the device and the page turned level
                            (ops.page_strips, ops.page_skew_scores, ops.page_rotate; the reference has a person draw the boxes instead);
  * `flatten_pages`         opt-in, in front of deskew and detection: the paper's brightness estimated per tile on the device and divided
                            out of the page (ops.page_tile_levels, ops.page_flatten; the reference reads the photo as it comes);
  * `find_page_quad`, `rectify_pages`   opt-in, in front of everything else: the outline of the sheet found in the photo - where the paper
                            begins and ends in every row and column on the device, four lines fitted through those points on the host -
                            and the sheet warped flat (ops.page_extents, ops.page_warp);
  * `ingest_pages`, `estimate_orientation`   opt-in, the very first step: a decoded COLOUR photo, interleaved or planar, in the layout it
                            arrived in, made grey with PIL's integer formula and turned upright by its EXIF orientation code in one
                            launch (ops.page_ingest; the reference does both on the host with PIL, ui/routes.py:98-118), and, for a photo
                            whose tag was stripped, the quarter turn estimated on the device from the staff lines (ops.page_col_profile,
                            ops.page_box_ink);
  * `estimate_staff_scale`, `assess_pages`   opt-in, on the page detection sees: the thickness of a staff line and the distance from line
                            to line from the histograms of vertical run lengths, sharpness and contrast from the levels and their
                            Laplacian (ops.page_runs, ops.page_sharpness; the reference measures nothing) - detection is then sized
                            from the music instead of the canvas, and a caller can refuse a photo that cannot be read;
  * `prepare_pages`         the stages above that change the page, in their one order ingest -> rectify -> flatten -> deskew, each keyword
                            read by the one rule of `resolve_stage`; returns the pages detection sees and the `Prepared` record;
  * `split_pages`           every box of every page cut out, resized as `DynamicResize` resizes the crop and written into ONE
                            `PackedPatches` by one launch pair (ops.crop_resize_to_patches) - no crop copies, no per-system launches;
  * `PageResult`            the per-system rows of the decode, joined per page as the service joins them, and per page the chain of
                            `PointMap`s (turn, homography, orientation) that leads from what was cropped back to the photo.

`inference.vitomr_inference.page_inference` strings them together.  There is no CPU fallback.

The detection rule assumes roughly LEVEL staff lines: a staff line must show up as a long horizontal run within single pixel rows, so a
page rotated by more than about one line thickness over `line_frac` of its width (a skewed phone photo) loses its line rows and its systems
with them.  `deskew_pages` levels such a page first (`page_inference(..., deskew=True)`): the skew is the candidate angle, of a fixed grid
up to `SkewConfig.max_angle` <= 15 degrees, along which the sheared row profile of the page is sharpest, refined by a parabola through its
neighbours, and the page is turned by it with bilinear sampling; `PageResult` then reports boxes in the levelled page and maps points back
to the page that was passed in.  Not handled here: perspective (that is `rectify_pages`) and page curl, a quarter-turn (that is
`ingest_pages`: `SkewConfig.max_angle` stops at 15 degrees), a coarse-to-fine angle search, and cropping straight from the unrotated
page (one resampling fewer).  The defaults of `SkewConfig` rest on the proportions of an engraved page, not on data: how well the
estimate and the rule do on real scans and photos has not been measured (no such data here); explicit boxes remain the fallback.

Every stage decides "ink or paper" with ONE threshold for the whole page (`value / 255 < ink_threshold`), so a page lit unevenly - falloff
towards the far edge, a vignette, the shadow of the hand and the phone - turns to "ink" wherever its paper falls below it, and bands merge
across systems.  `flatten_pages` (`page_inference(..., flatten=True)`) divides the local paper level out first: the median level of every
tile (`FlattenConfig.tile` pixels square), a tile that is mostly ink taking its brightest neighbour's instead, interpolated bilinearly
between the tile centres; a pixel becomes 255 * p / background.  Deskew, detection and the crops the model reads all see the flattened
page; geometry does not change.  Not handled: using the flattened page for detection only while cropping from the original, binarisation,
the dark table around a page (that is `rectify_pages`, which runs first), and ink areas more than two tiles wide in both directions (the
rescue reaches one tile); colour input is made grey first (`ingest_pages`), the shading of the three channels is not estimated apart.
The defaults of `FlattenConfig` were chosen on synthetic shading (ramps, a vignette, hard shadow edges): nothing has been measured on
real photographs (no such data here), nor how a trained checkpoint reads flattened crops.

Every stage above takes the tensor it is given for the sheet.  A phone photo is a sheet seen at an angle, lying on something darker: the
table counts as ink in every row, the bands merge and the detector finds one "system".  `rectify_pages`
(`page_inference(..., rectify=True)`) runs FIRST, so that flatten and deskew see the sheet and not the table: `find_page_quad` asks the
device where the first and the last run of `RectifyConfig.min_run` paper pixels lies in every row and column, fits a line through each of
the four sets of points on the host (a least-squares line through the central half, three rounds of keeping what lies within `tol` of it,
a final line) and intersects them; the sheet is then sampled through the homography that takes an output rectangle, grown by `inset`
pixels so that no fringe of the table comes along, to that quadrilateral, with exact integer arithmetic on the device.  `PageResult` then
reports boxes in the rectified (and levelled) page and maps points all the way back.  Not handled: page curl; a sheet lighter than
paper-coloured surroundings (a white sheet on a white desk has no outline), or one cut off by the frame on more than one side; folding
the rectification and the turn into one resampling; batching the stage over pages in one launch.  The defaults of `RectifyConfig` were
chosen on synthetic quadrilaterals over a noise table: nothing has been measured on real photographs (no such data here).

Every stage above takes ONE channel and a page that stands upright.  A decoded phone photo is (H, W, 3) uint8 - (3, H, W) from a torch
decoder - and a phone held upright stores its sensor rows sideways and says so in the EXIF orientation tag; without the turn the staff
lines run down the columns and the detection rule finds nothing.  Colour input and EXIF / quarter-turn orientation: that is
`ingest_pages` (`page_inference(..., orient=code)`), which runs before everything else: the photo is uploaded as it is and one launch
writes the grey, upright page - L = (19595 R + 38470 G + 7471 B + 32768) >> 16 as PIL's `convert("L")`, a fourth channel ignored, and the
index map of `ImageOps.exif_transpose` for the codes 1 .. 8, bit for bit; `PageResult` maps points back through the turn to the pixels of
the photo.  Where the tag is missing (upload pipelines strip it), `estimate_orientation` (`page_inference(..., orient=True)`) guesses one
of the codes 1, 3, 6, 8 with two integer decisions.  Sideways: the page has at least `OrientConfig.min_line_rows` line columns (columns
with an ink run of `line_frac` of the height) and more line columns than line rows.  Upside down: on the page turned level (by code 6 if
it was sideways), the leftmost `end_frac` of every detected system holds less ink than its rightmost `end_frac`, summed over the systems -
a system begins with clef, key and time signature and usually a brace, and ends with a thin barline.  That second rule is a HEURISTIC
chosen on synthetic pages, like the defaults of the other configs: nothing has been measured on real photographs (no such data here); the
EXIF code remains the primary path.  Not handled: float colour input; mirrored photos without a tag (the estimate never answers 2, 4, 5
or 7); reading the EXIF tag out of a file (the caller passes the number: PIL or any decoder gives it); JPEG decoding itself; folding the
quarter turn into the rectification warp (two passes over the page where one could do).

Every default of `DetectConfig` is a share of the canvas: right for a full engraved A4 page, wrong for a dense page of small staves (parts,
hymnals, pocket scores), for a last page that ends half way down and for a sheet that fills half the frame.  And nothing above says
whether a photo can be read at all: a blurred, washed-out or too-small one decodes to confident-looking tokens.  Both lack one
measurement, the size of the music in pixels.  `assess_pages` (`page_inference(..., assess=True)`) makes it the way classical OMR front
ends do: in every column the vertical runs of ink and of paper are histogrammed by length on the device (ops.page_runs); the most frequent
closed ink run is the staff-line thickness, the most frequent sum of an ink run and the paper run under it the distance from line to line
(`choose_staff_scale`, integers on the host).  `DetectConfig.resolved(H, W, staff_space)` then sizes merge_gap, min_height and margin from
180 staff spaces in place of H.  One more read of the page gives the level histogram and the variance of the Laplacian
(ops.page_sharpness): contrast, sharpness and their quotient, focus.  `AssessConfig` carries a gate over these numbers whose bounds all
default to None: no threshold is invented here, because nothing in this repository can calibrate one.  Not handled: sizing flatten,
deskew or rectify from the scale (they run before it can be measured), horizontal runs, a scale per system, any default threshold.
Nothing has been measured on real photographs (no such data here).
"""
import functools
import math
from dataclasses import dataclass
from typing import Callable, NamedTuple, Optional

import torch

from ._lib import EXTENTS_MAX_RUN, FLATTEN_TILES, PAGE_MAX_H, PAGE_MAX_W
from .utils import PackedPatches, stringify_lmx_seq

NO_GPU = "acai_omr_amd page input runs on the GPU (HIP page kernels); there is no CPU fallback"


def _num(v):
    """A real number: an int or a float, not a bool and not NaN."""
    return isinstance(v, (int, float)) and not isinstance(v, bool) and v == v


@dataclass
class DetectConfig:
    """Parameters of `detect_systems`.  A field left at None is sized from the page (H rows, W columns) when the page is seen, in proportion
    to an engraved A4 / letter page, whose staff is about H / 45 tall with H / 180 between its lines and at least H / 30 of white between
    systems:

      ink_threshold  a pixel is ink if its value (uint8 / 255) is below this;
      min_ink        a row is inked if it holds at least this many ink pixels            default max(1, W // 500): a speck of dust is not ink;
      merge_gap      inked rows at most this many rows apart belong to one band          default max(1, H // 200): under the white between
                                                                                         systems, over anything inside a staff;
      min_height     a band must be at least this tall                                   default max(1, H // 90): half a staff;
      line_frac      a line row holds an ink run of at least ceil(line_frac * W) pixels (a staff line; text and dashes do not reach it);
      min_line_rows  a band must hold at least this many line rows (five lines of a staff, each at least one row thick);
      margin         the box is the band's ink grown by this much on every side          default max(1, H // 100);
      max_systems    capacity of the device-side box list; more kept bands than this is an error."""
    ink_threshold: float = 0.5
    min_ink: Optional[int] = None
    merge_gap: Optional[int] = None
    min_height: Optional[int] = None
    line_frac: float = 0.5
    min_line_rows: int = 5
    margin: Optional[int] = None
    max_systems: int = 64

    def resolved(self, H, W, staff_space=None):
        """(min_ink, merge_gap, min_height, line_len, margin) for an H x W page.  staff_space (None: as above, from H): the distance from
        staff line to staff line in pixels as it was measured on the page (`estimate_staff_scale`: `StaffScale.pitch_bin`); merge_gap,
        min_height and margin, where left at None, are then sized from Hs = floor(180 * staff_space) in place of H - the height of the
        engraved page on which this music would have that distance, the class's own proportion - so a dense page of small staves, a
        last page that ends half way down and a sheet that fills half the frame are judged by their music and not by the canvas.
        min_ink and line_len are shares of the width and stay so."""
        pick = lambda v, d: int(d if v is None else v)   # noqa: E731
        if staff_space is not None:
            if isinstance(staff_space, bool) or not isinstance(staff_space, (int, float)) or not 0 < staff_space <= PAGE_MAX_H:
                raise ValueError(f"DetectConfig: staff_space = {staff_space!r} is not None or a positive number of pixels")
            H = int(math.floor(180 * staff_space))
        return (pick(self.min_ink, max(1, W // 500)), pick(self.merge_gap, max(1, H // 200)), pick(self.min_height, max(1, H // 90)),
                int(math.ceil(self.line_frac * W)), pick(self.margin, max(1, H // 100)))


def _device_page(page, device=None):
    """One page -> a (H, W) uint8 / fp32 GPU tensor (a CPU tensor is uploaded once; other float types are widened to fp32)."""
    if not torch.is_tensor(page) or page.dim() not in (2, 3) or (page.dim() == 3 and page.shape[0] != 1):
        raise TypeError("expected a page as a (H,W) or (1,H,W) tensor")
    if not torch.cuda.is_available():
        raise RuntimeError(NO_GPU)
    if page.dim() == 3:
        page = page[0]
    if not page.is_cuda:
        page = page.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    if page.dtype != torch.uint8:
        page = page.to(torch.float32)
    return page if page.stride(-1) == 1 and (page.shape[0] == 1 or page.stride(0) >= page.shape[1]) else page.contiguous()


def detect_systems(page, cfg=None, staff_space=None):
    """The staff systems of one page -> [(x0, y0, x1, y1), ...] in pixels, top to bottom; an empty page gives [].  Three launches and ONE
    device-to-host copy (the count and the boxes together).  More than cfg.max_systems systems: ValueError.  staff_space: passed on to
    `DetectConfig.resolved` (None: the defaults are sized from the page, as ever)."""
    from . import ops
    cfg = cfg or DetectConfig()
    page = _device_page(page)
    H, W = page.shape
    min_ink, merge_gap, min_height, line_len, margin = cfg.resolved(H, W) if staff_space is None else cfg.resolved(H, W, staff_space)
    ink, run = ops.page_profile(page, cfg.ink_threshold)
    out = torch.empty(4 + 4 * cfg.max_systems, dtype=torch.int32, device=page.device)
    ops.page_systems(page, ink, run, cfg.ink_threshold, min_ink, merge_gap, min_height, line_len, cfg.min_line_rows, margin, cfg.max_systems, out=out)
    host = out.cpu()
    count = int(host[0])
    if count > cfg.max_systems:
        raise ValueError(f"the page has {count} systems, more than max_systems = {cfg.max_systems}")
    return [tuple(int(v) for v in b) for b in host[4:4 + 4 * count].view(count, 4).tolist()]


@dataclass
class SkewConfig:
    """Parameters of `estimate_skew`, angles in degrees: the candidates are (k - n) step for k = 0 .. 2 n with n = round(max_angle / step)
    (max_angle <= 15, at most 1024 candidates); the page is cut into vertical strips of `strip` columns (8, 16, 32 or 64: a strip must be
    narrow enough for a staff line to stay within about a row across it at max_angle); ink_threshold as in `DetectConfig`."""
    max_angle: float = 10.0
    step: float = 0.125
    strip: int = 16
    ink_threshold: float = 0.5

    def candidates(self):
        if not (self.step > 0 and 0 <= self.max_angle <= 15):
            raise ValueError(f"SkewConfig: step = {self.step} must be positive and max_angle = {self.max_angle} within 0 .. 15 degrees")
        n = int(round(self.max_angle / self.step))
        if 2 * n + 1 > 1024:
            raise ValueError(f"SkewConfig: {2 * n + 1} candidate angles, more than 1024")
        return [(k - n) * self.step for k in range(2 * n + 1)]

    def slopes(self):
        """The candidates as Q16 slopes, round(tan(angle) * 65536) in float64: the device does no trigonometry."""
        return [int(round(math.tan(math.radians(a)) * 65536.0)) for a in self.candidates()]


def choose_skew(scores, cfg):
    """The integer scores of cfg's candidates -> the skew in degrees (float64 arithmetic on the host).  The maximum wins; among equal maxima
    the candidate nearest to 0, the negative one first (a blank page: exactly 0.0).  An interior winner k with den = s[k-1] - 2 s[k] + s[k+1]
    < 0 is refined by the vertex of the parabola through its neighbours: + step * 0.5 * (s[k-1] - s[k+1]) / den."""
    s = [int(v) for v in scores]
    cand = cfg.candidates()
    if len(s) != len(cand):
        raise ValueError(f"{len(s)} scores for {len(cand)} candidates")
    n, best = len(s) // 2, max(s)
    k = min((i for i, v in enumerate(s) if v == best), key=lambda i: (abs(i - n), i))
    angle = cand[k]
    if 0 < k < len(s) - 1:
        den = s[k - 1] - 2 * s[k] + s[k + 1]
        if den < 0:
            angle += cfg.step * 0.5 * (s[k - 1] - s[k + 1]) / den
    return float(angle)


def skew_scores(pages, cfg=None):
    """int64 [pages, candidates] on the device: per page two launches (ops.page_strips, ops.page_skew_scores) into one tensor; the slope
    table is uploaded once."""
    from . import ops
    cfg = cfg or SkewConfig()
    pages, _ = page_lists(pages, None)
    pages = [_device_page(p) for p in pages]
    if not pages:
        raise ValueError("skew_scores: no pages")
    table = ops.skew_slope_table(cfg.slopes(), pages[0].device)
    scores = torch.empty(len(pages), len(table[1]), dtype=torch.int64, device=pages[0].device)
    for i, p in enumerate(pages):
        ops.page_skew_scores(ops.page_strips(p, cfg.strip, cfg.ink_threshold), p.shape[1], cfg.strip, table, out=scores[i])
    return scores


def estimate_skew(pages, cfg=None):
    """One page or a list -> per page, the angle in degrees by which `ops.page_rotate` levels it: positive when the staff lines run down to
    the right.  Two launches per page, and ONE device-to-host copy (the scores of all pages) per call; the angle is chosen on the host
    (`choose_skew`).  A blank page gives exactly 0.0."""
    cfg = cfg or SkewConfig()
    return [choose_skew(row, cfg) for row in skew_scores(pages, cfg).cpu().tolist()]


def deskew_pages(pages, angles=None, cfg=None, fill=None):
    """One page or a list -> (the levelled pages, their angles).  angles: None - `estimate_skew` with cfg - or one float for all pages or a
    list with one per page.  Every page is turned by its angle (ops.page_rotate; fill: what lies outside the page, default the paper); an
    angle of exactly 0.0 returns the page itself (on the device), with no launch."""
    from . import ops
    pages, _ = page_lists(pages, None)
    pages = [_device_page(p) for p in pages]
    if angles is None:
        angles = estimate_skew(pages, cfg) if pages else []
    elif isinstance(angles, (int, float)):
        angles = [float(angles)] * len(pages)
    angles = [float(a) for a in angles]
    if len(angles) != len(pages):
        raise ValueError(f"{len(pages)} pages but {len(angles)} angles")
    return [p if a == 0.0 else ops.page_rotate(p, a, fill) for p, a in zip(pages, angles)], angles


@dataclass
class FlattenConfig:
    """Parameters of `flatten_pages`:

      tile       the paper level is estimated per tile of tile x tile pixels: 16, 32, 64 or 128   default (None): the largest of those that
                                                                                is <= max(16, H // 40) - wider than a staff is tall, so that
                                                                                the median of a tile over a staff is still paper;
      percent    a tile's level is the level below or at which this share of its pixels lie: an integer in 1 .. 100 (50: the median);
      ink_ratio  a tile whose level is below ink_ratio of the brightest level among its 3 x 3 neighbours is mostly ink and takes that
                 level; on the device rq = round(ink_ratio * 256), 0 <= rq <= 256, and 0 switches the rescue off;
      floor      no tile level is taken below this level (1 .. 255): what is darker is not lit paper, and dividing by it would only lift
                 noise.

    Anything else: ValueError, when the config is made and again when it is used."""
    tile: Optional[int] = None
    percent: int = 50
    ink_ratio: float = 1.0 / 3.0
    floor: int = 32

    def __post_init__(self):
        self.check()

    def check(self):
        """(percent, rq, floor) as the device takes them."""
        if self.tile is not None and (isinstance(self.tile, bool) or not isinstance(self.tile, int) or self.tile not in FLATTEN_TILES):
            raise ValueError(f"FlattenConfig: tile = {self.tile!r} is not None or one of {FLATTEN_TILES}")
        for name, lo, hi in (("percent", 1, 100), ("floor", 1, 255)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError(f"FlattenConfig: {name} = {v!r} is not an integer in {lo} .. {hi}")
        if isinstance(self.ink_ratio, bool) or not isinstance(self.ink_ratio, (int, float)) or not -1.0 < self.ink_ratio < 2.0:
            raise ValueError(f"FlattenConfig: ink_ratio = {self.ink_ratio!r} is not a number in 0 .. 1")
        rq = int(round(self.ink_ratio * 256))
        if not 0 <= rq <= 256:
            raise ValueError(f"FlattenConfig: ink_ratio = {self.ink_ratio!r} gives rq = {rq}, not in 0 .. 256")
        return self.percent, rq, self.floor

    def resolved(self, H):
        """(tile, percent, rq, floor) for a page of H rows."""
        tile = self.tile if self.tile is not None else max(t for t in FLATTEN_TILES if t <= max(16, H // 40))
        return (tile,) + self.check()


def flatten_pages(pages, cfg=None):
    """One page or a list -> the list of flattened pages on the device (new contiguous tensors of the pages' sizes and dtypes).  Two launches
    per page (ops.page_tile_levels, ops.page_flatten), nothing comes back to the host."""
    from . import ops
    cfg = cfg or FlattenConfig()
    pages, _ = page_lists(pages, None)
    out = []
    for p in (_device_page(p) for p in pages):
        tile, percent, rq, floor = cfg.resolved(p.shape[0])
        out.append(ops.page_flatten(p, ops.page_tile_levels(p, tile, percent), tile, rq, floor))
    return out


@dataclass
class RectifyConfig:
    """Parameters of `find_page_quad` and `rectify_pages`:

      paper_threshold  a pixel is paper if its value (uint8 / 255) is NOT below this (the ink test of the other stages, negated);
      min_run          a row or column meets the sheet where this many paper pixels follow one another (1 .. 256)
                                                                                default (None): max(4, min(H, W) // 100) - specks of
                                                                                light on the table are shorter, a margin is longer;
      tol              a point belongs to an edge if it lies within this many pixels of the fitted line (> 0);
      min_points       an edge must keep at least this many points (>= 2);
      min_area         the quadrilateral must cover at least this share of the frame (0 .. 1);
      inset            the output rectangle is grown by this many output pixels on every side before it is mapped to the quadrilateral,
                       so the rim of the sheet - where a pixel is part table - stays outside (>= 0);
      out_size         (OH, OW) of the rectified page                            default (None): the longer of each pair of opposite
                                                                                sides of the quadrilateral, rounded, plus one.

    Anything else: ValueError, when the config is made and again when it is used."""
    paper_threshold: float = 0.5
    min_run: Optional[int] = None
    tol: float = 1.5
    min_points: int = 16
    min_area: float = 0.25
    inset: float = 2
    out_size: Optional[tuple] = None

    def __post_init__(self):
        self.check()

    def check(self):
        if not _num(self.paper_threshold):
            raise ValueError(f"RectifyConfig: paper_threshold = {self.paper_threshold!r} is not a number")
        if self.min_run is not None and (isinstance(self.min_run, bool) or not isinstance(self.min_run, int) or not 1 <= self.min_run <= EXTENTS_MAX_RUN):
            raise ValueError(f"RectifyConfig: min_run = {self.min_run!r} is not None or an integer in 1 .. {EXTENTS_MAX_RUN}")
        if not _num(self.tol) or not self.tol > 0:
            raise ValueError(f"RectifyConfig: tol = {self.tol!r} is not a positive number")
        if isinstance(self.min_points, bool) or not isinstance(self.min_points, int) or self.min_points < 2:
            raise ValueError(f"RectifyConfig: min_points = {self.min_points!r} is not an integer >= 2")
        if not _num(self.min_area) or not 0 <= self.min_area <= 1:
            raise ValueError(f"RectifyConfig: min_area = {self.min_area!r} is not a share in 0 .. 1")
        if not _num(self.inset) or not 0 <= self.inset <= 1024:
            raise ValueError(f"RectifyConfig: inset = {self.inset!r} is not a number in 0 .. 1024")
        if self.out_size is not None:
            ok = isinstance(self.out_size, (tuple, list)) and len(self.out_size) == 2 and all(isinstance(v, int) and not isinstance(v, bool) for v in self.out_size)
            if not ok or not (1 <= self.out_size[0] <= PAGE_MAX_H and 1 <= self.out_size[1] <= PAGE_MAX_W):
                raise ValueError(f"RectifyConfig: out_size = {self.out_size!r} is not None or (OH, OW) within {PAGE_MAX_H} x {PAGE_MAX_W}")

    def resolved(self, H, W):
        """min_run for an H x W frame."""
        self.check()
        return max(4, min(H, W) // 100) if self.min_run is None else self.min_run


def _fit_edge(t, v, tol, min_points):
    """Points (t_k, v_k) of one edge in the order of t (float64 tensors) -> (a, b) of the line v = a t + b, or None.  The central half by
    index, n // 4 <= k < n - n // 4, gives the first least-squares line; three times the points (of ALL of the edge's) within tol of the
    line, measured along v, give the next one."""
    n = t.numel()
    keep = torch.zeros(n, dtype=torch.bool)
    keep[n // 4:n - n // 4] = True
    for rounds_left in (3, 2, 1, 0):
        tt, vv = t[keep], v[keep]
        if tt.numel() < 2 or (rounds_left == 0 and tt.numel() < min_points):
            return None
        tm, vm = tt.mean(), vv.mean()
        dt = tt - tm
        stt = (dt * dt).sum()
        if float(stt) == 0.0:
            return None
        a = (dt * (vv - vm)).sum() / stt
        b = vm - a * tm
        if rounds_left:
            keep = (v - (a * t + b)).abs() <= tol
    return float(a), float(b)


def _quad_ok(quad, H, W, min_area):
    """Convex, in the order TL, TR, BR, BL (clockwise as displayed, y down), at least min_area of the frame, and not the frame itself."""
    cross = []
    for i in range(4):
        (ax, ay), (bx, by), (cx, cy) = quad[i], quad[(i + 1) % 4], quad[(i + 2) % 4]
        cross.append((bx - ax) * (cy - by) - (by - ay) * (cx - bx))
    (tlx, tly), (trx, try_), (brx, bry), (blx, bly) = quad
    if not (all(c > 0 for c in cross) and tlx < trx and blx < brx and tly < bly and try_ < bry):
        return False
    area = 0.5 * abs(sum(quad[i][0] * quad[(i + 1) % 4][1] - quad[(i + 1) % 4][0] * quad[i][1] for i in range(4)))
    if area < min_area * H * W:
        return False
    frame = ((0, 0), (W - 1, 0), (W - 1, H - 1), (0, H - 1))
    return not all(abs(x - fx) <= 1 and abs(y - fy) <= 1 for (x, y), (fx, fy) in zip(quad, frame))


def fit_page_quad(extents, H, W, cfg=None):
    """`ops.page_extents` of an H x W frame, on the host (a tensor or a list of 2 H + 2 W integers) -> the sheet's corners [TL, TR, BR, BL]
    as (x, y) floats, or None.  float64 throughout.  The left edge is the points (row_lo[y], y) over the rows with row_hi >= 0, fitted as
    x = a y + b; the right edge (row_hi[y], y); the top and bottom edges (x, col_lo[x]) and (x, col_hi[x]) over the columns with
    col_hi >= 0, fitted as y = a x + b (`_fit_edge`); the corners are where the lines meet.  None when an edge keeps fewer than
    cfg.min_points points, the quadrilateral is not convex or not in that order, covers less than cfg.min_area of the frame, or has all
    four corners within a pixel of the frame's (the sheet fills the frame: nothing to do)."""
    cfg = cfg or RectifyConfig()
    cfg.check()
    e = torch.as_tensor(extents).to("cpu", torch.float64)
    if e.numel() != 2 * H + 2 * W:
        raise ValueError(f"extents: expected {2 * H + 2 * W} values for a {H} x {W} frame, got {e.numel()}")
    row_lo, row_hi, col_lo, col_hi = e[:H], e[H:2 * H], e[2 * H:2 * H + W], e[2 * H + W:]
    ys, xs = torch.nonzero(row_hi >= 0).flatten(), torch.nonzero(col_hi >= 0).flatten()
    yt, xt = ys.to(torch.float64), xs.to(torch.float64)
    lines = [_fit_edge(t, v, float(cfg.tol), cfg.min_points)
             for t, v in ((yt, row_lo[ys]), (yt, row_hi[ys]), (xt, col_lo[xs]), (xt, col_hi[xs]))]
    if any(ln is None for ln in lines):
        return None
    left, right, top, bottom = lines
    quad = []
    for (a1, b1), (a2, b2) in ((left, top), (right, top), (right, bottom), (left, bottom)):   # x = a1 y + b1 meets y = a2 x + b2
        d = 1.0 - a1 * a2
        if d == 0.0:
            return None
        x = (a1 * b2 + b1) / d
        quad.append((x, a2 * x + b2))
    return quad if _quad_ok(quad, H, W, cfg.min_area) else None


def find_page_quad(page, cfg=None):
    """The outline of the sheet in one photographed page -> [TL, TR, BR, BL] as (x, y) floats in the page's pixels, or None when no sheet
    is found or the sheet fills the frame (`fit_page_quad` has the rule).  One `ops.page_extents` call (two launches) and ONE device-to-host
    copy; the fit is float64 on the host."""
    from . import ops
    cfg = cfg or RectifyConfig()
    page = _device_page(page)
    H, W = page.shape
    return fit_page_quad(ops.page_extents(page, cfg.paper_threshold, cfg.resolved(H, W)).cpu(), H, W, cfg)


def _is_quad(q):
    return (isinstance(q, (list, tuple)) and len(q) == 4
            and all(isinstance(c, (list, tuple)) and len(c) == 2 and all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in c) for c in q))


def rectified_size(quad, cfg=None):
    """(OH, OW) a quad is rectified to: cfg.out_size, or the longer of each pair of opposite sides, rounded, plus one (pixel centres at both
    ends), within the page limits."""
    if cfg is not None and cfg.out_size is not None:
        return tuple(cfg.out_size)
    (tl, tr, br, bl), d = quad, lambda p, q: math.hypot(p[0] - q[0], p[1] - q[1])   # noqa: E731
    return (min(max(int(round(max(d(tl, bl), d(tr, br)))) + 1, 1), PAGE_MAX_H), min(max(int(round(max(d(tl, tr), d(bl, br)))) + 1, 1), PAGE_MAX_W))


def rectify_pages(pages, quads=None, cfg=None, fill=None):
    """One page or a list -> (the rectified pages, their quads).  quads: None - `find_page_quad` of every page with cfg - or one quad
    [TL, TR, BR, BL] for all pages, or a list with one per page in which an entry may be None (a UI lets its user tap the corners).  A page
    with a quad is sampled through `ops.homography_q30(quad, size, cfg.inset)` into a new page of `rectified_size(quad, cfg)` (one launch,
    ops.page_warp; fill: what lies outside the photo, default the paper); a page whose quad is None is returned as it is, with no launch."""
    from . import ops
    cfg = cfg or RectifyConfig()
    cfg.check()
    pages, _ = page_lists(pages, None)
    pages = [_device_page(p) for p in pages]
    if quads is None:
        quads = [find_page_quad(p, cfg) for p in pages]
    elif _is_quad(quads):
        quads = [quads] * len(pages)
    quads = list(quads)
    if len(quads) != len(pages) or not all(q is None or _is_quad(q) for q in quads):
        raise ValueError(f"{len(pages)} pages but {len(quads)} quads (each None or four (x, y) corners TL, TR, BR, BL)")
    quads = [None if q is None else [(float(x), float(y)) for x, y in q] for q in quads]
    out = []
    for p, q in zip(pages, quads):
        if q is None:
            out.append(p)
        else:
            size = rectified_size(q, cfg)
            out.append(ops.page_warp(p, ops.homography_q30(q, size, cfg.inset), size, fill))
    return out, quads


@dataclass
class OrientConfig:
    """Parameters of `estimate_orientation`:

      ink_threshold  a pixel is ink if its value (uint8 / 255) is below this;
      line_frac      a line row holds an ink run of at least ceil(line_frac * W) pixels, a line column one of ceil(line_frac * H);
      min_line_rows  a page is sideways only if it has at least this many line columns (and more of them than line rows);
      end_frac       the ends of a system of width w that are compared are its leftmost and rightmost max(1, round(end_frac * w)) columns;
      detect         the `DetectConfig` the systems are found with on the page turned level (None: its defaults).

    line_frac, min_line_rows as in `DetectConfig`; end_frac was chosen on synthetic pages (the clef, key and time signature of an engraved
    system fill about its first eighth): nothing has been measured on real photographs.  Anything else: ValueError."""
    ink_threshold: float = 0.5
    line_frac: float = 0.5
    min_line_rows: int = 5
    end_frac: float = 0.12
    detect: Optional[DetectConfig] = None

    def __post_init__(self):
        self.check()

    def check(self):
        if not _num(self.ink_threshold):
            raise ValueError(f"OrientConfig: ink_threshold = {self.ink_threshold!r} is not a number")
        if not _num(self.line_frac) or not 0 < self.line_frac <= 1:
            raise ValueError(f"OrientConfig: line_frac = {self.line_frac!r} is not a share in 0 .. 1")
        if isinstance(self.min_line_rows, bool) or not isinstance(self.min_line_rows, int) or self.min_line_rows < 1:
            raise ValueError(f"OrientConfig: min_line_rows = {self.min_line_rows!r} is not an integer >= 1")
        if not _num(self.end_frac) or not 0 < self.end_frac <= 0.5:
            raise ValueError(f"OrientConfig: end_frac = {self.end_frac!r} is not a share in 0 .. 0.5")
        if self.detect is not None and not isinstance(self.detect, DetectConfig):
            raise ValueError(f"OrientConfig: detect = {self.detect!r} is not None or a DetectConfig")


@dataclass
class StaffScale:
    """What `choose_staff_scale` reads off the run-length histograms of a page, in pixels of that page:

      line        the thickness of a staff line: the most frequent closed vertical ink run shorter than pitch_bin;
      space       the white between two staff lines, pitch_bin - line (also `staff_space`);
      pitch_bin   the distance from staff line to staff line: the most frequent sum of a closed ink run and the closed paper run under it;
      pitch       the same as a float: the count-weighted mean of the bins pitch_bin - 1 .. pitch_bin + 1;
      confidence  the share of all (ink run, paper run) pairs of the page that lie in those three bins, 0 .. 1."""
    line: int
    space: int
    pitch_bin: int
    pitch: float
    confidence: float

    @property
    def staff_space(self):
        return self.space


_GATES = ("min_staff_space", "min_model_staff_space", "min_sharpness", "min_focus", "min_contrast", "min_scale_confidence")


@dataclass
class AssessConfig:
    """Parameters of `estimate_staff_scale` and `assess_pages`:

      ink_threshold   a pixel is ink if its value (uint8 / 255) is below this, as in `DetectConfig`;
      paper_percent   `PageQuality.paper_level` is the level at or below which this share of the page's pixels lie (1 .. 100; 50: the
                      median, paper on any page that is mostly paper);
      ink_percent     `PageQuality.ink_level` likewise (1 .. 100; 2: darker than nearly everything, yet not one stray pixel);

    and the gate, six lower bounds that ALL default to None - no bound, `PageQuality.ok` is True and `reasons` is empty:

      min_staff_space        on `StaffScale.pitch`, pixels of the page from staff line to staff line (a page without a scale fails it);
      min_model_staff_space  on `PageResult.system_staff_space`, the same in pixels of what the model reads (`page_inference` only);
      min_sharpness          on `PageQuality.sharpness`;
      min_focus              on `PageQuality.focus`;
      min_contrast           on `PageQuality.contrast`, levels;
      min_scale_confidence   on `StaffScale.confidence` (a page without a scale fails it).

    No threshold is invented here: nothing in this repository can calibrate one (there are no real photographs in it, and no trained
    checkpoint whose error rate could be set against these numbers).  A caller who has both sets the bounds.  Anything else: ValueError,
    when the config is made and again when it is used."""
    ink_threshold: float = 0.5
    paper_percent: int = 50
    ink_percent: int = 2
    min_staff_space: Optional[float] = None
    min_model_staff_space: Optional[float] = None
    min_sharpness: Optional[float] = None
    min_focus: Optional[float] = None
    min_contrast: Optional[float] = None
    min_scale_confidence: Optional[float] = None

    def __post_init__(self):
        self.check()

    def check(self):
        if not _num(self.ink_threshold):
            raise ValueError(f"AssessConfig: ink_threshold = {self.ink_threshold!r} is not a number")
        for name in ("paper_percent", "ink_percent"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= 100:
                raise ValueError(f"AssessConfig: {name} = {v!r} is not an integer in 1 .. 100")
        for name in _GATES:
            v = getattr(self, name)
            if v is not None and (not _num(v) or v < 0 or v == float("inf")):
                raise ValueError(f"AssessConfig: {name} = {v!r} is not None or a finite number >= 0")
        if self.min_scale_confidence is not None and self.min_scale_confidence > 1:
            raise ValueError(f"AssessConfig: min_scale_confidence = {self.min_scale_confidence!r} is not a share in 0 .. 1")

    def failures(self, scale, sharpness, focus, contrast, model_staff_space=None):
        """The gate: one reason string per bound that is set and missed (model_staff_space: the smallest of the page's systems, None when
        it is not known - `assess_pages` - or the page has no system; the bound on it then does not apply)."""
        self.check()
        out = []

        def bound(name, value, what):
            lim = getattr(self, name)
            if lim is not None and (value is None or value < lim):
                out.append(f"{what} {'unknown' if value is None else format(value, '.6g')} is below {name} = {lim:g}")

        bound("min_staff_space", None if scale is None else scale.pitch, "staff space (pixels from line to line)")
        if model_staff_space is not None:
            bound("min_model_staff_space", model_staff_space, "staff space in model pixels")
        bound("min_sharpness", sharpness, "sharpness")
        bound("min_focus", focus, "focus")
        bound("min_contrast", contrast, "contrast")
        bound("min_scale_confidence", None if scale is None else scale.confidence, "staff scale confidence")
        return out


@dataclass
class PageQuality:
    """What `assess_pages` measures on one page:

      scale        its `StaffScale`, or None (a page without a closed ink run over a closed paper run: blank, or all ink);
      sharpness    the variance of the 4-neighbour Laplacian L = 4 p - up - down - left - right of the levels over the interior pixels: the
                   exact rational (n sum L^2 - (sum L)^2) / n^2 of the device's integer sums, converted to float once; 0.0 for a page
                   without interior pixels;
      paper_level, ink_level   the levels at `AssessConfig.paper_percent` and `ink_percent` of the level histogram;
      contrast     paper_level - ink_level;
      ink_share    the share of pixels whose level l counts as ink, float32(l) / 255 < ink_threshold;
      focus        sharpness / max(contrast, 1)^2, dimensionless: sharpness falls with the square of the contrast as well as with blur;
      ok, reasons  the gate of the `AssessConfig` (`AssessConfig.failures`): True and [] unless the caller set a bound that the page misses.

    sharpness and focus depend on what the page went through: bilinear resampling (rectify, deskew) lowers them a little and flattening
    stretches the levels, so values compare only under the same stage settings; `assess_pages` on the raw page judges the photo itself."""
    scale: Optional[StaffScale]
    sharpness: float
    paper_level: int
    ink_level: int
    contrast: int
    ink_share: float
    focus: float
    ok: bool = True
    reasons: tuple = ()


def choose_staff_scale(hists, cfg=None):
    """`ops.page_runs` of a page, on the host (a tensor or nested lists, [3][256] integers) -> its `StaffScale`, or None.  Integers, and
    float64 for the two quotients.  pitch_bin is the fullest of bins 2 .. 254 of row 2 (the lowest on ties; every bin empty: None - a
    blank page); line the fullest of bins 1 .. pitch_bin - 1 of row 0 (the lowest on ties); space = pitch_bin - line; pitch the
    count-weighted mean of bins pitch_bin - 1 .. pitch_bin + 1 of row 2; confidence the share of row 2's total in those three bins.
    cfg (an `AssessConfig`) is checked and otherwise unused: the rule has no parameter."""
    if cfg is not None:
        cfg.check()
    rows = hists.tolist() if torch.is_tensor(hists) else [list(r) for r in hists]
    if len(rows) != 3 or any(len(r) != 256 for r in rows):
        raise ValueError("choose_staff_scale: expected [3][256] run-length counts")
    ink, pair = [int(v) for v in rows[0]], [int(v) for v in rows[2]]
    pitch_bin = max(range(2, 255), key=lambda b: (pair[b], -b))
    if pair[pitch_bin] == 0:
        return None
    line = max(range(1, pitch_bin), key=lambda b: (ink[b], -b))
    near = range(pitch_bin - 1, pitch_bin + 2)
    n = sum(pair[b] for b in near)
    return StaffScale(line, pitch_bin - line, pitch_bin, sum(b * pair[b] for b in near) / n, n / sum(pair))


def _level_at(levels, percent):
    """The smallest level at or below which at least max(1, ceil(n * percent / 100)) of the n pixels lie (`ops.page_tile_levels`' rank)."""
    rank, acc = max(1, -(-sum(levels) * percent // 100)), 0
    for level, c in enumerate(levels):
        acc += c
        if acc >= rank:
            return level
    return 255


def page_quality(hists, stats, levels, cfg=None, model_staff_space=None):
    """The integers of `ops.page_runs` and `ops.page_sharpness`, on the host -> the `PageQuality` (`assess_pages` without the device)."""
    from fractions import Fraction
    cfg = cfg or AssessConfig()
    cfg.check()
    scale = choose_staff_scale(hists, cfg)
    s1, s2, n = (int(v) for v in stats)
    levels = [int(v) for v in levels]
    sharpness = float(Fraction(n * s2 - s1 * s1, n * n)) if n else 0.0
    paper, ink = _level_at(levels, cfg.paper_percent), _level_at(levels, cfg.ink_percent)
    thr = torch.tensor(float(cfg.ink_threshold), dtype=torch.float32)
    inked = (torch.arange(256, dtype=torch.float32) / torch.tensor(255.0, dtype=torch.float32) < thr).tolist()
    ink_share = sum(c for c, on in zip(levels, inked) if on) / max(sum(levels), 1)
    contrast = paper - ink
    focus = sharpness / max(contrast, 1) ** 2
    reasons = cfg.failures(scale, sharpness, focus, contrast, model_staff_space)
    return PageQuality(scale, sharpness, paper, ink, contrast, ink_share, focus, not reasons, tuple(reasons))


def _assess_launch(pages, cfg, sharp):
    """int64 [pages, 768 (+ 259)] on the device: one fill for all pages, then per page the launch pair of `ops.page_runs` and, with
    `sharp`, the launch of `ops.page_sharpness`."""
    from . import ops
    from ._lib import RUNS_WORDS, SHARP_WORDS
    pages, _ = page_lists(pages, None)
    pages = [_device_page(p) for p in pages]
    if not pages:
        raise ValueError("no pages")
    buf = torch.zeros(len(pages), RUNS_WORDS + (SHARP_WORDS if sharp else 0), dtype=torch.int64, device=pages[0].device)
    for p, row in zip(pages, buf):
        ops.page_runs(p, cfg.ink_threshold, out=row[:RUNS_WORDS])
        if sharp:
            ops.page_sharpness(p, out=row[RUNS_WORDS:])
    return buf


def assess_counts(pages, cfg=None):
    """The device half of `assess_pages`: per page (hists [3][256], stats [3], levels [256]) as lists of integers on the host, after the
    launches and the ONE copy of the call."""
    from ._lib import RUNS_WORDS
    cfg = cfg or AssessConfig()
    cfg.check()
    return [([r[0:256], r[256:512], r[512:RUNS_WORDS]], r[RUNS_WORDS:RUNS_WORDS + 3], r[RUNS_WORDS + 3:]) for r in _assess_launch(pages, cfg, True).cpu().tolist()]


def estimate_staff_scale(pages, cfg=None):
    """One page or a list -> per page its `StaffScale` or None (`choose_staff_scale`).  One launch pair per page (ops.page_runs) into one
    tensor, and ONE device-to-host copy for all pages."""
    from ._lib import RUNS_WORDS
    cfg = cfg or AssessConfig()
    cfg.check()
    return [choose_staff_scale([row[0:256], row[256:512], row[512:RUNS_WORDS]], cfg) for row in _assess_launch(pages, cfg, False).cpu().tolist()]


def assess_pages(pages, cfg=None, model_staff_space=None):
    """One page or a list -> per page its `PageQuality`: the staff scale from vertical run lengths, sharpness, contrast and focus from
    one more read of the page.  Three launches per page (ops.page_runs, ops.page_sharpness) after one fill, and ONE device-to-host copy
    per call; everything after the copy is integers and float64 on the host (`page_quality`).  The pages are judged as they are passed
    in: what `page_inference(assess=)` reports was measured behind its other stages (see `PageQuality`).  model_staff_space: per page
    the number `AssessConfig.min_model_staff_space` is held against, or None (the bound does not apply: it needs the resize).
    Out of scope: sizing flatten, deskew or rectify from the scale (they run before it can be measured), horizontal runs, a scale per
    system, any default threshold, and anything measured on real photographs (there are none here)."""
    cfg = cfg or AssessConfig()
    rows = assess_counts(pages, cfg)
    model = [None] * len(rows) if model_staff_space is None else list(model_staff_space)
    if len(model) != len(rows):
        raise ValueError(f"{len(rows)} pages but {len(model)} model staff spaces")
    return [page_quality(*r, cfg, m) for r, m in zip(rows, model)]


def _is_single_channel(page):
    return torch.is_tensor(page) and (page.dim() == 2 or (page.dim() == 3 and page.shape[0] == 1))


def _device_photo(page, device=None):
    """One decoded photo -> the same tensor on the GPU, in the layout and with the strides it came in (a CPU tensor is uploaded once, no
    host conversion); float types other than fp32 are widened to fp32 (single-channel only: `ops.page_ingest` refuses float colour)."""
    if not torch.is_tensor(page) or page.dim() not in (2, 3):
        raise TypeError("expected a photo as a (H,W), (H,W,C) or (C,H,W) tensor")
    if not torch.cuda.is_available():
        raise RuntimeError(NO_GPU)
    if not page.is_cuda:
        page = page.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    return page if page.dtype == torch.uint8 else page.to(torch.float32)


def photo_size(photo):
    """(H, W) of a photo as `ingest_pages` reads its shape (a tensor on the device)."""
    from .ops import _photo
    return _photo(photo)[:2]


def orientation_codes(orientation, n):
    """None, one EXIF code or one code per page -> the list of n codes (None: all 1).  Not an integer: TypeError; outside 1 .. 8 or the wrong
    number of them: ValueError."""
    from .ops import exif_code
    if orientation is None:
        return [1] * n
    if isinstance(orientation, (list, tuple)):
        if len(orientation) != n:
            raise ValueError(f"{n} pages but {len(orientation)} orientation codes")
        return [exif_code(c) for c in orientation]
    return [exif_code(orientation)] * n


def ingest_pages(pages, orientation=None, layout=None, device=None):
    """One decoded photo or a list -> the list of grey, upright (H', W') pages on the device, uint8 (fp32 for single-channel float input).
    A photo is (H, W), (1, H, W), interleaved (H, W, C) with C = 1, 3, 4 or planar (C, H, W) with C = 1, 3 (`ops._photo` says how the shape
    is read; layout = "hwc" / "chw" says it outright), uint8 - float colour is a TypeError.  orientation: None or 1 - grey only - or one
    EXIF code 1 .. 8 for all photos or a list with one per photo, applied as PIL's `ImageOps.exif_transpose` applies it.  A CPU tensor is
    uploaded once, in the layout it arrived in: the grey value (PIL's `convert("L")`) and the turn are ONE launch per photo on the device
    (ops.page_ingest).  A single-channel page with code 1 is returned as `_device_page` returns it: no launch, no copy."""
    from . import ops
    pages, _ = page_lists(pages, None)
    codes = orientation_codes(orientation, len(pages))
    out = []
    for p, c in zip(pages, codes):
        if c == 1 and layout is None and _is_single_channel(p):
            out.append(_device_page(p, device))
        else:
            out.append(ops.page_ingest(_device_photo(p, device), c, layout))
    return out


def orientation_is_sideways(run_rows, run_cols, H, W, cfg=None):
    """The first decision of `estimate_orientation`, on the host: run_rows [H] and run_cols [W] are the longest ink runs of the rows and of
    the columns.  A row is a line row if its run >= ceil(line_frac * W), a column a line column if its run >= ceil(line_frac * H); the page
    is sideways if it has at least min_line_rows line columns and more line columns than line rows."""
    cfg = cfg or OrientConfig()
    rows = sum(1 for v in run_rows if int(v) >= int(math.ceil(cfg.line_frac * W)))
    cols = sum(1 for v in run_cols if int(v) >= int(math.ceil(cfg.line_frac * H)))
    return cols >= cfg.min_line_rows and cols > rows


def orientation_end_boxes(boxes, cfg=None):
    """Per system box (x0, y0, x1, y1) its two ends, left then right: the leftmost and the rightmost e = max(1, round(end_frac * w)) columns
    (Python's rounding) over the box's rows -> a list of 2 n rectangles."""
    cfg = cfg or OrientConfig()
    out = []
    for x0, y0, x1, y1 in boxes:
        e = max(1, int(round(cfg.end_frac * (x1 - x0))))
        out += [(x0, y0, x0 + e, y1), (x1 - e, y0, x1, y1)]
    return out


def orientation_up_down(counts):
    """The second decision: the ink counts of `orientation_end_boxes` -> (upside down, confidence).  With L and R the sums over the left and
    the right ends, upside down iff R > L (no system, or a tie: upright); confidence = |L - R| / max(L + R, 1)."""
    left, right = sum(int(v) for v in counts[0::2]), sum(int(v) for v in counts[1::2])
    return right > left, abs(left - right) / max(left + right, 1)


def estimate_orientation(page, cfg=None):
    """One photo whose EXIF tag is missing -> (code, confidence): the orientation code, one of 1, 3, 6, 8 (mirrored pages do not occur in
    photos), that `ingest_pages` turns it upright with, and how lopsided the evidence for up against down was, 0.0 .. 1.0.  Colour photos
    are made grey first (one launch).  Two exact-integer decisions (`orientation_is_sideways`, `orientation_up_down`): the row and the
    column profile (ops.page_profile, ops.page_col_profile) say whether the staff lines run down the columns; if so the page is turned by
    code 6 into a temporary (ops.page_ingest); on the page whose lines are level the systems are detected (`detect_systems`) and ONE
    launch counts the ink of both ends of every system (ops.page_box_ink): a system begins with clef, key and time signature and ends with
    a thin barline, so the page is upside down iff the right ends hold more ink.  Level and upright: 1; level, upside down: 3; sideways and
    upright after the code-6 turn: 6; sideways and upside down after it: 8.  Four copies to the host (two profiles, the boxes, the counts).
    The up / down rule is a heuristic chosen on synthetic pages; nothing has been measured on real photographs.  A blank page, a page
    without systems and a tie give the code of an upright page with confidence 0.0."""
    from . import ops
    cfg = cfg or OrientConfig()
    cfg.check()
    if not torch.is_tensor(page):
        raise TypeError("estimate_orientation: expected one photo as a tensor")
    page = ingest_pages(page)[0]
    H, W = page.shape
    run_rows, run_cols = ops.page_profile(page, cfg.ink_threshold)[1].cpu().tolist(), ops.page_col_profile(page, cfg.ink_threshold)[1].cpu().tolist()
    sideways = orientation_is_sideways(run_rows, run_cols, H, W, cfg)
    level = ops.page_ingest(page, 6) if sideways else page
    rects = orientation_end_boxes(detect_systems(level, cfg.detect), cfg)
    if not rects:
        return (6 if sideways else 1), 0.0
    table = ops.h2d(torch.tensor(rects, dtype=torch.int32), level.device)
    down, confidence = orientation_up_down(ops.page_box_ink(level, table, cfg.ink_threshold).cpu().tolist())
    return ((8 if down else 6) if sideways else (3 if down else 1)), confidence


def orientation_to_photo_xy(code, source_size, x, y):
    """A point of the upright page -> the point of the (H, W) = source_size photo it was read from under orientation `code`: the index map
    of `ops.page_ingest` (integer coordinates are pixel centres, as in every other map here), exact for integers."""
    H, W = source_size
    return ((x, y), (W - 1 - x, y), (W - 1 - x, H - 1 - y), (x, H - 1 - y), (y, x), (y, H - 1 - x), (W - 1 - y, H - 1 - x), (W - 1 - y, x))[code - 1]


def orientation_from_photo_xy(code, source_size, px, py):
    """The inverse of `orientation_to_photo_xy`."""
    H, W = source_size
    return ((px, py), (W - 1 - px, py), (W - 1 - px, H - 1 - py), (px, H - 1 - py), (py, px), (H - 1 - py, px), (H - 1 - py, W - 1 - px), (py, W - 1 - px))[code - 1]


def system_staff_spaces(scales, plans):
    """Per system of `plan_systems`, the pitch of its page's `StaffScale` in MODEL pixels: pitch * resized height / box height (the resize
    scales both axes alike up to rounding; the height is the axis the pitch was measured along).  None where the page has no scale."""
    return [None if scales[p] is None else scales[p].pitch * size[0] / (y1 - y0) for p, (_, y0, _, y1), size, _ in plans]


def _pixel_box(box, H, W):
    x0, y0, x1, y1 = (int(v) for v in box)
    if not (0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H):
        raise ValueError(f"box {(x0, y0, x1, y1)} is empty or outside the {H} x {W} page")
    return x0, y0, x1, y1


def boxes_from_fractions(boxes, H, W):
    """The UI's boxes - dicts with x0, y0, x1, y1 or 4-tuples in that order, as fractions of the page - sorted by y0 (routes.py:122) -> pixel
    boxes.  Every coordinate is int(round(fraction * size)) with Python's rounding (ties to even), which is what PIL's `Image.crop` makes of
    the float box routes.py:126 hands it.  A box that comes out empty or outside the page: ValueError."""
    rows = [tuple(float(b[k]) for k in ("x0", "y0", "x1", "y1")) if isinstance(b, dict) else tuple(float(v) for v in b) for b in boxes]
    if any(len(r) != 4 for r in rows):
        raise ValueError("a box is x0, y0, x1, y1")
    return [_pixel_box((int(round(x0 * W)), int(round(y0 * H)), int(round(x1 * W)), int(round(y1 * H))), H, W)
            for x0, y0, x1, y1 in sorted(rows, key=lambda r: r[1])]


def pixel_boxes(boxes, H, W):
    """One page's boxes as a caller gives them - the UI's fraction boxes (the first is a dict, or holds a float: `boxes_from_fractions`)
    or pixel boxes (x0, y0, x1, y1) - -> pixel boxes of the H x W page, each checked to be non-empty and inside it."""
    fractions = bool(boxes) and (isinstance(boxes[0], dict) or any(isinstance(v, float) for v in boxes[0]))
    return boxes_from_fractions(boxes, H, W) if fractions else [_pixel_box(b, H, W) for b in boxes]


def _is_box(b):
    return isinstance(b, dict) or (isinstance(b, (list, tuple)) and len(b) == 4 and not isinstance(b[0], (list, tuple, dict)))


def page_lists(pages, boxes):
    """One page (with its boxes as one list) or a list of pages (with one list of boxes per page) -> the list form of both; boxes (where
    there are any) for another number of pages: ValueError."""
    if torch.is_tensor(pages):
        pages = [pages]
        if boxes is not None and (len(boxes) == 0 or _is_box(boxes[0])):
            boxes = [boxes]
    pages = list(pages)
    if boxes is not None and len(boxes) != len(pages):
        raise ValueError(f"{len(pages)} pages but boxes for {len(boxes)}")
    return pages, boxes


def plan_systems(pages_hw, boxes_per_page, resize):
    """[(page, (x0, y0, x1, y1), (OH, OW), (top, left, ch, cw)), ...] in page order, then in the order given: `resize._plan` of every box."""
    plans = []
    for p, ((H, W), boxes) in enumerate(zip(pages_hw, boxes_per_page)):
        for b in boxes:
            x0, y0, x1, y1 = _pixel_box(b, H, W)
            size, crop = resize._plan(y1 - y0, x1 - x0)
            plans.append((p, (x0, y0, x1, y1), size, crop))
    return plans


def split_pages(pages, boxes_per_page, resize, dtype=torch.float32):
    """`resize.to_patches` of every box of every page without cutting the boxes out first: pages = one page or a list (uint8, or float in
    [0, 1]), boxes_per_page = one list of pixel boxes (x0, y0, x1, y1) per page -> a `PackedPatches` with one image per box, in page order
    and then in the order given; its rows are, bit for bit, those of `resize.to_patches([page[y0:y1, x0:x1], ...])`.  One table upload and
    one `ops.crop_resize_to_patches` call (two launches) for everything."""
    from . import ops
    pages, boxes_per_page = page_lists(pages, boxes_per_page)
    pages = [_device_page(p, resize.device) for p in pages]
    plans = plan_systems([tuple(p.shape) for p in pages], boxes_per_page, resize)
    if not plans:
        raise ValueError("split_pages: no boxes")
    P = resize.patch_size
    dims = [(crop[2] // P, crop[3] // P) for _, _, _, crop in plans]
    out = torch.empty(sum(h * w for h, w in dims), P * P, dtype=dtype, device=pages[0].device)
    entries, row0, tmp_off = [], 0, 0
    for (p, (x0, y0, x1, y1), size, crop), (hp, wp) in zip(plans, dims):
        entries.append(ops.crop_resize_entry(pages[p], (x0, y0, x1 - x0, y1 - y0), size, crop, row0, tmp_off))
        row0 += hp * wp
        tmp_off += (y1 - y0) * size[1]
    ops.crop_resize_to_patches(entries, out, P, clamp01=True)
    return PackedPatches(out, dims, P)


_STAGES = {   # keyword of `page_inference` -> (its config, the test for values given in place of an estimate, those values in words)
    "orient": (OrientConfig, lambda v: not isinstance(v, bool) and isinstance(v, (int, list, tuple)), "one EXIF orientation code 1 .. 8 or a list with one per page"),
    "rectify": (RectifyConfig, lambda v: _is_quad(v) or (isinstance(v, (list, tuple)) and all(q is None or _is_quad(q) for q in v)),
                "one quad [TL, TR, BR, BL] or a list of quads (or None) per page"),
    "flatten": (FlattenConfig, None, None),
    "deskew": (SkewConfig, lambda v: _num(v) or (isinstance(v, (list, tuple)) and all(_num(a) for a in v)), "one angle in degrees or a list with one per page"),
    "assess": (AssessConfig, None, None)}


def resolve_stage(name, value):
    """The one rule for a stage keyword of `page_inference` -> (cfg, values).  None or False: (None, None), the stage is off.  True or an
    instance of the stage's config: (that config, None), the stage estimates with it.  What the stage's own test accepts - codes for
    orient (a bool is not a code), quads for rectify, angles for deskew: (the default config, the value), the stage applies the caller's
    values.  Anything else: TypeError.  Nothing is uploaded or launched; what is wrong with a number (a code outside 1 .. 8) is a
    ValueError from where the number is read."""
    Config, explicit, what = _STAGES[name]
    if value is None or value is False:
        return None, None
    if value is True or isinstance(value, Config):
        return (Config() if value is True else value), None
    if explicit is not None and explicit(value):
        return Config(), value
    raise TypeError(f"{name}: expected None, a bool{', ' if what else ' or '}a page.{Config.__name__}{', ' + what if what else ''}")


@dataclass
class Prepared:
    """What `prepare_pages` did to the pages, field for field what `PageResult` takes and documents under the same names
    (`PageResult(..., **vars(prepared))`).  A stage that was off leaves its field at None."""
    orientations: Optional[list]
    source_sizes: list
    quads: Optional[list]
    inset: float
    flattened: Optional[list]
    angles: Optional[list]
    page_sizes: list


def prepare_pages(pages, device=None, *, orient=None, rectify=None, flatten=None, deskew=None):
    """One page or a list, as `page_inference` takes them -> (the pages detection sees, on the device; the `Prepared` record).  The opt-in
    stages in their one order, ingest -> rectify -> flatten -> deskew (`ingest_pages`, `rectify_pages`, `flatten_pages`, `deskew_pages`
    say what each does and costs), every keyword by `resolve_stage`, all of them before the first upload.  With every stage off this is
    `ingest_pages(pages, None, device=device)` and nothing else.  orient=True estimates the code of every photo on a temporary
    (`estimate_orientation`) and then runs as orient=<those codes>: the same result, bit for bit."""
    (orient, codes), (rectify, quads) = resolve_stage("orient", orient), resolve_stage("rectify", rectify)
    (flatten, _), (deskew, angles) = resolve_stage("flatten", flatten), resolve_stage("deskew", deskew)
    pages, _ = page_lists(pages, None)
    if orient is None:
        pages = ingest_pages(pages, None, device=device)      # (single-channel pages: `_device_page` of each, nothing else)
        source_sizes = [tuple(p.shape) for p in pages]
    else:
        codes = None if codes is None else orientation_codes(codes, len(pages))
        photos = [_device_photo(p, device) for p in pages]
        if codes is None:
            codes = []
            for tmp in ingest_pages(photos):
                if rectify is not None and quads is None:     # a quad the caller gave refers to the upright page: the temporary is not it
                    tmp = rectify_pages(tmp, None, rectify)[0][0]
                if flatten is not None:
                    tmp = flatten_pages(tmp, flatten)[0]
                codes.append(estimate_orientation(tmp, orient)[0])
        source_sizes = [photo_size(p) for p in photos]
        pages = ingest_pages(photos, codes)
    if rectify is not None:
        pages, quads = rectify_pages(pages, quads, rectify)
    if flatten is not None:
        pages = flatten_pages(pages, flatten)
    if deskew is not None:
        pages, angles = deskew_pages(pages, angles, deskew)
    return pages, Prepared(orientations=codes, source_sizes=source_sizes, quads=quads, inset=2 if rectify is None else rectify.inset,
                           flattened=None if flatten is None else [True] * len(pages), angles=angles, page_sizes=[tuple(p.shape) for p in pages])


class PointMap(NamedTuple):
    """One link of the way from the page that was cropped back to the photo, a pair of functions of a point: `back(x, y)` leads towards
    the photo, `forth(x, y)` is its inverse.  `PageResult` keeps a list of them per page; a new stage that moves pixels adds one."""
    back: Callable
    forth: Callable


def turn_map(angle, size):
    """The turn that levelled an (H, W) = size page, as the kernel applied it: cos_q / 65536, sin_q / 65536 about the centre.  `back` takes a
    point of the levelled page to the page that was turned; `forth` is the exact inverse of that matrix (cos^2 + sin^2 is 1 only to 2^-16)."""
    from .ops import rotation_q16
    cos_q, sin_q = rotation_q16(angle)
    c, s, cx, cy = cos_q / 65536.0, sin_q / 65536.0, (size[1] - 1) / 2.0, (size[0] - 1) / 2.0
    det = c * c + s * s
    return PointMap(lambda x, y: (cx + c * (x - cx) - s * (y - cy), cy + s * (x - cx) + c * (y - cy)),
                    lambda x, y: (cx + (c * (x - cx) + s * (y - cy)) / det, cy + (c * (y - cy) - s * (x - cx)) / det))


def _project(m, x, y):
    den = m[6] * x + m[7] * y + m[8]
    return (m[0] * x + m[1] * y + m[2]) / den, (m[3] * x + m[4] * y + m[5]) / den


def homography_map(quad, size, inset):
    """The homography a page of (OH, OW) = size was rectified through: the nine integers of `ops.homography_q30(quad, size, inset)`, formed
    when a point is first mapped.  `back` takes a point of the rectified page to the page it was sampled from, in float64 (the kernel's own
    source coordinate is this, rounded down to 1 / 256 pixel); `forth` applies the adjugate of the integer matrix, formed exactly and
    scaled by its largest entry, in float64."""
    @functools.lru_cache(maxsize=None)
    def matrices():
        from .ops import homography_q30
        A, B, C, D, E, F, G, H, I = m = homography_q30(quad, size, inset)   # noqa: E741
        adj = [E * I - F * H, C * H - B * I, B * F - C * E, F * G - D * I, A * I - C * G, C * D - A * F, D * H - E * G, B * G - A * H, A * E - B * D]
        big = max(abs(v) for v in adj) or 1
        return [float(v) for v in m], [v / big for v in adj]   # (int / int: correctly rounded whatever the size)
    return PointMap(lambda x, y: _project(matrices()[0], x, y), lambda x, y: _project(matrices()[1], x, y))


def orientation_map(code, size):
    """The index map of orientation `code` on an (H, W) = size photo (`orientation_to_photo_xy` and its inverse): integers stay integers."""
    return PointMap(functools.partial(orientation_to_photo_xy, code, size), functools.partial(orientation_from_photo_xy, code, size))


class PageResult:
    """What `page_inference` returns.  Rows are systems, in page order and top to bottom within a page:

      boxes        per page, its list of pixel boxes (x0, y0, x1, y1), in the RECTIFIED and LEVELLED page when the page was rectified or
                   deskewed (what was cropped);
      flattened    per page, whether its illumination was flattened (what was cropped is then the flattened page);
      angles       per page, the angle in degrees it was turned by after rectification and flattening (0.0: not deskewed);
      page_sizes   per page, the (H, W) of the page that was turned and cropped - the rectified page when it was rectified: the turn is about
                   its centre (may be None when no page was turned or rectified);
      quads        per page, the corners [TL, TR, BR, BL] of the sheet in the page as it was passed in, or None: not rectified;
      source_sizes per page, the (H, W) of the page - the photo - as it was passed in (page_sizes when not given: nothing was rectified
                   or turned upright);
      orientations per page, the EXIF orientation code it was turned upright by before anything else (1: as it lay); rectification,
                   the quads and the angles refer to the upright page, of size `ops.oriented_size(*source_size, code)`;
      inset        the `RectifyConfig.inset` the quads were rectified with (the homography is `ops.homography_q30(quad, page_size, inset)`);
      seqs, log_probs, seq_mask   (N, T') as `continuous_inference` returns them, one row per system (None when there is no system at all);
      system_page  the page index of every row;
      sizes, windows   per row, the size (OH, OW) its box was resized to and the window (top, left, ch, cw) of it the model saw;
      patches_kept, patches_total   per row, the patches the encoder read and the patches of the window's grid: equal unless the call pruned
                   blank patches (page_inference(prune=), `prune.prune_patches`);
      quality      per page its `PageQuality`, measured on the page that detection saw, or None: the call did not assess
                   (page_inference(assess=));
      system_staff_space   per row, the distance from staff line to staff line in MODEL pixels - the page's `StaffScale.pitch` times the
                   resized height of the row's box over the box's height - or None: not assessed, or the page has no scale.  What
                   `AssessConfig.min_model_staff_space` is held against, and the number a UI needs to say "move closer";
      loops        one `loops.LoopReport` over the rows (stop, period, start per system; period 0 = the system did not loop), or None: the
                   call had no loop guard (page_inference(loop_guard=))."""

    def __init__(self, boxes, seqs, log_probs, seq_mask, system_page, sizes, windows, specials=(), angles=None, page_sizes=None, flattened=None,
                 quads=None, source_sizes=None, inset=2, orientations=None, patches_kept=None, patches_total=None, quality=None,
                 system_staff_space=None, loops=None):
        self.boxes, self.seqs, self.log_probs, self.seq_mask = boxes, seqs, log_probs, seq_mask
        self.loops = loops
        system_page = list(system_page)
        self.quality = [None] * len(boxes) if quality is None else list(quality)
        self.system_staff_space = [None] * len(system_page) if system_staff_space is None else [None if v is None else float(v) for v in system_staff_space]
        if len(self.quality) != len(boxes) or len(self.system_staff_space) != len(system_page):
            raise ValueError("PageResult: one quality (or None) per page and one staff space (or None) per system")
        self.patches_total = [None] * len(system_page) if patches_total is None else [int(n) for n in patches_total]   # (None: not recorded)
        self.patches_kept = list(self.patches_total) if patches_kept is None else [int(n) for n in patches_kept]
        if len(self.patches_total) != len(system_page) or len(self.patches_kept) != len(system_page):
            raise ValueError("PageResult: one patches_kept and one patches_total per system")
        self.quads = [None] * len(boxes) if quads is None else [None if q is None else [(float(x), float(y)) for x, y in q] for q in quads]
        self.source_sizes = None if source_sizes is None else [tuple(int(v) for v in hw) for hw in source_sizes]
        self.inset = inset
        if len(self.quads) != len(boxes) or (self.source_sizes is not None and len(self.source_sizes) != len(boxes)) or (
                any(q is not None for q in self.quads) and (page_sizes is None or len(page_sizes) != len(boxes))):
            raise ValueError("PageResult: one quad (or None) and one source size per page, and the page sizes with them when a page was rectified")
        self.flattened = [False] * len(boxes) if flattened is None else [bool(f) for f in flattened]
        if len(self.flattened) != len(boxes):
            raise ValueError("PageResult: one flattened flag per page")
        self.angles = [0.0] * len(boxes) if angles is None else [float(a) for a in angles]
        self.page_sizes = None if page_sizes is None else [tuple(int(v) for v in hw) for hw in page_sizes]
        if len(self.angles) != len(boxes) or (any(self.angles) and (self.page_sizes is None or len(self.page_sizes) != len(boxes))):
            raise ValueError("PageResult: one angle per page, and the page sizes with them when a page was turned")
        from .ops import exif_code
        self.orientations = [1] * len(boxes) if orientations is None else [exif_code(c) for c in orientations]
        if len(self.orientations) != len(boxes) or (any(c != 1 for c in self.orientations) and self.source_sizes is None):
            raise ValueError("PageResult: one orientation code per page, and the source sizes with them when a page was turned upright")
        if self.source_sizes is None:   # nothing was rectified: the page that was turned and cropped is the page that was passed in
            self.source_sizes = self.page_sizes
        self.system_page, self.sizes, self.windows = list(system_page), list(sizes), list(windows)
        self.specials = tuple(specials)   # the ids of <bos>, <eos>, <pad>: what tokens() leaves out
        self._flat = [b for page in boxes for b in page]
        self._maps = []   # per page its `PointMap`s, from the page that was cropped back to the photo; a stage that did nothing has none
        for p, (a, q, c) in enumerate(zip(self.angles, self.quads, self.orientations)):
            chain = [turn_map(a, self.page_sizes[p])] if a != 0.0 else []
            chain += [homography_map(q, self.page_sizes[p], inset)] if q is not None else []
            chain += [orientation_map(c, self.source_sizes[p])] if c != 1 else []
            self._maps.append(chain)

    def __len__(self):
        return len(self.system_page)

    def _rows(self, page):
        return [i for i, p in enumerate(self.system_page) if p == page]

    def tokens(self):
        """Per page, the tokens of its systems joined in reading order, without <bos>, <eos> and <pad>: a list of 1-D int64 tensors."""
        out = []
        for p in range(len(self.boxes)):
            parts = []
            for i in self._rows(p):
                t = self.seqs[i][self.seq_mask[i]]
                for s in self.specials:
                    t = t[t != s]
                parts.append(t)
            out.append(torch.cat(parts) if parts else torch.empty(0, dtype=torch.int64))
        return out

    def lmx(self, idxs_to_tokens):
        """Per page, `stringify_lmx_seq` of every system's row joined with " ", as the service joins them (routes.py:74-80, :179)."""
        return [" ".join(stringify_lmx_seq(self.seqs[i][self.seq_mask[i]], idxs_to_tokens) for i in self._rows(p)) for p in range(len(self.boxes))]

    @property
    def avg_log_probs(self):
        """Per system, sum(log_probs[mask]) / mask.sum(): the service's avgLogProb (routes.py:83).  fp32 (N,)."""
        if not len(self):
            return torch.empty(0)
        m = self.seq_mask
        return (self.log_probs * m).sum(1) / m.sum(1)

    @property
    def avg_confidence(self):
        """Per page, exp(mean of its systems' avg_log_probs): the service's avgConfidence (routes.py:190).  A page without systems: nan."""
        a = self.avg_log_probs
        return [math.exp(float(a[rows].mean())) if rows else float("nan") for rows in (self._rows(p) for p in range(len(self.boxes)))]

    def _affine(self, system):
        x0, y0, x1, y1 = self._flat[system]
        (OH, OW), (top, left, _, _) = self.sizes[system], self.windows[system]
        return x0, y0, (x1 - x0) / OW, (y1 - y0) / OH, top, left

    def to_source_xy(self, page, x, y):
        """A point of `page` as it was cropped (where `boxes` lie) -> the point of the page or photo the caller passed in: the page's maps
        backwards, one after the other - the turn, the homography, the orientation.  A page that only had its orientation changed keeps
        integers integers (a pixel for a pixel)."""
        for m in self._maps[page]:
            x, y = m.back(x, y)
        return x, y

    _to_source = to_source_xy   # the name this map had while it was private: kept for callers written against it

    def from_source_xy(self, page, x, y):
        """The inverse of `to_source_xy`: the same maps forwards, last first."""
        for m in reversed(self._maps[page]):
            x, y = m.forth(x, y)
        return x, y

    def to_page_xy(self, system, x, y):
        """Pixel (x, y) of the tensor the model saw of `system` (its box resized, then cropped to the window) -> pixels (floats) of the page
        the caller passed in: the resize's own map, source = (resized + 0.5) * scale - 0.5 per axis (align_corners = False), shifted by the
        window and the box, then `to_source_xy`.  With it a `TokenAlignment` of the system can be drawn on the page."""
        x0, y0, sx, sy, top, left = self._affine(system)
        return self.to_source_xy(self.system_page[system], x0 + (x + left + 0.5) * sx - 0.5, y0 + (y + top + 0.5) * sy - 0.5)

    def from_page_xy(self, system, px, py):
        """The inverse of `to_page_xy`."""
        x0, y0, sx, sy, top, left = self._affine(system)
        px, py = self.from_source_xy(self.system_page[system], px, py)
        return (px - x0 + 0.5) / sx - 0.5 - left, (py - y0 + 0.5) / sy - 0.5 - top

    def box_corners(self, system):
        """The corners (x0, y0), (x1, y0), (x1, y1), (x0, y1) of `system`'s box in the page the caller passed in: the box itself for a page
        that was neither rectified nor deskewed, a quadrilateral otherwise (for a UI to draw)."""
        x0, y0, x1, y1 = self._flat[system]
        return [self.to_source_xy(self.system_page[system], float(x), float(y)) for x, y in ((x0, y0), (x1, y0), (x1, y1), (x0, y1))]


def measure_boxes(page_result, report):
    """Each system's measure boxes on the page (host glue; an extension): for every row of `page_result` the list of its measures' boxes,
    each as the four corners (x0, y0), (x1, y0), (x1, y1), (x0, y1) of `report.box_px` - a `measures.MeasureReport` of the same rows, whose
    boxes are pixels of the tensor the model saw - taken to the pixels of the page the caller passed in (`PageResult.to_page_xy`: a
    quadrilateral when the page was rectified or turned, as `PageResult.box_corners` gives for the system itself).  A measure without a
    box (no map rows) is None.  One copy of the boxes to the host."""
    if report.box_px.shape[0] != len(page_result):
        raise ValueError(f"measure_boxes: a report of {report.box_px.shape[0]} rows for {len(page_result)} systems")
    boxes, counts = report.box_px.cpu().tolist(), report.count.cpu().tolist()
    out = []
    for s, (row, c) in enumerate(zip(boxes, counts)):
        quads = []
        for x0, y0, x1, y1 in row[:min(int(c), len(row))]:
            if math.isnan(x0):
                quads.append(None)
            else:
                quads.append([page_result.to_page_xy(s, x, y) for x, y in ((x0, y0), (x1, y0), (x1, y1), (x0, y1))])
        out.append(quads)
    return out
