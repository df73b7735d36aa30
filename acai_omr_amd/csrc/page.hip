// Whole pages (an extension; the reference's service crops hand-drawn boxes with PIL and decodes them one by one, acai_omr/ui/routes.py:93-129):
//   acai_page_profile            per row, the number of ink pixels and the longest run of them (a staff line is a long run),
//   acai_page_systems            the profiles -> bands of inked rows -> the bands that hold staff lines -> their boxes, all on the device,
//   acai_crop_resize_to_patches  every box of every page cut out, resized (the arithmetic of resize.hip, csrc/resize_taps.h) and written
//                                as patch rows in two launches.
// All three are bound by reading the page once or twice (an A4 page at 300 dpi is 8.7 MB of uint8); integer results use no atomics and
// reduce in a fixed order, so they do not depend on how the launches are scheduled.
#include "common.h"
#include "resize_taps.h"

namespace {

constexpr int LANE_PX = ACAI_PAGE_LANE_PIXELS, WAVE_PX = 64 * LANE_PX, PROFILE_WAVES = ACAI_PAGE_WAVES;

template <typename TI>
__device__ __forceinline__ bool is_ink(const TI *p, float thr) { return in_sample(p) < thr; }

// ---- profile ----------------------------------------------------------------------------------------------------------------------------
// What a stretch of pixels contributes to the longest run of the row it lies in: its length, the ink run it starts with, the one it ends
// with (both = len when it is all ink), the longest one inside it, and its ink count.  `join` is associative (not commutative).
struct Runs {
    int len, pre, suf, best, ink;
};

__device__ __forceinline__ Runs join(const Runs &a, const Runs &b) {
    Runs r;
    r.len = a.len + b.len;
    r.pre = a.pre == a.len ? a.len + b.pre : a.pre;
    r.suf = b.suf == b.len ? b.len + a.suf : b.suf;
    r.best = max(max(a.best, b.best), a.suf + b.pre);
    r.ink = a.ink + b.ink;
    return r;
}

__device__ __forceinline__ Runs shfl_down_runs(const Runs &a, int o) {
    return Runs{__shfl_down(a.len, o), __shfl_down(a.pre, o), __shfl_down(a.suf, o), __shfl_down(a.best, o), __shfl_down(a.ink, o)};
}

// One workgroup of 4 waves per row.  Wave w owns the contiguous span [w span, (w + 1) span) and walks it in steps of 256 pixels; in a step
// lane l holds the 4 consecutive pixels from 4 l on, so a wave reads 256 consecutive elements per step.  The lanes' summaries are joined in
// lane order by a shuffle-down tree (lane 0 ends up with the step's), lane 0 joins the steps, and thread 0 joins the four spans through LDS.
// Pixels past W count as paper, which ends a run like the edge of the page does.
template <typename TI>
__global__ __launch_bounds__(64 * PROFILE_WAVES) void page_profile_kernel(const TI *__restrict__ page, int W, int pitch, int span, float thr,
                                                                          int32_t *__restrict__ ink, int32_t *__restrict__ run) {
    __shared__ Runs parts[PROFILE_WAVES];
    const int y = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const TI *row = page + (size_t)y * pitch;
    Runs acc{0, 0, 0, 0, 0};
    for (int x0 = wave * span; x0 < (wave + 1) * span && x0 < W; x0 += WAVE_PX) {
        const int x = x0 + lane * LANE_PX;
        Runs r{0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < LANE_PX; ++k) {
            const bool on = x + k < W && is_ink(row + x + k, thr);
            r = join(r, Runs{1, on, on, on, on});
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const Runs other = shfl_down_runs(r, o);   // (a lane whose partner lies past lane 63 joins garbage; lane 0 never depends on it)
            r = join(r, other);
        }
        acc = join(acc, r);
    }
    if (lane == 0) parts[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        Runs t = parts[0];
        for (int w = 1; w < PROFILE_WAVES; ++w) t = join(t, parts[w]);
        ink[y] = t.ink;
        run[y] = t.best;
    }
}

// ---- bands ------------------------------------------------------------------------------------------------------------------------------
constexpr int BAND_THREADS = 1024, BAND_WAVES = BAND_THREADS / 64;

// Exclusive scan of one value per thread over the workgroup with a commutative `op`: forward (over the threads before this one) or, with
// REV, backward (over the threads after it).  `wtot` holds one value per wave.
template <bool REV, typename T, typename Op>
__device__ __forceinline__ T block_scan_excl(T v, T ident, Op op, T *wtot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T other = REV ? __shfl_down(inc, o) : __shfl_up(inc, o);
        if (REV ? lane + o < 64 : lane >= o) inc = op(inc, other);
    }
    __syncthreads();   // (the previous scan's readers of wtot are done)
    if (lane == (REV ? 0 : 63)) wtot[wave] = inc;
    __syncthreads();
    T ex = REV ? __shfl_down(inc, 1) : __shfl_up(inc, 1);
    if (lane == (REV ? 63 : 0)) ex = ident;
    for (int w = 0; w < BAND_WAVES; ++w)
        if (REV ? w > wave : w < wave) ex = op(ex, wtot[w]);
    return ex;
}

struct BandArgs {
    const int32_t *ink, *run;
    int H, W, min_ink, merge_gap, min_height, line_len, min_line_rows, max_systems;
};

// One workgroup; thread t owns the R = ceil(H / 1024) consecutive rows from t R on and walks them a few times, with what it needs to know
// about the rows of other threads arriving through five scans:
//   1. the last inked row before its rows, 2. the first inked row after them  -> which inked rows start and which end a band,
//   3. the number of line rows (run >= line_len) before its rows              -> line rows of a band = a difference of two prefix counts,
//   4. the latest band start before its rows, packed with the prefix count there -> an end row knows its band's y0 and line rows,
//   5. the number of kept bands that end before its rows                      -> the box index; the total is the count.
// A kept band k < max_systems leaves (0, y0, W, y1) in boxes[k] for page_extent_kernel to finish.
__global__ __launch_bounds__(BAND_THREADS) void page_bands_kernel(BandArgs a, int32_t *__restrict__ count, int32_t *__restrict__ boxes) {
    __shared__ unsigned long long wtot[BAND_WAVES];
    int *wtot32 = reinterpret_cast<int *>(wtot);
    const int R = (a.H + BAND_THREADS - 1) / BAND_THREADS;
    const int r0 = min((int)threadIdx.x * R, a.H), r1 = min(r0 + R, a.H);
    const int NONE = 0x7fffffff;
    auto imax = [](int p, int q) { return max(p, q); };
    auto imin = [](int p, int q) { return min(p, q); };
    auto iadd = [](int p, int q) { return p + q; };
    auto umax = [](unsigned long long p, unsigned long long q) { return p > q ? p : q; };

    int last = -1, first = NONE, lines = 0;
    for (int y = r0; y < r1; ++y) {
        if (a.ink[y] >= a.min_ink) {
            last = y;
            if (first == NONE) first = y;
        }
        lines += a.run[y] >= a.line_len;
    }
    const int prev_in = block_scan_excl<false>(last, -1, imax, wtot32);
    const int next_in = block_scan_excl<true>(first, NONE, imin, wtot32);
    const int lines_in = block_scan_excl<false>(lines, 0, iadd, wtot32);

    // a band start as (row + 1) << 32 | line rows before it: the largest is the latest, 0 is none
    auto walk_starts = [&](unsigned long long start, auto &&at_inked) {
        int prev = prev_in, L = lines_in;
        for (int y = r0; y < r1; ++y) {
            if (a.ink[y] >= a.min_ink) {
                if (prev < 0 || y - prev - 1 > a.merge_gap) start = ((unsigned long long)(y + 1) << 32) | (unsigned)L;
                prev = y;
                at_inked(y, start, L + (a.run[y] >= a.line_len));
            }
            L += a.run[y] >= a.line_len;
        }
        return start;
    };
    const unsigned long long own_start = walk_starts(0ull, [](int, unsigned long long, int) {});
    const unsigned long long start_in = block_scan_excl<false>(own_start, 0ull, umax, wtot);

    // every inked row q is judged once its successor is known: the next inked row of this thread, or next_in behind its last one
    auto walk_ends = [&](auto &&at_kept) {
        int q = -1, qL = 0;
        unsigned long long qstart = 0;
        auto judge = [&](int next) {
            if (q < 0 || (next != NONE && next - q - 1 <= a.merge_gap)) return;
            const int y0 = (int)(qstart >> 32) - 1, y1 = q + 1, nlines = qL - (int)(unsigned)qstart;
            if (y1 - y0 >= a.min_height && nlines >= a.min_line_rows) at_kept(y0, y1);
        };
        walk_starts(start_in, [&](int y, unsigned long long start, int L_incl) {
            judge(y);
            q = y, qL = L_incl, qstart = start;
        });
        judge(next_in);
    };
    int kept = 0;
    walk_ends([&](int, int) { ++kept; });
    int k = block_scan_excl<false>(kept, 0, iadd, wtot32);
    if (threadIdx.x == BAND_THREADS - 1) count[0] = k + kept;
    walk_ends([&](int y0, int y1) {
        if (k < a.max_systems) {
            int32_t *b = boxes + (size_t)k * 4;
            b[0] = 0, b[1] = y0, b[2] = a.W, b[3] = y1;
        }
        ++k;
    });
}

// The ink test in the element's own domain, for whole 16-byte loads: a uint8 value v is ink iff (float)v / 255 < thr, which is monotone in
// v, so iff v < the first value that is not (found by bisection with the very comparison the profile makes); fp32 compares as it is.
__device__ __forceinline__ int ink_limit_u8(float thr) {
    int lo = 0, hi = 256;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const unsigned char v = (unsigned char)mid;
        if (is_ink(&v, thr)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// One workgroup per box slot: the ink extent of rows [y0, y1) and the margins.  Wave w takes rows y0 + w, y0 + w + 16, ...  Where every row
// starts on a 16-byte boundary (base and pitch allow it: any contiguous page whose width is a multiple of 16 bytes) a lane reads 16 bytes
// per step, 1 KiB per wave; the columns behind the last whole 16 bytes, or all columns of a page that is not aligned, go one per lane.
template <typename TI>
__global__ __launch_bounds__(BAND_THREADS) void page_extent_kernel(const TI *__restrict__ page, int H, int W, int pitch, float thr, int margin,
                                                                   const int32_t *__restrict__ count, int32_t *__restrict__ boxes) {
    constexpr int VEC = 16 / (int)sizeof(TI);
    __shared__ int lo_s[BAND_WAVES], hi_s[BAND_WAVES];
    if ((int)blockIdx.x >= count[0]) return;
    int32_t *b = boxes + (size_t)blockIdx.x * 4;
    const int y0 = b[1], y1 = b[3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool aligned = ((reinterpret_cast<uintptr_t>(page) | ((size_t)pitch * sizeof(TI))) & 15) == 0;
    const int xv = aligned ? W / VEC * VEC : 0;
    const int limit = sizeof(TI) == 1 ? ink_limit_u8(thr) : 0;
    int lo = W, hi = 0;
    for (int y = y0 + wave; y < y1; y += BAND_WAVES) {
        const TI *row = page + (size_t)y * pitch;
        for (int x = lane * VEC; x < xv; x += 64 * VEC) {
            const uint4 v = *reinterpret_cast<const uint4 *>(row + x);
            const unsigned int word[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                bool on;
                if constexpr (sizeof(TI) == 1) on = (int)((word[k >> 2] >> (8 * (k & 3))) & 255u) < limit;
                else on = __uint_as_float(word[k]) < thr;
                if (on) lo = min(lo, x + k), hi = max(hi, x + k + 1);
            }
        }
        for (int x = xv + lane; x < W; x += 64)
            if (is_ink(row + x, thr)) lo = min(lo, x), hi = max(hi, x + 1);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lo = min(lo, __shfl_xor(lo, o)), hi = max(hi, __shfl_xor(hi, o));
    if (lane == 0) lo_s[wave] = lo, hi_s[wave] = hi;
    __syncthreads();   // (every thread has read y0 and y1 by now: thread 0 may overwrite them)
    if (threadIdx.x == 0) {
        for (int w = 1; w < BAND_WAVES; ++w) lo = min(lo, lo_s[w]), hi = max(hi, hi_s[w]);
        b[0] = max(lo - margin, 0), b[1] = max(y0 - margin, 0), b[2] = min(hi + margin, W), b[3] = min(y1 + margin, H);
    }
}

// ---- crop + resize into the patch stream ------------------------------------------------------------------------------------------------
// Width pass of every box: grid (x tiles of the widest target, rows of the tallest box, entries); blocks past an entry's own size leave.
__global__ __launch_bounds__(256) void crop_resize_width_kernel(const AcaiCropResize *__restrict__ table, float *__restrict__ tmp) {
    const AcaiCropResize e = table[blockIdx.z];
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (y >= e.h || x >= e.OW) return;
    const Axis ax = make_axis(e.w, e.OW);
    const size_t off = (size_t)(e.y0 + y) * e.pitch + e.x0;   // element 0 of the box's row: the window is clamped to [0, w) of the BOX
    const float t = e.in_u8 ? resample(ax, x, reinterpret_cast<const unsigned char *>(e.page) + off, 1)
                            : resample(ax, x, reinterpret_cast<const float *>(e.page) + off, 1);
    tmp[e.tmp_off + (size_t)y * e.OW + x] = t;
}

// Height pass: grid (x tiles, rows of the tallest target, entries); samples outside an entry's crop window are not computed.
__global__ __launch_bounds__(256) void crop_resize_height_kernel(const AcaiCropResize *__restrict__ table, const float *__restrict__ tmp,
                                                                 void *__restrict__ patches, int ld, int P, int bf16, int clamp01) {
    const AcaiCropResize e = table[blockIdx.z];
    const int x = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    const int y = i - e.top, xx = x - e.left;
    if (i >= e.OH || x >= e.OW || y < 0 || y >= e.ch || xx < 0 || xx >= e.cw) return;
    const Axis ay = make_axis(e.h, e.OH);
    float t = resample(ay, i, tmp + e.tmp_off + x, (size_t)e.OW);
    if (clamp01) t = fminf(fmaxf(t, 0.f), 1.f);
    store_patch_sample(PatchOut{patches, ld, e.row0, P, e.top, e.left, e.ch, e.cw, bf16}, y, xx, t);
}

}  // namespace

#define ACAI_PAGE_CHECK(name)                                                                                                                   \
    ACAI_CHECK_ARG(page, name ": null page");                                                                                                    \
    ACAI_CHECK_ARG(H > 0 && W > 0 && H <= ACAI_PAGE_MAX_H && W <= ACAI_PAGE_MAX_W && pitch >= W, name ": bad page %d x %d, pitch %d (H <= %d, W <= %d)", H, W, \
                   pitch, ACAI_PAGE_MAX_H, ACAI_PAGE_MAX_W)

extern "C" int acai_page_profile(const void *page, int in_u8, int H, int W, int pitch, float ink_threshold, int32_t *ink, int32_t *run, void *stream) {
    ACAI_PAGE_CHECK("acai_page_profile");
    ACAI_CHECK_ARG(ink && run, "acai_page_profile: null output");
    hipStream_t st = (hipStream_t)stream;
    const int span = cdiv(cdiv(W, PROFILE_WAVES), WAVE_PX) * WAVE_PX;
    if (in_u8)
        hipLaunchKernelGGL(page_profile_kernel<unsigned char>, dim3(H), dim3(64 * PROFILE_WAVES), 0, st, reinterpret_cast<const unsigned char *>(page), W, pitch,
                           span, ink_threshold, ink, run);
    else
        hipLaunchKernelGGL(page_profile_kernel<float>, dim3(H), dim3(64 * PROFILE_WAVES), 0, st, reinterpret_cast<const float *>(page), W, pitch, span,
                           ink_threshold, ink, run);
    ACAI_LAUNCH_CHECK("acai_page_profile");
    return 0;
}

extern "C" int acai_page_systems(const void *page, int in_u8, int H, int W, int pitch, float ink_threshold, const int32_t *ink, const int32_t *run,
                                 int min_ink, int merge_gap, int min_height, int line_len, int min_line_rows, int margin, int max_systems,
                                 int32_t *count, int32_t *boxes, void *stream) {
    ACAI_PAGE_CHECK("acai_page_systems");
    ACAI_CHECK_ARG(ink && run && count && boxes, "acai_page_systems: null operand");
    // (min_ink >= 1: an inked row then has an ink pixel, so every kept band has an extent)
    ACAI_CHECK_ARG(min_ink >= 1 && merge_gap >= 0 && min_height >= 0 && line_len >= 0 && min_line_rows >= 0 && margin >= 0,
                   "acai_page_systems: min_ink = %d must be >= 1 and merge_gap, min_height, line_len, min_line_rows, margin >= 0", min_ink);
    ACAI_CHECK_ARG(max_systems > 0 && max_systems <= 65535, "acai_page_systems: max_systems = %d is a grid dimension (1 .. 65535)", max_systems);
    hipStream_t st = (hipStream_t)stream;
    const BandArgs a{ink, run, H, W, min_ink, merge_gap, min_height, line_len, min_line_rows, max_systems};
    hipLaunchKernelGGL(page_bands_kernel, dim3(1), dim3(BAND_THREADS), 0, st, a, count, boxes);
    ACAI_LAUNCH_CHECK("acai_page_systems (bands)");
    if (in_u8)
        hipLaunchKernelGGL(page_extent_kernel<unsigned char>, dim3(max_systems), dim3(BAND_THREADS), 0, st, reinterpret_cast<const unsigned char *>(page), H, W,
                           pitch, ink_threshold, margin, count, boxes);
    else
        hipLaunchKernelGGL(page_extent_kernel<float>, dim3(max_systems), dim3(BAND_THREADS), 0, st, reinterpret_cast<const float *>(page), H, W, pitch,
                           ink_threshold, margin, count, boxes);
    ACAI_LAUNCH_CHECK("acai_page_systems (extents)");
    return 0;
}

extern "C" int acai_crop_resize_to_patches(const AcaiCropResize *table, const AcaiCropResize *host_table, int n, float *tmp, int64_t tmp_elems,
                                           void *patches, int ld, int64_t patch_rows, int P, int out_dtype, int clamp01, void *stream) {
    ACAI_CHECK_ARG(table && host_table && tmp && patches, "acai_crop_resize_to_patches: null operand");
    ACAI_CHECK_ARG(n > 0 && n <= 65535, "acai_crop_resize_to_patches: %d entries: the entry is a grid dimension (1 .. 65535)", n);
    ACAI_CHECK_ARG(P > 0 && ld >= P * P && patch_rows >= 0 && tmp_elems >= 0, "acai_crop_resize_to_patches: bad P = %d, ld = %d", P, ld);
    ACAI_CHECK_ARG(out_dtype == ACAI_F32 || out_dtype == ACAI_BF16, "acai_crop_resize_to_patches: bad output dtype");
    int max_h = 0, max_oh = 0, max_ow = 0;
    for (int i = 0; i < n; ++i) {
        const AcaiCropResize &e = host_table[i];
        ACAI_CHECK_ARG(e.page && e.page_h > 0 && e.page_w > 0 && e.pitch >= e.page_w, "acai_crop_resize_to_patches: entry %d: bad page %d x %d, pitch %d", i,
                       e.page_h, e.page_w, e.pitch);
        ACAI_CHECK_ARG(e.x0 >= 0 && e.y0 >= 0 && e.w > 0 && e.h > 0 && e.x0 <= e.page_w - e.w && e.y0 <= e.page_h - e.h,
                       "acai_crop_resize_to_patches: entry %d: box (x0 %d, y0 %d, w %d, h %d) outside its %d x %d page", i, e.x0, e.y0, e.w, e.h, e.page_h,
                       e.page_w);
        ACAI_CHECK_ARG(e.OH > 0 && e.OW > 0 && e.top >= 0 && e.left >= 0 && e.ch > 0 && e.cw > 0 && e.top <= e.OH - e.ch && e.left <= e.OW - e.cw &&
                           e.ch % P == 0 && e.cw % P == 0,
                       "acai_crop_resize_to_patches: entry %d: crop window (%d, %d, %d, %d) outside %d x %d or not a multiple of the patch size", i, e.top,
                       e.left, e.ch, e.cw, e.OH, e.OW);
        ACAI_CHECK_ARG(e.h <= 65535 && e.OH <= 65535, "acai_crop_resize_to_patches: entry %d: h and OH are grid dimensions (<= 65535)", i);
        ACAI_CHECK_ARG(e.row0 >= 0 && (int64_t)e.row0 + (int64_t)(e.ch / P) * (e.cw / P) <= patch_rows,
                       "acai_crop_resize_to_patches: entry %d: rows %d .. lie outside the %lld rows of the patch stream", i, e.row0, (long long)patch_rows);
        ACAI_CHECK_ARG(e.tmp_off >= 0 && e.tmp_off + (int64_t)e.h * e.OW <= tmp_elems,
                       "acai_crop_resize_to_patches: entry %d: its %d x %d width-pass samples at %lld lie outside tmp (%lld floats)", i, e.h, e.OW,
                       (long long)e.tmp_off, (long long)tmp_elems);
        max_h = e.h > max_h ? e.h : max_h, max_oh = e.OH > max_oh ? e.OH : max_oh, max_ow = e.OW > max_ow ? e.OW : max_ow;
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(crop_resize_width_kernel, dim3(cdiv(max_ow, 256), max_h, n), dim3(256), 0, st, table, tmp);
    ACAI_LAUNCH_CHECK("acai_crop_resize_to_patches (width)");
    hipLaunchKernelGGL(crop_resize_height_kernel, dim3(cdiv(max_ow, 256), max_oh, n), dim3(256), 0, st, table, (const float *)tmp, patches, ld, P,
                       out_dtype == ACAI_BF16 ? 1 : 0, clamp01);
    ACAI_LAUNCH_CHECK("acai_crop_resize_to_patches (height)");
    return 0;
}
