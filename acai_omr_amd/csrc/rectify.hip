// Page rectification (an extension; the reference's service takes "phone captured JPEGs" as they come, acai_omr/ui/routes.py): a photographed
// sheet is a quadrilateral of paper on something darker.
//   acai_page_extents   per row and per column, where the first and the last run of at least R paper pixels lies: the points the host fits
//                       the sheet's four edges through,
//   acai_page_warp      the page sampled through a homography with integer coefficients, bilinear, with the taps and the blend of
//                       acai_page_rotate.
// Every result is defined in integers (the fp32 blend aside): partial results meet by integer min / max only, and the warp's source
// coordinates are exact floor quotients of 64-bit integers, so nothing depends on how the launches are scheduled.
#include "common.h"
#include "resize_taps.h"

namespace {

// ---- extents ----------------------------------------------------------------------------------------------------------------------------
constexpr int EXT_THREADS = 256, EXT_ROW_WAVES = EXT_THREADS / 64, EXT_UNITS = 32, EXT_COL_ROWS = ACAI_EXTENTS_TILE_ROWS, EXT_MAX_RUN = ACAI_EXTENTS_MAX_RUN;

// (deskew.hip and page.hip have the same function: the first uint8 value that is not ink at thr, by bisection with the comparison the
// per-element path makes)
__device__ __forceinline__ int ink_limit_u8(float thr) {
    int lo = 0, hi = 256;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const unsigned char v = (unsigned char)mid;
        if (in_sample(&v) < thr) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The paper bits of one loaded unit.
template <typename TI>
__device__ __forceinline__ unsigned int unit_bits(const uint4 v, float thr, int limit) {
    constexpr int VEC = 16 / (int)sizeof(TI);
    const unsigned int word[4] = {v.x, v.y, v.z, v.w};
    unsigned int m = 0;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        bool ink;
        if constexpr (sizeof(TI) == 1) ink = (int)((word[k >> 2] >> (8 * (k & 3))) & 255u) < limit;
        else ink = __uint_as_float(word[k]) < thr;
        m |= (unsigned int)!ink << k;
    }
    return m;
}

// A unit is 16 bytes of a row (16 uint8 pixels or 4 fp32 ones) starting at column x; bit k of the result says that pixel x + k is paper,
// that is, not ink.  A unit inside the row and on a 16-byte boundary is one load; the unit across W, and every unit of a page that is not
// aligned, goes element by element; pixels from W on are never read and never paper (they end every run).
template <typename TI>
__device__ __forceinline__ unsigned int paper_bits(const TI *__restrict__ src, int x, int W, bool aligned, float thr, int limit) {
    constexpr int VEC = 16 / (int)sizeof(TI);
    unsigned int m = 0;
    if (x >= W) return 0;
    if (aligned && x + VEC <= W) {
        m = unit_bits<TI>(*reinterpret_cast<const uint4 *>(src), thr, limit);
    } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k)
            if (x + k < W) m |= (unsigned int)!(in_sample(src + k) < thr) << k;
    }
    return m;
}

// Rows.  A wave owns a row and walks it in steps of 64 units, one unit per lane.  A stretch [a, b) of the row is summed up by four numbers:
//   pe   the first pixel that is not paper (b if all are): [a, pe) is the paper run at its start,
//   ss   one past the last pixel that is not paper (a if all are paper): [ss, b) is the paper run at its end,
//   lo   the smallest start and hi the largest end of a run of >= R paper pixels found inside it (W and -1: none yet).
// Two neighbouring stretches A = [a, mid), B = [mid, b) join to one: the run across the seam is [A.ss, B.pe), and if it holds R pixels it
// offers lo = A.ss and hi = B.pe - 1; lo and hi only ever meet by min and max.  A lane sums up its unit from the bits, the lanes join by a
// butterfly (after step o every lane holds the summary of its aligned group of 2 o lanes), and the row so far joins the step.
// The workgroups also write the "none" values of the column halves, which the column kernel (launched after this one) lowers and raises.
template <typename TI>
__global__ __launch_bounds__(EXT_THREADS) void page_row_extents_kernel(const TI *__restrict__ page, int H, int W, int pitch, float thr, int R,
                                                                       int32_t *__restrict__ out) {
    constexpr int VEC = 16 / (int)sizeof(TI);
    constexpr unsigned int FULL = (1u << VEC) - 1u;
    for (int i = blockIdx.x * EXT_THREADS + threadIdx.x; i < W; i += gridDim.x * EXT_THREADS) out[2 * H + i] = H, out[2 * H + W + i] = -1;
    const int lane = threadIdx.x & 63, y = blockIdx.x * EXT_ROW_WAVES + (threadIdx.x >> 6);
    if (y >= H) return;                                                              // (the whole wave)
    const bool aligned = ((reinterpret_cast<uintptr_t>(page) | ((size_t)pitch * sizeof(TI))) & 15) == 0;
    const int limit = sizeof(TI) == 1 ? ink_limit_u8(thr) : 0;
    const TI *row = page + (size_t)y * pitch;
    int cpe = 0, css = 0, clo = W, chi = -1;                                         // the row so far: [0, xs)
    unsigned int ahead = paper_bits(row + lane * VEC, lane * VEC, W, aligned, thr, limit);
    for (int xs = 0; xs < W; xs += 64 * VEC) {
        const int x = xs + lane * VEC, xn = x + 64 * VEC;
        const unsigned int m = ahead, inv = ~m & FULL;
        ahead = paper_bits(row + xn, xn, W, aligned, thr, limit);                    // the next step's load is on its way during the joins (0 behind W)
        int pe = inv ? x + __builtin_ctz(inv) : x + VEC, ss = inv ? x + 32 - __builtin_clz(inv) : x, lo = W, hi = -1;
        if (R <= VEC) {                                                              // runs inside the unit: w = the starts of R set bits
            unsigned int w = m;
            for (int s = 1; s < R;) {
                const int d = min(s, R - s);
                w &= w >> d, s += d;
            }
            if (w) lo = x + __builtin_ctz(w), hi = x + 31 - __builtin_clz(w) + R - 1;
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int ope = __shfl_xor(pe, o), oss = __shfl_xor(ss, o), olo = __shfl_xor(lo, o), ohi = __shfl_xor(hi, o);
            const bool upper = (lane & o) != 0;
            const int mid = xs + ((lane & ~(2 * o - 1)) + o) * VEC;
            const int ape = upper ? ope : pe, ass = upper ? oss : ss, bpe = upper ? pe : ope, bss = upper ? ss : oss;
            lo = min(lo, olo), hi = max(hi, ohi);
            if (bpe - ass >= R) lo = min(lo, ass), hi = max(hi, bpe - 1);
            pe = ape == mid ? bpe : ape;
            ss = bss == mid ? ass : bss;
        }
        clo = min(clo, lo), chi = max(chi, hi);
        if (pe - css >= R) clo = min(clo, css), chi = max(chi, pe - 1);
        cpe = cpe == xs ? pe : cpe;
        css = ss == xs ? css : ss;
    }
    if (lane == 0) out[y] = clo, out[H + y] = chi;
}

// Columns.  Grid (x tiles, chunks of EXT_COL_ROWS rows).  A workgroup reads its chunk and the R - 1 rows above it (the halo: a run that
// ends in the chunk may have begun there), 32 units of 16 bytes wide, as in the row kernel, and keeps the paper bits in LDS; then a thread
// walks a column down with a run counter.  A window of R paper rows that ENDS in row y is reported by the chunk that owns y, and by no other:
// it lowers col_lo towards y - R + 1 and raises col_hi towards y with one integer atomic min / max per column and chunk.
template <typename TI>
__global__ __launch_bounds__(EXT_THREADS) void page_col_extents_kernel(const TI *__restrict__ page, int H, int W, int pitch, float thr, int R,
                                                                       int32_t *__restrict__ col_lo, int32_t *__restrict__ col_hi) {
    constexpr int VEC = 16 / (int)sizeof(TI), ROWS_PER_STEP = EXT_THREADS / EXT_UNITS;
    __shared__ unsigned short bits[EXT_COL_ROWS + EXT_MAX_RUN - 1][EXT_UNITS];
    const int y0 = blockIdx.y * EXT_COL_ROWS, y1 = min(y0 + EXT_COL_ROWS, H), top = max(y0 - (R - 1), 0), rows = y1 - top;
    const int u0 = blockIdx.x * EXT_UNITS, u = threadIdx.x & (EXT_UNITS - 1), r = threadIdx.x / EXT_UNITS;
    const bool aligned = ((reinterpret_cast<uintptr_t>(page) | ((size_t)pitch * sizeof(TI))) & 15) == 0;
    const int limit = sizeof(TI) == 1 ? ink_limit_u8(thr) : 0;
    const int x = (u0 + u) * VEC;
    int i = r;
    if (aligned && (u0 + EXT_UNITS) * VEC <= W) {                                    // a tile of whole units (the same for the workgroup): four loads in flight per lane
        constexpr int AHEAD = 4;
        for (; i + (AHEAD - 1) * ROWS_PER_STEP < rows; i += AHEAD * ROWS_PER_STEP) {
            uint4 v[AHEAD];
#pragma unroll
            for (int k = 0; k < AHEAD; ++k) v[k] = *reinterpret_cast<const uint4 *>(page + (size_t)(top + i + k * ROWS_PER_STEP) * pitch + x);
#pragma unroll
            for (int k = 0; k < AHEAD; ++k) bits[i + k * ROWS_PER_STEP][u] = (unsigned short)unit_bits<TI>(v[k], thr, limit);
        }
    }
    for (; i < rows; i += ROWS_PER_STEP)
        bits[i][u] = (unsigned short)paper_bits(page + (size_t)(top + i) * pitch + x, x, W, aligned, thr, limit);
    __syncthreads();
    // a thread walks its columns c, c + 256, ... of the tile side by side (uint8: two; fp32: the first 128 threads one each)
    constexpr int COLS = (EXT_UNITS * VEC + EXT_THREADS - 1) / EXT_THREADS;
    int cur[COLS], lo[COLS], hi[COLS];
#pragma unroll
    for (int j = 0; j < COLS; ++j) cur[j] = 0, lo[j] = H, hi[j] = -1;
    const int c0 = threadIdx.x;
    if (c0 < EXT_UNITS * VEC) {
#pragma unroll 4
        for (int i = 0; i < rows; ++i) {
            const int y = top + i;
#pragma unroll
            for (int j = 0; j < COLS; ++j) {
                const int c = c0 + j * EXT_THREADS;
                cur[j] = (bits[i][c / VEC] >> (c % VEC)) & 1 ? cur[j] + 1 : 0;
                if (cur[j] >= R && y >= y0) lo[j] = min(lo[j], y - R + 1), hi[j] = y;
            }
        }
#pragma unroll
        for (int j = 0; j < COLS; ++j) {
            const int xc = u0 * VEC + c0 + j * EXT_THREADS;
            if (xc < W && hi[j] >= 0) atomicMin(col_lo + xc, lo[j]), atomicMax(col_hi + xc, hi[j]);
        }
    }
}

// ---- warp -------------------------------------------------------------------------------------------------------------------------------
constexpr int WARP_THREADS = 256, WARP_LANE_PX = 4;

struct WarpCoef {
    long long c[9];
};

// floor(n / d) for d > 0, exactly.  The quotient is estimated in double: with |estimate| < 2^50 the three roundings (of n, of d - exact below
// 2^53 - and of the division) leave it within 0.4 of n / d, so its floor is off by at most one, and the remainder n - q d, formed modulo
// 2^64, lies in [-d, 2 d) and says which way (d < 2^62: the entry point checks it).  Beyond that the 64-bit division itself.
__device__ __forceinline__ long long floor_div(long long n, long long d) {
    const double e = floor((double)n / (double)d);
    if (fabs(e) < 0x1p50) {
        long long q = (long long)e;
        const long long r = (long long)((unsigned long long)n - (unsigned long long)q * (unsigned long long)d);
        if (r < 0) --q;
        else if (r >= d) ++q;
        return q;
    }
    const long long q = n / d;
    return n % d < 0 ? q - 1 : q;
}

template <typename TI>
__device__ __forceinline__ TI warp_tap(const TI *__restrict__ page, int H, int W, int pitch, int iy, int ix, TI fill) {
    return (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W ? page[(size_t)iy * pitch + ix] : fill;
}

// Grid (x tiles, output rows).  A lane makes 4 consecutive pixels of one output row: the three linear forms at the first, stepped by A, D
// and G from one pixel to the next; two exact floor divisions per pixel; the taps and the blend are page_rotate_kernel's.  An integer
// coordinate beyond the page by more than a pixel is pulled to two pixels outside before it is narrowed to 32 bits: all four taps read
// `fill` either way.  The 4 results leave as one word where the output row starts on such a boundary, one by one where not.
template <typename TI>
__global__ __launch_bounds__(WARP_THREADS) void page_warp_kernel(const TI *__restrict__ page, int H, int W, int pitch, WarpCoef k, TI fill, TI *__restrict__ out,
                                                                 int OW, int out_pitch) {
    const int x0 = (blockIdx.x * WARP_THREADS + threadIdx.x) * WARP_LANE_PX, y = blockIdx.y;
    if (x0 >= OW) return;
    // (the forms are summed modulo 2^64: the entry point bounds their values inside the output, not every product on the way there)
    auto form = [&](int f) { return (unsigned long long)k.c[3 * f] * (unsigned long long)x0 + (unsigned long long)k.c[3 * f + 1] * (unsigned long long)y + (unsigned long long)k.c[3 * f + 2]; };
    unsigned long long nx = form(0), ny = form(1), den = form(2);
    TI res[WARP_LANE_PX];
#pragma unroll
    for (int j = 0; j < WARP_LANE_PX; ++j, nx += (unsigned long long)k.c[0], ny += (unsigned long long)k.c[3], den += (unsigned long long)k.c[6]) {
        res[j] = fill;
        if (x0 + j >= OW) continue;                                                  // (behind the row the forms are not checked)
        const long long sxq = floor_div((long long)nx * 256, (long long)den), syq = floor_div((long long)ny * 256, (long long)den);
        const int ix = (int)min(max(sxq >> 8, -2ll), (long long)W + 1), iy = (int)min(max(syq >> 8, -2ll), (long long)H + 1);
        const int fx = (int)(sxq & 255), fy = (int)(syq & 255);
        const TI t00 = warp_tap(page, H, W, pitch, iy, ix, fill), t01 = warp_tap(page, H, W, pitch, iy, ix + 1, fill);
        const TI t10 = warp_tap(page, H, W, pitch, iy + 1, ix, fill), t11 = warp_tap(page, H, W, pitch, iy + 1, ix + 1, fill);
        if constexpr (sizeof(TI) == 1) {
            const int top = (256 - fx) * t00 + fx * t01, bot = (256 - fx) * t10 + fx * t11;
            res[j] = (unsigned char)(((256 - fy) * top + fy * bot + 32768) >> 16);
        } else {
            const float wx = (float)fx * (1.0f / 256.0f), wy = (float)fy * (1.0f / 256.0f);
            const float top = (1.0f - wx) * t00 + wx * t01, bot = (1.0f - wx) * t10 + wx * t11;
            res[j] = (1.0f - wy) * top + wy * bot;
        }
    }
    TI *dst = out + (size_t)y * out_pitch + x0;
    constexpr size_t WORD = sizeof(TI) * WARP_LANE_PX;
    const bool whole = ((reinterpret_cast<uintptr_t>(out) | ((size_t)out_pitch * sizeof(TI))) & (WORD - 1)) == 0 && x0 + WARP_LANE_PX <= OW;
    if (whole) {
        if constexpr (sizeof(TI) == 1) *reinterpret_cast<uchar4 *>(dst) = make_uchar4(res[0], res[1], res[2], res[3]);
        else *reinterpret_cast<float4 *>(dst) = make_float4(res[0], res[1], res[2], res[3]);
    } else {
#pragma unroll
        for (int j = 0; j < WARP_LANE_PX; ++j)
            if (x0 + j < OW) dst[j] = res[j];
    }
}

}  // namespace

#define ACAI_RECTIFY_PAGE_CHECK(name)                                                                                                           \
    ACAI_CHECK_ARG(page, name ": null page");                                                                                                    \
    ACAI_CHECK_ARG(H > 0 && W > 0 && H <= ACAI_PAGE_MAX_H && W <= ACAI_PAGE_MAX_W && pitch >= W, name ": bad page %d x %d, pitch %d (H <= %d, W <= %d)", H, W, \
                   pitch, ACAI_PAGE_MAX_H, ACAI_PAGE_MAX_W)

extern "C" int acai_page_extents(const void *page, int in_u8, int H, int W, int pitch, float paper_threshold, int min_run, int32_t *out, void *stream) {
    ACAI_RECTIFY_PAGE_CHECK("acai_page_extents");
    ACAI_CHECK_ARG(min_run >= 1 && min_run <= EXT_MAX_RUN, "acai_page_extents: min_run %d (1 .. %d)", min_run, EXT_MAX_RUN);
    ACAI_CHECK_ARG(out, "acai_page_extents: null output");
    hipStream_t st = (hipStream_t)stream;
    const dim3 rows(cdiv(H, EXT_ROW_WAVES)), cols(cdiv(cdiv(W, in_u8 ? 16 : 4), EXT_UNITS), cdiv(H, EXT_COL_ROWS));
    int32_t *col_lo = out + 2 * (size_t)H, *col_hi = col_lo + W;
    if (in_u8) {
        const unsigned char *p = reinterpret_cast<const unsigned char *>(page);
        hipLaunchKernelGGL(page_row_extents_kernel<unsigned char>, rows, dim3(EXT_THREADS), 0, st, p, H, W, pitch, paper_threshold, min_run, out);
        hipLaunchKernelGGL(page_col_extents_kernel<unsigned char>, cols, dim3(EXT_THREADS), 0, st, p, H, W, pitch, paper_threshold, min_run, col_lo, col_hi);
    } else {
        const float *p = reinterpret_cast<const float *>(page);
        hipLaunchKernelGGL(page_row_extents_kernel<float>, rows, dim3(EXT_THREADS), 0, st, p, H, W, pitch, paper_threshold, min_run, out);
        hipLaunchKernelGGL(page_col_extents_kernel<float>, cols, dim3(EXT_THREADS), 0, st, p, H, W, pitch, paper_threshold, min_run, col_lo, col_hi);
    }
    ACAI_LAUNCH_CHECK("acai_page_extents");
    return 0;
}

extern "C" int acai_page_warp(const void *page, int in_u8, int H, int W, int pitch, const int64_t coef[9], float fill, void *out, int OH, int OW, int out_pitch,
                              void *stream) {
    ACAI_RECTIFY_PAGE_CHECK("acai_page_warp");
    ACAI_CHECK_ARG(coef, "acai_page_warp: null coefficients");
    ACAI_CHECK_ARG(OH > 0 && OW > 0 && OH <= ACAI_PAGE_MAX_H && OW <= ACAI_PAGE_MAX_W && out_pitch >= OW, "acai_page_warp: bad output %d x %d, pitch %d (OH <= %d, OW <= %d)",
                   OH, OW, out_pitch, ACAI_PAGE_MAX_H, ACAI_PAGE_MAX_W);
    ACAI_CHECK_ARG(out && out != page, "acai_page_warp: bad output (null, or in place)");
    ACAI_CHECK_ARG(!in_u8 || (fill >= 0.f && fill <= 255.f && fill == (float)(int)fill), "acai_page_warp: fill = %g of a uint8 page is an integer in 0 .. 255",
                   (double)fill);
    // the three forms are linear: inside the output rectangle each lies between its values at the four corners
    const __int128 lim = (__int128)1 << 62;
    const int cx[4] = {0, OW - 1, OW - 1, 0}, cy[4] = {0, 0, OH - 1, OH - 1};
    for (int i = 0; i < 4; ++i) {
        __int128 v[3];
        for (int f = 0; f < 3; ++f) v[f] = (__int128)coef[3 * f] * cx[i] + (__int128)coef[3 * f + 1] * cy[i] + (__int128)coef[3 * f + 2];
        ACAI_CHECK_ARG(v[2] > 0 && v[2] < lim, "acai_page_warp: the denominator at output corner (%d, %d) is not in 1 .. 2^62 - 1", cx[i], cy[i]);
        for (int f = 0; f < 2; ++f)
            ACAI_CHECK_ARG((v[f] < 0 ? -v[f] : v[f]) * 256 < lim, "acai_page_warp: |%s numerator| * 256 at output corner (%d, %d) reaches 2^62", f ? "y" : "x", cx[i], cy[i]);
    }
    WarpCoef k;
    for (int i = 0; i < 9; ++i) k.c[i] = coef[i];
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(cdiv(cdiv(OW, WARP_LANE_PX), WARP_THREADS), OH);
    if (in_u8)
        hipLaunchKernelGGL(page_warp_kernel<unsigned char>, grid, dim3(WARP_THREADS), 0, st, reinterpret_cast<const unsigned char *>(page), H, W, pitch, k,
                           (unsigned char)fill, reinterpret_cast<unsigned char *>(out), OW, out_pitch);
    else
        hipLaunchKernelGGL(page_warp_kernel<float>, grid, dim3(WARP_THREADS), 0, st, reinterpret_cast<const float *>(page), H, W, pitch, k, fill,
                           reinterpret_cast<float *>(out), OW, out_pitch);
    ACAI_LAUNCH_CHECK("acai_page_warp");
    return 0;
}
