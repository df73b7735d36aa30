// Page deskew (an extension; the reference's service takes "phone captured JPEGs" and has a person draw the boxes, acai_omr/ui/routes.py):
//   acai_page_strips       per row and vertical strip of S columns, the number of ink pixels (the page is read once),
//   acai_page_skew_scores  for every candidate slope, the strip profile sheared along it and summed over the strips, scored by the energy
//                          of its row-to-row differences: level staff lines make the sharpest row profile,
//   acai_page_rotate       the page turned about its centre, bilinear, with Q16 source coordinates.
// Every result is defined in integers (the fp32 rotation aside), so none depends on how the launches are scheduled: the one atomic sum is a
// 64-bit integer one.
#include "common.h"
#include "resize_taps.h"

namespace {

// ---- strips -----------------------------------------------------------------------------------------------------------------------------
constexpr int STRIP_ROWS = ACAI_STRIP_TILE_ROWS, STRIP_UNITS = ACAI_STRIP_TILE_UNITS, STRIP_THREADS = 256;
constexpr int STRIP_MAX_TILE_STRIPS = STRIP_UNITS * 16 / 8;   // a uint8 tile is 512 pixels wide: 64 strips of 8

// The ink test in the element's own domain (page.hip does the same for its wide loads): a uint8 value v is ink iff (float)v / 255 < thr,
// which is monotone in v, so iff v < the first value that is not; found by bisection with the very comparison the per-element path makes.
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

// A unit is 16 bytes of a row: 16 uint8 pixels or 4 fp32 ones.  A workgroup owns a tile of 64 rows x 32 units (512 bytes of each row) and
// walks it in 8 steps; in a step a wave reads 2 rows x 512 contiguous bytes, one unit per lane.  A unit that lies inside the row and on a
// 16-byte boundary (base and pitch allow it) is one load; the units across W, and every unit of a page that is not aligned, go element by
// element, and elements behind W never count.  A strip is a whole number of units (their counts meet by xor shuffles over the lanes of the
// strip, which never straddle a tile) or, for S = 8 on uint8, half a unit.  The tile's counts are turned through LDS so that the stores
// run along y, the contiguous direction of P [nS][H].
template <typename TI>
__global__ __launch_bounds__(STRIP_THREADS) void page_strips_kernel(const TI *__restrict__ page, int H, int W, int pitch, float thr, int S, int nS,
                                                                    unsigned char *__restrict__ P) {
    constexpr int VEC = 16 / (int)sizeof(TI);
    __shared__ int cnt[STRIP_MAX_TILE_STRIPS][STRIP_ROWS + 1];   // (+ 1: a wave's stores of one step hit 32 strips x 2 rows)
    const int y0 = blockIdx.y * STRIP_ROWS, u0 = blockIdx.x * STRIP_UNITS;
    const int u = threadIdx.x & (STRIP_UNITS - 1), r = threadIdx.x / STRIP_UNITS;
    const bool aligned = ((reinterpret_cast<uintptr_t>(page) | ((size_t)pitch * sizeof(TI))) & 15) == 0;
    const int limit = sizeof(TI) == 1 ? ink_limit_u8(thr) : 0;
    const int x = (u0 + u) * VEC;
    const int ups = S >= VEC ? S / VEC : 1;                      // units per strip
#pragma unroll
    for (int i = 0; i < STRIP_ROWS / (STRIP_THREADS / STRIP_UNITS); ++i) {
        const int ry = r + i * (STRIP_THREADS / STRIP_UNITS), y = y0 + ry;
        int lo = 0, hi = 0;                                      // ink in the first and in the second half of the unit
        if (y < H && x < W) {
            const TI *src = page + (size_t)y * pitch + x;
            if (aligned && x + VEC <= W) {
                const uint4 v = *reinterpret_cast<const uint4 *>(src);
                const unsigned int word[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    bool on;
                    if constexpr (sizeof(TI) == 1) on = (int)((word[k >> 2] >> (8 * (k & 3))) & 255u) < limit;
                    else on = __uint_as_float(word[k]) < thr;
                    if (k < VEC / 2) lo += on;
                    else hi += on;
                }
            } else {
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const bool on = x + k < W && in_sample(src + k) < thr;
                    if (k < VEC / 2) lo += on;
                    else hi += on;
                }
            }
        }
        if (S < VEC) {                                           // uint8, S = 8: two strips per unit
            cnt[2 * u][ry] = lo, cnt[2 * u + 1][ry] = hi;
        } else {
            int c = lo + hi;
            for (int o = 1; o < ups; o <<= 1) c += __shfl_xor(c, o);
            if ((u & (ups - 1)) == 0) cnt[u / ups][ry] = c;
        }
    }
    __syncthreads();
    const int tile_strips = STRIP_UNITS * VEC / S, s0 = (int)((long long)u0 * VEC / S);
    for (int i = threadIdx.x; i < tile_strips * STRIP_ROWS; i += STRIP_THREADS) {
        const int ry = i & (STRIP_ROWS - 1), s = i / STRIP_ROWS;
        if (y0 + ry < H && s0 + s < nS) P[(size_t)(s0 + s) * H + y0 + ry] = (unsigned char)cnt[s][ry];
    }
}

// ---- skew scores ------------------------------------------------------------------------------------------------------------------------
constexpr int SKEW_ROW_THREADS = 256, SKEW_LANE_ROWS = 4, SKEW_SPLIT = 4, SKEW_THREADS = SKEW_ROW_THREADS * SKEW_SPLIT, SKEW_CHUNK = ACAI_SKEW_CHUNK;
static_assert(SKEW_CHUNK == SKEW_ROW_THREADS * SKEW_LANE_ROWS - 1, "a chunk is the rows of one workgroup less the one-row halo");

// Grid (slope k, chunk c).  The workgroup forms Q_k for the 1024 rows from c * 1023 on - the last one is the halo, the first row of the next
// chunk - and sums the squares of the 1023 differences between them (those with y + 1 < H).  Its 1024 threads are 4 groups of 256: thread t
// of every group owns the 4 consecutive rows from 4 t on, and group g adds up the strips s = g, g + 4, ... (the loop is bound by the
// latency of its loads: four groups put four times the loads in flight).  Per strip a thread reads its 4 counts with one load (P is
// [nS][H]: consecutive rows are consecutive bytes; the sheared start is on no boundary) and adds them into two registers of two 16-bit sums
// each (Q <= W <= 16384), or byte by byte where the 4 rows cross the top or the bottom of the page, outside of which P counts as 0.  The
// offsets depend on (s, k) only: scalar arithmetic.  P is read through L2 (all of it is 0.5 MB for an A4 page; the rows a chunk needs of a
// strip shift by up to tan(15 deg) W / 2 over the strips, more than a chunk for such a page, so a staged slice would be most of P again).
// The groups' sums meet in LDS; group 0 squares the differences; thread sums -> wave (shuffles) -> workgroup (LDS) -> ONE 64-bit integer
// atomic add per workgroup into scores[k], zeroed before the launch: integer addition commutes, so the result is the same in any order.
__global__ __launch_bounds__(SKEW_THREADS) void page_skew_scores_kernel(const unsigned char *__restrict__ P, int H, int W, int S, int nS,
                                                                        const int32_t *__restrict__ slopes, unsigned long long *__restrict__ scores) {
    __shared__ unsigned int even_s[SKEW_SPLIT][SKEW_ROW_THREADS], odd_s[SKEW_SPLIT][SKEW_ROW_THREADS];
    __shared__ int first[SKEW_ROW_THREADS];
    __shared__ unsigned long long part[SKEW_THREADS / 64];
    const int k = blockIdx.x, m = slopes[k];
    const int t = threadIdx.x & (SKEW_ROW_THREADS - 1), g = threadIdx.x / SKEW_ROW_THREADS;
    const int r = blockIdx.y * SKEW_CHUNK + t * SKEW_LANE_ROWS;                     // this thread's first row
    unsigned int even = 0, odd = 0;                                                 // rows r, r + 2 | rows r + 1, r + 3
    auto offset = [&](int s) { return (m * (s * S + S / 2 - W / 2) + 32768) >> 16; };   // |m dx| < 2^15 2^15: no overflow
    // off is monotone in s: a thread whose 4 rows stay inside the page at both ends of the strip range (most threads, at small slopes all
    // but those of the first and last rows) loads without a test, several strips in flight
    const int off_a = offset(0), off_b = offset(nS - 1);
    if (r + min(off_a, off_b) >= 0 && r + max(off_a, off_b) + SKEW_LANE_ROWS <= H) {
#pragma unroll 8
        for (int s = g; s < nS; s += SKEW_SPLIT) {
            unsigned int w;
            __builtin_memcpy(&w, P + (size_t)s * H + (r + offset(s)), 4);
            even += w & 0x00ff00ffu;
            odd += (w >> 8) & 0x00ff00ffu;
        }
    } else if (r < H) {
        for (int s = g; s < nS; s += SKEW_SPLIT) {
            const int q = r + offset(s);
            const unsigned char *col = P + (size_t)s * H;
            unsigned int w = 0;
            if (q >= 0 && q + SKEW_LANE_ROWS <= H) {
                __builtin_memcpy(&w, col + q, 4);
            } else if (q > -SKEW_LANE_ROWS && q < H) {
#pragma unroll
                for (int j = 0; j < SKEW_LANE_ROWS; ++j)
                    if (q + j >= 0 && q + j < H) w |= (unsigned int)col[q + j] << (8 * j);
            }
            even += w & 0x00ff00ffu;
            odd += (w >> 8) & 0x00ff00ffu;
        }
    }
    even_s[g][t] = even, odd_s[g][t] = odd;
    __syncthreads();
    unsigned long long sum = 0;
    int Q[SKEW_LANE_ROWS] = {0, 0, 0, 0};
    if (g == 0) {
#pragma unroll
        for (int o = 1; o < SKEW_SPLIT; ++o) even += even_s[o][t], odd += odd_s[o][t];
        Q[0] = (int)(even & 0xffffu), Q[1] = (int)(odd & 0xffffu), Q[2] = (int)(even >> 16), Q[3] = (int)(odd >> 16);
        first[t] = Q[0];
    }
    __syncthreads();
    if (g == 0) {
#pragma unroll
        for (int j = 0; j < SKEW_LANE_ROWS; ++j) {
            const bool last = j == SKEW_LANE_ROWS - 1;
            if (last && t == SKEW_ROW_THREADS - 1) break;                           // the halo row starts no difference of this chunk
            if (r + j + 1 < H) {
                const long long d = (last ? first[t + 1] : Q[j + 1]) - Q[j];
                sum += (unsigned long long)(d * d);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = part[0];
        for (int w = 1; w < SKEW_ROW_THREADS / 64; ++w) total += part[w];           // (the waves of group 0)
        if (total) atomicAdd(scores + k, total);
    }
}

// ---- rotate -----------------------------------------------------------------------------------------------------------------------------
constexpr int ROT_THREADS = 256, ROT_LANE_PX = 4;

template <typename TI>
__device__ __forceinline__ TI tap(const TI *__restrict__ page, int H, int W, int pitch, int iy, int ix, TI fill) {
    return (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W ? page[(size_t)iy * pitch + ix] : fill;
}

// Grid (x tiles, rows).  A lane makes 4 consecutive pixels of one output row: the source coordinates of the first in 64-bit integers as the
// header defines them, and from one pixel to the next sx grows by exactly cos_q and sy by sin_q (the sum under the shift grows by an even
// number).  The 4 results leave as one word - 4 bytes, or 16 for fp32 - where the output row starts on such a boundary, one by one where it
// does not or the row ends inside the word.
template <typename TI>
__global__ __launch_bounds__(ROT_THREADS) void page_rotate_kernel(const TI *__restrict__ page, int H, int W, int pitch, int cos_q, int sin_q, TI fill,
                                                                  TI *__restrict__ out, int out_pitch) {
    const int x0 = (blockIdx.x * ROT_THREADS + threadIdx.x) * ROT_LANE_PX, y = blockIdx.y;
    if (x0 >= W) return;
    const long long dx2 = 2ll * x0 - (W - 1), dy2 = 2ll * y - (H - 1);
    long long sx = ((long long)cos_q * dx2 - (long long)sin_q * dy2 + (long long)(W - 1) * 65536) >> 1;
    long long sy = ((long long)sin_q * dx2 + (long long)cos_q * dy2 + (long long)(H - 1) * 65536) >> 1;
    TI res[ROT_LANE_PX];
#pragma unroll
    for (int j = 0; j < ROT_LANE_PX; ++j, sx += cos_q, sy += sin_q) {
        const int ix = (int)(sx >> 16), iy = (int)(sy >> 16), fx = (int)(sx >> 8) & 255, fy = (int)(sy >> 8) & 255;
        const TI t00 = tap(page, H, W, pitch, iy, ix, fill), t01 = tap(page, H, W, pitch, iy, ix + 1, fill);
        const TI t10 = tap(page, H, W, pitch, iy + 1, ix, fill), t11 = tap(page, H, W, pitch, iy + 1, ix + 1, fill);
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
    constexpr size_t WORD = sizeof(TI) * ROT_LANE_PX;
    const bool whole = ((reinterpret_cast<uintptr_t>(out) | ((size_t)out_pitch * sizeof(TI))) & (WORD - 1)) == 0 && x0 + ROT_LANE_PX <= W;
    if (whole) {
        if constexpr (sizeof(TI) == 1) *reinterpret_cast<uchar4 *>(dst) = make_uchar4(res[0], res[1], res[2], res[3]);
        else *reinterpret_cast<float4 *>(dst) = make_float4(res[0], res[1], res[2], res[3]);
    } else {
#pragma unroll
        for (int j = 0; j < ROT_LANE_PX; ++j)
            if (x0 + j < W) dst[j] = res[j];
    }
}

}  // namespace

#define ACAI_DESKEW_PAGE_CHECK(name)                                                                                                            \
    ACAI_CHECK_ARG(page, name ": null page");                                                                                                    \
    ACAI_CHECK_ARG(H > 0 && W > 0 && H <= ACAI_PAGE_MAX_H && W <= ACAI_PAGE_MAX_W && pitch >= W, name ": bad page %d x %d, pitch %d (H <= %d, W <= %d)", H, W, \
                   pitch, ACAI_PAGE_MAX_H, ACAI_PAGE_MAX_W)
#define ACAI_STRIP_CHECK(name) ACAI_CHECK_ARG(S == 8 || S == 16 || S == 32 || S == 64, name ": strip width %d is not 8, 16, 32 or 64", S)

extern "C" int acai_page_strips(const void *page, int in_u8, int H, int W, int pitch, float ink_threshold, int S, uint8_t *strips, void *stream) {
    ACAI_DESKEW_PAGE_CHECK("acai_page_strips");
    ACAI_STRIP_CHECK("acai_page_strips");
    ACAI_CHECK_ARG(strips, "acai_page_strips: null output");
    hipStream_t st = (hipStream_t)stream;
    const int nS = cdiv(W, S), units = cdiv(W, in_u8 ? 16 : 4);
    const dim3 grid(cdiv(units, STRIP_UNITS), cdiv(H, STRIP_ROWS));
    if (in_u8)
        hipLaunchKernelGGL(page_strips_kernel<unsigned char>, grid, dim3(STRIP_THREADS), 0, st, reinterpret_cast<const unsigned char *>(page), H, W, pitch,
                           ink_threshold, S, nS, strips);
    else
        hipLaunchKernelGGL(page_strips_kernel<float>, grid, dim3(STRIP_THREADS), 0, st, reinterpret_cast<const float *>(page), H, W, pitch, ink_threshold, S,
                           nS, strips);
    ACAI_LAUNCH_CHECK("acai_page_strips");
    return 0;
}

extern "C" int acai_page_skew_scores(const uint8_t *strips, int H, int W, int S, const int32_t *slopes, const int32_t *host_slopes, int K, int64_t *scores,
                                     void *stream) {
    ACAI_CHECK_ARG(strips && slopes && host_slopes && scores, "acai_page_skew_scores: null operand");
    ACAI_CHECK_ARG(H > 0 && W > 0 && H <= ACAI_PAGE_MAX_H && W <= ACAI_PAGE_MAX_W, "acai_page_skew_scores: bad page %d x %d (H <= %d, W <= %d)", H, W,
                   ACAI_PAGE_MAX_H, ACAI_PAGE_MAX_W);
    ACAI_STRIP_CHECK("acai_page_skew_scores");
    ACAI_CHECK_ARG(K >= 1 && K <= ACAI_SKEW_MAX_SLOPES, "acai_page_skew_scores: %d slopes (1 .. %d)", K, ACAI_SKEW_MAX_SLOPES);
    for (int k = 0; k < K; ++k)
        ACAI_CHECK_ARG(host_slopes[k] >= -ACAI_SKEW_MAX_SLOPE && host_slopes[k] <= ACAI_SKEW_MAX_SLOPE, "acai_page_skew_scores: slope %d = %d beyond +-%d (tan 15 deg in Q16)",
                       k, host_slopes[k], ACAI_SKEW_MAX_SLOPE);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(scores, 0, (size_t)K * sizeof(int64_t), st);
    if (e != hipSuccess) return acai_set_err((int)e, "acai_page_skew_scores (zeroing): %s", hipGetErrorString(e));
    const int chunks = H > 1 ? cdiv(H - 1, SKEW_CHUNK) : 1;
    hipLaunchKernelGGL(page_skew_scores_kernel, dim3(K, chunks), dim3(SKEW_THREADS), 0, st, strips, H, W, S, cdiv(W, S), slopes,
                       reinterpret_cast<unsigned long long *>(scores));
    ACAI_LAUNCH_CHECK("acai_page_skew_scores");
    return 0;
}

extern "C" int acai_page_rotate(const void *page, int in_u8, int H, int W, int pitch, int cos_q, int sin_q, float fill, void *out, int out_pitch,
                                void *stream) {
    ACAI_DESKEW_PAGE_CHECK("acai_page_rotate");
    ACAI_CHECK_ARG(out && out_pitch >= W && out != page, "acai_page_rotate: bad output (pitch %d, not in place)", out_pitch);
    ACAI_CHECK_ARG(cos_q >= -65536 && cos_q <= 65536 && sin_q >= -65536 && sin_q <= 65536, "acai_page_rotate: cos_q = %d, sin_q = %d are Q16 (|.| <= 65536)", cos_q,
                   sin_q);
    ACAI_CHECK_ARG(!in_u8 || (fill >= 0.f && fill <= 255.f && fill == (float)(int)fill), "acai_page_rotate: fill = %g of a uint8 page is an integer in 0 .. 255",
                   (double)fill);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(cdiv(cdiv(W, ROT_LANE_PX), ROT_THREADS), H);
    if (in_u8)
        hipLaunchKernelGGL(page_rotate_kernel<unsigned char>, grid, dim3(ROT_THREADS), 0, st, reinterpret_cast<const unsigned char *>(page), H, W, pitch, cos_q,
                           sin_q, (unsigned char)fill, reinterpret_cast<unsigned char *>(out), out_pitch);
    else
        hipLaunchKernelGGL(page_rotate_kernel<float>, grid, dim3(ROT_THREADS), 0, st, reinterpret_cast<const float *>(page), H, W, pitch, cos_q, sin_q, fill,
                           reinterpret_cast<float *>(out), out_pitch);
    ACAI_LAUNCH_CHECK("acai_page_rotate");
    return 0;
}
