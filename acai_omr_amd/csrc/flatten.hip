// Page illumination flattening (an extension; the reference's service takes "phone captured JPEGs", acai_omr/ui/routes.py, and every page
// stage here tells ink from paper by ONE global threshold):
//   acai_page_tile_levels  per tile of T x T pixels, the rank-th smallest level of its pixels (the paper, at the default median),
//   acai_page_flatten      that grid smoothed (a mostly-ink tile takes its brightest neighbour, everything is floored), interpolated
//                          bilinearly between the tile centres and divided out of every pixel.
// Every step is defined in integers (include/acai_omr_hip.h); the fp32 output is one correctly rounded multiply.  The only atomics are
// integer adds in LDS, whose sums do not depend on their order.
#include "common.h"

namespace {

// A unit is 16 bytes of a row: 16 uint8 pixels or 4 fp32 ones.  A unit that lies inside the row and on a 16-byte boundary (base and pitch
// allow it) is one load; the units across W, and every unit of a view that is not aligned, go element by element, and nothing behind W is
// read (deskew.hip's acai_page_strips reads the same way).
template <typename TI>
__device__ __forceinline__ bool rows_aligned(const TI *base, int pitch) {
    return ((reinterpret_cast<uintptr_t>(base) | ((size_t)pitch * sizeof(TI))) & 15) == 0;
}

__device__ __forceinline__ int level_of(unsigned char v) { return v; }
// (the product and the sum are rounded one after the other: contracted into an FMA they would be rounded once, which numpy cannot restate)
__device__ __forceinline__ int level_of(float v) { return (int)fminf(fmaxf(floorf(__fadd_rn(__fmul_rn(v, 255.0f), 0.5f)), 0.0f), 255.0f); }

// The n <= VEC pixels of the unit at src -> px[]; returns n.
template <typename TI, int VEC>
__device__ __forceinline__ int load_unit(const TI *__restrict__ src, int x, int W, bool aligned, TI (&px)[VEC]) {
    if (aligned && x + VEC <= W) {
        const uint4 v = *reinterpret_cast<const uint4 *>(src);
        __builtin_memcpy(px, &v, 16);
        return VEC;
    }
    const int n = min(VEC, W - x);
#pragma unroll
    for (int k = 0; k < VEC; ++k) px[k] = k < n ? src[k] : TI(0);
    return n;
}

// ---- tile levels ------------------------------------------------------------------------------------------------------------------------
constexpr int LV_THREADS = 256, LV_WAVES = LV_THREADS / 64;

// A wave owns one tile and one 256-bin histogram in LDS; a workgroup is 4 such waves on 4 consecutive tiles (of one tile row mostly, so its
// loads of a pixel row are neighbours).  The wave's lanes cover the tile T / VEC units across and 64 / (T / VEC) rows down per step.  A
// lane adds its unit to the histogram run by run - one LDS atomic per run of equal levels, so flat paper costs one add per unit and not
// sixteen on one address.  Then lane l sums bins 4 l .. 4 l + 3, the sums are scanned over the wave by shuffles, and the first lane whose
// inclusive sum reaches the rank walks its four bins.
template <typename TI>
__global__ __launch_bounds__(LV_THREADS) void page_tile_levels_kernel(const TI *__restrict__ page, int H, int W, int pitch, int lt, int percent, int GW, int tiles,
                                                                      unsigned char *__restrict__ g) {
    constexpr int VEC = 16 / (int)sizeof(TI);
    __shared__ __attribute__((aligned(16))) unsigned int hist[LV_WAVES][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = blockIdx.x * LV_WAVES + wave, T = 1 << lt;
    const bool live = t < tiles;
    unsigned int *h = hist[wave];
    *reinterpret_cast<uint4 *>(h + 4 * lane) = make_uint4(0, 0, 0, 0);
    __syncthreads();
    int n = 0;
    if (live) {
        const int ti = t / GW, tj = t - ti * GW, y0 = ti << lt, x0 = tj << lt;
        const int th = min(T, H - y0), tw = min(T, W - x0), upr = T / VEC;
        n = th * tw;
        const int x = x0 + (lane & (upr - 1)) * VEC;
        const bool aligned = rows_aligned(page, pitch);
        if (x < W) {
            // four steps' loads are issued before the first of them is counted (T = 64, uint8: the whole tile): the adds wait on LDS, and
            // one 16-byte load in flight per lane would leave the wave waiting on memory in between
            constexpr int AHEAD = 4;
            const int rps = 64 / upr;
            for (int base = lane / upr; base < th; base += AHEAD * rps) {
                TI px[AHEAD][VEC];
                int nv[AHEAD];
#pragma unroll
                for (int j = 0; j < AHEAD; ++j) {
                    const int ry = base + j * rps;
                    nv[j] = ry < th ? load_unit<TI, VEC>(page + (size_t)(y0 + ry) * pitch + x, x, W, aligned, px[j]) : 0;
                }
#pragma unroll
                for (int j = 0; j < AHEAD; ++j) {
                    if (nv[j] == 0) continue;
                    int cur = level_of(px[j][0]), cnt = 1;
#pragma unroll
                    for (int k = 1; k < VEC; ++k) {
                        if (k < nv[j]) {
                            const int l = level_of(px[j][k]);
                            if (l == cur) {
                                ++cnt;
                            } else {
                                atomicAdd(h + cur, (unsigned int)cnt);
                                cur = l, cnt = 1;
                            }
                        }
                    }
                    atomicAdd(h + cur, (unsigned int)cnt);
                }
            }
        }
    }
    __syncthreads();
    if (!live) return;
    const int rank = max(1, (n * percent + 99) / 100);                   // n <= 2^14: no overflow
    const uint4 c = *reinterpret_cast<const uint4 *>(h + 4 * lane);
    const int own = (int)(c.x + c.y + c.z + c.w);
    int incl = own;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    const unsigned long long reached = __ballot(incl >= rank);           // never empty: lane 63 holds n >= rank
    if (lane == __ffsll((long long)reached) - 1) {
        const int need = rank - (incl - own);                            // in 1 .. own
        int L = 4 * lane, a = (int)c.x;
        if (a < need) {
            a += (int)c.y, ++L;
            if (a < need) {
                a += (int)c.z, ++L;
                if (a < need) ++L;
            }
        }
        g[t] = (unsigned char)L;
    }
}

// ---- flatten ----------------------------------------------------------------------------------------------------------------------------
constexpr int FL_THREADS = 256, FL_UNITS = 32, FL_ROWS = 16;            // a workgroup: 16 pixel rows (inside one tile row) x 32 units
constexpr int FL_MAX_COLS = FL_UNITS * 16 / 16 + 2;                     // grid columns a stretch of 512 uint8 pixels can touch at T = 16

// Grid (stretch of 32 units, chunk of 16 rows).  The 16 rows lie in tile row i = y / T, so their pixels interpolate between rows i - 1, i
// and i + 1 of the smoothed grid s, and s needs the raw grid one further out: the workgroup stages raw rows i - 2 .. i + 2 of the columns
// its stretch touches (one more on either side; 0 outside the grid, the identity of the maximum), forms the three rows of s at the CLAMPED
// indices next to them, and builds the reciprocal table, all in LDS.  A lane owns one unit of two rows: within 8 pixels (half a uint8
// unit; tile centres are multiples of 8) the four grid taps are the same, so it interpolates down the two columns once and along x per
// pixel - the same integers as the header's formula, which is exact - and each pixel costs one table read and one multiply.
template <typename TI>
__global__ __launch_bounds__(FL_THREADS) void page_flatten_kernel(const TI *__restrict__ page, int H, int W, int pitch, const unsigned char *__restrict__ g, int GH,
                                                                  int GW, int lt, int rq, int floor_level, TI *__restrict__ out, int out_pitch) {
    constexpr int VEC = 16 / (int)sizeof(TI), HV = VEC < 8 ? VEC : 8;
    __shared__ unsigned char raw[5][FL_MAX_COLS + 2];
    __shared__ unsigned char s[3][FL_MAX_COLS];
    __shared__ unsigned int recip[256];
    const int T = 1 << lt, D = 2 * T, tid = threadIdx.x;
    const int ya = blockIdx.y * FL_ROWS, i = ya >> lt;
    const int c0 = blockIdx.x * FL_UNITS * VEC, c1 = min(c0 + FL_UNITS * VEC, W);
    const int jb0 = (2 * c0 + 1 - T) >> (lt + 1);                        // first grid column of the stretch, -1 left of the first centre
    const int nb = ((2 * (c1 - 1) + 1 - T) >> (lt + 1)) + 2 - jb0;       // <= FL_MAX_COLS
    // this lane's unit of rows r0 and r0 + 8: loaded first, so that the page is on its way while the grid is staged
    const int x = c0 + (tid & (FL_UNITS - 1)) * VEC, r0 = ya + tid / FL_UNITS, yb = min(ya + FL_ROWS, H);
    constexpr int LANE_ROWS = FL_ROWS / (FL_THREADS / FL_UNITS);
    const bool in_aligned = rows_aligned(page, pitch), out_aligned = rows_aligned(out, out_pitch);
    TI px[LANE_ROWS][VEC];
    int nv[LANE_ROWS];
#pragma unroll
    for (int j = 0; j < LANE_ROWS; ++j) {
        const int y = r0 + j * (FL_THREADS / FL_UNITS);
        nv[j] = x < W && y < yb ? load_unit<TI, VEC>(page + (size_t)y * pitch + x, x, W, in_aligned, px[j]) : 0;
    }
    recip[tid] = tid ? (255u * 65536u + (unsigned)tid / 2u) / (unsigned)tid : 0u;   // (an exact integer division, once per thread)
    for (int e = tid; e < 5 * (nb + 2); e += FL_THREADS) {
        const int r = e / (nb + 2), c = e - r * (nb + 2), gi = i - 2 + r, gj = jb0 - 1 + c;
        raw[r][c] = (unsigned)gi < (unsigned)GH && (unsigned)gj < (unsigned)GW ? g[(size_t)gi * GW + gj] : (unsigned char)0;
    }
    __syncthreads();
    for (int e = tid; e < 3 * nb; e += FL_THREADS) {
        const int k = e / nb, b = e - k * nb;
        const int rr = min(max(i - 1 + k, 0), GH - 1) - (i - 2), cc = min(max(jb0 + b, 0), GW - 1) - (jb0 - 1);   // in 1 .. 3, 1 .. nb
        int m = 0;
#pragma unroll
        for (int dr = -1; dr <= 1; ++dr)
#pragma unroll
            for (int dc = -1; dc <= 1; ++dc) m = max(m, (int)raw[rr + dr][cc + dc]);
        const int own = raw[rr][cc];
        s[k][b] = (unsigned char)max(floor_level, own * 256 < m * rq ? m : own);
    }
    __syncthreads();
    const int sh = 2 * (lt + 1);
#pragma unroll
    for (int j = 0; j < LANE_ROWS; ++j) {
        if (nv[j] == 0) continue;
        const int y = r0 + j * (FL_THREADS / FL_UNITS);
        const int uy = 2 * y + 1 - T, k = (uy >> (lt + 1)) - (i - 1), wy = uy & (D - 1);   // k in {0, 1}
        TI res[VEC];
#pragma unroll
        for (int hf = 0; hf < VEC / HV; ++hf) {
            if (hf * HV >= nv[j]) break;
            const int ux = 2 * (x + hf * HV) + 1 - T, b = (ux >> (lt + 1)) - jb0, wx0 = ux & (D - 1);
            const int va = (D - wy) * s[k][b] + wy * s[k + 1][b], vb = (D - wy) * s[k][b + 1] + wy * s[k + 1][b + 1];
#pragma unroll
            for (int p = 0; p < HV; ++p) {
                const int wx = wx0 + 2 * p;                              // < D: the half unit ends before the next tile centre
                const unsigned int r = recip[((D - wx) * va + wx * vb + D * D / 2) >> sh];   // the sum is < 2^24; the index in floor .. 255
                if constexpr (sizeof(TI) == 1) res[hf * HV + p] = (unsigned char)min(255u, ((unsigned)px[j][hf * HV + p] * r + 32768u) >> 16);
                else res[hf * HV + p] = fminf(1.0f, px[j][hf * HV + p] * ((float)r * 0x1p-16f));
            }
        }
        TI *dst = out + (size_t)y * out_pitch + x;
        if (out_aligned && nv[j] == VEC) {
            uint4 v;
            __builtin_memcpy(&v, res, 16);
            *reinterpret_cast<uint4 *>(dst) = v;
        } else {
#pragma unroll
            for (int p = 0; p < VEC; ++p)
                if (p < nv[j]) dst[p] = res[p];
        }
    }
}

int log2_tile(int tile) { return tile == 16 ? 4 : tile == 32 ? 5 : tile == 64 ? 6 : tile == 128 ? 7 : -1; }

}  // namespace

#define ACAI_FLATTEN_PAGE_CHECK(name)                                                                                                           \
    ACAI_CHECK_ARG(page, name ": null page");                                                                                                    \
    ACAI_CHECK_ARG(H > 0 && W > 0 && H <= ACAI_PAGE_MAX_H && W <= ACAI_PAGE_MAX_W && pitch >= W, name ": bad page %d x %d, pitch %d (H <= %d, W <= %d)", H, W, \
                   pitch, ACAI_PAGE_MAX_H, ACAI_PAGE_MAX_W);                                                                                     \
    ACAI_CHECK_ARG(log2_tile(tile) > 0, name ": tile %d is not 16, 32, 64 or 128", tile)

extern "C" int acai_page_tile_levels(const void *page, int in_u8, int H, int W, int pitch, int tile, int percent, uint8_t *levels, void *stream) {
    ACAI_FLATTEN_PAGE_CHECK("acai_page_tile_levels");
    ACAI_CHECK_ARG(percent >= 1 && percent <= 100, "acai_page_tile_levels: percent = %d (1 .. 100)", percent);
    ACAI_CHECK_ARG(levels, "acai_page_tile_levels: null output");
    hipStream_t st = (hipStream_t)stream;
    const int lt = log2_tile(tile), GH = cdiv(H, tile), GW = cdiv(W, tile), tiles = GH * GW;   // <= 4096 x 1024
    const dim3 grid(cdiv(tiles, LV_WAVES));
    if (in_u8)
        hipLaunchKernelGGL(page_tile_levels_kernel<unsigned char>, grid, dim3(LV_THREADS), 0, st, reinterpret_cast<const unsigned char *>(page), H, W, pitch, lt,
                           percent, GW, tiles, levels);
    else
        hipLaunchKernelGGL(page_tile_levels_kernel<float>, grid, dim3(LV_THREADS), 0, st, reinterpret_cast<const float *>(page), H, W, pitch, lt, percent, GW,
                           tiles, levels);
    ACAI_LAUNCH_CHECK("acai_page_tile_levels");
    return 0;
}

extern "C" int acai_page_flatten(const void *page, int in_u8, int H, int W, int pitch, const uint8_t *levels, int tile, int rq, int floor_level, void *out,
                                 int out_pitch, void *stream) {
    ACAI_FLATTEN_PAGE_CHECK("acai_page_flatten");
    ACAI_CHECK_ARG(levels, "acai_page_flatten: null tile levels");
    ACAI_CHECK_ARG(rq >= 0 && rq <= 256, "acai_page_flatten: rq = %d (0 .. 256, ink_ratio in 1 / 256)", rq);
    ACAI_CHECK_ARG(floor_level >= 1 && floor_level <= 255, "acai_page_flatten: floor = %d (a level, 1 .. 255)", floor_level);
    ACAI_CHECK_ARG(out && out_pitch >= W && out != page, "acai_page_flatten: bad output (pitch %d, not in place)", out_pitch);
    hipStream_t st = (hipStream_t)stream;
    const int lt = log2_tile(tile), GH = cdiv(H, tile), GW = cdiv(W, tile);
    const dim3 grid(cdiv(cdiv(W, in_u8 ? 16 : 4), FL_UNITS), cdiv(H, FL_ROWS));   // <= 128 x 4096
    if (in_u8)
        hipLaunchKernelGGL(page_flatten_kernel<unsigned char>, grid, dim3(FL_THREADS), 0, st, reinterpret_cast<const unsigned char *>(page), H, W, pitch, levels, GH,
                           GW, lt, rq, floor_level, reinterpret_cast<unsigned char *>(out), out_pitch);
    else
        hipLaunchKernelGGL(page_flatten_kernel<float>, grid, dim3(FL_THREADS), 0, st, reinterpret_cast<const float *>(page), H, W, pitch, levels, GH, GW, lt, rq,
                           floor_level, reinterpret_cast<float *>(out), out_pitch);
    ACAI_LAUNCH_CHECK("acai_page_flatten");
    return 0;
}
