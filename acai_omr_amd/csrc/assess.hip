// Page assessment (an extension; the reference's service decodes whatever photo it is handed, acai_omr/ui/routes.py, and every page stage
// here is sized from the canvas, not from the music):
//   acai_page_runs       the lengths of the vertical runs of ink and of paper of a page, and of every ink run together with the paper run
//                        under it, as three 256-bin histograms: the most frequent ink run is the staff-line thickness, the most frequent
//                        pair the distance from staff line to staff line (the first step of every classical OMR front end),
//   acai_page_sharpness  the histogram of the page's levels and the sum and the sum of squares of its 4-neighbour Laplacian: contrast and
//                        focus.
// Integers only (include/acai_omr_hip.h has the definitions): the only atomics are integer adds, in LDS first and then one per non-empty
// bin and workgroup in global memory, so the results do not depend on the launch geometry or on how the launches are scheduled.
#include "common.h"
#include "resize_taps.h"
#include "assess_walk.h"

namespace {

constexpr int LANE_PX = 4, WG_WAVES = 4, WG_THREADS = 64 * WG_WAVES, ROWS_AHEAD = 8;

template <typename TI>
__device__ __forceinline__ bool is_ink(const TI *p, float thr) { return in_sample(p) < thr; }

// A uint8 value v is ink iff (float)v / 255 < thr, which is monotone in v: iff v < the first value that is not, found by bisection with the
// comparison itself (as csrc/page.hip and csrc/ingest.hip do).
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

__device__ __forceinline__ int cdiv_dev(int a, int b) { return (a + b - 1) / b; }

// csrc/flatten.hip's levels, statement for statement
__device__ __forceinline__ int level_of(unsigned char v) { return v; }
__device__ __forceinline__ int level_of(float v) { return (int)fminf(fmaxf(floorf(__fadd_rn(__fmul_rn(v, 255.0f), 0.5f)), 0.0f), 255.0f); }

// ---- runs -------------------------------------------------------------------------------------------------------------------------------
// (the bookkeeping itself is plain C++ in assess_walk.h: `Walk` carries a column's current run and counts a run when the next one begins)
constexpr int RC = ACAI_RUNS_CHUNK_ROWS;
static_assert(RC >= 1 && RC <= 63, "a run inside a chunk must fit the 6 bits the summary word has for it");

struct LdsCount {
    unsigned int *h;
    __device__ __forceinline__ void operator()(int row, int bin) const { atomicAdd(h + row * 256 + bin, 1u); }
};
using ColWalk = acai_runs::Walk<LdsCount>;

// Grid (groups of 64 lanes x 4 columns, groups of 4 chunks); wave w of a workgroup walks chunk 4 blockIdx.y + w.  A lane owns 4 adjacent
// columns and walks its chunk's rows down, ROWS_AHEAD rows loaded before the first of them is looked at: a wave reads 256 consecutive pixels
// of every row.  Runs that begin and end inside the chunk, and pairs of two such runs, are counted here, in the workgroup's histograms h;
// the chunk's first and last run of every column, with the run next to each, go to `work` as one word (acai_runs::pack).
template <typename TI>
__global__ __launch_bounds__(WG_THREADS) void runs_chunk_kernel(const TI *__restrict__ page, int H, int W, int pitch, float thr, int32_t *__restrict__ work,
                                                                unsigned long long *__restrict__ hist) {
    __shared__ unsigned int h[3 * 256];
    for (int b = threadIdx.x; b < 3 * 256; b += WG_THREADS) h[b] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunk = blockIdx.y * WG_WAVES + wave, y0 = chunk * RC, y1 = min(y0 + RC, H);
    const int x0 = (blockIdx.x * 64 + lane) * LANE_PX;
    if (y0 < H && x0 < W) {
        const int n = min(LANE_PX, W - x0);
        const int limit = sizeof(TI) == 1 ? ink_limit_u8(thr) : 0;
        ColWalk c[LANE_PX] = {ColWalk(LdsCount{h}), ColWalk(LdsCount{h}), ColWalk(LdsCount{h}), ColWalk(LdsCount{h})};
        int y = y0;
        if (n == LANE_PX) {
            for (; y + ROWS_AHEAD <= y1; y += ROWS_AHEAD) {
                TI v[ROWS_AHEAD][LANE_PX];
#pragma unroll
                for (int u = 0; u < ROWS_AHEAD; ++u) __builtin_memcpy(v[u], page + (size_t)(y + u) * pitch + x0, sizeof(v[u]));
#pragma unroll
                for (int u = 0; u < ROWS_AHEAD; ++u) {
#pragma unroll
                    for (int k = 0; k < LANE_PX; ++k) {
                        if constexpr (sizeof(TI) == 1) c[k].pixel((int)v[u][k] < limit);
                        else c[k].pixel(is_ink(&v[u][k], thr));
                    }
                }
            }
        }
        for (; y < y1; ++y) {                                  // the rows left over, and every row of the lane at the ragged edge (n < 4)
            const TI *row = page + (size_t)y * pitch + x0;
#pragma unroll
            for (int k = 0; k < LANE_PX; ++k)
                if (k < n) c[k].pixel(is_ink(row + k, thr));
        }
        int32_t *w = work + (size_t)chunk * W + x0;
#pragma unroll
        for (int k = 0; k < LANE_PX; ++k)
            if (k < n) w[k] = acai_runs::pack(c[k].summary());
    }
    __syncthreads();
    for (int b = threadIdx.x; b < 3 * 256; b += WG_THREADS)
        if (h[b]) atomicAdd(hist + b, (unsigned long long)h[b]);
}

// The join, in two levels inside one workgroup of JOIN_SEGS waves on 64 columns: the walk down a column is sequential, and one lane per
// column over all chunks is as many dependent steps as the page has chunks.  Wave s walks the chunks of segment s of every column - the
// same `Walk`, fed summaries instead of pixels - counts what closes inside its segment and leaves the segment's own summary in LDS; wave 0
// then walks the JOIN_SEGS summaries of its columns and counts what crosses a segment's edge.  The run a column ends with touches row
// H - 1 and is never counted.  The loads do not depend on the walk: unrolled, several chunks' go out together.
constexpr int JOIN_SEGS = 8, JOIN_THREADS = 64 * JOIN_SEGS;

__global__ __launch_bounds__(JOIN_THREADS) void runs_join_kernel(const int32_t *__restrict__ work, int W, int chunks, unsigned long long *__restrict__ hist) {
    __shared__ unsigned int h[3 * 256];
    __shared__ acai_runs::Summary seg_sum[JOIN_SEGS][64];
    __shared__ int seg_runs[JOIN_SEGS][64];
    for (int b = threadIdx.x; b < 3 * 256; b += JOIN_THREADS) h[b] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
    const int x = blockIdx.x * 64 + lane;
    const int per = cdiv_dev(chunks, JOIN_SEGS), c0 = min(seg * per, chunks), c1 = min(c0 + per, chunks);
    if (x < W) {
        ColWalk walk(LdsCount{h});
#pragma unroll 4
        for (int c = c0; c < c1; ++c) walk.stretch(acai_runs::unpack(work[(size_t)c * W + x]));
        seg_runs[seg][lane] = walk.n;
        if (walk.n) seg_sum[seg][lane] = walk.summary();
    }
    __syncthreads();
    if (seg == 0 && x < W) {
        ColWalk walk(LdsCount{h});
        for (int s = 0; s < JOIN_SEGS; ++s)
            if (seg_runs[s][lane]) walk.stretch(seg_sum[s][lane]);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < 3 * 256; b += JOIN_THREADS)
        if (h[b]) atomicAdd(hist + b, (unsigned long long)h[b]);
}

// ---- sharpness --------------------------------------------------------------------------------------------------------------------------
constexpr int SC = ACAI_SHARP_CHUNK_ROWS;
static_assert(SC * LANE_PX * 1020 * 1020 < 0x7fffffff, "a lane's sum of squares over its chunk is kept in 32 bits");

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The same grid and lanes as runs_chunk_kernel.  A wave walks rows y0 - 1 .. y1 of its chunk [y0, y1) (those of them that exist), three
// rows of levels in registers at a time: the rows of the chunk go into the wave's own histogram, and the middle row's Laplacian is formed
// from the rows around it, the left and right neighbours across lanes by shuffles; lanes 0 and 63 read theirs from the page.  A lane adds
// equal neighbouring levels of its 4 pixels to the histogram as one (flat paper: one add per lane and row).  out = (sum L, sum L^2, count,
// levels [256]).
template <typename TI>
__global__ __launch_bounds__(WG_THREADS) void sharpness_kernel(const TI *__restrict__ page, int H, int W, int pitch, unsigned long long *__restrict__ out) {
    __shared__ unsigned int hist[WG_WAVES][256];
    __shared__ long long part[WG_WAVES][2];
    for (int b = threadIdx.x; b < WG_WAVES * 256; b += WG_THREADS) (&hist[0][0])[b] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunk = blockIdx.y * WG_WAVES + wave, y0 = chunk * SC, y1 = min(y0 + SC, H);
    const int x0 = (blockIdx.x * 64 + lane) * LANE_PX, n = max(0, min(LANE_PX, W - x0));
    unsigned int *h = hist[wave];
    int a1 = 0;
    unsigned int a2 = 0;
    if (y0 < H) {                                              // (the same for every lane of the wave: all 64 take part in the shuffles)
        const int ys = max(y0 - 1, 0), ye = min(y1, H - 1);    // first and last row that is read
        const int m0 = max(y0, 1), m1 = min(y1, H - 1);        // the chunk's interior rows [m0, m1)
        const bool edge_l = lane == 0 && x0 > 0, edge_r = lane == 63 && x0 + LANE_PX < W;
        int a[LANE_PX] = {0, 0, 0, 0}, b[LANE_PX] = {0, 0, 0, 0}, bl = 0, br = 0;
        for (int yb = ys; yb <= ye; yb += ROWS_AHEAD) {
            TI v[ROWS_AHEAD][LANE_PX], vl[ROWS_AHEAD], vr[ROWS_AHEAD];
#pragma unroll
            for (int u = 0; u < ROWS_AHEAD; ++u) {
                const TI *row = page + (size_t)min(yb + u, ye) * pitch;
                if (n == LANE_PX) {
                    __builtin_memcpy(v[u], row + x0, sizeof(v[u]));
                } else {
#pragma unroll
                    for (int k = 0; k < LANE_PX; ++k) v[u][k] = k < n ? row[x0 + k] : TI(0);
                }
                vl[u] = edge_l ? row[x0 - 1] : TI(0);
                vr[u] = edge_r ? row[x0 + LANE_PX] : TI(0);
            }
#pragma unroll
            for (int u = 0; u < ROWS_AHEAD; ++u) {
                const int y = yb + u;
                if (y > ye) break;
                int c[LANE_PX];
#pragma unroll
                for (int k = 0; k < LANE_PX; ++k) c[k] = level_of(v[u][k]);
                const int from_l = __shfl_up(c[LANE_PX - 1], 1), from_r = __shfl_down(c[0], 1);
                const int cl = lane == 0 ? level_of(vl[u]) : from_l, cr = lane == 63 ? level_of(vr[u]) : from_r;
                if (y >= y0 && y < y1 && n > 0) {
                    int cur = c[0], cnt = 1;
#pragma unroll
                    for (int k = 1; k < LANE_PX; ++k) {
                        if (k < n) {
                            if (c[k] == cur) {
                                ++cnt;
                            } else {
                                atomicAdd(h + cur, (unsigned int)cnt);
                                cur = c[k], cnt = 1;
                            }
                        }
                    }
                    atomicAdd(h + cur, (unsigned int)cnt);
                }
                if (y - 1 >= m0 && y - 1 < m1) {               // rows y - 2, y - 1, y are a, b, c
#pragma unroll
                    for (int k = 0; k < LANE_PX; ++k) {
                        const int x = x0 + k;
                        if (x >= 1 && x <= W - 2) {
                            const int left = k ? b[k - 1] : bl, right = k < LANE_PX - 1 ? b[k + 1] : br;
                            const int L = 4 * b[k] - a[k] - c[k] - left - right;
                            a1 += L, a2 += (unsigned int)(L * L);
                        }
                    }
                }
#pragma unroll
                for (int k = 0; k < LANE_PX; ++k) a[k] = b[k], b[k] = c[k];
                bl = cl, br = cr;
            }
        }
    }
    const long long s1 = wave_sum_i64((long long)a1), s2 = wave_sum_i64((long long)a2);
    if (lane == 0) part[wave][0] = s1, part[wave][1] = s2;
    __syncthreads();
    unsigned int total = 0;
#pragma unroll
    for (int w = 0; w < WG_WAVES; ++w) total += hist[w][threadIdx.x];
    if (total) atomicAdd(out + 3 + threadIdx.x, (unsigned long long)total);
    if (threadIdx.x == 0) {
        long long t1 = 0, t2 = 0;
        for (int w = 0; w < WG_WAVES; ++w) t1 += part[w][0], t2 += part[w][1];
        if (t1) atomicAdd(out + 0, (unsigned long long)t1);    // (two's complement: the sum of the signed parts)
        if (t2) atomicAdd(out + 1, (unsigned long long)t2);
        if (blockIdx.x == 0 && blockIdx.y == 0 && H >= 3 && W >= 3) atomicAdd(out + 2, (unsigned long long)(H - 2) * (unsigned long long)(W - 2));
    }
}

}  // namespace

#define ACAI_PAGE_CHECK(name)                                                                                                                   \
    ACAI_CHECK_ARG(page, name ": null page");                                                                                                    \
    ACAI_CHECK_ARG(H > 0 && W > 0 && H <= ACAI_PAGE_MAX_H && W <= ACAI_PAGE_MAX_W && pitch >= W, name ": bad page %d x %d, pitch %d (H <= %d, W <= %d)", H, W, \
                   pitch, ACAI_PAGE_MAX_H, ACAI_PAGE_MAX_W)

extern "C" int acai_page_runs(const void *page, int in_u8, int H, int W, int pitch, float ink_threshold, int64_t *hist, int32_t *work, int64_t work_elems,
                              void *stream) {
    ACAI_PAGE_CHECK("acai_page_runs");
    const int chunks = cdiv(H, RC);                                                       // <= 2048
    ACAI_CHECK_ARG(hist && work && work_elems >= (int64_t)chunks * W, "acai_page_runs: null output, or work holds %lld int32 where %lld are needed",
                   (long long)work_elems, (long long)chunks * W);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *hg = reinterpret_cast<unsigned long long *>(hist);
    const dim3 grid(cdiv(cdiv(W, LANE_PX), 64), cdiv(chunks, WG_WAVES));                  // <= 64 x 512
    if (in_u8)
        hipLaunchKernelGGL(runs_chunk_kernel<unsigned char>, grid, dim3(WG_THREADS), 0, st, reinterpret_cast<const unsigned char *>(page), H, W, pitch,
                           ink_threshold, work, hg);
    else
        hipLaunchKernelGGL(runs_chunk_kernel<float>, grid, dim3(WG_THREADS), 0, st, reinterpret_cast<const float *>(page), H, W, pitch, ink_threshold, work, hg);
    ACAI_LAUNCH_CHECK("acai_page_runs (chunks)");
    hipLaunchKernelGGL(runs_join_kernel, dim3(cdiv(W, 64)), dim3(JOIN_THREADS), 0, st, (const int32_t *)work, W, chunks, hg);
    ACAI_LAUNCH_CHECK("acai_page_runs (join)");
    return 0;
}

extern "C" int acai_page_sharpness(const void *page, int in_u8, int H, int W, int pitch, int64_t *out, void *stream) {
    ACAI_PAGE_CHECK("acai_page_sharpness");
    ACAI_CHECK_ARG(out, "acai_page_sharpness: null output");
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *og = reinterpret_cast<unsigned long long *>(out);
    const dim3 grid(cdiv(cdiv(W, LANE_PX), 64), cdiv(cdiv(H, SC), WG_WAVES));
    if (in_u8)
        hipLaunchKernelGGL(sharpness_kernel<unsigned char>, grid, dim3(WG_THREADS), 0, st, reinterpret_cast<const unsigned char *>(page), H, W, pitch, og);
    else
        hipLaunchKernelGGL(sharpness_kernel<float>, grid, dim3(WG_THREADS), 0, st, reinterpret_cast<const float *>(page), H, W, pitch, og);
    ACAI_LAUNCH_CHECK("acai_page_sharpness");
    return 0;
}
