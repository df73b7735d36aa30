// Per-measure results (an extension; no reference counterpart): token rows cut at delimiter tokens, and what the per-token passes know
// reduced over the spans between them.
//   acai_token_segments        one wave per row: segment index per token, the segments' bounds and their count (ballot / popcount scan);
//   acai_segment_reduce        one wave per (plane, row, segment): sum, min, max, arg-min, arg-max of per-token values;
//   acai_attn_map_segment_sum  the maps of acai_attn_probs_mean summed over each segment's rows: one map per segment;
//   acai_attn_map_extent       one workgroup per map row: the quantile box of its column and row marginals.
// Plain VALU, shuffle and LDS work.  No floating-point atomics and fixed reduction orders: the same bits on every run.  Everything that comes
// from device memory (lengths, bounds, counts, ranges) is clamped to the buffers before it indexes anything.
#include "common.h"

#include <math.h>

namespace {

constexpr int SEG_MAX_DELIMS = 8;
constexpr int SEG_WAVES = 4;       // rows (token_segments) or spans (segment_reduce) per workgroup
constexpr int RED_MAX_K = 8;
constexpr int SS_COLS = 256;       // columns per workgroup of the segment sum, one per thread
constexpr int EXT_MAX_B = 512;
constexpr int EXT_MAX_SIDE = 4096;
constexpr int EXT_THREADS = 256;

struct SegArgs {
    const int64_t *tokens;
    const int32_t *lens;
    int32_t *seg, *count, *bounds;
    int64_t delims[SEG_MAX_DELIMS];
    int64_t stop;
    int R, ld, nd, cap;
};

// Chunks of 64 tokens; `carry` is the number of delimiters before the chunk, E the row's end once a stop token was seen.  Every lane holds
// the same carry and E (they come from ballots), so there is no divergence in the control flow.
__global__ __launch_bounds__(64 * SEG_WAVES) void token_segments_kernel(const SegArgs a) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * SEG_WAVES + (threadIdx.x >> 6);
    if (r >= a.R) return;
    const int L = min(max(a.lens[r], 0), a.ld);
    const int64_t *row = a.tokens + (size_t)r * a.ld;
    int32_t *seg = a.seg + (size_t)r * a.ld;
    int32_t *bnd = a.bounds + (size_t)r * a.cap * 2;
    int carry = 0, E = L;
    for (int p0 = 0; p0 < a.ld; p0 += 64) {
        const int p = p0 + lane;
        if (p0 >= E) {   // past the end: nothing is read any more
            if (p < a.ld) seg[p] = -1;
            continue;
        }
        const bool valid = p < L;
        const int64_t tok = valid ? row[p] : 0;
        const unsigned long long stops = __ballot(valid && a.stop >= 0 && tok == a.stop);
        if (stops) E = p0 + __ffsll((long long)stops) - 1;
        bool d = false;
        for (int i = 0; i < a.nd; ++i) d |= tok == a.delims[i];
        d = d && valid && p < E;
        const unsigned long long dm = __ballot(d);
        const int c = carry + __popcll(dm & (~0ull >> (63 - lane)));   // delimiters at indices <= p
        if (p < a.ld) seg[p] = p < E ? c - 1 : -1;
        if (d) {
            if (c - 1 < a.cap) bnd[2 * (c - 1)] = p;
            if (c >= 2 && c - 2 < a.cap) bnd[2 * (c - 2) + 1] = p;
        }
        carry += __popcll(dm);
    }
    const int n = min(carry, a.cap);
    if (lane == 0) {
        a.count[r] = carry;
        if (carry >= 1 && carry - 1 < a.cap) bnd[2 * (carry - 1) + 1] = E;
    }
    for (int m = n + lane; m < a.cap; m += 64) bnd[2 * m] = bnd[2 * m + 1] = -1;
}

struct RedArgs {
    const float *values;
    const int32_t *bounds, *count;
    float *sum, *vmin, *vmax;
    int32_t *argmin, *argmax;
    int K, R, ld, cap;
};

__global__ __launch_bounds__(64 * SEG_WAVES) void segment_reduce_kernel(const RedArgs a) {
    const int lane = threadIdx.x & 63;
    const size_t w = (size_t)blockIdx.x * SEG_WAVES + (threadIdx.x >> 6);
    const size_t per_plane = (size_t)a.R * a.cap;
    if (w >= per_plane * a.K) return;
    const int m = (int)(w % a.cap), r = (int)((w / a.cap) % a.R);
    const size_t k = w / per_plane;
    float s = 0.f, lo = INFINITY, hi = -INFINITY;
    int ilo = 0x7fffffff, ihi = 0x7fffffff;
    if (m < min(a.count[r], a.cap)) {
        const int start = max(a.bounds[((size_t)r * a.cap + m) * 2], 0), end = min(a.bounds[((size_t)r * a.cap + m) * 2 + 1], a.ld);
        const float *v = a.values + (k * a.R + r) * (size_t)a.ld;
        for (int p = start + lane; p < end; p += 64) {   // ascending p: the first of equal values stays
            const float x = v[p];
            s += x;
            if (x < lo) { lo = x; ilo = p; }
            if (x > hi) { hi = x; ihi = p; }
        }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        s += __shfl_xor(s, o);
        const float olo = __shfl_xor(lo, o), ohi = __shfl_xor(hi, o);
        const int oilo = __shfl_xor(ilo, o), oihi = __shfl_xor(ihi, o);
        if (olo < lo || (olo == lo && oilo < ilo)) { lo = olo; ilo = oilo; }
        if (ohi > hi || (ohi == hi && oihi < ihi)) { hi = ohi; ihi = oihi; }
    }
    if (lane == 0) {
        const bool none = ilo == 0x7fffffff;   // a slot past the count, or an empty span
        a.sum[w] = none ? 0.f : s;
        a.vmin[w] = none ? 0.f : lo;
        a.vmax[w] = none ? 0.f : hi;
        a.argmin[w] = none ? -1 : ilo;
        a.argmax[w] = none ? -1 : ihi;
    }
}

struct SsumArgs {
    const float *map;
    const int64_t *map_off, *seg_map_off;
    const int32_t *cu_q, *cu_k, *cu_seg, *ranges;
    const float *weights;   // may be NULL: all ones
    float *out;
};

// Workgroup (x, m, b): columns x * 256 .. of segment m of image b, its map rows added in ascending order.  Consecutive threads read
// consecutive floats of every map row, and every element of a range is read exactly once.
__global__ __launch_bounds__(SS_COLS) void map_segment_sum_kernel(const SsumArgs a) {
    const int b = blockIdx.z, m = blockIdx.y;
    const int g0 = a.cu_seg[b];
    if (m >= a.cu_seg[b + 1] - g0) return;
    const int q0 = a.cu_q[b], T = a.cu_q[b + 1] - q0;
    const int S = a.cu_k[b + 1] - a.cu_k[b];
    const int s = blockIdx.x * SS_COLS + threadIdx.x;
    if (s >= S) return;
    const int t0 = max(a.ranges[2 * (size_t)(g0 + m)], 0), t1 = min(a.ranges[2 * (size_t)(g0 + m) + 1], T);
    const float *col = a.map + a.map_off[b] + s;
    float acc = 0.f;
    if (a.weights) {
        const float *w = a.weights + q0;
#pragma unroll 8
        for (int t = t0; t < t1; ++t) acc = fmaf(w[t], col[(size_t)t * S], acc);
    } else {
#pragma unroll 8
        for (int t = t0; t < t1; ++t) acc += col[(size_t)t * S];
    }
    a.out[a.seg_map_off[b] + (size_t)m * S + s] = acc;
}

struct ExtArgs {
    const float *map;
    const int64_t *map_off;
    const int32_t *cu_q, *cu_k;
    float *ext;
    float q;
    int32_t grid_w[EXT_MAX_B];
};

__device__ __forceinline__ float wave_sum_butterfly(float v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

// The two quantile positions of the header's rule for the marginal marg[0 .. n): one lane adds it up in ascending order for m, then walks
// the same running sums (the same additions, so the same bits) until both targets are reached.
__device__ void quantile_pair(const float *marg, int n, float q, float *lo_out, float *hi_out) {
    float m = 0.f;
    for (int i = 0; i < n; ++i) m += marg[i];
    if (!(m > 0.f)) {
        *lo_out = *hi_out = 0.f;
        return;
    }
    const float tlo = q * m, thi = (1.f - q) * m;
    float plo = (float)n, phi = (float)n, prev = 0.f;
    bool flo = false, fhi = false;
    for (int i = 0; i < n && !fhi; ++i) {
        const float ai = marg[i], ci = prev + ai;
        if (ai > 0.f) {
            if (!flo && ci >= tlo) { plo = (float)i + (tlo - prev) / ai; flo = true; }
            if (ci >= thi) { phi = (float)i + (thi - prev) / ai; fhi = true; }
        }
        prev = ci;
    }
    *lo_out = plo;
    *hi_out = phi;
}

// One workgroup per map row.  Column marginal: thread x adds its column top to bottom; row marginal: one wave per grid row, lanes strided
// over x, then the butterfly.  Both live in LDS; lane 0 of wave 0 scans the columns while lane 0 of wave 1 scans the rows.
__global__ __launch_bounds__(EXT_THREADS) void map_extent_kernel(const ExtArgs a) {
    __shared__ float colm[EXT_MAX_SIDE], rowm[EXT_MAX_SIDE];
    const int b = blockIdx.y, t = blockIdx.x;
    const int q0 = a.cu_q[b];
    if (t >= a.cu_q[b + 1] - q0) return;
    const int S = a.cu_k[b + 1] - a.cu_k[b];
    const int gw = a.grid_w[b];
    const int nx = min(gw, S), ny = S > 0 ? (S + gw - 1) / gw : 0;
    float *o = a.ext + (size_t)(q0 + t) * 4;
    if (S <= 0 || ny > EXT_MAX_SIDE) {   // (a grid taller than the LDS rows: refused on the host where the lengths are known)
        if (threadIdx.x < 4) o[threadIdx.x] = 0.f;
        return;
    }
    const float *row = a.map + a.map_off[b] + (size_t)t * S;
    for (int x = threadIdx.x; x < nx; x += EXT_THREADS) {
        float c = 0.f;
        for (int s = x; s < S; s += gw) c += row[s];
        colm[x] = c;
    }
    const int lane = threadIdx.x & 63;
    for (int y = threadIdx.x >> 6; y < ny; y += EXT_THREADS / 64) {
        const int s0 = y * gw, s1 = min(s0 + gw, S);
        float c = 0.f;
        for (int s = s0 + lane; s < s1; s += 64) c += row[s];
        c = wave_sum_butterfly(c);
        if (lane == 0) rowm[y] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) quantile_pair(colm, nx, a.q, o + 0, o + 2);
    if (threadIdx.x == 64) quantile_pair(rowm, ny, a.q, o + 1, o + 3);
}

}  // namespace

extern "C" int acai_token_segments(const int64_t *tokens, int ld, const int32_t *lens, int R, const int64_t *delims, int n_delims, int64_t stop,
                                   int cap, int32_t *seg, int32_t *count, int32_t *bounds, void *stream) {
    ACAI_CHECK_ARG(R >= 0 && ld >= 1, "acai_token_segments: bad dims R=%d ld=%d", R, ld);
    ACAI_CHECK_ARG(n_delims >= 1 && n_delims <= SEG_MAX_DELIMS && delims, "acai_token_segments: n_delims=%d (1 .. %d delimiter ids)", n_delims,
                   SEG_MAX_DELIMS);
    ACAI_CHECK_ARG(cap >= 1, "acai_token_segments: cap=%d (must be >= 1)", cap);
    ACAI_CHECK_ARG(stop >= -1, "acai_token_segments: stop=%lld (a token id, or -1 for none)", (long long)stop);
    if (R == 0) return 0;
    ACAI_CHECK_ARG(tokens && lens && seg && count && bounds, "acai_token_segments: null operand");
    SegArgs a{tokens, lens, seg, count, bounds, {}, stop, R, ld, n_delims, cap};
    for (int i = 0; i < n_delims; ++i) a.delims[i] = delims[i];
    hipLaunchKernelGGL(token_segments_kernel, dim3(cdiv(R, SEG_WAVES)), dim3(64 * SEG_WAVES), 0, (hipStream_t)stream, a);
    ACAI_LAUNCH_CHECK("acai_token_segments");
    return 0;
}

extern "C" int acai_segment_reduce(const float *values, int K, int R, int ld, const int32_t *bounds, const int32_t *count, int cap, float *sum,
                                   float *vmin, float *vmax, int32_t *argmin, int32_t *argmax, void *stream) {
    ACAI_CHECK_ARG(K >= 1 && K <= RED_MAX_K, "acai_segment_reduce: K=%d (1 .. %d planes)", K, RED_MAX_K);
    ACAI_CHECK_ARG(R >= 0 && ld >= 1 && cap >= 1, "acai_segment_reduce: bad dims R=%d ld=%d cap=%d", R, ld, cap);
    if (R == 0) return 0;
    ACAI_CHECK_ARG(values && bounds && count && sum && vmin && vmax && argmin && argmax, "acai_segment_reduce: null operand");
    const long long waves = (long long)K * R * cap;
    ACAI_CHECK_ARG(waves <= 0x7fffffffLL, "acai_segment_reduce: K * R * cap = %lld spans are too many", waves);
    RedArgs a{values, bounds, count, sum, vmin, vmax, argmin, argmax, K, R, ld, cap};
    hipLaunchKernelGGL(segment_reduce_kernel, dim3((unsigned)((waves + SEG_WAVES - 1) / SEG_WAVES)), dim3(64 * SEG_WAVES), 0, (hipStream_t)stream, a);
    ACAI_LAUNCH_CHECK("acai_segment_reduce");
    return 0;
}

extern "C" int acai_attn_map_segment_sum(const float *map, const int64_t *map_off, const int32_t *cu_q, const int32_t *cu_k, const float *weights,
                                         const int32_t *ranges, const int32_t *cu_seg, const int64_t *seg_map_off, int B, int max_k, int max_seg,
                                         float *out, void *stream) {
    ACAI_CHECK_ARG(B >= 0 && B <= 65535 && max_k >= 0 && max_seg >= 0 && max_seg <= 65535,
                   "acai_attn_map_segment_sum: bad dims B=%d max_k=%d max_seg=%d (B, max_seg <= 65535)", B, max_k, max_seg);
    if (B == 0 || max_seg == 0 || max_k == 0) return 0;
    ACAI_CHECK_ARG(map && map_off && cu_q && cu_k && ranges && cu_seg && seg_map_off && out, "acai_attn_map_segment_sum: null operand");
    SsumArgs a{map, map_off, seg_map_off, cu_q, cu_k, cu_seg, ranges, weights, out};
    hipLaunchKernelGGL(map_segment_sum_kernel, dim3(cdiv(max_k, SS_COLS), max_seg, B), dim3(SS_COLS), 0, (hipStream_t)stream, a);
    ACAI_LAUNCH_CHECK("acai_attn_map_segment_sum");
    return 0;
}

extern "C" int acai_attn_map_extent(const float *map, const int64_t *map_off, const int32_t *cu_q, const int32_t *cu_k, const int32_t *grid_w,
                                    int B, int max_q, float q, float *ext, void *stream) {
    ACAI_CHECK_ARG(B >= 0 && B <= EXT_MAX_B && max_q >= 0, "acai_attn_map_extent: bad dims B=%d max_q=%d (B <= %d)", B, max_q, EXT_MAX_B);
    ACAI_CHECK_ARG(q >= 0.f && q < 0.5f, "acai_attn_map_extent: q=%g (0 <= q < 0.5)", (double)q);
    if (B == 0 || max_q == 0) return 0;
    ACAI_CHECK_ARG(map && map_off && cu_q && cu_k && grid_w && ext, "acai_attn_map_extent: null operand");
    ExtArgs a{map, map_off, cu_q, cu_k, ext, q, {}};
    for (int b = 0; b < B; ++b) {
        ACAI_CHECK_ARG(grid_w[b] >= 1 && grid_w[b] <= EXT_MAX_SIDE, "acai_attn_map_extent: grid_w[%d] = %d (1 .. %d)", b, grid_w[b], EXT_MAX_SIDE);
        a.grid_w[b] = grid_w[b];
    }
    hipLaunchKernelGGL(map_extent_kernel, dim3(max_q, B), dim3(EXT_THREADS), 0, (hipStream_t)stream, a);
    ACAI_LAUNCH_CHECK("acai_attn_map_extent");
    return 0;
}
