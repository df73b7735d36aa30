// The decode step's GEMVs (see decode.hip for the step they are chained into).
//   skinny_gemm   : y[B,N] = x[B,K] . W[N,K]^T, 8 lanes per weight row (128 contiguous bytes per row per
//                   wave instruction), x staged once per workgroup in LDS (bf16 or fp32), v_dot2_f32_bf16.
//   skinny_mfma / skinny_chain : the bf16 forms on the matrix cores, with the LayerNorm fusions of the decode chain.
#include "decode_internal.h"

namespace {

constexpr int SK_KC = 1024;  // k elements of x staged in LDS per pass
constexpr int SK_BC = 8;     // batch rows per pass

// diagnostic stamp buffer: [launch][1024 workgroups][8] (tools/stamp_decode.py); one slot per skinny launch, handed out in launch order
static unsigned long long *g_stamps = nullptr;
static int g_stamp_cap = 0, g_stamp_next = 0;

template <typename TW, bool FAST>
__global__ __launch_bounds__(256) void skinny_gemm_kernel(SkinnyArgs a) {
    constexpr int ES = sizeof(TW), EPC = 16 / ES;
    __shared__ __attribute__((aligned(16))) unsigned char xs_raw[SK_BC * SK_KC * ES];
    TW *xs = reinterpret_cast<TW *>(xs_raw);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kq = lane & 7, rsub = lane >> 3;
    const int n = blockIdx.x * 32 + wave * 8 + rsub;
    const TW *W = reinterpret_cast<const TW *>(a.W);
    const bool row_ok = n < a.N;

    for (int b0 = 0; b0 < a.B; b0 += SK_BC) {
        const int nb = min(SK_BC, a.B - b0);
        float acc[SK_BC];
#pragma unroll
        for (int b = 0; b < SK_BC; ++b) acc[b] = 0.f;
        for (int k0 = 0; k0 < a.K; k0 += SK_KC) {
            const int kc = min(SK_KC, a.K - k0);
            __syncthreads();  // previous pass has finished reading xs
            for (int i = tid; i < SK_BC * SK_KC; i += 256) {
                const int b = i / SK_KC, k = i - b * SK_KC;
                const float v = (b < nb && k < kc) ? a.x[(size_t)(b0 + b) * a.ldx + k0 + k] : 0.f;
                DT<TW>::st(xs + i, v);  // bf16 mode: autocast's input cast
            }
            __syncthreads();
            if (row_ok) {
                const int nsteps = (kc + 8 * EPC - 1) / (8 * EPC);
#pragma unroll 4
                for (int s = 0; s < nsteps; ++s) {
                    const int kl = (s * 8 + kq) * EPC;  // local k of this lane's chunk
                    uint4 wv = make_uint4(0, 0, 0, 0);
                    if constexpr (FAST) {
                        if (kl < kc) wv = *reinterpret_cast<const uint4 *>(W + (size_t)n * a.ldw + k0 + kl);
                    } else {
                        union { uint4 v; TW e[EPC]; } u;
                        u.v = wv;
#pragma unroll
                        for (int e = 0; e < EPC; ++e)
                            if (kl + e < kc) u.e[e] = W[(size_t)n * a.ldw + k0 + kl + e];
                        wv = u.v;
                    }
#pragma unroll
                    for (int b = 0; b < SK_BC; ++b) {
                        const uint4 xv = *reinterpret_cast<const uint4 *>(xs + b * SK_KC + kl);
                        if constexpr (ES == 2) {
                            acc[b] = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, wv.x), __builtin_bit_cast(bf16x2, xv.x), acc[b], false);
                            acc[b] = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, wv.y), __builtin_bit_cast(bf16x2, xv.y), acc[b], false);
                            acc[b] = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, wv.z), __builtin_bit_cast(bf16x2, xv.z), acc[b], false);
                            acc[b] = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, wv.w), __builtin_bit_cast(bf16x2, xv.w), acc[b], false);
                        } else {
                            const f32x4 w4 = __builtin_bit_cast(f32x4, wv), x4 = __builtin_bit_cast(f32x4, xv);
                            acc[b] = fmaf(w4[0], x4[0], acc[b]);
                            acc[b] = fmaf(w4[1], x4[1], acc[b]);
                            acc[b] = fmaf(w4[2], x4[2], acc[b]);
                            acc[b] = fmaf(w4[3], x4[3], acc[b]);
                        }
                    }
                }
            }
        }
        // reduce over the 8 lanes of a row; afterwards lane kq owns batch row b0 + kq
        float mine = 0.f;
#pragma unroll
        for (int b = 0; b < SK_BC; ++b) {
            float v = acc[b];
            v += __shfl_xor(v, 1);
            v += __shfl_xor(v, 2);
            v += __shfl_xor(v, 4);
            if (kq == b) mine = v;
        }
        const int b = b0 + kq;
        if (row_ok && kq < nb) {
            float v = mine + (a.bias ? a.bias[n] : 0.f);
            const bool rnd = a.flags & ACAI_GEMM_ROUND_BF16;
            if (rnd) v = round_bf16(v);
            if (a.flags & ACAI_GEMM_GELU) {
                v = gelu_erf(v);
                if (rnd) v = round_bf16(v);
            }
            if (a.k_cache && n >= a.E) {  // KVCache.update (K:94-95): position = entries already cached
                const int kv = (n - a.E) / a.E, e = (n - a.E) - kv * a.E, hh = e / a.dh, dd = e - hh * a.dh;
                const size_t off = (((size_t)b * a.H + hh) * a.Tmax + a.step[1]) * a.dhp + dd;
                DT<TW>::st(reinterpret_cast<TW *>(kv ? a.v_cache : a.k_cache) + off, v);
            }
            if (a.residual) v += a.residual[(size_t)b * a.ldr + n];
            a.y[(size_t)b * a.ldy + n] = v;
        }
    }
}

// ---- bf16 weights: MFMA skinny GEMM ---------------------------------------------------------------------------
// Workgroup = 16 weight rows x all of K; wave w owns K/4 of it, so every lane streams its 16-byte fragments of the
// weight rows straight into VGPRs (8 loads in flight per lane, issued BEFORE anything else) and
// v_mfma_f32_16x16x32_bf16 does the K reduction: A = W[16 rows][32 k], B = x^T[32 k][16 batch columns], D[row][batch]
// in fp32.  No cross-lane shuffles.  While the weight loads fly, the four waves build the bf16 activation image in
// LDS (pitch K*2+16 bytes: conflict-free ds_read_b128 over 16 rows): each wave reads whole rows of x into registers
// once, optionally applies the LayerNorm (post-LN decoder: x = LN(z)) from in-register statistics, rounds to bf16
// (= autocast's input cast).  The 4 K-slices meet in LDS once.  Fusions that remove launches from the decode step:
// LN on load, published (mean, rstd) for the residual path of a later launch, bf16 activations in / out.

// 16-byte non-temporal load: decoder weights (and K/V) are read exactly once per decode step
template <int NV>
__device__ __forceinline__ void skm_row_stats(const float4 (&v)[NV], int K, int lane, float eps, float &mean, float &rstd) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j)
        if (j * 256 + lane * 4 < K) s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
    mean = wave_sum(s) / (float)K;
    float qq = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j)
        if (j * 256 + lane * 4 < K) {
            const float d0 = v[j].x - mean, d1 = v[j].y - mean, d2 = v[j].z - mean, d3 = v[j].w - mean;
            qq += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
        }
    rstd = 1.0f / sqrtf(wave_sum(qq) / (float)K + eps);
}

// LayerNorm statistics of a row are taken of x - p, p = the row's first element: the pre-LN residual stream may carry an offset large
// against its spread, which one-pass E[x^2] - mean^2 (and a mean rounded at |mean|'s ulp) would turn into a relative variance error of
// ~2^-24 mean^2 / var (offset / spread 3000: the variance off by 100 %).  x - p is exact (Sterbenz) for values within a factor 2 of p.
// p comes from a scalar load of the wave-uniform row address, waited for on its own counter, so it adds no wait on the vector loads.
__device__ __forceinline__ float skm_pivot(const float *row) {
    const unsigned long long u = reinterpret_cast<unsigned long long>(row);
    const unsigned long long r = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(u >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((unsigned)u);
    float p;
    asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(p) : "s"(r));
    return p;
}

template <int NV>
__device__ __forceinline__ void skm_shift(float4 (&v)[NV], int K, int lane, float p) {
#pragma unroll
    for (int j = 0; j < NV; ++j)
        if (j * 256 + lane * 4 < K) {
            v[j].x -= p; v[j].y -= p; v[j].z -= p; v[j].w -= p;
        }
}

// NV = float4 registers per lane for one fp32 activation row (K <= 256 * NV); NW = waves per workgroup = K slices
// (NW = K/256 puts a slice's 8 weight fragments per lane in flight at once: one HBM round trip per workgroup)
template <bool XBF16, int NV, int NW>
__global__ __launch_bounds__(64 * NW) void skinny_mfma_kernel(SkinnyArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int R = a.rows_per_block;                            // weight rows of this workgroup (4, 8 or 16)
    const int n0 = blockIdx.x * R;
    const int K = a.K, Kw = K / NW, kbase = wave * Kw, nch = Kw >> 5;
    const int pitch = K * 2 + 16;
    const bool row_ok = r < R && n0 + r < a.N;
    const bf16_t *Wrow = reinterpret_cast<const bf16_t *>(a.W) + (size_t)(row_ok ? n0 + r : 0) * a.ldw + kbase + 8 * q;
    float *red = reinterpret_cast<float *>(smem);              // [NW][256] floats
    unsigned char *xs = smem + NW * 1024;                      // [rows][pitch] bf16 activation image
    auto stamp = [&](int k) {
        if (a.stamps && tid == 0) a.stamps[(size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 8 + k] = __builtin_amdgcn_s_memrealtime();
    };
    stamp(0);

    // batch tiles of 16 rows: one per workgroup along grid.y (B > 16: GRPO rollouts, max_batch_size = 32 inference) - the tiles of a weight
    // row block re-read its weights from L2 instead of queueing four latency chains inside one workgroup (64 rows: 24 -> 17 us per launch)
    for (int bt = blockIdx.y * 16; bt < a.B; bt += 16 * gridDim.y) {
        const int nb = min(16, a.B - bt);
        // 1. first batch of weight fragments.  Loads return in issue order, so whatever is requested first is waited for first: the activation
        // rows (whose consumer chain - statistics, LDS image, barrier - is the long one) are requested BEFORE the weights and the epilogue
        // operands, which are only needed after the barrier (+1-2 % tokens/s over weights-first on the same box).
        uint4 wf[8];
        bool w_requested = false;
        auto request_weights = [&]() {
            if (w_requested) return;
            w_requested = true;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                wf[c] = make_uint4(0, 0, 0, 0);
                if (c < nch && row_ok) wf[c] = a.w_cached ? *reinterpret_cast<const uint4 *>(Wrow + 32 * c) : ld_nt16(Wrow + 32 * c);
            }
        };
        constexpr bool X_FIRST = !XBF16 && NV <= 4;   // (the bf16-input and NV = 16 paths keep weights first)
        // 1b. wave 0 also fetches everything its epilogue needs now, so that nothing is loaded after the reduction
        float e_bias[4] = {0.f, 0.f, 0.f, 0.f}, e_res[4] = {0.f, 0.f, 0.f, 0.f}, e_rw[4] = {1.f, 1.f, 1.f, 1.f}, e_rb[4] = {0.f, 0.f, 0.f, 0.f};
        float rmean = 0.f, rrstd = 1.f;
        bool e_requested = false;
        auto request_epilogue = [&]() {
            if (e_requested) return;
            e_requested = true;
            if (wave == 0) {
                const int b = bt + r;
                const bool col_ok = r < nb;
                if (a.rln_w && col_ok) {
                    rmean = a.rstats[b * 2];
                    rrstd = a.rstats[b * 2 + 1];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int n = n0 + 4 * q + i;
                    if (4 * q + i < R && n < a.N) {
                        if (a.bias) e_bias[i] = a.bias[n];
                        if (a.residual && col_ok) e_res[i] = a.residual[(size_t)b * a.ldr + n];
                        if (a.rln_w) {
                            e_rw[i] = a.rln_w[n];
                            e_rb[i] = a.rln_b[n];
                        }
                    }
                }
            }
        };
        if (!X_FIRST) {
            request_weights();
            request_epilogue();
        }
        // 2. activation image: wave w takes rows w, w+4 (together), then w+8, w+12; lane takes 4-element groups
        if constexpr (XBF16) {
            // plain copy of the bf16 rows (global loads and LDS stores do not alias: the compiler hoists the loads of a row)
            for (int b0 = wave; b0 < nb; b0 += NW) {
                const bf16_t *xr0 = reinterpret_cast<const bf16_t *>(a.x) + (size_t)(bt + b0) * a.ldx;
#pragma unroll
                for (int j = 0; j < SKM_MAXK / 512; ++j) {
                    const int k = j * 512 + lane * 8;
                    if (k < K) *reinterpret_cast<uint4 *>(xs + b0 * pitch + k * 2) = *reinterpret_cast<const uint4 *>(xr0 + k);
                }
            }
        } else if constexpr (NV <= 4) {
            for (int b0 = wave; b0 < nb; b0 += 2 * NW) {
                const bool two = b0 + NW < nb;
                const float *xr0 = a.x + (size_t)(bt + b0) * a.ldx, *xr1 = a.x + (size_t)(bt + (two ? b0 + NW : b0)) * a.ldx;
                float4 v0[NV], v1[NV], lw[NV], lb[NV];
#pragma unroll
                for (int j = 0; j < NV; ++j)
                    if (j * 256 + lane * 4 < K) {
                        v0[j] = *reinterpret_cast<const float4 *>(xr0 + j * 256 + lane * 4);
                        v1[j] = *reinterpret_cast<const float4 *>(xr1 + j * 256 + lane * 4);
                        if (a.ln_w) {
                            lw[j] = *reinterpret_cast<const float4 *>(a.ln_w + j * 256 + lane * 4);
                            lb[j] = *reinterpret_cast<const float4 *>(a.ln_b + j * 256 + lane * 4);
                        }
                    }
                request_weights();   // behind this wave's activation rows
                request_epilogue();
                if (a.ln_w) {
                    // both rows' sum and sum of squares ride the same 6 cross-lane steps (4 independent chains).  Shifted one-pass
                    // variance: the sums run over x - p with p = the row's first element, so a common offset of the row (the pre-LN
                    // residual stream) does not cancel catastrophically in E[x^2] - mean^2; the rows stay shifted until normalised
                    const float p0 = skm_pivot(xr0), p1 = skm_pivot(xr1);
                    skm_shift<NV>(v0, K, lane, p0);
                    skm_shift<NV>(v1, K, lane, p1);
                    float t0 = 0.f, u0 = 0.f, t1 = 0.f, u1 = 0.f;
#pragma unroll
                    for (int j = 0; j < NV; ++j)
                        if (j * 256 + lane * 4 < K) {
                            t0 += (v0[j].x + v0[j].y) + (v0[j].z + v0[j].w);
                            u0 += (v0[j].x * v0[j].x + v0[j].y * v0[j].y) + (v0[j].z * v0[j].z + v0[j].w * v0[j].w);
                            t1 += (v1[j].x + v1[j].y) + (v1[j].z + v1[j].w);
                            u1 += (v1[j].x * v1[j].x + v1[j].y * v1[j].y) + (v1[j].z * v1[j].z + v1[j].w * v1[j].w);
                        }
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        t0 += __shfl_xor(t0, o);
                        u0 += __shfl_xor(u0, o);
                        t1 += __shfl_xor(t1, o);
                        u1 += __shfl_xor(u1, o);
                    }
                    const float invK = 1.0f / (float)K;
                    const float m0 = t0 * invK, m1 = t1 * invK;
                    const float s0 = 1.0f / sqrtf(fmaxf(u0 * invK - m0 * m0, 0.f) + a.ln_eps), s1 = 1.0f / sqrtf(fmaxf(u1 * invK - m1 * m1, 0.f) + a.ln_eps);
                    if (lane == 0 && a.stats_out && blockIdx.x == 0) {
                        a.stats_out[(bt + b0) * 2] = p0 + m0;
                        a.stats_out[(bt + b0) * 2 + 1] = s0;
                        if (two) {
                            a.stats_out[(bt + b0 + NW) * 2] = p1 + m1;
                            a.stats_out[(bt + b0 + NW) * 2 + 1] = s1;
                        }
                    }
#pragma unroll
                    for (int j = 0; j < NV; ++j)
                        if (j * 256 + lane * 4 < K) {
                            v0[j].x = (v0[j].x - m0) * s0 * lw[j].x + lb[j].x; v0[j].y = (v0[j].y - m0) * s0 * lw[j].y + lb[j].y;
                            v0[j].z = (v0[j].z - m0) * s0 * lw[j].z + lb[j].z; v0[j].w = (v0[j].w - m0) * s0 * lw[j].w + lb[j].w;
                            v1[j].x = (v1[j].x - m1) * s1 * lw[j].x + lb[j].x; v1[j].y = (v1[j].y - m1) * s1 * lw[j].y + lb[j].y;
                            v1[j].z = (v1[j].z - m1) * s1 * lw[j].z + lb[j].z; v1[j].w = (v1[j].w - m1) * s1 * lw[j].w + lb[j].w;
                        }
                }
#pragma unroll
                for (int j = 0; j < NV; ++j)
                    if (j * 256 + lane * 4 < K) {
                        const int kb = (j * 256 + lane * 4) * 2;
                        *reinterpret_cast<uint2 *>(xs + b0 * pitch + kb) = make_uint2(pack_bf16(v0[j].x, v0[j].y), pack_bf16(v0[j].z, v0[j].w));
                        if (two) *reinterpret_cast<uint2 *>(xs + (b0 + NW) * pitch + kb) = make_uint2(pack_bf16(v1[j].x, v1[j].y), pack_bf16(v1[j].z, v1[j].w));
                    }
            }
        } else {
            for (int b = wave; b < nb; b += NW) {
                const float *xr = a.x + (size_t)(bt + b) * a.ldx;
                float4 v[NV];
#pragma unroll
                for (int j = 0; j < NV; ++j)
                    if (j * 256 + lane * 4 < K) v[j] = *reinterpret_cast<const float4 *>(xr + j * 256 + lane * 4);
                float mean = 0.f, rstd = 1.f;
                if (a.ln_w) {
                    const float p = skm_pivot(xr);   // (as above: the statistics of x - p, the row stays shifted)
                    skm_shift<NV>(v, K, lane, p);
                    skm_row_stats<NV>(v, K, lane, a.ln_eps, mean, rstd);
                    if (lane == 0 && a.stats_out && blockIdx.x == 0) {
                        a.stats_out[(bt + b) * 2] = p + mean;
                        a.stats_out[(bt + b) * 2 + 1] = rstd;
                    }
                }
#pragma unroll
                for (int j = 0; j < NV; ++j)
                    if (j * 256 + lane * 4 < K) {
                        const int k = j * 256 + lane * 4;
                        if (a.ln_w) {
                            const float4 w4 = *reinterpret_cast<const float4 *>(a.ln_w + k), b4 = *reinterpret_cast<const float4 *>(a.ln_b + k);
                            v[j].x = (v[j].x - mean) * rstd * w4.x + b4.x; v[j].y = (v[j].y - mean) * rstd * w4.y + b4.y;
                            v[j].z = (v[j].z - mean) * rstd * w4.z + b4.z; v[j].w = (v[j].w - mean) * rstd * w4.w + b4.w;
                        }
                        *reinterpret_cast<uint2 *>(xs + b * pitch + k * 2) = make_uint2(pack_bf16(v[j].x, v[j].y), pack_bf16(v[j].z, v[j].w));
                    }
            }
        }
        request_weights();   // waves without an activation row of this tile
        request_epilogue();
        stamp(1);
        __syncthreads();
        stamp(2);
        // 3. MFMA over this wave's K slice; batch columns >= nb read row 0 (their outputs are never stored)
        const unsigned char *xfrag = xs + (r < nb ? r : 0) * pitch + (kbase + 8 * q) * 2;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < nch; c0 += 8) {
            uint4 wn[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) {  // next batch of weight fragments (none when NW covers K in one batch)
                wn[c] = make_uint4(0, 0, 0, 0);
                if constexpr (NW * 256 < SKM_MAXK)
                    if (c0 + 8 + c < nch && row_ok) wn[c] = a.w_cached ? *reinterpret_cast<const uint4 *>(Wrow + 32 * (c0 + 8 + c)) : ld_nt16(Wrow + 32 * (c0 + 8 + c));
            }
#pragma unroll
            for (int c = 0; c < 8; ++c)
                if (c0 + c < nch) {
                    const uint4 xf = *reinterpret_cast<const uint4 *>(xfrag + 64 * (c0 + c));
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf[c]), __builtin_bit_cast(bf16x8, xf), acc, 0, 0, 0);
                }
#pragma unroll
            for (int c = 0; c < 8; ++c) wf[c] = wn[c];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) red[wave * 256 + lane * 4 + i] = acc[i];
        stamp(3);
        __syncthreads();
        stamp(4);
        if (wave == 0) {
            // D layout: col (batch) = lane & 15, row (weight row) = 4 * (lane >> 4) + i
            const int b = bt + r;
            const bool col_ok = r < nb;
            const bool rnd = a.flags & ACAI_GEMM_ROUND_BF16;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = n0 + 4 * q + i;
                if (4 * q + i >= R || n >= a.N || !col_ok) continue;
                float v = e_bias[i];
#pragma unroll
                for (int w = 0; w < NW; ++w) v += red[w * 256 + lane * 4 + i];
                if (rnd) v = round_bf16(v);
                if (a.flags & ACAI_GEMM_GELU) {
                    v = gelu_erf(v);
                    if (rnd) v = round_bf16(v);
                }
                if (a.k_cache && n >= a.E) {
                    const int kv = (n - a.E) / a.E, e = (n - a.E) - kv * a.E, hh = e / a.dh, dd = e - hh * a.dh;
                    const size_t off = (((size_t)b * a.H + hh) * a.Tmax + a.step[1]) * a.dhp + dd;
                    reinterpret_cast<bf16_t *>(kv ? a.v_cache : a.k_cache)[off] = f2bf(v);
                }
                if (a.residual) v += a.rln_w ? (e_res[i] - rmean) * rrstd * e_rw[i] + e_rb[i] : e_res[i];
                if (a.y_bf16)
                    reinterpret_cast<bf16_t *>(a.y)[(size_t)b * a.ldy + n] = f2bf(v);
                else
                    a.y[(size_t)b * a.ldy + n] = v;
            }
        }
        stamp(5);
        __syncthreads();
    }
}

// ---- the decode chain's GEMV at its hot shapes (K = 256 * NW: K = 1024 fp32 or bf16 activations, K = 4096 bf16 activations) --------------
// Same arithmetic and fusions as skinny_mfma_kernel (bit-identical results), rebuilt around what in-kernel stamps showed on MI355X
// (tools/stamp_decode.py): of a 5-7 us launch, 2.7-5.2 us passed before the activation image was complete and ~1 us in the epilogue, because
//   * the compiler fetched the 200-byte argument struct in SIX dependent scalar-load stages (each a cold round trip after a kernel boundary):
//     here every argument is forced into SGPRs by one batch of s_loads and one wait;
//   * loads sat inside per-lane branches, so the first use of the activation rows waited with vmcnt(0) for the weight fragments (HBM) and the
//     epilogue operands as well: here every load is unconditional (clamped address, or a buffer load whose out-of-range lanes return zero), in
//     straight-line code, so the compiler's counted waits are exact - activations first, weights stay in flight across the barrier, epilogue
//     operands are requested after the barrier and land under the weight wait;
//   * one wave reduced and finished all 4 x 64 outputs: here wave i finishes accumulator register i of every lane (4 waves in parallel).
// Every chain form runs four waves.  At K = 4096 (linear2) a wave owns four of the sixteen K slices and keeps sixteen separate accumulator
// chains, so the bits are those of one wave per slice.  Per-wave stamps of the sixteen-wave form (profiles/decode_ingest_order_lin2_waves.txt)
// showed all sixteen waves entering within 0.2 us but their 4 KB chunks landing in four groups 0.6 us apart - waves 0-3, 4-7, 8-11, 12-15,
// one wave per SIMD in each group: a CU takes in the cold 64 KB image at ~27 GB/s whoever asks for it, and twelve waves idle at the barrier
// meanwhile.  Four waves with sixteen 1 KB requests each get the same image complete 0.2 us sooner and cost less to launch and to
// synchronise (kernel 4.6 -> 4.2 us).  Starting every workgroup of an XCD at another piece of the image did not change that rate.
typedef __attribute__((vector_size(16))) unsigned int skm_v4u;

// NW = K slices of 256 (one fp32 accumulator chain each, summed in slice order at the end); WV = waves, each owning NW / WV consecutive slices
template <bool XBF16, int LN, int NW, bool WFIRST = false, int WV = NW>   // LN: 0 = none, 1 = LayerNorm on load, 2 = two LayerNorms in a row (unembed: norm3 of the last layer, then the final norm)
__global__ __launch_bounds__(64 * WV) void skinny_chain_kernel(SkinnyArgs a) {
    constexpr bool HAS_LN = LN > 0;
    constexpr int K = 256 * NW, PITCH = K * 2 + 16, SPW = NW / WV;
    static_assert(NW % WV == 0 && WV >= 4, "whole slices per wave; waves 0..3 finish the outputs");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    asm volatile("" ::"s"(a.x), "s"(a.W), "s"(a.bias), "s"(a.residual), "s"(a.y), "s"(a.ldx), "s"(a.ldw), "s"(a.ldr), "s"(a.ldy), "s"(a.B), "s"(a.N),
                 "s"(a.flags), "s"(a.k_cache), "s"(a.v_cache), "s"(a.step));
    asm volatile("" ::"s"(a.E), "s"(a.H), "s"(a.dh), "s"(a.dhp), "s"(a.Tmax), "s"(a.ln_w), "s"(a.ln_b), "s"(a.ln_eps), "s"(a.stats_out), "s"(a.rln_w),
                 "s"(a.rln_b), "s"(a.rstats), "s"(a.y_bf16), "s"(a.rows_per_block), "s"(a.stamps));
    if constexpr (LN == 2) asm volatile("" ::"s"(a.ln2_w), "s"(a.ln2_b), "s"(a.ln2_eps));
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int R = a.rows_per_block, n0 = blockIdx.x * R, bt = blockIdx.y * 16;
    const int nb = min(16, a.B - bt);
    float *red = reinterpret_cast<float *>(smem);   // [NW][256]
    unsigned char *xs = smem + NW * 1024;           // [rows][PITCH] bf16 activation image
    auto stamp = [&](int k) {
        if (a.stamps && tid == 0) a.stamps[(size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 8 + k] = __builtin_amdgcn_s_memrealtime();
    };
    stamp(0);

    // weight fragments: lane (r, q) of wave w owns 8 x 16 B per slice of row n0 + r at k = 256 (SPW w + t) + 8 q + 32 c.  Buffer loads: lanes
    // without a row are out of range and read zeros - no branch.  Non-temporal: every weight byte is read once per step.
    const bool row_ok = r < R && n0 + r < a.N;
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.W), 0, (int)((size_t)a.N * a.ldw * 2), 0x00020000);
    const unsigned woff = row_ok ? (unsigned)(((size_t)(n0 + r) * a.ldw + wave * (256 * SPW) + 8 * q) * 2) : 0xFFF00000u;
    skm_v4u wf[8 * SPW];
    auto request_weights = [&]() {
#pragma unroll
        for (int c = 0; c < 8 * SPW; ++c) wf[c] = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, woff + 64 * c, 0, 2);
    };

    if constexpr (XBF16 && NW == 4) {
        // K = 1024, bf16 rows (the attention output as decode_attn_kernel stores it): the image is copied as it is, wave w takes rows w and
        // w + 4 (then w + 8, w + 12 when the tile has more than 8 rows), a row = two coalesced 1 KB loads.  A wave without a row copies row 0
        // again (same bytes to the same place) instead of branching around its loads.
        auto copy = [&](int ra, int rb, bool first) {
            const int ca = ra < nb ? ra : 0, cb = rb < nb ? rb : 0;
            const bf16_t *pa = reinterpret_cast<const bf16_t *>(a.x) + (size_t)(bt + ca) * a.ldx + lane * 8;
            const bf16_t *pb = reinterpret_cast<const bf16_t *>(a.x) + (size_t)(bt + cb) * a.ldx + lane * 8;
            const uint4 a0 = *reinterpret_cast<const uint4 *>(pa), a1 = *reinterpret_cast<const uint4 *>(pa + 512),
                        b0 = *reinterpret_cast<const uint4 *>(pb), b1 = *reinterpret_cast<const uint4 *>(pb + 512);
            __builtin_amdgcn_sched_barrier(0);
            if (first) request_weights();   // behind this wave's activation rows: loads return in issue order
            __builtin_amdgcn_sched_barrier(0);
            *reinterpret_cast<uint4 *>(xs + ca * PITCH + lane * 16) = a0;
            *reinterpret_cast<uint4 *>(xs + ca * PITCH + lane * 16 + 1024) = a1;
            *reinterpret_cast<uint4 *>(xs + cb * PITCH + lane * 16) = b0;
            *reinterpret_cast<uint4 *>(xs + cb * PITCH + lane * 16 + 1024) = b1;
        };
        copy(wave, wave + 4, true);
        if (nb > 8) copy(wave + 8, wave + 12, false);
    } else if constexpr (XBF16 && WV == 4) {
        // K = 4096 on four waves: a pass of the image (8 rows, 64 KB) is 8 x 8 pieces of 1 KB.  Wave w takes columns w and w + 4 of pieces in
        // every row: 16 coalesced loads per lane, all requested before the lane's 32 weight fragments.  A piece of a row the tile does not
        // have is the same column's piece of row 0 again (same bytes to the same place) instead of a branch around a load.
        static_assert(!(XBF16 && WV == 4) || K == 4096, "eight 1 KB pieces per row");
        const unsigned va_off = wave * 1024 + lane * 16, vb_off = va_off + 4096;   // byte offsets inside a row, global and LDS alike
        auto copy = [&](int pass, bool first) {
            skm_v4u x[16];   // (an array of uint4 went to scratch)
            int row[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                row[i] = pass * 8 + i < nb ? pass * 8 + i : 0;
                const unsigned char *xr = reinterpret_cast<const unsigned char *>(a.x) + (size_t)(bt + row[i]) * a.ldx * 2;
                x[2 * i] = *reinterpret_cast<const skm_v4u *>(xr + va_off);
                x[2 * i + 1] = *reinterpret_cast<const skm_v4u *>(xr + vb_off);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (first) request_weights();   // behind this wave's pieces: loads return in issue order
            __builtin_amdgcn_sched_barrier(0);   // all requests, then the first wait
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                *reinterpret_cast<skm_v4u *>(xs + row[i] * PITCH + va_off) = x[2 * i];
                *reinterpret_cast<skm_v4u *>(xs + row[i] * PITCH + vb_off) = x[2 * i + 1];
            }
        };
        copy(0, true);
        if (nb > 8) copy(1, false);
    } else if constexpr (XBF16) {
        // K = 4096 on sixteen waves (ACAI_SKINNY_INGEST=0, an A/B aid: a step launches the four-wave form above).  The [nb][K] image is
        // copied in half-row chunks (4 KB), wave w takes chunk w (and w + 16 when the tile has more than 8 rows): 4 loads in flight per wave.  A wave without a chunk copies chunk 0 again (same bytes
        // to the same place) instead of branching around its loads.
        auto copy = [&](int ch, bool first) {
            const int c = ch < 2 * nb ? ch : 0;
            const bf16_t *xr = reinterpret_cast<const bf16_t *>(a.x) + (size_t)(bt + (c >> 1)) * a.ldx + (c & 1) * (K / 2) + lane * 8;
            unsigned char *xd = xs + (c >> 1) * PITCH + ((c & 1) * (K / 2) + lane * 8) * 2;
            static_assert(!XBF16 || K == 4096, "four 16-byte pieces per lane and chunk");   // (named registers: an array here went to scratch)
            if (first && WFIRST) request_weights();   // A/B: the HBM round trip (long) requested ahead of the L2 one
            const uint4 x0 = *reinterpret_cast<const uint4 *>(xr), x1 = *reinterpret_cast<const uint4 *>(xr + 512),
                        x2 = *reinterpret_cast<const uint4 *>(xr + 1024), x3 = *reinterpret_cast<const uint4 *>(xr + 1536);
            if (first && !WFIRST) request_weights();
            __builtin_amdgcn_sched_barrier(0);
            *reinterpret_cast<uint4 *>(xd) = x0;
            *reinterpret_cast<uint4 *>(xd + 1024) = x1;
            *reinterpret_cast<uint4 *>(xd + 2048) = x2;
            *reinterpret_cast<uint4 *>(xd + 3072) = x3;
        };
        copy(wave, true);
        if (nb > 8) copy(wave + 16, false);
    } else {
        static_assert(XBF16 || NW == 4, "fp32 activations: K = 1024");
        // wave w builds rows w and w + 4 (then w + 8, w + 12 when the tile has more than 8 rows); lane takes 4 consecutive k per 256
        auto build = [&](int ra, int rb, bool first) {
            const bool oka = ra < nb, okb = rb < nb;
            const float *pa = a.x + (size_t)(bt + (oka ? ra : 0)) * a.ldx + lane * 4, *pb = a.x + (size_t)(bt + (okb ? rb : 0)) * a.ldx + lane * 4;
            float4 va[4], vb[4], lw[4], lb[4], lw2[4], lb2[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                va[j] = *reinterpret_cast<const float4 *>(pa + j * 256);
                vb[j] = *reinterpret_cast<const float4 *>(pb + j * 256);
            }
            if constexpr (HAS_LN) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    lw[j] = *reinterpret_cast<const float4 *>(a.ln_w + j * 256 + lane * 4);
                    lb[j] = *reinterpret_cast<const float4 *>(a.ln_b + j * 256 + lane * 4);
                }
            }
            if constexpr (LN == 2) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    lw2[j] = *reinterpret_cast<const float4 *>(a.ln2_w + j * 256 + lane * 4);
                    lb2[j] = *reinterpret_cast<const float4 *>(a.ln2_b + j * 256 + lane * 4);
                }
            }
            __builtin_amdgcn_sched_barrier(0);   // (without it hipcc hoisted the weight requests above the activation rows: -4 % tokens/s)
            if (first) request_weights();   // behind this wave's activation rows: loads return in issue order
            __builtin_amdgcn_sched_barrier(0);   // every load above is in flight before anything is waited for (hipcc otherwise sinks the LN / weight loads below the statistics)
            if constexpr (HAS_LN) {
                // both rows' sum and sum of squares ride the same 6 cross-lane steps; shifted one-pass variance (as skinny_mfma_kernel)
                const float p0 = skm_pivot(pa - lane * 4), p1 = skm_pivot(pb - lane * 4);
                skm_shift<4>(va, K, lane, p0);
                skm_shift<4>(vb, K, lane, p1);
                float t0 = 0.f, u0 = 0.f, t1 = 0.f, u1 = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    t0 += (va[j].x + va[j].y) + (va[j].z + va[j].w);
                    u0 += (va[j].x * va[j].x + va[j].y * va[j].y) + (va[j].z * va[j].z + va[j].w * va[j].w);
                    t1 += (vb[j].x + vb[j].y) + (vb[j].z + vb[j].w);
                    u1 += (vb[j].x * vb[j].x + vb[j].y * vb[j].y) + (vb[j].z * vb[j].z + vb[j].w * vb[j].w);
                }
                t0 = wave_sum_dpp(t0);   // four independent chains on the DPP network
                u0 = wave_sum_dpp(u0);
                t1 = wave_sum_dpp(t1);
                u1 = wave_sum_dpp(u1);
                const float invK = 1.0f / (float)K;
                const float m0 = t0 * invK, m1 = t1 * invK;
                const float s0 = 1.0f / sqrtf(fmaxf(u0 * invK - m0 * m0, 0.f) + a.ln_eps), s1 = 1.0f / sqrtf(fmaxf(u1 * invK - m1 * m1, 0.f) + a.ln_eps);
                if (lane == 0 && a.stats_out && blockIdx.x == 0) {
                    if (oka) {
                        a.stats_out[(bt + ra) * 2] = p0 + m0;
                        a.stats_out[(bt + ra) * 2 + 1] = s0;
                    }
                    if (okb) {
                        a.stats_out[(bt + rb) * 2] = p1 + m1;
                        a.stats_out[(bt + rb) * 2 + 1] = s1;
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    va[j].x = (va[j].x - m0) * s0 * lw[j].x + lb[j].x; va[j].y = (va[j].y - m0) * s0 * lw[j].y + lb[j].y;
                    va[j].z = (va[j].z - m0) * s0 * lw[j].z + lb[j].z; va[j].w = (va[j].w - m0) * s0 * lw[j].w + lb[j].w;
                    vb[j].x = (vb[j].x - m1) * s1 * lw[j].x + lb[j].x; vb[j].y = (vb[j].y - m1) * s1 * lw[j].y + lb[j].y;
                    vb[j].z = (vb[j].z - m1) * s1 * lw[j].z + lb[j].z; vb[j].w = (vb[j].w - m1) * s1 * lw[j].w + lb[j].w;
                }
            }
            if constexpr (LN == 2) {   // the second norm on the fp32 rows in registers (two-pass variance: the rows are O(1) after the first)
                float t0 = 0.f, t1 = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    t0 += (va[j].x + va[j].y) + (va[j].z + va[j].w);
                    t1 += (vb[j].x + vb[j].y) + (vb[j].z + vb[j].w);
                }
                const float invK = 1.0f / (float)K;
                const float m0 = wave_sum_dpp(t0) * invK, m1 = wave_sum_dpp(t1) * invK;
                float u0 = 0.f, u1 = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    va[j].x -= m0; va[j].y -= m0; va[j].z -= m0; va[j].w -= m0;
                    vb[j].x -= m1; vb[j].y -= m1; vb[j].z -= m1; vb[j].w -= m1;
                    u0 += (va[j].x * va[j].x + va[j].y * va[j].y) + (va[j].z * va[j].z + va[j].w * va[j].w);
                    u1 += (vb[j].x * vb[j].x + vb[j].y * vb[j].y) + (vb[j].z * vb[j].z + vb[j].w * vb[j].w);
                }
                const float s0 = 1.0f / sqrtf(wave_sum_dpp(u0) * invK + a.ln2_eps), s1 = 1.0f / sqrtf(wave_sum_dpp(u1) * invK + a.ln2_eps);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    va[j].x = va[j].x * s0 * lw2[j].x + lb2[j].x; va[j].y = va[j].y * s0 * lw2[j].y + lb2[j].y;
                    va[j].z = va[j].z * s0 * lw2[j].z + lb2[j].z; va[j].w = va[j].w * s0 * lw2[j].w + lb2[j].w;
                    vb[j].x = vb[j].x * s1 * lw2[j].x + lb2[j].x; vb[j].y = vb[j].y * s1 * lw2[j].y + lb2[j].y;
                    vb[j].z = vb[j].z * s1 * lw2[j].z + lb2[j].z; vb[j].w = vb[j].w * s1 * lw2[j].w + lb2[j].w;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int kb = (j * 256 + lane * 4) * 2;
                if (oka) *reinterpret_cast<uint2 *>(xs + ra * PITCH + kb) = make_uint2(pack_bf16(va[j].x, va[j].y), pack_bf16(va[j].z, va[j].w));
                if (okb) *reinterpret_cast<uint2 *>(xs + rb * PITCH + kb) = make_uint2(pack_bf16(vb[j].x, vb[j].y), pack_bf16(vb[j].z, vb[j].w));
            }
        };
        build(wave, wave + 4, true);
        if (nb > 8) build(wave + 8, wave + 12, false);
    }
    stamp(1);
    __syncthreads();
    stamp(2);

    // epilogue operands of the output this lane will finish (wave i < 4 finishes accumulator register i): requested now, used after the
    // reduction - they land while the weight fragments are waited for
    const int oi = wave & 3;
    const int on = n0 + 4 * q + oi, ob = bt + r;
    const bool out_ok = wave < 4 && 4 * q + oi < R && on < a.N && r < nb;
    float e_bias = 0.f, e_res = 0.f, e_rw = 1.f, e_rb = 0.f, rmean = 0.f, rrstd = 1.f;
    if (wave < 4) {
        const int cn = out_ok ? on : 0, cb = out_ok ? ob : 0;
        if (a.bias) e_bias = a.bias[cn];
        if (a.residual) e_res = a.residual[(size_t)cb * a.ldr + cn];
        if (a.rln_w) {
            e_rw = a.rln_w[cn];
            e_rb = a.rln_b[cn];
            rmean = a.rstats[cb * 2];
            rrstd = a.rstats[cb * 2 + 1];
        }
    }
    // MFMA over this wave's K slices, one accumulator chain of eight per slice; batch columns >= nb read row 0 (their outputs are never stored)
    const unsigned char *xfrag = xs + (r < nb ? r : 0) * PITCH + (wave * (256 * SPW) + 8 * q) * 2;
#pragma unroll
    for (int t = 0; t < SPW; ++t) {
        uint4 xf[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) xf[c] = *reinterpret_cast<const uint4 *>(xfrag + 512 * t + 64 * c);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 8; ++c)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf[8 * t + c]), __builtin_bit_cast(bf16x8, xf[c]), acc, 0, 0, 0);
        *reinterpret_cast<f32x4 *>(red + (wave * SPW + t) * 256 + lane * 4) = acc;
    }
    stamp(3);
    __syncthreads();
    stamp(4);
    if (wave < 4) {
        // D layout: col (batch) = lane & 15, row (weight row) = 4 * (lane >> 4) + register
        float v = e_bias;
#pragma unroll
        for (int w = 0; w < NW; ++w) v += red[w * 256 + lane * 4 + oi];
        const bool rnd = a.flags & ACAI_GEMM_ROUND_BF16;
        if (rnd) v = round_bf16(v);
        if (a.flags & ACAI_GEMM_GELU) {
            v = gelu_erf(v);
            if (rnd) v = round_bf16(v);
        }
        if (out_ok) {
            if (a.k_cache && on >= a.E) {   // KVCache.update (K:94-95): position = entries already cached
                const int kv = (on - a.E) / a.E, e = (on - a.E) - kv * a.E, hh = e / a.dh, dd = e - hh * a.dh;
                const size_t off = (((size_t)ob * a.H + hh) * a.Tmax + a.step[1]) * a.dhp + dd;
                reinterpret_cast<bf16_t *>(kv ? a.v_cache : a.k_cache)[off] = f2bf(v);
            }
            if (a.residual) v += a.rln_w ? (e_res - rmean) * rrstd * e_rw + e_rb : e_res;
            if (a.y_bf16)
                reinterpret_cast<bf16_t *>(a.y)[(size_t)ob * a.ldy + on] = f2bf(v);
            else
                a.y[(size_t)ob * a.ldy + on] = v;
        }
    }
    stamp(5);
}

}  // namespace

bool skinny_mfma_ok(const SkinnyArgs &a) {
    return (a.K % 256 == 0) && a.K <= SKM_MAXK && (a.ldw % 8 == 0) && (a.ldx % 8 == 0) && aligned16(a.W) && aligned16(a.x) &&
           (!a.ln_w || (aligned16(a.ln_w) && aligned16(a.ln_b)));
}

template <typename TW>
int launch_skinny(const SkinnyArgs &a, hipStream_t st) {
    if (a.x_bf16 && (a.ln_w || a.stats_out)) return acai_set_err(-1, "skinny_gemm: LayerNorm on load needs fp32 activations");
    if constexpr (sizeof(TW) == 2) {
        if (skinny_mfma_ok(a)) {
            const int rows = a.B < 16 ? ((a.B + 3) & ~3) : 16;
            const bool wide = a.x_bf16 && a.K == 4096;  // 16 K-slices: every weight fragment of the workgroup in flight at once
            const size_t lds = (wide ? 16 : 4) * 1024 + (size_t)rows * (a.K * 2 + 16);
            static bool attr_done[ACAI_MAX_DEV] = {};
            if (acai_first_on_device(attr_done)) {  // opt in to > 64 KB of dynamic LDS (K = 4096 activation image); per device
                hipFuncSetAttribute(reinterpret_cast<const void *>(skinny_mfma_kernel<false, 4, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
                hipFuncSetAttribute(reinterpret_cast<const void *>(skinny_mfma_kernel<false, 16, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
                hipFuncSetAttribute(reinterpret_cast<const void *>(skinny_mfma_kernel<true, 1, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
                hipFuncSetAttribute(reinterpret_cast<const void *>(skinny_mfma_kernel<true, 1, 16>), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
            }
            // one CU ingests only ~25 GB/s from HBM: spread a small weight matrix over >= ~200 workgroups by giving each
            // fewer than 16 rows (the unused MFMA rows load nothing)
            SkinnyArgs b = a;
            static const int rpb = getenv("ACAI_SKINNY_ROWS") ? atoi(getenv("ACAI_SKINNY_ROWS")) : 0;
            b.w_cached = 0;
            // weight cache policy (A/B aid): 0 = default-policy loads for every matrix, 2 = default policy below 8 MB (candidates for the
            // Infinity Cache across steps) and non-temporal above, unset = non-temporal everywhere
            static const int ntm = getenv("ACAI_SKINNY_NT") ? atoi(getenv("ACAI_SKINNY_NT")) : 1;
            if (ntm == 0 || (ntm == 2 && (size_t)a.N * a.K * 2 < (8u << 20))) b.w_cached = 1;
            b.rows_per_block = rpb ? rpb : (a.N >= 2560 ? 16 : (a.N >= 1600 ? 8 : 4));
            b.stamps = nullptr;
            if (g_stamps && g_stamp_next < g_stamp_cap) b.stamps = g_stamps + (size_t)(g_stamp_next++) * 1024 * 8;
            // (the K = 4096 form holds a 131 KB activation image: one workgroup per CU, so its batch tiles stay a loop inside the workgroup)
            static const bool no_chain = getenv("ACAI_SKINNY_CHAIN") && atoi(getenv("ACAI_SKINNY_CHAIN")) == 0;   // A/B aid
            const bool chain_ok = !no_chain && (size_t)a.N * a.ldw * 2 < 0xFFF00000u && (a.ldx % 8 == 0);   // (row statistics are only published with a LayerNorm on load, as in skinny_mfma_kernel)
            if (a.ln2_w && !(chain_ok && a.K == 1024 && !a.x_bf16 && a.ln_w)) return acai_set_err(-1, "skinny_gemm: the double LayerNorm needs the chain kernel (K = 1024, fp32 activations)");
            if (chain_ok && (a.K == 1024 || (a.K == 4096 && a.x_bf16))) {   // (bf16 activations never carry a LayerNorm on load: refused above)
                static bool attr2[ACAI_MAX_DEV] = {};
                if (acai_first_on_device(attr2)) {
                    hipFuncSetAttribute(reinterpret_cast<const void *>(skinny_chain_kernel<true, 0, 16>), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
                    hipFuncSetAttribute(reinterpret_cast<const void *>(skinny_chain_kernel<true, 0, 16, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
                    hipFuncSetAttribute(reinterpret_cast<const void *>(skinny_chain_kernel<true, 0, 16, false, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
                }
                const dim3 cgrid(cdiv(a.N, b.rows_per_block), cdiv(a.B, 16));
                const int nw = a.K == 4096 ? 16 : 4;
                const size_t clds = (size_t)nw * 1024 + (size_t)rows * (a.K * 2 + 16);
                static const bool wfirst = getenv("ACAI_LIN2_WFIRST") && atoi(getenv("ACAI_LIN2_WFIRST")) == 1;   // A/B aid
                // A/B aid: 0 = the K = 4096 form on sixteen waves (one K slice each), unset = on four waves (four slices each); same bits
                static const bool four_waves = !(getenv("ACAI_SKINNY_INGEST") && atoi(getenv("ACAI_SKINNY_INGEST")) == 0);
                if (a.x_bf16 && a.K == 1024)
                    hipLaunchKernelGGL((skinny_chain_kernel<true, 0, 4>), cgrid, dim3(256), clds, st, b);
                else if (a.x_bf16 && wfirst)
                    hipLaunchKernelGGL((skinny_chain_kernel<true, 0, 16, true>), cgrid, dim3(1024), clds, st, b);
                else if (a.x_bf16 && four_waves)
                    hipLaunchKernelGGL((skinny_chain_kernel<true, 0, 16, false, 4>), cgrid, dim3(256), clds, st, b);
                else if (a.x_bf16)
                    hipLaunchKernelGGL((skinny_chain_kernel<true, 0, 16>), cgrid, dim3(1024), clds, st, b);
                else if (a.ln_w && a.ln2_w)
                    hipLaunchKernelGGL((skinny_chain_kernel<false, 2, 4>), cgrid, dim3(256), clds, st, b);
                else if (a.ln_w)
                    hipLaunchKernelGGL((skinny_chain_kernel<false, 1, 4>), cgrid, dim3(256), clds, st, b);
                else
                    hipLaunchKernelGGL((skinny_chain_kernel<false, 0, 4>), cgrid, dim3(256), clds, st, b);
                ACAI_LAUNCH_CHECK("skinny_chain");
                return 0;
            }
            const dim3 grid(cdiv(a.N, b.rows_per_block), wide ? 1 : cdiv(a.B, 16));
            if (wide)
                hipLaunchKernelGGL((skinny_mfma_kernel<true, 1, 16>), grid, dim3(1024), lds, st, b);
            else if (a.x_bf16)
                hipLaunchKernelGGL((skinny_mfma_kernel<true, 1, 4>), grid, dim3(256), lds, st, b);
            else if (a.K <= 1024)
                hipLaunchKernelGGL((skinny_mfma_kernel<false, 4, 4>), grid, dim3(256), lds, st, b);
            else
                hipLaunchKernelGGL((skinny_mfma_kernel<false, 16, 4>), grid, dim3(256), lds, st, b);
            ACAI_LAUNCH_CHECK("skinny_mfma");
            return 0;
        }
    }
    if (a.ln_w || a.rln_w || a.x_bf16 || a.y_bf16) return acai_set_err(-1, "skinny_gemm: fused LayerNorm needs the bf16 MFMA path (K %% 128 == 0, 16-byte aligned operands)");
    constexpr int EPC = 16 / sizeof(TW);
    const bool fast = (a.K % EPC == 0) && (a.ldw % EPC == 0) && aligned16(a.W);
    dim3 grid(cdiv(a.N, 32));
    if (fast)
        hipLaunchKernelGGL((skinny_gemm_kernel<TW, true>), grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((skinny_gemm_kernel<TW, false>), grid, dim3(256), 0, st, a);
    ACAI_LAUNCH_CHECK("skinny_gemm");
    return 0;
}
template int launch_skinny<float>(const SkinnyArgs &, hipStream_t);
template int launch_skinny<bf16_t>(const SkinnyArgs &, hipStream_t);

// Stand-alone entry points for the module-level API (CachedMultiheadAttention.cached_forward K:123-140,
// F.linear on (B,1,E) K:193,215): the same kernels acai_decode_step chains.
extern "C" int acai_skinny_gemm(const float *x, int ldx, const void *W, int ldw, const float *bias, const float *residual, int ldr,
                                float *y, int ldy, int B, int N, int K, int dtype, int flags, void *stream) {
    ACAI_CHECK_ARG(x && W && y && B > 0 && N > 0 && K > 0 && ldx >= K && ldw >= K && ldy >= N, "acai_skinny_gemm: bad arguments");
    SkinnyArgs s{};
    s.x = x; s.W = W; s.bias = bias; s.residual = residual; s.y = y;
    s.ldx = ldx; s.ldw = ldw; s.ldr = ldr; s.ldy = ldy; s.B = B; s.N = N; s.K = K; s.flags = flags;
    if (dtype == ACAI_BF16) return launch_skinny<bf16_t>(s, (hipStream_t)stream);
    if (dtype == ACAI_F32) return launch_skinny<float>(s, (hipStream_t)stream);
    return acai_set_err(-1, "acai_skinny_gemm: bad dtype %d", dtype);
}

// The full option set of the decode GEMV (what acai_decode_step chains): LayerNorm on load, published row statistics,
// LayerNorm of the residual, bf16 activations in / out.  Exposed so that tests and micro-benchmarks can hit each fusion.
extern "C" int acai_skinny_gemm_ex(const void *x, int ldx, int x_dtype, const void *W, int ldw, const float *bias, const float *residual,
                                   int ldr, void *y, int ldy, int y_dtype, int B, int N, int K, int dtype, int flags, const float *ln_w,
                                   const float *ln_b, float ln_eps, float *stats_out, const float *rln_w, const float *rln_b,
                                   const float *rstats, void *stream) {
    ACAI_CHECK_ARG(x && W && y && B > 0 && N > 0 && K > 0 && ldx >= K && ldw >= K && ldy >= N, "acai_skinny_gemm_ex: bad arguments");
    ACAI_CHECK_ARG(!rln_w || (rln_b && rstats && residual), "acai_skinny_gemm_ex: residual LayerNorm needs weights, bias, statistics and a residual");
    SkinnyArgs s{};
    s.x = (const float *)x; s.W = W; s.bias = bias; s.residual = residual; s.y = (float *)y;
    s.ldx = ldx; s.ldw = ldw; s.ldr = ldr; s.ldy = ldy; s.B = B; s.N = N; s.K = K; s.flags = flags;
    s.ln_w = ln_w; s.ln_b = ln_b; s.ln_eps = ln_eps; s.stats_out = stats_out; s.rln_w = rln_w; s.rln_b = rln_b; s.rstats = rstats;
    s.x_bf16 = x_dtype == ACAI_BF16; s.y_bf16 = y_dtype == ACAI_BF16;
    if (dtype == ACAI_BF16) return launch_skinny<bf16_t>(s, (hipStream_t)stream);
    if (dtype == ACAI_F32) return launch_skinny<float>(s, (hipStream_t)stream);
    return acai_set_err(-1, "acai_skinny_gemm_ex: bad dtype %d", dtype);
}

// Diagnostic: from now on every MFMA skinny launch (up to cap_launches, 1024 workgroups each) writes s_memrealtime stamps of its stages
// into buf[launch][workgroup][8]; buf = NULL switches it off and rewinds the slot counter.  Not part of the product path.
extern "C" int acai_debug_stamps(void *buf, int cap_launches) {
    g_stamps = (unsigned long long *)buf;
    g_stamp_cap = buf ? cap_launches : 0;
    g_stamp_next = 0;
    return 0;
}
