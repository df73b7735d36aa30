// C[M,N] = epi(A[M,K] . W[N,K]^T + bias) (+ residual): the nn.Linear of every projection on the path
// (reference: acai_omr/models/models.py:29,57,204,205,428,655-660; kv_caching.py:193,215,244).
//
// gfx950 design: 128x128 block tile, 4 waves (2x2), each wave owns 64x64 = 2x2 MFMA 32x32 tiles in
// 64 accumulator VGPRs.  Both operands are K-contiguous ("NT"), which is exactly the MFMA A/B lane
// layout (lane (r,h) holds 8 consecutive k of row r), so A and W tiles are staged as 128-byte row
// segments (bf16: BK = 64, fp32: BK = 32) with a 144-byte LDS pitch: ds_read_b128 of 32 rows at one
// column offset is then bank-conflict free (36*r mod 64 distinct over each 16-lane group).
// bf16 -> v_mfma_f32_32x32x16_bf16; fp32 -> v_mfma_f32_32x32x2_f32 (exact fp32 fma chain; one
// ds_read_b128 feeds four K=2 MFMAs because lane-half h takes k = 8s+4h+j, j = 0..3).
// Global -> register prefetch of tile t+1 is issued before the MFMAs of tile t (issue-early /
// write-late staging), one LDS stage, ~3 workgroups per CU cover each other's barriers.
//
// This file: the register-staged kernel and the LDS-DMA kernels that run one output tile per workgroup.
#include "gemm_device.h"

namespace {

template <typename T, int EPI, bool FAST, bool TA = false, bool TB = false>
__global__ __launch_bounds__(256) void gemm_nt_kernel(GemmArgs g) {
    constexpr int EPC = 16 / sizeof(T);     // elements per 16-byte chunk
    constexpr int BK = ROWB / sizeof(T);    // k elements per tile
    // A transposed operand keeps its natural [k][128 rows] image in LDS (16-byte stores, no scatter); its MFMA fragments are
    // read with ds_read_b64_tr_b16 (bf16: two 4x16 transposing reads per fragment; pitch 320 B puts the 4 k-rows of both
    // 16-lane groups of a half-wave on disjoint banks) or one ds_read_b32 per K=2 MFMA (fp32).
    constexpr int PT = sizeof(T) == 2 ? 320 : 528;
    constexpr int SZA = TA ? BK * PT : BM * PITCH, SZB = TB ? BK * PT : BN * PITCH;
    __shared__ __attribute__((aligned(16))) unsigned char lds[SZA + SZB];
    unsigned char *ldsA = lds, *ldsB = lds + SZA;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int lr = lane & 31, lh = lane >> 5;

    // XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs, so give each XCD a
    // contiguous run of tiles along N (they share the same A panel in that XCD's L2).
    const int nbn = (g.N + BN - 1) / BN, nbm = (g.M + BM - 1) / BM;
    const int nwg = nbn * nbm;
    int pid = blockIdx.x;
    int kslice = 0;
    if (g.ksplit > 1) {
        kslice = pid / nwg;
        pid -= kslice * nwg;
    }
    {
        const int q = nwg / 8, r = nwg % 8, xcd = pid % 8, idx = pid / 8;
        pid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int bm0 = (pid / nbn) * BM, bn0 = (pid % nbn) * BN;

    const T *A = reinterpret_cast<const T *>(g.A);
    const T *W = reinterpret_cast<const T *>(g.W);

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    uint4 ra[4], rb[4];
    int nkt = (g.K + BK - 1) / BK, kt_begin = 0;
    if (g.ksplit > 1) {
        const int per = (nkt + g.ksplit - 1) / g.ksplit;
        kt_begin = kslice * per;
        nkt = min(nkt, kt_begin + per);
        if (kt_begin >= nkt) return;  // uniform per workgroup, before any barrier
    }

    // transposed staging: chunk c -> k index c / (128/EPC), row group c % (128/EPC) (consecutive lanes walk the contiguous dim)
    constexpr int RG = 128 / EPC;  // 16-byte row groups per 128-row tile
    auto load_tile = [&](int kt) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = tid + 256 * i, row = c >> 3, k0 = kt * BK + (c & 7) * EPC;
            if constexpr (TA) ra[i] = load_chunk_t<T, FAST>(A, g.lda, kt * BK + c / RG, g.K, bm0 + (c % RG) * EPC, g.M);
            else ra[i] = load_chunk<T, FAST>(A, g.lda, bm0 + row, g.M, k0, g.K);
            if constexpr (TB) rb[i] = load_chunk_t<T, FAST>(W, g.ldw, kt * BK + c / RG, g.K, bn0 + (c % RG) * EPC, g.N);
            else rb[i] = load_chunk<T, FAST>(W, g.ldw, bn0 + row, g.N, k0, g.K);
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = tid + 256 * i, row = c >> 3, cb = (c & 7) * 16;
            if constexpr (TA) *reinterpret_cast<uint4 *>(ldsA + (c / RG) * PT + (c % RG) * 16) = ra[i];
            else *reinterpret_cast<uint4 *>(ldsA + row * PITCH + cb) = ra[i];
            if constexpr (TB) *reinterpret_cast<uint4 *>(ldsB + (c / RG) * PT + (c % RG) * 16) = rb[i];
            else *reinterpret_cast<uint4 *>(ldsB + row * PITCH + cb) = rb[i];
        }
    };

    // fragment of 32 rows starting at `rowbase`, k-step s (bf16: k = 16s + 8h + j; fp32: k = 8s + 4h + e), from a row-major image
    // (ds_read_b128) or from a transposed operand's natural image
    auto frag = [&](const unsigned char *img, bool trans, int rowbase, int s) -> uint4 {
        if (!trans) return *reinterpret_cast<const uint4 *>(img + (rowbase + lr) * PITCH + s * 32 + lh * 16);
        if constexpr (sizeof(T) == 2) {
            typedef __attribute__((ext_vector_type(4))) short s4;
            typedef __attribute__((address_space(3))) s4 *lds_s4;
            const int i16 = lane & 15, g1 = (lane >> 4) & 1;  // lane 4q+p of a 16-lane group addresses row q, columns 4p..4p+3
            const unsigned char *p0 = img + (16 * s + 8 * lh + (i16 >> 2)) * PT + (rowbase + 16 * g1 + 4 * (i16 & 3)) * 2;
            const s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(p0));
            const s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(p0 + 4 * PT));
            union { s4 v[2]; uint4 u; } r;
            r.v[0] = lo;
            r.v[1] = hi;
            return r.u;
        } else {
            const unsigned char *p0 = img + (8 * s + 4 * lh) * PT + (rowbase + lr) * 4;
            uint4 r;
            r.x = *reinterpret_cast<const uint32_t *>(p0);
            r.y = *reinterpret_cast<const uint32_t *>(p0 + PT);
            r.z = *reinterpret_cast<const uint32_t *>(p0 + 2 * PT);
            r.w = *reinterpret_cast<const uint32_t *>(p0 + 3 * PT);
            return r;
        }
    };

    load_tile(kt_begin);
    store_tile();
    __syncthreads();
    for (int kt = kt_begin; kt < nkt; ++kt) {
        if (kt + 1 < nkt) load_tile(kt + 1);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            uint4 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[i] = frag(ldsA, TA, wm * 64 + i * 32, s);
                fb[i] = frag(ldsB, TB, wn * 64 + i * 32, s);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if constexpr (sizeof(T) == 2) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[i]),
                                                                            __builtin_bit_cast(bf16x8, fb[j]), acc[i][j], 0, 0, 0);
                    } else {
                        const f32x4 a4 = __builtin_bit_cast(f32x4, fa[i]), b4 = __builtin_bit_cast(f32x4, fb[j]);
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], b4[e], acc[i][j], 0, 0, 0);
                    }
                }
        }
        __syncthreads();
        if (kt + 1 < nkt) {
            store_tile();
            __syncthreads();
        }
    }

    if constexpr (EPI == 0 && TA && TB) {
        if (g.ksplit > 0) {
            gemm_accum_epilogue(g, acc, bm0, bn0, wm, wn, lr, lh);
            return;
        }
    }
    gemm_epilogue<EPI, TA && TB>(g, acc, bm0, bn0, wm, wn, lr, lh);
}

// ---- NT main loop with direct-to-LDS staging (global_load_lds, 16 B per lane) ------------------------------------------------
// For row-major operands with K % BK == 0: no staging VGPRs, two LDS stages (64 KB), tile t+1 in flight while tile t feeds the MFMAs,
// one barrier per K-step.  An LDS-DMA wave instruction writes 1 KiB linearly (lane l -> base + 16 l = row l/8, slot l%8 of an unpadded
// 128-byte row), so the bank-conflict fix is an XOR swizzle applied on BOTH sides: lane l fetches the global chunk (l%8) ^ ((row/2)%8) and
// the fragment read of logical chunk c goes to slot c ^ ((row/2)%8).  Rows beyond M / N are clamped (their outputs are never stored).
// WM = waves along M: 2 -> 128x128 tile, 4 waves (two workgroups per CU); 4 -> 256x128 tile, 8 waves (one workgroup per CU).  A CU takes in
// only ~55 GB/s through the LDS-DMA path, which caps the 128x128 tile (64 flop per staged byte) near 0.9 PF; the 256-row tile stages
// 25 % fewer bytes per flop and is used whenever it still yields >= 2 tiles per CU.
template <typename T, int EPI, int WM>
__global__ __launch_bounds__(WM * 128) __attribute__((amdgpu_waves_per_eu(2))) void gemm_nt_glds_kernel(GemmArgs g) {
    constexpr int BK = ROWB / sizeof(T);
    constexpr int BMT = WM * 64, NW = WM * 2;          // tile rows, waves
    constexpr int GA = BMT / 8 / NW, GW = BN / 8 / NW;  // 8-row groups (1 KiB LDS-DMA instructions) per wave and K-step: A, W
    constexpr int STAGE = (BMT + BN) * ROWB;           // 32 / 48 KB
    // Two DISTINCT LDS objects, addressed statically (the K loop is unrolled by two): the compiler's wait-count pass can then prove that
    // the fragment reads of one stage do not alias the LDS-DMA in flight into the other.  With one array and a run-time stage index it
    // put `s_waitcnt vmcnt(0)` in front of the first ds_read of every K-step, i.e. it drained tile t+1 before computing tile t.
    __shared__ __attribute__((aligned(16))) unsigned char lds0[STAGE];
    __shared__ __attribute__((aligned(16))) unsigned char lds1[STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, lr = lane & 31, lh = lane >> 5;
    const int nbn = (g.N + BN - 1) / BN, nbm = (g.M + BMT - 1) / BMT, nwg = nbn * nbm;
    int pid = blockIdx.x;
    {
        const int q = nwg / 8, r = nwg % 8, xcd = pid % 8, idx = pid / 8;
        pid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int bm0 = (pid / nbn) * BMT, bn0 = (pid % nbn) * BN;
    const T *A = reinterpret_cast<const T *>(g.A);
    const T *W = reinterpret_cast<const T *>(g.W);
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    // this lane's source chunk inside an 8-row group: row l/8; the 16-byte slot is XORed with bits 1..3 of the tile row (see SWZ below)
    const int grow = lane >> 3;
    const T *srcA[GA], *srcW[GW];
#pragma unroll
    for (int i = 0; i < GA; ++i) {
        const int row = (wave * GA + i) * 8 + grow;
        const int gslot = (lane & 7) ^ ((row >> 1) & 7);
        srcA[i] = A + (size_t)min(bm0 + row, g.M - 1) * g.lda + gslot * (16 / sizeof(T));
    }
#pragma unroll
    for (int i = 0; i < GW; ++i) {
        const int row = (wave * GW + i) * 8 + grow;
        const int gslot = (lane & 7) ^ ((row >> 1) & 7);
        srcW[i] = W + (size_t)min(bn0 + row, g.N - 1) * g.ldw + gslot * (16 / sizeof(T));
    }
    typedef __attribute__((address_space(3))) void *lds_ptr;
    typedef const __attribute__((address_space(1))) void *glb_ptr;
    auto issue = [&](int kt, unsigned char *base) {
#pragma unroll
        for (int i = 0; i < GA; ++i)
            __builtin_amdgcn_global_load_lds((glb_ptr)(srcA[i] + (size_t)kt * BK), (lds_ptr)(base + (wave * GA + i) * 1024), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < GW; ++i)
            __builtin_amdgcn_global_load_lds((glb_ptr)(srcW[i] + (size_t)kt * BK), (lds_ptr)(base + BMT * ROWB + (wave * GW + i) * 1024), 16, 0, 0);
    };
    // Fragment read of logical 16-byte chunk c of tile row r goes to slot c ^ ((r >> 1) & 7).  A 256-byte bank row holds two tile rows, and a
    // ds_read_b128 is served 16 lanes (= 16 consecutive tile rows, one k-half) per cycle: bit 0 of r picks the half of the bank row, bits 1..3 the
    // slot inside it, so the 16 lanes hit 16 different 16-byte bank groups (slot ^ (r & 7) paired rows r and r + 8: 2-way conflicts).
    // Fragments are double-buffered: the reads of k-slice s+1 are issued before the MFMAs of slice s.
    auto compute = [&](const unsigned char *sa) {
        const unsigned char *sb = sa + BMT * ROWB;
        uint4 fa[2][2], fb[2][2];
        auto frags = [&](int s, uint4 (&xa)[2], uint4 (&xb)[2]) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int ra = wm * 64 + i * 32 + lr, rb = wn * 64 + i * 32 + lr;
                xa[i] = *reinterpret_cast<const uint4 *>(sa + ra * ROWB + (((s * 2 + lh) ^ ((ra >> 1) & 7)) << 4));
                xb[i] = *reinterpret_cast<const uint4 *>(sb + rb * ROWB + (((s * 2 + lh) ^ ((rb >> 1) & 7)) << 4));
            }
        };
        frags(0, fa[0], fb[0]);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if (s + 1 < 4) frags(s + 1, fa[(s + 1) & 1], fb[(s + 1) & 1]);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if constexpr (sizeof(T) == 2) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[s & 1][i]), __builtin_bit_cast(bf16x8, fb[s & 1][j]), acc[i][j], 0, 0, 0);
                    } else {
                        const f32x4 a4 = __builtin_bit_cast(f32x4, fa[s & 1][i]), b4 = __builtin_bit_cast(f32x4, fb[s & 1][j]);
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], b4[e], acc[i][j], 0, 0, 0);
                    }
                }
        }
    };
    const int nkt = g.K / BK;
    issue(0, lds0);
    __syncthreads();  // with an LDS-DMA in flight this is s_waitcnt vmcnt(0) + s_barrier
    int kt = 0;
    for (; kt + 2 <= nkt; kt += 2) {
        issue(kt + 1, lds1);
        compute(lds0);
        __syncthreads();  // tile kt+1 has landed (vmcnt(0)) and every wave is done reading stage 0
        if (kt + 2 < nkt) issue(kt + 2, lds0);
        compute(lds1);
        __syncthreads();
    }
    if (kt < nkt) {  // odd tile count: the last tile sits in stage 0
        compute(lds0);
        __syncthreads();
    }
    // ---- epilogue (see gemm_vec_epilogue) ------------------------------------------------------------------------------------------------
    if (EPI != 0 || !g.vec_epi) {
        gemm_epilogue<EPI, false>(g, acc, bm0, bn0, wm, wn, lr, lh);
        return;
    }
    // every wave is past the last barrier: both stages are free; a wave stages 32 rows x 68 floats = 8.5 KB
    float *stg = reinterpret_cast<float *>((wave < WM ? lds0 : lds1) + (wave % WM) * (STAGE / WM));
    gemm_vec_epilogue<32>(g, acc, stg, bm0, bn0, wm, wn, lane);
}

// ---- 256x128 tile, 8 waves, THREE LDS stages (144 KB): two K-tiles in flight ------------------------------------------------------------
// The two-stage kernels are latency-bound, not MFMA-bound (PMC: MFMA busy 36 %, a third of the wave cycles in s_waitcnt, L2 hit rate 64 %):
// with one tile in flight per workgroup a CU has 64 KB outstanding, and 64 KB x 256 CUs / ~1.2 us of loaded L2/fabric latency is exactly the
// ~13.7 TB/s staging rate observed at 0.88 PF.  Throughput = (bytes in flight) x (flop per staged byte) / latency, so this variant keeps
// 2 x 48 KB in flight per CU on a tile with 1.33x the flop per byte.  One barrier per K-step:
//     s_waitcnt vmcnt(6)   this wave's six LDS-DMA instructions of tile t have landed (those of t+1 may still fly)
//     s_barrier            everybody's have; and everybody is done reading tile t-1, whose stage is reused next
//     issue tile t+2 -> stage (t+2) % 3;  MFMAs of tile t from stage t % 3
// (wait and barrier are one asm block: the fence inside __syncthreads() would drain vmcnt to 0).
template <typename T, int EPI>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2))) void gemm_nt_glds3_kernel(GemmArgs g) {
    constexpr int WM = 4;
    constexpr int BK = ROWB / sizeof(T);
    constexpr int BMT = WM * 64, NW = WM * 2;          // tile rows, waves
    constexpr int GA = BMT / 8 / NW, GW = BN / 8 / NW;  // 8-row groups (1 KiB LDS-DMA instructions) per wave and K-step: A, W
    constexpr int STAGE = (BMT + BN) * ROWB;           // 32 / 48 KB
    // DISTINCT LDS objects, addressed statically (the K loop is unrolled by the stage count): the compiler's wait-count pass can then prove that
    // the fragment reads of one stage do not alias the LDS-DMA in flight into the other.  With one array and a run-time stage index it
    // put `s_waitcnt vmcnt(0)` in front of the first ds_read of every K-step, i.e. it drained tile t+1 before computing tile t.
    __shared__ __attribute__((aligned(16))) unsigned char lds0[STAGE];
    __shared__ __attribute__((aligned(16))) unsigned char lds1[STAGE];
    __shared__ __attribute__((aligned(16))) unsigned char lds2[STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, lr = lane & 31, lh = lane >> 5;
    const int nbn = (g.N + BN - 1) / BN, nbm = (g.M + BMT - 1) / BMT, nwg = nbn * nbm;
    int pid = blockIdx.x;
    {
        const int q = nwg / 8, r = nwg % 8, xcd = pid % 8, idx = pid / 8;
        pid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int bm0 = (pid / nbn) * BMT, bn0 = (pid % nbn) * BN;
    const T *A = reinterpret_cast<const T *>(g.A);
    const T *W = reinterpret_cast<const T *>(g.W);
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    // this lane's source chunk inside an 8-row group: row l/8; the 16-byte slot is XORed with bits 1..3 of the tile row (see SWZ below)
    const int grow = lane >> 3;
    const T *srcA[GA], *srcW[GW];
#pragma unroll
    for (int i = 0; i < GA; ++i) {
        const int row = (wave * GA + i) * 8 + grow;
        const int gslot = (lane & 7) ^ ((row >> 1) & 7);
        srcA[i] = A + (size_t)min(bm0 + row, g.M - 1) * g.lda + gslot * (16 / sizeof(T));
    }
#pragma unroll
    for (int i = 0; i < GW; ++i) {
        const int row = (wave * GW + i) * 8 + grow;
        const int gslot = (lane & 7) ^ ((row >> 1) & 7);
        srcW[i] = W + (size_t)min(bn0 + row, g.N - 1) * g.ldw + gslot * (16 / sizeof(T));
    }
    typedef __attribute__((address_space(3))) void *lds_ptr;
    typedef const __attribute__((address_space(1))) void *glb_ptr;
    // The LDS-DMA instructions are issued from inline asm: the compiler's wait-count pass tracks only a few LDS-DMA writers and, past that,
    // guards every LDS read with s_waitcnt vmcnt(0) - which would drain the two tiles in flight.  Hidden from it, the only vmcnt waits in the
    // loop are the counted ones below (no other vector-memory instruction is issued between the prologue and the epilogue).
    auto issue = [&](int kt, unsigned char *base) {
        const uint32_t lbase = (uint32_t)(uintptr_t)(lds_ptr)base;
#pragma unroll
        for (int i = 0; i < GA; ++i) {
            const uint32_t dst = __builtin_amdgcn_readfirstlane(lbase + (wave * GA + i) * 1024);
            glds16(dst, srcA[i] + (size_t)kt * BK);
        }
#pragma unroll
        for (int i = 0; i < GW; ++i) {
            const uint32_t dst = __builtin_amdgcn_readfirstlane(lbase + BMT * ROWB + (wave * GW + i) * 1024);
            glds16(dst, srcW[i] + (size_t)kt * BK);
        }
    };
    // Fragment read of logical 16-byte chunk c of tile row r goes to slot c ^ ((r >> 1) & 7).  A 256-byte bank row holds two tile rows, and a
    // ds_read_b128 is served 16 lanes (= 16 consecutive tile rows, one k-half) per cycle: bit 0 of r picks the half of the bank row, bits 1..3 the
    // slot inside it, so the 16 lanes hit 16 different 16-byte bank groups (slot ^ (r & 7) paired rows r and r + 8: 2-way conflicts).
    // Fragments are double-buffered: the reads of k-slice s+1 are issued before the MFMAs of slice s.
    auto compute = [&](const unsigned char *sa) {
        const unsigned char *sb = sa + BMT * ROWB;
        uint4 fa[2][2], fb[2][2];
        auto frags = [&](int s, uint4 (&xa)[2], uint4 (&xb)[2]) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int ra = wm * 64 + i * 32 + lr, rb = wn * 64 + i * 32 + lr;
                xa[i] = *reinterpret_cast<const uint4 *>(sa + ra * ROWB + (((s * 2 + lh) ^ ((ra >> 1) & 7)) << 4));
                xb[i] = *reinterpret_cast<const uint4 *>(sb + rb * ROWB + (((s * 2 + lh) ^ ((rb >> 1) & 7)) << 4));
            }
        };
        frags(0, fa[0], fb[0]);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if (s + 1 < 4) frags(s + 1, fa[(s + 1) & 1], fb[(s + 1) & 1]);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if constexpr (sizeof(T) == 2) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[s & 1][i]), __builtin_bit_cast(bf16x8, fb[s & 1][j]), acc[i][j], 0, 0, 0);
                    } else {
                        const f32x4 a4 = __builtin_bit_cast(f32x4, fa[s & 1][i]), b4 = __builtin_bit_cast(f32x4, fb[s & 1][j]);
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], b4[e], acc[i][j], 0, 0, 0);
                    }
                }
        }
    };
    static_assert(GA + GW == 6, "the counted wait below assumes six LDS-DMA instructions per wave and tile");
    const int nkt = g.K / BK;
    issue(0, lds0);
    if (nkt > 1) issue(1, lds1);
    auto step = [&](int kt, const unsigned char *cur, unsigned char *nxt2) {
        if (kt + 1 < nkt)
            asm volatile("s_waitcnt vmcnt(6)\n\ts_barrier" ::: "memory");
        else
            asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        if (kt + 2 < nkt) issue(kt + 2, nxt2);
        compute(cur);
    };
    for (int kt = 0; kt < nkt; kt += 3) {
        step(kt, lds0, lds2);
        if (kt + 1 < nkt) step(kt + 1, lds1, lds0);
        if (kt + 2 < nkt) step(kt + 2, lds2, lds1);
    }
    __syncthreads();  // all tiles consumed, nothing in flight: the stages become the epilogue's staging space
    // ---- epilogue (see gemm_vec_epilogue) ------------------------------------------------------------------------------------------------
    if (EPI != 0 || !g.vec_epi) {
        gemm_epilogue<EPI, false>(g, acc, bm0, bn0, wm, wn, lr, lh);
        return;
    }
    // every wave is past the last barrier: both stages are free; a wave stages 32 rows x 68 floats = 8.5 KB
    float *stg = reinterpret_cast<float *>((wave < WM ? lds0 : lds1) + (wave % WM) * (STAGE / WM));
    gemm_vec_epilogue<32>(g, acc, stg, bm0, bn0, wm, wn, lane);
}

// ---- 256x256 tile, 8 waves x (128 x 64), two 64 KB LDS-DMA stages -----------------------------------------------------------------------
// A CU takes in at most ~60-70 GB/s through the LDS-DMA path.  A 256x128 K-step stages 48 KB for 1024 MFMA cycles per SIMD (~0.54 us at
// 1.9 GHz): 89 GB/s would be needed, so those kernels run staging-bound at ~45 % MFMA utilisation however deep the ring is.  The 256x256
// tile stages 64 KB for 2048 MFMA cycles (59 GB/s): the first shape on which the matrix cores, not the staging path, can set the pace.
template <typename T, int EPI>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2))) void gemm_nt_256_kernel(GemmArgs g) {
    constexpr int BK = ROWB / sizeof(T);
    constexpr int BT = 256, STAGE = 2 * BT * ROWB;   // 64 KB: A image (256 rows) then W image (256 rows)
    __shared__ __attribute__((aligned(16))) unsigned char lds0[STAGE];
    __shared__ __attribute__((aligned(16))) unsigned char lds1[STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3, lr = lane & 31, lh = lane >> 5;
    const int nbn = (g.N + BT - 1) / BT, nbm = (g.M + BT - 1) / BT, nwg = nbn * nbm;
    int pid = blockIdx.x;
    {
        const int q = nwg / 8, r = nwg % 8, xcd = pid % 8, idx = pid / 8;
        pid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int bm0 = (pid / nbn) * BT, bn0 = (pid % nbn) * BT;
    const T *A = reinterpret_cast<const T *>(g.A);
    const T *W = reinterpret_cast<const T *>(g.W);
    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    const int grow = lane >> 3;
    const T *srcA[4], *srcW[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = (wave * 4 + i) * 8 + grow, gslot = (lane & 7) ^ ((row >> 1) & 7);
        srcA[i] = A + (size_t)min(bm0 + row, g.M - 1) * g.lda + gslot * (16 / sizeof(T));
        srcW[i] = W + (size_t)min(bn0 + row, g.N - 1) * g.ldw + gslot * (16 / sizeof(T));
    }
    typedef __attribute__((address_space(3))) void *lds_ptr;
    typedef const __attribute__((address_space(1))) void *glb_ptr;
    auto issue = [&](int kt, unsigned char *base) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            __builtin_amdgcn_global_load_lds((glb_ptr)(srcA[i] + (size_t)kt * BK), (lds_ptr)(base + (wave * 4 + i) * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((glb_ptr)(srcW[i] + (size_t)kt * BK), (lds_ptr)(base + BT * ROWB + (wave * 4 + i) * 1024), 16, 0, 0);
        }
    };
    auto compute = [&](const unsigned char *sa) {
        const unsigned char *sb = sa + BT * ROWB;
        uint4 fa[2][4], fb[2][2];
        auto frags = [&](int s, uint4 (&xa)[4], uint4 (&xb)[2]) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int ra = wm * 128 + i * 32 + lr;
                xa[i] = *reinterpret_cast<const uint4 *>(sa + ra * ROWB + (((s * 2 + lh) ^ ((ra >> 1) & 7)) << 4));
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int rb = wn * 64 + j * 32 + lr;
                xb[j] = *reinterpret_cast<const uint4 *>(sb + rb * ROWB + (((s * 2 + lh) ^ ((rb >> 1) & 7)) << 4));
            }
        };
        frags(0, fa[0], fb[0]);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if (s + 1 < 4) frags(s + 1, fa[(s + 1) & 1], fb[(s + 1) & 1]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if constexpr (sizeof(T) == 2) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[s & 1][i]), __builtin_bit_cast(bf16x8, fb[s & 1][j]), acc[i][j], 0, 0, 0);
                    } else {
                        const f32x4 a4 = __builtin_bit_cast(f32x4, fa[s & 1][i]), b4 = __builtin_bit_cast(f32x4, fb[s & 1][j]);
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], b4[e], acc[i][j], 0, 0, 0);
                    }
                }
        }
    };
    const int nkt = g.K / BK;
    issue(0, lds0);
    __syncthreads();
    int kt = 0;
    for (; kt + 2 <= nkt; kt += 2) {
        issue(kt + 1, lds1);
        compute(lds0);
        __syncthreads();
        if (kt + 2 < nkt) issue(kt + 2, lds0);
        compute(lds1);
        __syncthreads();
    }
    if (kt < nkt) {
        compute(lds0);
        __syncthreads();
    }
    // epilogue: the wave's 128 x 64 block as two 64 x 64 halves through the shared routines (constant indices only: a run-time index
    // into acc would push all 128 accumulator registers to scratch)
    auto epi_half = [&](auto ihc) {
        constexpr int ih = decltype(ihc)::value;
        f32x16 half[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) half[i][j] = acc[2 * ih + i][j];
        const int bmh = bm0 + wm * 128 + ih * 64;
        if (EPI != 0 || !g.vec_epi) {
            gemm_epilogue<EPI, false>(g, half, bmh, bn0, 0, wn, lr, lh);
        } else {
            float *stg = reinterpret_cast<float *>((wave < 4 ? lds0 : lds1) + (wave & 3) * (STAGE / 4));
            gemm_vec_epilogue<32>(g, half, stg, bmh, bn0, 0, wn, lane);
        }
    };
    epi_half(std::integral_constant<int, 0>{});
    epi_half(std::integral_constant<int, 1>{});
}

template <typename T, int EPI, bool TA, bool TB>
void launch_reg(const AcaiGemmLaunch &l, const GemmArgs &g, hipStream_t st) {
    if (l.fast) hipLaunchKernelGGL((gemm_nt_kernel<T, EPI, true, TA, TB>), dim3(l.grid), dim3(l.block), 0, st, g);
    else hipLaunchKernelGGL((gemm_nt_kernel<T, EPI, false, TA, TB>), dim3(l.grid), dim3(l.block), 0, st, g);
}

template <typename T, int EPI>
void launch_tile(const AcaiGemmLaunch &l, bool ta, bool tb, const GemmArgs &g, hipStream_t st) {
    const dim3 grid(l.grid), block(l.block);
    switch (l.kernel) {
        case ACAI_GEMM_K_GLDS:
            if (l.wm == 4) hipLaunchKernelGGL((gemm_nt_glds_kernel<T, EPI, 4>), grid, block, 0, st, g);
            else hipLaunchKernelGGL((gemm_nt_glds_kernel<T, EPI, 2>), grid, block, 0, st, g);
            break;
        case ACAI_GEMM_K_GLDS3: hipLaunchKernelGGL((gemm_nt_glds3_kernel<T, EPI>), grid, block, 0, st, g); break;
        case ACAI_GEMM_K_256: hipLaunchKernelGGL((gemm_nt_256_kernel<T, EPI>), grid, block, 0, st, g); break;
        default:   // ACAI_GEMM_K_REG: the one kernel that takes transposed operands (plain epilogue only)
            if constexpr (EPI == 0) {
                if (ta && tb) return launch_reg<T, EPI, true, true>(l, g, st);
                if (ta) return launch_reg<T, EPI, true, false>(l, g, st);
                if (tb) return launch_reg<T, EPI, false, true>(l, g, st);
            }
            launch_reg<T, EPI, false, false>(l, g, st);
    }
}

}  // namespace

void gemm_launch_tile(const AcaiGemmLaunch &l, int elem_size, int epi, bool trans_a, bool trans_w, const GemmArgs &g, hipStream_t st) {
    if (elem_size == 2) epi ? launch_tile<bf16_t, 1>(l, trans_a, trans_w, g, st) : launch_tile<bf16_t, 0>(l, trans_a, trans_w, g, st);
    else epi ? launch_tile<float, 1>(l, trans_a, trans_w, g, st) : launch_tile<float, 0>(l, trans_a, trans_w, g, st);
}
