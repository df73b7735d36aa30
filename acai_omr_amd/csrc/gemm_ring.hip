// GEMM kernels whose LDS-DMA ring runs across output tiles (persistent, one workgroup per CU) and the weight-gradient kernels on the
// two-stage / three-stage staging (C = A . W^T family of gemm.hip; tile constants and GemmArgs: gemm_internal.h).
#include "gemm_device.h"

namespace {

// ---- dW = dY^T . X with direct-to-LDS staging (bf16) ----------------------------------------------------------------------------------
// Both operands are stored contraction-major ([Kc][M] and [Kc][N], Kc = tokens): a K-step stages 64 token rows x 128 columns of each in its
// natural image (256-byte rows, four rows per 1 KiB LDS-DMA instruction) and the MFMA fragments - eight consecutive tokens of one column -
// come from ds_read_b64_tr_b16.  A transposing read covers 4 token rows x 64 bytes per 32 lanes; with 256-byte rows those four rows share
// their banks, so the 64-byte block index is XORed with (token row & 3) on both sides (DMA source address / fragment address).  Two LDS
// stages as distinct objects, split-K over the tokens with fp32 atomics into the gradient (as the register-staged form it replaces, which
// ran at ~0.4 PF with one stage and two barriers per K-step).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void gemm_tn_glds_kernel(GemmArgs g) {
    typedef bf16_t T;
    constexpr int BKT = 64, STAGE = 2 * BKT * 256;  // 32 KB: A image then W image
    __shared__ __attribute__((aligned(16))) unsigned char lds0[STAGE];
    __shared__ __attribute__((aligned(16))) unsigned char lds1[STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, lr = lane & 31, lh = lane >> 5;
    const int nbn = (g.N + BN - 1) / BN, nbm = (g.M + BM - 1) / BM, nwg = nbn * nbm;
    int pid = blockIdx.x, kslice = 0;
    if (g.ksplit > 1) {
        kslice = pid / nwg;
        pid -= kslice * nwg;
    }
    {
        const int q = nwg / 8, r = nwg % 8, xcd = pid % 8, idx = pid / 8;
        pid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int bm0 = (pid / nbn) * BM, bn0 = (pid % nbn) * BN;
    int nkt = g.K / BKT, kt_begin = 0;
    if (g.ksplit > 1) {
        const int per = (nkt + g.ksplit - 1) / g.ksplit;
        kt_begin = kslice * per;
        nkt = min(nkt, kt_begin + per);
        if (kt_begin >= nkt) return;  // uniform per workgroup, before any barrier
    }
    const T *A = reinterpret_cast<const T *>(g.A);
    const T *W = reinterpret_cast<const T *>(g.W);
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    // LDS-DMA instruction j = wave * 4 + i covers token rows 4j .. 4j+3 of the stage; lane l lands at row 4j + l/16, 16-byte unit l%16, which
    // holds logical unit (l%16) ^ ((row & 3) << 2).  Columns beyond M / N are clamped to the last whole chunk (their outputs are never stored).
    const T *srcA[4], *srcW[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = (wave * 4 + i) * 4 + (lane >> 4);
        const int u = (lane & 15) ^ ((r & 3) << 2);
        srcA[i] = A + (size_t)r * g.lda + min(bm0 + u * 8, g.M - 8);
        srcW[i] = W + (size_t)r * g.ldw + min(bn0 + u * 8, g.N - 8);
    }
    typedef __attribute__((address_space(3))) void *lds_ptr;
    typedef const __attribute__((address_space(1))) void *glb_ptr;
    auto issue = [&](int kt, unsigned char *base) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            __builtin_amdgcn_global_load_lds((glb_ptr)(srcA[i] + (size_t)kt * BKT * g.lda), (lds_ptr)(base + (wave * 4 + i) * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((glb_ptr)(srcW[i] + (size_t)kt * BKT * g.ldw), (lds_ptr)(base + BKT * 256 + (wave * 4 + i) * 1024), 16, 0, 0);
        }
    };
    typedef __attribute__((ext_vector_type(4))) short s4;
    typedef __attribute__((address_space(3))) s4 *lds_s4;
    const int i16 = lane & 15, g1 = (lane >> 4) & 1;
    // fragment of output rows rowbase .. rowbase+31, contraction slice s: element j of lane half h is token 16 s + 8 h + j
    auto frag = [&](const unsigned char *img, int rowbase, int s) -> uint4 {
        const int m = 16 * s + 8 * lh + (i16 >> 2), bc = (rowbase + 16 * g1 + 4 * (i16 & 3)) * 2;
        const int o = m * 256 + ((((bc >> 6) ^ (m & 3))) << 6) + (bc & 63);   // rows m and m + 4 share (m & 3)
        union { s4 v[2]; uint4 u; } r;
        r.v[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(img + o));
        r.v[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(img + o + 4 * 256));
        return r.u;
    };
    auto compute = [&](const unsigned char *sa) {
        const unsigned char *sb = sa + BKT * 256;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            uint4 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[i] = frag(sa, wm * 64 + i * 32, s);
                fb[i] = frag(sb, wn * 64 + i * 32, s);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[i]), __builtin_bit_cast(bf16x8, fb[j]), acc[i][j], 0, 0, 0);
        }
    };
    issue(kt_begin, lds0);
    __syncthreads();
    int kt = kt_begin;
    for (; kt + 2 <= nkt; kt += 2) {
        issue(kt + 1, lds1);
        compute(lds0);
        __syncthreads();
        if (kt + 2 < nkt) issue(kt + 2, lds0);
        compute(lds1);
        __syncthreads();
    }
    if (kt < nkt) compute(lds0);
    gemm_accum_epilogue(g, acc, bm0, bn0, wm, wn, lr, lh);
}

// ---- persistent 256x128 kernel: the three-stage LDS-DMA ring runs ACROSS output tiles ------------------------------------------------------
// The per-tile fixed cost of the three-stage kernel is ~9 us (workgroup dispatch, address set-up, the first DMA round trip, epilogue): two
// thirds of a K = 512 tile (8 K-steps, 4.3 us of MFMA).  Here one workgroup per CU walks a list of tiles (XCD-contiguous ranges, as the
// non-persistent order) and its producer cursor simply keeps going: while tile i is in its last K-steps and its epilogue, the first two
// K-tiles of tile i+1 are already in flight.  The epilogue stages through the ring slot the last K-step just freed (16 rows per pass), behind
// one extra barrier; the step after an epilogue drains vmcnt to 0 (output stores share the counter with the DMA).
template <typename T, int EPI>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2))) void gemm_nt_pers_kernel(GemmArgs g) {
    constexpr int BK = ROWB / sizeof(T);
    constexpr int WM = 4, BMT = 256, NW = 8, GA = BMT / 8 / NW, GW = BN / 8 / NW, STAGE = (BMT + BN) * ROWB;
    static_assert(GA + GW == 6, "counted wait assumes six LDS-DMA instructions per wave and K-tile");
    __shared__ __attribute__((aligned(16))) unsigned char lds[3 * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1, lr = lane & 31, lh = lane >> 5;
    const int nbn = (g.N + BN - 1) / BN, nbm = (g.M + BMT - 1) / BMT, ntiles = nbn * nbm;
    // my tiles: XCD x = blockIdx % 8 owns a contiguous range, its workgroups interleave inside it
    const int w = blockIdx.x, nwg = gridDim.x, xcd = w % 8, j0 = w / 8;
    const int per_xcd = (nwg - xcd + 7) / 8;
    const int tq = ntiles / 8, tr = ntiles % 8;
    const int t_start = xcd < tr ? xcd * (tq + 1) : tr * (tq + 1) + (xcd - tr) * tq, t_count = tq + (xcd < tr ? 1 : 0);
    const int n_my = j0 < t_count ? (t_count - j0 + per_xcd - 1) / per_xcd : 0;
    const int nkt = g.K / BK, total = n_my * nkt;
    if (total == 0) return;
    const T *A = reinterpret_cast<const T *>(g.A);
    const T *W = reinterpret_cast<const T *>(g.W);
    typedef __attribute__((address_space(3))) void *lds_ptr;
    const uint32_t lds_base = (uint32_t)(uintptr_t)(lds_ptr)lds;

    // ---- producer cursor ----
    const int grow = lane >> 3;
    const T *srcA[GA], *srcW[GW];
    int p_tile = 0, p_kt = 0;
    auto set_tile = [&](int ti) {
        const int t = t_start + j0 + ti * per_xcd, bm0 = (t / nbn) * BMT, bn0 = (t % nbn) * BN;
#pragma unroll
        for (int i = 0; i < GA; ++i) {
            const int row = (wave * GA + i) * 8 + grow, gslot = (lane & 7) ^ ((row >> 1) & 7);
            srcA[i] = A + (size_t)min(bm0 + row, g.M - 1) * g.lda + gslot * (16 / sizeof(T));
        }
#pragma unroll
        for (int i = 0; i < GW; ++i) {
            const int row = (wave * GW + i) * 8 + grow, gslot = (lane & 7) ^ ((row >> 1) & 7);
            srcW[i] = W + (size_t)min(bn0 + row, g.N - 1) * g.ldw + gslot * (16 / sizeof(T));
        }
    };
    auto issue = [&](int slot) {   // next K-tile of the producer cursor -> ring slot
        const uint32_t lb = lds_base + slot * STAGE;
#pragma unroll
        for (int i = 0; i < GA; ++i) {
            const uint32_t dst = __builtin_amdgcn_readfirstlane(lb + (wave * GA + i) * 1024);
            glds16(dst, srcA[i] + (size_t)p_kt * BK);
        }
#pragma unroll
        for (int i = 0; i < GW; ++i) {
            const uint32_t dst = __builtin_amdgcn_readfirstlane(lb + BMT * ROWB + (wave * GW + i) * 1024);
            glds16(dst, srcW[i] + (size_t)p_kt * BK);
        }
        if (++p_kt == nkt) {
            p_kt = 0;
            if (++p_tile < n_my) set_tile(p_tile);
        }
    };

    f32x16 acc[2][2];
    auto zero_acc = [&]() {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    };
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

    set_tile(0);
    issue(0);
    if (total > 1) issue(1);
    zero_acc();
    int c_tile = 0, c_kt = 0, slot = 0;
    bool drained = false;   // the previous step ended with an epilogue: its stores are still counted in vmcnt
    for (int q = 0; q < total; ++q) {
        if (!drained && q + 1 < total)
            asm volatile("s_waitcnt vmcnt(6)\n\ts_barrier" ::: "memory");
        else
            asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        drained = false;
        if (q + 2 < total) issue(slot == 0 ? 2 : slot - 1);   // slot of step q + 2 = (slot + 2) % 3
        compute(lds + slot * STAGE);
        if (++c_kt == nkt) {
            c_kt = 0;
            const int t = t_start + j0 + c_tile * per_xcd, bm0 = (t / nbn) * BMT, bn0 = (t % nbn) * BN;
            if (EPI != 0 || !g.vec_epi) {
                gemm_epilogue<EPI, false>(g, acc, bm0, bn0, wm, wn, lr, lh);
            } else {
                asm volatile("s_barrier" ::: "memory");   // every wave is done reading this slot: it becomes the staging space
                float *stg = reinterpret_cast<float *>(lds + slot * STAGE + wave * (STAGE / NW));
                gemm_vec_epilogue<16>(g, acc, stg, bm0, bn0, wm, wn, lane);
            }
            zero_acc();
            ++c_tile;
            drained = true;
        }
        slot = slot == 2 ? 0 : slot + 1;
    }
}

// ---- persistent 256x256 kernel on a ring of five 32 KB half-stages (round 2) ------------------------------------------------------------
// The short-K GEMMs of the training steps (K = 512..768: 8-12 K-tiles per output tile) are bound by what a CU takes in through the LDS-DMA
// path - 33 GB/s from the Infinity Cache, 66-73 from its XCD's L2, and the 256x128 persistent ring sustains ~35 with ~75 % L2 hits - not by
// the matrix cores (31 % busy).  A 256x256 tile needs 64 KB per K-tile for twice the MFMA work of the 256x128 tile's 48 KB: 1.5x the flops
// per staged byte.  Three whole 64 KB stages do not fit the 160 KB of LDS, so the ring runs on HALF-stages: unit 2q is the A image
// ([256 rows][128 B], the layout of the other LDS-DMA kernels) of K-step q, unit 2q+1 its W image, unit u lives in slot u % 5.  While
// K-step q is computed (two slots), units A(q+1), W(q+1), A(q+2) are in flight in the other three: 96 KB, as much as the three-stage ring.
// Per step: s_waitcnt vmcnt(4) (only the four DMA instructions of the youngest unit may be outstanding), ONE raw barrier, issue W(q+2) and
// A(q+3) into the two slots step q-1 just freed, 32 MFMAs per wave.  The ring runs ACROSS output tiles (XCD-contiguous tile ranges, one
// workgroup per CU); the epilogue stages through the two slots its last K-step read (behind one extra barrier).
template <typename T, int EPI>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2))) void gemm_nt_pers256_kernel(GemmArgs g) {
    static_assert(sizeof(T) == 2 && EPI == 0, "bf16 row-major operands, plain epilogue");
    constexpr int BK = ROWB / sizeof(T);
    constexpr int BT = 256, UNIT = BT * ROWB, NSLOT = 5;   // 32 KB per unit
    __shared__ __attribute__((aligned(16))) unsigned char lds[NSLOT * UNIT];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3, lr = lane & 31, lh = lane >> 5;
    const int nbn = (g.N + BT - 1) / BT, nbm = (g.M + BT - 1) / BT, ntiles = nbn * nbm;
    // my tiles: XCD x = blockIdx % 8 owns a contiguous range, its workgroups interleave inside it
    const int w = blockIdx.x, nwg = gridDim.x, xcd = w % 8, j0 = w / 8;
    const int per_xcd = (nwg - xcd + 7) / 8;
    const int tq = ntiles / 8, tr = ntiles % 8;
    const int t_start = xcd < tr ? xcd * (tq + 1) : tr * (tq + 1) + (xcd - tr) * tq, t_count = tq + (xcd < tr ? 1 : 0);
    const int n_my = j0 < t_count ? (t_count - j0 + per_xcd - 1) / per_xcd : 0;
    const int nkt = g.K / BK, total = n_my * nkt;
    if (total == 0) return;
    const T *A = reinterpret_cast<const T *>(g.A);
    const T *W = reinterpret_cast<const T *>(g.W);
    typedef __attribute__((address_space(3))) void *lds_ptr;
    const uint32_t lds_base = (uint32_t)(uintptr_t)(lds_ptr)lds;

    // ---- producer: one cursor per operand (A runs one K-step ahead of W) ----
    const int grow = lane >> 3;
    const T *srcA[4], *srcW[4];
    int a_tile = 0, a_kt = 0, w_tile = 0, w_kt = 0, p_slot = 0;
    auto tile_origin = [&](int ti, int &bm0, int &bn0) {
        const int t = t_start + j0 + ti * per_xcd;
        bm0 = (t / nbn) * BT;
        bn0 = (t % nbn) * BT;
    };
    auto set_a = [&](int ti) {
        int bm0, bn0;
        tile_origin(ti, bm0, bn0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = (wave * 4 + i) * 8 + grow, gslot = (lane & 7) ^ ((row >> 1) & 7);
            srcA[i] = A + (size_t)min(bm0 + row, g.M - 1) * g.lda + gslot * (16 / sizeof(T));
        }
    };
    auto set_w = [&](int ti) {
        int bm0, bn0;
        tile_origin(ti, bm0, bn0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = (wave * 4 + i) * 8 + grow, gslot = (lane & 7) ^ ((row >> 1) & 7);
            srcW[i] = W + (size_t)min(bn0 + row, g.N - 1) * g.ldw + gslot * (16 / sizeof(T));
        }
    };
    // next A / W unit -> slot p_slot; nothing once the work list is exhausted.  Two functions with a fixed call order (A W A | W A | W A ...),
    // not one that picks the operand from the unit's parity: indexed that way the source-pointer arrays went to scratch memory, and every
    // reload drained vmcnt to 0 in front of the next DMA
    int a_done = 0, w_done = 0;   // K-steps issued per operand
    auto next_slot = [&]() { p_slot = p_slot == NSLOT - 1 ? 0 : p_slot + 1; };
    auto issue_a = [&]() {
        if (a_done >= total) return;
        const uint32_t lb = lds_base + p_slot * UNIT;
#pragma unroll
        for (int i = 0; i < 4; ++i) glds16(__builtin_amdgcn_readfirstlane(lb + (wave * 4 + i) * 1024), srcA[i] + (size_t)a_kt * BK);
        if (++a_kt == nkt) {
            a_kt = 0;
            if (++a_tile < n_my) set_a(a_tile);
        }
        ++a_done;
        next_slot();
    };
    auto issue_w = [&]() {
        if (w_done >= total) return;
        const uint32_t lb = lds_base + p_slot * UNIT;
#pragma unroll
        for (int i = 0; i < 4; ++i) glds16(__builtin_amdgcn_readfirstlane(lb + (wave * 4 + i) * 1024), srcW[i] + (size_t)w_kt * BK);
        if (++w_kt == nkt) {
            w_kt = 0;
            if (++w_tile < n_my) set_w(w_tile);
        }
        ++w_done;
        next_slot();
    };

    f32x16 acc[4][2];
    auto zero_acc = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    };
    auto compute = [&](const unsigned char *sa, const unsigned char *sb) {
        uint4 fa[2][4], fb[2][2];
        auto frags = [&](int s4, uint4 (&xa)[4], uint4 (&xb)[2]) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int ra = wm * 128 + i * 32 + lr;
                xa[i] = *reinterpret_cast<const uint4 *>(sa + ra * ROWB + (((s4 * 2 + lh) ^ ((ra >> 1) & 7)) << 4));
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int rb = wn * 64 + j * 32 + lr;
                xb[j] = *reinterpret_cast<const uint4 *>(sb + rb * ROWB + (((s4 * 2 + lh) ^ ((rb >> 1) & 7)) << 4));
            }
        };
        frags(0, fa[0], fb[0]);
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            if (s4 + 1 < 4) frags(s4 + 1, fa[(s4 + 1) & 1], fb[(s4 + 1) & 1]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[s4 & 1][i]), __builtin_bit_cast(bf16x8, fb[s4 & 1][j]), acc[i][j], 0, 0, 0);
        }
    };

    set_a(0);
    set_w(0);
    issue_a();   // A(0)
    issue_w();   // W(0)
    issue_a();   // A(1)
    zero_acc();
    int c_tile = 0, c_kt = 0, slot_a = 0;   // slot of A(q); W(q) sits in the next one
    bool drained = false;   // the previous step ended with an epilogue: its stores are still counted in vmcnt
    for (int q = 0; q < total; ++q) {
        // A(q), W(q) have landed: of everything issued, only A(q+1) - the youngest unit, four instructions per wave - may be outstanding
        if (!drained && q + 1 < total)
            asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
        else
            asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        drained = false;
        issue_w();   // W(q+1) -> the slot A(q-1) left
        issue_a();   // A(q+2) -> the slot W(q-1) left
        const int slot_w = slot_a == NSLOT - 1 ? 0 : slot_a + 1;
        compute(lds + slot_a * UNIT, lds + slot_w * UNIT);
        if (++c_kt == nkt) {
            c_kt = 0;
            int bm0, bn0;
            tile_origin(c_tile, bm0, bn0);
            // the wave's 128 x 64 block as two 64 x 64 halves through the shared routines (constant indices only: a run-time index into
            // acc would push all 128 accumulator registers to scratch)
            const bool vec = g.vec_epi;
            if (vec) asm volatile("s_barrier" ::: "memory");   // every wave is done reading these two slots: they become the staging space
            auto epi_half = [&](auto ihc) {
                constexpr int ih = decltype(ihc)::value;
                f32x16 half[2][2];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) half[i][j] = acc[2 * ih + i][j];
                const int bmh = bm0 + wm * 128 + ih * 64;
                if (!vec) {
                    gemm_epilogue<EPI, false>(g, half, bmh, bn0, 0, wn, lr, lh);
                } else {
                    float *stg = reinterpret_cast<float *>(lds + (wave < 4 ? slot_a : slot_w) * UNIT + (wave & 3) * (UNIT / 4));
                    gemm_vec_epilogue<16>(g, half, stg, bmh, bn0, 0, wn, lane);
                }
            };
            epi_half(std::integral_constant<int, 0>{});
            epi_half(std::integral_constant<int, 1>{});
            zero_acc();
            ++c_tile;
            drained = true;
        }
        slot_a = slot_a + 2 >= NSLOT ? slot_a + 2 - NSLOT : slot_a + 2;
    }
}

// ---- dW = dY^T X on the three-stage ring (round 2) -------------------------------------------------------------------------------------
// gemm_tn_glds_kernel keeps ONE 64-token tile in flight per workgroup (two stages, `__syncthreads()` drains the LDS-DMA): a K-step of a
// 128x128 tile is ~0.2 us of MFMA work against >= 1 us of loaded fabric latency, and two co-resident workgroups do not cover it (0.61-0.69 PF
// on the MAE's weight gradients).  This form is the NT ring's structure on the token-major operands: 256 (dY columns) x 128 (X columns) tile,
// 8 waves as 4 x 2, THREE 48 KB stages (two [64 tokens][128 col] images of dY, one of X, each in gemm_tn_glds_kernel's swizzled layout and
// read with the same transposing fragment reads), two K-tiles in flight behind a counted `s_waitcnt vmcnt(6)` and ONE raw barrier per K-step,
// LDS-DMA issued from inline asm so the compiler's wait-count pass never sees it.  Split-K over the tokens, fp32 atomics per 32x32 block.
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2))) void gemm_tn_ring_kernel(GemmArgs g) {
    typedef bf16_t T;
    constexpr int BKT = 64, IMG = BKT * 256, STAGE = 3 * IMG, BMT = 256;   // 16 KB per image, 48 KB per stage
    __shared__ __attribute__((aligned(16))) unsigned char lds[3 * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1, lr = lane & 31, lh = lane >> 5;
    const int nbn = (g.N + BN - 1) / BN, nbm = (g.M + BMT - 1) / BMT, nwg = nbn * nbm;
    int pid = blockIdx.x, kslice = 0;
    if (g.ksplit > 1) {
        kslice = pid / nwg;
        pid -= kslice * nwg;
    }
    const int bm0 = (pid / nbn) * BMT, bn0 = (pid % nbn) * BN;
    int nkt = (g.K + BKT - 1) / BKT, kt_begin = 0;   // the last K-tile may be ragged: its missing token rows arrive as zeros (blds16)
    if (g.ksplit > 1) {
        const int per = (nkt + g.ksplit - 1) / g.ksplit;
        kt_begin = kslice * per;
        nkt = min(nkt, kt_begin + per);
        if (kt_begin >= nkt) return;  // uniform per workgroup, before any barrier
    }
    const int nk = nkt - kt_begin;
    const T *A = reinterpret_cast<const T *>(g.A);
    const T *W = reinterpret_cast<const T *>(g.W);
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    // LDS-DMA instruction j (0..15) of an image covers token rows 4j .. 4j+3; lane l lands at row 4j + l/16, 16-byte unit l%16, which holds logical
    // unit (l%16) ^ ((row & 3) << 2).  Wave w issues j = 2w, 2w+1 of each of the three images: six instructions per wave and K-tile.
    // Columns beyond M / N are clamped to the last whole chunk (their outputs are never stored).
    uint32_t src[6];   // byte offsets from the K-tile's first token row (the host checks that they fit 32 bits)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = (wave * 2 + i) * 4 + (lane >> 4);
        const int u = (lane & 15) ^ ((r & 3) << 2);
        src[i] = (uint32_t)r * (uint32_t)(g.lda * 2) + (uint32_t)min(bm0 + u * 8, g.M - 8) * 2;
        src[2 + i] = (uint32_t)r * (uint32_t)(g.lda * 2) + (uint32_t)min(bm0 + 128 + u * 8, g.M - 8) * 2;
        src[4 + i] = (uint32_t)r * (uint32_t)(g.ldw * 2) + (uint32_t)min(bn0 + u * 8, g.N - 8) * 2;
    }
    typedef __attribute__((address_space(3))) void *lds_ptr;
    const uint32_t lds_base = (uint32_t)(uintptr_t)(lds_ptr)lds;
    auto issue = [&](int kt, int slot) {
        const uint32_t lb = lds_base + slot * STAGE;
        const int rows = min(g.K - kt * BKT, BKT);   // token rows of this K-tile that exist
        const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(A + (size_t)kt * BKT * g.lda), 0, rows * g.lda * 2, 0x00020000);
        const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(W + (size_t)kt * BKT * g.ldw), 0, rows * g.ldw * 2, 0x00020000);
#pragma unroll
        for (int m = 0; m < 3; ++m)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const uint32_t dst = __builtin_amdgcn_readfirstlane(lb + m * IMG + (wave * 2 + i) * 1024);
                blds16(dst, m == 2 ? rw : ra, src[2 * m + i]);
            }
    };
    typedef __attribute__((ext_vector_type(4))) short s4;
    typedef __attribute__((address_space(3))) s4 *lds_s4;
    const int i16 = lane & 15, g1 = (lane >> 4) & 1;
    // fragment of output rows rowbase .. rowbase+31 of one 128-column image, contraction slice s: element j of lane half h is token 16 s + 8 h + j
    auto frag = [&](const unsigned char *img, int rowbase, int s) -> uint4 {
        const int m = 16 * s + 8 * lh + (i16 >> 2), bc = (rowbase + 16 * g1 + 4 * (i16 & 3)) * 2;
        const int o = m * 256 + ((((bc >> 6) ^ (m & 3))) << 6) + (bc & 63);   // rows m and m + 4 share (m & 3)
        union { s4 v[2]; uint4 u; } r;
        r.v[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(img + o));
        r.v[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(img + o + 4 * 256));
        return r.u;
    };
    const int a_img = (wm >> 1) * IMG, a_row = (wm & 1) * 64;   // this wave's 64 dY columns: image wm / 2, rows (wm % 2) * 64 ..
    auto compute = [&](const unsigned char *st) {
        const unsigned char *sa = st + a_img, *sb = st + 2 * IMG;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            uint4 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[i] = frag(sa, a_row + i * 32, s);
                fb[i] = frag(sb, wn * 64 + i * 32, s);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[i]), __builtin_bit_cast(bf16x8, fb[j]), acc[i][j], 0, 0, 0);
        }
    };
    issue(kt_begin, 0);
    if (nk > 1) issue(kt_begin + 1, 1);
    int slot = 0;
    for (int q = 0; q < nk; ++q) {
        if (q + 1 < nk)
            asm volatile("s_waitcnt vmcnt(6)\n\ts_barrier" ::: "memory");   // this wave's six pieces of tile q have landed (tile q + 1 may still fly); everybody's have
        else
            asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        if (q + 2 < nk) issue(kt_begin + q + 2, slot == 0 ? 2 : slot - 1);   // the stage read in step q - 1: every wave is past it
        compute(lds + slot * STAGE);
        slot = slot == 2 ? 0 : slot + 1;
    }
    gemm_accum_epilogue(g, acc, bm0, bn0, wm, wn, lr, lh);
}

}  // namespace

void gemm_launch_ring(const AcaiGemmLaunch &l, int elem_size, int epi, const GemmArgs &g, hipStream_t st) {
    const dim3 grid(l.grid), block(l.block);
    switch (l.kernel) {
        case ACAI_GEMM_K_PERS:
            if (elem_size == 2) {
                if (epi) hipLaunchKernelGGL((gemm_nt_pers_kernel<bf16_t, 1>), grid, block, 0, st, g);
                else hipLaunchKernelGGL((gemm_nt_pers_kernel<bf16_t, 0>), grid, block, 0, st, g);
            } else {
                if (epi) hipLaunchKernelGGL((gemm_nt_pers_kernel<float, 1>), grid, block, 0, st, g);
                else hipLaunchKernelGGL((gemm_nt_pers_kernel<float, 0>), grid, block, 0, st, g);
            }
            break;
        // (bf16 operands and the plain epilogue only: the planner names these for nothing else)
        case ACAI_GEMM_K_PERS256: hipLaunchKernelGGL((gemm_nt_pers256_kernel<bf16_t, 0>), grid, block, 0, st, g); break;
        case ACAI_GEMM_K_TN_GLDS: hipLaunchKernelGGL(gemm_tn_glds_kernel, grid, block, 0, st, g); break;
        default: hipLaunchKernelGGL(gemm_tn_ring_kernel, grid, block, 0, st, g); break;   // ACAI_GEMM_K_TN_RING
    }
}
