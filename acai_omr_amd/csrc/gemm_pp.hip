// The ping-pong GEMM kernels (two wave groups one segment apart on a ring of half-stages) and their register epilogue: the row-major
// gemm_nt_pp_kernel and the weight-gradient gemm_tn_pp_kernel (tile constants and GemmArgs: gemm_internal.h).
#include "gemm_device.h"

namespace {

// barrier / LDS wait of a ping-pong segment boundary: fenced against the scheduler on both sides, so no instruction moves across
#define PP_BAR()                                      \
    do {                                              \
        __builtin_amdgcn_sched_barrier(0);            \
        asm volatile("s_barrier" ::: "memory");       \
        __builtin_amdgcn_sched_barrier(0);            \
    } while (0)
#define PP_LGKM0()                                               \
    do {                                                         \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       \
        __builtin_amdgcn_sched_barrier(0);                       \
    } while (0)

// ---- register epilogue of the swapped 16x16x32 layout (gemm_nt_pp_kernel) ----------------------------------------------------------------
// Lane (lm = lane & 15, lq = lane >> 4) of accumulator [mb][nb] holds C[m0 + mb*16 + lm][n0 + nb*16 + 4*lq + e], e = 0..3: four consecutive
// columns of one row.  fp32 rows are stored / loaded 16 bytes per lane as they stand (16 rows x 64 contiguous bytes per wave instruction).
// bf16: the two packed dwords of blocks nb = 2p and 2p+1 are exchanged between neighbouring 16-lane rows (v_permlane16_swap: odd rows of the
// first operand <-> even rows of the second), after which lane row r holds EIGHT consecutive columns: block 2p + (r & 1), columns 8 (r >> 1) ..;
// the exchange is an involution, so a 16-byte bf16 load at the swapped position followed by the same exchange yields the original layout
// (the saved pre-activation of aux_mode 2).  Every global access is a raw buffer access whose out-of-range lanes (rows >= M, columns >= N:
// offset forced beyond num_records) are dropped by the hardware range check: no divergent branch, and the instruction count per tile is exact
// (the caller's counted vmcnt wait relies on it).  Arithmetic and its order are gemm_vec_epilogue's.
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;
__device__ __forceinline__ void pp_swap2(uint32_t &x, uint32_t &y) {
    const u32x2_t r = __builtin_amdgcn_permlane16_swap(x, y, false, false);
    x = r[0];
    y = r[1];
}
// MODE (compile-time: one kernel instantiation per epilogue form - with every form in one body the kernel was > 100 KB of code, more than the
// instruction cache, and a plain bf16 epilogue took ~10 us per tile walking around the other forms' blocks)
template <int MODE>
__device__ __forceinline__ void gemm_pp_epilogue(const GemmArgs &g, const f32x4 (&acc)[8][4], int m0, int n0, int lane, float bv, void *dst = nullptr,
                                                 int ldd = 0) {
    const int lm = lane & 15, lq = lane >> 4;
    constexpr bool obf = MODE & PP_OBF, do_gelu = MODE & PP_GELU, has_res = MODE & PP_RES, has_scale = MODE & PP_SCALE;
    constexpr int aux_mode = (MODE & PP_AUX1) ? 1 : ((MODE & PP_AUX2) ? 2 : ((MODE & PP_AUX3) ? 3 : ((MODE & PP_AUX4) ? 4 : 0)));
    const bool do_round = g.flags & ACAI_GEMM_ROUND_BF16;
    const bool pre_round = do_round && (do_gelu || aux_mode != 0 || has_res || !obf);
    constexpr int es = obf ? 2 : 4;
    // (dst / ldd: the deferred forms write their first, plain bf16 pass somewhere else than C - see gemm_nt_pp_kernel)
    void *const Cp = dst ? dst : g.C;
    const int ldc = dst ? ldd : g.ldc;
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(Cp, 0, (int)((size_t)g.M * ldc * es), 0x00020000);
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(has_res ? g.residual : reinterpret_cast<const float *>(g.C)), 0,
                                                                        has_res ? (int)((size_t)g.M * g.ldr * 4) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(aux_mode ? g.aux : g.C, 0, aux_mode ? (int)((size_t)g.M * g.ldaux * es) : 0, 0x00020000);
    constexpr uint32_t OOB = 0xFFFFFFF0u;
    // swapped (bf16) position of this lane inside a block pair: block 2p + (lq & 1), columns 8 (lq >> 1) .. + 7
    const int sw_col = n0 + (lq & 1) * 16 + (lq >> 1) * 8;
    f32x4 bias4[4];
    bool colok[4];
    auto take_bias = [&](int p) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int nb = 2 * p + t, col = n0 + nb * 16 + 4 * lq;
            colok[nb] = col < g.N;
            // lane L of `bv` holds bias[n0 + L] (zero beyond N / without a bias), loaded by the caller a K-step ahead: a vector-memory load HERE
            // would be waited for behind the LDS-DMA just issued (vmcnt counts in order) - 3.6 us per tile on the decoder's in-projection
#pragma unroll
            for (int e = 0; e < 4; ++e) bias4[nb][e] = __shfl(bv, nb * 16 + 4 * lq + e);
        }
    };
    // Loop order.  Default: block pair p outermost (only its eight per-column constants are live), then two halves of four 16-row blocks.
    // P_INNER (the two GELU forms, bf16 output): pairs of 16-row blocks outermost, p innermost - a lane's two 64-byte halves of a 128-byte
    // line (the stores of C and of the kept pre-activation, the loads of the saved pre-activation) are then issued back to back.  With p
    // outermost they were half an epilogue apart, and under these forms' 1.6 GB of stores / loads per launch L2 evicted lines half written
    // and fetched lines twice (tools/pmc_gemm.sh, M = 131072, N = 3072, K = 512: forward WRITE_SIZE 2.24 GB for 1.61 GB of output - 743 -> 633 us
    // with this order; gelu' form FETCH_SIZE 2.2 GB for 0.94 GB of operands, WRITE_SIZE 1.08 GB for 0.81 GB).
    constexpr bool P_INNER = obf && (aux_mode != 0);   // (the plain bf16 forms measured the same either way: their lines survive in L2)
    if constexpr (P_INNER) {
        take_bias(0);
        take_bias(1);
    }
#pragma unroll
    for (int it_o = 0; it_o < 4; ++it_o) {
        if constexpr (!P_INNER) {
            if ((it_o & 1) == 0) take_bias(it_o >> 1);
        }
        // Every load of this group first (the saved pre-activation of aux_mode 2, the fp32 residual: 4 or 8 x 16 bytes per lane), then
        // the arithmetic and the stores: load -> use -> store per 16 rows made a chain of 16 dependent memory round trips per epilogue
        // (~30 us per tile on the decoder's gelu' GEMM).
        // (four (block, p) slots at a time: all eight blocks of a p spilled the residual form)
        u32x4_t prex[8][2], prer[8][2];
#pragma unroll
        for (int sl = 0; sl < 4; ++sl) {
            const int p = P_INNER ? (sl & 1) : (it_o >> 1);
            const int mb = P_INNER ? 2 * it_o + (sl >> 1) : 4 * (it_o & 1) + sl;
            const int row = m0 + mb * 16 + lm;
            const bool rowok = row < g.M;
            if constexpr (aux_mode == 2 || aux_mode == 4) {
                if constexpr (obf) {
                    const bool swok = rowok && (sw_col + p * 32) < g.N;
                    prex[mb][P_INNER ? p : 0] = __builtin_amdgcn_raw_buffer_load_b128(rx, swok ? (uint32_t)(((size_t)row * g.ldaux + sw_col + p * 32) * 2) : OOB, 0, 0);
                } else {
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        const int nb = 2 * p + t, col = n0 + nb * 16 + 4 * lq;
                        prex[mb][t] = __builtin_amdgcn_raw_buffer_load_b128(rx, (rowok && colok[nb]) ? (uint32_t)(((size_t)row * g.ldaux + col) * 4) : OOB, 0, 0);
                    }
                }
            }
            if constexpr (has_res) {
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int nb = 2 * p + t, col = n0 + nb * 16 + 4 * lq;
                    prer[mb][t] = __builtin_amdgcn_raw_buffer_load_b128(rr, (rowok && colok[nb]) ? (uint32_t)(((size_t)row * g.ldr + col) * 4) : OOB, 0, 0);
                }
            }
        }
#pragma unroll
        for (int sl = 0; sl < 4; ++sl) {
            const int p = P_INNER ? (sl & 1) : (it_o >> 1);
            const int mb = P_INNER ? 2 * it_o + (sl >> 1) : 4 * (it_o & 1) + sl;
            const int row = m0 + mb * 16 + lm;
            const bool rowok = row < g.M;
            f32x4 v[2];
            uint32_t rp[2][2] = {};
            const bool swok = rowok && (sw_col + p * 32) < g.N;
            const uint32_t off_sw_c = swok ? (uint32_t)(((size_t)row * ldc + sw_col + p * 32) * 2) : OOB;
            const uint32_t off_sw_x = swok ? (uint32_t)(((size_t)row * g.ldaux + sw_col + p * 32) * 2) : OOB;
            float a0[2][4] = {};
            if constexpr (aux_mode == 2 || aux_mode == 4) {
                if constexpr (obf) {
                    const u32x4_t L = prex[mb][P_INNER ? p : 0];
                    uint32_t x0 = L[0], x1 = L[1], y0 = L[2], y1 = L[3];
                    pp_swap2(x0, y0);
                    pp_swap2(x1, y1);
                    a0[0][0] = __uint_as_float(x0 << 16); a0[0][1] = __uint_as_float(x0 & 0xFFFF0000u);
                    a0[0][2] = __uint_as_float(x1 << 16); a0[0][3] = __uint_as_float(x1 & 0xFFFF0000u);
                    a0[1][0] = __uint_as_float(y0 << 16); a0[1][1] = __uint_as_float(y0 & 0xFFFF0000u);
                    a0[1][2] = __uint_as_float(y1 << 16); a0[1][3] = __uint_as_float(y1 & 0xFFFF0000u);
                } else {
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        const u32x4_t L = prex[mb][t];
#pragma unroll
                        for (int e = 0; e < 4; ++e) a0[t][e] = __uint_as_float(L[e]);
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int nb = 2 * p + t;
                v[t] = acc[mb][nb] + bias4[nb];
                if constexpr (has_scale) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[t][e] *= (n0 + nb * 16 + 4 * lq + e) < g.scale_cols ? g.col_scale : 1.0f;
                }
                if (pre_round) {
                    // rounded in PAIRS: one v_cvt_pk_bf16_f32 per two values and a shift / mask to widen them again (per value it was one
                    // conversion + one shift: the GELU forms' epilogues are VALU-bound); the packed words are also what aux_mode 1 stores
                    rp[t][0] = pack_bf16(v[t][0], v[t][1]);
                    rp[t][1] = pack_bf16(v[t][2], v[t][3]);
                    v[t][0] = __uint_as_float(rp[t][0] << 16); v[t][1] = __uint_as_float(rp[t][0] & 0xFFFF0000u);
                    v[t][2] = __uint_as_float(rp[t][1] << 16); v[t][3] = __uint_as_float(rp[t][1] & 0xFFFF0000u);
                }
            }
            [[maybe_unused]] float dg[2][4];   // aux_mode 3: gelu'(pre-activation), formed with the GELU below from one Phi(-|a|)
            if constexpr (aux_mode == 3) {
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float gv;
                        gelu_erf_both(v[t][e], gv, dg[t][e]);
                        v[t][e] = gv;
                    }
            }
            if constexpr (aux_mode == 1 || aux_mode == 3) {   // keep the pre-activation (1) / its GELU derivative (3)
                if constexpr (obf) {
                    uint32_t x0, x1, y0, y1;
                    if constexpr (aux_mode == 3) {
                        x0 = pack_bf16(dg[0][0], dg[0][1]); x1 = pack_bf16(dg[0][2], dg[0][3]); y0 = pack_bf16(dg[1][0], dg[1][1]); y1 = pack_bf16(dg[1][2], dg[1][3]);
                    } else if (pre_round) {
                        x0 = rp[0][0]; x1 = rp[0][1]; y0 = rp[1][0]; y1 = rp[1][1];
                    } else {
                        x0 = pack_bf16(v[0][0], v[0][1]); x1 = pack_bf16(v[0][2], v[0][3]); y0 = pack_bf16(v[1][0], v[1][1]); y1 = pack_bf16(v[1][2], v[1][3]);
                    }
                    pp_swap2(x0, y0);
                    pp_swap2(x1, y1);
                    __builtin_amdgcn_raw_buffer_store_b128(u32x4_t{x0, x1, y0, y1}, rx, off_sw_x, 0, 0);
                } else {
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        const int nb = 2 * p + t, col = n0 + nb * 16 + 4 * lq;
                        const uint32_t o = (rowok && colok[nb]) ? (uint32_t)(((size_t)row * g.ldaux + col) * 4) : OOB;
                        if constexpr (aux_mode == 3) __builtin_amdgcn_raw_buffer_store_b128(u32x4_t{__float_as_uint(dg[t][0]), __float_as_uint(dg[t][1]), __float_as_uint(dg[t][2]), __float_as_uint(dg[t][3])}, rx, o, 0, 0);
                        else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v[t]), rx, o, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int nb = 2 * p + t, col = n0 + nb * 16 + 4 * lq;
                if constexpr (aux_mode == 2) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[t][e] *= gelu_erf_grad(a0[t][e]);
                }
                if constexpr (aux_mode == 4) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[t][e] *= a0[t][e];
                }
                if constexpr (do_gelu) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if constexpr (aux_mode != 3) v[t][e] = gelu_erf(v[t][e]);   // (3: done above, together with the derivative)
                        if (do_round && !obf) v[t][e] = round_bf16(v[t][e]);   // (bf16 output: the pack below is that rounding)
                    }
                }
                if constexpr (has_res) v[t] += __builtin_bit_cast(f32x4, prer[mb][t]);
                if constexpr (!obf) {
                    const uint32_t o = (rowok && colok[nb]) ? (uint32_t)(((size_t)row * ldc + col) * 4) : OOB;
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v[t]), rc, o, 0, 0);
                }
            }
            if constexpr (obf) {
                uint32_t x0 = pack_bf16(v[0][0], v[0][1]), x1 = pack_bf16(v[0][2], v[0][3]), y0 = pack_bf16(v[1][0], v[1][1]), y1 = pack_bf16(v[1][2], v[1][3]);
                pp_swap2(x0, y0);
                pp_swap2(x1, y1);
#ifdef ACAI_GEMM_ABLATE
                const int dbg = g.flags >> 8;
#else
                constexpr int dbg = 0;
#endif
                if (dbg & 128) asm volatile("" ::"v"(x0), "v"(x1), "v"(y0), "v"(y1));
                else __builtin_amdgcn_raw_buffer_store_b128(u32x4_t{x0, x1, y0, y1}, rc, (dbg & 64) ? (off_sw_c & 0xFFFF0u) : off_sw_c, 0, 0);
            }
        }
    }
}

// ---- persistent 256x256 ring with PING-PONG wave groups and a REGISTER epilogue (round 3) -----------------------------------------------
// What round 2 measured on the short-K GEMMs of the training steps (K = 512..768): the main loop of the rings runs at ~40-45 % of the matrix
// pipe and the epilogue (LDS transposition + stores, nothing else running on the CU meanwhile) adds another 50 % on top.  Both have one cause:
// the two waves of a SIMD run the same program in lock-step behind one barrier per K-step - both read fragments, both issue MFMAs, both
// transpose and store - so the matrix pipe idles whenever "the" wave does anything else.  This kernel keeps pers256's ring (five 32 KB
// half-stage slots, LDS-DMA from inline asm, counted vmcnt waits, persistent XCD-contiguous tile lists) and changes three things:
//  1. Ping-pong: a K-step is four barrier-separated segments per wave - R(kh=0): 12 ds_read_b128, M(kh=0): 32 MFMAs, R(kh=1), M(kh=1) - and
//     waves 4-7 (the lower 128 rows of the tile; they share SIMDs with waves 0-3) run ONE SEGMENT BEHIND waves 0-3: while one wave of a
//     SIMD issues its 32 MFMAs the other reads its fragments, issues its LDS-DMA or runs its epilogue.  Fragments are single-buffered (the
//     partner's MFMAs cover the read latency), so the loop needs 48 fragment registers instead of 96.
//  2. v_mfma_f32_16x16x32_bf16 with the operands SWAPPED (W fragment as the A operand): D[n][m], a lane holds FOUR CONSECUTIVE COLUMNS of one
//     output row.  fp32 outputs store 16 bytes per lane straight from the accumulators; bf16 outputs exchange the packed halves of two
//     neighbouring 16-column blocks between the 16-lane rows (v_permlane16_swap) and also store 16 bytes per lane - 16 rows x 64 contiguous
//     bytes per wave instruction, no LDS transposition, no epilogue barrier, no staging space.  (The 16x16x32 shape also holds a higher clock
//     than 32x32x16 at equal cycles per flop on this chip: MI355X_MICROARCH.md, DVFS item 7.)
//  3. The epilogue of tile i runs in the first R segment of tile i+1 of the same wave - i.e. beside the partner's MFMAs - and its stores stay
//     in flight: they are raw buffer stores (out-of-range lanes dropped by the range check, so the instruction COUNT is exact) issued between
//     the segment's two LDS-DMA groups, and the K-step's counted wait allows for them (vmcnt counts stores and LDS-DMA together, in order).
// Segment / barrier ledger (b_s = barrier at the end of global segment s; waves 0-3 = G0, waves 4-7 = G1):
//     G0: R(q,0) = seg 4q, M(q,0) = 4q+1, R(q,1) = 4q+2, M(q,1) = 4q+3;    G1: the same one segment later (4q+1 .. 4q+4)
//     slots of K-step q are last read in seg 4q+3 (G1, reads waited with lgkmcnt(0) before b_{4q+3}) and refilled from seg 4q+4 on;
//     every wave waits for ITS pieces of K-step q+1 (vmcnt) before b_{4q+3}; the first read of K-step q+1 is in seg 4q+4.
template <typename T, int MODE>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2))) void gemm_nt_pp_kernel(GemmArgs g) {
    static_assert(sizeof(T) == 2, "bf16 row-major operands");
    constexpr int BK = ROWB / sizeof(T);
    constexpr int BT = 256, UNIT = BT * ROWB, NSLOT = 5;   // 32 KB per unit
    __shared__ __attribute__((aligned(16))) unsigned char lds[NSLOT * UNIT];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3, grp = wm;
    const int lm = lane & 15, lq = lane >> 4;
    const int nbn = (g.N + BT - 1) / BT, nbm = (g.M + BT - 1) / BT, ntiles = nbn * nbm;
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

    // timing ablations (-DACAI_GEMM_ABLATE builds only - tools/ablate_pp.py, tools/build_variant.sh; ACAI_GEMM_DEBUG bits, results are wrong):
    // 1 no counted waits, 2 no LDS-DMA, 4 no epilogue, 8 no MFMAs, 16 no fragment reads, 32 start-up skew of the workgroups.  The production
    // build compiles them out (a stray high flag bit or a leftover environment variable silently dropped stores).
#ifdef ACAI_GEMM_ABLATE
    const int dbg = g.flags >> 8;
#else
    constexpr int dbg = 0;
#endif
    // ---- producer (as pers256): one cursor per operand, A runs one K-step ahead of W ----
    // Sources as a uniform base (SGPR pair: the tile's first row, advanced per K-step) + a 32-bit byte offset per lane: (row within the tile,
    // clamped to the operand's last row) x pitch + the swizzled 16-byte slot.  24-bit multiplies (the host checks pitch < 2^24 bytes).
    const int grow = lane >> 3;
    const int r0 = wave * 32 + grow;                                  // this lane's tile row for piece i: r0 + 8 i
    const uint32_t g0 = (uint32_t)(((lane & 7) ^ (grow >> 1)) << 4);   // its slot for even i; odd i: ^ 64
    const uint32_t pitchA = (uint32_t)g.lda * 2, pitchW = (uint32_t)g.ldw * 2;
    uint32_t offA[4], offW[4];
    const T *tileA = A, *tileW = W;
    int a_tile = 0, a_kt = 0, w_tile = 0, w_kt = 0, p_slot = 0;
    auto tile_origin = [&](int ti, int &bm0, int &bn0) {
        const int t = t_start + j0 + ti * per_xcd;
        bm0 = (t / nbn) * BT;
        bn0 = (t % nbn) * BT;
    };
    auto set_a = [&](int ti) {
        int bm0, bn0;
        tile_origin(ti, bm0, bn0);
        tileA = A + (size_t)bm0 * g.lda;
        const int last = g.M - 1 - bm0;
#pragma unroll
        for (int i = 0; i < 4; ++i) offA[i] = __umul24(min(r0 + 8 * i, last), pitchA) + (g0 ^ ((i & 1) << 6));
    };
    auto set_w = [&](int ti) {
        int bm0, bn0;
        tile_origin(ti, bm0, bn0);
        tileW = W + (size_t)bn0 * g.ldw;
        const int last = g.N - 1 - bn0;
#pragma unroll
        for (int i = 0; i < 4; ++i) offW[i] = __umul24(min(r0 + 8 * i, last), pitchW) + (g0 ^ ((i & 1) << 6));
    };
    int a_done = 0, w_done = 0;
    auto next_slot = [&]() { p_slot = p_slot == NSLOT - 1 ? 0 : p_slot + 1; };
    auto issue_a = [&]() -> bool {
        if (a_done >= total) return false;
        const uint32_t lb = lds_base + p_slot * UNIT;
        const T *base = tileA + (size_t)a_kt * BK;   // uniform
        if (!(dbg & 2)) glds16s_x4(__builtin_amdgcn_readfirstlane(lb + wave * 4096), base, offA[0], offA[1], offA[2], offA[3]);
        if (++a_kt == nkt) {
            a_kt = 0;
            if (++a_tile < n_my) set_a(a_tile);
        }
        ++a_done;
        next_slot();
        return true;
    };
    auto issue_w = [&]() -> bool {
        if (w_done >= total) return false;
        const uint32_t lb = lds_base + p_slot * UNIT;
        const T *base = tileW + (size_t)w_kt * BK;
        if (!(dbg & 2)) glds16s_x4(__builtin_amdgcn_readfirstlane(lb + wave * 4096), base, offW[0], offW[1], offW[2], offW[3]);
        if (++w_kt == nkt) {
            w_kt = 0;
            if (++w_tile < n_my) set_w(w_tile);
        }
        ++w_done;
        next_slot();
        return true;
    };

    // ---- consumer: swapped 16x16x32 MFMAs; lane (lm, lq) of accumulator [mb][nb] holds C[mb*16 + lm][nb*16 + 4*lq + 0..3] ----
    f32x4 acc[8][4];
    auto zero_acc = [&]() {
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    // logical 16-byte chunk c = 4 kh + lq of tile row r sits in slot c ^ ((r >> 1) & 7); (r >> 1) & 7 = (lm >> 1) & 7 for every row this lane
    // reads (the rows differ by multiples of 16).  16 lanes of a ds_read_b128 group then cover 16 distinct 16-byte bank groups.
    const int swz = (lm >> 1) & 7;
    const int offk0 = (lq ^ swz) << 4, offk1 = ((4 + lq) ^ swz) << 4;
    const int a_off = (wm * 128 + lm) * ROWB, w_off = (wn * 64 + lm) * ROWB;
    uint4 fa[8], fw[4];
    auto reads = [&](const unsigned char *sa, const unsigned char *sb, int offk) {
#pragma unroll
        for (int j = 0; j < 4; ++j) fw[j] = *reinterpret_cast<const uint4 *>(sb + w_off + j * 16 * ROWB + offk);
#pragma unroll
        for (int i = 0; i < 8; ++i) fa[i] = *reinterpret_cast<const uint4 *>(sa + a_off + i * 16 * ROWB + offk);
    };
    auto mfmas = [&]() {
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fw[j]), __builtin_bit_cast(bf16x8, fa[i]), acc[i][j], 0, 0, 0);
    };
    // counted wait of K-step q: everything up to W(q+1) has landed; younger and allowed in flight: the epilogue's stores (n_st of them when an
    // epilogue ran in this K-step) and the four pieces of A(q+2) (when it exists)
    auto wait_step = [&](int allow) {
        switch (allow) {
            case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
            case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
            case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
            case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
            case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
            case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
            case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
            case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
            case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
            case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
            case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
            case 16: asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); break;
            case 20: asm volatile("s_waitcnt vmcnt(20)" ::: "memory"); break;
            case 32: asm volatile("s_waitcnt vmcnt(32)" ::: "memory"); break;
            case 36: asm volatile("s_waitcnt vmcnt(36)" ::: "memory"); break;
            default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        }
    };
    constexpr int n_st = (MODE & PP_OBF) ? ((MODE & (PP_AUX1 | PP_AUX3)) ? 32 : 16) : 32;   // store instructions per wave and tile (host: vec_epi only)

    // The bias of the tile in flight, one column per lane (lane L: bias[bn0 + wn*64 + L]); the epilogue distributes it with ds_bpermute and
    // issues no vector-memory load of its own.  A compiler-visible load anywhere in this loop is waited for with vmcnt(0) at its first use,
    // i.e. behind whatever LDS-DMA is in flight then (vmcnt counts in order): 2.5-3.6 us per tile, measured at three placements.  So the load is
    // an asm statement the wait-count pass does not see, issued in front of the K-step's LDS-DMA; the counted wait at the end of the same K-step
    // retires it together with everything older than W(q+1), and it is read at the top of the NEXT K-step.
    // Rule for every such untracked load in this kernel (bias, deferred chunks): ONE load statement and ONE take statement per loop iteration,
    // both unconditional and in straight-line code, the value handed from the load's "=v" output to the take's "+v" operand.  A first version
    // loaded under `if (tile start)` into a register tied through the asm statements: the branches' merge points made the register allocator
    // copy the value right behind the load statement - i.e. read it before the data had landed.  (Accumulator registers as destinations would
    // be out of the compiler's reach, but a kernel that touches AGPRs gets its 256 registers split 128 / 128 on gfx950: 100+ spills here.)
    uint32_t bias_raw = 0;
    int c_tile = 0, c_kt = 0, slot_a = 0;
    auto load_bias = [&]() {      // this K-step's tile
        int bm0, bn0;
        tile_origin(c_tile < n_my ? c_tile : n_my - 1, bm0, bn0);
        const uint32_t off = (uint32_t)min(bn0 + wn * 64 + lane, g.N - 1) * 4;
        const float *bp = g.bias ? g.bias : reinterpret_cast<const float *>(g.W);   // (no bias: any valid address; the value is not used)
        asm volatile("global_load_dword %0, %1, %2" : "=v"(bias_raw) : "v"(g.bias ? off : 0u), "s"(bp) : "memory");
    };
    // ---- PP_DEFER: the expensive half of a GELU epilogue leaves the tile boundary -----------------------------------------------------------
    // The GELU forms (forward: C = gelu(a), aux = a; backward: C = v gelu'(aux)) spend ~10k cycles of VALU per wave and tile at the boundary,
    // beside ONE 512-cycle MFMA segment of the partner wave: 2 x 10k exposed per tile against 16k of MFMA time (K = 512).  Deferred form: the
    // boundary epilogue only stores the bf16-rounded linear output (a into aux / v into C - both are rounded to bf16 before the GELU step in
    // the undeferred arithmetic too, so nothing changes numerically), and the GELU step runs in CHUNKS of 8 columns x 16 rows per lane - one
    // 16-byte piece of the SAME lane's own stores, read back from L2 - one chunk per R segment of the next tile, i.e. beside the partner's MFMAs
    // for the whole tile.  A chunk's piece is loaded one segment ahead by an untracked asm load (as the bias is: a compiler-visible load would be
    // waited for behind the LDS-DMA in flight), in FRONT of that segment's LDS-DMA, so waiting for it (vmcnt(4): only the DMA pieces are
    // younger) never waits for a DMA.
    // MEASURED (round 3, tools/bench_pp.py, same box): slower - MAE decoder lin1 + GELU 833 against 686 us, its gelu' GEMM 962 against 825 us,
    // the encoder's 283 / 304 against 236 / 254 us.  A chunk is ~1100 cycles of VALU in an R segment whose partner's M segment is 512: every
    // barrier interval stretches to the chunk, 32 intervals per tile, where the boundary form pays its 2 x 10k once - the two waves of a SIMD
    // share one VALU port, so 20k VALU cycles per SIMD and tile cannot hide behind 16k of MFMA however they are cut - and the chunks come back
    // from L2 / MALL (0.8 GB more reads on lin1).  Off by default (variant 8 selects it); the test keeps it runnable.
    constexpr bool DEFER = MODE & PP_DEFER;
    constexpr int NL = (MODE & PP_AUX2) ? 2 : 1;     // loads per chunk
    // two chunk slots: X is loaded in R(q,0) and finished in R(q,1), Y is loaded in R(q,1) and finished in R(q+1,0); *2: the saved
    // pre-activation of the backward form.  Loads and takes are unconditional (an idle slot reloads chunk 0 and drops its result), see the rule
    // at the bias load.
    u32x4_t cX = {0, 0, 0, 0}, cX2 = {0, 0, 0, 0}, cY = {0, 0, 0, 0}, cY2 = {0, 0, 0, 0};
    int d_m0 = 0, d_n0 = 0, d_next = 16;   // tile being drained (its wave block's origin) and its next chunk to load (16: nothing to drain)
    int idX = -1, idY = -1;                // chunk id in each slot (-1: idle)
    // one chunk per R segment: a tile has 2 nkt of them for its predecessor's 16 chunks (host: nkt >= 8, i.e. K >= 512 - every MLP of the path)
    const __amdgpu_buffer_rsrc_t d_rc = __builtin_amdgcn_make_buffer_rsrc(g.C, 0, (int)((size_t)g.M * g.ldc * 2), 0x00020000);
    auto chunk_off = [&](int c, int ld, bool &ok) -> uint32_t {
        const int row = d_m0 + (c & 7) * 16 + lm, col = d_n0 + (lq & 1) * 16 + (lq >> 1) * 8 + (c >> 3) * 32;
        ok = c >= 0 && row < g.M && col < g.N;
        return ok ? (uint32_t)row * (uint32_t)(ld * 2) + (uint32_t)col * 2 : 0u;
    };
    auto chunk_load = [&](int c, u32x4_t &L, u32x4_t &A2) {
        bool ok;
        if constexpr (MODE & PP_AUX2) {
            const uint32_t oc = chunk_off(c, g.ldc, ok), ox = chunk_off(c, g.ldaux, ok);
            asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(L) : "v"(oc), "s"(g.C) : "memory");
            asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(A2) : "v"(ox), "s"(g.aux) : "memory");
        } else {
            const uint32_t ox = chunk_off(c, g.ldaux, ok);
            asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(L) : "v"(ox), "s"(g.aux) : "memory");
        }
    };
    // wait for the slot's loads: only the LDS-DMA pieces issued behind them (four, or none at the end of the work list) may stay outstanding
    auto chunk_take = [&](bool dma_behind, u32x4_t &L, u32x4_t &A2) {
        // (the statement that carries the registers is unconditional: with one take per branch the merge point copied the in-flight registers)
        if (!dma_behind) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if constexpr (MODE & PP_AUX2) asm volatile("s_waitcnt vmcnt(4)" : "+v"(L), "+v"(A2)::"memory");
        else asm volatile("s_waitcnt vmcnt(4)" : "+v"(L)::"memory");
    };
    auto chunk_finish = [&](int c, const u32x4_t &L, const u32x4_t &A2) {
        bool ok;
        const uint32_t oc = chunk_off(c, g.ldc, ok);
        u32x4_t o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float lo = __uint_as_float(L[i] << 16), hi = __uint_as_float(L[i] & 0xFFFF0000u);
            if constexpr (MODE & PP_AUX2) {
                lo *= gelu_erf_grad(__uint_as_float(A2[i] << 16));
                hi *= gelu_erf_grad(__uint_as_float(A2[i] & 0xFFFF0000u));
            } else {
                lo = gelu_erf(lo);
                hi = gelu_erf(hi);
            }
            o[i] = pack_bf16(lo, hi);
        }
        __builtin_amdgcn_raw_buffer_store_b128(o, d_rc, ok ? oc : 0xFFFFFFF0u, 0, 0);
    };

    set_a(0);
    set_w(0);
    issue_a();   // A(0)
    issue_w();   // W(0)
    issue_a();   // A(1)
    zero_acc();
    if (total > 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    PP_BAR();              // b_{-1}: K-step 0 has landed for everybody
    if (dbg & 32) {
        for (int i = 0; i < (int)(blockIdx.x / 8 % 8); ++i) __builtin_amdgcn_s_sleep(32);   // ~ (w/8 % 8) x 1 us
    }
    if (grp == 1) PP_BAR();   // G1 runs one segment behind
    bool dma_prev = true;    // the segment before the first one of the loop issued A(1)
    for (int q = 0; q <= total; ++q) {
        const bool live = q < total;    // the extra pass q == total only runs the last tile's epilogue (and keeps the barrier count)
        const int slot_w = slot_a == NSLOT - 1 ? 0 : slot_a + 1;
        const unsigned char *sa = lds + slot_a * UNIT, *sb = lds + slot_w * UNIT;
        // ---- R(q, 0) ----
        const bool boundary = c_kt == 0 && q > 0;
        if (!live) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (no counted wait came after the last K-step's bias / chunk loads)
        asm volatile("" : "+v"(bias_raw));   // take: the load of the K-step before was retired by that K-step's counted wait
        const float bv = g.bias ? __uint_as_float(bias_raw) : 0.f;
        int allow = q + 2 < total ? 4 : 0;
        if constexpr (DEFER) {
            // slot Y (loaded in R(q-1,1), in front of A(q+1)'s pieces): take and finish - at a tile boundary this is the old tile's last chunk
            chunk_take(live && dma_prev, cY, cY2);
            if (idY >= 0) chunk_finish(idY, cY, cY2);
            if (boundary) {
                // the plain bf16 pass of the tile just finished; its chunks start below
                int bm0, bn0;
                tile_origin(c_tile - 1, bm0, bn0);
                if (!(dbg & 4)) {
                    if constexpr (MODE & PP_AUX2) gemm_pp_epilogue<PP_OBF>(g, acc, bm0 + wm * 128, bn0 + wn * 64, lane, bv);
                    else gemm_pp_epilogue<PP_OBF>(g, acc, bm0 + wm * 128, bn0 + wn * 64, lane, bv, g.aux, g.ldaux);
                }
                zero_acc();
                d_m0 = bm0 + wm * 128;
                d_n0 = bn0 + wn * 64;
                d_next = 0;
            }
            load_bias();
            idX = (live && d_next < 16) ? d_next++ : -1;
            chunk_load(idX, cX, cX2);
            dma_prev = issue_w();   // W(q+1) -> the slot A(q-1) left
        } else {
            load_bias();
            issue_w();   // W(q+1) -> the slot A(q-1) left
            if (boundary) {
                int bm0, bn0;
                tile_origin(c_tile - 1, bm0, bn0);
                if (!(dbg & 4)) {
                    gemm_pp_epilogue<MODE>(g, acc, bm0 + wm * 128, bn0 + wn * 64, lane, bv);
                    allow += n_st;
                }
                zero_acc();
            }
        }
        if (live && !(dbg & 16)) reads(sa, sb, offk0);   // (after the epilogue: the fragment registers are not live across it)
        PP_LGKM0();
        PP_BAR();
        // ---- M(q, 0) ----
        if (live && !(dbg & 8)) mfmas();
        PP_BAR();
        // ---- R(q, 1) ----
        if constexpr (DEFER) {
            chunk_take(dma_prev, cX, cX2);   // slot X, loaded in R(q,0) in front of W(q+1)'s pieces
            if (idX >= 0) {
                chunk_finish(idX, cX, cX2);
                allow += 1;                  // its store is younger than W(q+1) ...
            }
            idY = (live && d_next < 16) ? d_next++ : -1;
            chunk_load(idY, cY, cY2);
            allow += NL;                     // ... and so are slot Y's loads
            dma_prev = issue_a();            // A(q+2) -> the slot W(q-1) left
        } else {
            issue_a();   // A(q+2) -> the slot W(q-1) left (the K-step's eight LDS-DMA pieces are split over its two R segments)
        }
        if (live && !(dbg & 16)) reads(sa, sb, offk1);
        PP_LGKM0();
        if (grp == 1 && q + 1 < total && !(dbg & 1)) wait_step(allow);
        PP_BAR();
        // ---- M(q, 1) ----
        if (live && !(dbg & 8)) mfmas();
        if (grp == 0 && q + 1 < total && !(dbg & 1)) wait_step(allow);
        PP_BAR();
        if (live && ++c_kt == nkt) {
            c_kt = 0;
            ++c_tile;
        }
        slot_a = slot_a + 2 >= NSLOT ? slot_a + 2 - NSLOT : slot_a + 2;
    }
    if (grp == 0) PP_BAR();
    if constexpr (DEFER) {
        // the last tile's chunks: nothing else is in flight any more, so plain (compiler-tracked) loads, all requested before the first is used
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(g.aux, 0, (int)((size_t)g.M * g.ldaux * 2), 0x00020000);
        u32x4_t Ls[16], As[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            bool ok;
            if constexpr (MODE & PP_AUX2) {
                Ls[c] = __builtin_amdgcn_raw_buffer_load_b128(d_rc, chunk_off(c, g.ldc, ok), 0, 0);
                As[c] = __builtin_amdgcn_raw_buffer_load_b128(rx, chunk_off(c, g.ldaux, ok), 0, 0);
            } else {
                Ls[c] = __builtin_amdgcn_raw_buffer_load_b128(rx, chunk_off(c, g.ldaux, ok), 0, 0);
                As[c] = Ls[c];
            }
        }
#pragma unroll
        for (int c = 0; c < 16; ++c) chunk_finish(c, Ls[c], As[c]);
    }
}

// ---- dW = dY^T X with ping-pong wave groups on the ring of half-stages (round 3) ---------------------------------------------------------
// gemm_tn_ring_kernel (256 x 128 tile, three 48 KB stages, both waves of a SIMD in lock-step behind one barrier per K-step) ran the MAE's
// weight gradients at 0.71-0.89 PF.  This is gemm_nt_pp_kernel's structure on the token-major operands: 256 (dY columns) x 256 (X columns)
// tile, 8 waves as 2 x 4 (128 x 64 each, 16x16x32 MFMAs: 128 accumulator registers), K-step = 64 tokens, a unit = one operand's
// [64 tokens][256 columns] image (32 KB, as two [64][128-column] images of 256-byte rows), five unit slots, the dY unit two K-steps ahead and
// the X unit one, LDS-DMA from inline asm behind counted waits, and the two wave groups one segment apart (R: fragment reads + this
// segment's four LDS-DMA pieces, M: 32 MFMAs; two of each per K-step).  Fragments - eight consecutive tokens of one column - come from
// ds_read_b64_tr_b16 out of the natural image, whose 16-byte chunk c of token row r sits in slot c ^ (((r & 3) << 2) | ((r >> 2) & 3)): the
// four token rows of a transposing read land in four different 64-byte blocks and the two 16-lane groups of a half-wave (token rows 8 apart)
// in different 32-byte halves (cdna_hip_programming.md T10, image (b)).  One (tile, K-slice) per workgroup, split-K over the tokens so that
// about one workgroup per CU exists, fp32 atomics straight from the accumulators: the un-swapped 16x16 layout gives a lane one column and
// four consecutive rows, so a wave instruction adds four 64-byte row segments.
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2))) void gemm_tn_pp_kernel(GemmArgs g) {
    typedef bf16_t T;
    constexpr int BKT = 64, BT = 256, UNIT = BKT * BT * 2, NSLOT = 5, IMG = BKT * 256;   // 32 KB per unit, 16 KB per 128-column image
    __shared__ __attribute__((aligned(16))) unsigned char lds[NSLOT * UNIT];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3, grp = wm;
    const int nbn = (g.N + BT - 1) / BT, nbm = (g.M + BT - 1) / BT, nwg = nbn * nbm;
    int pid = blockIdx.x, kslice = 0;
    if (g.ksplit > 1) {
        kslice = pid / nwg;
        pid -= kslice * nwg;
    }
    const int bm0 = (pid / nbn) * BT, bn0 = (pid % nbn) * BT;
    int nkt = (g.K + BKT - 1) / BKT, kt_begin = 0;   // the last K-step may be ragged: its missing token rows arrive as zeros (blds16_x4)
    if (g.ksplit > 1) {
        const int per = (nkt + g.ksplit - 1) / g.ksplit;
        kt_begin = kslice * per;
        nkt = min(nkt, kt_begin + per);
        if (kt_begin >= nkt) return;  // uniform per workgroup, before any barrier
    }
    const int total = nkt - kt_begin;
    const T *A = reinterpret_cast<const T *>(g.A) + (size_t)kt_begin * BKT * g.lda;
    const T *W = reinterpret_cast<const T *>(g.W) + (size_t)kt_begin * BKT * g.ldw;
    const int rows_left0 = g.K - kt_begin * BKT;   // token rows from this slice's first K-step to the end of the operands
    typedef __attribute__((address_space(3))) void *lds_ptr;
    const uint32_t lds_base = (uint32_t)(uintptr_t)(lds_ptr)lds;

    // ---- producer: piece j (0..31) of a unit = image j / 16, token rows 4 (j % 16) .. + 3; wave w issues pieces 4w .. 4w+3 (4 KB of LDS in a row).
    // Lane l of a piece: token row 4 (j % 16) + l / 16, LDS slot l % 16 <- logical chunk (l % 16) ^ swz(row).  Columns beyond the operand
    // are clamped to its last whole chunk (their outputs are never stored).
    uint32_t offA[4], offW[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = wave * 4 + i, row = 4 * (j & 15) + (lane >> 4);
        const int ch = (lane & 15) ^ (((row & 3) << 2) | ((row >> 2) & 3));
        const int col = 128 * (j >> 4) + 8 * ch;
        offA[i] = (uint32_t)row * (uint32_t)(g.lda * 2) + (uint32_t)min(bm0 + col, g.M - 8) * 2;
        offW[i] = (uint32_t)row * (uint32_t)(g.ldw * 2) + (uint32_t)min(bn0 + col, g.N - 8) * 2;
    }
    int a_done = 0, w_done = 0, p_slot = 0;
    auto next_slot = [&]() { p_slot = p_slot == NSLOT - 1 ? 0 : p_slot + 1; };
    auto issue_a = [&]() {
        if (a_done >= total) return;
        blds16_x4(__builtin_amdgcn_readfirstlane(lds_base + p_slot * UNIT + wave * 4096),
                  __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(A + (size_t)a_done * BKT * g.lda), 0, min(rows_left0 - a_done * BKT, BKT) * g.lda * 2, 0x00020000),
                  offA[0], offA[1], offA[2], offA[3]);
        ++a_done;
        next_slot();
    };
    auto issue_w = [&]() {
        if (w_done >= total) return;
        blds16_x4(__builtin_amdgcn_readfirstlane(lds_base + p_slot * UNIT + wave * 4096),
                  __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(W + (size_t)w_done * BKT * g.ldw), 0, min(rows_left0 - w_done * BKT, BKT) * g.ldw * 2, 0x00020000),
                  offW[0], offW[1], offW[2], offW[3]);
        ++w_done;
        next_slot();
    };

    // ---- consumer: D[m][n] += sum_tokens dY[token][m] X[token][n]; lane (col = lane & 15, lq = lane >> 4) of accumulator [mb][nb] holds
    // C[mb*16 + 4*lq + e][nb*16 + col], e = 0..3 ----
    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // transposing fragment read of the 16-column block at image column c0, contraction slice kh (32 tokens): lane 4q'+p' of a 16-lane group
    // addresses token row t0 + q', columns c0 + 4p' .. + 3, t0 = 32 kh + 8 (lane >> 4) (+ 4 for the second read); lane i receives column i.
    // Everything lane-dependent is folded into two byte offsets per kh (first / second read); the block's column enters as XOR (c0 / 8) << 4.
    typedef __attribute__((ext_vector_type(4))) short s4;
    typedef __attribute__((address_space(3))) s4 *lds_s4;
    const int l16 = lane & 15, qp = l16 >> 2, pp = l16 & 3, lq = lane >> 4;
    int fro[2][2];
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
        for (int h4 = 0; h4 < 2; ++h4) {
            const int row = 32 * kh + 8 * lq + 4 * h4 + qp;
            fro[kh][h4] = row * 256 + ((((pp >> 1)) ^ (((row & 3) << 2) | ((row >> 2) & 3))) << 4) + 8 * (pp & 1);
        }
    uint4 fa[8], fw[4];
    auto frag = [&](const unsigned char *img, int c0, int kh) -> uint4 {
        union { s4 v[2]; uint4 u; } r;
        r.v[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(img + (fro[kh][0] ^ ((c0 >> 3) << 4))));
        r.v[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(img + (fro[kh][1] ^ ((c0 >> 3) << 4))));
        return r.u;
    };
    auto reads = [&](const unsigned char *sa, const unsigned char *sb, int kh) {
        // this wave's 128 dY columns are image wm of the dY unit; its 64 X columns are columns (wn & 1) * 64 .. of image wn >> 1 of the X unit
#pragma unroll
        for (int j = 0; j < 4; ++j) fw[j] = frag(sb + (wn >> 1) * IMG, (wn & 1) * 64 + j * 16, kh);
#pragma unroll
        for (int i = 0; i < 8; ++i) fa[i] = frag(sa + wm * IMG, i * 16, kh);
    };
    // Bias gradient beside the weight gradient (g.colsum): the column sums of dY are one more product of the dY fragments already in registers,
    // against a B operand of ones.  The 16-column fragments of a 128-column group are dealt over the tile columns (workgroups bn) and the four
    // waves that share them: fragment i belongs to the workgroup with bn % nbn == i % nbn and its wave wn == (i / nbn) % 4, slot i / (4 nbn) -
    // at most two extra MFMAs per 32 and wave (one from nbn = 2 on), instead of a separate pass over dY (colsum_vec_kernel: 1.9 ms per MAE step).
    const bool do_cs = g.colsum != nullptr;
    const int cs_b = pid % nbn;
    f32x4 csacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    const uint4 ones8 = make_uint4(0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u);
    auto cs_mine = [&](int i) -> bool { return (i % nbn) == cs_b && ((i / nbn) & 3) == wn && i / (4 * nbn) < 2; };
    auto mfmas = [&]() {
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fa[i]), __builtin_bit_cast(bf16x8, fw[j]), acc[i][j], 0, 0, 0);
        if (do_cs) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (cs_mine(i)) {   // (wave-uniform)
                    if (i / (4 * nbn) == 0) csacc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fa[i]), __builtin_bit_cast(bf16x8, ones8), csacc[0], 0, 0, 0);
                    else csacc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fa[i]), __builtin_bit_cast(bf16x8, ones8), csacc[1], 0, 0, 0);
                }
        }
    };
    issue_a();   // A(0)
    issue_w();   // W(0)
    issue_a();   // A(1)
    if (total > 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    PP_BAR();
    if (grp == 1) PP_BAR();   // G1 runs one segment behind
    int slot_a = 0;
    for (int q = 0; q < total; ++q) {
        const int slot_w = slot_a == NSLOT - 1 ? 0 : slot_a + 1;
        const unsigned char *sa = lds + slot_a * UNIT, *sb = lds + slot_w * UNIT;
        // ---- R(q, 0) ----
        issue_w();   // X(q+1) -> the slot dY(q-1) left
        reads(sa, sb, 0);
        PP_LGKM0();
        PP_BAR();
        // ---- M(q, 0) ----
        mfmas();
        PP_BAR();
        // ---- R(q, 1) ----
        issue_a();   // dY(q+2) -> the slot X(q-1) left
        reads(sa, sb, 1);
        PP_LGKM0();
        if (grp == 1 && q + 1 < total) {
            if (q + 2 < total) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        PP_BAR();
        // ---- M(q, 1) ----
        mfmas();
        if (grp == 0 && q + 1 < total) {
            if (q + 2 < total) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        PP_BAR();
        slot_a = slot_a + 2 >= NSLOT ? slot_a + 2 - NSLOT : slot_a + 2;
    }
    if (grp == 0) PP_BAR();
    if (do_cs && (lane & 15) == 0) {   // every column n of the 16x16 result holds the same sums: lanes with n = 0 add rows 4 lq .. 4 lq + 3
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (cs_mine(i)) {
                const f32x4 v = i / (4 * nbn) == 0 ? csacc[0] : csacc[1];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int m = bm0 + wm * 128 + i * 16 + 4 * lq + e;
                    if (m < g.M) atomicAdd(g.colsum + m, v[e]);
                }
            }
    }
    // ---- split-K accumulation: four 64-byte row segments per wave instruction ----
    const int m0 = bm0 + wm * 128 + 4 * lq, n0 = bn0 + wn * 64 + (lane & 15);
#pragma unroll
    for (int mb = 0; mb < 8; ++mb) {
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int col = n0 + nb * 16;
            if (col < g.N) {
                float *base = reinterpret_cast<float *>(g.C) + (size_t)(m0 + mb * 16) * g.ldc + col;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (m0 + mb * 16 + e < g.M) atomicAdd(base + (size_t)e * g.ldc, acc[mb][nb][e]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

#undef PP_BAR
#undef PP_LGKM0

}  // namespace

void gemm_launch_pp(const AcaiGemmLaunch &l, const GemmArgs &g, hipStream_t st) {
    const dim3 grid(l.grid), block(l.block);
    if (l.kernel == ACAI_GEMM_K_TN_PP) {
        hipLaunchKernelGGL(gemm_tn_pp_kernel, grid, block, 0, st, g);
        return;
    }
    switch (l.pp_mode) {
#define PP_CASE(M) case (M): hipLaunchKernelGGL((gemm_nt_pp_kernel<bf16_t, (M)>), grid, block, 0, st, g); break
        PP_CASE(PP_OBF | PP_GELU | PP_AUX1 | PP_DEFER);
        PP_CASE(PP_OBF | PP_AUX2 | PP_DEFER);
        PP_CASE(PP_OBF);
        PP_CASE(PP_OBF | PP_SCALE);
        PP_CASE(PP_OBF | PP_GELU | PP_AUX1);
        PP_CASE(PP_OBF | PP_AUX2);
        PP_CASE(PP_OBF | PP_GELU | PP_AUX3);
        PP_CASE(PP_OBF | PP_AUX4);
        PP_CASE(0);
        PP_CASE(PP_RES);
#undef PP_CASE
        default: break;   // unreachable: pp_mode_ok() sent every other form to variant 6
    }
}
