// Which kernels a GEMM call runs: the selection rule of the C ABI entries in gemm.hip as ONE pure function of a plain query
// (AcaiGemmQuery -> at most two AcaiGemmLaunch, include/acai_omr_hip.h).  Plain C++17: no HIP call, no getenv, no static state, so it
// compiles with the host compiler alone and tests/test_gemm_plan_cpu.py calls it (acai_gemm_plan) without a GPU.  Every threshold below is
// measured; the tools named next to each one reproduce it.
#pragma once
#include <stddef.h>

#include "../../include/acai_omr_hip.h"

// epilogue form of a launch as gemm_nt_pp_kernel's MODE (AcaiGemmLaunch.pp_mode)
enum { PP_OBF = ACAI_PP_OBF, PP_GELU = ACAI_PP_GELU, PP_AUX1 = ACAI_PP_AUX1, PP_AUX2 = ACAI_PP_AUX2, PP_RES = ACAI_PP_RES,
       PP_SCALE = ACAI_PP_SCALE, PP_DEFER = ACAI_PP_DEFER, PP_AUX3 = ACAI_PP_AUX3, PP_AUX4 = ACAI_PP_AUX4 };

constexpr int GEMM_MAX_LAUNCHES = 2;

static inline int gemm_cdiv(int a, int b) { return (a + b - 1) / b; }

static inline int pp_mode(const AcaiGemmQuery &q) {
    return (q.out_dtype == ACAI_BF16 ? PP_OBF : 0) | ((q.flags & ACAI_GEMM_GELU) ? PP_GELU : 0) | (q.aux_mode == 1 ? PP_AUX1 : 0) | (q.aux_mode == 2 ? PP_AUX2 : 0) |
           (q.aux_mode == 3 ? PP_AUX3 : 0) | (q.aux_mode == 4 ? PP_AUX4 : 0) |
           (q.has_residual ? PP_RES : 0) | (q.scale_cols > 0 ? PP_SCALE : 0);
}
// ... and the forms it is instantiated for (the others keep variant 6)
static inline bool pp_mode_ok(int m) {
    return m == PP_OBF || m == (PP_OBF | PP_SCALE) || m == (PP_OBF | PP_GELU | PP_AUX1) || m == (PP_OBF | PP_AUX2) || m == 0 || m == PP_RES ||
           m == (PP_OBF | PP_GELU | PP_AUX3) || m == (PP_OBF | PP_AUX4);
}

// One row-major LDS-DMA launch over `M` rows starting at `row0` (bf16: K % 64 == 0, fp32: K % 32 == 0, 16-byte chunks).  variant
// (acai_gemm_set_variant; tests and A/B runs): 0 auto, 1 128x128 two-stage, 2 256x128 two-stage, 3 256x128 three-stage, 4 256x128 persistent
// three-stage ring, 5 256x256 two-stage, 6 persistent 256x256 ring of half-stages, 7 ping-pong ring with the register epilogue, 8 = 7 with
// the GELU forms' deferred epilogue.  A pinned variant falls back 7 -> 6 -> 5 where its kernel has no such instantiation, and 4 / 5 / 6 / 7 -> 1
// under 8 tiles.
static inline AcaiGemmLaunch gemm_plan_rowmajor(const AcaiGemmQuery &q, int row0, int M, int vec_epi) {
    const bool bf16_lin = q.elem_size == 2 && q.epi == 0;   // what the persistent 256x256 ring and the ping-pong ring are instantiated for
    const int n_cu = q.n_cu, ktiles = q.K / (128 / q.elem_size);
    const int nwg = gemm_cdiv(M, 128) * gemm_cdiv(q.N, 128), nwg4 = gemm_cdiv(M, 256) * gemm_cdiv(q.N, 128), nwg256 = gemm_cdiv(M, 256) * gemm_cdiv(q.N, 256);
    int v = q.variant;
    bool defer = false;   // variant 8 = 7 with the GELU forms' deferred epilogue (PP_DEFER: measured slower, kept as an experiment - see there)
    if (v == 8) {
        v = 7;
        defer = true;
    }
    // auto (tools/bench_gemm.py, bf16): up to 24 K-tiles the persistent ring wins (0.61-0.71 PF on K = 512..768 against 0.53-0.64 for
    // one tile per workgroup); from 64 K-tiles the 256x256 tile does (1.00-1.02 PF at 4096^3 / 8192^3 against 0.95-0.98); between, the
    // three-stage 256x128 kernel; small problems keep two 128x128 workgroups per CU.
    // (fp32: the 256x256 tile never beats the three-stage kernel - 102 against 137 TF at 32768 x 768 x 3072 - and a K-tile is 32 floats)
    // The 256x256 tile only when its tiles fill whole rounds of the chip (260 tiles on 256 CUs are two rounds: 16416 x 1024 x 4096 took
    // 240 us on it against 170 us on the 128x128 kernel, tools/bench_gemm_tf.py); long-K problems of only a few rounds then go to the
    // 128x128 kernel, whose two co-resident workgroups cover each other (170 against 192 us for the three-stage tile there).
    const int rounds256 = gemm_cdiv(nwg256, n_cu);
    const bool fills256 = nwg256 >= n_cu && nwg256 * 100 >= rounds256 * n_cu * 85;
    if (v == 0)
        v = nwg4 >= 512 ? (ktiles <= 24 ? 4 : (q.elem_size == 2 && ktiles >= 64 ? (fills256 ? 5 : (nwg4 < 4 * n_cu ? 1 : 3)) : 3)) : 1;
    // Mid-size problems at 16-24 K-tiles (the teacher-forced decoder stream: 8208 rows, K = 1024): two co-resident 128x128 workgroups beat the
    // persistent ring until it has ~8 rounds of tiles to run across (tools/bench_gemm_tf.py: N = 3072 89 -> 80 us, N = 4096 116 -> 100 us at
    // M = 8208; still ahead at M = 20000)
    if (q.variant == 0 && v == 4 && ktiles >= 16 && nwg4 < 2048) v = 1;
    if (q.variant == 0 && bf16_lin) {
        // The persistent 256x256 ring of half-stages (6) where its tiles fill whole rounds of the chip (>= 95 %): 1.5x the flops per staged byte
        // pays on the decoder's 131072-token GEMMs and on N = 3072 (tools/bench_mae_gemms.py: lin1 + GELU 977 -> 868 us, lin2 537 -> 481,
        // dX of the in-projection 346 -> 307); it loses where a quarter of the last round idles (N = 768: 384 tiles) and ties on K = N = 512.
        if ((v == 4 || v == 3) && ktiles < 64 && nwg256 >= n_cu && nwg256 * 100 >= rounds256 * n_cu * 95 && !(q.N <= 512 && ktiles <= 8)) v = 6;
        // Wherever one of the large-tile kernels was chosen, the ping-pong ring (7) replaces it when the launch has one of its epilogue
        // forms (tools/bench_pp.py, MAE step shapes, same box: every shape faster - 0.82-1.02 PF on the plain / residual forms against 0.32-0.84).
        if (v >= 3 && v <= 6) v = 7;
        // ... and it replaces the 128x128 kernel on mid-size problems when it needs fewer rounds of the chip: 128x128 tiles run two workgroups
        // per CU, a 256x256 tile (four of them) takes ~1.54 of their tile times on the ring.  The teacher-forced decoder stream (M = 16 x 513
        // = 8208 rows: 520 tiles of 128x128 at N = 1024, two rounds for 1.02 rounds of work) is the case: 37.9 -> 31.8 us at K = 1024,
        // 111.8 -> 96.0 us at K = 4096, N = 3072 76.7 -> 60.7 us (tools/bench_gemm_tf.py); M = 8192 (exactly one round) keeps the 128x128 kernel.
        if (v == 1 && nwg256 >= 8) {
            const int rounds1 = gemm_cdiv(nwg, 2 * n_cu), rounds7 = gemm_cdiv(nwg256, n_cu);
            if (rounds7 * 154 < rounds1 * 100) v = 7;
        }
    }
    if (v == 7) {   // the register epilogue addresses C / residual / aux through 32-bit buffer offsets
        const size_t lim = 0xFFFFFF00ull, esz = q.out_dtype == ACAI_BF16 ? 2 : 4;
        const bool fits = (size_t)M * q.ldc * esz < lim && (!q.has_residual || (size_t)M * q.ldr * 4 < lim) && (!q.aux_mode || (size_t)M * q.ldaux * esz < lim);
        const bool src32 = (size_t)q.lda * 2 < (1u << 24) && (size_t)q.ldw * 2 < (1u << 24);   // 24-bit multiplies in the lane offsets of the LDS-DMA sources
        if (!bf16_lin || !fits || !src32 || !vec_epi || !pp_mode_ok(pp_mode(q))) v = 6;
    }
    if ((v == 5 || v == 6 || v == 7) && nwg256 < 8) v = 1;
    if (v == 4 && nwg4 < 8) v = 1;
    if (v == 6 && !bf16_lin) v = 5;

    AcaiGemmLaunch l{};
    l.vec_epi = vec_epi;
    l.row0 = row0;
    l.rows = M;
    l.k = q.K;
    l.block = 512;
    switch (v) {
        case 7:
            l.kernel = ACAI_GEMM_K_PP;
            l.grid = nwg256 < n_cu ? nwg256 : n_cu;
            l.pp_mode = pp_mode(q);
            // the GELU forms can defer their GELU step into the next tile's R segments (see PP_DEFER) when a tile has enough of them;
            // off by default: 833 against 686 us on the MAE decoder's lin1, 962 against 825 us on its gelu' GEMM (tools/bench_pp.py)
            if (defer && ktiles >= 8 && (l.pp_mode == (PP_OBF | PP_GELU | PP_AUX1) || l.pp_mode == (PP_OBF | PP_AUX2))) l.pp_mode |= PP_DEFER;
            break;
        case 6: l.kernel = ACAI_GEMM_K_PERS256; l.grid = nwg256 < n_cu ? nwg256 : n_cu; break;
        case 5: l.kernel = ACAI_GEMM_K_256; l.grid = nwg256; break;
        case 4: l.kernel = ACAI_GEMM_K_PERS; l.grid = nwg4 < n_cu ? nwg4 : n_cu; break;
        case 3: l.kernel = ACAI_GEMM_K_GLDS3; l.grid = nwg4; break;
        case 2: l.kernel = ACAI_GEMM_K_GLDS; l.wm = 4; l.grid = nwg4; break;
        default: l.kernel = ACAI_GEMM_K_GLDS; l.wm = 2; l.grid = nwg; l.block = 256; break;
    }
    return l;
}

// The plan of one GEMM call: writes 1 or 2 launches to `out` and returns how many.
static inline int gemm_plan(const AcaiGemmQuery &q, AcaiGemmLaunch *out) {
    const int EPC = 16 / q.elem_size, BKE = 128 / q.elem_size;   // elements per 16-byte chunk / per K-tile
    const bool TA = q.trans_a, TB = q.trans_w, dw = TA && TB && q.epi == 0;
    // 16-byte chunks run along K for row-major operands and along the row index for transposed ones
    const bool fast = (q.lda % EPC == 0) && (q.ldw % EPC == 0) && q.a_aligned && q.w_aligned && (TA ? q.M % EPC == 0 : q.K % EPC == 0) &&
                      (TB ? q.N % EPC == 0 : q.K % EPC == 0);
    // C (and the residual / aux) allow 16-byte row accesses -> LDS-transposed epilogue
    const int vec_epi = (q.epi == 0) && (q.ldc % 8 == 0) && (q.N % 8 == 0) && q.c_aligned && (!q.has_residual || (q.ldr % 4 == 0 && q.r_aligned)) &&
                        (!q.aux_mode || (q.ldaux % 8 == 0 && q.aux_aligned));
    int nwg = gemm_cdiv(q.M, 128) * gemm_cdiv(q.N, 128), ksplit = 0;
    if (dw) {
        // dW = dY^T X: few output tiles, K = number of rows (1e4..1e5): split K until ~3 workgroups per CU exist
        const int nkt = gemm_cdiv(q.K, BKE);
        int ks = gemm_cdiv(768, nwg);
        ks = ks < 1 ? 1 : (ks > nkt / 4 ? (nkt / 4 < 1 ? 1 : nkt / 4) : ks);
        ksplit = ks;
        nwg *= ks;
    }
    AcaiGemmLaunch l{};
    l.vec_epi = vec_epi;
    l.rows = q.M;
    l.k = q.K;
    l.ksplit = ksplit;
    if (dw && q.elem_size == 2 && fast && q.K >= 64 && q.M % 8 == 0 && q.N % 8 == 0 && q.M >= 8 && q.N >= 8) {
        // Token counts that are not a multiple of 64 (16 x 513 decoder tokens): the ring and ping-pong kernels take the ragged last tile
        // themselves - out-of-range rows of a buffer LDS-DMA arrive as zeros; the two-stage kernel takes the whole 64-token tiles and the
        // register-staged kernel accumulates the remaining rows into the same gradient.
        // The three-stage ring (256 x 128 tiles, one workgroup per CU) when the reduction is long enough to fill it: split K until ~256
        // workgroups exist - one resident workgroup per CU, never more workgroups than CUs (a second, nearly empty round doubles the time)
        const int tiles_r = gemm_cdiv(q.M, 256) * gemm_cdiv(q.N, 128), nkt_r = gemm_cdiv(q.K, 64);
        int ks_r = 256 / tiles_r;
        if (ks_r < 1) ks_r = 1;
        if (ks_r > nkt_r / 8) ks_r = nkt_r / 8;
        // the ping-pong form (256 x 256 tiles) where the operands' lane offsets fit 32 bits
        const int tiles_p = gemm_cdiv(q.M, 256) * gemm_cdiv(q.N, 256);
        int ks_p = 256 / tiles_p;
        if (ks_p < 1) ks_p = 1;
        if (ks_p > nkt_r / 8) ks_p = nkt_r / 8;
        const bool pp_fits = (size_t)64 * q.lda * 2 + (size_t)q.M * 2 < 0xFFFFFF00ull && (size_t)64 * q.ldw * 2 + (size_t)q.N * 2 < 0xFFFFFF00ull;
        // (short K-slices keep the 256 x 128 ring: with fewer than ~24 K-steps per workgroup the atomics of the larger tile's extra
        // splits cost more than the main loop gains - encoder dWo, 768 x 768 from 32768 tokens: 82 us on the ring, 89 us here)
        if (ks_p >= 1 && nkt_r >= 16 && pp_fits && nkt_r / ks_p >= 24) {
            l.kernel = ACAI_GEMM_K_TN_PP;
            l.grid = tiles_p * ks_p;
            l.block = 512;
            l.ksplit = ks_p;
            l.colsum = q.want_colsum != 0;   // only the ping-pong kernel forms the column sums itself
        } else if (ks_r >= 1 && nkt_r >= 16 && pp_fits) {
            l.kernel = ACAI_GEMM_K_TN_RING;
            l.grid = tiles_r * ks_r;
            l.block = 512;
            l.ksplit = ks_r;
        } else {
            const int k64 = q.K - q.K % 64;
            l.kernel = ACAI_GEMM_K_TN_GLDS;
            l.grid = nwg;
            l.block = 256;
            l.k = k64;
            if (k64 < q.K) {
                out[0] = l;
                AcaiGemmLaunch t{};
                t.kernel = ACAI_GEMM_K_REG;
                t.fast = 1;
                t.grid = gemm_cdiv(q.M, 128) * gemm_cdiv(q.N, 128);
                t.block = 256;
                t.ksplit = 1;
                t.vec_epi = vec_epi;
                t.rows = q.M;
                t.k0 = k64;
                t.k = q.K - k64;
                out[1] = t;
                return 2;
            }
        }
        out[0] = l;
        return 1;
    }
    if (fast && !TA && !TB && q.K % BKE == 0) {
        // A few rows past a multiple of 256 (the teacher-forced decoder stream: 16 x 513 = 8208 = 32 x 256 + 16 rows) can cost a whole round of tiles:
        // N = 4096 is 528 tiles of 256 x 256 on 256 CUs (three rounds for 2.06 of work: 86 us against 65 at M = 8192), N = 1024 is 520 tiles of
        // 128 x 128 on 512 resident workgroups (two rounds for 1.02: 33.5 us against 25.7; K = 4096: 99 against 74).  Where the full 256-row part
        // alone saves such a round, it is planned by itself (the auto rule then picks what it picks for a round number) and the remainder rows
        // follow as a second, small launch of the same epilogue form (tools/bench_gemm_tf.py).
        const int rem = q.M % 256, Mm = q.M - rem;
        if (q.elem_size == 2 && q.epi == 0 && q.variant == 0 && rem > 0 && rem <= 32 && Mm >= 4096) {
            const int nbn256 = gemm_cdiv(q.N, 256), full256 = gemm_cdiv(q.M, 256) * nbn256, main256 = (Mm / 256) * nbn256;
            // (measured, tools/bench_gemm_tf.py, M = 8208: N = 4096 90.5 -> 81.5 us, N = 2048 59.7 -> 49.8.  The other case - N = 1024, where the
            // 8192-row part is exactly one round of 128 x 128 tiles - LOSES: the 16-row remainder takes 16 us at K = 1024 and 46 us at K = 4096 on
            // the eight workgroups of the generic kernel, 41.7 against 33.5 us and 121 against 101 us in all; it would need a skinny kernel with
            // the training epilogue forms, so that rule is not applied)
            if (main256 >= q.n_cu && gemm_cdiv(main256, q.n_cu) < gemm_cdiv(full256, q.n_cu)) {
                out[0] = gemm_plan_rowmajor(q, 0, Mm, vec_epi);
                out[1] = gemm_plan_rowmajor(q, Mm, rem, vec_epi);
                return 2;
            }
        }
        out[0] = gemm_plan_rowmajor(q, 0, q.M, vec_epi);
        return 1;
    }
    l.kernel = ACAI_GEMM_K_REG;
    l.fast = fast;
    l.grid = nwg;
    l.block = 256;
    out[0] = l;
    return 1;
}
