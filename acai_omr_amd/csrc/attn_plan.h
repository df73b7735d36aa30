// Which kernels a varlen attention call runs: the selection rule of acai_attn_varlen_fwd / acai_attn_varlen_bwd[_ws] (attn.hip) as ONE pure
// function of a plain query (AcaiAttnQuery -> at most four AcaiAttnLaunch, include/acai_omr_hip.h).  Plain C++17: no HIP call, no getenv, no
// static state, so it compiles with the host compiler alone and tests/test_attn_plan_cpu.py calls it (acai_attn_plan) without a GPU.  A launch
// carries every argument the host decides (tail, tail256, nblk, ...): the launchers in the kernel files decide nothing.  Every threshold
// below is measured; the tools named next to each one reproduce it.
#pragma once
#include <limits.h>
#include <stddef.h>

#include "../../include/acai_omr_hip.h"

constexpr int ATTN_MAX_LAUNCHES = 4;
// what the kernel files fix and the plan has to know (each file static_asserts its own figure against these)
constexpr int ATTN_BWD_TT = 64;             // attn_bwd.hip: streamed-side rows per tile
constexpr int ATTN_BWD1P_LDS = 153088;      // attn_bwd1p.hip: LDS_TOTAL
// row pitch in bytes of TileLayout<ES, DHP> (common.h): swizzled bf16 rows, fp32 rows padded by 16 bytes
constexpr int attn_tile_pitch(int es, int dhp) { return es == 2 ? dhp * 2 : dhp * 4 + 16; }
// bytes of workspace the one-pass backward needs: the fp32 query gradient the key blocks add into.  (64 rows more than the gradient: a
// workgroup's first two tiles "add" the zero-filled partial sets to the sequence's first 64 rows without a range check - for a sequence
// shorter than that, or the last one, those adds of 0.0 land in the next sequence's rows or in the padding)
static inline size_t attn_bwd1p_workspace(int total_q, int H) { return ((size_t)total_q + 64) * H * 32 * sizeof(float); }

static inline int attn_cdiv(int a, int b) { return (a + b - 1) / b; }

// XCD-aware block order of the one-dimensional attention grids: on for batches the host knows to be equal-length, off for ragged ones (the
// static split of the (sequence, head) pairs over the XCDs leaves the one with the longest sequences working alone at the end: attn_bwd1p.hip
// has the measurement).  ACAI_ATTN_OV_XCD_ORDER = 0 / 1 forces it off / on for the d_h = 64 kernels; the one-pass backward follows equal_len alone.
static inline bool attn_xcd_order(const AcaiAttnQuery &q, bool equal_len) {
    const int force = q.ov[ACAI_ATTN_OV_XCD_ORDER];
    return force < 0 ? equal_len : force != 0;
}

static inline AcaiAttnLaunch attn_launch_3d(int kernel, const AcaiAttnQuery &q, int rows, int rows_per_wg, int block, int lds_bytes) {
    AcaiAttnLaunch l{};
    l.kernel = kernel;
    l.grid_x = attn_cdiv(rows, rows_per_wg);
    l.grid_y = q.H;
    l.grid_z = q.B;
    l.block = block;
    l.lds_bytes = lds_bytes;
    l.rows = rows;
    return l;
}
// the kernels with a one-dimensional grid of nblk blocks per (sequence, head); nblk is handed over negative for the plain block order
static inline AcaiAttnLaunch attn_launch_1d(int kernel, const AcaiAttnQuery &q, int nblk, int rows_per_blk, bool xcd, int lds_bytes) {
    AcaiAttnLaunch l{};
    l.kernel = kernel;
    l.grid_x = nblk * q.H * q.B;
    l.grid_y = l.grid_z = 1;
    l.block = 256;
    l.lds_bytes = lds_bytes;
    l.nblk = xcd ? nblk : -nblk;
    l.rows = nblk * rows_per_blk;
    return l;
}

// attn_fwd_kernel / attn_bwd_dq_kernel / attn_bwd_dkv_kernel: the template form of an instantiation
static inline AcaiAttnLaunch attn_with_form(AcaiAttnLaunch l, const AcaiAttnQuery &q, bool fast, int nq) {
    l.elem_size = q.elem_size;
    l.dhp = q.dh <= 32 ? 32 : 64;
    l.fast = fast;
    l.drop = q.dropout != 0;
    l.pre = q.q_prescaled != 0;
    l.nq = nq;
    return l;
}

// bf16, d_h = 64 exactly, q prescaled, no dropout, no causal mask, aligned operands (attn_fwd64.hip, attn_fwd64w.hip)
static inline int attn_plan_fwd64(const AcaiAttnQuery &q, AcaiAttnLaunch *out) {
    const int form = q.ov[ACAI_ATTN_OV_FWD64];
    if (form == ACAI_ATTN_FWD64_NW4 || form == ACAI_ATTN_FWD64_NW8) {   // the 32-queries-per-wave kernel everywhere (A/B aid)
        const int nw = form == ACAI_ATTN_FWD64_NW8 ? 8 : 4;
        out[0] = attn_launch_3d(ACAI_ATTN_K_FWD64, q, q.max_q, 32 * nw, 64 * nw, 0);
        out[0].waves = nw;
        return 1;
    }
    // 64 queries per wave, one wave per SIMD, with a tail launch.  A sequence's last 256-query block goes to the tail kernel when it holds
    // <= 32 rows.  When every sequence is max_q long (B * max_q rows in all) the host knows whether such a tail exists and launches only what
    // is needed; were that reading of the arguments wrong, the wide kernel (tail = 0) still covers every row.
    const bool all_equal = (long long)q.B * q.max_q == (long long)q.total_q;
    const int rem = q.max_q % 256;
    const bool need_tail = !all_equal || (rem > 0 && rem <= 32);
    const int tail = need_tail ? 32 : 0;
    // (equal lengths: the wide grid covers the full blocks only - workgroups that exit at once still wait for a whole free CU each, one
    // per (sequence, head): 192 against 147 us on the decoder's 513-query cross attention)
    const int wide_q = (all_equal && need_tail) ? q.max_q - rem : q.max_q;
    int n = 0;
    if (wide_q > 0) {
        // (the order follows the rows of THIS launch: an equal-length batch whose tail went to the tail kernel counts as ragged here)
        const bool xcd = attn_xcd_order(q, (long long)q.B * wide_q == (long long)q.total_q);
        out[n] = attn_launch_1d(ACAI_ATTN_K_FWD64W, q, attn_cdiv(wide_q, 256), 256, xcd, 0);
        out[n].rows = wide_q;
        out[n++].tail = tail;
    }
    if (need_tail) {
        out[n] = attn_launch_3d(ACAI_ATTN_K_FWD64_TAIL, q, 32, 32, 512, 0);
        out[n++].tail = tail;
    }
    return n;
}

static inline int attn_plan_fwd(const AcaiAttnQuery &q, AcaiAttnLaunch *out, int *refusal) {
    const int EPC = 16 / q.elem_size, QB = 128;   // elements per 16-byte chunk; queries per workgroup
    const bool fast = (q.dh % EPC == 0) && (q.ldq % EPC == 0) && (q.ldk % EPC == 0) && (q.ldv % EPC == 0) && (q.ldo % EPC == 0) && q.aligned;
    // train-mode attention dropout is its own instantiation, so the common kernel carries no hash code / registers; the prescaled-q form
    // (training path) exists for 16-byte-aligned operands only
    if (q.q_prescaled && !fast) {
        *refusal = ACAI_ATTN_REFUSE_PRESCALED;
        return 0;
    }
    int nq = 1;
    if (q.q_prescaled && !q.dropout && q.elem_size == 2) {
        // d_h = 64 exactly, no causal mask: the software-pipelined kernels of attn_fwd64.hip / attn_fwd64w.hip
        if (q.dh == 64 && !q.causal && q.ov[ACAI_ATTN_OV_FWD64] != ACAI_ATTN_FWD64_GENERIC) return attn_plan_fwd64(q, out);
        // the training steps' form: two query blocks per wave when the sequences are long enough to fill the chip
        // (d_h = 64 keeps one block: two need 256 registers + 55 spilt even with the zero reference, and measured 5 % slower - 0.97 against 0.92 ms)
        if (q.dh <= 32 && q.ov[ACAI_ATTN_OV_TWO_BLOCK] && q.max_q >= 512) nq = 2;
    }
    out[0] = attn_with_form(attn_launch_3d(ACAI_ATTN_K_FWD, q, q.max_q, nq * QB, 256, 0), q, fast, nq);
    return 1;
}

static inline int attn_plan_bwd(const AcaiAttnQuery &q, AcaiAttnLaunch *out, int *refusal) {
    const int ES = q.elem_size, EPC = 16 / ES, OB = 128;   // lane-owned rows per workgroup of attn_bwd.hip
    const int dhp = q.dh <= 32 ? 32 : 64;
    const int max_q = q.max_q, max_k = q.max_k;
    const bool fast = (q.dh % EPC == 0) && (q.ldq % EPC == 0) && (q.ldk % EPC == 0) && (q.ldv % EPC == 0) && (q.lddo % EPC == 0) && (q.ldo % EPC == 0) &&
                      (q.lddq % EPC == 0) && (q.lddk % EPC == 0) && (q.lddv % EPC == 0) && q.aligned &&   // vector stores of the gradients too
                      (size_t)max_q * (size_t)(q.ldq > q.lddo ? q.ldq : q.lddo) * ES < 0x7FFFFF00ull &&
                      (size_t)max_k * (size_t)(q.ldk > q.ldv ? q.ldk : q.ldv) * ES < 0x7FFFFF00ull;         // the staging's 32-bit buffer resources
    const int RP = attn_tile_pitch(ES, dhp);
    const int lds_dq = 2 * (2 * ATTN_BWD_TT * RP), lds_dkv = 2 * (2 * ATTN_BWD_TT * RP + 2 * ATTN_BWD_TT * (int)sizeof(float));   // two stages each
    if (q.q_prescaled && !fast) {
        *refusal = ACAI_ATTN_REFUSE_PRESCALED;
        return 0;
    }
    if (q.accum_dkv && !(ES == 2 && fast)) {
        *refusal = ACAI_ATTN_REFUSE_ACCUM;
        return 0;
    }
    const bool training_form = ES == 2 && q.q_prescaled && !q.dropout;   // (prescaled: aligned operands)
    if (training_form && dhp == 32) {
        // One pass over the scores (attn_bwd1p.hip) when the caller lent a workspace and the sequences are long (short ones keep the two-kernel
        // form: a workgroup's prologue weighs more); 32-bit byte offsets into one sequence's [max_q][H][32] fp32 rows.  ACAI_ATTN_OV_BWD_1P = 0
        // keeps the two kernels below, whose dQ is bit-reproducible - the one-pass form adds the key blocks' contributions to a query's
        // gradient in arrival order.
        if (q.ov[ACAI_ATTN_OV_BWD_1P] && q.dh == 32 && !q.causal && !q.accum_dkv && max_k >= 512 && max_q >= 512 &&
            (long long)(max_q + 64) * q.H * 128 < 0x7FFFFF00ll && q.workspace_bytes > 0 &&
            (unsigned long long)q.workspace_bytes >= attn_bwd1p_workspace(q.total_q, q.H)) {
            // equal_len: the host can tell that all sequences have max_q queries and max_k keys (the XCD-aware block order); when max_k is a
            // multiple of 512 as well, the slot for the keys past a sequence's last full 512-key block is left out
            const bool eq = q.total_k > 0 && (long long)q.B * max_k == (long long)q.total_k && (long long)q.B * max_q == (long long)q.total_q;
            const int partial = eq && max_k % 512 == 0 ? 0 : 1;
            AcaiAttnLaunch l = attn_launch_1d(ACAI_ATTN_K_BWD1P, q, max_k / 512 + partial, 512, true, ATTN_BWD1P_LDS);
            l.tail256 = eq ? 1 : 0;   // (this kernel's use of the field: the XCD-aware block order)
            l.partial_blocks = partial;
            l.equal_len = eq ? 1 : 0;
            out[0] = l;
            return 1;
        }
        // the training steps' form on long sequences: two lane-owned blocks per wave
        if (q.ov[ACAI_ATTN_OV_TWO_BLOCK] && !q.causal && !q.accum_dkv && max_q >= 512 && max_k >= 512) {
            out[0] = attn_launch_3d(ACAI_ATTN_K_BWD_DQ2, q, max_q, 2 * OB, 256, lds_dq);
            out[1] = attn_launch_3d(ACAI_ATTN_K_BWD_DKV2, q, max_k, 2 * OB, 256, lds_dkv);
            out[0].nq = out[1].nq = 2;
            return 2;
        }
    }
    const int wide = q.ov[ACAI_ATTN_OV_BWD64_WIDE];
    if (training_form && wide && !q.causal && q.dh == 64) {
        // the training steps' d_h = 64 form: one wave per SIMD, two lane-owned blocks per wave (attn_bwd64w.hip) over every sequence's full
        // 256-row blocks; the rows past them (none for the encoder's 256-multiples, one for the decoder's 513 tokens) stay with the
        // one-block kernels, offset by tail256.  ACAI_ATTN_OV_BWD64_WIDE: 0 off, 1 dQ only, 2 dK/dV only, 3 both; -1 = auto.
        // Measured (tools/bench_cross_train_attn.py, 16 x 16 heads, same box): the wide dQ form is 1-5 % faster than the one-block kernel
        // (encoder 4096 x 4096: 1533 against 1561 us; decoder cross 512 x 4096: 184 against 210 us).  The wide dK/dV form is 10 % faster on the
        // encoder (1886 against 2091 us; 16 x 12 heads: backward 2.51 against 2.63 ms) once its K / V fragments were pinned to the accumulator
        // half (before that it spilt to scratch and ran 2894 us), but SLOWER where the streamed query loop is short (decoder cross attention,
        // 513 queries: 9 tiles per workgroup, 663 against 607 us for the pair - one wave per SIMD has nobody to cover a workgroup's prologue):
        // auto takes it from 2048 streamed queries on.  Why the gains are small: every d_h = 64 attention kernel executes ~1 PFLOP/s of MFMA
        // work, the rate this chip sustains at its loaded clock.
        const bool wq = (wide & 1) && max_q >= 256, wk = (wide & 2) && max_k >= 256 && !q.accum_dkv && (wide > 0 || max_q >= 2048);
        // when every sequence is max_q long (B * max_q rows in all) the host knows whether a tail exists; keys: only for self-attention
        const bool eq_q = (long long)q.B * max_q == (long long)q.total_q, eq_k = eq_q && q.cu_k_is_cu_q && max_k == max_q;
        int n = 0;
        if (wq) out[n++] = attn_launch_1d(ACAI_ATTN_K_BWD64W_DQ, q, max_q / 256, 256, attn_xcd_order(q, eq_q), 0);
        if (!wq || !eq_q || max_q % 256) {
            const int rows = wq ? (eq_q ? max_q % 256 : 255) : max_q;
            out[n] = attn_with_form(attn_launch_3d(ACAI_ATTN_K_BWD_DQ, q, rows, OB, 256, lds_dq), q, fast, 1);
            out[n++].tail256 = wq ? 1 : 0;
        }
        if (wk) out[n++] = attn_launch_1d(ACAI_ATTN_K_BWD64W_DKV, q, max_k / 256, 256, attn_xcd_order(q, eq_k), 0);
        if (!wk || !eq_k || max_k % 256) {
            const int rows = wk ? (eq_k ? max_k % 256 : 255) : max_k;
            out[n] = attn_with_form(attn_launch_3d(ACAI_ATTN_K_BWD_DKV, q, rows, OB, 256, lds_dkv), q, fast, 1);
            out[n++].tail256 = wk ? 2 : 0;
        }
        return n;
    }
    out[0] = attn_with_form(attn_launch_3d(ACAI_ATTN_K_BWD_DQ, q, max_q, OB, 256, lds_dq), q, fast, 1);
    out[1] = attn_with_form(attn_launch_3d(ACAI_ATTN_K_BWD_DKV, q, max_k, OB, 256, lds_dkv), q, fast, 1);
    return 2;
}

// The plan of one attention call: writes up to ATTN_MAX_LAUNCHES launches to `out` and returns how many; 0 with *refusal set when the call
// is refused.
static inline int attn_plan(const AcaiAttnQuery &q, AcaiAttnLaunch *out, int *refusal) {
    *refusal = ACAI_ATTN_REFUSE_NONE;
    return q.backward ? attn_plan_bwd(q, out, refusal) : attn_plan_fwd(q, out, refusal);
}

// acai_attn_varlen_bwd_workspace_bytes: what a backward call with these arguments, aligned packed operands and all the workspace it may
// want would take
static inline size_t attn_plan_workspace_bytes(AcaiAttnQuery q) {
    q.backward = 1;
    q.aligned = 1;
    q.ldq = q.ldk = q.ldv = q.ldo = q.lddo = q.lddq = q.lddk = q.lddv = q.H * q.dh;
    q.workspace_bytes = LLONG_MAX;
    AcaiAttnLaunch l[ATTN_MAX_LAUNCHES];
    int refusal = 0;
    return attn_plan(q, l, &refusal) == 1 && l[0].kernel == ACAI_ATTN_K_BWD1P ? attn_bwd1p_workspace(q.total_q, q.H) : 0;
}
