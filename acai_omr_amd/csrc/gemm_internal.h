// Internal interface between the GEMM sources (gemm.hip: C ABI entries and the launch switch; gemm_tile.hip, gemm_ring.hip, gemm_pp.hip: the
// kernels by family).  Not installed and not part of the C ABI (include/acai_omr_hip.h).  The __device__ helpers that more than one kernel
// file uses are in gemm_device.h; the selection rule is in gemm_plan.h.
#pragma once
#include <stdlib.h>

#include "common.h"
#include "gemm_plan.h"

constexpr int BM = 128, BN = 128, ROWB = 128, PITCH = 144;

struct GemmArgs {
    const void *A, *W;
    const float *bias, *residual;
    void *C;
    int lda, ldw, ldr, ldc, M, N, K, out_dtype, flags;
    int vec_epi; // host-checked: C (and the residual) allow 16-byte row accesses -> LDS-transposed epilogue
    int ksplit;  // > 0: split-K over `ksplit` workgroups per tile, fp32 atomic accumulation into C (weight gradients: K = rows)
    // aux_mode 1: `aux` (dtype of C) also receives the pre-activation while C gets GELU of it (training forward keeps both);
    // aux_mode 2: C = round(acc) * gelu'(aux)  (the dX GEMM of linear2 applies the GELU derivative of the saved pre-activation)
    // aux_mode 3 (round 4, what the training steps use): as 1, but `aux` receives gelu'(pre-activation) - the forward epilogue holds
    //             Phi(-|a|) anyway - and aux_mode 4: C = round(acc) * aux, ONE multiply per element in the backward epilogue, which was
    //             VALU-bound on the derivative (tools/ablate_gelu_grad.py)
    void *aux;
    int ldaux, aux_mode;
    // columns [0, scale_cols) of (A.W^T + bias) are multiplied by col_scale before rounding (the in-projection's q for the attention kernels)
    int scale_cols;
    float col_scale;
    // dW form (TA && TB): also accumulate the column sums of the token-major A operand (= the bias gradient next to dW = dY^T X) into colsum[M]
    float *colsum;
    // EPI == 1 (cross K/V prefill scatter)
    const int32_t *row_seq, *row_pos, *seq_len;
    const int64_t *seq_off;
    void *k_out, *v_out;
    int E, dh, dhp;
};

// Each kernel file's host launcher: launches the instantiation that `l` names (l.kernel must be one of the file's) on l.grid x l.block with `g`.
// elem_size 2: bf16 operands, 4: fp32; epi as AcaiGemmQuery.epi.
void gemm_launch_tile(const AcaiGemmLaunch &l, int elem_size, int epi, bool trans_a, bool trans_w, const GemmArgs &g, hipStream_t st);   // K_REG, K_GLDS, K_GLDS3, K_256
void gemm_launch_ring(const AcaiGemmLaunch &l, int elem_size, int epi, const GemmArgs &g, hipStream_t st);   // K_PERS, K_PERS256, K_TN_GLDS, K_TN_RING
void gemm_launch_pp(const AcaiGemmLaunch &l, const GemmArgs &g, hipStream_t st);                             // K_PP, K_TN_PP (bf16, epi 0)
