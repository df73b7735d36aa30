// Shared by the varlen attention sources: the two argument blocks and the launchers.  attn.hip (the C ABI entries) states a call as an
// AcaiAttnQuery, asks attn_plan.h which kernels run, fills the host-decided fields below from each AcaiAttnLaunch and hands launch and
// argument block to the launcher of the file that holds the kernel.  The kernels stay in their files' anonymous namespaces.
#pragma once
#include "attn_plan.h"
#include "common.h"

// Forward (attn_varlen.hip: every dtype / head size / mask; attn_fwd64.hip, attn_fwd64w.hip: the bf16 d_h = 64 forms of the training steps).
struct AttnArgs {
    const void *q, *k, *v;
    void *out;
    const int32_t *cu_q, *cu_k;
    int ldq, ldk, ldv, ldo, H, dh, causal;
    float scale_log2e;
    uint32_t drop_thr, drop_seed;  // attention-probability dropout (nn.MultiheadAttention(dropout=p) in train mode): keep iff hash >= thr
    float drop_scale;
    float *lse;   // optional [H][total_q]: log2-domain log-sum-exp of the scaled scores (saved for the backward pass)
    int total_q;
    int nqb;      // = AcaiAttnLaunch::nblk.  attn_fwd64w.hip: query blocks per (sequence, head) of its one-dimensional grid; > 0: XCD-aware block order
    int tail;     // = AcaiAttnLaunch::tail.  attn_fwd64*.hip: > 0 = a sequence's last 256-query block goes to attn_fwd64_tail_kernel when it holds <= tail (32) rows
};

// Backward (attn_bwd.hip: every dtype / head size / mask / dropout; attn_bwd64w.hip: bf16 d_h = 64; attn_bwd1p.hip: bf16 d_h = 32 in one pass).
struct BwdArgs {
    const void *q, *k, *v, *o, *dout;
    void *dq, *dk, *dv;
    const float *lse, *delta;  // [H][total_q]
    const int32_t *cu_q, *cu_k;
    int ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv, H, dh, causal, total_q;
    float scale_log2e, scale;
    uint32_t drop_thr, drop_seed;  // the forward's attention-probability dropout, regenerated element-wise
    float drop_scale;
    int accum_dkv; // 1: dk, dv += instead of = (bf16, aligned operands only): a second pass over the same K / V adds its gradient in the kernel's epilogue
    int tail256;   // = AcaiAttnLaunch::tail256.  attn_bwd.hip one-block kernels: > 0 = cover only the rows past each sequence's last full 256-row block (the full blocks belong to attn_bwd64w.hip); attn_bwd1p.hip: != 0 = XCD-aware block order
    int nblk;      // = AcaiAttnLaunch::nblk.  attn_bwd64w.hip / attn_bwd1p.hip: key or query blocks per (sequence, head) of their one-dimensional grids; attn_bwd64w.hip: > 0 = XCD-aware block order
};

// One launcher per kernel file: maps the launch's template form to the instantiation, sets the dynamic-LDS attribute (once per device) and
// launches with the launch's grid, block and LDS size.  `a` already carries the launch's arguments.
void acai_attn_launch_fwd(const AcaiAttnLaunch &l, const AttnArgs &a, hipStream_t st);      // attn_varlen.hip: K_FWD
void acai_attn_launch_fwd64(const AcaiAttnLaunch &l, const AttnArgs &a, hipStream_t st);    // attn_fwd64.hip: K_FWD64, K_FWD64_TAIL
void acai_attn_launch_fwd64w(const AcaiAttnLaunch &l, const AttnArgs &a, hipStream_t st);   // attn_fwd64w.hip: K_FWD64W
void acai_attn_launch_bwd(const AcaiAttnLaunch &l, const BwdArgs &a, hipStream_t st);       // attn_bwd.hip: K_BWD_DQ, K_BWD_DKV, K_BWD_DQ2, K_BWD_DKV2
void acai_attn_launch_bwd64w(const AcaiAttnLaunch &l, const BwdArgs &a, hipStream_t st);    // attn_bwd64w.hip: K_BWD64W_DQ, K_BWD64W_DKV
// attn_bwd1p.hip: K_BWD1P's three launches; workspace: attn_bwd1p_workspace(total_q, H) bytes of device memory, used only inside the call
void acai_attn_launch_bwd1p(const AcaiAttnLaunch &l, const BwdArgs &a, void *workspace, hipStream_t st);

static inline dim3 acai_attn_grid(const AcaiAttnLaunch &l) { return dim3(l.grid_x, l.grid_y, l.grid_z); }
