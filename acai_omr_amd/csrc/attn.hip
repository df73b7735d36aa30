// F.scaled_dot_product_attention on packed ragged streams and its backward (reference: acai_omr/models/models.py:30-34, 186-190, 351-360,
// 422-426; training loops pre_train.py:59, omr_teacher_force_train.py:118).
//
// This file: the C ABI entries.  Each validates, states the call as a query, asks the planner which kernels run (attn_plan.h, a pure
// function) and launches the plan.  The kernels live in attn_varlen.hip, attn_fwd64.hip, attn_fwd64w.hip, attn_bwd.hip, attn_bwd64w.hip and
// attn_bwd1p.hip, so editing this file recompiles none.
#include "attn_internal.h"

#include <limits.h>

namespace {

int g_override[ACAI_ATTN_OV_COUNT] = {1, ACAI_ATTN_FWD64_AUTO, -1, 1, -1};   // acai_attn_set_override
constexpr int OV_MIN[ACAI_ATTN_OV_COUNT] = {0, ACAI_ATTN_FWD64_AUTO, -1, 0, -1}, OV_MAX[ACAI_ATTN_OV_COUNT] = {1, ACAI_ATTN_FWD64_GENERIC, 3, 1, 1};

// the plan of the most recent attention entry call on this thread (acai_attn_last_plan)
thread_local AcaiAttnLaunch t_last_plan[ATTN_MAX_LAUNCHES];
thread_local int t_last_n = 0;

void set_overrides(AcaiAttnQuery &q) {
    for (int i = 0; i < ACAI_ATTN_OV_COUNT; ++i) q.ov[i] = g_override[i];
}

}  // namespace

extern "C" int acai_attn_set_override(int which, int value) {
    ACAI_CHECK_ARG(which >= 0 && which < ACAI_ATTN_OV_COUNT, "acai_attn_set_override: no override %d", which);
    ACAI_CHECK_ARG(value >= OV_MIN[which] && value <= OV_MAX[which], "acai_attn_set_override: override %d takes %d .. %d", which, OV_MIN[which], OV_MAX[which]);
    g_override[which] = value;
    return 0;
}

extern "C" int acai_attn_get_override(int which, int *value_out) {
    ACAI_CHECK_ARG(which >= 0 && which < ACAI_ATTN_OV_COUNT && value_out, "acai_attn_get_override: no override %d", which);
    *value_out = g_override[which];
    return 0;
}

extern "C" int acai_attn_plan(const AcaiAttnQuery *query, AcaiAttnLaunch *launches_out, int *n_out, int *refusal_out) {
    ACAI_CHECK_ARG(query && launches_out && n_out, "acai_attn_plan: null argument");
    const AcaiAttnQuery &q = *query;
    bool ok = (q.elem_size == 2 || q.elem_size == 4) && q.B > 0 && q.H > 0 && q.dh > 0 && q.dh <= 64 && q.max_q > 0 && (!q.backward || q.max_k > 0);
    for (int i = 0; i < ACAI_ATTN_OV_COUNT; ++i) ok = ok && q.ov[i] >= OV_MIN[i] && q.ov[i] <= OV_MAX[i];
    ACAI_CHECK_ARG(ok, "acai_attn_plan: bad query");
    int refusal = 0;
    *n_out = attn_plan(q, launches_out, &refusal);
    if (refusal_out) *refusal_out = refusal;
    return 0;
}

extern "C" int acai_attn_last_plan(AcaiAttnLaunch *launches_out, int *n_out) {
    ACAI_CHECK_ARG(launches_out && n_out, "acai_attn_last_plan: null argument");
    for (int i = 0; i < t_last_n; ++i) launches_out[i] = t_last_plan[i];
    *n_out = t_last_n;
    return 0;
}

// q_prescaled: q already carries the factor log2(e) / sqrt(dh) (acai_gemm_nt_ex's column scale on the in-projection); the kernel then
// takes K . Q^T as the score in the log2 domain.  `lse` has the same meaning either way.
extern "C" int acai_attn_varlen_fwd(const void *q, int ldq, const void *k, int ldk, const void *v, int ldv, void *out, int ldo,
                                    const int32_t *cu_q, const int32_t *cu_k, int B, int H, int dh, int max_q, int causal,
                                    int dtype, float *lse, int total_q, float dropout_p, uint32_t dropout_seed, int q_prescaled, void *stream) {
    t_last_n = 0;
    ACAI_CHECK_ARG(q && k && v && out && cu_q && cu_k, "acai_attn_varlen_fwd: null operand");
    ACAI_CHECK_ARG(B > 0 && H > 0 && dh > 0 && dh <= 64 && max_q > 0, "acai_attn_varlen_fwd: bad dims B=%d H=%d dh=%d max_q=%d (dh <= 64)", B, H, dh, max_q);
    ACAI_CHECK_ARG(ldq >= H * dh && ldk >= H * dh && ldv >= H * dh && ldo >= H * dh, "acai_attn_varlen_fwd: row stride smaller than H*dh");
    ACAI_CHECK_ARG(B <= 65535 && H <= 65535, "acai_attn_varlen_fwd: grid too large");
    ACAI_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "acai_attn_varlen_fwd: dropout_p out of range");
    AttnArgs a{q, k, v, out, cu_q, cu_k, ldq, ldk, ldv, ldo, H, dh, causal, 0.f, (uint32_t)((double)dropout_p * 4294967296.0), dropout_seed,
               1.0f / (1.0f - dropout_p), lse, total_q};
    a.scale_log2e = 1.4426950408889634f / sqrtf((float)dh);
    if (dtype != ACAI_BF16 && dtype != ACAI_F32) return acai_set_err(-1, "acai_attn_varlen_fwd: bad dtype %d", dtype);
    AcaiAttnQuery qy{};
    qy.elem_size = dtype == ACAI_BF16 ? 2 : 4;
    qy.B = B; qy.H = H; qy.dh = dh; qy.max_q = max_q; qy.total_q = total_q;
    qy.causal = causal != 0; qy.dropout = a.drop_thr != 0; qy.q_prescaled = q_prescaled != 0;
    qy.ldq = ldq; qy.ldk = ldk; qy.ldv = ldv; qy.ldo = ldo;
    qy.aligned = aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out);
    qy.cu_k_is_cu_q = cu_k == cu_q;
    set_overrides(qy);
    int refusal = 0;
    const int n = attn_plan(qy, t_last_plan, &refusal);
    if (refusal) return acai_set_err(-1, "acai_attn_varlen_fwd: q_prescaled needs 16-byte aligned operands and d_h %% %d == 0", 16 / qy.elem_size);
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < n; ++i) {
        const AcaiAttnLaunch &l = t_last_plan[i];
        AttnArgs w = a;
        w.nqb = l.nblk;
        w.tail = l.tail;
        switch (l.kernel) {
            case ACAI_ATTN_K_FWD64W: acai_attn_launch_fwd64w(l, w, st); break;
            case ACAI_ATTN_K_FWD64:
            case ACAI_ATTN_K_FWD64_TAIL: acai_attn_launch_fwd64(l, w, st); break;
            default: acai_attn_launch_fwd(l, w, st); break;
        }
    }
    t_last_n = n;
    ACAI_LAUNCH_CHECK("acai_attn_varlen_fwd");
    return 0;
}

extern "C" int acai_attn_varlen_bwd_ws(const void *q, int ldq, const void *k, int ldk, const void *v, int ldv, const void *o, int ldo,
                                       const void *dout, int lddo, void *dq, int lddq, void *dk, int lddk, void *dv, int lddv, const float *lse,
                                       float *delta, const int32_t *cu_q, const int32_t *cu_k, int B, int H, int dh, int max_q, int max_k,
                                       int total_q, int total_k, int causal, int dtype, float dropout_p, uint32_t dropout_seed, int q_prescaled,
                                       void *workspace, size_t workspace_bytes, void *stream) {
    t_last_n = 0;
    ACAI_CHECK_ARG(q && k && v && o && dout && dq && dk && dv && lse && delta && cu_q && cu_k, "acai_attn_varlen_bwd: null operand");
    ACAI_CHECK_ARG(B > 0 && H > 0 && dh > 0 && dh <= 64 && max_q > 0 && max_k > 0 && total_q > 0 && B <= 65535 && H <= 65535,
                   "acai_attn_varlen_bwd: bad dims");
    ACAI_CHECK_ARG(total_k >= 0 && (workspace || !workspace_bytes), "acai_attn_varlen_bwd_ws: bad workspace / total_k");
    BwdArgs a{};
    a.q = q; a.k = k; a.v = v; a.o = o; a.dout = dout; a.dq = dq; a.dk = dk; a.dv = dv; a.lse = lse; a.delta = delta; a.cu_q = cu_q; a.cu_k = cu_k;
    a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo; a.lddo = lddo; a.lddq = lddq; a.lddk = lddk; a.lddv = lddv;
    ACAI_CHECK_ARG((causal & ~3) == 0, "acai_attn_varlen_bwd: causal takes bit 0 (causal mask) and bit 1 (accumulate dk / dv)");
    a.H = H; a.dh = dh; a.causal = causal & 1; a.accum_dkv = (causal >> 1) & 1; a.total_q = total_q;
    ACAI_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "acai_attn_varlen_bwd: dropout_p out of range");
    a.drop_thr = (uint32_t)((double)dropout_p * 4294967296.0); a.drop_seed = dropout_seed; a.drop_scale = 1.0f / (1.0f - dropout_p);
    a.scale = 1.0f / sqrtf((float)dh);
    a.scale_log2e = 1.4426950408889634f * a.scale;
    if (dtype != ACAI_BF16 && dtype != ACAI_F32) return acai_set_err(-1, "acai_attn_varlen_bwd: bad dtype %d", dtype);
    AcaiAttnQuery qy{};
    qy.backward = 1;
    qy.elem_size = dtype == ACAI_BF16 ? 2 : 4;
    qy.B = B; qy.H = H; qy.dh = dh; qy.max_q = max_q; qy.max_k = max_k; qy.total_q = total_q; qy.total_k = total_k;
    qy.causal = a.causal; qy.accum_dkv = a.accum_dkv; qy.dropout = a.drop_thr != 0; qy.q_prescaled = q_prescaled != 0;
    qy.ldq = ldq; qy.ldk = ldk; qy.ldv = ldv; qy.ldo = ldo; qy.lddo = lddo; qy.lddq = lddq; qy.lddk = lddk; qy.lddv = lddv;
    qy.aligned = aligned16(q) && aligned16(k) && aligned16(v) && aligned16(dout) && aligned16(o) && aligned16(dq) && aligned16(dk) && aligned16(dv);
    qy.cu_k_is_cu_q = cu_k == cu_q;
    qy.workspace_bytes = !workspace ? 0 : workspace_bytes < (size_t)LLONG_MAX ? (long long)workspace_bytes : LLONG_MAX;
    set_overrides(qy);
    int refusal = 0;
    const int n = attn_plan(qy, t_last_plan, &refusal);
    if (refusal == ACAI_ATTN_REFUSE_PRESCALED)
        return acai_set_err(-1, "acai_attn_varlen_bwd: q_prescaled needs 16-byte aligned operands and d_h %% %d == 0", 16 / qy.elem_size);
    if (refusal) return acai_set_err(-1, "acai_attn_varlen_bwd: accumulating dk / dv needs bf16 and 16-byte aligned operands");
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < n; ++i) {
        const AcaiAttnLaunch &l = t_last_plan[i];
        BwdArgs w = a;
        w.tail256 = l.tail256;
        w.nblk = l.nblk;
        switch (l.kernel) {
            case ACAI_ATTN_K_BWD1P: acai_attn_launch_bwd1p(l, w, workspace, st); break;
            case ACAI_ATTN_K_BWD64W_DQ:
            case ACAI_ATTN_K_BWD64W_DKV: acai_attn_launch_bwd64w(l, w, st); break;
            default: acai_attn_launch_bwd(l, w, st); break;
        }
    }
    t_last_n = n;
    ACAI_LAUNCH_CHECK("acai_attn_varlen_bwd");
    return 0;
}

extern "C" size_t acai_attn_varlen_bwd_workspace_bytes(int B, int H, int dh, int max_q, int max_k, int total_q, int total_k, int causal, int dtype,
                                                       float dropout_p, int q_prescaled) {
    if (dtype != ACAI_BF16 || !q_prescaled || dropout_p != 0.f || B <= 0 || H <= 0 || H > 65535 || dh <= 0 || dh > 64 || total_q <= 0) return 0;
    AcaiAttnQuery qy{};
    qy.elem_size = 2;
    qy.B = B; qy.H = H; qy.dh = dh; qy.max_q = max_q; qy.max_k = max_k; qy.total_q = total_q; qy.total_k = total_k;
    qy.causal = causal & 1; qy.accum_dkv = (causal >> 1) & 1; qy.q_prescaled = 1;
    set_overrides(qy);
    return attn_plan_workspace_bytes(qy);
}

extern "C" int acai_attn_varlen_bwd(const void *q, int ldq, const void *k, int ldk, const void *v, int ldv, const void *o, int ldo,
                                    const void *dout, int lddo, void *dq, int lddq, void *dk, int lddk, void *dv, int lddv, const float *lse,
                                    float *delta, const int32_t *cu_q, const int32_t *cu_k, int B, int H, int dh, int max_q, int max_k,
                                    int total_q, int causal, int dtype, float dropout_p, uint32_t dropout_seed, int q_prescaled, void *stream) {
    return acai_attn_varlen_bwd_ws(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, dq, lddq, dk, lddk, dv, lddv, lse, delta, cu_q, cu_k, B, H, dh, max_q, max_k,
                                   total_q, 0, causal, dtype, dropout_p, dropout_seed, q_prescaled, nullptr, 0, stream);
}
