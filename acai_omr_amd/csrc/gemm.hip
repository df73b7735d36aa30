// C[M,N] = epi(A[M,K] . W[N,K]^T + bias) (+ residual): the nn.Linear of every projection on the path
// (reference: acai_omr/models/models.py:29,57,204,205,428,655-660; kv_caching.py:193,215,244).
//
// This file: the C ABI entries.  Each validates, states the call as a query, asks the planner which kernels run (gemm_plan.h, a pure
// function) and launches the plan.  The kernels live in gemm_tile.hip, gemm_ring.hip and gemm_pp.hip, so editing this file recompiles none.
#include "gemm_internal.h"

namespace {

int g_gemm_variant = 0;   // acai_gemm_set_variant

// the plan of the most recent GEMM entry call on this thread (acai_gemm_last_plan)
thread_local AcaiGemmLaunch t_last_plan[GEMM_MAX_LAUNCHES];
thread_local int t_last_n = 0;

int device_cus() {
    static const int n_cu = [] {
        int dev = 0, n = 256;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 256;
        return n > 0 ? n : 256;
    }();
    return n_cu;
}

// `g` holds the whole problem; a launch takes its row range [row0, row0 + rows) and its reduction range [k0, k0 + k) of it
GemmArgs launch_args(const GemmArgs &g, const AcaiGemmLaunch &l, int elem_size, bool trans_a, bool trans_w) {
    const size_t esz = g.out_dtype == ACAI_BF16 ? 2 : 4;
    GemmArgs a = g;
    a.M = l.rows;
    a.K = l.k;
    a.ksplit = l.ksplit;
    a.vec_epi = l.vec_epi;
    if (!l.colsum) a.colsum = nullptr;
    // a row-major operand advances by whole rows along M and by elements along K; a transposed one (stored [K][M]) the other way round
    const size_t a_off = trans_a ? (size_t)l.k0 * g.lda + l.row0 : (size_t)l.row0 * g.lda + l.k0;
    const size_t w_off = trans_w ? (size_t)l.k0 * g.ldw : (size_t)l.k0;
    a.A = reinterpret_cast<const unsigned char *>(g.A) + a_off * elem_size;
    a.W = reinterpret_cast<const unsigned char *>(g.W) + w_off * elem_size;
    a.C = reinterpret_cast<unsigned char *>(g.C) + (size_t)l.row0 * g.ldc * esz;
    if (g.residual) a.residual = g.residual + (size_t)l.row0 * g.ldr;
    if (g.aux) a.aux = reinterpret_cast<unsigned char *>(g.aux) + (size_t)l.row0 * g.ldaux * esz;
#ifdef ACAI_GEMM_ABLATE
    if (l.kernel == ACAI_GEMM_K_PP)
        if (const char *d = getenv("ACAI_GEMM_DEBUG")) a.flags |= atoi(d) << 8;
#endif
    return a;
}

// Plans and launches one GEMM; *colsum_formed (if given): a launch of the plan formed g.colsum itself.
int run(const GemmArgs &g, int elem_size, int epi, bool trans_a, bool trans_w, hipStream_t st, bool *colsum_formed = nullptr) {
    AcaiGemmQuery q{};
    q.elem_size = elem_size; q.epi = epi; q.trans_a = trans_a; q.trans_w = trans_w;
    q.M = g.M; q.N = g.N; q.K = g.K;
    q.lda = g.lda; q.ldw = g.ldw; q.ldc = g.ldc; q.ldr = g.ldr; q.ldaux = g.ldaux;
    q.a_aligned = aligned16(g.A); q.w_aligned = aligned16(g.W); q.c_aligned = aligned16(g.C);
    q.r_aligned = aligned16(g.residual); q.aux_aligned = aligned16(g.aux);
    q.out_dtype = g.out_dtype; q.flags = g.flags; q.aux_mode = g.aux_mode;
    q.has_residual = g.residual != nullptr;
    q.scale_cols = g.scale_cols;
    q.want_colsum = g.colsum != nullptr;
    q.variant = g_gemm_variant;
    q.n_cu = device_cus();
    t_last_n = gemm_plan(q, t_last_plan);
    for (int i = 0; i < t_last_n; ++i) {
        const AcaiGemmLaunch &l = t_last_plan[i];
        const GemmArgs a = launch_args(g, l, elem_size, trans_a, trans_w);
        switch (l.kernel) {
            case ACAI_GEMM_K_PP:
            case ACAI_GEMM_K_TN_PP: gemm_launch_pp(l, a, st); break;
            case ACAI_GEMM_K_PERS:
            case ACAI_GEMM_K_PERS256:
            case ACAI_GEMM_K_TN_GLDS:
            case ACAI_GEMM_K_TN_RING: gemm_launch_ring(l, elem_size, epi, a, st); break;
            default: gemm_launch_tile(l, elem_size, epi, trans_a, trans_w, a, st); break;
        }
        ACAI_LAUNCH_CHECK("acai_gemm");
        if (colsum_formed && l.colsum) *colsum_formed = true;
    }
    return 0;
}

}  // namespace

extern "C" int acai_gemm_set_variant(int variant) {
    ACAI_CHECK_ARG(variant >= 0 && variant <= 8, "acai_gemm_set_variant: 0 (auto) .. 8");
    g_gemm_variant = variant;
    return 0;
}

extern "C" int acai_gemm_plan(const AcaiGemmQuery *query, AcaiGemmLaunch *launches_out, int *n_out) {
    ACAI_CHECK_ARG(query && launches_out && n_out, "acai_gemm_plan: null argument");
    const AcaiGemmQuery &q = *query;
    ACAI_CHECK_ARG((q.elem_size == 2 || q.elem_size == 4) && (q.epi == 0 || q.epi == 1) && q.M > 0 && q.N > 0 && q.K > 0 && q.n_cu > 0 &&
                       q.variant >= 0 && q.variant <= 8 && !(q.epi == 1 && (q.trans_a || q.trans_w)),
                   "acai_gemm_plan: bad query");
    *n_out = gemm_plan(q, launches_out);
    return 0;
}

extern "C" int acai_gemm_last_plan(AcaiGemmLaunch *launches_out, int *n_out) {
    ACAI_CHECK_ARG(launches_out && n_out, "acai_gemm_last_plan: null argument");
    for (int i = 0; i < t_last_n; ++i) launches_out[i] = t_last_plan[i];
    *n_out = t_last_n;
    return 0;
}

extern "C" int acai_gemm_nt_ex(const void *A, int lda, const void *W, int ldw, const float *bias, const float *residual, int ldr,
                               void *C, int ldc, void *aux, int ldaux, int aux_mode, int M, int N, int K, int in_dtype, int out_dtype, int flags,
                               int scale_cols, float col_scale, void *stream) {
    t_last_n = 0;
    ACAI_CHECK_ARG(A && W && C, "acai_gemm_nt: null operand");
    ACAI_CHECK_ARG(M >= 0 && N > 0 && K > 0, "acai_gemm_nt: bad shape M=%d N=%d K=%d", M, N, K);
    ACAI_CHECK_ARG(lda >= K && ldw >= K && ldc >= N && (!residual || ldr >= N), "acai_gemm_nt: leading dimension smaller than row");
    ACAI_CHECK_ARG((in_dtype == ACAI_F32 || in_dtype == ACAI_BF16) && (out_dtype == ACAI_F32 || out_dtype == ACAI_BF16),
                   "acai_gemm_nt: bad dtype");
    ACAI_CHECK_ARG(aux_mode >= 0 && aux_mode <= 4 && (aux_mode == 0 || (aux && ldaux >= N)), "acai_gemm_nt_ex: bad aux operand (mode %d)", aux_mode);
    ACAI_CHECK_ARG((aux_mode != 1 && aux_mode != 3) || (flags & ACAI_GEMM_GELU), "acai_gemm_nt_ex: aux_mode 1 / 3 keep the pre-activation / its derivative of a GELU epilogue");
    ACAI_CHECK_ARG((aux_mode != 2 && aux_mode != 4) || !(flags & ACAI_GEMM_GELU), "acai_gemm_nt_ex: aux_mode 2 / 4 (GELU derivative) exclude the GELU flag");
    ACAI_CHECK_ARG((flags & ~(ACAI_GEMM_GELU | ACAI_GEMM_ROUND_BF16)) == 0, "acai_gemm_nt: unknown flag bits 0x%x", flags);
    if (M == 0) return 0;
    GemmArgs g{};
    g.A = A; g.W = W; g.bias = bias; g.residual = residual; g.C = C;
    g.lda = lda; g.ldw = ldw; g.ldr = ldr; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
    g.out_dtype = out_dtype; g.flags = flags;
    g.aux = aux; g.ldaux = ldaux; g.aux_mode = aux_mode;
    ACAI_CHECK_ARG(scale_cols >= 0 && scale_cols <= N, "acai_gemm_nt_ex: scale_cols %d outside [0, N]", scale_cols);
    g.scale_cols = scale_cols; g.col_scale = col_scale;
    return run(g, in_dtype == ACAI_BF16 ? 2 : 4, 0, false, false, (hipStream_t)stream);
}

extern "C" int acai_gemm_nt(const void *A, int lda, const void *W, int ldw, const float *bias, const float *residual, int ldr,
                            void *C, int ldc, int M, int N, int K, int in_dtype, int out_dtype, int flags, void *stream) {
    return acai_gemm_nt_ex(A, lda, W, ldw, bias, residual, ldr, C, ldc, nullptr, 0, 0, M, N, K, in_dtype, out_dtype, flags, 0, 1.0f, stream);
}

// General form for the backward pass: C[M,N] = op(A) . op(W)^T (+bias) (+residual), logical A [M,K], logical W [N,K];
// trans_a: A is stored [K][M] (lda = row stride of that storage); trans_w: W is stored [K][N].
//   dX = dY . W       : A = dY [M,N'] row-major,  W stored [N'][K'] = "[K_red][N_out]" -> trans_w = 1
//   dW = dY^T . X     : A = dY stored [M_red][N] -> trans_a = 1;  W-operand = X stored [M_red][K] -> trans_w = 1
extern "C" int acai_gemm(const void *A, int lda, int trans_a, const void *W, int ldw, int trans_w, const float *bias, const float *residual,
                         int ldr, void *C, int ldc, int M, int N, int K, int in_dtype, int out_dtype, int flags, void *stream) {
    t_last_n = 0;
    ACAI_CHECK_ARG(A && W && C, "acai_gemm: null operand");
    ACAI_CHECK_ARG((flags & ~(ACAI_GEMM_GELU | ACAI_GEMM_ROUND_BF16)) == 0, "acai_gemm: unknown flag bits 0x%x", flags);
    ACAI_CHECK_ARG(M >= 0 && N > 0 && K > 0, "acai_gemm: bad shape M=%d N=%d K=%d", M, N, K);
    ACAI_CHECK_ARG(lda >= (trans_a ? M : K) && ldw >= (trans_w ? N : K) && ldc >= N && (!residual || ldr >= N), "acai_gemm: leading dimension smaller than row");
    ACAI_CHECK_ARG((in_dtype == ACAI_F32 || in_dtype == ACAI_BF16) && (out_dtype == ACAI_F32 || out_dtype == ACAI_BF16), "acai_gemm: bad dtype");
    ACAI_CHECK_ARG(!(trans_a && trans_w) || (out_dtype == ACAI_F32 && !bias && !residual && !flags),
                   "acai_gemm: trans_a && trans_w accumulates into an fp32 C (no bias / residual / flags)");
    if (M == 0) return 0;
    GemmArgs g{};
    g.A = A; g.W = W; g.bias = bias; g.residual = residual; g.C = C;
    g.lda = lda; g.ldw = ldw; g.ldr = ldr; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
    g.out_dtype = out_dtype; g.flags = flags;
    return run(g, in_dtype == ACAI_BF16 ? 2 : 4, 0, trans_a != 0, trans_w != 0, (hipStream_t)stream);
}

// dW[M][N] += dY^T X and, optionally, db[M] += column sums of dY: the two parameter gradients of an nn.Linear from one pass over dY
// (autograd of F.linear, models.py:29,57,...; torch computes them as mm + sum).  bf16 operands [K tokens][.], fp32 accumulators (zero them for
// fresh gradients).  The ping-pong weight-gradient kernel forms the sums from the dY fragments it holds; other shapes take acai_colsum.
extern "C" int acai_gemm_dw(const void *dY, int ldy, const void *X, int ldx, float *dW, int lddw, float *db, int M, int N, int K, int dtype, void *stream) {
    t_last_n = 0;
    ACAI_CHECK_ARG(dY && X && dW, "acai_gemm_dw: null operand");
    ACAI_CHECK_ARG(M > 0 && N > 0 && K > 0 && ldy >= M && ldx >= N && lddw >= N, "acai_gemm_dw: bad shape M=%d N=%d K=%d", M, N, K);
    ACAI_CHECK_ARG(dtype == ACAI_F32 || dtype == ACAI_BF16, "acai_gemm_dw: bad dtype");
    GemmArgs g{};
    g.A = dY; g.W = X; g.C = dW; g.lda = ldy; g.ldw = ldx; g.ldc = lddw; g.M = M; g.N = N; g.K = K;
    g.out_dtype = ACAI_F32;
    g.colsum = dtype == ACAI_BF16 ? db : nullptr;
    bool colsum_formed = false;   // the plan's kernel also formed the column sums (else: a separate pass below)
    const int rc = run(g, dtype == ACAI_BF16 ? 2 : 4, 0, true, true, (hipStream_t)stream, &colsum_formed);
    if (rc) return rc;
    if (db && !colsum_formed) return acai_colsum(dY, ldy, db, K, M, dtype, stream);
    return 0;
}

extern "C" int acai_cross_kv_prefill(const void *mem, int ldm, const void *Wkv, int ldw, const float *bkv, const int32_t *row_seq,
                                     const int32_t *row_pos, const int64_t *seq_off, const int32_t *seq_len, void *k_out,
                                     void *v_out, int M, int E, int H, int dh, int dhp, int dtype, int flags, void *stream) {
    t_last_n = 0;
    ACAI_CHECK_ARG(mem && Wkv && row_seq && row_pos && seq_off && seq_len && k_out && v_out, "acai_cross_kv_prefill: null operand");
    // (the scatter epilogue divides by E and dh)
    ACAI_CHECK_ARG(M >= 0 && E > 0 && H > 0 && dh > 0, "acai_cross_kv_prefill: bad shape M=%d E=%d H=%d dh=%d", M, E, H, dh);
    ACAI_CHECK_ARG(E == H * dh && dhp >= dh && ldm >= E && ldw >= E, "acai_cross_kv_prefill: bad dims E=%d H=%d dh=%d dhp=%d", E, H, dh, dhp);
    ACAI_CHECK_ARG(dtype == ACAI_F32 || dtype == ACAI_BF16, "acai_cross_kv_prefill: bad dtype");
    // The scatter epilogue applies no flag: a bf16 cache is rounded by its store (ROUND_BF16 is a no-op there), an fp32 cache would silently
    // stay unrounded, and there is no GELU form.
    ACAI_CHECK_ARG((flags & ~ACAI_GEMM_ROUND_BF16) == 0, "acai_cross_kv_prefill: flag bits 0x%x (only ACAI_GEMM_ROUND_BF16 is accepted)", flags);
    ACAI_CHECK_ARG(!(flags & ACAI_GEMM_ROUND_BF16) || dtype == ACAI_BF16, "acai_cross_kv_prefill: ACAI_GEMM_ROUND_BF16 needs a bf16 cache (fp32 output is not rounded)");
    if (M == 0) return 0;
    GemmArgs g{};
    g.A = mem; g.W = Wkv; g.bias = bkv; g.lda = ldm; g.ldw = ldw; g.M = M; g.N = 2 * E; g.K = E;
    g.out_dtype = dtype; g.flags = flags;
    g.row_seq = row_seq; g.row_pos = row_pos; g.seq_off = seq_off; g.seq_len = seq_len; g.k_out = k_out; g.v_out = v_out;
    g.E = E; g.dh = dh; g.dhp = dhp;
    return run(g, dtype == ACAI_BF16 ? 2 : 4, 1, false, false, (hipStream_t)stream);
}
