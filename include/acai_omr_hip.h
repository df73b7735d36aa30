/*
 * acai_omr_hip.h - C ABI of the MI355X (gfx950) backend for the acai-omr model hot path.
 *
 * The reference (jsnchon/acai-omr) is pure Python on stock PyTorch: it has no FFI of its own.
 * Each entry point below therefore replaces the stock ATen op sequence behind one reference
 * call site (file:line cited per function; acai_omr/models/models.py = M, kv_caching.py = K).
 * Callers own every buffer (PyTorch-ROCm tensors in practice); nothing here allocates, frees,
 * synchronises or reads device memory on the host, so every call is hipGraph-capturable.
 * All launches go to the hipStream_t passed as `stream` (void* in this header so that plain C /
 * ctypes callers need no HIP headers).  Return value: 0 = ok, negative = argument error,
 * positive = hipError_t; acai_last_error() gives a message.  No C++ exception crosses the ABI.
 *
 * dtypes: ACAI_F32 = fp32 storage + exact-fp32 MFMA (v_mfma_f32_32x32x2_f32);
 *         ACAI_BF16 = bf16 storage + bf16 MFMA with fp32 accumulate;
 *         ACAI_FP8_E4M3 = OCP e4m3fn storage with one fp32 power-of-two scale per row (the decode cross K/V of an FP8 memory cache only).
 * The residual stream, LayerNorm, softmax statistics, biases and logits are always fp32.
 */
#ifndef ACAI_OMR_HIP_H
#define ACAI_OMR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACAI_ABI_VERSION 1
#define ACAI_F32 0
#define ACAI_BF16 1
#define ACAI_FP8_E4M3 2

/* gemm epilogue flags */
#define ACAI_GEMM_GELU 1       /* exact-erf GELU after bias (M:31 activation="gelu", M:657 nn.GELU) */
#define ACAI_GEMM_ROUND_BF16 2 /* round (acc + bias) to bf16 first: restates autocast's bf16 linear output */

int acai_version(void);
const char *acai_last_error(void);

/* nn.LayerNorm (M:33, eps 1e-6 final norms; torch TransformerEncoderLayer norm1/2/3 eps 1e-5).
 * y = LN(x) * w + b over the last dim; out_f32 and/or out_bf16 may be NULL. */
int acai_layernorm_fwd(const float *x, const float *w, const float *b, float eps, float *out_f32, void *out_bf16,
                       int rows, int dim, void *stream);

/* nn.Linear / F.linear (M:29,57,204,205,428,655-660; K:193,215,244):
 * C[M,N] = epi(A[M,K] . W[N,K]^T + bias[N]) (+ residual[M,N]); A, W have dtype `in_dtype`,
 * C has `out_dtype`; bias and residual are fp32 (NULL = absent). */
int acai_gemm_nt(const void *A, int lda, const void *W, int ldw, const float *bias, const float *residual, int ldr,
                 void *C, int ldc, int M, int N, int K, int in_dtype, int out_dtype, int flags, void *stream);
/* acai_gemm_nt with an auxiliary [M][N] operand of C's dtype (the MLP of nn.TransformerEncoderLayer / DecoderLayer in training:
 * linear1 -> GELU -> linear2, acai_omr/models/models.py:30-34,186-190,422-426 and their autograd):
 *   aux_mode 1 (with ACAI_GEMM_GELU): aux receives the pre-activation (bias added, bf16-rounded if asked), C its GELU - the forward keeps both;
 *   aux_mode 2: C = round(A.W^T) * gelu'(aux) - the dX GEMM of linear2 multiplies by the GELU derivative of the saved pre-activation;
 *   aux_mode 3 (with ACAI_GEMM_GELU): as 1, but aux receives gelu'(pre-activation) - the forward epilogue holds Phi(-|a|) for the GELU anyway;
 *   aux_mode 4: C = round(A.W^T) * aux - with 3, the backward epilogue is one multiply per element (what the training steps use since round 4;
 *               the derivative is rounded to C's dtype once more than in the 1 / 2 pair: 2^-9 relative in bf16, nothing in fp32).
 * scale_cols > 0: columns [0, scale_cols) of (A.W^T + bias) are multiplied by col_scale before rounding - the in-projection of
 * nn.MultiheadAttention hands q to the attention kernels as q * log2(e) / sqrt(dh) (acai_attn_varlen_fwd, q_prescaled). */
int acai_gemm_nt_ex(const void *A, int lda, const void *W, int ldw, const float *bias, const float *residual, int ldr,
                    void *C, int ldc, void *aux, int ldaux, int aux_mode, int M, int N, int K, int in_dtype, int out_dtype, int flags,
                    int scale_cols, float col_scale, void *stream);
/* Testing / tuning aid: pin the row-major GEMM kernel (0 auto; 1 128x128 two-stage; 2 256x128 two-stage; 3 256x128 three-stage; 4 256x128
 * persistent three-stage ring; 5 256x256 two-stage; 6 persistent 256x256 ring of half-stages; 7 ping-pong wave groups with the register
 * epilogue; 8 = 7 with the GELU forms' deferred epilogue).  A pinned variant still falls back when the shape cannot use it.  No reference counterpart. */
int acai_gemm_set_variant(int variant);

/* The same contraction with either operand stored reduction-major, for the backward of nn.Linear (autograd of M:29,57,...):
 *   dX = dY . W   -> acai_gemm(dY, ldy, 0,  W, ldw, 1, ...)  (M = rows, N = in_features, K = out_features)
 *   dW = dY^T . X -> acai_gemm(dY, ldy, 1,  X, ldx, 1, ...)  (M = out_features, N = in_features, K = rows)
 * trans_a: A stored [K][M]; trans_w: W stored [K][N].  residual may alias C.
 * trans_a && trans_w (weight gradient, K = number of rows): C must be fp32 and is ACCUMULATED into with fp32 atomics
 * (split-K over workgroups); zero it for a fresh gradient.  No bias / residual / flags in that form. */
int acai_gemm(const void *A, int lda, int trans_a, const void *W, int ldw, int trans_w, const float *bias, const float *residual, int ldr,
              void *C, int ldc, int M, int N, int K, int in_dtype, int out_dtype, int flags, void *stream);
/* Both parameter gradients of an nn.Linear from one pass over the output gradient (autograd of F.linear: torch's mm + sum):
 * dW[M][N] += dY[K][M]^T X[K][N] and, if db != NULL, db[M] += sum over the K token rows of dY.  fp32 accumulators (zero them for fresh
 * gradients), bf16 or fp32 operands.  M = out_features, N = in_features, K = token rows. */
int acai_gemm_dw(const void *dY, int ldy, const void *X, int ldx, float *dW, int lddw, float *db, int M, int N, int K, int dtype, void *stream);

/* MemoryCache.cache_memory_keys_and_vals (K:235-253): KV = mem . W_kv^T + b_kv with W_kv = rows E..3E of the
 * cross-attention in_proj; written head-major and ragged for the decode kernels:
 * k_out[seq_off[b] + (h*len[b] + s)*dhp + d], same for v_out; row_seq/row_pos give (b, s) of each memory row.
 * The memory rows may come in any order (row_seq / row_pos need not be sorted; seq_off need not be monotonic), as long as each (b, s)
 * occurs once.  Only the lanes d < dh are written: the pad lanes [dh, dhp) of every row, and whatever lies between the sequences' regions,
 * keep their contents - the caller zeroes the buffers once (the engine allocates them with torch.zeros).
 * M >= 0 (0: nothing is written), E = H * dh, H and dh > 0, dhp >= dh.  flags: 0 or ACAI_GEMM_ROUND_BF16, the latter only with
 * dtype = ACAI_BF16, where the store rounds to bf16 anyway (the flag changes nothing); ACAI_GEMM_ROUND_BF16 with an fp32 cache,
 * ACAI_GEMM_GELU and unknown bits are refused. */
int acai_cross_kv_prefill(const void *mem, int ldm, const void *Wkv, int ldw, const float *bkv, const int32_t *row_seq,
                          const int32_t *row_pos, const int64_t *seq_off, const int32_t *seq_len, void *k_out, void *v_out,
                          int M, int E, int H, int dh, int dhp, int dtype, int flags, void *stream);

/* Which kernels a GEMM call runs.  The selection rule is a pure host function of the query below (csrc/gemm_plan.h): acai_gemm_plan
 * evaluates it without touching a device, acai_gemm_last_plan reports what the most recent acai_gemm_nt[_ex] / acai_gemm / acai_gemm_dw /
 * acai_cross_kv_prefill call of the calling thread launched (n = 0 before the first one and after a call with M = 0).  A plan has one
 * launch, or two: the rows past a multiple of 256 as a second launch (row0 / rows), or the tokens past a multiple of 64 of a weight
 * gradient as a register-staged second launch (k0 / k).  No reference counterpart. */
enum {
    ACAI_GEMM_K_REG = 0,       /* gemm_nt_kernel: register-staged, guarded loads (`fast`: 16-byte chunks) */
    ACAI_GEMM_K_GLDS = 1,      /* gemm_nt_glds_kernel: two LDS-DMA stages, `wm` = 2 (128x128 tile) or 4 (256x128) */
    ACAI_GEMM_K_GLDS3 = 2,     /* gemm_nt_glds3_kernel: 256x128, three stages */
    ACAI_GEMM_K_PERS = 3,      /* gemm_nt_pers_kernel: persistent 256x128 three-stage ring */
    ACAI_GEMM_K_256 = 4,       /* gemm_nt_256_kernel: 256x256, two stages */
    ACAI_GEMM_K_PERS256 = 5,   /* gemm_nt_pers256_kernel: persistent 256x256 ring of half-stages */
    ACAI_GEMM_K_PP = 6,        /* gemm_nt_pp_kernel: ping-pong ring with the register epilogue, instantiation `pp_mode` */
    ACAI_GEMM_K_TN_GLDS = 7,   /* gemm_tn_glds_kernel: weight gradient, two LDS-DMA stages, whole 64-token tiles only */
    ACAI_GEMM_K_TN_RING = 8,   /* gemm_tn_ring_kernel: weight gradient, 256x128 three-stage ring */
    ACAI_GEMM_K_TN_PP = 9      /* gemm_tn_pp_kernel: weight gradient, 256x256 ping-pong, forms the column sums itself */
};
/* AcaiGemmLaunch.pp_mode bits (the epilogue form gemm_nt_pp_kernel is instantiated for) */
enum { ACAI_PP_OBF = 1, ACAI_PP_GELU = 2, ACAI_PP_AUX1 = 4, ACAI_PP_AUX2 = 8, ACAI_PP_RES = 16, ACAI_PP_SCALE = 32,
       ACAI_PP_DEFER = 64, ACAI_PP_AUX3 = 128, ACAI_PP_AUX4 = 256 };
typedef struct AcaiGemmQuery {
    int elem_size;               /* operand element: 2 (bf16) or 4 (fp32) */
    int epi;                     /* 0: linear epilogue; 1: the cross K/V prefill scatter */
    int trans_a, trans_w;
    int M, N, K;
    int lda, ldw, ldc, ldr, ldaux;
    int a_aligned, w_aligned, c_aligned, r_aligned, aux_aligned;   /* the operand's base is 16-byte aligned (r / aux: read only when present) */
    int out_dtype, flags, aux_mode;
    int has_residual;
    int scale_cols;
    int want_colsum;             /* weight gradient: column sums of A are asked for beside it */
    int variant;                 /* acai_gemm_set_variant */
    int n_cu;                    /* compute units of the device */
} AcaiGemmQuery;
typedef struct AcaiGemmLaunch {
    int kernel;                  /* ACAI_GEMM_K_* */
    int wm, fast, pp_mode;       /* template form: K_GLDS / K_REG / K_PP (0 elsewhere) */
    int grid, block;
    int ksplit, vec_epi;
    int row0, rows;              /* output rows [row0, row0 + rows) */
    int k0, k;                   /* reduction range [k0, k0 + k) */
    int colsum;                  /* this launch also forms the column sums */
} AcaiGemmLaunch;
/* launches_out: room for two launches; *n_out: how many the plan has. */
int acai_gemm_plan(const AcaiGemmQuery *query, AcaiGemmLaunch *launches_out, int *n_out);
int acai_gemm_last_plan(AcaiGemmLaunch *launches_out, int *n_out);

/* nn.Unfold(P, stride P) on one (1,H,W) fp32 image, transposed to rows of P*P pixels (M:23,48-52);
 * rows are written starting at out + row0*ld (dtype `out_dtype`). */
int acai_patchify(const float *img, int H, int W, int P, void *out, int ld, int row0, int out_dtype, void *stream);

/* DynamicResize / PatchDivisibleResize resize step (acai_omr/utils/utils.py:325-330 `v2.Resize(...)`, :351-356 `F.resize(img, size,
 * BICUBIC, antialias=True)` on a float32 C x H x W tensor = aten `_upsample_bicubic2d_aa`, align_corners = False), optionally followed by
 * DynamicResize's `.clamp(0.0, 1.0)` (:367).  img [C][H][W] -> out [C][OH][OW], all fp32 contiguous; tmp holds C*H*OW floats (the
 * width pass).  C*H, OH and C <= 65535. */
int acai_resize_bicubic_aa(const float *img, int C, int H, int W, float *tmp, float *out, int OH, int OW, int clamp01, void *stream);

/* The same resize of ONE grayscale image written straight into the packed patch stream the encoder's projection GEMM reads (SURVEY 8f-2:
 * `DynamicResize` -> `Encoder.batchify`'s Unfold, acai_omr/utils/utils.py:334-367 + acai_omr/models/models.py:48-52, without the image tensor
 * in between): img is fp32 [H][W] in [0, 1], or uint8 (in_u8 = 1) scaled by 1/255 on load (`v2.ToDtype(torch.float32, scale=True)`,
 * acai_omr/train/pre_train.py:56); the crop window (top, left, ch, cw) of the OH x OW result (DynamicResize's centre crop, :360-364; the whole
 * image: 0, 0, OH, OW; ch, cw multiples of P) becomes rows row0 .. row0 + (ch/P)(cw/P) - 1 of `patches` [rows][ld >= P*P] in `out_dtype`
 * (fp32 / bf16), row (y/P)(cw/P) + x/P, column (y%P) P + x%P as nn.Unfold(P, stride P) orders them.  tmp holds H*OW floats. */
int acai_resize_to_patches(const void *img, int in_u8, int H, int W, float *tmp, void *patches, int ld, int row0, int OH, int OW, int top,
                           int left, int ch, int cw, int P, int out_dtype, int clamp01, void *stream);

/* out[i,:] = table[idx[i],:] (+ add[i,:]) : pos_embedding slices (M:50), nn.Embedding (M:460),
 * MAE shuffle / restore index_select (M:114,123,229). table/out fp32. */
int acai_gather_rows(const float *table, const int32_t *idx, const float *add, float *out, int rows, int dim, void *stream);

/* OMREncoder.interpolate_pe (M:291-302): F.interpolate(pos_embedding (Hin,Win,E) as NCHW, size=(Hout,Wout), mode="bilinear",
 * align_corners=False), result (Hout*Wout, E) row-major - aten's upsample_bilinear2d arithmetic (source index (dst + 0.5) * in/out - 0.5
 * clamped at 0, neighbour clamped at in-1).  bwd: dtable[Hin*Win, E] += the transposed stencil applied to dout (float atomics; dtable is
 * NOT zeroed here). */
int acai_pe_interp_fwd(const float *table, int Hin, int Win, int E, float *out, int Hout, int Wout, void *stream);
int acai_pe_interp_bwd(const float *dout, int Hout, int Wout, int E, float *dtable, int Hin, int Win, void *stream);

/* Diagnostic aid (tools/stamp_decode.py): s_memrealtime stamps of the decode GEMV kernel's stages, buf[launch][1024][8] uint64. */
int acai_debug_stamps(void *buf, int cap_launches);

/* Hardware-assumption probe (tests/test_gpu_kernels.py::test_lds_dma_out_of_range_lanes_write_zeros): one wave issues the weight-gradient
 * GEMMs' `buffer_load_dwordx4 ... offen lds` (gemm_tn_glds / gemm_tn_pp kernels, ragged last token tile) over a 1 KiB LDS image preset to
 * 0xFFFFFFFF with a resource of `valid_bytes` bytes at `src`; out[256] receives the image.  The kernels rely on lanes past num_records
 * writing ZEROS (observed on gfx950 / ROCm 7.2, not documented): a ROCm change shows up as a red test instead of wrong gradients. */
int acai_debug_lds_dma_oob(const void *src, int valid_bytes, void *out, void *stream);

/* Probe of the butterfly stages decode attention builds on (tests/test_gpu_lane_xor.py): every row of in[rows][64] is one wave; out[0][r]
 * receives the stage made by lane_xor_add<offset> (op 0) or lane_xor_max<offset> (op 1) of csrc/common.h - DPP quad permutes and row
 * rotation, v_permlane16/32_swap - and out[1][r] the same stage made with __shfl_xor.  offset 1, 2, 8, 16, 32: equal bit for bit on any
 * input.  offset 4 probes the row_half_mirror form, which equals the shuffle only where the four lanes of every quad hold one value. */
int acai_debug_lane_xor(const float *in, int rows, int offset, int op, float *out, void *stream);

/* autocast's fp32 -> bf16 input cast (round to nearest even) for an activation that feeds a bf16 GEMM. */
int acai_cast_f32_bf16(const float *x, void *y, int64_t n, void *stream);

/* F.scaled_dot_product_attention on packed ragged streams (torch nn.MultiheadAttention inside
 * nn.TransformerEncoderLayer M:30-34,186-190 and nn.TransformerDecoderLayer M:422-426).
 * q row i of sequence b is q + (cu_q[b]+i)*ldq + h*dh; same for k, v (cu_k) and out.
 * causal != 0 applies the triu(diagonal=1) mask of M:468.  dh <= 64.
 * lse (optional, [H][total_q] fp32): log2-domain log-sum-exp of the scaled scores, saved for acai_attn_varlen_bwd.
 * dropout_p > 0: attention-probability dropout (nn.MultiheadAttention(dropout=p) in train mode); the keep mask is a counter-based
 * hash of (dropout_seed, head, query, key) that the backward regenerates.
 * q_prescaled != 0: q already carries the softmax scale in the log2 domain, q' = q * log2(e) / sqrt(dh) - applied by the in-projection's
 * epilogue (acai_gemm_nt_ex scale_cols / col_scale) before its one rounding, as torch's math SDPA applies the scale to q before the
 * product - so K . q' is the exponent itself and the kernel spends no multiply per score.  Needs 16-byte aligned operands. */
int acai_attn_varlen_fwd(const void *q, int ldq, const void *k, int ldk, const void *v, int ldv, void *out, int ldo,
                         const int32_t *cu_q, const int32_t *cu_k, int B, int H, int dh, int max_q, int causal,
                         int dtype, float *lse, int total_q, float dropout_p, uint32_t dropout_seed, int q_prescaled, void *stream);

/* Backward of acai_attn_varlen_fwd (autograd of the same SDPA; training loops pre_train.py:59, omr_teacher_force_train.py:118).
 * o / lse are the forward's outputs, dout the incoming gradient; dq/dk/dv take the layout of q/k/v (own row strides).
 * delta: workspace [H][total_q] floats.  Deterministic (no atomics): S and P are recomputed per kernel.
 * q_prescaled != 0: q is the forward's q' (see there); dq is still the gradient with respect to the UNSCALED in-projection output
 * (what the in-projection's backward GEMMs consume), dk and dv are unchanged in meaning.
 * `causal`: bit 0 = the causal mask; bit 1 (round 4) = dk, dv += instead of = (bf16, 16-byte aligned operands): when two passes attend to ONE stored
 * K / V (ScheduledSamplingViTOMR.forward_train's two decoder passes over the same memory, models.py:822-834) the second pass's backward adds
 * its gradient in the kernel's epilogue - fp32 add, one rounding - instead of autograd summing two [keys, 2E] tensors afterwards. */
int acai_attn_varlen_bwd(const void *q, int ldq, const void *k, int ldk, const void *v, int ldv, const void *o, int ldo,
                         const void *dout, int lddo, void *dq, int lddq, void *dk, int lddk, void *dv, int lddv, const float *lse,
                         float *delta, const int32_t *cu_q, const int32_t *cu_k, int B, int H, int dh, int max_q, int max_k,
                         int total_q, int causal, int dtype, float dropout_p, uint32_t dropout_seed, int q_prescaled, void *stream);
/* The same backward with a caller-lent device workspace (round 4).  With bf16, d_h = 32, q_prescaled, no dropout / mask / accumulation and
 * max_q, max_k >= 512 - the MAE decoder's self-attention (models.py:186-190), ragged batches included - dQ, dK and dV come from ONE pass over
 * the scores (attn_bwd1p.hip): the key blocks add their part of a query's gradient to the fp32 workspace with float atomics, so dQ is
 * reproducible to fp32 rounding, not bit for bit (acai_attn_set_override(ACAI_ATTN_OV_BWD_1P, 0), or no workspace, keeps the two-kernel form,
 * which is).  total_k = the rows of k / v (0 = unknown: when it equals B * max_k with max_k % 512 == 0 the launch for partial key blocks is left out).  acai_attn_varlen_bwd_workspace_bytes: bytes that form needs for a call with these
 * arguments, 0 when it does not apply (then any workspace is ignored).  The workspace is used only inside the call (stream order). */
size_t acai_attn_varlen_bwd_workspace_bytes(int B, int H, int dh, int max_q, int max_k, int total_q, int total_k, int causal, int dtype,
                                            float dropout_p, int q_prescaled);
int acai_attn_varlen_bwd_ws(const void *q, int ldq, const void *k, int ldk, const void *v, int ldv, const void *o, int ldo,
                            const void *dout, int lddo, void *dq, int lddq, void *dk, int lddk, void *dv, int lddv, const float *lse,
                            float *delta, const int32_t *cu_q, const int32_t *cu_k, int B, int H, int dh, int max_q, int max_k,
                            int total_q, int total_k, int causal, int dtype, float dropout_p, uint32_t dropout_seed, int q_prescaled,
                            void *workspace, size_t workspace_bytes, void *stream);

/* Which kernels an acai_attn_varlen_* call runs.  The selection rule is a pure host function of the query below (csrc/attn_plan.h):
 * acai_attn_plan evaluates it without touching a device, acai_attn_last_plan reports what the most recent acai_attn_varlen_fwd /
 * acai_attn_varlen_bwd[_ws] call of the calling thread launched (n = 0 before the first one and after a refused call).  A plan has up to
 * four launches, in stream order: the forward at most two (wide kernel, tail kernel), the d_h = 64 backward at most four (wide dQ, dQ of the
 * rows past the full 256-row blocks, wide dK / dV, dK / dV of the rows past them); the one-pass backward is ONE entry that stands for its
 * delta / main / scale launches.  No reference counterpart. */
enum {
    ACAI_ATTN_K_FWD = 0,         /* attn_fwd_kernel<elem, dhp, fast, drop, pre, nq> (attn_varlen.hip) */
    ACAI_ATTN_K_FWD64 = 1,       /* attn_fwd64_kernel<waves> (attn_fwd64.hip): 32 queries per wave, 4 or 8 waves */
    ACAI_ATTN_K_FWD64W = 2,      /* attn_fwd64w_kernel (attn_fwd64w.hip): 64 queries per wave, one wave per SIMD */
    ACAI_ATTN_K_FWD64_TAIL = 3,  /* attn_fwd64_tail_kernel: a sequence's last 256-query block of <= `tail` rows, keys split over 8 waves */
    ACAI_ATTN_K_BWD_DQ = 4,      /* attn_bwd_dq_kernel<elem, dhp, fast, drop, pre> (attn_bwd.hip) */
    ACAI_ATTN_K_BWD_DKV = 5,     /* attn_bwd_dkv_kernel<elem, dhp, fast, drop, pre> */
    ACAI_ATTN_K_BWD_DQ2 = 6,     /* attn_bwd_dq2_kernel: bf16, d_h <= 32, two blocks per wave */
    ACAI_ATTN_K_BWD_DKV2 = 7,    /* attn_bwd_dkv2_kernel */
    ACAI_ATTN_K_BWD64W_DQ = 8,   /* attn_bwd64w_dq_kernel (attn_bwd64w.hip): the full 256-query blocks */
    ACAI_ATTN_K_BWD64W_DKV = 9,  /* attn_bwd64w_dkv_kernel: the full 256-key blocks */
    ACAI_ATTN_K_BWD1P = 10       /* bwd1p_delta_kernel, attn_bwd1p_kernel (whose grid / block / LDS the entry holds), bwd1p_scale_kernel */
};
/* Process-wide overrides of the rule (tests and A/B runs; acai_attn_set_override copies them into every query, so the plan stays pure). */
enum {
    ACAI_ATTN_OV_TWO_BLOCK = 0,  /* 1 (default) / 0: two blocks per wave at d_h <= 32 on long sequences, forward and backward */
    ACAI_ATTN_OV_FWD64 = 1,      /* the bf16 prescaled unmasked d_h = 64 forward: ACAI_ATTN_FWD64_* */
    ACAI_ATTN_OV_BWD64_WIDE = 2, /* its backward: -1 auto (default), 0 one-block kernels, 1 wide dQ, 2 wide dK / dV, 3 both */
    ACAI_ATTN_OV_BWD_1P = 3,     /* 1 (default) / 0: the one-pass d_h = 32 backward when a workspace is lent */
    ACAI_ATTN_OV_XCD_ORDER = 4,  /* XCD-aware block order of the d_h = 64 kernels' one-dimensional grids: -1 auto (default: equal-length batches), 0, 1 */
    ACAI_ATTN_OV_COUNT = 5
};
enum { ACAI_ATTN_FWD64_AUTO = 0 /* wide + tail */, ACAI_ATTN_FWD64_NW4 = 1, ACAI_ATTN_FWD64_NW8 = 2 /* attn_fwd64_kernel<4> / <8> */,
       ACAI_ATTN_FWD64_GENERIC = 3 /* attn_fwd_kernel */ };
/* why a plan is empty: the entry then fails with its error text */
enum { ACAI_ATTN_REFUSE_NONE = 0, ACAI_ATTN_REFUSE_PRESCALED = 1 /* q_prescaled without aligned operands */,
       ACAI_ATTN_REFUSE_ACCUM = 2 /* accumulating dk / dv without bf16 and aligned operands */ };
typedef struct AcaiAttnQuery {
    int backward;                /* 0: acai_attn_varlen_fwd, 1: acai_attn_varlen_bwd[_ws] */
    int elem_size;               /* 2 (bf16) or 4 (fp32) */
    int B, H, dh, max_q, max_k, total_q, total_k;   /* forward: max_k, total_k unused; total_k = 0: unknown */
    int causal, accum_dkv, dropout, q_prescaled;
    int ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv; /* row strides in elements (forward: the first four) */
    int aligned;                 /* every operand's base (backward: the gradients' too) is 16-byte aligned */
    int cu_k_is_cu_q;            /* self-attention: the keys' offsets are the queries' */
    int ov[ACAI_ATTN_OV_COUNT];  /* acai_attn_set_override */
    long long workspace_bytes;   /* backward: bytes of workspace lent (0: none) */
} AcaiAttnQuery;
typedef struct AcaiAttnLaunch {
    int kernel;                  /* ACAI_ATTN_K_* */
    int elem_size, dhp, fast, drop, pre, nq, waves;   /* template form: element, head-size class 32 / 64, 16-byte loads, dropout, prescaled q,
                                                         blocks per wave, K_FWD64's waves (forms a kernel does not have: 0) */
    int grid_x, grid_y, grid_z, block, lds_bytes;     /* lds_bytes: dynamic LDS */
    /* host-decided kernel arguments */
    int tail;                    /* AttnArgs::tail: K_FWD64W leaves, K_FWD64_TAIL takes, last blocks of <= tail rows */
    int tail256;                 /* BwdArgs::tail256.  K_BWD_DQ / K_BWD_DKV: 1 / 2 = only the rows past each sequence's last full 256-row
                                    block (dQ / dK, dV).  K_BWD1P: 1 = XCD-aware block order */
    int nblk;                    /* AttnArgs::nqb / BwdArgs::nblk: blocks per (sequence, head) of a one-dimensional grid; < 0: plain block order */
    int partial_blocks, equal_len;   /* K_BWD1P: a slot for the keys past the last full 512-key block; batch known to be equal-length */
    int rows;                    /* rows per sequence that the grid covers */
} AcaiAttnLaunch;
/* launches_out: room for four launches; *n_out: how many the plan has; *refusal_out (may be NULL): ACAI_ATTN_REFUSE_*. */
int acai_attn_plan(const AcaiAttnQuery *query, AcaiAttnLaunch *launches_out, int *n_out, int *refusal_out);
int acai_attn_last_plan(AcaiAttnLaunch *launches_out, int *n_out);
int acai_attn_set_override(int which, int value);
int acai_attn_get_override(int which, int *value_out);

/* Backward of nn.LayerNorm: dx (fp32) from x, w, dy; dw/db (both or neither NULL) are ACCUMULATED with fp32 atomics (zero or seed
 * them); dx_bf16 (may be NULL; needs dim % 256 == 0, dim <= 1024): bf16 copy of dx for the GEMM that consumes it; dxsum (may be NULL, same
 * condition; ACCUMULATED): column sums of dx as that GEMM sees it = the consuming nn.Linear's bias gradient; stats: workspace [rows][2]. */
int acai_layernorm_bwd(const float *x, const float *w, const float *dy, float eps, float *dx, void *dx_bf16, float *dw, float *db, float *dxsum,
                       float *stats, int rows, int dim, void *stream);
/* exact-erf GELU as a stand-alone pass (training keeps the pre-activation) and its derivative: da = dh * gelu'(a). */
int acai_gelu_fwd(const void *a, void *h, int64_t n, int dtype, void *stream);
int acai_gelu_bwd(const void *a, const void *dh, void *da, int64_t n, int dtype, void *stream);
/* out[c] += sum_r x[r,c] (bias gradients); out fp32, accumulated with atomics. */
int acai_colsum(const void *x, int ld, float *out, int rows, int cols, int dtype, void *stream);
/* dst[idx[r],:] += src[r,:] (gradients of nn.Embedding M:460, pos_embedding slices M:50, MAE index_select M:114,229).
 * shared_row >= 0: the caller guarantees that only that index occurs more than once (the MAE mask token) - the other rows are then
 * updated without atomics; shared_row < 0: every row through fp32 atomics. */
int acai_scatter_add_rows(const float *src, const int32_t *idx, float *dst, int rows, int dim, int shared_row, void *stream);
/* Token-to-image alignment (an extension; no reference counterpart): the attention probabilities that acai_attn_varlen_fwd never
 * materialises, as a weighted mean over heads.  q / k / cu_q / cu_k / H / dh / dtype as there (packed, ragged, any row stride >= H*dh; no
 * causal mask: cross-attention); max_q / max_k bound the sequence lengths.  lse [H][total_q]: the log2-domain log-sum-exp that
 * acai_attn_varlen_fwd wrote for the SAME q and k; head_w [H] fp32 and map_off [B] int64 (element offsets into out) live on the device.
 * Image b owns the dense fp32 block [T_b][S_b] at out + map_off[b], row pitch S_b:
 *   out[t][s] = (accumulate ? out[t][s] : 0) + sum_h head_w[h] * exp2(q_h[t] . k_h[s] * log2(e) / sqrt(dh) - lse[h][t])
 * summed in head order (the same bits every run; a head of weight 0 is skipped); nothing outside the blocks is written.  bf16 with dh 32 /
 * 64 and 16-byte aligned rows runs on the matrix cores, everything else as plain fp32 FMAs (fp32 operands are never rounded to bf16).
 * Enqueues one kernel: no allocation, no host synchronisation.  Errors: null operand, dh > 64, H < 1, unknown dtype. */
int acai_attn_probs_mean(const void *q, int ldq, const void *k, int ldk, const int32_t *cu_q, const int32_t *cu_k, int B, int H, int dh,
                         int max_q, int max_k, int dtype, const float *lse, int total_q, const float *head_w, const int64_t *map_off,
                         float *out, int accumulate, void *stream);
/* One launch reduces every row of such maps to a location.  grid_w [B] int32 on the HOST (checked here, carried as kernel arguments;
 * B <= 512): patches per image row - patch s of image b sits at x = s % grid_w[b], y = s / grid_w[b] (the encoder's row-major order).
 * patch [total_q] int32: arg-max patch, the lower index on ties.  loc [total_q][6] fp32: row sum m, peak probability, centroid
 * (sum p (x + 1/2) / m, sum p (y + 1/2) / m), standard deviations around it (sx, sy).  fp32 accumulation in a fixed order; a row with
 * m == 0 gives centroid and spread 0 and patch 0.  Errors: null operand, grid_w[b] < 1, B > 512. */
int acai_attn_map_locate(const float *map, const int64_t *map_off, const int32_t *cu_q, const int32_t *cu_k, const int32_t *grid_w,
                         int B, int max_q, int32_t *patch, float *loc, void *stream);
/* Per-token confidence (an extension; no reference counterpart): what a decode step's selection launch knew and threw away.  logits [N][V]
 * fp32, rows back to back; chosen [N] int64 in [0, V) (the CALLER checks that: the kernel reads logits[r][chosen[r]]); 1 <= top_k <= min(8, V);
 * temperature > 0.  One launch, one wave per row.  With z = logits[r] / temperature and lse = logsumexp(z):
 *   log_prob[r] = z[chosen[r]] - lse;   entropy[r] = -sum_i p_i log p_i in nats (p_i = 0 contributes 0);
 *   rank[r]     = how many tokens come before chosen[r] in the row's order - raw logit descending, then index ascending (0: the arg-max,
 *                 first index on ties, as the greedy step picks it);
 *   top_ids[r][0..top_k), top_log_probs[r][0..top_k) = the first top_k tokens of that order and their z - lse.
 * The order is decided on the raw fp32 logits, so the integer outputs are exact.  -inf logits are allowed: log-probability -inf, ordered
 * last by index; a row whose maximum is -inf or that holds a NaN is outside the contract.  The same bits on every run.  N == 0 returns
 * at once.  Errors: null operand, V < 1, top_k or temperature out of range. */
int acai_token_confidence(const float *logits, const int64_t *chosen, int N, int V, int top_k, float temperature, float *log_prob,
                          float *entropy, int32_t *rank, int32_t *top_ids, float *top_log_probs, void *stream);
/* The maps of acai_attn_probs_mean (map / map_off / cu_q / cu_k as there) summed over the token axis with one fp32 weight per token
 * (weights [total_q], packed like the tokens): out[cu_k[b] + s] = sum_t weights[cu_q[b] + t] * map_b[t][s], fp32 [total_k], packed like the
 * patches.  max_q / max_k bound the sequence lengths.  The token axis is cut into splits of 32 tokens, one workgroup per split and 256
 * columns, so that one image fills the device; each split is summed in token order and a second launch adds the splits in order: the same
 * bits on every run, no atomics.  partial: workspace of ceil(max_q / 32) * total_k floats (may be NULL when max_q <= 32: one launch).  An
 * image without tokens gets zeros.  Errors: null operand, bad dims, B > 65535. */
int acai_attn_map_weighted_sum(const float *map, const int64_t *map_off, const int32_t *cu_q, const int32_t *cu_k, const float *weights,
                               int B, int max_q, int max_k, int64_t total_k, float *partial, float *out, void *stream);

/* Per-measure results (measures.hip; an extension, no reference counterpart): token rows cut at delimiter tokens, and per-token results
 * reduced over the spans between them.  All four entries enqueue kernels only - no allocation, no host synchronisation, capturable in a
 * hipGraph - use no floating-point atomics (the same bits on every run), check their arguments before the launch (-1, nothing launched) and
 * return at once for zero rows.  What they read from DEVICE memory to index with (lengths, bounds, counts, ranges) is clamped to the buffers.
 *
 * acai_token_segments: tokens [R][ld] int64 (row stride = ld >= 1), lens [R] int32 read on the device and clamped to [0, ld]; delims: 1 .. 8
 * token ids in a HOST array (carried as kernel arguments); stop: the <eos> id, or -1 for none; cap >= 1.  For row r with clamped length L:
 *   E        = the first p < L with tokens[r][p] == stop, L without one;   c(p) = the number of delimiter tokens at indices <= p;
 *   seg      [R][ld]     int32: c(p) - 1 for p < E (so -1 before the first delimiter, <bos> included), -1 for E <= p < ld;
 *   count    [R]         int32: c(E - 1), 0 when E == 0 - the TRUE count, also when it exceeds cap;
 *   bounds   [R][cap][2] int32: for m < min(count, cap) (start, end) = (index of the m-th delimiter, index of the next delimiter or E);
 *                               (-1, -1) for min(count, cap) <= m < cap.
 * Every element of seg, count and bounds is written.  One wave per row, chunks of 64 tokens, a ballot / popcount scan with a carry.
 * Errors: null operand, ld < 1, R < 0, n_delims outside 1 .. 8, cap < 1, stop < -1.
 *
 * acai_segment_reduce: values [K][R][ld] fp32, 1 <= K <= 8; bounds / count / cap as acai_token_segments wrote them.  Outputs [K][R][cap]: sum,
 * min, max fp32 and argmin, argmax int32 (token indices within the row; the lowest index on ties) of values[k][r][start .. end) for
 * m < min(count[r], cap); 0 and -1 beyond (and for a span that is empty after clamping to [0, ld]).  Every element is written.  One wave per
 * (k, r, m): lane j takes start + j, start + j + 64, ... in ascending order, then a fixed xor butterfly (1, 2, .. 32) - a sum is at most
 * ceil(len / 64) + 6 additions deep.  A NaN inside a span is outside the contract.  Errors: null operand, K outside 1 .. 8, ld < 1, cap < 1,
 * R < 0, K * R * cap >= 2^31.
 *
 * acai_attn_map_segment_sum: the segmented form of acai_attn_map_weighted_sum.  map / map_off / cu_q / cu_k as there; weights [total_q] fp32
 * or NULL (all ones; the same bits as a tensor of ones); ranges [total_seg][2] int32: half-open ranges [t0, t1) of MAP ROWS within the
 * image's block (map row t belongs to token index t + 1: pass token bounds minus one), clamped to [0, T_b] on the device - an empty or
 * out-of-block range is for the caller to refuse; cu_seg [B + 1] int32; seg_map_off [B] int64, all in device memory.  Image b with n_b
 * segments owns the dense [n_b][S_b] block at out + seg_map_off[b]:
 *   out[m][s] = sum over t in range m, ascending, of weights[cu_q[b] + t] * map_b[t][s]          (fmaf into one accumulator per column)
 * - the layout of per-token maps with cu_seg in the place of cu_q, so acai_attn_map_locate, acai_attn_map_expand and acai_attn_map_extent
 * apply to it unchanged.  max_k bounds S_b, max_seg bounds n_b (either 0, or B == 0: returns at once).  One workgroup per (segment, 256
 * columns): coalesced loads, every map element of a range read once.  Errors: null operand, bad dims, B or max_seg > 65535.
 *
 * acai_attn_map_extent: a quantile box for every row of such maps (per token or per segment).  grid_w [B] int32 on the HOST, as
 * acai_attn_map_locate takes it, 1 .. 4096; 0 <= q < 0.5.  For a row p over S_b patches, n_x = min(grid_w, S_b) columns and n_y =
 * ceil(S_b / grid_w) grid rows (the last may be partial): column marginal a[x] = sum_y p[y * grid_w + x], C[i] = a[0] + .. + a[i] added in
 * that order (C[-1] = 0), m = C[n - 1];
 *   pos(target) = i + (target - C[i - 1]) / a[i] for the smallest i with C[i] >= target and a[i] > 0; n without such an i;
 *   x0 = pos(q m), x1 = pos((1 - q) m);   y0, y1 the same from the row marginal and its own m.
 * ext [total rows][4] fp32 = (x0, y0, x1, y1) in patch units, row cu_q[b] + t; m == 0 gives zeros (per axis), as does n_y > 4096 (for the
 * caller to refuse: S_b is device data).  One workgroup per row; marginals in LDS; fixed orders.  max_q == 0 or B == 0 returns at once.
 * Errors: null operand, B > 512, grid_w outside 1 .. 4096, q outside [0, 0.5). */
int acai_token_segments(const int64_t *tokens, int ld, const int32_t *lens, int R, const int64_t *delims, int n_delims, int64_t stop, int cap,
                        int32_t *seg, int32_t *count, int32_t *bounds, void *stream);
int acai_segment_reduce(const float *values, int K, int R, int ld, const int32_t *bounds, const int32_t *count, int cap, float *sum, float *vmin,
                        float *vmax, int32_t *argmin, int32_t *argmax, void *stream);
int acai_attn_map_segment_sum(const float *map, const int64_t *map_off, const int32_t *cu_q, const int32_t *cu_k, const float *weights,
                              const int32_t *ranges, const int32_t *cu_seg, const int64_t *seg_map_off, int B, int max_k, int max_seg, float *out,
                              void *stream);
int acai_attn_map_extent(const float *map, const int64_t *map_off, const int32_t *cu_q, const int32_t *cu_k, const int32_t *grid_w, int B,
                         int max_q, float q, float *ext, void *stream);

/* nn.Dropout on a projection output followed by the residual add (torch TransformerEncoderLayer dropout1/dropout2, decoder dropout1-3,
 * transition head M:658): out = residual + keep * x / (1 - p); residual may be NULL (plain dropout, and its own backward on dy).
 * keep mask = counter-based hash of (seed, row, col). */
int acai_dropout_add(const void *x, const float *residual, void *out, int rows, int cols, float p, uint32_t seed, int x_dtype, int out_dtype,
                     void *stream);
/* MAELoss (M:271-288) forward + backward on packed rows: *loss += sum_r mask_r * mean_d((pred - that)^2) * inv_count,
 * dpred (may be NULL) = d loss / d pred; that = (target - mean) / sqrt(var_unbiased + 1e-6). */
int acai_mae_loss(const float *pred, const float *target, const unsigned char *mask, float inv_count, float *loss, float *dpred,
                  int rows, int dim, void *stream);
/* OMRCELoss (M:784-796) forward + backward: mean cross entropy over rows whose target != ignore_index, with nn.CrossEntropyLoss's
 * label_smoothing (M:786-788; 0 = plain NLL). */
int acai_ce_loss(const float *logits, int ld, const int64_t *target, int ignore_index, float inv_count, float label_smoothing, float *loss,
                 float *dlogits, int rows, int V, void *stream);

/* GRPO objective and entropy bonus (acai_omr/train/omr_grpo_train.py:240-283: calc_grpo_objective, calc_policy_theta_entropy /
 * calc_entropy_bonus; grpo_update calls both on the same theta logits, :354-355) in one pass over logits [R][T][V] (contiguous, dtype
 * ACAI_F32 / ACAI_BF16, 16-byte aligned, V <= 1024).  Position (r, t) counts when mask[r*T + t] == 0 (rollout_attention_mask, uint8); its action
 * is rollouts[r*ld_roll + t + 1] (int64), its old log-probability old_lp[r*ld_old + t + 1]; adv[R] are the advantages.  clip_lo / clip_hi =
 * 1 -/+ epsilon, logv = log(V) as the reference rounds it (fp32).  out[0] = objective = sum_r (sum_t min(ratio A, clip(ratio) A) / len_r) /
 * num_groups, out[1] = bonus = mean_r (sum_t H / len_r) / logv.  stats [R*T][4] and rowstat [R][4] (fp32, 16-byte aligned) are workspaces the
 * backward reads.  Deterministic: fixed-order reductions, no atomics.  Entropy terms with p_c == 0 count 0 (the reference gives NaN for -inf logits).
 * _bwd: dlogits (logits' dtype, zero at masked positions) of grad_out[0] * objective + grad_out[1] * bonus, grad_out = 2 floats in DEVICE memory
 * (no host sync); autograd's tie and band rules for the min / clip (grpo.hip). */
int acai_grpo_objective_fwd(const void *logits, int dtype, const int64_t *rollouts, int ld_roll, const float *old_lp, int ld_old,
                            const unsigned char *mask, const float *adv, int R, int T, int V, float clip_lo, float clip_hi, int num_groups,
                            float logv, float *stats, float *rowstat, float *out, void *stream);
int acai_grpo_objective_bwd(const void *logits, int dtype, const int64_t *rollouts, int ld_roll, const unsigned char *mask, const float *stats,
                            const float *rowstat, const float *grad_out, int R, int T, int V, int num_groups, float logv, void *dlogits,
                            void *stream);

/* Batched unit-cost Levenshtein distance (insert, delete, substitute cost 1 each) between ragged token rows in device memory (seqdist.hip): the
 * token-level edit cost of the GRPO reward and the numerator of the symbol error rate.  pred [R][ld_pred] and tgt [R / group][ld_tgt] are int64
 * rows (row stride = width = ld), pred_len [R] and tgt_len [R / group] int32.  Pair r compares pred[r][0 .. pred_len[r]) with
 * tgt[r / group][0 .. tgt_len[r / group]): `group` consecutive rows of pred share one target row (G rollouts of one image), R % group == 0.
 * out [R] int32 receives the distances.  The lengths are read ON THE DEVICE and clamped to [0, ld] there: no host synchronisation, no allocation,
 * one kernel launch, capturable in a hipGraph.  Either length may be 0 (the distance is then the other length); positions past a row's length are
 * never read.  ld_pred, ld_tgt <= 4096; a larger one is refused (-1).  Token ids are compared by their low 32 bits: exact for ids in [0, 2^31),
 * no vocabulary size is assumed.  Integer arithmetic without atomics: results are the same on every run. */
int acai_edit_distance(const int64_t *pred, int ld_pred, const int32_t *pred_len, const int64_t *tgt, int ld_tgt, const int32_t *tgt_len, int R,
                       int group, int32_t *out, void *stream);

/* The edit ALIGNMENT behind that distance (seqalign.hip): which pred tokens match, are substituted or inserted, which target tokens are deleted,
 * and where.  Rows, lengths, `group`, the clamping of the lengths on the device, the 4096-token limit and the comparison of ids by their low
 * 32 bits are acai_edit_distance's.  Outputs, all written by the launch (no atomics: the same bits on every run):
 *   counts      [R][4]       int32: matches, substitutions, insertions, deletions (the last three add up to the distance);
 *   pred_op     [R][ld_pred] int8:  0 match, 1 substitution, 2 insertion; -1 past the row's length;
 *   pred_to_tgt [R][ld_pred] int32: the aligned target index; -1 for an insertion and past the length;
 *   tgt_to_pred [R][ld_tgt]  int32: the aligned pred index; -1 for a deleted target token and past the length;
 *   tgt_slot    [R][ld_tgt]  int32: pred tokens consumed before target token j on the path (non-decreasing in j; for a deleted token: the pred
 *                                   index it is missing in front of, in [0, pred_len]); -1 past the length.
 * The target-side outputs have one row per PRED row (group rows of them per target row).
 * THE ALIGNMENT IS CANONICAL.  On the table D[i][j] (pred prefix i, target prefix j), start at (pred_len, tgt_len); at (i, j):
 *   1. if i > 0, j > 0 and D[i-1][j-1] + [pred[i-1] != tgt[j-1]] == D[i][j]: step diagonally (match or substitution);
 *   2. otherwise, if i > 0 and D[i-1][j] + 1 == D[i][j]: insertion (pred token i-1 is extra), i decreases;
 *   3. otherwise: deletion (target token j-1 is missing), j decreases.
 * workspace: device memory, 16-byte aligned, of at least acai_edit_align_workspace_bytes(ld_pred, ld_tgt, R) bytes (the direction words of the
 * forward sweep: (min(ld) + 63) * ceil(2 W / 32) * 256 bytes per pair, W the strip width of max(ld); 0 for arguments acai_edit_align
 * refuses).  Every pointer, R % group == 0, the widths and the workspace size are checked BEFORE the launch (-1).  One kernel launch, no host
 * synchronisation, no allocation: capturable in a hipGraph. */
size_t acai_edit_align_workspace_bytes(int ld_pred, int ld_tgt, int rows);
int acai_edit_align(const int64_t *pred, int ld_pred, const int32_t *pred_len, const int64_t *tgt, int ld_tgt, const int32_t *tgt_len, int R,
                    int group, int32_t *counts, int8_t *pred_op, int32_t *pred_to_tgt, int32_t *tgt_to_pred, int32_t *tgt_slot, void *workspace,
                    size_t workspace_bytes, void *stream);

/* Fused multi-tensor AdamW: one launch steps every parameter tensor (reference: torch.optim.AdamW in acai_omr/train/pre_train.py:105 and
 * omr_teacher_force_train.py:207 over the param groups of acai_omr/models/models.py:761-781; the cosine/warm-up schedule of
 * acai_omr/utils/utils.py:204-222 only changes `lr`).  All tables live in DEVICE memory.  tensors[i]: fp32 parameter, gradient and the two
 * moment buffers (n elements) + the index of its hyper-parameter group; groups[j]: this step's lr, betas, eps, weight decay and bias
 * corrections bc1 = 1 - beta1^t, sqrt(bc2) = sqrt(1 - beta2^t).  chunk_tensor / chunk_off: one entry per workgroup = (tensor, first element)
 * of a chunk of chunk_elems (multiple of 4) elements.  grad_scale multiplies every gradient on load (loss-scale / accumulation mean; 1 = none). */
typedef struct AcaiAdamWTensor {
    float *p;
    const float *g;
    float *m, *v;
    int64_t n;
    int32_t group, pad_;
    float bias_c1, bias_c2_sqrt; /* 1 - beta1^t, sqrt(1 - beta2^t) with THIS tensor's step count t (torch keeps `step` per parameter) */
} AcaiAdamWTensor;
typedef struct AcaiAdamWGroup {
    float lr, beta1, beta2, eps, weight_decay, pad0_, pad1_, pad2_;
} AcaiAdamWGroup;
int acai_adamw_step(const AcaiAdamWTensor *tensors, const AcaiAdamWGroup *groups, const int32_t *chunk_tensor, const int64_t *chunk_off,
                    int n_chunks, int chunk_elems, float grad_scale, void *stream);

/* Global gradient norm over the tensors of an AdamW tensor table, and the AdamW step that clips by it (reference:
 * torch.nn.utils.clip_grad_norm_(max_norm=1.0) between backward and optimizer.step(), acai_omr/train/omr_grpo_train.py:367).  No host
 * synchronisation, no write of scaled gradients, no float atomics: the result repeats bit for bit from run to run.
 *
 * acai_grad_norm reads only `g` and `n` of tensors[]; chunk_tensor / chunk_off are the tables acai_adamw_step takes, and tensor_chunk0
 * (n_tensors + 1 int32, device) holds each tensor's first chunk, tensor_chunk0[n_tensors] = n_chunks: the chunks of a tensor are contiguous
 * and in element order.  workspace: n_chunks doubles (device, 8-byte aligned).  Two launches: per chunk, the sum of g * g in fp64; then one
 * workgroup adds the chunks of each tensor and the tensors, in fp64 and in a fixed order.  It writes
 *   tensor_norm[i] (optional, may be NULL)   |grad_scale| * sqrt(sum over tensor i), fp32
 *   result[ACAI_GRAD_NORM_TOTAL]             N = the norm of grad_scale * g over all tensors, fp32
 *   result[ACAI_GRAD_NORM_COEF]              c = min(1, max_norm / (N + 1e-6)), in fp32 from the fp32 N (torch's formula and order; a NaN
 *                                            N gives a NaN c, as torch's clamp does); c = 1 when max_norm is not positive or not finite
 *   result[ACAI_GRAD_NORM_FINITE]            1.0f if N is finite, 0.0f otherwise
 * result has ACAI_GRAD_NORM_WORDS floats.
 *
 * acai_adamw_step_clipped is acai_adamw_step with the gradient multiplier grad_scale * result[ACAI_GRAD_NORM_COEF].  With skip_nonfinite != 0
 * and result[ACAI_GRAD_NORM_FINITE] == 0 it leaves parameters and both moments untouched and adds 1 to *skipped (device int32). */
#define ACAI_GRAD_NORM_TOTAL 0
#define ACAI_GRAD_NORM_COEF 1
#define ACAI_GRAD_NORM_FINITE 2
#define ACAI_GRAD_NORM_WORDS 4
int acai_grad_norm(const AcaiAdamWTensor *tensors, const int32_t *chunk_tensor, const int64_t *chunk_off, const int32_t *tensor_chunk0,
                   int n_tensors, int n_chunks, int chunk_elems, float grad_scale, float max_norm, double *workspace, float *tensor_norm,
                   float *result, void *stream);
int acai_adamw_step_clipped(const AcaiAdamWTensor *tensors, const AcaiAdamWGroup *groups, const int32_t *chunk_tensor, const int64_t *chunk_off,
                            int n_chunks, int chunk_elems, float grad_scale, const float *result, int skip_nonfinite, int32_t *skipped,
                            void *stream);

/* The operand copies autocast makes of the fp32 master weights (torch casts each nn.Linear weight / bias to bf16 on every call under
 * torch.autocast, omr_teacher_force_train.py:112-116; this path caches them per parameter version) for ALL parameters in one launch, after an
 * optimizer step: per entry any of the bf16 copy [rows][cols], the transposed bf16 copy [cols][rows] (the dX GEMM's row-major operand) and
 * the bf16-rounded fp32 copy (biases).  `table` is device memory; tile0 = running sum of ceil(rows/64) * ceil(cols/64) over the entries
 * before this one, n_tiles the total.  src and the destinations are contiguous; destinations are 8-byte aligned. */
typedef struct AcaiCastEntry {
    const float *src;
    void *dst16, *dst16t;
    float *dst32r;
    int32_t rows, cols, tile0, pad_;
} AcaiCastEntry;
int acai_cast_weights(const AcaiCastEntry *table, int n_entries, int n_tiles, void *stream);

/* ---- KV-cached greedy decode (K:190-223, K:292-302, M:518-528, M:575-583) ------------------------------- */
typedef struct {
    const void *self_in_w;   const float *self_in_b;   /* self_attn.in_proj_{weight,bias} [3E,E] */
    const void *self_out_w;  const float *self_out_b;  /* self_attn.out_proj */
    const void *cross_q_w;   const float *cross_q_b;   /* rows 0..E of multihead_attn.in_proj (K:212-213) */
    const void *cross_out_w; const float *cross_out_b; /* multihead_attn.out_proj */
    const void *lin1_w;      const float *lin1_b;      /* linear1 [F,E] */
    const void *lin2_w;      const float *lin2_b;      /* linear2 [E,F] */
    const float *n1_w, *n1_b, *n2_w, *n2_b, *n3_w, *n3_b;
    void *k_self, *v_self;              /* KVCache (K:35-41) as [Bmax][H][Tmax][dhp] */
    const void *k_cross, *v_cross;      /* acai_cross_kv_prefill output (bf16 / fp32), or acai_cross_kv_quantize_fp8 output (ACAI_DEC_CROSS_FP8) */
    const float *k_cross_scale, *v_cross_scale;  /* ACAI_DEC_CROSS_FP8: per-row scales of k_cross / v_cross, else unused */
} AcaiDecLayer;

/* AcaiDecoder.flags: besides ACAI_GEMM_ROUND_BF16, ACAI_DEC_CROSS_FP8 = the cross K/V of every layer is e4m3fn with per-row scales
 * (bf16 decoder, cross_group 1).  Its rows are dhp8 = max(dhp, 16) elements (element offset cross_off[b] + (h*S_b + s)*dhp8, scale at
 * that offset / dhp8), and `partial` must hold B*H*cross_nsplit*(dhp8+2) floats.  The self-attention caches keep `dtype`. */
#define ACAI_DEC_CROSS_FP8 256


typedef struct {
    int32_t B, E, H, dh, dhp, F, V, L, Tmax, dtype, flags, max_len;
    int32_t self_chunk, cross_chunk;    /* keys per attention workgroup */
    int32_t self_nsplit, cross_nsplit;  /* workgroups per (b, h) */
    int32_t bos, pad, eos;
    int32_t cross_group;   /* > 1: every `cross_group` consecutive rows share one memory (GRPO rollouts of one image): its K/V is streamed once per group */
    const AcaiDecLayer *layers;         /* host array of L entries */
    const float *emb;                   /* vocab_embedding.weight [V,E] fp32 */
    const float *pos;                   /* decoder pos_embedding [Tmax,E] fp32 */
    const float *fn_w, *fn_b;           /* decoder_blocks.norm (eps 1e-6) */
    const void *unembed_w;              /* [V,E] in `dtype` */
    const float *unembed_b;
    const int64_t *cross_off;           /* [B] element offset of sequence b in k_cross / v_cross */
    const int32_t *cross_len;           /* [B] memory length S_b */
    int64_t *seqs;                      /* [B,max_len] token ids, seqs[:,0] = <bos> (M:568-569) */
    float *logprobs;                    /* [B,max_len] (M:570) */
    int32_t *step;                      /* device scalar t: next position to fill (starts at 1) */
    int32_t *finished;                  /* [B] flags + [B] = count of unfinished rows after the step */
    float *x, *xn, *qkv, *attn, *proj, *hid, *logits, *partial; /* workspaces, see DESIGN.md */
    uint32_t *tickets;                  /* B*H zeroed arrival counters for the in-launch split merge; NULL = separate combine launch */
    float *stats;                       /* 6*B floats: published LayerNorm (mean, rstd) rows; NULL disables the fused-LN path */
} AcaiDecoder;

/* Input of the FIRST step after the device-side loop state was armed: x = vocab_embedding[seqs[:, t-1]] + pos_embedding[t], t = step[0]
 * (M:521-524 with quirk Q1).  Every later step's input is written by the previous step's argmax / sampling kernel. */
int acai_decode_embed(const AcaiDecoder *dec, void *stream);
/* One greedy step t = *step for all B rows: input x = embedding of seqs[:,t-1] at pos_embedding[t] (quirk Q1, M:576), 12x cached_forward,
 * final norm, unembed, argmax + log_softmax gather, seqs[:,t] / logprobs[:,t] update, finished flags, ++*step.  Enqueues only kernels:
 * capture it in a hipGraph and replay.
 * CONTRACT (E % 4 == 0): the step does NOT embed its own input - dec->x must hold it: written by acai_decode_embed after arming, and by every
 * step's argmax / sampling kernel for the next one.  acai_decode_logits and acai_decode_hidden overwrite dec->x: after either, call
 * acai_decode_embed again before the next acai_decode_step / acai_decode_sample_step.  ENFORCED since round 4: the library records per
 * decoder state (keyed by dec->x) whether x holds a chained step's input - set by acai_decode_embed, kept by the step entry points, cleared
 * by acai_decode_logits / acai_decode_hidden - and acai_decode_step / acai_decode_sample_step return an argument error (rc < 0,
 * acai_last_error() names acai_decode_embed) when it does not.  Replays of a captured graph do not pass through the check.
 * tickets: the in-launch merge is used only while decode_attn_kernel's residency is the one it was validated at (two workgroups per CU,
 * hipOccupancyMaxActiveBlocksPerMultiprocessor); otherwise the step issues the separate combine launch as if tickets were NULL. */
int acai_decode_step(const AcaiDecoder *dec, void *stream);
/* One SAMPLING decode step for every sequence (GRPOViTOMR.cached_forward_rollout_policy, acai_omr/models/models.py:988-1049): as
 * acai_decode_step, but the next token is drawn from softmax(top_k(logits) / temperature) and its log-probability is taken under
 * softmax(top_k(logits)) (models.py:1006-1019).  The draw is the inverse CDF of uniforms[b * max_len + t] over the kept logits in
 * descending order (ties: lower index first), 1 <= top_k <= 64: torch.multinomial's random stream is replaced by caller-supplied uniforms. */
int acai_decode_sample_step(const AcaiDecoder *d, const float *uniforms, int top_k, float temperature, void *stream);

/* Beam-search state (an extension: the reference decodes greedily only).  Decode row i*K + k is beam slot k of image i; the rows of an
 * image are one cross-attention group (dec->cross_group = K).  All buffers are device memory, armed by the caller:
 *   anc/tok/lp: two parity copies [2][rows][pitch] of the lineage of every row, copy (t & 1) valid before step t = step[0]; anc[r][p] =
 *               the cache row holding row r's self K/V at position p (armed: r), tok / lp = the row's tokens and per-token log-probs
 *               (armed: <bos> at 0, <pad> after; 0).  A step reads copy (t & 1) and writes copy (t + 1) & 1: the parity is taken on the
 *               device from step[0], so graphs of any step count may be mixed.
 *   cum:        [B] fp32 cumulative log-probability (armed: 0 for slot 0, -inf for slots 1..K-1).
 *   len:        [B] int32 generated length (tokens after <bos>, <eos> included) once the row finished, 0 while it runs (armed: 0). */
typedef struct {
    int32_t K;         /* beam width, 1..16; dec->B % K == 0 */
    int32_t pitch;     /* positions per lineage row, >= dec->max_len */
    int32_t rows;      /* rows per parity copy, >= dec->B */
    int32_t pad_;
    int32_t *anc;
    int64_t *tok;
    float *lp;
    float *cum;
    int32_t *len;
} AcaiBeam;
/* One BEAM-SEARCH decode step t = step[0] for every row: the greedy step's layers with the self attention read through the ancestor table
 * (the K/V caches are never moved), then per image: every live row (cum > -inf, not finished) proposes its K best tokens by raw logit
 * (lower index first on ties) with score cum + lp, lp = (logit - max) - log(sum exp(logit - max)) in fp32 (the greedy step's reduction);
 * a finished row proposes itself extended by <pad> (lp 0, score unchanged); the K best candidates by score (ties: lower parent slot, then
 * lower rank) become slots 0..K-1 with their parent's lineage plus the new token; a chosen <eos> finishes the row (len = t).  Writes cum,
 * len, finished[] and the unfinished count finished[B], the next step's input x, and advances step[0] / step[1].  Slots left without a
 * candidate get cum = -inf and count as finished.  Same checks and the same x contract as acai_decode_sample_step (dec->x must hold the
 * step's input: acai_decode_embed after arming); V <= 512, E % 4 == 0, self_chunk <= 16384. */
int acai_decode_beam_step(const AcaiDecoder *d, const AcaiBeam *bs, void *stream);

/* Continuous-batching state (slot mode; an extension: the reference decodes one static batch).  Each decode row is a SLOT that decodes one
 * image at a time; when it finishes, the caller harvests it and re-arms the row for the next queued image while the other rows go on.
 * The self-attention cache of every row is a ring of Tmax positions: every step writes its self K/V at the shared ring write index step[1]
 * (the same skinny kernels as the greedy step), and the step advances step[1] modulo Tmax.  A row armed when the index was w reads its key
 * j at ring position (w + j) % Tmax.  A row ends by t = cap - 1 <= max_len - 1 <= Tmax - 1, so its window never overwrites its own keys.
 * step[0] is not used in slot mode.  All buffers are device memory:
 *   t:     [rows] int32 local time of each row: the index its next token is written at (armed: 1);
 *   first: [rows] int32 ring index of the row's key 0 (armed: step[1] at arming, read on the device);
 *   cap:   [rows] int32 per-row cap: the row finishes after writing index cap - 1 (armed: 2 <= cap <= max_len).
 * Idle rows (nothing to decode) are kept finished: finished[b] = 1 makes the step write nothing for them.  To keep their cross attention
 * cheap the caller gives them cross_len[b] = 1 inside their own cross K/V region; nothing an idle row computes reaches seqs / logprobs. */
typedef struct {
    int32_t *t;
    int32_t *first;
    int32_t *cap;
    int32_t rows;      /* entries of t / first / cap, >= dec->B */
    int32_t pad_;
} AcaiSlots;
/* One SLOT-MODE greedy step for every row: the greedy step's layers with the self attention of row b over its own t[b] keys on the ring,
 * then for every unfinished row the greedy token and log-prob (the greedy step's reduction) written at seqs[b][t[b]] / logprobs[b][t[b]];
 * a row that emits <eos> or reaches t[b] = cap[b] - 1 is marked finished and writes nothing after that; an unfinished row advances t[b]
 * and gets its next input x[b] = vocab_embedding[token] + pos_embedding[t[b] + 1] (quirk Q1).  Writes the unfinished count finished[B]
 * and advances step[1] modulo Tmax.  Needs cross_group == 1, E % 4 == 0, 2 <= max_len <= Tmax, and the same x contract as
 * acai_decode_step: x must hold the input of every unfinished row (acai_decode_slot_arm sets it; acai_decode_logits / acai_decode_hidden
 * clear it). */
int acai_decode_slot_step(const AcaiDecoder *d, const AcaiSlots *sl, void *stream);
/* One SLOT-MODE SAMPLING step: acai_decode_slot_step with acai_decode_sample_step's token choice.  The layers, the ring self attention,
 * idle rows, finished[] / finished[B], t[] / cap[] and the next input are the greedy slot step's; for every unfinished row b at its LOCAL time
 * t[b] the step keeps the top_k largest logits (ties: lower index first), draws by inverse CDF over softmax(kept / temperature) in
 * descending order with u = uniforms[urow[b] * ld_uniforms + t[b]] and records log_softmax(kept)[drawn] (no temperature) at
 * logprobs[b][t[b]].  uniforms: device fp32 table in [0, 1), ld_uniforms >= max_len floats per row; urow: device int32 [B], the table row
 * of the sequence slot b decodes (the caller writes it when it arms the slot, ordered before the step; rows of idle slots are not read).
 * The per-row arithmetic is the static sampler's own, so a sequence draws what it draws alone through acai_decode_sample_step with its
 * table row.  Same checks and x contract as acai_decode_slot_step, plus 1 <= top_k <= 64, temperature > 0, V <= 512.  With dec->tickets
 * the token choice runs one wave per row over ceil(B / 4) workgroups and uses tickets[0] (zero before, zero after) to close the step;
 * without, one workgroup takes all rows.  Enqueues kernels only (capturable). */
int acai_decode_slot_sample_step(const AcaiDecoder *d, const AcaiSlots *sl, const float *uniforms, int ld_uniforms, const int32_t *urow,
                                 int top_k, float temperature, void *stream);
/* Arms n rows for new sequences (n >= 0).  rows: device int32 [2][n] - rows[i] the decode row, rows[n + i] its cap (clamped to
 * [2, max_len]).  The caller has already set the row's cross_len and prefilled its cross K/V region (e.g. acai_cross_kv_prefill at the
 * row's cross_off), ordered before the next step.  Per row: seqs = <bos> then <pad>, logprobs = 0, finished = 0,
 * t = 1, first = step[1] (read on the device, so arming is stream-ordered after the steps before it), cap, and x = vocab_embedding[<bos>] +
 * pos_embedding[1].  Rows outside [0, B) are ignored.  Marks x valid for acai_decode_slot_step: the caller keeps every row it did not arm
 * either finished or chained from the previous slot step. */
int acai_decode_slot_arm(const AcaiDecoder *d, const AcaiSlots *sl, const int32_t *rows, int n, void *stream);
/* Streaming of a slot-mode run (an extension): collects what slots 0 .. B-1 wrote since the caller last looked, so that one small copy
 * brings a poll's news to the host.  seqs / logprobs: the rows the slot steps write, max_len entries apart; slot_t / finished: AcaiSlots.t
 * and the decoder's flags; mark: device int32 [rows] the caller owns - the first index of each slot not yet handed out (the caller sets 1
 * when it arms a slot, so that <bos> is never sent, and 2 for a parked slot, which is finished at t = 1 and must send nothing).  Per slot s:
 *   end = finished[s] ? t[s] + 1 : t[s]   (the steps leave t at the last token of a finished row and past the last token otherwise),
 *   n = clamp(end - mark[s], 0, ld);   out_tok[s][0 .. n) = (int32) seqs[s][mark[s] .. mark[s] + n);   out_lp[s][0 .. n) likewise from
 *   logprobs;   hdr[s] = {n, mark[s] as it was, finished[s] != 0, 0};   then mark[s] += n - what did not fit stays for the next call.
 * out_tok (int32) and out_lp (fp32) are [B][ld], hdr is int32 [B][4]; entries past n are left as they were.  The three are meant to be
 * views of ONE allocation, so that a single copy fetches them.  Nothing else is written: seqs, logprobs, t and finished are read only.
 * One wave per slot, plain vector stores, no atomics.  Enqueues one kernel, ordered on `stream` after the steps whose tokens it reads
 * and before an acai_decode_slot_arm that re-arms a slot it has not read yet.  Refused (rc < 0, nothing launched): a null pointer, B < 1,
 * rows < B, ld < 1, ld > max_len.  (end is held to max_len and a negative mark sends nothing, so no index leaves a row.) */
int acai_decode_slot_flush(const int64_t *seqs, const float *logprobs, int max_len, const int32_t *slot_t, const int32_t *finished,
                           int32_t *mark, int rows, int B, int ld, int32_t *out_tok, float *out_lp, int32_t *hdr, void *stream);
/* Speculative greedy decoding state (draft and verify; an extension: the reference emits one token per step).  An image owns R = D + 1
 * consecutive decode rows that share its cross K/V (dec->cross_group = R, dec->B = images * R).  With t the image's next index to write,
 * row j of a verify step consumes the token at index t - 1 + j - row 0 the last emitted token, rows 1..D the draft tokens - at
 * pos_embedding[t + j] (quirk Q1) and predicts index t + j.  Every row appends its self K/V at the shared write index step[1] of its own
 * cache row; key p of the image is found through tab[i][p] = 8 * (cache position) + (row of the image), so nothing is moved when drafts
 * are accepted or dropped.  step[0] is not used.  The image's tokens and log-probs land in row i (not i * R) of dec->seqs / dec->logprobs,
 * its flag in finished[i], the count of unfinished images in finished[B].  All buffers are device memory:
 *   t:      [rows] int32 next index to write (armed: 1);
 *   cap:    [rows] int32 the run's max_len for the image: it finishes at <eos> or once index cap - 1 is written (2 <= cap <= max_len);
 *   steps:  [rows] int32 verify steps the image took part in (armed: 0);
 *   tab:    [rows][pitch] int32 key table (armed: 0; acai_decode_spec_arm and every step set entries t - 1 .. t - 1 + D);
 *   next:   [rows][8] int32 the tokens the next step's rows consume: [0] the last emitted token, [1..D] the drafts, -1 = none;
 *   drafts: NULL, or [rows][pitch] int32: drafts[i][p] is the token proposed for index p (outside [0, V): none) and replaces the lookup.
 * The caller arms seqs (<bos> then <pad>), logprobs (0), finished (0), step = {1, 0}, t, cap, steps and tab, then calls
 * acai_decode_spec_arm once. */
typedef struct {
    int32_t D;         /* draft tokens per step, 1..7 */
    int32_t ngram;     /* longest suffix the prompt-lookup drafter matches, 1..8 (unused with drafts) */
    int32_t pitch;     /* entries per image of tab / drafts: max_len <= pitch <= Tmax */
    int32_t rows;      /* images the arrays hold, >= dec->B / (D + 1) */
    int32_t *t;
    int32_t *cap;
    int32_t *steps;
    int32_t *tab;
    int32_t *next;
    const int32_t *drafts;
} AcaiSpec;
/* Opens a speculative run on the armed state: drafts the first step (t = 1), sets the table entries and every row's input x, writes
 * finished[B].  Marks x valid for acai_decode_spec_step. */
int acai_decode_spec_arm(const AcaiDecoder *d, const AcaiSpec *sp, void *stream);
/* One VERIFY step for every image: the greedy step's layers on all B rows (the same GEMV kernels; self attention of row j over the image's
 * t + j keys through tab; cross attention by the per-row kernel, the rows aliasing the image's K/V, so that a row's arithmetic is the plain
 * greedy step's), then one launch per step: g_j = the greedy token and log-prob of row j (the greedy step's reduction); n = the number of
 * leading drafts with draft_j == g_{j-1}; g_0 .. g_n and their log-probs are written at indices t .. t + n, cut at the first <eos> and at
 * cap - 1; t, finished[] and finished[B] are updated; the next step is drafted - from drafts when given, else for m = ngram .. 1 the most
 * recent earlier occurrence of the sequence's last m tokens, the first m with a match proposing the up to D tokens that followed it - and
 * next, tab and x are written; step[1] advances.  A row whose draft is none, or whose index would reach cap, is idle: what it computes is
 * never read and every index it forms is clamped.  The emitted tokens and log-probs are those of acai_decode_step run token by token.
 * Needs 1 <= D <= 7, B % (D + 1) == 0, cross_group == D + 1, no FP8 cross K/V, max_len <= pitch <= Tmax, rows >= B / (D + 1), ngram in
 * [1, 8] unless drafts is given, self_chunk <= 16384, and x valid (acai_decode_spec_arm; acai_decode_logits / acai_decode_hidden clear it).
 * A run takes at most max_len - 1 steps, so step[1] stays below Tmax.  Enqueues kernels only (capturable). */
int acai_decode_spec_step(const AcaiDecoder *d, const AcaiSpec *sp, void *stream);

/* Prompted decoding (an extension: the reference starts every sequence from <bos> alone).  Sequence i is given the tokens of its output
 * indices 1 .. len[i] (index 0 is always <bos>); from index len[i] + 1 on it decodes greedily.  Both tables are device memory and are read
 * by every step (the caller fills them before the first step and keeps them until the last has run):
 *   tok: [rows][pitch] int32, tok[i][p] the token of output index p for 1 <= p <= len[i]; column 0 and the columns past len[i] are not read.
 *        The caller keeps the ids inside [0, V), never <bos> or <pad>, and <eos> only at index len[i]; an entry outside [0, V) is not
 *        forced (the step is greedy at that index), so that no table content can make the step index out of bounds;
 *   len: [rows] int32 prompt lengths, clamped on the device to [0, min(pitch, max_len) - 1]; 0 = plain greedy decoding of that row. */
typedef struct {
    const int32_t *tok;
    const int32_t *len;
    int32_t pitch;     /* entries per row of tok, >= dec->max_len */
    int32_t rows;      /* rows of tok / len, >= dec->B (speculative entry points: >= dec->B / (D + 1), one row per image) */
} AcaiPrompt;
/* One PROMPTED greedy step t = *step for all B rows: acai_decode_step's layers and unembed, then one selection launch.  A row with
 * t <= len[b] takes tok[b][t] whatever the model prefers; a row with t > len[b] takes the arg-max as acai_decode_step does.  Either way
 * logprobs[b][t] = (logit[token] - max) - logf(sum_j expf(logit[j] - max)) with acai_decode_step's max / sum reduction, rounded to bf16
 * where that step rounds: where the token is the arg-max the first term is exactly 0 and the value is bitwise acai_decode_step's.  The
 * launch also writes seqs[b][t], the next step's input x[b] = vocab_embedding[token] + pos_embedding[t + 1] (quirk Q1), finished[b] (set
 * by <eos>, forced or chosen), the unfinished count finished[B] - a row with t < len[b] always counts as unfinished - and advances step[0]
 * / step[1].  Works for fp32 and bf16 decoders and with an FP8 cross K/V.  Same checks and the same x contract as acai_decode_step, plus
 * non-null tok / len, pitch >= max_len and rows >= B.  Enqueues kernels only (capturable). */
int acai_decode_prompt_step(const AcaiDecoder *d, const AcaiPrompt *prompt, void *stream);
/* acai_decode_spec_arm for a prompted run (prompt row i belongs to image i): the drafts of the first step are the prompt's tokens of
 * indices 1 .. min(D, len[i]) and none beyond; with len[i] = 0 they come from sp's usual source.  Same checks as acai_decode_spec_arm,
 * plus non-null tok / len, prompt->pitch >= max_len and prompt->rows >= B / (D + 1). */
int acai_decode_spec_prompt_arm(const AcaiDecoder *d, const AcaiSpec *sp, const AcaiPrompt *prompt, void *stream);
/* One VERIFY step of a prompted speculative run: acai_decode_spec_step in which row j of an image at write index t, predicting index
 * t + j, emits g_j = tok[i][t + j] while t + j <= len[i] (log-prob as in acai_decode_prompt_step) and its greedy token beyond.  Acceptance,
 * the cut at <eos> and cap - 1, tab, next, x, steps and step[1] are acai_decode_spec_step's.  While the new write index t' <= len[i] the
 * drafts of the next step are the prompt's tokens of indices t' .. min(t' + D - 1, len[i]) and none beyond - so a prompt's drafts are all
 * accepted, and len[i] prompt tokens plus the first free token take ceil((len[i] + 1) / (D + 1)) steps; once t' > len[i] the drafts come
 * from sp's usual source.  What is written equals acai_decode_prompt_step run token by token.  Same checks as acai_decode_spec_step and
 * acai_decode_spec_prompt_arm. */
int acai_decode_spec_prompt_step(const AcaiDecoder *d, const AcaiSpec *sp, const AcaiPrompt *prompt, void *stream);
/* Prompt prefill (an extension): the C >= 1 prompt tokens that ALL rows have (C <= min_b len[b]) computed in one teacher-forced pass by the
 * caller instead of C prompt steps.  The pass runs B sequences of C tokens - row b's tokens of output indices 0 .. C - 1, index 0 being
 * <bos> - at positions 1 .. C (quirk Q1) over the rows' memories, at the decoder's precision, and keeps per layer the self-attention
 * in-projection `qkv` [(b * C + p)][ld] in the decoder's dtype and at the end the logits [(b * C + j)][V] fp32 (row b * C + j scores output
 * index j + 1).  Then, on one stream:
 *   acai_decode_prefill_self_kv per layer: k_self / v_self [b][h][p][d] = qkv[b * C + p][E + h * dh + d] / [2E + h * dh + d] for b < B,
 *     p < C, d < dh.  Nothing else is written (positions >= C, pad columns d >= dh, rows >= B keep their content).  qkv is read in place,
 *     16 bytes at a time where dh, ld and the addresses allow.  Errors: null qkv, layer outside [0, L), C outside [1, max_len - 1],
 *     ld < 3E.
 *   acai_decode_prefill_arm once: seqs[b][0] = <bos>, seqs[b][1 .. C] = tok[b][1 .. C], logprobs[b][j + 1] = (logit[token] - max) -
 *     logf(sum expf(logit - max)) with acai_decode_prompt_step's reduction and rounding, finished[b] = (tok[b][C] == <eos>), finished[B] =
 *     the count acai_decode_prompt_step leaves at t = C (a row with C < len[b] is unfinished), step = {C + 1, C}, x[b] =
 *     vocab_embedding[tok[b][C]] + pos_embedding[C + 1] when C + 1 < Tmax: the state C calls of acai_decode_prompt_step leave, the
 *     log-probs up to the difference between the pass's logits and the steps'.  acai_decode_prompt_step goes on from t = C + 1.  The
 *     caller keeps every tok[b][1 .. C] inside [0, V) and C <= len[b]: an entry that is not falls back to that position's own arg-max
 *     (memory-safe, but not what the steps would have done - there the later positions would have seen the arg-max).  Errors: null
 *     prompt tables or logits, C outside [1, max_len - 1], prompt->rows < B, prompt->pitch < max_len, V > 512.
 * Both enqueue one kernel (capturable) and launch nothing when they return an error. */
int acai_decode_prefill_self_kv(const AcaiDecoder *d, int layer, const void *qkv, int ld, int C, void *stream);
int acai_decode_prefill_arm(const AcaiDecoder *d, const AcaiPrompt *prompt, const float *logits, int C, void *stream);
/* Grammar-constrained decoding (an extension: the reference knows no grammar).  A token automaton is a table next[state][token]: an entry
 * >= 0 is the state after emitting that token, an entry < 0 forbids the token in that state.  All arrays are device memory:
 *   next:   [states][V] int16, every non-negative entry < states;
 *   resync: [V] int16 in [0, states): the state taken after a token the table did not allow (here: out of a state that allows none);
 *   state:  [rows] int32, the state of every decode row; the caller arms it to `start` before the first step (slot mode: when it arms the
 *           slot), ordered before the step; the steps advance it.  A value outside [0, states) is clamped where it is read.
 * There is no accept set: a row may end in state s exactly when next[s][<eos>] >= 0. */
typedef struct {
    const int16_t *next;
    const int16_t *resync;
    int32_t *state;
    int32_t states;    /* 1 .. 32767 */
    int32_t start;     /* the state after <bos>, in [0, states); also taken after a token outside [0, V) */
    int32_t rows;      /* entries of state, >= dec->B */
    int32_t pad_;
} AcaiGrammar;
/* One CONSTRAINED greedy step: acai_decode_step's layers and unembed, then one selection launch in which row b reads its state
 * s = clamp(state[b], 0, states - 1) and the table row next[s][:]; a token i with next[s][i] < 0 counts as a -inf logit in the arg-max (first
 * index on ties) and in the sum of exponentials, so logprobs[b][t] is the log-softmax over the ALLOWED tokens (the policy actually run) and
 * state[b] = next[s][token].  If s allows no token the row is unconstrained at this step and state[b] = resync[token] (a defensive path).
 * seqs, finished[], finished[B], step[], the bf16 rounding of the log-prob and the next input x are acai_decode_step's; a finished row goes on
 * emitting (masked) tokens as it does there.  With a table that allows every token the step is acai_decode_step bit for bit.  Same checks
 * and x contract as acai_decode_step, plus non-null next / resync / state, 1 <= states <= 32767, 0 <= start < states, rows >= B, V <= 512.
 * Enqueues kernels only (capturable). */
int acai_decode_grammar_step(const AcaiDecoder *d, const AcaiGrammar *g, void *stream);
/* One CONSTRAINED sampling step: acai_decode_sample_step whose top-k rounds, draw and log_softmax(kept) run over the allowed tokens of the
 * row's state only; with fewer than top_k allowed tokens the kept set is the allowed set (one allowed token is drawn with log-prob 0 whatever
 * u is).  State handling and checks as acai_decode_grammar_step, plus acai_decode_sample_step's. */
int acai_decode_grammar_sample_step(const AcaiDecoder *d, const AcaiGrammar *g, const float *uniforms, int top_k, float temperature, void *stream);
/* The SLOT-MODE forms: acai_decode_slot_step / acai_decode_slot_sample_step with the constrained token choice.  A finished or idle row
 * reads and writes neither its tokens nor its state; the caller sets state[b] = start when it arms slot b (before acai_decode_slot_arm's
 * step).  Checks: the slot step's and acai_decode_grammar_step's. */
int acai_decode_slot_grammar_step(const AcaiDecoder *d, const AcaiSlots *sl, const AcaiGrammar *g, void *stream);
int acai_decode_slot_grammar_sample_step(const AcaiDecoder *d, const AcaiSlots *sl, const AcaiGrammar *g, const float *uniforms, int ld_uniforms,
                                         const int32_t *urow, int top_k, float temperature, void *stream);
/* Walks R finished token rows through a token automaton (grammar.hip): the inputs of the GRPO well-formedness reward.  tokens [R][ld] int64
 * (row stride = ld), lens [R] int32, read ON THE DEVICE and clamped to [0, ld]; next [states][V] / resync [V] int16 as in AcaiGrammar.  Row r
 * starts in s = start (index 0 is <bos> and is not checked); for p = 1 .. len - 1 with k = tokens[r][p]: k outside [0, V) is one violation
 * and s = start; next[s][k] < 0 is one violation and s = resync[k]; otherwise s = next[s][k].  violations[r] (int32) receives the count,
 * complete[r] (int32) is 1 iff len >= 2, the last token is `eos` and its transition was allowed.  Rows run in parallel, each is a serial
 * chain; the table is staged in LDS when states * V * 2 bytes fit 156 KB (a bigram automaton at V = 227 is 103 KB) and read from global
 * memory otherwise.  One launch, no host synchronisation, no allocation (capturable).  1 <= states <= 32767, 0 <= start < states, V >= 1. */
int acai_grammar_scan(const int64_t *tokens, int ld, const int32_t *lens, int R, const int16_t *next, const int16_t *resync, int states, int start,
                      int V, int eos, int32_t *violations, int32_t *complete, void *stream);
/* The loop guard (an extension: the reference lets a row that fell into a repeat cycle run to its cap).  One rule for the steps below,
 * acai_repeat_scan and the tests.  With P = max_period, R = min_repeats, M = min_tokens and need(p) = max((R - 1) p, M): index 0 is <bos> and
 * never takes part; run_p(t) is the number of consecutive indices i ending at t with seq[i] == seq[i - p] and i - p >= 1.  A row fires at
 * the first t at which some p in 1 .. P has run_p(t) >= need(p); the smallest such p wins.  The report is stop = t, period = p and
 * start = t - need(p) - p + 1, the first index of the periodic stretch; a row that never fires keeps period = 0.  All arrays are device memory:
 *   run:                  [rows][64] int32, run_p of row b in run[b][p - 1]; entries at and past P hold 0;
 *   stop, period, start:  [rows] int32, the report.
 * The caller zeroes a row's 64 counters and three report words before the row's first step (slot mode: when it arms the slot). */
typedef struct {
    int32_t *run;
    int32_t *stop;
    int32_t *period;
    int32_t *start;
    int32_t rows;          /* rows of the four arrays, >= dec->B */
    int32_t max_period;    /* P, 1 .. 64 */
    int32_t min_repeats;   /* R >= 2 */
    int32_t min_tokens;    /* M >= 1 */
} AcaiLoop;
/* One GUARDED greedy step: acai_decode_step, whose selection launch also applies the rule to every unfinished row - the wave that chose
 * the row's token compares it with the row's tokens 1 .. P indices back and updates run[b][] (O(1) a step; the row is not scanned).  A row
 * that fires keeps the token at t, gets finished[b] = 1 and leaves the unfinished count; no <eos> is written, and the row goes on emitting
 * like any finished row.  If the token at t is <eos> the row ends as acai_decode_step ends it and no report is written.  A finished row is
 * not examined and its counters stand.  With a guard that cannot fire the step is acai_decode_step bit for bit.  Same checks and x contract
 * as acai_decode_step, plus non-null run / stop / period / start, rows >= B, 1 <= max_period <= 64, min_repeats >= 2, min_tokens >= 1.
 * Enqueues kernels only (capturable); no launch is added to acai_decode_step's. */
int acai_decode_loop_step(const AcaiDecoder *d, const AcaiLoop *loop, void *stream);
/* The SLOT-MODE form: acai_decode_slot_step in which a row also finishes when it fires - finished = <eos> or cap or loop, and t[b] is left
 * at the row's last token as for a cap.  A finished or idle row reads and writes nothing of the guard's.  Checks: the slot step's and
 * acai_decode_loop_step's. */
int acai_decode_slot_loop_step(const AcaiDecoder *d, const AcaiSlots *sl, const AcaiLoop *loop, void *stream);
/* TEST ENTRY (tests/test_gpu_loop_select.py): ONE selection launch of acai_decode_loop_step (slot == 0) or acai_decode_slot_loop_step
 * (slot != 0; sl as acai_debug_decode_select's slot forms take it) on logits the caller wrote, with acai_debug_decode_select's contract for
 * the descriptor, `chained` and the preconditions.  Refused (rc < 0, nothing launched): a null decoder, logits, step, finished, seqs or
 * logprobs; B, V, E or Tmax < 1 or max_len < 2; chained with a null emb / pos / x or E % 4 != 0; slot with chained == 0, null t / cap,
 * rows < B or max_len > Tmax; and what acai_decode_loop_step refuses of `loop`. */
int acai_debug_decode_loop_select(int slot, const AcaiDecoder *d, const AcaiSlots *sl, const AcaiLoop *loop, int chained, void *stream);
/* The same rule over N finished token rows (loops.hip): rows from any decode mode, and metrics.  tokens [N][ld] int64 (row stride = ld);
 * lens [N] int32, read ON THE DEVICE and clamped to [0, ld], or NULL for rows of ld tokens.  One wave per row sweeps t forward with the
 * counters in registers.  Row n gets stop[n], period[n], start[n] of its first firing and end[n], the last index below its length up to
 * which seq[i] == seq[i - period] keeps holding from stop on; a row that never fires gets four zeros.  An <eos> is a token like any other
 * here: bound a row by lens to leave it out.  One launch, no host synchronisation, no allocation (capturable). */
int acai_repeat_scan(const int64_t *tokens, const int32_t *lens, int N, int ld, int max_period, int min_repeats, int min_tokens, int32_t *stop,
                     int32_t *period, int32_t *start, int32_t *end, void *stream);
/* The same without the token bookkeeping: logits for caller-supplied tokens/time_step (OMRDecoder.cached_generate). */
int acai_decode_logits(const AcaiDecoder *dec, const int64_t *tokens, int time_step, void *stream);

/* CachedTransformerDecoder.cached_generate (K:292-302): x_in [B,E] fp32 is this step's embedding; the hidden state after
 * the L cached layers and the optional final norm lands in dec->xn.  emb / pos / unembed may be NULL for this call. */
int acai_decode_hidden(const AcaiDecoder *dec, const float *x_in, void *stream);

/* 1 when a decode step with `dec->tickets` set merges the split partials of its attention launches inside those launches (last-arriver
 * hand-off), 0 when it takes the separate combine launch instead (tickets ignored: the hand-off is used only at the workgroup residency it
 * was validated at, or as ACAI_DATTN_MERGE forces), negative for a bad argument.  Same arithmetic either way (kv_caching.py:131 - the SDPA
 * of a cached step); bench.py reports it so that a silent change of path shows in the headline line. */
int acai_decode_merge_in_launch(int dtype, int dhp);

/* F.linear on a (B,1,K) activation (K:193,215; nn.Linear inside cached_forward K:139,222): y[B,N] = x[B,K].W[N,K]^T
 * + bias (+GELU) (+residual); x, y, bias, residual fp32, W in `dtype` (bf16: x is rounded to bf16 first, as autocast does). */
int acai_skinny_gemm(const float *x, int ldx, const void *W, int ldw, const float *bias, const float *residual, int ldr,
                     float *y, int ldy, int B, int N, int K, int dtype, int flags, void *stream);

/* acai_skinny_gemm with the fusions the decode step uses (bf16 weights, K % 256 == 0): x may be bf16 (x_dtype), y may be bf16;
 * ln_w/ln_b: x := LayerNorm(x) on load (norm1/2/3 of the post-LN layer, K:208,220,222), its per-row (mean, rstd) optionally
 * published to stats_out[B][2] (fp32 x only: refused for bf16 x); rln_w/rln_b/rstats: residual := LayerNorm(residual) from published
 * statistics. */
int acai_skinny_gemm_ex(const void *x, int ldx, int x_dtype, const void *W, int ldw, const float *bias, const float *residual, int ldr,
                        void *y, int ldy, int y_dtype, int B, int N, int K, int dtype, int flags, const float *ln_w, const float *ln_b,
                        float ln_eps, float *stats_out, const float *rln_w, const float *rln_b, const float *rstats, void *stream);

/* CachedMultiheadAttention.cached_forward's SDPA (K:131-136) for one query per sequence:
 * keys/values of sequence b, head h at kc/vc + seq_off[b] + (h*seq_len[b] + s)*dhp; out[b, h*dh + d] fp32.
 * partial: workspace of B*H*nsplit*(dhp+2) floats; chunk*nsplit must cover max(seq_len).
 * out == NULL stops after the split partials (m, l, o[dhp]) - the streaming kernel alone, for benchmarking.
 * tickets: NULL = a second launch merges the splits; else B*H zeroed counters: the last-arriving workgroup of each (b,h)
 * merges them inside the launch (agent-scope release / acquire hand-off) and re-zeroes its counter. */
int acai_decode_attn(const float *q, int ldq, const void *kc, const void *vc, const int64_t *seq_off, const int32_t *seq_len,
                     float *partial, float *out, int ldo, int B, int H, int dh, int dhp, int chunk, int nsplit, int dtype,
                     int round_out, uint32_t *tickets, void *stream);
/* The same over an FP8 (ACAI_FP8_E4M3) cache: element (b, h, s, d) is kc[seq_off[b] + (h*seq_len[b] + s)*dhp + d] * k_scale[row], row =
 * (seq_off[b] + (h*seq_len[b] + s)*dhp) / dhp (likewise V); dhp 16, 32 or 64. */
int acai_decode_attn_fp8(const float *q, int ldq, const void *kc, const void *vc, const float *k_scale, const float *v_scale,
                         const int64_t *seq_off, const int32_t *seq_len, float *partial, float *out, int ldo, int B, int H, int dh,
                         int dhp, int chunk, int nsplit, int round_out, uint32_t *tickets, void *stream);

/* TEST ENTRY (tests/test_gpu_decode_self_attn.py): the self-attention forms of a decode step on caller-supplied operands.  It exists for
 * tests and launches exactly the step's kernels: it fills the kernel's arguments as the step does for its self attention and goes through the
 * step's own dispatch.  form: 0 plain, 1 ancestor table (beam step), 2 ring (slot step), 3 key table (speculative verify step).
 *   q [B][ldq] fp32, head h at column h*dh (any alignment, any ldq); k_cache / v_cache [rows][H][Tmax][dhp] in `dtype` (ACAI_F32 / ACAI_BF16).
 *   Key p of row b, and the row's key count `len`:
 *     0  k_cache[b][h][p];                                         len = step[1] + 1
 *     1  k_cache[table[(step[0] & 1) * table_stride + b * table_pitch + p]][h][p];   len = step[1] + 1
 *        (table: the two parity copies of [rows][table_pitch] int32, table_stride = rows * table_pitch, table_pitch >= Tmax)
 *     2  k_cache[b][h][(table[b] + p) % Tmax] (table[b] in [0, Tmax));   len = row_len[b] in [1, Tmax]
 *     3  R = table_stride rows per image (1 .. 8, B % R == 0), i = b / R: e = table[i * table_pitch + p] names cache row i * R + (e & 7),
 *        position e >> 3 (both clamped into the image's rows and the cache);   len = max(1, min(row_len[i] + b % R, table_pitch, chunk * nsplit))
 *   partial: B*H*nsplit*(dhp+2) floats; chunk * nsplit >= Tmax; forms 1 and 3 stage chunk table entries in LDS: chunk <= 16384.
 *   out [B][ldo]: written by the attention launch itself when nsplit == 1 or `tickets` (B*H zeroed counters, re-zeroed by the launch) is
 *   given, else by the separate combine launch; NULL stops after the partials.  round_out: values rounded to bf16.  out_bf16 (only where the
 *   attention launch writes out): out holds bf16 rows, ldo in bf16 elements.  A refused call launches nothing. */
int acai_debug_decode_self_attn(int form, const float *q, int ldq, const void *k_cache, const void *v_cache, const int32_t *step,
                                const int32_t *row_len, const int32_t *table, int table_pitch, int64_t table_stride, float *partial, void *out,
                                int ldo, int B, int H, int dh, int dhp, int Tmax, int chunk, int nsplit, int dtype, int round_out, int out_bf16,
                                uint32_t *tickets, void *stream);
/* TEST ENTRY: acai_decode_attn's operands through the matrix-core rollout-group kernel, launched exactly as a step with cross_group > 1
 * launches it: rows b = i*group .. i*group + group - 1 share the ragged K/V of seq_off / seq_len[i*group] (the arrays keep one entry per
 * row).  bf16 and dhp == 64 only, B % group == 0, out required; nsplit > 1 needs tickets (the kernel merges inside the launch only; one
 * counter per (first row of a 16-row tile, head), B*H zeroed counters cover them). */
int acai_debug_decode_attn_group(const float *q, int ldq, const void *kc, const void *vc, const int64_t *seq_off, const int32_t *seq_len,
                                 float *partial, float *out, int ldo, int B, int H, int dh, int dhp, int chunk, int nsplit, int dtype,
                                 int round_out, uint32_t *tickets, int group, void *stream);
/* TEST ENTRY (tests/test_gpu_select_kernels.py): ONE token-selection launch of a decode step on logits the caller wrote into dec->logits.  It
 * exists for tests and calls exactly the launch helper the step of that form calls after its layers; no layer runs, and the descriptor need
 * hold only what selection reads: logits, V, B, max_len, Tmax, E, eos, bos, pad, flags (ACAI_GEMM_ROUND_BF16: log-probs rounded to bf16),
 * seqs, logprobs, step, finished, emb, pos, x, tickets.  Every other field is ignored (layers may be NULL).  form:
 *   ACAI_SELECT_ARGMAX               acai_decode_step's selection              ACAI_SELECT_SAMPLE               acai_decode_sample_step's
 *   ACAI_SELECT_PROMPT               acai_decode_prompt_step's (prompt)        ACAI_SELECT_GRAMMAR_SAMPLE       acai_decode_grammar_sample_step's
 *   ACAI_SELECT_GRAMMAR_ARGMAX       acai_decode_grammar_step's (g)            ACAI_SELECT_SLOT_SAMPLE          acai_decode_slot_sample_step's
 *   ACAI_SELECT_SLOT_ARGMAX          acai_decode_slot_step's (sl)              ACAI_SELECT_SLOT_GRAMMAR_SAMPLE  acai_decode_slot_grammar_sample_step's
 *   ACAI_SELECT_SLOT_GRAMMAR_ARGMAX  acai_decode_slot_grammar_step's (sl, g)   ACAI_SELECT_BEAM                 acai_decode_beam_step's (bs)
 * What each writes is what its step documents above.  sl / g / prompt / bs are read by the forms that name them and may be NULL otherwise
 * (AcaiSlots.first is not read).  The draw (sampled forms): uniforms, top_k, temperature as in acai_decode_sample_step; a static form reads
 * uniforms[b * max_len + t] and ignores ld_uniforms / urow, a slot form reads uniforms[urow[b] * ld_uniforms + t[b]].  chained != 0: the launch
 * also writes the next step's input x (what a step does when E % 4 == 0); the slot and beam forms always do and refuse chained == 0.
 * PRECONDITIONS the entry cannot check, as for the steps: the time index read on the device (step[0], a slot's t[b]) lies inside the rows
 * (< max_len, < pitch), and every live row has at least one finite logit among the tokens it may choose (decode selection).
 * Refused (rc < 0, acai_last_error() names acai_debug_decode_select, nothing launched): a form outside [0, 9]; a null decoder or a null
 * logits / step / finished (seqs / logprobs but for the beam form); B, V, E or Tmax < 1 or max_len < 2; chained with a null emb / pos / x or
 * E % 4 != 0; a slot form with null t / cap, rows < B or max_len > Tmax; a grammar form with null next / resync / state, states outside
 * [1, 32767], start outside [0, states) or rows < B; the prompt form with null tok / len, pitch < max_len or rows < B; a sampled form with null
 * uniforms, (slot) null urow or ld_uniforms < max_len, top_k outside [1, 64], temperature <= 0 or V > 512; the beam form with a null beam
 * array, K outside [1, 16] or not dividing B, rows < B, pitch < max_len or V > 512.  The greedy forms take any V. */
#define ACAI_SELECT_ARGMAX 0
#define ACAI_SELECT_PROMPT 1
#define ACAI_SELECT_GRAMMAR_ARGMAX 2
#define ACAI_SELECT_SLOT_ARGMAX 3
#define ACAI_SELECT_SLOT_GRAMMAR_ARGMAX 4
#define ACAI_SELECT_SAMPLE 5
#define ACAI_SELECT_GRAMMAR_SAMPLE 6
#define ACAI_SELECT_SLOT_SAMPLE 7
#define ACAI_SELECT_SLOT_GRAMMAR_SAMPLE 8
#define ACAI_SELECT_BEAM 9
int acai_debug_decode_select(int form, const AcaiDecoder *d, const AcaiSlots *sl, const AcaiGrammar *g, const AcaiPrompt *prompt,
                             const AcaiBeam *bs, const float *uniforms, int ld_uniforms, const int32_t *urow, int top_k, float temperature,
                             int chained, void *stream);
/* TEST ENTRY (tests/test_gpu_spec_accept.py): the ONE launch that closes every step of acai_decode_spec_arm / _spec_step / _spec_prompt_arm /
 * _spec_prompt_step, on the state and the logits the caller wrote.  It exists for tests and goes through the helper those steps call - the
 * unprompted launch when prompt is NULL, the prompted one otherwise - with `arm` passed through (arm != 0: the launch of the _arm entry points,
 * which reads no logits and writes no token; arm == 0: the launch after a verify step's layers).  No layer runs, and the descriptor need
 * hold only what this launch reads: logits (arm == 0), V, B, max_len, Tmax, E, eos, pad, flags (ACAI_GEMM_ROUND_BF16), seqs, logprobs, step,
 * finished, emb, pos, x; sp and prompt as the steps take them.  cross_group, the layers, the unembed and the x-valid contract are not
 * looked at.  What it writes is what AcaiSpec and the four entry points document above: per image the accepted tokens and log-probs,
 * t, steps, finished[i]; for every image that is unfinished afterwards next[i][0 .. D], tab[i][t' - 1 .. t' - 1 + D] (indices below pitch)
 * and x of its D + 1 rows (any E >= 1); finished[B]; step[1] unless arm.  An image whose flag is already set has nothing of it written; one
 * whose t lies outside [1, cap - 1] only gets its flag set; one that finishes in this launch gets no next / tab / x.
 * PRECONDITIONS the entry cannot check, as for acai_debug_decode_select: every row of a live image has at least one finite logit and no NaN;
 * the time indices read on the device (t[], step[1]) are the caller's to keep inside the rows (t and cap are clamped as stated, step[1] is
 * clamped to Tmax - 1 where it is used).
 * Refused (rc < 0, acai_last_error() names acai_debug_decode_spec_accept, nothing launched): a null decoder; a null seqs, logprobs, step,
 * finished, emb, pos or x; null logits unless arm; B, V or E < 1; max_len outside [2, Tmax]; a null sp or a null t, cap, steps, tab or
 * next; D outside [1, 7]; B % (D + 1) != 0; rows < B / (D + 1); pitch outside [max_len, Tmax]; ngram outside [1, 8] unless drafts is given;
 * with a prompt: null tok / len, prompt pitch < max_len or prompt rows < B / (D + 1). */
int acai_debug_decode_spec_accept(const AcaiDecoder *d, const AcaiSpec *sp, const AcaiPrompt *prompt, int arm, void *stream);

/* FP8 memory cache prefill: rows row0 .. row0+nrows-1 (dhp = 16, 32 or 64 elements each, at element offset row*dhp) of the bf16 cross K/V
 * written by acai_cross_kv_prefill -> the same rows of k_out / v_out in OCP e4m3fn, and k_scale[row] / v_scale[row].  The scale is 2^e,
 * e the smallest integer with amax(row) 2^-e <= 448 (at least -126; 0 for an all-zero row); q = round-to-nearest-even(x 2^-e).
 * All four row buffers 16-byte aligned. */
int acai_cross_kv_quantize_fp8(const void *k_in, const void *v_in, void *k_out, void *v_out, float *k_scale, float *v_scale,
                               int64_t row0, int64_t nrows, int dhp, void *stream);

/* ---- camera augmentation of the training input pipeline -------------------------------------------------------------------------------
 * `v2.RandomApply([GaussianBlur(15, sigma), GaussianNoise(sigma), RandomRotation(degrees, BILINEAR), RandomPerspective(scale, p=1),
 * ColorJitter(brightness, saturation, contrast, hue=0)], p=AUGMENTATION_P)` and the GrandStaff pair (perspective + jitter) of
 * acai_omr/train/pre_train.py:178-190, omr_teacher_force_train.py:320-331, omr_grpo_train.py:530-541, on one-channel fp32 images in [0, 1].
 * The three entry points below are batched over a RAGGED list of images through a read-only table of AcaiAugImage in device memory: one
 * launch covers every image (grid z = image, blocks beyond an image's H x W leave at once), so the launches of a call do not grow with the
 * number of images.  Slots: -1 = the image's `src`, 0 / 1 = its two H x W scratch buffers `buf`; a stage reads one slot and writes another.
 * An image whose `apply` is 0 is skipped by every stage and copied from `src`, bit for bit, by the last one.  All random draws are made
 * by the caller and arrive in the table. */
#define ACAI_AUG_MAX_TAPS 32
#define ACAI_AUG_MEAN_PARTS 128
#define ACAI_AUG_BRIGHTNESS 1       /* AcaiAugImage.jitter: brightness is applied */
#define ACAI_AUG_CONTRAST 2         /* contrast is applied */
#define ACAI_AUG_BRIGHTNESS_FIRST 4 /* brightness before contrast (the only observable part of ColorJitter's random order) */
typedef struct AcaiAugImage {
    const float *src;    /* H x W input, never written */
    float *buf[2];       /* H x W scratch each */
    const float *noise;  /* H x W standard-normal draws (NULL: no noise and no clamp for this image) */
    float *out;          /* H x W result of the image form (NULL in the patch form) */
    double *partials;    /* ACAI_AUG_MEAN_PARTS partial sums of the contrast mean */
    double rot_cos, rot_sin; /* cos / sin of the rotation angle */
    double persp[8];     /* perspective coefficients c0 .. c7 */
    int32_t H, W, apply, jitter;
    int32_t ktaps, row0; /* blur taps (odd, <= ACAI_AUG_MAX_TAPS; 1 with w[0] = 1 is the identity); first patch row of the patch form */
    float noise_sigma, fb, fc, pad_;
    float w[ACAI_AUG_MAX_TAPS]; /* blur weights, softmax(-(x / sigma)^2) over linspace(-lim, lim, ktaps) */
} AcaiAugImage;

/* GaussianBlur + GaussianNoise: separable convolution with `w` over the image reflect-padded by ktaps / 2 (F.pad(mode="reflect"): H and W
 * must exceed ktaps / 2), rows first (in_slot -> tmp_slot), then columns (tmp_slot -> out_slot), and with do_noise
 * clamp(blurred + noise_sigma * noise, 0, 1) in the column pass.  do_blur = 0: the column pass alone, in_slot -> out_slot (ktaps must be 1). */
int acai_augment_blur_noise(const AcaiAugImage *table, int n_images, int max_h, int max_w, int in_slot, int tmp_slot, int out_slot,
                            int do_blur, int do_noise, void *stream);
/* RandomRotation (perspective = 0) or RandomPerspective (perspective = 1), in_slot -> out_slot: F.grid_sample(bilinear, zeros,
 * align_corners=False) of the image and of an all-ones mask, multiplied (torchvision's fill path with fill = 0).  Output pixel (x, y) samples
 *   rotation:    (cos xc - sin yc + W/2 - 0.5, sin xc + cos yc + H/2 - 0.5), xc = x + 0.5 - W/2, yc = y + 0.5 - H/2
 *   perspective: ((c0 X + c1 Y + c2) / d - 0.5, (c3 X + c4 Y + c5) / d - 0.5), X = x + 0.5, Y = y + 0.5, d = c6 X + c7 Y + 1
 * with the coordinates evaluated in fp64 and the interpolation in fp32. */
int acai_augment_warp(const AcaiAugImage *table, int n_images, int max_h, int max_w, int in_slot, int out_slot, int perspective, void *stream);
/* ColorJitter on one channel + the output stage: brightness clamp(v fb, 0, 1), contrast clamp(fc v + (1 - fc) mean, 0, 1) with the mean
 * of the whole image as it is when contrast is applied (partial sums in a fixed order, no atomics: bit-reproducible), in the order
 * `jitter` gives; saturation does nothing on one channel.  do_jitter = 0: output only.  patches == NULL: every image is written to its `out`;
 * otherwise its nn.Unfold(P, stride P) rows go to rows row0 .. of `patches` [rows][ld >= P*P] in out_dtype (fp32 / bf16) as
 * acai_resize_to_patches orders them (H and W multiples of P). */
int acai_augment_jitter_out(const AcaiAugImage *table, int n_images, int max_h, int max_w, int in_slot, int do_jitter, void *patches,
                            int ld, int P, int out_dtype, void *stream);

/* ---- whole pages: find the staff systems, cut them out, resize them into the patch stream ----------------------------------------------
 * The reference's service takes a page and hand-drawn boxes, crops each with PIL and transforms and decodes the crops one by one
 * (acai_omr/ui/routes.py:93-129, `setup_inference` / `multiple_img_stream_inference_wrapper`).  The three entry points below are the device
 * side of doing that for all systems of all pages at once, and of finding the boxes when none are drawn (an extension: the reference has no
 * detector; its tests import a `SystemDetectionDataset` that was never written).  A page is one channel, fp32 in [0, 1] or uint8 (in_u8 = 1,
 * read as (float)p / 255 like acai_resize_to_patches), [H][pitch] with pitch >= W in elements.  Integer outputs are exact and do not depend
 * on the launch order: no atomics. */
#define ACAI_PAGE_LANE_PIXELS 4   /* acai_page_profile: consecutive pixels per lane, 64 lanes = 256 pixels per wave step ... */
#define ACAI_PAGE_WAVES 4         /* ... and each of a row's 4 waves owns one contiguous span of ceil(ceil(W / 4) / 256) * 256 pixels */
#define ACAI_PAGE_MAX_W 16384
#define ACAI_PAGE_MAX_H 65535

/* Row profiles: ink[y] = number of pixels of row y with value < ink_threshold, run[y] = the longest run of consecutive such pixels
 * (staff lines are the long runs).  One workgroup per row; W <= ACAI_PAGE_MAX_W, H <= ACAI_PAGE_MAX_H. */
int acai_page_profile(const void *page, int in_u8, int H, int W, int pitch, float ink_threshold, int32_t *ink, int32_t *run, void *stream);

/* The profiles -> system boxes, in two launches with no host step between them.  A row is inked if ink[y] >= min_ink (>= 1).  A band is a
 * maximal set of inked rows in which consecutive inked rows are separated by at most merge_gap other rows, [y0, y1) from its first inked
 * row to one past its last.  It is kept if y1 - y0 >= min_height and at least min_line_rows of its rows have run[y] >= line_len.  Of a
 * kept band, x0 / x1 are the leftmost / one past the rightmost column with a pixel < ink_threshold in rows [y0, y1) (a second read of the
 * page, of the kept bands only), and its box is (max(x0 - margin, 0), max(y0 - margin, 0), min(x1 + margin, W), min(y1 + margin, H)).
 * count[0] = the number of kept bands (may exceed max_systems); boxes [max_systems][4] = the first max_systems of them, top to bottom;
 * rows of `boxes` from min(count, max_systems) on are not written. */
int acai_page_systems(const void *page, int in_u8, int H, int W, int pitch, float ink_threshold, const int32_t *ink, const int32_t *run,
                      int min_ink, int merge_gap, int min_height, int line_len, int min_line_rows, int margin, int max_systems,
                      int32_t *count, int32_t *boxes, void *stream);

/* One box to cut, resize and pack (acai_crop_resize_to_patches). */
typedef struct AcaiCropResize {
    const void *page;       /* the page the box lies in, [page_h][pitch] */
    int64_t tmp_off;        /* where this entry's h x OW width-pass samples start in `tmp`, in floats */
    int32_t page_h, page_w; /* only read on the host (the box must lie inside the page) */
    int32_t pitch, in_u8;
    int32_t x0, y0, w, h;   /* the source box */
    int32_t OH, OW;         /* the size the box is resized to */
    int32_t top, left, ch, cw; /* the window of the OH x OW result that is kept (multiples of P) */
    int32_t row0, pad_;     /* first row of the patch stream */
} AcaiCropResize;

/* acai_resize_to_patches over a table of n boxes, each cut from its own page, in TWO launches whatever n is: the width pass of every box
 * into `tmp`, then the height pass of every box into its rows of `patches` [patch_rows][ld >= P*P] (nn.Unfold order, out_dtype, clamp01).
 * "Crop, then resize": a sample's taps are clamped to the BOX, so entry e gets, bit for bit, what acai_resize_to_patches writes for the
 * contiguous copy of page[y0 : y0 + h, x0 : x0 + w] (the same window, weights and accumulation order: csrc/resize_taps.h).
 * `table` is the device copy the kernels read; `host_table` holds the same n entries in host memory and is what is checked here: boxes
 * inside their pages, windows inside (OH, OW) and multiples of P, rows inside `patches`, samples inside `tmp` (tmp_elems floats), and
 * n, max h and max OH are grid dimensions (<= 65535). */
int acai_crop_resize_to_patches(const AcaiCropResize *table, const AcaiCropResize *host_table, int n, float *tmp, int64_t tmp_elems,
                                void *patches, int ld, int64_t patch_rows, int P, int out_dtype, int clamp01, void *stream);

/* ---- page deskew: estimate the skew of a page and turn it level (csrc/deskew.hip) ---------------------------------------------------------
 * The detection rule of acai_page_systems needs level staff lines; a photographed page is not level.  A page is as acai_page_profile takes
 * it (uint8 or fp32, pitch >= W, the same ink test in_sample(p) < ink_threshold, the same size limits).  Everything below is defined in
 * integers, fp32 rotation aside, and the results do not depend on how the launches are scheduled.  Shifts are arithmetic. */
#define ACAI_STRIP_TILE_ROWS 64    /* acai_page_strips: a workgroup owns 64 rows x 32 units of 16 bytes (16 uint8 or 4 fp32 pixels) ... */
#define ACAI_STRIP_TILE_UNITS 32   /* ... one unit per lane and step; a strip is a whole number of units or, uint8 at S = 8, half a unit */
#define ACAI_SKEW_CHUNK 1023       /* acai_page_skew_scores: row differences per workgroup (256 threads x 4 rows, the last row is the halo) */
#define ACAI_SKEW_MAX_SLOPES 1024
#define ACAI_SKEW_MAX_SLOPE 17560  /* round(tan(15 deg) * 65536) */

/* Strip profile.  The page is cut into vertical strips of S columns, S in {8, 16, 32, 64}, nS = ceil(W / S); strips[s][y] = the number of
 * ink pixels of row y in columns [s S, min((s + 1) S, W)).  Columns behind W (the pitch padding) never count.  LAYOUT: uint8 [nS][H] (a
 * count is at most 64) - the rows of one strip are contiguous, which is the direction acai_page_skew_scores walks.  One read of the page,
 * 16 bytes per lane where base and pitch are multiples of 16 bytes, element by element where not. */
int acai_page_strips(const void *page, int in_u8, int H, int W, int pitch, float ink_threshold, int S, uint8_t *strips, void *stream);

/* Skew scores of K candidate slopes m_k in Q16 (m = round(tan(angle) * 65536), |m| <= ACAI_SKEW_MAX_SLOPE, 1 <= K <= ACAI_SKEW_MAX_SLOPES):
 *   dx(s) = s S + S / 2 - W / 2 (integer divisions),  off(s, k) = (m_k dx(s) + 32768) >> 16,
 *   Q_k[y] = sum over s of strips[s][y + off(s, k)], rows outside [0, H) contributing 0,
 *   scores[k] = sum over y in [0, H - 2] of (Q_k[y + 1] - Q_k[y])^2 in 64 bits (H = 1: 0).
 * `strips` is what acai_page_strips wrote for the same H, W, S.  `slopes` is the device copy of the table, `host_slopes` the same K values
 * in host memory (what is checked here).  scores [K] is zeroed on the stream, then ONE launch over (slope, chunk of ACAI_SKEW_CHUNK row
 * differences) adds one 64-bit integer atomic per workgroup: integer sums, so the result is the same whatever the order. */
int acai_page_skew_scores(const uint8_t *strips, int H, int W, int S, const int32_t *slopes, const int32_t *host_slopes, int K, int64_t *scores,
                          void *stream);

/* The page turned about its centre by the angle with cos_q = round(cos * 65536), sin_q = round(sin * 65536): a positive angle turns what is
 * displayed counter-clockwise.  Output pixel (x, y) of `out` [H][out_pitch >= W] (the input's element type, not in place) is sampled at,
 * in 64-bit integers with dx2 = 2 x - (W - 1), dy2 = 2 y - (H - 1),
 *   sx = (cos_q dx2 - sin_q dy2 + (W - 1) 65536) >> 1,   sy = (sin_q dx2 + cos_q dy2 + (H - 1) 65536) >> 1,
 *   ix = sx >> 16, iy = sy >> 16, fx = (sx >> 8) & 255, fy = (sy >> 8) & 255,
 * bilinear over the taps t00 = (iy, ix), t01 = (iy, ix + 1), t10 = (iy + 1, ix), t11 = (iy + 1, ix + 1); a tap outside the page reads
 * `fill` (uint8: an integer in 0 .. 255).  uint8: ((256 - fy) ((256 - fx) t00 + fx t01) + fy ((256 - fx) t10 + fx t11) + 32768) >> 16, so
 * angle 0 is the identity and (cos_q, sin_q) = (0, 65536) a quarter turn of a square page.  fp32: the same weights f / 256 in fp32.
 * A lane makes 4 consecutive pixels and stores them as one word where `out` and out_pitch are multiples of it (4 bytes; fp32: 16). */
int acai_page_rotate(const void *page, int in_u8, int H, int W, int pitch, int cos_q, int sin_q, float fill, void *out, int out_pitch, void *stream);

/* ---- page illumination flattening: estimate the paper's brightness locally and divide it out (csrc/flatten.hip) ---------------------------
 * Every page stage above tells ink from paper by one global threshold; a photographed page is not evenly lit.  A page is as
 * acai_page_profile takes it (uint8 or fp32 in [0, 1], pitch >= W, the same size limits).  Everything is defined in integers, so no result
 * depends on how the launches are scheduled; the fp32 output is one correctly rounded fp32 multiply.  Shifts are arithmetic.
 *
 * LEVEL of a pixel: a uint8 value itself; of an fp32 value v, min(255, max(0, (int)floorf(v * 255.0f + 0.5f))), the product and the sum
 * each rounded to fp32 (no FMA).
 *
 * Tile levels.  T = tile in {16, 32, 64, 128}, GH = ceil(H / T), GW = ceil(W / T).  Tile (i, j) holds the n pixels of rows
 * [i T, min((i + 1) T, H)) and columns [j T, min((j + 1) T, W)); rank = max(1, (n percent + 99) / 100), 1 <= percent <= 100;
 * levels[i][j] = the smallest level L such that at least rank of the tile's pixels have a level <= L (the rank-th smallest level).
 * LAYOUT: uint8 [GH][GW], contiguous.  One read of the page; a wave per tile builds a 256-bin histogram with integer LDS atomics (sums that
 * do not depend on their order) and scans it.  Columns behind W (the pitch padding) are never read. */
int acai_page_tile_levels(const void *page, int in_u8, int H, int W, int pitch, int tile, int percent, uint8_t *levels, void *stream);

/* The page divided by its interpolated paper level, ONE launch.  With g = levels [GH][GW] as acai_page_tile_levels wrote it for the same
 * H, W, tile:
 *   rescue and floor   m[i][j] = max of g over the 3 x 3 neighbourhood of (i, j) clipped at the grid's border (the tile itself included);
 *                      s[i][j] = max(floor, g[i][j] * 256 < m[i][j] * rq ? m[i][j] : g[i][j]),  0 <= rq <= 256 (rq = round(ink_ratio * 256);
 *                      0: no rescue),  1 <= floor <= 255.  A tile that is mostly ink takes its brightest neighbour's level instead of
 *                      passing ink off as paper; a shadow, rarely 1 / ink_ratio times darker than the paper beside it, keeps its own.
 *   background         per axis, with coordinate c, grid size G and D = 2 T:  u = 2 c + 1 - T,  j0 = floor(u / D),  w = u - j0 D (odd, in
 *                      [1, D)),  the grid indices clamp(j0, 0, G - 1) and clamp(j0 + 1, 0, G - 1): tile centres, the border replicated;
 *                      bg = ((D - wy) ((D - wx) s00 + wx s01) + wy ((D - wx) s10 + wx s11) + D D / 2) >> log2(D D)   (< 2^24 before the
 *                      shift; floor <= bg <= 255);
 *   output             recip[b] = (255 * 65536 + b / 2) / b in integers (b = 1 .. 255; <= 16 711 680, exact in fp32);
 *                      uint8: out = min(255, (p recip[bg] + 32768) >> 16) in unsigned 32 bits, no float arithmetic;
 *                      fp32:  out = fminf(1.0f, v * ((float)recip[bg] * 0x1p-16f)).
 * `out` [H][out_pitch >= W] has the input's element type and is not the input.  Every pixel is read once and written once, 16 bytes per
 * lane where base and pitch (of the page for loads, of `out` for stores) are multiples of 16 bytes, element by element where not and
 * across W; nothing behind W is read or written.  A workgroup covers 16 rows of one tile row and stages the five raw grid rows they depend
 * on (three rows of s, each a 3 x 3 maximum), s and recip in LDS. */
int acai_page_flatten(const void *page, int in_u8, int H, int W, int pitch, const uint8_t *levels, int tile, int rq, int floor_level, void *out,
                      int out_pitch, void *stream);

/* ---- page rectification: find the sheet's outline in the photo and warp it flat (csrc/rectify.hip) --------------------------------------
 * Every page stage above takes the tensor it is given for the sheet; a phone photo is a sheet seen at an angle, lying on something darker.
 * A page is as acai_page_profile takes it (uint8 or fp32, pitch >= W, the same size limits).  A pixel is PAPER when it is not ink under the
 * ink test of the stages above at paper_threshold: !(in_sample(p) < paper_threshold).  Everything is defined in integers, the fp32 blend
 * aside, and no result depends on how the launches are scheduled.  Shifts are arithmetic, divisions marked "floor" round down. */
#define ACAI_EXTENTS_MAX_RUN 256   /* acai_page_extents: the longest run that can be asked for ... */
#define ACAI_EXTENTS_TILE_ROWS 64  /* ... and the rows of a column workgroup's chunk (it also reads the min_run - 1 rows above them) */

/* Paper extents, R = min_run in 1 .. ACAI_EXTENTS_MAX_RUN.  out is int32 [2 H + 2 W]:
 *   out[y]             row_lo[y] = the smallest x with pixels x .. x + R - 1 of row y all paper, W if there is none;
 *   out[H + y]         row_hi[y] = the largest x with pixels x - R + 1 .. x of row y all paper, -1 if there is none;
 *   out[2 H + x]       col_lo[x] = the smallest y with pixels y .. y + R - 1 of column x all paper, H if there is none;
 *   out[2 H + W + x]   col_hi[x] = the largest y with pixels y - R + 1 .. y of column x all paper, -1 if there is none.
 * Columns behind W (the pitch padding) are never read and end every run.  TWO launches, each reading the page once: a wave per row joins
 * the run summaries of its lanes' 16-byte units and writes row_lo / row_hi (and the "none" values of the column halves); then workgroups
 * over (512 bytes of the rows, ACAI_EXTENTS_TILE_ROWS rows) walk their columns down, having also read the R - 1 rows above their chunk (a
 * run that ends in the chunk may begin there), and lower col_lo / raise col_hi with integer atomic min / max: the same whatever the order.
 * 16 bytes per lane where base and pitch are multiples of 16 bytes, element by element where not and across W. */
int acai_page_extents(const void *page, int in_u8, int H, int W, int pitch, float paper_threshold, int min_run, int32_t *out, void *stream);

/* The page seen through the homography coef = {A, B, C, D, E, F, G, H, I} (nine 64-bit integers in host memory, passed by value into the
 * launch).  Output pixel (x, y) of `out` [OH][out_pitch >= OW] (the input's element type, not the input; OH, OW within the page limits) is
 * sampled at, all in 64-bit integers,
 *   den = G x + H y + I,   sxq = floor((A x + B y + C) * 256 / den),   syq = floor((D x + E y + F) * 256 / den),
 *   ix = sxq >> 8, fx = sxq & 255, iy = syq >> 8, fy = syq & 255,
 * with the taps and the blend of acai_page_rotate: t00 = (iy, ix), t01 = (iy, ix + 1), t10 = (iy + 1, ix), t11 = (iy + 1, ix + 1), a tap
 * outside the page reads `fill` (uint8: an integer in 0 .. 255); uint8: ((256 - fy) ((256 - fx) t00 + fx t01) + fy ((256 - fx) t10 + fx t11)
 * + 32768) >> 16; fp32: the same weights f / 256 in fp32.  So A = E = I = 2^30 and the rest 0 is the identity.  Refused, with an error
 * that begins "acai_page_warp:": at any of the four output corners (0, 0), (OW - 1, 0), (OW - 1, OH - 1), (0, OH - 1), den <= 0 or
 * den >= 2^62, or |A x + B y + C| * 256 or |D x + E y + F| * 256 reaching 2^62 (the forms are linear, so the corners bound them over the
 * whole output); out == page; bad sizes.  The quotients are exact: a double estimate corrected by the integer remainder, the 64-bit
 * division where the estimate could be off by more than one.  A lane makes 4 consecutive pixels, stepping the forms by A, D, G. */
int acai_page_warp(const void *page, int in_u8, int H, int W, int pitch, const int64_t coef[9], float fill, void *out, int OH, int OW, int out_pitch,
                   void *stream);

/* ---- page ingest: colour photos and EXIF / quarter-turn orientation (csrc/ingest.hip) ------------------------------------------------------
 * The reference makes the grey, upright page on the host with PIL: Image.open(...).convert("L") (acai_omr/ui/routes.py:98,115,
 * train/datasets.py:32,122) and ImageOps.exif_transpose (ui/routes.py:118).  Here the decoded photo is uploaded as it is and one launch
 * makes the page, with the same bits.  Everything is defined in integers; no atomics. */
#define ACAI_COL_CHUNK_ROWS 64   /* acai_page_col_profile: a chunk of rows is max(64, ceil(H / 64)) rows ... */
#define ACAI_COL_MAX_CHUNKS 64   /* ... so there are ceil(H / that) <= 64 chunks, and `work` holds 4 * chunks * W int32 */

/* src is an image of H rows, W columns and C channels whose element (row r, column c, channel k) lies at src[r row_stride + c pix_stride +
 * k chan_stride], strides in elements: interleaved (H, W, C), planar (C, H, W), a slice of a larger tensor, all the same kernel.  uint8
 * (in_u8 = 1) with C = 1, 3 or 4, or fp32 with C = 1.  The grey value of a uint8 pixel is PIL's: the channel itself for C = 1, otherwise
 * (19595 R + 38470 G + 7471 B + 32768) >> 16 of channels 0, 1, 2 (a fourth channel is ignored, as PIL's RGBA -> L ignores it); an fp32
 * pixel is moved as 32 bits, whatever they hold.  orientation is an EXIF code, applied as ImageOps.exif_transpose applies it: pixel (y, x)
 * of `out` [OH][out_pitch >= OW] (uint8, or fp32 for fp32 input; not the source) is the grey value of source element
 *   1: [y, x]          2: [y, W-1-x]      3: [H-1-y, W-1-x]    4: [H-1-y, x]        and OH x OW = H x W,
 *   5: [x, y]          6: [H-1-x, y]      7: [H-1-x, W-1-y]    8: [x, W-1-y]        and OH x OW = W x H.
 * OH <= ACAI_PAGE_MAX_H, OW <= ACAI_PAGE_MAX_W.  ONE launch.  A lane makes 4 consecutive output pixels from 4 C source bytes read as
 * dwords; codes 5 .. 8 pass a 128 x 128 tile of grey values through LDS so that source rows are read and output rows written whole. */
int acai_page_ingest(const void *src, int in_u8, int H, int W, int C, int64_t pix_stride, int64_t row_stride, int64_t chan_stride, int orientation,
                     void *out, int out_pitch, void *stream);

/* Column profiles of a page as acai_page_profile takes it: ink[x] = number of pixels of column x with value < ink_threshold, run[x] = the
 * longest run of consecutive such pixels down the column: acai_page_profile of the transposed page (the reference has no counterpart; a
 * page that lies on its side has its staff lines in the columns).  TWO launches: lanes own 4 adjacent columns and walk a chunk of rows
 * down, leaving (leading run, trailing run, best run, ink) per column and chunk in `work` (work_elems int32, at least 4 * chunks * W, see
 * ACAI_COL_CHUNK_ROWS); one lane per column then joins its chunks from the top down. */
int acai_page_col_profile(const void *page, int in_u8, int H, int W, int pitch, float ink_threshold, int32_t *ink, int32_t *run, int32_t *work,
                          int64_t work_elems, void *stream);

/* out[i] = the number of pixels with value < ink_threshold in rows [y0, y1), columns [x0, x1) of the page, for the n rectangles boxes [n][4]
 * = (x0, y0, x1, y1) in device memory (clipped to the page on the device; an empty one counts 0).  ONE launch, none for n = 0;
 * n <= 65535.  The reference has no counterpart: it is how the orientation estimate asks which end of a system holds the clef. */
int acai_page_box_ink(const void *page, int in_u8, int H, int W, int pitch, float ink_threshold, const int32_t *boxes, int n, int32_t *out, void *stream);

/* ---- page assessment: staff scale from run lengths, focus and contrast (csrc/assess.hip) ------------------------------------------------------
 * An extension; the reference decodes whatever photo it is handed.  A page is as acai_page_profile takes it (uint8 or fp32, pitch >= W, the
 * same size limits).  Integers only: the only atomics are integer adds, so the results are the same bits on every run and for every
 * launch geometry.  Both entry points ADD to their output: the caller zeroes it (one fill serves all pages of a call). */
#define ACAI_RUNS_CHUNK_ROWS 32    /* acai_page_runs: a wave walks 32 rows of 256 columns; `work` holds ceil(H / 32) * W int32 */
#define ACAI_SHARP_CHUNK_ROWS 32   /* acai_page_sharpness: likewise, plus the row above and the row below */

/* Vertical run-length histograms, hist int64 [3][256].  A pixel is ink exactly as in acai_page_profile: in_sample(p) < ink_threshold.  In
 * every column take the maximal vertical runs of equal colour.  A run that touches row 0 or row H - 1 is OPEN - its true length is not
 * known - and is never counted; every other run is closed.
 *   hist[0][min(n, 255)] += 1  for every closed ink run of n rows,
 *   hist[1][min(n, 255)] += 1  for every closed paper run of n rows,
 *   hist[2][min(b + w, 255)] += 1  for every closed ink run of b rows that is directly followed, downwards, by a closed paper run of w rows.
 * Bin 0 of every row stays as it was.  (The most frequent closed ink run of an engraved page is the thickness of a staff line, the most
 * frequent pair the distance from staff line to staff line.)  TWO launches: a wave owns 256 columns (a lane 4 adjacent ones, so a wave reads
 * 256 consecutive pixels of a row) of a chunk of ACAI_RUNS_CHUNK_ROWS rows and walks them down; runs that begin and end inside the chunk, and
 * pairs of two such runs, are counted there - in LDS, then one global add per non-empty bin and workgroup - and the first and last run of
 * every (column, chunk), with the run next to each, are left in `work` (work_elems int32, at least ceil(H / ACAI_RUNS_CHUNK_ROWS) * W); one
 * lane per column then joins its chunks from the top down and counts the runs and pairs that cross or touch a chunk's edge. */
int acai_page_runs(const void *page, int in_u8, int H, int W, int pitch, float ink_threshold, int64_t *hist, int32_t *work, int64_t work_elems,
                   void *stream);

/* Levels and their Laplacian in one read of the page, out int64 [3 + 256].  The level of a pixel is acai_page_tile_levels': a uint8 value as
 * it is, an fp32 value v as floor(v * 255 + 0.5) (the product and the sum rounded one after the other) clamped to 0 .. 255.
 *   out[3 + l] += the number of pixels of level l, over the whole page,
 *   out[0] += sum L, out[1] += sum L * L, out[2] += count over the interior pixels (rows 1 .. H - 2, columns 1 .. W - 2), where
 *   L = 4 p - up - down - left - right on levels, and count = (H - 2) (W - 2), or 0 when H < 3 or W < 3.
 * |L| <= 1020, so the sums fit 64 bits for every page within the size limits.  ONE launch: the waves and lanes of acai_page_runs, three
 * rows of levels in registers; per-lane sums are added up over the wave by shuffles and over the workgroup in LDS, then one global add
 * per workgroup and sum, and one per non-empty level. */
int acai_page_sharpness(const void *page, int in_u8, int H, int W, int pitch, int64_t *out, void *stream);

/* ---- blank-patch pruning ahead of the encoder (csrc/prune.hip) -------------------------------------------------------------------------------
 * An extension; the reference encodes every patch.  The packed patch stream [M][L] (L = P * P elements per row, fp32 or bf16, rows `pitch`
 * elements apart; the base need not be the start of an allocation) loses the rows that are paper.  THREE launches for a whole batch and one
 * copy of the per-image kept counts to the host, which sizes the output between the second and the third.  Integers only, no atomics: the
 * same result on every run, kept patches in ascending order.
 * The device table is int32 [B][ACAI_PRUNE_TABLE_COLS], per image: h_p, w_p, its first row in the full stream, the first row of its
 * positional grid in the positional table, that grid's width (the table's own width, or w_p for an interpolated grid appended to it), and
 * three words that are not read.  The caller guarantees h_p, w_p >= 1 and that the images' row ranges lie inside the M rows. */
#define ACAI_PRUNE_TABLE_COLS 8
#define ACAI_PRUNE_MAX_HALO 3
#define ACAI_PRUNE_MAX_GRID (1 << 20)   /* patches of one image */
#define ACAI_PRUNE_MAX_IMAGES 65535

/* ink[r] = the number of elements of row r that are strictly below ink_level, compared on the stored value widened to fp32 (a NaN element is
 * not ink).  One wave per row; 16-byte loads where base and pitch are multiples of 16 bytes, element by element where not and for the
 * L % (16 / element size) trailing elements.  Any L >= 1. */
int acai_patch_ink(const void *patches, int dtype, int M, int L, int64_t pitch, float ink_level, int32_t *ink, void *stream);

/* One workgroup per image.  inked[r][c] = ink > max_ink; keep[r][c] = some inked patch (r', c') of the SAME image with max(|r - r'|,
 * |c - c'|) <= halo; an image without an inked patch keeps all of its patches.  The kept local indices r * w_p + c are written in ascending
 * order from the image's first row on into kept_local [M] (the rest of its slot is left as it was) and their number into count[i].  The
 * block-wide exclusive scan of keep is formed from the waves' 64-bit ballots and popcounts, with the wave totals passed through LDS and a
 * running base across chunks of 256 patches.  max_grid: the largest h_p * w_p of the table, at most ACAI_PRUNE_MAX_GRID;
 * halo in 0 .. ACAI_PRUNE_MAX_HALO; B <= ACAI_PRUNE_MAX_IMAGES. */
int acai_patch_keep(const int32_t *ink, const int32_t *table, int B, int max_grid, int max_ink, int halo, int32_t *kept_local, int32_t *count,
                    void *stream);

/* cu_out int32 [B + 1]: the exclusive prefix sums of count, in device memory; total = cu_out[B].  Row j of `out` [total][L] (the input's
 * dtype, contiguous, not the input) is the kept patch row it stands for, bit for bit; kept[j] is its local index in its image's grid and
 * pe_idx[j] = pe_base + (kept / w_p) * pe_w + kept % w_p the row of the positional table that belongs to it.  One wave per row. */
int acai_patch_compact(const void *patches, int dtype, int L, int64_t pitch, const int32_t *table, const int32_t *kept_local, const int32_t *cu_out,
                       int B, int total, void *out, int32_t *kept, int32_t *pe_idx, void *stream);

/* Per-token maps over kept patches -> over the full grid.  Image b holds T_b = cu_q[b + 1] - cu_q[b] rows of K_b = cu_kept[b + 1] - cu_kept[b]
 * columns at in + in_off[b] and gets T_b rows of S_b = cu_full[b + 1] - cu_full[b] columns at out + out_off[b]:
 * out_b[t][kept[cu_kept[b] + j]] = in_b[t][j].  `out` is zeroed by the caller; a kept index outside [0, S_b) is skipped.  max_q <= 65535. */
int acai_attn_map_expand(const float *in, const int64_t *in_off, float *out, const int64_t *out_off, const int32_t *cu_q, const int32_t *cu_kept,
                         const int32_t *cu_full, const int32_t *kept, int B, int max_q, int max_kept, void *stream);

/* hipGraph helpers (capture on `stream`, replay). */
int acai_graph_begin(void *stream);
int acai_graph_end(void *stream, void **graph_exec_out);
int acai_graph_launch(void *graph_exec, void *stream);
int acai_graph_destroy(void *graph_exec);

#ifdef __cplusplus
}
#endif
#endif
