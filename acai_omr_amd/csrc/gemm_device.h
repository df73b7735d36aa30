// __device__ helpers that more than one GEMM kernel file uses: the guarded chunk loads of the register-staged kernel, the register and
// LDS-transposed epilogues, the split-K accumulation epilogue, and the LDS-DMA instructions issued from inline asm.
#pragma once
#include "gemm_internal.h"
#include <type_traits>

namespace {

template <typename T, bool FAST>
__device__ __forceinline__ uint4 load_chunk(const T *base, int ld, int row, int rows, int k0, int K) {
    constexpr int EPC = 16 / sizeof(T);
    uint4 r = make_uint4(0, 0, 0, 0);
    if (row >= rows) return r;
    if constexpr (FAST) {
        if (k0 < K) r = *reinterpret_cast<const uint4 *>(base + (size_t)row * ld + k0);
    } else {
        union { uint4 v; T e[EPC]; } u;
        u.v = r;
#pragma unroll
        for (int e = 0; e < EPC; ++e)
            if (k0 + e < K) u.e[e] = base[(size_t)row * ld + k0 + e];
        r = u.v;
    }
    return r;
}

// Transposed storage (backward GEMMs: dX = dY.W reads W as [K][N]; dW = dY^T.X reads both operands reduction-major):
// the operand is stored [k][row] with `row` contiguous.  A thread still owns one 16-byte global chunk (EPC consecutive
// rows at one k) and scatters its elements into EPC LDS rows, so the LDS image and the MFMA loop are unchanged.
template <typename T, bool FAST>
__device__ __forceinline__ uint4 load_chunk_t(const T *base, int ld, int k, int K, int row0, int rows) {
    constexpr int EPC = 16 / sizeof(T);
    uint4 r = make_uint4(0, 0, 0, 0);
    if (k >= K) return r;
    if constexpr (FAST) {
        if (row0 < rows) r = *reinterpret_cast<const uint4 *>(base + (size_t)k * ld + row0);
    } else {
        union { uint4 v; T e[EPC]; } u;
        u.v = r;
#pragma unroll
        for (int e = 0; e < EPC; ++e)
            if (row0 + e < rows) u.e[e] = base[(size_t)k * ld + row0 + e];
        r = u.v;
    }
    return r;
}

// ---- epilogue shared by both main loops: C/D layout col = lane&31, row = (e&3) + 8*(e>>2) + 4*(lane>>5) ----------------
template <int EPI, bool ACCUM>
__device__ __forceinline__ void gemm_epilogue(const GemmArgs &g, const f32x16 (&acc)[2][2], int bm0, int bn0, int wm, int wn, int lr, int lh) {
    constexpr bool TA = ACCUM, TB = ACCUM;
    const bool do_gelu = g.flags & ACAI_GEMM_GELU, do_round = g.flags & ACAI_GEMM_ROUND_BF16;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = bn0 + wn * 64 + j * 32 + lr;
        if (col >= g.N) continue;
        const float bv = g.bias ? g.bias[col] : 0.f;
        const float cs = col < g.scale_cols ? g.col_scale : 1.0f;
        int kv = 0, hh = 0, dd = 0;
        if constexpr (EPI == 1) {
            kv = col / g.E;
            const int e = col - kv * g.E;
            hh = e / g.dh;
            dd = e - hh * g.dh;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = bm0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                if (row >= g.M) continue;
                float v = acc[i][j][e] + bv;
                if constexpr (EPI == 0) {
                    v *= cs;
                    if (do_round) v = round_bf16(v);
                    if (g.aux_mode == 1 || g.aux_mode == 3) {
                        const float keep = g.aux_mode == 1 ? v : gelu_erf_grad(v);
                        if (g.out_dtype == ACAI_BF16) reinterpret_cast<bf16_t *>(g.aux)[(size_t)row * g.ldaux + col] = f2bf(keep);
                        else reinterpret_cast<float *>(g.aux)[(size_t)row * g.ldaux + col] = keep;
                    } else if (g.aux_mode == 2 || g.aux_mode == 4) {
                        const float a0 = g.out_dtype == ACAI_BF16 ? bf2f(reinterpret_cast<const bf16_t *>(g.aux)[(size_t)row * g.ldaux + col])
                                                                  : reinterpret_cast<const float *>(g.aux)[(size_t)row * g.ldaux + col];
                        v *= g.aux_mode == 2 ? gelu_erf_grad(a0) : a0;
                    }
                    if (do_gelu) {
                        v = gelu_erf(v);
                        if (do_round) v = round_bf16(v);
                    }
                    if (g.residual) v += g.residual[(size_t)row * g.ldr + col];
                    if (g.out_dtype == ACAI_BF16)
                        reinterpret_cast<bf16_t *>(g.C)[(size_t)row * g.ldc + col] = f2bf(v);
                    else
                        reinterpret_cast<float *>(g.C)[(size_t)row * g.ldc + col] = v;
                } else {
                    const int b = g.row_seq[row], s = g.row_pos[row];
                    const int64_t off = g.seq_off[b] + ((int64_t)hh * g.seq_len[b] + s) * g.dhp + dd;
                    void *dst = kv ? g.v_out : g.k_out;
                    if (g.out_dtype == ACAI_BF16)
                        reinterpret_cast<bf16_t *>(dst)[off] = f2bf(v);
                    else
                        reinterpret_cast<float *>(dst)[off] = v;
                }
            }
    }
}

// Split-K accumulation epilogue (weight gradients): fp32 atomics straight from the C/D layout - a wave instruction adds two 128-byte row
// segments, the shape the atomic units take at full rate.  One 32x32 block at a time behind a scheduling barrier: left to itself the compiler
// materialises all 64 row addresses first, which cost the register-staged dW kernel 430 registers (one wave per SIMD).
__device__ __forceinline__ void gemm_accum_epilogue(const GemmArgs &g, const f32x16 (&acc)[2][2], int bm0, int bn0, int wm, int wn, int lr, int lh) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = bn0 + wn * 64 + j * 32 + lr, row0 = bm0 + wm * 64 + i * 32 + 4 * lh;
            if (col < g.N) {
                float *base = reinterpret_cast<float *>(g.C) + (size_t)row0 * g.ldc + col;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int ro = (e & 3) + 8 * (e >> 2);
                    if (row0 + ro < g.M) atomicAdd(base + (size_t)ro * g.ldc, acc[i][j][e]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
}

// ---- LDS-transposed epilogue of the LDS-DMA kernels -----------------------------------------------------------------------------------
// The MFMA C/D layout gives a lane one column and 16 scattered rows: storing from it means 2- or 4-byte stores in 64/128-byte runs, which
// bounds the short-K GEMMs (K = 512..768: 8-12 K-steps per output tile).  Each wave therefore transposes its 64x64 block through `stg`
// (its share of the now free LDS stages), 32 rows at a time, and writes 16 bytes per lane along the rows.  Bias and bf16 rounding are applied
// on the way in; GELU (optionally keeping the pre-activation in `aux`), the GELU-derivative product and the fp32 residual on the way out.
template <int ROWS = 32>   // rows staged per pass: 32 (8.5 KB of LDS per wave) or 16 (4.25 KB: the persistent kernel has one free stage)
__device__ __forceinline__ void gemm_vec_epilogue(const GemmArgs &g, const f32x16 (&acc)[2][2], float *stg, int bm0, int bn0, int wm, int wn, int lane) {
    constexpr int EP = 68;  // floats per staged row (64 + 4: 16-byte aligned rows, conflict-light)
    constexpr int NP = 32 / ROWS;   // passes per 32-row block
    const int lr = lane & 31, lh = lane >> 5;
    const int ldc_e = g.ldc, n_valid = g.N - (bn0 + wn * 64);
    const bool do_gelu = g.flags & ACAI_GEMM_GELU, do_round = g.flags & ACAI_GEMM_ROUND_BF16;
    // The bf16 rounding on the way into LDS is skipped when the value goes straight to a bf16 store, which rounds the same number the same way
    // (measured: no change in tile time -- the epilogue is a latency chain, not VALU issue).
    const bool pre_round = do_round && (do_gelu || g.aux_mode != 0 || g.residual != nullptr || g.out_dtype != ACAI_BF16);
    // `a4`: the saved pre-activation of these four columns (aux_mode 2, loaded by the caller in one access per lane)
    auto finish = [&](f32x4 &v, int row, int col, const float (&a4)[4]) {   // four consecutive columns of one row, after bias / rounding
        if (g.aux_mode == 2) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] *= gelu_erf_grad(a4[e]);
        } else if (g.aux_mode == 4) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] *= a4[e];
        }
        if (do_gelu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = gelu_erf(v[e]);
                if (do_round) v[e] = round_bf16(v[e]);
            }
        }
        if (g.residual) v += *reinterpret_cast<const f32x4 *>(g.residual + (size_t)row * g.ldr + col);
    };
#pragma unroll
    for (int ip = 0; ip < 2 * NP; ++ip) {
        const int i = ip / NP, pass = ip % NP;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = bn0 + wn * 64 + j * 32 + lr;
            const float bv = (g.bias && col < g.N) ? g.bias[col] : 0.f;
            const float cs = col < g.scale_cols ? g.col_scale : 1.0f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                if (NP == 2 && (e >> 3) != pass) continue;   // 16-row passes: registers 0..7 hold rows 0..15, 8..15 rows 16..31
                float v = (acc[i][j][e] + bv) * cs;
                if (pre_round) v = round_bf16(v);
                stg[((e & 3) + 8 * ((e >> 2) & (NP == 2 ? 1 : 3)) + 4 * lh) * EP + j * 32 + lr] = v;
            }
        }
        // same wave wrote and now reads: LDS operations of a wave complete in order
        const int row_base = bm0 + wm * 64 + i * 32 + pass * ROWS, col_base = bn0 + wn * 64;
        if (g.out_dtype == ACAI_BF16) {
#pragma unroll
            for (int it = 0; it < ROWS / 8; ++it) {
                const int idx = it * 64 + lane, r = idx >> 3, c8 = (idx & 7) * 8;
                const int row = row_base + r;
                if (row < g.M && c8 < n_valid) {
                    f32x4 v0 = *reinterpret_cast<const f32x4 *>(stg + r * EP + c8), v1 = *reinterpret_cast<const f32x4 *>(stg + r * EP + c8 + 4);
                    float a0[4] = {0.f, 0.f, 0.f, 0.f}, a1[4] = {0.f, 0.f, 0.f, 0.f};
                    bf16_t *auxp = reinterpret_cast<bf16_t *>(g.aux) + (size_t)row * g.ldaux + col_base + c8;
                    if (g.aux_mode == 2 || g.aux_mode == 4) {        // saved pre-activation / derivative: ONE 16-byte load per lane
                        const uint4 r4 = *reinterpret_cast<const uint4 *>(auxp);
                        a0[0] = __uint_as_float(r4.x << 16); a0[1] = __uint_as_float(r4.x & 0xFFFF0000u);
                        a0[2] = __uint_as_float(r4.y << 16); a0[3] = __uint_as_float(r4.y & 0xFFFF0000u);
                        a1[0] = __uint_as_float(r4.z << 16); a1[1] = __uint_as_float(r4.z & 0xFFFF0000u);
                        a1[2] = __uint_as_float(r4.w << 16); a1[3] = __uint_as_float(r4.w & 0xFFFF0000u);
                    } else if (g.aux_mode == 1) {  // keep the pre-activation: ONE 16-byte store per lane (was two 8-byte ones: the tail is store-issue bound)
                        uint4 p4;
                        p4.x = pack_bf16(v0[0], v0[1]); p4.y = pack_bf16(v0[2], v0[3]); p4.z = pack_bf16(v1[0], v1[1]); p4.w = pack_bf16(v1[2], v1[3]);
                        *reinterpret_cast<uint4 *>(auxp) = p4;
                    } else if (g.aux_mode == 3) {  // keep gelu'(pre-activation)
                        uint4 p4;
                        p4.x = pack_bf16(gelu_erf_grad(v0[0]), gelu_erf_grad(v0[1])); p4.y = pack_bf16(gelu_erf_grad(v0[2]), gelu_erf_grad(v0[3]));
                        p4.z = pack_bf16(gelu_erf_grad(v1[0]), gelu_erf_grad(v1[1])); p4.w = pack_bf16(gelu_erf_grad(v1[2]), gelu_erf_grad(v1[3]));
                        *reinterpret_cast<uint4 *>(auxp) = p4;
                    }
                    finish(v0, row, col_base + c8, a0);
                    finish(v1, row, col_base + c8 + 4, a1);
                    uint4 o;
                    o.x = pack_bf16(v0[0], v0[1]); o.y = pack_bf16(v0[2], v0[3]); o.z = pack_bf16(v1[0], v1[1]); o.w = pack_bf16(v1[2], v1[3]);
                    *reinterpret_cast<uint4 *>(reinterpret_cast<bf16_t *>(g.C) + (size_t)row * ldc_e + col_base + c8) = o;
                }
            }
        } else {
#pragma unroll
            for (int it = 0; it < ROWS / 4; ++it) {
                const int idx = it * 64 + lane, r = idx >> 4, c4 = (idx & 15) * 4;
                const int row = row_base + r;
                if (row < g.M && c4 < n_valid) {
                    f32x4 v0 = *reinterpret_cast<const f32x4 *>(stg + r * EP + c4);
                    float a0[4] = {0.f, 0.f, 0.f, 0.f};
                    float *auxp = reinterpret_cast<float *>(g.aux) + (size_t)row * g.ldaux + col_base + c4;
                    if (g.aux_mode == 2 || g.aux_mode == 4) {
                        const f32x4 r4 = *reinterpret_cast<const f32x4 *>(auxp);
#pragma unroll
                        for (int e = 0; e < 4; ++e) a0[e] = r4[e];
                    } else if (g.aux_mode == 1) {
                        *reinterpret_cast<f32x4 *>(auxp) = v0;
                    } else if (g.aux_mode == 3) {
                        *reinterpret_cast<f32x4 *>(auxp) = f32x4{gelu_erf_grad(v0[0]), gelu_erf_grad(v0[1]), gelu_erf_grad(v0[2]), gelu_erf_grad(v0[3])};
                    }
                    finish(v0, row, col_base + c4, a0);
                    *reinterpret_cast<f32x4 *>(reinterpret_cast<float *>(g.C) + (size_t)row * ldc_e + col_base + c4) = v0;
                }
            }
        }
    }
}

// One 16-byte-per-lane LDS-DMA instruction from inline asm (hidden from the compiler's wait-count pass, see gemm_nt_glds3_kernel): M0 carries
// the wave-uniform LDS destination; it is saved and restored around the instruction, so the asm has no reserved-register clobber.
__device__ __forceinline__ void glds16(uint32_t lds_dst, const void *src) {
    uint32_t m0_save;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(m0_save)
                 : "s"(lds_dst), "v"(src)
                 : "memory");
}

// the same with the source as a uniform base (SGPR pair) + a 32-bit byte offset per lane
__device__ __forceinline__ void glds16s(uint32_t lds_dst, const void *sbase, uint32_t voff) {
    uint32_t m0_save;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %3\n\ts_mov_b32 m0, %0"
                 : "=&s"(m0_save)
                 : "s"(lds_dst), "v"(voff), "s"(sbase)
                 : "memory");
}

// four pieces of one 32 KB unit (consecutive 1 KiB destinations 8 KiB apart: wave w's pieces of a [256][128 B] image) in one block: one M0
// save / restore instead of four
__device__ __forceinline__ void glds16s_x4(uint32_t lds_dst, const void *sbase, uint32_t o0, uint32_t o1, uint32_t o2, uint32_t o3) {
    uint32_t m0_save;
    asm volatile("s_mov_b32 %0, m0\n\t"
                 "s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %6\n\t"
                 "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, %6\n\t"
                 "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %4, %6\n\t"
                 "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %5, %6\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(m0_save)
                 : "s"(lds_dst), "v"(o0), "v"(o1), "v"(o2), "v"(o3), "s"(sbase)
                 : "memory", "scc");
}

// The same through a buffer resource (buffer_load_dwordx4 ... offen lds): lanes whose offset lies beyond the resource's num_records write
// ZEROS into LDS (measured, tools/experiments/lds_dma_oob.hip: per dword) - a ragged last K-tile of the token-major operands needs no
// remainder launch.  (Only the VGPR offset is range-checked, not an SGPR offset: the K-step's advance goes into the resource's base.)
__device__ __forceinline__ void blds16(uint32_t lds_dst, __amdgpu_buffer_rsrc_t rs, uint32_t voff) {
    uint32_t m0_save;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(m0_save)
                 : "s"(lds_dst), "v"(voff), "s"(rs)
                 : "memory");
}

__device__ __forceinline__ void blds16_x4(uint32_t lds_dst, __amdgpu_buffer_rsrc_t rs, uint32_t o0, uint32_t o1, uint32_t o2, uint32_t o3) {
    uint32_t m0_save;
    asm volatile("s_mov_b32 %0, m0\n\t"
                 "s_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %6, 0 offen lds\n\t"
                 "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tbuffer_load_dwordx4 %3, %6, 0 offen lds\n\t"
                 "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tbuffer_load_dwordx4 %4, %6, 0 offen lds\n\t"
                 "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tbuffer_load_dwordx4 %5, %6, 0 offen lds\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(m0_save)
                 : "s"(lds_dst), "v"(o0), "v"(o1), "v"(o2), "v"(o3), "s"(rs)
                 : "memory", "scc");
}

}  // namespace
