// Decode attention (see decode.hip for the step it is chained into).
//   decode_attn   : flash-decoding split over keys: grid (split, head, sequence), 8 lanes per key
//                   (dh 64 bf16 = 128 B), online softmax per lane group, in-wave + LDS combine, one
//                   (m, l, o[dh]) partial per workgroup; attn_combine merges the splits.
#include "decode_internal.h"

namespace {

// LPK = lanes per key = dhp * sizeof(TC) / 16.  RAGGED = cross attention over the ragged encoder memory (the dominant
// HBM stream of a decode step); !RAGGED = self attention over the [B][H][Tmax][dhp] cache.  Two instantiations so that
// rocprof reports them as separate kernels.  ANC (self attention of a beam step, !RAGGED only): the cache rows are read through the
// ancestor table - key p of row b from k_self[anc[b][p]][h][p][:] - staged in LDS (dynamic shared memory, chunk ints) before the key loop.
// SLOT (self attention of a continuous-batching step, !RAGGED only): the cache is a ring of Tmax positions shared by the rows' write index
// step[1]; row b has its own length seq_len[b] and its key j sits at position (slot_first[b] + j) % Tmax of its own cache row.
// TC = fp8e4m3_t (RAGGED only): the FP8 memory cache.  16 elements per 16-byte load, so LPK = dhp / 16 (4 lanes per key at d_h 64); the
// key's K and V scales are requested with its bytes and fold in outside the element loops: s = (q . k8) sk scale_log2e, acc += (p sv) v8,
// l += p.
// SPEC (self attention of a speculative verify step, !RAGGED only): the R rows of an image verify consecutive tokens of ONE sequence.  Row j
// of image i attends over keys 0 .. t[i] - 1 + j; key p is found through the image's table entry (cache row of the image, cache position),
// staged in LDS like the ancestor table.  The key loop runs over the logical index p exactly as the plain form's, so a row's sums are
// ordered as the greedy step orders them.  Every index formed from a table entry is clamped into the image's rows and the cache.
template <typename TC, int LPK, bool RAGGED, int U = 2, bool ANC = false, bool SLOT = false, bool SPEC = false>
__global__ __launch_bounds__(256) void decode_attn_kernel(DAttnArgs a) {
    static_assert(!(ANC && RAGGED), "the ancestor table indexes the self-attention cache");
    static_assert(!(SLOT && (RAGGED || ANC)), "the ring indexes the self-attention cache of the row itself");
    static_assert(!(SPEC && (RAGGED || ANC || SLOT)), "the key table indexes the self-attention cache of the image's rows");
    constexpr bool F8 = sizeof(TC) == 1;
    static_assert(!F8 || RAGGED, "FP8 storage is the cross K/V's only");
    constexpr int EPC = 16 / sizeof(TC), KPW = 64 / LPK;
    __shared__ float red[4][2 + 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kq = lane % LPK, kg = lane / LPK;
    const int split = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    // The launch is a latency chain after a kernel boundary (the self form moves a few KB; the cross form's ramp delays its first K/V byte).
    // Every argument the form uses comes in by ONE batch of scalar loads and one wait (left alone, the compiler fetched the struct in up to
    // four dependent stages, each a cold round trip), and PLAIN / RAGGED request what does not depend on the sequence length - q, and the
    // self form's first key groups - before they wait for the length.
    constexpr bool PLAIN = !RAGGED && !ANC && !SLOT && !SPEC;
    asm volatile("" ::"s"(a.q), "s"(a.kc), "s"(a.vc), "s"(a.partial), "s"(a.ldq), "s"(a.H), "s"(a.dh), "s"(a.dhp), "s"(a.Tmax), "s"(a.chunk),
                 "s"(a.nsplit), "s"(a.scale_log2e), "s"(a.out), "s"(a.ldo), "s"(a.round_out), "s"(a.tickets), "s"(a.out_bf16));
    if constexpr (RAGGED) asm volatile("" ::"s"(a.seq_off), "s"(a.seq_len));   // (Tmax, above, is not RAGGED's: it keeps ldq .. scale_log2e one load)
    if constexpr (PLAIN || ANC) asm volatile("" ::"s"(a.step));
    if constexpr (SLOT || SPEC) asm volatile("" ::"s"(a.seq_len));
    if constexpr (ANC || SLOT || SPEC) asm volatile("" ::"s"(a.anc), "s"(a.anc_pitch), "s"(a.anc_bstride));
    if constexpr (F8) asm volatile("" ::"s"(a.k_scale), "s"(a.v_scale));
    // the length's scalar loads: requested here, used only below the fence that follows the early requests
    [[maybe_unused]] int len_raw = 0;
    [[maybe_unused]] int64_t off_raw = 0;
    if constexpr (RAGGED) {
        len_raw = ld_uniform(a.seq_len + b);
        off_raw = ld_uniform(a.seq_off + b);
    } else if constexpr (PLAIN) len_raw = ld_uniform(a.step + 1);

    // q: EPC floats per lane as 16-byte loads at clamped addresses (a piece past dh re-reads the row's last piece; its lanes are zeroed
    // below), or - rows that are not 16-byte aligned, dh no multiple of 4 - as dword loads clamped to the row's last element.  No branch
    // around a load in either form.
    float qf[EPC];
    auto request_q = [&]() {
        const float *qr = a.q + (size_t)b * a.ldq + h * a.dh;
        if ((((uintptr_t)a.q | (uintptr_t)(unsigned)a.ldq * 4 | (uintptr_t)(unsigned)a.dh * 4) & 15) == 0 && a.dh >= 4) {
#pragma unroll
            for (int j = 0; j < EPC / 4; ++j) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(qr + min(kq * EPC + 4 * j, a.dh - 4));
#pragma unroll
                for (int e = 0; e < 4; ++e) qf[4 * j + e] = v[e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < EPC; ++e) qf[e] = qr[min(kq * EPC + e, a.dh - 1)];
        }
    };
    auto zero_q_past_dh = [&]() {
#pragma unroll
        for (int e = 0; e < EPC; ++e) qf[e] = kq * EPC + e < a.dh ? qf[e] : 0.f;
    };
    if constexpr (!ANC && !SPEC) request_q();   // (the table forms stage their table first: q held across that barrier costs them ~20 VGPRs)
    uint4 kn[U], vn[U];
    if constexpr (PLAIN) {
        // the first U key groups of the wave, requested before step[1] returns: the cache row of (b, h) is [Tmax][dhp] whatever the length,
        // and a key index clamped to Tmax - 1 stays inside it; the key loop's `key < c1` test discards what lies past the length
        const TC *K0 = reinterpret_cast<const TC *>(a.kc) + ((size_t)b * a.H + h) * ((size_t)a.Tmax * a.dhp) + kq * EPC;
        const TC *V0 = reinterpret_cast<const TC *>(a.vc) + ((size_t)b * a.H + h) * ((size_t)a.Tmax * a.dhp) + kq * EPC;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int key = max(min(split * a.chunk + wave * KPW + kg + u * 4 * KPW, a.Tmax - 1), 0);
            kn[u] = ld_nt16(K0 + (size_t)key * a.dhp);
            vn[u] = ld_nt16(V0 + (size_t)key * a.dhp);
        }
    }
    __builtin_amdgcn_sched_barrier(0);   // every request above is in flight before the length is waited for
    if constexpr (!ANC && !SPEC) zero_q_past_dh();

    int len, hstride;
    size_t base;
    if constexpr (RAGGED) {
        len = len_raw;
        hstride = len * a.dhp;
        base = (size_t)off_raw + (size_t)h * hstride;
    } else if constexpr (ANC) {
        len = a.step[1] + 1;
        hstride = a.Tmax * a.dhp;
        base = (size_t)h * hstride;   // + anc[b][p] * H * hstride per key
    } else if constexpr (SLOT) {
        len = a.seq_len[b];
        hstride = a.Tmax * a.dhp;
        base = ((size_t)b * a.H + h) * hstride;
    } else if constexpr (SPEC) {
        const int R = (int)a.anc_bstride, img = b / R;
        len = max(1, min(a.seq_len[img] + (b - img * R), min(a.anc_pitch, a.chunk * a.nsplit)));
        hstride = a.Tmax * a.dhp;
        base = ((size_t)img * R * a.H + h) * hstride;   // + (row of the image) * H * hstride per key
    } else {
        len = len_raw + 1;
        hstride = a.Tmax * a.dhp;
        base = ((size_t)b * a.H + h) * hstride;
    }
    float *part = a.partial + (((size_t)b * a.H + h) * a.nsplit + split) * (a.dhp + 2);
    const int c0 = split * a.chunk, c1 = min(len, c0 + a.chunk);
    const bool fused_merge = a.tickets && a.out && a.nsplit > 1;
    if (c0 >= len) {  // empty split: neutral element (m = -1e30, l = 0, o = 0)
        if (tid < a.dhp + 2) {
            if (fused_merge) __hip_atomic_store(part + tid, tid == 0 ? -1.0e30f : 0.f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else part[tid] = tid == 0 ? -1.0e30f : 0.f;
        }
        if (!fused_merge) return;
        // the neutral stores of wave 1 (elements 64, 65) must be drained before wave 0 takes the ticket below
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const TC *Kp = reinterpret_cast<const TC *>(a.kc) + base;
    const TC *Vp = reinterpret_cast<const TC *>(a.vc) + base;
    [[maybe_unused]] const float *Ks = nullptr, *Vs = nullptr;
    if constexpr (F8) {   // the scale of key s sits at row (base / dhp) + s
        const size_t row0 = base >> __builtin_ctz(a.dhp);
        Ks = a.k_scale + row0;
        Vs = a.v_scale + row0;
    }
    [[maybe_unused]] int32_t *anc_s = nullptr;
    if constexpr (ANC) {
        extern __shared__ int32_t anc_dyn[];
        anc_s = anc_dyn;
        const int32_t *ar = a.anc + (size_t)(a.step[0] & 1) * a.anc_bstride + (size_t)b * a.anc_pitch;
        for (int p = c0 + tid; p < c1; p += 256) anc_s[p - c0] = ar[p];
        __syncthreads();
    }
    if constexpr (SPEC) {
        extern __shared__ int32_t anc_dyn[];
        anc_s = anc_dyn;
        const int32_t *tr = a.spec_tab + (size_t)(b / (int)a.anc_bstride) * a.anc_pitch;
        for (int p = c0 + tid; p < c1; p += 256) anc_s[p - c0] = tr[p];
        __syncthreads();
    }
    [[maybe_unused]] int ring0 = 0;
    if constexpr (SLOT) ring0 = a.slot_first[b];
    auto key_off = [&](int key) -> size_t {
        if constexpr (ANC) return (size_t)anc_s[key - c0] * a.H * hstride + (size_t)key * a.dhp;
        else if constexpr (SPEC) {
            const unsigned e = (unsigned)anc_s[key - c0];
            const int r = min((int)(e & 7u), (int)a.anc_bstride - 1), pos = min((int)(e >> 3), a.Tmax - 1);
            return (size_t)r * a.H * hstride + (size_t)pos * a.dhp;
        }
        else if constexpr (SLOT) {
            const int p = ring0 + key;   // ring0 < Tmax, key < seq_len[b] <= Tmax
            return (size_t)(p >= a.Tmax ? p - a.Tmax : p) * a.dhp;
        } else return (size_t)key * a.dhp;
    };

    if constexpr (ANC || SPEC) {
        request_q();
        zero_q_past_dh();
    }
    float m = -1.0e30f, l = 0.f, acc[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) acc[e] = 0.f;

    // software pipeline: the U key groups of iteration i+1 are requested before iteration i is computed (a wave that computes has no load
    // in flight otherwise: PMC showed the VALU busy a third of the time and the waves waiting on memory for half of it)
    [[maybe_unused]] float ksn[U], vsn[U];
    auto request = [&](int key0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int key = key0 + u * 4 * KPW;
            kn[u] = vn[u] = make_uint4(0, 0, 0, 0);
            if constexpr (F8) ksn[u] = vsn[u] = 0.f;
            if (key < c1) {
                // every K/V byte is read exactly once per step: non-temporal loads (streaming cache policy)
                kn[u] = ld_nt16(Kp + key_off(key) + kq * EPC);
                vn[u] = ld_nt16(Vp + key_off(key) + kq * EPC);
                if constexpr (F8) {
                    ksn[u] = __builtin_nontemporal_load(Ks + key);
                    vsn[u] = __builtin_nontemporal_load(Vs + key);
                }
            }
        }
    };
    if constexpr (!PLAIN) request(c0 + wave * KPW + kg);   // (PLAIN: requested above, ahead of the length)
    for (int key0 = c0 + wave * KPW + kg; key0 < c1; key0 += 4 * KPW * U) {
        uint4 kk[U], vv[U];
        [[maybe_unused]] float ks[U], vs[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            kk[u] = kn[u];
            vv[u] = vn[u];
            if constexpr (F8) {
                ks[u] = ksn[u];
                vs[u] = vsn[u];
            }
        }
        if (key0 + 4 * KPW * U < c1) request(key0 + 4 * KPW * U);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int key = key0 + u * 4 * KPW;
            float kf[EPC], vf[EPC];
            if constexpr (F8) {   // v_cvt_pk_f32_fp8: two e4m3 bytes (word 0 or 1 of the dword) -> two floats
                const uint32_t kw[4] = {kk[u].x, kk[u].y, kk[u].z, kk[u].w}, vw[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const auto k0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)kw[e], false), k1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)kw[e], true);
                    const auto v0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)vw[e], false), v1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)vw[e], true);
                    kf[4 * e] = k0[0];
                    kf[4 * e + 1] = k0[1];
                    kf[4 * e + 2] = k1[0];
                    kf[4 * e + 3] = k1[1];
                    vf[4 * e] = v0[0];
                    vf[4 * e + 1] = v0[1];
                    vf[4 * e + 2] = v1[0];
                    vf[4 * e + 3] = v1[1];
                }
            } else if constexpr (sizeof(TC) == 2) {
                const uint32_t kw[4] = {kk[u].x, kk[u].y, kk[u].z, kk[u].w}, vw[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    kf[2 * e] = __uint_as_float(kw[e] << 16);
                    kf[2 * e + 1] = __uint_as_float(kw[e] & 0xffff0000u);
                    vf[2 * e] = __uint_as_float(vw[e] << 16);
                    vf[2 * e + 1] = __uint_as_float(vw[e] & 0xffff0000u);
                }
            } else {
                const f32x4 k4 = __builtin_bit_cast(f32x4, kk[u]), v4 = __builtin_bit_cast(f32x4, vv[u]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    kf[e] = k4[e];
                    vf[e] = v4[e];
                }
            }
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < EPC; ++e) s = fmaf(qf[e], kf[e], s);
            // the LPK lanes of the key: butterfly on the DPP network (after stages 1 and 2 the quads are uniform: the mirror form of stage 4)
            if constexpr (LPK > 1) s = lane_xor_add<1>(s);
            if constexpr (LPK > 2) s = lane_xor_add<2>(s);
            if constexpr (LPK > 4) s += lane_xor4_quad_uniform(s);
            if constexpr (LPK > 8) s = lane_xor_add<8>(s);
            if (key < c1) {  // uniform inside a lane group
                if constexpr (F8) s *= ks[u];
                s *= a.scale_log2e;
                const float mn = fmaxf(m, s), al = fast_exp2(m - mn), p = fast_exp2(s - mn);
                m = mn;
                l = l * al + p;
                float pv = p;
                if constexpr (F8) pv *= vs[u];
#pragma unroll
                for (int e = 0; e < EPC; ++e) acc[e] = acc[e] * al + pv * vf[e];
            }
        }
    }
    // merge the KPW lane groups of this wave (lanes with equal kq)
    // (lane_xor stages; offset 4 - LPK <= 4 - stays a __shfl_xor inside lane_xor<4>: the partner must keep kq, and the quads differ)
    float mw = m;
#define ACAI_MERGE_STAGE(O)                                  \
    if constexpr (LPK <= O) mw = lane_xor_max<O>(mw);
    ACAI_MERGE_STAGE(1) ACAI_MERGE_STAGE(2) ACAI_MERGE_STAGE(4) ACAI_MERGE_STAGE(8) ACAI_MERGE_STAGE(16) ACAI_MERGE_STAGE(32)
#undef ACAI_MERGE_STAGE
    const float f = fast_exp2(m - mw);
    l *= f;
#pragma unroll
    for (int e = 0; e < EPC; ++e) acc[e] *= f;
#define ACAI_MERGE_STAGE(O)                                  \
    if constexpr (LPK <= O) {                                \
        l = lane_xor_add<O>(l);                              \
        _Pragma("unroll") for (int e = 0; e < EPC; ++e) acc[e] = lane_xor_add<O>(acc[e]); \
    }
    ACAI_MERGE_STAGE(1) ACAI_MERGE_STAGE(2) ACAI_MERGE_STAGE(4) ACAI_MERGE_STAGE(8) ACAI_MERGE_STAGE(16) ACAI_MERGE_STAGE(32)
#undef ACAI_MERGE_STAGE
    if (kg == 0) {
        if (kq == 0) {
            red[wave][0] = mw;
            red[wave][1] = l;
        }
#pragma unroll
        for (int e = 0; e < EPC; ++e) red[wave][2 + kq * EPC + e] = acc[e];
    }
    __syncthreads();
    if (wave != 0) return;
    // Wave 0 finishes alone - lane d owns output dim d - so the tail needs no workgroup barrier: combine the four waves, publish the split's
    // partial (write-through), drain, take the ticket, and (last arrival only) merge all splits.
    const int d = lane;
    const float M = fmaxf(fmaxf(red[0][0], red[1][0]), fmaxf(red[2][0], red[3][0]));
    float v = 0.f, lsum = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const float f = fast_exp2(red[w][0] - M);
        v += red[w][2 + d] * f;
        lsum += red[w][1] * f;
    }
    if (a.nsplit == 1 && a.out) {
        if (d < a.dh) {
            float o = v / lsum;
            if (a.round_out) o = round_bf16(o);
            if (a.out_bf16) reinterpret_cast<bf16_t *>(a.out)[(size_t)b * a.ldo + h * a.dh + d] = f2bf(o);   // (exact: o is a bf16 value)
            else a.out[(size_t)b * a.ldo + h * a.dh + d] = o;
        }
        return;
    }
    if (c0 < len && d < a.dhp) {
        // fused merge: write-through (sc1) stores, so the hand-off needs no release fence (an L2 write-back per workgroup)
        if (fused_merge) {
            __hip_atomic_store(part + 2 + d, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (d == 0) {
                __hip_atomic_store(part, M, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(part + 1, lsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        } else {
            part[2 + d] = v;
            if (d == 0) {
                part[0] = M;
                part[1] = lsum;
            }
        }
    }
    if (!fused_merge) return;
    // In-launch merge of the split partials (placement-independent hand-off, write-through form): the partials were stored sc1 (agent-scope
    // atomic stores) by this wave, which drains them, then its lane 0 takes a ticket with an agent-scope atomic add; the wave that draws
    // nsplit-1 reads every partial with sc1 loads (agent-scope atomic loads bypass this CU's L1) and merges.  The counter re-arms itself.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int last = 0;
    if (lane == 0) {
        unsigned *cnt = a.tickets + (size_t)b * a.H + h;
        const unsigned t = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = t == (unsigned)(a.nsplit - 1);
        if (last) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    last = __builtin_amdgcn_readfirstlane(last);
    if (!last || d >= a.dhp) return;
    float *p = a.partial + ((size_t)b * a.H + h) * a.nsplit * (a.dhp + 2);
    auto ld = [&](int i) { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    float Mm = -1.0e30f, lm = 0.f, om = 0.f;
    // the merge sits on the step's critical path: request all (max, sum, value) triples of up to 8 splits before touching any of them
    // (a rolled loop issues one dependent L2 round trip after another: 3 x nsplit of them)
    for (int s0 = 0; s0 < a.nsplit; s0 += 8) {
        float pm[8], pl[8], po[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const bool in = s0 + u < a.nsplit;
            const int pb = (in ? s0 + u : s0) * (a.dhp + 2);
            pm[u] = in ? ld(pb) : -1.0e30f;
            pl[u] = in ? ld(pb + 1) : 0.f;
            po[u] = in ? ld(pb + 2 + d) : 0.f;
        }
        float Mc = Mm;
#pragma unroll
        for (int u = 0; u < 8; ++u) Mc = fmaxf(Mc, pm[u]);
        const float resc = fast_exp2(Mm - Mc);
        lm *= resc;
        om *= resc;
        Mm = Mc;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float w = fast_exp2(pm[u] - Mm);
            lm += pl[u] * w;
            om += po[u] * w;
        }
    }
    if (d < a.dh) {
        float o = om / lm;
        if (a.round_out) o = round_bf16(o);
        if (a.out_bf16) reinterpret_cast<bf16_t *>(a.out)[(size_t)b * a.ldo + h * a.dh + d] = f2bf(o);
        else a.out[(size_t)b * a.ldo + h * a.dh + d] = o;
    }
}

// ---- cross attention of a rollout GROUP (GRPO, models.py:883-891 / 988-1049) on the matrix cores (bf16, d_h padded to 64) --------------
// `group` consecutive decode rows share one image's cross K/V (the engine stores it once).  A workgroup owns (split, head, image, tile of
// 16 rows) and streams its K/V chunk ONCE for all of them: the HBM stream of a step no longer grows with the group size.  (A VALU form -
// GT dot products and softmax updates per key and lane group - was built first and measured SLOWER than letting the rows alias the
// stored K/V through the per-row kernel: 3.7-4.8 ms against 3.25 ms per step at 8 x 8; it is gone.)
// Up to 16 rollout rows of one image are the 16 columns of v_mfma_f32_16x16x32_bf16.  A wave owns 32-key tiles of the workgroup's chunk:
//   S[key][g]  = K . Q^T      A = K rows, loaded from global memory straight in the A layout (lane = key, 16 B = 8 dims), B = Q^T in registers
//   O^T[d][g] += V^T . P      B = P taken from the S accumulators as they stand (keys 4q+j of both 16-key halves = contraction slots 8q+j),
//                             A = V^T read with ds_read_b64_tr_b16 from the wave's private 4 KB image of the V tile (no barrier in the loop)
// so the K/V stream is read once per IMAGE and the per-key VALU work is the softmax of 8 scores per lane.  The running maximum of a query is
// kept equal across the four lanes that share its column (two shuffles when it is raised, lazily); partials / tickets / merge as above.
__global__ __launch_bounds__(256) void decode_attn_gmfma_kernel(DAttnArgs a, int group, int gtiles) {
    typedef bf16_t TC;
    typedef TileLayout<2, 64> TL;
    constexpr int GT = 16, KT = 32, DHP = 64;
    __shared__ __attribute__((aligned(16))) unsigned char vlds[4][KT * DHP * 2];
    __shared__ float red[4][GT][2 + 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int split = blockIdx.x, h = blockIdx.y, img = blockIdx.z / gtiles, gt = blockIdx.z % gtiles;
    const int row0 = img * group + gt * GT, ng = min(GT, group - gt * GT);
    const int len = a.seq_len[row0], hstride = len * DHP;
    const size_t base = (size_t)a.seq_off[row0] + (size_t)h * hstride;
    const int c0 = split * a.chunk, c1 = min(len, c0 + a.chunk);
    const bool fused_merge = a.tickets && a.out && a.nsplit > 1;
    auto part_of = [&](int g) { return a.partial + (((size_t)(row0 + g) * a.H + h) * a.nsplit + split) * (DHP + 2); };
    if (c0 >= len) {  // empty split: neutral elements
        if (tid < DHP + 2)
            for (int g = 0; g < ng; ++g) {
                if (fused_merge) __hip_atomic_store(part_of(g) + tid, tid == 0 ? -1.0e30f : 0.f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else part_of(g)[tid] = tid == 0 ? -1.0e30f : 0.f;
            }
        if (!fused_merge) return;
    }
    const TC *Kp = reinterpret_cast<const TC *>(a.kc) + base;
    const TC *Vp = reinterpret_cast<const TC *>(a.vc) + base;

    // Q^T fragments: lane (g = r16, kq) holds dims db * 32 + kq * 8 + 0..7 of query row0 + g (bf16, as the reference's autocast SDPA input)
    uint4 qb[2];
#pragma unroll
    for (int db = 0; db < 2; ++db) {
        float t[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int d = db * 32 + kq * 8 + e;
            t[e] = (r16 < ng && d < a.dh) ? a.q[(size_t)(row0 + r16) * a.ldq + h * a.dh + d] : 0.f;
        }
        qb[db] = make_uint4(pack_bf16(t[0], t[1]), pack_bf16(t[2], t[3]), pack_bf16(t[4], t[5]), pack_bf16(t[6], t[7]));
    }
    float m = -1.0e30f, l = 0.f;
    f32x4 oacc[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) oacc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    unsigned char *vimg = vlds[wave];
    typedef __attribute__((ext_vector_type(4))) short s4;
    typedef __attribute__((address_space(3))) s4 *lds_s4;

    for (int key0 = c0 + wave * KT; key0 < c1; key0 += 4 * KT) {
        uint4 kf[2][2], vv[4];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int key = key0 + sub * 16 + r16;
#pragma unroll
            for (int db = 0; db < 2; ++db) kf[sub][db] = key < c1 ? ld_nt16(Kp + (size_t)key * DHP + db * 32 + kq * 8) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = lane + 64 * i, row = c >> 3, key = key0 + row;
            vv[i] = key < c1 ? ld_nt16(Vp + (size_t)key * DHP + (c & 7) * 8) : make_uint4(0, 0, 0, 0);
        }
        f32x4 sc[2];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            sc[sub] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int db = 0; db < 2; ++db)
                sc[sub] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kf[sub][db]), __builtin_bit_cast(bf16x8, qb[db]), sc[sub], 0, 0, 0);
        }
        // this lane: keys key0 + 16 sub + 4 kq + j of query r16
        float tmax = -1.0e30f;
        bool ok[2][4];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ok[sub][j] = key0 + sub * 16 + 4 * kq + j < c1;
                sc[sub][j] *= a.scale_log2e;
                if (ok[sub][j]) tmax = fmaxf(tmax, sc[sub][j]);
            }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));   // equal on the four lanes of a query column
        if (__ballot(tmax > m + 8.0f)) {
            const float mn = fmaxf(m, tmax), al = fast_exp2(m - mn);
            m = mn;
            l *= al;
#pragma unroll
            for (int d = 0; d < 4; ++d) oacc[d] *= al;
        }
        float p[2][4];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                p[sub][j] = ok[sub][j] ? fast_exp2(sc[sub][j] - m) : 0.f;
                l += p[sub][j];
            }
        const uint4 pf = make_uint4(pack_bf16(p[0][0], p[0][1]), pack_bf16(p[0][2], p[0][3]), pack_bf16(p[1][0], p[1][1]), pack_bf16(p[1][2], p[1][3]));
        // V tile -> this wave's LDS image (the previous tile's transposing reads were consumed by its MFMAs: same wave, in order)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = lane + 64 * i;
            *reinterpret_cast<uint4 *>(vimg + TL::off(c >> 3, c & 7)) = vv[i];
        }
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int vrow = 4 * kq + (r16 >> 2), vchunk = d * 2 + ((r16 & 3) >> 1), vsub = 8 * (r16 & 1);
            union { s4 v[2]; uint4 u; } vf;
            vf.v[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(vimg + TL::off(vrow, vchunk) + vsub));
            vf.v[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(vimg + TL::off(vrow + 16, vchunk) + vsub));
            oacc[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vf.u), __builtin_bit_cast(bf16x8, pf), oacc[d], 0, 0, 0);
        }
    }
    // wave result: column g = r16; l summed over the four lanes of the column; O^T rows d = 16 dblk + 4 kq + j
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    if (kq == 0) {
        red[wave][r16][0] = m;
        red[wave][r16][1] = l;
    }
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int j = 0; j < 4; ++j) red[wave][r16][2 + d * 16 + 4 * kq + j] = oacc[d][j];
    __syncthreads();
    if (tid < DHP + 2 && c0 < len) {
        for (int g = 0; g < ng; ++g) {
            const float M = fmaxf(fmaxf(red[0][g][0], red[1][g][0]), fmaxf(red[2][g][0], red[3][g][0]));
            float v = 0.f, lsum = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const float f = fast_exp2(red[w][g][0] - M);
                v += red[w][g][tid] * f;
                lsum += red[w][g][1] * f;
            }
            if (a.nsplit == 1 && a.out) {
                const int d = tid - 2;
                if (d >= 0 && d < a.dh) {
                    float o = v / lsum;
                    if (a.round_out) o = round_bf16(o);
                    a.out[(size_t)(row0 + g) * a.ldo + h * a.dh + d] = o;
                }
            } else if (fused_merge) {
                __hip_atomic_store(part_of(g) + tid, tid == 0 ? M : v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                part_of(g)[tid] = tid == 0 ? M : v;
            }
        }
    }
    if (fused_merge) {   // see decode_attn_kernel: write-through partials, one ticket per (first row of the tile, head)
        __shared__ int s_last;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            unsigned *cnt = a.tickets + (size_t)row0 * a.H + h;
            const unsigned t = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int last = t == (unsigned)(a.nsplit - 1);
            if (last) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_last = last;
        }
        __syncthreads();
        if (s_last) {
            // wave w merges rows w, w + 4, ...; all partial triples of up to 8 splits are requested before any is used
            const int d = tid & 63;
            for (int g = tid >> 6; g < ng; g += 4) {
                float *pp = a.partial + ((size_t)(row0 + g) * a.H + h) * a.nsplit * (DHP + 2);
                auto ld = [&](int i) { return __hip_atomic_load(pp + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
                float M = -1.0e30f, ls = 0.f, o = 0.f;
                for (int s0 = 0; s0 < a.nsplit; s0 += 8) {
                    float pm[8], pl[8], po[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const bool in = s0 + u < a.nsplit;
                        const int base = (in ? s0 + u : s0) * (DHP + 2);
                        pm[u] = in ? ld(base) : -1.0e30f;
                        pl[u] = in ? ld(base + 1) : 0.f;
                        po[u] = in ? ld(base + 2 + d) : 0.f;
                    }
                    float Mc = M;
#pragma unroll
                    for (int u = 0; u < 8; ++u) Mc = fmaxf(Mc, pm[u]);
                    const float resc = fast_exp2(M - Mc);
                    ls *= resc;
                    o *= resc;
                    M = Mc;
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const float w = fast_exp2(pm[u] - M);
                        ls += pl[u] * w;
                        o += po[u] * w;
                    }
                }
                if (d < a.dh) {
                    float v = o / ls;
                    if (a.round_out) v = round_bf16(v);
                    a.out[(size_t)(row0 + g) * a.ldo + h * a.dh + d] = v;
                }
            }
        }
    }
}

// probe of lane_xor_add / lane_xor_max against the __shfl_xor stage they stand for (acai_debug_lane_xor): one wave per row of 64 values
template <int O, bool MAX>
__global__ __launch_bounds__(64) void lane_xor_probe_kernel(const float *in, float *out, int rows) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const float v = in[(size_t)r * 64 + lane], w = __shfl_xor(v, O);
    float got;
    if constexpr (O == 4) got = MAX ? fmaxf(v, lane_xor4_quad_uniform(v)) : v + lane_xor4_quad_uniform(v);
    else got = MAX ? lane_xor_max<O>(v) : lane_xor_add<O>(v);
    out[(size_t)r * 64 + lane] = got;
    out[((size_t)rows + r) * 64 + lane] = MAX ? fmaxf(v, w) : v + w;
}

// one wave per (b, h): out[b, h*dh + d] = sum_s o_s[d] 2^(m_s - M) / sum_s l_s 2^(m_s - M)
__global__ __launch_bounds__(64) void attn_combine_kernel(const float *partial, float *out, int ldo, int H, int dh, int dhp,
                                                          int nsplit, int round_out) {
    const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
    const float *p = partial + ((size_t)b * H + h) * nsplit * (dhp + 2);
    float M = -1.0e30f;
    for (int s = 0; s < nsplit; ++s) M = fmaxf(M, p[s * (dhp + 2)]);
    float l = 0.f, o = 0.f;
    for (int s = 0; s < nsplit; ++s) {
        const float w = fast_exp2(p[s * (dhp + 2)] - M);
        l += p[s * (dhp + 2) + 1] * w;
        if (d < dhp) o += p[s * (dhp + 2) + 2 + d] * w;
    }
    if (d < dh) {
        float v = o / l;
        if (round_out) v = round_bf16(v);  // SDPA output is bf16 under autocast
        out[(size_t)b * ldo + h * dh + d] = v;
    }
}

// ---- FP8 memory cache: bf16 cross K/V rows -> e4m3fn rows + one power-of-two scale per row -------------------------------------------
// Row r (elements r*dhp .. r*dhp + dhp - 1 of the ragged head-major layout) is owned by a group of LPR = dhp / 16 lanes, 16 elements each
// (32 bytes of bf16 in, 16 bytes of e4m3 out).  amax over the group by shuffles; scale 2^e with e the smallest integer such that
// amax 2^-e <= 448 (frexp: amax = m 2^k, m in [0.5, 1): e = k - 9 + (m > 0.875)), e >= -126 so that 2^e and 2^-e are normal floats; an
// all-zero row gets e = 0.  q = RNE(x 2^-e) by v_cvt_pk_fp8_f32 (OCP e4m3fn on gfx950): both steps are exact but for that one rounding, so
// the format restates bit for bit as torch's `(x.float() * 2^-e).to(torch.float8_e4m3fn)`.
__device__ __forceinline__ float pow2i(int e) { return __int_as_float((e + 127) << 23); }   // -126 <= e <= 127

template <int LPR>
__device__ __forceinline__ void quantize_row_part(const bf16_t *in, uint8_t *out, float *scale, int part) {
    const uint4 w0 = *reinterpret_cast<const uint4 *>(in), w1 = *reinterpret_cast<const uint4 *>(in + 8);
    const uint32_t w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
    float x[16], amax = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        x[2 * i] = __uint_as_float(w[i] << 16);
        x[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
        amax = fmaxf(amax, fmaxf(fabsf(x[2 * i]), fabsf(x[2 * i + 1])));
    }
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    int k = 0;
    const float m = frexpf(amax, &k);
    const int e = amax > 0.f ? max(k - 9 + (m > 0.875f ? 1 : 0), -126) : 0;
    const float inv = pow2i(-e);
    uint32_t q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int v = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * i] * inv, x[4 * i + 1] * inv, 0, false);
        v = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * i + 2] * inv, x[4 * i + 3] * inv, v, true);
        q[i] = (uint32_t)v;
    }
    *reinterpret_cast<uint4 *>(out) = make_uint4(q[0], q[1], q[2], q[3]);
    if (part == 0) *scale = pow2i(e);
}

template <int LPR>
__global__ __launch_bounds__(256) void cross_kv_quantize_fp8_kernel(const bf16_t *kin, const bf16_t *vin, uint8_t *k8, uint8_t *v8, float *ks,
                                                                    float *vs, long long row0, long long nrows) {
    constexpr int DHP = 16 * LPR;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long r = g / LPR;
    const int part = (int)(g % LPR);
    if (r >= nrows) return;   // the lanes of a row exit together (LPR divides 64): the shuffles stay inside live groups
    const size_t row = (size_t)(row0 + r), e0 = row * DHP + part * 16;
    quantize_row_part<LPR>(kin + e0, k8 + e0, ks + row, part);
    quantize_row_part<LPR>(vin + e0, v8 + e0, vs + row, part);
}

}  // namespace

// rollout groups: B rows = B / group images x group rows (bf16, dhp = 64; needs the in-launch merge or a single split)
int launch_dattn_group(const DAttnArgs &a, int B, int group, hipStream_t st) {
    const int gtm = cdiv(group, 16);
    hipLaunchKernelGGL(decode_attn_gmfma_kernel, dim3(a.nsplit, a.H, (B / group) * gtm), dim3(256), 0, st, a, group, gtm);
    ACAI_LAUNCH_CHECK("decode_attn_gmfma");
    return 0;
}

// FP8 memory cache: the RAGGED form only (static and streamed greedy, and the slots' cross attention), dhp 16 / 32 / 64
int launch_dattn_fp8(const DAttnArgs &a, int B, hipStream_t st) {
    if (!a.seq_off || !a.k_scale || !a.v_scale) return acai_set_err(-1, "decode_attn: the FP8 cache form needs ragged offsets and K / V scales");
    dim3 grid(a.nsplit, a.H, B);
    switch (a.dhp) {
        case 16: hipLaunchKernelGGL((decode_attn_kernel<fp8e4m3_t, 1, true>), grid, dim3(256), 0, st, a); break;
        case 32: hipLaunchKernelGGL((decode_attn_kernel<fp8e4m3_t, 2, true>), grid, dim3(256), 0, st, a); break;
        case 64: hipLaunchKernelGGL((decode_attn_kernel<fp8e4m3_t, 4, true>), grid, dim3(256), 0, st, a); break;
        default: return acai_set_err(-1, "decode_attn: FP8 cache dhp=%d unsupported (16, 32 or 64)", a.dhp);
    }
    ACAI_LAUNCH_CHECK("decode_attn_fp8");
    return 0;
}

// The bf16 / fp32 forms.  `spec`: self attention of a speculative verify step (the SPEC instantiation); otherwise the descriptor picks the
// form: ragged offsets = cross attention (RAGGED), per-row lengths without offsets = the slots' ring (SLOT), an ancestor table = a beam
// step (ANC), none = plain self attention.  ANC and SPEC stage their table in LDS, chunk ints.
template <typename TC>
int launch_dattn(const DAttnArgs &a, int B, bool spec, hipStream_t st) {
    const int lpk = a.dhp * (int)sizeof(TC) / 16;
    static const int dattn_u = getenv("ACAI_DATTN_U") ? atoi(getenv("ACAI_DATTN_U")) : 2;   // key groups in flight per lane (A/B aid)
    dim3 grid(a.nsplit, a.H, B);
    const size_t tab = sizeof(int32_t) * a.chunk;
#define ACAI_DA(L)                                                                                        \
    case L:                                                                                               \
        if (spec) hipLaunchKernelGGL((decode_attn_kernel<TC, L, false, 2, false, false, true>), grid, dim3(256), tab, st, a);              \
        else if (a.seq_off && L == 8 && dattn_u == 4) hipLaunchKernelGGL((decode_attn_kernel<TC, 8, true, 4>), grid, dim3(256), 0, st, a);  \
        else if (a.seq_off && L == 8 && dattn_u == 3) hipLaunchKernelGGL((decode_attn_kernel<TC, 8, true, 3>), grid, dim3(256), 0, st, a);  \
        else if (a.seq_off) hipLaunchKernelGGL((decode_attn_kernel<TC, L, true>), grid, dim3(256), 0, st, a);  \
        else if (a.seq_len) hipLaunchKernelGGL((decode_attn_kernel<TC, L, false, 2, false, true>), grid, dim3(256), 0, st, a);             \
        else if (a.anc) hipLaunchKernelGGL((decode_attn_kernel<TC, L, false, 2, true>), grid, dim3(256), tab, st, a);                      \
        else hipLaunchKernelGGL((decode_attn_kernel<TC, L, false>), grid, dim3(256), 0, st, a);           \
        break;
    switch (lpk) {
        ACAI_DA(1) ACAI_DA(2) ACAI_DA(4) ACAI_DA(8) ACAI_DA(16)
        default: return acai_set_err(-1, "decode_attn: dhp=%d unsupported", a.dhp);
    }
#undef ACAI_DA
    ACAI_LAUNCH_CHECK(spec ? "decode_attn_spec" : "decode_attn");
    return 0;
}
template int launch_dattn<float>(const DAttnArgs &, int, bool, hipStream_t);
template int launch_dattn<bf16_t>(const DAttnArgs &, int, bool, hipStream_t);

int launch_attn_combine(const float *partial, float *out, int ldo, int B, int H, int dh, int dhp, int nsplit, int round_out, hipStream_t st) {
    hipLaunchKernelGGL(attn_combine_kernel, dim3(H, B), dim3(64), 0, st, partial, out, ldo, H, dh, dhp, nsplit, round_out);
    ACAI_LAUNCH_CHECK("attn_combine");
    return 0;
}

// The in-launch merge of the split partials (decode_attn_kernel: write-through stores, one agent-scope ticket per (sequence, head), the last
// arriver loads every partial) is a hand-off MEASURED on gfx950 / ROCm 7.2 with this kernel at TWO resident workgroups per CU - not an
// architectural guarantee (MI355X_MICROARCH.md, "Valid forms").  If a toolchain change moves the kernel's register count so that the residency
// is no longer the one it was validated at, the step falls back to the separate combine launch by itself (tickets ignored) instead of running
// the hand-off in a regime nobody tested.  ACAI_DATTN_MERGE=1 / 0 forces either path (A/B aid).
// `kernel` is the RAGGED instantiation of the cache type and lanes-per-key variant asked about (null: no such variant), `cached` its slot,
// [lo, hi] the residency range it was validated at.
static bool dattn_merge_validated(const void *kernel, int &cached, int lo, int hi, int elem_bytes, int lpk) {
    static const int force = getenv("ACAI_DATTN_MERGE") ? atoi(getenv("ACAI_DATTN_MERGE")) : -1;
    if (force >= 0) return force != 0;
    if (!kernel) return false;
    if (cached < 0) {
        int n = 0;
        const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, 256, 0);
        if (getenv("ACAI_DATTN_MERGE_DEBUG"))
            fprintf(stderr, "decode_attn_kernel<%d-byte cache, %d lanes per key>: hipOccupancyMaxActiveBlocksPerMultiprocessor = %d (err %d)\n", elem_bytes, lpk, n, (int)e);
        cached = (e == hipSuccess && n >= lo && n <= hi) ? 1 : 0;
    }
    return cached == 1;
}

bool dattn_merge_in_launch(int dtype, int dhp) {
    static_assert(ACAI_F32 == 0 && ACAI_BF16 == 1 && ACAI_FP8_E4M3 == 2, "the tables below are indexed by dtype");
#define ACAI_RAGGED(TC, L) reinterpret_cast<const void *>(&decode_attn_kernel<TC, L, true>)
    static const void *const kernels[3][5] = {   // [ACAI_F32 / ACAI_BF16 / ACAI_FP8_E4M3][lanes per key: 1, 2, 4, 8, 16]
        {ACAI_RAGGED(float, 1), ACAI_RAGGED(float, 2), ACAI_RAGGED(float, 4), ACAI_RAGGED(float, 8), ACAI_RAGGED(float, 16)},
        {ACAI_RAGGED(bf16_t, 1), ACAI_RAGGED(bf16_t, 2), ACAI_RAGGED(bf16_t, 4), ACAI_RAGGED(bf16_t, 8), ACAI_RAGGED(bf16_t, 16)},
        {ACAI_RAGGED(fp8e4m3_t, 1), ACAI_RAGGED(fp8e4m3_t, 2), ACAI_RAGGED(fp8e4m3_t, 4), nullptr, nullptr}};   // (FP8: dhp 16, 32, 64)
#undef ACAI_RAGGED
    static int cached[3][5] = {{-1, -1, -1, -1, -1}, {-1, -1, -1, -1, -1}, {-1, -1, -1, -1, -1}};
    const int es = dtype == ACAI_FP8_E4M3 ? 1 : dtype == ACAI_BF16 ? 2 : 4, lpk = dhp * es / 16;
    const int idx = lpk == 1 ? 0 : lpk == 2 ? 1 : lpk == 4 ? 2 : lpk == 8 ? 3 : lpk == 16 ? 4 : -1;
    const void *kernel = idx < 0 ? nullptr : kernels[dtype][idx];
    int &slot = cached[dtype][idx < 0 ? 0 : idx];
    // bf16 / fp32: the residency this build was validated at (rounds 2-4: determinism test, 512-step soak, every decode parity test), as the
    // occupancy API reports it on gfx950 / ROCm 7.2: 7 workgroups of 256 threads per CU (the launch itself puts 2 on a CU: 512 workgroups).
    // Round 4's first form of this check compared against 2, the API said 7, and the headline step silently took the separate combine launch
    // (0.712 against 0.689 ms) until the profile showed attn_combine_kernel back in it.
    if (dtype != ACAI_FP8_E4M3) return dattn_merge_validated(kernel, slot, 6, 8, es, lpk);
    // FP8 (its launches, like the bf16 form's, put two workgroups on a CU at the headline shape): this form carries 16 elements per lane
    // (94-104 VGPRs on gfx950 / ROCm 7.2, 4-5 waves per SIMD), so the API reports fewer resident workgroups than the bf16 form's 7; the
    // hand-off was validated with the launch at two workgroups per CU (tests/test_gpu_fp8_memory.py with the merge in the launch,
    // tools/bench_fp8_memory.py): any residency of at least 2 is that regime
    return dattn_merge_validated(kernel, slot, 2, 8, es, lpk);
}
extern "C" int acai_cross_kv_quantize_fp8(const void *k_in, const void *v_in, void *k_out, void *v_out, float *k_scale, float *v_scale,
                                          int64_t row0, int64_t nrows, int dhp, void *stream) {
    ACAI_CHECK_ARG(k_in && v_in && k_out && v_out && k_scale && v_scale, "acai_cross_kv_quantize_fp8: null operand");
    ACAI_CHECK_ARG(row0 >= 0 && nrows >= 0 && (dhp == 16 || dhp == 32 || dhp == 64), "acai_cross_kv_quantize_fp8: bad dims row0=%lld nrows=%lld dhp=%d",
                   (long long)row0, (long long)nrows, dhp);
    ACAI_CHECK_ARG(aligned16(k_in) && aligned16(v_in) && aligned16(k_out) && aligned16(v_out), "acai_cross_kv_quantize_fp8: operands must be 16-byte aligned");
    if (nrows == 0) return 0;
    const int lpr = dhp / 16;
    const dim3 grid((unsigned)((nrows * lpr + 255) / 256));
    hipStream_t st = (hipStream_t)stream;
    auto kin = (const bf16_t *)k_in, vin = (const bf16_t *)v_in;
    auto k8 = (uint8_t *)k_out, v8 = (uint8_t *)v_out;
    if (lpr == 1) hipLaunchKernelGGL(cross_kv_quantize_fp8_kernel<1>, grid, dim3(256), 0, st, kin, vin, k8, v8, k_scale, v_scale, (long long)row0, (long long)nrows);
    else if (lpr == 2) hipLaunchKernelGGL(cross_kv_quantize_fp8_kernel<2>, grid, dim3(256), 0, st, kin, vin, k8, v8, k_scale, v_scale, (long long)row0, (long long)nrows);
    else hipLaunchKernelGGL(cross_kv_quantize_fp8_kernel<4>, grid, dim3(256), 0, st, kin, vin, k8, v8, k_scale, v_scale, (long long)row0, (long long)nrows);
    ACAI_LAUNCH_CHECK("cross_kv_quantize_fp8");
    return 0;
}

extern "C" int acai_decode_attn(const float *q, int ldq, const void *kc, const void *vc, const int64_t *seq_off, const int32_t *seq_len,
                                float *partial, float *out, int ldo, int B, int H, int dh, int dhp, int chunk, int nsplit, int dtype,
                                int round_out, uint32_t *tickets, void *stream) {
    ACAI_CHECK_ARG(q && kc && vc && seq_off && seq_len && partial, "acai_decode_attn: null operand");
    ACAI_CHECK_ARG(B > 0 && H > 0 && dh > 0 && dhp >= dh && dhp <= 64 && (dhp & (dhp - 1)) == 0 && chunk > 0 && nsplit > 0,
                   "acai_decode_attn: bad dims");
    DAttnArgs a{};
    a.q = q; a.kc = kc; a.vc = vc; a.seq_off = seq_off; a.seq_len = seq_len; a.partial = partial;
    a.ldq = ldq; a.H = H; a.dh = dh; a.dhp = dhp; a.chunk = chunk; a.nsplit = nsplit;
    a.scale_log2e = 1.4426950408889634f / sqrtf((float)dh);
    hipStream_t st = (hipStream_t)stream;
    if (tickets && out) {
        a.out = out; a.ldo = ldo; a.round_out = round_out; a.tickets = tickets;
        return dtype == ACAI_BF16 ? launch_dattn<bf16_t>(a, B, false, st) : launch_dattn<float>(a, B, false, st);
    }
    int rc = dtype == ACAI_BF16 ? launch_dattn<bf16_t>(a, B, false, st) : launch_dattn<float>(a, B, false, st);
    if (rc || !out) return rc;  // out == NULL: partials only (lets a benchmark time the streaming kernel alone)
    return launch_attn_combine(partial, out, ldo, B, H, dh, dhp, nsplit, round_out, st);
}

extern "C" int acai_decode_attn_fp8(const float *q, int ldq, const void *kc, const void *vc, const float *k_scale, const float *v_scale,
                                    const int64_t *seq_off, const int32_t *seq_len, float *partial, float *out, int ldo, int B, int H, int dh,
                                    int dhp, int chunk, int nsplit, int round_out, uint32_t *tickets, void *stream) {
    ACAI_CHECK_ARG(q && kc && vc && k_scale && v_scale && seq_off && seq_len && partial, "acai_decode_attn_fp8: null operand");
    ACAI_CHECK_ARG(B > 0 && H > 0 && dh > 0 && dhp >= dh && (dhp == 16 || dhp == 32 || dhp == 64) && chunk > 0 && nsplit > 0,
                   "acai_decode_attn_fp8: bad dims");
    DAttnArgs a{};
    a.q = q; a.kc = kc; a.vc = vc; a.k_scale = k_scale; a.v_scale = v_scale; a.seq_off = seq_off; a.seq_len = seq_len; a.partial = partial;
    a.ldq = ldq; a.H = H; a.dh = dh; a.dhp = dhp; a.chunk = chunk; a.nsplit = nsplit;
    a.scale_log2e = 1.4426950408889634f / sqrtf((float)dh);
    hipStream_t st = (hipStream_t)stream;
    if (tickets && out) {
        a.out = out; a.ldo = ldo; a.round_out = round_out; a.tickets = tickets;
        return launch_dattn_fp8(a, B, st);
    }
    int rc = launch_dattn_fp8(a, B, st);
    if (rc || !out) return rc;
    return launch_attn_combine(partial, out, ldo, B, H, dh, dhp, nsplit, round_out, st);
}

// Test entry: the self-attention forms of a decode step on caller-supplied operands.  The DAttnArgs fields are the ones attend() in
// decode.hip sets for the self case, and the launch goes through launch_dattn, the step's own dispatch.
extern "C" int acai_debug_decode_self_attn(int form, const float *q, int ldq, const void *k_cache, const void *v_cache, const int32_t *step,
                                           const int32_t *row_len, const int32_t *table, int table_pitch, int64_t table_stride, float *partial,
                                           void *out, int ldo, int B, int H, int dh, int dhp, int Tmax, int chunk, int nsplit, int dtype,
                                           int round_out, int out_bf16, uint32_t *tickets, void *stream) {
    const char *fn = "acai_debug_decode_self_attn";
    ACAI_CHECK_ARG(form >= 0 && form <= 3, "%s: form %d is none of 0 plain, 1 ancestor, 2 ring, 3 speculative", fn, form);
    ACAI_CHECK_ARG(q && k_cache && v_cache && partial, "%s: null operand", fn);
    ACAI_CHECK_ARG(form >= 2 || step, "%s: the plain and ancestor forms need step", fn);
    ACAI_CHECK_ARG(form < 2 || row_len, "%s: the ring and speculative forms need row_len", fn);
    ACAI_CHECK_ARG(form == 0 || table, "%s: form %d needs its table", fn, form);
    ACAI_CHECK_ARG(dtype == ACAI_F32 || dtype == ACAI_BF16, "%s: bad dtype", fn);
    ACAI_CHECK_ARG(B > 0 && H > 0 && dh > 0 && dhp >= dh && dhp <= 64 && (dhp & (dhp - 1)) == 0 && dhp * (dtype == ACAI_BF16 ? 2 : 4) >= 16 &&
                       Tmax > 0 && chunk > 0 && nsplit > 0,
                   "%s: bad dims B=%d H=%d dh=%d dhp=%d Tmax=%d chunk=%d nsplit=%d", fn, B, H, dh, dhp, Tmax, chunk, nsplit);
    ACAI_CHECK_ARG((long)chunk * nsplit >= Tmax, "%s: attention split does not cover the cache (chunk %d x nsplit %d < Tmax %d)", fn, chunk,
                   nsplit, Tmax);
    ACAI_CHECK_ARG((form != 1 && form != 3) || chunk <= 16384, "%s: chunk %d above 16384 (the table is staged in LDS)", fn, chunk);
    ACAI_CHECK_ARG((form != 1 && form != 3) || table_pitch > 0, "%s: table_pitch %d", fn, table_pitch);
    ACAI_CHECK_ARG(form != 1 || table_pitch >= Tmax, "%s: ancestor table pitch %d below Tmax %d", fn, table_pitch, Tmax);
    ACAI_CHECK_ARG(form != 3 || (table_stride >= 1 && table_stride <= 8 && B % table_stride == 0),
                   "%s: %lld rows per image (1 .. 8, dividing B=%d)", fn, (long long)table_stride, B);
    ACAI_CHECK_ARG(!out_bf16 || (out && (nsplit == 1 || tickets)), "%s: bf16 rows are written by the attention launch only (out, and one split or tickets)", fn);
    DAttnArgs a{};
    a.q = q; a.kc = k_cache; a.vc = v_cache; a.ldq = ldq; a.H = H; a.dh = dh; a.dhp = dhp; a.Tmax = Tmax;
    a.partial = partial; a.scale_log2e = 1.4426950408889634f / sqrtf((float)dh);
    a.chunk = chunk; a.nsplit = nsplit;
    if (form < 2) a.step = step;
    else a.seq_len = row_len;
    if (form == 1) { a.anc = table; a.anc_pitch = table_pitch; a.anc_bstride = table_stride; }
    if (form == 2) a.slot_first = table;
    if (form == 3) { a.spec_tab = table; a.anc_pitch = table_pitch; a.anc_bstride = table_stride; }
    hipStream_t st = (hipStream_t)stream;
    auto launch = [&]() { return dtype == ACAI_BF16 ? launch_dattn<bf16_t>(a, B, form == 3, st) : launch_dattn<float>(a, B, form == 3, st); };
    if (out && (nsplit == 1 || tickets)) {
        a.out = (float *)out; a.ldo = ldo; a.round_out = round_out; a.out_bf16 = out_bf16 ? 1 : 0;
        if (nsplit > 1) a.tickets = tickets;
        return launch();
    }
    int rc = launch();
    if (rc || !out) return rc;
    return launch_attn_combine(partial, (float *)out, ldo, B, H, dh, dhp, nsplit, round_out, st);
}

// Test entry: acai_decode_attn through the rollout-group kernel (launch_dattn_group, as a step with cross_group > 1 launches it).
extern "C" int acai_debug_decode_attn_group(const float *q, int ldq, const void *kc, const void *vc, const int64_t *seq_off,
                                            const int32_t *seq_len, float *partial, float *out, int ldo, int B, int H, int dh, int dhp,
                                            int chunk, int nsplit, int dtype, int round_out, uint32_t *tickets, int group, void *stream) {
    const char *fn = "acai_debug_decode_attn_group";
    ACAI_CHECK_ARG(q && kc && vc && seq_off && seq_len && partial && out, "%s: null operand", fn);
    ACAI_CHECK_ARG(dtype == ACAI_BF16 && dhp == 64, "%s: the group kernel is bf16 with d_h padded to 64 only", fn);
    ACAI_CHECK_ARG(B > 0 && H > 0 && dh > 0 && dh <= dhp && chunk > 0 && nsplit > 0 && group > 0 && B % group == 0,
                   "%s: bad dims B=%d H=%d dh=%d chunk=%d nsplit=%d group=%d", fn, B, H, dh, chunk, nsplit, group);
    ACAI_CHECK_ARG(nsplit == 1 || tickets, "%s: more than one split needs tickets (the kernel merges inside the launch)", fn);
    DAttnArgs a{};
    a.q = q; a.kc = kc; a.vc = vc; a.seq_off = seq_off; a.seq_len = seq_len; a.partial = partial;
    a.ldq = ldq; a.H = H; a.dh = dh; a.dhp = dhp; a.chunk = chunk; a.nsplit = nsplit;
    a.scale_log2e = 1.4426950408889634f / sqrtf((float)dh);
    a.out = out; a.ldo = ldo; a.round_out = round_out;
    if (nsplit > 1) a.tickets = tickets;
    return launch_dattn_group(a, B, group, (hipStream_t)stream);
}

extern "C" int acai_debug_lane_xor(const float *in, int rows, int offset, int op, float *out, void *stream) {
    ACAI_CHECK_ARG(in && out && rows > 0 && (op == 0 || op == 1), "acai_debug_lane_xor: bad arguments");
    hipStream_t st = (hipStream_t)stream;
#define ACAI_LX(O)                                                                                                  \
    case O:                                                                                                         \
        if (op) hipLaunchKernelGGL((lane_xor_probe_kernel<O, true>), dim3(rows), dim3(64), 0, st, in, out, rows);   \
        else hipLaunchKernelGGL((lane_xor_probe_kernel<O, false>), dim3(rows), dim3(64), 0, st, in, out, rows);     \
        break;
    switch (offset) {
        ACAI_LX(1) ACAI_LX(2) ACAI_LX(4) ACAI_LX(8) ACAI_LX(16) ACAI_LX(32)
        default: return acai_set_err(-1, "acai_debug_lane_xor: offset %d is no butterfly stage of a wave of 64", offset);
    }
#undef ACAI_LX
    ACAI_LAUNCH_CHECK("acai_debug_lane_xor");
    return 0;
}

extern "C" int acai_decode_merge_in_launch(int dtype, int dhp) {
    if (dtype == ACAI_FP8_E4M3)
        ACAI_CHECK_ARG(dhp == 16 || dhp == 32 || dhp == 64, "acai_decode_merge_in_launch: bad FP8 dhp");
    else
        ACAI_CHECK_ARG((dtype == ACAI_BF16 || dtype == ACAI_F32) && dhp > 0 && dhp <= 64 && (dhp & (dhp - 1)) == 0, "acai_decode_merge_in_launch: bad dtype / dhp");
    return dattn_merge_in_launch(dtype, dhp) ? 1 : 0;
}
