// The loop guard's rule over finished token rows (acai_repeat_scan; the rule is stated at AcaiLoop in acai_omr_hip.h, the CPU statement is
// tests/loop_reference.py).  The decode-step side of the same rule is in decode_select.hip (loop_check): there a step updates the counters
// of one index, here a wave sweeps a whole row - rows of any decode mode (beam, speculative, sampled rollouts) after the fact, and metrics.
//
// One wave per row, four rows to a workgroup.  Lane p - 1 owns period p and keeps run_p, the length of the run of indices i ending at t
// with seq[i] == seq[i - p], in a register.  The run is a serial chain over t, but what it consumes - the comparisons - is not: the wave
// loads and compares eight indices ahead (two reads of the row per index, both consecutive addresses over the lanes), then walks the eight
// verdicts, one ballot each.  The first ballot with a set bit ends the sweep; its lowest bit is the smallest period.  The lanes then look
// 64 indices at a time for the first index that breaks that period.
// Lengths are read on the device and clamped to [0, ld]; every index read lies in [1, len).  Integer arithmetic, no atomics, no LDS.
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void repeat_scan_kernel(const int64_t *__restrict__ tokens, const int32_t *__restrict__ lens, int N, int ld, int P,
                                                          int R, int M, int32_t *__restrict__ stop, int32_t *__restrict__ period,
                                                          int32_t *__restrict__ start, int32_t *__restrict__ end) {
    const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;   // wave-uniform
    const int len = lens ? min(max(lens[n], 0), ld) : ld;
    const int64_t *row = tokens + (size_t)n * ld;
    const int p = lane + 1;
    const int need = max((R - 1) * p, M);   // (R, M <= ld + 1: the host clamps them; M >= 1, so a run of 0 never fires)
    int run = 0, st = 0, per = 0;
    for (int t0 = 2; t0 < len && !per; t0 += 8) {   // (the first index with a partner at or after index 1 is 2)
        bool same[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int t = t0 + j;
            const bool cmp = t < len && p <= P && t - p >= 1;
            same[j] = cmp && row[t - p] == row[t];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            run = same[j] ? run + 1 : 0;
            const unsigned long long hit = __ballot(run >= need);
            if (hit) {   // wave-uniform
                per = __builtin_ctzll(hit) + 1;
                st = t0 + j;
                break;
            }
        }
    }
    int first = 0, last = 0;
    if (per) {
        const int nd = max((R - 1) * per, M);
        first = st - nd - per + 1;
        last = st;
        for (int base = st + 1; base < len; base += 64) {   // (i - per >= st + 1 - per >= 1)
            const int i = base + lane;
            const bool broken = i >= len || row[i] != row[i - per];
            const unsigned long long m = __ballot(broken);
            if (m) {
                last = base + __builtin_ctzll(m) - 1;
                break;
            }
            last = base + 63;
        }
    }
    if (lane == 0) {
        stop[n] = st;
        period[n] = per;
        start[n] = first;
        end[n] = last;
    }
}

}  // namespace

extern "C" int acai_repeat_scan(const int64_t *tokens, const int32_t *lens, int N, int ld, int max_period, int min_repeats, int min_tokens,
                                int32_t *stop, int32_t *period, int32_t *start, int32_t *end, void *stream) {
    ACAI_CHECK_ARG(stop && period && start && end && N > 0 && ld >= 0 && ld <= (1 << 24) && (tokens || ld == 0),
                   "acai_repeat_scan: bad arguments (N=%d ld=%d)", N, ld);
    ACAI_CHECK_ARG(max_period >= 1 && max_period <= 64, "acai_repeat_scan: max_period %d outside [1, 64]", max_period);
    ACAI_CHECK_ARG(min_repeats >= 2, "acai_repeat_scan: min_repeats %d below 2", min_repeats);
    ACAI_CHECK_ARG(min_tokens >= 1, "acai_repeat_scan: min_tokens %d below 1", min_tokens);
    const int top = ld + 1;   // a need above the row never fires: clamped so that need(p) fits an int
    hipLaunchKernelGGL(repeat_scan_kernel, dim3(cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, tokens, lens, N, ld, max_period,
                       min(min_repeats, top), min(min_tokens, top), stop, period, start, end);
    ACAI_LAUNCH_CHECK("acai_repeat_scan");
    return 0;
}
