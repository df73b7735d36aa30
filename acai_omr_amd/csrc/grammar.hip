// Walks finished token rows through a token automaton (acai_grammar_scan): violation counts and the "ended with an allowed <eos>" flag that
// the GRPO well-formedness reward is made of (train/grpo.py: token_reward_rollouts with a grammar; the CPU statement is
// grammar.TokenAutomaton.violations).  The decode-step side of the same table is in decode_select.hip (grammar_row / grammar_advance).
//
// A row is a serial chain - the state after token p is the table entry at (state after p - 1, token p) - so one THREAD walks one row and the
// rows run in parallel.  What the chain waits for at every link is one table read, so the table is staged in LDS when it fits (a bigram
// automaton at V = 227: 227 x 227 x 2 = 103 KB of gfx950's 160 KB): an LDS read in place of an L2 / HBM one per token.  A larger table is read
// from global memory where it lies.  The tokens do not depend on the chain: every thread loads eight ahead.
//
// R is small against the chip (128 rollouts per update), and a workgroup that stages 100 KB can hold no second one on its CU anyway, so rows
// are spread over as many workgroups as there are CUs before a workgroup takes more than one row; all 256 threads stage, the first rpb walk.
// Lengths are read on the device and clamped to [0, ld]; token ids outside [0, V) never index the table; every state read from the tables is
// clamped to [0, states), so no table content can make the walk leave the tables.  Integer arithmetic, no atomics.
#include "common.h"

namespace {

constexpr int GRAMMAR_LDS_BYTES = 156 * 1024;   // of 160 KB: the table of the LDS form may take this much (the launch has no other LDS use)
constexpr int GRAMMAR_ROWS_MAX = 64;            // rows per workgroup at most (one wave walks)
constexpr int GRAMMAR_CUS = 256;                // workgroups to fill before one takes a second row

template <bool LDS>
__global__ __launch_bounds__(256) void grammar_scan_kernel(const int64_t *__restrict__ tokens, int ld, const int32_t *__restrict__ lens, int R, int rpb,
                                                           const int16_t *__restrict__ next, const int16_t *__restrict__ resync, int states, int start,
                                                           int V, int eos, int32_t *__restrict__ violations, int32_t *__restrict__ complete) {
    extern __shared__ __attribute__((aligned(16))) unsigned char scan_lds[];
    const int16_t *tab = next;
    if constexpr (LDS) {
        int16_t *l = reinterpret_cast<int16_t *>(scan_lds);
        const int n = states * V, n8 = ((reinterpret_cast<uintptr_t>(next) & 15) == 0) ? n / 8 : 0;   // 16-byte copies of an aligned table
        for (int i = threadIdx.x; i < n8; i += 256) reinterpret_cast<uint4 *>(l)[i] = reinterpret_cast<const uint4 *>(next)[i];
        for (int i = n8 * 8 + threadIdx.x; i < n; i += 256) l[i] = next[i];
        __syncthreads();
        tab = l;
    }
    const int r = blockIdx.x * rpb + threadIdx.x;
    if ((int)threadIdx.x >= rpb || r >= R) return;
    const int len = min(max(lens[r], 0), ld);
    const int64_t *row = tokens + (size_t)r * ld;
    int s = start, viol = 0, ended = 0;
    for (int p0 = 1; p0 < len; p0 += 8) {
        int64_t k[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) k[j] = p0 + j < len ? row[p0 + j] : -1;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (p0 + j >= len) break;
            const bool inside = k[j] >= 0 && k[j] < V;
            const int tok = inside ? (int)k[j] : 0;
            int n = -1;
            if constexpr (LDS) {
                if (inside) n = tab[s * V + tok];   // (states * V * 2 bytes fit the LDS: a 32-bit index)
            } else {
                if (inside) n = tab[(size_t)s * V + tok];
            }
            const bool ok = n >= 0;
            viol += ok ? 0 : 1;
            s = ok ? n : (inside ? max((int)resync[tok], 0) : start);
            s = min(s, states - 1);
            ended = ok && tok == eos;   // (the last position's value stands)
        }
    }
    violations[r] = viol;
    complete[r] = (len >= 2 && ended) ? 1 : 0;
}

}  // namespace

extern "C" int acai_grammar_scan(const int64_t *tokens, int ld, const int32_t *lens, int R, const int16_t *next, const int16_t *resync, int states,
                                 int start, int V, int eos, int32_t *violations, int32_t *complete, void *stream) {
    ACAI_CHECK_ARG(lens && next && resync && violations && complete && R > 0 && ld >= 0 && (tokens || ld == 0), "acai_grammar_scan: bad arguments");
    ACAI_CHECK_ARG(states >= 1 && states <= 32767 && start >= 0 && start < states && V >= 1 && V <= 65536,
                   "acai_grammar_scan: needs 1 <= states <= 32767, 0 <= start < states, 1 <= V <= 65536 (states=%d start=%d V=%d)", states, start, V);
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes = (size_t)states * V * sizeof(int16_t);
    const int rpb = min(GRAMMAR_ROWS_MAX, cdiv(R, GRAMMAR_CUS));
    const dim3 grid(cdiv(R, rpb));
    if (bytes <= (size_t)GRAMMAR_LDS_BYTES) {
        static bool attr_done[ACAI_MAX_DEV] = {};
        if (acai_first_on_device(attr_done))   // opt in to > 64 KB of dynamic LDS; per device
            hipFuncSetAttribute(reinterpret_cast<const void *>(grammar_scan_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, GRAMMAR_LDS_BYTES);
        hipLaunchKernelGGL(grammar_scan_kernel<true>, grid, dim3(256), (bytes + 15) & ~(size_t)15, st, tokens, ld, lens, R, rpb, next, resync, states,
                           start, V, eos, violations, complete);
    } else {
        hipLaunchKernelGGL(grammar_scan_kernel<false>, grid, dim3(256), 0, st, tokens, ld, lens, R, rpb, next, resync, states, start, V, eos,
                           violations, complete);
    }
    ACAI_LAUNCH_CHECK("acai_grammar_scan");
    return 0;
}
