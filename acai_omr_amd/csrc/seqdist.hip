// Batched unit-cost Levenshtein distance between ragged token rows that already live in HBM (acai_edit_distance): the token-level edit cost of
// the GRPO reward (train/grpo.py: calc_token_edit_costs) and the numerator of the symbol error rate (utils.symbol_error_rate).
//
// One WAVE per pair, no LDS hand-offs between threads and no barrier in the sweep.  The longer row (m tokens) lies along the 64 lanes: lane l owns
// the W = ceil(m / 64) consecutive columns l*W .. l*W+W-1 and keeps that strip of the previous DP row, and the strip's own tokens, in REGISTERS.
// The shorter row (n tokens, staged once in LDS, narrowed to 32 bits) is walked row by row with the lanes skewed by one step each: at step s lane l
// computes row s - l of its strip, so the only value that crosses lanes is the strip's last cell, which lane l + 1 needs exactly one step later -
// one DPP wave shift (v_mov_b32 wave_shr:1) per step.  n + ceil(m / W) - 1 steps in all.
//
// Cells are kept as D'[i][j] = D[i][j] - j.  That turns the insertion term D[i][j-1] + 1 into a bare D'[i][j-1], so the serial chain through a
// strip is ONE v_min3 per cell; the other two terms (D'[i-1][j] + 1, D'[i-1][j-1] - [a_i == b_j]) depend on the previous row only and issue ahead
// of it.  Four VALU instructions per cell.
//
// Why not the anti-diagonal sweep over LDS with a workgroup per pair: it pays a workgroup barrier and three LDS accesses per cell on each of the
// n + m diagonals (2,300 for a 768 x 1536 pair), and with R = 128 independent pairs the chip is short of waves either way - the quantity that
// matters is the latency of ONE pair, which is barriers x diagonals there and (VALU chain) x steps here.  A bit-parallel (Myers) form needs a
// per-token match mask of m bits; token ids are arbitrary 31-bit values, so the masks would have to be built per pair (a hash of up to 4096
// distinct ids), or compared on the fly at the DP's own cost.
//
// W is chosen on the device from the lengths (they are read there: no host sync) out of {1, 2, 4, 8, 12, 16, 24, 32, 48, 64}; every choice is its
// own fully unrolled instantiation, so strips index registers statically.  Columns past m (the padding of the last strip) hold a sentinel token and
// never feed a column to their left.  Token ids are compared as their low 32 bits: exact for ids in [0, 2^31).
// Lengths are clamped to [0, ld] on the device, so no length read from memory can index outside its row.
//
// Measured figures: DESIGN.md section 6 (tools/bench_edit_distance.py, profiles/edit_distance_bench.json).
#include "common.h"

namespace {

constexpr int SEQDIST_MAX = 4096;   // longest row on either side: 64 lanes x 64 columns
constexpr int SEQDIST_PAD = 64;     // LDS slack on either side of the staged row: lanes outside [0, n) read (and ignore) it

// lane l receives lane l-1's value (lane 0 keeps its own): DPP wave_shr:1
__device__ __forceinline__ int wave_shr1(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xF, 0xF, false); }

// D[n][m] of b = lng[0..m) (along the lanes) against a = sh[0..n) (in LDS); 1 <= n <= m <= 64 * W.  Every lane returns the distance.
template <int W>
__device__ __forceinline__ int strip_sweep(const int64_t *__restrict__ lng, int m, const int *sh, int n, int lane) {
    int pat[W], prev[W];
#pragma unroll
    for (int c = 0; c < W; ++c) {
        const int j = lane * W + c;
        pat[c] = j < m ? (int)lng[j] : -1;
        prev[c] = 0;   // D'[0][j] = D[0][j] - j = 0
    }
    const int steps = n + (m + W - 1) / W - 1;
    int last = 0;   // D'[row][l*W + W - 1] of the row this lane finished last
    int diag0 = 0;  // D'[row - 1][l*W - 1]: what came in from the left one step ago
    int tok = sh[-lane];
    for (int s = 0; s < steps; ++s) {
        const int in = wave_shr1(last);
        const int row = s - lane + 1;           // 1-based DP row of this lane at this step
        const int tok_next = sh[s + 1 - lane];  // (independent of the chain below: in flight while it runs)
        const int left0 = lane == 0 ? row : in; // column 0: D'[row][0] = row
        if (row >= 1 && row <= n) {
            int left = left0, diag = lane == 0 ? row - 1 : diag0;
#pragma unroll
            for (int c = 0; c < W; ++c) {
                const int up = prev[c];
                const int t = min(up + 1, diag - (tok == pat[c] ? 1 : 0));
                left = min(t, left);
                diag = up;
                prev[c] = left;
            }
            last = left;
        }
        diag0 = left0;
        tok = tok_next;
    }
    // the lane that owns column m holds D'[n][m] in a register chosen by a select chain (no dynamic register index)
    const int own = (m - 1) / W, idx = (m - 1) - own * W;
    int v = 0;
#pragma unroll
    for (int c = 0; c < W; ++c) v = c == idx ? prev[c] : v;
    return __shfl(v, own, 64) + m;
}

__global__ __launch_bounds__(64) void edit_distance_kernel(const int64_t *__restrict__ pred, int ld_pred, const int32_t *__restrict__ pred_len,
                                                           const int64_t *__restrict__ tgt, int ld_tgt, const int32_t *__restrict__ tgt_len, int group,
                                                           int32_t *__restrict__ out) {
    __shared__ int tokbuf[SEQDIST_MAX + 2 * SEQDIST_PAD];
    const int r = blockIdx.x, g = r / group, lane = threadIdx.x;
    const int lp = min(max(pred_len[r], 0), ld_pred), lt = min(max(tgt_len[g], 0), ld_tgt);
    const int64_t *prow = pred + (size_t)r * ld_pred, *trow = tgt + (size_t)g * ld_tgt;
    const bool pred_long = lp >= lt;
    const int64_t *lng = pred_long ? prow : trow, *sht = pred_long ? trow : prow;
    const int m = pred_long ? lp : lt, n = pred_long ? lt : lp;
    if (n == 0) {   // (uniform over the workgroup)
        if (lane == 0) out[r] = m;
        return;
    }
    int *sh = tokbuf + SEQDIST_PAD;
    for (int i = lane; i < n; i += 64) sh[i] = (int)sht[i];
    __syncthreads();
    const int w = (m + 63) >> 6;
    int d;
    if (w <= 1) d = strip_sweep<1>(lng, m, sh, n, lane);
    else if (w <= 2) d = strip_sweep<2>(lng, m, sh, n, lane);
    else if (w <= 4) d = strip_sweep<4>(lng, m, sh, n, lane);
    else if (w <= 8) d = strip_sweep<8>(lng, m, sh, n, lane);
    else if (w <= 12) d = strip_sweep<12>(lng, m, sh, n, lane);
    else if (w <= 16) d = strip_sweep<16>(lng, m, sh, n, lane);
    else if (w <= 24) d = strip_sweep<24>(lng, m, sh, n, lane);
    else if (w <= 32) d = strip_sweep<32>(lng, m, sh, n, lane);
    else if (w <= 48) d = strip_sweep<48>(lng, m, sh, n, lane);
    else d = strip_sweep<64>(lng, m, sh, n, lane);
    if (lane == 0) out[r] = d;
}

}  // namespace

extern "C" int acai_edit_distance(const int64_t *pred, int ld_pred, const int32_t *pred_len, const int64_t *tgt, int ld_tgt, const int32_t *tgt_len,
                                  int R, int group, int32_t *out, void *stream) {
    ACAI_CHECK_ARG(pred_len && tgt_len && out && R > 0 && group > 0 && R % group == 0 && ld_pred >= 0 && ld_tgt >= 0 && (pred || ld_pred == 0) &&
                   (tgt || ld_tgt == 0), "acai_edit_distance: bad arguments");
    ACAI_CHECK_ARG(ld_pred <= SEQDIST_MAX && ld_tgt <= SEQDIST_MAX, "acai_edit_distance: rows longer than %d tokens (ld_pred %d, ld_tgt %d)", SEQDIST_MAX,
                   ld_pred, ld_tgt);
    hipLaunchKernelGGL(edit_distance_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, pred, ld_pred, pred_len, tgt, ld_tgt, tgt_len, group, out);
    ACAI_LAUNCH_CHECK("acai_edit_distance");
    return 0;
}
