// Batched edit ALIGNMENT between ragged token rows in HBM (acai_edit_align): which pred tokens match, which are substituted or inserted, which
// target tokens are deleted, and where - the traceback that the distance kernel (seqdist.hip) does not keep.  utils.symbol_error_breakdown,
// utils.token_confusions and ViTOMR.error_maps are built on it.
//
// One WAVE per pair, in two phases of one launch.
//
// Forward: seqdist.hip's sweep - the longer row (m tokens) in W register columns per lane, the shorter (n tokens, in LDS) walked row by row with
// the lanes skewed by one step, one DPP wave shift per step, cells kept as D' = D - j.  While a cell is computed from its three candidates it
// also yields two DIRECTION BITS: "the diagonal does not attain the minimum" and "the insertion neighbour does not attain it" - all the
// canonical traceback needs to choose its move from that cell with the contract's priority (diagonal, then insertion, then deletion); whether
// a diagonal move is a match or a substitution the walk reads off the two tokens.  Both bits are differences of values the cell has anyway
// (see align_sweep): 9 VALU instructions per cell against the distance kernel's 4.  Which of "left" / "up" is the insertion neighbour depends
// on which side lies along the lanes: pred along the lanes makes "left" (one pred token fewer) the insertion, target along the lanes makes it
// "up" - a template parameter, so the unrolled strips carry no select for it.  The bits of a strip are packed into
// ceil(2W / 32) words per lane and stored to the workspace at [step][word][lane]: the 64 lanes of one step write consecutive dwords (a lane's
// DP row is step - lane + 1, so a row-major table would scatter every store over 64 lines).
//
// Traceback: a serial walk of at most n + m moves from (n, m).  The word of cell (row, column in lane l) lies at step row - 1 + l, and that step
// never grows along the path (up: -1, left: 0 or -1, diagonal: -1 or -2), so the path is served by a window that slides down over the steps: the
// wave fetches 16 KiB of consecutive steps at a time, coalesced, into LDS, with the window below it already in flight in registers while the
// walk runs.  Every value of the walk is wave-uniform (three independent LDS reads and a handful of scalar instructions per move); lane 0
// writes the outputs with plain vector stores.  The ends - the run of insertions or deletions left when one side is used up, and the -1 fill
// past each length - are written by all lanes.
//
// Lengths are clamped to [0, ld] on the device; every workspace index derives from the clamped lengths: step < n + 63 <= min(ld) + 63 and the
// words per step from W(m) <= W(max(ld)), which is what acai_edit_align_workspace_bytes sizes a pair's slice by.  No atomics: bit-reproducible.
//
// Register / scratch use and measured figures: DESIGN.md sections 5 and 6 (tools/bench_edit_alignment.py, profiles/edit_alignment_bench.json).
#include "common.h"

namespace {

constexpr int SEQALIGN_MAX = 4096;     // longest row on either side: 64 lanes x 64 columns
constexpr int SEQALIGN_PAD = 64;       // LDS slack on either side of the staged row: lanes outside [0, n) read (and ignore) it
constexpr int SEQALIGN_WIN = 4096;     // dwords of the traceback window in LDS (16 KiB)
constexpr int SEQALIGN_WIN_Q = SEQALIGN_WIN / 4 / 64;   // uint4 loads per lane and window

// strip width for a longer row of w = ceil(m / 64) columns per lane, and the direction words a lane stores per DP row
__host__ __device__ inline int align_strip_width(int w) {
    return w <= 1 ? 1 : w <= 2 ? 2 : w <= 4 ? 4 : w <= 8 ? 8 : w <= 12 ? 12 : w <= 16 ? 16 : w <= 24 ? 24 : w <= 32 ? 32 : w <= 48 ? 48 : 64;
}
__host__ __device__ inline int align_dir_words(int W) { return (2 * W + 31) / 32; }

// dwords of one pair's workspace slice for rows of at most ld_pred / ld_tgt tokens
inline size_t align_pair_dwords(int ld_pred, int ld_tgt) {
    const int nmax = ld_pred < ld_tgt ? ld_pred : ld_tgt, mmax = ld_pred < ld_tgt ? ld_tgt : ld_pred;
    return (size_t)(nmax + 63) * align_dir_words(align_strip_width((mmax + 63) >> 6)) * 64;
}

// lane l receives lane l-1's value (lane 0 keeps its own): DPP wave_shr:1
__device__ __forceinline__ int wave_shr1(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xF, 0xF, false); }

// The DP of b = lng[0..m) (along the lanes) against a = sh[0..n) (in LDS), 1 <= n <= m <= 64 * W, writing every cell's direction bits:
// ws[(step * NW + word) * 64 + lane]; word k holds the strip's columns 16 k .. min(16 k + 16, W) - 1, the FIRST of them in the highest of the
// used bit pairs (the word is shifted left by two per cell).  INS_LEFT: "left" is the insertion neighbour (pred lies along the lanes).
// Per cell (D' = D - j): t1 = up + 1, t2 = diag - [tokens equal], cell = min3(t1, t2, left).  Neighbouring Levenshtein cells differ by at most
// one, so t2 - cell is 0 or 1 - it IS the "diagonal does not attain the minimum" bit - and ins - cell is 0, 1 or 2.  (The columns past m hold
// a sentinel token: they are cells of a real table too, that of the row extended by sentinels, so their bits cannot spill into a neighbour's.)
template <int W, bool INS_LEFT>
__device__ __forceinline__ void align_sweep(const int64_t *__restrict__ lng, int m, const int *sh, int n, int lane, unsigned *__restrict__ ws) {
    constexpr int NW = (2 * W + 31) / 32;
    int pat[W], prev[W];
#pragma unroll
    for (int c = 0; c < W; ++c) {
        const int j = lane * W + c;
        pat[c] = j < m ? (int)lng[j] : -1;
        prev[c] = 0;   // D'[0][j] = D[0][j] - j = 0
    }
    const int steps = n + (m + W - 1) / W - 1;
    const bool owns = lane * W < m;   // (lanes past the row's end compute padding only: nothing of theirs is ever read)
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
            unsigned dirs[NW];
#pragma unroll
            for (int k = 0; k < NW; ++k) dirs[k] = 0;
#pragma unroll
            for (int c = 0; c < W; ++c) {
                const int up = prev[c];
                const int ne = (int)min((unsigned)(tok ^ pat[c]), 1u);
                const int t1 = up + 1, t2 = diag + ne - 1;
                const int cell = min(min(t1, t2), left);
                const int no_diag = t2 - cell;                                   // 0 or 1
                const int no_ins = min((INS_LEFT ? left : t1) - cell, 1);        // 0 or 1
                dirs[c >> 4] = (dirs[c >> 4] << 2) | (unsigned)(no_ins * 2 + no_diag);
                left = cell;
                diag = up;
                prev[c] = cell;
            }
            last = left;
            if (owns) {
#pragma unroll
                for (int k = 0; k < NW; ++k) ws[(s * NW + k) * 64 + lane] = dirs[k];
            }
        }
        diag0 = left0;
        tok = tok_next;
    }
}

template <bool INS_LEFT>
__device__ __forceinline__ void align_sweep_any(int W, const int64_t *__restrict__ lng, int m, const int *sh, int n, int lane,
                                                unsigned *__restrict__ ws) {
    switch (W) {
        case 1: align_sweep<1, INS_LEFT>(lng, m, sh, n, lane, ws); break;
        case 2: align_sweep<2, INS_LEFT>(lng, m, sh, n, lane, ws); break;
        case 4: align_sweep<4, INS_LEFT>(lng, m, sh, n, lane, ws); break;
        case 8: align_sweep<8, INS_LEFT>(lng, m, sh, n, lane, ws); break;
        case 12: align_sweep<12, INS_LEFT>(lng, m, sh, n, lane, ws); break;
        case 16: align_sweep<16, INS_LEFT>(lng, m, sh, n, lane, ws); break;
        case 24: align_sweep<24, INS_LEFT>(lng, m, sh, n, lane, ws); break;
        case 32: align_sweep<32, INS_LEFT>(lng, m, sh, n, lane, ws); break;
        case 48: align_sweep<48, INS_LEFT>(lng, m, sh, n, lane, ws); break;
        default: align_sweep<64, INS_LEFT>(lng, m, sh, n, lane, ws); break;
    }
}

// uint4 number q of the window whose first dword is ws[base] (base may be negative below step 0: those granules are skipped, never read)
__device__ __forceinline__ uint4 align_fetch(const unsigned *__restrict__ ws, int base, int q, int nq) {
    uint4 v = make_uint4(0, 0, 0, 0);
    const int g = base + 4 * q;
    if (q < nq && g >= 0) v = *reinterpret_cast<const uint4 *>(ws + g);
    return v;
}

__global__ __launch_bounds__(64) void edit_align_kernel(const int64_t *__restrict__ pred, int ld_pred, const int32_t *__restrict__ pred_len,
                                                        const int64_t *__restrict__ tgt, int ld_tgt, const int32_t *__restrict__ tgt_len, int group,
                                                        int32_t *__restrict__ counts, int8_t *__restrict__ pred_op,
                                                        int32_t *__restrict__ pred_to_tgt, int32_t *__restrict__ tgt_to_pred,
                                                        int32_t *__restrict__ tgt_slot, unsigned *__restrict__ workspace, size_t pair_dwords) {
    __shared__ int tokbuf[SEQALIGN_MAX + 2 * SEQALIGN_PAD];
    __shared__ int longbuf[SEQALIGN_MAX];   // the longer row's tokens, for the traceback (the sweep holds them in registers)
    __shared__ uint4 win4[SEQALIGN_WIN / 4];
    const int r = blockIdx.x, g = r / group, lane = threadIdx.x;
    const int lp = min(max(pred_len[r], 0), ld_pred), lt = min(max(tgt_len[g], 0), ld_tgt);
    const int64_t *prow = pred + (size_t)r * ld_pred, *trow = tgt + (size_t)g * ld_tgt;
    int8_t *op = pred_op + (size_t)r * ld_pred;
    int32_t *p2t = pred_to_tgt + (size_t)r * ld_pred, *t2p = tgt_to_pred + (size_t)r * ld_tgt, *slot = tgt_slot + (size_t)r * ld_tgt;
    const bool pred_long = lp >= lt;
    const int64_t *lng = pred_long ? prow : trow, *sht = pred_long ? trow : prow;
    const int m = pred_long ? lp : lt, n = pred_long ? lt : lp;
    int n_match = 0, n_sub = 0, n_ins = 0, n_del = 0;
    int ip = lp, jt = lt;   // the walk's position: pred tokens / target tokens still to be explained
    if (n > 0) {            // (uniform over the workgroup)
        unsigned *ws = workspace + (size_t)r * pair_dwords;
        int *sh = tokbuf + SEQALIGN_PAD;
        for (int i = lane; i < n; i += 64) sh[i] = (int)sht[i];
        for (int j = lane; j < m; j += 64) longbuf[j] = (int)lng[j];
        __syncthreads();
        const int W = align_strip_width((m + 63) >> 6), NW = align_dir_words(W);
        if (pred_long) align_sweep_any<true>(W, lng, m, sh, n, lane, ws);
        else align_sweep_any<false>(W, lng, m, sh, n, lane, ws);
        // the direction words were written by this wave through global memory: complete the stores and drop stale lines before reading them back
        __threadfence();
        __syncthreads();

        // ---- traceback ----
        unsigned *win = reinterpret_cast<unsigned *>(win4);
        const int step_dw = NW * 64;                    // dwords per step
        const int B = SEQALIGN_WIN / step_dw;           // steps per window (16 .. 64)
        const int nq = B * step_dw / 4;                 // uint4 granules per window (<= SEQALIGN_WIN / 4)
        int row = n, col = m;                           // sweep coordinates: row over the shorter side, col over the longer
        int l = (m - 1) / W, c = (m - 1) - l * W;       // lane and strip column of col
        int lo = row + l - B;                           // the window holds steps [lo, lo + B); the first need is step row - 1 + l
        uint4 nxt[SEQALIGN_WIN_Q];
#pragma unroll
        for (int q = 0; q < SEQALIGN_WIN_Q; ++q) win4[q * 64 + lane] = align_fetch(ws, lo * step_dw, q * 64 + lane, nq);
#pragma unroll
        for (int q = 0; q < SEQALIGN_WIN_Q; ++q) nxt[q] = align_fetch(ws, (lo - B) * step_dw, q * 64 + lane, nq);
        __syncthreads();
        while (row > 0 && col > 0) {
            const int s = row - 1 + l;
            while (s < lo) {   // slide the window down: the granules fetched ahead go to LDS, the window below them is requested
                lo -= B;
#pragma unroll
                for (int q = 0; q < SEQALIGN_WIN_Q; ++q) win4[q * 64 + lane] = nxt[q];
#pragma unroll
                for (int q = 0; q < SEQALIGN_WIN_Q; ++q) nxt[q] = align_fetch(ws, (lo - B) * step_dw, q * 64 + lane, nq);
                __syncthreads();
            }
            // the cell's direction bits, and the two tokens in case the move is diagonal (three independent LDS reads)
            const int k = c >> 4, hi = min(16 * k + 16, W);
            const unsigned word = (unsigned)__builtin_amdgcn_readfirstlane((int)win[((s - lo) * NW + k) * 64 + l]);
            const bool equal = __builtin_amdgcn_readfirstlane(sh[row - 1]) == __builtin_amdgcn_readfirstlane(longbuf[col - 1]);
            const unsigned bits = (word >> (2 * (hi - 1 - c))) & 3u;   // bit 0: the diagonal does not attain; bit 1: nor does the insertion
            ip = pred_long ? col : row;
            jt = pred_long ? row : col;
            bool dec_row, dec_col;
            if (!(bits & 1u)) {   // diagonal: pred token ip - 1 stands for target token jt - 1
                if (lane == 0) {
                    op[ip - 1] = equal ? 0 : 1;
                    p2t[ip - 1] = jt - 1;
                    t2p[jt - 1] = ip - 1;
                    slot[jt - 1] = ip - 1;
                }
                n_match += equal;
                n_sub += !equal;
                dec_row = dec_col = true;
            } else if (!(bits & 2u)) {   // insertion: pred token ip - 1 is extra
                if (lane == 0) {
                    op[ip - 1] = 2;
                    p2t[ip - 1] = -1;
                }
                ++n_ins;
                dec_row = !pred_long;
                dec_col = pred_long;
            } else {   // deletion: target token jt - 1 is missing in front of pred token ip
                if (lane == 0) {
                    t2p[jt - 1] = -1;
                    slot[jt - 1] = ip;
                }
                ++n_del;
                dec_row = pred_long;
                dec_col = !pred_long;
            }
            if (dec_row) --row;
            if (dec_col) {
                --col;
                if (--c < 0) {
                    c = W - 1;
                    --l;
                }
            }
        }
        ip = pred_long ? col : row;
        jt = pred_long ? row : col;
    }
    // one side is used up: what is left of pred is inserted, what is left of the target is deleted in front of pred token 0
    for (int i = lane; i < ip; i += 64) {
        op[i] = 2;
        p2t[i] = -1;
    }
    for (int j = lane; j < jt; j += 64) {
        t2p[j] = -1;
        slot[j] = 0;
    }
    n_ins += ip;
    n_del += jt;
    for (int i = lp + lane; i < ld_pred; i += 64) {
        op[i] = -1;
        p2t[i] = -1;
    }
    for (int j = lt + lane; j < ld_tgt; j += 64) {
        t2p[j] = -1;
        slot[j] = -1;
    }
    if (lane == 0) {
        int32_t *cnt = counts + (size_t)r * 4;
        cnt[0] = n_match;
        cnt[1] = n_sub;
        cnt[2] = n_ins;
        cnt[3] = n_del;
    }
}

}  // namespace

extern "C" size_t acai_edit_align_workspace_bytes(int ld_pred, int ld_tgt, int rows) {
    if (ld_pred < 0 || ld_tgt < 0 || rows <= 0 || ld_pred > SEQALIGN_MAX || ld_tgt > SEQALIGN_MAX) return 0;
    return align_pair_dwords(ld_pred, ld_tgt) * sizeof(unsigned) * (size_t)rows;
}

extern "C" int acai_edit_align(const int64_t *pred, int ld_pred, const int32_t *pred_len, const int64_t *tgt, int ld_tgt, const int32_t *tgt_len,
                               int R, int group, int32_t *counts, int8_t *pred_op, int32_t *pred_to_tgt, int32_t *tgt_to_pred, int32_t *tgt_slot,
                               void *workspace, size_t workspace_bytes, void *stream) {
    ACAI_CHECK_ARG(pred_len && tgt_len && counts && R > 0 && group > 0 && R % group == 0 && ld_pred >= 0 && ld_tgt >= 0 && (pred || ld_pred == 0) &&
                   (tgt || ld_tgt == 0), "acai_edit_align: bad arguments");
    ACAI_CHECK_ARG(((pred_op && pred_to_tgt) || ld_pred == 0) && ((tgt_to_pred && tgt_slot) || ld_tgt == 0), "acai_edit_align: missing output");
    ACAI_CHECK_ARG(ld_pred <= SEQALIGN_MAX && ld_tgt <= SEQALIGN_MAX, "acai_edit_align: rows longer than %d tokens (ld_pred %d, ld_tgt %d)", SEQALIGN_MAX,
                   ld_pred, ld_tgt);
    const size_t need = acai_edit_align_workspace_bytes(ld_pred, ld_tgt, R);
    ACAI_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0, "acai_edit_align: the workspace must be a 16-byte aligned device pointer");
    ACAI_CHECK_ARG(workspace_bytes >= need, "acai_edit_align: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipLaunchKernelGGL(edit_align_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, pred, ld_pred, pred_len, tgt, ld_tgt, tgt_len, group, counts,
                       pred_op, pred_to_tgt, tgt_to_pred, tgt_slot, (unsigned *)workspace, align_pair_dwords(ld_pred, ld_tgt));
    ACAI_LAUNCH_CHECK("acai_edit_align");
    return 0;
}
