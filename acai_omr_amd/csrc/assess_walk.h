// The run bookkeeping of acai_page_runs (csrc/assess.hip) as plain C++, so that it also compiles for the host: a column's pixels of one
// chunk -> what the chunk counts itself and a summary of what touches its edges; summaries, top down -> the counts across the edges and a
// summary of the stretch they cover.  No HIP in here; `Count` is anything callable as count(row, bin).
#pragma once

#if defined(__HIPCC__)
#define ACAI_WALK_HD __host__ __device__ __forceinline__
#else
#define ACAI_WALK_HD inline
#endif

namespace acai_runs {

ACAI_WALK_HD int imin(int a, int b) { return a < b ? a : b; }

// What a stretch of a column leaves for whoever joins it with the stretches above and below.  With r_1 .. r_k its runs: k as min(k, 4);
// the colours of r_1 and r_k; |r_1|, |r_k|, and for k >= 3 |r_2| and |r_{k-1}|.  r_2 .. r_{k-1} begin and end inside the stretch: they,
// and every pair (ink r_i, paper r_{i+1}) of them, were counted when the summary was made.  The join counts what touches an edge: r_1 and
// r_k joined with the neighbours' where the colours agree, and the pairs they are half of, (r_1, r_2) and (r_{k-1}, r_k).
struct Summary {
    int k, l1, l2, lp, ll;
    bool first_on, last_on;
};

// A chunk's summary in one word: a run inside a chunk of at most 63 rows fits 6 bits.
//   bits 0 .. 5 |r_1|, 6 .. 11 |r_2|, 12 .. 17 |r_{k-1}|, 18 .. 23 |r_k|, bit 24 r_1 is ink, bit 25 r_k is ink, bits 26 .. 27 min(k, 4) - 1
ACAI_WALK_HD int pack(const Summary &s) {
    return s.l1 | (s.l2 << 6) | (s.lp << 12) | (s.ll << 18) | ((int)s.first_on << 24) | ((int)s.last_on << 25) | ((s.k - 1) << 26);
}
ACAI_WALK_HD Summary unpack(int w) {
    return Summary{((w >> 26) & 3) + 1, w & 63, (w >> 6) & 63, (w >> 12) & 63, (w >> 18) & 63, (bool)((w >> 24) & 1), (bool)((w >> 25) & 1)};
}

// The walk down a column, run by run.  It carries the current run - colour `on`, length `len`, `open` while it is the walk's first (its
// true beginning is not known here), `local` when somebody counted it already - and `above`, the length of the closed ink run directly
// over it (0: none).  A run is counted when the run under it begins; the run the walk ends with is never counted.
template <typename Count>
struct Walk {
    Count count;
    int n = 0, len = 0, above = 0, l1 = 0, l2 = 0, prev = 0;
    bool on = false, open = true, local = false, first_on = false;

    ACAI_WALK_HD explicit Walk(Count c) : count(c) {}

    ACAI_WALK_HD void close() {
        if (!open) {
            if (!local) count(on ? 0 : 1, imin(len, 255));
            if (!on && above) count(2, imin(above + len, 255));
        }
        above = on && !open ? len : 0;
        if (n == 1) l1 = len;
        else if (n == 2) l2 = len;
        prev = len;
    }
    ACAI_WALK_HD void start(bool colour, int l, bool counted) { on = colour, len = l, local = counted, open = false, ++n; }

    // one pixel
    ACAI_WALK_HD void pixel(bool ink) {
        if (n == 0) {
            n = 1, len = 1, on = first_on = ink;
        } else if (ink == on) {
            ++len;
        } else {
            close();
            start(ink, 1, false);
        }
    }

    // the summary of the stretch below what was walked so far
    ACAI_WALK_HD void stretch(const Summary &s) {
        if (n == 0) {
            n = 1, len = s.l1, on = first_on = s.first_on;
        } else if (s.first_on == on) {
            len += s.l1;                                       // (the carried run is some stretch's last: never `local`)
        } else {
            close();
            start(s.first_on, s.l1, false);
        }
        if (s.k >= 2) {
            if (s.k >= 3) {
                close();
                start(!s.first_on, s.l2, true);
                if (s.k >= 4) {                                // r_3 .. r_{k-2} and the pairs among r_2 .. r_{k-1} are counted
                    close();
                    start(!s.last_on, s.lp, true);
                    above = 0;
                }
            }
            close();
            start(s.last_on, s.ll, false);
        }
    }

    // what was walked, for the next level (n >= 1).  A stretch that hid runs (k >= 4) leaves n >= 4, so min(n, 4) is the class of the true
    // number of runs, and l2 / prev are the true second and last-but-one run.
    ACAI_WALK_HD Summary summary() const { return Summary{imin(n, 4), n == 1 ? len : l1, n >= 3 ? l2 : 0, n >= 3 ? prev : 0, len, first_on, on}; }
};

}  // namespace acai_runs
