// The run bookkeeping of acai_page_runs (acai_omr_amd/csrc/assess_walk.h) on the host: a column walked the kernels' way - pixels of a chunk,
// chunk summaries of a segment, segment summaries - against the runs of the whole column counted directly, for chunk sizes, segment
// counts, heights and run lengths around every edge.  tests/test_assess_cpu.py compiles and runs it; exit code 0 and "ok" mean equal.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <algorithm>
#include "assess_walk.h"
using namespace acai_runs;
struct HostCount { long long *h; void operator()(int row, int bin) const { h[row * 256 + bin]++; } };
static void brute(const std::vector<bool> &col, long long *h) {
    std::vector<std::pair<bool,int>> r;
    for (bool v : col) { if (!r.empty() && r.back().first == v) r.back().second++; else r.push_back({v, 1}); }
    for (size_t i = 1; i + 1 < r.size(); ++i) {
        h[(r[i].first ? 0 : 1) * 256 + std::min(r[i].second, 255)]++;
        if (r[i].first && i + 2 < r.size()) h[2 * 256 + std::min(r[i].second + r[i + 1].second, 255)]++;
    }
}
static void kernel_way(const std::vector<bool> &col, int RC, int SEGS, long long *h) {
    const int H = (int)col.size(), chunks = (H + RC - 1) / RC;
    std::vector<int> work(chunks);
    for (int c = 0; c < chunks; ++c) {
        Walk<HostCount> w(HostCount{h});
        for (int y = c * RC; y < std::min(c * RC + RC, H); ++y) w.pixel(col[y]);
        work[c] = pack(w.summary());
    }
    const int per = (chunks + SEGS - 1) / SEGS;
    std::vector<Summary> ss(SEGS); std::vector<int> nn(SEGS);
    for (int s = 0; s < SEGS; ++s) {
        Walk<HostCount> w(HostCount{h});
        for (int c = std::min(s * per, chunks); c < std::min(s * per + per, chunks); ++c) w.stretch(unpack(work[c]));
        nn[s] = w.n; if (w.n) ss[s] = w.summary();
    }
    Walk<HostCount> w(HostCount{h});
    for (int s = 0; s < SEGS; ++s) if (nn[s]) w.stretch(ss[s]);
}
int main() {
    srand(7); long long cases = 0;
    for (int RC : {1, 2, 3, 5, 32, 63}) for (int SEGS : {1, 2, 3, 8}) for (int H = 1; H <= 700; H += (H < 80 ? 1 : 37)) for (int t = 0; t < 12; ++t) {
        std::vector<bool> col(H);
        const int mode = t % 6; const double p = mode == 0 ? 0.5 : mode == 1 ? 0.05 : mode == 2 ? 0.95 : 0.3;
        if (mode < 4) for (int y = 0; y < H; ++y) col[y] = rand() / (double)RAND_MAX < p;
        else { bool v = rand() & 1; int y = 0; while (y < H) { int n = 1 + rand() % (mode == 4 ? 3 * RC + 2 : 320); for (int i = 0; i < n && y < H; ++i) col[y++] = v; v = !v; } }
        long long a[768] = {0}, b[768] = {0};
        brute(col, a); kernel_way(col, RC, SEGS, b);
        if (memcmp(a, b, sizeof a)) { printf("MISMATCH RC=%d SEGS=%d H=%d t=%d\n", RC, SEGS, H, t); return 1; }
        ++cases;
    }
    printf("ok %lld cases\n", cases); return 0;
}
