// Page ingest (an extension; the reference converts and turns an uploaded photo on the host with PIL: Image.open(...).convert("L"),
// acai_omr/ui/routes.py:98,115 and train/datasets.py:32,122, and ImageOps.exif_transpose, ui/routes.py:118):
//   acai_page_ingest       a decoded photo in the layout it arrived in (interleaved or planar, 1 / 3 / 4 channels, any strides) -> the grey,
//                          upright page in ONE launch: PIL's integer grey value and the EXIF orientation's index map, bit for bit;
//   acai_page_col_profile  per column, the number of ink pixels and the longest run of them: the column counterpart of acai_page_profile
//                          (a page that lies on its side has its staff lines in the columns);
//   acai_page_box_ink      the ink count of every rectangle of a device table in one launch (which end of a system holds the clef).
// All three are bound by reading their input once; results are exact integers (or moved bits) and no atomics are used, so nothing depends
// on how the launches are scheduled.
//
// A lane always makes 4 consecutive output pixels.  Photos arrive as slices with any offset and any width, so neither the 4 C source bytes
// of such a group nor its 4 output bytes start on a word boundary in general: both sides use dword accesses at byte addresses (global
// memory takes them on gfx950; __builtin_memcpy states the alignment of 1 to the compiler) and only the ragged end of a row, at most one
// lane per row, goes byte by byte.
#include "common.h"
#include "resize_taps.h"

namespace {

enum { LAYOUT_ANY = 0, LAYOUT_PACKED = 1, LAYOUT_PLANAR = 2 };

// A uint8 source image: element (row r, column c, channel k) lies at p[r rs + c ps + k cs].  PACKED: the C channels of a pixel are adjacent
// and so are the pixels of a row (ps == C, cs == 1); PLANAR: three planes whose rows are contiguous (ps == 1); ANY: everything else.
struct Src {
    const unsigned char *p;
    long long ps, rs, cs;
    int H, W, C, layout;
};

// PIL's RGB -> L (ImagingConvert rgb2l): (19595 R + 38470 G + 7471 B + 32768) >> 16; the weights sum to 65536, so grey stays grey.
__device__ __forceinline__ unsigned grey(unsigned r, unsigned g, unsigned b) { return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16; }

template <int N>
__device__ __forceinline__ void load_words(const unsigned char *q, unsigned (&w)[N]) { __builtin_memcpy(w, q, 4 * N); }

template <int N>
__device__ __forceinline__ unsigned byte_of(const unsigned (&w)[N], int i) { return (w[i >> 2] >> (8 * (i & 3))) & 255u; }

// The grey values of the n (1 .. 4) pixels from q on, in ascending column order, as the bytes 0 .. n - 1 of a word.  A whole group of a
// PACKED or PLANAR image is read as C dwords; they cover exactly the 4 pixels' own bytes.
__device__ __forceinline__ unsigned grey4(const unsigned char *q, int n, const Src &s) {
    unsigned v = 0;
    if (n == 4 && s.layout == LAYOUT_PACKED) {
        if (s.C == 1) {
            unsigned w[1];
            load_words(q, w);
            return w[0];
        }
        if (s.C == 3) {
            unsigned w[3];
            load_words(q, w);
#pragma unroll
            for (int k = 0; k < 4; ++k) v |= grey(byte_of(w, 3 * k), byte_of(w, 3 * k + 1), byte_of(w, 3 * k + 2)) << (8 * k);
            return v;
        }
        unsigned w[4];   // (the fourth channel is not read into the value: PIL's RGBA -> L ignores it)
        load_words(q, w);
#pragma unroll
        for (int k = 0; k < 4; ++k) v |= grey(w[k] & 255u, (w[k] >> 8) & 255u, (w[k] >> 16) & 255u) << (8 * k);
        return v;
    }
    if (n == 4 && s.layout == LAYOUT_PLANAR) {
        unsigned r[1], g[1], b[1];
        load_words(q, r), load_words(q + s.cs, g), load_words(q + 2 * s.cs, b);
#pragma unroll
        for (int k = 0; k < 4; ++k) v |= grey(byte_of(r, k), byte_of(g, k), byte_of(b, k)) << (8 * k);
        return v;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < n) {
            const unsigned char *e = q + k * s.ps;
            v |= (s.C == 1 ? (unsigned)e[0] : grey(e[0], e[s.cs], e[2 * s.cs])) << (8 * k);
        }
    return v;
}

// n (1 .. 4) pixels, the bytes 0 .. n - 1 of v, to o: one dword store for a whole group.
__device__ __forceinline__ void store4(unsigned char *o, unsigned v, int n) {
    if (n == 4) {
        __builtin_memcpy(o, &v, 4);
        return;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (k < n) o[k] = (unsigned char)(v >> (8 * k));
}

// The bytes 0 .. n - 1 of v in reverse order (n in 1 .. 4).
__device__ __forceinline__ unsigned reverse_bytes(unsigned v, int n) { return __builtin_bswap32(v) >> (8 * (4 - n)); }

// ---- orientations 1 .. 4: a row of the output is a row of the input, forwards or backwards ------------------------------------------------
// Grid (groups of 256 lanes x 4 pixels, rows).  Output pixels x .. x + n - 1 of row y are source pixels sx .. sx + n - 1 of row sy, mirrored
// within the group when flip_h: the group is read in ascending order either way.
constexpr int ROW_THREADS = 256;

__global__ __launch_bounds__(ROW_THREADS) void ingest_rows_kernel(Src s, int flip_h, int flip_v, unsigned char *__restrict__ out, int out_pitch) {
    const int y = blockIdx.y, x = (blockIdx.x * ROW_THREADS + threadIdx.x) * 4;
    if (x >= s.W) return;
    const int n = min(4, s.W - x);
    const int sy = flip_v ? s.H - 1 - y : y, sx = flip_h ? s.W - x - n : x;
    unsigned v = grey4(s.p + sy * s.rs + sx * s.ps, n, s);
    if (flip_h) v = reverse_bytes(v, n);
    store4(out + (size_t)y * out_pitch + x, v, n);
}

// ---- orientations 5 .. 8: a row of the output is a column of the input ------------------------------------------------------------------
// A workgroup owns a tile of TILE x TILE source pixels.  It reads the tile's rows as the row kernel does (a wave reads 2 rows of 128
// pixels, 4 C bytes per lane), converts to grey on the way in and keeps the tile in LDS as dwords of 4 pixels.  Then a lane takes the 4 x 4
// pixels of source rows 4 bi .. 4 bi + 3, columns 4 bj .. 4 bj + 3: four dword reads, transposed in registers, four dword stores - one to
// each of 4 output rows, and the 32 lanes with consecutive bi write 128 consecutive bytes of one output row.  LDS dword (r, cd) is kept at
// column (cd + (r >> 2)) % 32 of row r: a wave half writes 32 consecutive dwords of one row and reads (4 bi + k, bj) for 32 consecutive
// bi, which the rotation spreads over all 32 banks (a plain or padded pitch cannot: 4 rows apart is a multiple of 4 dwords whatever the
// pitch).
constexpr int TILE = 128, TILE_DW = TILE / 4, TURN_THREADS = 256;

__device__ __forceinline__ int tile_slot(int r, int cd) { return r * TILE_DW + ((cd + (r >> 2)) & (TILE_DW - 1)); }

__global__ __launch_bounds__(TURN_THREADS) void ingest_turn_kernel(Src s, int flip_r, int flip_c, unsigned char *__restrict__ out, int out_pitch) {
    __shared__ unsigned tile[TILE * TILE_DW];
    const int r0 = blockIdx.y * TILE, c0 = blockIdx.x * TILE;
    for (int i = threadIdx.x; i < TILE * TILE_DW; i += TURN_THREADS) {
        const int r = i / TILE_DW, cd = i % TILE_DW;
        const int gr = r0 + r, gc = c0 + 4 * cd;
        unsigned v = 0;
        if (gr < s.H && gc < s.W) v = grey4(s.p + gr * s.rs + gc * s.ps, min(4, s.W - gc), s);
        tile[tile_slot(r, cd)] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TILE_DW * TILE_DW; i += TURN_THREADS) {
        const int bi = i % TILE_DW, bj = i / TILE_DW;
        const int gr = r0 + 4 * bi, gc = c0 + 4 * bj;
        if (gr >= s.H || gc >= s.W) continue;
        const int nr = min(4, s.H - gr), nc = min(4, s.W - gc);
        unsigned w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = tile[tile_slot(4 * bi + k, bj)];
        const int ox = flip_r ? s.H - gr - nr : gr;   // source rows gr .. gr + nr - 1 are output columns ox .. ox + nr - 1, backwards when flip_r
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            if (m >= nc) break;
            unsigned t = ((w[0] >> (8 * m)) & 255u) | (((w[1] >> (8 * m)) & 255u) << 8) | (((w[2] >> (8 * m)) & 255u) << 16) | (((w[3] >> (8 * m)) & 255u) << 24);
            if (flip_r) t = reverse_bytes(t, nr);
            const int oy = flip_c ? s.W - 1 - (gc + m) : gc + m;
            store4(out + (size_t)oy * out_pitch + ox, t, nr);
        }
    }
}

// ---- single-channel fp32: the same index maps on 32-bit words, whatever they hold -------------------------------------------------------
constexpr int F_TILE = 64;

__global__ __launch_bounds__(256) void ingest_rows_f32_kernel(const uint32_t *__restrict__ p, long long ps, long long rs, int H, int W, int flip_h, int flip_v,
                                                              uint32_t *__restrict__ out, int out_pitch) {
    const int y = blockIdx.y, x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    out[(size_t)y * out_pitch + x] = p[(flip_v ? H - 1 - y : y) * rs + (flip_h ? W - 1 - x : x) * ps];
}

__global__ __launch_bounds__(256) void ingest_turn_f32_kernel(const uint32_t *__restrict__ p, long long ps, long long rs, int H, int W, int flip_r, int flip_c,
                                                              uint32_t *__restrict__ out, int out_pitch) {
    __shared__ uint32_t tile[F_TILE][F_TILE + 1];
    const int r0 = blockIdx.y * F_TILE, c0 = blockIdx.x * F_TILE;
    for (int i = threadIdx.x; i < F_TILE * F_TILE; i += 256) {
        const int r = i / F_TILE, c = i % F_TILE;
        if (r0 + r < H && c0 + c < W) tile[r][c] = p[(r0 + r) * rs + (c0 + c) * ps];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < F_TILE * F_TILE; i += 256) {
        const int c = i / F_TILE, r = i % F_TILE;
        if (r0 + r < H && c0 + c < W) {
            const int oy = flip_c ? W - 1 - (c0 + c) : c0 + c, ox = flip_r ? H - 1 - (r0 + r) : r0 + r;
            out[(size_t)oy * out_pitch + ox] = tile[r][c];
        }
    }
}

// ---- ink test ---------------------------------------------------------------------------------------------------------------------------
template <typename TI>
__device__ __forceinline__ bool is_ink(const TI *p, float thr) { return in_sample(p) < thr; }

// A uint8 value v is ink iff (float)v / 255 < thr, which is monotone in v: iff v < the first value that is not, found by bisection with the
// comparison itself (as csrc/page.hip does for its 16-byte loads).
__device__ __forceinline__ int ink_limit_u8(float thr) {
    int lo = 0, hi = 256;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const unsigned char v = (unsigned char)mid;
        if (is_ink(&v, thr)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ---- column profile ---------------------------------------------------------------------------------------------------------------------
// Grid (groups of 64 lanes x 4 columns, chunks of rows), one wave per workgroup.  A lane owns 4 adjacent columns and walks its chunk's rows
// down: a wave reads 256 consecutive pixels of every row.  Per column and chunk it leaves (leading run, trailing run, best run, ink) in
// work [chunk][4][W]; the rows of a chunk are known, so that is the whole of page.hip's `Runs`.
constexpr int COL_LANE_PX = 4, COL_ROWS_AHEAD = 8;

template <typename TI>
__global__ __launch_bounds__(64) void col_profile_kernel(const TI *__restrict__ page, int H, int W, int pitch, int chunk_rows, float thr,
                                                         int32_t *__restrict__ work) {
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * COL_LANE_PX;
    if (x0 >= W) return;
    const int n = min(COL_LANE_PX, W - x0);
    const int y0 = blockIdx.y * chunk_rows, y1 = min(y0 + chunk_rows, H);
    const int limit = sizeof(TI) == 1 ? ink_limit_u8(thr) : 0;
    int pre[COL_LANE_PX], cur[COL_LANE_PX], best[COL_LANE_PX], ink[COL_LANE_PX];
    bool all[COL_LANE_PX];
#pragma unroll
    for (int k = 0; k < COL_LANE_PX; ++k) pre[k] = cur[k] = best[k] = ink[k] = 0, all[k] = true;
    auto step = [&](int k, bool on) {
        if (on) {
            ++cur[k], ++ink[k];
            best[k] = max(best[k], cur[k]);
        } else {
            if (all[k]) pre[k] = cur[k], all[k] = false;
            cur[k] = 0;
        }
    };
    int y = y0;
    if (n == COL_LANE_PX) {   // COL_ROWS_AHEAD rows are loaded before the first of them is looked at: the walk is bound by load latency
        for (; y + COL_ROWS_AHEAD <= y1; y += COL_ROWS_AHEAD) {
            TI v[COL_ROWS_AHEAD][COL_LANE_PX];
#pragma unroll
            for (int u = 0; u < COL_ROWS_AHEAD; ++u) __builtin_memcpy(v[u], page + (size_t)(y + u) * pitch + x0, sizeof(v[u]));
#pragma unroll
            for (int u = 0; u < COL_ROWS_AHEAD; ++u) {
#pragma unroll
                for (int k = 0; k < COL_LANE_PX; ++k) {
                    if constexpr (sizeof(TI) == 1) step(k, (int)v[u][k] < limit);
                    else step(k, is_ink(&v[u][k], thr));
                }
            }
        }
    }
    for (; y < y1; ++y) {     // the rows left over, and every row of the lane at the ragged edge (n < 4)
        const TI *row = page + (size_t)y * pitch + x0;
#pragma unroll
        for (int k = 0; k < COL_LANE_PX; ++k)
            if (k < n) step(k, is_ink(row + k, thr));
    }
    int32_t *w = work + (size_t)blockIdx.y * 4 * W + x0;
#pragma unroll
    for (int k = 0; k < COL_LANE_PX; ++k)
        if (k < n) {
            w[k] = all[k] ? cur[k] : pre[k];
            w[(size_t)W + k] = cur[k];
            w[(size_t)2 * W + k] = best[k];
            w[(size_t)3 * W + k] = ink[k];
        }
}

// One lane per column joins its chunks from the top down (page.hip's `join`, with the chunk's row count for len).  The walk is bound by the
// latency of its loads - up to 64 chunks in sequence, a few thousand lanes in all - so the workgroups are single waves, for as many CUs as
// there are, and the loop is unrolled: the loads of 8 chunks depend on nothing and go out together.
constexpr int JOIN_THREADS = 64;

__global__ __launch_bounds__(JOIN_THREADS) void col_join_kernel(const int32_t *__restrict__ work, int H, int W, int chunk_rows, int chunks, int32_t *__restrict__ ink,
                                                       int32_t *__restrict__ run) {
    const int x = blockIdx.x * JOIN_THREADS + threadIdx.x;
    if (x >= W) return;
    int len = 0, suf = 0, best = 0, total = 0;
#pragma unroll 8
    for (int c = 0; c < chunks; ++c) {
        const int32_t *w = work + (size_t)c * 4 * W + x;
        const int blen = min(chunk_rows, H - c * chunk_rows), bpre = w[0], bsuf = w[W], bbest = w[(size_t)2 * W], bink = w[(size_t)3 * W];
        best = max(max(best, bbest), suf + bpre);
        suf = bsuf == blen ? blen + suf : bsuf;
        len += blen, total += bink;
    }
    ink[x] = total;
    run[x] = best;
}

// ---- box ink ----------------------------------------------------------------------------------------------------------------------------
// One workgroup of BOX_WAVES = 16 waves per rectangle (x0, y0, x1, y1), clipped to the page here (the table lives on the device: the host
// has not seen it): wave w counts rows y0 + w, y0 + w + 16, ..., a lane every 64th column of them.
constexpr int BOX_WAVES = 16;

template <typename TI>
__global__ __launch_bounds__(64 * BOX_WAVES) void box_ink_kernel(const TI *__restrict__ page, int H, int W, int pitch, float thr, const int32_t *__restrict__ boxes,
                                                      int32_t *__restrict__ out) {
    __shared__ int part[BOX_WAVES];
    const int32_t *b = boxes + (size_t)blockIdx.x * 4;
    const int x0 = max(b[0], 0), y0 = max(b[1], 0), x1 = min(b[2], W), y1 = min(b[3], H);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int count = 0;
    for (int y = y0 + wave; y < y1; y += BOX_WAVES) {
        const TI *row = page + (size_t)y * pitch;
        for (int x = x0 + lane; x < x1; x += 64) count += is_ink(row + x, thr);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o);
    if (lane == 0) part[wave] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < BOX_WAVES; ++w) count += part[w];
        out[blockIdx.x] = count;
    }
}

}  // namespace

#define ACAI_PAGE_CHECK(name)                                                                                                                   \
    ACAI_CHECK_ARG(page, name ": null page");                                                                                                    \
    ACAI_CHECK_ARG(H > 0 && W > 0 && H <= ACAI_PAGE_MAX_H && W <= ACAI_PAGE_MAX_W && pitch >= W, name ": bad page %d x %d, pitch %d (H <= %d, W <= %d)", H, W, \
                   pitch, ACAI_PAGE_MAX_H, ACAI_PAGE_MAX_W)

extern "C" int acai_page_ingest(const void *src, int in_u8, int H, int W, int C, int64_t pix_stride, int64_t row_stride, int64_t chan_stride, int orientation,
                                void *out, int out_pitch, void *stream) {
    ACAI_CHECK_ARG(src && out && src != out, "acai_page_ingest: null operand, or out is the source");
    ACAI_CHECK_ARG(orientation >= 1 && orientation <= 8, "acai_page_ingest: orientation %d is not an EXIF code 1 .. 8", orientation);
    ACAI_CHECK_ARG(C == 1 || ((C == 3 || C == 4) && in_u8), "acai_page_ingest: %d channels of %s: expected 1, or 3 / 4 of uint8", C, in_u8 ? "uint8" : "fp32");
    const bool turn = orientation >= 5;
    const int OH = turn ? W : H, OW = turn ? H : W;
    ACAI_CHECK_ARG(H > 0 && W > 0 && OH <= ACAI_PAGE_MAX_H && OW <= ACAI_PAGE_MAX_W && out_pitch >= OW,
                   "acai_page_ingest: a %d x %d source gives a %d x %d page, out_pitch %d (H <= %d, W <= %d)", H, W, OH, OW, out_pitch, ACAI_PAGE_MAX_H,
                   ACAI_PAGE_MAX_W);
    ACAI_CHECK_ARG(pix_stride >= 1 && (H == 1 || row_stride >= 1) && (C == 1 || chan_stride >= 1), "acai_page_ingest: strides must be positive");
    hipStream_t st = (hipStream_t)stream;
    // the table of include/acai_omr_hip.h: which source index runs backwards
    const int flip_h = orientation == 2 || orientation == 3, flip_v = orientation == 3 || orientation == 4;     // 1 .. 4: columns, rows
    const int flip_r = orientation == 6 || orientation == 7, flip_c = orientation == 7 || orientation == 8;     // 5 .. 8: source row, source column
    if (!in_u8) {
        const uint32_t *p = reinterpret_cast<const uint32_t *>(src);
        if (turn)
            hipLaunchKernelGGL(ingest_turn_f32_kernel, dim3(cdiv(W, F_TILE), cdiv(H, F_TILE)), dim3(256), 0, st, p, (long long)pix_stride, (long long)row_stride,
                               H, W, flip_r, flip_c, reinterpret_cast<uint32_t *>(out), out_pitch);
        else
            hipLaunchKernelGGL(ingest_rows_f32_kernel, dim3(cdiv(W, 256), H), dim3(256), 0, st, p, (long long)pix_stride, (long long)row_stride, H, W, flip_h,
                               flip_v, reinterpret_cast<uint32_t *>(out), out_pitch);
        ACAI_LAUNCH_CHECK("acai_page_ingest (fp32)");
        return 0;
    }
    Src s{reinterpret_cast<const unsigned char *>(src), (long long)pix_stride, (long long)row_stride, (long long)chan_stride, H, W, C, LAYOUT_ANY};
    if (C == 1 ? pix_stride == 1 : (chan_stride == 1 && pix_stride == C)) s.layout = LAYOUT_PACKED;
    else if (C == 3 && pix_stride == 1) s.layout = LAYOUT_PLANAR;
    if (turn)
        hipLaunchKernelGGL(ingest_turn_kernel, dim3(cdiv(W, TILE), cdiv(H, TILE)), dim3(TURN_THREADS), 0, st, s, flip_r, flip_c,
                           reinterpret_cast<unsigned char *>(out), out_pitch);
    else
        hipLaunchKernelGGL(ingest_rows_kernel, dim3(cdiv(cdiv(W, 4), ROW_THREADS), H), dim3(ROW_THREADS), 0, st, s, flip_h, flip_v,
                           reinterpret_cast<unsigned char *>(out), out_pitch);
    ACAI_LAUNCH_CHECK("acai_page_ingest");
    return 0;
}

extern "C" int acai_page_col_profile(const void *page, int in_u8, int H, int W, int pitch, float ink_threshold, int32_t *ink, int32_t *run, int32_t *work,
                                     int64_t work_elems, void *stream) {
    ACAI_PAGE_CHECK("acai_page_col_profile");
    // at least ACAI_COL_CHUNK_ROWS rows per chunk, at most ACAI_COL_MAX_CHUNKS chunks
    const int chunk_rows = cdiv(H, ACAI_COL_MAX_CHUNKS) > ACAI_COL_CHUNK_ROWS ? cdiv(H, ACAI_COL_MAX_CHUNKS) : ACAI_COL_CHUNK_ROWS;
    const int chunks = cdiv(H, chunk_rows);
    ACAI_CHECK_ARG(ink && run && work && work_elems >= (int64_t)4 * chunks * W, "acai_page_col_profile: null output, or work holds %lld int32 where %lld are needed",
                   (long long)work_elems, (long long)4 * chunks * W);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(cdiv(cdiv(W, COL_LANE_PX), 64), chunks);
    if (in_u8)
        hipLaunchKernelGGL(col_profile_kernel<unsigned char>, grid, dim3(64), 0, st, reinterpret_cast<const unsigned char *>(page), H, W, pitch, chunk_rows,
                           ink_threshold, work);
    else
        hipLaunchKernelGGL(col_profile_kernel<float>, grid, dim3(64), 0, st, reinterpret_cast<const float *>(page), H, W, pitch, chunk_rows, ink_threshold, work);
    ACAI_LAUNCH_CHECK("acai_page_col_profile (chunks)");
    hipLaunchKernelGGL(col_join_kernel, dim3(cdiv(W, JOIN_THREADS)), dim3(JOIN_THREADS), 0, st, (const int32_t *)work, H, W, chunk_rows, chunks, ink, run);
    ACAI_LAUNCH_CHECK("acai_page_col_profile (join)");
    return 0;
}

extern "C" int acai_page_box_ink(const void *page, int in_u8, int H, int W, int pitch, float ink_threshold, const int32_t *boxes, int n, int32_t *out,
                                 void *stream) {
    ACAI_PAGE_CHECK("acai_page_box_ink");
    ACAI_CHECK_ARG(n >= 0 && n <= 65535, "acai_page_box_ink: %d rectangles: the rectangle is a grid dimension (0 .. 65535)", n);
    if (n == 0) return 0;
    ACAI_CHECK_ARG(boxes && out, "acai_page_box_ink: null operand");
    hipStream_t st = (hipStream_t)stream;
    if (in_u8)
        hipLaunchKernelGGL(box_ink_kernel<unsigned char>, dim3(n), dim3(64 * BOX_WAVES), 0, st, reinterpret_cast<const unsigned char *>(page), H, W, pitch, ink_threshold, boxes,
                           out);
    else
        hipLaunchKernelGGL(box_ink_kernel<float>, dim3(n), dim3(64 * BOX_WAVES), 0, st, reinterpret_cast<const float *>(page), H, W, pitch, ink_threshold, boxes, out);
    ACAI_LAUNCH_CHECK("acai_page_box_ink");
    return 0;
}
