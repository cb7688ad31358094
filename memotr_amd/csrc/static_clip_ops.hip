// static_clip_ops.hip -- a training clip from one still image: the reference's MultiRandomShift chain (crop a shifted
// window of the previous frame, resize it back; Pillow's 8-bit bilinear) for all T frames in one gfx950 launch (C ABI
// and the arithmetic: include/static_clip_ops_hip.h; the definition and where it comes from: DESIGN.md).
//
// Frame k is a vertical resample of frame k - 1 moved s columns to the left, so column x of frame k is the vertical
// pass applied k times to column x + k * s of the image: the chain never mixes columns.  One workgroup owns a strip of
// source columns and
//   1. copies the strip into LDS as ALIGNED dwords (a row of 3-byte pixels starts on any byte: every row keeps its own
//      misalignment 0..3 in front), then reorders it into the first of two LDS images: flip and channel swap applied,
//      rows of P dwords, P odd so that threads on consecutive rows sit on different banks;
//   2. writes the strip to frame 0, then T - 1 times runs the vertical pass from one LDS image into the other (one
//      thread per row, the row's taps in registers) and writes the result to frame k at columns moved by k * s,
//      clipped at column 0.  The stores are aligned dwords put together from the LDS bytes, consecutive threads on
//      consecutive dwords of a row; bytes where a row segment starts or ends;
//   3. zero-fills the columns x >= w - k * s of frame k that lie in its strip (the black that PIL pads with).
// The image is read once and no intermediate frame is read back.  A strip is as wide as the LDS of one workgroup
// allows for this h (plan()); an image too tall for even the narrowest strip takes shift_chain_global_kernel, which
// keeps the same chain in the output frames: frame k is computed from the bytes the SAME workgroup wrote to frame
// k - 1 (a column has one owner for the whole chain), same arithmetic, same result.
//
// The tap counts are run-time loop bounds and row indices are clamped.  All arithmetic is 32-bit integer.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/static_clip_ops_hip.h"

namespace {

thread_local char g_err[256] = {0};      // text of this thread's last error; read by staticclip_last_error() only

int fail(int code, const char *msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

constexpr int THREADS = 512;
constexpr int LDS_MAX = 64 * 1024;       // what one workgroup asks for at most (two workgroups fit a CU's 160 KiB)
constexpr int MAX_QUADS = 16;            // a strip is 4 * m columns (12 * m bytes, whole dwords), m <= 16
constexpr int REG_TAPS = 3;              // taps kept in registers: an enlarging triangle filter has at most 3
constexpr int GLOBAL_STRIP = 64;         // strip of the global-memory path
constexpr int XCDS = 8;                  // workgroup b runs on XCD b % 8: neighbouring strips share an L2

struct Args {
    const uint8_t *src;
    long row_pitch;
    int h, w, T, flip, swap_rb, s, y0, hc;
    const int32_t *xmin, *cnt, *kk;
    int ks;
    uint8_t *out;
    long out_row_pitch, out_frame_pitch;
    int strip, nstrips, chunk, P;        // P: dwords of one LDS row
};

__host__ __device__ inline int row_dwords(int m) { return (3 * m + 1) | 1; }    // + 1 for the misalignment, odd

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ int level(int acc) { return clampi(acc >> 22, 0, 255); }

// strip of this workgroup; neighbouring strips go to one XCD, where their parts of an output cache line meet in L2
__device__ __forceinline__ int strip_of_block(const Args &a) {
    const int b = blockIdx.x;
    return (b % XCDS) * a.chunk + b / XCDS;
}

// Bytes b_lo .. b_lo + nbytes - 1 of every LDS row (img == nullptr: zeros) to h global rows; dst0 is where byte b_lo of
// row 0 goes, any alignment.  Consecutive threads take consecutive aligned dwords of a destination row.
__device__ __forceinline__ void store_rows(const uint32_t *img, int P, int h, int b_lo, int nbytes, uint8_t *dst0,
                                           long pitch, int tid) {
    const int slots = (nbytes + 3) / 4 + 1;
    const int total = h * slots;
    for (int i = tid; i < total; i += THREADS) {
        const int r = i / slots, sl = i - r * slots;
        uint8_t *g = dst0 + (size_t)r * (size_t)pitch;
        const int rel = 4 * sl - (int)((uintptr_t)g & 3);   // first byte, relative to b_lo, of this aligned dword
        if (rel >= nbytes)
            continue;
        const uint32_t *row = img + r * P;
        if (rel >= 0 && rel + 4 <= nbytes) {
            uint32_t v = 0;
            if (img) {
                const int b = b_lo + rel, sh = b & 3;
                v = row[b >> 2];
                if (sh)
                    v = (uint32_t)((((uint64_t)row[(b >> 2) + 1] << 32) | v) >> (8 * sh));
            }
            *reinterpret_cast<uint32_t *>(g + rel) = v;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int b = rel + q;
                if (b >= 0 && b < nbytes)
                    g[b] = img ? reinterpret_cast<const uint8_t *>(row)[b_lo + b] : (uint8_t)0;
            }
        }
    }
}

__global__ __launch_bounds__(THREADS) void shift_chain_lds_kernel(const Args a) {
    extern __shared__ uint32_t smem[];
    const int st = strip_of_block(a);
    if (st >= a.nstrips)
        return;
    const int tid = threadIdx.x, h = a.h, P = a.P;
    const int c0 = st * a.strip, n = min(a.strip, a.w - c0), nb = 3 * n, rw = (nb + 3) / 4;
    uint32_t *cur = smem, *nxt = smem + h * P;

    // 1. the strip's bytes as they lie in memory (columns mc0 .. mc0 + n - 1), aligned dwords, into `nxt`
    const int mc0 = a.flip ? a.w - c0 - n : c0;
    for (int i = tid; i < h * P; i += THREADS) {
        const int r = i / P, d = i - r * P;
        const uint8_t *first = a.src + (size_t)r * (size_t)a.row_pitch + (size_t)mc0 * 3;
        const int mis = (int)((uintptr_t)first & 3);
        if (d * 4 < mis + nb)                               // a dword is loaded only if it holds a byte of the row
            nxt[i] = reinterpret_cast<const uint32_t *>(first - mis)[d];
    }
    __syncthreads();
    // ... reordered into `cur`: p_0 of the strip, byte 3 * x + c of a row at its place, zeros behind the last column
    for (int i = tid; i < h * rw; i += THREADS) {
        const int r = i / rw, d = i - r * rw;
        const uint8_t *first = a.src + (size_t)r * (size_t)a.row_pitch + (size_t)mc0 * 3;
        const uint8_t *raw = reinterpret_cast<const uint8_t *>(nxt + r * P) + (int)((uintptr_t)first & 3);
        uint32_t v = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int b = 4 * d + q;
            if (b < nb) {
                const int x = b / 3, c = b - 3 * x;
                v |= (uint32_t)raw[3 * (a.flip ? n - 1 - x : x) + (a.swap_rb ? 2 - c : c)] << (8 * q);
            }
        }
        cur[r * P + d] = v;
    }
    __syncthreads();

    for (int k = 0; k < a.T; ++k) {
        const long moved = (long)k * a.s;                   // frame k shows source column x + moved at column x
        if (k > 0 && moved < c0 + n) {                      // (a strip that has left the frame stays out: no pass)
            for (int y = tid; y < h; y += THREADS) {        // 2. the vertical pass, cur -> nxt
                const int cnt = min(a.cnt[y], a.ks), r0 = a.y0 + a.xmin[y];
                const int32_t *kk = a.kk + (size_t)y * (size_t)a.ks;
                int wgt[REG_TAPS], off[REG_TAPS];
#pragma unroll
                for (int j = 0; j < REG_TAPS; ++j) {
                    wgt[j] = j < cnt ? kk[j] : 0;
                    off[j] = clampi(r0 + j, 0, h - 1) * P;
                }
                for (int d = 0; d < rw; ++d) {
                    int acc[4] = {1 << 21, 1 << 21, 1 << 21, 1 << 21};
#pragma unroll
                    for (int j = 0; j < REG_TAPS; ++j) {
                        const uint32_t v = cur[off[j] + d];
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            acc[q] += (int)((v >> (8 * q)) & 255u) * wgt[j];
                    }
                    for (int j = REG_TAPS; j < cnt; ++j) {
                        const uint32_t v = cur[clampi(r0 + j, 0, h - 1) * P + d];
                        const int wj = kk[j];
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            acc[q] += (int)((v >> (8 * q)) & 255u) * wj;
                    }
                    nxt[y * P + d] = (uint32_t)level(acc[0]) | (uint32_t)level(acc[1]) << 8 |
                                     (uint32_t)level(acc[2]) << 16 | (uint32_t)level(acc[3]) << 24;
                }
            }
            __syncthreads();
            uint32_t *t = cur;
            cur = nxt;
            nxt = t;
        }
        uint8_t *frame = a.out + (size_t)k * (size_t)a.out_frame_pitch;
        if (moved < c0 + n) {                               // strip columns skip .. n - 1 are inside frame k
            const int skip = moved > c0 ? (int)(moved - c0) : 0;
            store_rows(cur, P, h, 3 * skip, 3 * (n - skip), frame + ((long)c0 + skip - moved) * 3, a.out_row_pitch, tid);
        }
        const long z0 = max((long)c0, (long)a.w - moved);   // 3. the black columns of frame k inside this strip
        if (z0 < c0 + n)
            store_rows(nullptr, P, h, 0, 3 * (int)(c0 + n - z0), frame + z0 * 3, a.out_row_pitch, tid);
    }
}

// The same chain without LDS, for an image too tall for it: frame k from the bytes this workgroup wrote to frame k - 1.
__global__ __launch_bounds__(THREADS) void shift_chain_global_kernel(const Args a) {
    const int st = strip_of_block(a);
    if (st >= a.nstrips)
        return;
    const int tid = threadIdx.x;
    const int c0 = st * a.strip, n = min(a.strip, a.w - c0), nb = 3 * n;
    const long total = (long)a.h * nb;
    for (long i = tid; i < total; i += THREADS) {           // frame 0
        const int y = (int)(i / nb), b = (int)(i - (long)y * nb), x = b / 3, c = b - 3 * x;
        const int col = a.flip ? a.w - 1 - (c0 + x) : c0 + x;
        a.out[(size_t)y * (size_t)a.out_row_pitch + (size_t)(c0 + x) * 3 + c] =
            a.src[(size_t)y * (size_t)a.row_pitch + (size_t)col * 3 + (a.swap_rb ? 2 - c : c)];
    }
    for (int k = 1; k < a.T; ++k) {
        const long moved = (long)k * a.s;
        uint8_t *frame = a.out + (size_t)k * (size_t)a.out_frame_pitch;
        if (moved < c0 + n) {
            __threadfence();
            __syncthreads();                                // frame k - 1 of this strip is complete and visible
            const uint8_t *prev = frame - a.out_frame_pitch;
            const int skip = moved > c0 ? (int)(moved - c0) : 0;
            for (long i = tid; i < total; i += THREADS) {
                const int y = (int)(i / nb), b = (int)(i - (long)y * nb), x = b / 3, c = b - 3 * x;
                if (x < skip)
                    continue;
                const long col = (long)c0 + x - moved;      // in frame k; the same source column is at col + s in k - 1
                const int cnt = min(a.cnt[y], a.ks), r0 = a.y0 + a.xmin[y];
                const int32_t *kk = a.kk + (size_t)y * (size_t)a.ks;
                int acc = 1 << 21;
                for (int j = 0; j < cnt; ++j)
                    acc += (int)prev[(size_t)clampi(r0 + j, 0, a.h - 1) * (size_t)a.out_row_pitch +
                                     (size_t)(col + a.s) * 3 + c] * kk[j];
                frame[(size_t)y * (size_t)a.out_row_pitch + (size_t)col * 3 + c] = (uint8_t)level(acc);
            }
        }
        const long z0 = max((long)c0, (long)a.w - moved);
        if (z0 < c0 + n) {
            const int zb = 3 * (int)(c0 + n - z0);
            const long ztotal = (long)a.h * zb;
            for (long i = tid; i < ztotal; i += THREADS) {
                const long y = i / zb;
                frame[(size_t)y * (size_t)a.out_row_pitch + (size_t)z0 * 3 + (size_t)(i - y * zb)] = 0;
            }
        }
    }
}

// strip width (columns) and LDS bytes for an h x w image; lds == 0: the global-memory path
void plan(int h, int w, int *strip, int *lds) {
    int m = 0;                                              // widest strip whose two images fit the LDS
    while (m < MAX_QUADS && 8L * h * row_dwords(m + 1) <= LDS_MAX)
        ++m;
    if (m == 0) {
        *strip = GLOBAL_STRIP;
        *lds = 0;
        return;
    }
    // ... but no wider than leaves 256 strips, one per CU, where the image has that many columns; 8 at the least:
    // a narrower strip only shortens the contiguous bytes a row store covers
    int par = w / (4 * 256);
    if (par < 2) par = 2;
    if (m > par) m = par;
    *strip = 4 * m;
    *lds = 8 * h * row_dwords(m);
}

}  // namespace

extern "C" {

int staticclip_abi_version(void) { return STATICCLIP_ABI_VERSION; }
const char *staticclip_last_error(void) { return g_err; }

int staticclip_plan(int h, int w, int *strip, int *lds_bytes) {
    if (!strip || !lds_bytes) return fail(1, "staticclip_plan: null pointer");
    if (h <= 0 || w <= 0) return fail(2, "staticclip_plan: non-positive size");
    plan(h, w, strip, lds_bytes);
    g_err[0] = 0;
    return 0;
}

int staticclip_shift_chain(const uint8_t *src, long row_pitch, int h, int w, int T, int flip, int swap_rb,
                           int s, int y0, int hc,
                           const int32_t *xmin, const int32_t *cnt, const int32_t *kk, int ksize,
                           uint8_t *out, long out_row_pitch, long out_frame_pitch, void *stream) {
    if (!src || !xmin || !cnt || !kk || !out) return fail(1, "staticclip_shift_chain: null pointer");
    if (h <= 0 || w <= 0) return fail(2, "staticclip_shift_chain: non-positive size");
    if (T < 1) return fail(3, "staticclip_shift_chain: clip length below 1");
    if (ksize <= 0) return fail(4, "staticclip_shift_chain: non-positive tap count");
    if ((flip != 0 && flip != 1) || (swap_rb != 0 && swap_rb != 1))
        return fail(5, "staticclip_shift_chain: flip or swap_rb is not 0 or 1");
    if (row_pitch < 3L * w) return fail(6, "staticclip_shift_chain: row pitch smaller than 3 * w");
    if (out_row_pitch < 3L * w) return fail(6, "staticclip_shift_chain: output row pitch smaller than 3 * w");
    if (T > 1 && out_frame_pitch < (long)(h - 1) * out_row_pitch + 3L * w)
        return fail(6, "staticclip_shift_chain: output frame pitch smaller than a frame");
    if (s < 0) return fail(7, "staticclip_shift_chain: negative column shift");
    if (y0 < 0 || hc < 1 || (long)y0 + hc > h)
        return fail(8, "staticclip_shift_chain: row window is not inside the image");

    Args a;
    a.src = src; a.row_pitch = row_pitch; a.h = h; a.w = w; a.T = T; a.flip = flip; a.swap_rb = swap_rb;
    a.s = s; a.y0 = y0; a.hc = hc; a.xmin = xmin; a.cnt = cnt; a.kk = kk; a.ks = ksize;
    a.out = out; a.out_row_pitch = out_row_pitch; a.out_frame_pitch = out_frame_pitch;
    int lds = 0;
    plan(h, w, &a.strip, &lds);
    a.nstrips = (w + a.strip - 1) / a.strip;
    a.chunk = (a.nstrips + XCDS - 1) / XCDS;
    a.P = lds ? lds / (8 * h) : 0;
    const dim3 grid((unsigned)(a.chunk * XCDS));
    if (lds)
        hipLaunchKernelGGL(shift_chain_lds_kernel, grid, dim3(THREADS), (size_t)lds, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(shift_chain_global_kernel, grid, dim3(THREADS), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "staticclip_shift_chain: %s", hipGetErrorString(e));
        return (int)e;
    }
    g_err[0] = 0;
    return 0;
}

}  // extern "C"
