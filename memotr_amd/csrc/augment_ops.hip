// augment_ops.hip -- training-clip augmentation pixels: Pillow's 8-bit bilinear resample (two passes), optional flip,
// channel swap, HSV jitter, normalisation and padding in one gfx950 kernel (C ABI and the arithmetic:
// include/augment_ops_hip.h; the definition and where it comes from: DESIGN.md).
//
// One workgroup (4 waves) owns a tile of 16 output rows x 64 output columns of one frame.  The source bytes the tile
// reads form a rectangle: rows xmin_y[first row] .. xmin_y[last row] + cnt, columns xmin_x[first column] ..
// xmin_x[last column] + cnt (mirrored when flipping).  The workgroup
//   1. copies that rectangle into LDS as ALIGNED dwords (a row of 3-byte pixels starts on any byte: every row keeps
//      its own misalignment 0..3 in front), all loads issued before the first is needed;
//   2. runs the horizontal pass over it, one wave per source row and one lane per tile column, into a second LDS
//      image of BYTES, rounded and clamped: Pillow's intermediate;
//   3. runs the vertical pass from those bytes, one thread per row and 4 columns (12 bytes = 3 dwords per tap), and
//      the output stage in registers: either HWC bytes (the intermediate of the crop branch) or HSV jitter -> table
//      -> three fp32 planes with 16-byte stores, tiles or parts of tiles outside oh x ow storing zeros (the padding).
// A tile whose rectangle does not fit the LDS the launch was given (a reduction by more than ~3x in both axes) takes
// the direct path instead: every thread recomputes the horizontal taps of its pixels from global memory for each
// vertical tap; same arithmetic, same result.
//
// The tap counts are run-time loop bounds.  All arithmetic is 32-bit integer, the float values come out of a table:
// nothing here can be contracted or reordered.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/augment_ops_hip.h"

namespace {

thread_local char g_err[256] = {0};      // text of this thread's last error; read by augops_last_error() only

int fail(int code, const char *msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int TILE_X = 64;               // output columns per workgroup: 16 threads x 4
constexpr int TILE_Y = 16;               // output rows per workgroup
constexpr int THREADS = 256;
constexpr int MID_PITCH = TILE_X * 3;    // bytes of one row of the intermediate (a multiple of 4)
constexpr int LUT_WORDS = 3 * 256;
constexpr int HSV_WORDS = 2 * 256;
constexpr int MAX_SRC_WORDS = 10 * 1024; // 40 KB of staged source bytes
constexpr int MAX_MID_ROWS = 96;         // 18 KB of intermediate bytes

struct Args {
    const uint8_t *src;
    long row_pitch, frame_pitch;
    int T, h, w, flip, swap_rb;
    const int32_t *xmin_x, *cnt_x, *kk_x;
    const int32_t *xmin_y, *cnt_y, *kk_y;
    int ks_x, ks_y, oh, ow;
    uint8_t *out_u8;
    long out_row_pitch, out_frame_pitch;
    float *out_f32;
    int Hp, Wp;
    const float *lut;
    const int32_t *hsv_div;
    int use_hsv, dh, ds, dv, reverse;
    int mid_rows, src_words;             // LDS behind the tables: mid_rows * MID_PITCH bytes, then src_words dwords
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ int level(int acc) { return clampi(acc >> 22, 0, 255); }

// the HSV round trip of one pixel; `tab`: sdiv[256], hdiv[256]
__device__ __forceinline__ void hsv_jitter(int &r, int &g, int &b, const int32_t *tab, int dh, int ds, int dv) {
    int v = max(r, max(g, b));
    const int d = v - min(r, min(g, b));
    int s = (d * tab[v] + 2048) >> 12;
    const int h0 = v == r ? g - b : (v == g ? b - r + 2 * d : r - g + 4 * d);
    int h = (h0 * tab[256 + d] + 2048) >> 12;
    if (h < 0) h += 180;
    h = (h + dh) % 180;
    if (h < 0) h += 180;
    s = clampi(s + ds, 0, 255);
    v = clampi(v + dv, 0, 255);
    const int sec = h / 30, f = h - sec * 30, D = 7650;
    const int p = (v * (255 - s) * 30 + D / 2) / D;
    const int q = (v * (D - s * f) + D / 2) / D;
    const int t = (v * (D - s * (30 - f)) + D / 2) / D;
    switch (sec) {
        case 0: r = v; g = t; b = p; break;
        case 1: r = q; g = v; b = p; break;
        case 2: r = p; g = v; b = t; break;
        case 3: r = p; g = q; b = v; break;
        case 4: r = t; g = p; b = v; break;
        default: r = v; g = p; b = q; break;
    }
}

template <int STAGE>
__global__ __launch_bounds__(THREADS) void resample_u8_kernel(const Args a) {
    constexpr int TAB_WORDS = STAGE == AUGOPS_STAGE_F32 ? LUT_WORDS + HSV_WORDS : 0;
    extern __shared__ uint32_t smem[];
    float *lut = reinterpret_cast<float *>(smem);
    int32_t *hsv_div = reinterpret_cast<int32_t *>(smem + LUT_WORDS);
    uint32_t *mid = smem + TAB_WORDS;
    uint32_t *img = mid + a.mid_rows * (MID_PITCH / 4);

    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TILE_X, y0 = blockIdx.y * TILE_Y, t = blockIdx.z;
    const uint8_t *frame = a.src + (size_t)t * (size_t)a.frame_pitch;

    if (STAGE == AUGOPS_STAGE_F32) {
        for (int i = tid; i < LUT_WORDS; i += THREADS)
            lut[i] = a.lut[i];
        if (a.use_hsv)
            for (int i = tid; i < HSV_WORDS; i += THREADS)
                hsv_div[i] = a.hsv_div[i];
    }

    // the source rectangle of this tile (workgroup-uniform), in window coordinates: rows ry0 .. ry0 + nrows - 1,
    // columns cx0 .. cx1 - 1; in memory the columns start at sc0 (the mirror image when flipping)
    int cx0 = 0, cx1 = 1, ry0 = 0, nrows = 0, sc0 = 0, row_words = 0;
    bool staged = false;
    if (x0 < a.ow && y0 < a.oh) {
        const int xl = min(x0 + TILE_X, a.ow) - 1, yl = min(y0 + TILE_Y, a.oh) - 1;
        cx0 = clampi(a.xmin_x[x0], 0, a.w - 1);
        cx1 = clampi(a.xmin_x[xl] + a.cnt_x[xl], cx0 + 1, a.w);
        ry0 = clampi(a.xmin_y[y0], 0, a.h - 1);
        nrows = clampi(a.xmin_y[yl] + a.cnt_y[yl], ry0 + 1, a.h) - ry0;
        sc0 = a.flip ? a.w - cx1 : cx0;
        const int len = (cx1 - cx0) * 3;                    // bytes of one row
        row_words = (len + 3) / 4 + 1;                      // the misalignment in front is at most 3 bytes
        staged = nrows <= a.mid_rows && (long)nrows * row_words <= (long)a.src_words;
        if (staged) {
            const int total = nrows * row_words;
            for (int i = tid; i < total; i += THREADS) {
                const int r = i / row_words, d = i - r * row_words;
                const uint8_t *first = frame + (size_t)(ry0 + r) * (size_t)a.row_pitch + (size_t)sc0 * 3;
                const int mis = (int)((uintptr_t)first & 3);
                if (d * 4 < mis + len)                      // a dword is loaded only if it holds a byte of the row
                    img[i] = reinterpret_cast<const uint32_t *>(first - mis)[d];
            }
        }
    }
    __syncthreads();

    if (staged) {                                           // horizontal pass: LDS dwords -> LDS bytes
        const uint8_t *bytes = reinterpret_cast<const uint8_t *>(img);
        uint8_t *midb = reinterpret_cast<uint8_t *>(mid);
        const int tcols = min(TILE_X, a.ow - x0);
        const int total = nrows * TILE_X;
        for (int i = tid; i < total; i += THREADS) {
            const int r = i / TILE_X, xc = i - r * TILE_X;
            if (xc >= tcols)
                continue;
            const int x = x0 + xc;
            const int xm = a.xmin_x[x], cnt = min(a.cnt_x[x], a.ks_x);
            const int32_t *kk = a.kk_x + (size_t)x * (size_t)a.ks_x;
            const uint8_t *first = frame + (size_t)(ry0 + r) * (size_t)a.row_pitch + (size_t)sc0 * 3;
            const uint8_t *row = bytes + r * row_words * 4 + (int)((uintptr_t)first & 3);
            int acc[3] = {1 << 21, 1 << 21, 1 << 21};
            for (int k = 0; k < cnt; ++k) {
                const int col = clampi(xm + k, cx0, cx1 - 1);
                const uint8_t *p = row + ((a.flip ? a.w - 1 - col : col) - sc0) * 3;
                const int wgt = kk[k];
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    acc[c] += (int)p[a.swap_rb ? 2 - c : c] * wgt;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c)
                midb[r * MID_PITCH + xc * 3 + c] = (uint8_t)level(acc[c]);
        }
    }
    __syncthreads();

    const int y = y0 + (tid >> 4), x = x0 + 4 * (tid & 15);
    const bool live = y < a.oh && x < a.ow;
    int q[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            q[j][c] = 1 << 21;
    if (live) {                                             // vertical pass
        const int ym = a.xmin_y[y], cnt = min(a.cnt_y[y], a.ks_y);
        const int32_t *kk = a.kk_y + (size_t)y * (size_t)a.ks_y;
        if (staged) {
            for (int k = 0; k < cnt; ++k) {
                const int r = clampi(ym + k, ry0, ry0 + nrows - 1) - ry0;
                const uint32_t *m = mid + r * (MID_PITCH / 4) + 3 * (tid & 15);
                const uint32_t d[3] = {m[0], m[1], m[2]};
                const int wgt = kk[k];
#pragma unroll
                for (int i = 0; i < 12; ++i)
                    q[i / 3][i % 3] += (int)((d[i / 4] >> (8 * (i % 4))) & 255u) * wgt;
            }
        } else {
            for (int k = 0; k < cnt; ++k) {
                const uint8_t *row = frame + (size_t)clampi(ym + k, 0, a.h - 1) * (size_t)a.row_pitch;
                const int wgt = kk[k];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int xi = x + j;
                    if (xi >= a.ow)
                        continue;
                    const int xm = a.xmin_x[xi], cntx = min(a.cnt_x[xi], a.ks_x);
                    const int32_t *kkx = a.kk_x + (size_t)xi * (size_t)a.ks_x;
                    int acc[3] = {1 << 21, 1 << 21, 1 << 21};
                    for (int kx = 0; kx < cntx; ++kx) {
                        const int col = clampi(xm + kx, 0, a.w - 1);
                        const uint8_t *p = row + (size_t)(a.flip ? a.w - 1 - col : col) * 3;
                        const int wx = kkx[kx];
#pragma unroll
                        for (int c = 0; c < 3; ++c)
                            acc[c] += (int)p[a.swap_rb ? 2 - c : c] * wx;
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        q[j][c] += level(acc[c]) * wgt;
                }
            }
        }
    }

    if (STAGE == AUGOPS_STAGE_U8) {
        if (!live)
            return;
        uint8_t *dst = a.out_u8 + (size_t)t * (size_t)a.out_frame_pitch + (size_t)y * (size_t)a.out_row_pitch;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x + j < a.ow) {
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    dst[(size_t)(x + j) * 3 + c] = (uint8_t)level(q[j][c]);
            }
    } else {
        if (y >= a.Hp || x >= a.Wp)
            return;
        f32x4_t o[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        if (live) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (x + j >= a.ow)
                    continue;                               // right padding inside a live quad stays 0
                int r = level(q[j][0]), g = level(q[j][1]), b = level(q[j][2]);
                if (a.use_hsv)
                    hsv_jitter(r, g, b, hsv_div, a.dh, a.ds, a.dv);
                o[0][j] = lut[r & 255];
                o[1][j] = lut[256 + (g & 255)];
                o[2][j] = lut[512 + (b & 255)];
            }
        }
        const size_t plane = (size_t)a.Hp * (size_t)a.Wp;
        const int to = a.reverse ? a.T - 1 - t : t;
        float *dst = a.out_f32 + (size_t)to * 3 * plane + (size_t)y * (size_t)a.Wp + (size_t)x;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            *reinterpret_cast<f32x4_t *>(dst + c * plane) = o[c];
    }
}

long min_l(long a, long b) { return a < b ? a : b; }

}  // namespace

extern "C" {

int augops_abi_version(void) { return AUGOPS_ABI_VERSION; }
const char *augops_last_error(void) { return g_err; }

int augops_resample_u8(const uint8_t *src, long row_pitch, long frame_pitch, int T, int h, int w, int flip, int swap_rb,
                       const int32_t *xmin_x, const int32_t *cnt_x, const int32_t *kk_x, int ksize_x,
                       const int32_t *xmin_y, const int32_t *cnt_y, const int32_t *kk_y, int ksize_y,
                       int oh, int ow, int stage,
                       uint8_t *out_u8, long out_row_pitch, long out_frame_pitch,
                       float *out_f32, int Hp, int Wp, const float *lut, const int32_t *hsv_div, int use_hsv,
                       int dh, int ds, int dv, int reverse, void *stream) {
    if (T < 0) return fail(2, "augops_resample_u8: negative frame count");
    if (T == 0) { g_err[0] = 0; return 0; }
    if (stage != AUGOPS_STAGE_U8 && stage != AUGOPS_STAGE_F32)
        return fail(3, "augops_resample_u8: stage is not AUGOPS_STAGE_U8 or AUGOPS_STAGE_F32");
    const bool f32 = stage == AUGOPS_STAGE_F32;
    if (!src || !xmin_x || !cnt_x || !kk_x || !xmin_y || !cnt_y || !kk_y)
        return fail(1, "augops_resample_u8: null pointer");
    if (f32 ? (!out_f32 || !lut) : !out_u8) return fail(1, "augops_resample_u8: null pointer");
    if (h <= 0 || w <= 0 || oh <= 0 || ow <= 0) return fail(2, "augops_resample_u8: non-positive size");
    if (ksize_x <= 0 || ksize_y <= 0) return fail(4, "augops_resample_u8: non-positive tap count");
    if ((flip != 0 && flip != 1) || (swap_rb != 0 && swap_rb != 1))
        return fail(5, "augops_resample_u8: flip or swap_rb is not 0 or 1");
    if (row_pitch < 3L * w) return fail(6, "augops_resample_u8: row pitch smaller than 3 * w");
    if (T > 1 && frame_pitch < 0) return fail(6, "augops_resample_u8: negative frame pitch");
    if (f32) {
        if (Hp <= 0 || Wp <= 0) return fail(2, "augops_resample_u8: non-positive size");
        if (Hp < oh || Wp < ow) return fail(7, "augops_resample_u8: padded size smaller than the output size");
        if (Wp % 4 != 0) return fail(8, "augops_resample_u8: Wp is not a multiple of 4");
        if (((uintptr_t)out_f32 & 15) != 0) return fail(9, "augops_resample_u8: out_f32 is not 16-byte aligned");
        if ((use_hsv != 0 && use_hsv != 1) || (reverse != 0 && reverse != 1))
            return fail(5, "augops_resample_u8: use_hsv or reverse is not 0 or 1");
        if (use_hsv && !hsv_div) return fail(1, "augops_resample_u8: null pointer");
        if (use_hsv && (dh < -32768 || dh > 32768 || ds < -32768 || ds > 32768 || dv < -32768 || dv > 32768))
            return fail(10, "augops_resample_u8: HSV gain outside +-32768");
    } else {
        if (out_row_pitch < 3L * ow) return fail(6, "augops_resample_u8: output row pitch smaller than 3 * ow");
        if (T > 1 && out_frame_pitch < 0) return fail(6, "augops_resample_u8: negative output frame pitch");
    }
    const int gh = f32 ? Hp : oh, gw = f32 ? Wp : ow;
    const long gy = ((long)gh + TILE_Y - 1) / TILE_Y;
    if (T > 65535 || gy > 65535) return fail(11, "augops_resample_u8: more than 65535 frames or row tiles");

    // LDS for the largest source rectangle a tile of these tables can need: a filter of ksize taps has a support of
    // (ksize - 1) / 2 >= the scale factor, so TILE outputs span at most (TILE + 1) * support + 2 inputs (an upper
    // bound; the kernel checks each tile's own rectangle against what it was given)
    const long rows = min_l((long)(TILE_Y + 1) * ((ksize_y - 1) / 2) + 2, h);
    const long cols = min_l((long)(TILE_X + 1) * ((ksize_x - 1) / 2) + 2, w);
    const long mid_rows = min_l(rows, MAX_MID_ROWS);
    const long src_words = min_l(rows * ((cols * 3 + 3) / 4 + 1), MAX_SRC_WORDS);

    Args a;
    a.src = src; a.row_pitch = row_pitch; a.frame_pitch = frame_pitch; a.T = T; a.h = h; a.w = w;
    a.flip = flip; a.swap_rb = swap_rb;
    a.xmin_x = xmin_x; a.cnt_x = cnt_x; a.kk_x = kk_x; a.xmin_y = xmin_y; a.cnt_y = cnt_y; a.kk_y = kk_y;
    a.ks_x = ksize_x; a.ks_y = ksize_y; a.oh = oh; a.ow = ow;
    a.out_u8 = out_u8; a.out_row_pitch = out_row_pitch; a.out_frame_pitch = out_frame_pitch;
    a.out_f32 = out_f32; a.Hp = Hp; a.Wp = Wp; a.lut = lut; a.hsv_div = hsv_div;
    a.use_hsv = f32 ? use_hsv : 0; a.dh = dh; a.ds = ds; a.dv = dv; a.reverse = f32 ? reverse : 0;
    a.mid_rows = (int)mid_rows; a.src_words = (int)src_words;
    const dim3 grid((unsigned)((gw + TILE_X - 1) / TILE_X), (unsigned)gy, (unsigned)T);
    const size_t lds = ((f32 ? LUT_WORDS + HSV_WORDS : 0) + mid_rows * (MID_PITCH / 4) + src_words) * 4;
    if (f32)
        hipLaunchKernelGGL(resample_u8_kernel<AUGOPS_STAGE_F32>, grid, dim3(THREADS), lds, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(resample_u8_kernel<AUGOPS_STAGE_U8>, grid, dim3(THREADS), lds, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "augops_resample_u8: %s", hipGetErrorString(e));
        return (int)e;
    }
    g_err[0] = 0;
    return 0;
}

}  // extern "C"
