// jpeg_enc.hip -- libjpeg_enc_hip.so: the device stage of the baseline JPEG encoder as two gfx950 kernels, and the
// host Huffman stage (jpeg_encode_core.h, plain C++) behind a C ABI (include/jpeg_enc_hip.h; the definition and what
// each launch reads and writes: DESIGN.md 5.8).  The mirror image of jpeg_ops.hip.
//
// Launch 1, ycc_kernel: a workgroup owns 64 x 16 luma samples of the whole-MCU plane, a lane 4 samples of one row.
// It reads 12 interleaved bytes (three dwords where the quad is whole and the address allows it, clamped byte loads
// on the ragged edge: the clamping IS the edge replication), writes 4 Y bytes as one dword and, in 4:4:4, 4 Cb and
// 4 Cr bytes the same way.  In 4:2:0 the lanes of even rows also own the two chroma samples under their quad: the
// 2 x 2 averages of the Cb / Cr of source rows 2 * cy' and min(2 * cy' + 1, H - 1), cy' = min(cy, ceil(H / 2) - 1)
// (block rows below the image replicate the last DOWNSAMPLED row), bias 1, 2 along the columns; 2 bytes per plane.
// Launch 2, fdct_quant_kernel: one workgroup = 4 waves = 32 blocks, a block = 8 lanes.  Lane r loads row r of the
// block (8 bytes), runs the row pass on samples - 128 and stores it to LDS (int32, block stride 72 words, as the
// decoder's IDCT); lane c then reads column c, runs the column pass, quantises against the table (copied from the
// kernel arguments to LDS once per workgroup) and writes back in place; lane r finally packs row r as 8 int16 and
// stores 16 bytes.  A dummy luma block of 4:2:0 (beyond ceil(W / 8) columns or ceil(H / 8) rows) transforms the real
// block its DC comes from and keeps only that DC: no block depends on another block's output.
//
// All arithmetic is 32-bit integer; plain vector loads and stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>
#include <thread>
#include <vector>

#include "../../include/jpeg_enc_hip.h"
#include "jpeg_encode_core.h"

static_assert(sizeof(jpegenc_info) == sizeof(jpegenc::Info), "jpegenc_info and jpegenc::Info must have one layout");

namespace {

thread_local char g_err[JPEGENC_ERR_LEN] = {0};      // text of this thread's last error

int fail(int code, const char *msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));

constexpr int FDCT_THREADS = 256;
constexpr int FDCT_BLOCKS = FDCT_THREADS / 8;        // blocks per workgroup
constexpr int LDS_STRIDE = 72;                       // words per block in LDS: 64 + 8
constexpr int TILE_X = JPEGENC_TILE_X, TILE_Y = JPEGENC_TILE_Y;
constexpr int YCC_THREADS = (TILE_X / 4) * TILE_Y;

struct YccArgs {
    const uint8_t *frame;
    uint8_t *planes;
    long row_pitch, frame_pitch, planes_pitch;
    long plane_off[3];
    int W, H, PW, PH;                                // image size, luma plane size (whole MCUs)
    int sub, ch, swap_rb;                            // sub: 1 for 4:2:0; ch: ceil(H / 2)
};

struct Quad { int r[4], g[4], b[4]; };

// Pixels (x0 .. x0 + 3, y) of the frame, x clamped to W - 1 (y is already inside).
__device__ __forceinline__ void load_quad(const YccArgs &a, const uint8_t *frame, int x0, int y, Quad &q) {
    const uint8_t *row = frame + (size_t)y * a.row_pitch;
    const uint8_t *p = row + (size_t)x0 * 3;
    uint8_t px[12];
    if (x0 + 3 < a.W && ((uintptr_t)p & 3) == 0) {
        const unsigned *d = reinterpret_cast<const unsigned *>(p);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned w = d[k];
            px[4 * k] = w & 255; px[4 * k + 1] = (w >> 8) & 255; px[4 * k + 2] = (w >> 16) & 255; px[4 * k + 3] = w >> 24;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint8_t *s = row + (size_t)min(x0 + j, a.W - 1) * 3;
            px[3 * j] = s[0]; px[3 * j + 1] = s[1]; px[3 * j + 2] = s[2];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        q.r[j] = px[3 * j + (a.swap_rb ? 2 : 0)];
        q.g[j] = px[3 * j + 1];
        q.b[j] = px[3 * j + (a.swap_rb ? 0 : 2)];
    }
}

__device__ __forceinline__ int to_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__device__ __forceinline__ int to_cb(int r, int g, int b) {
    return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
}
__device__ __forceinline__ int to_cr(int r, int g, int b) {
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

__global__ __launch_bounds__(YCC_THREADS) void ycc_kernel(const YccArgs a) {
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TILE_X + (tid % (TILE_X / 4)) * 4, y = blockIdx.y * TILE_Y + tid / (TILE_X / 4);
    if (y >= a.PH || x0 >= a.PW)                     // PW is a multiple of 8: a quad is inside whole or not at all
        return;
    const uint8_t *frame = a.frame + (size_t)blockIdx.z * a.frame_pitch;
    uint8_t *planes = a.planes + (size_t)blockIdx.z * a.planes_pitch;
    const int sy = min(y, a.H - 1);
    Quad q;
    load_quad(a, frame, x0, sy, q);
    unsigned yw = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) yw |= (unsigned)to_y(q.r[j], q.g[j], q.b[j]) << (8 * j);
    *reinterpret_cast<unsigned *>(planes + a.plane_off[0] + (size_t)y * a.PW + x0) = yw;
    if (!a.sub) {
        unsigned bw = 0, rw = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bw |= (unsigned)to_cb(q.r[j], q.g[j], q.b[j]) << (8 * j);
            rw |= (unsigned)to_cr(q.r[j], q.g[j], q.b[j]) << (8 * j);
        }
        *reinterpret_cast<unsigned *>(planes + a.plane_off[1] + (size_t)y * a.PW + x0) = bw;
        *reinterpret_cast<unsigned *>(planes + a.plane_off[2] + (size_t)y * a.PW + x0) = rw;
        return;
    }
    if (y & 1)
        return;
    const int cy = y >> 1, cye = min(cy, a.ch - 1);
    const int r0 = 2 * cye, r1 = min(r0 + 1, a.H - 1);   // r0 <= H - 1 because cye <= ceil(H / 2) - 1
    Quad top, bot;
    if (r0 == sy) top = q;
    else load_quad(a, frame, x0, r0, top);
    load_quad(a, frame, x0, r1, bot);
    unsigned bw = 0, rw = 0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        int sb = 1 + k, sr = 1 + k;                  // the bias: 1, 2, 1, 2 ... along the output columns
#pragma unroll
        for (int j = 2 * k; j < 2 * k + 2; ++j) {
            sb += to_cb(top.r[j], top.g[j], top.b[j]) + to_cb(bot.r[j], bot.g[j], bot.b[j]);
            sr += to_cr(top.r[j], top.g[j], top.b[j]) + to_cr(bot.r[j], bot.g[j], bot.b[j]);
        }
        bw |= (unsigned)(sb >> 2) << (8 * k);
        rw |= (unsigned)(sr >> 2) << (8 * k);
    }
    const size_t at = (size_t)cy * (a.PW >> 1) + (x0 >> 1);
    *reinterpret_cast<uint16_t *>(planes + a.plane_off[1] + at) = (uint16_t)bw;
    *reinterpret_cast<uint16_t *>(planes + a.plane_off[2] + at) = (uint16_t)rw;
}

struct FdctArgs {
    const uint8_t *planes;
    int16_t *coef;
    long planes_pitch, coef_pitch;
    long plane_off[3], coef_off[3];
    int first[3];                                    // index of component c's first block in the frame's block list
    int blocks_w[3];
    int total;
    int wb, hb, sub;                                 // real luma blocks: ceil(W / 8), ceil(H / 8); sub: 1 for 4:2:0
    uint8_t qt[128];                                 // luma, chroma; natural order
};

// One pass of the LL&M forward DCT (libjpeg's jfdctint.c) on 8 values.  ROWS: outputs 0 and 4 scaled up by 2 bits,
// the others descaled by 11; columns: 0 and 4 descaled by 2, the others by 15; all with rounding.
template <bool ROWS>
__device__ __forceinline__ void fdct_1d(const int (&d)[8], int (&o)[8]) {
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int SHIFT = ROWS ? 11 : 15, HALF = 1 << (SHIFT - 1);
    if (ROWS) {
        o[0] = (t10 + t11) << 2;
        o[4] = (t10 - t11) << 2;
    } else {
        o[0] = (t10 + t11 + 2) >> 2;
        o[4] = (t10 - t11 + 2) >> 2;
    }
    int z1 = (t12 + t13) * 4433;
    o[2] = (z1 + t13 * 6270 + HALF) >> SHIFT;
    o[6] = (z1 + t12 * -15137 + HALF) >> SHIFT;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int m4 = t4 * 2446, m5 = t5 * 16819, m6 = t6 * 25172, m7 = t7 * 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    o[7] = (m4 + z1 + z3 + HALF) >> SHIFT;
    o[5] = (m5 + z2 + z4 + HALF) >> SHIFT;
    o[3] = (m6 + z2 + z3 + HALF) >> SHIFT;
    o[1] = (m7 + z1 + z4 + HALF) >> SHIFT;
}

__global__ __launch_bounds__(FDCT_THREADS) void fdct_quant_kernel(const FdctArgs a) {
    __shared__ __attribute__((aligned(16))) int lds[FDCT_BLOCKS * LDS_STRIDE];
    __shared__ int qt[128];
    const int tid = threadIdx.x, r = tid & 7, slot = tid >> 3;
    if (tid < 128) qt[tid] = a.qt[tid];
    const int g = blockIdx.x * FDCT_BLOCKS + slot;
    const bool live = g < a.total;
    const int c = !live ? 0 : (g >= a.first[2] ? 2 : (g >= a.first[1] ? 1 : 0));
    const int idx = live ? g - a.first[c] : 0;
    const int bw = a.blocks_w[c], by = idx / bw, bx = idx - by * bw;
    int sby = by, sbx = bx;
    bool dummy = false;
    if (c == 0 && a.sub) {                           // the block a dummy takes its DC from; itself when real
        dummy = by >= a.hb || bx >= a.wb;
        sby = min(by, a.hb - 1);
        sbx = min(by < a.hb ? bx : (bx | 1), a.wb - 1);
    }
    int *mine = lds + slot * LDS_STRIDE;

    if (live) {                                      // lane r: row r
        const uint8_t *src = a.planes + (size_t)blockIdx.y * a.planes_pitch + a.plane_off[c] +
                             ((size_t)sby * 8 + r) * ((size_t)bw * 8) + (size_t)sbx * 8;
        const u32x2_t px = *reinterpret_cast<const u32x2_t *>(src);
        int d[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = (int)((px[k >> 2] >> (8 * (k & 3))) & 255) - 128;
        fdct_1d<true>(d, o);
        i32x4_t lo = {o[0], o[1], o[2], o[3]}, hi = {o[4], o[5], o[6], o[7]};
        *reinterpret_cast<i32x4_t *>(mine + r * 8) = lo;
        *reinterpret_cast<i32x4_t *>(mine + r * 8 + 4) = hi;
    }
    __syncthreads();
    if (live) {                                      // lane r: column r, in place, quantised
        int x[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = mine[k * 8 + r];
        fdct_1d<false>(x, o);
        const int *q = qt + (c ? 64 : 0);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const unsigned dq = (unsigned)q[k * 8 + r] << 3;
            const unsigned mag = ((unsigned)abs(o[k]) + (dq >> 1)) / dq;
            int v = o[k] < 0 ? -(int)mag : (int)mag;
            if (dummy && (k | r)) v = 0;
            mine[k * 8 + r] = v;
        }
    }
    __syncthreads();
    if (live) {                                      // lane r: row r, 8 int16 as one 16-byte store
        const i32x4_t lo = *reinterpret_cast<const i32x4_t *>(mine + r * 8);
        const i32x4_t hi = *reinterpret_cast<const i32x4_t *>(mine + r * 8 + 4);
        i32x4_t w;
        w[0] = (lo[0] & 0xffff) | (int)((unsigned)lo[1] << 16);
        w[1] = (lo[2] & 0xffff) | (int)((unsigned)lo[3] << 16);
        w[2] = (hi[0] & 0xffff) | (int)((unsigned)hi[1] << 16);
        w[3] = (hi[2] & 0xffff) | (int)((unsigned)hi[3] << 16);
        int16_t *dst = a.coef + (size_t)blockIdx.y * a.coef_pitch + a.coef_off[c] + (size_t)idx * 64 + r * 8;
        *reinterpret_cast<i32x4_t *>(dst) = w;
    }
}

int check_info(const jpegenc_info *f, const char *who) {
    if (jpegenc::check_info(reinterpret_cast<const jpegenc::Info *>(f)) == 0) return 0;
    char msg[JPEGENC_ERR_LEN];
    snprintf(msg, sizeof(msg), "%s: the geometry is not the one jpegenc_geometry makes (4:4:4 or 4:2:0, 1 .. 65535)", who);
    return fail(2, msg);
}

}  // namespace

extern "C" {

int jpegenc_abi_version(void) { return JPEGENC_ABI_VERSION; }
const char *jpegenc_last_error(void) { return g_err; }

int jpegenc_geometry(int width, int height, int hmax, jpegenc_info *info) {
    if (!info) return fail(1, "jpegenc_geometry: null pointer");
    if (jpegenc::geometry(width, height, hmax, reinterpret_cast<jpegenc::Info *>(info)))
        return fail(2, "jpegenc_geometry: width or height outside 1 .. 65535, or sampling that is not 1 or 2");
    g_err[0] = 0;
    return 0;
}

int jpegenc_quant_tables(int quality, uint16_t *qt_out) {
    if (!qt_out) return fail(1, "jpegenc_quant_tables: null pointer");
    if (jpegenc::quant_tables(quality, qt_out)) return fail(2, "jpegenc_quant_tables: quality outside 1 .. 100");
    g_err[0] = 0;
    return 0;
}

int64_t jpegenc_huffman_encode(const int16_t *coef, const uint16_t *qt, const jpegenc_info *info, uint8_t *out,
                               size_t cap) {
    if (!coef || !qt || !info || (!out && cap)) return fail(-1, "jpegenc_huffman_encode: null pointer");
    const int64_t n = jpegenc::encode(coef, qt, reinterpret_cast<const jpegenc::Info *>(info), out, cap);
    if (n == -1) return fail(-1, "jpegenc_huffman_encode: the geometry is not the one jpegenc_geometry makes");
    if (n == -2) return fail(-2, "jpegenc_huffman_encode: a quantisation table entry outside 1 .. 255");
    if (n == -3) return fail(-3, "jpegenc_huffman_encode: a coefficient that baseline coding cannot express");
    g_err[0] = 0;
    return n;
}

int jpegenc_huffman_encode_batch(const int16_t *const *coefs, const uint16_t *const *qts, const jpegenc_info *info,
                                 int n_frames, uint8_t *const *outs, const size_t *caps, int64_t *sizes,
                                 int n_threads) {
    if (n_frames < 0) return fail(-1, "jpegenc_huffman_encode_batch: negative frame count"), -1;
    if (n_frames == 0) { g_err[0] = 0; return 0; }
    if (!coefs || !qts || !info || !outs || !caps || !sizes)
        return fail(-1, "jpegenc_huffman_encode_batch: null pointer"), -1;
    if (n_threads < 1) return fail(-1, "jpegenc_huffman_encode_batch: fewer than 1 thread"), -1;
    int workers = n_threads < n_frames ? n_threads : n_frames;
    if (workers > JPEGENC_MAX_THREADS) workers = JPEGENC_MAX_THREADS;

    std::atomic<int> next(0), failed(0);
    auto work = [&]() {
        for (int i = next.fetch_add(1); i < n_frames; i = next.fetch_add(1)) {
            if (!coefs[i] || !qts[i] || (!outs[i] && caps[i]))
                sizes[i] = -1;
            else
                sizes[i] = jpegenc::encode(coefs[i], qts[i], reinterpret_cast<const jpegenc::Info *>(info), outs[i],
                                           caps[i]);
            if (sizes[i] < 0 || (uint64_t)sizes[i] > caps[i]) failed.fetch_add(1);
        }
    };
    if (workers == 1) {
        work();
    } else {
        std::vector<std::thread> pool;
        pool.reserve(workers - 1);
        for (int t = 1; t < workers; ++t) pool.emplace_back(work);
        work();
        for (auto &t : pool) t.join();
    }
    g_err[0] = 0;
    return failed.load();
}

int64_t jpegenc_planes_bytes(const jpegenc_info *info) {
    if (!info || check_info(info, "jpegenc_planes_bytes")) return -1;
    return info->coef_count;                         // a byte per coefficient: the planes are whole blocks
}

int jpegenc_forward_u8(const uint8_t *frame, int64_t row_pitch, int64_t frame_pitch, const jpegenc_info *info,
                       const uint16_t *qt, uint8_t *planes, int64_t planes_bytes_given, int16_t *coef_dev,
                       int64_t coef_pitch, int B, int swap_rb, void *stream) {
    const char *who = "jpegenc_forward_u8";
    char msg[JPEGENC_ERR_LEN];
    auto bad = [&](int code, const char *what) {
        snprintf(msg, sizeof(msg), "%s: %s", who, what);
        return fail(code, msg);
    };
    if (B < 0) return bad(2, "negative batch size");
    if (B == 0) { g_err[0] = 0; return 0; }
    if (!frame || !info || !qt || !planes || !coef_dev) return bad(1, "null pointer");
    if (int rc = check_info(info, who)) return rc;
    if (((uintptr_t)coef_dev & 15) || ((uintptr_t)planes & 15)) return bad(3, "coef_dev or planes is not 16-byte aligned");
    if (coef_pitch & 7) return bad(3, "the coefficient pitch is not a multiple of 8 elements");
    if (B > 1 && coef_pitch < info->coef_count) return bad(4, "coefficient pitch below the frame's count");
    const int64_t per_frame = info->coef_count;
    if (planes_bytes_given < per_frame * B) return bad(5, "the planes workspace is smaller than B frames need");
    if (row_pitch < 3L * info->width) return bad(6, "row pitch smaller than 3 * width");
    if (B > 1 && frame_pitch < row_pitch * (info->height - 1) + 3L * info->width) return bad(6, "frames overlap");
    if (swap_rb != 0 && swap_rb != 1) return bad(7, "swap_rb is not 0 or 1");
    if (B > 65535) return bad(8, "more than 65535 frames");
    for (int k = 0; k < 128; ++k)
        if (qt[k] < 1 || qt[k] > 255) return bad(9, "a quantisation table entry outside 1 .. 255");

    YccArgs ya;
    ya.frame = frame; ya.planes = planes;
    ya.row_pitch = row_pitch; ya.frame_pitch = frame_pitch; ya.planes_pitch = per_frame;
    ya.W = info->width; ya.H = info->height;
    ya.PW = info->blocks_w[0] * 8; ya.PH = info->blocks_h[0] * 8;
    ya.sub = info->hmax - 1; ya.ch = (info->height + 1) / 2; ya.swap_rb = swap_rb;

    FdctArgs fa;
    fa.planes = planes; fa.coef = coef_dev;
    fa.planes_pitch = per_frame; fa.coef_pitch = coef_pitch;
    int64_t blocks = 0;
    for (int c = 0; c < 3; ++c) {
        fa.first[c] = (int)blocks;
        fa.coef_off[c] = info->coef_offset[c];
        fa.plane_off[c] = ya.plane_off[c] = blocks * 64;
        fa.blocks_w[c] = info->blocks_w[c];
        blocks += (int64_t)info->blocks_w[c] * info->blocks_h[c];
    }
    fa.total = (int)blocks;                          // at most 3 * 8192 * 8192: fits
    fa.wb = (info->width + 7) / 8; fa.hb = (info->height + 7) / 8; fa.sub = ya.sub;
    for (int k = 0; k < 128; ++k) fa.qt[k] = (uint8_t)qt[k];

    const dim3 ygrid((unsigned)((ya.PW + TILE_X - 1) / TILE_X), (unsigned)((ya.PH + TILE_Y - 1) / TILE_Y), (unsigned)B);
    hipLaunchKernelGGL(ycc_kernel, ygrid, dim3(YCC_THREADS), 0, (hipStream_t)stream, ya);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return bad((int)e, hipGetErrorString(e));
    const dim3 fgrid((unsigned)((blocks + FDCT_BLOCKS - 1) / FDCT_BLOCKS), (unsigned)B);
    hipLaunchKernelGGL(fdct_quant_kernel, fgrid, dim3(FDCT_THREADS), 0, (hipStream_t)stream, fa);
    e = hipGetLastError();
    if (e != hipSuccess) return bad((int)e, hipGetErrorString(e));
    g_err[0] = 0;
    return 0;
}

}  // extern "C"
