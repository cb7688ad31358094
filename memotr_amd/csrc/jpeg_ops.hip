// jpeg_ops.hip -- libjpeg_ops_hip.so: the host entropy stage (jpeg_entropy_core.h, plain C++) behind a C ABI, and the
// device stage of the JPEG decoder as two gfx950 kernels (C ABI and the arithmetic: include/jpeg_ops_hip.h; the
// definition and what each stage costs: DESIGN.md, "JPEG decode").
//
// Launch 1, idct_kernel: one workgroup = 4 waves = 32 blocks, a block = 8 lanes, lane r loads row r of the block as
// one 16-byte load (8 int16) and the matching 16 bytes of the quantisation table.  The dequantised row goes to LDS
// (int32, block stride 72 words: the column reads of the four blocks of a 32-lane half fall on 32 different banks),
// lane c then reads column c, runs the column pass and writes it back in place; after a second barrier lane r reads
// row r, runs the row pass, clamps and stores 8 bytes of its component's uint8 plane.  Planes are whole MCUs wide
// and high, so no lane of a live block is out of bounds.
// Launch 2, colour_kernel: a workgroup owns 64 x 16 output pixels, a lane 4 pixels of one row: 4 Y bytes as one
// dword, the chroma samples the triangle filter needs around them (indices clamped to the TRUE chroma plane), the
// colour transform, and 12 interleaved bytes -- three dword stores where the address allows it, byte stores on the
// ragged edge.  Every pixel is checked against the true width and height.
//
// All arithmetic is 32-bit integer (built with -fwrapv: products of hostile coefficients wrap, as the numpy statement's
// do); plain vector loads and stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>
#include <thread>
#include <vector>

#include "../../include/jpeg_ops_hip.h"
#include "jpeg_entropy_core.h"

static_assert(sizeof(jpegops_info) == sizeof(jpegcore::Info), "jpegops_info and jpegcore::Info must have one layout");
static_assert(JPEGOPS_ERR_LEN == jpegcore::ERR_LEN, "error text length");
static_assert(JPEGOPS_UNSUPPORTED == (int)jpegcore::ERR_PROGRESSIVE, "first unsupported-kind code");

namespace {

thread_local char g_err[JPEGOPS_ERR_LEN] = {0};      // text of this thread's last error

int fail(int code, const char *msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));

constexpr int IDCT_THREADS = 256;
constexpr int IDCT_BLOCKS = IDCT_THREADS / 8;        // blocks per workgroup
constexpr int LDS_STRIDE = 72;                       // words per block in LDS: 64 + 8
constexpr int TILE_X = JPEGOPS_TILE_X, TILE_Y = JPEGOPS_TILE_Y;
constexpr int COLOUR_THREADS = (TILE_X / 4) * TILE_Y;

struct IdctArgs {
    const int16_t *coef;
    const uint16_t *qt;
    uint8_t *planes;
    long coef_pitch, qt_pitch, planes_pitch;
    long coef_off[3], plane_off[3];
    int first[3];                                    // index of component c's first block in the frame's block list
    int blocks_w[3];
    int total;
};

// One pass of the LL&M inverse DCT (libjpeg's jidctint.c) on 8 values, descaled by SHIFT with rounding.
template <int SHIFT>
__device__ __forceinline__ void idct_1d(const int (&x)[8], int (&o)[8]) {
    int z1 = (x[2] + x[6]) * 4433;
    const int t2 = z1 + x[6] * -15137, t3 = z1 + x[2] * 6270;
    const int t0 = (x[0] + x[4]) * 8192, t1 = (x[0] - x[4]) * 8192;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int o0 = x[7], o1 = x[5], o2 = x[3], o3 = x[1];
    z1 = o0 + o3;
    int z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
    const int z5 = (z3 + z4) * 9633;
    o0 *= 2446; o1 *= 16819; o2 *= 25172; o3 *= 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4;
    constexpr int HALF = 1 << (SHIFT - 1);
    o[0] = (t10 + o3 + HALF) >> SHIFT; o[7] = (t10 - o3 + HALF) >> SHIFT;
    o[1] = (t11 + o2 + HALF) >> SHIFT; o[6] = (t11 - o2 + HALF) >> SHIFT;
    o[2] = (t12 + o1 + HALF) >> SHIFT; o[5] = (t12 - o1 + HALF) >> SHIFT;
    o[3] = (t13 + o0 + HALF) >> SHIFT; o[4] = (t13 - o0 + HALF) >> SHIFT;
}

__device__ __forceinline__ int level(int v) { return min(max(v, 0), 255); }

__global__ __launch_bounds__(IDCT_THREADS) void idct_kernel(const IdctArgs a) {
    __shared__ __attribute__((aligned(16))) int lds[IDCT_BLOCKS * LDS_STRIDE];
    const int tid = threadIdx.x, r = tid & 7, slot = tid >> 3;
    const int g = blockIdx.x * IDCT_BLOCKS + slot;
    const bool live = g < a.total;
    const int c = !live ? 0 : (g >= a.first[2] ? 2 : (g >= a.first[1] ? 1 : 0));
    const int idx = live ? g - a.first[c] : 0;
    int *mine = lds + slot * LDS_STRIDE;

    if (live) {
        const int16_t *src = a.coef + (size_t)blockIdx.y * a.coef_pitch + a.coef_off[c] + (size_t)idx * 64 + r * 8;
        const uint16_t *q = a.qt + (size_t)blockIdx.y * a.qt_pitch + c * 64 + r * 8;
        const i32x4_t cw = *reinterpret_cast<const i32x4_t *>(src);
        const i32x4_t qw = *reinterpret_cast<const i32x4_t *>(q);
        i32x4_t lo, hi;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cv = cw[j], qv = qw[j];
            const int d0 = (int)(int16_t)(cv & 0xffff) * (qv & 0xffff);
            const int d1 = (cv >> 16) * (int)((unsigned)qv >> 16);
            if (j < 2) { lo[2 * j] = d0; lo[2 * j + 1] = d1; }
            else { hi[2 * j - 4] = d0; hi[2 * j - 3] = d1; }
        }
        *reinterpret_cast<i32x4_t *>(mine + r * 8) = lo;
        *reinterpret_cast<i32x4_t *>(mine + r * 8 + 4) = hi;
    }
    __syncthreads();
    if (live) {                                      // lane r: column r, in place
        int x[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = mine[k * 8 + r];
        idct_1d<11>(x, o);
#pragma unroll
        for (int k = 0; k < 8; ++k) mine[k * 8 + r] = o[k];
    }
    __syncthreads();
    if (live) {                                      // lane r: row r
        const i32x4_t lo = *reinterpret_cast<const i32x4_t *>(mine + r * 8);
        const i32x4_t hi = *reinterpret_cast<const i32x4_t *>(mine + r * 8 + 4);
        const int x[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        int o[8];
        idct_1d<18>(x, o);
        u32x2_t px;
        px[0] = (unsigned)level(o[0] + 128) | (unsigned)level(o[1] + 128) << 8 | (unsigned)level(o[2] + 128) << 16 |
                (unsigned)level(o[3] + 128) << 24;
        px[1] = (unsigned)level(o[4] + 128) | (unsigned)level(o[5] + 128) << 8 | (unsigned)level(o[6] + 128) << 16 |
                (unsigned)level(o[7] + 128) << 24;
        const int bw = a.blocks_w[c], by = idx / bw, bx = idx - by * bw;
        uint8_t *dst = a.planes + (size_t)blockIdx.y * a.planes_pitch + a.plane_off[c] +
                       ((size_t)by * 8 + r) * ((size_t)bw * 8) + (size_t)bx * 8;
        *reinterpret_cast<u32x2_t *>(dst) = px;
    }
}

struct ColourArgs {
    const uint8_t *planes;
    uint8_t *out;
    long planes_pitch, row_pitch, frame_pitch;
    long plane_off[3];
    int pw[3];                                       // plane widths (bytes per row)
    int W, H, cw, ch;                                // image size, true chroma plane size
    int ncomp, hshift, vshift, fancy, swap_rb;
};

// Component `p` at full resolution for pixel (x, y).
__device__ __forceinline__ int chroma_at(const ColourArgs &a, const uint8_t *p, int pw, int x, int y) {
    if (a.hshift == 0)
        return p[(size_t)y * pw + x];
    const int i = x >> 1;
    if (!a.fancy)
        return p[(size_t)(y >> a.vshift) * pw + i];
    const int il = max(i - 1, 0), ir = min(i + 1, a.cw - 1);
    if (a.vshift == 0) {
        const uint8_t *row = p + (size_t)y * pw;
        const int c = row[i];
        if (x & 1)
            return i == a.cw - 1 ? c : (3 * c + row[ir] + 2) >> 2;
        return i == 0 ? c : (3 * c + row[il] + 1) >> 2;
    }
    const int near = y >> 1, far = min(max((y & 1) ? near + 1 : near - 1, 0), a.ch - 1);
    const uint8_t *rn = p + (size_t)near * pw, *rf = p + (size_t)far * pw;
    const int s = 3 * rn[i] + rf[i];
    if (x & 1)
        return i == a.cw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * rn[ir] + rf[ir] + 7) >> 4;
    return i == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * rn[il] + rf[il] + 8) >> 4;
}

__global__ __launch_bounds__(COLOUR_THREADS) void colour_kernel(const ColourArgs a) {
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TILE_X + (tid % (TILE_X / 4)) * 4, y = blockIdx.y * TILE_Y + tid / (TILE_X / 4);
    if (y >= a.H || x0 >= a.W)
        return;
    const uint8_t *planes = a.planes + (size_t)blockIdx.z * a.planes_pitch;
    // plane rows are whole blocks wide: the dword at x0 (a multiple of 4 below W) is inside the row
    const unsigned yw = *reinterpret_cast<const unsigned *>(planes + a.plane_off[0] + (size_t)y * a.pw[0] + x0);
    const int n = min(4, a.W - x0);
    uint8_t px[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int yy = (yw >> (8 * j)) & 255;
        int r = yy, g = yy, b = yy;
        if (a.ncomp == 3 && j < n) {
            const int cb = chroma_at(a, planes + a.plane_off[1], a.pw[1], x0 + j, y) - 128;
            const int cr = chroma_at(a, planes + a.plane_off[2], a.pw[2], x0 + j, y) - 128;
            r = level(yy + ((91881 * cr + 32768) >> 16));
            b = level(yy + ((116130 * cb + 32768) >> 16));
            g = level(yy + ((-22554 * cb - 46802 * cr + 32768) >> 16));
        }
        px[3 * j] = (uint8_t)(a.swap_rb ? b : r);
        px[3 * j + 1] = (uint8_t)g;
        px[3 * j + 2] = (uint8_t)(a.swap_rb ? r : b);
    }
    uint8_t *dst = a.out + (size_t)blockIdx.z * a.frame_pitch + (size_t)y * a.row_pitch + (size_t)x0 * 3;
    if (n == 4 && ((uintptr_t)dst & 3) == 0) {
        unsigned *d = reinterpret_cast<unsigned *>(dst);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            d[k] = (unsigned)px[4 * k] | (unsigned)px[4 * k + 1] << 8 | (unsigned)px[4 * k + 2] << 16 |
                   (unsigned)px[4 * k + 3] << 24;
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (k < 3 * n)
                dst[k] = px[k];
    }
}

int check_info(const jpegops_info *f, const char *who) {
    char msg[JPEGOPS_ERR_LEN];
    const char *what = nullptr;
    if (f->width < 1 || f->height < 1 || f->width > 65535 || f->height > 65535) what = "width or height outside 1 .. 65535";
    else if (f->ncomp != 1 && f->ncomp != 3) what = "component count is not 1 or 3";
    else if (!((f->hmax == 1 && f->vmax == 1) || (f->hmax == 2 && f->vmax == 1) || (f->hmax == 2 && f->vmax == 2)))
        what = "sampling is not 1x1, 2x1 or 2x2";
    else if (f->ncomp == 1 && f->hmax != 1) what = "a one-component frame with sampling factors";
    else if (f->mcus_x != (f->width + 8 * f->hmax - 1) / (8 * f->hmax) ||
             f->mcus_y != (f->height + 8 * f->vmax - 1) / (8 * f->vmax))
        what = "MCU counts do not match the size";
    if (!what) {
        int64_t off = 0;
        for (int c = 0; c < f->ncomp && !what; ++c) {
            const int h = c == 0 ? f->hmax : 1, v = c == 0 ? f->vmax : 1;
            if (f->h[c] != h || f->v[c] != v || f->blocks_w[c] != f->mcus_x * h || f->blocks_h[c] != f->mcus_y * v ||
                f->coef_offset[c] != off)
                what = "component geometry does not match the size";
            off += (int64_t)f->blocks_w[c] * f->blocks_h[c] * 64;
        }
        if (!what && f->coef_count != off) what = "coefficient count does not match the size";
    }
    if (!what) return 0;
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return fail(2, msg);
}

int64_t planes_bytes(const jpegops_info *f) {
    int64_t n = 0;
    for (int c = 0; c < f->ncomp; ++c) n += (int64_t)f->blocks_w[c] * f->blocks_h[c] * 64;
    return n;
}

}  // namespace

extern "C" {

int jpegops_abi_version(void) { return JPEGOPS_ABI_VERSION; }
const char *jpegops_last_error(void) { return g_err; }

int jpegops_parse_header(const uint8_t *bytes, size_t n, jpegops_info *info) {
    if (!bytes || !info) return fail(1, "jpegops_parse_header: null pointer");
    return jpegcore::parse_header(bytes, n, reinterpret_cast<jpegcore::Info *>(info), g_err);
}

int jpegops_entropy_decode(const uint8_t *bytes, size_t n, jpegops_info *info, int16_t *coef_out, size_t coef_bytes,
                           uint16_t *qt_out) {
    if (!bytes || !info || !coef_out || !qt_out) return fail(1, "jpegops_entropy_decode: null pointer");
    return jpegcore::decode(bytes, n, reinterpret_cast<jpegcore::Info *>(info), coef_out, coef_bytes, qt_out, g_err);
}

int jpegops_entropy_decode_batch(const uint8_t *const *streams, const size_t *sizes, int n_frames, jpegops_info *infos,
                                 int16_t *const *coef_outs, const size_t *coef_bytes, uint16_t *const *qt_outs,
                                 int *status, char *errors, int n_threads) {
    if (n_frames < 0) return fail(-1, "jpegops_entropy_decode_batch: negative frame count"), -1;
    if (n_frames == 0) { g_err[0] = 0; return 0; }
    if (!streams || !sizes || !infos || !coef_outs || !coef_bytes || !qt_outs || !status)
        return fail(-1, "jpegops_entropy_decode_batch: null pointer"), -1;
    if (n_threads < 1) return fail(-1, "jpegops_entropy_decode_batch: fewer than 1 thread"), -1;
    int workers = n_threads < n_frames ? n_threads : n_frames;
    if (workers > JPEGOPS_MAX_THREADS) workers = JPEGOPS_MAX_THREADS;

    std::atomic<int> next(0), failed(0);
    auto work = [&]() {
        char text[JPEGOPS_ERR_LEN];
        for (int i = next.fetch_add(1); i < n_frames; i = next.fetch_add(1)) {
            text[0] = 0;
            if (!streams[i] || !coef_outs[i] || !qt_outs[i]) {
                status[i] = 1;
                snprintf(text, sizeof(text), "null pointer");
            } else {
                status[i] = jpegcore::decode(streams[i], sizes[i], reinterpret_cast<jpegcore::Info *>(infos + i),
                                             coef_outs[i], coef_bytes[i], qt_outs[i], text);
            }
            if (errors) memcpy(errors + (size_t)i * JPEGOPS_ERR_LEN, text, JPEGOPS_ERR_LEN);
            if (status[i]) failed.fetch_add(1);
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

int64_t jpegops_planes_bytes(const jpegops_info *info) {
    if (!info || check_info(info, "jpegops_planes_bytes")) return -1;
    return planes_bytes(info);
}

int jpegops_decode_pixels_u8(const int16_t *coef_dev, int64_t coef_pitch, const uint16_t *qt_dev, int64_t qt_pitch,
                             const jpegops_info *info, uint8_t *planes, int64_t planes_bytes_given, uint8_t *out,
                             int64_t row_pitch, int64_t frame_pitch, int B, int swap_rb, void *stream) {
    const char *who = "jpegops_decode_pixels_u8";
    char msg[JPEGOPS_ERR_LEN];
    auto bad = [&](int code, const char *what) {
        snprintf(msg, sizeof(msg), "%s: %s", who, what);
        return fail(code, msg);
    };
    if (B < 0) return bad(2, "negative batch size");
    if (B == 0) { g_err[0] = 0; return 0; }
    if (!coef_dev || !qt_dev || !info || !planes || !out) return bad(1, "null pointer");
    if (int rc = check_info(info, who)) return rc;
    if (((uintptr_t)coef_dev & 15) || ((uintptr_t)qt_dev & 15) || ((uintptr_t)planes & 15))
        return bad(3, "coef_dev, qt_dev or planes is not 16-byte aligned");
    if ((coef_pitch & 7) || (qt_pitch & 7)) return bad(3, "a pitch is not a multiple of 8 elements");
    if (B > 1 && (coef_pitch < info->coef_count || qt_pitch < 0)) return bad(4, "coefficient pitch below the frame's count");
    const int64_t per_frame = planes_bytes(info);
    if (planes_bytes_given < per_frame * B) return bad(5, "the planes workspace is smaller than B frames need");
    if (row_pitch < 3L * info->width) return bad(6, "row pitch smaller than 3 * width");
    if (B > 1 && frame_pitch < row_pitch * (info->height - 1) + 3L * info->width) return bad(6, "frames overlap");
    if (swap_rb != 0 && swap_rb != 1) return bad(7, "swap_rb is not 0 or 1");
    if (B > 65535) return bad(8, "more than 65535 frames");

    IdctArgs ia;
    ia.coef = coef_dev; ia.qt = qt_dev; ia.planes = planes;
    ia.coef_pitch = coef_pitch; ia.qt_pitch = qt_pitch; ia.planes_pitch = per_frame;
    int64_t blocks = 0;
    for (int c = 0; c < 3; ++c) {
        const bool on = c < info->ncomp;
        const int64_t n = on ? (int64_t)info->blocks_w[c] * info->blocks_h[c] : 0;
        ia.first[c] = on ? (int)blocks : 0x7fffffff;
        ia.coef_off[c] = on ? info->coef_offset[c] : 0;
        ia.plane_off[c] = blocks * 64;
        ia.blocks_w[c] = on ? info->blocks_w[c] : 1;
        blocks += n;
    }
    ia.total = (int)blocks;                          // at most 3 * 8192 * 8192: fits
    const dim3 igrid((unsigned)((blocks + IDCT_BLOCKS - 1) / IDCT_BLOCKS), (unsigned)B);
    hipLaunchKernelGGL(idct_kernel, igrid, dim3(IDCT_THREADS), 0, (hipStream_t)stream, ia);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return bad((int)e, hipGetErrorString(e));

    ColourArgs ca;
    ca.planes = planes; ca.out = out;
    ca.planes_pitch = per_frame; ca.row_pitch = row_pitch; ca.frame_pitch = frame_pitch;
    for (int c = 0; c < 3; ++c) {
        ca.plane_off[c] = ia.plane_off[c];
        ca.pw[c] = c < info->ncomp ? info->blocks_w[c] * 8 : 0;
    }
    ca.W = info->width; ca.H = info->height;
    ca.cw = (info->width + info->hmax - 1) / info->hmax;
    ca.ch = (info->height + info->vmax - 1) / info->vmax;
    ca.ncomp = info->ncomp; ca.hshift = info->hmax - 1; ca.vshift = info->vmax - 1;
    ca.fancy = ca.cw > 2;                            // libjpeg's rule: a plane of 1 or 2 columns is replicated
    ca.swap_rb = swap_rb;
    const dim3 cgrid((unsigned)((info->width + TILE_X - 1) / TILE_X), (unsigned)((info->height + TILE_Y - 1) / TILE_Y),
                     (unsigned)B);
    hipLaunchKernelGGL(colour_kernel, cgrid, dim3(COLOUR_THREADS), 0, (hipStream_t)stream, ca);
    e = hipGetLastError();
    if (e != hipSuccess) return bad((int)e, hipGetErrorString(e));
    g_err[0] = 0;
    return 0;
}

}  // extern "C"
