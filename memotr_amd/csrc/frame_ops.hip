// frame_ops.hip -- raw video frame (uint8, H x W x 3) -> padded, normalised fp32 planes in one gfx950 kernel
// (C ABI and the arithmetic: include/frame_ops_hip.h; the definition and where it comes from: DESIGN.md).
//
// One workgroup (4 waves) owns a tile of 4 output rows x 256 output columns of one frame.  The source bytes the tile
// reads form a rectangle: rows s0y[first row] .. s1y[last row], bytes 3*s0x[first column] .. 3*s1x[last column]+2.  The
// workgroup copies that rectangle into LDS as ALIGNED dwords (a row of 3-byte pixels starts on any byte, and so does
// each of its rows when the pitch is not a multiple of 4: every row keeps its own misalignment 0..3 in front), all
// loads issued before the first is needed; then wave k computes output row k, lane l the columns 4l..4l+3 of the
// tile, from LDS bytes, and stores 16 bytes per plane.  Tiles or parts of tiles outside th x tw store zeros: the
// padding is written in the same pass.  A tile whose rectangle does not fit the LDS the launch was given (a
// reduction by more than ~5x) reads its bytes from global memory instead; same arithmetic, same result.
//
// All arithmetic is 32-bit integer, the float values come out of a table: nothing here can be contracted or reordered.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/frame_ops_hip.h"

namespace {

thread_local char g_err[256] = {0};      // text of this thread's last error; read by frameops_last_error() only

int fail(int code, const char *msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int TILE_X = 256;              // output columns per workgroup: 64 lanes x 4
constexpr int TILE_Y = 4;                // output rows per workgroup: one per wave
constexpr int THREADS = 64 * TILE_Y;
constexpr int LUT_WORDS = 3 * 256;
constexpr int MAX_LDS_BYTES = 60 * 1024;

struct Args {
    const uint8_t *src;
    long row_pitch, frame_pitch;
    int h, w;
    const int32_t *s0x, *s1x;
    const int16_t *a1x;
    const int32_t *s0y, *s1y;
    const int16_t *b1y;
    int th, tw, Hp, Wp;
    const float *lut;
    int swap_rb;
    float *out;
    int img_words;                       // dwords of LDS behind the table
};

// The four columns of one lane for the three channels.  `p0` / `p1`: byte 0 of source column 0 of the two source rows
// (LDS image or global memory: the address space follows the caller's pointer after inlining).
template <typename P>
__device__ __forceinline__ void four_columns(const Args &a, P p0, P p1, int b0, int b1, int x, const float *lut,
                                             f32x4_t (&o)[3]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int xi = x + j;
        if (xi >= a.tw)
            continue;                    // right padding inside a live quad stays 0
        const int i0 = a.s0x[xi] * 3, i1 = a.s1x[xi] * 3;
        const int a1 = a.a1x[xi], a0 = 2048 - a1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int sc = a.swap_rb ? 2 - c : c;
            const int r0 = (int)p0[i0 + sc] * a0 + (int)p0[i1 + sc] * a1;
            const int r1 = (int)p1[i0 + sc] * a0 + (int)p1[i1 + sc] * a1;
            const int q = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
            o[c][j] = lut[c * 256 + (q & 255)];
        }
    }
}

__global__ __launch_bounds__(THREADS) void resize_normalize_u8_kernel(const Args a) {
    extern __shared__ uint32_t smem[];
    float *lut = reinterpret_cast<float *>(smem);
    uint32_t *img = smem + LUT_WORDS;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * TILE_X, y0 = blockIdx.y * TILE_Y;
    const uint8_t *frame = a.src + (size_t)blockIdx.z * (size_t)a.frame_pitch;

    for (int i = tid; i < LUT_WORDS; i += THREADS)
        lut[i] = a.lut[i];

    // the source rectangle of this tile (workgroup-uniform)
    int c0 = 0, ry0 = 0, row_words = 0;
    bool staged = false;
    if (x0 < a.tw && y0 < a.th) {
        const int xl = min(x0 + TILE_X, a.tw) - 1, yl = min(y0 + TILE_Y, a.th) - 1;
        c0 = a.s0x[x0];
        ry0 = a.s0y[y0];
        const int len = (a.s1x[xl] - c0 + 1) * 3;          // bytes of one row
        const int nrows = a.s1y[yl] - ry0 + 1;
        row_words = (len + 3) / 4 + 1;                      // the misalignment in front is at most 3 bytes
        staged = len > 0 && nrows > 0 && (long)nrows * row_words <= (long)a.img_words;
        if (staged) {
            const int total = nrows * row_words;
            for (int i = tid; i < total; i += THREADS) {
                const int r = i / row_words, d = i - r * row_words;
                const uint8_t *first = frame + (size_t)(ry0 + r) * (size_t)a.row_pitch + (size_t)c0 * 3;
                const int mis = (int)((uintptr_t)first & 3);
                if (d * 4 < mis + len)                      // a dword is loaded only if it holds a byte of the row
                    img[i] = reinterpret_cast<const uint32_t *>(first - mis)[d];
            }
        }
    }
    __syncthreads();

    const int y = y0 + wave, x = x0 + 4 * lane;
    if (y >= a.Hp || x >= a.Wp)
        return;
    f32x4_t o[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    if (y < a.th && x < a.tw) {
        const int r0 = a.s0y[y], r1 = a.s1y[y];
        const int b1 = a.b1y[y], b0 = 2048 - b1;
        const uint8_t *g0 = frame + (size_t)r0 * (size_t)a.row_pitch;
        const uint8_t *g1 = frame + (size_t)r1 * (size_t)a.row_pitch;
        if (staged) {
            const uint8_t *bytes = reinterpret_cast<const uint8_t *>(img);
            const int m0 = (int)((uintptr_t)(g0 + (size_t)c0 * 3) & 3), m1 = (int)((uintptr_t)(g1 + (size_t)c0 * 3) & 3);
            four_columns(a, bytes + ((r0 - ry0) * row_words * 4 + m0 - c0 * 3),
                         bytes + ((r1 - ry0) * row_words * 4 + m1 - c0 * 3), b0, b1, x, lut, o);
        } else {
            four_columns(a, g0, g1, b0, b1, x, lut, o);
        }
    }
    const size_t plane = (size_t)a.Hp * (size_t)a.Wp;
    float *dst = a.out + (size_t)blockIdx.z * 3 * plane + (size_t)y * (size_t)a.Wp + (size_t)x;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        *reinterpret_cast<f32x4_t *>(dst + c * plane) = o[c];
}

}  // namespace

extern "C" {

int frameops_abi_version(void) { return FRAMEOPS_ABI_VERSION; }
const char *frameops_last_error(void) { return g_err; }

int frameops_resize_normalize_u8(const uint8_t *src, long row_pitch, long frame_pitch, int B, int h, int w,
                                 const int32_t *s0x, const int32_t *s1x, const int16_t *a1x, const int32_t *s0y,
                                 const int32_t *s1y, const int16_t *b1y, int th, int tw, int Hp, int Wp,
                                 const float *lut, int swap_rb, float *out, void *stream) {
    if (B < 0) return fail(2, "frameops_resize_normalize_u8: negative batch size");
    if (B == 0) { g_err[0] = 0; return 0; }
    if (!src || !s0x || !s1x || !a1x || !s0y || !s1y || !b1y || !lut || !out)
        return fail(1, "frameops_resize_normalize_u8: null pointer");
    if (h <= 0 || w <= 0 || th <= 0 || tw <= 0 || Hp <= 0 || Wp <= 0)
        return fail(2, "frameops_resize_normalize_u8: non-positive size");
    if (Hp < th || Wp < tw) return fail(3, "frameops_resize_normalize_u8: padded size smaller than the target size");
    if (Wp % 4 != 0) return fail(4, "frameops_resize_normalize_u8: Wp is not a multiple of 4");
    if (((uintptr_t)out & 15) != 0) return fail(5, "frameops_resize_normalize_u8: out is not 16-byte aligned");
    if (row_pitch < 3L * w) return fail(6, "frameops_resize_normalize_u8: row pitch smaller than 3 * w");
    if (B > 1 && frame_pitch < 0) return fail(6, "frameops_resize_normalize_u8: negative frame pitch");
    if (swap_rb != 0 && swap_rb != 1) return fail(7, "frameops_resize_normalize_u8: swap_rb is not 0 or 1");
    const long gy = ((long)Hp + TILE_Y - 1) / TILE_Y;
    if (B > 65535 || gy > 65535) return fail(8, "frameops_resize_normalize_u8: more than 65535 frames or row tiles");

    // LDS for the largest source rectangle a tile of this geometry can need (an upper bound from the scale factors;
    // the kernel checks each tile's own rectangle against what it was given)
    const long cols = (long)((double)TILE_X * w / tw) + 4, rows = (long)((double)TILE_Y * h / th) + 4;
    const long row_words = ((cols < w ? cols : w) * 3 + 3) / 4 + 1;
    long img_words = (rows < h ? rows : h) * row_words;
    const long cap = MAX_LDS_BYTES / 4 - LUT_WORDS;
    if (img_words > cap) img_words = cap;

    Args a;
    a.src = src; a.row_pitch = row_pitch; a.frame_pitch = frame_pitch; a.h = h; a.w = w;
    a.s0x = s0x; a.s1x = s1x; a.a1x = a1x; a.s0y = s0y; a.s1y = s1y; a.b1y = b1y;
    a.th = th; a.tw = tw; a.Hp = Hp; a.Wp = Wp; a.lut = lut; a.swap_rb = swap_rb; a.out = out;
    a.img_words = (int)img_words;
    const dim3 grid((unsigned)((Wp + TILE_X - 1) / TILE_X), (unsigned)gy, (unsigned)B);
    hipLaunchKernelGGL(resize_normalize_u8_kernel, grid, dim3(THREADS), (size_t)(LUT_WORDS + img_words) * 4,
                       (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "frameops_resize_normalize_u8: %s", hipGetErrorString(e));
        return (int)e;
    }
    g_err[0] = 0;
    return 0;
}

}  // extern "C"
