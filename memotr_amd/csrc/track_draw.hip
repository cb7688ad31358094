// track_draw.hip -- libtrack_draw_hip.so: the track overlay as one gfx950 kernel (C ABI, the table layout and the
// drawing rules: include/track_draw_hip.h; the numpy statement that is the definition: memotr_amd/render.py).
//
// draw_kernel: a workgroup owns 64 x 16 pixels (the tile of the JPEG colour launches), a lane 4 pixels of one row.
// The table is taken in chunks of 64 rows: lane i of wave 0 tests row base + i (the clipped box united with the tab)
// against the tile, a ballot gives every hit its place in table order, and the hit rows are copied to LDS; after a
// barrier every lane walks only those rows over its 4 pixels in registers.  The pixels are loaded when the first
// row hits; a tile no row touches copies (out of place) or returns at once (in place).  12 bytes go in and out as
// three dwords where the quad is whole and the address allows it, as bytes otherwise.
//
// Integer arithmetic only; plain vector loads and stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/track_draw_hip.h"

namespace {

thread_local char g_err[TRACKDRAW_ERR_LEN] = {0};    // text of this thread's last error

int fail(int code, const char *msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

constexpr int TILE_X = TRACKDRAW_TILE_X, TILE_Y = TRACKDRAW_TILE_Y, CHUNK = TRACKDRAW_CHUNK;
constexpr int THREADS = (TILE_X / 4) * TILE_Y;
constexpr int ROW = TRACKDRAW_ROW_WORDS;
constexpr int COORD_MAX = 1 << 24;                   // coordinates are clamped to +-2^24: sums with the thickness fit
static_assert(CHUNK == 64, "one wavefront culls a chunk");

// 5 x 7 digits, 7 rows each, bit 4 the leftmost column
#define TRACKDRAW_FONT_ROWS                                                                                     \
    {0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E}, {0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E},                   \
    {0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F}, {0x1E, 0x01, 0x01, 0x0E, 0x01, 0x01, 0x1E},                   \
    {0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02}, {0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E},                   \
    {0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E}, {0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08},                   \
    {0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E}, {0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C}
const uint8_t FONT_HOST[10][7] = {TRACKDRAW_FONT_ROWS};
__constant__ uint8_t FONT[10][7] = {TRACKDRAW_FONT_ROWS};

struct DrawArgs {
    const uint8_t *in;
    uint8_t *out;
    long in_pitch, out_pitch;
    const int *table;
    int W, H, n, thickness, scale, alpha, inplace;
};

__device__ __forceinline__ int clampc(int v) { return min(max(v, -COORD_MAX), COORD_MAX); }

__global__ __launch_bounds__(THREADS) void draw_kernel(const DrawArgs a) {
    __shared__ int rows[CHUNK * ROW];
    __shared__ int count;
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * TILE_X, ty0 = blockIdx.y * TILE_Y;
    const int x0 = tx0 + (tid % (TILE_X / 4)) * 4, y = ty0 + tid / (TILE_X / 4);
    const bool inside = y < a.H && x0 < a.W;
    const int npx = inside ? min(4, a.W - x0) : 0;
    const int tile_x1 = min(tx0 + TILE_X, a.W) - 1, tile_y1 = min(ty0 + TILE_Y, a.H) - 1;
    const uint8_t *src = a.in + (size_t)(inside ? y : 0) * a.in_pitch + (size_t)(inside ? x0 : 0) * 3;
    uint8_t px[12];
    bool loaded = false;

    auto load = [&]() {
        if (npx == 4 && ((uintptr_t)src & 3) == 0) {
            const unsigned *s = reinterpret_cast<const unsigned *>(src);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const unsigned w = s[k];
                px[4 * k] = w & 255; px[4 * k + 1] = (w >> 8) & 255; px[4 * k + 2] = (w >> 16) & 255; px[4 * k + 3] = w >> 24;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) px[k] = k < 3 * npx ? src[k] : 0;
        }
    };

    for (int base = 0; base < a.n; base += CHUNK) {
        __syncthreads();                             // the previous chunk's rows have been read by every lane
        if (tid < CHUNK) {                           // wave 0: one table row per lane
            const int i = base + tid;
            int r[ROW];
            bool hit = false;
            if (i < a.n) {
                const int *t = a.table + (size_t)i * ROW;
#pragma unroll
                for (int k = 0; k < ROW; ++k) r[k] = t[k];
#pragma unroll
                for (int k = 0; k < 4; ++k) { r[k] = clampc(r[k]); r[5 + k] = clampc(r[5 + k]); }
                // an inverted box and a box wholly off the frame draw nothing, their tabs included
                if (r[2] >= r[0] && r[3] >= r[1] && r[2] >= 0 && r[3] >= 0 && r[0] < a.W && r[1] < a.H) {
                    const bool box = r[0] <= tile_x1 && r[2] >= tx0 && r[1] <= tile_y1 && r[3] >= ty0;
                    const bool tab = r[5] <= tile_x1 && r[7] >= tx0 && r[6] <= tile_y1 && r[8] >= ty0;
                    hit = box || tab;
                }
            }
            const unsigned long long mask = __ballot(hit);
            if (hit) {
                const int pos = __popcll(mask & ((1ull << tid) - 1));
#pragma unroll
                for (int k = 0; k < ROW; ++k) rows[pos * ROW + k] = r[k];
            }
            if (tid == 0) count = __popcll(mask);
        }
        __syncthreads();
        const int m = count;                         // the same in every lane of the workgroup
        if (m == 0 || !inside) continue;
        if (!loaded) { load(); loaded = true; }
        for (int j = 0; j < m; ++j) {
            const int *r = rows + j * ROW;
            const int x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
            const int bx1 = r[5], by1 = r[6], bx2 = r[7], by2 = r[8];
            const bool in_box_y = y >= y1 && y <= y2, in_tab_y = y >= by1 && y <= by2;
            if (!in_box_y && !in_tab_y) continue;
            const unsigned colour = (unsigned)r[4], text = (unsigned)r[9];
            const int t = a.thickness, s = a.scale;
            const bool inner_y = y >= y1 + t && y <= y2 - t;
            const int grow = in_tab_y && y - by1 - 1 >= 0 ? (y - by1 - 1) / s : 7;      // glyph row, 7: none
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int x = x0 + p;
                if (in_box_y && x >= x1 && x <= x2) {
                    if (!(inner_y && x >= x1 + t && x <= x2 - t)) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) px[3 * p + c] = (colour >> (8 * c)) & 255;
                    } else if (a.alpha > 0) {
#pragma unroll
                        for (int c = 0; c < 3; ++c)
                            px[3 * p + c] = (uint8_t)((((colour >> (8 * c)) & 255) * a.alpha +
                                                       px[3 * p + c] * (255 - a.alpha) + 127) / 255);
                    }
                }
                if (in_tab_y && x >= bx1 && x <= bx2) {
                    unsigned v = colour;
                    const int dx = x - bx1 - 1;
                    if (grow < 7 && dx >= 0) {
                        const int k = dx / (6 * s), col = (dx - k * 6 * s) / s;
                        if (k < r[10] && col < 5) {
                            const int g = k < 8 ? (r[11] >> (4 * k)) & 15 : (r[12] >> (4 * (k - 8))) & 15;
                            if (g < 10 && ((FONT[g][grow] >> (4 - col)) & 1)) v = text;
                        }
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c) px[3 * p + c] = (v >> (8 * c)) & 255;
                }
            }
        }
    }
    if (!inside) return;
    if (!loaded) {
        if (a.inplace) return;
        load();
    }
    uint8_t *dst = a.out + (size_t)y * a.out_pitch + (size_t)x0 * 3;
    if (npx == 4 && ((uintptr_t)dst & 3) == 0) {
        unsigned *d = reinterpret_cast<unsigned *>(dst);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            d[k] = (unsigned)px[4 * k] | (unsigned)px[4 * k + 1] << 8 | (unsigned)px[4 * k + 2] << 16 |
                   (unsigned)px[4 * k + 3] << 24;
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (k < 3 * npx) dst[k] = px[k];
    }
}

}  // namespace

extern "C" {

int trackdraw_abi_version(void) { return TRACKDRAW_ABI_VERSION; }
const char *trackdraw_last_error(void) { return g_err; }
void trackdraw_font(uint8_t *out) { if (out) memcpy(out, FONT_HOST, sizeof(FONT_HOST)); }

int trackdraw_draw_u8(const uint8_t *in, int64_t in_pitch, uint8_t *out, int64_t out_pitch, int width, int height,
                      const int32_t *table, int n, int thickness, int font_scale, int fill_alpha, void *stream) {
    char msg[TRACKDRAW_ERR_LEN];
    auto bad = [&](int code, const char *what) {
        snprintf(msg, sizeof(msg), "trackdraw_draw_u8: %s", what);
        return fail(code, msg);
    };
    if (n < 0) return bad(2, "negative row count");
    if (!in || !out || (n > 0 && !table)) return bad(1, "null pointer");
    if (width < 1 || height < 1 || width > 65535 || height > 65535) return bad(2, "width or height outside 1 .. 65535");
    if (in_pitch < 3L * width || out_pitch < 3L * width) return bad(3, "a row pitch smaller than 3 * width");
    const bool inplace = in == out;
    if (inplace && in_pitch != out_pitch) return bad(3, "in place with two different pitches");
    if (!inplace) {
        const uintptr_t a0 = (uintptr_t)in, a1 = a0 + (uintptr_t)in_pitch * (height - 1) + 3u * width;
        const uintptr_t b0 = (uintptr_t)out, b1 = b0 + (uintptr_t)out_pitch * (height - 1) + 3u * width;
        if (a0 < b1 && b0 < a1) return bad(4, "in and out overlap without being equal");
    }
    if ((uintptr_t)table & 3) return bad(5, "the table is not 4-byte aligned");
    if (thickness < 1 || thickness > 65535) return bad(6, "thickness outside 1 .. 65535");
    if (font_scale < 1 || font_scale > 64) return bad(6, "font_scale outside 1 .. 64");
    if (fill_alpha < 0 || fill_alpha > 255) return bad(6, "fill_alpha outside 0 .. 255");
    g_err[0] = 0;
    if (n == 0 && inplace) return 0;

    DrawArgs a;
    a.in = in; a.out = out; a.in_pitch = in_pitch; a.out_pitch = out_pitch; a.table = table;
    a.W = width; a.H = height; a.n = n; a.thickness = thickness; a.scale = font_scale; a.alpha = fill_alpha;
    a.inplace = inplace;
    const dim3 grid((unsigned)((width + TILE_X - 1) / TILE_X), (unsigned)((height + TILE_Y - 1) / TILE_Y));
    hipLaunchKernelGGL(draw_kernel, grid, dim3(THREADS), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return bad((int)e, hipGetErrorString(e));
    return 0;
}

}  // extern "C"
