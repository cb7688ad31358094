// msda_attn_map.h -- attention maps: where the decoder queries of a track sample, as a picture.
//
// Two kernels, both all-integer past the first float multiply, both defined by the numpy statements of
// memotr_amd/attention_maps.py (attention_heat_host, blend_heat_host) and equal to them bit for bit:
//   * msda_attn_heat_kernel<FUSED>: every weighted sampling point of the chosen query rows is stamped into a uint64
//     plane of heat cells.  ONE body, two point sources: materialised (loc, attn), or the raw query projection and the
//     reference points, from which the points are formed with msda_common.h's arithmetic (the bits
//     msda_fused_points_f32 writes) and never reach memory.
//     One workgroup owns one tile of kHeatTile x kHeatTile cells of one plane: it walks the plane's (entry, layer,
//     head) rows eight lanes to a row, culls every point against the tile, sums in LDS (64-bit LDS atomics: integer
//     sums are order-free) and writes each cell once with a plain store -- no zero-fill launch, no global atomics but
//     one atomicMax per workgroup for the plane's peak.
//   * msda_attn_blend_kernel: the heat planes blended into a uint8 frame.  The level of a cell (one 64-bit division) is
//     computed once per (plane, cell) of the workgroup's pixel tile into LDS, the pixels then only look it up.
// Included by msda_hip.hip inside its anonymous namespace.
#pragma once

constexpr int kHeatTile = 32;             // cells per tile side: 8 KiB of uint64 sums in LDS
constexpr int kHeatThreads = 1024;        // at most: the launch picks 256 .. 1024 by the rows a plane has (heat_threads)
constexpr int kHeatMaxLayers = 8;
constexpr int kHeatMaxRadius = 8;
constexpr int kBlendMaxPlanes = 16;
constexpr int kBlendTileW = 64, kBlendTileH = 16;      // pixels per workgroup: 4 consecutive pixels per thread

// The layers of one launch, by value.  `a` / `b`: (loc, attn) of batch item 0 for the plain source, (proj, ref) for the
// fused one.
struct HeatLayers {
    const float *a[kHeatMaxLayers];
    const float *b[kHeatMaxLayers];
    int Lq[kHeatMaxLayers];
    int proj_stride[kHeatMaxLayers];
    int ref_dim[kHeatMaxLayers];
    int n;
};

// weight of a point in 1/4096: 0 unless attn > 0 (NaN and negatives included), else rint(min(attn, 1) * 4096), ties to
// even
__device__ __forceinline__ unsigned heat_weight(float attn) {
    if (!(attn > 0.f)) return 0u;
    return (unsigned)(int)rintf(fminf(attn, 1.0f) * 4096.0f);
}

// Threads per workgroup.  A workgroup walks the (entry, layer, head) rows of its plane eight lanes to a row, each step a
// chain of dependent loads: its time goes with rows / (threads / 8), so many rows per plane want many threads; with few
// rows per plane most of a large workgroup would idle while fewer workgroups fit a CU.  Measured at 270 x 480 cells, six
// layers (profiles/attention_maps.md): one plane of 40 rows 101 us at 256 threads, 44 us at 1024; sixteen planes of one
// row 26 us at 256, 34 us at 1024.  The result does not depend on it.
inline int heat_threads(long rows_per_plane_items) {
    int threads = 256;
    while (threads < kHeatThreads && (long)(threads / 8) * 4 <= rows_per_plane_items) threads *= 2;
    return threads;
}

template <bool FUSED>
__global__ __launch_bounds__(kHeatThreads) void msda_attn_heat_kernel(
    const HeatLayers ly, const int64_t *__restrict__ shapes, int M, int L, int P, const int32_t *__restrict__ rows,
    const int32_t *__restrict__ planes, int K, const uint16_t *__restrict__ stamp, int r, float sx, float sy,
    unsigned long long *__restrict__ heat, unsigned long long *__restrict__ peak, int n_planes, int hc, int wc,
    int accumulate) {
#pragma clang fp contract(off)
    __shared__ unsigned long long s_heat[kHeatTile * kHeatTile];
    __shared__ unsigned short s_stamp[(2 * kHeatMaxRadius + 1) * (2 * kHeatMaxRadius + 1)];
    __shared__ unsigned long long s_max;

    const int tid = threadIdx.x, nt = blockDim.x;
    const int tiles_x = (wc + kHeatTile - 1) / kHeatTile;
    const int x0 = ((int)blockIdx.x % tiles_x) * kHeatTile, y0 = ((int)blockIdx.x / tiles_x) * kHeatTile;
    const int x1 = min(x0 + kHeatTile, wc), y1 = min(y0 + kHeatTile, hc);       // the tile's cells inside the plane
    const int p = blockIdx.y;
    const int side = 2 * r + 1;

    for (int i = tid; i < kHeatTile * kHeatTile; i += nt) s_heat[i] = 0ull;
    for (int i = tid; i < side * side; i += nt) s_stamp[i] = stamp[i];
    if (tid == 0) s_max = 0ull;
    __syncthreads();

    const int LP = L * P;
    const int group = tid >> 3, sub = tid & 7;          // eight lanes to a (entry, layer, head) row
    const long n_items = (long)K * ly.n * M;
    const float lo = -(float)(r + 1), hi_x = (float)(wc + r + 1), hi_y = (float)(hc + r + 1);

    for (long item = group; item < n_items; item += nt / 8) {
        const int k = (int)(item / (ly.n * M));
        const int rem = (int)(item - (long)k * (ly.n * M));
        const int li = rem / M, m = rem - li * M;
        if (planes[k] != p) continue;       // (p is in range: entries of planes outside 0 .. n_planes - 1 match no tile)
        const int q = rows[k];
        if (q < 0 || q >= ly.Lq[li]) continue;
        // all eight lanes of the row are here or none is: the DPP reductions of the softmax see whole rows
        PointSrc src;
        src.loc = src.attn = src.proj = src.ref = nullptr;
        src.mask = nullptr;
        src.proj_stride = ly.proj_stride[li];
        src.n_off = 2 * M * LP;
        src.ref_dim = ly.ref_dim[li];
        const float *lg = nullptr;
        float mx = 0.f, rsum = 0.f;
        if (FUSED) {
            src.proj = ly.a[li];
            src.ref = ly.b[li];
            lg = fused_logits<long>(src, (long)q, m, LP);
            row_softmax_stats<8>(lg, LP, sub, mx, rsum);
        } else {
            src.loc = ly.a[li];
            src.attn = ly.b[li];
        }
        const long pm = (long)q * M + m;
        for (int t = sub; t < LP; t += 8) {
            f32x2 xy;
            float a;
            if (FUSED) {
                const int l = t / P;
                xy = fused_location<long>(src, (long)q, m, L, P, t, l, (int)shapes[2 * l], (int)shapes[2 * l + 1]);
                a = sm_exp(lg[t], mx) * rsum;
            } else {
                xy = *reinterpret_cast<const f32x2 *>(src.loc + (pm * LP + t) * 2);
                a = src.attn[pm * LP + t];
            }
            const float x = xy.x * sx, y = xy.y * sy;
            if (!(x >= lo && x < hi_x && y >= lo && y < hi_y)) continue;           // NaN and +-inf leave here
            const int ix = (int)floorf(x), iy = (int)floorf(y);
            if (ix + r < x0 || ix - r >= x1 || iy + r < y0 || iy - r >= y1) continue;   // the stamp misses the tile
            const unsigned wq = heat_weight(a);
            if (wq == 0u) continue;
            const int cy_lo = max(iy - r, y0), cy_hi = min(iy + r, y1 - 1);
            const int cx_lo = max(ix - r, x0), cx_hi = min(ix + r, x1 - 1);
            for (int cy = cy_lo; cy <= cy_hi; ++cy) {
                for (int cx = cx_lo; cx <= cx_hi; ++cx) {
                    const unsigned long long v =
                        (unsigned long long)wq * (unsigned long long)s_stamp[(cy - iy + r) * side + (cx - ix + r)];
                    if (v) atomicAdd(&s_heat[(cy - y0) * kHeatTile + (cx - x0)], v);
                }
            }
        }
    }
    __syncthreads();

    unsigned long long best = 0ull;
    for (int i = tid; i < kHeatTile * kHeatTile; i += nt) {
        const int cy = y0 + i / kHeatTile, cx = x0 + i % kHeatTile;
        if (cy < y1 && cx < x1) {
            unsigned long long *dst = heat + ((long)p * hc + cy) * wc + cx;
            unsigned long long v = s_heat[i];
            if (accumulate) v += *dst;
            *dst = v;
            best = v > best ? v : best;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, kWave);
        best = other > best ? other : best;
    }
    if ((tid & (kWave - 1)) == 0 && best) atomicMax(&s_max, best);
    __syncthreads();
    if (tid == 0 && s_max) atomicMax(peak + p, s_max);
}

// level of a cell: 0 when the scale is 0, else min(255, (heat * 255 + s / 2) / s) in wrapping uint64 arithmetic
__device__ __forceinline__ unsigned heat_level(unsigned long long h, unsigned long long s) {
    if (s == 0ull) return 0u;
    const unsigned long long v = (h * 255ull + s / 2ull) / s;
    return v > 255ull ? 255u : (unsigned)v;
}

__device__ __forceinline__ unsigned blend_channel(unsigned px, unsigned colour, unsigned a) {
    return (colour * a + px * (255u - a) + 127u) / 255u;
}

__global__ __launch_bounds__(256) void msda_attn_blend_kernel(
    const uint8_t *src, long src_pitch, uint8_t *dst, long dst_pitch, int W, int H,     // (src may be dst: in place)
    const unsigned long long *__restrict__ heat, const unsigned long long *__restrict__ peak,
    const uint8_t *__restrict__ lut, int n_planes, int hc, int wc, int cell, int max_alpha,
    unsigned long long full_scale) {
    __shared__ uint8_t s_level[kBlendMaxPlanes * kBlendTileW * kBlendTileH];

    const int tid = threadIdx.x;
    const int x0 = (int)blockIdx.x * kBlendTileW, y0 = (int)blockIdx.y * kBlendTileH;
    const int xe = min(x0 + kBlendTileW, W) - 1, ye = min(y0 + kBlendTileH, H) - 1;     // last pixel of the tile
    const int cx0 = x0 / cell, cy0 = y0 / cell;
    const int ncx = xe / cell - cx0 + 1, ncy = ye / cell - cy0 + 1;
    const int n_cells = ncx * ncy;

    for (int i = tid; i < n_planes * n_cells; i += 256) {
        const int p = i / n_cells, c = i - p * n_cells;
        const int cy = cy0 + c / ncx, cx = cx0 + c % ncx;
        const unsigned long long s = full_scale ? full_scale : peak[p];
        s_level[i] = (uint8_t)heat_level(heat[((long)p * hc + cy) * wc + cx], s);
    }
    __syncthreads();

    const int y = y0 + tid / (kBlendTileW / 4);
    const int xa = x0 + (tid % (kBlendTileW / 4)) * 4;
    if (y > ye || xa > xe) return;
    const int n_px = min(4, xe - xa + 1);
    const uint8_t *sp = src + (long)y * src_pitch + (long)xa * 3;
    uint8_t *dp = dst + (long)y * dst_pitch + (long)xa * 3;
    const bool wide = n_px == 4 && (((uintptr_t)sp | (uintptr_t)dp) & 3u) == 0u;

    unsigned px[12];
    if (wide) {
        const unsigned *s4 = reinterpret_cast<const unsigned *>(sp);
#pragma unroll
        for (int w = 0; w < 3; ++w) {
            const unsigned v = s4[w];
#pragma unroll
            for (int b = 0; b < 4; ++b) px[4 * w + b] = (v >> (8 * b)) & 255u;
        }
    } else {
#pragma unroll
        for (int b = 0; b < 12; ++b) px[b] = b < 3 * n_px ? sp[b] : 0u;
    }
    const int crow = (y / cell - cy0) * ncx - cx0;
    for (int p = 0; p < n_planes; ++p) {
        const uint8_t *lv = s_level + p * n_cells + crow;
        const uint8_t *colours = lut + (long)p * 768;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < n_px) {
                const unsigned level = lv[(xa + j) / cell];
                const unsigned a = (level * (unsigned)max_alpha + 127u) / 255u;
                if (a > 0u) {
                    const uint8_t *c3 = colours + level * 3u;
#pragma unroll
                    for (int c = 0; c < 3; ++c) px[3 * j + c] = blend_channel(px[3 * j + c], c3[c], a);
                }
            }
        }
    }
    if (wide) {
        unsigned *d4 = reinterpret_cast<unsigned *>(dp);
#pragma unroll
        for (int w = 0; w < 3; ++w)
            d4[w] = px[4 * w] | (px[4 * w + 1] << 8) | (px[4 * w + 2] << 16) | (px[4 * w + 3] << 24);
    } else {
#pragma unroll
        for (int b = 0; b < 12; ++b)
            if (b < 3 * n_px) dp[b] = (uint8_t)px[b];
    }
}

