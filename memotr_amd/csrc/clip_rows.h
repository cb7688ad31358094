// clip_rows.h -- passes over the rows of an activation matrix: column sums (plain, per chunk, with the ReLU mask of a
// backward), residual add + LayerNorm with its backward, and the backbone's shift + ReLU.
// Included by clip_ops.hip after clip_common.h.
#pragma once

namespace {
// 32 columns x 8 row lanes per workgroup; lane (ty, tx) sums rows ty, ty + 8, ... of column tile tx.
// The sums of all column-sum kernels are kept in fp64 and rounded once: a lane's rows are a strided subset, so an fp32
// partial sum grows to (rows / lanes) * max|x| even where neighbouring rows cancel, and its rounding error with it
// (alternating +-1e4 over 2048 rows: 0.3 absolute against a true sum of ~50).  The kernels are bound by their loads.
__global__ __launch_bounds__(256) void colsum_kernel(const float *__restrict__ x, long rows, int cols,
                                                    float *__restrict__ out) {
    __shared__ double s_part[8][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + tx;
    double a0 = 0., a1 = 0., a2 = 0., a3 = 0.;
    if (c < cols) {
        long r = ty;
        for (; r + 24 < rows; r += 32) {          // four independent loads in flight
            a0 += x[r * cols + c];
            a1 += x[(r + 8) * cols + c];
            a2 += x[(r + 16) * cols + c];
            a3 += x[(r + 24) * cols + c];
        }
        for (; r < rows; r += 8) a0 += x[r * cols + c];
    }
    s_part[ty][tx] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (ty == 0 && c < cols) {
        double t = s_part[0][tx];
#pragma unroll
        for (int i = 1; i < 8; ++i) t += s_part[i][tx];
        out[c] = (float)t;
    }
}

// Short matrices (a few hundred rows) are latency-bound, not bandwidth-bound: one workgroup per FOUR columns, thread t
// takes rows t, t + 256, ... as 16-byte loads (one or two per thread at 310 rows), then a wavefront shuffle reduction
// and one LDS step over the four wavefronts.  6.0 -> ~3 us at 310 x 256 against the 32 x 8 tile above.
__global__ __launch_bounds__(256) void colsum_quad_kernel(const float *__restrict__ x, long rows, int cols,
                                                         float *__restrict__ out) {
    __shared__ f64x4_t s_w[4];
    const int c = blockIdx.x * 4;
    f64x4_t a = {0., 0., 0., 0.};
    for (long r = threadIdx.x; r < rows; r += 256) {
        const f32x4_t v = *reinterpret_cast<const f32x4_t *>(x + r * cols + c);
        a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a.x += __shfl_xor(a.x, o, 64);
        a.y += __shfl_xor(a.y, o, 64);
        a.z += __shfl_xor(a.z, o, 64);
        a.w += __shfl_xor(a.w, o, 64);
    }
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        const f64x4_t t = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
        const f32x4_t r = {(float)t.x, (float)t.y, (float)t.z, (float)t.w};
        *reinterpret_cast<f32x4_t *>(out + c) = r;
    }
}

// the same tile over one chunk of rows per workgroup row (blockIdx.y): partial sums for tall matrices
__device__ __forceinline__ float colsum_ld(const float *x, long i) { return x[i]; }
__device__ __forceinline__ float colsum_ld(const uint16_t *x, long i) {      // bf16 storage, fp32 sums
    return __uint_as_float(((unsigned)x[i]) << 16);
}

template <typename TX>
__global__ __launch_bounds__(256) void colsum_partial_kernel(const TX *__restrict__ x, long rows, int cols,
                                                            int chunk_rows, float *__restrict__ partial) {
    __shared__ double s_part[8][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + tx;
    const long r0 = (long)blockIdx.y * chunk_rows;
    const long r1 = r0 + chunk_rows < rows ? r0 + chunk_rows : rows;
    double a0 = 0., a1 = 0., a2 = 0., a3 = 0.;
    if (c < cols) {
        long r = r0 + ty;
        for (; r + 24 < r1; r += 32) {
            a0 += colsum_ld(x, r * cols + c);
            a1 += colsum_ld(x, (r + 8) * cols + c);
            a2 += colsum_ld(x, (r + 16) * cols + c);
            a3 += colsum_ld(x, (r + 24) * cols + c);
        }
        for (; r < r1; r += 8) a0 += colsum_ld(x, r * cols + c);
    }
    s_part[ty][tx] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (ty == 0 && c < cols) {
        double t = s_part[0][tx];
#pragma unroll
        for (int i = 1; i < 8; ++i) t += s_part[i][tx];
        partial[(long)blockIdx.y * cols + c] = (float)t;
    }
}

// The ReLU mask of a fused-ReLU Linear's backward and the first pass of its bias gradient in ONE pass over the
// gradient: g2 = y > 0 ? g : 0 is written and summed per (32-column tile, row chunk) on the way.  For the encoder
// FFN's first linear (111,615 x 2048 floats per layer of a 5-frame clip) the separate column sum re-read 914 MB.
__device__ __forceinline__ void colsum_st(float *x, long i, float v) { x[i] = v; }

template <typename TX>
__global__ __launch_bounds__(256) void relu_bwd_colsum_partial_kernel(const TX *__restrict__ g, const TX *__restrict__ y,
                                                                     long rows, int cols, int chunk_rows,
                                                                     TX *__restrict__ g2, float *__restrict__ partial) {
    __shared__ double s_part[8][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + tx;
    const long r0 = (long)blockIdx.y * chunk_rows;
    const long r1 = r0 + chunk_rows < rows ? r0 + chunk_rows : rows;
    double a0 = 0., a1 = 0., a2 = 0., a3 = 0.;
    if (c < cols) {
        long r = r0 + ty;
        for (; r + 24 < r1; r += 32) {
            const long i0 = r * cols + c, i1 = (r + 8) * cols + c, i2 = (r + 16) * cols + c, i3 = (r + 24) * cols + c;
            const float v0 = colsum_ld(y, i0) <= 0.f ? 0.f : colsum_ld(g, i0);
            const float v1 = colsum_ld(y, i1) <= 0.f ? 0.f : colsum_ld(g, i1);
            const float v2 = colsum_ld(y, i2) <= 0.f ? 0.f : colsum_ld(g, i2);
            const float v3 = colsum_ld(y, i3) <= 0.f ? 0.f : colsum_ld(g, i3);
            colsum_st(g2, i0, v0); colsum_st(g2, i1, v1); colsum_st(g2, i2, v2); colsum_st(g2, i3, v3);
            a0 += v0; a1 += v1; a2 += v2; a3 += v3;
        }
        for (; r < r1; r += 8) {
            const long i0 = r * cols + c;
            const float v0 = colsum_ld(y, i0) <= 0.f ? 0.f : colsum_ld(g, i0);
            colsum_st(g2, i0, v0);
            a0 += v0;
        }
    }
    s_part[ty][tx] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (ty == 0 && c < cols) {
        double t = s_part[0][tx];
#pragma unroll
        for (int i = 1; i < 8; ++i) t += s_part[i][tx];
        partial[(long)blockIdx.y * cols + c] = (float)t;
    }
}

// ----------------------------------------------------------------------------------------
// residual add + LayerNorm over rows of 256 floats: one wavefront per row, 4 floats per lane
// ----------------------------------------------------------------------------------------
// WITH_Q (ABI 11): q = y + pos is written in the same pass from the y still in registers -- the next encoder layer's
// query, which was a torch add (read 2, write 1 tensor) right after this kernel.  y is the same expression either way.
template <bool WITH_Q>
__global__ __launch_bounds__(256) void add_layer_norm_fwd_kernel(const float *__restrict__ x,
                                                                const float *__restrict__ res,
                                                                const float *__restrict__ gamma,
                                                                const float *__restrict__ beta,
                                                                const float *__restrict__ pos, long rows, float eps,
                                                                float *__restrict__ sum, float *__restrict__ y,
                                                                float *__restrict__ q, float *__restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const long off = row * CLIPOPS_LN_COLS + lane * 4;
    const f32x4_t a = *reinterpret_cast<const f32x4_t *>(x + off);
    const f32x4_t b = *reinterpret_cast<const f32x4_t *>(res + off);
    const f32x4_t s = a + b;
    *reinterpret_cast<f32x4_t *>(sum + off) = s;
    const float mean = wave_sum64((s.x + s.y) + (s.z + s.w)) * (1.f / CLIPOPS_LN_COLS);
    const f32x4_t d = s - mean;
    const float var = wave_sum64((d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w)) * (1.f / CLIPOPS_LN_COLS);
    const float rstd = rsqrtf(var + eps);
    const f32x4_t g = *reinterpret_cast<const f32x4_t *>(gamma + lane * 4);
    const f32x4_t be = *reinterpret_cast<const f32x4_t *>(beta + lane * 4);
    const f32x4_t yv = (d * rstd) * g + be;
    *reinterpret_cast<f32x4_t *>(y + off) = yv;
    if (WITH_Q) *reinterpret_cast<f32x4_t *>(q + off) = yv + *reinterpret_cast<const f32x4_t *>(pos + off);
    if (lane == 0) {
        stats[2 * row] = mean;
        stats[2 * row + 1] = rstd;
    }
}

// a workgroup walks chunk_rows rows (4 at a time, one per wavefront) and keeps the column sums of its rows
__global__ __launch_bounds__(256) void add_layer_norm_bwd_kernel(const float *__restrict__ gy,
                                                                const float *__restrict__ sum,
                                                                const float *__restrict__ stats,
                                                                const float *__restrict__ gamma, long rows,
                                                                int chunk_rows, float *__restrict__ gsum,
                                                                float *__restrict__ partial) {
    __shared__ f32x4_t s_acc[4][2][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const f32x4_t gm = *reinterpret_cast<const f32x4_t *>(gamma + lane * 4);
    f32x4_t acc_g = {0.f, 0.f, 0.f, 0.f}, acc_b = {0.f, 0.f, 0.f, 0.f};
    const long r0 = (long)blockIdx.x * chunk_rows;
    const long r1 = r0 + chunk_rows < rows ? r0 + chunk_rows : rows;
    for (long row = r0 + wave; row < r1; row += 4) {
        const long off = row * CLIPOPS_LN_COLS + lane * 4;
        const f32x4_t g = *reinterpret_cast<const f32x4_t *>(gy + off);
        const f32x4_t s = *reinterpret_cast<const f32x4_t *>(sum + off);
        const float mean = stats[2 * row], rstd = stats[2 * row + 1];
        const f32x4_t xh = (s - mean) * rstd;
        const f32x4_t gh = g * gm;
        const float c1 = wave_sum64((gh.x + gh.y) + (gh.z + gh.w)) * (1.f / CLIPOPS_LN_COLS);
        const float c2 = wave_sum64((gh.x * xh.x + gh.y * xh.y) + (gh.z * xh.z + gh.w * xh.w)) * (1.f / CLIPOPS_LN_COLS);
        *reinterpret_cast<f32x4_t *>(gsum + off) = (gh - c1 - xh * c2) * rstd;
        acc_g += g * xh;
        acc_b += g;
    }
    s_acc[wave][0][lane] = acc_g;
    s_acc[wave][1][lane] = acc_b;
    __syncthreads();
    if (wave < 2) {                       // wave 0: gamma part, wave 1: beta part
        const f32x4_t t = (s_acc[0][wave][lane] + s_acc[1][wave][lane]) + (s_acc[2][wave][lane] + s_acc[3][wave][lane]);
        *reinterpret_cast<f32x4_t *>(partial + (long)blockIdx.x * 2 * CLIPOPS_LN_COLS + wave * CLIPOPS_LN_COLS + lane * 4) = t;
    }
}

// The same backward for a LayerNorm whose output has up to three consumers (ABI 11): the incoming gradient is
// (ga + gb) + gc, summed in registers (gb / gc may be null: skipped) and never written out, and the column sums of
// grad_sum -- the bias gradient of the Linear that produced `res` -- ride along.  Those are kept in fp64 like every
// column sum here and leave the workgroup as a float pair (hi, lo = the rounding remainder) in rows 2 * chunk and
// 2 * chunk + 1 of `zpartial`: the finishing colsum adds both in fp64, so a chunk's sum is not rounded to fp32 on the way.
__global__ __launch_bounds__(256) void add_layer_norm_bwd_fanin_kernel(const float *__restrict__ ga,
                                                                      const float *__restrict__ gb,
                                                                      const float *__restrict__ gc,
                                                                      const float *__restrict__ sum,
                                                                      const float *__restrict__ stats,
                                                                      const float *__restrict__ gamma, long rows,
                                                                      int chunk_rows, float *__restrict__ gsum,
                                                                      float *__restrict__ partial,
                                                                      float *__restrict__ zpartial) {
    __shared__ f32x4_t s_acc[4][2][64];
    __shared__ f64x4_t s_z[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const f32x4_t gm = *reinterpret_cast<const f32x4_t *>(gamma + lane * 4);
    f32x4_t acc_g = {0.f, 0.f, 0.f, 0.f}, acc_b = {0.f, 0.f, 0.f, 0.f};
    f64x4_t acc_z = {0., 0., 0., 0.};
    const long r0 = (long)blockIdx.x * chunk_rows;
    const long r1 = r0 + chunk_rows < rows ? r0 + chunk_rows : rows;
    for (long row = r0 + wave; row < r1; row += 4) {
        const long off = row * CLIPOPS_LN_COLS + lane * 4;
        f32x4_t g = *reinterpret_cast<const f32x4_t *>(ga + off);
        if (gb) g += *reinterpret_cast<const f32x4_t *>(gb + off);
        if (gc) g += *reinterpret_cast<const f32x4_t *>(gc + off);
        const f32x4_t s = *reinterpret_cast<const f32x4_t *>(sum + off);
        const float mean = stats[2 * row], rstd = stats[2 * row + 1];
        const f32x4_t xh = (s - mean) * rstd;
        const f32x4_t gh = g * gm;
        const float c1 = wave_sum64((gh.x + gh.y) + (gh.z + gh.w)) * (1.f / CLIPOPS_LN_COLS);
        const float c2 = wave_sum64((gh.x * xh.x + gh.y * xh.y) + (gh.z * xh.z + gh.w * xh.w)) * (1.f / CLIPOPS_LN_COLS);
        const f32x4_t dz = (gh - c1 - xh * c2) * rstd;
        *reinterpret_cast<f32x4_t *>(gsum + off) = dz;
        acc_g += g * xh;
        acc_b += g;
        acc_z.x += dz.x; acc_z.y += dz.y; acc_z.z += dz.z; acc_z.w += dz.w;
    }
    s_acc[wave][0][lane] = acc_g;
    s_acc[wave][1][lane] = acc_b;
    s_z[wave][lane] = acc_z;
    __syncthreads();
    if (wave < 2) {                       // wave 0: gamma part, wave 1: beta part
        const f32x4_t t = (s_acc[0][wave][lane] + s_acc[1][wave][lane]) + (s_acc[2][wave][lane] + s_acc[3][wave][lane]);
        *reinterpret_cast<f32x4_t *>(partial + (long)blockIdx.x * 2 * CLIPOPS_LN_COLS + wave * CLIPOPS_LN_COLS + lane * 4) = t;
    } else if (wave == 2) {               // wave 2: the column sums of grad_sum
        const f64x4_t t = (s_z[0][lane] + s_z[1][lane]) + (s_z[2][lane] + s_z[3][lane]);
        const f32x4_t hi = {(float)t.x, (float)t.y, (float)t.z, (float)t.w};
        const f32x4_t lo = {(float)(t.x - (double)hi.x), (float)(t.y - (double)hi.y), (float)(t.z - (double)hi.z),
                            (float)(t.w - (double)hi.w)};
        float *zp = zpartial + (long)blockIdx.x * 2 * CLIPOPS_LN_COLS + lane * 4;
        *reinterpret_cast<f32x4_t *>(zp) = hi;
        *reinterpret_cast<f32x4_t *>(zp + CLIPOPS_LN_COLS) = lo;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Frozen-BN shift + (residual) + ReLU of a ResNet bottleneck in ONE pass over the convolution's output, in place.
// The backbone (reference models/backbone.py:70-76: torchvision's resnet50 with FrozenBatchNorm2d) does this as three
// element-wise passes over activations of up to 344 MB each (5 frames x 256 x 200 x 336): conv bias, `out += identity`,
// ReLU.  NCHW: one (image, channel) plane per blockIdx.y, so the shift is a scalar of the block.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sr_bf16(uint16_t h) { return __uint_as_float((unsigned)h << 16); }
__device__ __forceinline__ uint16_t sr_to_bf16(float f) {          // round to nearest even (NaN stays NaN)
    unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

template <bool RES>
__global__ __launch_bounds__(256) void shift_relu_f32_kernel(float *__restrict__ x, const float *__restrict__ shift,
                                                             const float *__restrict__ res, long planes, int C, long HW,
                                                             int vec) {
    for (long plane = blockIdx.y; plane < planes; plane += gridDim.y) {
        const float b = shift[plane % C];
        float *xp = x + plane * HW;
        const float *rp = RES ? res + plane * HW : nullptr;
        if (vec) {
            const long n4 = HW >> 2;
            for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
                float4 v = reinterpret_cast<float4 *>(xp)[i];
                if (RES) {
                    const float4 r = reinterpret_cast<const float4 *>(rp)[i];
                    v.x = (v.x + b) + r.x; v.y = (v.y + b) + r.y; v.z = (v.z + b) + r.z; v.w = (v.w + b) + r.w;
                } else {
                    v.x += b; v.y += b; v.z += b; v.w += b;
                }
                // (max(v, 0) would turn NaN into 0; torch's relu keeps it: v < 0 ? 0 : v)
                v.x = v.x < 0.f ? 0.f : v.x; v.y = v.y < 0.f ? 0.f : v.y;
                v.z = v.z < 0.f ? 0.f : v.z; v.w = v.w < 0.f ? 0.f : v.w;
                reinterpret_cast<float4 *>(xp)[i] = v;
            }
        } else {
            for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += (long)gridDim.x * blockDim.x) {
                float v = xp[i] + b;
                if (RES) v += rp[i];
                xp[i] = v < 0.f ? 0.f : v;
            }
        }
    }
}

// bf16 storage (the autocast step): the bias add and the residual add round to bf16 one after the other, like the two
// torch kernels they replace
template <bool RES>
__global__ __launch_bounds__(256) void shift_relu_bf16_kernel(uint16_t *__restrict__ x, const float *__restrict__ shift,
                                                              const uint16_t *__restrict__ res, long planes, int C,
                                                              long HW, int vec) {
    for (long plane = blockIdx.y; plane < planes; plane += gridDim.y) {
        const float b = sr_bf16(sr_to_bf16(shift[plane % C]));          // autocast hands the convolution a bf16 bias
        uint16_t *xp = x + plane * HW;
        const uint16_t *rp = RES ? res + plane * HW : nullptr;
        if (vec) {
            const long n8 = HW >> 3;
            for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
                uint4 v = reinterpret_cast<uint4 *>(xp)[i];
                uint4 r = {0u, 0u, 0u, 0u};
                if (RES) r = reinterpret_cast<const uint4 *>(rp)[i];
                unsigned *vw = reinterpret_cast<unsigned *>(&v);
                const unsigned *rw = reinterpret_cast<const unsigned *>(&r);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float lo = sr_bf16((uint16_t)(vw[k] & 0xffffu)) + b, hi = sr_bf16((uint16_t)(vw[k] >> 16)) + b;
                    if (RES) {
                        lo = sr_bf16(sr_to_bf16(lo)) + sr_bf16((uint16_t)(rw[k] & 0xffffu));
                        hi = sr_bf16(sr_to_bf16(hi)) + sr_bf16((uint16_t)(rw[k] >> 16));
                    }
                    lo = lo < 0.f ? 0.f : lo;
                    hi = hi < 0.f ? 0.f : hi;
                    vw[k] = (unsigned)sr_to_bf16(lo) | ((unsigned)sr_to_bf16(hi) << 16);
                }
                reinterpret_cast<uint4 *>(xp)[i] = v;
            }
        } else {
            for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += (long)gridDim.x * blockDim.x) {
                float v = sr_bf16(xp[i]) + b;
                if (RES) v = sr_bf16(sr_to_bf16(v)) + sr_bf16(rp[i]);
                xp[i] = sr_to_bf16(v < 0.f ? 0.f : v);
            }
        }
    }
}

// the body of clipops_colsum_partial_f32 / _bf16: `who` names the entry point, `what` the kernel in a launch error
template <typename TX>
int colsum_partial(const char *who, const char *what, const TX *x, long rows, int cols, int chunk_rows, float *partial,
                   void *stream) {
    if (rows < 0 || cols < 0 || chunk_rows <= 0) return fail(1, who, "bad dimension");
    if (cols == 0 || rows == 0) return ok();
    if (!x || !partial) return fail(1, who, "null pointer");
    const long chunks = (rows + chunk_rows - 1) / chunk_rows;
    if (chunks > 65535) return fail(1, who, "too many chunks");
    return launch(what, colsum_partial_kernel<TX>, dim3((cols + 31) / 32, (unsigned)chunks), dim3(256), 0, stream, x, rows,
                  cols, chunk_rows, partial);
}

int shift_relu_check(const void *x, const void *shift, long planes, int C, long HW, const char *who) {
    if (planes < 0 || C <= 0 || HW < 0) return fail(1, who);
    if (planes && HW && (!x || !shift)) return fail(1, who);
    return 0;
}

// `per` 16-byte pieces (or elements) of a plane: 1024 of them per workgroup column, at most 64 columns; a plane per row
dim3 shift_relu_grid(long per, long planes) {
    const long gx = (per + 1023) / 1024;
    return dim3((unsigned)(gx > 64 ? 64 : gx < 1 ? 1 : gx), (unsigned)(planes > 65535 ? 65535 : planes));
}
}  // namespace

extern "C" {
int clipops_colsum_f32(const float *x, long rows, int cols, float *out, void *stream) {
    if (rows < 0 || cols < 0) return fail(1, "clipops_colsum_f32: bad dimension");
    if (cols == 0) return ok();
    if (!out || (rows > 0 && !x)) return fail(1, "clipops_colsum_f32: null pointer");
    if (cols % 4 == 0 && rows <= 2048 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0)
        return launch("colsum_quad_kernel", colsum_quad_kernel, dim3(cols / 4), dim3(256), 0, stream, x, rows, cols, out);
    return launch("colsum_kernel", colsum_kernel, dim3((cols + 31) / 32), dim3(256), 0, stream, x, rows, cols, out);
}

int clipops_colsum_partial_f32(const float *x, long rows, int cols, int chunk_rows, float *partial, void *stream) {
    return colsum_partial("clipops_colsum_partial_f32", "colsum_partial_kernel", x, rows, cols, chunk_rows, partial, stream);
}

int clipops_colsum_partial_bf16(const uint16_t *x, long rows, int cols, int chunk_rows, float *partial, void *stream) {
    return colsum_partial("clipops_colsum_partial_bf16", "colsum_partial_kernel<bf16>", x, rows, cols, chunk_rows, partial,
                          stream);
}

int clipops_relu_bwd_colsum_partial_f32(const float *g, const float *y, long rows, int cols, int chunk_rows, float *g2,
                                        float *partial, void *stream) {
    if (rows < 0 || cols < 0 || chunk_rows <= 0) return fail(1, "clipops_relu_bwd_colsum_partial: bad dimension");
    if (cols == 0 || rows == 0) return ok();
    if (!g || !y || !g2 || !partial) return fail(1, "clipops_relu_bwd_colsum_partial: null pointer");
    const long chunks = (rows + chunk_rows - 1) / chunk_rows;
    if (chunks > 65535) return fail(1, "clipops_relu_bwd_colsum_partial: too many chunks");
    return launch("relu_bwd_colsum_partial_kernel", relu_bwd_colsum_partial_kernel<float>, dim3((cols + 31) / 32,
                  (unsigned)chunks), dim3(256), 0, stream, g, y, rows, cols, chunk_rows, g2, partial);
}

int clipops_add_layer_norm_fwd_f32(const float *x, const float *res, const float *gamma, const float *beta, long rows,
                                   float eps, float *sum, float *y, float *stats, void *stream) {
    if (rows < 0) return fail(1, "clipops_add_layer_norm_fwd_f32: negative row count");
    if (rows == 0) return ok();
    if (!x || !res || !gamma || !beta || !sum || !y || !stats) return fail(1, "clipops_add_layer_norm_fwd_f32: null pointer");
    return launch("add_layer_norm_fwd_kernel", add_layer_norm_fwd_kernel<false>, dim3((unsigned)((rows + 3) / 4)),
                  dim3(256), 0, stream, x, res, gamma, beta, nullptr, rows, eps, sum, y, nullptr, stats);
}

int clipops_add_layer_norm_pos_fwd_f32(const float *x, const float *res, const float *gamma, const float *beta,
                                       const float *pos, long rows, float eps, float *sum, float *y, float *q,
                                       float *stats, void *stream) {
    if (rows < 0) return fail(1, "clipops_add_layer_norm_pos_fwd_f32: negative row count");
    if (rows == 0) return ok();
    if (!x || !res || !gamma || !beta || !pos || !sum || !y || !q || !stats)
        return fail(1, "clipops_add_layer_norm_pos_fwd_f32: null pointer");
    return launch("add_layer_norm_fwd_kernel<pos>", add_layer_norm_fwd_kernel<true>, dim3((unsigned)((rows + 3) / 4)),
                  dim3(256), 0, stream, x, res, gamma, beta, pos, rows, eps, sum, y, q, stats);
}

int clipops_add_layer_norm_bwd_f32(const float *grad_y, const float *sum, const float *stats, const float *gamma,
                                   long rows, int chunk_rows, float *grad_sum, float *partial, void *stream) {
    if (rows < 0 || chunk_rows <= 0) return fail(1, "clipops_add_layer_norm_bwd_f32: bad dimension");
    if (rows == 0) return ok();
    if (!grad_y || !sum || !stats || !gamma || !grad_sum || !partial)
        return fail(1, "clipops_add_layer_norm_bwd_f32: null pointer");
    return launch("add_layer_norm_bwd_kernel", add_layer_norm_bwd_kernel,
                  dim3((unsigned)((rows + chunk_rows - 1) / chunk_rows)), dim3(256), 0, stream, grad_y, sum, stats, gamma,
                  rows, chunk_rows, grad_sum, partial);
}

int clipops_add_layer_norm_fanin_bwd_f32(const float *g0, const float *g1, const float *g2, const float *sum,
                                         const float *stats, const float *gamma, long rows, int chunk_rows,
                                         float *grad_sum, float *partial, float *colsum_partial, void *stream) {
    if (rows < 0 || chunk_rows <= 0) return fail(1, "clipops_add_layer_norm_fanin_bwd_f32: bad dimension");
    if (rows == 0) return ok();
    const float *g[3] = {nullptr, nullptr, nullptr};      // the non-null slots, in slot order
    int n = 0;
    if (g0) g[n++] = g0;
    if (g1) g[n++] = g1;
    if (g2) g[n++] = g2;
    if (n == 0) return fail(1, "clipops_add_layer_norm_fanin_bwd_f32: no gradient input");
    if (!sum || !stats || !gamma || !grad_sum || !partial || !colsum_partial)
        return fail(1, "clipops_add_layer_norm_fanin_bwd_f32: null pointer");
    return launch("add_layer_norm_bwd_fanin_kernel", add_layer_norm_bwd_fanin_kernel,
                  dim3((unsigned)((rows + chunk_rows - 1) / chunk_rows)), dim3(256), 0, stream, g[0], g[1], g[2], sum,
                  stats, gamma, rows, chunk_rows, grad_sum, partial, colsum_partial);
}

int clipops_shift_relu_f32(float *x, const float *shift, const float *res, long planes, int C, long HW, void *stream) {
    if (shift_relu_check(x, shift, planes, C, HW, "clipops_shift_relu_f32: bad argument")) return 1;
    if (planes == 0 || HW == 0) return ok();
    const int vec = (HW % 4 == 0) && ((uintptr_t)x % 16 == 0) && (!res || (uintptr_t)res % 16 == 0);
    return launch("shift_relu_f32_kernel", res ? shift_relu_f32_kernel<true> : shift_relu_f32_kernel<false>,
                  shift_relu_grid(vec ? HW / 4 : HW, planes), dim3(256), 0, stream, x, shift, res, planes, C, HW, vec);
}

int clipops_shift_relu_bf16(uint16_t *x, const float *shift, const uint16_t *res, long planes, int C, long HW, void *stream) {
    if (shift_relu_check(x, shift, planes, C, HW, "clipops_shift_relu_bf16: bad argument")) return 1;
    if (planes == 0 || HW == 0) return ok();
    const int vec = (HW % 8 == 0) && ((uintptr_t)x % 16 == 0) && (!res || (uintptr_t)res % 16 == 0);
    return launch("shift_relu_bf16_kernel", res ? shift_relu_bf16_kernel<true> : shift_relu_bf16_kernel<false>,
                  shift_relu_grid(vec ? HW / 8 : HW, planes), dim3(256), 0, stream, x, shift, res, planes, C, HW, vec);
}
}  // extern "C"
