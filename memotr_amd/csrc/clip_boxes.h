// clip_boxes.h -- the decoder's box chain: sine embedding of the anchors, the clamped logit, box refinement.
// Included by clip_ops.hip after clip_common.h.
#pragma once

namespace {
// ----------------------------------------------------------------------------------------
// decoder glue: sine embedding of the anchors, clamped logit, box refinement
// ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sine_embed_fwd_kernel(const float *__restrict__ pos,
                                                            const float *__restrict__ dim_t, long n, int K, int F,
                                                            float scale, float *__restrict__ out) {
#pragma clang fp contract(off)
    const long total = n * K * F;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int j = (int)(i % F);
        const long ik = i / F;                      // = row * K + k
        const float e = (pos[ik] * scale) / dim_t[j];
        out[i] = (j & 1) ? cosf(e) : sinf(e);
    }
}

// one wavefront per (row, coordinate): the F terms of its gradient, summed in a fixed order
__global__ __launch_bounds__(256) void sine_embed_bwd_kernel(const float *__restrict__ pos,
                                                            const float *__restrict__ dim_t, long n, int K, int F,
                                                            float scale, const float *__restrict__ g,
                                                            float *__restrict__ gpos) {
    const int lane = threadIdx.x & 63;
    const long waves = ((long)gridDim.x * blockDim.x) >> 6;
    for (long ik = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; ik < n * K; ik += waves) {
        const float ps = pos[ik] * scale;
        float acc = 0.f;
        for (int j = lane; j < F; j += 64) {
            const float e = ps / dim_t[j];
            const float d = (j & 1) ? -sinf(e) : cosf(e);
            acc += (g[ik * F + j] * d) / dim_t[j];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) gpos[ik] = acc * scale;
    }
}

__device__ __forceinline__ float clamp_keep_nan(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

__device__ __forceinline__ float inv_sigmoid(float x, float eps) {
    return logf(clamp_keep_nan(x, eps, 1.f) / clamp_keep_nan(1.f - x, eps, 1.f));
}

// d inverse_sigmoid / dx with torch's clamp(min, max) masks (the gradient passes where min <= v <= max)
__device__ __forceinline__ float inv_sigmoid_grad(float x, float eps) {
    const float u = 1.f - x;
    const float x1 = clamp_keep_nan(x, eps, 1.f), x2 = clamp_keep_nan(u, eps, 1.f);
    const float a = (x >= eps && x <= 1.f) ? 1.f / x1 : 0.f;
    const float b = (u >= eps && u <= 1.f) ? 1.f / x2 : 0.f;
    return a + b;
}

__global__ __launch_bounds__(256) void inverse_sigmoid_fwd_kernel(const float *__restrict__ x, long n, float eps,
                                                                 float *__restrict__ y) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        y[i] = inv_sigmoid(x[i], eps);
}

__global__ __launch_bounds__(256) void inverse_sigmoid_bwd_kernel(const float *__restrict__ x,
                                                                 const float *__restrict__ g, long n, float eps,
                                                                 float *__restrict__ gx) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        gx[i] = g[i] * inv_sigmoid_grad(x[i], eps);
}

__global__ __launch_bounds__(256) void refine_boxes_fwd_kernel(const float *__restrict__ delta,
                                                              const float *__restrict__ ref, long n, float eps,
                                                              float *__restrict__ out) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        out[i] = sigmoidf(delta[i] + inv_sigmoid(ref[i], eps));
}

// Layer 0 of the Deformable-DETR variant (reference models/deformable_decoder.py:141-149 and memotr.py:148-158): the box
// head refines all four coordinates of the 4-d reference, the decoder only xy and takes sigmoid(delta) for wh.  Both boxes
// from one read of `delta`, one thread per row of four; element for element the arithmetic of refine_boxes_fwd_kernel
// (`dec` wh: the same sigmoid with inverse_sigmoid(0.5) == 0 added).  VEC: all four pointers are 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(256) void refine_boxes_split_fwd_kernel(const float *__restrict__ delta,
                                                                    const float *__restrict__ ref, long n_rows,
                                                                    float eps, float *__restrict__ head,
                                                                    float *__restrict__ dec) {
    for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += (long)gridDim.x * blockDim.x) {
        float4 d, f;
        if (VEC) {
            d = reinterpret_cast<const float4 *>(delta)[r];
            f = reinterpret_cast<const float4 *>(ref)[r];
        } else {
            d = make_float4(delta[4 * r], delta[4 * r + 1], delta[4 * r + 2], delta[4 * r + 3]);
            f = make_float4(ref[4 * r], ref[4 * r + 1], ref[4 * r + 2], ref[4 * r + 3]);
        }
        float4 h, c;
        h.x = sigmoidf(d.x + inv_sigmoid(f.x, eps));
        h.y = sigmoidf(d.y + inv_sigmoid(f.y, eps));
        h.z = sigmoidf(d.z + inv_sigmoid(f.z, eps));
        h.w = sigmoidf(d.w + inv_sigmoid(f.w, eps));
        c.x = h.x;
        c.y = h.y;
        c.z = sigmoidf(d.z);
        c.w = sigmoidf(d.w);
        if (VEC) {
            reinterpret_cast<float4 *>(head)[r] = h;
            reinterpret_cast<float4 *>(dec)[r] = c;
        } else {
            head[4 * r] = h.x; head[4 * r + 1] = h.y; head[4 * r + 2] = h.z; head[4 * r + 3] = h.w;
            dec[4 * r] = c.x; dec[4 * r + 1] = c.y; dec[4 * r + 2] = c.z; dec[4 * r + 3] = c.w;
        }
    }
}

__global__ __launch_bounds__(256) void refine_boxes_bwd_kernel(const float *__restrict__ out,
                                                              const float *__restrict__ ref,
                                                              const float *__restrict__ g, long n, float eps,
                                                              float *__restrict__ gdelta, float *__restrict__ gref) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float y = out[i];
        const float gs = (g[i] * (1.f - y)) * y;          // sigmoid backward
        gdelta[i] = gs;
        if (gref) gref[i] = gs * inv_sigmoid_grad(ref[i], eps);
    }
}
}  // namespace

extern "C" {
int clipops_sine_embed_fwd_f32(const float *pos, const float *dim_t, long n, int K, int F, float scale, float *out,
                               void *stream) {
    if (n < 0 || K <= 0 || F <= 0) return fail(1, "clipops_sine_embed_fwd_f32: bad dimension");
    if (n == 0) return ok();
    if (!pos || !dim_t || !out) return fail(1, "clipops_sine_embed_fwd_f32: null pointer");
    return launch("sine_embed_fwd_kernel", sine_embed_fwd_kernel, dim3(grid_for(n * K * F)), dim3(256), 0, stream, pos,
                  dim_t, n, K, F, scale, out);
}

int clipops_sine_embed_bwd_f32(const float *pos, const float *dim_t, long n, int K, int F, float scale,
                               const float *grad_out, float *grad_pos, void *stream) {
    if (n < 0 || K <= 0 || F <= 0) return fail(1, "clipops_sine_embed_bwd_f32: bad dimension");
    if (n == 0) return ok();
    if (!pos || !dim_t || !grad_out || !grad_pos) return fail(1, "clipops_sine_embed_bwd_f32: null pointer");
    return launch("sine_embed_bwd_kernel", sine_embed_bwd_kernel, dim3(grid_for(n * K * 64)), dim3(256), 0, stream, pos,
                  dim_t, n, K, F, scale, grad_out, grad_pos);
}

int clipops_inverse_sigmoid_fwd_f32(const float *x, long n, float eps, float *y, void *stream) {
    if (n < 0) return fail(1, "clipops_inverse_sigmoid_fwd_f32: negative count");
    if (n == 0) return ok();
    if (!x || !y) return fail(1, "clipops_inverse_sigmoid_fwd_f32: null pointer");
    return launch("inverse_sigmoid_fwd_kernel", inverse_sigmoid_fwd_kernel, dim3(grid_for(n)), dim3(256), 0, stream, x, n,
                  eps, y);
}

int clipops_inverse_sigmoid_bwd_f32(const float *x, const float *grad_y, long n, float eps, float *grad_x,
                                    void *stream) {
    if (n < 0) return fail(1, "clipops_inverse_sigmoid_bwd_f32: negative count");
    if (n == 0) return ok();
    if (!x || !grad_y || !grad_x) return fail(1, "clipops_inverse_sigmoid_bwd_f32: null pointer");
    return launch("inverse_sigmoid_bwd_kernel", inverse_sigmoid_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, stream, x,
                  grad_y, n, eps, grad_x);
}

int clipops_refine_boxes_fwd_f32(const float *delta, const float *ref, long n, float eps, float *out, void *stream) {
    if (n < 0) return fail(1, "clipops_refine_boxes_fwd_f32: negative count");
    if (n == 0) return ok();
    if (!delta || !ref || !out) return fail(1, "clipops_refine_boxes_fwd_f32: null pointer");
    return launch("refine_boxes_fwd_kernel", refine_boxes_fwd_kernel, dim3(grid_for(n)), dim3(256), 0, stream, delta, ref,
                  n, eps, out);
}

int clipops_refine_boxes_split_fwd_f32(const float *delta, const float *ref, long n_rows, float eps, float *out_head,
                                       float *out_dec, void *stream) {
    if (n_rows < 0) return fail(1, "clipops_refine_boxes_split_fwd_f32: negative count");
    if (n_rows == 0) return ok();
    if (!delta || !ref || !out_head || !out_dec) return fail(1, "clipops_refine_boxes_split_fwd_f32: null pointer");
    if (out_head == out_dec) return fail(1, "clipops_refine_boxes_split_fwd_f32: the two outputs alias");
    const bool vec = (((uintptr_t)delta | (uintptr_t)ref | (uintptr_t)out_head | (uintptr_t)out_dec) & 15) == 0;
    return launch("refine_boxes_split_fwd_kernel",
                  vec ? refine_boxes_split_fwd_kernel<true> : refine_boxes_split_fwd_kernel<false>, dim3(grid_for(n_rows)),
                  dim3(256), 0, stream, delta, ref, n_rows, eps, out_head, out_dec);
}

int clipops_refine_boxes_bwd_f32(const float *out, const float *ref, const float *grad_out, long n, float eps,
                                 float *grad_delta, float *grad_ref, void *stream) {
    if (n < 0) return fail(1, "clipops_refine_boxes_bwd_f32: negative count");
    if (n == 0) return ok();
    if (!out || !ref || !grad_out || !grad_delta) return fail(1, "clipops_refine_boxes_bwd_f32: null pointer");
    return launch("refine_boxes_bwd_kernel", refine_boxes_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, stream, out, ref,
                  grad_out, n, eps, grad_delta, grad_ref);
}
}  // extern "C"
