// opt_ops.hip -- gradient-norm clipping and the AdamW update of a whole parameter list as two launches (C ABI, table
// layout, the arithmetic and its order: include/opt_ops_hip.h; the same statement in torch ops: memotr_amd/optim.py;
// why it is cut this way and what it moves: DESIGN.md, "Optimizer step").
//
//   sumsq_kernel   one workgroup per chunk of OPTSTEP_CHUNK elements: sum of g^2 in float64, one partial per chunk
//   adamw_kernel   one workgroup per chunk: adds the partials (a few thousand doubles, from L2) in a fixed order, forms
//                  the clip factor and the group's scalars once, then streams p, g, m, v through registers
// Both are memory-bound with no reuse: 4 B per element in the first, 28 B in the second.  A thread takes 16-byte pieces
// 256 apart, two in flight; a tensor whose four pointers are not all 16-byte aligned takes the 4-byte path, and the
// last numel % 4 elements of a tensor always do.  No atomics: the same inputs give the same bits.  float32 arithmetic
// with contraction off (the build passes -ffp-contract=off) and correctly rounded division and square root.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/opt_ops_hip.h"

namespace {

thread_local char g_err[256] = {0};      // text of this thread's last error; read by optstep_last_error() only

int fail(int code, const char *msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

constexpr int BLOCK = 256;
constexpr int CHUNK = OPTSTEP_CHUNK;
static_assert(CHUNK % (4 * BLOCK) == 0, "a full chunk is a whole number of 16-byte pieces per thread");

// The table's pointers are device memory: loads and stores through them are global ones, not flat ones.
typedef float f4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) const float cgfloat;
typedef __attribute__((address_space(1))) f4 gf4;
typedef __attribute__((address_space(1))) const f4 cgf4;

__device__ __forceinline__ bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Sum of red[0 .. BLOCK) in a fixed tree order; every thread gets the result.
__device__ __forceinline__ double block_sum(double x, double *red) {
    const int tid = threadIdx.x;
    red[tid] = x;
    __syncthreads();
    for (int half = BLOCK / 2; half > 0; half >>= 1) {
        if (tid < half) red[tid] = red[tid] + red[tid + half];
        __syncthreads();
    }
    const double total = red[0];
    __syncthreads();
    return total;
}

// The chunk of this workgroup: false when the row points outside the tables or the tensor has no gradient.
struct Piece {
    int t;
    int64_t begin;
    int len;
    optstep_tensor row;
};

__device__ __forceinline__ bool piece_of(const optstep_tensor *tensors, const optstep_chunk *chunks, int n_tensors,
                                         Piece &pc) {
    const optstep_chunk ch = chunks[blockIdx.x];
    pc.t = __builtin_amdgcn_readfirstlane(ch.tensor);
    const int index = __builtin_amdgcn_readfirstlane(ch.index);
    if (pc.t < 0 || pc.t >= n_tensors || index < 0) return false;
    pc.row = tensors[pc.t];
    pc.begin = (int64_t)index * CHUNK;
    if (pc.begin >= pc.row.numel) return false;
    const int64_t left = pc.row.numel - pc.begin;
    pc.len = left < CHUNK ? (int)left : CHUNK;
    return true;
}

__global__ __launch_bounds__(BLOCK) void sumsq_kernel(const optstep_tensor *__restrict__ tensors,
                                                      const optstep_chunk *__restrict__ chunks, int n_tensors,
                                                      double *__restrict__ partials, const float *__restrict__ steps,
                                                      float *__restrict__ steps_prev) {
    __shared__ double red[BLOCK];
    const int tid = threadIdx.x;
    Piece pc;
    const bool ok = piece_of(tensors, chunks, n_tensors, pc);
    if (!ok || pc.row.g == nullptr) {
        if (tid == 0) partials[blockIdx.x] = 0.0;
        return;
    }
    if (pc.begin == 0 && tid == 0) steps_prev[pc.t] = steps[pc.t];
    cgfloat *g = (cgfloat *)(pc.row.g + pc.begin);
    double acc = 0.0;
    if (aligned16(pc.row.g)) {
        cgf4 *g4 = (cgf4 *)g;
        const int n4 = pc.len >> 2;
#pragma unroll 4
        for (int i = tid; i < n4; i += BLOCK) {
            const f4 x = g4[i];
            acc += (double)x.x * (double)x.x;
            acc += (double)x.y * (double)x.y;
            acc += (double)x.z * (double)x.z;
            acc += (double)x.w * (double)x.w;
        }
        const int i = (n4 << 2) + tid;                        // the last numel % 4 elements of the tensor
        if (i < pc.len) acc += (double)g[i] * (double)g[i];
    } else {
#pragma unroll 4
        for (int i = tid; i < pc.len; i += BLOCK) acc += (double)g[i] * (double)g[i];
    }
    const double total = block_sum(acc, red);
    if (tid == 0) partials[blockIdx.x] = total;
}

// The scalars of one chunk's update, each rounded to float32 once from its float64 value.
struct Scalars {
    float c, d, w, b, o, s, q, e;
};

__device__ __forceinline__ void update(float &p, float g, float &m, float &v, const Scalars &k) {
    const float gs = g * k.c;
    m = m + k.w * (gs - m);
    v = v * k.b + (k.o * gs) * gs;
    const float denom = sqrtf(v) / k.q + k.e;
    p = p * k.d - k.s * (m / denom);
}

__device__ __forceinline__ void update4(f4 &p, const f4 &g, f4 &m, f4 &v, const Scalars &k) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float P = p[c], M = m[c], V = v[c];
        update(P, g[c], M, V, k);
        p[c] = P;
        m[c] = M;
        v[c] = V;
    }
}

__global__ __launch_bounds__(BLOCK) void adamw_kernel(const optstep_tensor *__restrict__ tensors,
                                                      const optstep_chunk *__restrict__ chunks, int n_tensors,
                                                      int n_chunks, const double *__restrict__ partials,
                                                      float *__restrict__ steps, const float *__restrict__ steps_prev,
                                                      const optstep_hyper hyper, int n_groups, double max_norm,
                                                      float *__restrict__ total_norm_out) {
    __shared__ double red[BLOCK];
    __shared__ Scalars shared_k;
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int i = tid; i < n_chunks; i += BLOCK) acc += partials[i];
    const double total = sqrt(block_sum(acc, red));
    double coef = 1.0;
    if (max_norm > 0.0) {
        const double c = max_norm / (total + 1e-6);
        coef = c > 1.0 ? 1.0 : c;                             // (NaN goes through, as torch.clamp's)
    }
    if (blockIdx.x == 0 && tid == 0) *total_norm_out = (float)total;

    Piece pc;
    if (!piece_of(tensors, chunks, n_tensors, pc) || pc.row.g == nullptr) return;
    const int grp = __builtin_amdgcn_readfirstlane(pc.row.group);
    if (grp < 0 || grp >= n_groups) return;
    if (tid == 0) {
        const optstep_group h = hyper.group[grp];
        const float step = steps_prev[pc.t] + 1.0f;
        const double bc1 = 1.0 - pow(h.beta1, (double)step);
        const double bc2 = 1.0 - pow(h.beta2, (double)step);
        Scalars k;
        k.c = (float)coef;
        k.d = (float)(1.0 - h.lr * h.weight_decay);
        k.w = (float)(1.0 - h.beta1);
        k.b = (float)h.beta2;
        k.o = (float)(1.0 - h.beta2);
        k.s = (float)(h.lr / bc1);
        k.q = (float)sqrt(bc2);
        k.e = (float)h.eps;
        shared_k = k;
        if (pc.begin == 0) steps[pc.t] = step;
    }
    __syncthreads();
    const Scalars k = shared_k;

    gfloat *p = (gfloat *)(pc.row.p + pc.begin);
    cgfloat *g = (cgfloat *)(pc.row.g + pc.begin);
    gfloat *m = (gfloat *)(pc.row.m + pc.begin);
    gfloat *v = (gfloat *)(pc.row.v + pc.begin);
    int done = 0;                                             // elements the 16-byte path covers
    if (aligned16(pc.row.p) && aligned16(pc.row.g) && aligned16(pc.row.m) && aligned16(pc.row.v)) {
        gf4 *p4 = (gf4 *)p;
        cgf4 *g4 = (cgf4 *)g;
        gf4 *m4 = (gf4 *)m;
        gf4 *v4 = (gf4 *)v;
        const int n4 = pc.len >> 2;
        int i = tid;
        for (; i + BLOCK < n4; i += 2 * BLOCK) {              // two pieces in flight: eight loads before the first store
            const int j = i + BLOCK;
            f4 P0 = p4[i], P1 = p4[j];
            const f4 G0 = g4[i], G1 = g4[j];
            f4 M0 = m4[i], M1 = m4[j];
            f4 V0 = v4[i], V1 = v4[j];
            update4(P0, G0, M0, V0, k);
            update4(P1, G1, M1, V1, k);
            p4[i] = P0;
            m4[i] = M0;
            v4[i] = V0;
            p4[j] = P1;
            m4[j] = M1;
            v4[j] = V1;
        }
        if (i < n4) {
            f4 P0 = p4[i];
            const f4 G0 = g4[i];
            f4 M0 = m4[i];
            f4 V0 = v4[i];
            update4(P0, G0, M0, V0, k);
            p4[i] = P0;
            m4[i] = M0;
            v4[i] = V0;
        }
        done = n4 << 2;
    }
    for (int i = done + tid; i < pc.len; i += BLOCK) {        // unaligned tensors, and the last numel % 4 elements
        float P = p[i], M = m[i], V = v[i];
        update(P, g[i], M, V, k);
        p[i] = P;
        m[i] = M;
        v[i] = V;
    }
}

// ------------------------------------------------------------------------------------------------------ host side
int check_launch(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
        return 3;
    }
    g_err[0] = 0;
    return 0;
}

int check_counts(int n_tensors, int n_chunks, const char *who) {
    char msg[200];
    if (n_tensors < 0 || n_chunks < 0) {
        snprintf(msg, sizeof(msg), "%s: negative count (%d tensors, %d chunks)", who, n_tensors, n_chunks);
        return fail(1, msg);
    }
    if (n_chunks > OPTSTEP_MAX_CHUNKS) {
        snprintf(msg, sizeof(msg), "%s: %d chunks exceed the %d one launch covers", who, n_chunks, OPTSTEP_MAX_CHUNKS);
        return fail(2, msg);
    }
    return 0;
}

}  // namespace

extern "C" {

int optstep_abi_version(void) { return OPTSTEP_ABI_VERSION; }

const char *optstep_last_error(void) { return g_err; }

int optstep_sumsq(const optstep_tensor *tensors, const optstep_chunk *chunks, int n_tensors, int n_chunks,
                  double *partials, const float *steps, float *steps_prev, void *stream) {
    if (const int rc = check_counts(n_tensors, n_chunks, "optstep_sumsq")) return rc;
    if (n_chunks == 0) { g_err[0] = 0; return 0; }
    if (!tensors || !chunks || !partials || !steps || !steps_prev) return fail(1, "optstep_sumsq: null pointer");
    if (n_tensors == 0) return fail(1, "optstep_sumsq: chunks without tensors");
    hipLaunchKernelGGL(sumsq_kernel, dim3(n_chunks), dim3(BLOCK), 0, (hipStream_t)stream, tensors, chunks, n_tensors,
                       partials, steps, steps_prev);
    return check_launch("sumsq_kernel");
}

int optstep_adamw(const optstep_tensor *tensors, const optstep_chunk *chunks, int n_tensors, int n_chunks,
                  const double *partials, float *steps, const float *steps_prev, const optstep_hyper *hyper,
                  int n_groups, double max_norm, float *total_norm_out, void *stream) {
    if (const int rc = check_counts(n_tensors, n_chunks, "optstep_adamw")) return rc;
    if (n_groups < 1 || n_groups > OPTSTEP_MAX_GROUPS) {
        char msg[200];
        snprintf(msg, sizeof(msg), "optstep_adamw: n_groups = %d is outside 1 .. %d", n_groups, OPTSTEP_MAX_GROUPS);
        return fail(1, msg);
    }
    if (!hyper) return fail(1, "optstep_adamw: null pointer (hyper)");
    for (int i = 0; i < n_groups; ++i) {                      // what torch.optim.AdamW's constructor refuses
        const optstep_group &h = hyper->group[i];
        const bool ok = h.lr >= 0.0 && isfinite(h.lr) && h.eps >= 0.0 && isfinite(h.eps) && h.weight_decay >= 0.0 &&
                        isfinite(h.weight_decay) && h.beta1 >= 0.0 && h.beta1 < 1.0 && h.beta2 >= 0.0 && h.beta2 < 1.0;
        if (!ok) {
            char msg[200];
            snprintf(msg, sizeof(msg), "optstep_adamw: invalid hyper-parameter in group %d (lr %g, weight_decay %g, "
                     "betas %g %g, eps %g)", i, h.lr, h.weight_decay, h.beta1, h.beta2, h.eps);
            return fail(1, msg);
        }
    }
    if (n_chunks == 0) { g_err[0] = 0; return 0; }
    if (!tensors || !chunks || !partials || !steps || !steps_prev || !total_norm_out)
        return fail(1, "optstep_adamw: null pointer");
    if (n_tensors == 0) return fail(1, "optstep_adamw: chunks without tensors");
    hipLaunchKernelGGL(adamw_kernel, dim3(n_chunks), dim3(BLOCK), 0, (hipStream_t)stream, tensors, chunks, n_tensors,
                       n_chunks, partials, steps, steps_prev, *hyper, n_groups, max_norm, total_norm_out);
    return check_launch("adamw_kernel");
}

}  // extern "C"
