// clip_common.h -- what the kernel families of libclip_ops_hip.so share: the error text and the launch path of the entry
// points, the dynamic-LDS opt-in, box arithmetic, wave reductions and the ballot ranks.
// Included first by clip_ops.hip, at file scope; every family header opens the anonymous namespace again for its kernels.
#pragma once

namespace {
thread_local char g_err[256] = {0};

int fail(int code, const char *msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

// the same for entry points that share a body: "<entry point>: <what is wrong>"
int fail(int code, const char *who, const char *msg) {
    snprintf(g_err, sizeof(g_err), "%s: %s", who, msg);
    return code;
}

// nothing to do, or done: no error text, code 0
int ok() {
    g_err[0] = 0;
    return 0;
}

int check_launch(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    g_err[0] = 0;
    return 0;
}

// one kernel launch of an entry point, checked under the kernel's name: 0, or the HIP error with g_err set
template <typename K, typename... A>
int launch(const char *what, K kernel, dim3 grid, dim3 block, size_t lds, void *stream, const A &...args) {
    hipLaunchKernelGGL(kernel, grid, block, lds, (hipStream_t)stream, args...);
    return check_launch(what);
}

int grid_for(long total) {
    long g = (total + 255) / 256;
    if (g < 1) g = 1;
    return (int)(g > 4096 ? 4096 : g);
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// dynamic LDS above 64 KiB has to be allowed once per kernel and device (one bit per device ordinal in `done`)
int allow_lds(const void *kernel, size_t lds, std::atomic<unsigned long long> &done) {
    if (lds <= 64 * 1024) return 0;
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return 0;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 2048);
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "hipFuncSetAttribute: %s", hipGetErrorString(e));
        return (int)e;
    }
    done.fetch_or(bit, std::memory_order_release);
    return 0;
}

typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef double f64x4_t __attribute__((ext_vector_type(4)));

struct Box {
    float x1, y1, x2, y2;
};

// cxcywh -> xyxy (reference utils/box_ops.py:16-20)
__device__ __forceinline__ Box to_xyxy(float cx, float cy, float w, float h) {
#pragma clang fp contract(off)
    Box b;
    b.x1 = cx - 0.5f * w;
    b.y1 = cy - 0.5f * h;
    b.x2 = cx + 0.5f * w;
    b.y2 = cy + 0.5f * h;
    return b;
}

// generalised IoU of two xyxy boxes (reference utils/box_ops.py:49-70, one pair)
__device__ __forceinline__ float giou_pair(const Box a, const Box b) {
#pragma clang fp contract(off)
    const float iw = fmaxf(fminf(a.x2, b.x2) - fmaxf(a.x1, b.x1), 0.f);
    const float ih = fmaxf(fminf(a.y2, b.y2) - fmaxf(a.y1, b.y1), 0.f);
    const float inter = iw * ih;
    const float area_a = (a.x2 - a.x1) * (a.y2 - a.y1);
    const float area_b = (b.x2 - b.x1) * (b.y2 - b.y1);
    const float uni = area_a + area_b - inter;
    const float iou = inter / uni;
    const float hw = fmaxf(fmaxf(a.x2, b.x2) - fminf(a.x1, b.x1), 0.f);
    const float hh = fmaxf(fmaxf(a.y2, b.y2) - fminf(a.y1, b.y1), 0.f);
    const float hull = hw * hh;
    return iou - (hull - uni) / hull;
}

// IoU of two xyxy boxes (reference utils/box_ops.py:23-46, one pair): pair_iou_kernel and the track hand-over share it
__device__ __forceinline__ float iou_pair(const Box a, const Box b) {
#pragma clang fp contract(off)
    const float iw = fmaxf(fminf(a.x2, b.x2) - fmaxf(a.x1, b.x1), 0.f);
    const float ih = fmaxf(fminf(a.y2, b.y2) - fmaxf(a.y1, b.y1), 0.f);
    const float inter = iw * ih;
    const float uni = (a.x2 - a.x1) * (a.y2 - a.y1) + (b.x2 - b.x1) * (b.y2 - b.y1) - inter;
    return inter / uni;
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

__device__ __forceinline__ float powg(float x, float gamma) { return gamma == 2.f ? x * x : powf(x, gamma); }

__device__ __forceinline__ float wave_sum64(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// The ballot ranks of a workgroup of NW wavefronts: `before` = the flagged threads below this one, `total` = all of them
// (a 64-bit ballot and the population count of the lower lanes inside a wavefront, the wave totals through LDS).  The
// caller puts a barrier in front of the next use of `wave_total`.
template <int NW>
__device__ __forceinline__ void bank_ranks(bool flag, int lane, int wave, int *wave_total, int &before, int &total) {
    const unsigned long long m = __ballot(flag);
    const int below = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_total[wave] = __popcll(m);
    __syncthreads();
    before = below;
    total = 0;
    for (int v = 0; v < NW; ++v) {
        const int t = wave_total[v];
        before += v < wave ? t : 0;
        total += t;
    }
}
}  // namespace
