// clip_attention.h -- multi-head self-attention over the decoder queries: forward and the two backward kernels, K / V
// (or Q / dO) of a head staged in dynamic LDS.
// Included by clip_ops.hip after clip_common.h.
#pragma once

namespace {
// ----------------------------------------------------------------------------------------
// multi-head self-attention over the decoder queries (head_dim 32, L <= 512): forward and backward
// ----------------------------------------------------------------------------------------
// One workgroup = kRows rows x kLanes lanes (256 threads) of one (batch, head).  A lane of a row visits the rows of
// the OTHER axis j = lane, lane + kLanes, ... : 32-float dot products against rows staged in LDS (pitch 36 floats: the
// sixteen lanes of a row cover all 64 banks exactly once per ds_read_b128, the four rows of a wavefront read the same
// addresses = broadcast).  16 lanes per row: a decoder call is only ~2,500 rows x 320 keys, so the per-lane chain
// (20 keys) sets the kernel's latency, not throughput.
constexpr int kLanes = 16;         // lanes per row
constexpr int kRows = 256 / kLanes;  // rows per workgroup
constexpr int kHd = 32;            // head dimension
constexpr int kPitch = 36;         // LDS row pitch in floats

__device__ __forceinline__ void load_row32(const float *p, float *r) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const f32x4_t v = *reinterpret_cast<const f32x4_t *>(p + 4 * i);
        r[4 * i] = v.x; r[4 * i + 1] = v.y; r[4 * i + 2] = v.z; r[4 * i + 3] = v.w;
    }
}

__device__ __forceinline__ float dot32(const float *a, const float *lds_row) {
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const f32x4_t v = *reinterpret_cast<const f32x4_t *>(lds_row + 4 * i);
        s0 = fmaf(a[4 * i], v.x, s0);
        s1 = fmaf(a[4 * i + 1], v.y, s1);
        s0 = fmaf(a[4 * i + 2], v.z, s0);
        s1 = fmaf(a[4 * i + 3], v.w, s1);
    }
    return s0 + s1;
}

// the same sum from two register rows.  D = dO . O of the backward uses the association of dot32 on purpose: where a
// row attends to ONE key (L = 1, a single live key) O is that key's V bit for bit, and dO . V_j - D must be exactly zero
__device__ __forceinline__ float dot32r(const float *a, const float *b) {
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        s0 = fmaf(a[4 * i], b[4 * i], s0);
        s1 = fmaf(a[4 * i + 1], b[4 * i + 1], s1);
        s0 = fmaf(a[4 * i + 2], b[4 * i + 2], s0);
        s1 = fmaf(a[4 * i + 3], b[4 * i + 3], s1);
    }
    return s0 + s1;
}

__device__ __forceinline__ void axpy32(float *acc, float w, const float *lds_row) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const f32x4_t v = *reinterpret_cast<const f32x4_t *>(lds_row + 4 * i);
        acc[4 * i] = fmaf(w, v.x, acc[4 * i]);
        acc[4 * i + 1] = fmaf(w, v.y, acc[4 * i + 1]);
        acc[4 * i + 2] = fmaf(w, v.z, acc[4 * i + 2]);
        acc[4 * i + 3] = fmaf(w, v.w, acc[4 * i + 3]);
    }
}

// sum / max over the kLanes lanes of a row (they differ in the low bits of the lane id)
__device__ __forceinline__ float sum8l(float x) {
#pragma unroll
    for (int o = 1; o < kLanes; o <<= 1) x += __shfl_xor(x, o, 64);
    return x;
}
__device__ __forceinline__ float max8l(float x) {
#pragma unroll
    for (int o = 1; o < kLanes; o <<= 1) x = fmaxf(x, __shfl_xor(x, o, 64));
    return x;
}

// cooperative copy of L rows (32 floats each, `rs` apart) into LDS at pitch kPitch
__device__ __forceinline__ void stage_rows(float *dst, const float *src, long rs, int L) {
    for (int i = threadIdx.x; i < L * 8; i += blockDim.x) {
        const int r = i >> 3, c = (i & 7) * 4;
        *reinterpret_cast<f32x4_t *>(dst + r * kPitch + c) = *reinterpret_cast<const f32x4_t *>(src + r * rs + c);
    }
}

__global__ __launch_bounds__(256) void mha_fwd_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                     const float *__restrict__ v, long q_bs, long q_rs, long k_bs,
                                                     long k_rs, long v_bs, long v_rs,
                                                     const uint8_t *__restrict__ key_mask, int H, int L, float scale,
                                                     float *__restrict__ out, float *__restrict__ lse) {
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    float *Ks = s_mem, *Vs = s_mem + (size_t)L * kPitch;
    const int h = blockIdx.y, b = blockIdx.z;
    stage_rows(Ks, k + b * k_bs + h * kHd, k_rs, L);
    stage_rows(Vs, v + b * v_bs + h * kHd, v_rs, L);
    __syncthreads();
    const int row = blockIdx.x * kRows + threadIdx.x / kLanes, sub = threadIdx.x % kLanes;
    const bool row_ok = row < L;
    const int rowc = row_ok ? row : L - 1;
    float qr[kHd];
    load_row32(q + b * q_bs + rowc * q_rs + h * kHd, qr);
#pragma unroll
    for (int i = 0; i < kHd; ++i) qr[i] *= scale;
    const uint8_t *mk = key_mask ? key_mask + (long)b * L : nullptr;
    float m = -INFINITY, l = 0.f, acc[kHd];
#pragma unroll
    for (int i = 0; i < kHd; ++i) acc[i] = 0.f;
    for (int j = sub; j < L; j += kLanes) {
        if (mk && mk[j]) continue;
        const float s = dot32(qr, Ks + j * kPitch);
        const float m_new = fmaxf(m, s);
        const float corr = expf(m - m_new), p = expf(s - m_new);      // exp(-inf) = 0 on the first key
        l = l * corr + p;
#pragma unroll
        for (int i = 0; i < kHd; ++i) acc[i] *= corr;
        axpy32(acc, p, Vs + j * kPitch);
        m = m_new;
    }
    // merge the lanes of the row
    const float M = max8l(m);
    const float w = (m == -INFINITY) ? 0.f : expf(m - M);          // a lane may have seen no key at all
    const float Lsum = sum8l(l * w);
    const float inv = 1.f / Lsum;
    float *o = out + ((long)b * L + rowc) * (H * kHd) + h * kHd;
#pragma unroll
    for (int i = 0; i < kHd; ++i) {
        const float t = sum8l(acc[i] * w) * inv;
        if (row_ok && (i >> 2) == sub) o[i] = t;                   // lane `sub` stores floats 4*sub .. 4*sub+3
    }
    if (row_ok && sub == 0) lse[((long)b * H + h) * L + row] = M + logf(Lsum);
}

// grad_q: same decomposition as the forward (a workgroup = kRows query rows; K and V of the head in LDS)
__global__ __launch_bounds__(256) void mha_bwd_q_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                       const float *__restrict__ v, long q_bs, long q_rs, long k_bs,
                                                       long k_rs, long v_bs, long v_rs,
                                                       const uint8_t *__restrict__ key_mask,
                                                       const float *__restrict__ out, const float *__restrict__ lse,
                                                       const float *__restrict__ go, int H, int L, float scale,
                                                       float *__restrict__ gq, long gq_bs, long gq_rs) {
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    float *Ks = s_mem, *Vs = s_mem + (size_t)L * kPitch;
    const int h = blockIdx.y, b = blockIdx.z;
    stage_rows(Ks, k + b * k_bs + h * kHd, k_rs, L);
    stage_rows(Vs, v + b * v_bs + h * kHd, v_rs, L);
    __syncthreads();
    const int row = blockIdx.x * kRows + threadIdx.x / kLanes, sub = threadIdx.x % kLanes;
    const bool row_ok = row < L;
    const int rowc = row_ok ? row : L - 1;
    float qr[kHd], gr[kHd], acc[kHd];
    load_row32(q + b * q_bs + rowc * q_rs + h * kHd, qr);
    const long orow = ((long)b * L + rowc) * (H * kHd) + h * kHd;
    load_row32(go + orow, gr);
    float D = 0.f;                                                  // rowsum(dP o P) = dO . O
    {
        float orr[kHd];
        load_row32(out + orow, orr);
        D = dot32r(gr, orr);
    }
#pragma unroll
    for (int i = 0; i < kHd; ++i) { qr[i] *= scale; acc[i] = 0.f; }
    const float ls = lse[((long)b * H + h) * L + rowc];
    const uint8_t *mk = key_mask ? key_mask + (long)b * L : nullptr;
    for (int j = sub; j < L; j += kLanes) {
        if (mk && mk[j]) continue;
        const float p = expf(dot32(qr, Ks + j * kPitch) - ls);
        const float ds = p * (dot32(gr, Vs + j * kPitch) - D);
        axpy32(acc, ds, Ks + j * kPitch);
    }
    float *g = gq + b * gq_bs + rowc * gq_rs + h * kHd;
#pragma unroll
    for (int i = 0; i < kHd; ++i) {
        const float t = sum8l(acc[i]) * scale;
        if (row_ok && (i >> 2) == sub) g[i] = t;
    }
}

// grad_k, grad_v: a workgroup = kRows KEY rows; Q and dO of the head in LDS, lse and D = dO . O per query too
__global__ __launch_bounds__(256) void mha_bwd_kv_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                        const float *__restrict__ v, long q_bs, long q_rs, long k_bs,
                                                        long k_rs, long v_bs, long v_rs,
                                                        const uint8_t *__restrict__ key_mask,
                                                        const float *__restrict__ out, const float *__restrict__ lse,
                                                        const float *__restrict__ go, int H, int L, float scale,
                                                        float *__restrict__ gk, long gk_bs, long gk_rs,
                                                        float *__restrict__ gv, long gv_bs, long gv_rs) {
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    float *Qs = s_mem, *Gs = s_mem + (size_t)L * kPitch;
    float *s_lse = Gs + (size_t)L * kPitch, *s_D = s_lse + L;
    const int h = blockIdx.y, b = blockIdx.z;
    stage_rows(Qs, q + b * q_bs + h * kHd, q_rs, L);
    // Q is kept SCALED, as the forward and grad_q hold it: (q * scale) . k is then the forward's score bit for bit and
    // exp(s - lse) the forward's probability (scaling k instead moved s by an ulp: p = 1 +- 5e-7 where it is exactly 1).
    // Each thread scales the float4s it staged itself, so no barrier is needed in between.
    for (int i = threadIdx.x; i < L * 8; i += blockDim.x) {
        f32x4_t *p4 = reinterpret_cast<f32x4_t *>(Qs + (i >> 3) * kPitch + (i & 7) * 4);
        *p4 = *p4 * scale;
    }
    stage_rows(Gs, go + (long)b * L * (H * kHd) + h * kHd, (long)H * kHd, L);
    for (int i = threadIdx.x; i < L; i += blockDim.x) s_lse[i] = lse[((long)b * H + h) * L + i];
    __syncthreads();
    for (int i = threadIdx.x; i < L; i += blockDim.x) {             // D_i = dO_i . O_i
        const float *o = out + ((long)b * L + i) * (H * kHd) + h * kHd;
        float orr[kHd];
        load_row32(o, orr);
        s_D[i] = dot32(orr, Gs + i * kPitch);
    }
    __syncthreads();
    const int row = blockIdx.x * kRows + threadIdx.x / kLanes, sub = threadIdx.x % kLanes;
    const bool row_ok = row < L;
    const int rowc = row_ok ? row : L - 1;
    const bool dead = key_mask && key_mask[(long)b * L + rowc];     // a masked key receives no gradient
    float kr[kHd], vr[kHd], ak[kHd], av[kHd];
    load_row32(k + b * k_bs + rowc * k_rs + h * kHd, kr);
    load_row32(v + b * v_bs + rowc * v_rs + h * kHd, vr);
#pragma unroll
    for (int i = 0; i < kHd; ++i) { ak[i] = 0.f; av[i] = 0.f; }
    if (!dead) {
        for (int i = sub; i < L; i += kLanes) {
            const float p = expf(dot32(kr, Qs + i * kPitch) - s_lse[i]);
            const float ds = p * (dot32(vr, Gs + i * kPitch) - s_D[i]);
            axpy32(av, p, Gs + i * kPitch);
            axpy32(ak, ds, Qs + i * kPitch);
        }
    }
    float *pk = gk + b * gk_bs + rowc * gk_rs + h * kHd, *pv = gv + b * gv_bs + rowc * gv_rs + h * kHd;
#pragma unroll
    for (int i = 0; i < kHd; ++i) {
        const float tk = sum8l(ak[i]), tv = sum8l(av[i]);           // (ak sums ds * (q * scale) already)
        if (row_ok && (i >> 2) == sub) {
            pk[i] = tk;
            pv[i] = tv;
        }
    }
}

std::atomic<unsigned long long> g_lds_fwd{0}, g_lds_bq{0}, g_lds_bkv{0};

int mha_check(const void *q, const void *k, const void *v, int B, int H, int L) {
    if (B < 0 || H <= 0 || L < 0) return fail(1, "clipops_mha: bad dimension");
    if (L > CLIPOPS_MHA_MAX_L) return fail(2, "clipops_mha: L exceeds CLIPOPS_MHA_MAX_L");
    if ((long)B * L > 0 && (!q || !k || !v)) return fail(1, "clipops_mha: null pointer");
    return 0;
}
}  // namespace

extern "C" {
int clipops_mha_fwd_f32(const float *q, const float *k, const float *v, long q_bs, long q_rs, long k_bs, long k_rs,
                        long v_bs, long v_rs, const uint8_t *key_mask, int B, int H, int L, float scale, float *out,
                        float *lse, void *stream) {
    int rc = mha_check(q, k, v, B, H, L);
    if (rc) return rc;
    if ((long)B * L == 0) return ok();
    if (!out || !lse) return fail(1, "clipops_mha_fwd_f32: null pointer");
    const size_t lds = (size_t)2 * L * kPitch * sizeof(float);
    if ((rc = allow_lds(reinterpret_cast<const void *>(mha_fwd_kernel), lds, g_lds_fwd))) return rc;
    return launch("mha_fwd_kernel", mha_fwd_kernel, dim3((L + kRows - 1) / kRows, H, B), dim3(256), lds, stream, q, k, v,
                  q_bs, q_rs, k_bs, k_rs, v_bs, v_rs, key_mask, H, L, scale, out, lse);
}

int clipops_mha_bwd_f32(const float *q, const float *k, const float *v, long q_bs, long q_rs, long k_bs, long k_rs,
                        long v_bs, long v_rs, const uint8_t *key_mask, const float *out, const float *lse,
                        const float *grad_out, int B, int H, int L, float scale, float *grad_q, long gq_bs, long gq_rs,
                        float *grad_k, long gk_bs, long gk_rs, float *grad_v, long gv_bs, long gv_rs, void *stream) {
    int rc = mha_check(q, k, v, B, H, L);
    if (rc) return rc;
    if ((long)B * L == 0) return ok();
    if (!out || !lse || !grad_out || !grad_q || !grad_k || !grad_v) return fail(1, "clipops_mha_bwd_f32: null pointer");
    const size_t lds_q = (size_t)2 * L * kPitch * sizeof(float);
    const size_t lds_kv = lds_q + (size_t)2 * L * sizeof(float);
    if ((rc = allow_lds(reinterpret_cast<const void *>(mha_bwd_q_kernel), lds_q, g_lds_bq))) return rc;
    if ((rc = allow_lds(reinterpret_cast<const void *>(mha_bwd_kv_kernel), lds_kv, g_lds_bkv))) return rc;
    const dim3 grid((L + kRows - 1) / kRows, H, B);
    if ((rc = launch("mha_bwd_q_kernel", mha_bwd_q_kernel, grid, dim3(256), lds_q, stream, q, k, v, q_bs, q_rs, k_bs, k_rs,
                     v_bs, v_rs, key_mask, out, lse, grad_out, H, L, scale, grad_q, gq_bs, gq_rs)))
        return rc;
    return launch("mha_bwd_kv_kernel", mha_bwd_kv_kernel, grid, dim3(256), lds_kv, stream, q, k, v, q_bs, q_rs, k_bs, k_rs,
                  v_bs, v_rs, key_mask, out, lse, grad_out, H, L, scale, grad_k, gk_bs, gk_rs, grad_v, gv_bs, gv_rs);
}
}  // extern "C"
