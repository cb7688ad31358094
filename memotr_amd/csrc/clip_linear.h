// clip_linear.h -- the query-sized linears on fp32 MFMA: forward and one-launch backward, operands straight from global
// memory (the direct form) or staged through LDS (the shipped form), same bits.
// Included by clip_ops.hip after clip_common.h.
#pragma once

namespace {
// ---------------------------------------------------------------------------------------------------------------
// Backward of a query-sized Linear (a few hundred rows) in ONE launch: grad_x = G' W, grad_w = G'^T X, grad_b = colsum G',
// G' = grad_y (masked by y > 0 when the forward fused a ReLU).  torch issues [threshold_backward,] two GEMMs and a
// reduction -- four dependent launches of ~5 us each inside the decoder's hipGraphs for ~0.1 GFLOP; the three results
// depend on the same inputs only, so they are tiles of one grid here.
//   * one 32 x 32 output tile per workgroup, fp32 MFMA 32x32x2 (bit-for-bit a k-ordered fmaf chain), the contraction
//     split over the four wavefronts and added up through LDS;
//   * lane l feeds A[i = l & 31][k] and B[k][j = l & 31] for k = 8 c + 4 (l >> 5) + {0..3}: four MFMAs per 8 k;
//   * operands straight from global memory (the whole problem sits in L2), zero-filled past the edges.
// ---------------------------------------------------------------------------------------------------------------
typedef float lb_f32x16 __attribute__((ext_vector_type(16)));

// One workgroup's tile.  GX: C = G' W (A rows are rows of G: one 16-byte load per lane and chunk when OUT % 4 == 0);
// else C = G'^T X (A columns are rows of G: coalesced dwords).  LB_U chunks of 8 k are requested before the first MFMA
// of the group -- without that every chunk waits a memory round trip and the kernel takes 40 us at K = 1024.
#ifndef MSDA_LB_U
#define MSDA_LB_U 4
#endif
constexpr int LB_U = MSDA_LB_U;

template <bool GX, bool RELU>
__device__ __forceinline__ void linear_bwd_tile(const float *__restrict__ g, const float *__restrict__ y,
                                                const float *__restrict__ Bp, int M, int N, int K, int OUT, int i0, int j0,
                                                float *__restrict__ C, float *__restrict__ gb, float (*s_c)[16][64],
                                                float (*s_b)[32]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = i0 + (lane & 31), j = j0 + (lane & 31), kq = (lane >> 5) * 4;
    const bool iok = i < M, jok = j < N;
    const int chunks = (K + 7) / 8, per = (chunks + 3) / 4;
    const int c_lo = wave * per, c_hi = (c_lo + per) < chunks ? (c_lo + per) : chunks;
    const bool vec = GX && (OUT % 4 == 0);
    lb_f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    for (int c = c_lo; c < c_hi; c += LB_U) {
        float a[LB_U][4], b[LB_U][4], m[LB_U][4];
#pragma unroll
        for (int u = 0; u < LB_U; ++u) {
            const int k0 = (c + u) * 8 + kq;
            const bool cok = c + u < c_hi;
            if (vec) {
                float4 av = {0.f, 0.f, 0.f, 0.f}, mv = {1.f, 1.f, 1.f, 1.f};
                if (cok && iok && k0 < K) {          // (K = OUT is a multiple of 4 and k0 one too: all four or none)
                    av = *reinterpret_cast<const float4 *>(g + (long)i * OUT + k0);
                    if (RELU) mv = *reinterpret_cast<const float4 *>(y + (long)i * OUT + k0);
                }
                a[u][0] = av.x; a[u][1] = av.y; a[u][2] = av.z; a[u][3] = av.w;
                m[u][0] = mv.x; m[u][1] = mv.y; m[u][2] = mv.z; m[u][3] = mv.w;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = k0 + q;
                const bool kok = cok && k < K;
                if (!vec) {
                    const long idx = GX ? (long)i * OUT + k : (long)k * OUT + i;
                    a[u][q] = (iok && kok) ? g[idx] : 0.f;
                    m[u][q] = (RELU && iok && kok) ? y[idx] : 1.f;
                }
                b[u][q] = (jok && kok) ? Bp[(long)k * N + j] : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < LB_U; ++u) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float av = RELU ? (m[u][q] <= 0.f ? 0.f : a[u][q]) : a[u][q];      // (y <= 0 ? 0 : g -- aten's threshold_backward: a NaN activation passes g)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[u][q], acc, 0, 0, 0);
                bsum += av;
            }
        }
    }
    // add the four partial tiles (and bias sums) up; wavefront v finishes accumulator registers 4v .. 4v + 3
#pragma unroll
    for (int r = 0; r < 16; ++r) s_c[wave][r][lane] = acc[r];
    bsum += __shfl_xor(bsum, 32, 64);
    if (lane < 32) s_b[wave][lane] = bsum;
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int r = wave * 4 + rr;
        const float v = (s_c[0][r][lane] + s_c[1][r][lane]) + (s_c[2][r][lane] + s_c[3][r][lane]);
        const int row = i0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row < M && jok) C[(long)row * N + j] = v;
    }
    if (!GX && gb != nullptr && j0 == 0 && wave == 0 && lane < 32 && i0 + lane < M)
        gb[i0 + lane] = (s_b[0][lane] + s_b[1][lane]) + (s_b[2][lane] + s_b[3][lane]);
}

template <bool RELU>
__global__ __launch_bounds__(256) void linear_bwd_kernel(const float *__restrict__ g, const float *__restrict__ y,
                                                         const float *__restrict__ x, const float *__restrict__ w,
                                                         int R, int IN, int OUT, float *__restrict__ gx,
                                                         float *__restrict__ gw, float *__restrict__ gb, int n_gx,
                                                         int gx_tj, int gw_tj) {
    __shared__ float s_c[4][16][64];
    __shared__ float s_b[4][32];
    const int tile = blockIdx.x;
    // C (M x N) = A (M x K) B (K x N):   gx: A = G' (R x OUT), B = W (OUT x IN)     gw: A = G'^T (OUT x R), B = X (R x IN)
    if (tile < n_gx) {
        linear_bwd_tile<true, RELU>(g, y, w, R, IN, OUT, OUT, (tile / gx_tj) * 32, (tile % gx_tj) * 32, gx, nullptr, s_c, s_b);
    } else {
        const int t = tile - n_gx;
        linear_bwd_tile<false, RELU>(g, y, x, OUT, IN, R, OUT, (t / gw_tj) * 32, (t % gw_tj) * 32, gw, gb, s_c, s_b);
    }
}

// Forward of the same linears: y = [relu](x W^T + b), one 32 x 32 tile per workgroup.  Both operands are contiguous
// along the contraction (x rows, W rows), so a lane's four k of a chunk are ONE 16-byte load each.
template <bool RELU>
__global__ __launch_bounds__(256) void linear_fwd_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                         const float *__restrict__ bias, int R, int IN, int OUT,
                                                         float *__restrict__ yout, int tj) {
    __shared__ float s_c[4][16][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = (blockIdx.x / tj) * 32, j0 = (blockIdx.x % tj) * 32;
    const int i = i0 + (lane & 31), j = j0 + (lane & 31), kq = (lane >> 5) * 4;
    const bool iok = i < R, jok = j < OUT;
    const int chunks = (IN + 7) / 8, per = (chunks + 3) / 4;
    const int c_lo = wave * per, c_hi = (c_lo + per) < chunks ? (c_lo + per) : chunks;
    lb_f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int c = c_lo; c < c_hi; c += LB_U) {
        float4 a[LB_U], b[LB_U];
#pragma unroll
        for (int u = 0; u < LB_U; ++u) {
            const int k0 = (c + u) * 8 + kq;
            const bool kok = c + u < c_hi && k0 < IN;          // (IN is a multiple of 4: the launcher checks)
            a[u] = (iok && kok) ? *reinterpret_cast<const float4 *>(x + (long)i * IN + k0) : float4{0.f, 0.f, 0.f, 0.f};
            b[u] = (jok && kok) ? *reinterpret_cast<const float4 *>(w + (long)j * IN + k0) : float4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < LB_U; ++u) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].x, b[u].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].y, b[u].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].z, b[u].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].w, b[u].w, acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) s_c[wave][r][lane] = acc[r];
    __syncthreads();
    const float bj = (bias != nullptr && jok) ? bias[j] : 0.f;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int r = wave * 4 + rr;
        float v = ((s_c[0][r][lane] + s_c[1][r][lane]) + (s_c[2][r][lane] + s_c[3][r][lane])) + bj;
        if (RELU) v = v < 0.f ? 0.f : v;
        const int row = i0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row < R && jok) yout[(long)row * OUT + j] = v;
    }
}

// ---- the same tiles with their operands staged through LDS (the shipped form; MEMOTR_LINEAR_STAGED=0 launches the
//      kernels above) ----
// The arithmetic is the kernels' above, MFMA for MFMA: the same lane -> (i, j, k) mapping, the same quarter of the
// chunks per wavefront in the same k order, the same reduction.  Only where an operand comes from differs: the workgroup
// first brings the A and B tile of the whole contraction into LDS -- every thread issues its 16-byte loads of both
// operands (and of the ReLU mask, applied on the way in) back to back, so the tile costs ONE memory round trip where the
// direct form pays one per LB_U chunks with four dwords per lane and chunk for every operand that is not contiguous along k.
// Two LDS images, both read without bank conflicts by lanes l & 31 along i / j with the half-waves 4 k apart:
//   ROW  the operand is contiguous along k (G for grad_x; x and W forward): [32 rows][pitch 32 S + 4]; a lane's four k
//        are one ds_read_b128 (pitch / 4 is odd: the 16 lanes of a b128 group hit 16 distinct bank quads);
//   COL  the operand is contiguous along i / j (W and X backward, G for grad_w): [k][32]; four ds_read_b32.
// LDS holds LS_S chunks of 8 k per wavefront; a longer contraction goes in K blocks (OUT > 512 or rows > 512 backward,
// IN > 512 forward), block b holding chunks b S .. b S + S - 1 of EVERY wavefront's quarter.  A launch asks for exactly
// its largest tile's images (66 KB at K = 256, 80 KB for the weight-gradient tiles of 320 rows: two workgroups per CU);
// the 16.5 KB of the reduction lie over the images once every wavefront is done with them.
// `VEC`: every operand base is 16-byte aligned and every pitch a multiple of 4; otherwise the same pieces come in as
// dwords.  Pieces past an edge are zero (their loads are redirected to the operand's first element and discarded, so
// that the loads stay unconditional and issue together).
constexpr int LS_S = 16;
constexpr int LS_RED_FLOATS = 4 * 16 * 64 + 4 * 32;          // s_c and s_b of the reduction, over the images once they are spent

__host__ __device__ constexpr int ls_pitch(int S) { return 32 * S + 4; }
// chunks of 8 k per wavefront that LDS holds of a contraction of length K, and the floats of an image of that many
__host__ __device__ constexpr int ls_chunks(int K) { return (((K + 7) / 8 + 3) / 4) < LS_S ? (((K + 7) / 8 + 3) / 4) : LS_S; }
__host__ __device__ constexpr int ls_image(bool row, int S) { return row ? 32 * ls_pitch(S) : 8 * 4 * S * 32; }
// dynamic LDS of a launch whose tiles contract over K with these images (the reduction re-uses the images' bytes)
constexpr size_t ls_bytes(bool a_row, bool b_row, int K) {
    const int n = ls_image(a_row, ls_chunks(K)) + ls_image(b_row, ls_chunks(K));
    return sizeof(float) * (size_t)(n > LS_RED_FLOATS ? n : LS_RED_FLOATS);
}

// piece (w, it) of a thread for K block b: `off` where its four floats start in the operand, `n` how many of them are
// real (0 .. 4), `lds` where they go in the image (-1: no such slot, or one past the contraction's last chunk, which no
// MFMA reads).  lim / t0: rows (ROW) or columns (COL) of the operand and the tile's first one.
template <bool ROW>
__device__ __forceinline__ void ls_piece(int w, int it, int b, int S, int per, int K, int lim, int t0, long ld, long &off,
                                         int &n, int &lds) {
    const int g8 = threadIdx.x >> 3, f = threadIdx.x & 7;
    int left;
    if (ROW) {          // 8 threads per row: 8 consecutive 16-byte pieces = 4 chunks of wavefront w's quarter
        const int fi = f + 8 * it, t = fi >> 1, cw = b * S + t;
        const int k0 = 8 * (w * per + cw) + 4 * (fi & 1);
        left = (fi < 2 * S && cw < per && t0 + g8 < lim) ? K - k0 : 0;
        off = (long)(t0 + g8) * ld + k0;
        lds = (fi < 2 * S && cw < per && 8 * (w * per + cw) < K) ? g8 * ls_pitch(S) + 8 * (w * S + t) + 4 * (fi & 1) : -1;
    } else {            // 8 threads per k: the 32 columns of the tile
        const int kr = g8 + 32 * it, cw = b * S + (kr >> 3);
        const int k = 8 * (w * per + b * S) + kr;
        left = (kr < 8 * S && cw < per && k < K) ? lim - (t0 + 4 * f) : 0;
        off = (long)k * ld + t0 + 4 * f;
        lds = (kr < 8 * S && cw < per && 8 * (w * per + cw) < K) ? (8 * w * S + kr) * 32 + 4 * f : -1;
    }
    n = left < 0 ? 0 : (left > 4 ? 4 : left);
}

template <bool VEC>
__device__ __forceinline__ float4 ls_load4(const float *__restrict__ src, long off, int n) {
    float4 v;
    if (VEC) {          // (n is 0 or 4: pitches, K and the tile origins are multiples of 4)
        v = *reinterpret_cast<const float4 *>(src + (n > 0 ? off : 0));
        if (n <= 0) v = float4{0.f, 0.f, 0.f, 0.f};
    } else {
        v.x = src[n > 0 ? off : 0];
        v.y = src[n > 1 ? off + 1 : 0];
        v.z = src[n > 2 ? off + 2 : 0];
        v.w = src[n > 3 ? off + 3 : 0];
        v.x = n > 0 ? v.x : 0.f; v.y = n > 1 ? v.y : 0.f; v.z = n > 2 ? v.z : 0.f; v.w = n > 3 ? v.w : 0.f;
    }
    return v;
}

// K block b of both operands into LDS.  A is masked by y on the way in when RELU: y <= 0 ? 0 : g, aten's
// threshold_backward (a NaN activation passes g); zero-filled pieces stay zero under it.
template <bool AROW, bool BROW, bool RELU, bool VEC>
__device__ __forceinline__ void ls_stage(const float *__restrict__ a_src, const float *__restrict__ y_src, long a_ld,
                                         int a_lim, int a_t0, const float *__restrict__ b_src, long b_ld, int b_lim,
                                         int b_t0, int K, int per, int S, int b, float *__restrict__ As,
                                         float *__restrict__ Bs) {
    const int n_it = (S + 3) / 4;
    for (int it0 = 0; it0 < n_it; it0 += 2) {
        float4 va[2][4], vy[2][4], vb[2][4];
        int la[2][4], lb[2][4];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                long off;
                int n;
                ls_piece<AROW>(w, it0 + u, b, S, per, K, a_lim, a_t0, a_ld, off, n, la[u][w]);
                va[u][w] = ls_load4<VEC>(a_src, off, n);
                if (RELU) vy[u][w] = ls_load4<VEC>(y_src, off, n);
                ls_piece<BROW>(w, it0 + u, b, S, per, K, b_lim, b_t0, b_ld, off, n, lb[u][w]);
                vb[u][w] = ls_load4<VEC>(b_src, off, n);
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                float4 a = va[u][w];
                if (RELU) {
                    const float4 m = vy[u][w];
                    a.x = m.x <= 0.f ? 0.f : a.x; a.y = m.y <= 0.f ? 0.f : a.y;
                    a.z = m.z <= 0.f ? 0.f : a.z; a.w = m.w <= 0.f ? 0.f : a.w;
                }
                if (la[u][w] >= 0) *reinterpret_cast<float4 *>(As + la[u][w]) = a;
                if (lb[u][w] >= 0) *reinterpret_cast<float4 *>(Bs + lb[u][w]) = vb[u][w];
            }
        }
    }
}

// a wavefront's n_t chunks of the staged block: per chunk the four MFMAs (and bias-sum adds) of the direct form
template <bool AROW, bool BROW>
__device__ __forceinline__ void ls_mfma(const float *__restrict__ As, const float *__restrict__ Bs, int S, int n_t,
                                        lb_f32x16 &acc, float &bsum) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l = lane & 31, kq = (lane >> 5) * 4;
    n_t = __builtin_amdgcn_readfirstlane(n_t);          // (uniform: a scalar trip count)
    const float *ap = AROW ? As + l * ls_pitch(S) + 8 * wave * S + kq : As + (8 * wave * S + kq) * 32 + l;
    const float *bp = BROW ? Bs + l * ls_pitch(S) + 8 * wave * S + kq : Bs + (8 * wave * S + kq) * 32 + l;
    auto read = [&](int t, float *a, float *b) {
        if (AROW) {
            const float4 v = *reinterpret_cast<const float4 *>(ap + 8 * t);
            a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) a[q] = ap[(8 * t + q) * 32];
        }
        if (BROW) {
            const float4 v = *reinterpret_cast<const float4 *>(bp + 8 * t);
            b[0] = v.x; b[1] = v.y; b[2] = v.z; b[3] = v.w;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) b[q] = bp[(8 * t + q) * 32];
        }
    };
    auto mfma4 = [&](const float *a, const float *b) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], b[q], acc, 0, 0, 0);
            bsum += a[q];
        }
    };
    if (n_t <= 0) return;
    float a0[4], b0[4], a1[4], b1[4];
    read(0, a0, b0);
    int t = 0;
    for (; t + 2 <= n_t; t += 2) {          // the next chunk's LDS reads are in flight under this chunk's MFMAs
        read(t + 1, a1, b1);
        mfma4(a0, b0);
        read(t + 2 < n_t ? t + 2 : t + 1, a0, b0);
        mfma4(a1, b1);
    }
    if (t < n_t) mfma4(a0, b0);
}

// the whole contraction of one tile: C (32 x 32 at i0, j0) += A B over K, this wavefront's quarter in `acc`
template <bool AROW, bool BROW, bool RELU, bool VEC>
__device__ __forceinline__ void ls_contract(const float *__restrict__ a_src, const float *__restrict__ y_src, long a_ld,
                                            int a_lim, int a_t0, const float *__restrict__ b_src, long b_ld, int b_lim,
                                            int b_t0, int K, float *__restrict__ smem, lb_f32x16 &acc, float &bsum) {
    const int wave = threadIdx.x >> 6;
    const int chunks = (K + 7) / 8, per = (chunks + 3) / 4;
    const int mine = (chunks - wave * per) < per ? (chunks - wave * per) : per;          // c_hi - c_lo (may be <= 0)
    const int S = ls_chunks(K);
    float *As = smem, *Bs = As + ls_image(AROW, S);
    for (int b = 0; b * S < per; ++b) {
        if (b) __syncthreads();                    // every wavefront is done with the block before
        ls_stage<AROW, BROW, RELU, VEC>(a_src, y_src, a_ld, a_lim, a_t0, b_src, b_ld, b_lim, b_t0, K, per, S, b, As, Bs);
        __syncthreads();
        const int n_t = (mine - b * S) < S ? (mine - b * S) : S;
        ls_mfma<AROW, BROW>(As, Bs, S, n_t, acc, bsum);
    }
    __syncthreads();          // the caller's reduction buffers lie over the images
}

template <bool GX, bool RELU, bool VEC>
__device__ __forceinline__ void linear_bwd_tile_staged(const float *__restrict__ g, const float *__restrict__ y,
                                                       const float *__restrict__ Bp, int M, int N, int K, int OUT, int i0,
                                                       int j0, float *__restrict__ C, float *__restrict__ gb,
                                                       float *__restrict__ smem) {
    float(*s_c)[16][64] = reinterpret_cast<float(*)[16][64]>(smem);
    float(*s_b)[32] = reinterpret_cast<float(*)[32]>(smem + 4 * 16 * 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = j0 + (lane & 31);
    const bool jok = j < N;
    lb_f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    // GX: A rows are rows of G (ROW image); else A columns are rows of G (COL image).  B rows are rows of W / X.
    ls_contract<GX, false, RELU, VEC>(g, y, OUT, M, i0, Bp, N, N, j0, K, smem, acc, bsum);
    // add the four partial tiles (and bias sums) up, as linear_bwd_tile does
#pragma unroll
    for (int r = 0; r < 16; ++r) s_c[wave][r][lane] = acc[r];
    bsum += __shfl_xor(bsum, 32, 64);
    if (lane < 32) s_b[wave][lane] = bsum;
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int r = wave * 4 + rr;
        const float v = (s_c[0][r][lane] + s_c[1][r][lane]) + (s_c[2][r][lane] + s_c[3][r][lane]);
        const int row = i0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row < M && jok) C[(long)row * N + j] = v;
    }
    if (!GX && gb != nullptr && j0 == 0 && wave == 0 && lane < 32 && i0 + lane < M)
        gb[i0 + lane] = (s_b[0][lane] + s_b[1][lane]) + (s_b[2][lane] + s_b[3][lane]);
}

template <bool RELU, bool VEC>
__global__ __launch_bounds__(256) void linear_bwd_staged_kernel(const float *__restrict__ g, const float *__restrict__ y,
                                                                const float *__restrict__ x, const float *__restrict__ w,
                                                                int R, int IN, int OUT, float *__restrict__ gx,
                                                                float *__restrict__ gw, float *__restrict__ gb, int n_gx,
                                                                int gx_tj, int gw_tj) {
    extern __shared__ __attribute__((aligned(16))) float s_linear[];
    const int tile = blockIdx.x;
    if (tile < n_gx) {
        linear_bwd_tile_staged<true, RELU, VEC>(g, y, w, R, IN, OUT, OUT, (tile / gx_tj) * 32, (tile % gx_tj) * 32, gx,
                                                nullptr, s_linear);
    } else {
        const int t = tile - n_gx;
        linear_bwd_tile_staged<false, RELU, VEC>(g, y, x, OUT, IN, R, OUT, (t / gw_tj) * 32, (t % gw_tj) * 32, gw, gb,
                                                 s_linear);
    }
}

template <bool RELU, bool VEC>
__global__ __launch_bounds__(256) void linear_fwd_staged_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                                const float *__restrict__ bias, int R, int IN, int OUT,
                                                                float *__restrict__ yout, int tj) {
    extern __shared__ __attribute__((aligned(16))) float s_linear[];
    float(*s_c)[16][64] = reinterpret_cast<float(*)[16][64]>(s_linear);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = (blockIdx.x / tj) * 32, j0 = (blockIdx.x % tj) * 32;
    const int j = j0 + (lane & 31);
    const bool jok = j < OUT;
    lb_f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float unused = 0.f;
    ls_contract<true, true, false, VEC>(x, nullptr, IN, R, i0, w, IN, OUT, j0, IN, s_linear, acc, unused);
#pragma unroll
    for (int r = 0; r < 16; ++r) s_c[wave][r][lane] = acc[r];
    __syncthreads();
    const float bj = (bias != nullptr && jok) ? bias[j] : 0.f;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int r = wave * 4 + rr;
        float v = ((s_c[0][r][lane] + s_c[1][r][lane]) + (s_c[2][r][lane] + s_c[3][r][lane])) + bj;
        if (RELU) v = v < 0.f ? 0.f : v;
        const int row = i0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row < R && jok) yout[(long)row * OUT + j] = v;
    }
}

// MEMOTR_LINEAR_STAGED=0: the direct-from-global kernels (the A/B switch of both entry points, read at every launch)
bool linear_staged() {
    const char *e = getenv("MEMOTR_LINEAR_STAGED");
    return !(e && e[0] == '0' && e[1] == 0);
}
}  // namespace

extern "C" {
int clipops_linear_bwd_f32(const float *grad_y, const float *y_relu, const float *x, const float *w, int rows,
                           int in_features, int out_features, float *grad_x, float *grad_w, float *grad_b,
                           void *stream) {
    if (rows < 0 || in_features <= 0 || out_features <= 0) return fail(1, "clipops_linear_bwd_f32: bad dimension");
    if (!grad_y || !x || !w) return fail(1, "clipops_linear_bwd_f32: null pointer");
    if (grad_b && !grad_w) return fail(1, "clipops_linear_bwd_f32: grad_b is computed with grad_w");
    const int gx_ti = (rows + 31) / 32, gx_tj = (in_features + 31) / 32;
    const int gw_ti = (out_features + 31) / 32, gw_tj = gx_tj;
    const int n_gx = grad_x ? gx_ti * gx_tj : 0, n_gw = grad_w ? gw_ti * gw_tj : 0;
    if (n_gx + n_gw == 0) return ok();
    if (rows == 0) {          // nothing to contract over: the weight and bias gradients are zero
        if (grad_w && hipMemsetAsync(grad_w, 0, sizeof(float) * (size_t)out_features * in_features, (hipStream_t)stream) != hipSuccess)
            return fail(3, "clipops_linear_bwd_f32: memset failed");
        if (grad_b && hipMemsetAsync(grad_b, 0, sizeof(float) * (size_t)out_features, (hipStream_t)stream) != hipSuccess)
            return fail(3, "clipops_linear_bwd_f32: memset failed");
        return ok();
    }
    const dim3 grid(n_gx + n_gw);
    if (linear_staged()) {
        static std::atomic<unsigned long long> done[4];
        const size_t lds = std::max(grad_x ? ls_bytes(true, false, out_features) : 0, grad_w ? ls_bytes(false, false, rows) : 0);
        const bool vec = in_features % 4 == 0 && out_features % 4 == 0 && aligned16(grad_y) && aligned16(x) &&
                         aligned16(w) && (!y_relu || aligned16(y_relu));
        const int which = (y_relu ? 2 : 0) + (vec ? 1 : 0);
        auto kernel = which == 3 ? linear_bwd_staged_kernel<true, true> : which == 2 ? linear_bwd_staged_kernel<true, false>
                      : which == 1 ? linear_bwd_staged_kernel<false, true> : linear_bwd_staged_kernel<false, false>;
        int rc;
        if ((rc = allow_lds(reinterpret_cast<const void *>(kernel), lds, done[which]))) return rc;
        return launch("linear_bwd_staged_kernel", kernel, grid, dim3(256), lds, stream, grad_y, y_relu, x, w, rows,
                      in_features, out_features, grad_x, grad_w, grad_b, n_gx, gx_tj, gw_tj);
    }
    return launch("linear_bwd_kernel", y_relu ? linear_bwd_kernel<true> : linear_bwd_kernel<false>, grid, dim3(256), 0,
                  stream, grad_y, y_relu, x, w, rows, in_features, out_features, grad_x, grad_w, grad_b, n_gx, gx_tj,
                  gw_tj);
}

int clipops_linear_fwd_f32(const float *x, const float *w, const float *bias, int rows, int in_features,
                           int out_features, int relu, float *y, void *stream) {
    if (rows < 0 || in_features <= 0 || out_features <= 0) return fail(1, "clipops_linear_fwd_f32: bad dimension");
    if (in_features % 4) return fail(2, "clipops_linear_fwd_f32: in_features must be a multiple of 4");
    if (rows == 0) return ok();
    if (!x || !w || !y) return fail(1, "clipops_linear_fwd_f32: null pointer");
    const int ti = (rows + 31) / 32, tj = (out_features + 31) / 32;
    if (linear_staged()) {
        static std::atomic<unsigned long long> done[4];
        const size_t lds = ls_bytes(true, true, in_features);
        const bool vec = aligned16(x) && aligned16(w);
        const int which = (relu ? 2 : 0) + (vec ? 1 : 0);
        auto kernel = which == 3 ? linear_fwd_staged_kernel<true, true> : which == 2 ? linear_fwd_staged_kernel<true, false>
                      : which == 1 ? linear_fwd_staged_kernel<false, true> : linear_fwd_staged_kernel<false, false>;
        int rc;
        if ((rc = allow_lds(reinterpret_cast<const void *>(kernel), lds, done[which]))) return rc;
        return launch("linear_fwd_staged_kernel", kernel, dim3(ti * tj), dim3(256), lds, stream, x, w, bias, rows,
                      in_features, out_features, y, tj);
    }
    return launch("linear_fwd_kernel", relu ? linear_fwd_kernel<true> : linear_fwd_kernel<false>, dim3(ti * tj), dim3(256),
                  0, stream, x, w, bias, rows, in_features, out_features, y, tj);
}
}  // extern "C"
