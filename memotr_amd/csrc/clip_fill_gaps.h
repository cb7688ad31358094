// clip_fill_gaps.h -- gap filling and short-track removal on a device result table, five launches in stream order.
// Included by clip_ops.hip after clip_common.h and clip_tracks.h (the counters' capacity rule).
#pragma once

namespace {
// ---- gap filling and short-track removal on a result table (include/clip_ops_hip.h: clipops_fill_gaps_f32) ----
// Workspace, int32: cell[n_seq][n_ids][n_frames] | right[the same] | offs[n_seq][n_frames].
//   cell   -1 empty; v >= 0 the table row that sits there; v <= -2 a filled cell whose left neighbour is row -(v + 2)
//   right  pass 1 of the track kernel: the next occupied frame at or after the cell; of a filled cell afterwards: the
//          table row of its right neighbour
//   offs   the surviving cells of a (sequence, frame), then the output row its first survivor goes to
// Five launches in stream order: clear, scatter, one workgroup per track, count + scan over (sequence, frame), write.
// Integer atomics only (who owns a cell, the status bits): a table without duplicates gives the same bits every time.
constexpr int FG_THREADS = 1024, FG_WAVES = FG_THREADS / 64, FG_NONE = 0x7fffffff;

__global__ __launch_bounds__(256) void fg_clear_kernel(int32_t *__restrict__ cell, long cells) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < cells; i += (long)gridDim.x * 256) cell[i] = -1;
}

__global__ __launch_bounds__(256) void fg_scatter_kernel(const int64_t *__restrict__ rows_i,
                                                         const int32_t *__restrict__ counters, int n, int W, int n_seq,
                                                         int n_ids, int n_frames, int32_t *__restrict__ cell,
                                                         int32_t *__restrict__ status) {
    const int c0 = counters[0], stored = c0 < 0 ? 0 : (c0 < n ? c0 : n);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < stored; i += (long)gridDim.x * 256) {
        const int64_t *r = rows_i + i * W;
        const int64_t seq = W == 4 ? r[0] : 0, frame = r[W - 3], id = r[W - 2];
        int bad = 0;
        if (seq < 0 || seq >= n_seq) bad |= CLIPOPS_FG_SEQUENCE;
        if (id < 0 || id >= n_ids) bad |= CLIPOPS_FG_ID;
        if (frame < 0 || frame >= n_frames) bad |= CLIPOPS_FG_FRAME;
        if (bad) {
            atomicOr(status, bad);
            continue;
        }
        if (atomicCAS(cell + ((seq * n_ids + id) * n_frames + frame), -1, (int)i) != -1)
            atomicOr(status, CLIPOPS_FG_DUPLICATE);
    }
}

// One workgroup per track, frames in chunks of 1024, one thread a frame.  Pass 1 walks the chunks from the last to the
// first: a suffix minimum of the occupied frames (shuffles inside a wavefront, wave results and the carry of the later
// chunks through LDS) leaves every cell's next occupied frame in `right`, and the ballots count the track's rows.  Pass 2
// walks forward with the prefix maximum: an empty cell with an occupied frame on either side and at most max_gap missing
// frames between them becomes a filled cell.  A thread writes only its own cell, and only empty cells change while the
// occupied ones are read by others; a track shorter than min_length is emptied instead.
__global__ __launch_bounds__(FG_THREADS) void fg_track_kernel(int32_t *__restrict__ cell, int32_t *__restrict__ right,
                                                              int n_frames, int max_gap, int min_length) {
    __shared__ int wave_val[FG_WAVES], wave_cnt[FG_WAVES];
    int32_t *A = cell + (long)blockIdx.x * n_frames, *B = right + (long)blockIdx.x * n_frames;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_chunks = (int)(((long)n_frames + FG_THREADS - 1) / FG_THREADS);
    int carry = FG_NONE, length = 0;
    for (int c = n_chunks - 1; c >= 0; --c) {
        const long f = (long)c * FG_THREADS + tid;
        const bool occ = f < n_frames && A[f] >= 0;
        int v = occ ? (int)f : FG_NONE;
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_down(v, d);
            if (lane + d < 64) v = min(v, o);
        }
        const unsigned long long m = __ballot(occ);
        if (lane == 0) wave_val[wave] = v, wave_cnt[wave] = __popcll(m);
        __syncthreads();
        int later = carry, all = carry;
        for (int w = 0; w < FG_WAVES; ++w) {
            const int t = wave_val[w];
            if (w > wave) later = min(later, t);
            all = min(all, t);
            length += wave_cnt[w];
        }
        if (f < n_frames) B[f] = min(v, later);
        carry = all;
        __syncthreads();                            // wave_val and wave_cnt are written again by the next chunk
    }
    const bool keep = length >= min_length;
    carry = -1;
    for (int c = 0; c < n_chunks; ++c) {
        const long f = (long)c * FG_THREADS + tid;
        const int a = f < n_frames ? A[f] : -1;
        int v = a >= 0 ? (int)f : -1;
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(v, d);
            if (lane >= d) v = max(v, o);
        }
        if (lane == 63) wave_val[wave] = v;
        __syncthreads();
        int earlier = carry, all = carry;
        for (int w = 0; w < FG_WAVES; ++w) {
            const int t = wave_val[w];
            if (w < wave) earlier = max(earlier, t);
            all = max(all, t);
        }
        if (f < n_frames) {
            if (!keep) {
                if (a >= 0) A[f] = -1;
            } else if (a < 0) {
                const int f0 = max(v, earlier), f1 = B[f];
                if (f0 >= 0 && f1 != FG_NONE && f1 - f0 - 1 <= max_gap) {
                    A[f] = -(A[f0] + 2);
                    B[f] = A[f1];
                }
            }
        }
        carry = all;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void fg_count_kernel(const int32_t *__restrict__ cell, long n_sf, int n_ids, int n_frames,
                                                       int32_t *__restrict__ offs) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_sf) return;
    const int32_t *p = cell + (i / n_frames) * n_ids * n_frames + i % n_frames;
    int c = 0;
    for (int id = 0; id < n_ids; ++id) c += p[(long)id * n_frames] != -1;
    offs[i] = c;
}

// offs[i] <- counters[0] + the survivors of all (sequence, frame) before i (clamped to 2^31 - 1: no row lands there), and
// the counters by clipops_result_rows_f32's capacity rule.  One workgroup: an inclusive scan by shuffles inside a
// wavefront, wave totals through LDS, a running base across chunks of 1024.
__global__ __launch_bounds__(FG_THREADS) void fg_scan_kernel(int32_t *__restrict__ offs, long n_sf,
                                                             int32_t *__restrict__ counters, int capacity) {
    __shared__ int wave_val[FG_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int stored0 = counters[0], dropped0 = counters[1];
    const long start = stored0 < 0 ? 0 : stored0;
    long base = 0;
    for (long i0 = 0; i0 < n_sf; i0 += FG_THREADS) {
        const long i = i0 + tid;
        const int mine = i < n_sf ? offs[i] : 0;
        int v = mine;
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(v, d);
            if (lane >= d) v += o;
        }
        if (lane == 63) wave_val[wave] = v;
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < FG_WAVES; ++w) {
            const int t = wave_val[w];
            before += w < wave ? t : 0;
            total += t;
        }
        if (i < n_sf) {
            const long at = start + base + before + v - mine;
            offs[i] = (int)(at < FG_NONE ? at : FG_NONE);
        }
        base += total;
        __syncthreads();
    }
    __syncthreads();                                // every thread has read the counters
    if (tid == 0) store_counters(counters, stored0, dropped0, base, capacity);
}

// One workgroup per (sequence, frame): the ids in chunks of 256, ranked by ballots (bank_ranks); a survivor's row is its
// source row as it stands, or left + (right - left) * (k / (m + 1)) of the five float columns, every operation rounded
// once, with the id and the label of the left row.
__global__ __launch_bounds__(256) void fg_write_kernel(const float *__restrict__ rows_f, const int64_t *__restrict__ rows_i,
                                                       int W, const int32_t *__restrict__ cell,
                                                       const int32_t *__restrict__ right, const int32_t *__restrict__ offs,
                                                       int n_ids, int n_frames, float *__restrict__ out_f,
                                                       int64_t *__restrict__ out_i, int capacity) {
#pragma clang fp contract(off)
    __shared__ int wave_total[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long sf = blockIdx.x, seq = sf / n_frames, frame = sf % n_frames;
    const long first = seq * n_ids * n_frames + frame, start = offs[sf];
    int base = 0;
    for (int id0 = 0; id0 < n_ids; id0 += 256) {    // (n_ids is uniform: every thread makes every trip)
        const int id = id0 + (int)threadIdx.x;
        const long c = first + (long)id * n_frames;
        const int v = id < n_ids ? cell[c] : -1;
        int before, total;
        bank_ranks<4>(v != -1, lane, wave, wave_total, before, total);
        const long pos = start + base + before;
        if (v != -1 && pos < capacity) {
            float *of = out_f + pos * 5;
            int64_t *oi = out_i + pos * W;
            if (v >= 0) {
                for (int j = 0; j < 5; ++j) of[j] = rows_f[(long)v * 5 + j];
                for (int j = 0; j < W; ++j) oi[j] = rows_i[(long)v * W + j];
            } else {
                const long l = -(v + 2), r = right[c];
                const int64_t *li = rows_i + l * W, *ri = rows_i + r * W;
                const int64_t f0 = li[W - 3], f1 = ri[W - 3];
                const float t = (float)(int)(frame - f0) / (float)(int)(f1 - f0);
                for (int j = 0; j < 5; ++j) {       // (contract(off): the product rounds before the sum)
                    const float a = rows_f[l * 5 + j], b = rows_f[r * 5 + j];
                    of[j] = a + (b - a) * t;
                }
                if (W == 4) oi[0] = seq;
                oi[W - 3] = frame, oi[W - 2] = li[W - 2], oi[W - 1] = li[W - 1];
            }
        }
        base += total;
        __syncthreads();                            // wave_total is written again by the next chunk
    }
}
}  // namespace

extern "C" {
long clipops_fill_gaps_workspace(int n_seq, int n_ids, int n_frames) {
    if (n_seq < 0 || n_ids < 0 || n_frames < 0) return -1;
    const __int128 cells = (__int128)n_seq * n_ids * n_frames;
    if (cells > 0x7fffffffL) return -2;
    return 2 * (long)cells + (long)n_seq * n_frames;
}

int clipops_fill_gaps_f32(const float *rows_f, const int64_t *rows_i, const int32_t *counters, int n, int W, int n_seq,
                          int n_ids, int n_frames, int max_gap, int min_length, int32_t *workspace, float *out_f,
                          int64_t *out_i, int32_t *out_counters, int32_t *status, int capacity, void *stream) {
    if (n < 0 || n_seq < 0 || n_ids < 0 || n_frames < 0 || capacity < 0)
        return fail(1, "clipops_fill_gaps_f32: negative size");
    if (max_gap < 0 || min_length < 0) return fail(1, "clipops_fill_gaps_f32: negative max_gap or min_length");
    if (W != 3 && W != 4) return fail(1, "clipops_fill_gaps_f32: W is 3 (frame, id, label) or 4 (sequence, frame, id, label)");
    if (W == 3 && n_seq > 1) return fail(1, "clipops_fill_gaps_f32: rows without a sequence column take n_seq <= 1");
    if (n == 0) return ok();
    const long words = clipops_fill_gaps_workspace(n_seq, n_ids, n_frames);
    if (words == -2) return fail(2, "clipops_fill_gaps_f32: more than 2^31 - 1 cells");
    if (!rows_f || !rows_i || !counters || !out_counters || !status || (words > 0 && !workspace) ||
        (capacity > 0 && (!out_f || !out_i)))
        return fail(1, "clipops_fill_gaps_f32: null pointer");
    const long n_sf = (long)n_seq * n_frames, cells = n_sf * n_ids;
    int32_t *cell = workspace, *right = workspace + cells, *offs = workspace + 2 * cells;
    if (cells > 0 && launch("fg_clear_kernel", fg_clear_kernel, dim3(grid_for(cells)), dim3(256), 0, stream, cell, cells))
        return 3;
    // (without a cell every stored row is out of range: the scatter alone says so)
    if (launch("fg_scatter_kernel", fg_scatter_kernel, dim3(grid_for(n)), dim3(256), 0, stream, rows_i, counters, n, W,
               n_seq, n_ids, n_frames, cell, status))
        return 3;
    if (cells == 0) return 0;
    if (launch("fg_track_kernel", fg_track_kernel, dim3((unsigned)(n_seq * (long)n_ids)), dim3(FG_THREADS), 0, stream, cell,
               right, n_frames, max_gap, min_length))
        return 3;
    if (launch("fg_count_kernel", fg_count_kernel, dim3((unsigned)((n_sf + 255) / 256)), dim3(256), 0, stream, cell, n_sf,
               n_ids, n_frames, offs))
        return 3;
    if (launch("fg_scan_kernel", fg_scan_kernel, dim3(1), dim3(FG_THREADS), 0, stream, offs, n_sf, out_counters, capacity))
        return 3;
    return launch("fg_write_kernel", fg_write_kernel, dim3((unsigned)n_sf), dim3(256), 0, stream, rows_f, rows_i, W, cell,
                  right, offs, n_ids, n_frames, out_f, out_i, capacity) ? 3 : 0;
}
}  // extern "C"
