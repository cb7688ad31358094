// clip_tracks.h -- the device side of the online tracker and of the submit path: result rows, the track bank, the
// bank's result rows, the overlay's draw table, and the error analysis (CLEAR's match events, the draw table coloured
// by event; the cross-class pairs of BDD100K).  One statement of the kept-track rule and of the counters' capacity rule serves the first four (and
// clip_fill_gaps.h, included after this header); one statement of a draw-table row serves both tables.
// Included by clip_ops.hip after clip_common.h.
#pragma once

namespace {
// The kept-track rule (SequenceTracker._report): a track is reported when its best class score and its pixel area pass
// the thresholds; its box goes out as pixel xyxy.  Every float operation rounds once.
struct KeptTrack {
    bool keep;
    float score, x1, y1, x2, y2;                    // the box only where `keep`
};

__device__ __forceinline__ KeptTrack kept_track(const float *__restrict__ boxes, const float *__restrict__ scores, long i,
                                                int K, float ori_w, float ori_h, float score_thresh, float area_thresh) {
    KeptTrack r = {false, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float *sc = scores + i * K;
    float s = sc[0];
    for (int k = 1; k < K; ++k) {                   // torch's max: a NaN wins and stays
        const float v = sc[k];
        if (v > s || v != v) s = v;
    }
    const float cx = boxes[4 * i], cy = boxes[4 * i + 1], w = boxes[4 * i + 2], h = boxes[4 * i + 3];
    const float area = __fmul_rn(__fmul_rn(__fmul_rn(w, ori_w), h), ori_h);
    r.score = s;
    if (!(s > score_thresh && area > area_thresh)) return r;      // false for a NaN on either side
    const float hw = __fmul_rn(0.5f, w), hh = __fmul_rn(0.5f, h);
    r.keep = true;
    r.x1 = __fmul_rn(__fsub_rn(cx, hw), ori_w);
    r.y1 = __fmul_rn(__fsub_rn(cy, hh), ori_h);
    r.x2 = __fmul_rn(__fadd_rn(cx, hw), ori_w);
    r.y2 = __fmul_rn(__fadd_rn(cy, hh), ori_h);
    return r;
}

// the five float columns of a result row
__device__ __forceinline__ void kept_store(float *__restrict__ rf, const KeptTrack &t) {
    rf[0] = t.x1, rf[1] = t.y1, rf[2] = t.x2, rf[3] = t.y2, rf[4] = t.score;
}

// The capacity rule of a result table's counters: of `base` new rows the table stores what fits behind the stored0 it
// holds and counts the rest as dropped.  One lane calls it, after every thread has read the counters.  I: the type the
// caller counts its rows in (int; long in fg_scan_kernel, whose sums are clamped, not wrapped).
template <typename I>
__device__ __forceinline__ void store_counters(int32_t *__restrict__ counters, int stored0, int dropped0, I base,
                                               int capacity) {
    const I room = stored0 < 0 ? 0 : (capacity > stored0 ? capacity - stored0 : 0);
    const I stored = base < room ? base : room;
    counters[0] = (int)(stored0 + stored);
    counters[1] = (int)(dropped0 + (base - stored));
}

// ---- result rows of the submit path (ABI 12): the score / area filter and the pixel boxes of SequenceTracker._report,
//      compacted onto the end of a device-resident table -- one launch per frame, no host read ----
// one workgroup; rows in chunks of 256: a 64-bit ballot and the population count of the lower lanes place a row inside
// its wavefront, the four wave totals go through LDS, `base` runs across chunks.  Both counters are read before
// anything is written and written once, by one lane, with plain stores.  Every float operation rounds once.
__global__ __launch_bounds__(256) void result_rows_kernel(const float *__restrict__ boxes, const float *__restrict__ scores,
                                                          const int64_t *__restrict__ ids,
                                                          const int64_t *__restrict__ labels, int n, int K, int64_t frame,
                                                          float ori_w, float ori_h, float score_thresh, float area_thresh,
                                                          float *__restrict__ rows_f, int64_t *__restrict__ rows_i,
                                                          int32_t *__restrict__ counters, int capacity) {
    __shared__ int wave_total[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int stored0 = counters[0], dropped0 = counters[1];
    int base = 0;                                   // rows kept by the chunks before this one
    for (int c0 = 0; c0 < n; c0 += 256) {           // (n is uniform: every thread makes every trip)
        const int i = c0 + (int)threadIdx.x;
        KeptTrack t = {false, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (i < n) t = kept_track(boxes, scores, i, K, ori_w, ori_h, score_thresh, area_thresh);
        int before, total;
        bank_ranks<4>(t.keep, lane, wave, wave_total, before, total);
        if (t.keep) {
            const long pos = (long)stored0 + base + before;
            if (pos >= 0 && pos < capacity) {
                kept_store(rows_f + pos * 5, t);
                int64_t *ri = rows_i + pos * 3;
                ri[0] = frame;
                ri[1] = ids[i];
                ri[2] = labels[i];
            }
        }
        base += total;
        __syncthreads();                            // wave_total is written again by the next chunk
    }
    if (threadIdx.x == 0) store_counters(counters, stored0, dropped0, base, capacity);
}

// ---- track bank (include/clip_ops_hip.h: clipops_bank_*): the online tracker's bookkeeping for B sequences at once,
//      on fixed-size slot tables -- no row count ever reaches the host ----
// One workgroup per stream, three phases separated by barriers:
//   1. the slots that are free when the call begins, in slot order, into the bank's free_list (ballot + population count
//      inside a wavefront, wave totals through LDS, a running base across chunks of 1024 slots);
//   2. one wavefront per live slot: refresh from model row n_det + s, age, retire (the row is zeroed);
//   3. detect rows in chunks of 1024: one thread decides a row's birth and label, the same ballot scheme ranks the born
//      rows, rank j takes free_list[j]; the (row, slot) pairs of the chunk go through LDS and one wavefront copies a pair.
// Phases 2 and 3 write disjoint slots (live / free at the start).  Every counter is read before anything is written and
// written once by one lane with plain stores; no atomics.
// (16 wavefronts: phase 2 is a chain of dependent loads per slot, and a wavefront walks its slots one after another)
constexpr int BANK_THREADS = 1024, BANK_WAVES = BANK_THREADS / 64;

// Where a bank kernel's thresholds come from: one value for every stream (the scalar entry points) or an array with one
// value per stream (the _streams entry points: a threshold sweep runs one sequence under B settings).  Both give the
// kernels the same float32 / int64 values to compare against, so stream b of a _streams call has the bits of the scalar
// call made with stream b's values.
struct BankUpdateScalars {
    float det_v, track_v;
    int64_t miss_v;
    __device__ __forceinline__ float det(int) const { return det_v; }
    __device__ __forceinline__ float track(int) const { return track_v; }
    __device__ __forceinline__ int64_t miss(int) const { return miss_v; }
};
struct BankUpdatePerStream {
    const float *det_a, *track_a;
    const int64_t *miss_a;
    __device__ __forceinline__ float det(int b) const { return det_a[b]; }
    __device__ __forceinline__ float track(int b) const { return track_a[b]; }
    __device__ __forceinline__ int64_t miss(int b) const { return miss_a[b]; }
};
struct BankRowsScalars {
    float score_v, area_v;
    __device__ __forceinline__ float score(int) const { return score_v; }
    __device__ __forceinline__ float area(int) const { return area_v; }
};
struct BankRowsPerStream {
    const float *score_a, *area_a;
    __device__ __forceinline__ float score(int b) const { return score_a[b]; }
    __device__ __forceinline__ float area(int b) const { return area_a[b]; }
};

template <typename Thresholds>
__global__ __launch_bounds__(BANK_THREADS) void bank_update_kernel(clipops_bank_model m, clipops_bank bank, int n_det, int cap,
                                                          int K, int C, int use_dab, Thresholds th) {
#pragma clang fp contract(off)
    __shared__ int wave_total[BANK_WAVES], wave_live[BANK_WAVES], pair_row[BANK_THREADS], pair_slot[BANK_THREADS];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // (one workgroup is one stream: the three values are uniform over it and read once)
    const float det_thresh = th.det(b), track_thresh = th.track(b);
    const int64_t miss_tolerance = th.miss(b);
    const int QW = use_dab ? C : 2 * C;
    const long bc = (long)b * cap;
    int64_t *ids = bank.ids + bc, *labels = bank.labels + bc, *dtime = bank.disappear_time + bc;
    int32_t *free_list = bank.free_list + bc;
    float *boxes = bank.boxes + bc * 4, *ref_pts = bank.ref_pts + bc * 4;
    float *logits = bank.logits + bc * K, *scores = bank.scores + bc * K;
    float *out_embed = bank.output_embed + bc * C, *long_mem = bank.long_memory + bc * C;
    float *last_out = bank.last_output + bc * C, *query = bank.query_embed + bc * QW;
    const float *m_logits = m.ptr[CLIPOPS_BK_LOGITS] + b * m.batch_stride[CLIPOPS_BK_LOGITS];
    const float *m_boxes = m.ptr[CLIPOPS_BK_BOXES] + b * m.batch_stride[CLIPOPS_BK_BOXES];
    const float *m_out = m.ptr[CLIPOPS_BK_OUTPUTS] + b * m.batch_stride[CLIPOPS_BK_OUTPUTS];
    const float *m_ref = m.ptr[CLIPOPS_BK_LAST_REF] + b * m.batch_stride[CLIPOPS_BK_LAST_REF];
    const float *m_query = m.ptr[CLIPOPS_BK_QUERIES] + b * m.batch_stride[CLIPOPS_BK_QUERIES];
    const long rs_logits = m.row_stride[CLIPOPS_BK_LOGITS], rs_boxes = m.row_stride[CLIPOPS_BK_BOXES];
    const long rs_out = m.row_stride[CLIPOPS_BK_OUTPUTS], rs_ref = m.row_stride[CLIPOPS_BK_LAST_REF];
    const long rs_query = m.row_stride[CLIPOPS_BK_QUERIES];
    const int64_t next0 = bank.next_id[b];
    const int dropped0 = bank.counters[2 * b + 1];

    // ---- 1. free slots, as they are before this call
    int n_free = 0;
    for (int s0 = 0; s0 < cap; s0 += BANK_THREADS) {
        const int s = s0 + (int)threadIdx.x;
        const bool is_free = s < cap && ids[s] < 0;
        int before, total;
        bank_ranks<BANK_WAVES>(is_free, lane, wave, wave_total, before, total);
        if (is_free) free_list[n_free + before] = s;
        n_free += total;
        __syncthreads();                            // wave_total is written again; ids are written from here on
    }

    // ---- 2. live slots: one wavefront each (s, id, label and the decision are uniform over the wavefront)
    int live = 0;
    for (int s = wave; s < cap; s += BANK_WAVES) {
        const int64_t id = ids[s], d0 = dtime[s];
        int64_t lab = labels[s];
        if (id < 0) continue;
        const long r = (long)n_det + s;
        const float *lg = m_logits + r * rs_logits;
        lab = lab < 0 ? 0 : (lab >= K ? K - 1 : lab);
        const float own = sigmoidf(lg[lab]);
        const int64_t d = own < track_thresh ? d0 + 1 : 0;             // (a NaN score does not age the track)
        if (d >= miss_tolerance) {                                      // retired: the slot holds zeros again
            for (int c = lane; c < K; c += 64) logits[(long)s * K + c] = 0.f, scores[(long)s * K + c] = 0.f;
            if (lane < 4) boxes[s * 4L + lane] = 0.f, ref_pts[s * 4L + lane] = 0.f;
            for (int c = lane; c < C; c += 64)
                out_embed[(long)s * C + c] = 0.f, long_mem[(long)s * C + c] = 0.f, last_out[(long)s * C + c] = 0.f;
            for (int c = lane; c < QW; c += 64) query[(long)s * QW + c] = 0.f;
            if (lane == 0) ids[s] = -1, labels[s] = 0, dtime[s] = 0;
        } else {
            for (int c = lane; c < K; c += 64) {
                const float v = lg[c];
                logits[(long)s * K + c] = v;
                scores[(long)s * K + c] = sigmoidf(v);
            }
            if (lane < 4) boxes[s * 4L + lane] = m_boxes[r * rs_boxes + lane];
            for (int c = lane; c < C; c += 64) out_embed[(long)s * C + c] = m_out[r * rs_out + c];
            if (lane == 0) dtime[s] = d;
            ++live;
        }
    }
    if (lane == 0) wave_live[wave] = live;
    __syncthreads();

    // ---- 3. births
    int born_base = 0;                              // born rows of the chunks before this one
    for (int c0 = 0; c0 < n_det; c0 += BANK_THREADS) {      // (n_det is uniform: every thread makes every trip)
        const int r = c0 + (int)threadIdx.x;
        bool born = false;
        int label = 0;
        if (r < n_det) {
            const float *lg = m_logits + r * rs_logits;
            float best = sigmoidf(lg[0]);
            bool nan = best != best;
            for (int k = 1; k < K; ++k) {           // the lowest index of the maximum
                const float v = sigmoidf(lg[k]);
                nan |= v != v;
                if (v > best) best = v, label = k;
            }
            born = !nan && best >= det_thresh;
        }
        int before, total;
        bank_ranks<BANK_WAVES>(born, lane, wave, wave_total, before, total);
        const int room = n_free > born_base ? n_free - born_base : 0;
        const int n_pairs = total < room ? total : room;
        if (born && before < n_pairs) {
            const int slot = free_list[born_base + before];
            pair_row[before] = r;
            pair_slot[before] = slot;
            ids[slot] = next0 + born_base + before;
            labels[slot] = label;
            dtime[slot] = 0;
        }
        __syncthreads();
        for (int p = wave; p < n_pairs; p += BANK_WAVES) {
            const long row = pair_row[p], s = pair_slot[p];
            const float *lg = m_logits + row * rs_logits;
            for (int c = lane; c < K; c += 64) {
                const float v = lg[c];
                logits[s * K + c] = v;
                scores[s * K + c] = sigmoidf(v);
            }
            if (lane < 4) {
                boxes[s * 4 + lane] = m_boxes[row * rs_boxes + lane];
                ref_pts[s * 4 + lane] = m_ref[row * rs_ref + lane];
            }
            for (int c = lane; c < C; c += 64) {
                const float o = m_out[row * rs_out + c], q = m_query[row * rs_query + c];
                out_embed[s * C + c] = o;
                last_out[s * C + c] = o;
                long_mem[s * C + c] = q;
                if (use_dab) {
                    query[s * QW + c] = q;
                } else {
                    query[s * QW + c] = m.det_embed[row * m.det_row_stride + c];
                    query[s * QW + C + c] = q;
                }
            }
        }
        born_base += total;
        __syncthreads();                            // wave_total and the pairs are written again by the next chunk
    }
    if (threadIdx.x == 0) {
        const int placed = born_base < n_free ? born_base : n_free;
        bank.next_id[b] = next0 + placed;
        int live_after = placed;
        for (int v = 0; v < BANK_WAVES; ++v) live_after += wave_live[v];
        bank.counters[2 * b] = live_after;
        bank.counters[2 * b + 1] = dropped0 + (born_base - placed);
    }
}

// clipops_result_rows_f32's filter and arithmetic over the B * cap slots of a bank, streams in order, free slots skipped:
// one workgroup, so that the rows of all streams land in one table in a fixed order.  The stream of a slot is
// slot / cap, and the two thresholds are that stream's.
template <typename Thresholds>
__global__ __launch_bounds__(256) void bank_result_rows_kernel(const float *__restrict__ boxes,
                                                               const float *__restrict__ scores,
                                                               const int64_t *__restrict__ ids,
                                                               const int64_t *__restrict__ labels, int n_slots, int cap,
                                                               int K, const int64_t *__restrict__ seq_frame,
                                                               const float *__restrict__ ori_wh, Thresholds th,
                                                               float *__restrict__ rows_f,
                                                               int64_t *__restrict__ rows_i,
                                                               int32_t *__restrict__ counters, int capacity) {
    __shared__ int wave_total[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int stored0 = counters[0], dropped0 = counters[1];
    int base = 0;
    for (int c0 = 0; c0 < n_slots; c0 += 256) {
        const int i = c0 + (int)threadIdx.x;
        KeptTrack t = {false, 0.f, 0.f, 0.f, 0.f, 0.f};
        int b = 0;
        if (i < n_slots && ids[i] >= 0) {
            b = i / cap;
            t = kept_track(boxes, scores, i, K, ori_wh[2 * b], ori_wh[2 * b + 1], th.score(b), th.area(b));
        }
        int before, total;
        bank_ranks<4>(t.keep, lane, wave, wave_total, before, total);
        if (t.keep) {
            const long pos = (long)stored0 + base + before;
            if (pos >= 0 && pos < capacity) {
                kept_store(rows_f + pos * 5, t);
                int64_t *ri = rows_i + pos * 4;
                ri[0] = seq_frame[2 * b];
                ri[1] = seq_frame[2 * b + 1];
                ri[2] = ids[i];
                ri[3] = labels[i];
            }
        }
        base += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) store_counters(counters, stored0, dropped0, base, capacity);
}

// ---- the overlay's draw table from device tracks (include/clip_ops_hip.h: clipops_draw_table_f32) ----
// One workgroup per stream.  A slot's key is its id when the slot is kept (bank_result_rows_kernel's filter, id below
// 2^31) and -1 otherwise; the row of a kept slot is the number of kept slots of the stream with a smaller id (equal ids,
// which a bank never holds, in slot order).  Slots go through in chunks of 1024, one thread each; for every chunk of slots
// the keys of every chunk pass through LDS and each thread counts the ones below its own -- all pairs, no atomics, and
// every thread also counts the kept slots of the stream, so the padding rows are known without another pass.
struct DrawKey {
    int key;                                        // the id of a kept slot, -1 otherwise
    float x1, y1, x2, y2;
};

__device__ __forceinline__ DrawKey draw_table_key(const float *__restrict__ boxes, const float *__restrict__ scores,
                                                  const int64_t *__restrict__ ids, long i, int K, float ori_w,
                                                  float ori_h, float score_thresh, float area_thresh) {
    DrawKey r = {-1, 0.f, 0.f, 0.f, 0.f};
    const int64_t id = ids[i];
    if (id < 0 || id > 0x7fffffffLL) return r;
    const KeptTrack t = kept_track(boxes, scores, i, K, ori_w, ori_h, score_thresh, area_thresh);
    if (!t.keep) return r;
    r.key = (int)id;
    r.x1 = t.x1, r.y1 = t.y1, r.x2 = t.x2, r.y2 = t.y2;
    return r;
}

// floor(v + 0.5) in float32, NaN -> 0, clamped to +-2^24 (render.track_table)
__device__ __forceinline__ int draw_table_round(float v) {
    const float r = floorf(__fadd_rn(v, 0.5f));
    if (r != r) return 0;
    return (int)fminf(fmaxf(r, -16777216.f), 16777216.f);
}

// render.palette_entry(i), i in 0 .. 63, as r | g << 8 | b << 16
__device__ __forceinline__ int draw_table_palette(int i) {
    const int hue = (i * 13 % 64) * 24, sector = hue >> 8, f = hue & 255;
    const int lo = i % 3 == 0 ? 0 : (i % 3 == 1 ? 64 : 112);
    const int up = lo + (255 - lo) * f / 255, down = lo + (255 - lo) * (255 - f) / 255;
    int r, g, b;
    switch (sector) {
        case 0: r = 255, g = up, b = lo; break;
        case 1: r = down, g = 255, b = lo; break;
        case 2: r = lo, g = 255, b = up; break;
        case 3: r = lo, g = down, b = 255; break;
        case 4: r = up, g = lo, b = 255; break;
        default: r = 255, g = lo, b = down; break;
    }
    return r | g << 8 | b << 16;
}

constexpr int DRAW_ROW_WORDS = 16;                  // TRACKDRAW_ROW_WORDS of include/track_draw_hip.h

// One row as render.track_table writes it for `id` and the float32 xyxy box, in the colour rgb = r | g << 8 | b << 16
// (bytes 0 and 2 swapped for bgr): the rounded corners, the tab above the box (inside it at the top edge, shifted left
// at the right edge of a frame `width` wide), the text colour by the integer luma rule, the packed decimal digits.
__device__ __forceinline__ void draw_table_row(int32_t *__restrict__ row, int id, float bx1, float by1, float bx2,
                                               float by2, int rgb, int bgr, int font_scale, int width) {
    const int x1 = draw_table_round(bx1), y1 = draw_table_round(by1);
    const int r = rgb & 255, g = (rgb >> 8) & 255, bl = rgb >> 16;
    int n_digits = 1;
    for (int v = id; v >= 10; v /= 10) ++n_digits;
    unsigned lo_word = 0, hi_word = 0;              // glyph k is the k-th digit from the left
    for (int k = n_digits - 1, v = id; k >= 0; --k, v /= 10) {
        const unsigned d = (unsigned)(v % 10);
        if (k < 8) lo_word |= d << (4 * k);
        else hi_word |= d << (4 * (k - 8));
    }
    const int tab_w = (6 * n_digits - 1) * font_scale + 2, tab_h = 7 * font_scale + 2;
    const int ty1 = y1 - tab_h >= 0 ? y1 - tab_h : y1;
    const int tx1 = min(x1, width - tab_w);
    row[0] = x1, row[1] = y1, row[2] = draw_table_round(bx2), row[3] = draw_table_round(by2);
    row[4] = bgr ? (bl | g << 8 | r << 16) : rgb;
    row[5] = tx1, row[6] = ty1, row[7] = tx1 + tab_w - 1, row[8] = ty1 + tab_h - 1;
    row[9] = ((77 * r + 150 * g + 29 * bl) >> 8) >= 128 ? 0 : 0xFFFFFF;
    row[10] = n_digits, row[11] = (int32_t)lo_word, row[12] = (int32_t)hi_word;
    row[13] = row[14] = row[15] = 0;
}

// the row that draws nothing: x2 < x1
__device__ __forceinline__ void draw_table_padding(int32_t *__restrict__ row) {
    for (int k = 0; k < DRAW_ROW_WORDS; ++k) row[k] = (k == 2 || k == 3) ? -1 : 0;
}

__global__ __launch_bounds__(BANK_THREADS) void draw_table_kernel(const float *__restrict__ boxes,
                                                                  const float *__restrict__ scores,
                                                                  const int64_t *__restrict__ ids, int cap, int K,
                                                                  const float *__restrict__ ori_wh, float score_thresh,
                                                                  float area_thresh, int bgr, int font_scale,
                                                                  int32_t *__restrict__ table) {
    __shared__ int4 keys4[BANK_THREADS / 4];
    int *keys = reinterpret_cast<int *>(keys4);
    const int b = blockIdx.x, tid = threadIdx.x;
    const long bc = (long)b * cap;
    const float ori_w = ori_wh[2 * b], ori_h = ori_wh[2 * b + 1];
    int32_t *rows = table + bc * DRAW_ROW_WORDS;
    int total = 0;                                  // kept slots of the stream (every thread counts them all)
    for (int i0 = 0; i0 < cap; i0 += BANK_THREADS) {             // (cap is uniform: every thread makes every trip)
        const int i = i0 + tid;
        DrawKey mine = {-1, 0.f, 0.f, 0.f, 0.f};
        if (i < cap) mine = draw_table_key(boxes, scores, ids, bc + i, K, ori_w, ori_h, score_thresh, area_thresh);
        int rank = 0;
        total = 0;
        for (int j0 = 0; j0 < cap; j0 += BANK_THREADS) {
            int kj = mine.key;
            if (j0 != i0) {
                const int j = j0 + tid;
                kj = j < cap ? draw_table_key(boxes, scores, ids, bc + j, K, ori_w, ori_h, score_thresh, area_thresh).key
                             : -1;
            }
            keys[tid] = kj;
            __syncthreads();
            const int nj4 = (min(BANK_THREADS, cap - j0) + 3) >> 2;     // (every thread wrote a key: -1 past cap)
#pragma unroll 4
            for (int q = 0; q < nj4; ++q) {         // four keys a read: the loop is a chain of LDS latencies otherwise
                const int4 k4 = keys4[q];
                const int k[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    total += k[e] >= 0;
                    rank += k[e] >= 0 && (k[e] < mine.key || (k[e] == mine.key && j0 + 4 * q + e < i));
                }
            }
            __syncthreads();                        // keys is written again by the next chunk
        }
        if (mine.key < 0) continue;
        const int rgb = draw_table_palette(mine.key & 63);
        draw_table_row(rows + (long)rank * DRAW_ROW_WORDS, mine.key, mine.x1, mine.y1, mine.x2, mine.y2, rgb, bgr,
                       font_scale, (int)ori_w);
    }
    for (int p = total + tid; p < cap; p += BANK_THREADS) {      // the rows that draw nothing: x2 < x1
        draw_table_padding(rows + (long)p * DRAW_ROW_WORDS);
    }
}

// ---- error analysis (include/clip_ops_hip.h: clipops_clear_events_f64, clipops_error_table_f64) ----
// CLEAR's walk a second time.  trackeval_clear (track_eval.hip) makes the same decisions and keeps their counts; that
// library's entry points are fixed, so the walk that keeps the decisions is stated here, on the same assign_core.h.  It
// needs less state: per ground-truth id the tracker id of its last match (`last`) and the evaluated frame that match
// happened in (`last_at`).  "Matched in the previous evaluated frame" is last_at == step - 1, so nothing is reset per
// frame; frames without ground truth or without tracker rows are not evaluated frames and do not advance `step`.
constexpr double EVENTS_EPS = 0x1p-52;              // np.finfo('float').eps
constexpr double EVENTS_THRESHOLD = 0.5;

struct EventsView {
    const double *s;
    const int32_t *gid, *tid;       // the frame's ids
    const int32_t *last, *last_at;  // [G]
    int k, G, prev_step;
    __device__ __forceinline__ double at(int i, int j) const {
        const double v = s[(size_t)i * k + j];
        if (v < EVENTS_THRESHOLD - EVENTS_EPS) return -0.0;
        const int g = gid[i];
        const bool kept = (unsigned)g < (unsigned)G && last_at[g] == prev_step && last[g] == tid[j];
        return -((kept ? 1000.0 : 0.0) + v);
    }
};

__host__ __device__ inline size_t events_align16(size_t n) { return (n + 15) & ~(size_t)15; }
// LDS of one sequence: the pair lists (2 * mn int32), last and last_at (2 * max_gt_ids int32), the solver's scratch
__host__ inline size_t events_lds_bytes(int max_gt, int max_tr, int max_gt_ids) {
    const int mn = max_gt < max_tr ? max_gt : max_tr, mx = max_gt < max_tr ? max_tr : max_gt;
    return events_align16((size_t)2 * mn * 4) + events_align16((size_t)2 * max_gt_ids * 4) +
           events_align16(assign::work_bytes(mn, mx));
}

__device__ __forceinline__ int wave_sum_i32(int x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// One wavefront per sequence.  A frame's rows are first written as unmatched by all lanes; behind the barriers of the
// solver, lane p of the pair pass overwrites the two rows of pair p.  Ids are unique in a frame, so the pairs of a frame
// touch different entries of last / last_at and the pass needs no order; the counts are lane sums, reduced at the end.
__global__ __launch_bounds__(64) void clear_events_kernel(const double *__restrict__ sim,
                                                           const int64_t *__restrict__ sim_off,
                                                           const int32_t *__restrict__ gt_off,
                                                           const int32_t *__restrict__ tr_off,
                                                           const int32_t *__restrict__ gt_ids,
                                                           const int32_t *__restrict__ tr_ids,
                                                           const int32_t *__restrict__ seq_off,
                                                           const int32_t *__restrict__ n_gt_ids, int max_gt, int max_tr,
                                                           int max_gt_ids, int mn, int32_t *__restrict__ gt_partner,
                                                           int32_t *__restrict__ gt_flags,
                                                           int32_t *__restrict__ tr_partner,
                                                           int32_t *__restrict__ counts, int32_t *__restrict__ status) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char s_events[];
    const int s = blockIdx.x, lane = threadIdx.x;
    const int G = n_gt_ids[s];
    int32_t *rows = reinterpret_cast<int32_t *>(s_events), *cols = rows + mn;
    int32_t *last = reinterpret_cast<int32_t *>(s_events + events_align16((size_t)2 * mn * 4));
    int32_t *last_at = last + max_gt_ids;
    unsigned char *work = s_events + events_align16((size_t)2 * mn * 4) + events_align16((size_t)2 * max_gt_ids * 4);
    const WaveLanes lanes{lane};
    const int f_begin = seq_off[s], f_end = seq_off[s + 1];
    int rc = (G < 0 || G > max_gt_ids) ? -2 : 0;
    int n_tp = 0, n_fn = 0, n_fp = 0, n_idsw = 0, n_frag = 0;           // this lane's share
    int step = 0;                                   // evaluated frames so far
    if (rc == 0) {
        lanes.each(G, [&](int i) { last[i] = -1; last_at[i] = -2; });
        lanes.sync();
    }
    for (int f = f_begin; rc == 0 && f < f_end; ++f) {
        const int g0 = gt_off[f], g = gt_off[f + 1] - g0, k0 = tr_off[f], k = tr_off[f + 1] - k0;
        if (g < 0 || k < 0 || g > max_gt || k > max_tr) {
            rc = -2;
            break;
        }
        lanes.each(g, [&](int i) { gt_partner[g0 + i] = -1; gt_flags[g0 + i] = 0; });
        lanes.each(k, [&](int j) { tr_partner[k0 + j] = -1; });
        if (g == 0) {
            if (lane == 0) n_fp += k;
            continue;
        }
        if (k == 0) {
            if (lane == 0) n_fn += g;
            continue;
        }
        const int32_t *gid = gt_ids + g0, *tid = tr_ids + k0;
        const double *sm = sim + sim_off[f];
        const EventsView view{sm, gid, tid, last, last_at, k, G, step - 1};
        const int n = assign::solve_view(lanes, view, g, k, work, rows, cols);
        if (n < 0) {
            rc = -1;
            break;
        }
        lanes.sync();                               // the frame's unmatched rows are written; the pairs are visible
        int n_match = 0;
        lanes.each(n, [&](int p) {
            const int i = rows[p], j = cols[p];
            if (sm[(size_t)i * k + j] < EVENTS_THRESHOLD - EVENTS_EPS) return;      // (a kept score is >= 0.5 - eps > eps)
            const int gi = gid[i], tj = tid[j];
            if ((unsigned)gi >= (unsigned)G) return;
            const int before = last[gi];
            const bool sw = before >= 0 && before != tj;
            const bool fr = before >= 0 && last_at[gi] != step - 1;
            last[gi] = tj;
            last_at[gi] = step;
            gt_partner[g0 + i] = j;
            gt_flags[g0 + i] = (sw ? CLIPOPS_EVENT_SWITCH : 0) | (fr ? CLIPOPS_EVENT_FRAG : 0);
            tr_partner[k0 + j] = i;
            n_idsw += sw, n_frag += fr, ++n_match;
        });
        n_tp += n_match;
        n_fn -= n_match, n_fp -= n_match;           // (with lane 0's g and k below: g - matches, k - matches)
        if (lane == 0) n_fn += g, n_fp += k;
        ++step;
        lanes.sync();                               // last / last_at are read by the next frame's solver
    }
    lanes.sync();
    if (rc != 0) {                                  // nothing of a failed sequence is left half written
        const int a0 = gt_off[f_begin], a1 = gt_off[f_end], b0 = tr_off[f_begin], b1 = tr_off[f_end];
        lanes.each(a1 - a0, [&](int i) { gt_partner[a0 + i] = -1; gt_flags[a0 + i] = 0; });
        lanes.each(b1 - b0, [&](int j) { tr_partner[b0 + j] = -1; });
        n_tp = n_fn = n_fp = n_idsw = n_frag = 0;
    }
    n_tp = wave_sum_i32(n_tp), n_fn = wave_sum_i32(n_fn), n_fp = wave_sum_i32(n_fp);
    n_idsw = wave_sum_i32(n_idsw), n_frag = wave_sum_i32(n_frag);
    if (lane == 0) {
        int32_t *o = counts + (size_t)s * 5;
        o[0] = n_tp, o[1] = n_fn, o[2] = n_fp, o[3] = n_idsw, o[4] = n_frag;
        status[s] = rc;
    }
}

// r | g << 8 | b << 16 of an event kind; -1: the kind is not drawn
__device__ __forceinline__ int error_table_colour(int kind) {
    switch (kind) {
        case CLIPOPS_KIND_MATCH: return 0 | 200 << 8 | 0 << 16;
        case CLIPOPS_KIND_SWITCH: return 255 | 0 << 8 | 255 << 16;
        case CLIPOPS_KIND_MISS: return 255 | 200 << 8 | 0 << 16;
        case CLIPOPS_KIND_FP: return 255 | 0 << 8 | 0 << 16;
        default: return -1;
    }
}

// One workgroup per frame: the ground-truth rows, then the tracker rows, in chunks of 256; a drawn row's place is the
// number of drawn rows before it (result_rows_kernel's ballot ranks, `base` running across chunks and sides).
__global__ __launch_bounds__(256) void error_table_kernel(const double *__restrict__ gt_boxes,
                                                          const double *__restrict__ tr_boxes,
                                                          const int32_t *__restrict__ gt_off,
                                                          const int32_t *__restrict__ tr_off,
                                                          const int32_t *__restrict__ gt_ids,
                                                          const int32_t *__restrict__ tr_ids,
                                                          const int32_t *__restrict__ gt_kind,
                                                          const int32_t *__restrict__ tr_kind, int max_rows, int width,
                                                          int bgr, int font_scale, int32_t *__restrict__ table) {
#pragma clang fp contract(off)
    __shared__ int wave_total[4];
    const int f = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t *rows = table + (long)f * max_rows * DRAW_ROW_WORDS;
    long base = 0;                                  // drawn rows before this chunk
    for (int side = 0; side < 2; ++side) {
        const double *boxes = side ? tr_boxes : gt_boxes;
        const int32_t *ids = side ? tr_ids : gt_ids, *kinds = side ? tr_kind : gt_kind;
        const int r0 = side ? tr_off[f] : gt_off[f], n = (side ? tr_off[f + 1] : gt_off[f + 1]) - r0;
        for (int c0 = 0; c0 < n; c0 += 256) {       // (n is uniform: every thread makes every trip)
            const int i = c0 + (int)threadIdx.x;
            int kind = CLIPOPS_KIND_IGNORED, id = -1;
            if (i < n) kind = kinds[r0 + i], id = ids[r0 + i];
            const bool drawn = id >= 0 && (side ? (kind == CLIPOPS_KIND_MATCH || kind == CLIPOPS_KIND_SWITCH ||
                                                   kind == CLIPOPS_KIND_FP)
                                                : kind == CLIPOPS_KIND_MISS);
            int before, total;
            bank_ranks<4>(drawn, lane, wave, wave_total, before, total);
            const long pos = base + before;
            if (drawn && pos < max_rows) {
                const double *b = boxes + (long)(r0 + i) * 4;
                draw_table_row(rows + pos * DRAW_ROW_WORDS, id, (float)b[0], (float)b[1], (float)(b[0] + b[2]),
                               (float)(b[1] + b[3]), error_table_colour(kind), bgr, font_scale, width);
            }
            base += total;
            __syncthreads();                        // wave_total is written again by the next chunk
        }
    }
    for (long p = base + threadIdx.x; p < max_rows; p += 256) draw_table_padding(rows + p * DRAW_ROW_WORDS);
}

// ---- BDD100K error analysis (include/clip_ops_hip.h: clipops_bdd_cross_class_f64) ----
// What the per-class walks cannot see: a box that is a MISS in one class and a false positive in another.  One wavefront
// per input frame pairs the frame's MISS rows with its FP rows of a DIFFERENT class, maximising the summed IoU.
// TrackEval's class id -> class index in its order of evaluation, -1: not evaluated (as track_eval_bdd.hip)
__device__ __forceinline__ int bdd_class_index(int id) {
    switch (id) {
        case 1: return 0;       // pedestrian
        case 2: return 1;       // rider
        case 4: return 2;       // car
        case 5: return 3;       // bus
        case 6: return 4;       // truck
        case 7: return 5;       // train
        case 10: return 6;      // motorcycle
        case 11: return 7;      // bicycle
        default: return -1;
    }
}

// the candidates of a frame, compacted into LDS in order of appearance: row within the frame, class index
struct CrossSide {
    const double *boxes;        // the frame's first box
    const int32_t *row, *cls;   // [n] LDS
};

// IoU of corner boxes in the operation order of track_eval_bdd.hip's similarity_kernel (the same bits), thresholded by
// the project's rule; 0 for two rows of one class
struct CrossView {
    CrossSide g, t;
    __device__ __forceinline__ double score(int i, int j) const {
#pragma clang fp contract(off)                      // (the areas' products must not fuse into the union's sum)
        if (g.cls[i] == t.cls[j]) return 0.0;
        const double *a = g.boxes + (size_t)g.row[i] * 4, *b = t.boxes + (size_t)t.row[j] * 4;
        const double ax0 = a[0], ay0 = a[1], ax1 = a[2], ay1 = a[3];
        const double bx0 = b[0], by0 = b[1], bx1 = b[2], by1 = b[3];
        const double w = (ax1 < bx1 ? ax1 : bx1) - (ax0 > bx0 ? ax0 : bx0);
        const double h = (ay1 < by1 ? ay1 : by1) - (ay0 > by0 ? ay0 : by0);
        double inter = (w > 0.0 ? w : 0.0) * (h > 0.0 ? h : 0.0);
        const double area1 = (ax1 - ax0) * (ay1 - ay0), area2 = (bx1 - bx0) * (by1 - by0);
        double uni = area1 + area2 - inter;
        if (area1 <= EVENTS_EPS || area2 <= EVENTS_EPS || uni <= EVENTS_EPS) inter = 0.0;
        if (uni <= EVENTS_EPS) uni = 1.0;
        const double v = inter / uni;
        return v < EVENTS_THRESHOLD - EVENTS_EPS ? 0.0 : v;
    }
    __device__ __forceinline__ double at(int i, int j) const { return -score(i, j); }
};

// LDS of one frame: the pair lists (2 * mn int32), row and class of the candidates of both sides, the solver's scratch
__host__ inline size_t cross_lds_bytes(int max_gt, int max_tr) {
    const int mn = max_gt < max_tr ? max_gt : max_tr, mx = max_gt < max_tr ? max_tr : max_gt;
    return events_align16((size_t)2 * mn * 4) + events_align16((size_t)2 * (max_gt + max_tr) * 4) +
           events_align16(assign::work_bytes(mn, mx));
}

// Rows of `kinds[0 .. n)` equal to `want` whose class is evaluated, 64 per ballot, into row / cls while they fit `cap`;
// returns their number (wave-uniform).  Every row's three outputs get the values of "no partner" on the way.
__device__ __forceinline__ int cross_compact(const int32_t *__restrict__ kinds, const int32_t *__restrict__ classes, int n,
                                             int want, int cap, int lane, int32_t *row, int32_t *cls,
                                             int32_t *__restrict__ partner, int32_t *__restrict__ partner_class,
                                             double *__restrict__ iou) {
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    int total = 0;
    for (int base = 0; base < n; base += 64) {              // (wave-uniform trip count: every lane votes)
        const int i = base + lane;
        int ci = -1;
        if (i < n) {
            partner[i] = -1, partner_class[i] = -1, iou[i] = 0.0;
            if (kinds[i] == want) ci = bdd_class_index(classes[i]);
        }
        const unsigned long long votes = __ballot(ci >= 0);
        const int at = total + __popcll(votes & below);
        if (ci >= 0 && at < cap) row[at] = i, cls[at] = ci;
        total += __popcll(votes);
    }
    return total;
}

__global__ __launch_bounds__(64) void bdd_cross_class_kernel(const double *__restrict__ gt_boxes,
                                                              const double *__restrict__ tr_boxes,
                                                              const int32_t *__restrict__ gt_classes,
                                                              const int32_t *__restrict__ tr_classes,
                                                              const int32_t *__restrict__ gt_off,
                                                              const int32_t *__restrict__ tr_off,
                                                              const int32_t *__restrict__ gt_kind,
                                                              const int32_t *__restrict__ tr_kind, int max_gt, int max_tr,
                                                              int mn, int32_t *__restrict__ gt_partner,
                                                              int32_t *__restrict__ gt_class, double *__restrict__ gt_iou,
                                                              int32_t *__restrict__ tr_partner,
                                                              int32_t *__restrict__ tr_class, double *__restrict__ tr_iou,
                                                              int32_t *__restrict__ status) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char s_cross[];
    const int f = blockIdx.x, lane = threadIdx.x;
    const int g0 = gt_off[f], g = gt_off[f + 1] - g0, k0 = tr_off[f], k = tr_off[f + 1] - k0;
    int32_t *rows = reinterpret_cast<int32_t *>(s_cross), *cols = rows + mn;
    int32_t *g_row = reinterpret_cast<int32_t *>(s_cross + events_align16((size_t)2 * mn * 4));
    int32_t *g_cls = g_row + max_gt, *t_row = g_cls + max_gt, *t_cls = t_row + max_tr;
    unsigned char *work = s_cross + events_align16((size_t)2 * mn * 4) + events_align16((size_t)2 * (max_gt + max_tr) * 4);
    const WaveLanes lanes{lane};
    const int ng = cross_compact(gt_kind + g0, gt_classes + g0, g, CLIPOPS_KIND_MISS, max_gt, lane, g_row, g_cls,
                                 gt_partner + g0, gt_class + g0, gt_iou + g0);
    const int nt = cross_compact(tr_kind + k0, tr_classes + k0, k, CLIPOPS_KIND_FP, max_tr, lane, t_row, t_cls,
                                 tr_partner + k0, tr_class + k0, tr_iou + k0);
    lanes.sync();                                   // the candidates and the rows' "no partner" are written
    int rc = 0;
    if (ng > max_gt || nt > max_tr) {
        rc = -2;
    } else if (ng > 0 && nt > 0) {
        const CrossView view{{gt_boxes + (size_t)g0 * 4, g_row, g_cls}, {tr_boxes + (size_t)k0 * 4, t_row, t_cls}};
        const int n = assign::solve_view(lanes, view, ng, nt, work, rows, cols);
        if (n < 0) rc = -1;
        lanes.each(n, [&](int p) {                  // (n < 0: no trip)
            const int i = rows[p], j = cols[p];
            const double v = view.score(i, j);
            if (!(v > EVENTS_EPS)) return;
            const int gi = g0 + g_row[i], tj = k0 + t_row[j];
            gt_partner[gi] = t_row[j], gt_class[gi] = t_cls[j], gt_iou[gi] = v;
            tr_partner[tj] = g_row[i], tr_class[tj] = g_cls[i], tr_iou[tj] = v;
        });
    }
    if (lane == 0) status[f] = rc;
}

// ---- association analysis (include/clip_ops_hip.h: clipops_hota_events_f64, clipops_identity_pairs_i32,
//      clipops_assoc_reduce_f64, clipops_timeline_u8) ----
// HOTA's and Identity's assignments a second time.  trackeval_hota_match and trackeval_identity (track_eval.hip) solve the
// same problems and keep sums; that library's entry points are fixed, so the two cost views it keeps private are stated
// here again, on the same assign_core.h, and the pairs are kept.
constexpr int ASSOC_ALPHAS = CLIPOPS_ASSOC_ALPHAS;

struct AssocAlphas {
    double v[ASSOC_ALPHAS];
};

struct HotaEventsView {
    const double *s, *align;        // the frame's similarity; the sequence's alignment table [G, K]
    const int32_t *gid, *tid;       // the frame's ids
    int k, K;
    __device__ __forceinline__ double at(int i, int j) const {      // (ids are relabelled 0 .. n - 1, as for HotaView)
#pragma clang fp contract(off)
        return -(align[(long)gid[i] * K + tid[j]] * s[(size_t)i * k + j]);
    }
};

__host__ inline size_t assoc_solve_lds_bytes(int n_rows, int n_cols) {
    const int mn = n_rows < n_cols ? n_rows : n_cols, mx = n_rows < n_cols ? n_cols : n_rows;
    return events_align16((size_t)2 * mn * 4) + events_align16(assign::work_bytes(mn, mx));
}

// One wavefront per frame.  All lanes first write the frame's rows as unmatched; behind the barriers of the solver, lane p
// of the pair pass overwrites the two rows of pair p and counts the pair into matches[a] for every threshold a < level.
__global__ __launch_bounds__(64) void hota_events_kernel(const double *__restrict__ sim,
                                                          const int64_t *__restrict__ sim_off,
                                                          const int32_t *__restrict__ gt_off,
                                                          const int32_t *__restrict__ tr_off,
                                                          const int32_t *__restrict__ gt_ids,
                                                          const int32_t *__restrict__ tr_ids,
                                                          const int32_t *__restrict__ frame_seq,
                                                          const int32_t *__restrict__ n_tr_ids,
                                                          const int64_t *__restrict__ cell_off,
                                                          const double *__restrict__ alignment, const AssocAlphas alphas,
                                                          int max_gt, int max_tr, int mn, int32_t *__restrict__ gt_partner,
                                                          int32_t *__restrict__ gt_level, int32_t *__restrict__ tr_partner,
                                                          int32_t *__restrict__ tr_level, int32_t *__restrict__ matches,
                                                          int32_t *__restrict__ status) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char s_assoc[];
    const int f = blockIdx.x, lane = threadIdx.x;
    const int g0 = gt_off[f], g = gt_off[f + 1] - g0, k0 = tr_off[f], k = tr_off[f + 1] - k0;
    int32_t *rows = reinterpret_cast<int32_t *>(s_assoc), *cols = rows + mn;
    const WaveLanes lanes{lane};
    lanes.each(g, [&](int i) { gt_partner[g0 + i] = -1; gt_level[g0 + i] = 0; });
    lanes.each(k, [&](int j) { tr_partner[k0 + j] = -1; tr_level[k0 + j] = 0; });
    int rc = 0, n = 0;
    const int s = frame_seq[f];
    const int K = n_tr_ids[s];
    const long c0 = cell_off[s], cells = cell_off[s + 1] - c0;
    const double *sm = sim + sim_off[f];
    const int32_t *gid = gt_ids + g0, *tid = tr_ids + k0;
    if (g < 0 || k < 0 || g > max_gt || k > max_tr) {
        rc = -2;
    } else if (g > 0 && k > 0) {
        const HotaEventsView view{sm, alignment + c0, gid, tid, k, K};
        n = assign::solve_view(lanes, view, g, k, s_assoc + events_align16((size_t)2 * mn * 4), rows, cols);
        if (n < 0) {
            rc = -1;
            n = 0;
        }
    }
    lanes.sync();                                   // the frame's unmatched rows are written; the pairs are visible
    lanes.each(n, [&](int p) {
        const int i = rows[p], j = cols[p];
        const double v = sm[(size_t)i * k + j];
        int level = 0;
#pragma unroll
        for (int a = 0; a < ASSOC_ALPHAS; ++a) level += v >= alphas.v[a] - EVENTS_EPS;
        if (level == 0) return;
        gt_partner[g0 + i] = j, gt_level[g0 + i] = level;
        tr_partner[k0 + j] = i, tr_level[k0 + j] = level;
        if (!matches) return;
        const int gi = gid[i], tj = tid[j];
        const long c = (long)gi * K + tj;
        if (gi < 0 || (unsigned)tj >= (unsigned)K || c >= cells) return;
        int32_t *mc = matches + ASSOC_ALPHAS * c0 + c;
        for (int a = 0; a < level; ++a) atomicAdd(mc + (long)a * cells, 1);
    });
    if (lane == 0) status[f] = rc;
}

// Identity's cost, a function of the counts (evaluation._identity_host's fn + fp): never a matrix in memory
struct IdentityPairsView {
    const int32_t *gc, *tc, *idm;   // detections per gt id, per tracker id; frames with sim >= 0.5 per (gt id, tracker id)
    int G, K;
    __device__ __forceinline__ double fn(int i, int j) const {
        if (i >= G) return 0.0;
        if (j < K) return (double)gc[i] - (double)idm[(long)i * K + j];
        return j - K == i ? (double)gc[i] : 1e10;
    }
    __device__ __forceinline__ double fp(int i, int j) const {
        if (j >= K) return 0.0;
        if (i < G) return (double)tc[j] - (double)idm[(long)i * K + j];
        return i - G == j ? (double)tc[j] : 1e10;
    }
    __device__ __forceinline__ double at(int i, int j) const { return fn(i, j) + fp(i, j); }
};

// One wavefront per sequence: the (G + K) x (G + K) problem; row r < G paired with column c < K is the map g -> k, any
// other pair leaves its id unmatched.  The problem is square, so every id of either side is in exactly one pair.
__global__ __launch_bounds__(64) void identity_pairs_kernel(const int32_t *__restrict__ n_gt_ids,
                                                             const int32_t *__restrict__ n_tr_ids,
                                                             const int64_t *__restrict__ cell_off,
                                                             const int32_t *__restrict__ gid_off,
                                                             const int32_t *__restrict__ tid_off,
                                                             const int32_t *__restrict__ gt_count,
                                                             const int32_t *__restrict__ tr_count,
                                                             const int32_t *__restrict__ id_matches, int max_ids,
                                                             int32_t *__restrict__ gt_id_partner,
                                                             int32_t *__restrict__ gt_idtp,
                                                             int32_t *__restrict__ tr_id_partner,
                                                             int32_t *__restrict__ tr_idtp, int32_t *__restrict__ status) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char s_assoc[];
    const int s = blockIdx.x, lane = threadIdx.x;
    const int G = n_gt_ids[s], K = n_tr_ids[s], N = G + K;
    int32_t *rows = reinterpret_cast<int32_t *>(s_assoc), *cols = rows + max_ids;
    int32_t *gp = gt_id_partner + gid_off[s], *gtp = gt_idtp + gid_off[s];
    int32_t *tp = tr_id_partner + tid_off[s], *ttp = tr_idtp + tid_off[s];
    const int32_t *idm = id_matches + cell_off[s];
    const WaveLanes lanes{lane};
    int rc = 0, n = 0;
    if (G < 0 || K < 0) {                           // (no table of such a sequence has an entry)
        if (lane == 0) status[s] = -2;
        return;
    }
    lanes.each(G, [&](int i) { gp[i] = -1; gtp[i] = 0; });
    lanes.each(K, [&](int j) { tp[j] = -1; ttp[j] = 0; });
    if (N > max_ids) {
        rc = -2;
    } else if (G > 0 && K > 0) {                    // (with an empty side every id keeps its own slot)
        const IdentityPairsView view{gt_count + gid_off[s], tr_count + tid_off[s], idm, G, K};
        n = assign::solve_view(lanes, view, N, N, s_assoc + events_align16((size_t)2 * max_ids * 4), rows, cols);
        if (n < 0) {
            rc = -1;
            n = 0;
        }
    }
    lanes.sync();
    lanes.each(n, [&](int p) {
        const int r = rows[p], c = cols[p];
        if (r < G && c < K) {
            const int both = idm[(long)r * K + c];
            gp[r] = c, gtp[r] = both;
            tp[c] = r, ttp[c] = both;
        }
    });
    if (lane == 0) status[s] = rc;
}

__device__ __forceinline__ double assoc_wave_sum_f64(double v) {     // a fixed xor tree: the same bits on every lane
#pragma clang fp contract(off)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// One wavefront per (id, sequence, side).  Lane l walks the other side's ids l, l + 64, ... in ascending order; integer
// sums meet in shuffles, double sums are the lanes' partials through the fixed tree above.
__global__ __launch_bounds__(64) void assoc_reduce_kernel(const int32_t *__restrict__ n_gt_ids,
                                                           const int32_t *__restrict__ n_tr_ids,
                                                           const int64_t *__restrict__ cell_off,
                                                           const int32_t *__restrict__ gid_off,
                                                           const int32_t *__restrict__ tid_off,
                                                           const int32_t *__restrict__ gt_count,
                                                           const int32_t *__restrict__ tr_count,
                                                           const int32_t *__restrict__ matches, int a0,
                                                           int32_t *__restrict__ gt_tp, double *__restrict__ gt_num,
                                                           int32_t *__restrict__ gt_top, int32_t *__restrict__ tr_tp,
                                                           double *__restrict__ tr_num, int32_t *__restrict__ tr_top) {
#pragma clang fp contract(off)
    const int id = blockIdx.x, s = blockIdx.y, side = blockIdx.z, lane = threadIdx.x;
    const int G = n_gt_ids[s], K = n_tr_ids[s];
    const int n_mine = side ? K : G, n_other = side ? G : K;
    if (id >= n_mine) return;
    const long c0 = cell_off[s], cells = (long)G * K;
    const int32_t *gc = gt_count + gid_off[s], *tc = tr_count + tid_off[s];
    const long row = (long)(side ? tid_off[s] : gid_off[s]) + id;
    int32_t *o_tp = (side ? tr_tp : gt_tp) + row * ASSOC_ALPHAS;
    double *o_num = (side ? tr_num : gt_num) + row * 2 * ASSOC_ALPHAS;
    int32_t *o_top = (side ? tr_top : gt_top) + row * 3;
    const double mine = (double)(side ? tc[id] : gc[id]);
    const long stride = side ? K : 1, first = side ? id : (long)id * K;     // the cell of (id, other) in [G, K]
    for (int a = 0; a < ASSOC_ALPHAS; ++a) {
        const int32_t *mc = matches + ASSOC_ALPHAS * c0 + (long)a * cells + first;
        int tp = 0, partners = 0, top = -1, top_count = 0;
        double ass = 0.0, part = 0.0;
        for (int o = lane; o < n_other; o += 64) {
            const int mi = mc[(long)o * stride];
            const double m = (double)mi, theirs = (double)(side ? gc[o] : tc[o]);
            const double d = mine + theirs - m;
            ass += m * (m / (d > 1.0 ? d : 1.0));
            part += m * (m / (mine > 1.0 ? mine : 1.0));
            tp += mi;
            partners += mi > 0;
            if (mi > top_count) top = o, top_count = mi;            // (ascending ids: a tie keeps the lower one)
        }
        tp = wave_sum_i32(tp);
        ass = assoc_wave_sum_f64(ass);
        part = assoc_wave_sum_f64(part);
        if (a == a0) {
            partners = wave_sum_i32(partners);
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const int oc = __shfl_xor(top_count, off, 64), ot = __shfl_xor(top, off, 64);
                if (oc > top_count || (oc == top_count && oc > 0 && ot < top)) top = ot, top_count = oc;
            }
            if (lane == 0) o_top[0] = partners, o_top[1] = top, o_top[2] = top_count;
        }
        if (lane == 0) {
            o_tp[a] = tp;
            o_num[a] = ass;
            o_num[ASSOC_ALPHAS + a] = part;
        }
    }
}

// One workgroup per frame: the colour of every identity in this frame's column is built in LDS (black, grey for a row
// that is no true positive at alpha_index, else the partner's palette colour), TIMELINE_IDS identities a pass; then the
// cell_w-wide strip of those identities is stored.  Ids are unique within a frame, so no two rows write one entry.
constexpr int TIMELINE_IDS = 8192;

__global__ __launch_bounds__(256) void timeline_kernel(const int32_t *__restrict__ gt_off,
                                                       const int32_t *__restrict__ gt_ids,
                                                       const int32_t *__restrict__ partner_id,
                                                       const int32_t *__restrict__ level, int G, int n_frames,
                                                       int alpha_index, int cell_w, int cell_h, int bgr,
                                                       uint8_t *__restrict__ image) {
    __shared__ int colour[TIMELINE_IDS];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int r0 = gt_off[f], n = gt_off[f + 1] - r0;
    const size_t pitch = (size_t)n_frames * cell_w * 3;
    for (int base = 0; base < G; base += TIMELINE_IDS) {             // (G is uniform: every thread makes every trip)
        const int ids = min(TIMELINE_IDS, G - base);
        for (int i = tid; i < ids; i += 256) colour[i] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += 256) {
            const int g = gt_ids[r0 + i] - base;
            if (g < 0 || g >= ids) continue;
            const int p = partner_id[r0 + i];
            int c = 96 | 96 << 8 | 96 << 16;
            if (level[r0 + i] > alpha_index && p >= 0) {
                c = draw_table_palette(p & 63);
                if (bgr) c = (c & 0xFF00) | (c & 0xFF) << 16 | (c >> 16 & 0xFF);
            }
            colour[g] = c;
        }
        __syncthreads();
        const int per_id = cell_h * cell_w;
        for (long e = tid; e < (long)ids * per_id; e += 256) {
            const int g = (int)(e / per_id), q = (int)(e - (long)g * per_id), y = q / cell_w, x = q - y * cell_w;
            const int c = colour[g];
            uint8_t *px = image + ((size_t)(base + g) * cell_h + y) * pitch + ((size_t)f * cell_w + x) * 3;
            px[0] = (uint8_t)(c & 0xFF), px[1] = (uint8_t)(c >> 8 & 0xFF), px[2] = (uint8_t)(c >> 16 & 0xFF);
        }
        __syncthreads();                            // colour is written again by the next pass
    }
}

// The argument checks the scalar and the per-stream entry points of the bank share, reported under the caller's name:
// 1 = launch, 0 = nothing to do (ok() is set), -code = fail()'s code.
int bank_update_args(const char *who, const clipops_bank_model *model, const clipops_bank *bank, int B, int n_det, int cap,
                     int K, int C, int use_dab) {
    if (B < 0 || n_det < 0 || cap < 0) return -fail(1, who, "negative size");
    if (K < 1 || C < 1) return -fail(1, who, "K < 1 or C < 1");
    if (cap < 1) return -fail(1, who, "a bank without slots");
    if (B == 0) return ok();
    if (!model || !bank) return -fail(1, who, "null pointer");
    for (int i = 0; i < CLIPOPS_BK_N_MODEL; ++i) {
        if (!model->ptr[i]) return -fail(1, who, "null model pointer");
        if (model->row_stride[i] < 0 || model->batch_stride[i] < 0) return -fail(1, who, "negative stride");
    }
    if (!use_dab && (!model->det_embed || model->det_row_stride < 0))
        return -fail(1, who, "det_embed is required without DAB");
    if (!bank->ids || !bank->labels || !bank->disappear_time || !bank->boxes || !bank->ref_pts || !bank->logits ||
        !bank->scores || !bank->output_embed || !bank->long_memory || !bank->last_output || !bank->query_embed ||
        !bank->next_id || !bank->counters || !bank->free_list)
        return -fail(1, who, "null bank pointer");
    return 1;
}

int bank_rows_args(const char *who, const float *boxes, const float *scores, const int64_t *ids, const int64_t *labels,
                   int B, int cap, int K, const int64_t *seq_frame, const float *ori_wh, const float *rows_f,
                   const int64_t *rows_i, const int32_t *counters, int capacity) {
    if (B < 0 || cap < 0 || capacity < 0) return -fail(1, who, "negative size");
    if (K < 1) return -fail(1, who, "K < 1");
    if ((long)B * cap > 0x7fffffffL) return -fail(1, who, "more than 2^31 - 1 slots");
    if ((long)B * cap == 0) return ok();
    if (!boxes || !scores || !ids || !labels || !seq_frame || !ori_wh || !counters ||
        (capacity > 0 && (!rows_f || !rows_i)))
        return -fail(1, who, "null pointer");
    return 1;
}
}  // namespace

extern "C" {
int clipops_result_rows_f32(const float *boxes, const float *scores, const int64_t *ids, const int64_t *labels, int n,
                            int K, int64_t frame, float ori_w, float ori_h, float score_thresh, float area_thresh,
                            float *rows_f, int64_t *rows_i, int32_t *counters, int capacity, void *stream) {
    if (n < 0 || capacity < 0) return fail(1, "clipops_result_rows_f32: negative size");
    if (K < 1) return fail(1, "clipops_result_rows_f32: K < 1");
    if (n == 0) return ok();
    if (!boxes || !scores || !ids || !labels || !counters || (capacity > 0 && (!rows_f || !rows_i)))
        return fail(1, "clipops_result_rows_f32: null pointer");
    return launch("result_rows_kernel", result_rows_kernel, dim3(1), dim3(256), 0, stream, boxes, scores, ids, labels, n, K,
                  frame, ori_w, ori_h, score_thresh, area_thresh, rows_f, rows_i, counters, capacity) ? 3 : 0;
}

int clipops_bank_update_f32(const clipops_bank_model *model, const clipops_bank *bank, int B, int n_det, int cap, int K,
                            int C, int use_dab, float det_score_thresh, float track_score_thresh,
                            int64_t miss_tolerance, void *stream) {
    const char *who = "clipops_bank_update_f32";
    const int todo = bank_update_args(who, model, bank, B, n_det, cap, K, C, use_dab);
    if (todo <= 0) return -todo;
    const BankUpdateScalars th = {det_score_thresh, track_score_thresh, miss_tolerance};
    return launch("bank_update_kernel", bank_update_kernel<BankUpdateScalars>, dim3(B), dim3(BANK_THREADS), 0, stream,
                  *model, *bank, n_det, cap, K, C, use_dab, th) ? 3 : 0;
}

int clipops_bank_update_streams_f32(const clipops_bank_model *model, const clipops_bank *bank, int B, int n_det, int cap,
                                    int K, int C, int use_dab, const float *det_score_thresh,
                                    const float *track_score_thresh, const int64_t *miss_tolerance, void *stream) {
    const char *who = "clipops_bank_update_streams_f32";
    const int todo = bank_update_args(who, model, bank, B, n_det, cap, K, C, use_dab);
    if (todo <= 0) return -todo;
    if (!det_score_thresh || !track_score_thresh || !miss_tolerance) return fail(1, who, "null threshold array");
    const BankUpdatePerStream th = {det_score_thresh, track_score_thresh, miss_tolerance};
    return launch("bank_update_kernel", bank_update_kernel<BankUpdatePerStream>, dim3(B), dim3(BANK_THREADS), 0, stream,
                  *model, *bank, n_det, cap, K, C, use_dab, th) ? 3 : 0;
}

int clipops_bank_result_rows_f32(const float *boxes, const float *scores, const int64_t *ids, const int64_t *labels,
                                 int B, int cap, int K, const int64_t *seq_frame, const float *ori_wh,
                                 float score_thresh, float area_thresh, float *rows_f, int64_t *rows_i,
                                 int32_t *counters, int capacity, void *stream) {
    const char *who = "clipops_bank_result_rows_f32";
    const int todo = bank_rows_args(who, boxes, scores, ids, labels, B, cap, K, seq_frame, ori_wh, rows_f, rows_i,
                                    counters, capacity);
    if (todo <= 0) return -todo;
    const BankRowsScalars th = {score_thresh, area_thresh};
    return launch("bank_result_rows_kernel", bank_result_rows_kernel<BankRowsScalars>, dim3(1), dim3(256), 0, stream,
                  boxes, scores, ids, labels, B * cap, cap, K, seq_frame, ori_wh, th, rows_f, rows_i, counters,
                  capacity) ? 3 : 0;
}

int clipops_bank_result_rows_streams_f32(const float *boxes, const float *scores, const int64_t *ids,
                                         const int64_t *labels, int B, int cap, int K, const int64_t *seq_frame,
                                         const float *ori_wh, const float *score_thresh, const float *area_thresh,
                                         float *rows_f, int64_t *rows_i, int32_t *counters, int capacity, void *stream) {
    const char *who = "clipops_bank_result_rows_streams_f32";
    const int todo = bank_rows_args(who, boxes, scores, ids, labels, B, cap, K, seq_frame, ori_wh, rows_f, rows_i,
                                    counters, capacity);
    if (todo <= 0) return -todo;
    if (!score_thresh || !area_thresh) return fail(1, who, "null threshold array");
    const BankRowsPerStream th = {score_thresh, area_thresh};
    return launch("bank_result_rows_kernel", bank_result_rows_kernel<BankRowsPerStream>, dim3(1), dim3(256), 0, stream,
                  boxes, scores, ids, labels, B * cap, cap, K, seq_frame, ori_wh, th, rows_f, rows_i, counters,
                  capacity) ? 3 : 0;
}

int clipops_draw_table_f32(const float *boxes, const float *scores, const int64_t *ids, int B, int cap, int K,
                           const float *ori_wh, float score_thresh, float area_thresh, int bgr, int font_scale,
                           int32_t *table, void *stream) {
    if (B < 0 || cap < 0) return fail(1, "clipops_draw_table_f32: negative size");
    if (K < 1) return fail(1, "clipops_draw_table_f32: K < 1");
    if (font_scale < 1 || font_scale > 64) return fail(1, "clipops_draw_table_f32: font_scale outside 1 .. 64");
    if ((long)B * cap > 0x7fffffffL) return fail(1, "clipops_draw_table_f32: more than 2^31 - 1 slots");
    if ((long)B * cap == 0) return ok();
    if (!boxes || !scores || !ids || !ori_wh || !table) return fail(1, "clipops_draw_table_f32: null pointer");
    return launch("draw_table_kernel", draw_table_kernel, dim3(B), dim3(BANK_THREADS), 0, stream, boxes, scores, ids, cap,
                  K, ori_wh, score_thresh, area_thresh, bgr ? 1 : 0, font_scale, table) ? 3 : 0;
}

int clipops_clear_events_f64(const double *sim, const int64_t *sim_off, const int32_t *gt_off, const int32_t *tr_off,
                             const int32_t *gt_ids, const int32_t *tr_ids, const int32_t *seq_off, int n_seqs,
                             const int32_t *n_gt_ids, int max_gt, int max_tr, int max_gt_ids, int32_t *gt_partner,
                             int32_t *gt_flags, int32_t *tr_partner, int32_t *counts, int32_t *status, void *stream) {
    const char *who = "clipops_clear_events_f64";
    if (n_seqs < 0 || max_gt < 0 || max_tr < 0 || max_gt_ids < 0) return fail(1, who, "negative size");
    if (max_gt > CLIPOPS_EVENTS_MAX_DIM || max_tr > CLIPOPS_EVENTS_MAX_DIM || max_gt_ids > CLIPOPS_EVENTS_MAX_DIM)
        return fail(2, who, "a frame or an id count exceeds CLIPOPS_EVENTS_MAX_DIM = 2048");
    if (n_seqs == 0) return ok();
    if (!sim || !sim_off || !gt_off || !tr_off || !gt_ids || !tr_ids || !seq_off || !n_gt_ids || !gt_partner ||
        !gt_flags || !tr_partner || !counts || !status)
        return fail(1, who, "null pointer");
    static std::atomic<unsigned long long> allowed{0};
    const size_t lds = events_lds_bytes(max_gt, max_tr, max_gt_ids);    // (at most 126 KiB at the largest sizes)
    if (allow_lds(reinterpret_cast<const void *>(clear_events_kernel), lds, allowed)) return 3;
    return launch("clear_events_kernel", clear_events_kernel, dim3(n_seqs), dim3(64), lds, stream, sim, sim_off, gt_off,
                  tr_off, gt_ids, tr_ids, seq_off, n_gt_ids, max_gt, max_tr, max_gt_ids,
                  max_gt < max_tr ? max_gt : max_tr, gt_partner, gt_flags, tr_partner, counts, status) ? 3 : 0;
}

int clipops_error_table_f64(const double *gt_boxes, const double *tr_boxes, const int32_t *gt_off, const int32_t *tr_off,
                            const int32_t *gt_ids, const int32_t *tr_ids, const int32_t *gt_kind, const int32_t *tr_kind,
                            int n_frames, int max_rows, int width, int height, int bgr, int font_scale, int32_t *table,
                            void *stream) {
    const char *who = "clipops_error_table_f64";
    if (n_frames < 0 || max_rows < 0) return fail(1, who, "negative size");
    if (width < 1 || height < 1 || width > 65535 || height > 65535) return fail(1, who, "width or height outside 1 .. 65535");
    if (font_scale < 1 || font_scale > 64) return fail(1, who, "font_scale outside 1 .. 64");
    if ((long)n_frames * max_rows > 0x7fffffffL) return fail(1, who, "more than 2^31 - 1 table rows");
    if ((long)n_frames * max_rows == 0) return ok();
    if (!gt_boxes || !tr_boxes || !gt_off || !tr_off || !gt_ids || !tr_ids || !gt_kind || !tr_kind || !table)
        return fail(1, who, "null pointer");
    return launch("error_table_kernel", error_table_kernel, dim3(n_frames), dim3(256), 0, stream, gt_boxes, tr_boxes,
                  gt_off, tr_off, gt_ids, tr_ids, gt_kind, tr_kind, max_rows, width, bgr ? 1 : 0, font_scale, table) ? 3 : 0;
}

int clipops_bdd_cross_class_f64(const double *gt_boxes, const double *tr_boxes, const int32_t *gt_classes,
                                const int32_t *tr_classes, const int32_t *gt_off, const int32_t *tr_off,
                                const int32_t *gt_kind, const int32_t *tr_kind, int n_frames, int max_gt, int max_tr,
                                int32_t *gt_partner, int32_t *gt_class, double *gt_iou, int32_t *tr_partner,
                                int32_t *tr_class, double *tr_iou, int32_t *status, void *stream) {
    const char *who = "clipops_bdd_cross_class_f64";
    if (n_frames < 0 || max_gt < 0 || max_tr < 0) return fail(1, who, "negative size");
    if (max_gt > CLIPOPS_EVENTS_MAX_DIM || max_tr > CLIPOPS_EVENTS_MAX_DIM)
        return fail(2, who, "a candidate count exceeds CLIPOPS_EVENTS_MAX_DIM = 2048");
    if (n_frames == 0) return ok();
    if (!gt_boxes || !tr_boxes || !gt_classes || !tr_classes || !gt_off || !tr_off || !gt_kind || !tr_kind ||
        !gt_partner || !gt_class || !gt_iou || !tr_partner || !tr_class || !tr_iou || !status)
        return fail(1, who, "null pointer");
    static std::atomic<unsigned long long> allowed{0};
    const size_t lds = cross_lds_bytes(max_gt, max_tr);                 // (at most 132 KiB at the largest sizes)
    if (allow_lds(reinterpret_cast<const void *>(bdd_cross_class_kernel), lds, allowed)) return 3;
    return launch("bdd_cross_class_kernel", bdd_cross_class_kernel, dim3(n_frames), dim3(64), lds, stream, gt_boxes,
                  tr_boxes, gt_classes, tr_classes, gt_off, tr_off, gt_kind, tr_kind, max_gt, max_tr,
                  max_gt < max_tr ? max_gt : max_tr, gt_partner, gt_class, gt_iou, tr_partner, tr_class, tr_iou,
                  status) ? 3 : 0;
}

int clipops_hota_events_f64(const double *sim, const int64_t *sim_off, const int32_t *gt_off, const int32_t *tr_off,
                            const int32_t *gt_ids, const int32_t *tr_ids, const int32_t *frame_seq, int n_frames,
                            const int32_t *n_tr_ids, const int64_t *cell_off, const double *alignment,
                            const double *alphas, int max_gt, int max_tr, int32_t *gt_partner, int32_t *gt_level,
                            int32_t *tr_partner, int32_t *tr_level, int32_t *matches, int32_t *status, void *stream) {
    const char *who = "clipops_hota_events_f64";
    if (n_frames < 0 || max_gt < 0 || max_tr < 0) return fail(1, who, "negative size");
    if (max_gt > CLIPOPS_EVENTS_MAX_DIM || max_tr > CLIPOPS_EVENTS_MAX_DIM)
        return fail(2, who, "a frame exceeds CLIPOPS_EVENTS_MAX_DIM = 2048");
    if (n_frames == 0) return ok();
    if (!sim || !sim_off || !gt_off || !tr_off || !gt_ids || !tr_ids || !frame_seq || !n_tr_ids || !cell_off ||
        !alignment || !alphas || !gt_partner || !gt_level || !tr_partner || !tr_level || !status)
        return fail(1, who, "null pointer");
    AssocAlphas a;
    for (int i = 0; i < ASSOC_ALPHAS; ++i) a.v[i] = alphas[i];
    static std::atomic<unsigned long long> allowed{0};
    const size_t lds = assoc_solve_lds_bytes(max_gt, max_tr);           // (at most 100 KiB at the largest sizes)
    if (allow_lds(reinterpret_cast<const void *>(hota_events_kernel), lds, allowed)) return 3;
    return launch("hota_events_kernel", hota_events_kernel, dim3(n_frames), dim3(64), lds, stream, sim, sim_off, gt_off,
                  tr_off, gt_ids, tr_ids, frame_seq, n_tr_ids, cell_off, alignment, a, max_gt, max_tr,
                  max_gt < max_tr ? max_gt : max_tr, gt_partner, gt_level, tr_partner, tr_level, matches, status) ? 3 : 0;
}

int clipops_identity_pairs_i32(int n_seqs, const int32_t *n_gt_ids, const int32_t *n_tr_ids, const int64_t *cell_off,
                               const int32_t *gid_off, const int32_t *tid_off, const int32_t *gt_count,
                               const int32_t *tr_count, const int32_t *id_matches, int max_ids, int32_t *gt_id_partner,
                               int32_t *gt_idtp, int32_t *tr_id_partner, int32_t *tr_idtp, int32_t *status,
                               void *stream) {
    const char *who = "clipops_identity_pairs_i32";
    if (n_seqs < 0 || max_ids < 0) return fail(1, who, "negative size");
    if (max_ids > CLIPOPS_EVENTS_MAX_DIM)
        return fail(2, who, "ground-truth plus tracker ids of a sequence exceed CLIPOPS_EVENTS_MAX_DIM = 2048");
    if (n_seqs == 0) return ok();
    if (!n_gt_ids || !n_tr_ids || !cell_off || !gid_off || !tid_off || !gt_count || !tr_count || !id_matches ||
        !gt_id_partner || !gt_idtp || !tr_id_partner || !tr_idtp || !status)
        return fail(1, who, "null pointer");
    static std::atomic<unsigned long long> allowed{0};
    const size_t lds = assoc_solve_lds_bytes(max_ids, max_ids);
    if (allow_lds(reinterpret_cast<const void *>(identity_pairs_kernel), lds, allowed)) return 3;
    return launch("identity_pairs_kernel", identity_pairs_kernel, dim3(n_seqs), dim3(64), lds, stream, n_gt_ids, n_tr_ids,
                  cell_off, gid_off, tid_off, gt_count, tr_count, id_matches, max_ids, gt_id_partner, gt_idtp,
                  tr_id_partner, tr_idtp, status) ? 3 : 0;
}

int clipops_assoc_reduce_f64(int n_seqs, const int32_t *n_gt_ids, const int32_t *n_tr_ids, const int64_t *cell_off,
                             const int32_t *gid_off, const int32_t *tid_off, const int32_t *gt_count,
                             const int32_t *tr_count, const int32_t *matches, int max_side_ids, int alpha_index,
                             int32_t *gt_tp, double *gt_num, int32_t *gt_top, int32_t *tr_tp, double *tr_num,
                             int32_t *tr_top, void *stream) {
    const char *who = "clipops_assoc_reduce_f64";
    if (n_seqs < 0 || max_side_ids < 0) return fail(1, who, "negative size");
    if (alpha_index < 0 || alpha_index >= CLIPOPS_ASSOC_ALPHAS) return fail(1, who, "alpha_index outside 0 .. 18");
    if (n_seqs > 65535) return fail(2, who, "more than 65535 sequences in one call");
    if (max_side_ids > CLIPOPS_EVENTS_MAX_DIM)
        return fail(2, who, "the ids of a sequence exceed CLIPOPS_EVENTS_MAX_DIM = 2048");
    if (n_seqs == 0 || max_side_ids == 0) return ok();
    if (!n_gt_ids || !n_tr_ids || !cell_off || !gid_off || !tid_off || !gt_count || !tr_count || !matches || !gt_tp ||
        !gt_num || !gt_top || !tr_tp || !tr_num || !tr_top)
        return fail(1, who, "null pointer");
    return launch("assoc_reduce_kernel", assoc_reduce_kernel, dim3(max_side_ids, n_seqs, 2), dim3(64), 0, stream,
                  n_gt_ids, n_tr_ids, cell_off, gid_off, tid_off, gt_count, tr_count, matches, alpha_index, gt_tp, gt_num,
                  gt_top, tr_tp, tr_num, tr_top) ? 3 : 0;
}

int clipops_timeline_u8(const int32_t *gt_off, const int32_t *gt_ids, const int32_t *partner_id, const int32_t *level,
                        int n_ids, int n_frames, int alpha_index, int cell_w, int cell_h, int bgr, uint8_t *image,
                        void *stream) {
    const char *who = "clipops_timeline_u8";
    if (n_ids < 0 || n_frames < 0) return fail(1, who, "negative size");
    if (cell_w < 1 || cell_h < 1) return fail(1, who, "cell_w or cell_h below 1");
    if (alpha_index < 0 || alpha_index >= CLIPOPS_ASSOC_ALPHAS) return fail(1, who, "alpha_index outside 0 .. 18");
    if ((long)n_ids * cell_h > 65535 || (long)n_frames * cell_w > 65535)
        return fail(2, who, "the image exceeds 65535 pixels on a side");
    if (n_ids == 0 || n_frames == 0) return ok();
    if (!gt_off || !gt_ids || !partner_id || !level || !image) return fail(1, who, "null pointer");
    return launch("timeline_kernel", timeline_kernel, dim3(n_frames), dim3(256), 0, stream, gt_off, gt_ids, partner_id,
                  level, n_ids, n_frames, alpha_index, cell_w, cell_h, bgr ? 1 : 0, image) ? 3 : 0;
}
}  // extern "C"
