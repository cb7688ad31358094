// msda_hip.hip -- multi-scale deformable attention for gfx950 (MI355X, CDNA4).
//
// Hand-written HIP; wave64, LDS-staged sampling records, buffer (SRSRC) gathers with
// hardware zero padding, DPP reductions, fixed-point LDS accumulation, hardware f32 atomics.
// No CUDA-compat layer.
//
// Semantics replaced (reference repository paths):
//   forward   models/ops/src/cuda/ms_deform_im2col_cuda.cuh:237-299 (+ bilinear :33-84)
//   backward  models/ops/src/cuda/ms_deform_im2col_cuda.cuh:301-403 (+ bilinear :87-159)
//   host side models/ops/src/cuda/ms_deform_attn_cuda.cu:20-153
//   fused prologue (msda_fused_*): models/ops/modules/ms_deform_attn.py:104-123 -- softmax over the L*P
//             logits, sampling locations from offsets + reference points, padding-mask fill of `value`
// C ABI: include/msda_hip.h.  Design notes, byte counts and rooflines: DESIGN.md.
//
// Sources: this file holds the host side's plans, the selector, the options and the C ABI; which kernels a call takes
// is msda_dispatch_fwd.h / msda_dispatch_bwd.h (one function per path, the drivers at their ends); the kernels live
// in msda_generic.h (any D / dtype), msda_fwd_gather.h (D = 32 through the vector L1), msda_fwd_win.h (pyramid
// self-attention forward, LDS windows), msda_tile.h + msda_bwd_tile_lv.h / msda_bwd_bins.h (pyramid backward),
// msda_bwd_rows.h (decoder-shaped backward), msda_fused_side.h (Jacobian side kernels), msda_select.h (statistics).
//
// Variant numbers (msda_set_option "fwd_variant" / "bwd_variant"; 0 = auto):
//   forward : 0 auto (fp32 pyramid self-attention with host shapes: 12 unless "fwd_win_auto" is 0 or the selector asks
//             for the gather; other D = 32 calls: 3) | 1 generic | 2,3,4 d32 gather with 2,4,1 points in flight |
//             12 msda_fwd_d32_win (msda_fwd_win.h): (batch, head, region) per workgroup, windows of levels 1-3 filled
//             by LDS-DMA around the measured mean offset, level 0 through the vector L1, pixel-pair LDS reads, one
//             head per XCD
//   backward: 0 auto (pyramid self-attention: 12, or rows / 10 by selector level and call form; other D = 32 calls:
//             msda_bwd_d32_rows, 32 lanes per row) | 1 generic | 10 region-tiled fixed-point windows, one pyramid
//             level per workgroup | 12 counting sort + register gather (msda_bwd_bins.h) | 13 global sort + gather
//             through a workspace, no fabric atomics (msda_bwd_sorted.h; selector level 2 when the caller gave scratch)
//   (rounds 1-2 also had a hybrid LDS/L1 forward -- 8, 9 -- and an all-levels-per-workgroup backward -- 8, 9, 11:
//    measured slower than what replaced them, DESIGN.md 4.1 / 4.2, and removed in round 5; those numbers now mean 0)
//
// Kernel families
//   *_generic   any D/L/P, f32 / f64 / bf16 storage: one thread per output scalar
//               (forward) or one block per (n,q,m) row (backward).  Correctness path for
//               shapes the specialised kernels do not cover (reference gradcheck sizes
//               D in {30,64,71,1025,...}).
//   *_d32_win / *_d32_tile_* / *_d32_rows   region- or row-organised specialisations, described at their definitions
//               (msda_fwd_win.h, below, msda_bwd_rows.h)
//   *_d32       MeMOTR geometry (D = 32 channels/head): the lanes that own one (n,q,m) row hold its
//               32 channels (8 lanes x 4 fp32 channels, 4 lanes x 8 bf16 channels).  Each lane prepares
//               the sampling record of a share of the row's L*P points exactly once, parks it in LDS, and the
//               lanes of the row then stream the records back as broadcast ds_read_b128.  Corner reads
//               are 16-byte buffer loads; invalid corners carry an out-of-range offset so the buffer unit
//               returns zeros (= the reference's per-corner zero padding, no divergent branches).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../include/msda_hip.h"
#include "msda_common.h"
#include "msda_select.h"

namespace {

using namespace msda;

template <typename T>
__device__ __forceinline__ void atomic_add_hw(T *p, T v) {
    unsafeAtomicAdd(p, v);  // global_atomic_add_f32 / _f64, no CAS loop
}

__device__ __forceinline__ float t_exp(float x) { return expf(x); }
__device__ __forceinline__ double t_exp(double x) { return exp(x); }

#include "msda_generic.h"
#include "msda_fwd_gather.h"
#include "msda_tile.h"
#include "msda_bwd_tile_lv.h"
#include "msda_fused_side.h"
#include "msda_fwd_win.h"
#include "msda_bwd_rows.h"
#include "msda_bwd_bins.h"
#include "msda_bwd_sorted.h"
#include "msda_attn_map.h"

// ----------------------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------------------
thread_local char g_err[256] = {0};
thread_local const char *g_kernel = "";

std::atomic<int> opt_fwd_variant{0}, opt_bwd_variant{0};
std::atomic<int> opt_fwd_block{256}, opt_bwd_block{256};
std::atomic<int> opt_fwd_grid_mult{32}, opt_bwd_grid_mult{16};
// (backward margin 4, round 3: +1 % at the initialisation's offsets, -21 / -37 % when they are 1.5x / 2x larger,
//  profiles/r03_bwd_margin_sweep.txt)
std::atomic<int> opt_bwd_tile_margin{4};
std::atomic<int> opt_bwd_split{1};        // fused backward with a workspace: prologue kernel + plain tiled kernel + finish kernel
std::atomic<int> opt_bwd_wide_log2{12};   // tiled backward: row-magnitude range (log2) that makes a region "wide"; 0 = off
std::atomic<int> opt_bwd_ablate{0};       // profiling only: drop parts of the tiled backward (results are then wrong)
std::atomic<int> opt_bwd_rows_block{0};   // threads per workgroup of msda_bwd_d32_rows (0: by problem size)
std::atomic<int> opt_bwd_bins_strip{4};   // counting-sort backward: region rows per strip of the block -> region walk
std::atomic<int> opt_bwd_bins_margin{6};     // small-margin level (level 0 of the selector)
std::atomic<int> opt_bwd_bins_margin_hi{9};  // large-margin level (level 1): the largest window that keeps 5 workgroups per CU
std::atomic<int> opt_deterministic{0};       // 1: the forward keeps ONE summation order whatever the statistics say (pyramid: the windowed kernel)
std::atomic<int> opt_auto_select{1};         // msda_select.h: follow the measured off-window share (0: level 0 always)
std::atomic<int> opt_sel_level{-1};          // >= 0: pin the selector's level (tests, benchmarks)
// backward thresholds, 1/1000 of the valid corners.  Level 2 is the sorted backward when the caller provides scratch
// (0.21-0.28 ms at every offset scale, profiles/r06_sorted_probe.txt: it overtakes the large-margin windows once ~0.2 % of
// the corners leave them) and the rows kernel's float atomics otherwise (0.5-1.1 ms: only past 10 %)
std::atomic<int> opt_sel_up0{5}, opt_sel_up1{2}, opt_sel_down1{2}, opt_sel_down2{1};
std::atomic<int> opt_sel_up1_rows{100}, opt_sel_down2_rows{60};
std::atomic<int> opt_sel_fwd_up{50}, opt_sel_fwd_down{20};                                  // forward thresholds  // counting-sort backward: window margin (the window is only a table of counters)
std::atomic<int> opt_bwd_soft{1};         // fused counting-sort backward: softmax + its Jacobian in the kernel when the caller passes the forward's output
std::atomic<int> opt_bwd_sorted{1};       // selector level 2: grad_value by sort + gather when the caller gave scratch (0: the rows kernel)
std::atomic<int> opt_bwd_sort_qc{0}, opt_bwd_sort_emult{0};   // sorted backward: queries per dots workgroup / chunks per emit workgroup (0: auto)
std::atomic<int> opt_bwd_rows{1};         // 0: few-query D = 32 calls keep the generic row-per-block backward
std::atomic<int> opt_fwd_head_major{0};    // gather forward: head-major task walk (one head per XCD)
std::atomic<int> opt_fwd_win_rlog{0};       // windowed forward: log2 of the region height on level 0 (0: auto)
std::atomic<int> opt_fwd_win_rlogx{0};      // log2 of the region width (at least the height; 0: as the height)
std::atomic<int> opt_fwd_win_bf16{0};       // 1: bf16 rows take the windowed forward too (built and measured in round 6: 51.0 vs 49.2 us
                                            // for the gather kernel, fp32 windows 45.6 -- profiles/r06_bf16_fwd_probe.txt; default: the gather)
std::atomic<int> opt_fwd_win_auto{1};       // 0: never pick the windowed forward on its own
std::atomic<int> opt_fwd_win_block{0};      // threads per workgroup (128 / 256 / 384 / 512; 0: auto)
std::atomic<int> opt_fwd_win_l0{1};         // first level served from an LDS window
std::atomic<int> opt_fwd_win_margins{0x3333};  // window margin per level, 4 bits each (level 0 in the low nibble)
std::atomic<int> opt_fwd_win_ablate{0};     // profiling only
std::atomic<int> opt_fwd_win_place{0};      // 1: measured window placement in every workgroup (rounds 3-4)
std::atomic<int> opt_fwd_win_grid{1};       // 1: the default shape may become equal regions of any size when that fills the slots in fewer rounds (0: never)
std::atomic<int> opt_fwd_win_rsy{0}, opt_fwd_win_rsx{0};   // region height / width on level 0 in pixels: grid mode with exactly this size (0: by estimate)
std::atomic<int> opt_fwd_win_wps{0};        // 3 / 4: force the 168- / 128-register build; 2 (256 threads): the 256-register build
std::atomic<int> opt_fwd_win_early{9};      // 0 / 2 / 4: level-0 points requested before the LDS phase (else: by register budget)
constexpr int kWinEarlyW4 = 0;              // ... of the 128-register build (0 and 2 time the same; 0 needs 107 registers, no spill)
std::atomic<int> opt_bwd_side_rows{1};      // slim split backward: side kernels with one lane per (query, head) row (0: one lane per point)
std::atomic<int> opt_fwd_win_trace_lo{0}, opt_fwd_win_trace_hi{0};   // profiling: device address of the timeline buffer (31 + 31 bits)

int fail(int code, const char *msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

int check_launch(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    g_err[0] = 0;
    return MSDA_OK;
}

int check_dims(const void *a, const void *b, const void *c, const void *d, const void *e, const void *f, int N, int S,
               int M, int D, int L, int Lq, int P) {
    if (!a || !b || !c || !d || !e || !f) return fail(MSDA_EINVAL, "null pointer argument");
    if (N < 0 || Lq < 0) return fail(MSDA_EINVAL, "negative batch/query count");
    if (S <= 0 || M <= 0 || D <= 0 || L <= 0 || P <= 0) return fail(MSDA_EINVAL, "non-positive dimension");
    // the reference kernels index with 32-bit ints (.cuh:255-270); keep the same envelope, loudly
    const double lim = 2147483647.0;
    if ((double)N * S * M * D > lim || (double)N * Lq * M * L * P * 2 > lim || (double)N * Lq * M * D > lim)
        return fail(MSDA_ERANGE, "tensor exceeds 2^31 elements");
    return MSDA_OK;
}

int clamp_grid(long want, int mult) {
    long cap = (long)kNumCU * (mult > 0 ? mult : 8);
    if (want < 1) want = 1;
    return (int)(want < cap ? want : cap);
}

// the specialised kernels address `value` (and the fp32 grad_value) with 32-bit byte offsets
bool d32_ok(int D, int L, long value_elems) { return D == 32 && L <= kMaxLevels && value_elems * 4 < 0x7fffff00L; }

// Plan the region tiling from the HOST copy of the level shapes.  Returns false when the tiled
// kernels do not apply (then the gather / generic kernels run).  Levels below `l0` get no window.
bool make_tile_plan(TilePlan &pl, const int64_t *shapes_host, int N, int S, int M, int D, int L, int Lq, int P,
                    long value_bytes, int margin, int l0, size_t lds_rows_extra, size_t fixed_lds, size_t &lds,
                    bool check_lds = true) {
    if (!shapes_host || D != 32 || L < 1 || L > kTileMaxL || Lq != S || L * P > kMaxFusedLP) return false;
    if (margin < 0) margin = 0;
    if (l0 < 0) l0 = 0;
    if (l0 > L) l0 = L;
    memset(&pl, 0, sizeof(pl));
    pl.N = N; pl.S = S; pl.M = M; pl.L = L; pl.P = P; pl.Lq = Lq; pl.l0 = l0;
    pl.value_bytes = (unsigned)value_bytes;
    long q = 0;
    int rows = 0, px = 0, RY = 0, RX = 0;
    for (int l = 0; l < kTileMaxL; ++l) {
        if (l < L) {
            const long H = shapes_host[2 * l], W = shapes_host[2 * l + 1];
            if (H <= 0 || W <= 0 || H > 32767 || W > 32767 || W * M >= (1L << 23)) return false;
            const int sh = L - 1 - l, side = 1 << sh;
            int win = side + 2 * margin;
            if (win > 32) win = 32;
            if (l < l0) win = 0;
            pl.H[l] = (int)H; pl.W[l] = (int)W; pl.qstart[l] = (int)q; pl.shift[l] = sh; pl.row0[l] = rows;
            pl.win[l] = win; pl.win_base[l] = px;
            int magic = 65537;
            if (win > 0) {
                magic = 65536 / win + 1;
                for (int x = 0; x < win * win; ++x)
                    if (((x * magic) >> 16) != x / win) return false;
            }
            pl.win_magic[l] = magic;
            q += H * W; rows += side * side; px += win * win;
            const int ry = (int)((H + side - 1) / side), rx = (int)((W + side - 1) / side);
            RY = ry > RY ? ry : RY;
            RX = rx > RX ? rx : RX;
        } else {  // inert padding so that table loads stay in range
            pl.H[l] = 1; pl.W[l] = 1; pl.qstart[l] = (int)q; pl.shift[l] = 0; pl.row0[l] = rows;
            pl.win[l] = 0; pl.win_magic[l] = 65537; pl.win_base[l] = px;
        }
    }
    if (q != S) return false;  // host shapes do not describe this value tensor
    if (px + (int)lds_rows_extra >= 65535) return false;    // window cells travel as 16-bit indices
    pl.row0[kTileMaxL] = rows; pl.win_base[kTileMaxL] = px;
    for (int l = L; l <= kTileMaxL; ++l) { pl.row0[l] = rows; pl.win_base[l] = px; }
    pl.rows = rows; pl.RY = RY; pl.RX = RX;
    if (rows > kTileMaxRows) return false;
    const long nb = (long)N * RY * RX * M;
    if (nb > (1L << 30)) return false;
    pl.n_blocks = (int)nb;
    lds = ((size_t)px + lds_rows_extra) * 128 + fixed_lds;
    return !check_lds || lds <= 160 * 1024 - 2048;
}

// LDS layout of msda_bwd_d32_bins (msda_bwd_bins.h) for `ni` items per thread; false when the call does not fit.
bool make_bins_plan(BinsPlan &bp, const TilePlan &pl, int ni, size_t &lds) {
    const int P = pl.P, n_items = pl.rows * P;
    if (P < 1 || n_items < 1 || n_items > kTileThreads * ni) return false;
    const int magic = 65536 / P + 1;
    for (int i = 0; i < kTileThreads * ni; ++i)
        if (((i * magic) >> 16) != i / P) return false;
    int win_max = 0;
    for (int l = 0; l < pl.L; ++l) win_max = pl.win[l] > win_max ? pl.win[l] : win_max;
    const int ncell = win_max * win_max;
    const int C = (((ncell + 63) / 64) + 3) & ~3;
    auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    size_t o = up16((size_t)(pl.rows + 1) * kBinsGRow);
    bp.n_items = n_items;
    bp.magic_p = magic;
    bp.scan_c = C;
    bp.strip = opt_bwd_bins_strip.load() > 0 ? opt_bwd_bins_strip.load() : 1;
    bp.o_x = (unsigned)o;                       // records + flags, later the sorted entries
    bp.o_fl = (unsigned)(o + (size_t)n_items * 16);
    const size_t rec_bytes = up16((size_t)n_items * 20), ent_bytes = up16((size_t)(4 * n_items + 1) * 8);
    o += rec_bytes > ent_bytes ? rec_bytes : ent_bytes;
    // union: ticket counters + row tables (dead after the sort) | flush transpose
    bp.o_st = (unsigned)o;
    bp.o_cnt = (unsigned)o;
    bp.o_rowp = (unsigned)(o + (size_t)C * 64 * 4);
    bp.o_rowa = (unsigned)(bp.o_rowp + up16((size_t)(pl.rows + 1) * 4));
    bp.o_rowq = (unsigned)(bp.o_rowa + up16((size_t)(pl.rows + 1) * 4));
    const size_t tab_bytes = (size_t)C * 64 * 4 + 3 * up16((size_t)(pl.rows + 1) * 4);
    const size_t st_bytes = (size_t)(kTileThreads / 64) * kBinsStageWave;
    o += tab_bytes > st_bytes ? tab_bytes : st_bytes;
    bp.o_start = (unsigned)o;
    o += up16((size_t)C * 64 * 2);
    bp.o_comp = (unsigned)o;
    o += (size_t)C * 64 * 4;
    bp.o_misc = (unsigned)o;
    o += 16 + (size_t)(kTileThreads / 64) * 16 * 4 + 16;
    o = up16(o);
    bp.o_dot = (unsigned)o;                     // (soft) <grad_out_row, out_row> per staged row
    o += up16((size_t)(pl.rows + 1) * 4);
    lds = o;
    return lds <= 64 * 1024;
}

// ---- grid mode of the windowed forward: which region size, if any ----
// Estimate of a launch in "row units": a workgroup costs kWinPrologueRows + its rows, the workgroups of one XCD (an eighth
// of the launch: head-major numbering, one contiguous run per XCD) are handed to its 64 slots (32 CUs x two 512-thread
// workgroups) in dispatch order as slots free up.  The power-of-two plan's partial border regions come last; equal
// regions all cost the same.  Grid mode is taken when its best size is at least 7 % faster by this estimate AND keeps two
// workgroups per CU (LDS); the choice is cached per geometry.
constexpr int kWinPrologueRows = 140;      // (prologue ~ 10 of the 34 us a 340-row workgroup takes under load)

inline double win_makespan(const std::vector<int> &dur_one, long repeats, int slots) {
    std::vector<double> free_at((size_t)slots, 0.0);      // a binary heap by hand would be faster; this runs once per geometry
    double end = 0.0;
    for (long r = 0; r < repeats; ++r)
        for (int d : dur_one) {
            size_t k = 0;
            for (size_t i = 1; i < free_at.size(); ++i)
                if (free_at[i] < free_at[k]) k = i;
            free_at[k] += (double)(kWinPrologueRows + d);
            end = free_at[k] > end ? free_at[k] : end;
        }
    return end;
}

struct WinGridChoice {
    long key[12];
    int rsy, rsx;
};

inline void win_grid_choice(const WinPlan &p2, const int64_t *shapes_host, int N, int S, int M, int D, int L, int Lq, int P,
                            long value_bytes, int lwin0, const int *margins, int threads, int margin_bits, int &rsy,
                            int &rsx) {
    rsy = rsx = 0;
    if (L < 1 || L > kWinMaxL || (M % 8) != 0) return;
    static std::mutex mu;
    static std::vector<WinGridChoice> cache;
    WinGridChoice c;
    memset(&c, 0, sizeof(c));
    for (int l = 0; l < L; ++l) { c.key[2 * l] = shapes_host[2 * l]; c.key[2 * l + 1] = shapes_host[2 * l + 1]; }
    c.key[8] = N; c.key[9] = M; c.key[10] = ((long)L << 40) | ((long)P << 32) | ((long)lwin0 << 24) | (long)margin_bits;
    c.key[11] = threads;
    {
        std::lock_guard<std::mutex> g(mu);
        for (const WinGridChoice &e : cache)
            if (!memcmp(e.key, c.key, sizeof(c.key))) { rsy = e.rsy; rsx = e.rsx; return; }
    }
    const int slots = 64;
    const long per_xcd = (long)N * M / 8;              // (head, image) pairs per XCD
    // the power-of-two plan in its dispatch order: complete regions, right border column, bottom border row
    std::vector<int> d2;
    {
        auto rows_of = [&](int ry, int rx) {
            int rows = 0;
            for (int l = 0; l < L; ++l) {
                const int sy = p2.shy[l], sx = p2.shx[l];
                int hv = p2.H[l] - (ry << sy), wv = p2.W[l] - (rx << sx);
                hv = hv > (1 << sy) ? (1 << sy) : (hv < 0 ? 0 : hv);
                wv = wv > (1 << sx) ? (1 << sx) : (wv < 0 ? 0 : wv);
                rows += hv * wv;
            }
            return rows;
        };
        for (int ry = 0; ry < p2.RYf; ++ry) for (int rx = 0; rx < p2.RXf; ++rx) d2.push_back(rows_of(ry, rx));
        for (int ry = 0; ry < p2.RYf; ++ry) for (int rx = p2.RXf; rx < p2.RX; ++rx) d2.push_back(rows_of(ry, rx));
        for (int ry = p2.RYf; ry < p2.RY; ++ry) for (int rx = 0; rx < p2.RX; ++rx) d2.push_back(rows_of(ry, rx));
    }
    const double cost2 = win_makespan(d2, per_xcd, slots);
    double best = cost2 * 0.93;
    const long H0 = shapes_host[0], W0 = shapes_host[1];
    for (int ty = 4; ty <= 40; ++ty)
        for (int tx = 4; tx <= 32; ++tx) {
            const long nreg = ((H0 + ty - 1) / ty) * ((W0 + tx - 1) / tx);
            if (nreg * per_xcd < slots / 2) continue;                   // too few workgroups to fill the XCD at all
            // a lower bound before the plan: all regions at most ty tx (1 + 1/4 + 1/16 + 1/64) rows
            WinPlan g;
            size_t glds = 0;
            if (!make_win_plan_grid(g, shapes_host, N, S, M, D, L, Lq, P, value_bytes, ty, tx, lwin0, margins, threads, glds,
                                    4))
                continue;
            if (glds + 512 > 80 * 1024) continue;                       // two workgroups per CU, as the default shape
            const long w = nreg * per_xcd;
            const double cost = (double)((w + slots - 1) / slots) * (double)(kWinPrologueRows + g.rows);
            if (cost < best) { best = cost; rsy = ty; rsx = tx; }
        }
    c.rsy = rsy; c.rsx = rsx;
    std::lock_guard<std::mutex> g(mu);
    if (cache.size() >= 64) cache.erase(cache.begin());
    cache.push_back(c);
}

// Dynamic LDS above 64 KiB needs an opt-in per kernel; do it once per kernel and device for the full
// 160 KiB (the call costs host time, too much to repeat per launch).
template <typename K>
int allow_big_lds(K kernel, size_t lds) {
    if (lds <= 64 * 1024) return MSDA_OK;
    static std::atomic<unsigned long long> done{0};   // one bit per device ordinal (per template instance)
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return MSDA_OK;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 2048);
    if (e != hipSuccess) return fail((int)e, hipGetErrorString(e));
    done.fetch_or(bit, std::memory_order_release);
    return MSDA_OK;
}

// ---- msda_select.h, host side: the records and their table ----
SelSlot g_sel[kSelSlots];
std::mutex g_sel_mu;
unsigned long long *g_sel_pool_dev[64] = {nullptr};     // per device ordinal: kSelSlots records, one allocation
unsigned long long *g_sel_pool_host[64] = {nullptr}, *g_sel_pool_host_dev[64] = {nullptr};
bool g_sel_pool_failed[64] = {false};
unsigned long long g_sel_clock = 0, g_sel_tick = 0;
thread_local unsigned long long g_site = 0;
// msda_next_value_pixel_stride: elements between two pixels of `value` (and of `grad_value`) for the NEXT forward /
// backward call of this thread (0: contiguous, M * D).  Every compute entry point takes (reads and clears) it as its first
// statement and hands it down in the Call; nothing below the entry points reads it.
thread_local long g_value_stride = 0;
inline long take_value_stride() {
    const long v = g_value_stride;
    g_value_stride = 0;
    return v;
}
thread_local int g_sel_level = 0;           // level of this thread's last selected call (msda_selector_last)
thread_local float g_sel_frac = -1.f, g_sel_inner = -1.f;

bool stream_capturing(hipStream_t stream) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) != hipSuccess) {
        (void)hipGetLastError();
        return true;
    }
    return cs != hipStreamCaptureStatusNone;
}

// The device's block of records: ONE hipMalloc + one hipHostMalloc per device for the life of the process, made at the
// first call that is not inside a stream capture (allocation is not capturable).  g_sel_mu held.
bool sel_pool(int dev, hipStream_t stream) {
    const int d = dev & 63;
    if (g_sel_pool_dev[d]) return true;
    if (g_sel_pool_failed[d] || stream_capturing(stream)) return false;
    unsigned long long *pd = nullptr, *ph = nullptr, *phd = nullptr;
    const size_t dbytes = (size_t)kSelSlots * kSelDevWords * 8, hbytes = (size_t)kSelSlots * kSelHostWords * 8;
    if (hipMalloc((void **)&pd, dbytes) != hipSuccess || hipHostMalloc((void **)&ph, hbytes, hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void **)&phd, ph, 0) != hipSuccess || hipMemset(pd, 0, dbytes) != hipSuccess) {
        (void)hipGetLastError();
        if (pd) (void)hipFree(pd);
        if (ph) (void)hipHostFree(ph);
        g_sel_pool_failed[d] = true;
        return false;
    }
    memset(ph, 0, hbytes);
    g_sel_pool_dev[d] = pd; g_sel_pool_host[d] = ph; g_sel_pool_host_dev[d] = phd;
    return true;
}

// The record of a call site; null when the mechanism is off or the device's block does not exist yet (first call of
// the process inside a capture): the call then runs at level 0 without statistics.  A full table hands the least
// recently used record to the new key (its counters keep counting: the first record read is only a baseline; the
// forward's window placement words are cleared).
SelSlot *sel_acquire(int kind, int M, int L, int P, int dt, hipStream_t stream) {
    if (!opt_auto_select.load()) return nullptr;
    SelKey k;
    memset(&k, 0, sizeof(k));
    (void)hipGetDevice(&k.dev);
    k.kind = kind; k.site = g_site; k.M = M; k.L = L; k.P = P; k.dt = dt;
    std::lock_guard<std::mutex> lock(g_sel_mu);
    SelSlot *pick = nullptr;
    for (int i = 0; i < kSelSlots; ++i) {
        if (g_sel[i].used && g_sel[i].key == k) {
            g_sel[i].stamp = ++g_sel_clock;
            return &g_sel[i];
        }
        if (!g_sel[i].used) {
            if (!pick || pick->used) pick = &g_sel[i];
        } else if (g_sel[i].key.dev == k.dev && (!pick || (pick->used && g_sel[i].stamp < pick->stamp))) {
            pick = &g_sel[i];
        }
    }
    if (!pick || !sel_pool(k.dev, stream)) return nullptr;
    const int d = k.dev & 63, i = (int)(pick - g_sel);
    SelSlot &s = *pick;
    if (s.used) {
        // A record that changes hands keeps counting (the first read is a baseline), but the window placement the
        // old call site measured -- mean offsets and their "measured" bits -- would centre the new site's windows on
        // another module's offsets and report what leaves them: those words start over.  A memset cannot be recorded
        // into a capture (it would replay); a capturing call with no record of its own runs without one.
        if (stream_capturing(stream)) return nullptr;
#ifndef MSDA_SEL_KEEP_PLACEMENT      // (test builds only: the bug the reuse test pins)
        unsigned long long *const rec = g_sel_pool_dev[d] + (size_t)i * kSelDevWords;
        if (hipMemsetAsync(rec + kSelHintAccWord, 0, (size_t)(kSelHintValidWord + 1 - kSelHintAccWord) * 8, stream) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
#endif
    }
    s.key = k;
    s.dev = g_sel_pool_dev[d] + (size_t)i * kSelDevWords;
    s.host = g_sel_pool_host[d] + (size_t)i * kSelHostWords;
    s.host_dev = g_sel_pool_host_dev[d] + (size_t)i * kSelHostWords;
    s.primed = false;
    s.seen = s.host[9];
    memset(s.last, 0, sizeof(s.last));
    s.level = s.eff = 0; s.calls = 0u; s.frac = s.frac_inner = -1.f;      // (-1: nothing measured yet)
    s.polled = false; s.pub_seen = s.seen; s.scratch = false;
    s.stamp = ++g_sel_clock;
    s.used = true;
    return &s;
}

SelRule sel_rule(int kind, bool scratch = true) {
    SelRule r;
    if (kind == 0) { r.up0 = opt_sel_fwd_up.load(); r.down1 = opt_sel_fwd_down.load(); r.up1 = r.down2 = 0; }
    else {
        r.up0 = opt_sel_up0.load(); r.down1 = opt_sel_down1.load();
        r.up1 = scratch ? opt_sel_up1.load() : opt_sel_up1_rows.load();
        r.down2 = scratch ? opt_sel_down2.load() : opt_sel_down2_rows.load();
    }
    return r;
}

// Read what the launches have left in the host record and move the level (g_sel_mu held).  Per level the launches ran
// at, the difference to the counters seen last is judged once it holds kSelMinSample valid corners: a probe ran one
// level below the top and is judged by the top level's rule; counts of a level the record has moved away from are
// dropped.
void sel_refresh(SelSlot *s) {
    const unsigned long long seq = s->host[9];
    if (seq == s->seen) return;
    std::atomic_thread_fence(std::memory_order_acquire);
    unsigned long long cur[kSelLevels][3];
    for (int l = 0; l < kSelLevels; ++l)
        for (int c = 0; c < 3; ++c) cur[l][c] = s->host[l * 3 + c];
    s->seen = seq;
    if (!s->primed) {
        memcpy(s->last, cur, sizeof(cur));
        s->primed = true;
        return;
    }
    const int kind = s->key.kind, top = kind == 0 ? 1 : 2;
    const SelRule r = sel_rule(kind, s->scratch);
    for (int ran = 0; ran < kSelLevels; ++ran) {
        const unsigned long long dv = cur[ran][0] - s->last[ran][0];
        if (dv < kSelMinSample || dv > (1ull << 62)) continue;
        const float f = (float)((double)(cur[ran][1] - s->last[ran][1]) / (double)dv);
        const float fi = (float)((double)(cur[ran][2] - s->last[ran][2]) / (double)dv);
        memcpy(s->last[ran], cur[ran], sizeof(cur[ran]));
        if (s->level == top && ran == top - 1) {
            s->frac = f; s->frac_inner = fi;
            s->level = sel_next_level(kind, top, f * 1000.f, fi * 1000.f, r);
        } else if (ran == s->level) {
            s->frac = f; s->frac_inner = fi;
            s->level = sel_next_level(kind, ran, f * 1000.f, fi * 1000.f, r);
        }
    }
}

// The level for THIS call.  Eager calls count themselves: a level without windows probes one level down every
// kSelProbeEvery-th call (`probe` is then set).  A capturing call takes what the last msda_selector_poll() announced.
int sel_level(SelSlot *s, int kind, bool &probe, bool capturing = false) {
    probe = false;
    const int pinned = opt_sel_level.load();
    if (!s) return pinned >= 0 ? pinned : 0;
    std::lock_guard<std::mutex> lock(g_sel_mu);
    sel_refresh(s);
    g_sel_frac = s->frac;
    g_sel_inner = s->frac_inner;
    const int top = kind == 0 ? 1 : 2;
    int level;
    if (capturing) {
        level = pinned >= 0 ? pinned : s->eff;
        probe = pinned < 0 && level != s->level;
    } else {
        ++s->calls;
        level = pinned >= 0 ? pinned : s->level;
        // (`eff` belongs to msda_selector_poll() once a caller polls: the eager warm-up calls a graph cache makes in
        //  front of a capture used to reset it here, and the capture keyed on "probe one level down" then held the
        //  top level's kernel -- advisor, round 5.  Without a polling caller a capture takes the level of the last
        //  eager call, as before)
        if (!s->polled) s->eff = s->level;
        if (pinned < 0 && level == top && (s->calls % kSelProbeEvery) == 0u) {
            level = top - 1;
            probe = true;
        }
    }
    g_sel_level = level;
    return level;
}

// What sel_level() would answer for this thread's call site, without counting a call or creating a record (the
// workspace query: a caller sizes its scratch before the call).
int sel_peek(int kind, int M, int L, int P, int dt, hipStream_t stream) {
    const int pinned = opt_sel_level.load();
    if (pinned >= 0) return pinned;
    if (!opt_auto_select.load()) return 0;
    SelKey k;
    memset(&k, 0, sizeof(k));
    (void)hipGetDevice(&k.dev);
    k.kind = kind; k.site = g_site; k.M = M; k.L = L; k.P = P; k.dt = dt;
    const bool capturing = stream_capturing(stream);
    std::lock_guard<std::mutex> lock(g_sel_mu);
    for (int i = 0; i < kSelSlots; ++i)
        if (g_sel[i].used && g_sel[i].key == k) {
            g_sel[i].scratch = true;        // (a caller that asks will bring scratch: level 2 is then the sorted backward)
            sel_refresh(&g_sel[i]);
            return capturing ? g_sel[i].eff : g_sel[i].level;
        }
    return 0;
}

struct FusedArgs {     // null proj = the plain operator
    const float *proj = nullptr;
    int proj_stride = 0;
    const float *ref = nullptr;
    int ref_dim = 0;
    const unsigned char *mask = nullptr;
};

PointSrc make_src(const void *loc, const void *attn, const FusedArgs &fa, int M, int L, int P) {
    PointSrc s;
    s.loc = (const float *)loc;
    s.attn = (const float *)attn;
    s.proj = fa.proj;
    s.ref = fa.ref;
    s.mask = fa.mask;
    s.proj_stride = fa.proj_stride;
    s.n_off = 2 * M * L * P;
    s.ref_dim = fa.ref_dim;
    return s;
}

int check_fused(const FusedArgs &fa, int M, int L, int P) {
    if (!fa.proj || !fa.ref) return fail(MSDA_EINVAL, "null pointer argument");
    if (fa.ref_dim != 2 && fa.ref_dim != 4) return fail(MSDA_EINVAL, "reference points must have 2 or 4 coordinates");
    if (fa.proj_stride < 3 * M * L * P) return fail(MSDA_EINVAL, "projection rows shorter than 3*M*L*P");
    if (L * P > kMaxFusedLP) return fail(MSDA_ENOTSUP, "fused prologue supports at most 64 sampling points per head");
    return MSDA_OK;
}

// A side kernel of a call (zeroing, fused prologue / finish, the sort's stages): launched and checked under its own
// name.  check_launch touches only the error text, so msda_last_kernel() keeps naming the call's main kernel.
template <typename K, typename... A>
int launch_side(const char *what, K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, A... args) {
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
    return check_launch(what);
}

constexpr int kNotTaken = 1 << 30;      // a path's answer when the call does not fit it: the driver tries the next one

// One operator call: what the entry point was given (forward: `out`; backward: `grad_out` and the gradients) and the
// facts every path asks about, computed once by finish_call.  The forward instantiates it with TG = TC.
template <typename TV_, typename TC_, typename TG_>
struct Call {
    using TV = TV_; using TC = TC_; using TG = TG_;
    // storage types the specialised (D = 32) kernels exist for
    static constexpr bool kD32Type = sizeof(TC) == 4 && sizeof(TG) == 4 && (sizeof(TV) == 4 || sizeof(TV) == 2);
    int N = 0, S = 0, M = 0, D = 0, L = 0, Lq = 0, P = 0;
    const int64_t *shapes = nullptr, *lstart = nullptr, *shapes_host = nullptr;
    const TC *loc = nullptr, *attn = nullptr;
    FusedArgs fa;
    const TV *value = nullptr;
    TV *out = nullptr;
    const TV *grad_out = nullptr, *fwd_out = nullptr;
    TG *grad_value = nullptr;
    TC *grad_loc = nullptr, *grad_attn = nullptr;
    float *grad_proj = nullptr, *grad_ref_part = nullptr;
    int zero_grad_value = 0;
    float *workspace = nullptr;
    size_t workspace_bytes = 0;
    hipStream_t stream = nullptr;
    long vstride = 0;           // msda_next_value_pixel_stride, taken by the entry point (0: contiguous); below: derived
    bool fused = false, strided = false;
    long value_elems = 0, value_bytes = 0, n_rows = 0;      // n_rows: (batch, query, head) rows
    bool can32 = false;         // the specialised kernels can address this call
    bool can_tile = false;      // backward: pyramid self-attention with host shapes (bins / tile_lv)

    PointSrc src() const { return make_src(loc, attn, fa, M, L, P); }
};

// Validate a call and fill in its derived facts.  `io`: the forward's out / the backward's grad_out.  `empty`: no
// queries -- nothing to compute (the stride of such a call is not looked at).
template <typename C>
int finish_call(C &c, const void *io, bool backward, bool &empty) {
    using TV = typename C::TV;
    c.fused = c.fa.proj != nullptr;
    int rc = c.fused ? check_dims(c.value, c.shapes, c.lstart, c.fa.proj, c.fa.ref, io, c.N, c.S, c.M, c.D, c.L, c.Lq, c.P)
                     : check_dims(c.value, c.shapes, c.lstart, c.loc, c.attn, io, c.N, c.S, c.M, c.D, c.L, c.Lq, c.P);
    if (rc) return rc;
    if (c.fused && (rc = check_fused(c.fa, c.M, c.L, c.P))) return rc;
    if (backward && (!c.grad_value || (c.fused ? !c.grad_proj : (!c.grad_loc || !c.grad_attn))))
        return fail(MSDA_EINVAL, "null gradient pointer");
    const long row_elems = (long)c.M * c.D;
    c.strided = c.vstride != 0 && c.vstride != row_elems;
    if (backward && c.strided && c.zero_grad_value) return fail(MSDA_EINVAL, "value pixel stride: grad_value is the caller's to zero");
    c.n_rows = (long)c.N * c.Lq * c.M;
    empty = (long)c.N * c.Lq == 0;
    if (empty) return MSDA_OK;
    c.value_elems = (long)c.N * c.S * (c.strided ? c.vstride : row_elems);
    c.value_bytes = c.value_elems * (long)sizeof(TV);
    c.can32 = C::kD32Type && d32_ok(c.D, c.L, c.value_elems);
    if (c.strided) {        // the gather forward and the rows backward only
        if (c.vstride < row_elems || (c.vstride * (long)sizeof(TV)) % 16 != 0)
            return fail(MSDA_EINVAL, "value pixel stride: at least M * D elements, rows 16-byte aligned");
        if (!backward && !c.can32) return fail(MSDA_ENOTSUP, "value pixel stride: D = 32 float32 / bfloat16 calls only");
        if (backward && !(c.can32 && c.L * c.P <= kRowsMaxLP && c.n_rows < (1L << 31)))
            return fail(MSDA_ENOTSUP, "value pixel stride: D = 32 float32 / bfloat16 calls of at most 64 points only");
    }
    c.can_tile = !c.strided && c.can32 && c.shapes_host && c.Lq == c.S && c.L <= kTileMaxL && c.grad_ref_part == nullptr;
    return MSDA_OK;
}

#include "msda_dispatch_fwd.h"
#include "msda_dispatch_bwd.h"

// ---- the entry points' bodies: the C types of the ABI cast to the kernels' (uint16_t -> bf16_t), the arguments into a
//      Call.  `vstride` is what the entry point took from msda_next_value_pixel_stride ----
template <typename TV, typename TC>
int run_forward(long vstride, const void *value, const int64_t *shapes, const int64_t *lstart, const TC *loc, const TC *attn,
                const FusedArgs &fa, int N, int S, int M, int D, int L, int Lq, int P, void *out, const int64_t *shapes_host,
                void *stream) {
    Call<TV, TC, TC> c;
    c.N = N; c.S = S; c.M = M; c.D = D; c.L = L; c.Lq = Lq; c.P = P;
    c.shapes = shapes; c.lstart = lstart; c.shapes_host = shapes_host;
    c.loc = loc; c.attn = attn; c.fa = fa;
    c.value = (const TV *)value; c.out = (TV *)out;
    c.stream = (hipStream_t)stream; c.vstride = vstride;
    return forward_impl(c);
}

template <typename TV, typename TC, typename TG>
int run_backward(long vstride, const void *value, const int64_t *shapes, const int64_t *lstart, const TC *loc, const TC *attn,
                 const FusedArgs &fa, const void *grad_out, const void *fwd_out, int N, int S, int M, int D, int L, int Lq,
                 int P, TG *grad_value, TC *grad_loc, TC *grad_attn, float *grad_proj, float *grad_ref_part,
                 int zero_grad_value, const int64_t *shapes_host, void *workspace, size_t workspace_bytes, void *stream) {
    Call<TV, TC, TG> c;
    c.N = N; c.S = S; c.M = M; c.D = D; c.L = L; c.Lq = Lq; c.P = P;
    c.shapes = shapes; c.lstart = lstart; c.shapes_host = shapes_host;
    c.loc = loc; c.attn = attn; c.fa = fa;
    c.value = (const TV *)value; c.grad_out = (const TV *)grad_out; c.fwd_out = (const TV *)fwd_out;
    c.grad_value = grad_value; c.grad_loc = grad_loc; c.grad_attn = grad_attn;
    c.grad_proj = grad_proj; c.grad_ref_part = grad_ref_part; c.zero_grad_value = zero_grad_value;
    c.workspace = (float *)workspace; c.workspace_bytes = workspace_bytes;
    c.stream = (hipStream_t)stream; c.vstride = vstride;
    return backward_impl(c);
}

FusedArgs fused_args(const float *proj, int proj_stride, const float *ref, int ref_dim, const uint8_t *mask) {
    FusedArgs fa;
    fa.proj = proj; fa.proj_stride = proj_stride; fa.ref = ref; fa.ref_dim = ref_dim; fa.mask = mask;
    return fa;
}

}  // namespace

extern "C" {

int msda_abi_version(void) { return MSDA_ABI_VERSION; }

void msda_set_call_site(uint64_t site) { g_site = site; }

int msda_next_value_pixel_stride(long elements) {
    if (elements < 0) return fail(MSDA_EINVAL, "msda_next_value_pixel_stride: negative stride");
    g_value_stride = elements;
    return MSDA_OK;
}

int msda_selector_last(int *level, float *off_share, float *inner_share) {
    if (level) *level = g_sel_level;
    if (off_share) *off_share = g_sel_frac;
    if (inner_share) *inner_share = g_sel_inner;
    return MSDA_OK;
}

int msda_selector_next(int kind, int level, int off_permille, int inner_permille) {
    return sel_next_level(kind, level, (float)off_permille, (float)inner_permille, sel_rule(kind));
}

static int selector_poll_impl(const uint64_t *sites, int n_sites, int probe, uint64_t *signature) {
    int dev = 0, n = 0;
    (void)hipGetDevice(&dev);
    unsigned long long h = 0ull;
    const int pinned = opt_sel_level.load();
    if (opt_auto_select.load()) {
        std::lock_guard<std::mutex> lock(g_sel_mu);
        // (unfiltered: every kSelProbeEvery-th poll of the process is a probe tick; filtered: the caller counts its own)
        const bool probe_tick = sites ? probe != 0 : (++g_sel_tick % kSelProbeEvery) == 0ull;
        for (int i = 0; i < kSelSlots; ++i) {
            SelSlot &s = g_sel[i];
            if (!s.used || s.key.dev != dev) continue;
            if (sites) {
                bool mine = false;
                for (int k = 0; k < n_sites && !mine; ++k) mine = sites[k] == s.key.site;
                if (!mine) continue;
            }
            // launches are arriving (replayed graphs make no library call): the record is in use, whatever its stamp says
            if (s.host[9] != s.pub_seen) { s.pub_seen = s.host[9]; s.stamp = ++g_sel_clock; }
            sel_refresh(&s);
            const int top = s.key.kind == 0 ? 1 : 2;
            s.eff = (s.level == top && probe_tick) ? top - 1 : s.level;
            s.polled = true;
            const int level = pinned >= 0 ? pinned : s.eff;
            if (level != 0) {       // (records at level 0 -- the state before anything was measured -- leave no mark)
                // (site, direction, element size, level) -- not the slot index: the same levels give the same signature
                //  after the least-recently-used rule has moved a site to another record.  Order-independent (a sum of
                //  per-record hashes), for the same reason
                const unsigned long long w[2] = {s.key.site ^ ((unsigned long long)s.key.kind << 63) ^ ((unsigned long long)s.key.dt << 56),
                                                 (unsigned long long)level};
                unsigned long long hr = 0xcbf29ce484222325ull;
                for (int k = 0; k < 2; ++k)
                    for (int b = 0; b < 8; ++b) hr = (hr ^ ((w[k] >> (8 * b)) & 0xffull)) * 0x100000001b3ull;
                h += hr | 1ull;
            }
            ++n;
        }
    }
    if (signature) *signature = h;
    return n;
}

// For callers that REPLAY captured launches (no library call per launch): read every record of the current device,
// move the levels, and return a signature of the levels a call would run at now (0 when nothing is selected).  Every
// kSelProbeEvery-th poll announces one level down for the records that sit at a level without windows -- the graph
// captured under that signature is the probe.  Returns the number of records read.
int msda_selector_poll(uint64_t *signature) { return selector_poll_impl(nullptr, 0, 0, signature); }

// The same for the records of the given call sites only (ABI 6): a graph cache hashes the levels of the modules its
// graphs hold -- a level move or a probe of some other module's record no longer changes its key (advisor, round 5) --
// and decides itself when its records probe (`probe` != 0: records at a level without windows announce one level down).
int msda_selector_poll_sites(const uint64_t *sites, int n_sites, int probe, uint64_t *signature) {
    if (n_sites < 0 || (n_sites > 0 && !sites)) return fail(MSDA_EINVAL, "msda_selector_poll_sites: null site list");
    static const uint64_t none = 0;
    return selector_poll_impl(sites ? sites : &none, n_sites, probe, signature);
}
int msda_selector_reset(void) {
    std::lock_guard<std::mutex> lock(g_sel_mu);
    const size_t dbytes = (size_t)kSelSlots * kSelDevWords * 8, hbytes = (size_t)kSelSlots * kSelHostWords * 8;
    int cur = 0;
    (void)hipGetDevice(&cur);
    int rc = MSDA_OK;
    for (int d = 0; d < 64; ++d) {
        if (!g_sel_pool_dev[d]) continue;
        // (launches in flight still count into the block: wait for them, then clear it)
        if (hipSetDevice(d) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
            hipMemset(g_sel_pool_dev[d], 0, dbytes) != hipSuccess) {
            const hipError_t e = hipGetLastError();
            rc = fail((int)(e != hipSuccess ? e : hipErrorUnknown), "msda_selector_reset: device block not cleared");
            continue;
        }
        memset(g_sel_pool_host[d], 0, hbytes);
    }
    (void)hipSetDevice(cur);
    for (int i = 0; i < kSelSlots; ++i) g_sel[i].used = false;
    g_sel_level = 0;
    g_sel_frac = g_sel_inner = -1.f;
    return rc;
}
const char *msda_last_error(void) { return g_err; }
const char *msda_last_kernel(void) { return g_kernel; }

// ---- the compute entry points.  Each takes the thread's pending value stride FIRST -- before anything can fail -- so
//      that the setting never outlives the call it was made for.  The non-_ws forms are the _ws forms without scratch,
//      the _ws fused forms the _out forms without the forward's output; f32 / bf16 differ by the cast in run_*. ----
#define MSDA_DIMS int N, int S, int M, int D, int L, int Lq, int P
#define MSDA_LEVELS const int64_t *shapes_dev, const int64_t *lstart_dev
#define MSDA_PLAIN_BWD_TAIL(CT, TC) \
    const CT *grad_out, MSDA_DIMS, TC *grad_value, TC *grad_loc, TC *grad_attn, int zero_grad_value, const int64_t *shapes_host
#define MSDA_FUSED_HEAD(CT) \
    const CT *value, MSDA_LEVELS, const float *proj, int proj_stride, const float *ref, int ref_dim, const uint8_t *pad_mask
#define MSDA_FUSED_BWD_TAIL \
    MSDA_DIMS, float *grad_value, float *grad_proj, float *grad_ref_part, int zero_grad_value, const int64_t *shapes_host
// plain operator, forward and backward (SFX f32 / f64 / bf16; CT: the ABI's element type; TV / TC: the kernels')
#define MSDA_PLAIN_ENTRIES(SFX, CT, TV, TC)                                                                             \
    int msda_forward_##SFX(const CT *value, MSDA_LEVELS, const TC *loc, const TC *attn, MSDA_DIMS, CT *out,            \
                           const int64_t *shapes_host, void *stream) {                                                 \
        const long vstride = take_value_stride();                                                                      \
        return run_forward<TV, TC>(vstride, value, shapes_dev, lstart_dev, loc, attn, FusedArgs{}, N, S, M, D, L, Lq,  \
                                   P, out, shapes_host, stream);                                                       \
    }                                                                                                                  \
    int msda_backward_##SFX(const CT *value, MSDA_LEVELS, const TC *loc, const TC *attn, MSDA_PLAIN_BWD_TAIL(CT, TC),  \
                            void *stream) {                                                                            \
        const long vstride = take_value_stride();                                                                      \
        return run_backward<TV, TC, TC>(vstride, value, shapes_dev, lstart_dev, loc, attn, FusedArgs{}, grad_out,      \
                                        nullptr, N, S, M, D, L, Lq, P, grad_value, grad_loc, grad_attn, nullptr,      \
                                        nullptr, zero_grad_value, shapes_host, nullptr, 0, stream);                    \
    }
MSDA_PLAIN_ENTRIES(f32, float, float, float)
MSDA_PLAIN_ENTRIES(f64, double, double, double)
MSDA_PLAIN_ENTRIES(bf16, uint16_t, bf16_t, float)
// plain backward with scratch, and the fused prologue's forward / backward / backward with scratch / backward given the
// forward's output of the same call (ABI 6: with it the default backward of the encoder's self-attention is ONE kernel --
// no attention-weight kernel in front, no Jacobian kernel behind; bwd_pyramid)
#define MSDA_FUSED_BACKWARD(FWD_OUT, WS, WS_BYTES)                                                                      \
    const long vstride = take_value_stride();                                                                          \
    if (!proj) return fail(MSDA_EINVAL, "null pointer argument");                                                      \
    return run_backward<TV, float, float>(vstride, value, shapes_dev, lstart_dev, nullptr, nullptr,                    \
                                          fused_args(proj, proj_stride, ref, ref_dim, pad_mask), grad_out, FWD_OUT, N, \
                                          S, M, D, L, Lq, P, grad_value, nullptr, nullptr, grad_proj, grad_ref_part,   \
                                          zero_grad_value, shapes_host, WS, WS_BYTES, stream)
#define MSDA_WS_FUSED_ENTRIES(SFX, CT, TV_)                                                                             \
    int msda_backward_ws_##SFX(const CT *value, MSDA_LEVELS, const float *loc, const float *attn,                      \
                               MSDA_PLAIN_BWD_TAIL(CT, float), void *workspace, size_t workspace_bytes, void *stream) {\
        const long vstride = take_value_stride();                                                                      \
        return run_backward<TV_, float, float>(vstride, value, shapes_dev, lstart_dev, loc, attn, FusedArgs{},         \
                                               grad_out, nullptr, N, S, M, D, L, Lq, P, grad_value, grad_loc,          \
                                               grad_attn, nullptr, nullptr, zero_grad_value, shapes_host, workspace,   \
                                               workspace_bytes, stream);                                               \
    }                                                                                                                  \
    int msda_fused_forward_##SFX(MSDA_FUSED_HEAD(CT), MSDA_DIMS, CT *out, const int64_t *shapes_host, void *stream) {  \
        const long vstride = take_value_stride();                                                                      \
        if (!proj) return fail(MSDA_EINVAL, "null pointer argument");                                                  \
        return run_forward<TV_, float>(vstride, value, shapes_dev, lstart_dev, nullptr, nullptr,                       \
                                       fused_args(proj, proj_stride, ref, ref_dim, pad_mask), N, S, M, D, L, Lq, P,    \
                                       out, shapes_host, stream);                                                      \
    }                                                                                                                  \
    int msda_fused_backward_##SFX(MSDA_FUSED_HEAD(CT), const CT *grad_out, MSDA_FUSED_BWD_TAIL, void *stream) {        \
        using TV = TV_;                                                                                                \
        MSDA_FUSED_BACKWARD(nullptr, nullptr, 0);                                                                      \
    }                                                                                                                  \
    int msda_fused_backward_ws_##SFX(MSDA_FUSED_HEAD(CT), const CT *grad_out, MSDA_FUSED_BWD_TAIL, void *workspace,    \
                                     size_t workspace_bytes, void *stream) {                                           \
        using TV = TV_;                                                                                                \
        MSDA_FUSED_BACKWARD(nullptr, workspace, workspace_bytes);                                                      \
    }                                                                                                                  \
    int msda_fused_backward_out_##SFX(MSDA_FUSED_HEAD(CT), const CT *grad_out, const CT *fwd_out, MSDA_FUSED_BWD_TAIL, \
                                      void *workspace, size_t workspace_bytes, void *stream) {                         \
        using TV = TV_;                                                                                                \
        MSDA_FUSED_BACKWARD(fwd_out, workspace, workspace_bytes);                                                      \
    }
MSDA_WS_FUSED_ENTRIES(f32, float, float)
MSDA_WS_FUSED_ENTRIES(bf16, uint16_t, bf16_t)
size_t msda_fused_workspace_bytes(int N, int Lq, int M, int L, int P) {
    if (N < 0 || Lq < 0 || M <= 0 || L <= 0 || P <= 0) return 0;
    return (size_t)N * Lq * M * L * P * 3 * sizeof(float);
}

// Scratch the NEXT backward call of this thread's call site can use (ABI 6): the fused prologue's block
// (msda_fused_workspace_bytes) plus, when that call would build grad_value by sort + gather ("bwd_variant" 13, or
// selector level 2 for self-attention over the pyramid), the sort's records and tables.  0: the call needs none.
size_t msda_backward_workspace_bytes(int fused, int N, int S, int M, int D, int L, int Lq, int P, int elem_bytes,
                                     void *stream) {
    if (N <= 0 || S <= 0 || Lq <= 0 || M <= 0 || D <= 0 || L <= 0 || P <= 0) return 0;
    const size_t n_pts = (size_t)N * Lq * M * L * P;
    size_t bytes = fused ? n_pts * 3 * sizeof(float) : 0;
    const int variant = opt_bwd_variant.load();
    bool sorted = variant == 13;
    if (variant == 0 && opt_bwd_sorted.load() && D == 32 && Lq == S && L <= kTileMaxL && (elem_bytes == 4 || elem_bytes == 2))
        sorted = sel_peek(1, M, L, P, elem_bytes, (hipStream_t)stream) >= 2;
    if (sorted && D == 32) {
        SortPlan sp;
        if (make_sort_plan(sp, N, S, M, L, Lq, P, (size_t)elem_bytes, nullptr, opt_bwd_sort_qc.load(), opt_bwd_sort_emult.load())) bytes = ((bytes + 255) & ~(size_t)255) + sp.bytes;
    }
    return bytes;
}

int msda_fused_points_f32(const int64_t *shapes_dev, const float *proj, int proj_stride, const float *ref, int ref_dim,
                          int N, int M, int L, int Lq, int P, float *loc_out, float *attn_out, void *stream) {
    if (!shapes_dev || !proj || !ref || !loc_out || !attn_out) return fail(MSDA_EINVAL, "null pointer argument");
    if (N < 0 || Lq < 0 || M <= 0 || L <= 0 || P <= 0) return fail(MSDA_EINVAL, "bad dimension");
    const FusedArgs fa = fused_args(proj, proj_stride, ref, ref_dim, nullptr);
    const int rc = check_fused(fa, M, L, P);
    if (rc) return rc;
    const long n_rows = (long)N * Lq * M;
    if (n_rows == 0) { g_err[0] = 0; return MSDA_OK; }
    const PointSrc src = make_src(nullptr, nullptr, fa, M, L, P);
    if (L * P <= 16) {
        hipLaunchKernelGGL(msda_fused_points16_kernel, dim3(clamp_grid((n_rows * 16 + 255) / 256, 32)), dim3(256), 0,
                           (hipStream_t)stream, shapes_dev, src, n_rows, M, L, P, loc_out, attn_out);
        return check_launch("msda_fused_points16_kernel");
    }
    const int grid = clamp_grid((n_rows * 8 + 255) / 256, 16);
    hipLaunchKernelGGL(msda_fused_points_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, shapes_dev, src, n_rows,
                       M, L, P, loc_out, attn_out);
    return check_launch("msda_fused_points_kernel");
}

// ---- attention maps (ABI 8; memotr_amd/csrc/msda_attn_map.h) ----
static int attention_heat(bool fused, const int64_t *shapes_dev, const msda_heat_layer *layers, int n_layers, int M,
                          int L, int P, const int32_t *rows, const int32_t *planes, int K, const uint16_t *stamp,
                          int radius, float sx, float sy, uint64_t *heat, uint64_t *peak, int n_planes, int hc, int wc,
                          int accumulate, void *stream) {
    if (!layers || !stamp || !heat || !peak || (fused && !shapes_dev)) return fail(MSDA_EINVAL, "null pointer argument");
    if (K < 0 || (K > 0 && (!rows || !planes))) return fail(MSDA_EINVAL, "null row / plane table");
    if (n_layers < 1 || n_layers > kHeatMaxLayers) return fail(MSDA_EINVAL, "1 to 8 layers per launch");
    if (radius < 0 || radius > kHeatMaxRadius) return fail(MSDA_EINVAL, "stamp radius is 0 to 8");
    if (M <= 0 || L <= 0 || P <= 0 || n_planes <= 0 || hc <= 0 || wc <= 0) return fail(MSDA_EINVAL, "non-positive dimension");
    if (n_planes > 65535) return fail(MSDA_EINVAL, "at most 65535 heat planes");
    if ((double)n_planes * hc * wc > 2147483647.0 || (double)K * n_layers * M > 2147483647.0)
        return fail(MSDA_ERANGE, "heat planes / row table exceed 2^31 elements");
    if (fused && L * P > kMaxFusedLP) return fail(MSDA_ENOTSUP, "fused prologue supports at most 64 sampling points per head");
    HeatLayers ly;
    memset(&ly, 0, sizeof(ly));
    ly.n = n_layers;
    for (int i = 0; i < n_layers; ++i) {
        const msda_heat_layer &d = layers[i];
        if (!d.a || !d.b) return fail(MSDA_EINVAL, "null layer pointer");
        if (d.Lq < 0) return fail(MSDA_EINVAL, "negative query count");
        if (fused && d.ref_dim != 2 && d.ref_dim != 4) return fail(MSDA_EINVAL, "reference points must have 2 or 4 coordinates");
        if (fused && d.proj_stride < 3 * M * L * P) return fail(MSDA_EINVAL, "projection rows shorter than 3*M*L*P");
        if ((double)d.Lq * (fused ? (double)d.proj_stride : 2.0 * M * L * P) > 2147483647.0)
            return fail(MSDA_ERANGE, "tensor exceeds 2^31 elements");
        ly.a[i] = d.a; ly.b[i] = d.b; ly.Lq[i] = d.Lq; ly.proj_stride[i] = d.proj_stride; ly.ref_dim[i] = d.ref_dim;
    }
    const hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(peak, 0, sizeof(uint64_t) * (size_t)n_planes, st);    // (the kernel takes maxima into it)
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "hipMemsetAsync(peak): %s", hipGetErrorString(e));
        return (int)e;
    }
    const int tiles = ((wc + kHeatTile - 1) / kHeatTile) * ((hc + kHeatTile - 1) / kHeatTile);
    const int threads = heat_threads(((long)K * n_layers * M + n_planes - 1) / n_planes);     // (rows spread evenly: a guess)
    auto *h = reinterpret_cast<unsigned long long *>(heat);
    auto *pk = reinterpret_cast<unsigned long long *>(peak);
    if (fused)
        hipLaunchKernelGGL(msda_attn_heat_kernel<true>, dim3(tiles, n_planes), dim3(threads), 0, st, ly, shapes_dev, M, L, P,
                           rows, planes, K, stamp, radius, sx, sy, h, pk, n_planes, hc, wc, accumulate);
    else
        hipLaunchKernelGGL(msda_attn_heat_kernel<false>, dim3(tiles, n_planes), dim3(threads), 0, st, ly, shapes_dev, M, L,
                           P, rows, planes, K, stamp, radius, sx, sy, h, pk, n_planes, hc, wc, accumulate);
    return check_launch("msda_attn_heat_kernel");
}

int msda_attention_heat_points_f32(const msda_heat_layer *layers, int n_layers, int M, int L, int P,
                                   const int32_t *rows, const int32_t *planes, int K, const uint16_t *stamp, int radius,
                                   float sx, float sy, uint64_t *heat, uint64_t *peak, int n_planes, int hc, int wc,
                                   int accumulate, void *stream) {
    return attention_heat(false, nullptr, layers, n_layers, M, L, P, rows, planes, K, stamp, radius, sx, sy, heat, peak,
                          n_planes, hc, wc, accumulate, stream);
}

int msda_attention_heat_f32(const int64_t *shapes_dev, const msda_heat_layer *layers, int n_layers, int M, int L, int P,
                            const int32_t *rows, const int32_t *planes, int K, const uint16_t *stamp, int radius,
                            float sx, float sy, uint64_t *heat, uint64_t *peak, int n_planes, int hc, int wc,
                            int accumulate, void *stream) {
    return attention_heat(true, shapes_dev, layers, n_layers, M, L, P, rows, planes, K, stamp, radius, sx, sy, heat, peak,
                          n_planes, hc, wc, accumulate, stream);
}

int msda_attention_blend_u8(const uint8_t *src, long src_pitch, uint8_t *dst, long dst_pitch, int W, int H,
                            const uint64_t *heat, const uint64_t *peak, const uint8_t *lut, int n_planes, int cell,
                            int max_alpha, uint64_t full_scale, void *stream) {
    if (!src || !dst || !heat || !peak || !lut) return fail(MSDA_EINVAL, "null pointer argument");
    if (W <= 0 || H <= 0) return fail(MSDA_EINVAL, "non-positive frame size");
    if (cell < 1) return fail(MSDA_EINVAL, "cell size is at least 1 pixel");
    if (n_planes < 1 || n_planes > kBlendMaxPlanes) return fail(MSDA_EINVAL, "1 to 16 planes per launch");
    if (max_alpha < 0 || max_alpha > 255) return fail(MSDA_EINVAL, "max_alpha is 0 to 255");
    if (src_pitch < 3L * W || dst_pitch < 3L * W) return fail(MSDA_EINVAL, "row pitch shorter than 3 * W bytes");
    if ((H + kBlendTileH - 1) / kBlendTileH > 65535) return fail(MSDA_ERANGE, "frame too tall");
    const int hc = (H + cell - 1) / cell, wc = (W + cell - 1) / cell;
    hipLaunchKernelGGL(msda_attn_blend_kernel, dim3((W + kBlendTileW - 1) / kBlendTileW, (H + kBlendTileH - 1) / kBlendTileH),
                       dim3(256), 0, (hipStream_t)stream, src, src_pitch, dst, dst_pitch, W, H,
                       reinterpret_cast<const unsigned long long *>(heat),
                       reinterpret_cast<const unsigned long long *>(peak), lut, n_planes, hc, wc, cell, max_alpha,
                       (unsigned long long)full_scale);
    return check_launch("msda_attn_blend_kernel");
}

int msda_sample_indices_f32(const int64_t *shapes_dev, const float *loc, int N, int M, int L, int Lq, int P,
                            int32_t *h_low, int32_t *w_low, uint8_t *gate, void *stream) {
    if (!shapes_dev || !loc || !h_low || !w_low || !gate) return fail(MSDA_EINVAL, "null pointer argument");
    if (N < 0 || Lq < 0 || M <= 0 || L <= 0 || P <= 0) return fail(MSDA_EINVAL, "bad dimension");
    const long n_points = (long)N * Lq * M * L * P;
    if (n_points == 0) { g_err[0] = 0; return MSDA_OK; }
    const int grid = clamp_grid((n_points + 255) / 256, 16);
    hipLaunchKernelGGL(msda_indices_f32_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, shapes_dev, loc,
                       n_points, L, P, h_low, w_low, gate);
    return check_launch("msda_indices_f32_kernel");
}

static std::atomic<int> *find_opt(const char *key) {
    if (!key) return nullptr;
    if (!strcmp(key, "fwd_variant")) return &opt_fwd_variant;
    if (!strcmp(key, "bwd_variant")) return &opt_bwd_variant;
    if (!strcmp(key, "fwd_block")) return &opt_fwd_block;
    if (!strcmp(key, "bwd_block")) return &opt_bwd_block;
    if (!strcmp(key, "fwd_grid_mult")) return &opt_fwd_grid_mult;
    if (!strcmp(key, "bwd_grid_mult")) return &opt_bwd_grid_mult;
    if (!strcmp(key, "bwd_tile_margin")) return &opt_bwd_tile_margin;
    if (!strcmp(key, "bwd_ablate")) return &opt_bwd_ablate;
    if (!strcmp(key, "bwd_wide_log2")) return &opt_bwd_wide_log2;
    if (!strcmp(key, "bwd_split")) return &opt_bwd_split;
    if (!strcmp(key, "bwd_bins_margin")) return &opt_bwd_bins_margin;
    if (!strcmp(key, "bwd_bins_margin_hi")) return &opt_bwd_bins_margin_hi;
    if (!strcmp(key, "auto_select")) return &opt_auto_select;
    if (!strcmp(key, "deterministic")) return &opt_deterministic;
    if (!strcmp(key, "sel_level")) return &opt_sel_level;
    if (!strcmp(key, "sel_up0")) return &opt_sel_up0;
    if (!strcmp(key, "sel_up1")) return &opt_sel_up1;
    if (!strcmp(key, "sel_up1_rows")) return &opt_sel_up1_rows;
    if (!strcmp(key, "sel_down2_rows")) return &opt_sel_down2_rows;
    if (!strcmp(key, "sel_down1")) return &opt_sel_down1;
    if (!strcmp(key, "sel_down2")) return &opt_sel_down2;
    if (!strcmp(key, "sel_fwd_up")) return &opt_sel_fwd_up;
    if (!strcmp(key, "sel_fwd_down")) return &opt_sel_fwd_down;
    if (!strcmp(key, "bwd_bins_strip")) return &opt_bwd_bins_strip;
    if (!strcmp(key, "bwd_rows")) return &opt_bwd_rows;
    if (!strcmp(key, "bwd_sorted")) return &opt_bwd_sorted;
    if (!strcmp(key, "bwd_soft")) return &opt_bwd_soft;
    if (!strcmp(key, "bwd_sort_qc")) return &opt_bwd_sort_qc;
    if (!strcmp(key, "bwd_sort_emult")) return &opt_bwd_sort_emult;
    if (!strcmp(key, "bwd_rows_block")) return &opt_bwd_rows_block;
    if (!strcmp(key, "fwd_win_rlog")) return &opt_fwd_win_rlog;
    if (!strcmp(key, "fwd_win_rlogx")) return &opt_fwd_win_rlogx;
    if (!strcmp(key, "fwd_win_auto")) return &opt_fwd_win_auto;
    if (!strcmp(key, "fwd_win_bf16")) return &opt_fwd_win_bf16;
    if (!strcmp(key, "fwd_head_major")) return &opt_fwd_head_major;
    if (!strcmp(key, "fwd_win_block")) return &opt_fwd_win_block;
    if (!strcmp(key, "fwd_win_l0")) return &opt_fwd_win_l0;
    if (!strcmp(key, "fwd_win_margins")) return &opt_fwd_win_margins;
    if (!strcmp(key, "bwd_side_rows")) return &opt_bwd_side_rows;
    if (!strcmp(key, "fwd_win_trace_lo")) return &opt_fwd_win_trace_lo;
    if (!strcmp(key, "fwd_win_trace_hi")) return &opt_fwd_win_trace_hi;
    if (!strcmp(key, "fwd_win_ablate")) return &opt_fwd_win_ablate;
    if (!strcmp(key, "fwd_win_place")) return &opt_fwd_win_place;
    if (!strcmp(key, "fwd_win_wps")) return &opt_fwd_win_wps;
    if (!strcmp(key, "fwd_win_grid")) return &opt_fwd_win_grid;
    if (!strcmp(key, "fwd_win_rsy")) return &opt_fwd_win_rsy;
    if (!strcmp(key, "fwd_win_rsx")) return &opt_fwd_win_rsx;
    if (!strcmp(key, "fwd_win_early")) return &opt_fwd_win_early;
    return nullptr;
}

int msda_set_option(const char *key, int value) {
    std::atomic<int> *o = find_opt(key);
    if (!o || (value < 0 && !(o == &opt_sel_level && value == -1)))
        return fail(MSDA_EINVAL, "unknown option or negative value");
    o->store(value);
    return MSDA_OK;
}

int msda_get_option(const char *key, int *value) {
    std::atomic<int> *o = find_opt(key);
    if (!o || !value) return fail(MSDA_EINVAL, "unknown option");
    *value = o->load();
    return MSDA_OK;
}

}  // extern "C"
