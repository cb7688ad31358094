// msda_dispatch_bwd.h -- host side of the backward: which kernels a call takes, and their launches.  Included by
// msda_hip.hip inside its anonymous namespace, after msda_dispatch_fwd.h.  backward_impl (at the end) is the driver; a
// path returns kNotTaken when the call does not fit it.

enum class BwdPath { generic, rows, tile_lv, bins, sorted };

// "bwd_variant": 0 auto | 1 generic | 10 tile_lv | 12 bins | 13 sorted | every other number (those of kernels removed
// since): tile_lv, which hands a call it cannot take to the rows kernel
inline BwdPath bwd_path_of(int variant, bool &automatic) {
    automatic = variant == 0;
    return variant == 1 ? BwdPath::generic
                        : (variant == 12 ? BwdPath::bins : (variant == 13 ? BwdPath::sorted : BwdPath::tile_lv));
}

// grad_value is accumulated into: zeroed here on request -- by a kernel, not a memset node (a replayed hipGraph of
// ROCm 7.2 does not order MEMSET nodes behind the kernels before them unless DEBUG_CLR_GRAPH_PACKET_CAPTURE=0,
// tools/graph_memset_probe.py) -- together with whatever else the chosen path wants cleared (the sorted backward's
// bucket totals: one launch instead of two)
template <typename C>
int zero_launch(const C &c, unsigned *extra, unsigned extra_n) {
    if (!c.zero_grad_value && extra_n == 0u) return MSDA_OK;
    const size_t gv_words = (size_t)c.N * c.S * c.M * c.D * (sizeof(typename C::TG) / 4);
    const size_t n1 = c.zero_grad_value ? gv_words : 0;
    const size_t blocks = (n1 / 4 + extra_n + 255) / 256;
    return launch_side("msda_zero_words_kernel", msda_zero_words_kernel, dim3((unsigned)(blocks < 2048 ? (blocks ? blocks : 1) : 2048)),
                       dim3(256), 0, c.stream, reinterpret_cast<unsigned *>(c.grad_value), n1, extra, extra_n);
}

// ---- the split fused backward's side kernels (msda_fused_side.h): a prologue in front of the main kernel puts the
//      softmax weights (and the locations) into the caller's scratch, a finishing kernel behind it applies the Jacobians
//      to grad_proj in place.  Used by bwd_sorted and bwd_pyramid alike. ----

// rows16: the side kernels with one lane per (query, head) row -- 16 points as four 16-byte accesses.
// `rows_checked`: the caller has already established n_rows < 2^31 (the sorted path's own condition).
template <typename C>
bool side_rows16(const C &c, bool rows_checked) {
    return c.L * c.P == 16 && (c.fa.proj_stride % 4) == 0 && ((2 * c.M * c.L * c.P) % 4) == 0 && c.grad_ref_part == nullptr &&
           (((uintptr_t)c.fa.proj | (uintptr_t)c.grad_proj | (uintptr_t)c.workspace) & 15) == 0 &&
           (rows_checked || c.n_rows < (1L << 31)) && opt_bwd_side_rows.load() != 0;
}

// slim: the main kernel computes the sampling locations from the raw projection itself, so the scratch carries the
// weights only.  The counting-sort kernel can for any row of at most 16 points (one lane per point); the sort + gather
// kernels only in the one-lane-per-row form (`needs_rows16`).
template <typename C>
bool side_slim(const C &c, bool needs_rows16) {
    return c.L * c.P <= 16 && (!needs_rows16 || side_rows16(c, true));
}

// Weights into attn_ws, locations into loc_ws (null: not wanted; the rows16 kernel writes none).
template <typename C>
int launch_fused_prologue(const C &c, const PointSrc &src, bool rows16, float *loc_ws, float *attn_ws) {
    const long n_rows = c.n_rows;
    const char *const what = "msda_fused_points_kernel";
    if (rows16)
        return launch_side(what, msda_fused_attn16_rows_kernel, dim3(clamp_grid((n_rows + 255) / 256, 32)), dim3(256), 0,
                           c.stream, src, (unsigned)n_rows, (unsigned)c.M, attn_ws);
    if (c.L * c.P <= 16)
        return launch_side(what, msda_fused_points16_kernel, dim3(clamp_grid((n_rows * 16 + 255) / 256, 32)), dim3(256), 0,
                           c.stream, c.shapes, src, n_rows, c.M, c.L, c.P, loc_ws, attn_ws);
    return launch_side(what, msda_fused_points_kernel, dim3(clamp_grid((n_rows * 8 + 255) / 256, 16)), dim3(256), 0, c.stream,
                       c.shapes, src, n_rows, c.M, c.L, c.P, loc_ws, attn_ws);
}

// `split`: the main kernel ran on a materialised prologue (src.loc / src.attn in the scratch) and left the raw grad_loc /
// grad_attn in grad_proj; otherwise (the one-kernel fused tile_lv) only the softmax Jacobian is still to apply.
template <typename C>
int launch_fused_finish(const C &c, const PointSrc &src, bool split, bool rows16, int offsets_done) {
    const long n_rows = c.n_rows;
    const int jgrid = clamp_grid((n_rows * 8 + 255) / 256, 16);
    if (!split)
        return launch_side("msda_softmax_jacobian_kernel", msda_softmax_jacobian_kernel, dim3(jgrid), dim3(256), 0, c.stream,
                           src, n_rows, c.M, c.L * c.P, c.grad_proj);
    const char *const what = "msda_fused_finish_kernel";
    if (rows16 && offsets_done)
        return launch_side(what, msda_fused_finish16_rows_kernel, dim3(clamp_grid((n_rows + 255) / 256, 32)), dim3(256), 0,
                           c.stream, src, (unsigned)n_rows, (unsigned)c.M, c.grad_proj);
    if (c.L * c.P <= 16)
        return launch_side(what, msda_fused_finish16_kernel, dim3(clamp_grid((n_rows * 16 + 255) / 256, 32)), dim3(256), 0,
                           c.stream, c.shapes, src, n_rows, c.M, c.L, c.P, c.grad_proj, offsets_done);
    return launch_side(what, msda_fused_finish_kernel, dim3(jgrid), dim3(256), 0, c.stream, c.shapes, src, n_rows, c.M, c.L,
                       c.P, c.grad_proj);
}

// ---- sorted: grad_value by sort + gather through the caller's scratch (msda_bwd_sorted.h); everything else of the call
//      from the dots kernel.  Not tied to the pyramid: any D = 32 call the rows kernel takes.  Too little scratch (or
//      none): not taken -- the rows kernel with its atomics ----
template <typename C>
int bwd_sorted(const C &c) {
    using TV = typename C::TV;
    const int N = c.N, M = c.M, L = c.L, P = c.P;
    const long n_rows = c.n_rows;
    const bool fused = c.fused;
    const size_t fused_bytes = fused ? (((size_t)n_rows * L * P * 3 * sizeof(float) + 255) & ~(size_t)255) : 0;
    SortPlan sp;
    const bool fits = c.can32 && L * P <= kRowsMaxLP && n_rows < (1L << 31) && c.workspace != nullptr &&
                      c.workspace_bytes > fused_bytes &&
                      make_sort_plan(sp, N, c.S, M, L, c.Lq, P, sizeof(TV), (unsigned char *)c.workspace + fused_bytes,
                                     opt_bwd_sort_qc.load(), opt_bwd_sort_emult.load()) &&
                      fused_bytes + sp.bytes <= c.workspace_bytes && sort_dots_lds(sp.qc, L * P, sp.nbk).bytes <= 64u * 1024u;
    if (!fits) return kNotTaken;
    int rc;
    // grad_value (on request) and the bucket totals start from zero: one launch
    if ((rc = zero_launch(c, sp.cursor, (unsigned)((size_t)N * M * sp.nbk)))) return rc;
    const PointSrc src = c.src();
    // 1. fused: the softmax weights once per row into the scratch; the locations too unless the kernels below can compute
    //    them from the raw projection themselves (slim)
    PointSrc src_k = src;
    int fused_loc = 0, offsets_done = 0, soft16 = 0;
    bool rows16 = false;
    if (fused) {
        float *loc_ws = c.workspace, *attn_ws = c.workspace + (size_t)n_rows * L * P * 2;
        rows16 = side_slim(c, true);
        if (rows16) {
            // L * P = 16, 2-d reference points (the encoder's): the sixteen lanes of a row compute its softmax
            // in the dots and emit kernels themselves (one function, the bits of msda_fused_attn16_rows_kernel)
            // and the dots kernel applies the softmax Jacobian -- no side kernel, no weights in HBM.  4-d
            // reference points keep the weights in the scratch for the finishing kernel's location Jacobian
            fused_loc = 1;
            offsets_done = c.fa.ref_dim == 2 ? 1 : 0;
            soft16 = offsets_done;
        }
        if (!soft16 && (rc = launch_fused_prologue(c, src, rows16, loc_ws, attn_ws))) return rc;
        src_k.loc = loc_ws;
        src_k.attn = attn_ws;
    }
    // 2. per (batch, head, chunk of queries): grad_loc / grad_attn (fused: the columns of grad_proj) and the chunk's
    //    corner histogram
    const SortDotsLds dl = sort_dots_lds(sp.qc, L * P, sp.nbk);
    rc = launch_side("msda_bwd_sort_dots", msda_bwd_sort_dots<TV>, dim3((N * M * sp.nchunk + 7) & ~7), dim3(kSortThreads),
                     dl.bytes, c.stream, c.value, c.shapes, c.lstart, src_k, fused_loc, offsets_done, soft16, c.grad_out,
                     (float *)c.grad_loc, (float *)c.grad_attn, fused ? c.grad_proj : (float *)nullptr, sp, dl,
                     (unsigned)c.value_bytes);
    if (rc) return rc;
    if (fused && c.grad_ref_part != nullptr) {
        // (with gradients of the reference points wanted -- no caller of this package asks for them on this path -- the
        //  rows kernel without its atomics runs AFTER and overwrites the columns of grad_proj with its own, finished,
        //  results next to grad_ref_part; the dots kernel then only counts)
        const int threads = 256, per = threads / 32;
        rc = launch_side("msda_bwd_d32_rows<no atomics>", msda_bwd_d32_rows<TV, true, false>,
                         dim3(clamp_grid((n_rows + per - 1) / per, 64)), dim3(threads), 0, c.stream, c.value, c.shapes, c.lstart,
                         src, c.grad_out, N, c.S, M, L, c.Lq, P, (float *)c.grad_value, (float *)nullptr, (float *)nullptr,
                         c.grad_proj, c.grad_ref_part, (unsigned)c.value_bytes, (unsigned)(c.value_elems * 4),
                         (unsigned *)nullptr, 0u, 0u);
    } else if (fused && !soft16) {       // (soft16: finished by the dots kernel)
        rc = launch_fused_finish(c, src_k, true, rows16, offsets_done);
    }
    if (rc) return rc;
    // 3. scan -> emit -> gather -> reduce
    const int egrid = (N * M * ((sp.nchunk + sp.emult - 1) / sp.emult) + 7) & ~7;
    hipLaunchKernelGGL(msda_bwd_sort_scan, dim3(N * M), dim3(kSortThreads), 0, c.stream, sp);
    rc = launch_side("msda_bwd_sort_emit", msda_bwd_sort_emit, dim3(egrid), dim3(kSortThreads), (size_t)sp.nbk * 4, c.stream,
                     c.shapes, c.lstart, src_k, fused_loc, soft16, sp);
    if (rc) return rc;
    const bool b16 = sizeof(TV) == 2;
    g_kernel = fused ? (b16 ? "msda_bwd_d32_sorted<bf16,fused>" : "msda_bwd_d32_sorted<fused>")
                     : (b16 ? "msda_bwd_d32_sorted<bf16>" : "msda_bwd_d32_sorted");
    rc = launch_side(g_kernel, msda_bwd_sort_gather<TV>, dim3((N * M * sp.max_items + 7) & ~7), dim3(kSortThreads),
                     (size_t)(kSortSlice + 2) * 8 + (size_t)kSortBP * 8, c.stream, c.grad_out, (float *)c.grad_value, sp,
                     (unsigned)((size_t)n_rows * 32 * sizeof(TV)));
    if (rc) return rc;
    return launch_side("msda_bwd_sort_reduce", msda_bwd_sort_reduce, dim3((N * M * sp.nbk + 7) & ~7), dim3(kSortThreads), 0,
                       c.stream, (float *)c.grad_value, sp);
}

// What the selector decided for the counting-sort kernel: its record, the level, the window margin.
struct BinsSel {
    SelSlot *slot = nullptr;
    int level = 0, margin = 0, shrink = 0;
};

inline const char *bins_name(int ni, bool b16, bool split) {
    if (ni == 2)
        return split ? (b16 ? "msda_bwd_d32_tile_bins<bf16,split>" : "msda_bwd_d32_tile_bins<split>")
                     : (b16 ? "msda_bwd_d32_tile_bins<bf16>" : "msda_bwd_d32_tile_bins");
    return split ? (b16 ? "msda_bwd_d32_tile_bins<3,bf16,split>" : "msda_bwd_d32_tile_bins<3,split>")
                 : (b16 ? "msda_bwd_d32_tile_bins<3,bf16>" : "msda_bwd_d32_tile_bins<3>");
}

template <int NI, bool SOFT, typename C>
void launch_bins(const C &c, const PointSrc &src, const TilePlan &pl, const BinsPlan &bp, int grid, size_t lds) {
    using TV = typename C::TV;
    hipLaunchKernelGGL((msda_bwd_d32_bins<NI, TV, SOFT>), dim3(grid), dim3(kTileThreads), lds, c.stream, c.value, c.lstart, src,
                       c.grad_out, (float *)c.grad_value, (float *)c.grad_loc, (float *)c.grad_attn, c.grad_proj, pl, bp,
                       SOFT ? c.fwd_out : (const TV *)nullptr);
}

template <bool FU, typename C>
int launch_tile_lv(const C &c, const char *name, const PointSrc &src, const TilePlan &pl, int grid, size_t lds) {
    using TV = typename C::TV;
    if (const int rc = allow_big_lds(msda_bwd_d32_tile_lv<2, TV, FU>, lds)) return rc;
    g_kernel = name;
    hipLaunchKernelGGL((msda_bwd_d32_tile_lv<2, TV, FU>), dim3(grid), dim3(kTileThreads), lds, c.stream, c.value, c.lstart, src,
                       c.grad_out, (float *)c.grad_value, (float *)c.grad_loc, (float *)c.grad_attn, c.grad_proj, pl);
    return MSDA_OK;
}

// ---- pyramid self-attention, one pyramid level per workgroup: the counting-sort gather (msda_bwd_bins.h, `bins`) or the
//      region-tiled fixed-point windows (msda_bwd_tile_lv.h).  bins hands over to tile_lv when P > 8, when a fused call
//      cannot be split (the one-kernel fused form stays with tile_lv) or when its LDS plan does not fit; tile_lv without
//      a plan (or P > 8): not taken ----
template <typename C>
int bwd_pyramid(const C &c, bool bins, const BinsSel &bs) {
    using TV = typename C::TV;
    const int L = c.L, P = c.P;
    const long n_rows = c.n_rows;
    const bool fused = c.fused, b16 = sizeof(TV) == 2;
    // `fwd_out` (round 6): the forward's output of the same call, when the caller still holds it.  sum_j a_j ga_j of the
    // softmax Jacobian IS <grad_out_row, out_row>, so with it the counting-sort backward needs no side kernel
    const bool soft_ok = fused && c.fwd_out != nullptr && sizeof(TV) == 4 && c.fa.ref_dim == 2 && (c.fa.proj_stride % 4) == 0 &&
                         ((2 * c.M * L * P) % 4) == 0 && (((uintptr_t)c.fa.proj) & 15) == 0 && L == 4 && P == 4 &&
                         c.grad_ref_part == nullptr && opt_bwd_soft.load() != 0;
    const bool ws_ok = c.workspace != nullptr && c.workspace_bytes >= (size_t)n_rows * L * P * 3 * sizeof(float);
    const bool can_split = fused && opt_bwd_split.load() != 0;
    if (bins && (P > 8 || (fused && !(can_split && (soft_ok || ws_ok))))) bins = false;
    TilePlan pl;
    size_t lds_all = 0, bins_lds = 0;
    BinsPlan bp;
    memset(&bp, 0, sizeof(bp));
    int bins_ni = 0;
    if (bins) {
        if (make_tile_plan(pl, c.shapes_host, c.N, c.S, c.M, c.D, L, c.Lq, P, c.value_bytes, bs.margin, 0, 8, 0, lds_all, false))
            for (int ni = 2; ni <= 3 && !bins_ni; ++ni)
                if (make_bins_plan(bp, pl, ni, bins_lds)) bins_ni = ni;
        bins = bins_ni != 0;
        bp.shrink = bs.shrink;
        bp.level = bs.level;
        // (cumulative counters, fixed addresses: a captured launch counts like an eager one)
        bp.stats = bs.slot ? bs.slot->dev : nullptr;
        bp.stats_host = bs.slot ? bs.slot->host_dev : nullptr;
    }
    if (!bins && !(P <= 8 && make_tile_plan(pl, c.shapes_host, c.N, c.S, c.M, c.D, L, c.Lq, P, c.value_bytes,
                                            opt_bwd_tile_margin.load(), 0, 8, 0, lds_all)))
        return kNotTaken;
    int win_max = 0;
    for (int l = 0; l < L; ++l) win_max = pl.win[l] > win_max ? pl.win[l] : win_max;
    const size_t lds = bins ? bins_lds : (size_t)(win_max * win_max + 8) * 128 + (size_t)32 * (2 * P + 1) * 16;
    const int grid = (pl.n_blocks * L + 7) & ~7;
    PointSrc src = c.src();
    pl.ablate = opt_bwd_ablate.load();
    pl.wide_log2 = opt_bwd_wide_log2.load();
    // Split fused backward (needs the caller's workspace): materialise the prologue once -- the tiled
    // kernel would otherwise redo the row softmax and the location arithmetic in each of its L
    // workgroups per region -- run the plain kernel on it, finish the Jacobians in place.
    const bool soft = soft_ok && bins && opt_bwd_split.load() != 0;      // (no workspace needed)
    const bool split = can_split && (soft || ws_ok);
    // The counting-sort kernel computes the locations itself (one lane per point: the arithmetic is
    // cheap there) and, for 2-d reference points, writes the final offset gradients: the two side
    // kernels then move a third of the bytes (attention weights out, the softmax Jacobian in place).
    const bool slim = split && bins && side_slim(c, false);
    const int offsets_done = slim && c.fa.ref_dim == 2 ? 1 : 0;
    bp.fused_loc = slim ? 1 : 0;
    bp.offsets_done = offsets_done;
    bp.soft = soft ? 1 : 0;
    bool rows16 = false;
    int rc;
    if (split && !soft) {
        float *loc_ws = c.workspace, *attn_ws = c.workspace + (size_t)n_rows * L * P * 2;
        rows16 = slim && side_rows16(c, false);
        if ((rc = launch_fused_prologue(c, src, rows16, slim ? (float *)nullptr : loc_ws, attn_ws))) return rc;
        src.loc = loc_ws;
        src.attn = attn_ws;
    }
    if (bins && soft) {       // (fp32, L = P = 4) everything of the fused backward in the one kernel
        if constexpr (sizeof(TV) == 4) {
            g_kernel = bins_ni == 2 ? "msda_bwd_d32_tile_bins<split,soft>" : "msda_bwd_d32_tile_bins<3,split,soft>";
            if (bins_ni == 2) launch_bins<2, true>(c, src, pl, bp, grid, lds);
            else launch_bins<3, true>(c, src, pl, bp, grid, lds);
        }
    } else if (bins) {
        g_kernel = bins_name(bins_ni, b16, split);
        if (bins_ni == 2) launch_bins<2, false>(c, src, pl, bp, grid, lds);
        else launch_bins<3, false>(c, src, pl, bp, grid, lds);
    } else {
        if (split) rc = launch_tile_lv<false>(c, b16 ? "msda_bwd_d32_tile_lv<2,bf16,split>" : "msda_bwd_d32_tile_lv<2,split>", src, pl, grid, lds);
        else if (fused) rc = launch_tile_lv<true>(c, b16 ? "msda_bwd_d32_tile_lv<2,bf16,fused>" : "msda_bwd_d32_tile_lv<2,fused>", src, pl, grid, lds);
        else rc = launch_tile_lv<false>(c, b16 ? "msda_bwd_d32_tile_lv<2,bf16>" : "msda_bwd_d32_tile_lv<2>", src, pl, grid, lds);
        if (rc) return rc;
    }
    rc = check_launch(g_kernel);
    if (rc || !fused || soft) return rc;
    return launch_fused_finish(c, src, split, rows16, offsets_done);
}

// ---- rows: few-query calls at D = 32 (the decoder's cross-attention): 32 lanes per row, grad_value atomics in whole
//      128-byte rows, four points in flight (msda_bwd_rows.h) ----
template <typename C>
int bwd_rows(const C &c) {
    using TV = typename C::TV;
    if (!(c.can32 && c.L * c.P <= kRowsMaxLP && (opt_bwd_rows.load() != 0 || c.strided) && c.n_rows < (1L << 31)))
        return kNotTaken;
    const PointSrc src = c.src();
    // a row is a chain of dependent round trips (stage -> loads -> atomics -> reductions): small calls get one
    // wavefront (two rows) per workgroup so that every CU holds several chains
    int threads = opt_bwd_rows_block.load();
    if (threads != 64 && threads != 128 && threads != 256) threads = c.n_rows <= 16384 ? 64 : 256;
    const int per = threads / 32;
    const int grid = clamp_grid((c.n_rows + per - 1) / per, 64);
    const unsigned gv_bytes = (unsigned)(c.value_elems * 4), pix_elems = (unsigned)(c.strided ? c.vstride : 0);
    const bool b16 = sizeof(TV) == 2;
    if (c.fused) {
        g_kernel = b16 ? "msda_bwd_d32_rows<bf16,fused>" : "msda_bwd_d32_rows<fused>";
        hipLaunchKernelGGL((msda_bwd_d32_rows<TV, true>), dim3(grid), dim3(threads), 0, c.stream, c.value, c.shapes, c.lstart,
                           src, c.grad_out, c.N, c.S, c.M, c.L, c.Lq, c.P, (float *)c.grad_value, (float *)nullptr,
                           (float *)nullptr, c.grad_proj, c.grad_ref_part, (unsigned)c.value_bytes, gv_bytes,
                           (unsigned *)nullptr, 0u, pix_elems);
    } else {
        g_kernel = b16 ? "msda_bwd_d32_rows<bf16>" : "msda_bwd_d32_rows";
        hipLaunchKernelGGL((msda_bwd_d32_rows<TV, false>), dim3(grid), dim3(threads), 0, c.stream, c.value, c.shapes, c.lstart,
                           src, c.grad_out, c.N, c.S, c.M, c.L, c.Lq, c.P, (float *)c.grad_value, (float *)c.grad_loc,
                           (float *)c.grad_attn, (float *)nullptr, (float *)nullptr, (unsigned)c.value_bytes, gv_bytes,
                           (unsigned *)nullptr, 0u, pix_elems);
    }
    return check_launch(g_kernel);
}

// ---- generic: one block per (n, q, m) row, any D / dtype ----
template <typename C>
int bwd_generic(const C &c) {
    using TV = typename C::TV; using TC = typename C::TC; using TG = typename C::TG;
    int block = ((c.D + 63) / 64) * 64;
    if (block > 1024) block = 1024;
    const int grid = (int)(c.n_rows < 65536L * 16 ? c.n_rows : 65536L * 16);
    if constexpr (sizeof(TC) == 4) {
        if (c.fused) {
            g_kernel = "msda_bwd_generic<fused>";
            hipLaunchKernelGGL((msda_bwd_generic<TV, TC, TG, true>), dim3(grid), dim3(block), 0, c.stream, c.value, c.shapes,
                               c.lstart, (const TC *)nullptr, (const TC *)nullptr, c.src(), c.grad_out, c.N, c.S, c.M, c.D, c.L,
                               c.Lq, c.P, c.grad_value, (TC *)nullptr, (TC *)nullptr, c.grad_proj, c.grad_ref_part);
            return check_launch(g_kernel);
        }
    }
    g_kernel = "msda_bwd_generic";
    hipLaunchKernelGGL((msda_bwd_generic<TV, TC, TG, false>), dim3(grid), dim3(block), 0, c.stream, c.value, c.shapes, c.lstart,
                       c.loc, c.attn, PointSrc{}, c.grad_out, c.N, c.S, c.M, c.D, c.L, c.Lq, c.P, c.grad_value, c.grad_loc,
                       c.grad_attn, (float *)nullptr, (float *)nullptr);
    return check_launch(g_kernel);
}

// The driver.  Order of the paths, each handing a call it cannot take to the next:
//     sorted -> rows -> generic            bins -> tile_lv -> rows -> generic
// (sorted does its own zeroing of grad_value, together with its bucket totals; every other path starts behind the
//  zeroing launch.)  "bwd_variant" 1 is the generic kernel outright.
//   option 0: pyramid self-attention (can_tile) follows the selector (msda_select.h) -- level 0 / 1: bins at the small /
//             large window margin; level 2: sorted, or rows with "bwd_sorted" 0; every other call -> rows
//   a strided `value` / `grad_value` -> rows, whatever the option
// Measured on MI355X (profiles/): per-contribution global float atomics cap the backward at ~1.1 ms for the encoder call
// (L2 atomic throughput; the row-per-block kernel's 32-consecutive-lane pattern is the fastest of them).  Self-attention
// over the pyramid (Lq == S, host shapes known) therefore takes the counting-sort kernel (round 4: 145 us at the encoder
// shape; tile_lv 218, tile_q2 317), at the window margin the measured off-window share asks for -- or, when most points
// leave even the large window (uniformly random locations), no windows at all.
template <typename C>
int backward_impl(C &c) {
    using TV = typename C::TV;
    bool empty = false;
    int rc = finish_call(c, c.grad_out, true, empty);
    if (rc) return rc;
    if (empty) return zero_launch(c, nullptr, 0u);
    bool automatic = false;
    BwdPath path = bwd_path_of(opt_bwd_variant.load(), automatic);
    // `value` and `grad_value` as slices of wider tensors (msda_next_value_pixel_stride): the rows kernel only, and the
    // caller owns the zeroing of the whole gradient tensor
    if (c.strided) { automatic = false; path = BwdPath::rows; }
    BinsSel bs;
    bs.margin = opt_bwd_bins_margin.load();
    if (c.can_tile && (automatic || path == BwdPath::bins)) {
        bs.slot = sel_acquire(1, c.M, c.L, c.P, (int)sizeof(TV), c.stream);
        bool probe = false;
        bs.level = sel_level(bs.slot, 1, probe, bs.slot != nullptr && stream_capturing(c.stream));
        if (!automatic) bs.level = opt_sel_level.load() >= 0 ? bs.level : 0;         // forced: the selector only measures
        if (bs.level >= 1) {
            bs.shrink = opt_bwd_bins_margin_hi.load() - bs.margin;
            bs.margin = opt_bwd_bins_margin_hi.load();
            if (bs.shrink < 0) bs.shrink = 0;
        }
        if (automatic) path = bs.level >= 2 ? (opt_bwd_sorted.load() ? BwdPath::sorted : BwdPath::rows) : BwdPath::bins;
    } else if (automatic) {
        path = BwdPath::rows;
    }
    if constexpr (C::kD32Type) {
        if (path == BwdPath::sorted && (rc = bwd_sorted(c)) != kNotTaken) return rc;
    }
    if ((rc = zero_launch(c, nullptr, 0u))) return rc;
    if constexpr (C::kD32Type) {
        if ((path == BwdPath::bins || path == BwdPath::tile_lv) && c.can_tile &&
            (rc = bwd_pyramid(c, path == BwdPath::bins, bs)) != kNotTaken)
            return rc;
        if (path != BwdPath::generic && (rc = bwd_rows(c)) != kNotTaken) return rc;
    }
    return bwd_generic(c);
}
