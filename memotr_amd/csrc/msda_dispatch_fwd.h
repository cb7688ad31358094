// msda_dispatch_fwd.h -- host side of the forward: which kernel a call takes, and its launch.  Included by msda_hip.hip
// inside its anonymous namespace, after the kernels, the plans, the selector, the options and `Call`.  forward_impl (at the
// end) is the driver; a path returns kNotTaken when the call does not fit it.

enum class FwdPath { generic, gather, windowed };

// "fwd_variant": 0 auto | 1 generic | 12 windowed | every other number the gather kernel (2, 3, 4 once chose its points
// in flight; the numbers of kernels removed since land here too)
inline FwdPath fwd_path_of(int variant, bool &automatic) {
    automatic = variant == 0;
    return variant == 1 ? FwdPath::generic : (variant == 12 ? FwdPath::windowed : FwdPath::gather);
}

template <typename C>
int fwd_generic(const C &c) {
    using TV = typename C::TV; using TC = typename C::TC;
    const long total = (long)c.N * c.Lq * c.M * c.D;
    const int grid = clamp_grid((total + 255) / 256, 32);
    if constexpr (sizeof(TC) == 4) {
        if (c.fused) {
            g_kernel = "msda_fwd_generic<fused>";
            hipLaunchKernelGGL((msda_fwd_generic<TV, TC, true>), dim3(grid), dim3(256), 0, c.stream, c.value, c.shapes,
                               c.lstart, (const TC *)nullptr, (const TC *)nullptr, c.src(), c.N, c.S, c.M, c.D, c.L, c.Lq,
                               c.P, c.out);
            return check_launch(g_kernel);
        }
    }
    g_kernel = "msda_fwd_generic";
    hipLaunchKernelGGL((msda_fwd_generic<TV, TC, false>), dim3(grid), dim3(256), 0, c.stream, c.value, c.shapes, c.lstart,
                       c.loc, c.attn, PointSrc{}, c.N, c.S, c.M, c.D, c.L, c.Lq, c.P, c.out);
    return check_launch(g_kernel);
}

// Direct gather with 4 points (16 corner rows) in flight per lane: the best of the round-1 sweep,
// profiles/r01_kbench_fwd_sweep.txt; the 1- and 2-point instantiations went in round 5
template <typename C>
int fwd_gather(const C &c, bool sel_head_major) {
    using TV = typename C::TV;
    const PointSrc src = c.src();
    constexpr int ROWS = RowGeom<TV>::kRows;
    int block = opt_fwd_block.load();
    if (block < 64 || block > 256 || (block & 63)) block = 256;  // kernels carry __launch_bounds__(256)
    const int wpb = block / 64;
    const int head_major = (opt_fwd_head_major.load() != 0 || sel_head_major) && (long)c.N * c.Lq >= 4096 ? 1 : 0;
    const long n_tasks = head_major ? (((long)c.N * c.Lq + ROWS - 1) / ROWS) * c.M : (c.n_rows + ROWS - 1) / ROWS;
    // small problems: one wave per block so every task gets its own CU slot
    int use_block = block;
    if (n_tasks < (long)kNumCU * wpb) use_block = 64;
    const int uwpb = use_block / 64;
    int grid = clamp_grid((n_tasks + uwpb - 1) / uwpb, opt_fwd_grid_mult.load());
    grid = (grid + 7) & ~7;  // whole blocks per XCD residue
    const size_t lds = (size_t)uwpb * ROWS * (2 * c.L * c.P + 1) * 16;
    const unsigned pixel_bytes = (unsigned)((c.strided ? c.vstride : (long)c.M * c.D) * (long)sizeof(TV));
    auto launch = [&](auto fu) {
        hipLaunchKernelGGL((msda_fwd_d32_gather<4, TV, decltype(fu)::value>), dim3(grid), dim3(use_block), lds, c.stream,
                           c.value, c.shapes, c.lstart, src, c.N, c.S, c.M, c.L, c.Lq, c.P, c.out, (unsigned)c.value_bytes,
                           head_major, pixel_bytes);
    };
    const bool b16 = sizeof(TV) == 2;
    if (c.fused) {
        g_kernel = b16 ? "msda_fwd_d32_gather<4,bf16,fused>" : "msda_fwd_d32_gather<4,fused>";
        launch(std::true_type{});
    } else {
        g_kernel = b16 ? "msda_fwd_d32_gather<4,bf16>" : "msda_fwd_d32_gather<4>";
        launch(std::false_type{});
    }
    return check_launch(g_kernel);
}

// One instantiation of the windowed kernel: LDS opt-in, launch, check.
template <typename TV, bool FU, int WPS, int NE, bool TRACE = false, int PB = 4, typename C>
int launch_win(const C &c, const char *name, const PointSrc &src, const WinPlan &wp, int threads, size_t lds) {
    if (const int rc = allow_big_lds(msda_fwd_d32_win<TV, FU, WPS, NE, TRACE, PB>, lds)) return rc;
    g_kernel = name;
    hipLaunchKernelGGL((msda_fwd_d32_win<TV, FU, WPS, NE, TRACE, PB>), dim3((wp.n_blocks + 7) & ~7), dim3(threads), lds,
                       c.stream, c.value, c.lstart, src, c.out, wp);
    return check_launch(g_kernel);
}

// Region shape and workgroup size of the windowed forward (options; 0 = auto).  Round 5: 16 x 16-pixel regions and 512
// threads -- 340 rows share one set of windows and one prologue (8 x 8: 85), two workgroups = 16 wavefronts per CU at 128
// registers; border regions hold only the rows that exist and are walked last, so the 616 workgroups of one 800 x 1333
// image end together on the 512 slots (46.0 vs 55.1 us fused, N = 5: 224 vs 289 us; profiles/r05_fwd_win_sweep_*.txt).
// A geometry that shape cannot take falls back to 8 x 8 / 256.  False: the windowed kernel does not apply to this call.
template <typename C>
bool fwd_win_plan(const C &c, const PointSrc &src, WinPlan &wp, size_t &lds, int &threads) {
    using TV = typename C::TV;
    const int mgs = opt_fwd_win_margins.load(), l0 = opt_fwd_win_l0.load(), eb = (int)sizeof(TV);
    const int margins[kWinMaxL] = {mgs & 15, (mgs >> 4) & 15, (mgs >> 8) & 15, (mgs >> 12) & 15};
    threads = opt_fwd_win_block.load();
    int rlogy = opt_fwd_win_rlog.load(), rlogx = opt_fwd_win_rlogx.load();
    const bool auto_shape = threads == 0 && rlogy == 0 && rlogx == 0;
    if (threads != 512 && threads != 384 && threads != 128 && threads != 256) threads = auto_shape ? 512 : 256;
    if (rlogy == 0) rlogy = auto_shape ? 4 : 3;
    if (rlogx == 0) rlogx = rlogy;
    constexpr int kMaskGroups = sizeof(TV) == 4 ? 8 : 4;      // fill groups a wavefront's lanes cover per level
    auto mask_fits = [&](const WinPlan &p) { return !(src.mask != nullptr && p.wgroups_max > kMaskGroups * (threads / 64)); };
    bool planned = make_win_plan(wp, c.shapes_host, c.N, c.S, c.M, c.D, c.L, c.Lq, c.P, c.value_bytes, rlogx, rlogy, l0,
                                 margins, threads, lds, eb) && mask_fits(wp);
    // Equal regions of any size (make_win_plan_grid) where they fill the workgroup slots in fewer rounds than the
    // power-of-two ones: asked for by size ("fwd_win_rsy" / "fwd_win_rsx"), or chosen by estimate for the default shape
    // (win_grid_choice, cached per geometry)
    int rsy = opt_fwd_win_rsy.load(), rsx = opt_fwd_win_rsx.load();
    if (rsy <= 0 && rsx <= 0 && auto_shape && planned && opt_fwd_win_grid.load() != 0 && sizeof(TV) == 4)
        win_grid_choice(wp, c.shapes_host, c.N, c.S, c.M, c.D, c.L, c.Lq, c.P, c.value_bytes, l0, margins, threads, mgs,
                        rsy, rsx);
    if (rsy > 0 || rsx > 0) {
        if (rsy <= 0) rsy = rsx;
        if (rsx <= 0) rsx = rsy;
        WinPlan gp;
        size_t glds = 0;
        if (make_win_plan_grid(gp, c.shapes_host, c.N, c.S, c.M, c.D, c.L, c.Lq, c.P, c.value_bytes, rsy, rsx, l0, margins,
                               threads, glds, eb) && mask_fits(gp)) {
            wp = gp;
            lds = glds;
            planned = true;
        }
    }
    if (!planned && auto_shape) {
        threads = 256;
        planned = make_win_plan(wp, c.shapes_host, c.N, c.S, c.M, c.D, c.L, c.Lq, c.P, c.value_bytes, 3, 3, l0, margins,
                                threads, lds, eb) && mask_fits(wp);
    }
    // (bf16 rows: the default shape only -- 512 threads, no early loads, no profiling build; else the gather)
    if (sizeof(TV) == 2 && (threads != 512 || opt_fwd_win_ablate.load() != 0 || opt_fwd_win_trace_lo.load() != 0 ||
                            opt_fwd_win_trace_hi.load() != 0))
        planned = false;
    return planned;
}

// Pyramid self-attention (msda_fwd_win.h): plan, statistics record, register budget, then the table of instantiations.
template <typename C>
int fwd_windowed(const C &c, SelSlot *slot, int sel) {
    using TV = typename C::TV;
    const PointSrc src = c.src();
    const bool fused = c.fused;
    WinPlan wp;
    size_t lds = 0; int threads = 0;
    if (!fwd_win_plan(c, src, wp, lds, threads)) return kNotTaken;
    wp.ablate = opt_fwd_win_ablate.load();
    wp.trace = reinterpret_cast<unsigned long long *>(((unsigned long long)opt_fwd_win_trace_hi.load() << 31) |
                                                      (unsigned long long)opt_fwd_win_trace_lo.load());
    // The kernel's publisher is wavefront 1: a 64-thread workgroup (options only) runs without statistics.
    // (The share's denominator counts a wavefront's staged rows sixteen steps per ballot, any step count.)
    const bool stats_ok = slot != nullptr && threads / 64 >= 2;
    if (stats_ok) {     // (cumulative counters, fixed addresses: a captured launch counts like an eager one)
        wp.stats = slot->dev;
        wp.stats_host = slot->host_dev;
        wp.sel_level = sel;
    }
    // windows placed from the record's running mean offsets (no round trip in front of the fill); without
    // a record, or on request, every workgroup measures its own first ("fwd_win_place" 1)
    wp.measure = (!stats_ok || c.M > kSelHintHeads || c.L > kSelHintLevels || opt_fwd_win_place.load() != 0) ? 1 : 0;
    // register budget by what the workgroup shape admits: three 256-thread workgroups per CU (40-53 KB
    // of LDS each) -> 168 registers, all four level-0 points requested before the LDS phase; 512-thread
    // workgroups (two per CU) or four small ones -> 128 registers, two of them
    int wps = opt_fwd_win_wps.load();
    const bool wide = wps == 2 && threads <= 256 && sizeof(TV) == 4 && !wp.trace && !wp.ablate;
    if (wps != 3 && wps != 4) wps = (threads <= 256 && lds + 640 > 40 * 1024) ? 3 : 4;
    int early = opt_fwd_win_early.load();          // 0 / 2 / 4 points; anything else: by budget
    if (threads > 256) {
        wps = 4;
        if (early == 4) early = 2;
    }
    if (early != 0 && early != 2 && early != 4) early = wps == 3 ? 4 : kWinEarlyW4;
    if (early == 4) wps = 3;
    // (the profiling instantiation -- timeline stamps, ablation bits -- exists for the default shape only)
    const bool profiling = wp.trace || wp.ablate;
    if (profiling && (wps == 3 || early == 2))
        return fail(MSDA_EINVAL, "fwd_win_trace / fwd_win_ablate: profiling build of the default launch shape only");
    if constexpr (sizeof(TV) == 2) {       // bf16 rows: the default shape only (512 threads, no early loads)
        return fused ? launch_win<TV, true, 4, 0>(c, "msda_fwd_d32_win<bf16,fused,w4>", src, wp, threads, lds)
                     : launch_win<TV, false, 4, 0>(c, "msda_fwd_d32_win<bf16,w4>", src, wp, threads, lds);
    } else {
        if (wide) {     // "fwd_win_wps" 2: two wavefronts per SIMD, 256 registers, twelve LDS points per wait
            // (six points per wait, "p6", was built and measured too: 67.5 / 70.1 us against p12's 65.9 / 68.6
            //  -- profiles/r06_fwd_win_sweep_wide.txt; not kept in the library)
            const bool e4 = opt_fwd_win_early.load() == 4;
            if (fused)
                return e4 ? launch_win<TV, true, 2, 4, false, 12>(c, "msda_fwd_d32_win<fused,w2,e4,p12>", src, wp, threads, lds)
                          : launch_win<TV, true, 2, 0, false, 12>(c, "msda_fwd_d32_win<fused,w2,p12>", src, wp, threads, lds);
            return e4 ? launch_win<TV, false, 2, 4, false, 12>(c, "msda_fwd_d32_win<w2,e4,p12>", src, wp, threads, lds)
                      : launch_win<TV, false, 2, 0, false, 12>(c, "msda_fwd_d32_win<w2,p12>", src, wp, threads, lds);
        }
        if (wps == 3)
            return fused ? launch_win<TV, true, 3, 4>(c, "msda_fwd_d32_win<fused,w3,e4>", src, wp, threads, lds)
                         : launch_win<TV, false, 3, 4>(c, "msda_fwd_d32_win<w3,e4>", src, wp, threads, lds);
        if (early == 2)
            return fused ? launch_win<TV, true, 4, 2>(c, "msda_fwd_d32_win<fused,w4,e2>", src, wp, threads, lds)
                         : launch_win<TV, false, 4, 2>(c, "msda_fwd_d32_win<w4,e2>", src, wp, threads, lds);
        if (fused)
            return profiling ? launch_win<TV, true, 4, 0, true>(c, "msda_fwd_d32_win<fused,w4>", src, wp, threads, lds)
                             : launch_win<TV, true, 4, 0>(c, "msda_fwd_d32_win<fused,w4>", src, wp, threads, lds);
        return profiling ? launch_win<TV, false, 4, 0, true>(c, "msda_fwd_d32_win<w4>", src, wp, threads, lds)
                         : launch_win<TV, false, 4, 0>(c, "msda_fwd_d32_win<w4>", src, wp, threads, lds);
    }
}

// The driver.  Order of the paths: windowed -> gather; generic stands alone (every call it is chosen for, it takes).
//   option 0: fp32 pyramid self-attention with host shapes (bf16 with "fwd_win_bf16") -> windowed, or the head-major
//             gather when the selector says the points have left the windows; other D = 32 calls -> gather; else generic
//   a strided `value` -> gather, whatever the option; any specialised path without D = 32 storage -> generic
template <typename C>
int forward_impl(C &c) {
    using TV = typename C::TV;
    bool empty = false;
    if (const int rc = finish_call(c, c.out, false, empty)) return rc;
    if (empty) { g_err[0] = 0; return MSDA_OK; }
    bool automatic = false;
    FwdPath path = fwd_path_of(opt_fwd_variant.load(), automatic);
    // `value` as a slice of a wider tensor (msda_next_value_pixel_stride): the gather kernel only -- the call sites that
    // use it are the decoder's (a few hundred queries), which take that kernel anyway
    if (c.strided) { automatic = false; path = FwdPath::gather; }
    SelSlot *slot = nullptr;
    int sel = 0; bool sel_head_major = false;
    if (automatic) {
        // self-attention over the pyramid (one query per pixel): coarse levels from per-head LDS windows; every
        // other D = 32 call: direct gather with 4 points (16 rows) in flight -- best of the sweeps in profiles/
        // (bf16 rows, round 6: the same kernel on 64-byte rows exists -- "fwd_win_bf16" 1 or "fwd_variant" 12 -- and is
        //  slower than the gather kernel: halving the LDS bytes bought nothing, the widening costs VALU)
        const bool pyramid = c.can32 && (sizeof(TV) == 4 || opt_fwd_win_bf16.load() != 0) && c.shapes_host != nullptr &&
                             c.Lq == c.S && c.L <= kWinMaxL && c.L * c.P <= 16 && opt_fwd_win_auto.load() != 0;
        path = pyramid ? FwdPath::windowed : (c.can32 ? FwdPath::gather : FwdPath::generic);
        if (pyramid) {      // msda_select.h: windows while the points stay near their queries, else the head-major gather
            slot = sel_acquire(0, c.M, c.L, c.P, (int)sizeof(TV), c.stream);
            bool probe = false;
            sel = sel_level(slot, 0, probe, slot != nullptr && stream_capturing(c.stream));
            // "deterministic": the windowed and the gather kernel add a row's points in different orders (same values to
            // 2e-5, different last bits), and the selector moves a call site between them from statistics of EARLIER calls;
            // with the option on, identical calls return identical bits -- the windowed kernel's, whose results do not depend
            // on where its windows sit (the record keeps measuring, nothing follows it)
            if (opt_deterministic.load()) sel = 0;
            if (sel >= 1) { path = FwdPath::gather; sel_head_major = true; }
        }
    } else if (path == FwdPath::windowed && c.can32 && c.shapes_host != nullptr) {
        slot = sel_acquire(0, c.M, c.L, c.P, (int)sizeof(TV), c.stream);     // forced: the selector only measures
        bool probe = false;
        (void)sel_level(slot, 0, probe, slot != nullptr && stream_capturing(c.stream));
    }
    if (path == FwdPath::generic || !c.can32) return fwd_generic(c);
    if constexpr (C::kD32Type) {
        if (path == FwdPath::windowed) {
            const int rc = fwd_windowed(c, slot, sel);
            if (rc != kNotTaken) return rc;
        }
        return fwd_gather(c, sel_head_major);
    }
    return fail(MSDA_ENOTSUP, "no specialised forward for this dtype");
}
