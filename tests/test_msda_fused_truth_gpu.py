"""The fused deformable-attention entry points against float64 truth (run with ``-m gpu`` on an MI355X).

tests/msda_fused_truth.py holds the truth, the derived per-element bounds (the in-kernel softmax and the prologue's
Jacobians included) and the case matrix; tests/test_msda_fused_truth_cpu.py shows that the float32 statement of the
operation stays inside those bounds on these inputs and that nine subtly wrong kernels do not.  Here every call

  * forces its path through the library's options (``forced`` of tests/test_msda_truth_gpu.py puts them back) and
    asserts the main kernel by name (``hip_lib.last_kernel()``);
  * first asserts that ``fused_points`` forms the locations of the CPU prologue bit for bit;
  * runs on a device copy of `value` whose masked rows, and one pixel no corner reads, hold +inf ("a padded pixel reads
    as 0"): every output stays finite;
  * asserts exact zeros in the grad_proj columns of the row that samples out of range, in grad_value's masked rows and
    in the cells nothing reaches, and the same grad_proj bits from a second call;
  * prints ``MSDA_FUSED_TRUTH <path> <case> <dtype> <kernel> out=.. grad_value=.. grad_proj=.. grad_ref=..`` (worst
    error / bound; "-": not produced by this call) and asserts every ratio <= 1.  profiles/msda_fused_truth.md records
    one run.  No threshold comes from those figures.

Which side kernels run (msda_dispatch_bwd.h: side_rows16, side_slim, offsets_done, soft16, soft) is not visible in a
name; the cases are built so that each choice is taken by some call and declined by another:
    fpyr4     L P = 16, 2-d, pitches multiples of 4   rows16 + offsets_done (bins), soft16 (sorted), soft (with fwd_output)
    fpyr4r4   ... 4-d reference points                rows16 prologue, finish16 with the location Jacobian; soft declined
    fpyr3odd  proj width 54                           rows16 / soft declined: points16 / finish16 (slim)
    fpyr4p3   L P = 12                                slim without rows16
    fpyr4p5   L P = 20                                msda_fused_points_kernel / msda_fused_finish_kernel (8 lanes per row)
    fpyr4 + two spare proj columns (pitch 386)        rows16 / soft / soft16 declined at L P = 16
    bwd_side_rows 0 against 1 on fpyr4 / fpyr4r4      the same grad_proj bits (msda_fused_side.h says so)

Hand-overs at these sizes (the name asserted is the dispatcher's target):
    fpyr4p5, fpyr4p8, windowed forward   L P > 16: make_win_plan declines, msda_fwd_d32_gather<4,[bf16,]fused>
                                         (the in-kernel softmax past 16 points is the gather and generic kernels')
    fpyr4p8, bins                        85 rows x 8 points = 680 items > 512: the three-items-per-thread plan,
                                         msda_bwd_d32_tile_bins<3,..split>
    flp33, flp64                         L P > kRowsMaxLP = 32: rows -> msda_bwd_generic<fused>
    fgen16, fgen64                       D != 32: the generic kernels
Not reached: msda_bwd_d32_tile_bins<3,split,soft> (soft needs L = P = 4, the three-item plan rows * P > 512; a region has
at most 85 rows); msda_bwd_d32_rows<no atomics> behind the sorted backward (wanting grad_ref makes the wrapper withhold
the host shapes and the scratch, so sorted is never chosen with it -- no caller of the package asks for it either); the
windowed forward's non-default launch shapes (w2 / w3 / e2: tests/test_msda_fwd_win_gpu.py sweeps them).
"""
import numpy as np
import pytest
import torch

import msda_fused_truth as ft
import msda_truth as mt
from test_msda_truth_gpu import forced

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(True, id="bf16"), pytest.param(False, id="f32")]
FPYR = [t for t in ft.TAGS if t.startswith("fpyr")]
D32 = [t for t in ft.TAGS if ft.CASES[t][3] == 32]


@pytest.fixture(scope="module")
def msda(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from memotr_amd import MultiScaleDeformableAttention as MSDA
    return MSDA


_DEVICE = {}


def device_case(g, T, bf16, spare):
    """The case on the device (shared, read-only).  Masked rows of the kernel's `value`, and one pixel no corner reads
    where there is one, hold +inf."""
    key = (g["tag"], bf16, spare)
    if key not in _DEVICE:
        from memotr_amd.MultiScaleDeformableAttention import tag_host_shapes
        value = g["value"].copy()
        live = T["n_grad_value"] == 0
        if g["mask"] is not None:
            value[g["mask"]] = np.inf
            live &= ~g["mask"][..., None]
        unread = np.argwhere(live)
        if len(unread):
            n, s, m = unread[len(unread) // 2]
            value[n, s, m, :] = np.inf
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        d = dict(value=up(value), shapes=up(g["shapes"]), level_start=up(g["level_start"]), proj=up(g["proj"]), ref=up(g["ref"]),
                 mask=None if g["mask"] is None else up(g["mask"]), grad_out=up(g["grad_out"]))
        if bf16:
            d["value"], d["grad_out"] = d["value"].bfloat16(), d["grad_out"].bfloat16()      # (already bf16 values: exact)
        if g["pyramid"]:
            tag_host_shapes(d["shapes"], g["shapes_list"])
        _DEVICE[key] = d
    return _DEVICE[key]


def assert_locations_are_the_cpu_prologues(msda, d, g, T):
    loc, _ = msda.fused_points(d["shapes"], d["proj"], d["ref"], g["M"], g["P"])
    assert np.array_equal(loc.cpu().numpy().view(np.uint32), T["loc"].view(np.uint32))


def forward(msda, d, g):
    return msda.ms_deform_attn_fused_forward(d["value"], d["shapes"], d["level_start"], d["proj"], d["ref"], d["mask"],
                                             g["M"], g["P"])


def backward(msda, d, g, need_ref, out):
    return msda.ms_deform_attn_fused_backward(d["value"], d["shapes"], d["level_start"], d["proj"], d["ref"], d["mask"],
                                              d["grad_out"], g["M"], g["P"], need_ref_grad=need_ref, fwd_output=out)


def outside_columns(g):
    """(n, q, columns of proj) of the row that samples out of range."""
    N, S, M, D, L, Lq, P = g["dims"]
    n, q, m = ft.special_rows(N, Lq, M)[2]
    LP = L * P
    return n, q, m, np.r_[m * 2 * LP:(m + 1) * 2 * LP, g["n_off"] + m * LP:g["n_off"] + (m + 1) * LP]


def report(path, tag, bf16, kernel, r):
    print(f"\nMSDA_FUSED_TRUTH {path} {tag} {'bf16' if bf16 else 'f32'} {kernel} " +
          " ".join(f"{k}={r[k]:.3f}" if k in r else f"{k}=-" for k in ("out", "grad_value", "grad_proj", "grad_ref")))


def b16(bf16):
    return "bf16," if bf16 else ""


# ------------------------------------------------------------------------------------------------ forward
def gather_name(tag, bf16):
    return f"msda_fwd_d32_gather<4,{b16(bf16)}fused>"


def win_name(tag, bf16):
    """make_win_plan (msda_fwd_win.h) takes a row of at most 16 points -- the default launch shape, w4; past that the
    windowed path hands over to the gather kernel."""
    shapes, P = ft.CASES[tag][0], ft.CASES[tag][4]
    return f"msda_fwd_d32_win<{b16(bf16)}fused,w4>" if len(shapes) * P <= 16 else gather_name(tag, bf16)


FWD_PATHS = {
    "gather": (dict(fwd_variant=3), D32, gather_name),
    "win": (dict(fwd_variant=12), FPYR, win_name),
    "generic": (dict(fwd_variant=1), ft.TAGS, lambda tag, bf16: "msda_fwd_generic<fused>"),
}


def assert_kernel(kernel, want, bf16):
    assert kernel == want and ("bf16" in kernel) == (bf16 and "generic" not in kernel), (kernel, want)


@pytest.mark.parametrize("bf16", DTYPES)
@pytest.mark.parametrize("path,tag", [pytest.param(p, t, id=f"{p}-{t}") for p, s in FWD_PATHS.items() for t in s[1]])
def test_fused_forward_within_the_derived_bound(msda, hip_lib, path, tag, bf16):
    g, T, B = ft.case_with_truth(tag, bf16)
    d = device_case(g, T, bf16, 0)
    opts, _, name = FWD_PATHS[path]
    assert_locations_are_the_cpu_prologues(msda, d, g, T)
    with forced(hip_lib, **opts):
        out = forward(msda, d, g)
        kernel = hip_lib.last_kernel()
    assert out.dtype == (torch.bfloat16 if bf16 else torch.float32)
    out = out.float().cpu().numpy()
    assert_kernel(kernel, name(tag, bf16), bf16)
    r = dict(out=mt.worst_ratio(out, T["out"], B["out"]))
    report("fwd:" + path, tag, bf16, kernel, r)
    n, q, m, _ = outside_columns(g)
    D = g["dims"][3]
    assert np.isfinite(out).all()
    assert not out[n, q, m * D:(m + 1) * D].any()               # out of range: exact zeros
    assert r["out"] <= 1.0, r


# ------------------------------------------------------------------------------------------------ backward
def rows_name(tag, bf16):
    return f"msda_bwd_d32_rows<{b16(bf16)}fused>"


def generic_name(tag, bf16):
    return "msda_bwd_generic<fused>"


def tile_lv_name(form):
    return lambda tag, bf16: f"msda_bwd_d32_tile_lv<2,{b16(bf16)}{form}>"


def bins_name(soft=False):
    def name(tag, bf16):
        shapes, P = ft.CASES[tag][0], ft.CASES[tag][4]
        rows = sum(4 ** k for k in range(len(shapes)))
        ni = "" if rows * P <= 512 else "3,"                  # make_bins_plan: two items per thread, else three
        return f"msda_bwd_d32_tile_bins<{ni}{b16(bf16)}split{',soft' if soft else ''}>"
    return name


def sorted_name(tag, bf16):
    return f"msda_bwd_d32_sorted<{b16(bf16)}fused>"


def bwd_path(opts, tags, name, need_ref=None, pass_out=False, soft=False, tile_lv=False, dtypes=(True, False)):
    return dict(opts=opts, tags=tags, name=name, need_ref=need_ref, pass_out=pass_out, soft=soft, tile_lv=tile_lv, dtypes=dtypes)


ROWS_CASES = ["fdec77", "fdec17", "fdec1", "flp15", "flp32"]
BWD_PATHS = {
    # the decoder's kernel, every workgroup size; and the pyramids when the reference points want a gradient
    "rows_b64": bwd_path(dict(bwd_variant=0, bwd_rows_block=64), ROWS_CASES, rows_name),
    "rows_b128": bwd_path(dict(bwd_variant=0, bwd_rows_block=128), ROWS_CASES, rows_name),
    "rows_b256": bwd_path(dict(bwd_variant=0, bwd_rows_block=256), ROWS_CASES, rows_name),
    "rows_ref": bwd_path(dict(bwd_variant=0), FPYR, rows_name, need_ref=True),
    "generic": bwd_path(dict(bwd_variant=0), ["flp33", "flp64", "fgen16", "fgen64"], generic_name, need_ref=True),
    "generic_forced": bwd_path(dict(bwd_variant=1), ["fdec77"], generic_name),
    "tile_lv_fused_m0": bwd_path(dict(bwd_variant=10, bwd_split=0, bwd_tile_margin=0), FPYR, tile_lv_name("fused"), tile_lv=True),
    "tile_lv_fused_m4": bwd_path(dict(bwd_variant=10, bwd_split=0, bwd_tile_margin=4), FPYR, tile_lv_name("fused"), tile_lv=True),
    "tile_lv_split_m0": bwd_path(dict(bwd_variant=10, bwd_split=1, bwd_tile_margin=0), FPYR, tile_lv_name("split"), tile_lv=True),
    "tile_lv_split_m4": bwd_path(dict(bwd_variant=10, bwd_split=1, bwd_tile_margin=4), FPYR, tile_lv_name("split"), tile_lv=True),
    "bins_m0": bwd_path(dict(bwd_variant=12, bwd_split=1, bwd_bins_margin=0), FPYR, bins_name()),
    "bins_m3": bwd_path(dict(bwd_variant=12, bwd_split=1, bwd_bins_margin=3), FPYR, bins_name()),
    # the encoder's one-kernel backward: the forward's output handed over
    "soft": bwd_path(dict(bwd_variant=12, bwd_split=1), ["fpyr4"], bins_name(soft=True), pass_out=True, soft=True, dtypes=(False,)),
    "soft_default": bwd_path(dict(bwd_variant=0), ["fpyr4"], bins_name(soft=True), pass_out=True, soft=True, dtypes=(False,)),
    "soft_bf16_declined": bwd_path(dict(bwd_variant=12, bwd_split=1), ["fpyr4"], bins_name(), pass_out=True, dtypes=(True,)),
    "soft_declined": bwd_path(dict(bwd_variant=12, bwd_split=1), ["fpyr3odd", "fpyr4p3", "fpyr4r4"], bins_name(), pass_out=True),
    "soft_off": bwd_path(dict(bwd_variant=12, bwd_split=1, bwd_soft=0), ["fpyr4"], bins_name(), pass_out=True),
    "sorted": bwd_path(dict(bwd_variant=13), ["fpyr4", "fpyr4r4", "fpyr4p3", "fpyr4p5"], sorted_name),
}

_TILE_LV_BOUND = {}


def run_backward(msda, hip_lib, path, tag, bf16, spare=0, **more_opts):
    """One checked call of the fused backward on (path, case); returns the outputs as numpy and the kernel's name."""
    spec = BWD_PATHS[path]
    g, T, B = ft.case_with_truth(tag, bf16, spare)
    N, S, M, D, L, Lq, P = g["dims"]
    d = device_case(g, T, bf16, spare)
    need_ref = g["need_ref"] if spec["need_ref"] is None else spec["need_ref"]
    assert_locations_are_the_cpu_prologues(msda, d, g, T)
    with forced(hip_lib, **dict(spec["opts"], **more_opts)):
        out = forward(msda, d, g) if spec["pass_out"] else None
        gv, gp, gr = backward(msda, d, g, need_ref, out)
        kernel = hip_lib.last_kernel()
        gp_again = backward(msda, d, g, need_ref, out)[1]
    assert gv.dtype == (torch.bfloat16 if bf16 else torch.float32) and gp.dtype == torch.float32
    assert torch.equal(gp.view(torch.int32), gp_again.view(torch.int32))         # a second call: the same bits
    gv, gp = gv.float().cpu().numpy(), gp.cpu().numpy()
    bound_gv = B["grad_value"]
    if spec["tile_lv"]:
        key = (tag, bf16, spare)
        if key not in _TILE_LV_BOUND:
            _TILE_LV_BOUND[key] = ft.tile_lv_bound(g, T, B, bf16)
        bound_gv = _TILE_LV_BOUND[key]
    r = {}
    if out is not None:
        out = out.float().cpu().numpy()
        r["out"] = mt.worst_ratio(out, T["out"], B["out"])
    r["grad_value"] = mt.worst_ratio(gv, T["grad_value"], bound_gv)
    r["grad_proj"] = mt.worst_ratio(gp, T["grad_proj"], B["grad_proj_soft" if "soft" in kernel else "grad_proj"])
    if need_ref:
        assert gr.dtype == torch.float32
        gr = gr.cpu().numpy()
        r["grad_ref"] = mt.worst_ratio(gr, T["grad_ref"], B["grad_ref"])
    else:
        assert gr is None
    report("bwd:" + path + ("" if not spare else f"+spare{spare}") + "".join(f",{k}={v}" for k, v in more_opts.items()),
           tag, bf16, kernel, r)
    return dict(g=g, T=T, kernel=kernel, out=out, grad_value=gv, grad_proj=gp, grad_ref=gr, ratios=r)


def assert_backward(res, want_kernel, bf16):
    g, T, gv, gp = res["g"], res["T"], res["grad_value"], res["grad_proj"]
    assert_kernel(res["kernel"], want_kernel, bf16)
    assert all(np.isfinite(x).all() for x in (gv, gp, res["out"], res["grad_ref"]) if x is not None)
    n, q, m, cols = outside_columns(g)
    assert not gp[n, q, cols].any()                                  # out of range: exact zeros
    assert not gp[..., 3 * g["M"] * g["L"] * g["P"]:].any()          # spare columns stay zero
    assert not gv[T["n_grad_value"] == 0].any()                      # masked rows and cells nothing reaches
    assert max(res["ratios"].values()) <= 1.0, res["ratios"]


def backward_params():
    return [pytest.param(p, t, b, id=f"{p}-{t}-{'bf16' if b else 'f32'}")
            for p, s in BWD_PATHS.items() for t in s["tags"] for b in s["dtypes"]]


@pytest.mark.parametrize("path,tag,bf16", backward_params())
def test_fused_backward_within_the_derived_bound(msda, hip_lib, path, tag, bf16):
    res = run_backward(msda, hip_lib, path, tag, bf16)
    assert_backward(res, BWD_PATHS[path]["name"](tag, bf16), bf16)
    assert ("soft" in res["kernel"]) == BWD_PATHS[path]["soft"], res["kernel"]


@pytest.mark.parametrize("bf16", DTYPES)
@pytest.mark.parametrize("margin", [0, 3])
@pytest.mark.parametrize("tag", ["fpyr4", "fpyr4r4"])
def test_one_lane_per_row_side_kernels_give_the_general_side_kernels_bits(msda, hip_lib, tag, margin, bf16):
    """msda_fused_side.h: the rows16 prologue / finish associate like the 16-lane butterflies, "so the bits are theirs"."""
    path = f"bins_m{margin}"
    res = [run_backward(msda, hip_lib, path, tag, bf16, bwd_side_rows=v) for v in (1, 0)]
    for x in res:
        assert_backward(x, BWD_PATHS[path]["name"](tag, bf16), bf16)
    assert np.array_equal(res[0]["grad_proj"].view(np.uint32), res[1]["grad_proj"].view(np.uint32))


@pytest.mark.parametrize("bf16", DTYPES)
@pytest.mark.parametrize("path", ["bins_m0", "soft_off", "soft_declined", "sorted", "tile_lv_split_m4"])
def test_spare_proj_columns_decline_the_aligned_forms_and_stay_zero(msda, hip_lib, path, bf16):
    """proj two columns wider than 3 M L P on fpyr4: the row pitch (386) is no multiple of 4, so side_rows16, soft16 and
    soft are declined even with the forward's output handed over; the spare columns of grad_proj stay zero (asserted on
    every call) and nothing reads the spare columns of proj (random there)."""
    res = run_backward(msda, hip_lib, path, "fpyr4", bf16, spare=2)
    assert res["g"]["proj"].shape[2] == 3 * 8 * 16 + 2
    assert_backward(res, BWD_PATHS[path]["name"]("fpyr4", bf16), bf16)
    assert "soft" not in res["kernel"]
