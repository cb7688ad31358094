"""Every bf16 deformable-attention path, and its fp32 twin, against float64 truth (run with ``-m gpu`` on an MI355X).

tests/msda_truth.py holds the truth, the derived per-element bounds and the case matrix; tests/test_msda_truth_cpu.py
shows that a correct kernel stays inside those bounds on these very inputs and that six subtly wrong ones do not.  Here
each kernel is forced through the library's options, asserted by name (``hip_lib.last_kernel()``) and held to

    |out - truth|        <= bound_bf16            (fp32: bound_f32)       every element
    |grad_value - truth| <= bound_bf16            accumulated in fp32, rounded once by the wrapper
                            (+ the fixed-point quantum for tile_lv: msda_truth.tile_lv_quantum)
    |grad_loc - truth|, |grad_attn - truth| <= bound_f32                 fp32 outputs on the bf16-rounded inputs

with exact zeros where a row samples out of range and an ``inf`` in a pixel no corner reads left unread (wherever the
case has such a pixel: on the dense pyramids every pixel is read).  Each test prints the worst error / bound per output;
profiles/msda_truth.md records them.  No threshold comes from those figures.

Kernels asserted by name, bf16 and fp32:
    forward   msda_fwd_d32_gather<4[,bf16]>, msda_fwd_d32_win<[bf16,]w4...> (the gather where the plan hands over),
              msda_fwd_generic (D = 16, 64), msda_fwd_d32_win<[bf16,]fused,w4> / msda_fwd_d32_gather<4[,bf16],fused>
    backward  msda_bwd_d32_rows[<bf16>], msda_bwd_d32_sorted[<bf16>], msda_bwd_d32_tile_bins[<bf16>] at margins 0 and 3,
              msda_bwd_d32_tile_lv<2[,bf16]> at margins 0 and 4, msda_bwd_generic (D = 16, 64)
Not reached at these sizes (the shapes are not enlarged for them): msda_bwd_d32_tile_bins<3,...> -- it needs the
two-items-per-thread LDS plan to fail, i.e. rows * P > 512, and a region has at most 85 rows; the split / soft / fused
backward instantiations belong to the fused entry: tests/test_msda_fused_truth_gpu.py holds them, the in-kernel softmax
and the prologue's Jacobians to float64 truth (tests/msda_fused_truth.py).  The fused FORWARD here is fed the points the
kernel itself exposes (``fused_points``), so the in-kernel softmax is not part of THIS file's budget.
"""
import numpy as np
import pytest
import torch

import msda_truth as mt

pytestmark = pytest.mark.gpu

OPTIONS = ("fwd_variant", "bwd_variant", "sel_level", "bwd_sorted", "fwd_win_bf16", "bwd_tile_margin", "bwd_bins_margin",
           "bwd_split", "bwd_soft", "bwd_side_rows", "bwd_rows_block")


@pytest.fixture(scope="module")
def msda(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from memotr_amd import MultiScaleDeformableAttention as MSDA
    return MSDA


class forced:
    """Set library options for one call sequence; every option of OPTIONS is back at its old value afterwards."""

    def __init__(self, lib, **opts):
        self.lib, self.opts = lib, opts

    def __enter__(self):
        self.saved = {k: self.lib.get_option(k) for k in OPTIONS}
        for k, v in self.opts.items():
            self.lib.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            self.lib.set_option(k, v)


def dev(a, bf16=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.bfloat16() if bf16 else t          # (already bf16 values: the cast is exact)


def device_args(g, t, bf16):
    """The case on the device.  Where a pixel exists that no corner reads, its `value` row is inf in the kernel's copy."""
    from memotr_amd.MultiScaleDeformableAttention import tag_host_shapes
    value = g["value"].copy()
    unread = np.argwhere(t["n_grad_value"] == 0)
    if len(unread):
        n, s, m = unread[len(unread) // 2]
        value[n, s, m, :] = np.inf
    shapes = dev(g["shapes"])
    if g["pyramid"]:
        tag_host_shapes(shapes, g["shapes_list"])
    return (dev(value, bf16), shapes, dev(g["level_start"]), dev(g["loc"]), dev(g["attn"])), len(unread) > 0


def report(what, case_id, bf16, kernel, r):
    print(f"\nMSDA_TRUTH {what} {case_id} {'bf16' if bf16 else 'f32'} {kernel} " +
          " ".join(f"{k}={v:.3f}" for k, v in r.items()))


def last_row(g):
    N, S, M, D, L, Lq, P = g["dims"]
    return N - 1, Lq - 1, M - 1, D


D32 = [c for c in mt.CASE_IDS if not c.startswith("gen")]
PYRAMIDS = [c for c in mt.CASE_IDS if c.startswith("pyr")]
GENERIC = [c for c in mt.CASE_IDS if c.startswith("gen")]

# path: (options, cases, kernel name for fp32, for bf16; a tuple: any of these prefixes)
FWD_PATHS = {
    "gather": (dict(fwd_variant=3), D32, "msda_fwd_d32_gather<4>", "msda_fwd_d32_gather<4,bf16>"),
    "win": (dict(fwd_variant=12), PYRAMIDS, ("msda_fwd_d32_win<w", "msda_fwd_d32_gather<4>"),
            ("msda_fwd_d32_win<bf16,w4>", "msda_fwd_d32_gather<4,bf16>")),
    "generic": (dict(), GENERIC, "msda_fwd_generic", "msda_fwd_generic"),
}
BWD_PATHS = {
    "rows": (dict(bwd_variant=0, sel_level=2, bwd_sorted=0), D32, "msda_bwd_d32_rows", "msda_bwd_d32_rows<bf16>"),
    "sorted": (dict(bwd_variant=13), D32, "msda_bwd_d32_sorted", "msda_bwd_d32_sorted<bf16>"),
    "bins_m0": (dict(bwd_variant=12, bwd_bins_margin=0), PYRAMIDS, "msda_bwd_d32_tile_bins", "msda_bwd_d32_tile_bins<bf16>"),
    "bins_m3": (dict(bwd_variant=12, bwd_bins_margin=3), PYRAMIDS, "msda_bwd_d32_tile_bins", "msda_bwd_d32_tile_bins<bf16>"),
    "tile_lv_m0": (dict(bwd_variant=10, bwd_tile_margin=0), PYRAMIDS, "msda_bwd_d32_tile_lv<2>", "msda_bwd_d32_tile_lv<2,bf16>"),
    "tile_lv_m4": (dict(bwd_variant=10, bwd_tile_margin=4), PYRAMIDS, "msda_bwd_d32_tile_lv<2>", "msda_bwd_d32_tile_lv<2,bf16>"),
    "generic": (dict(), GENERIC, "msda_bwd_generic", "msda_bwd_generic"),
}


def path_cases(paths):
    return [pytest.param(p, c, id=f"{p}-{c}") for p, spec in paths.items() for c in spec[1]]


def assert_kernel(name, want):
    if isinstance(want, tuple):
        assert any(name.startswith(w) for w in want), (name, want)
    else:
        assert name == want, (name, want)


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "f32"])
@pytest.mark.parametrize("path,case_id", path_cases(FWD_PATHS))
def test_forward_path_within_the_derived_bound(msda, hip_lib, path, case_id, bf16):
    g, t, b = mt.case_with_truth(case_id, bf16)
    opts, _, name32, name16 = FWD_PATHS[path]
    args, has_inf = device_args(g, t, bf16)
    with forced(hip_lib, **opts):
        out = msda.ms_deform_attn_forward(*args, 64)
        kernel = hip_lib.last_kernel()
    assert out.dtype == (torch.bfloat16 if bf16 else torch.float32)
    out = out.float().cpu().numpy()
    assert_kernel(kernel, name16 if bf16 else name32)
    r = dict(out=mt.worst_ratio(out, t["out"], b["out"]))
    report("fwd:" + path, case_id, bf16, kernel, r)
    n, q, m, D = last_row(g)
    assert not out[n, q, m * D:(m + 1) * D].any()               # out of range: exact zeros
    assert r["out"] <= 1.0, r


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "f32"])
@pytest.mark.parametrize("path,case_id", path_cases(BWD_PATHS))
def test_backward_path_within_the_derived_bound(msda, hip_lib, path, case_id, bf16):
    g, t, b = mt.case_with_truth(case_id, bf16)
    N, S, M, D, L, Lq, P = g["dims"]
    opts, _, name32, name16 = BWD_PATHS[path]
    args, has_inf = device_args(g, t, bf16)
    with forced(hip_lib, **opts):
        gv, gl, ga = msda.ms_deform_attn_backward(*args, dev(g["grad_out"], bf16), 64)
        kernel = hip_lib.last_kernel()
    assert gv.dtype == (torch.bfloat16 if bf16 else torch.float32) and gl.dtype == ga.dtype == torch.float32
    gv, gl, ga = gv.float().cpu().numpy(), gl.cpu().numpy(), ga.cpu().numpy()
    assert_kernel(kernel, name16 if bf16 else name32)
    bound_gv = b["grad_value"]
    if path.startswith("tile_lv"):       # the fixed-point windows: msda_bwd_tile_lv.h lines 13-18
        quantum = mt.tile_lv_quantum(g["shapes"], g["level_start"], g["loc"], g["attn"], g["grad_out"], N, S, M, D)
        bound_gv = bound_gv + (1.0 + (mt.U16 if bf16 else 0.0)) * quantum
    r = dict(grad_value=mt.worst_ratio(gv, t["grad_value"], bound_gv),
             grad_loc=mt.worst_ratio(gl, t["grad_loc"], b["grad_loc"]),
             grad_attn=mt.worst_ratio(ga, t["grad_attn"], b["grad_attn"]))
    report("bwd:" + path, case_id, bf16, kernel, r)
    n, q, m, _ = last_row(g)
    assert not gl[n, q, m].any() and not ga[n, q, m].any()      # out of range: exact zeros
    assert not gv[t["n_grad_value"] == 0].any()                 # cells nothing reaches stay zero (the inf one included)
    assert max(r.values()) <= 1.0, r


# ----------------------------------------------------------------------------- fused forward on the exposed points
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "f32"])
@pytest.mark.parametrize("variant,names", [(12, ("msda_fwd_d32_win<", "msda_fwd_d32_gather<4")), (3, ("msda_fwd_d32_gather<4",))],
                         ids=["win", "gather"])
def test_fused_forward_within_the_derived_bound_on_its_exposed_points(msda, hip_lib, variant, names, bf16):
    """The fused entry computes softmax and locations in-kernel; ``fused_points`` exposes the very bits it forms
    (tests/test_msda_fwd_win_gpu.py pins that), so truth on those points budgets only the sampling and the sum.  The softmax
    itself and the fused backward's Jacobians: tests/test_msda_fused_truth_gpu.py."""
    from fused_helpers import make_case
    from memotr_amd.MultiScaleDeformableAttention import tag_host_shapes
    shapes = mt.GEOMETRIES["pyr4"][0]
    c = make_case(61, 2, 8, 32, 4, 4, shapes, ref_dim=2, pyramid=True, off_px=2.0, with_mask=False)
    scale = (2.0 ** np.random.default_rng(61).uniform(-6, 6, (8, 32))).astype(np.float32)
    value = c["value"].numpy() * scale
    if bf16:
        value = mt.round_bf16(value)
    d = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in c.items()}
    tag_host_shapes(d["shapes"], shapes)
    with forced(hip_lib, fwd_variant=variant):
        out = msda.ms_deform_attn_fused_forward(dev(value, bf16), d["shapes"], d["level_start"], d["proj"], d["ref"], None, 8, 4)
        kernel = hip_lib.last_kernel()
    assert any(kernel.startswith(n) for n in names) and "fused" in kernel and ("bf16" in kernel) == bf16, kernel
    loc, attn = msda.fused_points(d["shapes"], d["proj"], d["ref"], 8, 4)
    t = mt.truth(value, c["shapes"].numpy(), c["level_start"].numpy(), loc.cpu().numpy(), attn.cpu().numpy())
    b = mt.bounds(t, (32, 4, 4), bf16)
    r = dict(out=mt.worst_ratio(out.float().cpu().numpy(), t["out"], b["out"]))
    report("fwd:fused", "pyr4-fused", bf16, kernel, r)
    assert r["out"] <= 1.0, r
