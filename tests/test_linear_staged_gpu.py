"""GPU: the query-sized linear kernels with their operands staged through LDS (clipops_linear_bwd_f32 /
clipops_linear_fwd_f32, the shipped form) against the direct-from-global form they replace (MEMOTR_LINEAR_STAGED=0) and
against float64 truth.  Staging changes where an MFMA operand comes from, not the MFMA sequence, so every output has to be
the direct form's bit for bit: at tile edges, on both sides of the K block of the weight-gradient tile (512 rows), with
dword staging (a pitch or a pointer that does not allow 16-byte loads), with outputs absent, and replayed from a graph.
"""
import itertools

import pytest
import torch

import clip_truth as T
from test_clip_ops_truth_gpu import check_analytic, cuda

pytestmark = pytest.mark.gpu

ROWS = (1, 31, 32, 33, 65, 310, 512, 513, 1024)          # tile edges, the typical call, the K block of grad_w +- 1
INS = (4, 36, 256)                                       # one partial tile, K % 8 and % 32 != 0, the model's width
OUTS = (1, 6, 33, 256, 512)                              # OUT % 4 != 0 (dword staging), partial tiles, the limit
GUARD = 12345.0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(clip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def both_forms(monkeypatch, fn):
    """fn() with the staged kernels and with the direct ones."""
    res = []
    for flag in ("1", "0"):
        monkeypatch.setenv("MEMOTR_LINEAR_STAGED", flag)
        res.append(fn())
    torch.cuda.synchronize()
    return res


def same_bits(case, names, staged, direct):
    for name, a, b in zip(names, staged, direct):
        assert (a is None) == (b is None), (case, name)
        # (bit patterns: torch.equal on the floats would call two equal NaNs different and -0.0 equal to 0.0)
        assert a is None or torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{case}: {name} differs from the direct form"


def run_linear(x, w, b, gy, relu):
    from memotr_amd.functions import clip_ops
    y = clip_ops.linear_fwd(x, w, b, relu)
    gx, gw, gb = clip_ops.linear_bwd(gy, y if relu else None, x, w)
    return y, gx, gw, gb


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("rows", ROWS)
def test_staged_outputs_are_the_direct_forms_bit_for_bit(rows, relu, monkeypatch):
    from memotr_amd.functions import clip_ops
    for in_f, out_f in itertools.product(INS, OUTS):
        x, w, b, gy = cuda(*T.linear_inputs(rows, in_f, out_f))
        assert clip_ops.linear_fwd_usable(x, w, b) and clip_ops.linear_bwd_usable(gy, x, w)
        staged, direct = both_forms(monkeypatch, lambda: run_linear(x, w, b, gy, relu))
        same_bits(f"{rows}x{in_f}->{out_f} relu={relu}", ("y", "grad_x", "grad_w", "grad_b"), staged, direct)


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("rows", ROWS)
def test_staged_outputs_against_float64_truth(rows, relu):
    """The bound of tests/test_clip_ops_truth_gpu.py::test_linear_tiles_at_their_edges: 4e-7 sqrt(K) of the output scale
    (fp32 MFMA is an fmaf chain: fp32 round-off of a K-term sum)."""
    failures = []
    for in_f, out_f in itertools.product(INS, OUTS):
        x, w, b, gy = cuda(*T.linear_inputs(rows, in_f, out_f))
        y, gx, gw, gb = run_linear(x, w, b, gy, relu)
        want = T.linear_truth(T.f64(x), T.f64(w), T.f64(b), relu)
        case = f"staged linear {rows}x{in_f}->{out_f} relu={relu}"
        check_analytic(case, "y", y, want, 4e-7 * in_f ** 0.5 * (float(want.abs().max()) + 1.0), failures)
        gm = T.f64(gy) * ((T.f64(y) > 0).double() if relu else 1.0)
        for what, g, t, k in (("grad_x", gx, gm @ T.f64(w), out_f), ("grad_w", gw, gm.t() @ T.f64(x), rows),
                              ("grad_b", gb, gm.sum(0), rows)):
            check_analytic(case, what, g, t, 4e-7 * k ** 0.5 * (float(t.abs().max()) + 1e-6) + 1e-6, failures)
    assert not failures, "\n".join(failures)


def test_staged_mask_is_threshold_backward_on_nan_and_negative_zero(monkeypatch):
    """Small-integer operands (every sum exact in any order) with a NaN and a -0.0 activation: the mask applied while
    staging is aten's threshold_backward (NaN passes g, -0.0 blocks it), and the direct form's bits."""
    from memotr_amd.functions import clip_ops
    x, w, gy, y = cuda(*T.linear_integer_inputs())
    masked = T.f64(torch.ops.aten.threshold_backward(gy, y, 0.0))
    staged, direct = both_forms(monkeypatch, lambda: clip_ops.linear_bwd(gy, y, x, w))
    same_bits("integer inputs", ("grad_x", "grad_w", "grad_b"), staged, direct)
    assert torch.equal(T.f64(staged[0]), masked @ T.f64(w))
    assert torch.equal(T.f64(staged[1]), masked.t() @ T.f64(x))
    assert torch.equal(T.f64(staged[2]), masked.sum(0))


def guarded(numel, lead):
    """A `numel` view `lead` floats into a buffer filled with GUARD, and the buffer."""
    buf = torch.full((lead + numel + 8,), GUARD, device="cuda")
    return buf[lead:lead + numel], buf


def guards_intact(buf, lead, numel):
    return bool((buf[:lead] == GUARD).all()) and bool((buf[lead + numel:] == GUARD).all())


def raw_bwd(gy, y, x, w, gx, gw, gb):
    """The C entry point with caller-placed outputs (None: absent)."""
    from memotr_amd import _clip_lib as L_
    rows, out_f = gy.shape
    ptr = lambda t: None if t is None else t.data_ptr()        # noqa: E731
    L_.check(L_.lib.clipops_linear_bwd_f32(ptr(gy), ptr(y), ptr(x), ptr(w), rows, x.shape[1], out_f, ptr(gx), ptr(gw), ptr(gb),
                                           torch.cuda.current_stream().cuda_stream), "clipops_linear_bwd_f32")


@pytest.mark.parametrize("rows,in_f,out_f", [(33, 36, 6), (310, 256, 256)])
@pytest.mark.parametrize("need", [s for s in itertools.product((False, True), repeat=3) if any(s)],
                         ids=lambda s: "".join(n for n, f in zip("xwb", s) if f))
def test_absent_outputs_and_sliced_destinations(rows, in_f, out_f, need, monkeypatch):
    """Every non-empty subset of (grad_x, grad_w, grad_b); grad_w / grad_b land in row slices of a larger buffer (as the
    packed parameters' gradients do), grad_x between guard words: the bits of the all-outputs call, nothing else written."""
    from memotr_amd.functions import clip_ops
    need_x, need_w, need_b = need
    x, w, b, gy = cuda(*T.linear_inputs(rows, in_f, out_f))
    y = clip_ops.linear_fwd(x, w, b, True)
    monkeypatch.setenv("MEMOTR_LINEAR_STAGED", "0")
    full = clip_ops.linear_bwd(gy, y, x, w)
    monkeypatch.setenv("MEMOTR_LINEAR_STAGED", "1")
    # through the Python entry: row slices of larger gradient buffers
    gw_big = torch.full((out_f + 3, in_f), GUARD, device="cuda")
    gb_big = torch.full((out_f + 11,), GUARD, device="cuda")
    got = clip_ops.linear_bwd(gy, y, x, w, need_x=need_x, need_w=need_w, need_b=need_b,
                              gw_out=gw_big[2:2 + out_f], gb_out=gb_big[3:3 + out_f])
    want = (full[0] if need_x else None, full[1] if (need_w or need_b) else None, full[2] if need_b else None)
    same_bits(f"{rows}x{in_f}->{out_f} need={need}", ("grad_x", "grad_w", "grad_b"), got, want)
    assert bool((gw_big[:2] == GUARD).all()) and bool((gw_big[2 + out_f:] == GUARD).all())
    assert bool((gb_big[:3] == GUARD).all()) and bool((gb_big[3 + out_f:] == GUARD).all())
    if not (need_w or need_b):
        assert bool((gw_big == GUARD).all())
    if not need_b:
        assert bool((gb_big == GUARD).all())
    # through the C entry: every output between guard words
    gx, gx_buf = guarded(rows * in_f, 4) if need_x else (None, None)
    gw, gw_buf = guarded(out_f * in_f, 4) if (need_w or need_b) else (None, None)
    gb, gb_buf = guarded(out_f, 4) if need_b else (None, None)
    raw_bwd(gy, y, x, w, gx, gw, gb)
    torch.cuda.synchronize()
    for name, out, buf, ref in (("grad_x", gx, gx_buf, full[0]), ("grad_w", gw, gw_buf, full[1]), ("grad_b", gb, gb_buf, full[2])):
        if out is not None:
            same_bits(f"raw {rows}x{in_f}->{out_f} need={need}", (name,), (out.view(ref.shape),), (ref,))
            assert guards_intact(buf, 4, out.numel()), f"{name}: a guard word was written"


def shifted(t):
    """The same values one float off the allocation's alignment."""
    buf = torch.empty(t.numel() + 1, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("rows,in_f,out_f", [(33, 36, 6), (310, 256, 256)])
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
def test_operands_and_outputs_one_float_off_alignment(rows, in_f, out_f, relu):
    """Views that are only 4-byte aligned stage with dword loads: the bits of the aligned call, guards untouched."""
    from memotr_amd import _clip_lib as L_
    from memotr_amd.functions import clip_ops
    x, w, b, gy = cuda(*T.linear_inputs(rows, in_f, out_f))
    y, gx, gw, gb = run_linear(x, w, b, gy, relu)
    xs, ws, bs, gys = shifted(x), shifted(w), shifted(b), shifted(gy)
    ys, ys_buf = guarded(rows * out_f, 5)
    L_.check(L_.lib.clipops_linear_fwd_f32(xs.data_ptr(), ws.data_ptr(), bs.data_ptr(), rows, in_f, out_f, 1 if relu else 0,
                                           ys.data_ptr(), torch.cuda.current_stream().cuda_stream), "clipops_linear_fwd_f32")
    ys = ys.view(rows, out_f)
    gxs, gx_buf = guarded(rows * in_f, 5)
    gws, gw_buf = guarded(out_f * in_f, 5)
    gbs, gb_buf = guarded(out_f, 5)
    raw_bwd(gys, ys if relu else None, xs, ws, gxs, gws, gbs)
    torch.cuda.synchronize()
    same_bits(f"shifted {rows}x{in_f}->{out_f} relu={relu}", ("y", "grad_x", "grad_w", "grad_b"),
              (ys, gxs.view(rows, in_f), gws.view(out_f, in_f), gbs), (y, gx, gw, gb))
    for name, buf, n in (("y", ys_buf, rows * out_f), ("grad_x", gx_buf, rows * in_f), ("grad_w", gw_buf, out_f * in_f),
                         ("grad_b", gb_buf, out_f)):
        assert guards_intact(buf, 5, n), f"{name}: a guard word was written"
    # and one operand at a time (the mask alone, the weight alone): still the same bits
    if relu:
        assert clip_ops.linear_bwd_usable(gy, x, w)
        for a in (clip_ops.linear_bwd(gy, ys, x, w), clip_ops.linear_bwd(gy, y, x, ws)):
            same_bits("one shifted operand", ("grad_x", "grad_w", "grad_b"), a, (gx, gw, gb))


def test_staged_kernels_replay_from_a_graph():
    """310 x 256 -> 256 with ReLU, forward and backward captured in one graph and replayed twice on rewritten inputs."""
    from memotr_amd.functions import clip_ops
    rows, in_f, out_f = 310, 256, 256
    first = cuda(*T.linear_inputs(rows, in_f, out_f))
    sets = [first, [-0.5 * t.flip(0) for t in first]]
    x, w, b, gy = (t.clone() for t in first)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        run_linear(x, w, b, gy, True)              # (allows the large LDS request outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        outs = run_linear(x, w, b, gy, True)
    for ts in (sets[1], sets[0]):
        for dst, src in zip((x, w, b, gy), ts):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        replayed = [o.clone() for o in outs]
        eager = run_linear(*ts, True)
        same_bits("graph replay", ("y", "grad_x", "grad_w", "grad_b"), replayed, eager)
