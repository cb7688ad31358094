#!/usr/bin/env python
"""The one-launch Linear backward (clipops_linear_bwd_f32) and the tile forward (clipops_linear_fwd_f32), replayed from
a hipGraph (the decoder's situation) at the decoder's shapes, against the library chains they replace.

    python tools/linear_bwd_probe.py [--out FILE] [--tree CHECKOUT] [--no-chain]
    python tools/linear_bwd_probe.py --counters [--labels FILE]

The result lines are printed, and written to `--out` when it is given.

Two operand modes per shape:
  warm   one operand set, every replayed call reads what the call before it read (L2-resident);
  cold   the graph holds one call per operand set, COLD_BYTES of sets in all, so that no set is L2-resident when its call
         runs (8 XCDs x 4 MiB of L2) -- the step's situation, where another kernel has just written every operand.
`--tree` imports memotr_amd from another checkout (A/B runs of two builds with one probe).
`--counters` launches each kernel a few times eagerly, warm then cold, for a `rocprofv3 --pmc` pass (a run of its own);
the launch order, one line per launch of a linear kernel, is printed, or written to `--labels` when it is given.
"""
import os
import sys

import torch


def _arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


sys.path.insert(0, _arg("--tree", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from memotr_amd.functions import clip_ops  # noqa: E402
from memotr_amd.modules.linear import configure_blas  # noqa: E402

SHAPES = ((320, 256, 256, False), (320, 256, 256, True), (320, 512, 256, True), (320, 256, 1024, True),
          (320, 1024, 256, False), (320, 256, 4, False), (320, 256, 768, False), (10, 256, 256, False))
COLD_BYTES = 40 << 20


def timed(fn, iters=200):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def graphed(fns):
    """The calls of `fns` back to back in one graph: what a dependent chain costs inside a replay."""
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for fn in fns[:3]:
            fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        for fn in fns:
            fn()
    return lambda: g.replay()


def in_graph(fns):
    """us per call of `fns` replayed from one graph (at least 20 calls per replay)."""
    fns = list(fns) * max(1, -(-20 // len(fns)))
    return timed(graphed(fns), 50) / len(fns)


def operand_sets(rows, in_f, out_f, relu, n):
    sets = []
    for _ in range(n):
        x = torch.randn(rows, in_f, device="cuda")
        w = torch.randn(out_f, in_f, device="cuda") / in_f ** 0.5
        gy = torch.randn(rows, out_f, device="cuda")
        bias = torch.randn(out_f, device="cuda")
        y = torch.relu(x @ w.t()) if relu else None
        sets.append((x, w, gy, bias, y))
    return sets


def n_cold_sets(rows, in_f, out_f):
    per_set = 4 * (rows * in_f + out_f * in_f + 2 * rows * out_f + out_f)
    return max(4, -(-COLD_BYTES // per_set))


def chain(s, relu):
    x, w, gy, _, y = s
    g2 = torch.ops.aten.threshold_backward(gy, y, 0.0) if relu else gy
    return g2 @ w, g2.t() @ x, clip_ops.colsum(g2)


def one(s):
    x, w, gy, _, y = s
    return clip_ops.linear_bwd(gy, y, x, w)


def lib_fwd(s, relu):
    x, w, _, bias, _ = s
    return torch._addmm_activation(bias, x, w.t(), use_gelu=False) if relu else torch.addmm(bias, x, w.t())


def one_fwd(s, relu):
    x, w, _, bias, _ = s
    return clip_ops.linear_fwd(x, w, bias, relu)


def write_lines(path, lines):
    """`lines` into `path`, or onto stdout when no path was given."""
    if path is None:
        print("\n".join(lines))
        return
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    open(path, "w").write("\n".join(lines) + "\n")


def counters(labels_path):
    """Eager launches for a counter pass: per shape 6 warm and then 12 cold launches of each kernel."""
    labels = []
    for rows, in_f, out_f, relu in SHAPES[:3] + SHAPES[7:]:
        cold = operand_sets(rows, in_f, out_f, relu, n_cold_sets(rows, in_f, out_f))
        warm = cold[0]
        torch.cuda.synchronize()
        for name, call in (("bwd", one), ("fwd", lambda s: one_fwd(s, relu))):
            if name == "fwd" and not clip_ops.linear_fwd_usable(warm[0], warm[1], warm[3]):
                continue
            for _ in range(6):
                call(warm)
                labels.append(f"{name} rows {rows} in {in_f} out {out_f} relu {int(relu)} warm")
            # (the later sets, most of COLD_BYTES, were written after these twelve: nothing of them is left in an L2)
            for s in cold[1:13]:
                call(s)
                labels.append(f"{name} rows {rows} in {in_f} out {out_f} relu {int(relu)} cold")
            torch.cuda.synchronize()
    write_lines(labels_path, labels)


def main():
    try:
        configure_blas()
    except Exception:  # noqa: BLE001
        pass
    if "--counters" in sys.argv:
        return counters(_arg("--labels"))
    out = _arg("--out")
    with_chain = "--no-chain" not in sys.argv
    lines = [f"# config_key {clip_ops.config_key()}  (us per call inside a replayed graph; warm / cold operands)"]
    print(lines[0], flush=True)
    for rows, in_f, out_f, relu in SHAPES:
        cold = operand_sets(rows, in_f, out_f, relu, n_cold_sets(rows, in_f, out_f))
        warm = cold[:1]
        line = f"rows {rows:4d} in {in_f:4d} out {out_f:4d} relu {int(relu)} sets {len(cold):3d}:  backward one launch "
        line += f"{in_graph([lambda s=s: one(s) for s in warm]):6.2f} / {in_graph([lambda s=s: one(s) for s in cold]):6.2f}"
        if with_chain:
            line += (f"  chain {in_graph([lambda s=s: chain(s, relu) for s in warm]):6.2f} / "
                     f"{in_graph([lambda s=s: chain(s, relu) for s in cold]):6.2f}")
        if clip_ops.linear_fwd_usable(warm[0][0], warm[0][1], warm[0][3]):
            line += (f"  ||  forward tile kernel {in_graph([lambda s=s: one_fwd(s, relu) for s in warm]):6.2f} / "
                     f"{in_graph([lambda s=s: one_fwd(s, relu) for s in cold]):6.2f}")
            if with_chain:
                line += (f"  library {in_graph([lambda s=s: lib_fwd(s, relu) for s in warm]):6.2f} / "
                         f"{in_graph([lambda s=s: lib_fwd(s, relu) for s in cold]):6.2f}")
        lines.append(line)
        print(line, flush=True)
        del cold, warm
        torch.cuda.empty_cache()
    if out is not None:          # (every line was printed as it was measured)
        write_lines(out, lines)


if __name__ == "__main__":
    main()
