"""GPU: the deformable-encoder stack (two layers, C = 256, 8 heads, 4 levels, 4 points) against float64 truth by the rule
of tests/decoder_truth.py, at the two row counts of tests/encoder_truth.py: ``small`` (336 rows, padded, N = 2: the
query-sized kernels) and ``rows10880`` (the library GEMMs, split-K weight gradients, GEMMs accumulating into the
LayerNorm-backward results, ``relu_bwd_colsum``, the two-pass column sum, 64-row fan-in chunks: what training runs).

Per tensor (``out``, the gradients of ``src``, ``pos`` and the 32 parameters), max |got - truth| <=
``clip_truth.measured_bound(error of the fp32 torch composition on the same inputs on this device, max |truth|)``.  The
composition (MEMOTR_FUSED_CLIP_OPS=0, MEMOTR_ENC_LAYER_NODE=0) is measured here, once per case, and capped at
``REF_ERROR_CAP`` of scale: above it a decision fell the other way on the device and the case is reseeded, the bound
stays.  Paths: ``node`` (the default: every layer an ``EncoderLayerNode``), ``composed`` (MEMOTR_ENC_LAYER_NODE=0, kernels
on; same forward bits as the node, gradients also held to the node's), ``checkpointed`` (``use_checkpoint=True``),
``no_grad`` (``eval()``, what tracking runs; ``out`` only) and a second ``node`` run on the same inputs.

Which gradients a second run reproduces bit for bit: the fused deformable-attention backward adds into ``grad_value``
with float atomics, whose order changes from run to run; everything else (GEMMs, column sums, LayerNorm kernels, the
gradient of the sampling offsets and attention logits, which every query row owns) sums in a fixed order.  The last
layer's ``grad_value`` reaches its own ``value_proj`` gradients and, through ``g_src``, everything in front of it: layer 0,
``grad::src`` and ``grad::pos``.  So ``out`` and the gradients of layer 1 other than ``value_proj`` are the same bits; the
rest is held to the bound around the first run.

tests/test_encoder_truth_cpu.py shows that the inputs take the same decisions in float32 and float64, that the cases
sit where they are meant to, and that the rule catches planted defects.  profiles/encoder_truth.md holds the figures
of one run (``pytest -s`` prints them).
"""
import copy
from types import SimpleNamespace

import pytest
import torch

import encoder_truth as et

pytestmark = pytest.mark.gpu

ON = {"MEMOTR_FUSED_CLIP_OPS": "1", "MEMOTR_ENC_LAYER_NODE": "1"}
COUNTED = ("linear_fwd", "relu_bwd_colsum", "splitk_weight_grad")
PATH_ENV = {"node": ON, "composed": dict(ON, MEMOTR_ENC_LAYER_NODE="0")}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib, clip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module", params=et.CASES, ids=lambda c: c.name)
def ground(request, _need_gpu):
    """Per case, once: the encoder on both devices, float64 truth, and the fp32 torch composition's error on this
    device (the reference of every bound)."""
    case = request.param
    cpu, x = et.build_encoder(case), et.encoder_inputs(case)
    gpu = copy.deepcopy(cpu).cuda()
    truth = et.encoder_truth(cpu, x)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MEMOTR_FUSED_CLIP_OPS", "0")
        mp.setenv("MEMOTR_ENC_LAYER_NODE", "0")
        ref = {k: t.cpu() for k, t in et.run_encoder(gpu, x, "cuda").items()}
    return SimpleNamespace(case=case, cpu=cpu, gpu=gpu, x=x, truth=truth, ref_err=et.dt.errors(ref, truth), runs={})


def _run(g, path, x=None, **kw):
    """One run of ``path`` (cached per case: the first ``node`` run is what the other paths are held to), with the
    calls of the branch points counted.  ``x``: other inputs than the case's (not cached)."""
    if path in g.runs and x is None:
        return g.runs[path]
    env = PATH_ENV.get(path, ON)
    from memotr_amd.functions import clip_ops
    from memotr_amd.functions.encoder_layer import EncoderLayerNode
    from memotr_amd.modules import linear
    counts = dict.fromkeys(COUNTED, 0)
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        for name in COUNTED:
            owner = linear if name == "splitk_weight_grad" else clip_ops

            def counting(*a, _f=getattr(owner, name), _n=name, **k):
                counts[_n] += 1
                return _f(*a, **k)

            mp.setattr(owner, name, counting)
        n0 = EncoderLayerNode.calls
        got = {k: t.cpu() for k, t in et.run_encoder(kw.pop("enc", g.gpu), g.x if x is None else x, "cuda", **kw).items()}
        counts["nodes"] = EncoderLayerNode.calls - n0
    if x is not None:
        return got, counts
    g.runs[path] = (got, counts)
    return g.runs[path]


def _hold(g, path, got, center, tensors=None):
    rows, bad = et.check(g.case.name, path, got, center, g.ref_err, g.truth, tensors)
    print(f"TRUTH-WORST {g.case.name} {path} ({len(rows)} tensors) {et.worst(rows)}")
    assert not bad, (g.case.name, path, [(r.tensor, r.err, r.bound) for r in bad])
    return rows


def test_the_reference_composition_is_inside_its_cap(ground):
    assert len(ground.truth) == et.N_TENSORS and all(et.out_scale(t) > 0 for t in ground.truth.values())
    et.reference_inside_cap(ground.case.name, ground.ref_err, ground.truth)


def test_node_path_meets_float64_truth_on_its_side_of_every_switch(ground):
    from memotr_amd.functions import clip_ops
    g = ground
    got, n = _run(g, "node")
    print(f"BRANCHES {g.case.name} node {n}")
    assert n["nodes"] == 2                                  # both layers ran as EncoderLayerNode
    assert n["splitk_weight_grad"] == 10                    # five weight gradients per layer
    if g.case is et.ROWS10880:      # the training side: library GEMMs, fused ReLU backward, 64-row chunks
        assert n["linear_fwd"] == 0 and n["relu_bwd_colsum"] == 2
        assert clip_ops._fanin_chunk_rows(g.case.rows) == 64
    else:                           # the kernels' side
        assert n["linear_fwd"] == 10 and n["relu_bwd_colsum"] == 0
        assert clip_ops._fanin_chunk_rows(g.case.rows) == 16
    _hold(g, "node", got, g.truth)
    assert all(bool(torch.isfinite(t).all()) for t in got.values())


def test_composed_path_meets_truth_and_the_node_has_its_forward_bits(ground):
    g = ground
    node, _ = _run(g, "node")
    comp, n = _run(g, "composed")
    assert n["nodes"] == 0
    if g.case is et.ROWS10880:
        assert n["linear_fwd"] == 0 and n["relu_bwd_colsum"] == 2 and n["splitk_weight_grad"] == 10
    else:
        assert n["linear_fwd"] == 10 and n["relu_bwd_colsum"] == 0 and n["splitk_weight_grad"] == 0
    _hold(g, "composed", comp, g.truth)
    assert torch.equal(node["out"], comp["out"])
    _hold(g, "node~composed", node, comp)


def test_checkpointed_encoder_meets_truth_without_the_node(ground):
    g = ground
    enc = copy.deepcopy(g.cpu)
    enc.use_checkpoint = True
    got, n = _run(g, "checkpointed", enc=enc.cuda())
    assert n["nodes"] == 0
    _hold(g, "checkpointed", got, g.truth)


def test_no_grad_eval_forward_meets_truth(ground):
    g = ground
    g.gpu.eval()
    try:
        got, n = _run(g, "no_grad", grad=False)
    finally:
        g.gpu.train()
    assert n["nodes"] == 0 and set(got) == {"out"}
    _hold(g, "no_grad", got, g.truth, ["out"])


def atomic_free(name: str) -> bool:
    """Tensors no float atomic contributes to (module docstring): ``out`` and layer 1 without its value projection."""
    return name == "out" or (name.startswith("grad::p::layers.1.") and ".value_proj." not in name)


def test_a_second_node_run_repeats_the_first(ground):
    g = ground
    first, _ = _run(g, "node")
    second, n = _run(g, "node-again")
    assert n["nodes"] == 2
    exact = [k for k in first if atomic_free(k)]
    assert len(exact) == 1 + 14 and len(first) == et.N_TENSORS
    differing = [k for k in exact if not torch.equal(first[k], second[k])]
    assert not differing, differing
    _hold(g, "node-again~node", second, first)
    print(f"REPEAT {g.case.name}: {sum(torch.equal(first[k], second[k]) for k in first)} of {len(first)} tensors bit-equal")


def test_exact_zeros_of_truth_are_exact_zeros_on_the_device(ground):
    """Where float64 truth is exactly zero a path has no round-off to make: it is zero there too.  The cases have such
    elements as they stand: on ``small`` the gradients of sampling offsets whose points all fall outside their (tiny)
    level, on ``rows10880`` the ``linear1`` / ``linear2`` gradients of a hidden unit of layer 1 that no row switches on.
    ``small`` is then run once more with the upstream gradient zeroed on the padded rows: nothing reads those rows (the
    residual, the LayerNorms and the FFN work row by row, a padded row's value is zeroed and what its query samples ends
    in its own row), so truth has exact zeros in the padded rows of ``grad::src`` and ``grad::pos`` -- asserted, so that
    the clause cannot go vacuous -- and both paths must have them too: the fan-in LayerNorm backward on rows of zeros,
    the GEMMs that accumulate into its result, ``zero_rows`` on ``grad_value``."""
    g = ground
    for path in ("node", "composed"):
        got, _ = _run(g, path)
        assert sum(int((t == 0).sum()) for t in g.truth.values()) > 500
        for k, t in g.truth.items():
            assert not bool(got[k][t == 0].any()), (path, k)
    if not g.case.padded:
        return
    pad = g.x["mask"]
    x = dict(g.x, up=g.x["up"].masked_fill(pad[..., None], 0.0))
    truth = et.encoder_truth(g.cpu, x)
    for k in ("grad::src", "grad::pos"):
        assert int(pad.sum()) > 0 and not bool(truth[k][pad].any()) and bool(truth[k][~pad].all(-1).all()), k
    for path in ("node", "composed"):
        got, n = _run(g, path, x=x)
        assert n["nodes"] == (2 if path == "node" else 0)
        for k, t in truth.items():
            assert bool(torch.isfinite(got[k]).all()) and not bool(got[k][t == 0].any()), (path, k)
        assert not bool(got["grad::src"][pad].any()) and not bool(got["grad::pos"][pad].any()), path
