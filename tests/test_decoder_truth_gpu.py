"""GPU: the decoder loop and the query updater at C = 256 (8 heads, D = 32) against float64 truth, by the rule of
tests/decoder_truth.py: per tensor, max |got - truth| <= clip_truth.measured_bound(error of the fp32 torch composition
on the same inputs on this device, max |truth|).  The composition's error is measured here, in the test, and capped at
1e-4 of scale (above that a decision fell the other way on the device: the case is reseeded, the bound stays).

Decoder paths: (a) eager with the kernels, (b) eager with MEMOTR_FUSED_CLIP_OPS=0 (the reference of the bound), (c) the
training capture -- one capture, two replays, the second on other values and another live track count inside the same
bucket, (d) the inference capture (no_grad, eval), forward only, replayed the same way.  (a), (c) and (d) are also held
to each other with the same bound around (a).  Query updater: ``update_fields`` eagerly, through ``UpdaterGraphs.run`` and
``update_bank`` against truth computed per stream on that stream's live rows alone.

tests/test_decoder_truth_cpu.py shows that the inputs take the same decisions in float32 and float64 and that the rule
catches planted defects.  profiles/decoder_truth.md holds the figures of one run (``pytest -s`` prints them).
"""
import copy

import pytest
import torch

import decoder_truth as dt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib, clip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _hold(name, path, got, center, ref_err, truth, tensors=None):
    rows, bad = dt.check(name, path, got, center, ref_err, truth, tensors)
    print(f"TRUTH-WORST {name} {path} ({len(rows)} tensors) {dt.worst(rows)}")
    assert not bad, (name, path, [(r.tensor, r.err, r.bound) for r in bad])


def _reference(monkeypatch, name, run, truth):
    """Path (b) and its error: the fp32 torch composition on this device."""
    with monkeypatch.context() as mp:
        mp.setenv("MEMOTR_FUSED_CLIP_OPS", "0")
        ref = run()
    ref_err = dt.errors(ref, truth)
    dt.reference_inside_cap(name, ref_err, truth)
    return ref_err


def _exact_decoder_assertions(case, path, got, x):
    nd = dt.ND
    if case.merge == 1:          # the track rows of layer 0 are the input's bits
        assert torch.equal(got["out::outs"][0][:, nd:].cpu(), x["tgt"][:, nd:]), path
    assert torch.equal(got["out::layer_inputs"][0].cpu(), x["tgt"]), path
    if "grad::tgt" in got:       # masked query rows take no gradient
        masked = x["query_mask"]
        assert not bool(got["grad::tgt"].cpu()[masked].any()), path
        assert all(bool(torch.isfinite(t).all()) for k, t in got.items() if k.startswith("grad::")), path


# ------------------------------------------------------------------------------------------------ decoder
@pytest.mark.parametrize("case", dt.GRAPH_CASES, ids=lambda c: c.name)
def test_decoder_paths_meet_float64_truth(monkeypatch, case):
    from memotr_amd.functions import clip_ops
    for k in ("MEMOTR_REQUIRE_GRAPHS", "MEMOTR_DECODER_GRAPHS", "MEMOTR_INFER_GRAPHS", "MEMOTR_FUSED_CLIP_OPS"):
        monkeypatch.setenv(k, "1")
    cpu = dt.build_decoder(case)
    gpu = copy.deepcopy(cpu).cuda()
    # which branch the FFN linears of this case take (clip_ops.linear_fwd_usable / linear_bwd_usable)
    rows, lin1 = torch.zeros(dt.B * (dt.ND + case.n_track), dt.C, device="cuda"), gpu.layers[0].linear1
    assert clip_ops.linear_fwd_usable(rows, lin1.weight, lin1.bias) == (case.d_ffn == 64)
    assert clip_ops.linear_bwd_usable(rows.new_zeros(rows.shape[0], case.d_ffn), rows, lin1.weight) == (case.d_ffn == 64)
    cache, infer = gpu.graphs(), gpu.infer_graphs().decode
    padded = {}
    run_graph = cache.run

    def spy(frame_slot, args, *more, **kw):          # the padded `tgt` the capture is fed: its gradient is looked at below
        args[0].retain_grad()
        padded["tgt"] = args[0]
        return run_graph(frame_slot, args, *more, **kw)

    monkeypatch.setattr(cache, "run", spy)
    for which in (0, 1):
        x = dt.decoder_inputs(case, which)
        name = f"{case.name}/{which}"
        nq = x["tgt"].shape[1]
        truth = dt.decoder_truth(monkeypatch, cpu, x)
        ref_err = _reference(monkeypatch, name, lambda: dt.run_decoder(gpu, x, "cuda"), truth)
        eager = dt.run_decoder(gpu, x, "cuda")                                                 # (a)
        assert (cache.captures, cache.replays, cache.eager) == (min(which, 1), which, 0)       # ... ran no graph
        _hold(name, "eager", eager, truth, ref_err, truth)
        _exact_decoder_assertions(case, "eager", eager, x)

        graph = dt.run_decoder(gpu, x, "cuda", frame_slot=0, clip_key=object())                # (c)
        assert (cache.captures, cache.replays, cache.eager, cache.failed) == (1, which + 1, 0, False)
        _hold(name, "train-graph", graph, truth, ref_err, truth)
        _hold(name, "train-graph~eager", graph, eager, ref_err, truth)
        _exact_decoder_assertions(case, "train-graph", graph, x)
        grad_padded = padded.pop("tgt").grad
        assert grad_padded.shape[1] == cache.bucket(nq, dt.ND) > nq
        assert not bool(grad_padded[:, nq:].any())                                             # padded rows: zero gradient
        assert torch.equal(grad_padded[:, :nq], graph["grad::tgt"])

        gpu.eval()                                                                             # (d)
        try:
            inference = dt.run_decoder(gpu, x, "cuda", grad=False)
        finally:
            gpu.train()
        assert (infer.captures, infer.replays, infer.eager, infer.failed) == (1, which + 1, 0, False)
        stacks = ["out::" + k for k in dt.STACKS]
        _hold(name, "infer-graph", inference, truth, ref_err, truth, stacks)
        _hold(name, "infer-graph~eager", inference, eager, ref_err, truth, stacks)
        _exact_decoder_assertions(case, "infer-graph", inference, x)


@pytest.mark.parametrize("case", dt.EAGER_ONLY_CASES, ids=lambda c: c.name)
def test_extra_track_attention_is_refused_by_the_graphs_and_meets_truth_eagerly(monkeypatch, case):
    for k in ("MEMOTR_REQUIRE_GRAPHS", "MEMOTR_DECODER_GRAPHS", "MEMOTR_INFER_GRAPHS", "MEMOTR_FUSED_CLIP_OPS"):
        monkeypatch.setenv(k, "1")
    cpu = dt.build_decoder(case)
    gpu = copy.deepcopy(cpu).cuda()
    x = dt.decoder_inputs(case)
    cache, infer = gpu.graphs(), gpu.infer_graphs()
    tgt, src = x["tgt"].cuda(), x["src"].cuda().requires_grad_(True)
    assert not cache.usable(tgt, src)
    for layer in gpu.layers:                 # ... for that reason and no other
        layer.extra_track_attn = False
    assert cache.usable(tgt, src)
    for layer in gpu.layers:
        layer.extra_track_attn = True
    truth = dt.decoder_truth(monkeypatch, cpu, x)
    ref_err = _reference(monkeypatch, case.name, lambda: dt.run_decoder(gpu, x, "cuda"), truth)
    eager = dt.run_decoder(gpu, x, "cuda", frame_slot=0, clip_key=object())          # asks for the graph, runs eagerly
    assert (cache.captures, cache.replays, cache.failed) == (0, 0, False)
    _hold(case.name, "eager", eager, truth, ref_err, truth)
    _exact_decoder_assertions(case, "eager", eager, x)
    gpu.eval()
    try:
        with torch.no_grad():
            assert not infer.decode_usable(gpu, tgt, src)
        inference = dt.run_decoder(gpu, x, "cuda", grad=False)
    finally:
        gpu.train()
    assert (infer.decode.captures, infer.decode.replays) == (0, 0)
    _hold(case.name, "eager-no-grad", inference, truth, ref_err, truth, ["out::" + k for k in dt.STACKS])


# ------------------------------------------------------------------------------------------------ query updater
@pytest.mark.parametrize("n", dt.UPDATER_ROWS)
@pytest.mark.parametrize("use_dab", (True, False), ids=("dab", "plain"))
def test_update_fields_paths_meet_float64_truth(monkeypatch, use_dab, n):
    for k in ("MEMOTR_REQUIRE_GRAPHS", "MEMOTR_UPDATER_GRAPHS", "MEMOTR_FUSED_CLIP_OPS"):
        monkeypatch.setenv(k, "1")
    cpu = dt.build_updater(use_dab)
    gpu = copy.deepcopy(cpu).cuda()
    cache = gpu.graphs()
    for i, rows in enumerate((n, dt.UPDATER_ALT_ROWS[n])):
        name = f"updater-{'dab' if use_dab else 'plain'}-r{rows}"
        fields, weights = dt.updater_fields(rows, use_dab)
        truth = dt.updater_truth(cpu, fields, weights)
        ref_err = _reference(monkeypatch, name, lambda: dt.run_updater(gpu, fields, weights, "cuda"), truth)
        eager = dt.run_updater(gpu, fields, weights, "cuda")
        assert (cache.captures, cache.replays) == (min(i, 1), i)
        _hold(name, "eager", eager, truth, ref_err, truth)
        graph = dt.run_updater(gpu, fields, weights, "cuda", graph_slot=(0, 0))
        assert (cache.captures, cache.replays, cache.eager, cache.failed) == (1, i + 1, 0, False)
        _hold(name, "graph", graph, truth, ref_err, truth)
        _hold(name, "graph~eager", graph, eager, ref_err, truth)
        for got in (eager, graph):
            assert all(bool(torch.isfinite(t).all()) for t in got.values())


@pytest.mark.parametrize("use_dab", (True, False), ids=("dab", "plain"))
def test_update_bank_meets_per_stream_float64_truth(monkeypatch, use_dab):
    from memotr_amd.models.track_bank import ROW_FIELDS
    monkeypatch.setenv("MEMOTR_FUSED_CLIP_OPS", "1")
    cpu = dt.build_updater(use_dab)
    gpu = copy.deepcopy(cpu).cuda()
    name = f"bank-{'dab' if use_dab else 'plain'}"
    _, per_stream = dt.build_bank(use_dab)
    truth = dt.bank_truth(cpu, per_stream, use_dab)

    def run():
        bank, _ = dt.build_bank(use_dab, "cuda")
        gpu.update_bank(bank)
        run.bank = bank
        return dt.bank_fields(bank)

    ref_err = _reference(monkeypatch, name, run, truth)
    got = run()
    _hold(name, "kernels", got, truth, ref_err, truth)
    free = ~dt.bank_live_slots()
    for k, t in got.items():
        assert not bool(t[free].any()), k                        # free slots still hold exact zeros
    for k in ROW_FIELDS:                                          # the stream without a track left nothing non-finite
        t = getattr(run.bank, k)
        assert not t.is_floating_point() or bool(torch.isfinite(t).all()), k
    assert torch.equal(run.bank.ids.cpu() >= 0, dt.bank_live_slots())
