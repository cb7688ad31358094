"""GPU: the clip criterion on scripted multi-frame clips against float64 truth (tests/criterion_truth.py has the rule, the
margins and the cap; tests/test_criterion_truth_cpu.py holds the two forms of truth to each other and to the reference).

Per case, on the device: the float32 torch composition (MEMOTR_FUSED_CLIP_OPS=0, boolean-mask selection) is measured and
held inside REF_ERROR_CAP; the default path (kernels on, keep_threshold set, the fused hand-over, deferred losses) makes
every integer decision as truth does and lands every loss, log value, active-set iou and leaf gradient inside
``clip_truth.measured_bound`` of that composition's error; every other switch setting gives the default path's bits.
Each comparison prints ``TRUTH <case> <what> ref= kernel= bound= scale=`` (pytest -s); profiles/criterion_truth.md records
a run."""
import functools

import pytest
import torch

import criterion_truth as ct

pytestmark = pytest.mark.gpu
DEVICE = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(clip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def composition(case):
    """The float32 torch composition on the device, once per case."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MEMOTR_FUSED_CLIP_OPS", "0")
        return ct.run_clip(case, DEVICE, torch.float32, ct.COMPOSED)


@functools.lru_cache(maxsize=None)
def default_path(case):
    """The default path, once per case (the environment of the caller's test must be the default one)."""
    return ct.run_clip(case, DEVICE, torch.float32, ct.DEFAULT)


def fused_frames(case):
    """Which frames the hand-over kernel covers: every clip has a ground truth and an active set of its own."""
    return [[all(n > 0 for n in case.gts[t]) and not any(f["fake"])] * case.B
            for t, f in enumerate(ct.truth(case)["frames"])]


@pytest.mark.parametrize("case", ct.CASES, ids=ct.CASE_IDS)
def test_reference_composition_inside_cap(case):
    ref, truth = composition(case), ct.truth(case)
    assert ct.decisions_of(ref) == ct.decisions_of(truth)
    assert ct.new_ids_agree(ref, truth)
    assert not any(any(f["fused"]) for f in ref["frames"])
    off = {k: (e, s) for k, (e, s) in ct.errors(ref, truth).items() if not e <= ct.REF_ERROR_CAP * s}
    assert not off, off


@pytest.mark.parametrize("case", ct.CASES, ids=ct.CASE_IDS)
def test_default_path_against_truth(case):
    truth = ct.truth(case)
    ref_errors = ct.errors(composition(case), truth)
    got = default_path(case)
    assert ct.decisions_of(got) == ct.decisions_of(truth)
    assert ct.new_ids_agree(got, truth)
    assert [f["fused"] for f in got["frames"]] == fused_frames(case)         # no quiet way round the hand-over kernel
    failures = []
    ct.check(case, got, ref_errors, truth, failures)
    assert not failures, "\n".join(failures)
    # the float fields of every active set are bit copies of the leaf rows truth takes them from
    assert ct.fields_are_copies(got, truth) == []


@pytest.mark.parametrize("case", ct.CASES, ids=ct.CASE_IDS)
def test_exact_zeros(case):
    got, truth = default_path(case), ct.truth(case)
    nd = case.nd
    for t, frame in enumerate(truth["frames"]):
        for b in range(case.B):
            n_tr = frame["n_tr"][b]
            for name in ct.leaf_names(case, t):
                g = got["grads"][name]
                if name.endswith("det_query_embed"):
                    continue
                assert not bool(g[b, nd + n_tr:].any()), (name, b, "padded slots")
            for li in range(case.layers):
                g = got["grads"][f"f{t}.boxes{li}"][b]
                q, _ = frame["pairs"][b][li]
                late = not (li > 0 and li - 1 < case.merge)
                matched = set(q) | ({nd + j for j, o in enumerate(frame["matched_idx"][b]) if o >= 0} if late else set())
                rest = [r for r in range(g.shape[0]) if r not in matched]
                assert not bool(g[rest].any()), (t, b, li, "unmatched rows")
                if case.gts[t][b] == 0:
                    assert not bool(g.any()), (t, b, li, "no ground truth")
                    assert bool(torch.isfinite(got["grads"][f"f{t}.logits{li}"][b]).all())


SWITCHES = {
    "handover-off": ({"MEMOTR_FUSED_HANDOVER": "0"}, ct.DEFAULT),
    "bookkeeping-off": ({"MEMOTR_FUSED_BOOKKEEPING": "0"}, ct.DEFAULT),
    "mask-selection": ({}, ct.Path(keep_rows=False, handover=False)),
    "one-piece": ({}, ct.Path(deferred=False)),
    "stacks": ({}, ct.Path(stacks=True)),
}


@pytest.mark.parametrize("switch", sorted(SWITCHES))
@pytest.mark.parametrize("case", ct.CASES, ids=ct.CASE_IDS)
def test_switches_give_the_default_paths_bits(case, switch, monkeypatch):
    """Every switch moves or regroups launches and copies; none changes an operand or an order of summation: the
    composed hand-over gathers the rows the kernel gathers and calls the same IoU routine on them, its backward adds
    the same two gradient rows; the torch bookkeeping produces the same integers; the mask selects the rows the index
    lists; the losses of a frame enter the clip's sums in frame order either way; the stacks hold the same layers."""
    want = default_path(case)
    env, path = SWITCHES[switch]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got = ct.run_clip(case, DEVICE, torch.float32, path)
    if switch in ("handover-off", "mask-selection"):
        assert not any(any(f["fused"]) for f in got["frames"])
    assert ct.new_ids_agree(got, want)
    assert ct.same_bits(got, want) == []


@pytest.mark.parametrize("case", ct.CASES, ids=ct.CASE_IDS)
def test_run_to_run(case):
    assert ct.same_bits(ct.run_clip(case, DEVICE, torch.float32, ct.DEFAULT), default_path(case)) == []
