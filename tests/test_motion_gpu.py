"""GPU: the three kernels of libtrack_motion_hip.so against the host statement of memotr_amd/models/motion.py on
random states, and the golden scenarios of the reference through ``SequenceTracker`` on the device.

Everything that is a copy, an integer or a float32 add / mul / div has to be the host's bits (``torch.equal``): the
returned ids, disappear_time and last_appear_boxes, the whole table, ``delta_out`` and every unchanged ``ref_pts``
row.  A changed ``ref_pts`` row holds a logarithm; it is compared with a float64 evaluation from the same float32
``last_appear_boxes`` and the (bit-equal) ``delta_out``:  |err| <= 6 * 2^-23 * max(1, |value|)  -- one correctly
rounded subtraction and division in front of the logarithm (<= 2^-23 absolute behind it), a logarithm good to 1 ulp
on either side, one add.
"""
import pytest
import torch

from motion_helpers import SCENARIOS, run_sequence_tracker, scenario

pytestmark = pytest.mark.gpu

CAPACITY = 512
THRESH = 0.6
MISS_TOLERANCE = 4
LAMBDA = 0.5
BOUND = 6 * 2.0 ** -23
EPS32 = float(torch.tensor(1e-5, dtype=torch.float32))


def random_case(n, L, K, seed):
    """A table with every count 0 .. L (full rows included: a push must trim) and n rows whose ids are a random
    permutation of a sparse subset of the table; disappear_time 0, 1, miss_tolerance - 1; own scores below, at and
    above the threshold (one float32 step away and far away)."""
    g = torch.Generator().manual_seed(seed)
    table_boxes = torch.rand((CAPACITY, L, 4), generator=g)
    table_count = torch.randint(0, L + 1, (CAPACITY,), generator=g).to(torch.int32)
    table_count[::3] = L
    ids = torch.randperm(CAPACITY, generator=g)[:n].long()
    labels = torch.randint(0, K, (n,), generator=g)
    at = torch.tensor(THRESH, dtype=torch.float32)
    levels = torch.stack((torch.tensor(0.05), torch.nextafter(at, torch.tensor(0.0)), at,
                          torch.nextafter(at, torch.tensor(1.0)), torch.tensor(0.95)))
    own = levels[torch.randint(0, 5, (n,), generator=g)]
    scores = torch.rand((n, K), generator=g)
    if n:
        scores.scatter_(1, labels[:, None], own[:, None])
    dt = torch.tensor([0, 1, MISS_TOLERANCE - 1])[torch.randint(0, 3, (n,), generator=g)]
    boxes = torch.rand((n, 4), generator=g)
    lab = torch.rand((n, 4), generator=g)
    lab.view(-1)[::7] = 0.0                       # the clamp at eps, both ends
    lab.view(-1)[3::11] = 1.0
    ref_pts = torch.randn((n, 4), generator=g)
    n_new = min(n, 5)
    new_boxes = torch.rand((n_new, 4), generator=g)
    return dict(table_boxes=table_boxes, table_count=table_count, ids=ids, labels=labels, scores=scores, dt=dt,
                boxes=boxes, lab=lab, ref_pts=ref_pts, new_boxes=new_boxes)


def make_state(case, L, min_length, device):
    from memotr_amd.models.motion import MotionState
    s = MotionState(L, min_length, device, capacity=CAPACITY)
    s.boxes.copy_(case["table_boxes"])
    s.count.copy_(case["table_count"])
    return s


def frame(state, case, device, first_id):
    """observe + register + extrapolate, as a frame issues them."""
    c = {k: v.to(device) for k, v in case.items()}
    ids, dt, lab = state.observe(c["scores"], c["labels"], c["boxes"], c["ids"], c["dt"], c["lab"], THRESH,
                                 MISS_TOLERANCE)
    state.register(first_id, c["new_boxes"])
    ref, delta = state.extrapolate(ids, dt, lab, c["ref_pts"], LAMBDA, return_delta=True)
    return ids, dt, lab, ref, delta


def assert_ref_pts(ref, delta, lab, ref_in, want_ref):
    """Unchanged rows are copies; changed rows (delta is bit-equal already) are held to float64 from float32 inputs."""
    ref, delta, lab = ref.cpu(), delta.cpu(), lab.cpu()
    changed = (want_ref != ref_in).any(dim=1) | (delta != 0).any(dim=1)
    assert torch.equal(ref[~changed], ref_in[~changed])
    x = lab[changed].double()
    truth = torch.log(x.clamp(EPS32, 1) / (1 - x).clamp(EPS32, 1)) + delta[changed].double()
    err = (ref[changed].double() - truth).abs()
    bound = BOUND * truth.abs().clamp(min=1)
    if changed.any():
        print(f"changed rows {int(changed.sum())}: max |err| / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())
    return int(changed.sum())


LENGTHS = [(2, 2), (5, 2), (5, 3), (5, 5), (16, 2), (16, 3), (16, 16)]        # (L, min_length): 2, 3 and L


@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("L,min_length", LENGTHS)
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_kernels_match_the_host_statement(n, L, min_length, K):
    case = random_case(n, L, K, seed=1000 * n + 10 * L + K)
    host, dev = make_state(case, L, min_length, "cpu"), make_state(case, L, min_length, "cuda")
    first_id = CAPACITY - 8                       # (the random ids may name these rows: register runs after observe)
    want = frame(host, case, "cpu", first_id)
    got = frame(dev, case, "cuda", first_id)
    for name, g, w in zip(("ids", "disappear_time", "last_appear_boxes"), got, want):
        assert g.is_cuda and g.dtype == w.dtype and torch.equal(g.cpu(), w), name
    assert torch.equal(dev.count.cpu(), host.count) and torch.equal(dev.boxes.cpu(), host.boxes)
    assert dev.boxes.shape == (CAPACITY, L, 4) and dev.count.dtype == torch.int32
    assert torch.equal(got[4].cpu(), want[4])                       # delta_out: add, mul, div only
    moved = assert_ref_pts(got[3], got[4], got[2], case["ref_pts"], want[3])
    if n >= 63:
        assert moved > 0 and int((want[0] < 0).sum()) > 0           # the case does extrapolate and retire
    host.check(), dev.check()
    # without delta_out (the frame loop's call): the same ref_pts
    ref_in = case["ref_pts"].cuda()
    again = dev.extrapolate(got[0], got[1], got[2], ref_in, LAMBDA)
    assert torch.equal(again, got[3])
    assert torch.equal(ref_in.cpu(), case["ref_pts"])               # out of place: the input keeps its values
    assert n == 0 or again.data_ptr() != ref_in.data_ptr()          # (tensors without elements have no storage)


def test_rows_outside_the_table_are_skipped_and_reported():
    L, K, n = 5, 8, 65
    case = random_case(n, L, K, seed=5)
    case["ids"][3], case["ids"][40] = -1, CAPACITY              # below the table and one past it
    host, dev = make_state(case, L, 3, "cpu"), make_state(case, L, 3, "cuda")
    want, got = frame(host, case, "cpu", CAPACITY - 8), frame(dev, case, "cuda", CAPACITY - 8)
    for g, w in zip(got[:3], want[:3]):
        assert torch.equal(g.cpu(), w)
    assert got[0][3].item() == -1 and got[0][40].item() == CAPACITY
    assert torch.equal(got[2][[3, 40]].cpu(), case["lab"][[3, 40]])
    assert torch.equal(got[3][[3, 40]].cpu(), case["ref_pts"][[3, 40]])
    assert torch.equal(dev.count.cpu(), host.count) and torch.equal(dev.boxes.cpu(), host.boxes)
    assert torch.equal(got[4].cpu(), want[4])
    assert dev.status.item() == host.status.item() == 3
    for s in (host, dev):
        with pytest.raises(RuntimeError, match="negative track id.*past the table"):
            s.check()


def test_register_across_a_doubling():
    from memotr_amd.models.motion import MotionState
    g = torch.Generator().manual_seed(3)
    first, second = torch.rand((6, 4), generator=g), torch.rand((70, 4), generator=g)
    states = []
    for device in ("cpu", "cuda"):
        s = MotionState(5, 3, device, capacity=8)
        s.register(0, first.to(device))
        s.register(6, second.to(device))          # 76 ids: 8 -> 128, the rows of the first call copied over
        assert s.capacity == 128 and s.boxes.shape == (128, 5, 4)
        states.append(s)
    host, dev = states
    assert torch.equal(dev.count.cpu(), host.count) and torch.equal(dev.boxes.cpu(), host.boxes)
    assert host.count.tolist() == [1] * 76 + [0] * 52
    assert torch.equal(dev.boxes[:76, 0].cpu(), torch.cat((first, second)))
    dev.check()


@pytest.mark.parametrize("name", SCENARIOS)
def test_golden_scenarios_on_the_device(name):
    """The reference's frame loop (tests/golden/gen_golden_motion.py) through SequenceTracker on the GPU."""
    sc = scenario(name)
    tracker, model, text = run_sequence_tracker(sc, device="cuda")
    assert tracker.tracker.motions.boxes.is_cuda
    moved = 0
    for f, (rec, fr) in enumerate(zip(model.records, sc["frames"])):
        for k in ("ids", "disappear_time", "last_appear_boxes"):
            want = fr["in_" + k]
            assert torch.equal(rec[k].cpu().reshape(want.shape), want), (f, k)
        got, want = rec["ref_pts"].cpu().double(), fr["in_ref_pts"].double()
        err, bound = (got - want).abs(), BOUND * want.abs().clamp(min=1)
        assert bool((err <= bound).all()), (f, float((err / bound).max()))
        if f:
            prev = {int(i): r for r, i in enumerate(sc["frames"][f - 1]["in_ids"])}
            moved += sum(1 for r, i in enumerate(fr["in_ids"].tolist()) if i in prev and not torch.equal(
                fr["in_ref_pts"][r], sc["frames"][f - 1]["in_ref_pts"][prev[i]]))
    assert moved >= 4
    assert text == sc["mot_lines"]                # (boxes are the scripted values: nothing device-computed in them)
    tracker.tracker.motions.check()
