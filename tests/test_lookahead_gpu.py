"""GPU: the frame announced as next is not the frame that arrives (memotr_amd/lookahead.py).  Every call of a run
announces a decoy -- another tensor object of the same shape, with other pixels -- so its encode half is queued on the
side stream, into the graph slot the following call writes too; the following call passes the real frame, must wait for
the queued half, drop it and encode the frame it was given.  Such a run gives what a run without lookahead gives, for
``SequenceTracker.step``, ``SequenceTracker.step_raw`` and ``MultiSequenceTracker.step_raw`` on two streams, with the
inference graphs on and off (scenario, margin and equivalence of tests/multi_track_cases.py)."""
import pytest
import torch

import multi_track_cases as M

from memotr_amd.data.frames import preprocess_frames, target_size
from memotr_amd.inference import SequenceTracker
from memotr_amd.inference_multi import MultiSequenceTracker

pytestmark = pytest.mark.gpu
SIZE = (M.FRAME_H, M.FRAME_W)


@pytest.fixture(scope="module")
def scenario(request):
    for lib in ("hip_lib", "clip_lib"):
        request.getfixturevalue(lib)
    return M.scenario_model(256).cuda(), M.sequences()


def normalised(frame_u8):
    """The (3, th, tw) image ``step`` takes: what ``step_raw`` makes of the frame, without the padding."""
    th, tw = target_size(*SIZE, *M.RAW_SIZE)
    return preprocess_frames(frame_u8.cuda(), size=(th, tw)).tensors[0, :, :th, :tw].clone()


def one_sequence(model, frames, decoy, raw):
    """``frames`` through a fresh SequenceTracker; ``decoy``: announced as the next frame of every call."""
    tracker = SequenceTracker(model, **M.OPTIONS)
    decisions = M.Decisions(tracker, model.query_updater.update_threshold)
    if raw:
        results = [tracker.step_raw(f, decoy) for f in frames]
    else:
        results = [tracker.step(f, *SIZE, next_image=decoy) for f in frames]
    return results, decisions.margin()


def two_streams(model, pair, decoys):
    tracker = MultiSequenceTracker(model, n_streams=2, cap=32, **M.OPTIONS)
    steps = [tracker.step_raw([a, b], decoys) for a, b in zip(*pair)]
    return [[s[0] for s in steps], [s[1] for s in steps]]


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("entry", ["step", "step_raw", "lockstep"])
def test_a_decoy_announced_as_the_next_frame_changes_nothing(scenario, monkeypatch, entry, graphs):
    monkeypatch.setenv("MEMOTR_REQUIRE_GRAPHS", "1")
    monkeypatch.setenv("MEMOTR_INFER_GRAPHS", "1" if graphs else "0")
    model, seqs = scenario
    enc, dec = model.infer_graphs().encode, model.transformer.decoder.infer_graphs().decode
    replays = enc.replays
    if entry == "lockstep":
        pair = [seqs[1][:3], seqs[2]]
        _, margin = M.single_runs(model, pair)
        decoys = [seqs[0][0].clone(), seqs[0][1].clone()]          # (a list of its own: no step's ``source``)
        want, got = two_streams(model, pair, None), two_streams(model, pair, decoys)
    else:
        raw = entry == "step_raw"
        frames, decoy = seqs[1], seqs[0][0].clone()
        if not raw:
            frames, decoy = [normalised(f) for f in frames], normalised(decoy)
        (want, margin), (got, _) = one_sequence(model, frames, None, raw), one_sequence(model, frames, decoy, raw)
        want, got = [want], [got]
    print(entry, "graphs" if graphs else "eager", "smallest decision margin:", margin)
    assert margin > M.MARGIN, f"a decision score lies {margin} from its threshold: choose another seed"
    assert sum(len(r.ids) for seq in want for r in seq) > 0
    M.assert_equivalent(want, got)
    assert not enc.failed and not dec.failed
    assert (enc.replays > replays) == graphs                       # (no quiet eager path with the graphs on)
