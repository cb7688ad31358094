"""CPU half of the clip-criterion truth tests (tests/criterion_truth.py has the rule, the margins and the cap): the two
forms of truth agree, form 2 reproduces a fixture written by the reference's own criterion, every case keeps its margins
and makes the same decisions in float32, the float32 composition stays inside a quarter of REF_ERROR_CAP, and the
comparison notices each of seven wrong criteria."""
import functools
import os

import numpy as np
import pytest
import torch

import criterion_truth as ct
from clip_truth import measured_bound
from conftest import GOLDEN_DIR, load_npz


@functools.lru_cache(maxsize=None)
def composition_f32(case):
    """The float32 composition on the CPU, once per case."""
    return ct.run_clip(case, "cpu", torch.float32, ct.COMPOSED)


@pytest.mark.parametrize("case", ct.CASES, ids=ct.CASE_IDS)
def test_the_two_forms_of_truth_agree(case):
    module, plain = ct.module_truth(case), ct.truth(case)
    assert ct.decisions_of(module) == ct.decisions_of(plain)
    assert ct.new_ids_agree(module, plain)
    assert module["n_gts"] == plain["n_gts"]
    # float64 sums of a few thousand terms formed in different orders: FORMS_AGREE of the scale (criterion_truth.py)
    off = {k: (e, s) for k, (e, s) in ct.errors(module, plain).items() if not e <= ct.FORMS_AGREE * s}
    assert not off, off
    assert ct.fields_are_copies(module, plain) == []


@pytest.mark.parametrize("case", ct.CASES, ids=ct.CASE_IDS)
def test_margins_hold_and_float32_decides_alike(case):
    margins = ct.decisions(case)
    assert ct.margins_hold(margins), margins
    f32, plain = composition_f32(case), ct.truth(case)
    assert ct.decisions_of(f32) == ct.decisions_of(plain)
    assert ct.new_ids_agree(f32, plain)
    off = {k: (e, s) for k, (e, s) in ct.errors(f32, plain).items() if not e <= ct.REF_ERROR_CAP / 4 * s}
    assert not off, off
    assert ct.fields_are_copies(f32, plain) == []


def test_every_kind_of_row_occurs():
    rows = {c.name: ct.truth(c)["rows"] for c in ct.CASES}
    frames = {c.name: ct.truth(c)["frames"] for c in ct.CASES}
    for c in ct.CASES:
        r = rows[c.name]
        assert r["stays"] + r["drifts_off"] > 0 and r["gone_kept"] > 0 and r["dead_kept"] > 0 and r["dead_dropped"] > 0, c.name
        assert r["late_restricted"] > 0, c.name
        if c.B == 2:        # the track counts differ in every frame that carries tracks: one clip always has padded slots
            assert all(f["n_tr"][0] != f["n_tr"][1] for f in frames[c.name][1:]), c.name
    for name in ("probe", "repeat-lose", "model-nd", "plain"):
        assert rows[name]["stays"] > 0 and rows[name]["drifts_off"] > 0, name
    assert rows["probe"]["early_with_tracks"] > 0 and rows["return"]["early_with_tracks"] > 0
    assert rows["probe"]["no_gt"] == 1 and rows["return"]["no_gt"] == 2
    assert rows["repeat-lose"]["repeated_owned"] == 1 and rows["repeat-lose"]["fake"] == 1
    assert frames["repeat-lose"][0]["n_tr"][1] == 0 and frames["repeat-lose"][1]["n_tr"][1] > 0    # it had tracks to lose
    assert rows["return"]["returns"] > 0
    # more ground truths than detect queries: every detect query of the first frame is matched, none is unclaimed
    assert [len(q) for q, _ in frames["crowded"][0]["pairs"][0]] == [8, 8]
    assert frames["model-nd"][1]["n_tr"][0] + 300 > 320


def test_statement_reproduces_the_reference_fixture():
    """tests/golden/criterion_clip.npz: the reference's own ClipCriterion and QueryUpdater selection on the first case, on
    the same scripted leaves (tests/golden/gen_golden_criterion.py).  The reference runs in float32 only, i.e. it is one
    more float32 composition on the CPU: its decisions are held exactly and its numbers to what the project's own
    composition is held to there, a quarter of REF_ERROR_CAP."""
    case = ct.GOLDEN_CASE
    ref = load_npz(os.path.join(GOLDEN_DIR, "criterion_clip.npz"))
    plain = ct.truth(case)
    # the inputs the fixture was computed from are the ones the script produces today
    for t, frame in enumerate(plain["frames"]):
        rec = ct.frame_inputs(case, t, [ref[f"track_ids.f{t}.clip{b}"].tolist() for b in range(case.B)])
        assert np.array_equal(ref[f"in.f{t}.logits"], rec["logits"].numpy())
        assert np.array_equal(ref[f"in.f{t}.boxes"], rec["boxes"].numpy())
        for b in range(case.B):
            ids, labels, boxes = ct.ground_truths(case, t, b)
            assert np.array_equal(ref[f"in.f{t}.clip{b}.gt_ids"], ids.numpy())
            assert np.array_equal(ref[f"in.f{t}.clip{b}.gt_boxes"], boxes.numpy())
            assert ref[f"track_ids.f{t}.clip{b}"].tolist() == ([] if t == 0 else plain["frames"][t - 1]["active_ids"][b])
    for name, pairs in ct.flat_pairs(plain).items():
        assert np.array_equal(ref[name], pairs), name
    mine = ct.to_numpy(plain)
    for k in [k for k in mine if k.startswith("loss.")] + [k for k in mine if k.startswith("grad.") and
                                                           ("logits" in k or "boxes" in k)]:
        want = ref[k]
        scale = float(np.abs(want).max()) if want.size else 0.0
        assert float(np.abs(mine[k] - want).max()) <= ct.REF_ERROR_CAP / 4 * scale, k


# wrong criterion -> (case, output) that must land outside measured_bound(CPU float32 error, scale)
CAUGHT_BY = {"a": ("probe", "loss.box_l1_loss"),
             "b": ("repeat-lose", "loss.box_l1_loss"),
             "c": ("probe", "loss"),
             "d": ("probe", "loss.box_l1_loss"),
             "e": ("probe", "loss.aux_label_focal_loss"),
             "f": ("probe", "loss.label_focal_loss"),
             "g": ("probe", "f1.iou")}


@pytest.mark.parametrize("variant", sorted(ct.VARIANTS))
def test_a_wrong_criterion_is_noticed(variant):
    name, what = CAUGHT_BY[variant]
    case = next(c for c in ct.CASES if c.name == name)
    plain = ct.truth(case)
    ref_errors = ct.errors(composition_f32(case), plain)
    wrong = ct.errors(ct.statement(case, variant), plain)
    err, scale = wrong[what]
    bound = measured_bound(ref_errors[what][0], scale)
    print(f"variant {variant} ({ct.VARIANTS[variant]}): {name} {what} off by {err:.3e}, bound {bound:.3e}")
    assert err > bound, (variant, err, bound)
