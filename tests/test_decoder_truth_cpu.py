"""CPU: the conditions under which tests/test_decoder_truth_gpu.py holds the decoder loop and the query updater to
float64 truth (tests/decoder_truth.py).

* The inputs.  For every case the GPU test uses, the float32 CPU run and the float64 CPU run take the same decisions,
  every one: the sign under each ReLU, the bilinear cell of each sampling point, ``score > update_threshold`` (and every
  score at least 1e-3 from the threshold).  Zero disagreements, not "few": one flipped decision puts both fp32 paths
  1e-3 .. 1e-2 from truth and the measured bound with them.  And no decision of the float64 run sits within a device's
  float32 round-off of its edge (``RELU_MARGIN``, ``CELL_MARGIN``), where it could still fall the other way on the GPU.
* The rule has teeth.  Defects planted into a float32 CPU copy, each in turn, land outside ``measured_bound`` of the
  float32 CPU composition; the untouched copy stays inside.
"""
import copy

import pytest
import torch

import decoder_truth as dt
from decoder_truth import Case


@pytest.fixture(scope="module", autouse=True)
def _libraries(hip_lib, clip_lib):
    """The package has no CPU fallback to import: its libraries are built first (nothing here launches a kernel)."""


# ------------------------------------------------------------------------------------------------ the cases themselves
def test_the_cases_reach_what_they_are_meant_to_reach():
    from memotr_amd.functions import clip_ops
    from memotr_amd.models import updater_graphs
    from memotr_amd.models.decoder_graphs import BUCKET, DecoderGraphs
    assert dt.ND % 16 != 0                                            # layer 0 splits inside an attention tile
    assert {c.n_track for c in dt.GRAPH_CASES} == set(dt.TRACKS) == set(dt.ALT_TRACKS)
    assert {(c.use_dab, c.merge) for c in dt.GRAPH_CASES} == {(a, m) for a in (True, False) for m in (0, 1)}
    for nt, alt in dt.ALT_TRACKS.items():       # the second replay: another live count, the same capture
        assert nt != alt and DecoderGraphs.bucket(dt.ND + nt, dt.ND) == DecoderGraphs.bucket(dt.ND + alt, dt.ND)
        assert DecoderGraphs.bucket(dt.ND + nt, dt.ND) > dt.ND + max(nt, alt)          # ... and every case is padded
    assert dt.ND + 13 == BUCKET + 1 and DecoderGraphs.bucket(dt.ND + 13, dt.ND) == 2 * BUCKET
    for n, alt in dt.UPDATER_ALT_ROWS.items():
        assert n != alt and -(-n // updater_graphs.BUCKET) == -(-alt // updater_graphs.BUCKET)
    assert {-(-n // updater_graphs.BUCKET) for n in dt.UPDATER_ROWS} == {1, 2, 3}
    # d_ffn 64: every FFN linear inside the kernels' limits; WIDE_FFN: linear1 (256 -> d_ffn) past the output limit both
    # ways, linear2 (d_ffn -> 256) past the forward kernel's input limit
    assert 64 <= clip_ops.LINEAR_BWD_MAX_OUT and 64 <= clip_ops.LINEAR_FWD_MAX_IN
    assert dt.WIDE_FFN > clip_ops.LINEAR_BWD_MAX_OUT and dt.WIDE_FFN > clip_ops.LINEAR_FWD_MAX_IN
    assert {c.d_ffn for c in dt.GRAPH_CASES} == {64, dt.WIDE_FFN}
    assert all(c.extra_track_attn for c in dt.EAGER_ONLY_CASES) and not any(c.extra_track_attn for c in dt.GRAPH_CASES)
    assert dt.masked_track_slots(7) == (3, 6) and dt.masked_track_slots(13) == (6, 12) and dt.masked_track_slots(1) == ()
    x = dt.decoder_inputs(Case(True, 7, 1))
    assert x["query_mask"][1].nonzero().flatten().tolist() == [dt.ND + 3, dt.ND + 6] and not x["query_mask"][0].any()
    assert bool((x["valid_ratios"][1] < 1).all()) and bool((x["valid_ratios"][0] == 1).all())
    assert bool(x["src_mask"][1].any()) and not bool(x["src_mask"][0].any())


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("case", dt.DECODER_CASES, ids=lambda c: c.name)
def test_float32_and_float64_take_the_same_decisions_in_every_decoder_case(monkeypatch, case, which):
    relu, cell, taken, margins, got32, got64 = dt.decoder_decisions(monkeypatch, case, which)
    assert taken > 50_000
    assert relu == 0 and cell == 0, (case.name, which, relu, cell, taken)
    assert margins[0] >= dt.RELU_MARGIN and margins[1] >= dt.CELL_MARGIN, (case.name, which, margins)
    # ... and with them the float32 composition is round-off away from truth
    for k, e in dt.errors(got32, got64).items():
        scale = dt.out_scale(got64[k])
        if scale == 0:      # a parameter no row reaches: the track attention of a layer 0 that sees the detect queries only
            assert e == 0 and case.extra_track_attn and (".0.track_attn." in k or ".0.norm4." in k), (k, e)
        else:
            assert e / scale < dt.REF_ERROR_CAP, (k, e, scale)


@pytest.mark.parametrize("use_dab", (True, False))
def test_float32_and_float64_take_the_same_decisions_in_every_updater_case(use_dab):
    qu = dt.build_updater(use_dab)
    sets = [dt.updater_fields(n, use_dab) for n in dt.UPDATER_ROWS + tuple(dt.UPDATER_ALT_ROWS.values())]
    _, per_stream = dt.build_bank(use_dab)
    sets += [(f, dt.updater_fields(len(slots), use_dab, seed=9)[1]) for f, slots in per_stream if f is not None]
    assert len(sets) == 10
    for fields, weights in sets:
        relu, pos, taken, margin = dt.updater_decisions(qu, fields, weights)
        assert taken > 1000 and relu == 0 and pos == 0, (len(fields[0]), relu, pos)
        assert margin >= dt.RELU_MARGIN, (len(fields[0]), margin)
        assert dt.score_margin(qu, fields[0]) >= dt.SCORE_MARGIN
        n_pos = int((fields[0].sigmoid().max(1).values > qu.update_threshold).sum())
        assert n_pos >= 1 and (len(fields[0]) < 5 or n_pos < len(fields[0]))            # both sides of the select


# ------------------------------------------------------------------------------------------------ planted defects
def planted_layer_forward(layer, defect):
    """``DeformableDecoderLayer.forward`` restated with one switch per planted defect (None: no defect -- the test holds
    this statement to the layer's own, bit for bit, before it trusts what the switches show)."""
    from memotr_amd.functions.clip_ops import add_layer_norm
    from memotr_amd.modules.attention import self_attention

    def forward(tgt, query_pos, reference_points, src, shapes, level_start, query_mask, src_padding_mask=None,
                merge_det_track=False, value=None):
        nd, track_tgt = layer.n_det_queries, None
        if not merge_det_track:
            tgt, track_tgt = tgt.split((nd, tgt.shape[1] - nd), dim=1)
            query_pos, reference_points, query_mask = query_pos[:, :nd], reference_points[:, :nd], query_mask[:, :nd]
        if layer.extra_track_attn:
            tgt = layer.forward_track_attn(tgt, query_pos, query_mask)
        v = tgt.detach() if defect == "detached_value_in_self_attention" else tgt
        attn = self_attention(layer.self_attn, tgt + query_pos, v, key_padding_mask=query_mask)
        tgt = add_layer_norm(tgt, attn, layer.norm2)
        q = tgt if defect == "no_query_pos_in_cross_attention" else tgt + query_pos
        cross = layer.cross_attn(q, reference_points, src, shapes, level_start, src_padding_mask, value)
        tgt = layer.forward_ffn(add_layer_norm(tgt, cross, layer.norm1))
        return tgt if track_tgt is None else torch.cat((tgt, track_tgt), dim=1)

    return forward


DECODER_DEFECTS = ("no_query_pos_in_cross_attention", "padded_key_let_through", "no_layer0_split",
                   "detached_value_in_self_attention")
N_PAD = 5


@pytest.fixture(scope="module", params=(True, False), ids=("dab", "plain"))
def defect_ground(request):
    """One case per variant (7 tracks, two of them masked in batch 1, layer 0 split): truth, the float32 CPU composition
    and its error -- computed once, shared by the defects."""
    case = Case(request.param, 7, 1)
    dec, x = dt.build_decoder(case), dt.decoder_inputs(case)
    with pytest.MonkeyPatch.context() as mp:
        truth = dt.decoder_truth(mp, dec, x)
        dt.truth_operator(mp)
        ref = dt.run_decoder(dec, x)
    return case, dec, x, truth, ref, dt.errors(ref, truth)


def _planted_run(monkeypatch, ground, defect, padded):
    case, dec, x, truth, ref, ref_err = ground
    bad = copy.deepcopy(dec)
    for layer in bad.layers:
        layer.forward = planted_layer_forward(layer, defect)
    if defect == "no_layer0_split":
        bad.merge_det_track_layer = 0
    dt.truth_operator(monkeypatch)
    if padded:
        open_slot = 2 if defect == "padded_key_let_through" else None
        return dt.run_decoder(bad, dt.padded_like_the_capture(x, N_PAD, open_slot), keep=x["tgt"].shape[1])
    return dt.run_decoder(bad, x)


def test_the_untouched_copy_stays_inside_the_bound(monkeypatch, defect_ground):
    case, dec, x, truth, ref, ref_err = defect_ground
    got = _planted_run(monkeypatch, defect_ground, None, padded=False)
    assert got.keys() == ref.keys() and all(torch.equal(got[k], ref[k]) for k in ref)       # the restated layer IS the layer
    rows, bad = dt.check(case.name, "cpu-untouched", got, truth, ref_err, truth)
    assert not bad and len(rows) == len(truth) > 90
    # the padded form (what a capture runs): same truth, nothing reaches the padded rows
    got = _planted_run(monkeypatch, defect_ground, None, padded=True)
    assert not bool(got.pop("grad::tgt(padding)").any())
    rows, bad = dt.check(case.name, "cpu-padded", got, truth, ref_err, truth)
    assert not bad, bad


@pytest.mark.parametrize("defect", DECODER_DEFECTS)
def test_a_planted_decoder_defect_lands_outside_the_bound(monkeypatch, defect_ground, defect):
    case, dec, x, truth, ref, ref_err = defect_ground
    got = _planted_run(monkeypatch, defect_ground, defect, padded=defect == "padded_key_let_through")
    got.pop("grad::tgt(padding)", None)
    rows, bad = dt.check(case.name, "cpu-" + defect, got, truth, ref_err, truth)
    assert bad, defect
    caught = {r.tensor for r in bad}
    if defect == "detached_value_in_self_attention":        # the forward is untouched: only gradients can tell
        assert not any(t.startswith("out::") for t in caught) and "grad::tgt" in caught
    else:
        assert "out::outs" in caught and "grad::tgt" in caught
    if defect == "no_layer0_split":                         # ... which the exact assertion of the GPU test sees as well
        assert not torch.equal(got["out::outs"][0][:, dt.ND:], x["tgt"][:, dt.ND:])
        assert torch.equal(ref["out::outs"][0][:, dt.ND:], x["tgt"][:, dt.ND:])


# ------------------------------------------------------------------------------------------------ update_bank
def _cross_stream_update_bank(qu, bank):
    """``QueryUpdater.update_bank`` with the planted defect: one attention over the slots of all streams."""
    n, cap = bank.n_streams, bank.cap
    live = bank.ids >= 0
    with torch.no_grad():
        new = qu.update_fields(*(getattr(bank, f).reshape(n * cap, -1) for f in qu.FIELDS),
                               key_mask=~live.reshape(1, n * cap), n_streams=1)
    for name, t in zip(qu.BANK_UPDATED, new):
        old = getattr(bank, name)
        setattr(bank, name, torch.where(live.reshape(-1, 1), t, old.reshape(n * cap, -1)).view(old.shape))


@pytest.mark.parametrize("use_dab", (True, False))
def test_update_bank_per_stream_truth_and_the_cross_stream_defect(use_dab):
    qu = dt.build_updater(use_dab)
    bank, per_stream = dt.build_bank(use_dab)
    truth = dt.bank_truth(qu, per_stream, use_dab)
    qu.update_bank(bank)
    ref = dt.bank_fields(bank)
    ref_err = dt.errors(ref, truth)
    free = ~dt.bank_live_slots()
    for k, t in ref.items():
        assert bool(torch.isfinite(t).all()) and not bool(t[free].any()), k          # the empty stream left nothing
        assert ref_err[k] / dt.out_scale(truth[k]) < dt.REF_ERROR_CAP, k
    bad_bank, _ = dt.build_bank(use_dab)
    _cross_stream_update_bank(qu, bad_bank)
    rows, bad = dt.check(f"bank-{'dab' if use_dab else 'plain'}", "cpu-cross-stream", dt.bank_fields(bad_bank), truth,
                         ref_err, truth)
    assert {r.tensor for r in bad} == {"out::query_embed"}       # the one field the memory attention reaches
