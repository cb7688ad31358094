"""Shared by tests/test_multi_tracker_cpu.py and tests/test_multi_tracker_gpu.py: a scenario of three short sequences,
the one-sequence runs they are compared with, the decision margins and the equivalence of DESIGN 5.13.

The random-init models score every query near 0.01, which decides nothing: ``spread_scores`` redraws the class heads so
that the scores spread over (0, 1), and the thresholds below then give births in several frames, misses and retirements.
Seeds are chosen (on the CPU, ``python tests/multi_track_cases.py``) so that no decision score of the one-sequence runs
lies within ``MARGIN`` of its threshold: inside that band the 1e-4 agreement of the scores could flip a decision.
"""
import numpy as np
import torch

import dataset_trees as T

LENGTHS = (2, 4, 3)
FRAME_H, FRAME_W = 64, 96
RAW_SIZE = (96, 160)
MARGIN = 1e-3
TOL = 1e-4                    # boxes (normalised by the image size) and scores: tests/test_model_gpu.py:620's bound
THRESHOLDS = dict(det_score_thresh=0.8, track_score_thresh=0.45, result_score_thresh=0.55, miss_tolerance=2)
OPTIONS = dict(use_dab=True, area_thresh=10, raw_size=RAW_SIZE, **THRESHOLDS)
# (model seed, class-head scale) per hidden size, found by `seed_search`
SEEDS = {64: (22, 6.0), 256: (2, 6.0)}


def build_model(hidden: int = 64):
    """The small model of tests/model_helpers.py (hidden 64), or its 256-wide form whose attention heads are the
    32 wide ones of the hand-written kernels (tests/test_frames_gpu.py: build_memotr_cuda), on the CPU."""
    from model_helpers import TinyBackbone, build_small_memotr, small_config
    if hidden == 64:
        return build_small_memotr()
    from memotr_amd.models.backbone import BackboneWithPE
    from memotr_amd.models.deformable_transformer import build as build_tr
    from memotr_amd.models.memotr import MeMOTR
    from memotr_amd.models.position_embedding import build as build_pe
    from memotr_amd.models.query_updater import build as build_qu
    cfg = small_config()
    cfg.update(HIDDEN_DIM=hidden, FFN_DIM=hidden)
    return MeMOTR(backbone=BackboneWithPE(TinyBackbone(), build_pe(cfg)), transformer=build_tr(cfg),
                  query_updater=build_qu(cfg), num_classes=1, n_det_queries=cfg["NUM_DET_QUERIES"],
                  n_feature_levels=4, hidden_dim=hidden, ffn_dim=hidden, dropout=0.0, use_dab=True)


def scenario_model(hidden: int = 64):
    seed, scale = SEEDS[hidden]
    torch.manual_seed(seed)
    return spread_scores(build_model(hidden).eval(), seed, scale)


def sequences(lengths=LENGTHS, first=0):
    """``len(lengths)`` sequences of (64, 96, 3) uint8 frames: a small crop of the dataset trees' drifting pattern."""
    out = []
    for s, n in enumerate(lengths):
        frames = []
        for i in range(n):
            px = T.frame_pixels(first + 17 * s + i)
            reps = (-(-FRAME_H // px.shape[0]), -(-FRAME_W // px.shape[1]), 1)
            frames.append(torch.from_numpy(np.ascontiguousarray(np.tile(px, reps)[:FRAME_H, :FRAME_W])))
        out.append(frames)
    return out


def spread_scores(model, seed: int, scale: float):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for head in model.class_embed:
            w = torch.randn(head.weight.shape, generator=g) * scale / head.weight.shape[1] ** 0.5
            head.weight.copy_(w.to(head.weight.device))
            head.bias.zero_()
    return model


class Decisions:
    """Wraps ``RuntimeTracker.update`` of a SequenceTracker: every score a threshold decides on, with that threshold."""

    def __init__(self, tracker, update_threshold):
        self.pairs = []
        inner, rt = tracker.tracker.update, tracker.tracker

        def update(model_outputs, tracks):
            scores = model_outputs["pred_logits"][0].sigmoid().cpu()
            n_det = len(model_outputs["det_query_embed"])
            top = scores.max(-1).values
            labels = tracks[0].labels.cpu()
            own = scores[n_det:].gather(1, labels[:, None]).squeeze(1)
            self.pairs += [(float(s), rt.det_score_thresh) for s in top[:n_det]]
            self.pairs += [(float(s), rt.track_score_thresh) for s in own]
            born = top[:n_det] >= rt.det_score_thresh
            for s in torch.cat((top[:n_det][born], top[n_det:])).tolist():          # the updater's and the report's
                self.pairs += [(s, update_threshold), (s, tracker.result_score_thresh)]
            return inner(model_outputs=model_outputs, tracks=tracks)

        tracker.tracker.update = update

    def margin(self) -> float:
        return min(abs(s - t) for s, t in self.pairs)


def single_runs(model, seqs, options=OPTIONS):
    """Every sequence through a fresh SequenceTracker: ``(results[seq][frame], smallest decision margin)``."""
    from memotr_amd.inference import SequenceTracker
    from memotr_amd.models.utils import get_model
    results, margin = [], float("inf")
    for frames in seqs:
        t = SequenceTracker(model, **options)
        d = Decisions(t, get_model(model).query_updater.update_threshold)
        results.append([r for _, r in t.track(frames)])
        margin = min(margin, d.margin())
    return results, margin


def multi_runs(tracker, seqs):
    """The sequences through ``track_many``: ``results[seq][frame]``."""
    results = [[None] * len(frames) for frames in seqs]
    for seq, idx, r in tracker.track_many(seqs):
        assert results[seq][idx] is None
        results[seq][idx] = r
    assert all(r is not None for rows in results for r in rows)
    return results


def assert_equivalent(want, got, ori_h=FRAME_H, ori_w=FRAME_W):
    """ids, labels and the reported (frame, id) rows are equal; boxes and scores agree to TOL."""
    assert len(want) == len(got)
    scale = torch.tensor([ori_w, ori_h, ori_w, ori_h], dtype=torch.float32)
    for s, (a_seq, b_seq) in enumerate(zip(want, got)):
        assert len(a_seq) == len(b_seq), s
        for f, (a, b) in enumerate(zip(a_seq, b_seq)):
            assert a.ids.tolist() == b.ids.tolist(), (s, f, a.ids.tolist(), b.ids.tolist())
            assert a.labels.tolist() == b.labels.tolist(), (s, f)
            assert float(((a.boxes - b.boxes) / scale).abs().max() if len(a.ids) else 0.0) <= TOL, (s, f)
            assert float((a.scores - b.scores).abs().max() if len(a.ids) else 0.0) <= TOL, (s, f)


def scenario_is_eventful(results) -> bool:
    """Births in more than one frame, and a track that stops being reported or retires, somewhere in the scenario."""
    births = sum(1 for seq in results for f, r in enumerate(seq)
                 if f > 0 and set(r.ids.tolist()) - set(seq[f - 1].ids.tolist()))
    losses = sum(1 for seq in results for f, r in enumerate(seq)
                 if f > 0 and set(seq[f - 1].ids.tolist()) - set(r.ids.tolist()))
    return births >= 1 and losses >= 1 and all(len(seq[-1].ids) > 0 for seq in results)


def seed_search(hidden: int, build, scales=(2.0, 3.0, 4.0, 6.0), seeds=range(1, 40)):
    """Prints the (seed, scale) pairs whose one-sequence runs keep every decision ``1.5 * MARGIN`` from its threshold."""
    seqs = sequences()
    for scale in scales:
        for seed in seeds:
            torch.manual_seed(seed)
            model = spread_scores(build().eval(), seed, scale)
            results, margin = single_runs(model, seqs)
            print(hidden, seed, scale, round(margin, 5), scenario_is_eventful(results),
                  [[len(r.ids) for r in seq] for seq in results], flush=True)


if __name__ == "__main__":
    import sys

    import model_helpers
    import memotr_amd.modules.ms_deform_attn as mod
    mod.MSDeformAttnFunction = model_helpers.OracleMSDeformAttnFunction
    hidden = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    seed_search(hidden, lambda: build_model(hidden))
