"""CPU: annotated output without a host result -- ``MultiSequenceTracker.track_many_annotated`` /
``track_many_annotated_logged``, ``SequenceTracker.track_annotated_logged``, ``render.MultiAnnotatedWriter`` and
``submit(annotate_dir=...)`` -- against ``encode_jpeg(draw_tracks_host(...))`` of the logged rows
(tests/multi_annotated_cases.py).  On CPU tensors the table is ``clip_ops.draw_table_reference`` and the writer's worker
draws and encodes with the host statements."""
import pytest

import multi_annotated_cases as A
import multi_track_cases as M
from model_helpers import patch_operator


@pytest.fixture(scope="module")
def model():
    return M.scenario_model(64)


@pytest.mark.parametrize("subsampling", ["4:2:0", "4:4:4"])
def test_the_logged_loop_writes_the_host_statements_files_of_the_logged_rows(model, monkeypatch, subsampling):
    patch_operator(monkeypatch)
    A.check_logged(model, "cpu", subsampling)


def test_the_generator_writes_the_files_of_the_results_it_yields(model, monkeypatch):
    patch_operator(monkeypatch)
    A.check_generator(model, "cpu")


def test_one_sequence_logged_writes_the_files_of_track_annotated(model, monkeypatch, tmp_path):
    patch_operator(monkeypatch)
    A.check_single(model, "cpu", tmp_path)


def test_submit_writes_one_annotated_file_per_frame_and_the_same_results(model, monkeypatch, tmp_path, request):
    request.getfixturevalue("hip_lib"), request.getfixturevalue("clip_lib")
    patch_operator(monkeypatch)
    thresholds = dict(DET_SCORE_THRESH=0.7, TRACK_SCORE_THRESH=0.45, RESULT_SCORE_THRESH=0.6, MISS_TOLERANCE=2,
                      USE_MOTION=False)
    A.check_submit(model, tmp_path, thresholds, dict(raw_size=M.RAW_SIZE, area_thresh=10))


def test_the_writer_refuses_what_it_cannot_write_and_reports_the_workers_error():
    A.check_writer_errors()
