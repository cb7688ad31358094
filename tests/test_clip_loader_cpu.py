"""``ClipLoader`` on the CPU statements of decode and augment (memotr_amd/data/loader.py): what is drawn, that the bytes
of a clip depend on (seed, epoch, index) alone, the composition of the stages, and the life of the producer thread."""
import os
import random
import threading

import numpy as np
import pytest
import torch

import clip_loader_helpers as H
import dataset_trees as trees

from memotr_amd.data import (ClipLoader, CorruptJpeg, augment_clip, augment_static_clip, clip_batch, decode_jpegs,
                             loader as L)


@pytest.fixture(scope="module")
def jpeg_lib():
    from memotr_amd.build import build_jpeg_lib
    build_jpeg_lib()


@pytest.fixture(scope="module")
def enc_lib():
    from memotr_amd.build import build_jpeg_enc_lib
    build_jpeg_enc_lib()


@pytest.fixture(scope="module")
def root(tmp_path_factory, jpeg_lib, enc_lib):
    return trees.write_trees(str(tmp_path_factory.mktemp("clips")), write_image=H.image_writer(48, 80),
                             only=("DanceTrack", "MOT17"))


def run_epoch(loader, epoch):
    return [H.snapshot(b) for b in loader.epoch(epoch)]


def test_the_test_frames_are_small_and_decode_back(root):
    path = os.path.join(root, "DanceTrack", "train", "dancetrack0002", "img1", "00000001.jpg")
    assert os.path.getsize(path) < 6000
    frames = decode_jpegs([path], "cpu")
    assert frames.shape == (1, 48, 80, 3) and frames.dtype == torch.uint8
    assert (frames[0].int() - torch.from_numpy(trees.frame_pixels(7)).int()).abs().float().mean() < 6.0


# ------------------------------------------------------------------------------------------------- what is drawn
def test_the_order_is_a_permutation_per_epoch_and_ranks_share_it():
    n = 10
    orders = [L.epoch_order(n, e, seed=5) for e in range(3)]
    assert all(sorted(o) == list(range(n)) for o in orders) and orders[0] != orders[1] != orders[2]
    g = torch.Generator()
    g.manual_seed(5 + 2)
    assert orders[2] == torch.randperm(n, generator=g).tolist()
    assert L.epoch_order(n, 1, seed=5, shuffle=False) == list(range(n))
    world = 3
    shards = [L.epoch_order(n, 1, seed=5, rank=r, world_size=world) for r in range(world)]
    assert [len(s) for s in shards] == [4, 4, 4]
    padded = [shards[k % world][k // world] for k in range(12)]
    assert padded[:n] == orders[1] and padded[n:] == orders[1][:2]              # DistributedSampler's wrap-around
    before_padding = [[v for k, v in enumerate(s) if k * world + r < n] for r, s in enumerate(shards)]
    assert sorted(sum(before_padding, [])) == list(range(n))                    # disjoint, and together the epoch
    assert L.epoch_order(2, 0, seed=0, rank=4, world_size=5, shuffle=False) == [0]      # wraps more than once
    with pytest.raises(ValueError):
        L.epoch_order(n, 0, seed=0, rank=3, world_size=3)


def test_a_samples_generators_depend_on_seed_epoch_and_index_only():
    a, b = L.sample_rngs(7, 2, 5), L.sample_rngs(7, 2, 5)
    assert a[0].random() == b[0].random() and a[1].uniform() == b[1].uniform()
    draws = {(L.sample_rngs(*k)[0].random(), L.sample_rngs(*k)[1].uniform())
             for k in ((7, 2, 5), (8, 2, 5), (7, 3, 5), (7, 2, 6), (2, 7, 5))}
    assert len(draws) == 5


def test_the_interval_is_drawn_first_then_the_plan(root):
    ds = H.dance_dataset(root)
    loader = ClipLoader(ds, "cpu", seed=3, shuffle=False)
    ds.set_epoch(0)
    rng, np_rng = L.sample_rngs(3, 0, 4)
    sample = ds.sample(4, rng)
    plan = ds.sample_plan(48, 80, rng, np_rng, False)
    frames = decode_jpegs(sample.paths, "cpu")
    want = clip_batch(*augment_clip(frames, sample.infos, plan, overflow_bbox=sample.overflow_bbox))
    got = loader.load(0, 4)
    assert len(got["imgs"][0]) == 2
    for f, g in zip(got["imgs"][0], want["imgs"][0]):
        assert torch.equal(f, g)
    for a, b in zip(got["infos"][0], want["infos"][0]):
        assert torch.equal(a["boxes"], b["boxes"]) and torch.equal(a["ids"], b["ids"])


# ------------------------------------------------------------------------------------------------- the same bytes
def test_prefetch_depth_and_decode_threads_do_not_change_the_bytes(root):
    ds = H.dance_dataset(root)
    base = run_epoch(ClipLoader(ds, "cpu", seed=11, prefetch=1, decode_threads=1), 0)
    assert len(base) == 10
    H.assert_same_epoch(base, run_epoch(ClipLoader(ds, "cpu", seed=11, prefetch=3, decode_threads=2), 0))
    assert {tuple(b[0].shape) for b in base} == {(2, 3, 64, 64)}
    assert len({b[0].numpy().tobytes() for b in base}) == len(base)             # ten different clips


def test_a_new_loader_reproduces_an_epoch_without_the_epochs_before_it(root):
    first = ClipLoader(H.dance_dataset(root), "cpu", seed=11)
    for e in (0, 1):
        run_epoch(first, e)
    want = run_epoch(first, 2)
    assert len(want) == 8 and want[0][0].shape[0] == 3                          # the second stage: clips of 3 frames
    H.assert_same_epoch(want, run_epoch(ClipLoader(H.dance_dataset(root), "cpu", seed=11), 2))
    other = run_epoch(ClipLoader(H.dance_dataset(root), "cpu", seed=12), 2)
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(want, other))


def test_rank_shards_are_the_strided_epoch(root):
    ds = H.dance_dataset(root)
    whole = run_epoch(ClipLoader(ds, "cpu", seed=4), 0)
    for rank in range(2):
        H.assert_same_epoch(whole[rank::2], run_epoch(ClipLoader(ds, "cpu", seed=4, rank=rank, world_size=2), 0))


# ------------------------------------------------------------------------------------------------- composition
@pytest.mark.parametrize("branch", ["plain", "crop"])
def test_a_loader_clip_is_decode_augment_clip_batch(root, branch):
    plan = H.PLAIN if branch == "plain" else H.CROP
    ds = H.dance_dataset(root, plans=[plan])
    got = run_epoch(ClipLoader(ds, "cpu", seed=9, shuffle=False), 2)
    ds.set_epoch(2)
    for index in range(len(ds)):
        rng, np_rng = L.sample_rngs(9, 2, index)
        sample = ds.sample(index, rng)
        assert ds.sample_plan(48, 80, rng, np_rng, False) is plan
        nested, infos = augment_clip(decode_jpegs(sample.paths, "cpu"), sample.infos, plan,
                                     overflow_bbox=sample.overflow_bbox)
        want = clip_batch(nested, infos)
        want["nested"] = nested
        H.assert_same(got[index], H.snapshot(want))
    assert got[0][2] == ((64, 64), (33, 41), (33, 41), (33, 41))
    assert sum(len(ids) for _, _, _, infos, _ in got for ids, _, _ in infos) > 20          # boxes came through
    assert all((boxes >= 0).all() and (boxes[:, :2] <= 1.5).all() for *_, infos, _ in got for _, _, boxes in infos)


@pytest.mark.parametrize("plan", [H.STATIC, H.STATIC_REVERSED], ids=["shift", "shift_reversed"])
def test_a_still_image_goes_through_augment_static_clip(root, plan):
    ds = H.mot_dataset(root, static_plans=[plan])
    got = run_epoch(ClipLoader(ds, "cpu", seed=9, shuffle=False), 0)           # epoch 0: CrowdHuman only
    assert len(got) == 3
    ds.set_epoch(0)
    for index in range(3):
        sample = ds.sample(index, random.Random(0))
        assert sample.static and len(set(sample.paths)) == 1 and len(sample.paths) == 2
        image = decode_jpegs(sample.paths[:1], "cpu")[0]
        nested, infos = augment_static_clip(image, sample.infos[0], plan, 2, overflow_bbox=sample.overflow_bbox)
        want = clip_batch(nested, infos)
        want["nested"] = nested
        H.assert_same(got[index], H.snapshot(want))
    assert not torch.equal(got[0][4][0], got[0][4][1])                          # the shift moved the second frame
    mixed = run_epoch(ClipLoader(ds, "cpu", seed=9, shuffle=False), 1)          # CrowdHuman first, then MOT17
    assert len(mixed) == 12
    H.assert_same_epoch(mixed[:3], got)


def test_bgr_decodes_in_that_order_and_swaps_back(root):
    ds = H.dance_dataset(root)
    H.assert_same_epoch(run_epoch(ClipLoader(ds, "cpu", seed=2, bgr=True), 4),
                        run_epoch(ClipLoader(ds, "cpu", seed=2), 4))


# ------------------------------------------------------------------------------------------------- errors, lifecycle
def test_a_corrupt_file_raises_at_its_own_clip_and_the_producer_is_joined(tmp_path, jpeg_lib, enc_lib):
    root = trees.write_trees(str(tmp_path), write_image=H.image_writer(48, 80), only=("DanceTrack",))
    bad = os.path.join(root, "DanceTrack", "train", "dancetrack0007", "img1", "00000001.jpg")
    data = open(bad, "rb").read()
    with open(bad, "wb") as f:
        f.write(data[:len(data) // 2])
    ds = H.dance_dataset(root)
    baseline = threading.active_count()
    it = ClipLoader(ds, "cpu", seed=1, shuffle=False, prefetch=3).epoch(0)
    delivered = [H.snapshot(next(it)) for _ in range(4)]                        # dancetrack0002's four clips
    assert all(d[0].shape == (2, 3, 64, 64) for d in delivered)
    with pytest.raises(CorruptJpeg):
        next(it)                                                                # (dancetrack0007, 1) reads the bad file
    with pytest.raises(StopIteration):
        next(it)
    assert threading.active_count() == baseline


def test_frames_of_different_sizes_are_refused(tmp_path, jpeg_lib, enc_lib):
    root = trees.write_trees(str(tmp_path), write_image=H.image_writer(48, 80), only=("DanceTrack",))
    H.image_writer(37, 53)(os.path.join(root, "DanceTrack", "train", "dancetrack0002", "img1", "00000002.jpg"), 0)
    it = ClipLoader(H.dance_dataset(root), "cpu", seed=1, shuffle=False).epoch(0)
    with pytest.raises(ValueError, match="differ in size"):
        next(it)


def test_streams_only_pillow_reads_take_the_fallback_path(tmp_path, jpeg_lib, enc_lib):
    Image = pytest.importorskip("PIL.Image")
    from memotr_amd.data import UnsupportedJpeg, parse_jpeg
    root = trees.write_trees(str(tmp_path), write_image=H.image_writer(48, 80), only=("DanceTrack",))
    seq = os.path.join(root, "DanceTrack", "train", "dancetrack0002", "img1")
    for t in range(1, 6):                                                       # progressive: not the host stage's kind
        Image.fromarray(trees.frame_pixels(t)).save(os.path.join(seq, f"{t:08d}.jpg"), quality=90, progressive=True)
    with pytest.raises(UnsupportedJpeg):
        parse_jpeg(os.path.join(seq, "00000001.jpg"))
    ds = H.dance_dataset(root, plans=[H.CROP])
    it = ClipLoader(ds, "cpu", seed=1, shuffle=False).epoch(0)
    got = H.snapshot(next(it))
    it.close()
    rng, _ = L.sample_rngs(1, 0, 0)
    sample = ds.sample(0, rng)
    frames = torch.stack([torch.from_numpy(np.asarray(Image.open(p).convert("RGB")).copy()) for p in sample.paths])
    nested, infos = augment_clip(frames, sample.infos, H.CROP, overflow_bbox=sample.overflow_bbox)
    want = clip_batch(nested, infos)
    want["nested"] = nested
    H.assert_same(got, H.snapshot(want))


def test_abandoning_the_generator_joins_the_producer(root):
    baseline = threading.active_count()
    loader = ClipLoader(H.dance_dataset(root), "cpu", seed=1, prefetch=1)
    it = loader.epoch(0)
    next(it)
    assert threading.active_count() == baseline + 1
    with pytest.raises(RuntimeError, match="still live"):
        next(loader.epoch(0))
    it.close()
    assert threading.active_count() == baseline
    it = loader.epoch(0)
    next(it)
    del it                                                                      # dropped, not closed
    assert threading.active_count() == baseline
    assert len(run_epoch(loader, 0)) == 10 and threading.active_count() == baseline


def test_decode_threads_are_capped_by_the_library(root):
    from memotr_amd import _jpeg_lib
    assert ClipLoader(H.dance_dataset(root), "cpu", decode_threads=1000).decode_threads == _jpeg_lib.MAX_THREADS == 16
    with pytest.raises(ValueError):
        ClipLoader(H.dance_dataset(root), "cpu", prefetch=0)


def test_train_from_config_puts_dataset_and_loader_in_front_of_fit(root, monkeypatch):
    import memotr_amd.models as models
    import memotr_amd.models.criterion as criterion
    import memotr_amd.train as train
    seen = {}

    def fit(config, model, crit, make_batches, *, device, **kwargs):
        seen.update(model=model, criterion=crit, device=device, kwargs=kwargs,
                    epochs=[[H.snapshot(b) for b in make_batches(e)] for e in (0, 2)])
        return "optimizer", "scheduler", {"start_epoch": 2}

    monkeypatch.setattr(models, "build_model", lambda config: torch.nn.Linear(2, 2))
    monkeypatch.setattr(criterion, "build", lambda config: "criterion")
    monkeypatch.setattr(train, "fit", fit)
    monkeypatch.setattr(H.D, "sample_clip_augment", lambda *a, **k: H.PLAIN)    # the real plans are 600+ pixels high
    config = dict(trees.DANCE_CONFIG, DATA_ROOT=root, SEED=11)
    baseline = threading.active_count()
    model, optimizer, scheduler, states = train.train_from_config(config, prefetch=1, decode_threads=1, log_every=7)
    assert isinstance(model, torch.nn.Linear) and (optimizer, scheduler) == ("optimizer", "scheduler")
    assert seen["criterion"] == "criterion" and seen["device"] == torch.device("cpu")
    assert seen["kwargs"] == dict(outputs_dir=None, impl=None, log_every=7, on_log=None)
    assert [len(e) for e in seen["epochs"]] == [10, 8] and threading.active_count() == baseline
    ds = H.dance_dataset(root, plans=[H.PLAIN])
    H.assert_same_epoch(seen["epochs"][1], run_epoch(ClipLoader(ds, "cpu", seed=11), 2))
