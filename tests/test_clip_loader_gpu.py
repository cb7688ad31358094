"""``ClipLoader`` on the device: the producer thread drives the JPEG decode, augment and static-clip kernels on the
loader's own stream, one or more clips ahead of the consumer; every byte must equal the CPU loader's (the host
statements of the same stages), whatever the prefetch depth, and the first clip must train.

Shapes: 48 x 80 and 37 x 53 frames (partial MCUs, a row pitch that is no multiple of 16), 4:2:0 and 4:4:4, clips of 2
and 3 frames, still images of 40 x 56; the plans are set by hand (clip_loader_helpers.py): the clips stay tiny."""
import dataclasses

import pytest
import torch

import clip_loader_helpers as H
import dataset_trees as trees

from memotr_amd.data import ClipLoader

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def libs():
    from memotr_amd import build
    for name in ("jpeg", "jpeg_enc", "augment", "static_clip"):
        build.build(name)


@pytest.fixture(scope="module")
def roots(tmp_path_factory, libs):
    """{(h, w, subsampling): DATA_ROOT}, written once."""
    made = {}
    for h, w, sub, only in ((48, 80, "4:2:0", ("DanceTrack",)), (37, 53, "4:4:4", ("DanceTrack",)),
                            (40, 56, "4:2:0", ("MOT17",))):
        made[(h, w, sub)] = trees.write_trees(str(tmp_path_factory.mktemp(f"clips_{h}x{w}")),
                                              write_image=H.image_writer(h, w, sub), only=only)
    return made


def run_epoch(loader, epoch):
    out = []
    for batch in loader.epoch(epoch):
        if loader.device.type == "cuda":
            assert batch["nested"].tensors.is_cuda and batch["imgs"][0][0].is_cuda
        out.append(H.snapshot(batch))
    return out


@pytest.mark.parametrize("size,sub,branch,epoch", [((48, 80), "4:2:0", "plain", 0), ((48, 80), "4:2:0", "crop", 2),
                                                   ((37, 53), "4:4:4", "plain", 2), ((37, 53), "4:4:4", "crop", 0)])
def test_an_epoch_on_the_device_equals_the_cpu_loader(roots, size, sub, branch, epoch):
    root = roots[size + (sub,)]
    plan = H.PLAIN if branch == "plain" else H.CROP
    want = run_epoch(ClipLoader(H.dance_dataset(root, plans=[plan]), "cpu", seed=5), epoch)
    got = run_epoch(ClipLoader(H.dance_dataset(root, plans=[plan]), "cuda", seed=5), epoch)
    assert len(want) == (10 if epoch == 0 else 8) and want[0][0].shape == (2 if epoch == 0 else 3, 3, 64, 64)
    assert want[0][2][1:] == ((33, 41),) * (2 if epoch == 0 else 3)
    H.assert_same_epoch(got, want)


@pytest.mark.parametrize("plan,epoch", [(H.STATIC, 0), (H.STATIC_REVERSED, 3)], ids=["shift", "shift_reversed"])
def test_still_images_and_sequences_in_one_epoch_equal_the_cpu_loader(roots, plan, epoch):
    root = roots[(40, 56, "4:2:0")]
    want = run_epoch(ClipLoader(H.mot_dataset(root, static_plans=[plan]), "cpu", seed=5), epoch)
    got = run_epoch(ClipLoader(H.mot_dataset(root, static_plans=[plan]), "cuda", seed=5), epoch)
    assert len(want) == (3 if epoch == 0 else 10)                  # CrowdHuman alone, then joined by MOT17 (T = 3)
    H.assert_same_epoch(got, want)


def test_the_prefetch_depth_does_not_change_the_bytes(roots):
    """Depth 3 keeps the producer up to four clips ahead: the pinned ring (depth + 1 slots) is written again while
    earlier uploads may still be queued, and clips wait in the hand-over while later ones are made."""
    root = roots[(48, 80, "4:2:0")]
    shallow = run_epoch(ClipLoader(H.dance_dataset(root), "cuda", seed=8, prefetch=1, decode_threads=1), 0)
    deep = run_epoch(ClipLoader(H.dance_dataset(root), "cuda", seed=8, prefetch=3, decode_threads=2), 0)
    H.assert_same_epoch(deep, shallow)
    H.assert_same_epoch(deep, run_epoch(ClipLoader(H.dance_dataset(root), "cpu", seed=8), 0))


def test_the_ground_truth_arrives_on_the_device_in_one_buffer(roots):
    root = roots[(48, 80, "4:2:0")]
    loader = ClipLoader(H.dance_dataset(root), "cuda", seed=8)
    it = loader.epoch(0)
    batch = next(it)
    device = torch.device("cuda")
    buf = batch["infos_buffer"]
    lo, hi = buf.data_ptr(), buf.data_ptr() + buf.numel()
    n = 0
    for info in batch["infos"][0]:
        assert set(info) == {"ids", "labels", "boxes"}
        assert info["ids"].dtype == info["labels"].dtype == torch.int64 and info["boxes"].dtype == torch.float32
        assert info["boxes"].shape == (len(info["ids"]), 4)
        for v in info.values():
            assert v.is_cuda and (v.numel() == 0 or lo <= v.data_ptr() < hi)
        n += len(info["ids"])
    assert n > 0 and buf.numel() == 32 * n
    # engine.clip_forward_backward's test for its "resident" path
    assert all(v.device.type == device.type for v in batch["infos"][0][0].values() if torch.is_tensor(v))
    it.close()


def test_the_first_loader_clip_trains_the_small_model(roots):
    from model_helpers import build_small_memotr, small_config

    from memotr_amd import build
    from memotr_amd.engine import build_optimizer, clip_forward_backward, optimizer_step
    from memotr_amd.models.criterion import build as build_criterion
    for name in ("msda", "clip", "opt"):
        build.build(name)
    cfg = small_config()
    cfg.update(MATCH_COST_CLASS=2, MATCH_COST_BBOX=5, MATCH_COST_GIOU=2, LOSS_WEIGHT_FOCAL=2, LOSS_WEIGHT_L1=5,
               LOSS_WEIGHT_GIOU=2, AUX_LOSS_WEIGHT=[1.0], SAMPLE_LENGTHS=[2, 3], LR=2e-4, LR_BACKBONE=2e-5,
               LR_POINTS=1e-5, WEIGHT_DECAY=5e-4, CLIP_MAX_NORM=0.1)
    torch.manual_seed(0)
    model = build_small_memotr().cuda().train()
    optimizer = build_optimizer(cfg, model)
    device = torch.device("cuda")
    plan = dataclasses.replace(H.PLAIN, final=(96, 128))           # the small model's frame size in the other GPU tests
    loader = ClipLoader(H.dance_dataset(roots[(48, 80, "4:2:0")], plans=[plan]), device, seed=8)
    before = [p.detach().clone() for p in model.parameters()]
    it = loader.epoch(0)
    batch = next(it)
    assert batch["imgs"][0][0].shape == (3, 96, 128) and sum(len(i["ids"]) for i in batch["infos"][0]) > 0
    loss, _ = clip_forward_backward(model, build_criterion(cfg), batch, device)
    optimizer_step(model, optimizer, cfg["CLIP_MAX_NORM"])
    it.close()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    assert sum(not torch.equal(a, p) for a, p in zip(before, model.parameters())) > 100
    assert all(torch.isfinite(p).all() for p in model.parameters())
