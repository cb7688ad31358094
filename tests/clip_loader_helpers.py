"""Shared by the clip-loader tests (test infrastructure): dataset trees with real, tiny JPEG frames written by the
project's own encoder, datasets whose plans are set by hand so that the augmented clips stay tiny, and the comparison
of two batches bit for bit."""
import dataclasses

import torch

import dataset_trees as trees

from memotr_amd.data import datasets as D
from memotr_amd.data.augment import ClipAugment

PLAIN = ClipAugment(flip=True, first=None, crop=None, final=(33, 41), hsv=(-3, 12, -20), reverse=True)
CROP = ClipAugment(flip=False, first=(60, 100), crop=(7, 13, 40, 50), final=(33, 41), hsv=(2, -9, 14), reverse=False)
STATIC = dataclasses.replace(PLAIN, reverse=False, shift=(-3, 2), shift_reverse=False)
STATIC_REVERSED = dataclasses.replace(CROP, shift=(-3, 2), shift_reverse=True)


def image_writer(h, w, subsampling="4:2:0", quality=90):
    from memotr_amd.data import encode_jpeg

    def write(path, index):
        with open(path, "wb") as f:
            f.write(encode_jpeg(torch.from_numpy(trees.frame_pixels(index, h, w)), quality=quality,
                                subsampling=subsampling))
    return write


class _HandPlans:
    """``sample_plan`` picks one of ``plans`` (``static_plans`` for a still image) with the sample's own generator."""
    plans = (PLAIN, CROP)
    static_plans = (STATIC, STATIC_REVERSED)

    def sample_plan(self, h, w, rng, np_rng, static=False):
        return rng.choice(self.static_plans if static else self.plans)


class DanceTrackHandPlans(_HandPlans, D.DanceTrackDataset):
    pass


class MOT17HandPlans(_HandPlans, D.MOT17Dataset):
    pass


def dance_dataset(root, plans=None, **overrides):
    ds = DanceTrackHandPlans(dict(trees.DANCE_CONFIG, DATA_ROOT=root, **overrides))
    if plans is not None:
        ds.plans = tuple(plans)
    return ds


def mot_dataset(root, static_plans=None, **overrides):
    ds = MOT17HandPlans(dict(trees.MOT_CONFIG, DATA_ROOT=root, **overrides))
    if static_plans is not None:
        ds.static_plans = tuple(static_plans)
    return ds


def snapshot(batch):
    """What a batch holds, on the host: (tensors, masks, sizes, [per frame (ids, labels, boxes)], frame views)."""
    nested = batch["nested"]
    infos = [tuple(info[k].cpu().clone() for k in ("ids", "labels", "boxes")) for info in batch["infos"][0]]
    return (nested.tensors.cpu().clone(), nested.masks.cpu().clone(), tuple(nested.sizes), infos,
            [f.cpu().clone() for f in batch["imgs"][0]])


def assert_same(a, b):
    ta, ma, sa, ia, fa = a
    tb, mb, sb, ib, fb = b
    assert sa == sb
    assert ta.shape == tb.shape and torch.equal(ta, tb)
    assert torch.equal(ma, mb)
    assert len(ia) == len(ib) and len(fa) == len(fb)
    for x, y in zip(ia, ib):
        for u, v in zip(x, y):
            assert u.dtype == v.dtype and u.shape == v.shape and torch.equal(u, v)
    for u, v in zip(fa, fb):
        assert torch.equal(u, v)


def assert_same_epoch(a, b):
    assert len(a) == len(b) and len(a) > 0
    for x, y in zip(a, b):
        assert_same(x, y)
