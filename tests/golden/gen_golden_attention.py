"""Generate the attention-tap golden vectors by importing the REFERENCE (build container only).

    python tests/golden/gen_golden_attention.py

Runs the reference's small DAB model of fixture M5 (gen_golden_model.py: same seeds, hence the same weights and the
same two frames -- asserted against model_M5_memotr_two_frames.npz) with ``visualize=True`` in a temporary working
directory, and stores what its decoder dumps per frame and layer -- ``sampling_locations_layer_*``,
``detection_ref_pts_layer_*``, ``track_ref_pts_layer_*`` -- as arrays in tests/golden/attention_tap.npz.  Only data is
written; no reference source is copied.
"""
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(OUT))
import gen_golden_model as G  # noqa: E402
from conftest import load_npz, save_npz  # noqa: E402


def main():
    G.install_stubs()
    torch.set_num_threads(1)
    import models.backbone as ref_backbone
    from models.deformable_transformer import build as build_tr
    from models.memotr import MeMOTR
    from models.position_embedding import build as build_pe
    from models.query_updater import build as build_qu
    from models.runtime_tracker import RuntimeTracker
    from structures.track_instances import TrackInstances
    from utils.nested_tensor import NestedTensor, tensor_list_to_nested_tensor
    cfg = G.small_config()
    cfg.update(VISUALIZE=True)

    class TinyBackbone(nn.Module):
        def __init__(self):
            super().__init__()
            self.backbone = G.TinyBody()
            self.strides = [8, 16, 32]
            self.num_channels = [8, 12, 16]

        def forward(self, nt):
            res = {}
            for name, out in self.backbone(nt.tensors).items():
                m = F.interpolate(nt.masks[None].float(), mode="nearest", size=out.shape[-2:]).to(nt.masks.dtype)[0]
                res[name] = NestedTensor(out, m)
            return res

    torch.manual_seed(50)
    model = MeMOTR(backbone=ref_backbone.BackboneWithPE(TinyBackbone(), build_pe(cfg)), transformer=build_tr(cfg),
                   query_updater=build_qu(cfg), num_classes=1, n_det_queries=20, n_feature_levels=4, hidden_dim=64,
                   ffn_dim=128, dropout=0.0, aux_loss=True, with_box_refine=True, use_checkpoint=False,
                   checkpoint_level=2, use_dab=True, visualize=True)
    G.randomize(model, 51)
    with torch.no_grad():
        for ce in model.class_embed:
            ce.bias.zero_()
    model.eval()
    m5 = load_npz(os.path.join(OUT, "model_M5_memotr_two_frames.npz"))
    for k, v in model.state_dict().items():
        assert np.array_equal(v.numpy(), m5["w::" + k]), f"weights differ from fixture M5: {k}"
    frames = [torch.from_numpy(m5[f"frame{i}"].copy()) for i in range(2)]
    thresh = float(m5["score_thresh"])
    tracker = RuntimeTracker(det_score_thresh=thresh, track_score_thresh=thresh, miss_tolerance=30, use_dab=True)
    tracks = [TrackInstances(hidden_dim=64, num_classes=1, use_dab=True)]
    arrs = {}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            with torch.no_grad():
                for i, fr in enumerate(frames):
                    res = model(frame=tensor_list_to_nested_tensor([fr]), tracks=tracks)
                    np.testing.assert_allclose(res["pred_bboxes"].numpy(), m5[f"f{i}_pred_bboxes"], rtol=0, atol=0)
                    dec = os.path.join(tmp, "outputs", "visualize_tmp", "decoder")
                    for lid in range(cfg["NUM_DEC_LAYERS"]):
                        for name in ("sampling_locations", "detection_ref_pts", "track_ref_pts"):
                            t = torch.load(os.path.join(dec, f"{name}_layer_{lid}.tensor"))
                            arrs[f"f{i}_{name}_layer_{lid}"] = t.numpy()
                    prev, new = tracker.update(model_outputs=res, tracks=tracks)
                    tracks = model.postprocess_single_frame(prev, new, None)
        finally:
            os.chdir(cwd)
    assert arrs["f1_sampling_locations_layer_1"].shape[0] > 20, "frame 2 carries no tracks"
    save_npz(os.path.join(OUT, "attention_tap.npz"), **arrs)
    for k, v in arrs.items():
        print(k, v.shape)


if __name__ == "__main__":
    main()
