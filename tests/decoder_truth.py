"""Test infrastructure: the decoder loop (models/deformable_decoder.py, models/decoder_graphs.py) and the query updater
(models/query_updater.py, models/updater_graphs.py) against float64 truth at the head size the kernels are written for
(C = 256, 8 heads, D = 32).  Shared by tests/test_decoder_truth_cpu.py and tests/test_decoder_truth_gpu.py.

Truth is the module's own eager code: ``copy.deepcopy(module).cpu().double()`` with the deformable-attention operator
swapped for the oracle's torch statement (``truth_operator``).  It runs on the fp32 inputs cast up, so it is the exact
function of the bits every fp32 path saw.

The rule (``check``).  Per tensor, error = max |got - truth| against scale = max |truth|.  A path passes when its error is
at most ``clip_truth.measured_bound(reference error, scale)``: 4 x the error the fp32 torch composition of the same module
(MEMOTR_FUSED_CLIP_OPS=0) makes on the same inputs on the same device, plus one fp32 ulp of the scale.  Two paths are
held to each other with the same bound around one of them.  Every comparison prints a ``TRUTH`` line with the three
figures relative to the scale.

The inputs (``SEEDS``).  A float32 decision that falls the other way in float64 -- the sign under a ReLU, the bilinear
cell of a sampling point, ``score > update_threshold`` -- puts every fp32 path 1e-3 .. 1e-2 from truth and inflates the
bound until it hides what these tests are for.  The seeds below were searched so that the float32 CPU run and the
float64 CPU run make the same decisions, every one (``decoder_decisions`` / ``updater_decisions``; the CPU test asserts
zero disagreements for every case the GPU test uses), and so that no decision of the float64 run sits closer to its
edge than a device's float32 round-off could carry it (``RELU_MARGIN``, ``CELL_MARGIN``).  ``REF_ERROR_CAP`` is the sanity cap of the GPU test on the
reference's own error: above it a decision fell the other way on the device and the case wants another seed, never a
wider bound.
"""
import contextlib
import copy
from typing import NamedTuple

import torch
import torch.nn as nn

from clip_truth import max_err, measured_bound, out_scale
from model_helpers import OracleMSDeformAttnFunction, patch_operator

C, N_HEADS, N_LEVELS, N_POINTS = 256, 8, 4, 4
SHAPES = [(9, 13), (5, 7), (3, 4), (2, 2)]
S = sum(h * w for h, w in SHAPES)
B = 2
N_LAYERS = 3
ND = 20                                   # detect queries: not a multiple of the 16 rows of an attention workgroup
TRACKS = (0, 1, 7, 13)                    # 13: 33 rows, one past the bucket of 32 -- the captured form pads to 64
ALT_TRACKS = {0: 3, 1: 5, 7: 11, 13: 17}  # the live count of the second replay: another one inside the same bucket
WIDE_FFN = 768                            # clip_ops.linear_fwd_usable / linear_bwd_usable: out > 512 (linear1, both ways) and
#                                           in > 256 (linear2 forward) go to the library GEMMs; 64 stays in the kernels
REF_ERROR_CAP = 1e-4
# How far every decision of the float64 run stays from its edge: a device sums in another order than the CPU and lands a few
# 1e-7 of the operand scale (pre-activations of order 1, pixel coordinates up to 13) from the CPU's float32 value, so a
# pre-activation or a coordinate closer than this to 0 / to a whole pixel could still fall the other way there.
RELU_MARGIN, CELL_MARGIN = 3e-6, 3e-6
STACKS = ("outs", "refs", "layer_inputs", "boxes")


# ------------------------------------------------------------------------------------------------ decoder cases
class Case(NamedTuple):
    use_dab: bool
    n_track: int
    merge: int                            # merge_det_track_layer
    extra_track_attn: bool = False
    d_ffn: int = 64

    @property
    def name(self):
        return (f"{'dab' if self.use_dab else 'plain'}-t{self.n_track}-m{self.merge}"
                + ("-xta" if self.extra_track_attn else "") + (f"-ffn{self.d_ffn}" if self.d_ffn != 64 else ""))


GRAPH_CASES = tuple(Case(dab, nt, m) for dab in (True, False) for nt in TRACKS for m in (0, 1)) \
    + (Case(True, 7, 1, d_ffn=WIDE_FFN), Case(False, 13, 0, d_ffn=WIDE_FFN))
EAGER_ONLY_CASES = (Case(False, 7, 1, extra_track_attn=True), Case(True, 13, 0, extra_track_attn=True))
DECODER_CASES = GRAPH_CASES + EAGER_ONLY_CASES

# (first inputs, inputs of the second replay) per case: the first seeds of 1, 3, 5, ... and 2, 4, 6, ... at which no decision
# of the float32 CPU run falls the other way and every decision keeps its margin (of 100,000 to 340,000 decisions per
# run one or two typically sit inside the margins, so most cases moved on from (1, 2))
SEEDS = {"dab-t0-m0": (1, 4), "dab-t0-m1": (1, 8), "dab-t1-m0": (1, 12), "dab-t1-m1": (7, 2), "dab-t7-m0": (7, 4),
         "dab-t7-m1": (5, 4), "dab-t13-m0": (7, 2), "dab-t13-m1": (5, 4), "plain-t0-m0": (3, 6), "plain-t0-m1": (3, 2),
         "plain-t1-m0": (1, 6), "plain-t1-m1": (5, 6), "plain-t7-m0": (1, 4), "plain-t7-m1": (7, 2),
         "plain-t13-m0": (1, 6), "plain-t13-m1": (5, 2), "dab-t7-m1-ffn768": (5, 28), "plain-t13-m0-ffn768": (1, 30),
         "dab-t13-m0-xta": (3, 6)}


def case_seeds(case):
    return SEEDS.get(case.name, (1, 2))


def _perturb(module, seed):
    """Layers that differ, non-degenerate offsets / attention logits, every bias and gain in play (as
    tests/test_encoder_layer_node_gpu.py sets them)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith("sampling_offsets.weight"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
            elif name.endswith("attention_weights.weight"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
            elif p.dim() == 1 and "sampling_offsets" not in name:
                p.add_(torch.randn(p.shape, generator=g) * 0.1)
            elif p.dim() == 2:
                p.add_(torch.randn(p.shape, generator=g) * 0.01)


def build_decoder(case: Case):
    """The decoder of ``case`` on the CPU in float32, training mode, ``bbox_embed`` with three different heads."""
    from memotr_amd.models.deformable_decoder import DeformableDecoder, DeformableDecoderLayer
    from memotr_amd.models.mlp import MLP
    torch.manual_seed(0)
    layer = DeformableDecoderLayer(d_model=C, d_ffn=case.d_ffn, dropout=0.0, activation="ReLU", n_levels=N_LEVELS,
                                   n_heads=N_HEADS, n_points=N_POINTS, extra_track_attn=case.extra_track_attn,
                                   n_det_queries=ND)
    dec = DeformableDecoder(layer, N_LAYERS, return_intermediate=True, merge_det_track_layer=case.merge,
                            n_det_queries=ND, d_model=C, use_dab=case.use_dab)
    dec.bbox_embed = nn.ModuleList(MLP(C, C, 4, 3) for _ in range(N_LAYERS))
    _perturb(dec, 7)
    return dec.train()


def masked_track_slots(n_track):
    """The track slots of batch 1 that are masked: one in the middle and one at the end (none below three tracks)."""
    return (n_track // 2, n_track - 1) if n_track >= 3 else ()


def decoder_inputs(case: Case, which: int = 0):
    """CPU float32 inputs of ``case``; ``which`` = 1: those of the second replay (other values, another live count)."""
    from memotr_amd.models.deformable_transformer import DeformableTransformer
    nt = case.n_track if which == 0 else ALT_TRACKS[case.n_track]
    nq = ND + nt
    g = torch.Generator().manual_seed(case_seeds(case)[which])
    masks, ratios = [], []
    for h, w in SHAPES:          # a padded border in batch 1: the last row and the last one or two columns
        m = torch.zeros(B, h, w, dtype=torch.bool)
        m[1, h - 1:, :] = True
        m[1, :, max(w - 2, 1):] = True
        masks.append(m.flatten(1))
        ratios.append(DeformableTransformer.get_valid_ratio(m))
    start = [0]
    for h, w in SHAPES[:-1]:
        start.append(start[-1] + h * w)
    query_mask = torch.zeros(B, nq, dtype=torch.bool)
    for slot in masked_track_slots(nt):
        query_mask[1, ND + slot] = True
    live = (~query_mask)[None, :, :, None].float()          # the loss looks at no masked row
    ref = torch.cat((torch.rand(B, nq, 2, generator=g) * 0.6 + 0.2, torch.rand(B, nq, 2, generator=g) * 0.3 + 0.1), -1)
    return dict(tgt=torch.randn(B, nq, C, generator=g), ref=ref, src=torch.randn(B, S, C, generator=g),
                query_pos=torch.randn(B, nq, C, generator=g) * 0.5, query_mask=query_mask,
                src_mask=torch.cat(masks, 1), valid_ratios=torch.stack(ratios, 1),
                w_outs=torch.randn(N_LAYERS, B, nq, C, generator=g) * live,
                w_boxes=torch.randn(N_LAYERS, B, nq, 4, generator=g) * live,
                level_start_index=torch.tensor(start, dtype=torch.int64))


def padded_like_the_capture(x, n_pad, open_slot=None):
    """``x`` with ``n_pad`` masked slots behind the track queries, as ``DeformableDecoder._forward_graphed`` pads them
    (zeros, anchors of 0.5, masked as keys).  ``open_slot``: that padded slot is NOT masked (a planted defect)."""
    y = dict(x)
    for k, fill in (("tgt", 0.0), ("ref", 0.5), ("query_pos", 0.0)):
        y[k] = torch.cat((x[k], x[k].new_full((B, n_pad, x[k].shape[-1]), fill)), 1)
    y["query_mask"] = torch.cat((x["query_mask"], torch.ones(B, n_pad, dtype=torch.bool)), 1)
    if open_slot is not None:
        y["query_mask"][:, x["tgt"].shape[1] + open_slot] = False
    for k in ("w_outs", "w_boxes"):
        y[k] = torch.cat((x[k], x[k].new_zeros(N_LAYERS, B, n_pad, x[k].shape[-1])), 2)
    return y


def run_decoder(dec, x, device="cpu", dtype=torch.float32, grad=True, frame_slot=None, clip_key=None, keep=None):
    """One call of ``dec`` on ``x`` and the backward of sum(outs * w_outs) + sum(boxes * w_boxes).  Returns {name:
    tensor}: ``out::<stack>`` the four returned stacks, ``grad::tgt|src|query_pos`` and ``grad::p::<parameter>`` (none
    with ``grad=False``).  ``keep``: only the first ``keep`` query rows are reported (the rest was padding)."""
    from memotr_amd.MultiScaleDeformableAttention import tag_host_shapes
    from memotr_amd.modules.ms_deform_attn import tag_masked_rows
    dev = torch.device(device)

    def to(t):
        return t.to(device=dev, dtype=dtype)

    tgt, src = to(x["tgt"]).clone().requires_grad_(grad), to(x["src"]).clone().requires_grad_(grad)
    query_pos = None if dec.use_dab else to(x["query_pos"]).clone().requires_grad_(grad)
    shapes = torch.tensor(SHAPES, dtype=torch.int64, device=dev)
    src_mask, query_mask = x["src_mask"].to(dev).clone(), x["query_mask"].to(dev).clone()
    if dev.type == "cuda":       # what DeformableTransformer.encode attaches
        tag_host_shapes(shapes, SHAPES)
        tag_masked_rows(src_mask)
    query_mask._no_padding = not bool(x["query_mask"].any())       # (MeMOTR.get_query_mask)
    dec.zero_grad(set_to_none=True)
    with torch.set_grad_enabled(grad):
        res = dec(tgt, to(x["ref"]), src, shapes, x["level_start_index"].to(dev), to(x["valid_ratios"]), query_pos,
                  query_mask, src_mask, frame_slot=frame_slot, clip_key=clip_key)
    rows = slice(None) if keep is None else slice(0, keep)
    got = {"out::" + k: t.detach()[:, :, rows].clone() for k, t in zip(STACKS, res)}
    if not grad:
        return got
    ((res[0] * to(x["w_outs"])).sum() + (res[3] * to(x["w_boxes"])).sum()).backward()
    got["grad::tgt"], got["grad::src"] = tgt.grad[:, rows].clone(), src.grad.clone()
    if query_pos is not None:
        got["grad::query_pos"] = query_pos.grad[:, rows].clone()
    if keep is not None:
        got["grad::tgt(padding)"] = tgt.grad[:, keep:].clone()
    for n, p in dec.named_parameters():
        got["grad::p::" + n] = torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()
    return got


# ------------------------------------------------------------------------------------------------ truth and decisions
class _RecordingOperator:
    """The oracle's statement of the operator that also notes the bilinear cell of every sampling point."""

    def __init__(self, cells, margins=None):
        self.cells, self.margins = cells, margins

    def apply(self, value, shapes, level_start, loc, attn, im2col_step):
        wh = shapes.flip(-1).to(loc.dtype)                                     # (L, 2) as (W, H)
        pixel = loc.detach() * wh[None, None, None, :, None, :] - 0.5
        self.cells.append(torch.floor(pixel).long())
        if self.margins is not None:
            self.margins.append(float((pixel - pixel.round()).abs().min()))
        return OracleMSDeformAttnFunction.apply(value, shapes, level_start, loc, attn, im2col_step)


def truth_operator(monkeypatch, cells=None, margins=None):
    """Swap the HIP operator for the oracle's torch statement (``model_helpers.patch_operator``); ``cells`` (a list)
    receives floor(pixel coordinates) of every call, ``margins`` the smallest distance of a coordinate from a whole pixel."""
    patch_operator(monkeypatch)
    if cells is not None:
        import memotr_amd.modules.ms_deform_attn as mod
        monkeypatch.setattr(mod, "MSDeformAttnFunction", _RecordingOperator(cells, margins))


@contextlib.contextmanager
def recorded_relus(module, masks, margins=None):
    """Every ReLU decision of a CPU run of ``module`` into ``masks``: ``nn.ReLU`` children through forward hooks (on their
    input: they work in place), and the ReLU that ``row_linear(..., relu=True)`` takes in its epilogue (the decoder FFN,
    the MLPs) through a wrapper.  ``margins`` receives the smallest |pre-activation| of every site."""
    import memotr_amd.models.deformable_decoder as dd
    import memotr_amd.models.mlp as mlp
    originals = [(m, m.row_linear) for m in (dd, mlp)]

    def wrapped(x, weight, bias=None, relu=False):
        y = originals[0][1](x, weight, bias, False)
        if not relu:
            return y
        note(y)
        return torch.relu(y)

    def note(y):
        masks.append((y > 0).detach())
        if margins is not None:
            margins.append(float(y.detach().abs().min()))

    hooks = [m.register_forward_pre_hook(lambda _m, inputs: note(inputs[0]))
             for m in module.modules() if isinstance(m, nn.ReLU)]
    for m, _ in originals:
        m.row_linear = wrapped
    try:
        yield
    finally:
        for m, orig in originals:
            m.row_linear = orig
        for h in hooks:
            h.remove()


def disagreements(a, b) -> int:
    assert len(a) == len(b) and len(a) > 0
    return sum(int((s != t).sum()) for s, t in zip(a, b))


def decoder_decisions(monkeypatch, case, which=0):
    """(ReLU disagreements, bilinear-cell disagreements, decisions taken, (ReLU margin, cell margin) of the float64 run)
    between the float32 and the float64 CPU run of ``case``; also returns the two results {name: tensor}."""
    dec, x = build_decoder(case), decoder_inputs(case, which)
    runs = []
    for module, dtype in ((dec, torch.float32), (copy.deepcopy(dec).double(), torch.float64)):
        relus, cells, m_relu, m_cell = [], [], [], []
        with monkeypatch.context() as mp, recorded_relus(module, relus, m_relu):
            truth_operator(mp, cells, m_cell)
            got = run_decoder(module, x, "cpu", dtype)
        runs.append((relus, cells, got, (min(m_relu), min(m_cell))))
    (r32, c32, got32, _), (r64, c64, got64, margins) = runs
    taken = sum(t.numel() for t in r64) + sum(t.numel() for t in c64)
    return disagreements(r32, r64), disagreements(c32, c64), taken, margins, got32, got64


def decoder_truth(monkeypatch, dec, x):
    """Float64 truth of ``dec`` on ``x``: the module's own eager code on the CPU, the oracle as the operator."""
    with monkeypatch.context() as mp:
        truth_operator(mp)
        return run_decoder(copy.deepcopy(dec).cpu().double(), x, "cpu", torch.float64)


# ------------------------------------------------------------------------------------------------ the rule
class Row(NamedTuple):
    tensor: str
    scale: float
    ref: float            # error of the reference path (absolute)
    err: float            # error of the path under test (absolute)
    bound: float
    rel: float = 1.0      # what the printed figures are divided by: the scale, or 1 for a tensor without one


def errors(got, center):
    assert got.keys() == center.keys(), sorted(set(got) ^ set(center))
    return {k: max_err(got[k], center[k]) for k in center}


def zero_floor(truth) -> float:
    """Below this a float64 truth tensor is the round-off of an exact zero (the gradient into the query and key of an
    attention over ONE key, a softmax of one term): 1e-12 of the run's largest tensor, four decades above what float64
    sums of a few hundred terms leave (1e-16) and six below anything a float32 path resolves.  Such a tensor has no scale
    to divide by: its figures are printed as they are and the reference is capped against the largest scale."""
    return 1e-12 * max(out_scale(t) for t in truth.values())


def check(case_name, path, got, center, ref_err, truth, tensors=None):
    """Hold ``got`` to ``center`` (truth itself, or another path) tensor by tensor: error <= measured_bound(error of the
    reference path against truth, scale of truth).  Prints one TRUTH line per tensor; returns (rows, violations)."""
    rows, floor = [], zero_floor(truth)
    for k in (center.keys() if tensors is None else tensors):
        scale = out_scale(truth[k])
        rel = scale if scale > floor else 1.0
        row = Row(k, scale, ref_err[k], max_err(got[k], center[k]), measured_bound(ref_err[k], scale), rel)
        rows.append(row)
        print(f"TRUTH {case_name} {path} {k} ref={row.ref / rel:.3e} kernel={row.err / rel:.3e} "
              f"bound={row.bound / rel:.3e}")
    return rows, [r for r in rows if not r.err <= r.bound]


def worst(rows):
    """The row closest to (or furthest past) its bound, as text: for the summary line of a path."""
    r = max(rows, key=lambda r: (r.err / r.bound) if r.bound > 0 else (0.0 if r.err == 0 else float("inf")))
    return f"{r.tensor} ref={r.ref / r.rel:.3e} kernel={r.err / r.rel:.3e} bound={r.bound / r.rel:.3e}"


def reference_inside_cap(case_name, ref_err, truth):
    """The reference path's own error, per tensor, relative to scale, against REF_ERROR_CAP."""
    floor = zero_floor(truth)
    rel = {k: e / (out_scale(truth[k]) if out_scale(truth[k]) > floor else floor * 1e12) for k, e in ref_err.items()}
    bad = {k: r for k, r in rel.items() if not r < REF_ERROR_CAP}
    assert not bad, (f"{case_name}: the fp32 composition is {bad} of scale from truth -- a decision fell the other way on "
                     "the device: reseed the case (decoder_truth.SEEDS), do not widen the bound")


# ------------------------------------------------------------------------------------------------ query updater
UPDATER_ROWS = (1, 5, 17, 33)                       # buckets of 16: 16, 16, 32, 48
UPDATER_ALT_ROWS = {1: 3, 5: 9, 17: 20, 33: 40}     # the live count of the second replay, same bucket
UPDATER_FFN = 64
UPDATE_THRESHOLD = 0.5
SCORE_MARGIN = 1e-3
UPDATER_OUT = ("ref_pts", "long_memory", "last_output", "query_embed")
UPDATER_DIFF = (3, 4, 5, 6)                         # output_embed, long_memory, last_output, query_embed
BANK_STREAMS, BANK_CAP = 3, 16


def build_updater(use_dab: bool):
    from memotr_amd.models.query_updater import QueryUpdater
    torch.manual_seed(0)
    qu = QueryUpdater(hidden_dim=C, ffn_dim=UPDATER_FFN, tp_drop_ratio=0.0, fp_insert_ratio=0.0, dropout=0.0,
                      use_checkpoint=False, use_dab=use_dab, update_threshold=UPDATE_THRESHOLD, long_memory_lambda=0.01)
    _perturb(qu, 11)
    return qu.train()


UPDATER_SEEDS = {(20, True): 121, ("bank", 0, True): 503}      # (the default seeds leave a pre-activation inside RELU_MARGIN)


def updater_fields(n, use_dab, seed=None):
    """The seven track fields of ``n`` rows (``QueryUpdater.FIELDS``) and the weights of the four outputs, CPU float32.
    Scores sit at least 0.07 from the threshold, about two thirds of them above it, row 0 always."""
    seed = UPDATER_SEEDS.get((n, use_dab), 100 + n) if seed is None else seed
    g = torch.Generator().manual_seed(seed)
    sign = torch.where(torch.rand(n, 1, generator=g) < 0.65, 1.0, -1.0)
    sign[0] = 1.0
    logits = sign * (0.3 + 2.0 * torch.rand(n, 1, generator=g))
    boxes = torch.rand(n, 4, generator=g) * 0.9 + 0.05
    widths = (4, C, C, C, C if use_dab else 2 * C)
    rest = [torch.randn(n, w, generator=g) for w in widths]
    weights = [torch.randn(n, w, generator=g) for w in (4, C, C, widths[-1])]
    return [logits, boxes] + rest, weights


def run_updater(qu, fields, weights, device="cpu", dtype=torch.float32, graph_slot=None, n_streams=1, key_mask=None):
    """``update_fields`` (``graph_slot``: through ``UpdaterGraphs.run``) and the backward of the weighted sum of its four
    outputs: {``out::<field>``, ``grad::<input field>``, ``grad::p::<parameter>``}."""
    dev = torch.device(device)
    f = [t.to(device=dev, dtype=dtype).clone() for t in fields]
    for i in UPDATER_DIFF:
        f[i].requires_grad_(True)
    qu.zero_grad(set_to_none=True)
    if graph_slot is None:
        out = qu.update_fields(*f, key_mask=None if key_mask is None else key_mask.to(dev), n_streams=n_streams)
    else:
        assert qu.graphs().usable(f)
        out = qu.graphs().run(graph_slot, f, clip_key=object())
        assert out is not None
    got = {"out::" + k: t.detach().clone() for k, t in zip(UPDATER_OUT, out)}
    sum((o * w.to(device=dev, dtype=dtype)).sum() for o, w in zip(out, weights)).backward()
    for i in UPDATER_DIFF:
        got["grad::" + qu.FIELDS[i]] = f[i].grad.clone()
    for n, p in qu.named_parameters():
        got["grad::p::" + n] = torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()
    return got


def updater_truth(qu, fields, weights):
    return run_updater(copy.deepcopy(qu).cpu().double(), fields, weights, "cpu", torch.float64)


def score_margin(qu, logits):
    """Smallest distance of a score from the update threshold, in float64."""
    return float((logits.double().sigmoid().max(1).values - qu.update_threshold).abs().min())


def updater_decisions(qu, fields, weights):
    """(ReLU disagreements, ``is_pos`` disagreements, decisions taken, ReLU margin of the float64 run) between the float32
    and the float64 CPU run."""
    runs = []
    for module, dtype in ((qu, torch.float32), (copy.deepcopy(qu).double(), torch.float64)):
        relus, margins = [], []
        with recorded_relus(module, relus, margins):
            run_updater(module, fields, weights, "cpu", dtype)
        runs.append((relus, fields[0].to(dtype).sigmoid().max(1).values > module.update_threshold, min(margins)))
    (r32, p32, _), (r64, p64, margin) = runs
    return disagreements(r32, r64), int((p32 != p64).sum()), sum(t.numel() for t in r64) + p64.numel(), margin


def bank_live_slots():
    """(BANK_STREAMS, BANK_CAP) bool: stream 0 full, stream 1 with holes in alternating slots, stream 2 without a track."""
    live = torch.zeros(BANK_STREAMS, BANK_CAP, dtype=torch.bool)
    live[0] = True
    live[1, 0::2] = True
    return live


def build_bank(use_dab, device="cpu"):
    """A ``TrackBank`` whose live slots hold the rows of ``updater_fields`` (seed per stream) and whose free slots hold
    zeros; returns (bank, per stream: (fields of the live rows, slots))."""
    from memotr_amd.models.query_updater import QueryUpdater
    from memotr_amd.models.track_bank import TrackBank
    bank = TrackBank(BANK_STREAMS, BANK_CAP, num_classes=1, hidden_dim=C, use_dab=use_dab, device=device)
    live, per_stream = bank_live_slots(), []
    for b in range(BANK_STREAMS):
        slots = live[b].nonzero().squeeze(1)
        fields = None
        if slots.numel():
            fields, _ = updater_fields(int(slots.numel()), use_dab, seed=UPDATER_SEEDS.get(("bank", b, use_dab), 500 + b))
            for name, t in zip(QueryUpdater.FIELDS, fields):
                getattr(bank, name)[b, slots.to(device)] = t.to(device)
            bank.ids[b, slots.to(device)] = torch.arange(slots.numel(), device=device)
        per_stream.append((fields, slots))
    return bank, per_stream


def bank_fields(bank):
    """The four fields ``update_bank`` rewrites, on the CPU: {``out::<field>``: (B, cap, width)}."""
    return {"out::" + k: getattr(bank, k).detach().cpu().clone() for k in UPDATER_OUT}


def bank_truth(qu, per_stream, use_dab):
    """Float64 truth of ``update_bank``: ``update_fields`` per stream on that stream's live rows alone, scattered into
    a zero bank."""
    q64 = copy.deepcopy(qu).cpu().double()
    widths = dict(zip(UPDATER_OUT, (4, C, C, C if use_dab else 2 * C)))
    truth = {"out::" + k: torch.zeros(BANK_STREAMS, BANK_CAP, w, dtype=torch.float64) for k, w in widths.items()}
    with torch.no_grad():
        for b, (fields, slots) in enumerate(per_stream):
            if fields is not None:
                for k, t in zip(UPDATER_OUT, q64.update_fields(*(t.double() for t in fields))):
                    truth["out::" + k][b, slots] = t
    return truth
