"""hipGraph capture of the query-independent half of a frame: backbone -> feature projections -> encoder, forward AND
backward, one graph pair per (call slot, batch shape, image geometry, precision).

Why (round 3): with the decoder loop in graphs the fp32 step is GPU-bound, but the bf16 extension (BASELINE config 5)
is not -- its kernels take ~100 ms per step while autocast's casts push the launch count to ~10 k and the host needs
~200 ms to issue them.  The encode half of a clip is ONE batched call on a fixed geometry (``engine.encode_chunks``),
~2-5 k launches forward + backward: captured, it costs the host two launches.

The capture itself follows models/graph_capture.py (one flat parameter argument, thread-local error mode) and
models/graph_cache.py (eager after a failed capture unless MEMOTR_REQUIRE_GRAPHS=1, no captures while geometries never
recur).  Under autocast it runs with the cast cache off (a cached cast would be a dangling pointer on replay).

What is captured is ``MeMOTR.encode_frame`` itself; what depends on the masks alone (flattened masks, valid ratios,
pyramid tensors) comes back from the warm-up call as constants, the graph's only output is ``memory``.
"""
from __future__ import annotations

import os
from typing import NamedTuple
import torch

from ..utils.nested_tensor import NestedTensor
from .graph_cache import GraphCache
from .graph_capture import CapturedPair, FlatParameters, capture_pair, encode_key_parts, geometry_pins

MAX_GRAPHS = 6           # each holds the activations of a whole batched encode


def enabled() -> bool:
    """MEMOTR_ENCODE_GRAPHS: "1" on, "0" off, default "auto" = under autocast only (the fp32 step is GPU-bound: the
    capture would buy idle gaps at the price of a second copy of the encode activations)."""
    v = os.environ.get("MEMOTR_ENCODE_GRAPHS", "auto")
    if v == "auto":
        return torch.is_autocast_enabled()
    return v != "0"


class EncodeEntry(NamedTuple):
    pair: CapturedPair           # fn(images, flat parameters) -> memory
    constants: dict              # what ``encode_frame`` returns besides ``memory``: it depends on the masks alone
    state: dict                  # {"busy": the slot's activations still wait for their backward}
    pins: list                   # what the captured kernels read through a baked pointer outside the graph's pool


class EncodeGraphs(GraphCache):
    """Cache of captured encode calls, owned by a ``MeMOTR``."""

    def __init__(self, core):
        super().__init__("encode", MAX_GRAPHS)
        self.core = core

    # ------------------------------------------------------------------ eligibility
    def usable(self, frame: NestedTensor) -> bool:
        c = self.core
        return (enabled() and os.environ.get("MEMOTR_DECODER_GRAPHS", "1") != "0" and not self.failed
                and frame is not None and frame.tensors.is_cuda and frame.masks is not None
                and getattr(frame, "sizes", None) is not None and torch.is_grad_enabled() and c.training
                and not c.use_checkpoint)

    def _names(self):
        """Parameters the encode half reads: backbone, projections, encoder, level embedding."""
        pre = ("backbone.", "feature_projs.", "transformer.encoder.", "transformer.level_embed")
        return [(n, p) for n, p in self.core.named_parameters() if n.startswith(pre)]

    # ------------------------------------------------------------------ one call
    def run(self, frame: NestedTensor, slot: int):
        """``core.encode_frame(frame)`` through the graph of call slot ``slot`` (the index of the encode call inside
        its clip: a graphed callable owns its activations until its backward has run); None -> caller runs eager."""
        amp = (torch.is_autocast_enabled(), str(torch.get_autocast_dtype("cuda")) if torch.is_autocast_enabled() else "")
        key = (slot, tuple(frame.tensors.shape), frame.sizes, amp) + encode_key_parts(self, self.core)
        entry = self.lookup(key, lambda: self._capture(frame, amp))
        if entry is None:
            return None
        if entry.state["busy"]:
            # this slot's activations are still waiting for their backward (a second encode call with the same slot
            # inside one clip): a replay would overwrite them -- this call runs eagerly
            self.eager += 1
            return None
        self.replays += 1
        memory = entry.pair.fn(frame.tensors, entry.pair.params.flat())       # (a flat tensor per call: no clip key)
        entry.state["busy"] = True

        def _released(grad, state=entry.state):
            state["busy"] = False        # the slot's backward is being queued: stream order protects the replay
            return grad

        memory.register_hook(_released)
        return dict(entry.constants, memory=memory)

    def _capture(self, frame: NestedTensor, amp):
        core = self.core
        # (of the whole model's parameters those of the encode half, in its order: no pairing, no look for shared modules)
        params = FlatParameters(core, self._names(), False)
        masks, geometry = frame.masks, frame.sizes
        amp_on, amp_dtype = amp[0], torch.get_autocast_dtype("cuda") if amp[0] else None
        constants = {}

        def run(images, flat):
            sub = params.substitution(flat)
            nested = NestedTensor(images, masks, geometry)
            # the ambient context does not reach a replay: the graph carries its own
            with (torch.autocast("cuda", dtype=amp_dtype, cache_enabled=False) if amp_on
                  else torch.autocast("cuda", enabled=False)):
                enc = torch.func.functional_call(core, sub, (), {"frame": nested, "stage": "encode_eager"})
            if not constants:
                constants.update({k: v for k, v in enc.items() if k != "memory"})
            return enc["memory"]

        # (make_graphed_callables refuses an ambient autocast with its cast cache on; `run` opens its own)
        with torch.autocast("cuda", enabled=False):
            pair = capture_pair(self, params, run, (frame.tensors.detach().clone(),), check_shared=False)
        # `constants` were taken from the FIRST (eager, warm-up) call: the geometry caches' own tensors -- ordinary
        # allocations that carry the host tag of the pyramid, not memory of the graph's pool.  Pinned besides them: the
        # capture's masks (`run` closes over them; the callable torch returns does not keep `run` alive, and the engine
        # builds a new NestedTensor every step -- found the hard way: replay 1 read a recycled mask)
        return pair and EncodeEntry(pair, dict(constants), {"busy": False}, [run, frame.masks] + geometry_pins(core))
