"""What the hipGraph captures of the model (models/{decoder,updater,encode,infer}_graphs.py) share: the capture context
(thread-local error mode, node census, memset-node check), the flat parameter argument and the capture of a forward /
backward pair, the encode captures' pins and key parts.  (Lookup / eviction policy: graph_cache.py, which needs no torch.)"""
from __future__ import annotations

import contextlib
import os
from typing import Callable, NamedTuple

import torch
import torch.nn as nn

from ..functions import clip_ops
from .graph_cache import selector_signature


# MEMOTR_GRAPH_CENSUS=1: every capture appends {node type: count} of its hipGraph here (tools/graph_census.py, the GPU
# tests).  What it is for: on ROCm 7.2 a MEMSET node is not ordered behind the kernels before it when a graph is
# replayed with the runtime's AQL-packet capture on (the default) -- tools/graph_memset_probe.py shows it in ten
# lines, DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 restores the order.  torch's multi-block reductions zero their semaphores
# with such a node (bias gradients of captured linears came back as garbage from the second replay on), so nothing
# inside the captured regions may reduce through them: the census is how the tests hold the graphs to ZERO memset
# nodes, whatever the runtime flag says.
CENSUS = [] if os.environ.get("MEMOTR_GRAPH_CENSUS", "0") == "1" else None
_NODE_TYPES = {0: "kernel", 1: "memcpy", 2: "memset", 3: "host", 4: "graph", 5: "empty", 6: "wait_event",
               7: "event_record"}
_MEMSET_SAFE = None              # memset_nodes_replay_safe(), once per process
_PATCH_LOCK = __import__("threading").RLock()


@contextlib.contextmanager
def _thread_local_capture(census=None):
    """``make_graphed_callables`` captures in the "global" error mode: ANY thread that touches the runtime while a
    capture is open (the RCCL watchdog polling its events under DistributedDataParallel, a data-loader thread pinning
    memory) invalidates it.  The decoder capture only needs the capturing threads themselves to behave, so the graph
    context is switched to "thread_local" for its duration.  ``census`` (a list, default: the module's ``CENSUS``)
    receives {node type: count} of every graph captured inside."""
    CENSUS = census if census is not None else globals()["CENSUS"]
    # The patch below replaces process-global names: one capture at a time (re-entrant for the capturing thread), and
    # the originals are read under the lock so that a nested use restores what it found.
    with _PATCH_LOCK:
        orig = torch.cuda.graph
        orig_graph_cls = torch.cuda.CUDAGraph

        class _Graph(orig):
            def __init__(self, *args, **kwargs):
                kwargs.setdefault("capture_error_mode", "thread_local")
                super().__init__(*args, **kwargs)

            def __exit__(self, *exc):
                out = super().__exit__(*exc)
                if exc[0] is None and CENSUS is not None:
                    CENSUS.append(graph_node_census(self.cuda_graph))
                return out

        if CENSUS is not None:       # (the raw hipGraph_t only survives capture_end when asked for)
            class _KeepGraph(orig_graph_cls):      # a subclass: isinstance(x, torch.cuda.CUDAGraph) keeps working
                def __new__(cls, *a, **k):
                    return orig_graph_cls.__new__(cls, keep_graph=True)

                def __init__(self, *a, **k):       # (the binding constructs in __init__, from the CALL's arguments)
                    super().__init__(True)

            torch.cuda.CUDAGraph = _KeepGraph
        torch.cuda.graph = _Graph
        # No cyclic garbage collection while a capture is open: a collection that happens to run then may finalise a
        # hipGraph of an EARLIER capture (a refused one, an evicted cache entry still held by a reference cycle or a
        # traceback), and releasing its memory pool under an open capture aborts the process (seen in round 6: the
        # query updater's capture right after a refused decoder capture).  Garbage is collected before, outside.
        import gc
        gc.collect()
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            yield
        finally:
            if gc_was_on:
                gc.enable()
            torch.cuda.graph = orig
            torch.cuda.CUDAGraph = orig_graph_cls


def memset_nodes_replay_safe() -> bool:
    """Does THIS process's HIP runtime order a memset node behind the kernels before it when a graph is replayed?
    (tools/graph_memset_probe.py in miniature, run once: kernel dirties a buffer | memset | kernel reads it.)  False
    on ROCm 7.2 unless DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 was in the environment when the runtime loaded."""
    global _MEMSET_SAFE
    if _MEMSET_SAFE is None:
        import ctypes
        hip = ctypes.CDLL("libamdhip64.so")
        n = 1 << 16
        dev = torch.device("cuda", torch.cuda.current_device())
        buf, x, out = torch.zeros(n, device=dev), torch.ones(n, device=dev), torch.empty(n, device=dev)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            buf.add_(1.0)
            torch.add(buf, x, out=out)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            buf.add_(1.0)
            rc = hip.hipMemsetAsync(ctypes.c_void_p(buf.data_ptr()), 0, ctypes.c_size_t(n * 4),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            torch.add(buf, x, out=out)
            buf.add_(3.0)
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize()
        _MEMSET_SAFE = rc == 0 and bool((out == x).all())
    return _MEMSET_SAFE


def checked_capture(make):
    """Run ``make()`` (a ``make_graphed_callables`` call) in thread-local capture mode.  When this runtime does not
    order memset nodes on replay, the captured graphs are inspected and a graph that contains one is refused -- a
    library may zero a workspace that way (the bf16 encode backward at 800 x 1333 holds six such nodes), and replaying
    it would corrupt results silently."""
    census = [] if (CENSUS is None and not memset_nodes_replay_safe()) else None
    with _thread_local_capture(census):
        fn = make()
    bad = [c for c in (census or []) if c.get("memset", 0) or "error" in c]
    if bad:
        raise RuntimeError(f"captured graph contains memset nodes {bad} and this HIP runtime does not order them on "
                           "replay: set DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 in the environment before torch is imported")
    return fn


def graph_node_census(cuda_graph) -> dict:
    """{node type: count} of a ``torch.cuda.CUDAGraph`` created with ``keep_graph=True``."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    raw = ctypes.c_void_p(cuda_graph.raw_cuda_graph())
    n = ctypes.c_size_t(0)
    if hip.hipGraphGetNodes(raw, None, ctypes.byref(n)) != 0:
        return {"error": 1}
    nodes = (ctypes.c_void_p * max(n.value, 1))()
    if hip.hipGraphGetNodes(raw, nodes, ctypes.byref(n)) != 0:
        return {"error": 1}
    out = {}
    for i in range(n.value):
        t = ctypes.c_int(-1)
        hip.hipGraphNodeGetType(ctypes.c_void_p(nodes[i]), ctypes.byref(t))
        name = _NODE_TYPES.get(t.value, f"type{t.value}")
        out[name] = out.get(name, 0) + 1
    return out


def paired_query_projections(root: nn.Module, named):
    """Order the parameters of ``root`` for the flat argument of a capture so that, for every deformable-attention module,
    ``sampling_offsets.weight`` is directly followed by ``attention_weights.weight`` and the two biases likewise: the
    stacked (offsets; logits) projection the module feeds its one query GEMM with is then a VIEW of the flat tensor, not a
    concatenation made by every replay (two kernels per layer and frame).
    Returns (names, parameters, groups): ``groups`` = [(member names, member shapes, stacked shape or None), ...] in flat
    order -- the flat tensor is split ONCE, by group; a pair is one piece of that split (``split_parameters``)."""
    from ..modules.ms_deform_attn import MSDeformAttn
    by_name = dict(named)
    pairs = []
    for mod_name, m in root.named_modules():
        if isinstance(m, MSDeformAttn) and os.environ.get("MEMOTR_QPROJ_VIEW", "1") != "0":
            pre = mod_name + "." if mod_name else ""
            keys = [pre + k for k in ("sampling_offsets.weight", "attention_weights.weight", "sampling_offsets.bias",
                                      "attention_weights.bias")]
            if all(k in by_name for k in keys) and by_name[keys[0]].dtype == by_name[keys[1]].dtype \
                    and by_name[keys[0]].shape[1:] == by_name[keys[1]].shape[1:]:
                pairs.append(keys)
    taken = {k for keys in pairs for k in keys}
    groups = [((n,), (tuple(p.shape),), None) for n, p in named if n not in taken]
    for w0, w1, b0, b1 in pairs:
        for a, b in ((w0, w1), (b0, b1)):
            pa, pb = by_name[a], by_name[b]
            groups.append(((a, b), (tuple(pa.shape), tuple(pb.shape)), (pa.shape[0] + pb.shape[0],) + tuple(pa.shape[1:])))
    names = tuple(n for g in groups for n in g[0])
    params = tuple(by_name[n] for n in names)
    return names, params, groups


def split_parameters(flat: torch.Tensor, groups) -> dict:
    """{name: view} of the flat parameter tensor for ``torch.func.functional_call``.  ONE split of ``flat`` (its backward:
    one concatenation); a pair's piece is the module's stacked weight (bias) as it lies, tagged on the
    ``sampling_offsets`` stand-ins for ``MSDeformAttn._fused_query_projection``.  The pair's members are views of the
    PIECE, and the fused module does not read them: nothing but the split stands between the flat tensor and the stack.
    (Round 6 first took the stack as ``flat.narrow(...)``: each narrow's backward is a zero-fill of the WHOLE flat tensor
    -- 46 MB -- a memcpy node and a full-size add: 12 memcpy nodes and 48 kernels per decoder backward graph, +3 ms per
    train step for the 0.06 ms the view saved in the forward; tools/qproj_ab.sh, profiles/r06_qproj_ab.txt.)"""
    def numel(shape):
        n = 1
        for d in shape:
            n *= d
        return n

    pieces = flat.split([sum(numel(sh) for sh in g[1]) for g in groups])
    sub, stacks = {}, {}
    for (names, shapes, stacked), piece in zip(groups, pieces):
        if stacked is None:
            sub[names[0]] = piece.view(shapes[0])
            continue
        off = 0
        for n, sh in zip(names, shapes):
            sub[n] = piece.narrow(0, off, numel(sh)).view(sh)
            off += numel(sh)
        stacks[names[0]] = piece.view(stacked)
    for first in [k for k in stacks if k.endswith("sampling_offsets.weight")]:
        sub[first]._msda_fused_qproj = (stacks[first], stacks[first[:-len("weight")] + "bias"])
    return sub


class FlatParameters:
    """The parameters ``named`` of ``root`` as the ONE flat tensor argument of a capture: names, ``nn.Parameter`` objects
    and the split back into them -- by ``paired_query_projections``, or in the order of ``named`` with one piece per
    parameter (what the pairing gives for a root without ``MSDeformAttn`` modules).  ``shared``: where the per-clip tensor
    of ``flat`` is kept; the captures of one cache (one per frame slot) pass the same dict and read the same tensor."""

    def __init__(self, root: nn.Module, named, pair_query_projections: bool, shared: dict = None):
        self.root = root
        named = list(named)
        if pair_query_projections:
            self.names, self.params, self.groups = paired_query_projections(root, named)
        else:
            self.names, self.params = tuple(n for n, _ in named), tuple(p for _, p in named)
            self.groups = [((n,), (tuple(p.shape),), None) for n, p in named]
        self._shared = {} if shared is None else shared

    def flat(self, clip_key=None):
        """All parameters as ONE tensor, made once per clip (``clip_key``: an object that lives as long as the clip; None:
        a tensor per call) and read by the graphs of all its frames.  A graph returns the gradient of each tensor argument
        in its own buffer and autograd adds the frames up argument by argument: ~170 parameter tensors were 170 copy / add
        kernels per frame outside the graphs (850 per train step, ~5 ms).  With one flat argument the frames' gradients
        meet in four adds, the cat's backward hands views to the parameters once per clip, and DistributedDataParallel's
        hooks still fire once per parameter."""
        params, cache = self.params, self._shared.get("flat")
        if (clip_key is not None and cache is not None and cache[0] is clip_key and len(cache[1]) == len(params)
                and all(a is b for a, b in zip(cache[1], params))):
            return cache[2]
        flat = torch.cat([p.reshape(-1) for p in params])
        if clip_key is not None:
            self._shared["flat"] = (clip_key, params, flat)
        return flat

    def substitution(self, flat: torch.Tensor) -> dict:
        """{name: view of ``flat``} for ``torch.func.functional_call`` on ``root``."""
        return split_parameters(flat, self.groups)

    def restored(self) -> bool:
        """After a capture: does every name still lead to the ``nn.Parameter`` it led to before?"""
        live = dict(self.root.named_parameters())
        return all(isinstance(p, nn.Parameter) and live.get(n) is p for n, p in zip(self.names, self.params))


class CapturedPair(NamedTuple):
    fn: Callable                 # forward and backward graph behind one autograd function: fn(*inputs, flat parameters)
    params: FlatParameters


def capture_pair(cache, params: FlatParameters, run, inputs, check_shared: bool = True):
    """``run(*inputs, flat)`` captured forward AND backward for the ``GraphCache`` ``cache``; None: the capture failed
    (``cache.capture_failed``), or a module of ``root`` is reachable under two names (``cache.failed``, silently: a model
    without box-refinement clones; ``check_shared=False``: only a part of ``root`` is substituted).

    The parameters travel as an ordinary tensor ARGUMENT (``run`` hands ``params.substitution(flat)`` to
    ``torch.func.functional_call``): the captured backward then differentiates with respect to a fresh leaf tensor only.
    Capturing with respect to the live ``nn.Parameter`` objects instead makes autograd reuse their gradient-accumulator
    nodes, which remember the stream they were created on -- any earlier use of a parameter on the default stream (an
    eager step, a kept-alive graph) then drags the legacy stream into the capture and hipStreamEndCapture faults."""
    root = params.root
    if check_shared and len(list(root.named_parameters())) != len(list(root.named_parameters(remove_duplicate=False))):
        cache.failed = True      # functional_call does not restore the parameters of such a module (see DecoderLoop)
        return None
    with torch.no_grad():
        sample = tuple(inputs) + (params.flat().requires_grad_(True),)
    try:
        fn = checked_capture(lambda: torch.cuda.make_graphed_callables(run, sample, num_warmup_iters=2,
                                                                       allow_unused_input=True))
    except Exception as exc:  # noqa: BLE001 -- capture is an optimisation; eager stays valid
        return cache.capture_failed(exc)
    assert params.restored(), f"{cache.what} parameters were replaced by the capture"
    cache.captures += 1
    return CapturedPair(fn, params)


def geometry_pins(core) -> list:
    """What the kernels of a captured encode read through a baked pointer that is NOT in the graph's own pool, besides the
    masks: the tensors the geometry caches handed out during the capture (a cache may evict; the graph may not notice)."""
    tr = core.transformer
    pins = [dict(tr.__dict__.get("_mask_derived", {})), dict(tr.__dict__.get("_pyramids", {}))]
    for m in core.modules():
        for attr in ("_cache", "_folded"):
            v = m.__dict__.get(attr)
            if v is not None:
                pins.append(dict(v) if isinstance(v, dict) else v)
    return pins


def encode_key_parts(owner, core) -> tuple:
    """(kernel configuration, backbone buffer versions, selector signature) for the key of an encode capture: it bakes in
    the folded batch-norm constants (a checkpoint loaded in place must not replay the old ones) and the kernel choice of the
    encoder's self-attention calls (replayed launches keep counting; the signature moves with the levels, msda_select.h)."""
    bufver = sum(b._version for b in core.backbone.buffers())
    return clip_ops.config_key(), bufver, selector_signature(owner, core.transformer.encoder)
