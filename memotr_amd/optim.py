"""``ClipAdamW``: clip_grad_norm_ + AdamW of a whole parameter list as two HIP launches (libopt_ops_hip.so).

What torch does in about twenty launches and three passes over the gradients -- the multi-tensor norms, the in-place
rescale of every ``.grad``, the fused Adam launches -- is one streaming computation: a sum-of-squares pass (4 B per
parameter) and an update pass that applies the clip factor in registers (28 B per parameter).  ``.grad`` stays as the
backward wrote it, nothing is read back to the host, and the result does not depend on the run (no atomics).

The statement (include/opt_ops_hip.h has it with the kernel's layout), per parameter tensor with a gradient g:

    total_norm = sqrt(sum over all g of g^2)                              float64
    coef       = min(1, max_norm / (total_norm + 1e-6)), 1 without clipping    float64 (torch's expression)
    step += 1;  bc1 = 1 - b1^step;  bc2 = 1 - b2^step                     float64
    c, d, w, b, o, s, q, e = float32 of coef, 1 - lr wd, 1 - b1, b2, 1 - b2, lr / bc1, sqrt(bc2), eps
    gs = g c;  m' = m + w (gs - m);  v' = v b + (o gs) gs;  p' = p d - s (m' / (sqrt(v') / q + e))      float32

which is ``torch.optim.AdamW`` (decoupled weight decay, no amsgrad) behind ``clip_grad_norm_(error_if_nonfinite=
False)``.  CUDA parameters take the kernels and nothing else; CPU parameters take the same statement in torch ops, in
the same order (``_step_cpu``), so CPU users and CPU tests get the same optimizer.

State: ``state[p] = {"step", "exp_avg", "exp_avg_sq"}`` as torch's AdamW keeps it; the moments are views into two
packed buffers and ``step`` a 0-dim float32 view into one per-tensor array, so ``state_dict()`` loads into
``torch.optim.AdamW`` and the other way round (``step`` may arrive as a CPU tensor or a number; after
``load_state_dict`` -- or when ``step`` finds other tensors in ``self.state`` than its views -- the state is copied
into the packed buffers again).

On the device the kernels read a table of {p, g, m, v, numel, group} rows.  Only its g column changes -- ``zero_grad()``
drops the gradients and the next backward allocates them again, mostly at the same addresses -- so the table is
uploaded only when a pointer differs from the last upload, from one of two pinned staging buffers whose previous copy
an event guards.  One stream per optimizer: the upload and both launches go on the current stream.
"""
from __future__ import annotations

import math

import numpy as np
import torch

_FLAGS = ("amsgrad", "maximize", "capturable", "differentiable")


def _refuse_flags(group: dict, where: str) -> None:
    for name in _FLAGS:
        if group.get(name, False):
            raise ValueError(f"ClipAdamW does not implement {name}=True ({where})")
    if not group.get("decoupled_weight_decay", True):
        raise ValueError(f"ClipAdamW decays the weights decoupled from the gradient: decoupled_weight_decay=False "
                         f"({where}) is torch.optim.Adam's rule")


class _Plan:
    """Everything ``step`` needs that depends on the parameter list only."""


class ClipAdamW(torch.optim.Optimizer):
    _plan = None

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *,
                 maximize=False, foreach=None, capturable=False, differentiable=False, fused=None):
        if isinstance(lr, torch.Tensor):
            raise ValueError("ClipAdamW takes lr as a number: it travels to the kernel by value")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        _refuse_flags(dict(amsgrad=amsgrad, maximize=maximize, capturable=capturable, differentiable=differentiable),
                      "constructor")
        # the keys of torch.optim.AdamW's defaults: state dicts and schedulers move between the two unchanged
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True)
        super().__init__(params, defaults)

    # ------------------------------------------------------------------------------------------------ the state
    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        _refuse_flags(self.param_groups[-1], "add_param_group")
        self._plan = None                       # adopted again, with the state kept, at the next step

    def load_state_dict(self, state_dict):
        for i, g in enumerate(state_dict["param_groups"]):
            _refuse_flags(g, f"load_state_dict, group {i}")
        super().load_state_dict(state_dict)
        for g in self.param_groups:             # (a checkpoint of an older torch lacks the newer keys)
            for k, v in self.defaults.items():
                g.setdefault(k, v)
        self._adopt()

    def _adopt(self) -> _Plan:
        """Pack the moments and step counts of every parameter (what ``self.state`` holds, zeros otherwise) into
        three buffers, point ``self.state`` at views of them and, on the device, build the kernels' tables."""
        params = [p for g in self.param_groups for p in g["params"]]
        group_of = [gi for gi, g in enumerate(self.param_groups) for _ in g["params"]]
        if not params:
            raise ValueError("ClipAdamW has no parameters")
        device = params[0].device
        for i, p in enumerate(params):
            if p.device != device:
                raise ValueError(f"parameter {i} is on {p.device}, parameter 0 on {device}: one device per optimizer")
            if p.dtype != torch.float32 or not p.is_contiguous() or p.is_sparse:
                raise ValueError(f"parameter {i} is not a contiguous float32 tensor ({p.dtype}, strides {p.stride()})")
        plan = _Plan()
        plan.params, plan.group_of, plan.device, plan.n = params, group_of, device, len(params)
        numel = [p.numel() for p in params]
        starts, at = [], 0
        for n in numel:                          # every tensor's moments start 16-byte aligned
            starts.append(at)
            at += -(-n // 4) * 4
        plan.exp_avg = torch.zeros(at, dtype=torch.float32, device=device)
        plan.exp_avg_sq = torch.zeros(at, dtype=torch.float32, device=device)
        steps = []
        for i, p in enumerate(params):
            m = plan.exp_avg[starts[i]:starts[i] + numel[i]].view(p.shape)
            v = plan.exp_avg_sq[starts[i]:starts[i] + numel[i]].view(p.shape)
            old = self.state.get(p)
            if old:
                m.copy_(old["exp_avg"])
                v.copy_(old["exp_avg_sq"])
                steps.append(float(old["step"]))
            else:
                steps.append(0.0)
            self.state[p] = {"exp_avg": m, "exp_avg_sq": v}
        plan.steps = torch.tensor(steps, dtype=torch.float32).to(device)
        for i, p in enumerate(params):
            self.state[p] = {"step": plan.steps[i], **self.state[p]}        # (torch's key order)
        plan.views = [(st["step"], st["exp_avg"], st["exp_avg_sq"]) for st in (self.state[p] for p in params)]
        plan.zero = torch.zeros((), dtype=torch.float32, device=device)
        if device.type == "cuda":
            self._build_tables(plan, numel)
        self._plan = plan
        return plan

    def _state_is_packed(self, plan: _Plan) -> bool:
        """False once somebody has put other tensors into ``self.state`` (a restore that assigns clones, say): they are
        adopted like a loaded state dict."""
        get = self.state.get
        for p, (step, m, v) in zip(plan.params, plan.views):
            st = get(p)
            if st is None or st.get("step") is not step or st.get("exp_avg") is not m or st.get("exp_avg_sq") is not v:
                return False
        return True

    def _build_tables(self, plan: _Plan, numel) -> None:
        from . import _opt_lib as L             # CUDA parameters without the library are an error, not a fallback
        if len(self.param_groups) > L.MAX_GROUPS:
            raise ValueError(f"{len(self.param_groups)} parameter groups: the kernel takes at most {L.MAX_GROUPS}")
        rows = np.zeros(plan.n, dtype=L.TENSOR_DTYPE)
        rows["p"] = [p.data_ptr() for p in plan.params]
        rows["m"] = [self.state[p]["exp_avg"].data_ptr() for p in plan.params]
        rows["v"] = [self.state[p]["exp_avg_sq"].data_ptr() for p in plan.params]
        rows["numel"], rows["group"] = numel, plan.group_of
        counts = [-(-n // L.CHUNK) for n in numel]
        chunks = np.zeros(sum(counts), dtype=L.CHUNK_DTYPE)
        chunks["tensor"] = np.repeat(np.arange(plan.n, dtype=np.int32), counts)
        chunks["index"] = np.concatenate([np.arange(c, dtype=np.int32) for c in counts]) if counts else []
        if len(chunks) > L.MAX_CHUNKS:
            raise ValueError(f"{len(chunks)} chunks of {L.CHUNK} elements: one launch covers {L.MAX_CHUNKS}")
        plan.L, plan.rows, plan.n_chunks = L, rows, len(chunks)
        dev = plan.device
        plan.chunks_dev = torch.from_numpy(chunks.view(np.uint8).copy()).to(dev)
        plan.table_dev = torch.zeros(max(rows.nbytes, 1), dtype=torch.uint8, device=dev)
        plan.partials = torch.zeros(max(plan.n_chunks, 1), dtype=torch.float64, device=dev)
        plan.steps_prev = torch.zeros(plan.n, dtype=torch.float32, device=dev)
        # two pinned staging tables: the one written now is not the one the previous upload may still be reading
        plan.staging = [torch.zeros(max(rows.nbytes, 1), dtype=torch.uint8).pin_memory() for _ in range(2)]
        plan.events = [torch.cuda.Event() for _ in range(2)]
        plan.flip, plan.uploaded = 0, None       # (nothing uploaded yet: the first step does)
        plan.hyper = L.Hyper()

    # ------------------------------------------------------------------------------------------------ the step
    @torch.no_grad()
    def step(self, max_norm=None, closure=None):
        """One clipped AdamW step; returns the total gradient norm (what ``clip_grad_norm_`` returns) as a 0-dim
        tensor on the parameters' device without synchronising.  ``max_norm`` None or <= 0: no clipping."""
        if closure is not None:
            with torch.enable_grad():
                closure()
        plan = self._plan
        if plan is None or not self._state_is_packed(plan):
            plan = self._adopt()
        max_norm = 0.0 if max_norm is None else float(max_norm)
        grads = [p.grad for p in plan.params]
        for i, g in enumerate(grads):
            if g is None:
                continue
            if g.device != plan.device:
                raise ValueError(f"gradient of parameter {i} is on {g.device}, the parameter on {plan.device}")
            if g.is_sparse or g.dtype != torch.float32 or not g.is_contiguous() or g.shape != plan.params[i].shape:
                raise ValueError(f"gradient of parameter {i} is not a contiguous float32 tensor of the parameter's "
                                 f"shape ({g.dtype}, layout {g.layout}, shape {tuple(g.shape)}, strides "
                                 f"{g.stride() if not g.is_sparse else None})")
        if all(g is None for g in grads):
            return plan.zero                    # nothing launched
        if plan.device.type != "cuda":
            return self._step_cpu(plan, grads, max_norm)
        L = plan.L
        rows = plan.rows
        rows["g"] = [0 if g is None else g.data_ptr() for g in grads]
        rows["p"] = [p.data_ptr() for p in plan.params]
        with torch.cuda.device(plan.device):
            image = rows.tobytes()
            if image != plan.uploaded:
                k = plan.flip
                plan.events[k].synchronize()    # the copy that last read this staging table has finished
                plan.staging[k].numpy()[:rows.nbytes] = rows.view(np.uint8)
                plan.table_dev.copy_(plan.staging[k], non_blocking=True)
                plan.events[k].record()
                plan.flip, plan.uploaded = k ^ 1, image
            for gi, g in enumerate(self.param_groups):
                h = plan.hyper.group[gi]
                h.lr, h.weight_decay, h.eps = float(g["lr"]), float(g["weight_decay"]), float(g["eps"])
                h.beta1, h.beta2 = float(g["betas"][0]), float(g["betas"][1])
            out = torch.empty((), dtype=torch.float32, device=plan.device)
            stream = torch.cuda.current_stream().cuda_stream
            L.check(L.lib.optstep_sumsq(plan.table_dev.data_ptr(), plan.chunks_dev.data_ptr(), plan.n, plan.n_chunks,
                                        plan.partials.data_ptr(), plan.steps.data_ptr(), plan.steps_prev.data_ptr(),
                                        stream), "optstep_sumsq")
            L.check(L.lib.optstep_adamw(plan.table_dev.data_ptr(), plan.chunks_dev.data_ptr(), plan.n, plan.n_chunks,
                                        plan.partials.data_ptr(), plan.steps.data_ptr(), plan.steps_prev.data_ptr(),
                                        plan.hyper, len(self.param_groups), max_norm, out.data_ptr(), stream),
                    "optstep_adamw")
        return out

    def _step_cpu(self, plan: _Plan, grads, max_norm: float):
        """The kernel's statement in torch ops, operation by operation (module docstring)."""
        f32 = lambda x: torch.tensor(x, dtype=torch.float32)      # noqa: E731  (one rounding of the float64 scalar)
        total = torch.stack([g.double().square().sum() for g in grads if g is not None]).sum().sqrt()
        coef = torch.ones((), dtype=torch.float64)
        if max_norm > 0.0:
            c = max_norm / (total + 1e-6)
            coef = torch.where(c > 1.0, torch.ones_like(c), c)    # (NaN goes through)
        c = coef.float()
        for i, (p, g) in enumerate(zip(plan.params, grads)):
            if g is None:
                continue
            h = self.param_groups[plan.group_of[i]]
            lr, wd, eps, (b1, b2) = float(h["lr"]), float(h["weight_decay"]), float(h["eps"]), h["betas"]
            st = self.state[p]
            st["step"] += 1
            step = float(st["step"])
            bc1, bc2 = 1.0 - float(b1) ** step, 1.0 - float(b2) ** step
            m, v = st["exp_avg"], st["exp_avg_sq"]
            gs = g * c
            m.add_(f32(1.0 - b1) * (gs - m))
            v.mul_(f32(b2)).add_((f32(1.0 - b2) * gs) * gs)
            denom = v.sqrt() / f32(math.sqrt(bc2)) + f32(eps)
            p.mul_(f32(1.0 - lr * wd)).sub_(f32(lr / bc1) * (m / denom))
        return total.float()
