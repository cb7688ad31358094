"""Test infrastructure: float64 truth of one clip + AdamW step and the error budget ``memotr_amd.optim.ClipAdamW`` is held
to, on CPU (tests/test_optim_cpu.py proves the budget on the torch-ops statement) and on the GPU (tests/test_optim_gpu.py:
memotr_amd/csrc/opt_ops.hip).  Plain numpy.

``one_step`` evaluates, in float64 from the float32 inputs, the statement of include/opt_ops_hip.h:

    total_norm = sqrt(sum g^2),  coef = min(1, max_norm / (total_norm + 1e-6))  (1 without clipping; NaN goes through)
    step' = step + 1,  bc1 = 1 - b1^step',  bc2 = 1 - b2^step',  w = 1 - b1,  d = 1 - lr wd,  s = lr / bc1,  q = sqrt(bc2)
    gs = g coef;   m' = m + w (gs - m);   v' = b2 v + ((1 - b2) gs) gs;   p' = p d - s (m' / (sqrt(v') / q + eps))

Beside each result stands its magnitude: the same expression with every term replaced by its absolute value,
    A_m = |m| + w (|gs| + |m|),   A_v = v'  (no term is negative),   A_p = |p| d + s (A_m / (sqrt(v') / q + eps))
(A_p carries A_m, not |m'|: the error of the computed m' is relative to A_m, and the update term inherits it).
|computed - x| <= gamma_k A_x, gamma_k = k u / (1 - k u), u = 2^-24, for ANY evaluation in which every float32 operation
rounds once (contracted or not) and no term passes through more than k roundings (Higham, Accuracy and Stability of
Numerical Algorithms, 2nd ed., lemma 3.1).  The kernel's division and square root are the correctly rounded ones: no
approximate reciprocal enters the count.

k per output, counted on the longest chain (each float32 scalar c, d, w, b2, 1 - b2, s, q, eps is its float64 value
rounded once; the float64 work behind them -- at most 2^13 additions deep for the norm of 2^34 elements, the powers,
the cancellation in 1 - b^step -- stays below 2^-39 relative and is covered by one rounding to spare per output):
  total_norm  2 + 1   float64 sum, square root (< 1 together), the store to float32 (1); 1 to spare
  c = coef    2       the float64 factor (< 1, from the norm's summation depth above) and its rounding to float32 (1)
  gs          3       c (2), the product (1)
  m'          7 + 1   the term w gs: gs (3), w (1), gs - m (1), times w (1), the sum (1) = 7; the term m: 1; w m: 4
  v'          10 + 1  the term ((1 - b2) gs) gs: 1 - b2 (1), gs twice (6), two products (2), the sum (1) = 10; b2 v: 3
  denom       9       sqrt(v'): half of v's 10 (5) and its own (1); q (1); the division (1); the sum with eps (1) = 9
                      (every term of v' and of denom is non-negative: the bound is relative to the value itself)
  p'          20 + 1  the update term: m' (7), denom (9), the division (1), s (1), times s (1), the difference (1) = 20;
                      the term p d: d (1), the product (1), the difference (1) = 3
The constants are counts, not fits: nothing here may be tuned to make a run pass.
"""
import math

import numpy as np

U32 = 2.0 ** -24
K_NORM, K_M, K_V, K_P = 3, 8, 11, 21


def bound(A, k):
    ku = k * U32
    return ku * np.asarray(A, dtype=np.float64) / (1.0 - ku)


def one_step(tensors, groups, max_norm):
    """tensors: [{"p", "g" (or None), "m", "v": float32 arrays, "step": the count before the step, "group": index}];
    groups: [{"lr", "weight_decay", "betas", "eps"}]; max_norm None or <= 0: no clipping.
    Returns {"total_norm", "coef", "tensors": [None (no gradient) or {"p", "m", "v", "A_p", "A_m", "A_v", "step"}]}."""
    with np.errstate(all="ignore"):
        sq = [math.fsum((np.asarray(t["g"], dtype=np.float64).ravel() ** 2).tolist())
              for t in tensors if t["g"] is not None]
        total = math.sqrt(math.fsum(sq)) if not any(math.isnan(x) for x in sq) else float("nan")
        coef = 1.0
        if max_norm is not None and max_norm > 0:
            c = max_norm / (total + 1e-6)
            coef = 1.0 if c > 1.0 else c                   # (NaN > 1 is False: NaN goes through)
        out = []
        for t in tensors:
            if t["g"] is None:
                out.append(None)
                continue
            h = groups[t["group"]]
            lr, wd, eps, (b1, b2) = float(h["lr"]), float(h["weight_decay"]), float(h["eps"]), h["betas"]
            step = float(t["step"]) + 1.0
            bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
            w, d, s, q = 1.0 - b1, 1.0 - lr * wd, lr / bc1, math.sqrt(bc2)
            p, g, m, v = (np.asarray(t[k], dtype=np.float64) for k in ("p", "g", "m", "v"))
            gs = g * coef
            m1 = m + w * (gs - m)
            A_m = np.abs(m) + w * (np.abs(gs) + np.abs(m))
            v1 = b2 * v + ((1.0 - b2) * gs) * gs
            denom = np.sqrt(v1) / q + eps
            p1 = p * d - s * (m1 / denom)
            A_p = np.abs(p) * abs(d) + s * (A_m / denom)
            out.append({"p": p1, "m": m1, "v": v1, "A_p": A_p, "A_m": A_m, "A_v": np.abs(v1), "step": step})
    return {"total_norm": total, "coef": coef, "tensors": out}


def worst_ratio(got, want, bnd):
    """max |got - want| / bound where the truth is finite; the NaN masks must be equal and an infinite truth must be
    met exactly (inf is returned otherwise).  A zero bound asks for an exact result."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    bnd = np.broadcast_to(np.asarray(bnd, dtype=np.float64), want.shape)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.size == 0:
        return 0.0
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return float("inf")
    inf = np.isinf(want)
    if not np.array_equal(got[inf], want[inf]):
        return float("inf")
    fin = np.isfinite(want)
    if not np.isfinite(got[fin]).all():
        return float("inf")
    err = np.abs(got[fin] - want[fin])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bnd[fin])
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------------------------------------ around an optimizer
def snapshot(optimizer):
    """The float32 state one step starts from, read from a ClipAdamW or a torch.optim.AdamW: a row per parameter in
    group order (a parameter without state yet: zero moments, step 0)."""
    rows = []
    for gi, group in enumerate(optimizer.param_groups):
        for p in group["params"]:
            st = optimizer.state.get(p) or {}
            arr = lambda x: x.detach().cpu().numpy().copy()                       # noqa: E731
            rows.append({"p": arr(p), "g": None if p.grad is None else arr(p.grad),
                         "m": arr(st["exp_avg"]) if st else np.zeros(tuple(p.shape), np.float32),
                         "v": arr(st["exp_avg_sq"]) if st else np.zeros(tuple(p.shape), np.float32),
                         "step": float(st["step"]) if st else 0.0, "group": gi})
    return rows


def hyper(optimizer):
    return [{k: g[k] for k in ("lr", "weight_decay", "betas", "eps")} for g in optimizer.param_groups]


def check_step(before, after, groups, max_norm, total_norm):
    """Worst ratio to the bound of every output of the step ``before`` -> ``after`` (two snapshots) and of the returned
    norm: {"p", "m", "v", "norm"}; the step counts must have advanced exactly and rows without a gradient must be
    bit-unchanged (asserted here)."""
    t = one_step(before, groups, max_norm)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for i, (b, a, w) in enumerate(zip(before, after, t["tensors"])):
        if w is None:
            for k in ("p", "m", "v"):
                assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (i, k)
            assert a["step"] == b["step"], i
            continue
        assert a["step"] == w["step"], (i, a["step"], w["step"])
        worst["p"] = max(worst["p"], worst_ratio(a["p"], w["p"], bound(w["A_p"], K_P)))
        worst["m"] = max(worst["m"], worst_ratio(a["m"], w["m"], bound(w["A_m"], K_M)))
        worst["v"] = max(worst["v"], worst_ratio(a["v"], w["v"], bound(w["A_v"], K_V)))
    worst["norm"] = worst_ratio(np.float64(total_norm), np.float64(t["total_norm"]), bound(abs(t["total_norm"]), K_NORM))
    return worst
