"""Test infrastructure: float64 truth of the FUSED deformable-attention entry points (msda_fused_forward_* /
msda_fused_backward_out_*), the error budget their kernels are held to and the case matrix.  Built on tests/msda_truth.py
(its ``truth``, ``bound_f32`` / ``bound_bf16``, ``k_*``, ``tile_lv_quantum``, ``round_bf16``); numpy, plus the torch CPU
prologue of tests/fused_helpers.py for the sampling locations.  tests/test_msda_fused_truth_cpu.py proves truth and budget
without a GPU, tests/test_msda_fused_truth_gpu.py applies them.

Inputs of a case: value (N, S, M, D), shapes, level_start, proj (N, Lq, >= 3 M L P) = [offsets | logits] float32, ref
(N, Lq, L, 2 | 4), mask (N, S) bool or None, grad_out (N, Lq, M D).

Truth
  loc     the float32 prologue of fused_helpers.prologue_cpu (the module's own operation order).  The kernels form these
          very bits (test_fused_locations_are_bit_identical_to_the_module_arithmetic), and the GPU tests assert so again
          before anything else, so truth and kernel sit on the same pixels.
  a       softmax of the float32 logits in float64.
  value'  value with the rows of masked pixels zero.
  t = msda_truth.truth(value', shapes, level_start, loc, a, grad_out), float32 positions.  From it, all in float64 and
  each with its magnitude A (the same expression with absolute values):
  out, grad_value     t's, with masked rows of grad_value (and of A, and of the contribution count) zero
  grad_logit_t        a_t (ga_t - sum_j a_j ga_j)                 A = a_t (A_ga_t + sum_j a_j A_ga_j)
  grad_offset         grad_loc / (W_l, H_l)              2-d reference points
                      grad_loc * ref_wh * 0.5 / P        4-d
  grad_ref            sum_{m,p} grad_loc                 2-d, and [..., :2] of 4-d
                      sum_{m,p} grad_loc * offset * 0.5 / P       [..., 2:] of 4-d
  grad_proj = [grad_offset | grad_logit] in the column order of proj.

Budget: a count of roundings, as in msda_truth.py (gamma_k A with k the longest chain of roundings of a term).
  c_a   the in-kernel softmax (msda_common.h: sm_exp, sm_rcp, row_softmax_stats) gives a weight the relative error
        c_a u, c_a = 6 Delta + L P + 6 with Delta = max - min logit of the row.  Read off the code:
          sm_exp(lg, mx) = exp2((lg - mx) * log2e): the subtraction is rounded (1), log2e is a rounded constant (1), the
          product is rounded (1) -- the argument x, |x| <= Delta log2e, carries 3 u |x| and exp2 turns an absolute error
          d of its argument into the relative error d ln 2: 3 Delta u.  exp2's own error: 1 ulp = 2 u.  e_t: 3 Delta + 2.
          The denominator adds L P such terms (each within 3 Delta + 2) with at most L P - 1 additions on any path of any
          summation order (the balanced tree has fewer): 3 Delta + 2 + L P - 1.  rcp: 1 ulp = 2 u.  e_t * rsum: 1.
          Sum: (3 Delta + 2) + (3 Delta + 2 + L P - 1) + 2 + 1 = 6 Delta + L P + 6.
        ASSUMPTION: v_exp_f32 and v_rcp_f32 are taken as accurate to 1 ulp.  Neither the programming guides at hand nor
        this repository state a figure (msda_common.h says "<= 2 ulp from the exact softmax" of the whole weight without
        a source); 1 ulp is what AMD's ISA documents give for both instructions.  Nobody has measured it here.  The
        generic kernels use expf and an IEEE division: less error, same budget.
  k per output
    out          k_out(L, P) + c_a                     every term of a row carries its weight's error once
    grad_value   k_grad_value(n) + max c_a             max over the rows of the cell's (batch, head): only they reach it
    offsets      k_grad_loc(D) + 3 + c_a               the weight is a factor of grad_loc; the Jacobian is at most 3
                                                       operations (0.5f / P, times ref_wh, times g; 2-d: one division)
    logits       k_grad_attn(D) + L P + 3 + 2 c_a      a enters twice (the factor a_t, and the a_j of the dot); the dot is
                                                       L P products and additions, then one subtraction, one product
    logits, soft max(the above, k_out(L, P) + c_a + D) the `soft` kernel takes sum_j a_j ga_j as <grad_out_row, out_row>
                                                       from the forward's stored output: the forward's chain, D
                                                       additions; its magnitude is sum_j a_j A_ga_j all the same
    grad_ref     k_grad_loc(D) + M P + max c_a         2-d: the M P - 1 additions over heads and points; max over the
                 ... + 3                               query's heads.  4-d: the offset Jacobian's 3 operations on top
  tile_lv paths add msda_truth.tile_lv_quantum to grad_value's bound; bf16 storage sends out and grad_value through
  bound_bf16, grad_proj and grad_ref are float32 outputs on the bf16-rounded value / grad_out.
Nothing here is fitted to a run.
"""
import numpy as np

import msda_truth as mt

PYR4 = [(20, 28), (10, 14), (5, 7), (3, 4)]
PYR4S = [(10, 14), (5, 7), (3, 4), (2, 2)]
DEC = [(25, 42), (13, 21), (7, 11), (4, 6)]
LP15 = [(6, 6), (3, 3), (2, 1)]

# The smallest geometries at which each path still has its tails.
# tag: (shapes, N, M, D, P, Lq or None = one query per pyramid pixel, ref_dim, mask, need_ref_grad)
CASES = {
    "fpyr4": (PYR4, 2, 8, 32, 4, None, 2, True, False),             # soft, soft16, rows16 + offsets_done
    "fpyr4r4": (PYR4, 1, 8, 32, 4, None, 4, False, False),          # rows16 with the finish kernel's location Jacobian
    "fpyr3odd": ([(13, 9), (7, 5), (4, 3)], 2, 3, 32, 2, None, 2, True, False),   # proj width 54: rows16 / soft decline
    "fpyr4p3": ([(17, 23), (9, 12), (5, 6), (3, 3)], 1, 8, 32, 3, None, 2, False, False),   # LP 12: points16 / finish16
    "fpyr4p5": (PYR4S, 1, 8, 32, 5, None, 2, True, False),          # LP 20: the 8-lanes-per-row side kernels
    "fpyr4p8": (PYR4S, 1, 2, 32, 8, None, 4, False, False),         # LP 32 on the tiled paths
    "fdec77": (DEC, 2, 8, 32, 4, 77, 4, True, True),                # rows<fused> + grad_ref_part
    "fdec17": (DEC, 1, 8, 32, 4, 17, 2, False, True),               # partial workgroup
    "fdec1": (DEC, 1, 8, 32, 4, 1, 2, False, True),                 # single query
    "flp15": (LP15, 3, 5, 32, 5, 11, 2, False, False),              # odd LP
    "flp32": (PYR4S, 1, 4, 32, 8, 37, 4, False, True),              # rows at kRowsMaxLP
    "flp33": (LP15, 1, 2, 32, 11, 21, 2, False, False),             # generic<fused> at D = 32, softmax groups 2..3
    "flp64": ([(6, 6), (3, 3), (2, 2), (1, 2)], 1, 2, 32, 16, 21, 4, False, False),      # ... group 4
    "fgen16": ([(8, 8), (4, 4)], 1, 2, 16, 2, 40, 2, True, False),  # D != 32: the generic kernels
    "fgen64": ([(8, 8), (4, 4)], 1, 2, 64, 2, 40, 2, True, False),
}
TAGS = list(CASES)
SPREAD = 40.0            # logit spread of the wide row


def special_rows(N, Lq, M):
    """(row of equal logits, row with a logit spread of SPREAD, row that samples out of range), each (n, q, m)."""
    return (0, 0, 0), ((0, 0, 1) if Lq == 1 else (0, 1, 0)), (N - 1, Lq - 1, M - 1)


def make_mask(shapes, lsi, N, S):
    """Differs between the batches; the last column of level 0 and a run across a level boundary; every level keeps
    unmasked pixels."""
    L = len(shapes)
    H0, W0 = int(shapes[0, 0]), int(shapes[0, 1])
    mask = np.zeros((N, S), dtype=bool)
    for n in range(N):
        mask[n, np.arange(H0) * W0 + W0 - 1] = True
        if n % 2 == 0:
            b = int(lsi[1]) if L > 1 else S // 2
            mask[n, b - 3:b + 2] = True
        else:
            b = int(lsi[L - 1])
            mask[n, b - 2:b + 1] = True
            mask[n, S // 3:S // 3 + 5] = True
    for l in range(L):
        lo = int(lsi[l])
        assert not mask[:, lo:lo + int(shapes[l].prod())].all(1).any()
    return mask


def make_case(tag, bf16, spare=0):
    """Inputs of one case, numpy.  `value` / `grad_out` carry the per-channel scale 2^U(-6, 6) of msda_truth.make_case
    (bf16: already rounded once); logits N(0, 2); offsets N(0, 2) pixels (2-d) or N(0, 1.5) box halves (4-d) around the
    query's own pixel centre (pyramid) or a uniform reference point.  Row `special_rows`: equal logits, a spread of 40,
    and offsets that put every point of the last query's last head far outside every level.  ``spare``: that many unused
    columns behind the 3 M L P of proj (random: nothing may read them)."""
    shapes_list, N, M, D, P, Lq, ref_dim, with_mask, need_ref = CASES[tag]
    rng = np.random.default_rng(2000 + 10 * TAGS.index(tag))
    shapes = np.asarray(shapes_list, dtype=np.int64)
    L = len(shapes)
    LP = L * P
    S = int(shapes.prod(1).sum())
    pyramid = Lq is None
    Lq = S if pyramid else Lq
    lsi = mt.level_starts(shapes)
    value = rng.standard_normal((N, S, M, D)).astype(np.float32)
    grad_out = rng.standard_normal((N, Lq, M, D)).astype(np.float32)
    value *= (2.0 ** rng.uniform(-6, 6, (M, D))).astype(np.float32)
    grad_out *= (2.0 ** rng.uniform(-6, 6, (M, D))).astype(np.float32)
    if pyramid:
        cen = []
        for (H, W) in shapes:
            ys, xs = np.meshgrid((np.arange(H) + 0.5) / H, (np.arange(W) + 0.5) / W, indexing="ij")
            cen.append(np.stack([xs.reshape(-1), ys.reshape(-1)], -1))
        ref = np.broadcast_to(np.concatenate(cen, 0)[None, :, None, :], (N, S, L, 2)).copy()
    else:
        ref = rng.uniform(0, 1, (N, Lq, L, 2))
    if ref_dim == 4:
        ref = np.concatenate([ref, rng.uniform(0.05, 0.3, (N, Lq, L, 2))], -1)
    off = rng.normal(0, 2.0 if ref_dim == 2 else 1.5, (N, Lq, M, L, P, 2))
    logits = rng.normal(0, 2.0, (N, Lq, M, LP))
    equal, wide, outside = special_rows(N, Lq, M)
    logits[equal] = 0.37
    logits[wide][0], logits[wide][1] = SPREAD / 2, -SPREAD / 2
    off[outside] = 1000.0 if ref_dim == 2 else 400.0 * P       # loc >= ref + 10 (4-d: ref_wh >= 0.05)
    proj = np.concatenate([off.reshape(N, Lq, -1), logits.reshape(N, Lq, -1), rng.standard_normal((N, Lq, spare))],
                          -1).astype(np.float32)
    mask = make_mask(shapes, lsi, N, S) if with_mask else None
    if bf16:
        value, grad_out = mt.round_bf16(value), mt.round_bf16(grad_out)
    return dict(tag=tag, value=value, shapes=shapes, shapes_list=shapes_list, level_start=lsi, proj=np.ascontiguousarray(proj),
                ref=np.ascontiguousarray(ref.astype(np.float32)), mask=mask,
                grad_out=np.ascontiguousarray(grad_out.reshape(N, Lq, M * D)), dims=(N, S, M, D, L, Lq, P), M=M, L=L, P=P,
                ref_dim=ref_dim, pyramid=pyramid, need_ref=need_ref, n_off=2 * M * LP)


def as_torch(g):
    """The case as the dict tests/fused_helpers.py and the GPU wrappers take (CPU tensors)."""
    import torch
    c = {k: torch.from_numpy(g[k]) for k in ("value", "shapes", "level_start", "proj", "ref", "grad_out")}
    c["mask"] = None if g["mask"] is None else torch.from_numpy(g["mask"])
    c.update(M=g["M"], L=g["L"], P=g["P"], shapes_list=g["shapes_list"])
    return c


def prologue_loc(g, dtype=np.float32):
    """Sampling locations by fused_helpers.prologue_cpu in ``dtype`` (float32: the bits the kernels form)."""
    import torch
    from fused_helpers import prologue_cpu
    td = torch.float32 if dtype == np.float32 else torch.float64
    loc, _ = prologue_cpu(torch.from_numpy(g["proj"]).to(td), torch.from_numpy(g["ref"]).to(td), torch.from_numpy(g["shapes"]),
                          g["M"], g["L"], g["P"])
    return np.ascontiguousarray(loc.numpy())


def logits_of(g):
    N, S, M, D, L, Lq, P = g["dims"]
    return g["proj"][..., g["n_off"]:g["n_off"] + M * L * P].reshape(N, Lq, M, L * P)


def softmax64(logits):
    x = np.asarray(logits, dtype=np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def jacobians(g, t, a, dot=None):
    """grad_proj (N, Lq, 3 M L P [+ spare zeros]) and grad_ref (N, Lq, L, 2 | 4) with their magnitudes from truth ``t``
    and the weights ``a`` (N, Lq, M, L P), float64.  ``dot``: sum_j a_j ga_j taken from elsewhere (N, Lq, M, 1)."""
    N, S, M, D, L, Lq, P = g["dims"]
    LP = L * P
    ga, A_ga = t["grad_attn"].reshape(N, Lq, M, LP), t["A_grad_attn"].reshape(N, Lq, M, LP)
    if dot is None:
        dot = (a * ga).sum(-1, keepdims=True)
    g_logit = a * (ga - dot)
    A_logit = a * (A_ga + (a * A_ga).sum(-1, keepdims=True))
    gl, A_gl = t["grad_loc"], t["A_grad_loc"]
    ref = g["ref"].astype(np.float64)
    off = g["proj"][..., :g["n_off"]].astype(np.float64).reshape(N, Lq, M, L, P, 2)
    if g["ref_dim"] == 2:
        J = 1.0 / g["shapes"][:, ::-1].astype(np.float64).reshape(1, 1, 1, L, 1, 2)          # (W_l, H_l)
    else:
        J = ref[:, :, None, :, None, 2:] * 0.5 / P
    g_off, A_off = gl * J, A_gl * np.abs(J)
    g_ref, A_ref = gl.sum((2, 4)), A_gl.sum((2, 4))
    if g["ref_dim"] == 4:
        g_ref = np.concatenate([g_ref, (gl * off * 0.5 / P).sum((2, 4))], -1)
        A_ref = np.concatenate([A_ref, (A_gl * np.abs(off) * 0.5 / P).sum((2, 4))], -1)
    spare = np.zeros((N, Lq, g["proj"].shape[2] - 3 * M * LP))
    cat = lambda o, lg: np.concatenate([o.reshape(N, Lq, -1), lg.reshape(N, Lq, -1), spare], -1)
    return dict(grad_proj=cat(g_off, g_logit), A_grad_proj=cat(A_off, A_logit), grad_ref=g_ref, A_grad_ref=A_ref)


def fused_truth(g, pos_dtype=np.float32, a=None, masked=True):
    """Every result of the fused entry in float64 with its magnitude: out, grad_value, grad_proj, grad_ref (+ A_*),
    n_grad_value, and the pieces (loc, a, t).  ``a`` / ``masked=False``: for the mutants of the CPU test."""
    loc = prologue_loc(g, pos_dtype)
    if a is None:
        a = softmax64(logits_of(g))
    N, S, M, D, L, Lq, P = g["dims"]
    value = g["value"].astype(np.float64)
    if g["mask"] is not None and masked:
        value[g["mask"]] = 0.0
    t = mt.truth(value, g["shapes"], g["level_start"], loc, a.reshape(N, Lq, M, L, P), g["grad_out"], pos_dtype=pos_dtype)
    res = dict(loc=loc, a=a, t=t, out=t["out"], A_out=t["A_out"], grad_value=t["grad_value"].copy(),
               A_grad_value=t["A_grad_value"].copy(), n_grad_value=t["n_grad_value"].copy())
    if g["mask"] is not None and masked:
        for k in ("grad_value", "A_grad_value", "n_grad_value"):
            res[k][g["mask"]] = 0.0
    res.update(jacobians(g, t, a))
    return res


def c_a(g):
    """Roundings of a softmax weight per (batch, query, head) row: 6 Delta + L P + 6 (module docstring)."""
    lg = logits_of(g).astype(np.float64)
    return 6.0 * (lg.max(-1) - lg.min(-1)) + g["L"] * g["P"] + 6.0


def counts(g, T):
    """k of every output element (module docstring), broadcast to the output's shape."""
    N, S, M, D, L, Lq, P = g["dims"]
    LP = L * P
    ca = c_a(g)                                                                    # (N, Lq, M)
    k = {}
    k["out"] = np.repeat(mt.k_out(L, P) + ca, D, axis=-1)                          # (N, Lq, M D)
    k["grad_value"] = (mt.k_grad_value(T["n_grad_value"]) + ca.max(1)[:, None, :])[..., None]
    k_off = np.broadcast_to((mt.k_grad_loc(D) + 3 + ca)[..., None], (N, Lq, M, 2 * LP))
    k_logit = np.broadcast_to((mt.k_grad_attn(D) + LP + 3 + 2 * ca)[..., None], (N, Lq, M, LP))
    k_soft = np.maximum(k_logit, (mt.k_out(L, P) + ca + D)[..., None])
    spare = np.zeros((N, Lq, g["proj"].shape[2] - 3 * M * LP))
    cat = lambda lg: np.concatenate([k_off.reshape(N, Lq, -1), lg.reshape(N, Lq, -1), spare], -1)
    k["grad_proj"], k["grad_proj_soft"] = cat(k_logit), cat(k_soft)
    k["grad_ref"] = (mt.k_grad_loc(D) + M * P + (3 if g["ref_dim"] == 4 else 0) + ca.max(2))[..., None, None] * \
        np.ones((1, 1, L, g["ref_dim"]))
    return k


def bounds(g, T, bf16):
    k = counts(g, T)
    store = (lambda x, A, kk: mt.bound_bf16(x, A, kk)) if bf16 else (lambda x, A, kk: mt.bound_f32(A, kk))
    return dict(out=store(T["out"], T["A_out"], k["out"]),
                grad_value=store(T["grad_value"], T["A_grad_value"], k["grad_value"]),
                grad_proj=mt.bound_f32(T["A_grad_proj"], k["grad_proj"]),
                grad_proj_soft=mt.bound_f32(T["A_grad_proj"], k["grad_proj_soft"]),
                grad_ref=mt.bound_f32(T["A_grad_ref"], k["grad_ref"]))


def tile_lv_bound(g, T, B, bf16):
    """grad_value's bound on the tile_lv paths: the fixed-point quantum on top (msda_bwd_tile_lv.h lines 13-18)."""
    N, S, M, D, L, Lq, P = g["dims"]
    quantum = mt.tile_lv_quantum(g["shapes"], g["level_start"], T["loc"], T["a"].astype(np.float32).reshape(N, Lq, M, L, P),
                                 g["grad_out"], N, S, M, D)
    return B["grad_value"] + (1.0 + (mt.U16 if bf16 else 0.0)) * quantum


_CACHE = {}


def case_with_truth(tag, bf16, spare=0):
    """(inputs, truth on them, bounds): computed once per session and shared; treat as read-only."""
    key = (tag, bool(bf16), spare)
    if key not in _CACHE:
        g = make_case(tag, bf16, spare)
        T = fused_truth(g)
        _CACHE[key] = (g, T, bounds(g, T, bf16))
    return _CACHE[key]
