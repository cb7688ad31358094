"""Test infrastructure: float64 truth of multi-scale deformable attention and the error budget every kernel of
memotr_amd/csrc/msda_*.h is held to (tests/test_msda_truth_cpu.py proves both without a GPU, tests/test_msda_truth_gpu.py
applies them).  Plain numpy, no C oracle, no torch.

``truth`` is one function, vectorised over (N, Lq, M, L, P).  The pixel a point falls on is decided in ``pos_dtype`` with
the rounding points msda_common.h documents (sample_setup): ``h_im = pos(pos(loc_y * H) - 0.5)``, ``h_low = floor(h_im)``,
the (-1, H) x (-1, W) gate and the per-corner bounds tests.  ``lh = h_im - h_low`` is exact in that type (Sterbenz / the
fraction of a float has no more bits than the float).  Everything after that -- bilinear weights, products, sums -- is
float64.  With ``pos_dtype=np.float32`` truth therefore sits on the same pixel as every kernel, knife edges included;
with ``np.float64`` it is the statement of oracle/msda_oracle.c in float64.

Beside each result x stands its magnitude A_x: the same expression with every product replaced by its absolute value.
|computed - x| <= gamma_k * A_x for ANY evaluation that rounds each intermediate once (any summation order, tree and DPP
reductions, contracted or uncontracted products) when no term passes through more than k roundings (Higham, Accuracy and
Stability of Numerical Algorithms, 2nd ed., section 4.2 and lemma 3.1), gamma_k = k u / (1 - k u), u = 2^-24.

k per output (``K_*``), counted on the longest chain a term can take:
  out         4 L P + 8   a corner term: 1 - lh, 1 - lw, their product, times the attention weight, times v (5; a
                          factored form -- bilinear value first, then the weight -- has no more) and at most 4 L P - 1
                          additions when the 4 L P corner terms of a row are added one after the other; 4 to spare
  grad_attn   4 D + 8     per channel: the corner weight (3), times v (1), three additions of the four corners (3),
                          times grad_out (1) = 8, and D - 1 additions over the channels: D + 7 <= 4 D + 8 for every D
  grad_loc    4 D + 16    per channel: 1 - lh (1), the corner difference and its scaling (2), the sum of the two
                          halves (1), times attention, times grad_out, times W or H (3), D - 1 additions: D + 6,
                          doubled for forms that scale each corner separately: within 4 D + 16 for every D
  grad_value  n + 8       a contribution: the corner weight (3), times attention (1), times grad_out (1), then at most
                          n - 1 additions of the n contributions a cell receives (atomics: any order) and the fp32
                          conversions of the staged paths (2): n + 6 <= n + 8
The constants are counts, not fits: nothing here may be tuned to make a run pass.

A bf16 result is the fp32 result rounded once to nearest-even: half a bf16 ulp of the truth, the fp32 error carried
through the rounding, and half the smallest bf16 subnormal (``bound_bf16``).
"""
import numpy as np

U32 = 2.0 ** -24          # unit round-off of fp32
U16 = 2.0 ** -8           # ... of bf16 (8 significant bits)
BF16_TINY = 2.0 ** -133   # the smallest bf16 subnormal


def k_out(L, P):
    return 4 * L * P + 8


def k_grad_attn(D):
    return 4 * D + 8


def k_grad_loc(D):
    return 4 * D + 16


def k_grad_value(n_grad_value):
    return np.asarray(n_grad_value, dtype=np.float64) + 8


def bound_f32(A, k):
    """gamma_k * A: a sum of fp32 operations in which no term passes through more than k roundings."""
    ku = np.asarray(k, dtype=np.float64) * U32
    return ku * np.asarray(A, dtype=np.float64) / (1.0 - ku)


def bound_bf16(x, A, k):
    """fp32 evaluation (bound_f32) followed by ONE round-to-nearest-even store to bf16."""
    return U16 * np.abs(x) + (1.0 + U16) * bound_f32(A, k) + BF16_TINY


def level_starts(shapes):
    hw = np.asarray(shapes, dtype=np.int64).prod(1)
    return np.concatenate([[0], np.cumsum(hw)[:-1]]).astype(np.int64)


def positions(shapes, loc, pos_dtype=np.float32):
    """The integer side and the fractions of every sampling point, each (N, Lq, M, L, P): h_low, w_low (int64), gate
    (bool), lh, lw (float64 copies of the exact ``pos_dtype`` differences)."""
    T = np.dtype(pos_dtype).type
    shapes = np.asarray(shapes, dtype=np.int64)
    loc = np.asarray(loc).astype(pos_dtype)
    L = shapes.shape[0]
    Hf = shapes[:, 0].astype(pos_dtype).reshape(1, 1, 1, L, 1)
    Wf = shapes[:, 1].astype(pos_dtype).reshape(1, 1, 1, L, 1)
    ph = (loc[..., 1] * Hf).astype(pos_dtype)             # the product is rounded first ...
    pw = (loc[..., 0] * Wf).astype(pos_dtype)
    h_im = (ph - T(0.5)).astype(pos_dtype)                # ... then 0.5 is subtracted: no contraction
    w_im = (pw - T(0.5)).astype(pos_dtype)
    gate = (h_im > T(-1)) & (w_im > T(-1)) & (h_im < Hf) & (w_im < Wf)
    fh, fw = np.floor(h_im), np.floor(w_im)
    lh = (h_im - fh).astype(np.float64)
    lw = (w_im - fw).astype(np.float64)
    with np.errstate(invalid="ignore"):
        h_low = np.where(gate, fh, 0).astype(np.int64)
        w_low = np.where(gate, fw, 0).astype(np.int64)
    return dict(h_low=h_low, w_low=w_low, gate=gate, lh=np.where(gate, lh, 0.0), lw=np.where(gate, lw, 0.0),
                h_floor=fh, w_floor=fw)


def corners(shapes, level_start, pos):
    """The four corners (00, 01, 10, 11) of every point: (valid (4, N, Lq, M, L, P) bool, pixel index into S (int64,
    0 where not valid), bilinear weight w_k, d w_k / d lw, d w_k / d lh), the last three float64."""
    shapes = np.asarray(shapes, dtype=np.int64)
    L = shapes.shape[0]
    H = shapes[:, 0].reshape(1, 1, 1, L, 1)
    W = shapes[:, 1].reshape(1, 1, 1, L, 1)
    start = np.asarray(level_start, dtype=np.int64).reshape(1, 1, 1, L, 1)
    h0, w0, gate, lh, lw = pos["h_low"], pos["w_low"], pos["gate"], pos["lh"], pos["lw"]
    hh, hw = 1.0 - lh, 1.0 - lw
    okh = (gate & (h0 >= 0), gate & (h0 + 1 <= H - 1))
    okw = (w0 >= 0, w0 + 1 <= W - 1)
    valid, index = [], []
    for dy in (0, 1):
        for dx in (0, 1):
            v = okh[dy] & okw[dx]
            valid.append(v)
            index.append(np.where(v, start + (h0 + dy) * W + (w0 + dx), 0))
    weight = np.stack([hh * hw, hh * lw, lh * hw, lh * lw])
    d_lw = np.stack([-hh, hh, -lh, lh])                    # d w_k / d lw: what grad_loc_x sums
    d_lh = np.stack([-hw, -lw, hw, lw])
    return np.stack(valid), np.stack(index), weight, d_lw, d_lh


def truth(value, shapes, level_start, loc, attn, grad_out=None, pos_dtype=np.float32):
    """out (N, Lq, M*D), grad_value (N, S, M, D), grad_loc (N, Lq, M, L, P, 2), grad_attn (N, Lq, M, L, P) in float64,
    each with its magnitude A_*, and n_grad_value (N, S, M): the contributions a cell receives.  Without ``grad_out``
    only the forward entries."""
    value = np.asarray(value, dtype=np.float64)
    attn = np.asarray(attn, dtype=np.float64)
    shapes = np.asarray(shapes, dtype=np.int64)
    N, S, M, D = value.shape
    _, Lq, _, L, P, _ = np.asarray(loc).shape
    pos = positions(shapes, loc, pos_dtype)
    valid, index, weight, d_lw, d_lh = corners(shapes, level_start, pos)
    n_ix = np.arange(N).reshape(N, 1, 1, 1)
    m_ix = np.arange(M).reshape(1, 1, M, 1)
    res = dict(pos=pos)
    out = np.zeros((N, Lq, M, D))
    A_out = np.zeros((N, Lq, M, D))
    if grad_out is not None:
        go = np.asarray(grad_out, dtype=np.float64).reshape(N, Lq, M, D)
        go_abs = np.abs(go)
        gv = np.zeros((N * S * M, D))
        A_gv = np.zeros((N * S * M, D))
        n_gv = np.zeros(N * S * M)
        gl = np.zeros((N, Lq, M, L, P, 2))
        A_gl = np.zeros((N, Lq, M, L, P, 2))
        ga = np.zeros((N, Lq, M, L, P))
        A_ga = np.zeros((N, Lq, M, L, P))
    a_abs = np.abs(attn)
    for l in range(L):
        Hl, Wl = float(shapes[l, 0]), float(shapes[l, 1])
        val = np.zeros((N, Lq, M, P, D))          # the bilinear value of the level's points and its partial sums
        A_val = np.zeros_like(val)
        dw = np.zeros_like(val)
        A_dw = np.zeros_like(val)
        dh = np.zeros_like(val)
        A_dh = np.zeros_like(val)
        for k in range(4):
            ok = valid[k][:, :, :, l, :]                                     # (N, Lq, M, P)
            idx = index[k][:, :, :, l, :]
            v = np.where(ok[..., None], value[n_ix, idx, m_ix, :], 0.0)      # (N, Lq, M, P, D); unread pixels stay unread
            w = (weight[k][:, :, :, l, :] * ok)[..., None]
            cw = (d_lw[k][:, :, :, l, :] * ok)[..., None]
            ch = (d_lh[k][:, :, :, l, :] * ok)[..., None]
            val += w * v
            A_val += w * np.abs(v)
            dw += cw * v
            A_dw += np.abs(cw) * np.abs(v)
            dh += ch * v
            A_dh += np.abs(ch) * np.abs(v)
            if grad_out is not None:
                flat = ((n_ix * S + idx) * M + m_ix)[ok]                     # cells of the valid corners
                aw = (attn[:, :, :, l, :, None] * w)                         # (N, Lq, M, P, 1)
                np.add.at(gv, flat, (aw * go[:, :, :, None, :])[ok])
                np.add.at(A_gv, flat, (np.abs(aw) * go_abs[:, :, :, None, :])[ok])
                np.add.at(n_gv, flat, 1.0)
        a = attn[:, :, :, l, :, None]
        out += (a * val).sum(3)
        A_out += (a_abs[:, :, :, l, :, None] * A_val).sum(3)
        if grad_out is not None:
            g = go[:, :, :, None, :]
            g_abs = go_abs[:, :, :, None, :]
            ga[:, :, :, l, :] = (g * val).sum(-1)
            A_ga[:, :, :, l, :] = (g_abs * A_val).sum(-1)
            gl[:, :, :, l, :, 0] = Wl * attn[:, :, :, l, :] * (g * dw).sum(-1)
            gl[:, :, :, l, :, 1] = Hl * attn[:, :, :, l, :] * (g * dh).sum(-1)
            A_gl[:, :, :, l, :, 0] = Wl * a_abs[:, :, :, l, :] * (g_abs * A_dw).sum(-1)
            A_gl[:, :, :, l, :, 1] = Hl * a_abs[:, :, :, l, :] * (g_abs * A_dh).sum(-1)
    res.update(out=out.reshape(N, Lq, M * D), A_out=A_out.reshape(N, Lq, M * D))
    if grad_out is not None:
        res.update(grad_value=gv.reshape(N, S, M, D), A_grad_value=A_gv.reshape(N, S, M, D),
                   n_grad_value=n_gv.reshape(N, S, M), grad_loc=gl, A_grad_loc=A_gl, grad_attn=ga, A_grad_attn=A_ga)
    return res


# ------------------------------------------------------------------------------------------------ the budget
def bounds(t, dims, bf16):
    """Per-element bound of every output of ``truth`` result ``t``; dims = (D, L, P).  bf16 storage rounds `out` and
    `grad_value` (accumulated in fp32, rounded once by the wrapper); grad_loc / grad_attn are fp32 outputs either way."""
    D, L, P = dims
    b = {}
    store = (lambda x, A, k: bound_bf16(x, A, k)) if bf16 else (lambda x, A, k: bound_f32(A, k))
    b["out"] = store(t["out"], t["A_out"], k_out(L, P))
    if "grad_value" in t:
        b["grad_value"] = store(t["grad_value"], t["A_grad_value"], k_grad_value(t["n_grad_value"])[..., None])
        b["grad_loc"] = bound_f32(t["A_grad_loc"], k_grad_loc(D))
        b["grad_attn"] = bound_f32(t["A_grad_attn"], k_grad_attn(D))
    return b


def worst_ratio(got, want, bound):
    """max |got - want| / bound over every element.  A zero bound asks for an exact result (ratio 0 if met, inf if
    not); a non-finite result is inf."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape == bound.shape, (got.shape, want.shape, bound.shape)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(r.max())


# ------------------------------------------------------------------------------------------------ tile_lv's quantum
def bound_exponent(x):
    """e with |x| < 2^e, as msda_bwd_tile_lv.h's bound_exponent: the float's exponent field - 126; zero and tiny
    values -> -100."""
    x = np.abs(np.asarray(x, dtype=np.float32))
    e = np.frexp(x)[1].astype(np.int64)          # x = m 2^e, 0.5 <= m < 1
    return np.where((x == 0) | (e < -100), -100, e)


def tile_lv_quantum(shapes, level_start, loc, attn, grad_out, N, S, M, D):
    """The fixed-point term of msda_bwd_d32_tile_lv's grad_value, (N, S, M, D).

    memotr_amd/csrc/msda_bwd_tile_lv.h lines 13-18: a workgroup owns (batch, region, head, level); its window holds
    grad_value as 32-bit fixed point with the power-of-two scales
        gexp[c]  |grad_out[:, c]| < 2^gexp[c] over the region's rows        (per batch, region, head, channel)
        aexp[l]  attention weights of level l < 2^aexp[l] over those rows   (per batch, region, head, level)
        K = min(30 - ceil(log2(rows * P)), 21),  rows = sum_l 4^(L-1-l) queries per region
    and every contribution is rounded once to a multiple of the quantum 2^-K 2^gexp[c] 2^aexp[l].  A cell therefore
    carries at most  sum over its contributions of 2^-K 2^gexp[c] 2^aexp[l]  beyond the fp32 budget (n_cell times the
    quantum when all of them come from one region; contributions from a neighbouring region bring that region's
    scales).  A region is the set of queries whose pixel falls into one cell of the coarsest level's grid (msda_tile.h):
    pixel (y, x) of level l belongs to region (y >> (L-1-l), x >> (L-1-l)).  Self-attention layout only (Lq == S).
    """
    shapes = np.asarray(shapes, dtype=np.int64)
    L = shapes.shape[0]
    _, Lq, _, _, P, _ = loc.shape
    assert Lq == S
    rows = sum(4 ** (L - 1 - l) for l in range(L))
    K = min(30 - int(np.ceil(np.log2(rows * P))), 21)
    reg = np.empty(Lq, dtype=np.int64)                       # region id of every query
    RX = max(-(-int(shapes[l, 1]) // (1 << (L - 1 - l))) for l in range(L))
    for l in range(L):
        Hl, Wl, sh = int(shapes[l, 0]), int(shapes[l, 1]), L - 1 - l
        y, x = np.divmod(np.arange(Hl * Wl), Wl)
        reg[int(level_start[l]):int(level_start[l]) + Hl * Wl] = (y >> sh) * RX + (x >> sh)
    n_reg = int(reg.max()) + 1
    go = np.abs(np.asarray(grad_out, dtype=np.float32).reshape(N, Lq, M, D))
    gmax = np.zeros((N, n_reg, M, D), dtype=np.float32)
    np.maximum.at(gmax, (np.arange(N)[:, None], reg[None, :]), go)
    amax = np.zeros((N, n_reg, M, L), dtype=np.float32)
    np.maximum.at(amax, (np.arange(N)[:, None], reg[None, :]), np.abs(np.asarray(attn, dtype=np.float32)).max(-1))
    gexp = bound_exponent(gmax).astype(np.float64)           # (N, n_reg, M, D)
    aexp = bound_exponent(amax).astype(np.float64)           # (N, n_reg, M, L)
    pos = positions(shapes, loc, np.float32)
    valid, index, _, _, _ = corners(shapes, level_start, pos)
    n_ix = np.arange(N).reshape(N, 1, 1, 1)
    m_ix = np.arange(M).reshape(1, 1, M, 1)
    q = np.zeros((N * S * M, D))
    for l in range(L):
        quantum = 2.0 ** (gexp[:, reg][:, :, :, None, :] + aexp[:, reg][:, :, :, l, None, None] - K)   # (N, Lq, M, 1, D)
        quantum = np.broadcast_to(quantum, (N, Lq, M, P, D))
        for k in range(4):
            ok = valid[k][:, :, :, l, :]
            flat = ((n_ix * S + index[k][:, :, :, l, :]) * M + m_ix)[ok]
            np.add.at(q, flat, quantum[ok])
    return q.reshape(N, S, M, D)


# ------------------------------------------------------------------------------------------------ the case matrix
def round_bf16(x):
    """float32 -> the nearest bf16 (ties to even), returned as float32: what ``tensor.bfloat16().float()`` gives."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


# The smallest geometries at which each path still has its tails (not the workload's).
GEOMETRIES = {
    # tag: (shapes, N, M, D, P, Lq or None = one query per pyramid pixel)
    "pyr4": ([(20, 28), (10, 14), (5, 7), (3, 4)], 2, 8, 32, 4, None),       # encoder layout, L = P = 4
    "pyr3odd": ([(13, 9), (7, 5), (4, 3)], 2, 3, 32, 2, None),               # M = 3: a wavefront's rows straddle queries
    "pyr1": ([(5, 5)], 1, 8, 32, 4, None),                                   # one query per region
    "dec300": ([(25, 42), (13, 21), (7, 11), (4, 6)], 1, 8, 32, 4, 300),     # few queries: rows / sorted / gather
    "dec17": ([(25, 42), (13, 21), (7, 11), (4, 6)], 1, 8, 32, 4, 17),
    "dec1": ([(25, 42), (13, 21), (7, 11), (4, 6)], 1, 8, 32, 4, 1),         # single query
    "lp15": ([(6, 6), (3, 3), (2, 1)], 3, 5, 32, 5, 11),                     # LP = 15, N = 3
    "gen16": ([(8, 8), (4, 4)], 1, 2, 16, 2, 40),                            # D != 32: the generic kernels
    "gen64": ([(8, 8), (4, 4)], 1, 2, 64, 2, 40),
}
VARIANTS = ("seeded", "edges")
CASE_IDS = [f"{g}-{v}" for g in GEOMETRIES for v in VARIANTS]
EDGE_POINTS = 64          # knife-edge locations per level of an "edges" case


def knife_edges(rng, H, W, n):
    """n (x, y) locations of a H x W level on pixel centres, borders and half pixels: (i + 0.5) / size for i in
    [-1, size], as tests/test_msda_gpu.py::test_index_arithmetic_is_bit_exact builds them."""
    ys = (rng.integers(-1, H + 1, n).astype(np.float32) + np.float32(0.5)) / np.float32(H)
    xs = (rng.integers(-1, W + 1, n).astype(np.float32) + np.float32(0.5)) / np.float32(W)
    return xs, ys


def make_case(case_id, bf16):
    """Inputs of one case of the matrix, numpy float32 (bf16: `value` / `grad_out` already rounded to bf16 once, so truth
    and kernel see the same numbers).  Seeded as seeded_case / pyramid_case of tests/test_msda_gpu.py build theirs: normal
    value / grad_out, normalised uniform attention weights, locations uniform in (-0.15, 1.15) or, on a pyramid, the
    query's own pixel centre plus N(0, 2) pixels.  `value` and `grad_out` carry a per-channel scale 2^U(-6, 6): outputs span
    four decades, so an absolute tolerance cannot hide a wrong low-magnitude channel.  "edges": 64 locations per level
    (point 0 of head 0) sit on knife edges and 64 more (point 1 of head 1) on their float32 neighbours.  The last
    query's last head of every case samples out of range."""
    tag, variant = case_id.split("-")
    shapes_list, N, M, D, P, Lq = GEOMETRIES[tag]
    seed = 1000 + 10 * list(GEOMETRIES).index(tag) + VARIANTS.index(variant)
    rng = np.random.default_rng(seed)
    shapes = np.asarray(shapes_list, dtype=np.int64)
    L = len(shapes)
    S = int(shapes.prod(1).sum())
    pyramid = Lq is None
    Lq = S if pyramid else Lq
    lsi = level_starts(shapes)
    value = rng.standard_normal((N, S, M, D)).astype(np.float32)
    loc = rng.uniform(-0.15, 1.15, (N, Lq, M, L, P, 2)).astype(np.float32)
    attn = rng.uniform(0, 1, (N, Lq, M, L, P)).astype(np.float32)
    attn /= attn.sum((-1, -2), keepdims=True)
    grad_out = rng.standard_normal((N, Lq, M, D)).astype(np.float32)
    if pyramid:
        ref = []
        for (H, W) in shapes:
            ys, xs = np.meshgrid((np.arange(H) + 0.5) / H, (np.arange(W) + 0.5) / W, indexing="ij")
            ref.append(np.stack([xs.reshape(-1), ys.reshape(-1)], -1))
        ref = np.concatenate(ref, 0)
        wh = shapes[:, ::-1].astype(np.float64)
        off = rng.normal(0, 2.0, (N, S, M, L, P, 2))
        loc = (ref[None, :, None, None, None, :] + off / wh[None, None, None, :, None, :]).astype(np.float32)
    value *= (2.0 ** rng.uniform(-6, 6, (M, D))).astype(np.float32)
    grad_out *= (2.0 ** rng.uniform(-6, 6, (M, D))).astype(np.float32)
    if variant == "edges":
        for l, (H, W) in enumerate(shapes):
            k = rng.integers(0, Lq, EDGE_POINTS)
            xs, ys = knife_edges(rng, int(H), int(W), EDGE_POINTS)
            loc[0, k, 0, l, 0, 0], loc[0, k, 0, l, 0, 1] = xs, ys
            loc[0, k, 1, l, 1, 0] = np.nextafter(xs, np.float32(-2))
            loc[0, k, 1, l, 1, 1] = np.nextafter(ys, np.float32(2))
    loc[N - 1, Lq - 1, M - 1] = 3.0       # one (query, head) row samples far outside every level: exact zeros
    if bf16:
        value, grad_out = round_bf16(value), round_bf16(grad_out)
    return dict(value=value, shapes=shapes, shapes_list=shapes_list, level_start=lsi, loc=loc, attn=attn,
                grad_out=np.ascontiguousarray(grad_out.reshape(N, Lq, M * D)), dims=(N, S, M, D, L, Lq, P),
                pyramid=pyramid)


_TRUTH_CACHE = {}


def case_with_truth(case_id, bf16):
    """(inputs, truth on them, bounds): computed once per session and shared; treat as read-only."""
    key = (case_id, bool(bf16))
    if key not in _TRUTH_CACHE:
        g = make_case(case_id, bf16)
        t = truth(g["value"], g["shapes"], g["level_start"], g["loc"], g["attn"], g["grad_out"])
        N, S, M, D, L, Lq, P = g["dims"]
        _TRUTH_CACHE[key] = (g, t, bounds(t, (D, L, P), bf16))
    return _TRUTH_CACHE[key]
