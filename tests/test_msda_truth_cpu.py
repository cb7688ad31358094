"""The float64 truth of tests/msda_truth.py and its error budget, proved without a GPU.

  * truth(pos_dtype=float64) is the C oracle's float64 statement (seeded shapes and every committed f64 golden);
  * truth(pos_dtype=float32) lands on the oracle's pixels bit for bit at knife edges;
  * a numpy model of a CORRECT kernel -- fp32 products, an fp32 sum in three orders, one round-to-nearest-even store
    to bf16 through torch.bfloat16 -- stays inside the bounds on every case of the GPU matrix;
  * six models of a SUBTLY WRONG kernel each leave the bounds on every case they apply to.
The last two together are what makes a case usable: tests/test_msda_truth_gpu.py runs the kernels on exactly these inputs.
"""
import numpy as np
import pytest
import torch

import msda_truth as mt
from conftest import golden_cases, load_golden

OUTPUTS = ("out", "grad_value", "grad_loc", "grad_attn")

# (seed, N, M, D, Lq, L, P, shapes): ORACLE_CASES of tests/test_msda_gpu.py
ORACLE_CASES = [
    (1, 1, 8, 32, 300, 4, 4, [(25, 42), (13, 21), (7, 11), (4, 6)]),
    (2, 2, 8, 32, 333, 4, 4, [(20, 30), (10, 15), (5, 8), (3, 4)]),
    (3, 1, 3, 32, 17, 2, 3, [(9, 7), (4, 5)]),
    (4, 3, 5, 32, 11, 3, 5, [(6, 6), (3, 3), (2, 1)]),
    (5, 1, 8, 32, 1, 4, 4, [(25, 42), (13, 21), (7, 11), (4, 6)]),
    (6, 1, 2, 16, 40, 2, 2, [(8, 8), (4, 4)]),
    (7, 1, 1, 1025, 3, 1, 2, [(3, 3)]),
    (8, 1, 8, 32, 64, 16, 1, [(3, 3)] * 16),
    (9, 1, 8, 32, 64, 17, 1, [(3, 3)] * 17),
]


def seeded_case(seed, N, M, D, Lq, L, P, shapes, dtype, lo=-0.15, hi=1.15):
    """tests/test_msda_gpu.py::seeded_case (that module is GPU-marked as a whole)."""
    rng = np.random.default_rng(seed)
    shapes = np.asarray(shapes, dtype=np.int64)
    S = int((shapes[:, 0] * shapes[:, 1]).sum())
    lsi = mt.level_starts(shapes)
    value = rng.standard_normal((N, S, M, D)).astype(dtype)
    loc = rng.uniform(lo, hi, (N, Lq, M, L, P, 2)).astype(dtype)
    attn = rng.uniform(0, 1, (N, Lq, M, L, P)).astype(dtype)
    attn /= attn.sum((-1, -2), keepdims=True)
    grad_out = rng.standard_normal((N, Lq, M * D)).astype(dtype)
    return dict(value=value, shapes=shapes, level_start=lsi, loc=loc, attn=attn, grad_out=grad_out)


def assert_is_the_oracle(t, want):
    """rtol 1e-12 per element, with the element's magnitude A as the floor of the scale: two float64 evaluations of a sum
    that cancels differ by 1e-16 A, not by 1e-16 |x|."""
    for name in OUTPUTS:
        scale = np.maximum(np.abs(want[name]), t["A_" + name])
        err = np.abs(t[name] - want[name])
        assert (err <= 1e-12 * scale).all(), (name, float((err / np.maximum(scale, 1e-300)).max()))


# ------------------------------------------------------------------------------------------------ truth = the oracle
@pytest.mark.parametrize("case", ORACLE_CASES, ids=lambda c: f"seed{c[0]}")
def test_truth_in_float64_positions_is_the_f64_oracle(case):
    from oracle import msda_oracle as oracle
    g = seeded_case(*case, np.float64)
    args = (g["value"], g["shapes"], g["level_start"], g["loc"], g["attn"])
    t = mt.truth(*args, g["grad_out"], pos_dtype=np.float64)
    gv, gl, ga = oracle.backward(*args, g["grad_out"])
    assert_is_the_oracle(t, dict(out=oracle.forward(*args), grad_value=gv, grad_loc=gl, grad_attn=ga))


@pytest.mark.parametrize("name", [n for n in golden_cases() if n.endswith("_f64")])
def test_truth_in_float64_positions_matches_the_f64_goldens(name):
    g = load_golden(name)
    t = mt.truth(g["value"], g["shapes"], g["level_start"], g["loc"], g["attn"], g.get("grad_out"), pos_dtype=np.float64)
    have = [k for k in OUTPUTS if k in g and k in t]
    assert "out" in have and ("grad_out" not in g or len(have) == 4), have
    for k in have:
        scale = np.maximum(np.abs(g[k].reshape(t[k].shape)), t["A_" + k])
        assert (np.abs(t[k] - g[k].reshape(t[k].shape)) <= 1e-12 * scale).all(), k


def test_truth_in_float32_positions_lands_on_the_oracles_pixels():
    """The knife-edge locations of test_index_arithmetic_is_bit_exact: pixel centres, borders, half pixels and their
    nextafter neighbours; integers and gate equal oracle.indices bit for bit."""
    from oracle import msda_oracle as oracle
    rng = np.random.default_rng(5)
    shapes = np.array([(100, 168), (50, 84), (25, 42), (13, 21)], dtype=np.int64)
    loc = rng.uniform(-0.05, 1.05, (2, 500, 8, 4, 4, 2)).astype(np.float32)
    for l, (H, W) in enumerate(shapes):
        k = rng.integers(0, 500, 64)
        ys = (rng.integers(-1, H + 1, 64).astype(np.float32) + 0.5) / np.float32(H)
        xs = (rng.integers(-1, W + 1, 64).astype(np.float32) + 0.5) / np.float32(W)
        loc[0, k, 0, l, 0, 1] = ys
        loc[0, k, 0, l, 0, 0] = xs
        loc[0, k, 1, l, 1, 1] = np.nextafter(ys, np.float32(2))
        loc[0, k, 1, l, 1, 0] = np.nextafter(xs, np.float32(-2))
    h_ref, w_ref, g_ref = oracle.indices(shapes, loc)
    p = mt.positions(shapes, loc, np.float32)
    live = g_ref.astype(bool)
    assert np.array_equal(p["gate"], live)
    assert np.array_equal(p["h_floor"][live].astype(np.int32), h_ref[live])
    assert np.array_equal(p["w_floor"][live].astype(np.int32), w_ref[live])
    assert live.mean() > 0.8
    # and the matrix's own edge cases sit on the same pixels as the oracle too
    for cid in mt.CASE_IDS:
        g = mt.make_case(cid, False)
        h_ref, w_ref, g_ref = oracle.indices(g["shapes"], g["loc"])
        p = mt.positions(g["shapes"], g["loc"], np.float32)
        live = g_ref.astype(bool)
        assert np.array_equal(p["gate"], live), cid
        assert np.array_equal(p["h_low"][live], h_ref[live]) and np.array_equal(p["w_low"][live], w_ref[live]), cid


def test_round_bf16_is_torchs_rounding():
    x = np.random.default_rng(0).standard_normal(1 << 16).astype(np.float32) * np.float32(2.0) ** np.arange(-8, 8).repeat(1 << 12)
    x[:4] = [0.0, -0.0, 1.00390625, 1.01171875]          # two exact ties: to even
    want = torch.from_numpy(x).bfloat16().float().numpy()
    assert np.array_equal(mt.round_bf16(x).view(np.uint32), want.view(np.uint32))


def test_bound_exponent_is_the_kernels():
    x = np.array([0.0, 1e-40, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0e38], dtype=np.float32)
    bits = x.view(np.uint32).astype(np.int64)
    want = np.where((bits == 0) | ((bits >> 23) - 126 < -100), -100, (bits >> 23) - 126)
    assert np.array_equal(mt.bound_exponent(x), want)
    assert (np.abs(x[2:]).astype(np.float64) < 2.0 ** want[2:]).all()


# ------------------------------------------------------------------------------------------------ the kernel model
F32 = np.float32
MUTANTS_BF16 = ("truncate", "bf16_products", "drop_corner", "swap_lh_lw", "swap_pair", "bf16_contributions")
MUTANTS_F32 = ("drop_corner", "swap_lh_lw")
ORDERS = ("forward", "reversed", "permuted")


def store(x, bf16, truncate=False):
    x = np.ascontiguousarray(x, dtype=F32)
    if not bf16:
        return x.astype(np.float64)
    if truncate:
        return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(F32).astype(np.float64)
    return torch.from_numpy(x).bfloat16().float().numpy().astype(np.float64)      # ONE round-to-nearest-even


def swap_pairs_in_one_lane_of_four(x):
    """Channels (2i, 2i+1) exchanged in the second quarter of the D channels: the two halves of a packed bf16 pair
    unpacked in the wrong order by one of the four lanes that share a row."""
    x = x.copy()
    D = x.shape[-1]
    lo, hi = D // 4, D // 2
    x[..., lo:hi:2], x[..., lo + 1:hi:2] = x[..., lo + 1:hi:2].copy(), x[..., lo:hi:2].copy()
    return x


def seq_sum(terms, order, rng):
    """fp32 sum over axis 1 of (R, J, ...) one term after the other, in the given order."""
    R, J = terms.shape[:2]
    if order == "reversed":
        terms = terms[:, ::-1]
    elif order == "permuted":
        idx = rng.permuted(np.tile(np.arange(J), (R, 1)), axis=1)
        terms = np.take_along_axis(terms, idx.reshape((R, J) + (1,) * (terms.ndim - 2)), 1)
    acc = np.zeros(terms.shape[:1] + terms.shape[2:], dtype=F32)
    for j in range(J):
        acc = acc + terms[:, j]
    return acc


def kernel_model(g, bf16, order, mutant=None):
    """A correct kernel in numpy float32 (``mutant``: one defect).  Returns the stored results as float64."""
    N, S, M, D, L, Lq, P = g["dims"]
    rng = np.random.default_rng(99)
    value, go = g["value"].astype(F32), g["grad_out"].reshape(N, Lq, M, D).astype(F32)
    if mutant == "swap_pair":
        value, go = swap_pairs_in_one_lane_of_four(value), swap_pairs_in_one_lane_of_four(go)
    pos = dict(mt.positions(g["shapes"], g["loc"], F32))
    if mutant == "swap_lh_lw":
        lvl = L - 1 if L > 1 else 0
        lh, lw = pos["lh"].copy(), pos["lw"].copy()
        lh[:, :, :, lvl], lw[:, :, :, lvl] = pos["lw"][:, :, :, lvl], pos["lh"][:, :, :, lvl]
        pos["lh"], pos["lw"] = lh, lw
    valid, index, _, _, _ = mt.corners(g["shapes"], g["level_start"], pos)
    R, J = N * Lq * M, L * P
    lh, lw = pos["lh"].astype(F32).reshape(R, J), pos["lw"].astype(F32).reshape(R, J)      # exact
    hh, hw = F32(1) - lh, F32(1) - lw
    w = np.stack([hh * hw, hh * lw, lh * hw, lh * lw], -1)                                # (R, J, 4) fp32
    valid = np.moveaxis(valid, 0, -1).reshape(R, J, 4).copy()
    index = np.moveaxis(index, 0, -1).reshape(R, J, 4)
    a = g["attn"].astype(F32).reshape(R, J)
    if mutant == "drop_corner":       # the lowest-weight live corner of the row, in 1 % of the rows (at least one)
        # (lowest among the corners a correct kernel cannot lose to rounding: a w > 2^-16 > gamma_k of a row whose
        #  weights sum to 1.  The float32 neighbours of a knife edge have corners of weight 2^-23: dropping one of
        #  those is inside the fp32 budget of any correct kernel and no bound can or should see it)
        aw = np.where(valid, a[..., None] * w, np.inf).reshape(R, J * 4)
        aw[aw <= 2.0 ** -16] = np.inf
        live = np.flatnonzero(np.isfinite(aw.min(1)))          # (a row that samples out of range has no corner to lose)
        rows = rng.choice(live, max(1, R // 100), replace=False)
        valid.reshape(R, J * 4)[rows, aw[rows].argmin(1)] = False
    w = np.where(valid, w, F32(0))
    n_ix = np.repeat(np.arange(N), Lq * M)[:, None, None]
    m_ix = np.tile(np.arange(M), N * Lq)[:, None, None]
    v = np.where(valid[..., None], value[n_ix, index, m_ix, :], F32(0))                   # (R, J, 4, D)
    res = {}
    # ---- forward: 4 L P corner terms of a row, one fp32 sum
    aw = a[..., None] * w                                                                  # (R, J, 4)
    terms = aw[..., None] * v
    if mutant == "bf16_products":
        terms = mt.round_bf16(terms)
    out = seq_sum(terms.reshape(R, J * 4, D), order, rng)
    res["out"] = store(out, bf16, mutant == "truncate").reshape(N, Lq, M * D)
    # ---- grad_attn / grad_loc: bilinear value and its derivatives per point, an fp32 sum over the channels
    go_r = go.reshape(R, 1, D)
    val = ((w[..., 0, None] * v[:, :, 0] + w[..., 1, None] * v[:, :, 1]) + w[..., 2, None] * v[:, :, 2]) + w[..., 3, None] * v[:, :, 3]
    okf = valid.astype(F32)
    hh_, hw_, lh_, lw_ = hh[..., None], hw[..., None], lh[..., None], lw[..., None]
    d_w = ((okf[..., 1, None] * hh_) * v[:, :, 1] - (okf[..., 0, None] * hh_) * v[:, :, 0]) + \
          ((okf[..., 3, None] * lh_) * v[:, :, 3] - (okf[..., 2, None] * lh_) * v[:, :, 2])
    d_h = ((okf[..., 2, None] * hw_) * v[:, :, 2] - (okf[..., 0, None] * hw_) * v[:, :, 0]) + \
          ((okf[..., 3, None] * lw_) * v[:, :, 3] - (okf[..., 1, None] * lw_) * v[:, :, 1])
    tga = go_r * a[..., None]                                                              # (R, J, D)
    ch = lambda x: seq_sum(np.moveaxis(x, -1, 1).reshape(R, D, J), order, rng)            # sum over the D channels
    Wl = np.repeat(g["shapes"][:, 1].astype(F32), P)[None, :]
    Hl = np.repeat(g["shapes"][:, 0].astype(F32), P)[None, :]
    res["grad_attn"] = ch(go_r * val).astype(np.float64).reshape(N, Lq, M, L, P)
    gl = np.stack([ch(d_w * tga) * Wl, ch(d_h * tga) * Hl], -1)
    res["grad_loc"] = gl.astype(np.float64).reshape(N, Lq, M, L, P, 2)
    # ---- grad_value: one fp32 contribution per live corner, added into an fp32 buffer in some order, rounded once
    contrib = (aw[..., None] * go.reshape(R, 1, 1, D))[valid]                              # (n, D)
    if mutant == "bf16_contributions":
        contrib = mt.round_bf16(contrib)
    cells = ((n_ix * S + index) * M + m_ix)[valid]
    if order == "reversed":
        contrib, cells = contrib[::-1], cells[::-1]
    elif order == "permuted":
        perm = rng.permutation(len(cells))
        contrib, cells = contrib[perm], cells[perm]
    gv = np.zeros((N * S * M, D), dtype=F32)
    np.add.at(gv, cells, contrib)
    res["grad_value"] = store(gv, bf16, mutant == "truncate").reshape(N, S, M, D)
    return res


def ratios(res, t, b):
    return {k: mt.worst_ratio(res[k], t[k], b[k]) for k in OUTPUTS}


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "f32"])
@pytest.mark.parametrize("case_id", mt.CASE_IDS)
def test_a_faithful_kernel_model_stays_inside_every_bound(case_id, bf16):
    g, t, b = mt.case_with_truth(case_id, bf16)
    worst = dict.fromkeys(OUTPUTS, 0.0)
    for order in ORDERS:
        r = ratios(kernel_model(g, bf16, order), t, b)
        worst = {k: max(worst[k], r[k]) for k in OUTPUTS}
    print(f"\n{case_id} {'bf16' if bf16 else 'f32'}: worst error / bound " + "  ".join(f"{k} {worst[k]:.3f}" for k in OUTPUTS))
    assert all(v < 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("case_id", mt.CASE_IDS)
def test_every_mutant_leaves_the_bounds(case_id):
    """Each wrong kernel breaks a bound on at least one element of every case: in the outputs its defect reaches."""
    g, t, b = mt.case_with_truth(case_id, True)
    g32, t32, b32 = mt.case_with_truth(case_id, False)
    reaches = {"truncate": ("out", "grad_value"), "bf16_products": ("out",), "bf16_contributions": ("grad_value",),
               "drop_corner": OUTPUTS, "swap_lh_lw": OUTPUTS,
               # (value AND grad_out pairs swapped: the channel dot products of grad_loc / grad_attn do not change)
               "swap_pair": ("out", "grad_value")}
    survivors = []
    for bf16, mutants, (gg, tt, bb) in ((True, MUTANTS_BF16, (g, t, b)), (False, MUTANTS_F32, (g32, t32, b32))):
        for mutant in mutants:
            r = ratios(kernel_model(gg, bf16, "forward", mutant), tt, bb)
            caught = [k for k in reaches[mutant] if r[k] > 1.0]
            print(f"\n{case_id} {'bf16' if bf16 else 'f32'} {mutant}: " + "  ".join(f"{k} {r[k]:.3g}" for k in reaches[mutant]))
            if not caught:
                survivors.append((mutant, bf16, r))
    assert not survivors, survivors
