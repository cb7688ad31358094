"""The float64 truth of the fused deformable-attention entry (tests/msda_fused_truth.py) and its budget, proved without a
GPU on the very cases tests/test_msda_fused_truth_gpu.py runs:

  * the float32 statement -- fused_helpers.expected: torch float32 prologue, float32 C oracle, autograd through the
    prologue -- stays inside every bound on every case, bf16-rounded inputs included;
  * nine models of a subtly wrong kernel each leave the bounds on every case they apply to, and each says which tolerance
    of tests/test_msda_fused_gpu.py (``check``) it would have passed;
  * with float64 positions the Jacobian formulas are torch autograd in float64 through prologue_cpu applied to the float64
    C oracle, to 1e-10 of the magnitude A.
"""
import numpy as np
import pytest
import torch

import msda_fused_truth as ft
import msda_truth as mt
from fused_helpers import expected, prologue_cpu

OUTPUTS = ("out", "grad_value", "grad_proj", "grad_ref")


def ratios(got, T, B, soft=False):
    return {k: mt.worst_ratio(got[k], T[k], B["grad_proj_soft" if soft and k == "grad_proj" else k]) for k in OUTPUTS}


def test_every_case_has_its_rows_and_its_mask():
    for tag in ft.TAGS:
        g, T, B = ft.case_with_truth(tag, False)
        N, S, M, D, L, Lq, P = g["dims"]
        equal, wide, outside = ft.special_rows(N, Lq, M)
        assert len({equal, wide, outside}) == 3, tag
        lg = ft.logits_of(g)
        assert np.ptp(lg[equal]) == 0.0 and abs(np.ptp(lg[wide]) - ft.SPREAD) < 1e-4, tag
        assert not T["t"]["pos"]["gate"][outside].any(), tag
        n, q, m = outside
        cols = np.r_[m * 2 * L * P:(m + 1) * 2 * L * P, g["n_off"] + m * L * P:g["n_off"] + (m + 1) * L * P]
        assert not T["grad_proj"][n, q, cols].any() and not T["A_grad_proj"][n, q, cols].any(), tag
        assert (ft.CASES[tag][7]) == (g["mask"] is not None)
        if g["mask"] is not None:
            mask, lsi, shapes = g["mask"], g["level_start"], g["shapes"]
            W0 = int(shapes[0, 1])
            assert mask[:, W0 - 1:int(shapes[0].prod()):W0].all(), tag                     # last column of level 0
            assert (mask[:, lsi[1:] - 1] & mask[:, lsi[1:]]).any(), tag                    # a run across a level boundary
            assert N == 1 or (mask[0] != mask[1]).any(), tag
            for l in range(L):
                assert not mask[:, lsi[l]:lsi[l] + shapes[l].prod()].all(1).any(), tag     # every level keeps pixels
            # (an earlier draft masked the whole last level: no mutant of the softmax Jacobian could show there)
            assert (T["t"]["A_grad_attn"].max(axis=(0, 1, 4)) > 0).all(), tag
            assert not T["grad_value"][mask].any()


# ------------------------------------------------------------------------------------------------ the fp32 statement
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "f32"])
@pytest.mark.parametrize("tag", ft.TAGS)
def test_the_float32_statement_stays_inside_every_bound(tag, bf16):
    g, T, B = ft.case_with_truth(tag, bf16)
    want = expected(ft.as_torch(g))
    got = {k: want[k].astype(np.float64) for k in OUTPUTS}
    if bf16:
        got["out"], got["grad_value"] = (mt.round_bf16(want[k]).astype(np.float64) for k in ("out", "grad_value"))
    assert np.array_equal(want["loc"].view(np.uint32), T["loc"].view(np.uint32))
    r = ratios(got, T, B)
    print(f"\nMSDA_FUSED_TRUTH cpu:fp32-statement {tag} {'bf16' if bf16 else 'f32'} " + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
    assert max(r.values()) < 1.0, r


# ------------------------------------------------------------------------------------------------ the mutants
def old_tolerances_passed(got, T, g):
    """The outputs on which ``check`` of tests/test_msda_fused_gpu.py (scale 1) would have accepted ``got`` for truth."""
    s = max(1.0, np.sqrt(g["dims"][3]) / 4)
    tol = dict(out=(1e-4, 4e-5 * s), grad_value=(1e-4, 2e-4 * s), grad_proj=(2e-4, 5e-4 * s), grad_ref=(2e-4, 2e-2 * s))
    return [k for k in OUTPUTS if np.allclose(got[k], T[k], rtol=tol[k][0], atol=tol[k][1])]


def mutant(name, g, T):
    """(outputs of the wrong kernel in float64, the outputs its defect reaches, soft budget?) or None: does not apply."""
    N, S, M, D, L, Lq, P = g["dims"]
    LP, t, a = L * P, T["t"], T["a"]
    ga = t["grad_attn"].reshape(N, Lq, M, LP)
    got = {k: T[k] for k in OUTPUTS}
    if name == "a_dot_drops_last_point":
        got.update(ft.jacobians(g, t, a, dot=(a[..., :-1] * ga[..., :-1]).sum(-1, keepdims=True)))
        return got, ("grad_proj",), False
    if name == "b_point0_without_dot":
        gp = T["grad_proj"].copy().reshape(N, Lq, -1)
        view = gp[..., g["n_off"]:g["n_off"] + M * LP].reshape(N, Lq, M, LP)
        view[..., 0] = a[..., 0] * ga[..., 0]
        gp[..., g["n_off"]:g["n_off"] + M * LP] = view.reshape(N, Lq, -1)
        got["grad_proj"] = gp
        return got, ("grad_proj",), False
    if name == "c_offsets_2d_divided_by_HW_swapped":
        if g["ref_dim"] != 2 or (g["shapes"][:, 0] == g["shapes"][:, 1]).all():
            return None
        gp = T["grad_proj"].copy()
        wh = g["shapes"][:, ::-1].astype(np.float64).reshape(1, 1, 1, L, 1, 2)
        off = gp[..., :g["n_off"]].reshape(N, Lq, M, L, P, 2) * wh / wh[..., ::-1]
        gp[..., :g["n_off"]] = off.reshape(N, Lq, -1)
        got["grad_proj"] = gp
        return got, ("grad_proj",), False
    if name == "d_offsets_4d_take_ref2_twice":
        if g["ref_dim"] != 4:
            return None
        gp = T["grad_proj"].copy()
        J = g["ref"].astype(np.float64)[:, :, None, :, None, 2:3] * 0.5 / P
        gp[..., :g["n_off"]] = (t["grad_loc"] * J).reshape(N, Lq, -1)
        got["grad_proj"] = gp
        return got, ("grad_proj",), False
    if name == "e_grad_ref_omits_one_head":
        gl = t["grad_loc"][:, :, 1:]
        gr = gl.sum((2, 4))
        if g["ref_dim"] == 4:
            off = g["proj"][..., :g["n_off"]].astype(np.float64).reshape(N, Lq, M, L, P, 2)[:, :, 1:]
            gr = np.concatenate([gr, (gl * off * 0.5 / P).sum((2, 4))], -1)
        got["grad_ref"] = gr
        return got, ("grad_ref",), False
    if name == "f_grad_ref_level0_scaled_1p00003":
        # A relative defect 3e-5 |x| shows where |x| > (k u / 3e-5) A.  With a single query the two elements it touches
        # belong to the query that also holds the spread-40 row: k = 144 + 32 + 262, k u = 2.6e-5, so it would take an
        # element without any cancellation (|x| > 0.87 A).  Not a property a case can promise: not applied at Lq = 1.
        if Lq == 1:
            return None
        gr = T["grad_ref"].copy()
        gr[:, :, 0] *= 1.0 + 3e-5
        got["grad_ref"] = gr
        return got, ("grad_ref",), False
    if name == "g_weights_from_bf16_logits":
        T2 = ft.fused_truth(g, a=ft.softmax64(mt.round_bf16(ft.logits_of(g))))
        return {k: T2[k] for k in OUTPUTS}, ("out", "grad_value", "grad_proj", "grad_ref"), False
    if name == "h_masked_pixel_read_and_written":
        if g["mask"] is None:
            return None
        T2 = ft.fused_truth(g, masked=False)
        return {k: T2[k] for k in OUTPUTS}, OUTPUTS, False
    if name == "i_soft_dot_from_bf16_out":
        if not (L == 4 and P == 4 and g["ref_dim"] == 2):
            return None
        go = g["grad_out"].astype(np.float64).reshape(N, Lq, M, D)
        out16 = mt.round_bf16(T["out"].astype(np.float32)).astype(np.float64).reshape(N, Lq, M, D)
        got.update(ft.jacobians(g, t, a, dot=(go * out16).sum(-1, keepdims=True)))
        return got, ("grad_proj",), True
    raise KeyError(name)


MUTANTS = ("a_dot_drops_last_point", "b_point0_without_dot", "c_offsets_2d_divided_by_HW_swapped",
           "d_offsets_4d_take_ref2_twice", "e_grad_ref_omits_one_head", "f_grad_ref_level0_scaled_1p00003",
           "g_weights_from_bf16_logits", "h_masked_pixel_read_and_written", "i_soft_dot_from_bf16_out")


@pytest.mark.parametrize("tag", ft.TAGS)
def test_every_mutant_leaves_the_bounds(tag):
    """Each wrong kernel breaks a bound in EVERY output its defect reaches, on every case it applies to; the soft form's
    exact dot <grad_out_row, out_row> itself stays inside the soft budget."""
    g, T, B = ft.case_with_truth(tag, False)
    survivors, applied = [], 0
    for name in MUTANTS:
        m = mutant(name, g, T)
        if m is None:
            continue
        applied += 1
        got, reaches, soft = m
        r = ratios(got, T, B, soft)
        old = old_tolerances_passed(got, T, g)
        passed_old = [k for k in reaches if k in old]
        print(f"\nMSDA_FUSED_TRUTH cpu:mutant {tag} {name}: " + " ".join(f"{k}={r[k]:.3g}" for k in reaches) +
              (f"  | passes test_msda_fused_gpu.check on {', '.join(passed_old)}" if passed_old else "  | fails the existing check too"))
        if name.startswith("f_"):
            assert "grad_ref" in old        # rtol 2e-4 / atol 2e-2 accepts a reference-point gradient off by 3e-5
        if not all(r[k] > 1.0 for k in reaches):
            survivors.append((name, {k: r[k] for k in reaches}))
        assert all(r[k] <= 1.0 for k in OUTPUTS if k not in reaches), (name, r)
    assert applied >= 6 and not survivors, survivors


# ------------------------------------------------------------------------------------------------ the formulas
@pytest.mark.parametrize("tag", ft.TAGS)
def test_float64_jacobians_are_autograd_through_the_module_prologue(tag):
    from oracle import msda_oracle as oracle
    g = ft.make_case(tag, False)
    T = ft.fused_truth(g, pos_dtype=np.float64)
    c = ft.as_torch(g)
    proj = c["proj"].double().requires_grad_(True)
    ref = c["ref"].double().requires_grad_(True)
    loc, attn = prologue_cpu(proj, ref, c["shapes"], g["M"], g["L"], g["P"])
    value = c["value"].double()
    if c["mask"] is not None:
        value = value.masked_fill(c["mask"][..., None, None], 0.0)
    args = (value.contiguous().numpy(), g["shapes"], g["level_start"], loc.detach().contiguous().numpy(),
            attn.detach().contiguous().numpy())
    out = oracle.forward(*args)
    gv, gl, ga = oracle.backward(*args, g["grad_out"].astype(np.float64))
    assert out.dtype == np.float64 and gl.dtype == np.float64
    if g["mask"] is not None:
        gv[g["mask"]] = 0.0
    torch.autograd.backward([loc, attn], [torch.from_numpy(gl), torch.from_numpy(ga)])
    want = dict(out=out, grad_value=gv, grad_proj=proj.grad.numpy(), grad_ref=ref.grad.numpy())
    for k in OUTPUTS:
        err = np.abs(T[k] - want[k].reshape(T[k].shape))
        assert (err <= 1e-10 * T["A_" + k]).all(), (tag, k, float((err / np.maximum(T["A_" + k], 1e-300)).max()))
