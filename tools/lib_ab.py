#!/usr/bin/env python
"""A/B of BUILDS of libmsda_hip.so inside one process on one box (box-to-box spread is 2-4 %, so decisions between
builds are taken here): every library given is loaded through ctypes directly (no ABI check -- older rounds' builds
qualify) and timed on the encoder call, forward fused / plain and (ABI >= 3) backward fused with workspace.

    python tools/lib_ab.py [--out gpurun_out/lib_ab.txt] [--rounds 3] name=path.so [name=path.so ...]
    (a name ending in "+opt=val,opt=val" applies msda_set_option pairs to that library first)

    python tools/lib_ab.py --bits [--out FILE] base=path.so [name=path.so ...]
    does not time: it runs a fixed list of small calls (ABI 7 libraries) that between them take every dispatch path,
    twice through each library, and prints per call the kernel msda_last_kernel() names and, per output tensor, whether
    the library agrees with the FIRST one.  The rule comes from the first library alone: an output it reproduces bit for
    bit over its two passes must be bit-equal in the others; one it does not (float atomics into grad_value) may differ
    by at most twice its own pass-to-pass maximum absolute difference.  Exit status 1 when a call disagrees.
"""
import argparse
import ctypes
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from memotr_amd.synth import make_inputs, to_fused_inputs  # noqa: E402

c_int, c_void_p = ctypes.c_int, ctypes.c_void_p
FWD = [c_void_p] * 5 + [c_int] * 7 + [c_void_p, c_void_p, c_void_p]
FUSED_FWD = [c_void_p] * 4 + [c_int, c_void_p, c_int, c_void_p] + [c_int] * 7 + [c_void_p, c_void_p, c_void_p]
FUSED_BWD_WS = ([c_void_p] * 4 + [c_int, c_void_p, c_int, c_void_p, c_void_p] + [c_int] * 7 + [c_void_p] * 3 +
                [c_int, c_void_p, c_void_p, ctypes.c_size_t, c_void_p])


def timed(fn, iters=200, min_warm_ms=40.0, batches=5):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < min_warm_ms:
        fn()
    per = iters // batches
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(batches)]
    for s, e in ev:
        s.record()
        for _ in range(per):
            fn()
        e.record()
    torch.cuda.synchronize()
    t = sorted(s.elapsed_time(e) / per for s, e in ev)
    return t[len(t) // 2] * 1e3


PYRAMID = [(20, 30), (10, 15), (5, 8), (3, 4)]


def bits_cases():
    """[(name, options, run(lib) -> {output name: tensor})]: the same inputs for every library and pass."""
    g = torch.Generator().manual_seed(5)
    rnd = lambda *shape: torch.randn(*shape, generator=g).cuda()        # noqa: E731
    uni = lambda *shape: torch.rand(*shape, generator=g).cuda()         # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    spare = torch.zeros(64, device="cuda")      # (an empty tensor has no storage; the library rejects null pointers)
    ptr = lambda t: None if t is None else (t.data_ptr() or spare.data_ptr())       # noqa: E731
    cases = []

    def geometry(shapes, M, P, Lq, D=32, N=2, ref_dim=2):
        L = len(shapes)
        sh = torch.tensor(shapes, dtype=torch.int64)
        S = int(sh.prod(1).sum())
        self_attn = Lq is None
        Lq = S if self_attn else Lq
        x = dict(N=N, S=S, M=M, D=D, L=L, Lq=Lq, P=P, ref_dim=ref_dim, hs=sh.contiguous() if self_attn else None,
                 shapes=sh.cuda(), lstart=torch.cat((sh.new_zeros(1), sh.prod(1).cumsum(0)[:-1])).cuda(),
                 value=rnd(N, S, M, D), go=rnd(N, Lq, M * D), proj=rnd(N, Lq, 3 * M * L * P))
        if self_attn:       # reference point = the query's own pixel centre, offsets of a few pixels
            ref = torch.cat([torch.stack(torch.meshgrid((torch.arange(h) + 0.5) / h, (torch.arange(w) + 0.5) / w,
                                                        indexing="ij")[::-1], -1).reshape(-1, 2) for h, w in shapes])
            x["ref"] = ref[None, :, None, :].expand(N, S, L, 2).contiguous().cuda()
            x["proj"][..., :2 * M * L * P] *= 2.0
        else:
            x["ref"] = uni(N, Lq, L, ref_dim) * (1.0 if ref_dim == 2 else 0.4) + 0.05
        x["attn"] = torch.softmax(x["proj"][..., 2 * M * L * P:].reshape(N, Lq, M, L * P), -1).reshape(N, Lq, M, L, P).contiguous()
        off = x["proj"][..., :2 * M * L * P].reshape(N, Lq, M, L, P, 2)
        wh = torch.stack((x["shapes"][:, 1], x["shapes"][:, 0]), -1).float()[None, None, None, :, None, :]
        x["loc"] = (x["ref"][:, :, None, :, None, :2] + off / wh).contiguous()
        return x

    def dims(x):
        return (x["N"], x["S"], x["M"], x["D"], x["L"], x["Lq"], x["P"])

    def add(name, opts, x, kind, dtype=torch.float32, fused=False, ws=False, out=False, ref_grad=False, stride=0):
        tdt = dtype if dtype != torch.float64 else torch.float64
        cdt = torch.float64 if dtype == torch.float64 else torch.float32
        suf = {torch.float32: "f32", torch.float64: "f64", torch.bfloat16: "bf16"}[dtype]
        N, S, M, D, L, Lq, P = dims(x)
        value, go = x["value"].to(tdt), x["go"].to(tdt)
        if stride:          # group 1 of a (N, S, stride / (M * D), M, D) tensor
            wide = rnd(N, S, stride // (M * D), M, D).to(tdt)
            wide[:, :, 1] = value
            value = wide[:, :, 1]
        loc, attn = x["loc"].to(cdt), x["attn"].to(cdt)
        fwd_out = rnd(N, Lq, M * D).to(tdt) if out else None
        hs = x["hs"]
        head = (ptr(value), ptr(x["shapes"]), ptr(x["lstart"]))
        fargs = (ptr(x["proj"]), x["proj"].shape[2], ptr(x["ref"]), x["ref_dim"], None)

        def run(lib):
            res = {}
            if stride:
                assert lib.msda_next_value_pixel_stride(stride) == 0
            if kind == "fwd":
                o = torch.full((N, Lq, M * D), 7.0, dtype=tdt, device="cuda")
                tail = (N, S, M, D, L, Lq, P, ptr(o), ptr(hs), stream)
                rc = (getattr(lib, f"msda_fused_forward_{suf}")(*head, *fargs, *tail) if fused else
                      getattr(lib, f"msda_forward_{suf}")(*head, ptr(loc), ptr(attn), *tail))
                res["out"] = o
            else:
                gdt = torch.float64 if dtype == torch.float64 else torch.float32
                gv = (torch.zeros(N, S, stride // (M * D), M, D, dtype=gdt, device="cuda") if stride else
                      torch.full((N, S, M, D), 7.0, dtype=gdt, device="cuda"))
                gvp = gv[:, :, 1] if stride else gv
                w = torch.empty(int(lib.msda_backward_workspace_bytes(int(fused), N, S, M, D, L, Lq, P, value.element_size(),
                                                                      stream)) + 256, dtype=torch.uint8, device="cuda") if ws else None
                wsa = (ptr(w), w.numel() if ws else 0)
                res["grad_value"] = gv
                if fused:
                    gp = torch.zeros_like(x["proj"])
                    gr = torch.zeros(N, Lq, M, L, x["ref_dim"], device="cuda") if ref_grad else None
                    rc = lib.msda_fused_backward_out_f32 if suf == "f32" else lib.msda_fused_backward_out_bf16
                    rc = rc(*head, *fargs, ptr(go), ptr(fwd_out), N, S, M, D, L, Lq, P, ptr(gvp), ptr(gp), ptr(gr),
                            0 if stride else 1, ptr(hs), *wsa, stream)
                    res["grad_proj"] = gp
                    if ref_grad:
                        res["grad_ref_part"] = gr
                else:
                    gl, ga = torch.zeros_like(loc), torch.zeros_like(attn)
                    tail = (ptr(go), N, S, M, D, L, Lq, P, ptr(gvp), ptr(gl), ptr(ga), 0 if stride else 1, ptr(hs))
                    rc = (getattr(lib, f"msda_backward_ws_{suf}")(*head, ptr(loc), ptr(attn), *tail, *wsa, stream) if ws else
                          getattr(lib, f"msda_backward_{suf}")(*head, ptr(loc), ptr(attn), *tail, stream))
                    res["grad_loc"], res["grad_attn"] = gl, ga
            assert rc == 0, (name, lib.msda_last_error())
            return res
        cases.append((name, opts, run))

    dec = geometry(PYRAMID, 8, 4, 100)                  # a few queries: gather / rows
    dec4 = geometry(PYRAMID, 8, 4, 100, ref_dim=4)
    pyr = geometry(PYRAMID, 8, 4, None)                 # one query per pixel, host shapes: windowed / bins
    wide = geometry(PYRAMID, 4, 5, None)                # L * P = 20: the wide prologue and finish kernels
    none = geometry(PYRAMID, 8, 4, 0)
    f32, f64, b16 = torch.float32, torch.float64, torch.bfloat16
    for dt, tag in ((f32, "f32"), (b16, "bf16")):
        add(f"decoder fwd plain {tag}", {}, dec, "fwd", dt)
        add(f"decoder fwd fused {tag}", {}, dec, "fwd", dt, fused=True)
        add(f"decoder bwd plain {tag}", {}, dec, "bwd", dt)
        add(f"decoder bwd fused {tag}", {}, dec, "bwd", dt, fused=True)
        add(f"pyramid fwd plain {tag}", {}, pyr, "fwd", dt)
        add(f"pyramid fwd fused {tag}", {}, pyr, "fwd", dt, fused=True)
        add(f"pyramid bwd plain {tag}", {}, pyr, "bwd", dt)
        add(f"pyramid bwd fused {tag}", {}, pyr, "bwd", dt, fused=True)
        add(f"pyramid bwd fused ws {tag}", {}, pyr, "bwd", dt, fused=True, ws=True)
        add(f"pyramid bwd fused out {tag}", {}, pyr, "bwd", dt, fused=True, out=True)
        add(f"pyramid bwd fused out ws {tag}", {}, pyr, "bwd", dt, fused=True, out=True, ws=True)
        add(f"strided fwd fused {tag}", {}, dec, "fwd", dt, fused=True, stride=3 * 8 * 32)
        add(f"strided bwd fused {tag}", {}, dec, "bwd", dt, fused=True, stride=3 * 8 * 32)
        add(f"sorted bwd plain ws {tag}", {"bwd_variant": 13}, pyr, "bwd", dt, ws=True)
        add(f"sorted bwd fused ws {tag}", {"bwd_variant": 13}, pyr, "bwd", dt, fused=True, ws=True)
    add("generic fwd f64", {}, dec, "fwd", f64)
    add("generic bwd f64", {}, dec, "bwd", f64)
    add("decoder bwd fused ref_grad f32", {}, dec4, "bwd", fused=True, ref_grad=True)
    add("pyramid bwd fused ws ref_grad f32", {}, pyr, "bwd", fused=True, ws=True, ref_grad=True)
    add("strided fwd plain f32", {}, dec, "fwd", stride=2 * 8 * 32)
    add("strided bwd plain f32", {}, dec, "bwd", stride=2 * 8 * 32)
    add("sorted bwd fused ws 4-d ref f32", {"bwd_variant": 13}, dec4, "bwd", fused=True, ws=True)
    add("sorted bwd fused ws ref_grad f32", {"bwd_variant": 13}, dec4, "bwd", fused=True, ws=True, ref_grad=True)
    add("sorted without scratch f32", {"bwd_variant": 13}, pyr, "bwd")
    add("tile_lv bwd plain f32", {"bwd_variant": 10}, pyr, "bwd")
    add("tile_lv bwd fused f32", {"bwd_variant": 10}, pyr, "bwd", fused=True)
    add("tile_lv bwd fused ws f32", {"bwd_variant": 10}, pyr, "bwd", fused=True, ws=True)
    add("bins forced bwd fused ws f32", {"bwd_variant": 12}, pyr, "bwd", fused=True, ws=True)
    add("bwd_variant 1 f32", {"bwd_variant": 1}, pyr, "bwd")
    add("bwd_variant 5 f32", {"bwd_variant": 5}, pyr, "bwd")
    add("bwd_variant 5 decoder f32", {"bwd_variant": 5}, dec, "bwd")
    for v in (1, 3, 12):
        add(f"fwd_variant {v} pyramid plain f32", {"fwd_variant": v}, pyr, "fwd")
        add(f"fwd_variant {v} pyramid fused f32", {"fwd_variant": v}, pyr, "fwd", fused=True)
    add("fwd_variant 12 decoder f32", {"fwd_variant": 12}, dec, "fwd")
    add("selector level 1 bwd fused ws f32", {"sel_level": 1}, pyr, "bwd", fused=True, ws=True)
    add("selector level 2 bwd fused ws f32", {"sel_level": 2}, pyr, "bwd", fused=True, ws=True)
    add("selector level 2 bwd plain f32", {"sel_level": 2}, pyr, "bwd")
    add("selector level 1 fwd fused f32", {"sel_level": 1}, pyr, "fwd", fused=True)
    add("wide fwd fused f32", {}, wide, "fwd", fused=True)
    add("wide bwd fused f32", {}, wide, "bwd", fused=True)
    add("wide bwd fused ws f32", {}, wide, "bwd", fused=True, ws=True)
    add("wide tile_lv bwd fused ws f32", {"bwd_variant": 10}, wide, "bwd", fused=True, ws=True)
    add("wide sorted bwd fused ws f32", {"bwd_variant": 13}, wide, "bwd", fused=True, ws=True)
    add("Lq = 0 fwd f32", {}, none, "fwd")
    add("Lq = 0 bwd f32", {}, none, "bwd")
    add("Lq = 0 bwd fused f32", {}, none, "bwd", fused=True)
    return cases


def bits_main(args):
    from memotr_amd._cabi import declare
    from memotr_amd._lib import SYMBOLS
    cases = bits_cases()
    libs = []
    for spec in args.libs:
        name, path = spec.split("=", 1)
        libs.append((name, declare(ctypes.CDLL(os.path.abspath(path)), SYMBOLS)))
    runs = {}               # (library, pass) -> [(kernel, {output: tensor})]
    for name, lib in libs:
        for p in range(2):
            assert lib.msda_selector_reset() == 0
            rec = []
            for cname, opts, run in cases:
                for k, v in opts.items():
                    assert lib.msda_set_option(k.encode(), v) == 0, (k, v)
                res = run(lib)
                torch.cuda.synchronize()
                rec.append((lib.msda_last_kernel().decode(), {k: t.clone() for k, t in res.items()}))
                for k in opts:
                    assert lib.msda_set_option(k.encode(), -1 if k == "sel_level" else 0) == 0
            runs[name, p] = rec
    base = libs[0][0]
    diff = lambda a, b: float((a.double() - b.double()).abs().max()) if a.numel() else 0.0       # noqa: E731
    lines = ["| call | kernel (" + base + ") | output | " + base + " pass 1 vs 2 | " +
             " | ".join(f"{n} vs {base}" for n, _ in libs[1:]) + " |", "|---|---|---|---|" + "---|" * (len(libs) - 1)]
    bad = 0
    for i, (cname, _, _) in enumerate(cases):
        k0, o0 = runs[base, 0][i]
        for j, key in enumerate(o0):
            same0 = torch.equal(o0[key], runs[base, 1][i][1][key])
            own = diff(o0[key], runs[base, 1][i][1][key])
            cells = []
            for n, _ in libs[1:]:
                kn, on = runs[n, 0][i]
                eq, d = torch.equal(o0[key], on[key]), diff(o0[key], on[key])
                ok = kn == k0 and (eq if same0 else d <= 2.0 * own)
                bad += not ok
                cells.append(("bit-equal" if eq else f"max abs diff {d:.3e}") + ("" if kn == k0 else f", KERNEL {kn}") +
                             (" ok" if ok else " FAIL"))
            lines.append(f"| {cname if j == 0 else ''} | {k0 if j == 0 else ''} | {key} | " +
                         ("bit-equal" if same0 else f"max abs diff {own:.3e}") + " | " + " | ".join(cells) + " |")
    lines.append("")
    lines.append(f"{len(cases)} calls, {bad} disagreements")
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", action="store_true", help="compare outputs and kernel names instead of timing (see above)")
    ap.add_argument("--out", default="gpurun_out/lib_ab.txt")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--mask", action="store_true", help="pass an all-false padding mask (what the model does)")
    ap.add_argument("libs", nargs="+")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    if args.bits:
        sys.exit(bits_main(args))
    x = make_inputs(device="cuda", batch=args.batch)
    f = to_fused_inputs(x)
    N, S, M, D = x["value"].shape
    Lq, L, P = x["loc"].shape[1], x["loc"].shape[3], x["loc"].shape[4]
    out = torch.empty(N, Lq, M * D, device="cuda")
    gv, gp = torch.empty_like(x["value"]), torch.empty_like(f["proj"])
    hs = x["shapes"].cpu().contiguous()
    stream = torch.cuda.current_stream().cuda_stream
    mask = torch.zeros(N, S, dtype=torch.bool, device="cuda") if args.mask else None
    mptr = mask.data_ptr() if mask is not None else None
    entries = []
    for spec in args.libs:
        name, path = spec.split("=", 1)
        opts = []
        if "+" in name:
            name, o = name.split("+", 1)
            opts = [kv.split(":") for kv in o.split(",")]
        lib = ctypes.CDLL(os.path.abspath(path))
        lib.msda_forward_f32.argtypes, lib.msda_fused_forward_f32.argtypes = FWD, FUSED_FWD
        lib.msda_last_kernel.restype = ctypes.c_char_p
        lib.msda_last_error.restype = ctypes.c_char_p
        lib.msda_set_option.argtypes = [ctypes.c_char_p, c_int]
        for k, v in opts:
            assert lib.msda_set_option(k.encode(), int(v)) == 0, (k, v)
        has_ws = hasattr(lib, "msda_fused_backward_ws_f32")
        ws = None
        if has_ws:
            lib.msda_fused_backward_ws_f32.argtypes = FUSED_BWD_WS
            lib.msda_fused_workspace_bytes.argtypes = [c_int] * 5
            lib.msda_fused_workspace_bytes.restype = ctypes.c_size_t
            ws = torch.empty((int(lib.msda_fused_workspace_bytes(N, Lq, M, L, P)),), dtype=torch.uint8, device="cuda")

        def fused(lib=lib):
            rc = lib.msda_fused_forward_f32(x["value"].data_ptr(), x["shapes"].data_ptr(), x["level_start"].data_ptr(),
                                            f["proj"].data_ptr(), f["proj"].shape[2], f["ref"].data_ptr(), 2, mptr,
                                            N, S, M, D, L, Lq, P, out.data_ptr(), hs.data_ptr(), stream)
            assert rc == 0, lib.msda_last_error()

        def plain(lib=lib):
            rc = lib.msda_forward_f32(x["value"].data_ptr(), x["shapes"].data_ptr(), x["level_start"].data_ptr(),
                                      x["loc"].data_ptr(), x["attn"].data_ptr(), N, S, M, D, L, Lq, P,
                                      out.data_ptr(), hs.data_ptr(), stream)
            assert rc == 0, lib.msda_last_error()

        def bwd(lib=lib, ws=ws):
            rc = lib.msda_fused_backward_ws_f32(x["value"].data_ptr(), x["shapes"].data_ptr(),
                                                x["level_start"].data_ptr(), f["proj"].data_ptr(), f["proj"].shape[2],
                                                f["ref"].data_ptr(), 2, mptr, x["grad_out"].data_ptr(), N, S, M, D, L,
                                                Lq, P, gv.data_ptr(), gp.data_ptr(), None, 1, hs.data_ptr(),
                                                ws.data_ptr(), ws.numel(), stream)
            assert rc == 0, lib.msda_last_error()
        entries.append((name + ("+" + ",".join(f"{k}:{v}" for k, v in opts) if opts else ""), lib, fused, plain,
                        bwd if has_ws else None))
    ref = None
    lines = []
    for name, lib, fused, plain, bwd in entries:          # same outputs first
        fused()
        torch.cuda.synchronize()
        if ref is None:
            ref = out.clone()
        lines.append(f"{name:40s} fused output vs first library: max |diff| {float((out - ref).abs().max()):.2e}"
                     f"  [{lib.msda_last_kernel().decode()}]")
    for r in range(args.rounds):
        for name, lib, fused, plain, bwd in entries:
            tf, tp = timed(fused), timed(plain)
            tb = timed(bwd, iters=50) if bwd is not None else float("nan")
            lines.append(f"round {r} {name:40s} fwd fused {tf:7.2f} us   plain {tp:7.2f} us   bwd fused {tb:8.2f} us")
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
