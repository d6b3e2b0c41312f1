"""Probe of the depth nest (forge_wino_gemm_dn, forge_wino_gemm_dn4): what the real kernels buy, per launch and on the headline.

    python tools/wino_dn_probe.py launch [--scenes B] [--out DIR]
        The gates, state and fusion_conv point-GEMM shapes of the step at R = 8192 B tile rows (32^3 voxels, C = 128): the nest (forge_wino_gemm_dn +
        forge_wino_output on 16 planes) against the four-point pair (forge_wino_gemm_half + forge_wino_output_half on 8 planes), device events over
        ITERS launches, best of 3, and the largest difference of the two results; then the F(4, 3) form: its operand transform of the hidden-state
        operand (forge_wino_input_dn4 against forge_wino_input), its GEMM (forge_wino_gemm_dn4) and the transform + GEMM + inverse pair against both
        the F(2, 3) nest's and the four-point form's; then, for gates and state with their GRU tails, the 24-point form (F(4, 3) along H as well,
        convops.WINO_DN4H) against the F(4, 3) nest, and the 36-point form (along W as well, convops.WINO_DN4HW) against the 24-point form, launch by
        launch: transform, GEMM, inverse.  -> DIR/<--tag>_launch.txt
    python tools/wino_dn_probe.py ab --parent-root DIR0 [--pairs 3] [--out DIR] [-- bench arguments]
        End to end: `python bench.py <bench arguments>` of a built checkout of the parent commit (DIR0) and of this tree, alternated --pairs times in
        fresh processes; one JSON line per run and the pair rule (new value_min above the parent's value_max in EVERY pair) with the median ratio.
        The parent runs from its own checkout rather than through FORGE_AMD_LIB: the binding of this tree lists forge_wino_gemm_dn, which the parent's
        library does not export.                                                                  -> DIR/<--tag>_headline.txt (appended)
    --tag names the record files (default r18_wino_dn4).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS = 30


def launch(args):
    sys.path.insert(0, ROOT)
    import torch
    from forge_amd import convops as co

    dev = torch.device("cuda:0")
    b, D, H, W, C = args.scenes, 32, 32, 32, 128
    Ht, Wt = H // 2, W // 2
    R, M = b * D * Ht * Wt, b * D * H * W
    g = torch.Generator().manual_seed(14)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)
    lines = ["depth nest per launch: %d scene(s), R = %d tile rows per point, C = %d; device events, %d launches, best of 3" % (b, R, C, ITERS)]

    def timed(fn):
        for _ in range(3):
            fn()
        best = 1e30
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(ITERS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) / ITERS)
        return best * 1e3                                          # us

    for name, C1, C2, Cout in (("gates", C, C, 2 * C), ("state", C, C, C), ("fusion_conv", C, 0, C)):
        Cin = C1 + C2
        V1, V2 = rn(16, R, C1), (rn(16, R, C2) if C2 else None)
        wp = rn(27, Cout, Cin) / (27 * Cin) ** 0.5
        F = co.WINO_FORMS
        U, Ud = co.wino_pack_packed(wp), co.wino_pack(F["dn"], wp)
        Mm = torch.empty(16 * R * Cout, device=dev)
        out_a, out_b = torch.empty(M, Cout, device=dev), torch.empty(M, Cout, device=dev)
        outp = lambda m, o: co.wino_output(m, None, None, None, 1.0, None, None, None, o, None, None, b, D, H, W, Cout, Cout, co.EPI_BIAS)
        g_dn = lambda: co.wino_form_gemm(F["dn"], V1, C1, V2, C2, Ud, Mm, b, D, Ht, Wt, Cout)
        g_h = lambda: co.wino_gemm(V1, C1, V2, C2, U, Mm, b, D, Ht, Wt, Cout, half=True)
        t = {"gemm_dn": timed(g_dn), "out16": timed(lambda: outp(g_dn(), out_a)) , "gemm_half": timed(g_h), "out8": timed(lambda: outp(g_h(), out_b))}
        outp(g_dn(), out_a)
        outp(g_h(), out_b)
        torch.cuda.synchronize()
        diff = (out_a - out_b).abs().max().item() / out_b.abs().max().item()
        tf = lambda us, taps: 2.0 * 16 * R * Cout * taps * Cin / us / 1e6
        lines.append("%-12s K/pos %3d Cout %3d | nest GEMM %7.1f us (%5.1f TF executed) + inverse = %7.1f us | four-point GEMM %7.1f us (%5.1f TF) + inverse = "
                     "%7.1f us | pair ratio %.3f, GEMM ratio %.3f | max |diff| / max |y| %.1e" % (
                         name, Cin, Cout, t["gemm_dn"], tf(t["gemm_dn"], 2), t["out16"], t["gemm_half"], tf(t["gemm_half"], 3), t["out8"],
                         t["out16"] / t["out8"], t["gemm_dn"] / t["gemm_half"], diff))
        # the F(4, 3) form: the hidden-state operand's transform is part of the pair (1.5 x the planes written)
        Ch = C2 or C1
        x = rn(M, Ch)
        Ud4 = co.wino_pack(F["dn4"], wp)
        W1, W2 = rn(16, R // 4 * 6, C1), (rn(16, R // 4 * 6, C2) if C2 else None)
        Vh, Vh6 = torch.empty(16, R, Ch, device=dev), torch.empty(16, R // 4 * 6, Ch, device=dev)
        g_d4 = lambda: co.wino_form_gemm(F["dn4"], W1, C1, W2, C2, Ud4, Mm, b, D, Ht, Wt, Cout)
        t_in, t_in6 = timed(lambda: co.wino_input(x, Ch, Ch, b, D, H, W, out=Vh)), timed(lambda: co.wino_form_input(F["dn4"], x, Ch, Ch, b, D, H, W, out=Vh6))
        t4 = timed(g_d4)
        full = lambda f_in, f_g, o: (f_in(), outp(f_g(), o))
        p4 = timed(lambda: full(lambda: co.wino_form_input(F["dn4"], x, Ch, Ch, b, D, H, W, out=Vh6), g_d4, out_a))
        p2 = timed(lambda: full(lambda: co.wino_input(x, Ch, Ch, b, D, H, W, out=Vh), g_dn, out_a))
        p1 = timed(lambda: full(lambda: co.wino_input(x, Ch, Ch, b, D, H, W, out=Vh), g_h, out_b))
        lines.append("%-12s F(4,3): GEMM %7.1f us (%5.1f TF executed), transform %6.1f us (plain %6.1f us) | transform + GEMM + inverse %7.1f us | "
                     "F(2,3) nest %7.1f us, four-point %7.1f us | ratio to F(2,3) %.3f, to four-point %.3f" % (
                         name, t4, tf(t4, 1.5), t_in6, t_in, p4, p2, p1, p4 / p2, p4 / p1))
    # the 24-point form (F(4, 3) along H as well, convops.WINO_DN4H) against the F(4, 3) nest, launch by launch, with the GRU tails of the steps
    lines.append("per launch, us: transform of the hidden-state operand | point GEMM | inverse transform with the GRU tail | sum")
    F4, FH, FHW = co.WINO_FORMS["dn4"], co.WINO_DN4H, co.WINO_DN4HW
    for name, Cout, epi in (("gates", 2 * C, co.EPI_GRU_GATES), ("state", C, co.EPI_GRU_OUT)):
        wp = rn(27, Cout, 2 * C) / (27 * 2 * C) ** 0.5
        x, h, z = rn(M, C), rn(M, C), torch.rand(M, C, generator=g).to(dev)
        o1, o2 = torch.empty(M, C, device=dev), torch.empty(M, C, device=dev)
        row = []
        for f in (F4, FH, FHW):
            Wf = W // f.tw
            Rf, rows = b * D * (H // f.th) * Wf, int(b * D * (H // f.th) * Wf * f.rows)
            U = co.wino_pack(f, wp)
            Vx, Vh = rn(f.points, rows, C), torch.empty(f.points, rows, C, device=dev)
            Mm = torch.empty(f.P * Rf * Cout, device=dev)
            t_in = timed(lambda: co.wino_form_input(f, x, C, C, b, D, H, W, out=Vh))
            gemm = lambda: co.wino_form_gemm(f, Vx, C, Vh, C, U, Mm, b, D, H // f.th, Wf, Cout)
            t_g = timed(gemm)
            P = gemm()
            inv = ((lambda: co.wino_output(P, None, None, None, 1.0, None, h, None, o1, o2, None, b, D, H, W, Cout, C, epi)) if epi == co.EPI_GRU_GATES else
                   (lambda: co.wino_output(P, None, None, None, 1.0, None, h, z, o1, None, None, b, D, H, W, Cout, C, epi)))
            t_o = timed(inv)
            wgs = (Rf // 256) * ((Cout + 127) // 128) * f.points
            row.append((f.name, t_in, t_g, t_o, wgs))
        for (n4, i4, g4, o4, w4), (nh, ih, gh, oh, wh) in zip(row, row[1:]):
            lines.append("%-6s %-5s %6.1f | %7.1f (%4d workgroups) | %6.1f | %7.1f    %-5s %6.1f | %7.1f (%4d workgroups) | %6.1f | %7.1f    ratios %.3f %.3f %.3f | %.3f" % (
                name, n4, i4, g4, w4, o4, i4 + g4 + o4, nh, ih, gh, wh, oh, ih + gh + oh, ih / i4, gh / g4, oh / o4, (ih + gh + oh) / (i4 + g4 + o4)))
    text = "\n".join(lines)
    print(text)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, args.tag + "_launch.txt"), "w") as f:
        f.write(text + "\n")


def _bench(root, bench_args, env=None):
    p = subprocess.run([sys.executable, "bench.py"] + bench_args, cwd=root, env=dict(os.environ, **(env or {})), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError("bench.py failed in %s (%d):\n%s" % (root, p.returncode, p.stderr[-2000:]))
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def ab(args):
    bench_args = args.bench or ["--gpus", "1", "--steps", "200", "--warmup", "20", "--repeats", "10"]
    keep = ("value", "value_min", "value_max", "unit", "ms_per_step", "psnr_vs_oracle_db", "max_abs_err_vs_oracle", "psnr_abs_diff_vs_oracle_db")
    lines, ratios, rule = ["# bench.py %s: parent and new alternated, %d pair(s)" % (" ".join(bench_args), args.pairs)], [], True
    for i in range(args.pairs):
        recs = {}
        for label, root in (("parent", args.parent_root), ("new", ROOT)):
            r = _bench(root, bench_args)
            r.update(r.get("repeats") or {})                       # value_min / value_max of the --repeats regions
            recs[label] = r
            lines.append("pair %d %-6s %s" % (i + 1, label, json.dumps({k: r[k] for k in keep if k in r})))
            print(lines[-1], flush=True)
        p, n = recs["parent"], recs["new"]
        if "value_min" in n and "value_max" in p:
            ok = n["value_min"] > p["value_max"]
            rule = rule and ok
            ratios.append(n["value"] / p["value"])
            lines.append("pair %d new value_min %.1f %s parent value_max %.1f, ratio of values %.4f" % (
                i + 1, n["value_min"], ">" if ok else "<=", p["value_max"], ratios[-1]))
            print(lines[-1], flush=True)
    if ratios:
        lines.append("pair rule (new value_min above parent value_max in every pair): %s; median ratio %.4f" % (
            "MET" if rule else "NOT MET", statistics.median(ratios)))
        print(lines[-1], flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, args.tag + "_headline.txt"), "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("launch", "ab"))
    ap.add_argument("--scenes", type=int, default=1)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--tag", default="r18_wino_dn4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    argv = sys.argv[1:]
    cut = argv.index("--") if "--" in argv else len(argv)       # after --: the arguments of bench.py (default: the headline run)
    a = ap.parse_args(argv[:cut])
    a.bench = argv[cut + 1:]
    if a.mode == "ab" and not a.parent_root:
        ap.error("ab needs --parent-root")
    launch(a) if a.mode == "launch" else ab(a)
