"""3DmFV-Net on the native kernels (PCOPS_MFV_NATIVE=1) and on the torch form (=0: broadcast algebra, F.conv3d), in
alternating fresh child processes on the same GPU:

  * one training step (forward, cross entropy, backward, Adam) at B = 64, N = 1024 with 125 and with 512 Gaussians;
  * the representation alone at B = 256, N = 2048, K = 512.

    python tools/bench_mfv3d.py [--steps 20] [--warmup 5] [--rounds 2] [--out profiles/mfv3d_bench.txt]

Per run: ms (median of the timed iterations) and torch.cuda.max_memory_allocated over them.  Native step runs also time every
pcops_fv3d / pcops_conv3d entry point of one extra step (HIP events around each launch) and price each convolution launch on
its VALID-TAP FLOPs -- 2 B Cin Cout (sum over voxels of the taps inside the grid) -- against the 157.3 TF fp32 matrix peak of
the MI355X.  No ratio is fixed in advance: the torch form is the yardstick, and a layer where the native kernel loses shows as
such."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_TF = 157.3
CONVS = ("pcops_conv3d_fwd", "pcops_conv3d_dgrad", "pcops_conv3d_wgrad")


def valid_pairs(r, k):
    """(tap, voxel) pairs of one axis with the tap inside the grid: 19 of 25 for r = k = 5"""
    h = k // 2
    return sum(1 for i in range(r) for d in range(-h, h + 1) if 0 <= i + d < r)


def _timed(fn, warmup, steps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), torch.cuda.max_memory_allocated() / 2 ** 20


def child(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from scanobjectnn_amd import _lib
    from scanobjectnn_amd.graph import Model
    from scanobjectnn_amd.mfv3d import mfv3d_net_cls as m
    from scanobjectnn_amd.mfv3d import tf_util as T
    from scanobjectnn_amd.mfv3d.gmm import get_3d_grid_gmm
    from scanobjectnn_amd.synth import synth_clouds, synth_labels
    dev = "cuda:0"
    native = os.environ.get("PCOPS_MFV_NATIVE", "1") != "0"
    gmm = get_3d_grid_gmm([args.gaussians] * 3, 0.04)
    x = torch.from_numpy(synth_clouds(args.batch, args.points, seed=1)).to(dev)
    res = {"what": args.what, "native": native, "batch": args.batch, "points": args.points, "gaussians": args.gaussians ** 3,
           "kernels": []}
    if args.what == "fv":
        w, mu, sigma = (torch.as_tensor(np.asarray(a), dtype=torch.float32, device=dev) for a in gmm)
        res["ms"], res["max_memory_allocated_mb"] = _timed(lambda: T.get_3dmfv(x, w, mu, sigma, flatten=False), args.warmup,
                                                           args.steps)
        print("RESULT " + json.dumps(res), flush=True)
        return
    y = torch.from_numpy(synth_labels(args.batch, seed=1)).to(dev)
    net = Model(m.bind(gmm, device=dev), device=dev, seed=0).build(x)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)

    def step():
        opt.zero_grad(set_to_none=True)
        m.get_loss(net(x, is_training=True, bn_decay=0.9)[0], y).backward()
        opt.step()

    res["ms"], res["max_memory_allocated_mb"] = _timed(step, args.warmup, args.steps)
    if native:
        calls = []

        def hook(name, phase, a):
            if not name.startswith(("pcops_fv3d_", "pcops_conv3d_")):
                return
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            if phase == "pre":
                calls.append([name, a[:5] if name in CONVS else a[:3], ev, None])
            else:
                calls[-1][3] = ev
        _lib._hooks.append(hook)
        step()
        torch.cuda.synchronize()
        _lib._hooks.remove(hook)
        for name, shape, e0, e1 in calls:
            rec = {"name": name, "shape": [int(v) for v in shape], "ms": e0.elapsed_time(e1)}
            if name in CONVS:
                b, r, k, cin, cout = rec["shape"]
                rec["valid_gflop"] = 2.0 * b * cin * cout * valid_pairs(r, k) ** 3 / 1e9
                rec["dense_gflop"] = 2.0 * b * cin * cout * (r * k) ** 3 / 1e9
                rec["tflops"] = rec["valid_gflop"] / rec["ms"]
                rec["peak_fraction"] = rec["tflops"] / PEAK_TF
            res["kernels"].append(rec)
    print("RESULT " + json.dumps(res), flush=True)


def parent(args):
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("# tools/bench_mfv3d.py: 3DmFV-Net, %d timed iterations (median), warmup %d, %d rounds of alternating child processes"
        % (args.steps, args.warmup, args.rounds))
    configs = [("step", 64, 1024, 5), ("step", 64, 1024, 8), ("fv", 256, 2048, 8)]
    for what, b, n, g in configs:
        for r in range(args.rounds):
            for native in ("1", "0"):
                env = dict(os.environ, PCOPS_MFV_NATIVE=native)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--what", what, "--batch", str(b), "--points", str(n),
                       "--gaussians", str(g), "--steps", str(args.steps), "--warmup", str(args.warmup)]
                t0 = time.time()
                out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=args.child_timeout)
                if out.returncode != 0:
                    say("child %s B=%d K=%d native=%s failed (exit %d): %s" % (what, b, g ** 3, native, out.returncode,
                                                                              out.stderr[-2000:]))
                    raise SystemExit(1)
                res = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
                results.append(res)
                say("%-4s B=%-3d N=%-4d K=%-3d %-6s round %d: %9.3f ms  peak %9.1f MB  (%.0f s)"
                    % (what, b, n, g ** 3, "native" if res["native"] else "torch", r, res["ms"], res["max_memory_allocated_mb"],
                       time.time() - t0))
    say("")
    for what, b, n, g in configs:
        sel = [r for r in results if (r["what"], r["batch"], r["gaussians"]) == (what, b, g ** 3)]
        nat, ref = [r for r in sel if r["native"]], [r for r in sel if not r["native"]]
        mn, mt = statistics.median(r["ms"] for r in nat), statistics.median(r["ms"] for r in ref)
        say("%s B=%d N=%d K=%d: native %.3f ms, torch %.3f ms: torch / native %.2f; peak memory %.0f MB vs %.0f MB"
            % ("training step" if what == "step" else "representation", b, n, g ** 3, mn, mt, mt / mn,
               max(r["max_memory_allocated_mb"] for r in nat), max(r["max_memory_allocated_mb"] for r in ref)))
        if what == "step":
            say("  3DmFV kernels of one native step (last round; convolutions on valid-tap FLOPs):")
            for k in nat[-1]["kernels"]:
                extra = ""
                if "tflops" in k:
                    extra = "  %7.3f of %7.3f GFLOP  %6.2f TF  %.3f of the fp32 matrix peak" % (
                        k["valid_gflop"], k["dense_gflop"], k["tflops"], k["peak_fraction"])
                say("    %-20s %-24s %8.3f ms%s" % (k["name"], k["shape"], k["ms"], extra))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
            f.write("# raw\n" + "\n".join(json.dumps(r) for r in results) + "\n")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--child", action="store_true")
    p.add_argument("--what", default="step", choices=["step", "fv"])
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--points", type=int, default=1024)
    p.add_argument("--gaussians", type=int, default=5, help="grid subdivisions per axis")
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--rounds", type=int, default=2)
    p.add_argument("--child_timeout", type=int, default=300)
    p.add_argument("--out", default="")
    args = p.parse_args()
    child(args) if args.child else parent(args)


if __name__ == "__main__":
    main()
