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
import os
import sys

import ab_bench

PEAK_TF = 157.3
CONVS = ("pcops_conv3d_fwd", "pcops_conv3d_dgrad", "pcops_conv3d_wgrad")


def valid_pairs(r, k):
    """(tap, voxel) pairs of one axis with the tap inside the grid: 19 of 25 for r = k = 5"""
    h = k // 2
    return sum(1 for i in range(r) for d in range(-h, h + 1) if 0 <= i + d < r)


def child(args):
    sys.path.insert(0, ab_bench.ROOT)
    import numpy as np
    import torch
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
        res["ms"], res["max_memory_allocated_mb"] = ab_bench.timed(lambda: T.get_3dmfv(x, w, mu, sigma, flatten=False),
                                                                   args.warmup, args.steps)
        return ab_bench.emit(res)
    y = torch.from_numpy(synth_labels(args.batch, seed=1)).to(dev)
    net = Model(m.bind(gmm, device=dev), device=dev, seed=0).build(x)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)

    def step():
        opt.zero_grad(set_to_none=True)
        m.get_loss(net(x, is_training=True, bn_decay=0.9)[0], y).backward()
        opt.step()

    res["ms"], res["max_memory_allocated_mb"] = ab_bench.timed(step, args.warmup, args.steps)
    if native:
        for name, shape, ms in ab_bench.time_entry_points(step, ("pcops_fv3d_", "pcops_conv3d_"),
                                                          lambda name: 5 if name in CONVS else 3):
            rec = {"name": name, "shape": shape, "ms": ms}
            if name in CONVS:
                b, r, k, cin, cout = shape
                rec["valid_gflop"] = 2.0 * b * cin * cout * valid_pairs(r, k) ** 3 / 1e9
                rec["dense_gflop"] = 2.0 * b * cin * cout * (r * k) ** 3 / 1e9
                rec["tflops"] = rec["valid_gflop"] / rec["ms"]
                rec["peak_fraction"] = rec["tflops"] / PEAK_TF
            res["kernels"].append(rec)
    ab_bench.emit(res)


def configs(args):
    """(child argv, environment overlay, the record fields of the config) in run order"""
    return [(["--child", "--what", what, "--batch", str(b), "--points", str(n), "--gaussians", str(g), "--steps",
              str(args.steps), "--warmup", str(args.warmup)], {}, {"what": what, "batch": b, "points": n, "gaussians": g ** 3})
            for what, b, n, g in (("step", 64, 1024, 5), ("step", 64, 1024, 8), ("fv", 256, 2048, 8))]


def header(args):
    return ("# tools/bench_mfv3d.py: 3DmFV-Net, %d timed iterations (median), warmup %d, %d rounds of alternating child processes"
            % (args.steps, args.warmup, args.rounds))


def run_line(res, r, seconds):
    return ("%-4s B=%-3d N=%-4d K=%-3d %-6s round %d: %9.3f ms  peak %9.1f MB  (%.0f s)"
            % (res["what"], res["batch"], res["points"], res["gaussians"], "native" if res["native"] else "torch", r, res["ms"],
               res["max_memory_allocated_mb"], seconds))


def summarise(results, args):
    lines = []
    for _, _, key in configs(args):
        nat, ref = ab_bench.split_on_off(results, key)
        mn, mt = ab_bench.median(nat), ab_bench.median(ref)
        lines.append("%s B=%d N=%d K=%d: native %.3f ms, torch %.3f ms: torch / native %.2f; peak memory %.0f MB vs %.0f MB"
                     % (("training step" if key["what"] == "step" else "representation", key["batch"], key["points"],
                         key["gaussians"], mn, mt, mt / mn) + ab_bench.peak_mb(nat, ref)))
        if key["what"] == "step":
            lines.append("  3DmFV kernels of one native step (last round; convolutions on valid-tap FLOPs):")
            for k in nat[-1]["kernels"]:
                extra = ""
                if "tflops" in k:
                    extra = "  %7.3f of %7.3f GFLOP  %6.2f TF  %.3f of the fp32 matrix peak" % (
                        k["valid_gflop"], k["dense_gflop"], k["tflops"], k["peak_fraction"])
                lines.append("    %-20s %-24s %8.3f ms%s" % (k["name"], k["shape"], k["ms"], extra))
    return lines


def parent(args):
    report, results = ab_bench.Report(), []
    report.say(header(args))
    for argv, env, _ in configs(args):
        for r in range(args.rounds):
            for value in ("1", "0"):
                res, seconds = ab_bench.run_child(os.path.abspath(__file__), argv, dict(env, PCOPS_MFV_NATIVE=value),
                                                  args.child_timeout)
                results.append(res)
                report.say(run_line(res, r, seconds))
    for line in [""] + summarise(results, args):
        report.say(line)
    report.write(args.out, results)


def main(argv=None):
    p = argparse.ArgumentParser()
    ab_bench.add_common_args(p, steps=20, warmup=5)
    p.add_argument("--what", default="step", choices=["step", "fv"])
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--points", type=int, default=1024)
    p.add_argument("--gaussians", type=int, default=5, help="grid subdivisions per axis")
    args = p.parse_args(argv)
    child(args) if args.child else parent(args)


if __name__ == "__main__":
    main()
