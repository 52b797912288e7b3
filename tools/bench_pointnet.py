"""PointNet (--model pointnet_cls) on the native per-cloud feature transform and regulariser (PCOPS_POINTNET_NATIVE=1,
csrc/tnet.hip) and on their torch forms (=0: a batched library GEMM forward and two backward; one batched product, four
elementwise launches and their backward), in alternating fresh child processes on the same GPU:

  * one training step (forward, loss with the regulariser, backward, Adam) at B = 32, N = 1024 (the reference's batch) and
    at B = 256, N = 2048;
  * the launchers alone at both sizes: the transform forward + backward against torch.matmul forward + backward, and the
    regulariser with its gradient against the torch expression with its backward.

    python tools/bench_pointnet.py [--steps 10] [--warmup 3] [--rounds 2] [--out profiles/pointnet_bench.txt]

Per run: ms per call -- the median over `--steps` timed windows, each `--inner_step` steps or `--inner_op` calls long between
two device events, divided by its length --, torch.cuda.max_memory_allocated over them, and the number of device launches a
call issues, counted as dispatched aten operators that compute (views and shape bookkeeping left out) plus libpcops calls.
These are CALL times: they include the host's launch work.  No ratio is fixed in advance: the torch form in the same
invocation is the yardstick, and a size where the native kernel loses shows as such.

KERNEL times come from a kernel trace in runs of their own, one per size and form (never combined with counter collection):

    PCOPS_POINTNET_NATIVE=<1|0> rocprofv3 --kernel-trace --stats -d DIR/<what>_b<B>_n<N>_native<1|0> -o p --output-format csv \
        -- python tools/bench_pointnet.py --child --what <transform|ortho> --batch B --num_point N --steps 3 --warmup 2 --inner_op 20
    python tools/bench_pointnet.py --kernel_stats DIR [--out profiles/pointnet_bench.txt]      (appends)"""
import argparse
import os
import sys

import ab_bench

SIZES = [(32, 1024), (256, 2048)]
LABEL = {"step": "training step", "transform": "transform fwd+bwd CALL time incl. launches",
         "ortho": "regulariser + gradient CALL time incl. launches"}


def child(args):
    sys.path.insert(0, ab_bench.ROOT)
    import torch
    from scanobjectnn_amd import train_util as TU
    from scanobjectnn_amd.graph import Model
    from scanobjectnn_amd.pointnet import pointnet_cls as m, tnet_ops
    from scanobjectnn_amd.synth import synth_clouds, synth_labels
    dev = "cuda:0"
    b, n = args.batch, args.num_point
    res = {"what": args.what, "native": tnet_ops.native_enabled(), "batch": b, "num_point": n}
    g = torch.Generator().manual_seed(b + n)
    if args.what == "transform":
        x = torch.randn(b, n, 64, generator=g).to(dev).requires_grad_(True)
        t = (torch.randn(b, 64, 64, generator=g) / 8).to(dev).requires_grad_(True)
        dout = torch.randn(b, n, 64, generator=g).to(dev)

        def step():
            x.grad = t.grad = None
            tnet_ops.apply_feature_transform(x, t).backward(dout)
    elif args.what == "ortho":
        q, _ = torch.linalg.qr(torch.randn(b, 64, 64, generator=g))
        t = (q + 1e-2 * torch.randn(b, 64, 64, generator=g)).to(dev).requires_grad_(True)

        def step():
            t.grad = None
            tnet_ops.ortho_regulariser(t, 0.001).backward()
    else:
        x = torch.from_numpy(synth_clouds(b, n, seed=1)).to(dev)
        y = torch.from_numpy(synth_labels(b, seed=1)).to(dev)
        net = Model(m.get_model, device=dev, seed=0).build(x)
        fp = TU.FlatParams(net)
        opt = TU.make_optimizer("adam", fp)

        def step():
            fp.begin_step()
            logits, end_points = net(x, is_training=True, bn_decay=0.5)
            m.get_loss(logits, y, end_points).backward()
            fp.collect()
            opt.step(0.001)

    inner = args.inner_step if args.what == "step" else args.inner_op
    res["ms"], res["max_memory_allocated_mb"] = ab_bench.timed(step, args.warmup, args.steps, inner)
    res["window_ms"] = res["ms"] * inner
    res["aten_ops"], res["pcops_calls"] = ab_bench.count_launches(step)
    ab_bench.emit(res)


def configs(args):
    """(child argv, environment overlay, the record fields of the config) in run order"""
    return [(["--child", "--what", what, "--batch", str(b), "--num_point", str(n), "--steps", str(args.steps), "--warmup",
              str(args.warmup), "--inner_step", str(args.inner_step), "--inner_op", str(args.inner_op)], {},
             {"what": what, "batch": b, "num_point": n}) for what in ("step", "transform", "ortho") for b, n in SIZES]


def header(args):
    return ("# tools/bench_pointnet.py: pointnet_cls; ms per call = median of %d timed windows of %d steps / %d launcher calls "
            "each, %d rounds of alternating child processes.  Call times include the host's launch work."
            % (args.steps, args.inner_step, args.inner_op, args.rounds))


def run_line(res, r, seconds):
    return ("%-9s B=%-3d N=%-4d %-6s round %d: %9.3f ms (windows of %4.0f ms)  peak %8.1f MB  launches %4d aten + %3d "
            "pcops  (%.0f s)" % (res["what"], res["batch"], res["num_point"], "native" if res["native"] else "torch", r,
                                 res["ms"], res["window_ms"], res["max_memory_allocated_mb"], res["aten_ops"],
                                 res["pcops_calls"], seconds))


def summarise(results, args):
    lines = []
    for _, _, key in configs(args):
        on, off = ab_bench.split_on_off(results, key)
        mn, mt = ab_bench.median(on), ab_bench.median(off)
        spread = ab_bench.spread([r["ms"] for r in on], [r["ms"] for r in off])
        lines.append("%s B=%d N=%d: native %.3f ms (rounds %s), torch %.3f ms (rounds %s): torch - native = %.3f ms, spread "
                     "between rounds %.3f ms: %s; ratio %.2f; peak memory %.0f MB vs %.0f MB; launches %d vs %d"
                     % ((LABEL[key["what"]], key["batch"], key["num_point"], mn, ab_bench.per_round(on), mt,
                         ab_bench.per_round(off), mt - mn, spread,
                         "more than the spread" if abs(mt - mn) > spread else "within the spread", mt / mn)
                        + ab_bench.peak_mb(on, off) + ab_bench.launches(on, off)))
    return lines


def parent(args):
    report, results = ab_bench.Report(), []
    report.say(header(args))
    for argv, env, _ in configs(args):
        for r in range(args.rounds):
            for value in ("1", "0"):
                res, seconds = ab_bench.run_child(os.path.abspath(__file__), argv, dict(env, PCOPS_POINTNET_NATIVE=value),
                                                  args.child_timeout)
                results.append(res)
                report.say(run_line(res, r, seconds))
    for line in [""] + summarise(results, args):
        report.say(line)
    report.write(args.out, results)


def kernel_stats(args):
    """every kernel of the trace under DIR/<run> (rocprofv3 --kernel-trace --stats, one run per size and form) that takes
    part in the transform or the regulariser: calls, average and minimum time, and the sum per call of the step"""
    lines = ["", "# kernel times: rocprofv3 --kernel-trace --stats, one run per launcher, size and form; us per launch.  The "
             "transform moves 3 b n 256 bytes forward + backward reads and 2 b n 256 bytes of writes."]
    for run in sorted(os.listdir(args.kernel_stats)):
        rows = [(r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:90], int(r["Calls"]),
                 float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3,
                 float(r["TotalDurationNs"]) / 1e3) for r in ab_bench.kernel_stats_rows(args.kernel_stats, run)]
        if not rows:
            continue
        calls = max(c for _, c, _, _, _ in rows)
        rows = [r for r in rows if r[1] * 4 >= calls]                     # the kernels of the timed loop, not of the setup
        for name, c, avg, mn, _ in rows:
            lines.append("%-34s %-90s calls %5d  avg %8.1f us  min %8.1f us" % (run, name, c, avg, mn))
        lines.append("%-34s all of the above per call of the loop: %.1f us" % (run, sum(r[4] for r in rows) / calls))
    ab_bench.Report.append(args.out, lines)


def main(argv=None):
    p = argparse.ArgumentParser()
    ab_bench.add_common_args(p, steps=10, warmup=3, windows=True)
    p.add_argument("--what", default="step", choices=["step", "transform", "ortho"])
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--num_point", type=int, default=1024)
    p.add_argument("--inner_step", type=int, default=10, help="training steps per window")
    p.add_argument("--inner_op", type=int, default=200, help="launcher calls per window")
    p.add_argument("--kernel_stats", default="", help="directory of rocprofv3 kernel traces to summarise")
    args = p.parse_args(argv)
    if args.kernel_stats:
        kernel_stats(args)
    else:
        child(args) if args.child else parent(args)


if __name__ == "__main__":
    main()
