"""PointNet's mask model (--model pointnet_seg) with the first conv of its segmentation head on the fused per-cloud +
per-point kernels (PCOPS_CLOUD_POINT_FUSED=1, csrc/cloudpoint.hip: the 64-deep product inside the streaming pass, neither
Q = X Wx nor dQ in memory) and on the route that exists without them (=0: rows_linear for Q, then the cloud-bias arm of the
fused stack -- kernels the parent commit has), in alternating fresh child processes on the same GPU:

  * one training step (forward, loss with the regulariser, backward, Adam) at B = 32, N = 1024 (the reference's batch,
    pointnet/train_seg.py:33-35) and at B = 256, N = 2048;
  * the layer alone at both sizes: conv6..9 of the head, `seg_ops.conv2d_stack_point_cloud` forward + backward on a (B, N, 64)
    per-point input and a (B, 1024) per-cloud input that both take a gradient.

    python tools/bench_pointnet_seg.py [--steps 10] [--warmup 3] [--rounds 2] [--out profiles/pointnet_seg_bench.txt]

Per run: ms per call -- the median over `--steps` timed windows, each `--inner_step` steps or `--inner_op` calls long between
two device events, divided by its length --, torch.cuda.max_memory_allocated over them, and the number of device launches a
call issues, counted as dispatched aten operators that compute plus libpcops calls.  These are CALL times: they include the
host's launch work.  No ratio is fixed in advance: the =0 route in the same invocation is the yardstick, and a size where the
fused kernels lose shows as such.  The child times the route the switch selects whatever `seg_ops.POINT_FUSED_MIN_ROWS` says
(it sets the policy to 0), so that the policy can be decided from these numbers.

KERNEL times come from a kernel trace in runs of their own, one per size and route (never combined with counter collection):

    PCOPS_CLOUD_POINT_FUSED=<1|0> rocprofv3 --kernel-trace --stats -d DIR/layer_b<B>_n<N>_fused<1|0> -o p --output-format csv \
        -- python tools/bench_pointnet_seg.py --child --what layer --batch B --num_point N --steps 3 --warmup 2 --inner_op 10
    python tools/bench_pointnet_seg.py --kernel_stats DIR [--out profiles/pointnet_seg_bench.txt]      (appends)"""
import argparse
import os
import sys

import ab_bench

SIZES = [(32, 1024), (256, 2048)]
LABEL = {"step": "training step", "layer": "conv6..9 fwd+bwd CALL time incl. launches"}
WIDTHS = [512, 256, 128, 128]


def child(args):
    sys.path.insert(0, ab_bench.ROOT)
    import torch
    from scanobjectnn_amd import fused_mlp, train_util as TU
    from scanobjectnn_amd.graph import Model
    from scanobjectnn_amd.pointnet import pointnet_seg as m, seg_ops
    from scanobjectnn_amd.synth import synth_clouds, synth_labels, synth_masks
    dev = "cuda:0"
    b, n = args.batch, args.num_point
    seg_ops.POINT_FUSED_MIN_ROWS = 0          # the switch alone decides: what is measured is the kernels, not the policy
    res = {"what": args.what, "native": fused_mlp.CLOUD_POINT_FUSED, "batch": b, "num_point": n,
           "route": "cloud_point" if seg_ops.point_fused(b, n, 64, WIDTHS[0]) else "rows_linear + cloud_bias"}
    g = torch.Generator().manual_seed(b + n)
    if args.what == "layer":
        glob = torch.randn(b, 1024, generator=g).to(dev).requires_grad_(True)

        def head(point_feat, is_training, bn_decay=None):
            return seg_ops.conv2d_stack_point_cloud(point_feat, glob, WIDTHS, ['conv6', 'conv7', 'conv8', 'conv9'], is_training,
                                                    bn_decay)
        x = torch.randn(b, n, 64, generator=g).to(dev).requires_grad_(True)
        dout = torch.randn(b, n, 1, WIDTHS[-1], generator=g).to(dev)
        net = Model(head, device=dev, seed=0).build(x)

        def step():
            x.grad = glob.grad = None
            net.zero_grad(set_to_none=True)
            net(x, is_training=True, bn_decay=0.5).backward(dout)
    else:
        x = torch.from_numpy(synth_clouds(b, n, seed=1)).to(dev)
        y = torch.from_numpy(synth_labels(b, seed=1)).to(dev)
        mask = torch.from_numpy(synth_masks(b, n, 1)).to(dev)
        net = Model(m.get_model, device=dev, seed=0).build(x)
        fp = TU.FlatParams(net)
        opt = TU.make_optimizer("adam", fp)

        def step():
            fp.begin_step()
            class_pred, seg_pred, end_points = net(x, is_training=True, bn_decay=0.5)
            m.get_loss(class_pred, seg_pred, y, mask, end_points)[0].backward()
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
             {"what": what, "batch": b, "num_point": n}) for what in ("step", "layer") for b, n in SIZES]


def header(args):
    return ("# tools/bench_pointnet_seg.py: pointnet_seg; ms per call = median of %d timed windows of %d steps / %d layer calls "
            "each, %d rounds of alternating child processes.  Call times include the host's launch work."
            % (args.steps, args.inner_step, args.inner_op, args.rounds))


def run_line(res, r, seconds):
    return ("%-6s B=%-3d N=%-4d %-25s round %d: %9.3f ms (windows of %4.0f ms)  peak %8.1f MB  launches %4d aten + %3d "
            "pcops  (%.0f s)" % (res["what"], res["batch"], res["num_point"], res["route"], r, res["ms"], res["window_ms"],
                                 res["max_memory_allocated_mb"], res["aten_ops"], res["pcops_calls"], seconds))


def summarise(results, args):
    lines = []
    for _, _, key in configs(args):
        on, off = ab_bench.split_on_off(results, key)
        mn, mt = ab_bench.median(on), ab_bench.median(off)
        spread = ab_bench.spread([r["ms"] for r in on], [r["ms"] for r in off])
        lines.append("%s B=%d N=%d: fused %.3f ms (rounds %s), rows_linear + cloud_bias %.3f ms (rounds %s): unfused - fused = "
                     "%.3f ms, spread between rounds %.3f ms: %s; ratio %.2f; peak memory %.0f MB vs %.0f MB; launches %d vs %d"
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
                res, seconds = ab_bench.run_child(os.path.abspath(__file__), argv, dict(env, PCOPS_CLOUD_POINT_FUSED=value),
                                                  args.child_timeout)
                results.append(res)
                report.say(run_line(res, r, seconds))
    for line in [""] + summarise(results, args):
        report.say(line)
    report.write(args.out, results)


def kernel_stats(args):
    """every kernel of the trace under DIR/<run> (rocprofv3 --kernel-trace --stats, one run per size and route) that the timed
    loop launches: calls, average and minimum time; the sum per call of the loop; and the same sum over the kernels that only
    this route launches, `<what>_b<B>_n<N>_fused<1|0>` against its twin -- the first conv's own kernels, since everything else
    in the loop is shared"""
    lines = ["", "# kernel times: rocprofv3 --kernel-trace --stats, one run per size and route; us per launch.  Algorithmic bytes "
             "of the first conv at c = 512, rows = b n: fused forward rows (256 + 2048), fused backward rows (2 x 2048 + 2 x "
             "256); unfused forward rows (256 + 3 x 2048), unfused backward rows (2 x 2048 + 2048) + rows (2 x 2048 + 2 x 256)."]
    runs = {}
    for run in sorted(os.listdir(args.kernel_stats)):
        rows = [(r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:90], int(r["Calls"]),
                 float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3,
                 float(r["TotalDurationNs"]) / 1e3) for r in ab_bench.kernel_stats_rows(args.kernel_stats, run)]
        if rows:
            top = max(c for _, c, _, _, _ in rows)
            runs[run] = [r for r in rows if r[1] * 4 >= top]              # the kernels of the timed loop, not of the setup
    for run, rows in runs.items():
        twin = run[:-1] + ("0" if run.endswith("1") else "1")
        shared = {r[0] for r in runs.get(twin, [])}
        calls = min(r[1] for r in rows)               # every kernel of the loop runs at least once per call of it
        for name, c, avg, mn, _ in rows:
            lines.append("%-24s %-90s calls %5d  avg %8.1f us  min %8.1f us%s"
                         % (run, name, c, avg, mn, "" if name in shared else "  [this route only]"))
        lines.append("%-24s all of the above per call of the loop (%d calls): %.1f us; this route's own kernels: %.1f us"
                     % (run, calls, sum(r[4] for r in rows) / calls, sum(r[4] for r in rows if r[0] not in shared) / calls))
    ab_bench.Report.append(args.out, lines)


def main(argv=None):
    p = argparse.ArgumentParser()
    ab_bench.add_common_args(p, steps=10, warmup=3, windows=True)
    p.add_argument("--what", default="step", choices=["step", "layer"])
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--num_point", type=int, default=1024)
    p.add_argument("--inner_step", type=int, default=5, help="training steps per window")
    p.add_argument("--inner_op", type=int, default=10, help="layer calls per window")
    p.add_argument("--kernel_stats", default="", help="directory of rocprofv3 kernel traces to summarise")
    args = p.parse_args(argv)
    if args.kernel_stats:
        kernel_stats(args)
    else:
        child(args) if args.child else parent(args)


if __name__ == "__main__":
    main()
