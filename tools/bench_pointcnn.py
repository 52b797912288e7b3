"""PointCNN (--model pointcnn_cls, setting modelnet_x3_l4; --model pointcnn_seg, setting object_dataset_x3) on the native
X-Conv contraction (PCOPS_XCONV_NATIVE=1) and on its dense torch form (=0: gather, cat, matmul, einsum), in alternating fresh
child processes on the same GPU:

  * one training step (forward, loss + regulariser, backward, Adam with the setting's epsilon) at N = 1024 with B = 32 (the
    setting's batch) and, for the classifier, B = 128;
  * the contractions of the model alone, forward + backward, at B = 32: the classifier's four X-Conv layers, or the five
    X-DeConv layers of pointcnn_seg;
  * pointcnn_seg only: the wide-channel path on and off (PCOPS_XCONV_GROUPS=1 / 0, both native) on the step and on xdconv_1
    and xdconv_2, the two layers beyond 256 channels.

    python tools/bench_pointcnn.py [--model pointcnn_seg] [--steps 10] [--warmup 3] [--rounds 2] [--out profiles/...txt]

Per run: ms per call -- the median over `--steps` timed windows, each window `--inner_step` steps or `--inner_layer` calls long
between two device events (a fraction of a second each), divided by its length --, torch.cuda.max_memory_allocated over them,
and the number of device launches a call issues, counted as dispatched aten operators that compute (views and shape bookkeeping
left out) plus libpcops calls.  These are CALL times: they include the host's launch work, and for the contractions alone (3-4
library launches against 9-17 aten launches of a few hundred microseconds in all) that is most of what they measure.  No ratio
is fixed in advance: the torch form in the same invocation is the yardstick, and a shape where the native kernel loses shows as
such.

KERNEL times come from a kernel trace in runs of their own, one per layer (never combined with counter collection):

    rocprofv3 --kernel-trace --stats -d DIR/layer<i> -o p --output-format csv -- \
        python tools/bench_pointcnn.py --child --what layer --layer <i> --steps 3 --warmup 2 --inner_layer 20
    python tools/bench_pointcnn.py --kernel_stats DIR [--out profiles/pointcnn_bench.txt]      (appends)

and for the wide path of pointcnn_seg one per layer (0, 1), option value and round, in DIR/layer<i>_g<0|1>_r<round>, the child
started with --model pointcnn_seg under PCOPS_XCONV_GROUPS=<0|1>; --kernel_stats DIR --model pointcnn_seg then sets the
forward and the data gradient (with its reduce pass) of both values side by side with the spread between the rounds.  It prints, per X-Conv kernel, calls, average and minimum time and the operand bytes it has to move (every operand once, the
gathered rows once per use) over the average time, beside the 8.0 TB/s HBM peak of the MI355X."""
import argparse
import os
import statistics
import sys

import ab_bench

# (n, p, K, c1, c2, dm) at N = 1024: the four X-Conv layers of modelnet_x3_l4, the five X-DeConv layers of object_dataset_x3
MODEL_LAYERS = {
    "pointcnn_cls": [(1024, 1024, 8, 24, 0, 4), (1024, 384, 12, 12, 48, 2), (384, 128, 16, 24, 96, 2),
                     (128, 128, 16, 48, 192, 2)],
    "pointcnn_seg": [(128, 128, 16, 96, 480, 1), (128, 128, 16, 96, 384, 1), (128, 384, 12, 48, 192, 1),
                     (384, 1024, 8, 24, 96, 1), (1024, 1024, 8, 12, 48, 1)],
}
SETTING = {"pointcnn_cls": "modelnet_x3_l4", "pointcnn_seg": "object_dataset_x3"}
WIDE_LAYERS = (0, 1)          # pointcnn_seg: xdconv_1 and xdconv_2 run in channel groups


def child(args):
    sys.path.insert(0, ab_bench.ROOT)
    import torch
    from scanobjectnn_amd import train_util as TU
    from scanobjectnn_amd.graph import Model
    import importlib
    from scanobjectnn_amd import _lib
    from scanobjectnn_amd.pointcnn import xconv_ops
    from scanobjectnn_amd.synth import synth_clouds, synth_labels, synth_masks
    m = importlib.import_module("scanobjectnn_amd.pointcnn." + args.model)
    dev = "cuda:0"
    native = xconv_ops.native_enabled()
    res = {"what": args.what, "native": native, "batch": args.batch, "layer": args.layer,
           "groups": _lib.get_option(_lib.OPT_XCONV_CHANNEL_GROUPS)}
    if args.what == "layer":
        n, p, k, c1, c2, dm = MODEL_LAYERS[args.model][args.layer]
        g = torch.Generator().manual_seed(args.layer)
        b = args.batch
        lifted = torch.randn(b, p, k, c1, generator=g).to(dev).requires_grad_(True)
        fts = torch.randn(b, n, c2, generator=g).to(dev).requires_grad_(True) if c2 else None
        idx = torch.randint(0, n, (b, p, k), generator=g, dtype=torch.int32).to(dev) if c2 else None
        X = torch.randn(b, p, k, k, generator=g).to(dev).requires_grad_(True)
        wd = torch.randn(k, c1 + c2, dm, generator=g).to(dev).requires_grad_(True)
        dout = torch.randn(b, p, (c1 + c2) * dm, generator=g).to(dev)
        leaves = [t for t in (lifted, fts, X, wd) if t is not None]

        def step():
            for t in leaves:
                t.grad = None
            xconv_ops.xconv_contract(lifted, fts, idx, X, wd).backward(dout)
    else:
        x = torch.from_numpy(synth_clouds(args.batch, 1024, seed=1)).to(dev)
        y = torch.from_numpy(synth_labels(args.batch, seed=1)).to(dev)
        net = Model(m.get_model, device=dev, seed=0).build(x)
        fp = TU.FlatParams(net)
        from scanobjectnn_amd.pointcnn import pointcnn_cls
        own = pointcnn_cls.trainer(argparse.Namespace(setting=SETTING[args.model]))
        opt = TU.make_optimizer("adam", fp, epsilon=own.adam_epsilon)
        if args.model == "pointcnn_seg":
            mask = torch.from_numpy(synth_masks(args.batch, 1024, 1)).to(dev).long()

            def loss_of(out):
                return m.get_loss(out[0], out[1], y, mask)[0]
        else:
            def loss_of(out):
                return m.get_loss(out, y)

        def step():
            fp.begin_step()
            loss = loss_of(net(x, is_training=True))
            (loss + own.regularization_loss(net)).backward()
            fp.collect()
            opt.step(own.learning_rate(0))

    inner = args.inner_layer if args.what == "layer" else args.inner_step
    res["ms"], res["max_memory_allocated_mb"] = ab_bench.timed(step, args.warmup, args.steps, inner)
    res["window_ms"] = res["ms"] * inner
    res["aten_ops"], res["pcops_calls"] = ab_bench.count_launches(step)
    ab_bench.emit(res)


def configs(args):
    """(child argv, environment overlay, the record fields of the config) in run order.  The last field names the switch
    that alternates: native against torch everywhere; pointcnn_seg also groups on / off, both native."""
    steps = [("step", 32, -1)] + ([("step", 128, -1)] if args.model == "pointcnn_cls" else [])
    runs = [c + ("PCOPS_XCONV_NATIVE",) for c in steps + [("layer", 32, i) for i in range(len(MODEL_LAYERS[args.model]))]]
    if args.model == "pointcnn_seg":
        runs += [c + ("PCOPS_XCONV_GROUPS",) for c in steps + [("layer", 32, i) for i in WIDE_LAYERS]]
    return [(["--child", "--model", args.model, "--what", what, "--batch", str(b), "--layer", str(layer), "--steps",
              str(args.steps), "--warmup", str(args.warmup), "--inner_step", str(args.inner_step), "--inner_layer",
              str(args.inner_layer)], {"PCOPS_XCONV_NATIVE": "1", "PCOPS_XCONV_GROUPS": "1"},
             {"what": what, "batch": b, "layer": layer, "switch": switch}) for what, b, layer, switch in runs]


def header(args):
    return ("# tools/bench_pointcnn.py: PointCNN %s %s, N = 1024; ms per call = median of %d timed windows of %d steps / "
            "%d contraction calls each, %d rounds of alternating child processes.  Call times include the host's launch work."
            % (args.model, SETTING[args.model], args.steps, args.inner_step, args.inner_layer, args.rounds))


def run_line(res, r, seconds, args):
    return ("%-5s B=%-3d %-28s %-10s round %d: %9.3f ms (windows of %4.0f ms)  peak %8.1f MB  launches %4d aten + %3d "
            "pcops  (%.0f s)"
            % (res["what"], res["batch"], "" if res["layer"] < 0 else str(MODEL_LAYERS[args.model][res["layer"]]),
               _label(res["switch"], res["on"]), r, res["ms"], res["window_ms"], res["max_memory_allocated_mb"],
               res["aten_ops"], res["pcops_calls"], seconds))


def summarise(results, args):
    lines = []
    for _, _, key in configs(args):
        on, off = ab_bench.split_on_off(results, key)
        mn, mt = ab_bench.median(on), ab_bench.median(off)
        label = "training step B=%d" % key["batch"] if key["what"] == "step" else \
            "contraction fwd+bwd CALL time incl. launches, B=%d (n, p, K, c1, c2, dm) = %s" % (
                key["batch"], MODEL_LAYERS[args.model][key["layer"]])
        lines.append("%s: %s %.3f ms (rounds %s), %s %.3f ms (rounds %s): ratio %.2f; peak memory %.0f MB vs %.0f MB; "
                     "launches %d vs %d"
                     % ((label, _label(key["switch"], True), mn, ab_bench.per_round(on), _label(key["switch"], False), mt,
                         ab_bench.per_round(off), mt / mn) + ab_bench.peak_mb(on, off) + ab_bench.launches(on, off)))
    return lines


def parent(args):
    report, results = ab_bench.Report(), []
    report.say(header(args))
    for argv, env, key in configs(args):
        for r in range(args.rounds):
            for value in ("1", "0"):
                res, seconds = ab_bench.run_child(os.path.abspath(__file__), argv, dict(env, **{key["switch"]: value}),
                                                  args.child_timeout)
                res["switch"], res["on"] = key["switch"], value == "1"
                results.append(res)
                report.say(run_line(res, r, seconds, args))
    for line in [""] + summarise(results, args):
        report.say(line)
    report.write(args.out, results)


def _label(switch, on):
    if switch == "PCOPS_XCONV_NATIVE":
        return "native" if on else "torch"
    return "groups" if on else "one group"


def operand_bytes(kernel, b, shape):
    """what one launch has to move: every operand once, the gathered fts rows once per use, the outputs once"""
    n, p, k, c1, c2, dm = shape
    P, c = b * p, c1 + c2
    reads = P * k * c + P * k * k + (P * k if c2 else 0)                 # lifted + gathered rows, X, idx
    if "fwd" in kernel:
        return 4 * (reads + k * c * dm + P * c * dm)
    if "dgrad" in kernel:
        return 4 * (reads + k * c * dm + P * c * dm + P * k * k + P * k * c)
    return 4 * (reads + P * c * dm)                                      # wgrad (its partial sums are small beside this)


def _trace_rows(directory, sub):
    """{short kernel name: (calls, average us, minimum us)} of the X-Conv kernels in the kernel trace under DIR/sub"""
    rows = {}
    for row in ab_bench.kernel_stats_rows(directory, sub, required=True):
        if "xconv" in row["Name"]:
            short = row["Name"].split("xconv_")[1].split("(")[0]
            rows[short] = (int(row["Calls"]), float(row["AverageNs"]) / 1e3, float(row["MinNs"]) / 1e3)
    return rows


def kernel_stats(args):
    """the X-Conv kernels of the traces under DIR/layer<i> (rocprofv3 --kernel-trace --stats, one run per layer)"""
    if args.model == "pointcnn_seg":
        return kernel_stats_groups(args)
    layers = MODEL_LAYERS[args.model]
    lines = ["", "# kernel times: rocprofv3 --kernel-trace --stats, one run per layer (B = %d); GB/s = operand bytes / average "
             "time, beside 8000 GB/s HBM peak" % args.batch]
    for layer in range(len(layers)):
        total = 0.0
        for short, (calls, avg, mn) in _trace_rows(args.kernel_stats, "layer%d" % layer).items():
            line = "layer %d %-28s xconv_%-32s calls %4d  avg %8.1f us  min %8.1f us" % (
                layer + 1, layers[layer], short, calls, avg, mn)
            if "reduce" not in short:
                gbs = operand_bytes(short, args.batch, layers[layer]) / (avg * 1e3)
                line += "  %7.1f MB  %6.0f GB/s  %.3f of peak" % (operand_bytes(short, args.batch, layers[layer]) / 1e6, gbs,
                                                                 gbs / 8000.0)
            total += avg
            lines.append(line)
        lines.append("layer %d: X-Conv kernels of one forward + backward %.1f us" % (layer + 1, total))
    ab_bench.Report.append(args.out, lines)


def _groups_verdict(layer, what, on, off, args):
    """one wide layer's kernel, average us per round with groups (on) and with one group (off)"""
    spread = ab_bench.spread(on, off)
    gain = statistics.mean(off) - statistics.mean(on)
    gbs = operand_bytes(what, args.batch, MODEL_LAYERS[args.model][layer]) / (statistics.mean(on) * 1e3)
    return ("xdconv_%d %-5s: groups %s us, one group %s us; one group - groups = %.1f us, spread between rounds "
            "%.1f us: %s; with groups %.0f GB/s, %.3f of the 8000 GB/s peak"
            % (layer + 1, what, " ".join("%.1f" % v for v in on), " ".join("%.1f" % v for v in off), gain, spread,
               "LOWER by more than the spread" if gain > spread else "NOT lower by more than the spread", gbs, gbs / 8000.0))


def kernel_stats_groups(args):
    """pointcnn_seg's wide layers under PCOPS_XCONV_GROUPS = 1 / 0: DIR/layer<i>_g<0|1>_r<round>, one trace each.  The data
    gradient with groups is its kernel plus the reduce pass over the groups' partial dX."""
    layers = MODEL_LAYERS[args.model]
    lines = ["", "# kernel times of the wide layers: rocprofv3 --kernel-trace --stats, one run per layer, option value and round "
             "(B = %d), average us per launch; dgrad with groups = its kernel + the reduce pass over the groups' dX" % args.batch]
    def one(rows, prefix):
        found = [v for k, v in rows.items() if k.startswith(prefix)]
        assert len(found) <= 1, sorted(rows)
        return found[0] if found else (0, 0.0, 0.0)

    for layer in WIDE_LAYERS:
        t = {("fwd", 1): [], ("fwd", 0): [], ("dgrad", 1): [], ("dgrad", 0): []}
        for r in range(args.rounds):
            rows = {g: _trace_rows(args.kernel_stats, "layer%d_g%d_r%d" % (layer, g, r)) for g in (1, 0)}
            # the reduce kernel also closes the weight gradient, with and without groups: what the groups add to its total
            # time, per data-gradient launch, is the data gradient's reduce pass
            red1, red0 = one(rows[1], "reduce_kernel"), one(rows[0], "reduce_kernel")
            extra = (red1[0] * red1[1] - red0[0] * red0[1]) / max(one(rows[1], "dgrad_kernel")[0], 1)
            for g in (1, 0):
                t[("fwd", g)].append(one(rows[g], "fwd_kernel")[1])
                t[("dgrad", g)].append(one(rows[g], "dgrad_kernel")[1] + (extra if g else 0.0))
                for short, (calls, avg, mn) in sorted(rows[g].items()):
                    lines.append("xdconv_%d %-26s groups=%d round %d xconv_%-30s calls %4d  avg %8.1f us  min %8.1f us"
                                 % (layer + 1, layers[layer], g, r, short, calls, avg, mn))
            lines.append("xdconv_%d round %d: the reduce pass over the groups' dX: %.1f us per data gradient" % (layer + 1, r, extra))
        for what in ("fwd", "dgrad"):
            lines.append(_groups_verdict(layer, what, t[(what, 1)], t[(what, 0)], args))
    ab_bench.Report.append(args.out, lines)


def main(argv=None):
    p = argparse.ArgumentParser()
    ab_bench.add_common_args(p, steps=10, warmup=3, windows=True)
    p.add_argument("--model", default="pointcnn_cls", choices=sorted(MODEL_LAYERS))
    p.add_argument("--what", default="step", choices=["step", "layer"])
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--layer", type=int, default=-1)
    p.add_argument("--inner_step", type=int, default=10, help="training steps per window")
    p.add_argument("--inner_layer", type=int, default=500, help="contraction calls per window")
    p.add_argument("--kernel_stats", default="", help="directory of per-layer rocprofv3 kernel traces to summarise")
    args = p.parse_args(argv)
    if args.kernel_stats:
        kernel_stats(args)
    else:
        child(args) if args.child else parent(args)


if __name__ == "__main__":
    main()
