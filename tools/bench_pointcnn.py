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
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (n, p, K, c1, c2, dm) at N = 1024: the four X-Conv layers of modelnet_x3_l4, the five X-DeConv layers of object_dataset_x3
MODEL_LAYERS = {
    "pointcnn_cls": [(1024, 1024, 8, 24, 0, 4), (1024, 384, 12, 12, 48, 2), (384, 128, 16, 24, 96, 2),
                     (128, 128, 16, 48, 192, 2)],
    "pointcnn_seg": [(128, 128, 16, 96, 480, 1), (128, 128, 16, 96, 384, 1), (128, 384, 12, 48, 192, 1),
                     (384, 1024, 8, 24, 96, 1), (1024, 1024, 8, 12, 48, 1)],
}
SETTING = {"pointcnn_cls": "modelnet_x3_l4", "pointcnn_seg": "object_dataset_x3"}
WIDE_LAYERS = (0, 1)          # pointcnn_seg: xdconv_1 and xdconv_2 run in channel groups
VIEWS = {"view", "reshape", "detach", "alias", "expand", "slice", "select", "t", "transpose", "unsqueeze", "squeeze",
         "as_strided", "empty", "empty_like", "empty_strided", "_unsafe_view", "permute", "split", "unbind", "narrow",
         "set_", "lift_fresh", "sym_size", "sym_stride", "sym_numel", "sym_storage_offset", "is_same_size", "new_empty"}


def _timed(fn, warmup, steps, inner):
    """median over `steps` windows of `inner` calls each, per call"""
    import torch
    for _ in range(warmup * inner):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / inner)
    return statistics.median(times), torch.cuda.max_memory_allocated() / 2 ** 20


def _count_launches(fn):
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode
    from scanobjectnn_amd import _lib
    count = [0, 0]

    class Log(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if str(func).split(".")[1] not in VIEWS:
                count[0] += 1
            return func(*args, **(kwargs or {}))

    def hook(name, phase, a):
        if phase == "pre":
            count[1] += 1
    _lib._hooks.append(hook)
    try:
        with torch.autograd.set_multithreading_enabled(False), Log():       # backward runs under the mode too
            fn()
    finally:
        _lib._hooks.remove(hook)
    torch.cuda.synchronize()
    return count


def child(args):
    sys.path.insert(0, ROOT)
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
    res["ms"], res["max_memory_allocated_mb"] = _timed(step, args.warmup, args.steps, inner)
    res["window_ms"] = res["ms"] * inner
    res["aten_ops"], res["pcops_calls"] = _count_launches(step)
    print("RESULT " + json.dumps(res), flush=True)


def parent(args):
    lines, results = [], []
    layers = MODEL_LAYERS[args.model]

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("# tools/bench_pointcnn.py: PointCNN %s %s, N = 1024; ms per call = median of %d timed windows of %d steps / "
        "%d contraction calls each, %d rounds of alternating child processes.  Call times include the host's launch work."
        % (args.model, SETTING[args.model], args.steps, args.inner_step, args.inner_layer, args.rounds))
    # (what, batch, layer, the switch that alternates): native against torch everywhere; pointcnn_seg also groups on / off
    steps = [("step", 32, -1)] + ([("step", 128, -1)] if args.model == "pointcnn_cls" else [])
    configs = [c + ("PCOPS_XCONV_NATIVE",) for c in steps + [("layer", 32, i) for i in range(len(layers))]]
    if args.model == "pointcnn_seg":
        configs += [c + ("PCOPS_XCONV_GROUPS",) for c in steps + [("layer", 32, i) for i in WIDE_LAYERS]]
    for what, b, layer, switch in configs:
        for r in range(args.rounds):
            for value in ("1", "0"):
                env = dict(os.environ, PCOPS_XCONV_NATIVE="1", PCOPS_XCONV_GROUPS="1")
                env[switch] = value
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--model", args.model, "--what", what, "--batch",
                       str(b), "--layer", str(layer), "--steps", str(args.steps), "--warmup", str(args.warmup),
                       "--inner_step", str(args.inner_step), "--inner_layer", str(args.inner_layer)]
                t0 = time.time()
                out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=args.child_timeout)
                if out.returncode != 0:
                    say("child %s B=%d layer %d %s=%s failed (exit %d): %s" % (what, b, layer, switch, value, out.returncode,
                                                                              out.stderr[-2000:]))
                    raise SystemExit(1)
                res = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
                res["switch"], res["on"] = switch, value == "1"
                results.append(res)
                say("%-5s B=%-3d %-28s %-10s round %d: %9.3f ms (windows of %4.0f ms)  peak %8.1f MB  launches %4d aten + %3d "
                    "pcops  (%.0f s)"
                    % (what, b, "" if layer < 0 else str(layers[layer]), _label(switch, value == "1"), r, res["ms"],
                       res["window_ms"], res["max_memory_allocated_mb"], res["aten_ops"], res["pcops_calls"],
                       time.time() - t0))
    say("")
    for what, b, layer, switch in configs:
        sel = [r for r in results if (r["what"], r["batch"], r["layer"], r["switch"]) == (what, b, layer, switch)]
        on, off = [r for r in sel if r["on"]], [r for r in sel if not r["on"]]
        mn, mt = statistics.median(r["ms"] for r in on), statistics.median(r["ms"] for r in off)
        label = "training step B=%d" % b if what == "step" else \
            "contraction fwd+bwd CALL time incl. launches, B=%d (n, p, K, c1, c2, dm) = %s" % (b, layers[layer])
        say("%s: %s %.3f ms (rounds %s), %s %.3f ms (rounds %s): ratio %.2f; peak memory %.0f MB vs %.0f MB; launches %d vs %d"
            % (label, _label(switch, True), mn, " ".join("%.3f" % r["ms"] for r in on), _label(switch, False), mt,
               " ".join("%.3f" % r["ms"] for r in off), mt / mn, max(r["max_memory_allocated_mb"] for r in on),
               max(r["max_memory_allocated_mb"] for r in off), on[-1]["aten_ops"] + on[-1]["pcops_calls"],
               off[-1]["aten_ops"] + off[-1]["pcops_calls"]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
            f.write("# raw\n" + "\n".join(json.dumps(r) for r in results) + "\n")


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
    """{short kernel name: (calls, average us, minimum us)} of the X-Conv kernels of DIR/sub/**/*kernel_stats.csv"""
    import csv
    import glob
    files = sorted(glob.glob(os.path.join(directory, sub, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        raise SystemExit("no kernel_stats.csv under %s/%s" % (directory, sub))
    rows = {}
    for row in csv.DictReader(open(files[-1])):
        if "xconv" in row["Name"]:
            short = row["Name"].split("xconv_")[1].split("(")[0]
            rows[short] = (int(row["Calls"]), float(row["AverageNs"]) / 1e3, float(row["MinNs"]) / 1e3)
    return rows


def kernel_stats(args):
    """the X-Conv kernels of DIR/layer<i>/**/*kernel_stats.csv (rocprofv3 --kernel-trace --stats, one run per layer)"""
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
    print("\n".join(lines))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


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
            on, off = t[(what, 1)], t[(what, 0)]
            spread = max(max(on) - min(on), max(off) - min(off))
            gain = statistics.mean(off) - statistics.mean(on)
            gbs = operand_bytes(what, args.batch, layers[layer]) / (statistics.mean(on) * 1e3)
            lines.append("xdconv_%d %-5s: groups %s us, one group %s us; one group - groups = %.1f us, spread between rounds "
                         "%.1f us: %s; with groups %.0f GB/s, %.3f of the 8000 GB/s peak"
                         % (layer + 1, what, " ".join("%.1f" % v for v in on), " ".join("%.1f" % v for v in off), gain, spread,
                            "LOWER by more than the spread" if gain > spread else "NOT lower by more than the spread", gbs,
                            gbs / 8000.0))
    print("\n".join(lines))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--child", action="store_true")
    p.add_argument("--model", default="pointcnn_cls", choices=sorted(MODEL_LAYERS))
    p.add_argument("--what", default="step", choices=["step", "layer"])
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--layer", type=int, default=-1)
    p.add_argument("--steps", type=int, default=10, help="timed windows per run")
    p.add_argument("--warmup", type=int, default=3, help="untimed windows first")
    p.add_argument("--inner_step", type=int, default=10, help="training steps per window")
    p.add_argument("--inner_layer", type=int, default=500, help="contraction calls per window")
    p.add_argument("--kernel_stats", default="", help="directory of per-layer rocprofv3 kernel traces to summarise")
    p.add_argument("--rounds", type=int, default=2)
    p.add_argument("--child_timeout", type=int, default=300)
    p.add_argument("--out", default="")
    args = p.parse_args()
    if args.kernel_stats:
        kernel_stats(args)
    else:
        child(args) if args.child else parent(args)


if __name__ == "__main__":
    main()
