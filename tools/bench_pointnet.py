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
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(32, 1024), (256, 2048)]
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
    res["ms"], res["max_memory_allocated_mb"] = _timed(step, args.warmup, args.steps, inner)
    res["window_ms"] = res["ms"] * inner
    res["aten_ops"], res["pcops_calls"] = _count_launches(step)
    print("RESULT " + json.dumps(res), flush=True)


def parent(args):
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("# tools/bench_pointnet.py: pointnet_cls; ms per call = median of %d timed windows of %d steps / %d launcher calls "
        "each, %d rounds of alternating child processes.  Call times include the host's launch work."
        % (args.steps, args.inner_step, args.inner_op, args.rounds))
    configs = [(what, b, n) for what in ("step", "transform", "ortho") for b, n in SIZES]
    for what, b, n in configs:
        for r in range(args.rounds):
            for value in ("1", "0"):
                env = dict(os.environ, PCOPS_POINTNET_NATIVE=value)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--what", what, "--batch", str(b), "--num_point",
                       str(n), "--steps", str(args.steps), "--warmup", str(args.warmup), "--inner_step", str(args.inner_step),
                       "--inner_op", str(args.inner_op)]
                t0 = time.time()
                out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=args.child_timeout)
                if out.returncode != 0:
                    say("child %s B=%d N=%d native=%s failed (exit %d): %s" % (what, b, n, value, out.returncode,
                                                                              out.stderr[-2000:]))
                    raise SystemExit(1)
                res = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
                results.append(res)
                say("%-9s B=%-3d N=%-4d %-6s round %d: %9.3f ms (windows of %4.0f ms)  peak %8.1f MB  launches %4d aten + %3d "
                    "pcops  (%.0f s)" % (what, b, n, "native" if res["native"] else "torch", r, res["ms"], res["window_ms"],
                                         res["max_memory_allocated_mb"], res["aten_ops"], res["pcops_calls"], time.time() - t0))
    say("")
    label = {"step": "training step", "transform": "transform fwd+bwd CALL time incl. launches",
             "ortho": "regulariser + gradient CALL time incl. launches"}
    for what, b, n in configs:
        sel = [r for r in results if (r["what"], r["batch"], r["num_point"]) == (what, b, n)]
        on, off = [r for r in sel if r["native"]], [r for r in sel if not r["native"]]
        mn, mt = statistics.median(r["ms"] for r in on), statistics.median(r["ms"] for r in off)
        spread = max(max(r["ms"] for r in on) - min(r["ms"] for r in on), max(r["ms"] for r in off) - min(r["ms"] for r in off))
        say("%s B=%d N=%d: native %.3f ms (rounds %s), torch %.3f ms (rounds %s): torch - native = %.3f ms, spread between "
            "rounds %.3f ms: %s; ratio %.2f; peak memory %.0f MB vs %.0f MB; launches %d vs %d"
            % (label[what], b, n, mn, " ".join("%.3f" % r["ms"] for r in on), mt, " ".join("%.3f" % r["ms"] for r in off),
               mt - mn, spread, "more than the spread" if abs(mt - mn) > spread else "within the spread", mt / mn,
               max(r["max_memory_allocated_mb"] for r in on), max(r["max_memory_allocated_mb"] for r in off),
               on[-1]["aten_ops"] + on[-1]["pcops_calls"], off[-1]["aten_ops"] + off[-1]["pcops_calls"]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
            f.write("# raw\n" + "\n".join(json.dumps(r) for r in results) + "\n")


def kernel_stats(args):
    """every kernel of DIR/<run>/**/*kernel_stats.csv (rocprofv3 --kernel-trace --stats, one run per size and form) that takes
    part in the transform or the regulariser: calls, average and minimum time, and the sum per call of the step"""
    import csv
    import glob
    lines = ["", "# kernel times: rocprofv3 --kernel-trace --stats, one run per launcher, size and form; us per launch.  The "
             "transform moves 3 b n 256 bytes forward + backward reads and 2 b n 256 bytes of writes."]
    for run in sorted(os.listdir(args.kernel_stats)):
        files = sorted(glob.glob(os.path.join(args.kernel_stats, run, "**", "*kernel_stats.csv"), recursive=True))
        if not files:
            continue
        rows = [(r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:90], int(r["Calls"]),
                 float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3,
                 float(r["TotalDurationNs"]) / 1e3) for r in csv.DictReader(open(files[-1]))]
        calls = max(c for _, c, _, _, _ in rows)
        rows = [r for r in rows if r[1] * 4 >= calls]                     # the kernels of the timed loop, not of the setup
        for name, c, avg, mn, _ in rows:
            lines.append("%-34s %-90s calls %5d  avg %8.1f us  min %8.1f us" % (run, name, c, avg, mn))
        lines.append("%-34s all of the above per call of the loop: %.1f us" % (run, sum(r[4] for r in rows) / calls))
    print("\n".join(lines))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--child", action="store_true")
    p.add_argument("--what", default="step", choices=["step", "transform", "ortho"])
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--num_point", type=int, default=1024)
    p.add_argument("--steps", type=int, default=10, help="timed windows per run")
    p.add_argument("--warmup", type=int, default=3, help="untimed windows first")
    p.add_argument("--inner_step", type=int, default=10, help="training steps per window")
    p.add_argument("--inner_op", type=int, default=200, help="launcher calls per window")
    p.add_argument("--kernel_stats", default="", help="directory of rocprofv3 kernel traces to summarise")
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
