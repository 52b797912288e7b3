"""One SpiderCNN training step (forward, cross entropy, backward, Adam) at N = 1024 on the SpiderConv kernels
(PCOPS_SPIDER_NATIVE=1) and on the dense torch form (=0), in alternating fresh child processes on the same GPU.

    python tools/bench_spidercnn.py [--batches 16 64] [--steps 20] [--warmup 5] [--rounds 2] [--out profiles/spidercnn_bench.txt]

Per run: ms/step (median of the timed steps), clouds/s, torch.cuda.max_memory_allocated over the timed steps; native
runs also time every spider entry point of one extra step (HIP events around each launch) and price each contraction
kernel (2 P K O FLOP, K = k C T) against the 157.3 TF fp32 matrix peak of the MI355X."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_TF = 157.3
CONTRACTIONS = ("pcops_spider_conv_fwd", "pcops_spider_conv_wgrad", "pcops_spider_conv_dgrad")


def child(args):
    sys.path.insert(0, ROOT)
    import torch
    from scanobjectnn_amd import _lib
    from scanobjectnn_amd.graph import Model
    from scanobjectnn_amd.spidercnn import spidercnn_cls_xyz as m
    from scanobjectnn_amd.synth import synth_clouds, synth_labels
    dev = "cuda:0"
    x = torch.from_numpy(synth_clouds(args.batch, 1024, seed=1)).to(dev)
    y = torch.from_numpy(synth_labels(args.batch, seed=1)).to(dev)
    net = Model(m.get_model, device=dev, seed=0).build(x)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)

    def step():
        opt.zero_grad(set_to_none=True)
        m.get_loss(net(x, is_training=True, bn_decay=0.9), y).backward()
        opt.step()

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    ms = statistics.median(times)
    res = {"native": os.environ.get("PCOPS_SPIDER_NATIVE", "1") != "0", "batch": args.batch, "ms_per_step": ms,
           "clouds_per_s": args.batch / ms * 1e3, "max_memory_allocated_mb": torch.cuda.max_memory_allocated() / 2 ** 20,
           "kernels": []}
    if res["native"]:
        calls = []

        def hook(name, phase, a):
            if not name.startswith(("pcops_spider_", "pcops_group_norm_relu_")):
                return
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            if phase == "pre":
                nint = 6 if name.startswith("pcops_spider_conv") else 4 if name.startswith("pcops_group_norm") else 2
                calls.append([name, a[:nint], ev, None])
            else:
                calls[-1][3] = ev
        _lib._hooks.append(hook)
        step()
        torch.cuda.synchronize()
        _lib._hooks.remove(hook)
        for name, shape, e0, e1 in calls:
            rec = {"name": name, "shape": [int(v) for v in shape], "ms": e0.elapsed_time(e1)}
            if name in CONTRACTIONS:
                b, n, c, k, t, o = rec["shape"]
                flop = 2.0 * b * n * k * c * t * o
                rec["tflops"] = flop / rec["ms"] / 1e9
                rec["peak_fraction"] = rec["tflops"] / PEAK_TF
            res["kernels"].append(rec)
    print("RESULT " + json.dumps(res), flush=True)


def parent(args):
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("# tools/bench_spidercnn.py: SpiderCNN training step, N = 1024, steps %d (median), warmup %d, %d rounds of "
        "alternating child processes" % (args.steps, args.warmup, args.rounds))
    for b in args.batches:
        for r in range(args.rounds):
            for native in ("1", "0"):
                env = dict(os.environ, PCOPS_SPIDER_NATIVE=native)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--batch", str(b), "--steps", str(args.steps),
                       "--warmup", str(args.warmup)]
                t0 = time.time()
                out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=args.child_timeout)
                if out.returncode != 0:
                    say("child B=%d native=%s failed (exit %d): %s" % (b, native, out.returncode, out.stderr[-2000:]))
                    raise SystemExit(1)
                res = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
                results.append(res)
                say("B=%-3d %-6s round %d: %8.2f ms/step %9.1f clouds/s  peak %8.1f MB  (%.0f s)"
                    % (b, "native" if res["native"] else "torch", r, res["ms_per_step"], res["clouds_per_s"],
                       res["max_memory_allocated_mb"], time.time() - t0))
    say("")
    for b in args.batches:
        nat = [r for r in results if r["batch"] == b and r["native"]]
        ref = [r for r in results if r["batch"] == b and not r["native"]]
        mn = statistics.median(r["ms_per_step"] for r in nat)
        mt = statistics.median(r["ms_per_step"] for r in ref)
        say("B=%d: native %.2f ms/step (%.1f clouds/s), torch %.2f ms/step (%.1f clouds/s): speed-up %.2fx; peak memory "
            "%.0f MB vs %.0f MB" % (b, mn, b / mn * 1e3, mt, b / mt * 1e3, mt / mn,
                                    max(r["max_memory_allocated_mb"] for r in nat),
                                    max(r["max_memory_allocated_mb"] for r in ref)))
        say("  spider kernels of one native step (last round):")
        for k in nat[-1]["kernels"]:
            extra = "  %6.1f TF  %.3f of the fp32 matrix peak" % (k["tflops"], k["peak_fraction"]) if "tflops" in k else ""
            say("    %-32s %-28s %8.3f ms%s" % (k["name"], k["shape"], k["ms"], extra))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
            f.write("# raw\n" + "\n".join(json.dumps(r) for r in results) + "\n")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--child", action="store_true")
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--batches", type=int, nargs="+", default=[16, 64])
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--rounds", type=int, default=2)
    p.add_argument("--child_timeout", type=int, default=300)
    p.add_argument("--out", default="")
    args = p.parse_args()
    child(args) if args.child else parent(args)


if __name__ == "__main__":
    main()
