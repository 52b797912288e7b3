"""One SpiderCNN training step (forward, cross entropy, backward, Adam) at N = 1024 on the SpiderConv kernels
(PCOPS_SPIDER_NATIVE=1) and on the dense torch form (=0), in alternating fresh child processes on the same GPU.

    python tools/bench_spidercnn.py [--batches 16 64] [--steps 20] [--warmup 5] [--rounds 2] [--out profiles/spidercnn_bench.txt]

Per run: ms/step (median of the timed steps), clouds/s, torch.cuda.max_memory_allocated over the timed steps; native
runs also time every spider entry point of one extra step (HIP events around each launch) and price each contraction
kernel (2 P K O FLOP, K = k C T) against the 157.3 TF fp32 matrix peak of the MI355X."""
import argparse
import os
import sys

import ab_bench

PEAK_TF = 157.3
CONTRACTIONS = ("pcops_spider_conv_fwd", "pcops_spider_conv_wgrad", "pcops_spider_conv_dgrad")


def child(args):
    sys.path.insert(0, ab_bench.ROOT)
    import torch
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

    ms, peak = ab_bench.timed(step, args.warmup, args.steps)
    res = {"native": os.environ.get("PCOPS_SPIDER_NATIVE", "1") != "0", "batch": args.batch, "ms_per_step": ms,
           "clouds_per_s": args.batch / ms * 1e3, "max_memory_allocated_mb": peak, "kernels": []}
    if res["native"]:
        def shape_len(name):
            return 6 if name.startswith("pcops_spider_conv") else 4 if name.startswith("pcops_group_norm") else 2
        for name, shape, launch_ms in ab_bench.time_entry_points(step, ("pcops_spider_", "pcops_group_norm_relu_"), shape_len):
            rec = {"name": name, "shape": shape, "ms": launch_ms}
            if name in CONTRACTIONS:
                b, n, c, k, t, o = shape
                flop = 2.0 * b * n * k * c * t * o
                rec["tflops"] = flop / rec["ms"] / 1e9
                rec["peak_fraction"] = rec["tflops"] / PEAK_TF
            res["kernels"].append(rec)
    ab_bench.emit(res)


def configs(args):
    """(child argv, environment overlay, the record fields of the config) in run order"""
    return [(["--child", "--batch", str(b), "--steps", str(args.steps), "--warmup", str(args.warmup)], {}, {"batch": b})
            for b in args.batches]


def header(args):
    return ("# tools/bench_spidercnn.py: SpiderCNN training step, N = 1024, steps %d (median), warmup %d, %d rounds of "
            "alternating child processes" % (args.steps, args.warmup, args.rounds))


def run_line(res, r, seconds):
    return ("B=%-3d %-6s round %d: %8.2f ms/step %9.1f clouds/s  peak %8.1f MB  (%.0f s)"
            % (res["batch"], "native" if res["native"] else "torch", r, res["ms_per_step"], res["clouds_per_s"],
               res["max_memory_allocated_mb"], seconds))


def summarise(results, args):
    lines = []
    for _, _, key in configs(args):
        nat, ref = ab_bench.split_on_off(results, key)
        b, mn, mt = key["batch"], ab_bench.median(nat, "ms_per_step"), ab_bench.median(ref, "ms_per_step")
        lines.append("B=%d: native %.2f ms/step (%.1f clouds/s), torch %.2f ms/step (%.1f clouds/s): speed-up %.2fx; peak memory "
                     "%.0f MB vs %.0f MB" % ((b, mn, b / mn * 1e3, mt, b / mt * 1e3, mt / mn) + ab_bench.peak_mb(nat, ref)))
        lines.append("  spider kernels of one native step (last round):")
        for k in nat[-1]["kernels"]:
            extra = "  %6.1f TF  %.3f of the fp32 matrix peak" % (k["tflops"], k["peak_fraction"]) if "tflops" in k else ""
            lines.append("    %-32s %-28s %8.3f ms%s" % (k["name"], k["shape"], k["ms"], extra))
    return lines


def parent(args):
    report, results = ab_bench.Report(), []
    report.say(header(args))
    for argv, env, _ in configs(args):
        for r in range(args.rounds):
            for value in ("1", "0"):
                res, seconds = ab_bench.run_child(os.path.abspath(__file__), argv, dict(env, PCOPS_SPIDER_NATIVE=value),
                                                  args.child_timeout)
                results.append(res)
                report.say(run_line(res, r, seconds))
    for line in [""] + summarise(results, args):
        report.say(line)
    report.write(args.out, results)


def main(argv=None):
    p = argparse.ArgumentParser()
    ab_bench.add_common_args(p, steps=20, warmup=5)
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--batches", type=int, nargs="+", default=[16, 64])
    args = p.parse_args(argv)
    child(args) if args.child else parent(args)


if __name__ == "__main__":
    main()
