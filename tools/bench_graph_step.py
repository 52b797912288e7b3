"""One training step replayed as a captured HIP graph (`--graph`, scanobjectnn_amd/captured_step.py) against the same step
issued eagerly, in alternating fresh child processes on the same GPU, for every family on the verified list at the
reference's own batch and cloud size, and for the flagship's GPU-bound configuration, where a tie is the expected outcome:

    python tools/bench_graph_step.py [--steps 10] [--warmup 3] [--rounds 2] [--out profiles/graph_step_ab.txt]

Per run: ms per step -- the median over `--steps` timed windows of `--inner` steps each between two device events --,
torch.cuda.max_memory_allocated over them and torch.cuda.memory_reserved after them (a replay allocates nothing, so the
graph side's peak counts only what lives outside the graph's pool: the memory it holds is the reserved figure), and what
one step dispatches from Python: aten operators that compute (views and shape bookkeeping left out) plus libpcops
calls.  The step is the trainer's: forward with training BN and dropout,
loss (with the model's regulariser where it has one), backward, gradient collection, Adam, the running sums; the input
copy into the static buffers and the one-element fill of Adam's step size are part of the graph side's step.  bn_decay
and lr are held fixed, so the graph side never re-captures inside the timed windows.  No ratio is fixed in advance: the
eager step in the same invocation is the yardstick, and a configuration where the graph loses shows as such.  Each child
runs under `--child_timeout`; a child that fails or outlasts it ends the run."""
import argparse
import importlib
import os
import sys

import ab_bench

# (model, batch, points): the reference trainers' own batch sizes (DESIGN.md sections 4.24-4.27), then the flagship's
# benchmark shape
CONFIGS = [("pointnet2_cls_ssg", 16, 1024), ("pointnet_cls", 32, 1024), ("dgcnn", 32, 1024), ("pointcnn_cls", 32, 1024),
           ("pointnet2_cls_ssg", 256, 2048)]


def child(args):
    sys.path.insert(0, ab_bench.ROOT)
    import torch
    from scanobjectnn_amd import captured_step as CS, train_util as TU
    from scanobjectnn_amd.graph import Model
    from scanobjectnn_amd.pointnet2 import evaluate_scenennobjects as EV, train as T
    from scanobjectnn_amd.synth import synth_clouds, synth_labels
    dev = torch.device("cuda", 0)
    b, n = args.batch, args.num_point
    targs = T.parse_args(["--model", args.model, "--batch_size", str(b), "--num_point", str(n)])
    assert CS.refusal(targs, 1, os.environ) is None
    mod = importlib.import_module(T.MODELS[args.model])
    x = torch.from_numpy(synth_clouds(b, n, seed=1)).to(dev)
    y = torch.from_numpy(synth_labels(b, seed=1)).to(dev).long()
    kw = {"num_class": targs.num_class} if targs.num_class != 15 else {}
    net = Model(T.model_fn(mod, targs, dev), device=dev, seed=0, **kw).build(x[:2])
    fp = TU.FlatParams(net)
    own = T.own_trainer(mod, targs)
    opt = TU.make_optimizer("adam", fp, **({"epsilon": own.adam_epsilon} if own else {}))
    scores = getattr(mod, "class_scores", lambda logits: logits)

    def body(x, y, m, bn_decay, tot, update):          # pointnet2/train.py's step of a classifier
        fp.begin_step()
        out = net(x, is_training=True, bn_decay=bn_decay)
        logits, end_points = EV.split_output(out)
        loss = EV.model_loss(mod, logits, y, end_points)
        (loss + own.regularization_loss(net) if own else loss).backward()
        fp.collect()
        update()
        with torch.no_grad():
            tot[0] += loss.detach()
            tot[1] += (scores(logits).argmax(dim=1) == y).sum()
            tot[2] += b

    lr, bn_decay = 0.001, 0.5
    if args.graph:
        cap = CS.CapturedStep(body, net, fp, opt, x, y)
        step = lambda: cap.step(x, y, None, lr, bn_decay)                              # noqa: E731
    else:
        tot = torch.zeros(3, dtype=torch.float64, device=dev)
        step = lambda: body(x, y, None, bn_decay, tot, lambda: opt.step(lr))           # noqa: E731
    res = {"model": args.model, "batch": b, "num_point": n, "on": bool(args.graph), "native": True}
    res["ms"], res["max_memory_allocated_mb"] = ab_bench.timed(step, args.warmup, args.steps, args.inner)
    res["reserved_mb"] = torch.cuda.memory_reserved() / 2 ** 20
    res["window_ms"] = res["ms"] * args.inner
    res["aten_ops"], res["pcops_calls"] = ab_bench.count_launches(step)
    res["captures"] = cap.captures if args.graph else 0
    ab_bench.emit(res)


def configs(args):
    return [(["--child", "--model", m, "--batch", str(b), "--num_point", str(n), "--steps", str(args.steps), "--warmup",
              str(args.warmup), "--inner", str(args.inner)], {"model": m, "batch": b, "num_point": n}) for m, b, n in CONFIGS]


def run_line(res, r, seconds):
    return ("%-18s B=%-3d N=%-4d %-5s round %d: %9.3f ms/step (windows of %5.0f ms)  peak %8.1f MB, reserved %8.1f MB  per "
            "step from Python: %4d aten + %4d pcops  (%.0f s)"
            % (res["model"], res["batch"], res["num_point"], "graph" if res["on"] else "eager", r, res["ms"], res["window_ms"],
               res["max_memory_allocated_mb"], res["reserved_mb"], res["aten_ops"], res["pcops_calls"], seconds))


def summarise(results, args):
    lines = []
    for _, key in configs(args):
        on, off = ab_bench.split_on_off(results, key)
        mg, me = ab_bench.median(on), ab_bench.median(off)
        spread = ab_bench.spread([r["ms"] for r in on], [r["ms"] for r in off])
        lines.append("%s B=%d N=%d: graph %.3f ms/step (rounds %s), eager %.3f ms/step (rounds %s): eager - graph = %.3f ms, "
                     "spread between rounds %.3f ms: %s; eager / graph %.2f; memory reserved %.0f MB vs %.0f MB; dispatched "
                     "from Python per step %d vs %d"
                     % ((key["model"], key["batch"], key["num_point"], mg, ab_bench.per_round(on), me,
                         ab_bench.per_round(off), me - mg, spread,
                         "more than the spread" if abs(me - mg) > spread else "within the spread", me / mg)
                        + (max(r["reserved_mb"] for r in on), max(r["reserved_mb"] for r in off))
                        + ab_bench.launches(on, off)))
    return lines


def parent(args):
    report, results = ab_bench.Report(), []
    report.say("# tools/bench_graph_step.py: one training step, captured graph against eager; ms per step = median of %d timed "
               "windows of %d steps each, %d rounds of alternating child processes.  Step times include the host's work."
               % (args.steps, args.inner, args.rounds))
    for argv, _ in configs(args):
        for r in range(args.rounds):
            for graph in ("0", "1"):
                res, seconds = ab_bench.run_child(os.path.abspath(__file__), argv + ["--graph", graph], {}, args.child_timeout)
                results.append(res)
                report.say(run_line(res, r, seconds))
    for line in [""] + summarise(results, args):
        report.say(line)
    report.write(args.out, results)


def main(argv=None):
    p = argparse.ArgumentParser()
    ab_bench.add_common_args(p, steps=10, warmup=3, windows=True)
    p.add_argument("--model", default="pointnet2_cls_ssg")
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--num_point", type=int, default=1024)
    p.add_argument("--graph", type=int, default=0, help="child: 1 replays the captured step, 0 issues it eagerly")
    p.add_argument("--inner", type=int, default=10, help="training steps per window")
    args = p.parse_args(argv)
    child(args) if args.child else parent(args)


if __name__ == "__main__":
    main()
