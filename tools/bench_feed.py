"""`--device_feed` (scanobjectnn_amd/device_feed.py, pcops_feed_batch) against the host-fed input side, in alternating fresh
child processes on the same GPU:

    python tools/bench_feed.py [--what view,step] [--rounds 2] [--out profiles/feed_ab.txt]

(a) view: seconds per epoch spent building the epoch's view of a synthetic RAGGED set (`--clouds` objects, sizes spread
    evenly over `--min_size` .. `--max_size` points, `--num_point` taken of each): `data_utils.get_current_data` on the host
    plus the upload, as `train.epoch_view` does it, against `DeviceFeed.begin_epoch` + `epoch_view`.  Median over `--steps`
    epochs, the device synchronised at the end of each.
(b) step: ms per training step INCLUDING its input side, with and without the feed, issued eagerly and replayed as a
    captured graph (`--graph`), for the trainer's step of `pointnet2_cls_ssg` at B = 16 and `dgcnn` at B = 32, N = 1024.
    Without the feed the input side is the trainer's: slice the epoch's view, rotate + jitter on the trainer's generator,
    contiguous, (graph: copy into the static inputs); with it: four integers into device memory and one launch (graph: the
    launch is part of the replay).  Median of `--steps` windows of `--inner` steps.

No number is fixed in advance: the host-fed side of the same invocation is the yardstick, a difference counts only beyond
the spread between rounds, and a configuration where the feed gains nothing shows as such.  Each child runs under
`--child_timeout`; a child that fails or outlasts it ends the run."""
import argparse
import importlib
import os
import sys
import time

import ab_bench

STEP_CONFIGS = [("pointnet2_cls_ssg", 16, 1024), ("dgcnn", 32, 1024)]


def ragged_set(clouds, lo, hi, seed=0):
    """`clouds` objects of lo .. hi points (evenly spread, shuffled), coordinates uniform in the unit cube: views of one array"""
    import numpy as np
    rng = np.random.default_rng(seed)
    sizes = np.linspace(lo, hi, clouds).astype(np.int64)
    rng.shuffle(sizes)
    flat = rng.random((int(sizes.sum()), 3), dtype=np.float32)
    ends = np.cumsum(sizes)
    return [flat[e - s:e] for s, e in zip(sizes, ends)], rng.integers(0, 15, clouds)


def child_view(args):
    import numpy as np
    import torch
    from scanobjectnn_amd import data_utils, device_feed as DF
    dev = torch.device("cuda", 0)
    data, labels = ragged_set(args.clouds, args.min_size, args.max_size)
    rng = np.random.RandomState(0)
    if args.feed:
        feed = DF.DeviceFeed(data, labels, None, args.num_point, 1, 1, 0, DF.NO_CONSTS, dev)

        def view(epoch):
            feed.begin_epoch(rng, epoch)
            return feed.epoch_view()[0]
    else:
        def view(epoch):
            cur, lab = data_utils.get_current_data(data, labels, args.num_point, rng=rng)
            x = torch.as_tensor(cur, dtype=torch.float32, device=dev)
            torch.as_tensor(lab.astype(np.int64), device=dev)
            return x
    times = []
    for epoch in range(args.warmup + args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = view(epoch)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    assert tuple(x.shape) == (args.clouds, args.num_point, 3)
    times = sorted(times[args.warmup:])
    ab_bench.emit({"what": "view", "on": bool(args.feed), "native": True, "clouds": args.clouds, "num_point": args.num_point,
                   "points": int(sum(pc.shape[0] for pc in data)), "ms": 1e3 * times[len(times) // 2],
                   "epochs_ms": [1e3 * t for t in times]})


def child_step(args):
    import numpy as np
    import torch
    from scanobjectnn_amd import captured_step as CS, device_feed as DF, provider, train_util as TU
    from scanobjectnn_amd.graph import Model
    from scanobjectnn_amd.pointnet2 import evaluate_scenennobjects as EV, train as T
    from scanobjectnn_amd.synth import synth_clouds, synth_labels
    dev = torch.device("cuda", 0)
    b, n = args.batch, args.num_point
    targs = T.parse_args(["--model", args.model, "--batch_size", str(b), "--num_point", str(n)] +
                         (["--device_feed"] if args.feed else []))
    assert CS.refusal(targs, 1, os.environ) is None
    mod = importlib.import_module(T.MODELS[args.model])
    assert DF.refusal(targs, mod, None, "cuda") is None
    nb = 8                                                        # batches of the epoch the steps walk round
    data, lab, _ = T.prepare_set(synth_clouds(nb * b, 2048, seed=1), synth_labels(nb * b, seed=1), None, targs, dev)
    net = Model(T.model_fn(mod, targs, dev), device=dev, seed=0).build(data[:2, :n].contiguous())
    fp = TU.FlatParams(net)
    opt = TU.make_optimizer("adam", fp)
    rng = np.random.RandomState(0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000)

    def body(x, y, m, bn_decay, tot, update):                     # pointnet2/train.py's step of a classifier
        fp.begin_step()
        logits, end_points = EV.split_output(net(x, is_training=True, bn_decay=bn_decay))
        loss = EV.model_loss(mod, logits, y, end_points)
        loss.backward()
        fp.collect()
        update()
        with torch.no_grad():
            tot[0] += loss.detach()
            tot[1] += (logits.argmax(dim=1) == y).sum()
            tot[2] += b

    lr, bn_decay, count = 0.001, 0.5, [0]
    tot = torch.zeros(3, dtype=torch.float64, device=dev)
    if args.feed:
        recipe, consts = DF.recipe_of(targs, mod)
        feed = DF.DeviceFeed(data, lab, None, n, b, 1000, recipe, consts, dev)
        feed.begin_epoch(rng, 0)
        cap = CS.CapturedStep(body, net, fp, opt, None, None, None, feed=feed) if args.graph else None

        def step():
            i = count[0]
            count[0] += 1
            if cap is not None:
                cap.step(None, None, None, lr, bn_decay, batch=((i % nb) * b, i))
            else:
                feed.set_batch((i % nb) * b, i)
                body(*feed.launch(), bn_decay, tot, lambda: opt.step(lr))
    else:
        cur, cl, _ = T.epoch_view(data, lab, None, n, rng, dev)
        cap = CS.CapturedStep(body, net, fp, opt, cur[:b], cl[:b]) if args.graph else None

        def step():
            i = count[0]
            count[0] += 1
            sl = slice((i % nb) * b, (i % nb) * b + b)
            x = provider.jitter_point_cloud(provider.rotate_point_cloud(cur[sl], generator=gen), generator=gen).contiguous()
            if cap is not None:
                cap.step(x, cl[sl], None, lr, bn_decay)
            else:
                body(x, cl[sl], None, bn_decay, tot, lambda: opt.step(lr))
    res = {"what": "step", "model": args.model, "batch": b, "num_point": n, "graph": bool(args.graph), "on": bool(args.feed),
           "native": True}
    res["ms"], res["max_memory_allocated_mb"] = ab_bench.timed(step, args.warmup, args.steps, args.inner)
    torch.cuda.synchronize()
    t0 = time.perf_counter()                                      # what the host takes to ISSUE a step, the device running behind
    for _ in range(3 * args.inner):
        step()
    res["host_issue_ms"] = 1e3 * (time.perf_counter() - t0) / (3 * args.inner)
    torch.cuda.synchronize()
    res["aten_ops"], res["pcops_calls"] = ab_bench.count_launches(step)
    ab_bench.emit(res)


def view_key(args):
    return {"what": "view", "clouds": args.clouds, "num_point": args.num_point}


def step_keys():
    return [{"what": "step", "model": m, "batch": b, "num_point": n, "graph": g} for m, b, n in STEP_CONFIGS for g in (False, True)]


def summarise(results, args):
    lines = []
    if any(r["what"] == "view" for r in results):
        on, off = ab_bench.split_on_off(results, view_key(args))
        mo, mf = ab_bench.median(on), ab_bench.median(off)
        spread = ab_bench.spread([r["ms"] for r in on], [r["ms"] for r in off])
        lines.append("epoch view of %d ragged clouds (%.0f M points), %d points each: host %.1f ms per epoch (rounds %s), feed "
                     "%.1f ms per epoch (rounds %s): host - feed = %.1f ms, spread between rounds %.1f ms: %s; host / feed %.1f"
                     % (args.clouds, on[0]["points"] / 1e6, args.num_point, mf, ab_bench.per_round(off), mo,
                        ab_bench.per_round(on), mf - mo, spread,
                        "more than the spread" if abs(mf - mo) > spread else "within the spread", mf / mo))
    for key in step_keys():
        on, off = ab_bench.split_on_off(results, key)
        if not on or not off:
            continue
        mo, mf = ab_bench.median(on), ab_bench.median(off)
        spread = ab_bench.spread([r["ms"] for r in on], [r["ms"] for r in off])
        lines.append("%s B=%d N=%d %s: host-fed %.3f ms/step (rounds %s), --device_feed %.3f ms/step (rounds %s): host-fed - "
                     "feed = %.3f ms, spread between rounds %.3f ms: %s; dispatched from Python per step %d vs %d"
                     % ((key["model"], key["batch"], key["num_point"], "--graph" if key["graph"] else "eager", mf,
                         ab_bench.per_round(off), mo, ab_bench.per_round(on), mf - mo, spread,
                         "more than the spread" if abs(mf - mo) > spread else "within the spread")
                        + tuple(reversed(ab_bench.launches(on, off)))))
    return lines


def parent(args):
    report, results = ab_bench.Report(), []
    what = args.what.split(",")
    report.say("# tools/bench_feed.py: --device_feed against the host-fed input side, %d rounds of alternating child processes.  "
               "view: ms per epoch, median of %d epochs, host clock around a synchronised device.  step: ms per step with its "
               "input side, median of %d windows of %d steps between device events." % (args.rounds, args.steps, args.steps, args.inner))
    script = os.path.abspath(__file__)
    common = ["--child", "--steps", str(args.steps), "--warmup", str(args.warmup), "--inner", str(args.inner)]
    if "view" in what:
        argv = common + ["--what", "view", "--clouds", str(args.clouds), "--min_size", str(args.min_size), "--max_size",
                         str(args.max_size), "--num_point", str(args.num_point)]
        for r in range(args.rounds):
            for feed in ("0", "1"):
                res, seconds = ab_bench.run_child(script, argv + ["--feed", feed], {}, args.child_timeout)
                results.append(res)
                report.say("view  %-5s round %d: %9.1f ms per epoch (epochs %s)  (%.0f s)"
                           % ("feed" if res["on"] else "host", r, res["ms"], " ".join("%.1f" % t for t in res["epochs_ms"]), seconds))
    if "step" in what:
        for m, b, n in STEP_CONFIGS:
            for graph in ("0", "1"):
                argv = common + ["--what", "step", "--model", m, "--batch", str(b), "--num_point", str(n), "--graph", graph]
                for r in range(args.rounds):
                    for feed in ("0", "1"):
                        res, seconds = ab_bench.run_child(script, argv + ["--feed", feed], {}, args.child_timeout)
                        results.append(res)
                        report.say("step  %-18s B=%-3d N=%-4d %-5s %-8s round %d: %9.3f ms/step (the host issues one in %6.3f ms)  "
                                   "per step from Python: %4d aten + %4d pcops  (%.0f s)"
                                   % (m, b, n, "graph" if res["graph"] else "eager", "feed" if res["on"] else "host-fed", r,
                                      res["ms"], res["host_issue_ms"], res["aten_ops"], res["pcops_calls"], seconds))
    for line in [""] + summarise(results, args):
        report.say(line)
    report.write(args.out, results)


def main(argv=None):
    p = argparse.ArgumentParser()
    ab_bench.add_common_args(p, steps=5, warmup=1, windows=True)
    p.add_argument("--what", default="view,step", help="parent: the measurements to take; child: the one to run")
    p.add_argument("--feed", type=int, default=0, help="child: 1 the device feed, 0 the host-fed path")
    p.add_argument("--graph", type=int, default=0, help="child (step): 1 replays the captured step, 0 issues it eagerly")
    p.add_argument("--model", default="pointnet2_cls_ssg")
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--num_point", type=int, default=1024)
    p.add_argument("--inner", type=int, default=10, help="step: training steps per window")
    p.add_argument("--clouds", type=int, default=2300, help="view: objects of the ragged set")
    p.add_argument("--min_size", type=int, default=20000)
    p.add_argument("--max_size", type=int, default=150000)
    args = p.parse_args(argv)
    if not args.child:
        return parent(args)
    sys.path.insert(0, ab_bench.ROOT)
    child_view(args) if args.what == "view" else child_step(args)


if __name__ == "__main__":
    main()
