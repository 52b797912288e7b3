"""`--graph` on the GPU (scanobjectnn_amd/captured_step.py): the Adam launch that reads its step size from device memory
gives the bits of the by-value launch; a captured run of every verified family is held to its eager run; a replay issues
no libpcops call from Python; a re-capture gives the previous graph's memory back; the trainer's flag end to end."""
import importlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from scanobjectnn_amd.synth import synth_clouds, synth_labels

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
GUARD = 64                # floats on either side of every buffer
SWEEP = 4096 * 256 * 4    # floats one sweep of the launch's largest grid covers: beyond it the kernel strides


# ------------------------------------------------------------------------------- 1. pcops_adam_step_dev == pcops_adam_step
@pytest.mark.parametrize("n", [4, 1028, SWEEP + 1028])
def test_adam_step_dev_gives_the_bits_of_adam_step(n):
    """three consecutive steps with three step sizes on the same gradients: p, m, v equal bit for bit, and the guard band
    on either side of every buffer of the device-lr launch keeps its fill"""
    from scanobjectnn_amd import _lib
    g = torch.Generator().manual_seed(n)

    def padded(values, fill):
        buf = torch.full((GUARD + n + GUARD,), fill, dtype=torch.float32, device=DEV)
        buf[GUARD:GUARD + n] = values.to(DEV)
        return buf

    p0, grads = torch.randn(n, generator=g), [torch.randn(n, generator=g) * (10.0 ** (k - 2)) for k in range(3)]
    sets = [[padded(p0, 7.0), padded(torch.zeros(n), -3.0), padded(torch.zeros(n), 5.0)] for _ in range(2)]
    lr_dev = torch.full((1 + 2 * GUARD,), 9.0, dtype=torch.float32, device=DEV)
    view = lambda t: t[GUARD:GUARD + n]                                    # noqa: E731
    for t, lr in enumerate((1e-3, 7e-4, 3.3e-2), start=1):
        lr_t = float(np.float32(lr * math.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)))
        grad = padded(grads[t - 1], 11.0)
        (pa, ma, va), (pb, mb, vb) = sets
        _lib.call("pcops_adam_step", n, view(pa).data_ptr(), view(grad).data_ptr(), view(ma).data_ptr(), view(va).data_ptr(),
                  0.9, 0.999, lr_t, 1e-8)
        lr_dev[GUARD:GUARD + 1].fill_(lr_t)
        _lib.call("pcops_adam_step_dev", n, view(pb).data_ptr(), view(grad).data_ptr(), view(mb).data_ptr(),
                  view(vb).data_ptr(), 0.9, 0.999, lr_dev[GUARD:].data_ptr(), 1e-8)
        for a, b, name in ((pa, pb, "p"), (ma, mb, "m"), (va, vb, "v")):
            assert torch.equal(view(a), view(b)), (name, t)
        assert torch.equal(grad[:GUARD], torch.full_like(grad[:GUARD], 11.0)) and torch.equal(view(grad).cpu(), grads[t - 1])
    assert not torch.equal(view(sets[1][0]).cpu(), p0)                       # the parameters did move
    for buf, fill in zip(sets[1], (7.0, -3.0, 5.0)):
        for band in (buf[:GUARD], buf[GUARD + n:]):
            assert torch.equal(band, torch.full_like(band, fill))
    assert torch.equal(lr_dev[:GUARD], torch.full_like(lr_dev[:GUARD], 9.0))
    assert torch.equal(lr_dev[GUARD + 1:], torch.full_like(lr_dev[GUARD + 1:], 9.0))


def test_a_launcher_that_clears_its_output_replays_as_it_runs():
    """pcops_group_point_grad clears its output and then adds into it with float atomics (the scatter-add of every
    family's backward pass outside --deterministic).  Captured and replayed three times into an output dirtied in
    between, and into a pool block that an earlier tensor of the same capture dirtied, it gives the eager result every
    time.  (As a memset node the clearing covered half the range from the second replay on: common.h pcops_zero_async.)
    Bar: the order of at most a handful of atomic float adds per destination, values of order 1 -- 1e-5 absolute."""
    from scanobjectnn_amd import _lib
    b, n, c, m, s = 8, 512, 48, 128, 8
    g = torch.Generator().manual_seed(0)
    idx = torch.randint(0, n, (b, m, s), generator=g, dtype=torch.int32).to(DEV)
    grad_out = torch.randn(b, m, s, c, generator=g).to(DEV)

    def scatter(out):
        _lib.call("pcops_group_point_grad", b, n, c, m, s, grad_out.data_ptr(), idx.data_ptr(), out.data_ptr())

    ref = torch.empty(b, n, c, device=DEV)
    scatter(ref)
    assert ref.abs().max().item() > 1.0
    outside, inside = torch.empty_like(ref), torch.empty_like(ref)
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(graph, stream=stream):
        scatter(outside)
        t = torch.empty_like(ref)
        t.fill_(7.0)
        del t
        out = torch.empty_like(ref)              # the block `t` just gave back
        scatter(out)
        inside.copy_(out)
        del out
    for replay in range(3):
        outside.fill_(5.0)
        graph.replay()
        torch.cuda.synchronize()
        for name, got in (("outside", outside), ("inside", inside)):
            assert (got - ref).abs().max().item() <= 1e-5, (name, replay)


# ------------------------------------------------------------------------------------ 2. captured against eager, per family
# the sizes of each family's own trainer test (test_models_gpu, test_pointcnn_gpu, test_pointnet_gpu); six steps in one
# epoch; decay_step = 3 batches, so that bn_decay goes 0.5 -> 0.75 at step 3: one re-capture in the middle of the run
FAMILIES = {
    "pointnet2_cls_ssg": ["--model", "pointnet2_cls_ssg", "--num_point", "512", "--batch_size", "8"],
    "dgcnn": ["--model", "dgcnn", "--num_point", "256", "--batch_size", "8"],
    "pointcnn_cls": ["--model", "pointcnn_cls", "--setting", "modelnet_x3_l4", "--num_point", "512", "--batch_size", "8"],
    "pointnet_cls": ["--model", "pointnet_cls", "--num_point", "256", "--batch_size", "16"],
    "pointnet2_cls_ssg-momentum": ["--model", "pointnet2_cls_ssg", "--num_point", "512", "--batch_size", "8",
                                   "--optimizer", "momentum"],
}


def _run(flags, tmp_path, graph):
    from scanobjectnn_amd.pointnet2 import train as T
    batch = int(flags[flags.index("--batch_size") + 1])
    args = T.parse_args(flags + ["--max_epoch", "1", "--synthetic_clouds", str(6 * batch), "--decay_step", str(3 * batch),
                                 "--deterministic", "--log_dir", str(tmp_path)] + (["--graph"] if graph else []))
    state = {}
    log = T.train(args, state)
    assert len(log) == 1 and log[0]["graph"] is graph and np.isfinite(log[0]["mean_loss"])
    opt = state["opt"]
    out = {"flat": state["fp"].flat, "tot": state["tot"]}
    out.update({"opt." + k: getattr(opt, k) for k in ("m", "v", "accum") if hasattr(opt, k)})
    out.update({"buffer." + k: v for k, v in state["net"].named_buffers()})
    assert any(k.endswith(("moving_mean", "pop_mean")) for k in out)
    return {k: v.detach().clone() for k, v in out.items()}, log[0], getattr(opt, "t", None)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_captured_run_is_the_eager_run(family, tmp_path, monkeypatch):
    """flat parameters, optimiser moments, every BN moving buffer and the epoch's running sums after six steps, --graph
    against eager.  The yardstick is the eager run against itself: two eager runs are compared first, and the captured run
    may differ from an eager run by no more than they differ from each other, tensor by tensor -- where they are equal,
    which is what --deterministic promises, the captured run has to pass torch.equal.  Dropout is patched out (a model's
    draws come from the device's default generator); the augmentation stays on: it runs outside the graph on the
    trainer's own generator.

    Measured on the MI355X, every family and the momentum case: the two eager runs' largest difference is 0 over all
    tensors (25 to 60 per family), so the bar for the captured run is equality, and it meets it (largest difference 0)."""
    from scanobjectnn_amd import _lib
    monkeypatch.setattr(torch.nn.functional, "dropout", lambda x, *a, **k: x)
    was = _lib.deterministic()
    try:
        e1, _, t1 = _run(FAMILIES[family], tmp_path, False)
        e2, _, _ = _run(FAMILIES[family], tmp_path, False)
        cap, rec, t2 = _run(FAMILIES[family], tmp_path, True)
    finally:
        _lib.set_deterministic(was)
    assert rec["captures"] == 2                    # step 0, and step 3 where bn_decay (and momentum's lr) moves
    assert t1 == t2                                # Adam's t kept counting on the host (None for momentum)
    assert set(e1) == set(e2) == set(cap)
    assert not torch.equal(e1["flat"], torch.zeros_like(e1["flat"])) and e1["tot"][2].item() == 6 * int(
        FAMILIES[family][FAMILIES[family].index("--batch_size") + 1])
    bars = {k: (e1[k].double() - e2[k].double()).abs().max().item() for k in e1}
    got = {k: (cap[k].double() - e1[k].double()).abs().max().item() for k in e1}
    print("%s: eager against eager: largest difference %.3g (%d of %d tensors differ); captured against eager: %.3g"
          % (family, max(bars.values()), sum(b > 0 for b in bars.values()), len(bars), max(got.values())))
    for k in sorted(e1):
        assert got[k] <= bars[k], (k, got[k], bars[k])
        if bars[k] == 0.0:
            assert torch.equal(cap[k], e1[k]), k


# -------------------------------------------------------------------------------- 3 / 4. the captured step on its own
def _pieces(batch=16, num_point=256):
    from scanobjectnn_amd import captured_step as CS, train_util as TU
    from scanobjectnn_amd.graph import Model
    mod = importlib.import_module("scanobjectnn_amd.pointnet.pointnet_cls")
    x = torch.from_numpy(synth_clouds(batch, num_point, seed=3)).to(DEV)
    y = torch.from_numpy(synth_labels(batch, seed=3)).to(DEV)
    net = Model(mod.get_model, device=DEV, seed=0).build(x)
    fp = TU.FlatParams(net)
    opt = TU.make_optimizer("adam", fp)

    def body(x, y, m, bn_decay, tot, update):
        fp.begin_step()
        logits, end_points = net(x, is_training=True, bn_decay=bn_decay)
        loss = mod.get_loss(logits, y, end_points)
        loss.backward()
        fp.collect()
        update()
        with torch.no_grad():
            tot[0] += loss.detach()
            tot[2] += x.shape[0]
    return CS.CapturedStep(body, net, fp, opt, x, y), body, opt, x, y


def _count_pcops_calls(fn):
    from scanobjectnn_amd import _lib
    count = [0]

    def hook(name, phase, args):
        count[0] += phase == "pre"
    _lib._hooks.append(hook)
    try:
        fn()
    finally:
        _lib._hooks.remove(hook)
    return count[0]


def test_replay_issues_no_libpcops_call_from_python():
    """three steady-state steps of the captured step (dropout on: its draws are part of the graph): no libpcops call leaves
    Python, where the eager step of the same model issues its launches one by one"""
    cap, body, opt, x, y = _pieces()
    tot = torch.zeros(3, dtype=torch.float64, device=DEV)
    eager = _count_pcops_calls(lambda: body(x, y, None, 0.5, tot, lambda: opt.step(0.001)))
    assert eager > 0
    first = _count_pcops_calls(lambda: cap.step(x, y, None, 0.001, 0.5))         # warm-up and capture: eager launches
    assert first > 0 and cap.captures == 1
    before = cap.fp.flat.clone()
    steady = _count_pcops_calls(lambda: [cap.step(x, y, None, lr, 0.5) for lr in (0.001, 0.001, 0.0007)])
    assert steady == 0 and cap.captures == 1
    assert opt.t == 5 and cap.tot[2].item() == 4 * x.shape[0]                     # one eager step, four captured ones
    assert torch.isfinite(cap.tot[0]).item() and not torch.equal(before, cap.fp.flat)
    cap.release()


def test_recapture_gives_the_previous_pool_back():
    """four captures (bn_decay 0.5, 0.75, 0.875, 0.9375) with replays in between: what the allocator holds after the third
    re-capture is what it held after the first, within 1 MB"""
    cap, _, _, x, y = _pieces()
    reserved = []
    for decay in (0.5, 0.75, 0.875, 0.9375):
        cap.step(x, y, None, 0.001, decay)
        reserved.append(torch.cuda.memory_reserved())
        cap.step(x, y, None, 0.001, decay)
    torch.cuda.synchronize()
    assert cap.captures == 4
    print("memory reserved after each capture (MB): %s" % ["%.1f" % (r / 2 ** 20) for r in reserved])
    assert reserved[3] <= reserved[1] + 2 ** 20
    cap.release()


# ------------------------------------------------------------------------------------------ 5. the trainer, end to end
def _train_child(extra, log_dir, env=None):
    out = subprocess.run([sys.executable, "-m", "scanobjectnn_amd.pointnet2.train", "--graph", "--model", "pointcnn_cls",
                          "--setting", "modelnet_x3_l4", "--num_point", "512", "--batch_size", "8", "--synthetic_clouds",
                          "16", "--log_dir", log_dir] + extra, cwd=ROOT, env=dict(os.environ, **(env or {})),
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    return lines, [json.loads(l) for l in lines if l.startswith("{")]


def test_trainer_with_graph_end_to_end(tmp_path):
    from scanobjectnn_amd.pointnet2 import evaluate_scenennobjects as EV
    log_dir = str(tmp_path / "log")
    lines, recs = _train_child(["--max_epoch", "2"], log_dir)
    assert len(recs) == 2 and all(r["graph"] is True and r["captures"] >= 1 for r in recs), lines
    assert all(np.isfinite(r["mean_loss"]) and r["mean_loss"] > 0 for r in recs)
    assert not any("refused" in l for l in lines)
    ev = EV.evaluate(EV.parse_args(["--model", "pointcnn_cls", "--setting", "modelnet_x3_l4", "--num_point", "512",
                                    "--batch_size", "8", "--synthetic_clouds", "16", "--model_path",
                                    os.path.join(log_dir, "model.pt"), "--dump_dir", str(tmp_path / "dump")]))
    assert ev["pred"].shape == (16,) and 0.0 <= ev["accuracy"] <= 1.0
    # the same command under PCOPS_SYNC=1 says why it is not captured, in one line, and trains eagerly
    lines, recs = _train_child(["--max_epoch", "1"], str(tmp_path / "log_sync"), env={"PCOPS_SYNC": "1"})
    assert sum(l.startswith("--graph refused, training eagerly:") and "PCOPS_SYNC" in l for l in lines) == 1
    assert len(recs) == 1 and recs[0]["graph"] is False and recs[0]["captures"] == 0 and np.isfinite(recs[0]["mean_loss"])
