"""PointNet's mask and part models on the GPU: the shared head (scanobjectnn_amd/pointnet/seg_ops.py) through autograd
against float64 at B = 2, N = 256; pointnet_seg and pointnet_partseg in eval mode against the float64 restatement of
tests/cloudpoint_ref.py (logits <= 1e-4); one training step of each against float64 with the model's own decisions imposed
(tests/pointnet_seg_step.py: every variable's gradient <= 1e-3 of its maximum, and the plan of the head's stack), in this
process and again with PCOPS_CLOUD_POINT_FUSED=0 in a child process; and the trainer with the evaluation command line of each
model on synthetic files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cloudpoint_checks as K
import cloudpoint_ref as R
import pointnet_seg_step as SS
from scanobjectnn_amd import _lib, fused_mlp
from scanobjectnn_amd.graph import Model
from scanobjectnn_amd.pointnet import pointnet_partseg, pointnet_seg, seg_ops
from scanobjectnn_amd.synth import synth_clouds, synth_labels, synth_masks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4


@pytest.fixture
def any_size(monkeypatch):
    """the fused first conv at every size the kernels take: the wrapper's size policy (seg_ops.POINT_FUSED_MIN_ROWS) is a
    matter of speed; these tests are about what the kernels compute"""
    monkeypatch.setattr(fused_mlp, "CLOUD_POINT_FUSED", True)
    monkeypatch.setattr(seg_ops, "POINT_FUSED_MIN_ROWS", 0)


def _calls(fn):
    seen = []
    hook = lambda name, phase, args: phase == "pre" and seen.append(name)       # noqa: E731
    _lib._hooks.append(hook)
    try:
        out = fn()
    finally:
        _lib._hooks.remove(hook)
    return out, seen


def test_layer_through_autograd(any_size):
    """conv6..9 on [per_point | per_cloud] at B = 2, N = 256 -- too few rows for the fused stack: the wrapper takes the plain
    layers -- and at B = 32 (8192 rows) on the fused kernels: output <= 1e-4 and every gradient <= 1e-3 of its maximum against
    float64 autograd of the CONCATENATED form (blocks of oracle/ref_models.py) with the run's own ReLU decisions imposed"""
    import decisions as DEC
    from oracle import ref_models as OR
    widths, scopes = [512, 256, 128, 128], ['conv6', 'conv7', 'conv8', 'conv9']
    for b, n, fused in ((2, 256, False), (32, 256, True)):
        g_ = K.gen("layer", b, n)
        pf = (0.5 * torch.randn(b, n, 64, generator=g_)).to(DEV).requires_grad_(True)
        gf = (0.5 * torch.randn(b, 1024, generator=g_)).to(DEV).requires_grad_(True)

        def head(x, is_training, bn_decay=None):
            return seg_ops.conv2d_stack_point_cloud(x, gf, widths, scopes, is_training, bn_decay)
        net = Model(head, device=DEV, seed=1).build(pf.detach())
        SS.PS.randomise(net, 3)
        sd = {k: v.clone() for k, v in net.state_dict().items()}
        rec = DEC.Recorder(net, DEV)
        with rec.recording():
            out, seen = _calls(lambda: net(pf, is_training=True, bn_decay=0.9))
        D = rec.decisions()
        assert out.shape == (b, n, 1, 128) and set(D.relu) == set(scopes)
        assert (seen.count("pcops_cloud_point_fwd") == 1) == fused
        gout = torch.randn(b, n, 1, 128, generator=g_).to(DEV)
        _, seen = _calls(lambda: out.backward(gout))
        assert (seen.count("pcops_cloud_point_bwd") == 1) == fused
        P = {k: v.requires_grad_(v.is_floating_point())
             for k, v in OR.params_from_state_dict(sd, dtype=torch.float64, device=DEV).items()}
        pf64, gf64 = pf.detach().double().requires_grad_(True), gf.detach().double().requires_grad_(True)
        with OR.imposing(D, None, {}):
            x64 = torch.cat([pf64, gf64.view(b, 1, 1024).expand(b, n, 1024)], dim=-1)
            for s in scopes:
                x64 = OR.dense(x64, P, s, True)
        want = x64.reshape(b, n, 1, 128)
        assert (out.double() - want).abs().max().item() <= TOL
        want.backward(gout.double())
        got = {k[len("graph."):]: p.grad for k, p in net.named_parameters()}
        assert tuple(got["conv6/weights"].shape) == (1, 1, 1088, 512)
        pairs = [("per_point", pf.grad, pf64.grad), ("per_cloud", gf.grad, gf64.grad)]
        pairs += [(k, got[k], P[k].grad) for k in got if not k.endswith("biases")]      # (a bias in front of a norm: zero)
        for name, g, ref in pairs:
            scale = ref.abs().max().item()
            assert scale > 1e-9, name
            assert (g.double() - ref).abs().max().item() <= SS.GRAD_TOL * scale, (name, b)


def _eval_net(m, seed):
    c = synth_clouds(8, 1024, seed=3)
    x = torch.from_numpy(c).to(DEV)
    net = Model(m.get_model, device=DEV, seed=seed).build(x)
    SS.PS.randomise(net, 5)
    return c, x, net


def test_eval_logits_against_float64(any_size):
    c, x, net = _eval_net(pointnet_seg, 1)
    P = R.params_from_state_dict(net.state_dict(), device=DEV)
    with torch.no_grad():
        (class_pred, seg_pred, end_points), seen = _calls(lambda: net(x, is_training=False))
        cp64, sp64, t64 = R.pointnet_seg(x.double(), P, False)
    assert seen.count("pcops_cloud_point_fwd") == 1 and "pcops_cloud_bias_fwd" not in seen
    assert class_pred.shape == (8, 15) and seg_pred.shape == (8, 1024, 2) and end_points["transform"].shape == (8, 64, 64)
    assert (class_pred.double() - cp64).abs().max().item() <= TOL
    assert (seg_pred.double() - sp64).abs().max().item() <= TOL
    assert (end_points["transform"].double() - t64).abs().max().item() <= TOL
    c, x, net = _eval_net(pointnet_partseg, 2)
    P = R.params_from_state_dict(net.state_dict(), device=DEV)
    with torch.no_grad():
        (seg_pred, end_points), seen = _calls(lambda: net(x, is_training=False))
        sp64, t64 = R.pointnet_partseg(x.double(), P, False)
    assert seen.count("pcops_cloud_point_fwd") == 1
    assert seg_pred.shape == (8, 1024, 6) and (seg_pred.double() - sp64).abs().max().item() <= TOL
    assert (end_points["transform"].double() - t64).abs().max().item() <= TOL


def test_small_batches_take_the_plain_layers_and_the_cpu_model_loads_the_state():
    """B N < 8192: no fused stack; the same variables, the same numbers to 1e-4 as the CPU model on the same state"""
    c = synth_clouds(2, 256, seed=4)
    x = torch.from_numpy(c).to(DEV)
    net = Model(pointnet_seg.get_model, device=DEV, seed=1).build(x)
    SS.PS.randomise(net, 7)
    cpu = Model(pointnet_seg.get_model, seed=9).build(torch.from_numpy(c))
    sd = {k: v.cpu() for k, v in net.state_dict().items()}
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(v.shape)) for k, v in cpu.state_dict().items()]
    cpu.load_state_dict(sd)
    with torch.no_grad():
        (a, sa, _), seen = _calls(lambda: net(x, is_training=False))
        b_, sb, _ = cpu(torch.from_numpy(c), is_training=False)
    assert "pcops_cloud_point_fwd" not in seen
    assert (a.cpu() - b_).abs().max().item() <= TOL and (sa.cpu() - sb).abs().max().item() <= TOL


@pytest.mark.parametrize("kind", ["seg", "partseg"])
def test_training_step_against_float64(kind, monkeypatch):
    monkeypatch.setattr(fused_mlp, "CLOUD_POINT_FUSED", True)
    (_, seen) = _calls(lambda: SS.check_step(kind))
    # the step ran the new kernels once each (the forward also runs when the model is built)
    assert seen.count("pcops_cloud_point_fwd") >= 1 and seen.count("pcops_cloud_point_bwd") == 1
    assert "pcops_cloud_bias_fwd" not in seen and "pcops_cloud_bias_bwd" not in seen


def test_training_steps_on_the_unfused_route_in_a_child_process():
    env = dict(os.environ, PCOPS_CLOUD_POINT_FUSED="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pointnet_seg_step.py")], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-2500:]
    assert "pointnet seg step ok (fused first conv off)" in out.stdout


def test_plan_takes_the_new_arm_only_when_asked():
    """the planner: the cloud_point arm for the raw 64-wide input under its flag bit, cloud_bias for the same stack handed Q,
    and an error -- not another arm -- where the raw input cannot be taken"""
    kw = dict(R=8192, S=1024, K0=None, widths=[512, 256, 128, 128], training=True, need_grad=True, need_dx=True, sync=False,
              w_aligned=[False, True, True, True], has_b=[False, True, True, True], geom=(8, 1024, 1))
    plan = fused_mlp.plan_stack(pool=2 | 16, present=("a0", "ctr", "wxyz"), point_k=64, **kw)
    assert (plan.layers[0].fwd, plan.layers[0].bwd, plan.layers[0].store_y) == ("cloud_point", "cloud_point", True)
    plan = fused_mlp.plan_stack(pool=2, present=("a0", "ctr"), **kw)
    assert (plan.layers[0].fwd, plan.layers[0].bwd) == ("cloud_bias", "cloud_bias")
    for bad in (dict(point_k=32), dict(point_k=64, widths=[96, 256, 128, 128])):
        with pytest.raises(_lib.PcopsError):
            fused_mlp.plan_stack(pool=2 | 16, present=("a0", "ctr", "wxyz"), **dict(kw, **bad))
    prev, fused_mlp.CLOUD_POINT_FUSED = fused_mlp.CLOUD_POINT_FUSED, False
    try:
        assert not seg_ops.point_fused(8, 1024, 64, 512)
        with pytest.raises(_lib.PcopsError):
            fused_mlp.plan_stack(pool=2 | 16, present=("a0", "ctr", "wxyz"), point_k=64, **kw)
    finally:
        fused_mlp.CLOUD_POINT_FUSED = prev
    # the size policy of the wrapper: today's route below 131 072 rows, the fused kernels from there
    assert seg_ops.POINT_FUSED_MIN_ROWS == 131072
    assert seg_ops.point_fused(256, 2048, 64, 512) == fused_mlp.CLOUD_POINT_FUSED and not seg_ops.point_fused(32, 1024, 64, 512)
    assert not seg_ops.point_fused(256, 2048, 32, 512) and not seg_ops.point_fused(256, 2048, 64, 1088)


def _write_set(path, kind, clouds, points, seed):
    data = synth_clouds(clouds, points, seed=seed)
    arrs = {"data": data, "label": synth_labels(clouds, seed)}
    if kind == "seg":
        arrs["mask"] = synth_masks(clouds, points, seed) * 2 - 1          # -1 background, 1 object: binarised by the loader
    else:
        arrs["parts"] = np.floor((data[:, :, 1] + 1.0) * 3.0).clip(0, 5).astype(np.int32)
    np.savez(path, **arrs)


@pytest.mark.parametrize("model,kind", [("pointnet_seg", "seg"), ("pointnet_partseg", "parts")])
def test_train_then_evaluate(model, kind, tmp_path):
    """two trainer steps (B = 16, N = 512: 8192 rows, the fused head) and the evaluation of the checkpoint, on synthetic files"""
    log_dir, dump = str(tmp_path / "log"), str(tmp_path / "dump")
    train_file, test_file = str(tmp_path / "train.npz"), str(tmp_path / "test.npz")
    _write_set(train_file, kind, 32, 512, 1)
    _write_set(test_file, kind, 16, 512, 2)
    common = ["--model", model, "--num_point", "512", "--batch_size", "16"]
    out = subprocess.run([sys.executable, "-m", "scanobjectnn_amd.pointnet2.train"] + common +
                         ["--max_epoch", "1", "--train_file", train_file, "--test_file", test_file, "--log_dir", log_dir],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    assert rec["epoch"] == 0 and rec["mean_loss"] > 0 and 0 <= rec["eval_acc"] <= 1
    assert ("eval_seg_acc" in rec) == (kind == "seg")
    sd = torch.load(os.path.join(log_dir, "model.pt"), map_location="cpu")
    assert tuple(sd["graph.conv6/weights"].shape) == (1, 1, 1088, 512)
    assert tuple(sd["graph.conv10/weights"].shape) == (1, 1, 128, 2 if kind == "seg" else 6)
    tool = "evaluate_seg_scenennobjects" if kind == "seg" else "evaluate_partseg"
    out = subprocess.run([sys.executable, "-m", "scanobjectnn_amd.pointnet2." + tool] + common +
                         ["--test_file", test_file, "--model_path", os.path.join(log_dir, "model.pt"), "--dump_dir", dump],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Model restored. (state-dict" in out.stdout and "total seen: 16" in out.stdout and "eval mean loss:" in out.stdout
    if kind == "seg":
        assert "seg accuracy:" in out.stdout and "eval avg class acc:" in out.stdout
        assert len(open(os.path.join(dump, "pred_label.txt")).read().splitlines()) == 16
    else:
        assert "eval seg accuracy:" in out.stdout and "eval avg class acc:" in out.stdout
        for name in ("background", "head", "back", "arm", "base", "seat"):
            assert "%10s:\t" % name in out.stdout
    assert os.path.exists(os.path.join(dump, "log_evaluate.txt"))
