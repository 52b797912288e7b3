"""PointNet on the GPU: the feature transform and the regulariser through autograd (scanobjectnn_amd/pointnet/tnet_ops.py)
against the torch forms and float64; pointnet_cls in eval mode against oracle/ref_models.pointnet_cls in float64 (logits
<= 1e-4); one training step against float64 with the model's own decisions imposed (tests/pointnet_step.py: every variable's
gradient <= 1e-3 of its maximum), in this process and again with PCOPS_POINTNET_NATIVE=0 in a child process; a state dict
saved on the GPU loaded into the CPU model; and the trainer and the evaluation command lines for both classifiers."""
import json
import os
import subprocess
import sys

import pytest
import torch

import pointnet_step as PS
import tnet_checks as K
import tnet_ref as R
from oracle import ref_models as OR
from scanobjectnn_amd.graph import Model
from scanobjectnn_amd.pointnet import pointnet_cls as m
from scanobjectnn_amd.pointnet import tnet_ops
from scanobjectnn_amd.synth import synth_clouds

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
W = 2.0 ** -10


def test_transform_through_autograd(monkeypatch):
    monkeypatch.delenv("PCOPS_POINTNET_NATIVE", raising=False)
    shape = (3, 70)
    X, T, G = K.inputs(shape, DEV)
    x, t = X.clone().requires_grad_(True), T.clone().requires_grad_(True)
    out = tnet_ops.apply_feature_transform(x, t)
    assert type(out.grad_fn).__name__ == "_TransformKBackward"
    K.check_sum(out.detach(), R.fwd(X, T), "out")
    (out * G).sum().backward()                       # two consumers of the output would add up to the same G
    ref = R.bwd(X, T, G)
    K.check_sum(x.grad, ref["dX"], "dX")
    K.check_sum(t.grad, ref["dT"], "dT")
    # the torch form, by the switch: the same numbers to fp32 rounding, and not the native node
    monkeypatch.setenv("PCOPS_POINTNET_NATIVE", "0")
    x2, t2 = X.clone().requires_grad_(True), T.clone().requires_grad_(True)
    out2 = tnet_ops.apply_feature_transform(x2, t2)
    assert type(out2.grad_fn).__name__ != "_TransformKBackward"
    (out2 * G).sum().backward()
    assert (out2 - out).abs().max().item() <= 1e-4 and (t2.grad - t.grad).abs().max().item() <= 1e-3
    monkeypatch.delenv("PCOPS_POINTNET_NATIVE")
    # the input without a gradient (dX == NULL), an unsupported width and a CPU tensor
    t3 = T.clone().requires_grad_(True)
    tnet_ops.apply_feature_transform(X, t3).backward(G)
    assert K.bits_equal(t3.grad, t.grad)
    assert type(tnet_ops.apply_feature_transform(X[..., :32].contiguous().requires_grad_(True),
                                                 T[:, :32, :32].contiguous()).grad_fn).__name__ != "_TransformKBackward"
    assert torch.equal(tnet_ops.apply_feature_transform(X.cpu(), T.cpu()), torch.matmul(X.cpu(), T.cpu()))


def test_regulariser_through_autograd(monkeypatch):
    monkeypatch.delenv("PCOPS_POINTNET_NATIVE", raising=False)
    T = K.ortho_inputs((3, "near"), DEV)
    t = T.clone().requires_grad_(True)
    val = tnet_ops.ortho_regulariser(t, W)
    assert type(val.grad_fn).__name__ == "_OrthoRegBackward"
    (3.0 * val).backward()
    ref = R.ortho(T, W)
    loss, A, L = ref["loss_parts"]
    assert abs(val.item() - loss.sum().item()) <= (K.C_BOUND * (L + 4) * K.U * A.sum()).item() + 4 * K.U * loss.sum().item()
    K.check_sum(t.grad, (3.0 * ref["dT"][0], 3.0 * ref["dT"][1], L + 1), "dT")
    monkeypatch.setenv("PCOPS_POINTNET_NATIVE", "0")
    t2 = T.clone().requires_grad_(True)
    val2 = tnet_ops.ortho_regulariser(t2, W)
    assert type(val2.grad_fn).__name__ != "_OrthoRegBackward"
    (3.0 * val2).backward()
    assert abs(val2.item() - val.item()) <= 1e-4 * abs(val.item()) + 1e-9
    K.check_sum(t2.grad, (3.0 * ref["dT"][0], 3.0 * ref["dT"][1], L + 1), "dT of the torch form")


def _eval_net():
    c = synth_clouds(8, 256, seed=3)
    x = torch.from_numpy(c).to(DEV)
    net = Model(m.get_model, device=DEV, seed=1).build(x)
    PS.randomise(net, 5)
    return c, x, net


def test_eval_logits_against_float64():
    c, x, net = _eval_net()
    P = OR.params_from_state_dict(net.state_dict(), dtype=torch.float64)
    with torch.no_grad():
        logits, end_points = net(x, is_training=False)
        want, t2 = OR.pointnet_cls(torch.from_numpy(c).double(), P, False)
    assert logits.shape == (8, 15) and end_points["transform"].shape == (8, 64, 64)
    assert (logits.cpu().double() - want).abs().max().item() <= TOL
    assert (end_points["transform"].cpu().double() - t2).abs().max().item() <= TOL
    assert (t2[0] - t2[1]).abs().max().item() > 1e-4                      # a different matrix for each cloud


def test_training_step_against_float64(monkeypatch):
    monkeypatch.delenv("PCOPS_POINTNET_NATIVE", raising=False)
    from scanobjectnn_amd import _lib
    seen = []
    hook = lambda name, phase, args: phase == "pre" and seen.append(name)       # noqa: E731
    _lib._hooks.append(hook)
    try:
        PS.check_step()
    finally:
        _lib._hooks.remove(hook)
    # the step ran the new kernels: the transform's backward and the regulariser once each (the forward also runs when the
    # model is built)
    assert seen.count("pcops_transformk_fwd") >= 1
    assert [seen.count(n) for n in ("pcops_transformk_bwd", "pcops_ortho_reg")] == [1, 1]


def test_training_step_with_the_torch_forms_in_a_child_process():
    env = dict(os.environ, PCOPS_POINTNET_NATIVE="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pointnet_step.py")], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-2500:]
    assert "pointnet step ok (native transform off)" in out.stdout


def test_state_dict_moves_to_the_cpu_model():
    c, x, net = _eval_net()
    cpu = Model(m.get_model, seed=9).build(torch.from_numpy(c))
    sd = {k: v.cpu() for k, v in net.state_dict().items()}
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(v.shape)) for k, v in cpu.state_dict().items()]
    cpu.load_state_dict(sd)
    with torch.no_grad():
        a, b = net(x, is_training=False)[0], cpu(torch.from_numpy(c), is_training=False)[0]
    assert (a.cpu() - b).abs().max().item() <= TOL
    # the same seed gives the same initial values on either device
    fresh = Model(m.get_model, device=DEV, seed=9).build(x)
    again = Model(m.get_model, seed=9).build(torch.from_numpy(c))
    for (k, v), (k2, v2) in zip(fresh.state_dict().items(), again.state_dict().items()):
        assert k == k2 and torch.equal(v.cpu(), v2), k


@pytest.mark.parametrize("model", ["pointnet_cls", "pointnet_cls_basic"])
def test_train_then_evaluate(model, tmp_path):
    log_dir, dump = str(tmp_path / "log"), str(tmp_path / "dump")
    common = ["--model", model, "--num_point", "256"]
    out = subprocess.run([sys.executable, "-m", "scanobjectnn_amd.pointnet2.train"] + common +
                         ["--batch_size", "16", "--max_epoch", "1", "--synthetic_clouds", "64", "--log_dir", log_dir],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    assert rec["epoch"] == 0 and rec["mean_loss"] > 0 and 0 <= rec["eval_acc"] <= 1
    sd = torch.load(os.path.join(log_dir, "model.pt"), map_location="cpu")
    assert tuple(sd["graph.conv1/weights"].shape) == (1, 3, 1, 64)
    assert ("graph.transform_net2/transform_feat/weights" in sd) == (model == "pointnet_cls")
    out = subprocess.run([sys.executable, "-m", "scanobjectnn_amd.pointnet2.evaluate_scenennobjects"] + common +
                         ["--batch_size", "16", "--synthetic_clouds", "32", "--model_path",
                          os.path.join(log_dir, "model.pt"), "--dump_dir", dump], cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Model restored. (state-dict" in out.stdout and "eval accuracy:" in out.stdout
    assert len(open(os.path.join(dump, "pred_label.txt")).read().splitlines()) == 32
