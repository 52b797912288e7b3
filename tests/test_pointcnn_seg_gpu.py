"""PointCNN's background-aware model (pointcnn_seg) on the op library: both heads and every variable's gradient against the
float64 restatement of tests/xdconv_ref.py with the product's own neighbour indices imposed, on a small setting whose first two
X-DeConv layers are wide enough (384 and 320 channels) to run in three channel groups; a bit-identical backward pass; two
steps of the trainer and the mask evaluation of its checkpoint end to end; the classifier's command line refusing the model;
and a tensor-bundle round trip of its variables."""
import json
import os
import subprocess
import sys

import pytest
import torch

import xconv_ref as R
import xdconv_checks as K
import xdconv_ref as RD
from scanobjectnn_amd import _lib
from scanobjectnn_amd.graph import Model
from scanobjectnn_amd.pointcnn import pointcnn_seg as m
from scanobjectnn_amd.pointcnn import pointfly as pf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N = 3, 64


def _cloud():
    return (torch.rand(B, N, 3, generator=K.gen("cloud")) * 2 - 1).to(DEV)


def _targets():
    return (torch.arange(B, device=DEV) % 15), (torch.rand(B, N, generator=K.gen("mask")) < 0.4).long().to(DEV)


def _record(monkeypatch):
    """every layer's dilated neighbour indices and every contraction's (K, c, groups); dropout off"""
    seen, shapes = [], []
    knn = pf.knn_indices_general

    def knn_rec(queries, points, k, *a, **kw):
        out = knn(queries, points, k, *a, **kw)
        seen.append(out)
        return out

    def hook(name, phase, args):
        if name == "pcops_xconv_fwd" and phase == "pre":
            shapes.append((args[3], args[4] + args[5], _lib.load().pcops_xconv_channel_groups(*args[:7])))

    monkeypatch.setattr(pf, "knn_indices_general", knn_rec)
    monkeypatch.setattr(torch.nn.functional, "dropout", lambda x, p=0.5, training=True, inplace=False: x)
    _lib._hooks.append(hook)
    return seen, shapes, hook


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
def test_model_against_float64(training, monkeypatch):
    """Both heads' logits within 1e-4 and every variable's gradient within 1e-3 of that gradient's largest element, the
    classifier's bars of tests/test_pointcnn_gpu.py (see there for the exactly-zero gradient of the X_1 betas in training
    mode, which the X-DeConv layers share)."""
    monkeypatch.delenv("PCOPS_XCONV_NATIVE", raising=False)
    setting = K.small_seg_setting()
    seen, shapes, hook = _record(monkeypatch)
    try:
        pts = _cloud()
        net = Model(m.bind(setting, m.get_model), device=DEV, seed=5).build(pts)
        K.randomise(net, 13)
        labels, mask = _targets()
        P = R.params_from_state_dict(net.state_dict(), device=DEV)      # the moving statistics move in a training pass
        for v in P.values():
            v.requires_grad_(True)
        del seen[:], shapes[:]
        cls, seg = net(pts, is_training=training)
        m.get_loss(cls, seg, labels, mask, seg_weight=0.3)[0].backward()
    finally:
        _lib._hooks.remove(hook)
    # the nine contractions: xdconv_1 and xdconv_2 in three channel groups, everything else in one
    assert shapes == [(4, 8, 1), (6, 20, 1), (8, 40, 1), (5, 80, 1), (5, 384, 3), (5, 320, 3), (8, 80, 1), (6, 40, 1),
                      (4, 20, 1)]
    dil = [lp['D'] for lp in setting.xconv_params] + [dp['D'] for dp in setting.xdconv_params]
    idx = [full[:, :, ::d] for full, d in zip(seen, dil)]
    want_cls, want_seg = RD.pointcnn_seg(pts.double(), P, setting, training, idx)
    RD.loss(want_cls, want_seg, labels, mask, 0.3)[0].backward()
    assert cls.shape == want_cls.shape == (B, 16, 15) and seg.shape == want_seg.shape == (B, N, 2)
    err_cls = (cls.detach().double() - want_cls.detach()).abs().max().item()
    err_seg = (seg.detach().double() - want_seg.detach()).abs().max().item()
    rows = []
    for name, p in net.named_parameters():
        key = name.split("graph.", 1)[1]
        q = P[key]
        scale = q.grad.abs().max().item()
        if training and key.endswith("_X_1_bn/beta"):                      # exactly zero: the norm's gamma sets the scale
            assert scale <= 1e-12
            scale = P[key[:-len("beta")] + "gamma"].grad.abs().max().item()
        rows.append(((p.grad.double() - q.grad).abs().max().item() / max(scale, 1e-300), name))
    rows.sort(reverse=True)
    print("training=%s class logits max-abs %.3g, mask logits max-abs %.3g; gradient error / largest element of the gradient, "
          "worst three: %s" % (training, err_cls, err_seg, ", ".join("%s %.3g" % (r[1], r[0]) for r in rows[:3])))
    assert err_cls <= 1e-4 and err_seg <= 1e-4
    assert rows[0][0] <= 1e-3, "%s: gradient error %.3g of the gradient's largest element" % (rows[0][1], rows[0][0])


def test_backward_is_bit_identical_in_deterministic_mode():
    pts = _cloud()
    labels, mask = _targets()
    net = Model(m.bind(K.small_seg_setting(), m.get_model), device=DEV, seed=3).build(pts)
    state = {k: v.clone() for k, v in net.state_dict().items()}
    prev = _lib.deterministic()
    _lib.set_deterministic(True)
    try:
        grads = []
        for _ in range(2):
            net.load_state_dict(state)
            net.zero_grad()
            torch.manual_seed(7)                                           # the dropout masks
            cls, seg = net(pts, is_training=True)
            m.get_loss(cls, seg, labels, mask)[0].backward()
            grads.append({k: p.grad.clone() for k, p in net.named_parameters()})
    finally:
        _lib.set_deterministic(prev)
    assert all(torch.isfinite(g).all() for g in grads[0].values())
    for k in grads[0]:
        assert K.bits_equal(grads[0][k], grads[1][k]), k


def test_variables_round_trip_through_a_tensor_bundle(tmp_path):
    from scanobjectnn_amd import tf_checkpoint
    pts = _cloud()
    a = Model(m.bind(K.small_seg_setting(), m.get_model), device=DEV, seed=1).build(pts)
    K.randomise(a, 2)
    prefix = str(tmp_path / "model.ckpt")
    tf_checkpoint.save_tf_checkpoint(a, prefix)
    names = set(tf_checkpoint.read_checkpoint(prefix))
    assert names == {k.split("graph.", 1)[1] for k in a.state_dict()}          # name for name
    assert {"xdconv_1_X_0/kernel", "xdconv_2_X_1/depthwise_weights", "xdconv_1_fts_conv/depthwise_kernel",
            "xdconv_5_fts_conv/pointwise_kernel", "xdconv_3_fts_fuse/kernel", "xdconv_4_fts_fuse_bn/moving_mean",
            "fc_class_1_bn/gamma", "fc_seg_0/kernel", "logits_classification/bias", "logits_segmentation/kernel"} <= names
    b = Model(m.bind(K.small_seg_setting(), m.get_model), device=DEV, seed=9).build(pts)
    loaded, missing, unexpected = tf_checkpoint.load_tf_checkpoint(b, prefix, strict=True)
    assert not missing and not unexpected and len(loaded) == len(a.state_dict())
    for x, y in zip(a(pts, is_training=False), b(pts, is_training=False)):
        assert torch.equal(x, y)


# ----------------------------------------------------------------------------------------------------------- end to end
def test_train_two_steps_then_evaluate(tmp_path):
    log_dir, dump = str(tmp_path / "log"), str(tmp_path / "dump")
    common = ["--model", "pointcnn_seg", "--num_point", "512"]                 # --setting falls back to object_dataset_x3
    out = subprocess.run([sys.executable, "-m", "scanobjectnn_amd.pointnet2.train"] + common +
                         ["--batch_size", "8", "--max_epoch", "1", "--synthetic_clouds", "16", "--deterministic",
                          "--log_dir", log_dir], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    assert rec["epoch"] == 0 and rec["mean_loss"] > 0 and rec["mean_loss"] == rec["mean_loss"]
    assert 0 <= rec["eval_acc"] <= 1 and 0 <= rec["eval_seg_acc"] <= 1 and 0 <= rec["train_acc"] <= 1
    sd = torch.load(os.path.join(log_dir, "model.pt"), map_location="cpu")
    assert tuple(sd["graph.xdconv_1_fts_conv/depthwise_kernel"].shape) == (1, 16, 576, 1)
    assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())

    out = subprocess.run([sys.executable, "-m", "scanobjectnn_amd.pointnet2.evaluate_seg_scenennobjects"] + common +
                         ["--batch_size", "8", "--synthetic_clouds", "16", "--num_votes", "2", "--model_path",
                          os.path.join(log_dir, "model.pt"), "--dump_dir", dump], cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Model restored. (state-dict" in out.stdout
    vals = {}
    for line in out.stdout.splitlines():
        for key in ("eval mean loss", "eval accuracy", "eval avg class acc", "seg accuracy"):
            if line.startswith(key + ":"):
                vals[key] = float(line.split(":")[1])
    assert set(vals) == {"eval mean loss", "eval accuracy", "eval avg class acc", "seg accuracy"}
    assert vals["eval mean loss"] > 0 and all(v == v and v < float("inf") for v in vals.values())
    assert 0 <= vals["eval accuracy"] <= 1 and 0 <= vals["seg accuracy"] <= 1
    assert len(open(os.path.join(dump, "pred_label.txt")).read().splitlines()) == 16

    # the classifier's command line refuses the model the way it refuses the _bga ones
    out = subprocess.run([sys.executable, "-m", "scanobjectnn_amd.pointnet2.evaluate_scenennobjects"] + common +
                         ["--model_path", os.path.join(log_dir, "model.pt"), "--dump_dir", dump], cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode != 0 and "evaluate_seg_scenennobjects" in out.stderr


def test_votes_are_taken_on_class_scores():
    """eval_seg_votes with the model's class_scores: per vote the softmax summed over the class head's points, summed over
    the votes; the mask logits summed over the votes"""
    import math
    import numpy as np
    from scanobjectnn_amd import provider
    from scanobjectnn_amd.pointnet2 import evaluate_seg_scenennobjects as EVS
    pts = _cloud()
    net = Model(m.bind(K.small_seg_setting(), m.get_model), device=DEV, seed=4).build(pts)
    K.randomise(net, 5)
    labels, mask = _targets()
    ev = EVS.eval_seg_votes(net, pts.cpu().numpy(), labels.cpu().numpy(), mask.cpu().numpy(), B, num_votes=2, device=DEV,
                            scores_fn=m.class_scores,
                            loss_fn=lambda cp, sp, y, mk: m.get_loss(cp, sp, y, mk, seg_weight=0.5)[0])
    with torch.no_grad():
        outs = [net(provider.rotate_point_cloud_by_angle(pts, v / 2.0 * math.pi * 2).contiguous(), is_training=False)
                for v in range(2)]
    scores = m.class_scores(outs[0][0]) + m.class_scores(outs[1][0])
    assert scores.shape == (B, 15) and (m.class_scores(outs[0][0]).sum(1) - 16).abs().max() < 1e-4      # 16 softmax rows
    assert np.array_equal(ev["pred"], scores.argmax(dim=1).cpu().numpy())
    assert np.array_equal(ev["seg_pred"], (outs[0][1] + outs[1][1]).argmax(dim=2).cpu().numpy())
    assert 0 <= ev["seg_accuracy"] <= 1 and ev["mean_loss"] > 0
