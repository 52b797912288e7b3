"""PointCNN on the op library: the X-Conv contraction through autograd against its torch form and against float64, the whole
classifier against the float64 restatement (tests/xconv_ref.py) with the product's own neighbour indices imposed, two steps of
the trainer and the evaluation of its checkpoint end to end, a bit-identical backward pass, and the reference's real setting
built once for shapes and variable names."""
import json
import os
import subprocess
import sys

import pytest
import torch

import xconv_checks as K
import xconv_ref as R
from scanobjectnn_amd import _lib
from scanobjectnn_amd.graph import Model
from scanobjectnn_amd.pointcnn import pointcnn_cls as m
from scanobjectnn_amd.pointcnn import pointfly as pf
from scanobjectnn_amd.pointcnn import xconv_ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ the layer
@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("shape", [(2, 40, 17, 12, 12, 48, 2), (1, 33, 33, 8, 24, 0, 4)], ids=K.case_id)
def test_xconv_fn_against_torch_form_and_float64(shape, det):
    lifted, fts, idx, X, wd, dout = K.inputs(shape, DEV)
    prev = _lib.deterministic()
    _lib.set_deterministic(det)
    try:
        leaves = [t.clone().requires_grad_(True) if t is not None else None for t in (lifted, fts, X, wd)]
        out = xconv_ops.xconv_contract(leaves[0], leaves[1], idx, leaves[2], leaves[3])
        out.backward(dout)
        tw = [t.clone().requires_grad_(True) if t is not None else None for t in (lifted, fts, X, wd)]
        ot = xconv_ops.xconv_torch(tw[0], tw[1], idx, tw[2], tw[3])
        ot.backward(dout)
        ref = R.dgrad(lifted, fts, idx, X, wd, dout)
        K.check_sum(out.detach(), R.fwd(lifted, fts, idx, X, wd), "out")
        K.check_sum(leaves[0].grad, ref["dlifted"], "dlifted")
        K.check_sum(leaves[2].grad, ref["dX"], "dX")
        K.check_sum(leaves[3].grad, R.wgrad(lifted, fts, idx, X, wd.shape, dout), "dwd")
        if fts is not None:
            _, _, dfg = xconv_ops.dgrad(lifted, fts, idx, X, wd, dout)
            K.check_sum(dfg, ref["dfg"], "dfts_grouped")
            K.check_sum(leaves[1].grad, R.scatter(dfg, idx, shape[1]), "dfts")
            if det:
                assert K.bits_equal(leaves[1].grad, _lib.scatter_grouped(dfg, idx, shape[1]))
        for a, b in zip([out.detach()] + [t.grad for t in leaves if t is not None],
                        [ot.detach()] + [t.grad for t in tw if t is not None]):
            assert (a - b).abs().max().item() <= 1e-3 * b.abs().max().item()
        # fts needs no gradient (and neither does anything in front of a first layer): dwd keeps its bits
        w0 = wd.clone().requires_grad_(True)
        xconv_ops.xconv_contract(lifted, fts, idx, X, w0).backward(dout)
        assert K.bits_equal(w0.grad, leaves[3].grad)
    finally:
        _lib.set_deterministic(prev)


def test_layer_raises_outside_the_kernels(monkeypatch):
    monkeypatch.delenv("PCOPS_XCONV_NATIVE", raising=False)
    lifted, fts, idx, X, wd, _ = K.inputs(K.UNSUPPORTED[0], DEV)
    with pytest.raises(_lib.PcopsError, match="PCOPS_XCONV_NATIVE=0"):
        xconv_ops.xconv_contract(lifted, fts, idx, X, wd)
    monkeypatch.setenv("PCOPS_XCONV_NATIVE", "0")
    assert xconv_ops.xconv_contract(lifted, fts, idx, X, wd).shape == (1, 20, 16)


# -------------------------------------------------------------------------------------------------------- whole classifier
def _record_indices(monkeypatch):
    seen = []
    knn = pf.knn_indices_general

    def knn_rec(queries, points, k, *a, **kw):
        out = knn(queries, points, k, *a, **kw)
        seen.append(out)
        return out

    monkeypatch.setattr(pf, "knn_indices_general", knn_rec)
    monkeypatch.setattr(torch.nn.functional, "dropout", lambda x, p=0.5, training=True, inplace=False: x)
    return seen


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
def test_classifier_against_float64(training, monkeypatch):
    """Logits within 1e-4 and every variable's gradient within 1e-3 of that gradient's largest element (the max-norm form
    tests/test_mfv3d_gpu.py applies) of the float64 classifier that takes the product's neighbour indices.  ELU is C1, so
    there are no activation decisions to impose; dropout is switched off on both sides.
    In training mode the beta of every X_1 norm has an exactly zero gradient: X_2 is linear (no activation) and goes straight
    into a training-mode norm, whose mean absorbs any per-channel constant added in front of X_2.  The float64 value is
    rounding noise of 1e-17 and a ratio to it says nothing; those betas are held to the scale of the same norm's gamma
    gradient instead, as tests/test_mfv3d_gpu.py does for the biases in front of its norms."""
    monkeypatch.delenv("PCOPS_XCONV_NATIVE", raising=False)
    setting = K.small_setting()
    seen = _record_indices(monkeypatch)
    pts = (torch.rand(4, 64, 3, generator=K.gen("cloud")) * 2 - 1).to(DEV)
    net = Model(m.bind(setting), device=DEV, seed=5).build(pts)
    K.randomise(net, 13)
    labels = torch.arange(4, device=DEV) % 15
    P = R.params_from_state_dict(net.state_dict(), device=DEV)      # the moving statistics move in a training pass
    for v in P.values():
        v.requires_grad_(True)
    del seen[:]
    logits = net(pts, is_training=training)
    m.get_loss(logits, labels).backward()
    idx = [full[:, :, ::lp['D']] for full, lp in zip(seen, setting.xconv_params)]
    want = R.pointcnn_cls(pts.double(), P, setting, training, idx)
    torch.nn.functional.cross_entropy(want.reshape(-1, 15), labels.repeat_interleave(want.shape[1])).backward()
    assert logits.shape == want.shape == ((4, 16, 15) if training else (4, 1, 15))
    err = (logits.detach().double() - want.detach()).abs().max().item()
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
    print("training=%s logits max-abs %.3g; gradient error / largest element of the gradient, worst three: %s"
          % (training, err, ", ".join("%s %.3g" % (r[1], r[0]) for r in rows[:3])))
    assert err <= 1e-4
    assert rows[0][0] <= 1e-3, "%s: gradient error %.3g of the gradient's largest element" % (rows[0][1], rows[0][0])


def test_backward_is_bit_identical_in_deterministic_mode():
    setting = K.small_setting()
    pts = (torch.rand(4, 64, 3, generator=K.gen("cloud")) * 2 - 1).to(DEV)
    labels = torch.arange(4, device=DEV) % 15
    net = Model(m.bind(setting), device=DEV, seed=3).build(pts)
    state = {k: v.clone() for k, v in net.state_dict().items()}
    prev = _lib.deterministic()
    _lib.set_deterministic(True)
    try:
        grads = []
        for _ in range(2):
            net.load_state_dict(state)
            net.zero_grad()
            torch.manual_seed(7)                                           # the dropout mask
            m.get_loss(net(pts, is_training=True), labels).backward()
            grads.append({k: p.grad.clone() for k, p in net.named_parameters()})
    finally:
        _lib.set_deterministic(prev)
    assert all(torch.isfinite(g).all() for g in grads[0].values())
    for k in grads[0]:
        assert K.bits_equal(grads[0][k], grads[1][k]), k


def test_reference_setting_shapes_and_names():
    """modelnet_x3_l4 at B = 2, N = 1024, forward only: the four contractions the kernels are built for, the output shapes of
    both modes, and the variable names and layouts a TensorFlow checkpoint of the reference holds"""
    calls = []
    hook = lambda name, phase, args: calls.append(args[:7]) if name == "pcops_xconv_fwd" and phase == "pre" else None  # noqa: E731
    _lib._hooks.append(hook)
    try:
        pts = torch.rand(2, 1024, 3, generator=K.gen("big")).to(DEV)
        net = Model(m.get_model, device=DEV, seed=0).build(pts)
        with torch.no_grad():
            assert net(pts, is_training=False).shape == (2, 1, 15)
            assert net(pts, is_training=True).shape == (2, 128, 15)
    finally:
        _lib._hooks.remove(hook)
    assert calls[:4] == [(2, 1024, 1024, 8, 24, 0, 4), (2, 1024, 384, 12, 12, 48, 2), (2, 384, 128, 16, 24, 96, 2),
                         (2, 128, 128, 16, 48, 192, 2)]
    sd = {k.split("graph.", 1)[1]: tuple(v.shape) for k, v in net.state_dict().items()}
    for name, shape in {"xconv_1_nn_fts_from_pts_0/kernel": (3, 24), "xconv_1_X_0/kernel": (1, 8, 3, 64),
                        "xconv_1_X_1/depthwise_weights": (1, 8, 8, 8), "xconv_1_X_2_bn/gamma": (64,),
                        "xconv_1_fts_conv/depthwise_kernel": (1, 8, 24, 4), "xconv_1_fts_conv/pointwise_kernel": (1, 1, 96, 48),
                        "xconv_2_fts_conv/depthwise_kernel": (1, 12, 60, 2), "xconv_4_fts_conv/pointwise_kernel": (1, 1, 480, 384),
                        "xconv_4_fts_conv_bn/moving_variance": (384,), "xconv_4_fts_global_0/kernel": (3, 96),
                        "fc0/kernel": (480, 384), "fc1_bn/beta": (192,), "logits/kernel": (192, 15),
                        "logits/bias": (15,)}.items():
        assert sd[name] == shape, name
    assert not any(k.endswith("/bias") for k in sd if k != "logits/bias")       # no bias where a norm follows
    assert sum(v.numel() for v in net.parameters()) == 594515


# ----------------------------------------------------------------------------------------------------------- end to end
def test_train_two_steps_then_evaluate(tmp_path):
    log_dir, dump = str(tmp_path / "log"), str(tmp_path / "dump")
    common = ["--model", "pointcnn_cls", "--setting", "modelnet_x3_l4", "--num_point", "512"]
    out = subprocess.run([sys.executable, "-m", "scanobjectnn_amd.pointnet2.train"] + common +
                         ["--batch_size", "8", "--max_epoch", "1", "--synthetic_clouds", "16", "--deterministic",
                          "--log_dir", log_dir], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    assert rec["epoch"] == 0 and rec["mean_loss"] > 0 and 0 <= rec["eval_acc"] <= 1
    sd = torch.load(os.path.join(log_dir, "model.pt"), map_location="cpu")
    assert tuple(sd["graph.xconv_3_fts_conv/depthwise_kernel"].shape) == (1, 16, 120, 2)
    out = subprocess.run([sys.executable, "-m", "scanobjectnn_amd.pointnet2.evaluate_scenennobjects"] + common +
                         ["--batch_size", "8", "--synthetic_clouds", "16", "--num_votes", "2", "--model_path",
                          os.path.join(log_dir, "model.pt"), "--dump_dir", dump], cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Model restored. (state-dict" in out.stdout and "eval accuracy:" in out.stdout
    lines = open(os.path.join(dump, "pred_label.txt")).read().splitlines()
    assert len(lines) == 16
    # the command line's predictions are the argmax of class_scores (the softmax summed over the points) SUMMED OVER THE
    # VOTES, restated here on the same checkpoint and the same clouds.  (The trainer's own eval_acc is taken on another draw
    # of the point subset -- the reference's trainer draws a fresh one per evaluation -- so the two need not be equal.)
    import math
    import numpy as np
    from scanobjectnn_amd import data_utils, provider
    from scanobjectnn_amd.pointnet2 import evaluate_scenennobjects as EV
    args = EV.parse_args(common + ["--synthetic_clouds", "16"])
    data, labels = EV.load_test_set(args)
    cur, lab = data_utils.get_current_data_h5(data, labels, 512, rng=np.random.RandomState(0))
    net = Model(m.get_model, device=DEV, seed=0).build(torch.zeros(2, 512, 3, device=DEV))
    net.load_state_dict(sd)
    pred = []
    with torch.no_grad():
        for b in range(2):
            pts = torch.as_tensor(cur[8 * b:8 * b + 8], dtype=torch.float32, device=DEV)
            votes = [m.class_scores(net(provider.rotate_point_cloud_by_angle(pts, v / 2.0 * math.pi * 2).contiguous(),
                                        is_training=False)) for v in range(2)]
            assert votes[0].shape == (8, 15) and (votes[0].sum(1) - 1).abs().max() < 1e-5     # one averaged point: a softmax
            pred += (votes[0] + votes[1]).argmax(dim=1).tolist()
    assert lines == ["%s, %s" % (EV.SHAPE_NAMES[p], EV.SHAPE_NAMES[l]) for p, l in zip(pred, np.squeeze(lab))]
    acc = float(np.mean(np.asarray(pred) == np.squeeze(lab)))
    assert "eval accuracy: %f" % acc in out.stdout
