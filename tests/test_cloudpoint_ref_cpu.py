"""The float64 definitions of tests/cloudpoint_ref.py held against each other and against what they must reject, without a
GPU: plain loops against dense forms; float64 autograd of Y = X Wx + Ctr behind a batch norm against the backward definition;
the relative-RMS bar of tests/cloudpoint_checks.py measured (a SEQUENTIAL fp32 evaluation of every case stays inside the
per-element bounds and sets the bar); one wrong restatement per edge rejected by the same bounds; both models' torch form on
the CPU against the float64 restatement; both losses against hand-computed values; the variables of both models enumerated by
hand from the reference's model files; the registration of both models and the command lines."""
import importlib

import pytest
import torch

import cloudpoint_checks as K
import cloudpoint_ref as R
from scanobjectnn_amd.graph import Model
from scanobjectnn_amd.pointnet import pointnet_partseg, pointnet_seg

TOL = 1e-4


# ------------------------------------------------------------------------------------------------- loops against dense forms
@pytest.mark.parametrize("case,rpp", [((1, 1, 64), 128), ((2, 5, 64), 2), ((3, 3, 128), 128)], ids=str)
def test_loops_against_dense(case, rpp):
    b, n, c = case
    X, Wx, Ctr, pivot, G, Y, p, q, t = K.inputs(case)
    for piv in (pivot, None):
        Yl, S1l, S2l = R.fwd_loops(b, n, X, Wx, Ctr, piv, rpp)
        (s1, _, _), (s2, _, _) = R.stats(b, n, X, Wx, Ctr, piv, rpp)
        assert (Yl - R.fwd(b, n, X, Wx, Ctr)[0]).abs().max() <= 1e-12
        assert S1l.shape == s1.shape == (b * -(-n // rpp), c)
        assert (S1l - s1).abs().max() <= 1e-11 and (S2l - s2).abs().max() <= 1e-10
    dX, dWx, dCtr = R.bwd_loops(b, n, G, Y, p, q, t, X, Wx)
    ref = R.bwd(b, n, G, Y, p, q, t, X, Wx)
    assert (dX - ref["dX"][0]).abs().max() <= 1e-11
    assert (dWx - ref["dWx"][0]).abs().max() <= 1e-11
    assert (dCtr - ref["dCtr"][0]).abs().max() <= 1e-11


def test_backward_definition_against_float64_autograd():
    """z = relu(bn(X Wx + Ctr[cloud])) with training statistics, loss = sum(z Gz): autograd's dX, dWx, dCtr are the
    definition's with (p, q, t) of the batch norm and the ReLU-masked upstream gradient"""
    b, n, c = 3, 7, 128
    X, Wx, Ctr, _, Gz, _, gamma, _, beta = K.inputs((b, n, c))
    x, w, ctr = (v.double().requires_grad_(True) for v in (X, Wx, Ctr))
    y = x @ w + ctr.view(b, 1, c).expand(b, n, c).reshape(b * n, c)
    mean = y.mean(0)
    var = ((y - mean) ** 2).mean(0)
    z = torch.relu(gamma.double() * (y - mean) / torch.sqrt(var + R.BN_EPS) + beta.double() - 1.0)
    (z * Gz.double()).sum().backward()
    Gm = Gz.double() * (z > 0)
    p, q, t = R.bn_backward_coeffs(y.detach(), Gm, gamma.double())
    ref = R.bwd(b, n, Gm, y.detach(), p, q, t, x.detach(), w.detach())
    assert (z > 0).any() and not (z > 0).all()
    for got, name in ((x.grad, "dX"), (w.grad, "dWx"), (ctr.grad, "dCtr")):
        assert (got - ref[name][0]).abs().max() <= 1e-10 * max(1.0, ref[name][0].abs().max().item()), name


# ------------------------------------------------------------------------------------------------------ the bar, measured
def _seq_fwd(b, n, X, Wx, Ctr, pivot):
    c = Wx.shape[1]
    acc = torch.zeros(b * n, c)
    for i in range(K.K_WIDTH):
        acc = acc + X[:, i:i + 1] * Wx[i]
    Y = acc + Ctr.view(b, 1, c).expand(b, n, c).reshape(b * n, c)
    per = -(-n // K.FWD_POINTS)
    d = torch.zeros(b, per * K.FWD_POINTS, c)
    d[:, :n] = (Y - pivot).view(b, n, c)
    d = d.view(b * per, K.FWD_POINTS, c)
    s1, s2 = torch.zeros(b * per, c), torch.zeros(b * per, c)
    for j in range(min(n, K.FWD_POINTS)):
        s1 = s1 + d[:, j]
        s2 = s2 + d[:, j] * d[:, j]
    return Y, s1, s2


def _seq_bwd(b, n, G, Y, p, q, t, X, Wx):
    c = Wx.shape[1]
    Dm = (p * G + q * Y) + t
    dX = torch.zeros(b * n, K.K_WIDTH)
    for ch in range(c):
        dX = dX + Dm[:, ch:ch + 1] * Wx[:, ch]
    dWx = torch.zeros(K.K_WIDTH, c)
    for r in range(b * n):
        dWx = dWx + X[r].view(-1, 1) * Dm[r]
    dCtr = torch.zeros(b, c)
    Dv = Dm.view(b, n, c)
    for j in range(n):
        dCtr = dCtr + Dv[:, j]
    return dX, dWx, dCtr


def test_fp32_sequential():
    """every case, evaluated sequentially in fp32, lies inside the per-element bounds; the worst relative RMS is the number
    beside cloudpoint_checks.RMS_BAR (the torch CPU arithmetic used here is elementwise: the same bits on every machine)"""
    worst = {}
    prev, K.RMS_BAR = K.RMS_BAR, 1.0         # the bar is what this test MEASURES: only the per-element bounds are asserted here
    try:
        for case in K.all_cases():
            b, n, c = case
            X, Wx, Ctr, pivot, G, Y, p, q, t = K.inputs(case)
            report = []
            Ys, s1, s2 = _seq_fwd(b, n, X, Wx, Ctr, pivot)
            K.check_sum(Ys, R.fwd(b, n, X, Wx, Ctr), "fwd Y", report=report)
            t1, t2 = R.stats(b, n, X, Wx, Ctr, pivot, K.FWD_POINTS)
            K.check_sum(s1, t1, "fwd S1", report=report)
            K.check_sum(s2, t2, "fwd S2", report=report)
            ref = R.bwd(b, n, G, Y, p, q, t, X, Wx)
            for got, name in zip(_seq_bwd(b, n, G, Y, p, q, t, X, Wx), ("dX", "dWx", "dCtr")):
                K.check_sum(got, ref[name], "bwd " + name, report=report)
            for what, _, rms in report:
                if rms > worst.get(what, (0.0, None))[0]:
                    worst[what] = (rms, case)
    finally:
        K.RMS_BAR = prev
    for what, (rms, case) in worst.items():
        print("fp32 sequential, worst relative RMS: %-9s %.3g at %s" % (what, rms, case))
    top = max(v[0] for v in worst.values())
    assert abs(top - K.RMS_FP32_SEQUENTIAL_WORST) <= 0.01 * top, (top, K.RMS_FP32_SEQUENTIAL_WORST)
    assert K.RMS_BAR == 2 * K.RMS_FP32_SEQUENTIAL_WORST


def test_case_tables_reach_every_edge():
    bs, ns, cs = ({case[i] for case in K.CASES} for i in range(3))
    assert {1, 15, 16, 17, 63, 64, 65, 129, 257, K.FWD_POINTS - 1, K.FWD_POINTS} <= ns
    assert bs == {1, 2, 3} and {64, 128, 512, 1024, 576} <= cs
    assert {tuple(K.passes(c)) for c in cs} >= {(1,), (2,), (8,), (8, 8), (8, 1), (8, 4, 2, 1)}
    parts = {p for _, p, _ in K.PARTS_CASES}
    assert {1, 2} <= parts and any(K.bwd_splits(b, n) == K.SPLIT_CAP for (b, n, _), _, _ in K.PARTS_CASES)
    for (b, n, c), want_parts, occupied in K.PARTS_CASES:
        s = K.bwd_splits(b, n)
        assert b * s == want_parts and -(-n // K.bwd_chunk(n, s)) == occupied, (b, n)
    assert any(occ < K.bwd_splits(b, n) for (b, n, _), _, occ in K.PARTS_CASES)     # a part that holds no row
    assert K.ws_floats(1, 64, 64) == 0 and K.ws_floats(3, 17, 64) == 3 * 64 * 64
    assert K.ws_floats(1, 65, 128) == 2 * 64 * 128 + 2 * 128


# --------------------------------------------------------------------------------- one wrong restatement per edge, rejected
def _rejected(out, triple, what):
    with pytest.raises(AssertionError):
        K.check_sum(out.float(), triple, what)


def test_wrong_restatements_are_rejected():
    case = (3, 70, 128)
    b, n, c = case
    X, Wx, Ctr, pivot, G, Y, p, q, t = K.inputs(case)
    y_ref = R.fwd(b, n, X, Wx, Ctr)
    K.check_sum(y_ref[0].float(), y_ref, "Y")                                  # (the right one passes)
    # the Ctr row of the neighbouring cloud
    _rejected(R.fwd(b, n, X, Wx, Ctr.roll(1, 0))[0], y_ref, "Y with the neighbour's Ctr")
    # the halves of conv6/weights swapped: the per-point rows are the FIRST 64 of the 64 + cc rows
    cc = 96
    g_ = K.gen("halves")
    W = (torch.randn(K.K_WIDTH + cc, c, generator=g_) + 0.5) / 8.0
    glob = torch.randn(b, cc, generator=g_) + 0.5
    right = R.fwd(b, n, X, W[:K.K_WIDTH], glob.double() @ W[K.K_WIDTH:].double())
    concat = torch.cat([X.double(), glob.double().view(b, 1, cc).expand(b, n, cc).reshape(b * n, cc)], 1) @ W.double()
    K.check_sum(concat.float(), right, "Y of the concatenation")
    swapped = R.fwd(b, n, X, W[cc:], glob.double() @ W[:cc].double())[0]
    _rejected(swapped, right, "Y with the halves swapped")
    # the pivot ignored
    s1, s2 = R.stats(b, n, X, Wx, Ctr, pivot, K.FWD_POINTS)
    z1, z2 = R.stats(b, n, X, Wx, Ctr, None, K.FWD_POINTS)
    _rejected(z1[0], s1, "S1 without the pivot")
    _rejected(z2[0], s2, "S2 without the pivot")
    # q Y left out; dCtr summed over the batch
    ref = R.bwd(b, n, G, Y, p, q, t, X, Wx)
    noq = R.bwd(b, n, G, Y, p, torch.zeros_like(q), t, X, Wx)
    for name in ("dX", "dWx", "dCtr"):
        K.check_sum(ref[name][0].float(), ref[name], name)
        _rejected(noq[name][0], ref[name], name + " without q Y")
    _rejected(ref["dCtr"][0].sum(0, keepdim=True).expand(b, c), ref["dCtr"], "dCtr summed over the batch")


# ------------------------------------------------------------------------------------------------------------- the models
def _randomise(net, seed):
    g_ = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, v in net.state_dict().items():
            r = torch.rand(v.shape, generator=g_).to(v.dtype)
            if name.endswith("/gamma") or name.endswith("/moving_variance"):
                v.copy_(0.5 + r)
            elif name.endswith("/beta") or name.endswith("/moving_mean") or name.endswith("/biases"):
                v.add_(0.4 * r - 0.2)
            elif "transform_" in name and name.endswith("/weights") and v.dim() == 2 and v.abs().max() == 0:
                v.copy_(0.02 * r - 0.01)


def _cloud(b, n, seed):
    return torch.randn(b, n, 3, generator=torch.Generator().manual_seed(seed)) * 0.4


def test_models_on_the_cpu_against_float64():
    """eval mode, as on the GPU (tests/test_pointnet_seg_gpu.py): logits <= 1e-4"""
    training = False
    x = _cloud(3, 33, 1)
    import scanobjectnn_amd.dgcnn.tf_util as td
    real = td.dropout
    td.dropout = lambda inputs, is_training, scope, keep_prob=0.5, noise_shape=None: inputs
    try:
        net = Model(pointnet_seg.get_model, seed=3).build(x)
        _randomise(net, 4)
        P = R.params_from_state_dict(net.state_dict())
        with torch.no_grad():
            cp, sp, ep = net(x, is_training=training, bn_decay=0.9)
            cp64, sp64, t64 = R.pointnet_seg(x.double(), P, training)
        assert cp.shape == (3, 15) and sp.shape == (3, 33, 2) and ep["transform"].shape == (3, 64, 64)
        assert (cp.double() - cp64).abs().max() <= TOL and (sp.double() - sp64).abs().max() <= TOL
        assert (ep["transform"].double() - t64).abs().max() <= TOL and (t64[0] - t64[1]).abs().max() > 1e-4
        net = Model(pointnet_partseg.get_model, seed=5).build(x)
        _randomise(net, 6)
        P = R.params_from_state_dict(net.state_dict())
        with torch.no_grad():
            sp, ep = net(x, is_training=training, bn_decay=0.9)
            sp64, t64 = R.pointnet_partseg(x.double(), P, training)
        assert sp.shape == (3, 33, 6) and (sp.double() - sp64).abs().max() <= TOL
        assert (ep["transform"].double() - t64).abs().max() <= TOL
    finally:
        td.dropout = real


def test_losses_against_hand_computed_values():
    import math
    T = torch.eye(64).repeat(2, 1, 1)
    T[0, 0, 0] = 2.0                      # T T^T - I = diag(3, 0, ...): l2_loss = 9 / 2
    T[1, 0, 1] = 1.0                      # row 0 = e0 + e1: (T T^T - I) has 1 at (0,0), (0,1), (1,0): l2_loss = 3 / 2
    ep = {"transform": T}
    class_pred = torch.zeros(2, 15)
    class_pred[0, 3] = math.log(15.0)     # softmax: 15 / 29 at class 3;  cloud 1 uniform: 1 / 15
    seg_pred = torch.zeros(2, 4, 2)
    seg_pred[0, :, 1] = math.log(3.0)     # cloud 0: p(1) = 3/4 at every point; cloud 1: 1/2
    gt_mask = torch.tensor([[1, 1, 1, 0], [0, 1, 0, 1]])
    total, classify, seg = pointnet_seg.get_loss(class_pred, seg_pred, torch.tensor([3, 7]), gt_mask, ep, seg_weight=0.25,
                                                 reg_weight=0.01)
    want_cls = 0.5 * (-math.log(15.0 / 29.0) + math.log(15.0))
    want_seg = 0.5 * ((-3 * math.log(0.75) - math.log(0.25)) / 4 + math.log(2.0))
    assert abs(classify.item() - want_cls) <= 1e-6 and abs(seg.item() - want_seg) <= 1e-6
    assert abs(total.item() - (0.75 * want_cls + 0.25 * want_seg + 0.01 * (4.5 + 1.5))) <= 1e-6
    assert abs(R.seg_ce(seg_pred.double(), gt_mask).item() - want_seg) <= 1e-12
    assert abs(R.ortho(T.double(), 0.01).item() - 0.06) <= 1e-12
    part_pred = torch.zeros(2, 4, 6)
    part_pred[0, :, 5] = math.log(5.0)    # cloud 0: p(5) = 1/2, every other part 1/10; cloud 1 uniform
    gt = torch.tensor([[5, 5, 0, 1], [0, 1, 2, 3]])
    want = 0.5 * ((2 * math.log(2.0) + 2 * math.log(10.0)) / 4 + math.log(6.0))
    assert abs(pointnet_partseg.get_loss(part_pred, gt, ep, reg_weight=0.01).item() - (want + 0.06)) <= 1e-6
    # the defaults of the reference: seg_weight 0.5, reg_weight 0.001
    total = pointnet_seg.get_loss(class_pred, seg_pred, torch.tensor([3, 7]), gt_mask, ep)[0]
    assert abs(total.item() - (0.5 * want_cls + 0.5 * want_seg + 0.006)) <= 1e-6


def _tnet_variables(scope, head, k_in, k):
    out = {}
    for name, cin, width in (("tconv1", k_in, 64), ("tconv2", 64, 128), ("tconv3", 128, 1024)):
        out["%s/%s/weights" % (scope, name)] = (1, 3, 1, width) if (name == "tconv1" and k_in == 3) else (1, 1, cin, width)
        out.update(_bn_variables("%s/%s" % (scope, name), width))
    for name, cin, width in (("tfc1", 1024, 512), ("tfc2", 512, 256)):
        out["%s/%s/weights" % (scope, name)] = (cin, width)
        out.update(_bn_variables("%s/%s" % (scope, name), width))
    out["%s/%s/weights" % (scope, head)] = (256, k * k)
    out["%s/%s/biases" % (scope, head)] = (k * k,)
    return out


def _bn_variables(scope, width):
    return {"%s/%s" % (scope, v): (width,) for v in ("biases", "bn/beta", "bn/gamma", "bn/moving_mean", "bn/moving_variance")}


def _front_variables():
    """pointnet_seg.py:30-62 / pointnet_partseg.py:29-61, by hand"""
    out = _tnet_variables("transform_net1", "transform_XYZ", 3, 3)
    out["conv1/weights"] = (1, 3, 1, 64)
    out.update(_bn_variables("conv1", 64))
    out["conv2/weights"] = (1, 1, 64, 64)
    out.update(_bn_variables("conv2", 64))
    out.update(_tnet_variables("transform_net2", "transform_feat", 64, 64))
    for i, cin, width in ((3, 64, 64), (4, 64, 128), (5, 128, 1024)):
        out["conv%d/weights" % i] = (1, 1, cin, width)
        out.update(_bn_variables("conv%d" % i, width))
    return out


def _head_variables(num_out):
    out = {}
    for i, cin, width in ((6, 1088, 512), (7, 512, 256), (8, 256, 128), (9, 128, 128)):
        out["conv%d/weights" % i] = (1, 1, cin, width)
        out.update(_bn_variables("conv%d" % i, width))
    out["conv10/weights"] = (1, 1, 128, num_out)
    out["conv10/biases"] = (num_out,)
    return out


def test_variable_names_and_shapes():
    x = _cloud(2, 20, 2)
    want = _front_variables()
    for name, cin, width in (("fc1", 1024, 512), ("fc2", 512, 256)):
        want["%s/weights" % name] = (cin, width)
        want.update(_bn_variables(name, width))
    want["fc3/weights"], want["fc3/biases"] = (256, 15), (15,)
    want.update(_head_variables(2))
    got = {k[len("graph."):]: tuple(v.shape) for k, v in Model(pointnet_seg.get_model, seed=0).build(x).state_dict().items()}
    assert got == want, sorted(set(got.items()) ^ set(want.items()))
    assert got["conv6/weights"] == (1, 1, 1088, 512) and got["conv10/weights"] == (1, 1, 128, 2)
    want = _front_variables()
    want.update(_head_variables(6))
    got = {k[len("graph."):]: tuple(v.shape)
           for k, v in Model(pointnet_partseg.get_model, seed=0).build(x).state_dict().items()}
    assert got == want, sorted(set(got.items()) ^ set(want.items()))
    assert got["conv10/weights"] == (1, 1, 128, 6)
    assert "fc1/weights" not in got                            # the part model has no class branch


# ------------------------------------------------------------------------------------------- registration and command lines
def test_models_are_registered():
    from scanobjectnn_amd.pointnet2 import evaluate_partseg as EP
    from scanobjectnn_amd.pointnet2 import evaluate_seg_scenennobjects as EVS
    from scanobjectnn_amd.pointnet2 import train
    assert importlib.import_module(train.MODELS["pointnet_seg"]) is pointnet_seg
    assert importlib.import_module(train.MODELS["pointnet_partseg"]) is pointnet_partseg
    assert train.MASK_MODELS == {"pointnet2_cls_bga", "dgcnn_bga", "pointcnn_seg"}
    assert train.MASK_MODELS_END_POINTS == {"pointnet_seg"}
    assert train.ALL_MASK_MODELS == train.MASK_MODELS | {"pointnet_seg"}
    for m in (pointnet_seg, pointnet_partseg):
        assert not hasattr(m, "trainer") and not hasattr(m, "flag_defaults")
    a = train.parse_args(["--model", "pointnet_seg"])
    assert (a.batch_size, a.num_point, a.seg_weight) == (16, 1024, 0.5)             # the trainer's defaults are unchanged
    assert train.parse_args(["--model", "pointnet_partseg"]).model == "pointnet_partseg"
    assert EVS.parse_args(["--model", "pointnet_seg"]).model == "pointnet_seg"
    with pytest.raises(SystemExit):
        EVS.parse_args(["--model", "pointnet_partseg"])
    a = EP.parse_args([])
    assert (a.model, a.batch_size, a.num_point, a.gpu, a.dump_dir, a.test_file, a.model_path) == (
        "pointnet_partseg", 1, 1024, 0, "dump/", "", "log/model.ckpt")
    assert EP.parse_args(["--model", "pointnet2_cls_partseg"]).model == "pointnet2_cls_partseg"
    with pytest.raises(SystemExit):
        EP.parse_args(["--model", "pointnet_seg"])
    assert EP.PART_NAMES == ["background", "head", "back", "arm", "base", "seat"]


def test_classifier_evaluation_refuses_the_mask_and_part_models(monkeypatch):
    from scanobjectnn_amd.pointnet2 import evaluate_scenennobjects as EV
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    for model in ("pointnet_seg", "pointnet_partseg"):
        with pytest.raises(SystemExit) as e:
            EV.evaluate(EV.parse_args(["--model", model]))
        assert "scanobjectnn_amd.pointnet2.evaluate_partseg" in str(e.value)


def test_eval_parts_metrics():
    """evaluate_partseg.eval_parts on a model that answers from a table: the reference's numbers by hand"""
    from scanobjectnn_amd.pointnet2 import evaluate_partseg as EP
    parts = torch.tensor([[0, 0, 1, 5], [1, 1, 5, 5]]).numpy()
    pred = torch.tensor([[0, 1, 1, 5], [1, 0, 5, 0]])

    def net(pts, is_training):
        i = int(pts[0, 0, 0].item())
        return torch.nn.functional.one_hot(pred[i:i + 1], 6).float(), {"transform": None}

    data = torch.zeros(2, 4, 3)
    data[1] = 1.0
    ev = EP.eval_parts(net, data.numpy(), parts, 1, device="cpu", loss_fn=lambda sp, gt, ep: torch.tensor(2.0))
    assert ev["total_seen"] == 2 and ev["mean_loss"] == 2.0 and ev["seg_accuracy"] == 5 / 8.0
    # part 0: 1 of 2, part 1: 2 of 3, part 5: 2 of 3; parts 2..4 never occur
    assert ev["per_part"] == [0.5, 2 / 3.0, -1.0, -1.0, -1.0, 2 / 3.0]
    assert abs(ev["avg_class_acc"] - (0.5 + 4 / 3.0) / 3) <= 1e-12
