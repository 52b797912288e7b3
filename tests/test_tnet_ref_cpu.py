"""The float64 definitions of tests/tnet_ref.py checked without a GPU: the plain loops against the dense forms, the dense
forms against float64 autograd of torch.matmul and of the regulariser expression of pointnet_cls.get_loss, a sequential fp32
evaluation of every definition inside the bounds the GPU tests apply (its relative RMS sets the family's bar in
tests/tnet_checks.py), the backward's split rule against the library's own answer (shape queries need no GPU), one
deliberately wrong restatement per edge rejected by those bounds, pointnet_cls_basic against its float64 restatement, and
the registration of both PointNet classifiers with the trainer and the evaluation."""
import pytest
import torch

import tnet_checks as K
import tnet_ref as R

ALL = K.CASES + [c[0] for c in K.SPLIT_CASES if c[0] not in K.CASES]
LOOP_CASES = [s for s in ALL if s[0] * s[1] <= 70]           # the plain loops are slow
W = 2.0 ** -10                                                # a regulariser weight that fp32 holds exactly


def _close(a, b, what):
    assert a.shape == b.shape, what
    assert (a - b).abs().max().item() <= 1e-12 * max(b.abs().max().item(), 1.0), what


# ------------------------------------------------------------------------------------------------- loops, dense, autograd
@pytest.mark.parametrize("shape", LOOP_CASES, ids=K.case_id)
def test_loops_against_dense(shape):
    X, T, G = K.inputs(shape)
    _close(R.fwd_loops(X, T), R.fwd(X, T)[0], "out")
    dX, dT = R.bwd_loops(X, T, G)
    ref = R.bwd(X, T, G)
    _close(dX, ref["dX"][0], "dX")
    _close(dT, ref["dT"][0], "dT")


def test_ortho_loops_against_dense():
    for case in [(1, "near"), (2, "random")]:
        T = K.ortho_inputs(case)
        loss, dT = R.ortho_loops(T, W)
        ref = R.ortho(T, W)
        _close(loss, ref["loss_parts"][0], "loss_parts")
        _close(dT, ref["dT"][0], "dT")


@pytest.mark.parametrize("shape", ALL, ids=K.case_id)
def test_dense_against_autograd(shape):
    X, T, G = K.inputs(shape)
    X64, T64 = X.double().requires_grad_(True), T.double().requires_grad_(True)
    out = torch.matmul(X64, T64)
    _close(R.fwd(X, T)[0], out.detach(), "out")
    out.backward(G.double())
    ref = R.bwd(X, T, G)
    _close(ref["dX"][0], X64.grad, "dX")
    _close(ref["dT"][0], T64.grad, "dT")
    for triple in (R.fwd(X, T), ref["dX"], ref["dT"]):
        assert (triple[1] >= triple[0].abs() * (1 - 1e-12)).all()
    assert R.fwd(X, T)[2] == 64 and ref["dX"][2] == 64 and ref["dT"][2] == shape[1]


@pytest.mark.parametrize("case", K.ORTHO_CASES, ids=K.case_id)
def test_ortho_against_get_loss_autograd(case):
    from scanobjectnn_amd.pointnet import pointnet_cls
    T = K.ortho_inputs(case)
    if case[1] == "near":                                      # the small difference it is in training
        assert 1e-3 < (T.double() @ T.double().transpose(1, 2) - torch.eye(64, dtype=torch.float64)).abs().max() < 0.2
    T64 = T.double().requires_grad_(True)
    pred = torch.zeros(case[0], 15, dtype=torch.float64)
    label = torch.zeros(case[0], dtype=torch.int64)
    ce = torch.nn.functional.cross_entropy(pred, label)
    reg = pointnet_cls.get_loss(pred, label, {"transform": T64}, reg_weight=W) - ce
    reg.backward()
    ref = R.ortho(T, W)
    assert abs(ref["loss_parts"][0].sum().item() - reg.item()) <= 1e-12 * max(reg.item(), 1.0)      # the SUM over the clouds
    _close(ref["dT"][0], T64.grad, "dT")
    for name in ("Gm", "loss_parts", "dT"):
        assert (ref[name][1] >= ref[name][0].abs() * (1 - 1e-12)).all() and ref[name][2] == 64


# --------------------------------------------------------------------------------------------- sequential fp32 evaluation
def _seq(terms):
    """sum of an iterable of fp32 tensors into ONE fp32 accumulator, in order"""
    acc = None
    for t in terms:
        acc = t.clone() if acc is None else acc + t
    return acc


def fp32_fwd(X, T):
    return _seq(X[:, :, i, None] * T[:, None, i, :] for i in range(64))


def fp32_bwd(X, T, G):
    dX = _seq(G[:, :, j, None] * T[:, None, :, j] for j in range(64))
    dT = _seq(X[:, p, :, None] * G[:, p, None, :] for p in range(X.shape[1]))
    return dX, dT


def fp32_ortho(T, weight):
    Gm = _seq(T[:, :, None, j] * T[:, None, :, j] for j in range(64)) - torch.eye(64)
    sq = (Gm * Gm).reshape(T.shape[0], -1)
    loss = torch.tensor(0.5 * weight) * _seq(sq[:, e] for e in range(64 * 64))
    dT = torch.tensor(2.0 * weight) * _seq(Gm[:, :, i2, None] * T[:, None, i2, :] for i2 in range(64))
    return Gm, loss, dT


def test_fp32_sequential(capsys):
    """every definition evaluated in fp32, one accumulator per element, terms in index order: inside the per-element bound
    and the family's RMS bar on every case.  The worst relative RMS per output is printed; twice the largest is
    tnet_checks.RMS_BAR."""
    worst = {}

    def note(report, case):
        for what, _, rms in report:
            if rms > worst.get(what, (0.0, None))[0]:
                worst[what] = (rms, case)

    for shape in ALL:
        X, T, G = K.inputs(shape)
        report = []
        K.check_sum(fp32_fwd(X, T), R.fwd(X, T), "fwd out", report=report)
        dX, dT = fp32_bwd(X, T, G)
        ref = R.bwd(X, T, G)
        K.check_sum(dX, ref["dX"], "bwd dX", report=report)
        K.check_sum(dT, ref["dT"], "bwd dT", report=report)
        note(report, shape)
    for case in K.ORTHO_CASES:
        T = K.ortho_inputs(case)
        report = []
        Gm, loss, dT = fp32_ortho(T, W)
        ref = R.ortho(T, W)
        K.check_sum(Gm, ref["Gm"], "ortho Gm", report=[])
        K.check_sum(loss, ref["loss_parts"], "ortho loss_parts", report=report)
        K.check_sum(dT, ref["dT"], "ortho dT", report=report)
        note(report, case)
    with capsys.disabled():
        for what, (rms, case) in sorted(worst.items()):
            print("\nfp32 sequential, worst relative RMS: %-20s %.3g at %s" % (what, rms, case), end="")
        print()
    assert max(v[0] for v in worst.values()) <= K.RMS_FP32_SEQUENTIAL_WORST * 1.005     # the recorded figure is current
    assert max(v[0] for v in worst.values()) >= K.RMS_FP32_SEQUENTIAL_WORST * 0.99


# -------------------------------------------------------------------------------------------------------- the split rule
def test_split_rule_against_the_library():
    from scanobjectnn_amd import _lib
    lib = _lib.load()
    for b in (1, 2, 3, 8, 31, 32, 33, 64, 100, 128, 255, 256, 257, 511, 512, 513, 4096):
        for n in list(range(1, 200)) + [255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2048, 4096, 8000]:
            if b * n * 64 >= 2 ** 31:
                continue
            s = K.bwd_splits(b, n)
            assert lib.pcops_transformk_supported(b, n, 64) == 1
            assert lib.pcops_transformk_bwd_splits(b, n, 64) == s, (b, n)
            assert lib.pcops_transformk_workspace_bytes(b, n, 64) == (b * s * 64 * 64 * 4 if s > 1 else 0), (b, n)
            chunk = K.bwd_chunk(n, s)
            assert chunk % K.POINT_TILE == 0 and s * chunk >= n and (s == 1 or chunk >= K.POINT_TILE)
    for (shape, splits, occupied) in K.SPLIT_CASES:
        assert K.bwd_splits(*shape) == splits, shape
        assert -(-shape[1] // K.bwd_chunk(shape[1], splits)) == occupied, shape
    assert sorted({c[1] for c in K.SPLIT_CASES}) == [1, 2, 4, 8, 16]                 # one case per count up to the cap
    assert any(c[2] < c[1] for c in K.SPLIT_CASES)                                   # ... some with splits that hold no point
    for (b, n, k) in K.UNSUPPORTED + [(0, 20, 64), (65536, 1, 64), (1 << 12, 1 << 13, 64)]:
        assert lib.pcops_transformk_supported(b, n, k) == 0
        assert lib.pcops_transformk_bwd_splits(b, n, k) == 0 and lib.pcops_transformk_workspace_bytes(b, n, k) == 0


# ------------------------------------------------------------------------------------------------- wrong restatements
def test_wrong_transform_transposed_is_rejected():
    for shape in [s for s in K.CASES if s[1] >= 15]:
        X, T, G = K.inputs(shape)
        with pytest.raises(AssertionError):
            K.check_sum(R.fwd(X, T.transpose(1, 2).contiguous())[0], R.fwd(X, T), "T transposed")
        with pytest.raises(AssertionError):
            K.check_sum(R.bwd(X, T.transpose(1, 2).contiguous(), G)["dX"][0], R.bwd(X, T, G)["dX"], "T transposed in dX")


def test_wrong_dT_without_the_tail_point_is_rejected():
    for shape in [s for s in K.CASES if s[1] >= 2]:
        X, T, G = K.inputs(shape)
        with pytest.raises(AssertionError):
            K.check_sum(R.bwd(X[:, :-1], T, G[:, :-1])["dT"][0], R.bwd(X, T, G)["dT"], "dT without the last point")


def test_wrong_regulariser_forms_are_rejected():
    eye = torch.eye(64, dtype=torch.float64)
    for case in K.ORTHO_CASES:
        T = K.ortho_inputs(case)
        ref = R.ortho(T, W)
        T64 = T.double()
        gram = T64.transpose(1, 2) @ T64 - eye                       # T^T T for T T^T: the same loss, another gradient
        with pytest.raises(AssertionError):
            K.check_sum(2 * W * (gram @ T64), ref["dT"], "T^T T")
        with pytest.raises(AssertionError):
            K.check_sum(0.5 * ref["dT"][0], ref["dT"], "the gradient without its factor 2")
        with pytest.raises(AssertionError):
            K.check_sum(ref["loss_parts"][0] * 2, ref["loss_parts"], "sum of squares without the half")


# ------------------------------------------------------------------------------------------------------------ the models
def test_pointnet_cls_basic_against_restatement():
    from scanobjectnn_amd.graph import Model
    from scanobjectnn_amd.pointnet import pointnet_cls_basic as m
    pts = torch.rand(4, 96, 3, generator=K.gen("cloud")) * 2 - 1
    net = Model(m.get_model, seed=3).build(pts)
    K.randomise(net, 4)
    names = [k for k in net.state_dict() if k.endswith("/weights")]
    assert names == ["graph.%s/weights" % s for s in ("conv1", "conv2", "conv3", "conv4", "conv5", "fc1", "fc2", "fc3")]
    assert tuple(net.state_dict()["graph.conv1/weights"].shape) == (1, 3, 1, 64)
    assert tuple(net.state_dict()["graph.fc3/weights"].shape) == (256, 15)
    with torch.no_grad():
        logits, end_points = net(pts, is_training=False)
    want = R.pointnet_cls_basic(pts.double(), R.params_from_state_dict(net.state_dict()))
    assert logits.shape == (4, 15) and end_points == {}
    assert (logits.double() - want).abs().max().item() <= 1e-5
    labels = torch.tensor([0, 3, 14, 7])
    assert abs(m.get_loss(logits, labels, end_points).item()
               - torch.nn.functional.cross_entropy(want, labels).item()) <= 1e-5
    net40 = Model(m.get_model, seed=3, num_class=40).build(pts)
    assert net40(pts, is_training=False)[0].shape == (4, 40)
    assert "num_class=15" in m.__doc__


def test_both_models_are_registered():
    from scanobjectnn_amd.pointnet2 import evaluate_scenennobjects as EV
    from scanobjectnn_amd.pointnet2 import train
    for m in ("pointnet_cls", "pointnet_cls_basic"):
        a = train.parse_args(["--model", m])
        assert (a.learning_rate, a.decay_step, a.decay_rate, a.batch_size, a.max_epoch) == (0.001, 200000, 0.7, 16, 250)
        assert a.model == m and m not in train.MASK_MODELS
        assert EV.parse_args(["--model", m]).model == m
        mod = __import__("importlib").import_module(train.MODELS[m])
        assert not hasattr(mod, "trainer") and not hasattr(mod, "flag_defaults")
    assert train.parse_args(["--model", "pointnet_cls", "--batch_size", "32"]).batch_size == 32     # the reference's batch


_CONVS = [("transform_net1/tconv1", (1, 3, 1, 64)), ("transform_net1/tconv2", (1, 1, 64, 128)),
          ("transform_net1/tconv3", (1, 1, 128, 1024)), ("transform_net1/tfc1", (1024, 512)),
          ("transform_net1/tfc2", (512, 256)), ("transform_net1/transform_XYZ", (256, 9)),
          ("conv1", (1, 3, 1, 64)), ("conv2", (1, 1, 64, 64)),
          ("transform_net2/tconv1", (1, 1, 64, 64)), ("transform_net2/tconv2", (1, 1, 64, 128)),
          ("transform_net2/tconv3", (1, 1, 128, 1024)), ("transform_net2/tfc1", (1024, 512)),
          ("transform_net2/tfc2", (512, 256)), ("transform_net2/transform_feat", (256, 4096)),
          ("conv3", (1, 1, 64, 64)), ("conv4", (1, 1, 64, 128)), ("conv5", (1, 1, 128, 1024)),
          ("fc1", (1024, 512)), ("fc2", (512, 256)), ("fc3", (256, 15))]
_NO_BN = ("transform_net1/transform_XYZ", "transform_net2/transform_feat", "fc3")


def pointnet_cls_variables():
    """names and shapes of pointnet_cls's state dict, in creation order: the trainable variables, then the moving statistics"""
    out = []
    for scope, shape in _CONVS:
        out += [("graph.%s/weights" % scope, shape), ("graph.%s/biases" % scope, shape[-1:])]
        if scope not in _NO_BN:
            out += [("graph.%s/bn/beta" % scope, shape[-1:]), ("graph.%s/bn/gamma" % scope, shape[-1:])]
    for scope, shape in _CONVS:
        if scope not in _NO_BN:
            out += [("graph.%s/bn/moving_mean" % scope, shape[-1:]), ("graph.%s/bn/moving_variance" % scope, shape[-1:])]
    return out


def test_pointnet_cls_state_dict_is_unchanged():
    from scanobjectnn_amd.graph import Model
    from scanobjectnn_amd.pointnet import pointnet_cls as m
    net = Model(m.get_model, seed=0).build(torch.zeros(2, 32, 3))
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == pointnet_cls_variables()
    assert len(pointnet_cls_variables()) == 108


def test_ops_fall_back_to_the_torch_expressions_off_the_gpu(monkeypatch):
    from scanobjectnn_amd.pointnet import tnet_ops
    X, T, _ = K.inputs((3, 70))
    assert torch.equal(tnet_ops.apply_feature_transform(X, T), torch.matmul(X, T))
    Tn = K.ortho_inputs((3, "near"))
    want = 0.5 * ((Tn @ Tn.transpose(1, 2) - torch.eye(64)) ** 2).sum() * 0.001
    assert torch.equal(tnet_ops.ortho_regulariser(Tn, 0.001), want)
    monkeypatch.setenv("PCOPS_POINTNET_NATIVE", "0")
    assert not tnet_ops.native_enabled()
