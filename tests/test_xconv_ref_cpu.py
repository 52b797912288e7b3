"""The float64 definitions of tests/xconv_ref.py checked without a GPU: the plain loops against the dense forms, the dense
gradients against float64 autograd of the dense forward, a sequential fp32 evaluation of every definition inside the bounds
the GPU tests apply (its relative RMS sets the family's bar in tests/xconv_checks.py), one deliberately wrong restatement per
edge rejected by those bounds, the classifier restatement against get_model in its torch form (PCOPS_XCONV_NATIVE=0) in
float64 on the CPU, and the trainer pieces pinned to hand-computed values."""
import math

import pytest
import torch

import xconv_checks as K
import xconv_ref as R

ALL = K.CASES + [c[0] for c in K.WGRAD_CASES if c[0] not in K.CASES]
LOOP_CASES = [s for s in ALL if s[0] * s[2] <= 130]          # the plain loops are slow: up to 130 points


def _close(a, b, what):
    assert a.shape == b.shape, what
    assert (a - b).abs().max().item() <= 1e-12 * max(b.abs().max().item(), 1.0), what


# ------------------------------------------------------------------------------------------------- loops, dense, autograd
@pytest.mark.parametrize("shape", LOOP_CASES, ids=K.case_id)
def test_loops_against_dense(shape):
    lifted, fts, idx, X, wd, dout = K.inputs(shape)
    _close(R.fwd_loops(lifted, fts, idx, X, wd), R.fwd(lifted, fts, idx, X, wd)[0], "fwd")
    dX, dl, dfg = R.dgrad_loops(lifted, fts, idx, X, wd, dout)
    ref = R.dgrad(lifted, fts, idx, X, wd, dout)
    _close(dX, ref["dX"][0], "dX")
    _close(dl, ref["dlifted"][0], "dlifted")
    _close(R.wgrad_loops(lifted, fts, idx, X, wd.shape, dout), R.wgrad(lifted, fts, idx, X, wd.shape, dout)[0], "dwd")
    if fts is not None:
        _close(dfg, ref["dfg"][0], "dfg")
        _close(R.scatter_loops(dfg.float(), idx, shape[1]), R.scatter(dfg.float(), idx, shape[1])[0], "scatter")


@pytest.mark.parametrize("shape", ALL, ids=K.case_id)
def test_dense_gradients_against_autograd(shape):
    lifted, fts, idx, X, wd, dout = K.inputs(shape)
    leaves = [t.double().requires_grad_(True) if t is not None else None for t in (lifted, fts, X, wd)]
    l64, f64, X64, w64 = leaves
    full = l64 if f64 is None else torch.cat([l64, R.gather(f64, idx)], dim=-1)
    out = torch.einsum('bpjc,jcm->bpcm', X64 @ full, w64).reshape(dout.shape)
    out.backward(dout.double())
    ref = R.dgrad(lifted, fts, idx, X, wd, dout)
    _close(ref["dX"][0], X64.grad, "dX")
    _close(ref["dlifted"][0], l64.grad, "dlifted")
    _close(R.wgrad(lifted, fts, idx, X, wd.shape, dout)[0], w64.grad, "dwd")
    if fts is not None:
        # the scatter is defined on the fp32 tensor it is given; here it is fed the float64 dfg through two fp32 halves
        hi = ref["dfg"][0].float()
        lo = (ref["dfg"][0] - hi.double()).float()
        _close(R.scatter(hi, idx, shape[1])[0] + R.scatter(lo, idx, shape[1])[0], f64.grad, "dfts")
    # the magnitude sums bound the values, and the chain lengths are those of the header
    for triple in (R.fwd(lifted, fts, idx, X, wd), ref["dX"], ref["dlifted"], R.wgrad(lifted, fts, idx, X, wd.shape, dout)):
        assert (triple[1] >= triple[0].abs() * (1 - 1e-12)).all()
    k, c, dm = wd.shape
    assert R.fwd(lifted, fts, idx, X, wd)[2] == 2 * k and ref["dX"][2] == c + dm and ref["dlifted"][2] == k + dm
    assert R.wgrad(lifted, fts, idx, X, wd.shape, dout)[2] == shape[0] * shape[2] + k


# --------------------------------------------------------------------------------------------- sequential fp32 evaluation
def _seq(terms):
    """sum of an iterable of fp32 tensors into ONE fp32 accumulator, in order"""
    acc = None
    for t in terms:
        acc = t.clone() if acc is None else acc + t
    return acc


def _fin32(lifted, fts, idx):
    return lifted if fts is None else torch.cat([lifted, R.gather(fts, idx)], dim=-1)


def _t32(F_, X):
    k = X.shape[-1]
    return _seq(X[..., :, j, None] * F_[..., None, j, :] for j in range(k))              # (b, p, k', c)


def fp32_fwd(lifted, fts, idx, X, wd):
    T = _t32(_fin32(lifted, fts, idx), X)
    b, p, k, c = T.shape
    return _seq(T[:, :, j, :, None] * wd[j] for j in range(k)).reshape(b, p, -1)


def fp32_dgrad(lifted, fts, idx, X, wd, dout):
    F_ = _fin32(lifted, fts, idx)
    b, p, k, c = F_.shape
    dm = wd.shape[2]
    g = dout.reshape(b, p, 1, c, dm)
    dT = _seq(wd[None, None, :, :, m] * g[..., m] for m in range(dm))                     # (b, p, k', c)
    dX = _seq(dT[..., :, None, ch] * F_[..., None, :, ch] for ch in range(c))             # (b, p, k', k)
    dF = _seq(X[..., j, :, None] * dT[..., j, None, :] for j in range(k))                 # (b, p, k, c)
    return dX, dF


def fp32_wgrad(lifted, fts, idx, X, wd, dout):
    T = _t32(_fin32(lifted, fts, idx), X)
    b, p, k, c = T.shape
    g = dout.reshape(b * p, 1, c, -1)
    T = T.reshape(b * p, k, c, 1)
    return _seq(T[q] * g[q] for q in range(b * p))


def fp32_scatter(dfg, idx, n):
    b, p, k, c = dfg.shape
    out = torch.zeros(b, n, c)
    rows, ids = dfg.reshape(b, p * k, c), idx.reshape(b, p * k).long()
    ar = torch.arange(b)
    for j in range(p * k):
        out[ar, ids[:, j]] += rows[:, j]
    return out


def test_fp32_sequential(capsys):
    """every definition evaluated in fp32, one accumulator per element, terms in index order: inside the per-element bound
    and the family's RMS bar on every case.  The worst relative RMS per entry point is printed; twice the largest is
    xconv_checks.RMS_BAR."""
    worst = {}
    for shape in ALL:
        lifted, fts, idx, X, wd, dout = K.inputs(shape)
        report = []
        K.check_sum(fp32_fwd(lifted, fts, idx, X, wd), R.fwd(lifted, fts, idx, X, wd), "fwd out", report=report)
        dX, dF = fp32_dgrad(lifted, fts, idx, X, wd, dout)
        ref = R.dgrad(lifted, fts, idx, X, wd, dout)
        c1 = shape[4]
        K.check_sum(dX, ref["dX"], "dgrad dX", report=report)
        K.check_sum(dF[..., :c1], ref["dlifted"], "dgrad dlifted", report=report)
        K.check_sum(fp32_wgrad(lifted, fts, idx, X, wd, dout), R.wgrad(lifted, fts, idx, X, wd.shape, dout), "wgrad dwd",
                    report=report)
        if fts is not None:
            dfg = dF[..., c1:].contiguous()
            K.check_sum(dfg, ref["dfg"], "dgrad dfts_grouped", report=report)
            K.check_sum(fp32_scatter(dfg, idx, shape[1]), R.scatter(dfg, idx, shape[1]), "scatter dfts", report=report)
        for what, _, rms in report:
            if rms > worst.get(what, (0.0, None))[0]:
                worst[what] = (rms, shape)
    with capsys.disabled():
        for what, (rms, shape) in sorted(worst.items()):
            print("\nfp32 sequential, worst relative RMS: %-20s %.3g at %s" % (what, rms, shape), end="")
        print()
    assert max(v[0] for v in worst.values()) <= K.RMS_FP32_SEQUENTIAL_WORST * 1.005     # the recorded figure is current


# ------------------------------------------------------------------------------------------------- wrong restatements
def wrong_channel_order(lifted, fts, idx, X, wd):
    """output channel m c + ch instead of ch dm + m"""
    F_ = R.fin(lifted, fts, idx)
    b, p = F_.shape[:2]
    return torch.einsum('bpjc,jcm->bpmc', X.double() @ F_, wd.double()).reshape(b, p, -1)


def wrong_x_transposed(lifted, fts, idx, X, wd):
    return R.fwd(lifted, fts, idx, X.transpose(2, 3).contiguous(), wd)[0]


def wrong_padding_counted(lifted, fts, idx, X, wd):
    """K padded to 16 WITHOUT zeroing: rows K..15 of X and of wd are whatever follows in memory (the next point's rows of
    X, wrapping at the end; wd wrapping on itself)"""
    F_ = R.fin(lifted, fts, idx)
    b, p, k, c = F_.shape
    dm = wd.shape[2]
    xf, wf = X.double().reshape(-1), wd.double().reshape(-1)
    q = torch.arange(b * p).view(-1, 1, 1)
    rows, cols = torch.arange(16).view(1, -1, 1), torch.arange(k).view(1, 1, -1)
    X16 = xf[((q * k + rows) * k + cols) % xf.numel()].view(b, p, 16, k)
    w16 = wf[torch.arange(16 * c * dm) % wf.numel()].view(16, c, dm)
    return torch.einsum('bpjc,jcm->bpcm', X16 @ F_, w16).reshape(b, p, -1)


def wrong_concat_swapped(lifted, fts, idx, X, wd):
    """Fin = concat(fts[idx], lifted)"""
    F_ = torch.cat([R.gather(fts.double(), idx), lifted.double()], dim=-1)
    b, p = F_.shape[:2]
    return torch.einsum('bpjc,jcm->bpcm', X.double() @ F_, wd.double()).reshape(b, p, -1)


WRONG = [
    (wrong_channel_order, lambda s: s[6] > 1 and s[4] + s[5] > 1),
    (wrong_x_transposed, lambda s: s[3] > 1),
    (wrong_padding_counted, lambda s: s[3] < 16),
    (wrong_concat_swapped, lambda s: s[5] > 0),
]


@pytest.mark.parametrize("wrong,applies", WRONG, ids=[w[0].__name__ for w in WRONG])
def test_wrong_restatement_is_rejected(wrong, applies):
    """on every case that has the edge, the wrong form falls outside the bound the GPU test applies to the forward"""
    cases = [s for s in K.CASES if applies(s)]
    assert len(cases) >= 2
    for shape in cases:
        lifted, fts, idx, X, wd, _ = K.inputs(shape)
        with pytest.raises(AssertionError):
            K.check_sum(wrong(lifted, fts, idx, X, wd), R.fwd(lifted, fts, idx, X, wd), wrong.__name__)


# ---------------------------------------------------------------------------------------------------------- the classifier
def _recorded_model(monkeypatch, setting, seed, pts):
    """the product's classifier in its torch form, in float64 on the CPU, recording each layer's dilated neighbour indices"""
    from scanobjectnn_amd.graph import Model
    from scanobjectnn_amd.pointcnn import pointcnn_cls as m, pointfly as pf
    monkeypatch.setenv("PCOPS_XCONV_NATIVE", "0")
    seen = []
    knn = pf.knn_indices_general

    def knn_rec(queries, points, k, *a, **kw):
        out = knn(queries, points, k, *a, **kw)
        seen.append(out)
        return out

    monkeypatch.setattr(pf, "knn_indices_general", knn_rec)
    monkeypatch.setattr(torch.nn.functional, "dropout", lambda x, p=0.5, training=True, inplace=False: x)
    net = Model(m.bind(setting), seed=seed).build(pts.float()).double()
    K.randomise(net, seed + 1)
    return net, seen, m


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
def test_classifier_restatement_against_torch_form(training, monkeypatch):
    setting = K.small_setting()
    pts = torch.rand(4, 64, 3, generator=K.gen("cloud"), dtype=torch.float64) * 2 - 1
    net, seen, m = _recorded_model(monkeypatch, setting, 3, pts)
    P = R.params_from_state_dict(net.state_dict())
    for v in P.values():
        v.requires_grad_(True)
    del seen[:]
    logits = net(pts, is_training=training)
    idx = [full[:, :, ::lp['D']] for full, lp in zip(seen, setting.xconv_params)]
    assert [tuple(i.shape) for i in idx] == [(4, 64, 4), (4, 24, 6), (4, 16, 8), (4, 16, 5)]
    want = R.pointcnn_cls(pts, P, setting, training, idx)
    assert logits.shape == want.shape == ((4, 16, 15) if training else (4, 1, 15))
    assert (logits - want).abs().max().item() <= 1e-10
    labels = torch.arange(4) % 15
    m.get_loss(logits, labels).backward()
    torch.nn.functional.cross_entropy(want.reshape(-1, 15), labels.repeat_interleave(want.shape[1])).backward()
    for name, p in net.named_parameters():
        q = P[name.split("graph.", 1)[1]]
        assert (p.grad - q.grad).abs().max().item() <= 1e-9 * max(q.grad.abs().max().item(), 1e-6), name


def test_variables_round_trip_through_a_tensor_bundle(monkeypatch, tmp_path):
    """the variables carry TensorFlow's names and layouts: written as a tensor bundle and read back name for name"""
    from scanobjectnn_amd import tf_checkpoint
    from scanobjectnn_amd.graph import Model
    from scanobjectnn_amd.pointcnn import pointcnn_cls as m
    monkeypatch.setenv("PCOPS_XCONV_NATIVE", "0")
    pts = torch.rand(2, 64, 3, generator=K.gen("cloud"))
    a = Model(m.bind(K.small_setting()), seed=1).build(pts)
    K.randomise(a, 2)
    prefix = str(tmp_path / "model.ckpt")
    tf_checkpoint.save_tf_checkpoint(a, prefix)
    names = set(tf_checkpoint.read_checkpoint(prefix))
    assert {"xconv_1_X_0/kernel", "xconv_1_X_1/depthwise_weights", "xconv_2_fts_conv/depthwise_kernel",
            "xconv_2_fts_conv/pointwise_kernel", "xconv_4_fts_global_bn/gamma", "fc1_bn/moving_variance", "logits/bias"} <= names
    b = Model(m.bind(K.small_setting()), seed=9).build(pts)
    loaded, missing, unexpected = tf_checkpoint.load_tf_checkpoint(b, prefix, strict=True)
    assert not missing and not unexpected and len(loaded) == len(a.state_dict())
    assert torch.equal(a(pts, is_training=False), b(pts, is_training=False))


# ------------------------------------------------------------------------------------------------------- trainer pieces
def test_learning_rate_schedule():
    from scanobjectnn_amd.pointcnn import pointcnn_cls as m, settings as S
    from scanobjectnn_amd.pointnet2 import train
    assert S.modelnet_x3_l4.learning_rate_min == 1e-6
    lr = m.trainer(train.parse_args(["--model", "pointcnn_cls"])).learning_rate           # the setting's 0.01, 8000, 0.5
    assert lr(0) == 0.01 and lr(7999) == 0.01                                              # counted in steps, a staircase
    assert lr(8000) == 0.005 and lr(23999) == 0.0025
    assert lr(8000 * 13) == 0.01 * 0.5 ** 13                                               # 1.22e-6: still above the floor
    assert lr(8000 * 14) == 1e-6 and lr(10 ** 9) == 1e-6                                   # 6.1e-7 clipped to lr_min
    assert m.learning_rate(5, 0.1, 2, 0.1, 1e-3) == 0.1 * 0.1 ** 2 and m.learning_rate(6, 0.1, 2, 0.1, 1e-3) == 1e-3


def test_trainer_flags_fall_back_to_the_setting_for_this_model_only():
    """--learning_rate, --decay_step, --decay_rate, --batch_size and --max_epoch: the setting's values when the command line
    leaves them out, the command line's when it gives them -- in the parsed flags AND in the schedule the loop uses -- and
    every other model keeps the trainer's defaults"""
    from scanobjectnn_amd.pointcnn import pointcnn_cls as m
    from scanobjectnn_amd.pointnet2 import train
    flags = lambda a: (a.learning_rate, a.decay_step, a.decay_rate, a.batch_size, a.max_epoch)      # noqa: E731
    a = train.parse_args(["--model", "pointcnn_cls"])
    assert flags(a) == (0.01, 8000, 0.5, 32, 400) and a.setting == "modelnet_x3_l4"
    a = train.parse_args(["--model", "pointcnn_cls", "--learning_rate", "0.001", "--decay_step", "10", "--decay_rate",
                          "0.1", "--batch_size", "8", "--max_epoch", "3"])
    assert flags(a) == (0.001, 10, 0.1, 8, 3)
    own = m.trainer(a)
    assert own.learning_rate(0) == 0.001 and own.learning_rate(9) == 0.001                # the flags, not the setting's 0.01
    assert own.learning_rate(10) == 0.001 * 0.1 and own.learning_rate(20) == 0.001 * 0.1 ** 2
    assert own.learning_rate(40) == 1e-6                                                   # 1e-7 clipped: the floor is the setting's
    assert own.adam_epsilon == 1e-2
    a = train.parse_args(["--model", "pointcnn_cls", "--decay_rate", "0.25"])              # one given, the rest fall back
    assert flags(a) == (0.01, 8000, 0.25, 32, 400) and m.trainer(a).learning_rate(8000) == 0.0025
    for model in sorted(set(train.MODELS) - {"pointcnn_cls"}):
        a = train.parse_args(["--model", model])
        assert flags(a) == (0.001, 200000, 0.7, 16, 250), model
        assert not hasattr(__import__("importlib").import_module(train.MODELS[model]), "trainer")
    assert flags(train.parse_args([])) == (0.001, 200000, 0.7, 16, 250)
    assert flags(train.parse_args(["--model", "dgcnn", "--learning_rate", "0.5", "--batch_size", "4"])) == \
        (0.5, 200000, 0.7, 4, 250)


def test_regulariser_counts_kernels_gammas_and_betas():
    from scanobjectnn_amd.graph import Model
    from scanobjectnn_amd.pointcnn import pointcnn_cls as m, pointfly as pf

    def tiny(x, is_training, bn_decay=None):
        return pf.dense(pf.dense(x, 2, 'a', is_training), 2, 'logits', is_training, with_bn=False, activation=None)

    net = Model(tiny, seed=0).build(torch.zeros(1, 3, 2))
    sd = net.state_dict()
    with torch.no_grad():
        sd["graph.a/kernel"].copy_(torch.tensor([[1.0, 2.0], [3.0, 4.0]]))                # 30
        sd["graph.a_bn/gamma"].copy_(torch.tensor([2.0, 1.0]))                            # 5
        sd["graph.a_bn/beta"].copy_(torch.tensor([0.5, -0.5]))                            # 0.5
        sd["graph.logits/kernel"].copy_(torch.tensor([[1.0, 0.0], [0.0, 2.0]]))           # 5
        sd["graph.logits/bias"].copy_(torch.tensor([7.0, 7.0]))                           # not counted
        sd["graph.a_bn/moving_mean"].copy_(torch.tensor([9.0, 9.0]))                      # not a trainable variable
    assert m.regularization_loss(net, 0.25).item() == 0.25 * 40.5 / 2
    own = m.trainer(__import__("argparse").Namespace(setting="modelnet_x3_l4"))            # the setting's weight decay
    assert abs(own.regularization_loss(net).item() - 1e-5 * 40.5 / 2) < 1e-12


def test_get_xforms_is_the_elementwise_product():
    from scanobjectnn_amd.pointcnn import pointfly as pf
    g = torch.Generator().manual_seed(5)
    xf, rot = pf.get_xforms(64, rotation_range=[0.3, math.pi, 0.2, 'u'], scaling_range=[0.1, 0.2, 0.3, 'g'], generator=g)
    off = xf - torch.diag_embed(torch.diagonal(xf, dim1=1, dim2=2))
    assert (off == 0).all()                                                                # diagonal: no rotation survives
    assert (rot @ rot.transpose(1, 2) - torch.eye(3)).abs().max() < 1e-6 and (rot.abs() > 1e-3).float().mean() > 0.9
    s = torch.diagonal(xf, dim1=1, dim2=2) / torch.diagonal(rot, dim1=1, dim2=2)
    for axis, sigma in enumerate((0.1, 0.2, 0.3)):                                        # s_i: a normal clipped at 3 sigma
        assert ((s[:, axis] - 1).abs() <= 3 * sigma + 1e-5).all() and (s[:, axis] - 1).abs().max() > sigma
    # rotation about y alone, the setting's range: R_ii = (cos, 1, cos), hand-computed for one angle
    r = pf.rotation_matrices(torch.zeros(1), torch.tensor([math.pi / 3]), torch.zeros(1))[0]
    want = torch.tensor([[0.5, 0.0, math.sqrt(3) / 2], [0.0, 1.0, 0.0], [-math.sqrt(3) / 2, 0.0, 0.5]])
    assert (r - want).abs().max() < 1e-6
    # 'rxyz': x, then y, then z about the rotating axes -- Rx(90) Rz(90) sends e_x to e_z
    r = pf.rotation_matrices(torch.tensor([math.pi / 2]), torch.zeros(1), torch.tensor([math.pi / 2]))[0]
    assert (r @ torch.tensor([1.0, 0.0, 0.0]) - torch.tensor([0.0, 0.0, 1.0])).abs().max() < 1e-6
    pts = torch.tensor([[[1.0, 2.0, 3.0]]])
    assert torch.equal(pf.augment(pts, torch.diag_embed(torch.tensor([[2.0, 0.5, -1.0]])), 0.0),
                       torch.tensor([[[2.0, 1.0, -3.0]]]))                                  # jitter 0.0 adds nothing


def test_class_scores_and_loss():
    from scanobjectnn_amd.pointcnn import pointcnn_cls as m
    ln = math.log
    logits = torch.tensor([[[0.0, ln(3.0)], [ln(3.0), 0.0], [0.0, ln(3.0)]]])               # softmax rows (1/4, 3/4) ...
    assert (m.class_scores(logits) - torch.tensor([[1.25, 1.75]])).abs().max() < 1e-6
    assert m.class_scores(logits).shape == (1, 2)
    want = -(ln(0.75) + ln(0.25) + ln(0.75)) / 3                                            # label 1 tiled over three points
    assert abs(m.get_loss(logits, torch.tensor([1])).item() - want) < 1e-6


def test_dilation_takes_every_dth_neighbour(monkeypatch):
    from scanobjectnn_amd.graph import Graph
    from scanobjectnn_amd.pointcnn import pointcnn, pointfly as pf, xconv_ops
    monkeypatch.setenv("PCOPS_XCONV_NATIVE", "0")
    asked, got = [], []
    monkeypatch.setattr(pf, "knn_indices_general",
                        lambda q, p, k, *a: asked.append(k) or torch.arange(k, dtype=torch.int32).expand(2, q.shape[1], k))
    contract = xconv_ops.xconv_contract
    monkeypatch.setattr(xconv_ops, "xconv_contract", lambda l, f, i, X, w: got.append(i) or contract(l, f, i, X, w))
    with Graph(seed=0).as_default(), torch.no_grad():
        out = pointcnn.xconv(torch.rand(2, 20, 3), torch.rand(2, 20, 8), torch.rand(2, 5, 3), 't_', 2, 4, 3, 5, 16, 2, False,
                             True, 2)
    assert asked == [12] and out.shape == (2, 5, 16)
    assert torch.equal(got[0], torch.tensor([0, 3, 6, 9], dtype=torch.int32).expand(2, 5, 4))
    with pytest.raises(ValueError, match="K \\* D"):
        with Graph(seed=0).as_default():
            pointcnn.xconv(torch.rand(2, 11, 3), None, torch.rand(2, 5, 3), 't_', 2, 4, 3, 5, 16, 2, False, True, 2)


def test_settings_and_switches(monkeypatch):
    from scanobjectnn_amd._lib import PcopsError
    from scanobjectnn_amd.pointcnn import pointcnn, settings as S, xconv_ops
    s = S.modelnet_x3_l4
    assert [(l['K'], l['D'], l['P'], l['C']) for l in s.xconv_params] == [(8, 1, -1, 48), (12, 2, 384, 96), (16, 2, 128, 192),
                                                                         (16, 3, 128, 384)]
    assert (s.epsilon, s.weight_decay, s.batch_size, s.fc_params[1]['dropout_rate']) == (1e-2, 1e-5, 32, 0.8)
    with pytest.raises(AttributeError, match="sampling"):
        S.as_setting(type("Bare", (), {"xconv_params": [], "fc_params": [], "with_global": False,
                                       "with_X_transformation": True, "sorting_method": None})())
    with pytest.raises(NotImplementedError, match="ids"):
        pointcnn.sample(torch.zeros(1, 8, 3), 4, 'ids', 'xconv_2_')
    assert torch.equal(pointcnn.sample(torch.arange(24.0).view(1, 8, 3), 4, 'random', ''), torch.arange(12.0).view(1, 4, 3))
    # the native route never falls back: off the GPU it raises, and an unsupported shape names the switch
    monkeypatch.delenv("PCOPS_XCONV_NATIVE", raising=False)
    lifted, fts, idx, X, wd, _ = K.inputs((1, 9, 5, 1, 3, 5, 1))
    with pytest.raises(PcopsError, match="no CPU fallback"):
        xconv_ops.xconv_contract(lifted, fts, idx, X, wd)
    lifted, fts, idx, X, wd, _ = K.inputs(K.UNSUPPORTED[0])
    with pytest.raises(PcopsError, match="PCOPS_XCONV_NATIVE=0"):
        xconv_ops.xconv_contract(lifted, fts, idx, X, wd)
    monkeypatch.setenv("PCOPS_XCONV_NATIVE", "0")
    assert xconv_ops.xconv_contract(lifted, fts, idx, X, wd).shape == (1, 20, 16)
