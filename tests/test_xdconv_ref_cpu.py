"""The wide-channel X-Conv path and PointCNN's background-aware model checked without a GPU: the channel-group rule for every
tile count, a sequential fp32 evaluation of every definition of tests/xconv_ref.py on the wide cases (its relative RMS sets
their bar in tests/xdconv_checks.py), the float64 restatement of the model (tests/xdconv_ref.py) against the product's torch
form (PCOPS_XCONV_NATIVE=0) in float64, one wrong restatement per decoder edge rejected, the loss against hand-computed
numbers, object_dataset_x3's variables built on the CPU, and the per-model fall-back of --setting."""
import math

import pytest
import torch

import test_xconv_ref_cpu as T          # the sequential fp32 evaluations (fp32_fwd, fp32_dgrad, fp32_wgrad)
import xconv_ref as R
import xdconv_checks as K
import xdconv_ref as RD

TOL = 1e-10                             # float64 against float64


# ----------------------------------------------------------------------------------------------------------- the group rule
def test_group_rule_for_every_tile_count():
    for tiles in range(1, 61):
        for c in (16 * tiles - 15, 16 * tiles):                  # the first and the last channel count of that tile count
            groups, per = K.channel_groups(c)
            assert K.channel_groups(c, option=0) == (1, tiles)
            if tiles <= 16:
                assert (groups, per) == (1, tiles)
                continue
            sizes = [min(per, tiles - g * per) for g in range(groups)]
            assert groups == -(-tiles // 8) and sum(sizes) == tiles
            assert min(sizes) >= 1 and max(sizes) <= 8, (tiles, sizes)
    assert K.channel_groups(256) == (1, 16) and K.channel_groups(257) == (3, 6)
    table = {272: (3, 6), 300: (3, 7), 384: (3, 8), 480: (4, 8), 576: (5, 8), 960: (8, 8)}
    assert {c: K.channel_groups(c) for c in table} == table
    assert sorted(K.channel_groups(s[4] + s[5])[0] for s in K.WIDE_CASES) == [3, 3, 4, 5, 8]
    import xconv_checks
    assert all(K.channel_groups(s[4] + s[5])[0] == 1 for s in xconv_checks.CASES)


# --------------------------------------------------------------------------------------------- sequential fp32 evaluation
def test_fp32_sequential_wide(capsys):
    """every definition in fp32, one accumulator per element, terms in index order: inside the per-element bound and the wide
    cases' RMS bar.  The worst relative RMS per entry point is printed; twice the largest is xdconv_checks.RMS_BAR."""
    worst = {}
    for shape in K.WIDE_CASES:
        lifted, fts, idx, X, wd, dout = K.inputs(shape)
        report = []
        K.check_sum(T.fp32_fwd(lifted, fts, idx, X, wd), R.fwd(lifted, fts, idx, X, wd), "fwd out", report=report)
        dX, dF = T.fp32_dgrad(lifted, fts, idx, X, wd, dout)
        ref = R.dgrad(lifted, fts, idx, X, wd, dout)
        c1 = shape[4]
        K.check_sum(dX, ref["dX"], "dgrad dX", report=report)
        K.check_sum(dF[..., :c1], ref["dlifted"], "dgrad dlifted", report=report)
        K.check_sum(T.fp32_wgrad(lifted, fts, idx, X, wd, dout), R.wgrad(lifted, fts, idx, X, wd.shape, dout), "wgrad dwd",
                    report=report)
        if fts is not None:
            K.check_sum(dF[..., c1:].contiguous(), ref["dfg"], "dgrad dfts_grouped", report=report)
        for what, _, rms in report:
            if rms > worst.get(what, (0.0, None))[0]:
                worst[what] = (rms, shape)
    with capsys.disabled():
        for what, (rms, shape) in sorted(worst.items()):
            print("\nfp32 sequential, wide cases, worst relative RMS: %-20s %.3g at %s" % (what, rms, shape), end="")
        print()
    top = max(v[0] for v in worst.values())
    assert K.RMS_FP32_SEQUENTIAL_WORST / 1.005 <= top <= K.RMS_FP32_SEQUENTIAL_WORST * 1.005     # the recorded figure is current


# ------------------------------------------------------------------------------------------------------- the whole model
B, N = 3, 64


def _recorded_model(monkeypatch, seed):
    """the product's model in its torch form, in float64 on the CPU, recording each layer's dilated neighbour indices"""
    from scanobjectnn_amd.graph import Model
    from scanobjectnn_amd.pointcnn import pointcnn_seg as m, pointfly as pf
    monkeypatch.setenv("PCOPS_XCONV_NATIVE", "0")
    seen = []
    knn = pf.knn_indices_general

    def knn_rec(queries, points, k, *a, **kw):
        out = knn(queries, points, k, *a, **kw)
        seen.append(out)
        return out

    monkeypatch.setattr(pf, "knn_indices_general", knn_rec)
    monkeypatch.setattr(torch.nn.functional, "dropout", lambda x, p=0.5, training=True, inplace=False: x)
    pts = torch.rand(B, N, 3, generator=K.gen("cloud"), dtype=torch.float64) * 2 - 1
    net = Model(m.bind(K.small_seg_setting(), m.get_model), seed=seed).build(pts.float()).double()
    K.randomise(net, seed + 1)
    return net, seen, m, pts


def _indices(seen, setting):
    dil = [lp['D'] for lp in setting.xconv_params] + [dp['D'] for dp in setting.xdconv_params]
    assert len(seen) == len(dil)
    return [full[:, :, ::d] for full, d in zip(seen, dil)]


def _targets():
    labels = torch.arange(B) % 15
    mask = (torch.rand(B, N, generator=K.gen("mask")) < 0.4).long()
    return labels, mask


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
def test_model_restatement_against_torch_form(training, monkeypatch):
    setting = K.small_seg_setting()
    net, seen, m, pts = _recorded_model(monkeypatch, 3)
    P = R.params_from_state_dict(net.state_dict())
    for v in P.values():
        v.requires_grad_(True)
    del seen[:]
    cls, seg = net(pts, is_training=training)
    idx = _indices(seen, setting)
    assert [tuple(i.shape) for i in idx] == [(B, 64, 4), (B, 24, 6), (B, 16, 8), (B, 16, 5),
                                             (B, 16, 5), (B, 16, 5), (B, 24, 8), (B, 64, 6), (B, 64, 4)]
    want_cls, want_seg = RD.pointcnn_seg(pts, P, setting, training, idx)
    assert cls.shape == want_cls.shape == (B, 16, 15) and seg.shape == want_seg.shape == (B, N, 2)     # no point mean
    assert (cls - want_cls).abs().max().item() <= TOL and (seg - want_seg).abs().max().item() <= TOL
    labels, mask = _targets()
    got = m.get_loss(cls, seg, labels, mask, seg_weight=0.3)
    want = RD.loss(want_cls, want_seg, labels, mask, 0.3)
    for a, b in zip(got, want):
        assert abs(a.item() - b.item()) <= TOL
    got[0].backward()
    want[0].backward()
    for name, p in net.named_parameters():
        q = P[name.split("graph.", 1)[1]]
        assert (p.grad - q.grad).abs().max().item() <= 1e-9 * max(q.grad.abs().max().item(), 1e-6), name


@pytest.mark.parametrize("wrong", ["swapped", "front", "stage"])
def test_wrong_decoder_restatement_is_rejected(wrong, monkeypatch):
    """each decoder edge moves the mask logits far outside the tolerance of the test above, or cannot even be evaluated on
    the product's variables and indices (a swapped row asks for another layer's widths); the class head, which no decoder
    edge reaches, stays exact"""
    setting = K.small_seg_setting()
    net, seen, m, pts = _recorded_model(monkeypatch, 3)
    P = R.params_from_state_dict(net.state_dict())
    del seen[:]
    with torch.no_grad():
        cls, seg = net(pts, is_training=False)
        idx = _indices(seen, setting)
        try:
            bad_cls, bad_seg = RD.pointcnn_seg(pts, P, setting, False, idx, wrong=wrong)
        except (RuntimeError, IndexError):
            assert wrong in ("swapped", "stage")                     # shapes that no longer fit the variables
            return
    assert (cls - bad_cls).abs().max().item() <= TOL
    assert (seg - bad_seg).abs().max().item() > 1e-3


def test_mask_loss_without_its_per_cloud_mean_is_rejected():
    g = K.gen("loss")
    cls, seg = torch.randn(B, 16, 15, generator=g, dtype=torch.float64), torch.randn(B, N, 2, generator=g, dtype=torch.float64)
    labels, mask = _targets()
    from scanobjectnn_amd.pointcnn import pointcnn_seg as m
    got = m.get_loss(cls, seg, labels, mask, seg_weight=0.3)
    for a, b in zip(got, RD.loss(cls, seg, labels, mask, 0.3)):
        assert abs(a.item() - b.item()) <= TOL
    bad = RD.loss(cls, seg, labels, mask, 0.3, wrong='sum')
    assert abs(got[1].item() - bad[1].item()) <= TOL                                  # the class term is the same ...
    assert abs(got[0].item() - bad[0].item()) > 1.0 and abs(got[2].item() - bad[2].item()) > 1.0
    # and an uneven weight tells the two terms apart: total = 0.7 classify + 0.3 seg, not their mean
    assert abs(got[0].item() - (0.7 * got[1].item() + 0.3 * got[2].item())) <= TOL
    assert abs(got[0].item() - 0.5 * (got[1].item() + got[2].item())) > 1e-3


def test_loss_against_hand_computed_numbers():
    from scanobjectnn_amd.pointcnn import pointcnn_seg as m
    ln = math.log
    # two clouds, two class-head points, two classes: softmax rows (1/4, 3/4) and (3/4, 1/4) | (1/2, 1/2) twice
    cls = torch.tensor([[[0.0, ln(3.0)], [ln(3.0), 0.0]], [[0.0, 0.0], [0.0, 0.0]]])
    labels = torch.tensor([1, 0])                                           # tiled over the points
    classify = -(ln(0.75) + ln(0.25) + ln(0.5) + ln(0.5)) / 4
    # three mask points per cloud: rows (1/4, 3/4) everywhere; masks (1, 1, 0) and (0, 0, 0)
    seg = torch.tensor([0.0, ln(3.0)]).expand(2, 3, 2).contiguous()
    mask = torch.tensor([[1, 1, 0], [0, 0, 0]])
    seg_loss = 0.5 * (-(2 * ln(0.75) + ln(0.25)) / 3 - ln(0.25))
    total, c, s = m.get_loss(cls, seg, labels, mask, seg_weight=0.25)
    assert abs(c.item() - classify) < 1e-6 and abs(s.item() - seg_loss) < 1e-6
    assert abs(total.item() - (0.75 * classify + 0.25 * seg_loss)) < 1e-6
    assert abs(m.get_loss(cls, seg, labels, mask)[0].item() - 0.5 * (classify + seg_loss)) < 1e-6     # the default weight
    assert (m.class_scores(cls) - torch.tensor([[1.0, 1.0], [1.0, 1.0]])).abs().max() < 1e-6


# ------------------------------------------------------------------------------------------------- the reference's setting
def test_object_dataset_x3_variables_on_cpu(monkeypatch):
    """object_dataset_x3 at B = 1, N = 1024 in the torch form: both output shapes, the five decoder contractions
    (K, c1, c2, dm) of DESIGN.md section 4.25, and the variable names and layouts a TensorFlow checkpoint of the reference holds"""
    from scanobjectnn_amd.graph import Model
    from scanobjectnn_amd.pointcnn import pointcnn_seg as m, settings as S, xconv_ops
    monkeypatch.setenv("PCOPS_XCONV_NATIVE", "0")
    s = S.object_dataset_x3
    assert [tuple(d[k] for k in ('K', 'D', 'pts_layer_idx', 'qrs_layer_idx')) for d in s.xdconv_params] == \
        [(16, 6, 3, 3), (16, 6, 3, 2), (12, 6, 2, 1), (8, 6, 1, 0), (8, 4, 0, 0)]
    assert s.xconv_params == S.modelnet_x3_l4.xconv_params and s.data_dim == 3 and not hasattr(s, "fc_params")
    assert [(l['C'], l['dropout_rate']) for l in s.fc_params_segmentation] == [(96, 0.0), (96, 0.5)]
    assert s.fc_params_classification == S.modelnet_x3_l4.fc_params
    calls = []
    contract = xconv_ops.xconv_contract

    def rec(lifted, fts, idx, X, wd):
        calls.append((lifted.shape[1], 0 if fts is None else fts.shape[1], lifted.shape[2], lifted.shape[3],
                      0 if fts is None else fts.shape[2], wd.shape[2]))
        return contract(lifted, fts, idx, X, wd)

    monkeypatch.setattr(xconv_ops, "xconv_contract", rec)
    pts = torch.rand(1, 1024, 3, generator=K.gen("big"))
    net = Model(m.get_model, seed=0).build(pts)
    with torch.no_grad():
        cls, seg = net(pts, is_training=False)
    assert cls.shape == (1, 128, 15) and seg.shape == (1, 1024, 2)
    # (query points, source points, K, c1, c2, dm): four encoder layers, then the decoder's table
    assert calls[-9:] == [(1024, 0, 8, 24, 0, 4), (384, 1024, 12, 12, 48, 2), (128, 384, 16, 24, 96, 2),
                          (128, 128, 16, 48, 192, 2),
                          (128, 128, 16, 96, 480, 1), (128, 128, 16, 96, 384, 1), (384, 128, 12, 48, 192, 1),
                          (1024, 384, 8, 24, 96, 1), (1024, 1024, 8, 12, 48, 1)]
    sd = {k.split("graph.", 1)[1]: tuple(v.shape) for k, v in net.state_dict().items()}
    for name, shape in {"xconv_4_fts_conv/pointwise_kernel": (1, 1, 480, 384), "fc_class_0/kernel": (480, 384),
                        "fc_class_1_bn/beta": (192,), "logits_classification/kernel": (192, 15),
                        "logits_classification/bias": (15,),
                        "xdconv_1_nn_fts_from_pts_0/kernel": (3, 96), "xdconv_1_X_0/kernel": (1, 16, 3, 256),
                        "xdconv_1_X_2/depthwise_weights": (1, 16, 16, 16),
                        "xdconv_1_fts_conv/depthwise_kernel": (1, 16, 576, 1),
                        "xdconv_1_fts_conv/pointwise_kernel": (1, 1, 576, 384), "xdconv_1_fts_fuse/kernel": (864, 384),
                        "xdconv_2_fts_conv/depthwise_kernel": (1, 16, 480, 1), "xdconv_2_fts_fuse/kernel": (384, 192),
                        "xdconv_3_fts_conv/depthwise_kernel": (1, 12, 240, 1), "xdconv_3_fts_fuse_bn/gamma": (96,),
                        "xdconv_4_fts_conv/pointwise_kernel": (1, 1, 120, 48), "xdconv_4_fts_fuse/kernel": (96, 48),
                        "xdconv_5_fts_conv/depthwise_kernel": (1, 8, 60, 1), "xdconv_5_fts_fuse_bn/moving_variance": (48,),
                        "fc_seg_0/kernel": (48, 96), "fc_seg_1/kernel": (96, 96), "logits_segmentation/kernel": (96, 2),
                        "logits_segmentation/bias": (2,)}.items():
        assert sd[name] == shape, name
    assert not any(k.startswith("fc0") or k.startswith("logits/") or "fts_global" in k and k.startswith("xdconv") for k in sd)
    assert [k for k in sd if k.endswith("/bias")] == ["logits_classification/bias", "logits_segmentation/bias"]


def test_bad_decoder_row_raises(monkeypatch):
    """K D larger than the source stage's point count: xconv()'s own check, named by the decoder's tag"""
    from scanobjectnn_amd.graph import Model
    from scanobjectnn_amd.pointcnn import pointcnn_seg as m, settings as S
    monkeypatch.setenv("PCOPS_XCONV_NATIVE", "0")
    s = K.small_seg_setting()
    s.xdconv_params = S.xdconv_params([(5, 3, 3, 3), (6, 3, 3, 2)])           # 18 neighbours of 16 points
    with pytest.raises(ValueError, match="xdconv_2_: K \\* D = 18 neighbours of 16 points"):
        Model(m.bind(s, m.get_model), seed=0).build(torch.rand(2, 64, 3))


# ---------------------------------------------------------------------------------------------------- settings and flags
def test_setting_falls_back_per_model():
    from scanobjectnn_amd.pointcnn import pointcnn_cls, pointcnn_seg as m, settings as S
    from scanobjectnn_amd.pointnet2 import evaluate_scenennobjects as EV, evaluate_seg_scenennobjects as EVS, train
    assert S.get("object_dataset_x3") is S.object_dataset_x3 and S.get("modelnet_x3_l4") is S.modelnet_x3_l4
    with pytest.raises(KeyError, match="modelnet_x3_l4, object_dataset_x3"):
        S.get("nope")
    a = train.parse_args(["--model", "pointcnn_seg"])
    assert a.setting == "object_dataset_x3"
    # the trainer numbers are the classifier's hook bound to THIS model's setting; the module has no hook of its own and its
    # flags keep the trainer's defaults (tests/test_xconv_ref_cpu.py pins both for every model but pointcnn_cls)
    assert not hasattr(m, "trainer") and not hasattr(m, "flag_defaults")
    own = train.own_trainer(m, a)
    assert isinstance(own, pointcnn_cls.Trainer) and own.setting is S.object_dataset_x3
    assert own.adam_epsilon == 1e-2 and own.learning_rate(0) == 0.001                 # the flag's default, the setting's epsilon
    a = train.parse_args(["--model", "pointcnn_seg", "--learning_rate", "0.01", "--decay_step", "8000", "--decay_rate", "0.5"])
    own = train.own_trainer(m, a)
    assert own.learning_rate(7999) == 0.01 and own.learning_rate(8000) == 0.005 and own.learning_rate(10 ** 9) == 1e-6
    a = train.parse_args(["--model", "pointcnn_cls"])
    assert train.own_trainer(pointcnn_cls, a).setting is S.modelnet_x3_l4
    import importlib
    assert train.own_trainer(importlib.import_module(train.MODELS["dgcnn_bga"]), train.parse_args(["--model", "dgcnn_bga"])) is None
    assert train.parse_args(["--model", "pointcnn_cls"]).setting == "modelnet_x3_l4"
    assert train.parse_args(["--model", "dgcnn"]).setting == "modelnet_x3_l4"           # read by no other model
    assert train.parse_args(["--model", "pointcnn_seg", "--setting", "modelnet_x3_l4"]).setting == "modelnet_x3_l4"
    assert EVS.parse_args(["--model", "pointcnn_seg"]).setting == "object_dataset_x3"
    assert EV.parse_args(["--model", "pointcnn_cls"]).setting == "modelnet_x3_l4"
    assert train.MASK_MODELS == {"pointnet2_cls_bga", "dgcnn_bga", "pointcnn_seg"}
    with pytest.raises(SystemExit):
        EVS.parse_args(["--model", "pointcnn_cls"])                                     # not a mask model
    # the trainer pieces are the classifier's own objects, not copies
    for name in ("class_scores", "augment"):
        assert getattr(m, name) is getattr(pointcnn_cls, name), name
    # a setting with neither kind of head is refused; either kind is taken
    bare = dict(xconv_params=[], with_global=False, sampling='random', with_X_transformation=True, sorting_method=None)
    with pytest.raises(AttributeError, match="fc_params"):
        S.as_setting(type("Bare", (), dict(bare))())
    with pytest.raises(AttributeError, match="fc_params"):
        S.as_setting(type("Half", (), dict(bare, fc_params_classification=[]))())
    S.as_setting(type("Cls", (), dict(bare, fc_params=[]))())
    S.as_setting(type("Seg", (), dict(bare, fc_params_classification=[], fc_params_segmentation=[]))())


def test_pointcnn_cls_flag_defaults_unchanged():
    import argparse
    from scanobjectnn_amd.pointcnn import pointcnn_cls as m
    want = {"learning_rate": 0.01, "decay_step": 8000, "decay_rate": 0.5, "batch_size": 32, "max_epoch": 400}
    assert m.flag_defaults(argparse.Namespace(setting="modelnet_x3_l4")) == want
    assert m.flag_defaults(argparse.Namespace()) == want                              # no --setting, no --model
    assert m.flag_defaults(argparse.Namespace(model="pointcnn_cls", setting=None)) == want
    assert m.setting_of(argparse.Namespace()).fc_params[1] == {'C': 192, 'dropout_rate': 0.8}
