"""One training step of pointnet_seg and of pointnet_partseg on the GPU against float64 (tests/test_pointnet_seg_gpu.py), as a
function and as a program: `python tests/pointnet_seg_step.py` runs the same check in a process of its own, so that the test
can repeat it under PCOPS_CLOUD_POINT_FUSED=0 (Q = X Wx through rows_linear, then the cloud-bias arm) without touching its own
process.  The companion of tests/pointnet_step.py, whose randomise() and bars it uses unchanged.

B = 8 clouds of 1024 points (B N = 8192: the fused stacks engage), dropout off on both sides.  The model's own discrete
decisions -- ReLU masks and arg-max members, read back by tests/decisions.py -- are imposed on the float64 restatement, which
is built from the blocks of oracle/ref_models.py on the CONCATENATION [point_feat | tiled global feature], so that what is
compared is arithmetic.  The regulariser's weight is raised from 0.001 to 1 as in tests/pointnet_step.py.  Every variable's
gradient: max |g - ref| <= 1e-3 max |ref|.  The plan of the head's stack is asserted: the cloud_point arm with the switch on,
cloud_bias with it off."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import pointnet_step as PS  # noqa: E402

DEV = PS.DEV
B, N = 8, 1024
REG_WEIGHT, GRAD_TOL, LOSS_TOL = PS.REG_WEIGHT, PS.GRAD_TOL, PS.LOSS_TOL


def _ref(kind, point_cloud, P, training):
    """pointnet_seg.py:24-108 / pointnet_partseg.py:23-93 in the blocks of oracle/ref_models.py -> (class_pred | None, seg_pred,
    feature transform)"""
    from oracle import ref_models as R

    def tnet(x, scope, head, k):
        t = R.dense(R.dense(x, P, scope + "/tconv1", training), P, scope + "/tconv2", training)
        t = R.dense(t, P, scope + "/tconv3", training, pool_dim=1)
        t = R.dense(R.dense(t, P, scope + "/tfc1", training), P, scope + "/tfc2", training)
        eye = torch.eye(k, dtype=t.dtype, device=t.device).flatten()
        return (t @ P["%s/%s/weights" % (scope, head)] + (P["%s/%s/biases" % (scope, head)] + eye)).reshape(-1, k, k)

    t1 = tnet(point_cloud, "transform_net1", "transform_XYZ", 3)
    net = R.dense(R.dense(point_cloud @ t1, P, "conv1", training), P, "conv2", training)
    t2 = tnet(net, "transform_net2", "transform_feat", 64)
    point_feat = net @ t2
    net = R.dense(R.dense(point_feat, P, "conv3", training), P, "conv4", training)
    global_feat = R.dense(net, P, "conv5", training, pool_dim=1)
    class_pred = None
    if kind == "seg":
        net = R.dense(R.dense(global_feat, P, "fc1", training), P, "fc2", training)
        class_pred = R.dense(net, P, "fc3", training, use_bn=False, act=False)
    b, n, _ = point_feat.shape
    net = torch.cat([point_feat, global_feat.reshape(b, 1, -1).expand(b, n, 1024)], dim=-1)
    for i in (6, 7, 8, 9):
        net = R.dense(net, P, "conv%d" % i, training)
    return class_pred, R.dense(net, P, "conv10", training, use_bn=False, act=False), t2


def _ce(logits, labels):
    return torch.nn.functional.cross_entropy(logits.reshape(-1, logits.shape[-1]), labels.reshape(-1).long())


def check_step(kind, verbose=True):
    """kind: "seg" | "partseg" -> {variable: max |g - ref| / max |ref|}; raises AssertionError outside the bars"""
    import decisions as DEC
    from oracle import ref_models as R
    from scanobjectnn_amd import fused_mlp
    from scanobjectnn_amd.dgcnn import tf_util as td
    from scanobjectnn_amd.graph import Model
    from scanobjectnn_amd.pointnet import pointnet_partseg, pointnet_seg, seg_ops
    from scanobjectnn_amd.synth import synth_clouds, synth_labels, synth_masks

    m = pointnet_seg if kind == "seg" else pointnet_partseg
    real_dropout, real_rows = td.dropout, seg_ops.POINT_FUSED_MIN_ROWS
    td.dropout = lambda inputs, is_training, scope, keep_prob=0.5, noise_shape=None: inputs
    seg_ops.POINT_FUSED_MIN_ROWS = 0        # the switch alone decides the route: the size policy is for speed, not for shapes
    try:
        c = synth_clouds(B, N, seed=5)
        x = torch.from_numpy(c).to(DEV)
        y = torch.from_numpy(synth_labels(B, seed=5)).to(DEV)
        if kind == "seg":
            gt = torch.from_numpy(synth_masks(B, N, 5)).to(DEV)
        else:
            bands = torch.from_numpy(c[:, :, 1]).add(1.0).mul(3.0).floor().clamp(0, 5)           # six height bands
            gt = bands.int().contiguous().to(DEV)
        net = Model(m.get_model, device=DEV, seed=2).build(x)
        PS.randomise(net, 6)
        sd = {k: v.clone() for k, v in net.state_dict().items()}
        rec = DEC.Recorder(net, DEV)
        with rec.recording():
            out = net(x, is_training=True, bn_decay=0.9)
            nodes = [e for e in rec.events if not isinstance(e, tuple) and hasattr(e, "plan")]
            plans = [[lp.fwd for lp in e.plan.layers] + [e.plan.layers[0].bwd] for e in nodes]
        if kind == "seg":
            class_pred, seg_pred, end_points = out
            loss = m.get_loss(class_pred, seg_pred, y, gt, end_points, reg_weight=REG_WEIGHT)[0]
        else:
            seg_pred, end_points = out
            loss = m.get_loss(seg_pred, gt, end_points, reg_weight=REG_WEIGHT)
        loss.backward()
        D = rec.decisions()
        got = {k[len("graph."):]: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
    finally:
        td.dropout, seg_ops.POINT_FUSED_MIN_ROWS = real_dropout, real_rows

    # the head ran as ONE stack of four layers whose first arm is the one the switch selects
    head = [p for p in plans if len(p) == 5]
    arm = fused_mlp.F_CLOUD_POINT if fused_mlp.CLOUD_POINT_FUSED else fused_mlp.F_CLOUD
    assert len(head) == 1 and head[0][0] == arm and head[0][4] == arm and head[0][1:4] == [fused_mlp.F_GEMM] * 3, plans

    P = {k: v.requires_grad_(v.is_floating_point())
         for k, v in R.params_from_state_dict(sd, dtype=torch.float64, device=DEV).items()}
    D64, report = R.Decisions(), {}
    with R.imposing(None, D64, None), torch.no_grad():
        _ref(kind, x.double(), P, True)
    assert set(D.relu) == set(D64.relu) and set(D.pool) == set(D64.pool), \
        (sorted(set(D.relu) ^ set(D64.relu)), sorted(set(D.pool) ^ set(D64.pool)))
    assert set(D.pool) == {"transform_net1/tconv3", "transform_net2/tconv3", "conv5"}
    assert {"conv6", "conv7", "conv8", "conv9"} <= set(D.relu)
    with R.imposing(D, None, report):
        cp64, sp64, t2 = _ref(kind, x.double(), P, True)
    eye = torch.eye(64, dtype=torch.float64, device=DEV)
    diff = t2 @ t2.transpose(1, 2) - eye
    reg64 = 0.5 * REG_WEIGHT * (diff * diff).sum()
    loss64 = (0.5 * _ce(cp64, y) + 0.5 * _ce(sp64, gt) if kind == "seg" else _ce(sp64, gt)) + reg64
    loss64.backward()
    if verbose:
        print("%s: seg_pred max |got - ref| %.3g (max |ref| %.3g)%s" % (
            kind, (seg_pred.double() - sp64).abs().max().item(), sp64.abs().max().item(),
            "; class_pred %.3g (max |ref| %.3g)" % ((class_pred.double() - cp64).abs().max().item(), cp64.abs().max().item())
            if kind == "seg" else ""))
    # (the training-mode logits are printed, not held to the eval-mode bar of 1e-4: behind sixteen layers on batch statistics
    # the mask logits of this input differ from float64 by 1.2e-4 of 3.1 on either route, the unfused one's kernels included;
    # the eval-mode logits are held to 1e-4 in tests/test_pointnet_seg_gpu.py, and the loss to 1e-4 here)
    assert abs(loss.item() - loss64.item()) <= LOSS_TOL * max(1.0, abs(loss64.item()))
    assert set(got) == {k for k, v in P.items() if v.requires_grad and not k.endswith(("moving_mean", "moving_variance"))}
    errs = {}
    for name, g in got.items():
        ref = P[name].grad if P[name].grad is not None else torch.zeros_like(P[name])
        scale = ref.abs().max().item()
        err = (g.double() - ref).abs().max().item()
        layer = name.split("/bn/")[0] if "/bn/" in name else name.rsplit("/", 1)[0]
        shift_before_bn = (name.endswith("biases") and layer + "/bn/gamma" in got) or (
            name.endswith("/bn/beta") and layer in D.pool)
        if shift_before_bn:
            # a per-channel shift in front of a batch norm has an analytically zero gradient (tests/pointnet_step.py): held to
            # 1e-3 of the largest weight gradient of its layer.  conv5's beta stays one here: the global feature also feeds
            # conv6 through the per-cloud columns, and conv6's own norm removes a shift that is the same in every row
            wref = P[layer + "/weights"].grad.abs().max().item()
            assert scale <= 1e-12 and err <= GRAD_TOL * wref, (name, scale, err, wref)
            continue
        assert scale > 1e-9, name
        errs[name] = err / scale
    if verbose:
        for name, e in sorted(errs.items(), key=lambda kv: -kv[1])[:6]:
            print("%-44s max err / max |ref| %.3g" % (name, e))
        print("%s: loss %.6f against %.6f (regulariser %.6f); decisions that differ from the float64 run's: %d" % (
            kind, loss.item(), loss64.item(), reg64.item(),
            sum(r["flips"] + r.get("active_flips", 0) for r in report.values())))
    worst = max(errs, key=errs.get)
    assert errs[worst] <= GRAD_TOL, (worst, errs[worst])
    return errs


if __name__ == "__main__":
    for kind in sys.argv[1:] or ["seg", "partseg"]:
        check_step(kind)
    from scanobjectnn_amd import fused_mlp
    print("pointnet seg step ok (fused first conv %s)" % ("on" if fused_mlp.CLOUD_POINT_FUSED else "off"))
