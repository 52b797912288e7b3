"""One training step of pointnet_cls on the GPU against float64 (tests/test_pointnet_gpu.py), as a function and as a
program: `python tests/pointnet_step.py` runs the same check in a process of its own, so that the test can repeat it under
PCOPS_POINTNET_NATIVE=0 (the torch forms of the feature transform and the regulariser) without touching its own process.

B = 8 clouds of 256 points, dropout off on both sides (the two generators cannot be aligned).  The model's own discrete
decisions -- ReLU masks and arg-max members, read back by tests/decisions.py -- are imposed on the float64 restatement, which
is built from the blocks of oracle/ref_models.py with the pooled layers (tconv3 of both T-Nets, conv5) as pooled layers, so
that what is compared is arithmetic.  The regulariser's weight is raised from 0.001 to 1 so that its gradient is a visible
share of the gradient of transform_net2/transform_feat.  Every variable's gradient: max |g - ref| <= 1e-3 max |ref|."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda:0"
B, N = 8, 256
REG_WEIGHT = 1.0
GRAD_TOL = 1e-3
LOSS_TOL = 1e-4


def randomise(net, seed):
    """non-trivial BN affine and moving statistics; a bias in front of a batch norm stays tiny (its gradient is analytically
    zero); the T-Net heads' zero weights become small so that the transforms differ from cloud to cloud"""
    g = torch.Generator().manual_seed(seed)
    names = dict(net.named_parameters())
    with torch.no_grad():
        for name, p in list(net.named_parameters()) + list(net.named_buffers()):
            if name.endswith("gamma") or name.endswith("moving_variance"):
                p.copy_((0.5 + torch.rand(p.shape, generator=g)).to(p.device))
            elif name.endswith("beta"):
                p.copy_((0.2 * torch.randn(p.shape, generator=g)).to(p.device))
            elif name.endswith("biases"):
                has_bn = name[:-len("biases")] + "bn/gamma" in names
                p.add_(((0.01 if has_bn else 0.05) * torch.randn(p.shape, generator=g)).to(p.device))
            elif name.endswith("moving_mean"):
                p.copy_((0.1 * torch.randn(p.shape, generator=g)).to(p.device))
            elif name.endswith("transform_XYZ/weights"):
                p.copy_((0.01 * torch.randn(p.shape, generator=g)).to(p.device))
            elif name.endswith("transform_feat/weights"):
                p.copy_((0.002 * torch.randn(p.shape, generator=g)).to(p.device))


def pointnet_cls_ref(point_cloud, P, training):
    """pointnet/models/pointnet_cls.py:21-75 in the blocks of oracle/ref_models.py -> (logits, feature transform); the three
    layers in front of a max over the points are pooled layers, whose arg-max decisions can be imposed"""
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
    net = R.dense(R.dense(net @ t2, P, "conv3", training), P, "conv4", training)
    net = R.dense(net, P, "conv5", training, pool_dim=1)
    net = R.dense(R.dense(net, P, "fc1", training), P, "fc2", training)
    return R.dense(net, P, "fc3", training, use_bn=False, act=False), t2


def check_step(verbose=True):
    """-> {variable: max |g - ref| / max |ref|}; raises AssertionError outside the bars"""
    import decisions as DEC
    from oracle import ref_models as R
    from scanobjectnn_amd.dgcnn import tf_util as td
    from scanobjectnn_amd.graph import Model
    from scanobjectnn_amd.pointnet import pointnet_cls as m
    from scanobjectnn_amd.synth import synth_clouds, synth_labels

    real_dropout = td.dropout
    td.dropout = lambda inputs, is_training, scope, keep_prob=0.5, noise_shape=None: inputs
    try:
        c = synth_clouds(B, N, seed=5)
        x = torch.from_numpy(c).to(DEV)
        y = torch.from_numpy(synth_labels(B, seed=5)).to(DEV)
        net = Model(m.get_model, device=DEV, seed=2).build(x)
        randomise(net, 6)
        sd = {k: v.clone() for k, v in net.state_dict().items()}
        rec = DEC.Recorder(net, DEV)
        with rec.recording():
            logits, end_points = net(x, is_training=True, bn_decay=0.9)
        loss = m.get_loss(logits, y, end_points, reg_weight=REG_WEIGHT)
        loss.backward()
        D = rec.decisions()
        got = {k[len("graph."):]: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
    finally:
        td.dropout = real_dropout

    P = {k: v.requires_grad_(v.is_floating_point())
         for k, v in R.params_from_state_dict(sd, dtype=torch.float64, device=DEV).items()}
    D64, report = R.Decisions(), {}
    with R.imposing(None, D64, None), torch.no_grad():
        pointnet_cls_ref(x.double(), P, True)
    assert set(D.relu) == set(D64.relu) and set(D.pool) == set(D64.pool), \
        (sorted(set(D.relu) ^ set(D64.relu)), sorted(set(D.pool) ^ set(D64.pool)))
    assert set(D.pool) == {"transform_net1/tconv3", "transform_net2/tconv3", "conv5"}
    with R.imposing(D, None, report):
        want, t2 = pointnet_cls_ref(x.double(), P, True)
    eye = torch.eye(64, dtype=torch.float64, device=DEV)
    diff = t2 @ t2.transpose(1, 2) - eye
    reg64 = 0.5 * REG_WEIGHT * (diff * diff).sum()
    loss64 = torch.nn.functional.cross_entropy(want, y.long()) + reg64
    loss64.backward()
    assert (logits.double() - want).abs().max().item() <= LOSS_TOL
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
            # a per-channel shift in front of a batch norm -- a bias behind which the layer's own norm follows, or the beta of
            # a layer whose max over the points goes straight into the batch-normalised tfc1 / fc1 -- has an analytically
            # zero gradient: what fp32 leaves is the rounding of the column sums of the gradient that reaches the layer's
            # output, the sums the layer's weight gradient is made of -- so it is held to the same 1e-3 of the largest
            # weight gradient of its layer
            wref = P[layer + "/weights"].grad.abs().max().item()
            assert scale <= 1e-12 and err <= GRAD_TOL * wref, (name, scale, err, wref)
            continue
        assert scale > 1e-9, name
        errs[name] = err / scale
    # the regulariser is a visible share of the gradient that reaches the feature transform's head
    reg_grad = 2 * REG_WEIGHT * (diff.detach() @ t2.detach())
    assert reg_grad.abs().max().item() > 1e-3
    if verbose:
        for name, e in sorted(errs.items(), key=lambda kv: -kv[1])[:6]:
            print("%-44s max err / max |ref| %.3g" % (name, e))
        print("loss %.6f against %.6f (regulariser %.6f); decisions that differ from the float64 run's: %d" % (
            loss.item(), loss64.item(), reg64.item(),
            sum(r["flips"] + r.get("active_flips", 0) for r in report.values())))
    worst = max(errs, key=errs.get)
    assert errs[worst] <= GRAD_TOL, (worst, errs[worst])
    return errs


if __name__ == "__main__":
    check_step()
    from scanobjectnn_amd.pointnet import tnet_ops
    print("pointnet step ok (native transform %s)" % ("on" if tnet_ops.native_enabled() else "off"))
