"""SpiderConv on its native kernels (csrc/spider.hip, spidercnn/spider_ops.py): every entry point against float64 torch,
the whole classifier at the reference size against oracle/ref_models.spidercnn_cls_xyz in float64, the memory the
expanded operand no longer takes, bit-identical backward passes, and the trainer / evaluator end to end."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import ref_models as R
from scanobjectnn_amd import _lib
from scanobjectnn_amd.graph import Model
from scanobjectnn_amd.spidercnn import spider_ops as S
from scanobjectnn_amd.spidercnn import spidercnn_cls_xyz as m
from scanobjectnn_amd.spidercnn import tf_util as st
from scanobjectnn_amd.synth import synth_clouds, synth_labels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 5


def _rel(got, want):
    return ((got.double() - want).norm() / want.norm().clamp_min(1e-300)).item()


def _layer_inputs(b, n, k, c, o, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.from_numpy(synth_clouds(b, n, seed=seed)).to(DEV)
    idx, delta = m.front_end(x, k)
    feat = (torch.rand((b, n, c), generator=gen) if c > 3 else x.cpu()).to(DEV).contiguous()
    theta = (0.5 * torch.randn((19, T), generator=gen)).to(DEV)
    tbias = (0.2 * torch.randn(T, generator=gen)).to(DEV)
    w = (torch.randn((k * c * T, o), generator=gen) / np.sqrt(k * c)).to(DEV)
    bias = (0.1 * torch.randn(o, generator=gen)).to(DEV)
    gamma = (0.5 + torch.rand(o, generator=gen)).to(DEV)
    beta = (0.2 * torch.randn(o, generator=gen)).to(DEV)
    return feat, idx, delta, theta, tbias, w, bias, gamma, beta


def _ref_layer(feat, idx, delta, theta, tbias, w, bias, gamma, beta, groups, mask=None):
    """float64 SpiderConv (SpiderCNN/utils/tf_util.py:168-236, :407-429); mask: the ReLU decisions to impose"""
    b, n, c = feat.shape
    k, o = idx.shape[2], w.shape[1]
    X, Y, Z = delta[..., 0], delta[..., 1], delta[..., 2]
    phi = torch.stack([X, Y, Z, X * Y * Z, X * Y, Y * Z, X * Z, X * X, Y * Y, Z * Z, X * X * Y, X * Y * Y, X * X * Z,
                       X * Z * Z, Y * Y * Z, Y * Z * Z, X * X * X, Y * Y * Y, Z * Z * Z], -1)
    g = phi @ theta + tbias                                               # (B,N,k,T)
    grouped = R.batch_gather(feat, idx.long())                            # (B,N,k,C)
    A = (grouped.unsqueeze(-1) * g.unsqueeze(3)).reshape(b * n, k * c * T)
    y = (A @ w + bias).reshape(b, n, o)
    yg = y.reshape(b, n, groups, o // groups)
    var, mean = torch.var_mean(yg, dim=(1, 3), unbiased=False, keepdim=True)
    z = ((yg - mean) / torch.sqrt(var + 1e-6)).reshape(b, n, o) * gamma + beta
    out = z * mask if mask is not None else torch.relu(z)
    return g, y, z, out


def _f64(*ts):
    return [t.detach().double().requires_grad_(t.dtype.is_floating_point) if t.dtype.is_floating_point else t
            for t in ts]


# the four layers of the classifier, a ragged cloud, and a shape with a channel tail in a third K block (C = 40), a
# second 64-column tile of 16 columns (O = 80) and 5-channel groups
CASES = [(2, 512, 20, 3, 32), (2, 512, 20, 32, 64), (2, 512, 20, 64, 128), (2, 512, 20, 128, 256), (3, 300, 7, 32, 64),
         (2, 300, 20, 40, 80)]


@pytest.mark.parametrize("b,n,k,c,o", CASES)
def test_entry_points_against_float64(b, n, k, c, o):
    feat, idx, delta, theta, tbias, w, bias, gamma, beta = _layer_inputs(b, n, k, c, o, seed=c + o + n)
    groups = min(16, o)
    g = S.taylor_fwd(delta, theta, tbias)
    y = S.conv_fwd(feat, idx, g, w, bias)
    out, mean, rstd = S.group_norm_relu_fwd(y, gamma, beta, groups)
    mask = (out > 0).double()
    F64 = _f64(feat, idx, delta, theta, tbias, w, bias, gamma, beta)
    g64, y64, z64, out64 = _ref_layer(*F64, groups, mask=mask)
    assert (g.double() - g64).abs().max().item() <= 3e-5 * g64.abs().max().item()
    assert (y.double() - y64).abs().max().item() <= 3e-5 * y64.abs().max().item()
    assert (out.double() - out64).abs().max().item() <= 3e-5 * out64.abs().max().item()
    flips = int(((z64 > 0).double() != mask).sum())
    assert flips <= 2, flips                                               # rounding-level ties only

    gen = torch.Generator().manual_seed(7)
    dout = torch.randn(out.shape, generator=gen).to(DEV)
    # the float64 gradients of every variable through the whole layer
    out64.backward(dout.double())
    feat64, theta64, tbias64, w64, bias64, gamma64, beta64 = F64[0], F64[3], F64[4], F64[5], F64[6], F64[7], F64[8]
    # the native backward, entry point by entry point
    dy, dgamma, dbeta = S.group_norm_relu_bwd(dout, y, out, gamma, mean, rstd, groups)
    dw, db = S.conv_wgrad(feat, idx, g, dy)
    dfg, dg = S.conv_dgrad(feat, idx, g, w, dy)
    dtheta, dtbias = S.taylor_bwd(delta, dg)
    dfeat = S.scatter_grouped(dfg, idx, n)
    for name, got, want in (("dgamma", dgamma, gamma64.grad), ("dbeta", dbeta, beta64.grad), ("dW", dw, w64.grad),
                            ("db", db, bias64.grad), ("dF", dfeat, feat64.grad), ("dtheta", dtheta, theta64.grad),
                            ("dtbias", dtbias, tbias64.grad)):
        assert _rel(got, want) <= 1e-4, (name, _rel(got, want))
    # the autograd Function gives the same numbers as the entry points
    leaves = [t.detach().clone().requires_grad_(True) for t in (feat, theta, tbias, w, bias, gamma, beta)]
    res = S.spider_conv(leaves[0], idx, delta, *leaves[1:], groups)
    assert torch.equal(res, out)
    res.backward(dout)
    assert torch.equal(leaves[3].grad, dw) and torch.equal(leaves[2].grad, dtbias)


def test_first_layer_needs_no_feature_gradient():
    """fanConv1 reads the raw cloud: dgrad without dF still gives dg, hence dtheta"""
    feat, idx, delta, theta, tbias, w, bias, gamma, beta = _layer_inputs(2, 256, 20, 3, 32, seed=3)
    theta = theta.clone().requires_grad_(True)
    out = S.spider_conv(feat, idx, delta, theta, tbias, w, bias, gamma, beta, 16)
    out.sum().backward()
    assert theta.grad is not None and torch.isfinite(theta.grad).all() and theta.grad.abs().sum() > 0


def _no_dropout(monkeypatch):
    monkeypatch.setattr(st, "dropout", lambda inputs, is_training, scope, keep_prob=0.5, noise_shape=None: inputs)


def _randomise(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in list(net.named_parameters()) + list(net.named_buffers()):
            if name.endswith("gamma"):
                p.copy_((0.5 + torch.rand(p.shape, generator=g)).to(p.device))
            elif name.endswith("beta") or name.endswith("taylor/biases"):
                p.copy_((0.2 * torch.randn(p.shape, generator=g)).to(p.device))
            elif name.endswith("moving_variance"):
                p.copy_((0.5 + torch.rand(p.shape, generator=g)).to(p.device))


@contextlib.contextmanager
def _recording_spider_and_topk(rec):
    """the product pass's own decisions: each SpiderConv layer's ReLU mask and the top-k pool's indices"""
    real_conv, real_topk = S.spider_conv, torch.topk

    def conv(*a, **kw):
        out = real_conv(*a, **kw)
        rec["relu"].append((out.detach() > 0))
        return out

    def topk(x, *a, **kw):
        res = real_topk(x, *a, **kw)
        rec["topk"].append(res.indices)
        return res
    S.spider_conv, torch.topk = conv, topk
    try:
        yield
    finally:
        S.spider_conv, torch.topk = real_conv, real_topk


@contextlib.contextmanager
def _imposing_spider_and_topk(rec, report):
    """evaluate ref_models.spidercnn_cls_xyz with those decisions: the first four torch.relu calls are the SpiderConv
    layers (masks imposed, flips counted with their float64 pre-activation), the top-k pool takes the product's
    members; every later ReLU (the FC head) is the float64 run's own"""
    real_relu, real_topk = torch.relu, torch.topk
    state = {"relu": 0}

    def relu(z):
        i = state["relu"]
        state["relu"] += 1
        if i >= len(rec["relu"]):
            return real_relu(z)
        mask = rec["relu"][i].to(z.device)
        own = z.detach() > 0
        flipped = own != mask
        report["relu_flips"] += int(flipped.sum())
        if flipped.any():
            report["worst_abs_z"] = max(report["worst_abs_z"], z.detach()[flipped].abs().max().item())
        return z * mask.to(z.dtype)

    def topk(x, k, dim=-1, *a, **kw):
        own = real_topk(x, k, dim=dim).indices
        ind = rec["topk"][0].to(x.device)
        report["topk_flips"] += int((own != ind).sum())
        return torch.return_types.topk((torch.gather(x, dim, ind), ind))
    torch.relu, torch.topk = relu, topk
    try:
        yield
    finally:
        torch.relu, torch.topk = real_relu, real_topk


def test_model_step_against_float64_at_reference_size(monkeypatch):
    """B = 16, N = 1024, one train-mode step: logits within 1e-4 of the float64 restatement (evaluated on the GPU),
    every variable's gradient within 1e-3 of float64 autograd for the variables with >= 1e-4 of the gradient norm"""
    _no_dropout(monkeypatch)
    c = synth_clouds(16, 1024, seed=31)
    x = torch.from_numpy(c).to(DEV)
    y = torch.from_numpy(synth_labels(16, seed=31)).to(DEV)
    net = Model(m.get_model, device=DEV, seed=4).build(x)
    _randomise(net, 17)
    P = R.params_from_state_dict(net.state_dict(), dtype=torch.float64, device=DEV)
    rec = {"relu": [], "topk": []}
    with _recording_spider_and_topk(rec):
        logits = net(x, is_training=True, bn_decay=0.9)
    m.get_loss(logits, y).backward()
    assert len(rec["relu"]) == 4 and len(rec["topk"]) == 1
    leaves = {k: v.requires_grad_(True) for k, v in P.items() if not k.endswith(("moving_mean", "moving_variance"))}
    report = {"relu_flips": 0, "worst_abs_z": 0.0, "topk_flips": 0}
    with _imposing_spider_and_topk(rec, report):
        want = R.spidercnn_cls_xyz(x.double(), P, True)
    print("decisions of the product pass that differ from float64's own: %s" % report)
    assert report["worst_abs_z"] <= 1e-4
    assert (logits.detach().double() - want).abs().max().item() <= 1e-4
    torch.nn.functional.cross_entropy(want, y.long()).backward()
    grads = {n[len("graph."):]: p.grad for n, p in net.named_parameters()}
    total = torch.sqrt(sum((v.grad.double() ** 2).sum() for v in leaves.values())).item()
    checked = 0
    for name, v in leaves.items():
        gn = v.grad.norm().item()
        if gn < 1e-4 * total:
            continue
        assert _rel(grads[name], v.grad) <= 1e-3, (name, _rel(grads[name], v.grad))
        checked += 1
    assert checked >= 20


def _step_peak(monkeypatch, native):
    monkeypatch.setenv("PCOPS_SPIDER_NATIVE", "1" if native else "0")
    x = torch.from_numpy(synth_clouds(16, 1024, seed=41)).to(DEV)
    y = torch.from_numpy(synth_labels(16, seed=41)).to(DEV)
    net = Model(m.get_model, device=DEV, seed=0).build(x)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    m.get_loss(net(x, is_training=True, bn_decay=0.9), y).backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del net
    torch.cuda.empty_cache()
    return peak


def test_no_expanded_operand_in_memory(monkeypatch):
    native = _step_peak(monkeypatch, True)
    dense = _step_peak(monkeypatch, False)
    print("peak allocated over the step: native %.1f MB, dense torch form %.1f MB" % (native / 2 ** 20, dense / 2 ** 20))
    assert native * 3 <= dense


def test_backward_bit_identical_in_deterministic_mode():
    prev = _lib.deterministic()
    _lib.set_deterministic(True)
    try:
        x = torch.from_numpy(synth_clouds(4, 512, seed=51)).to(DEV)
        y = torch.from_numpy(synth_labels(4, seed=51)).to(DEV)
        net = Model(m.get_model, device=DEV, seed=2).build(x)
        _randomise(net, 5)
        runs = []
        for _ in range(2):
            torch.manual_seed(0)
            for p in net.parameters():
                p.grad = None
            m.get_loss(net(x, is_training=True, bn_decay=0.9), y).backward()
            runs.append({n: p.grad.clone() for n, p in net.named_parameters()})
        for n in runs[0]:
            assert torch.equal(runs[0][n], runs[1][n]), n
    finally:
        _lib.set_deterministic(prev)


def test_train_and_evaluate_end_to_end(tmp_path):
    from indep_bundle import _indep_bundle
    from scanobjectnn_amd import data_utils as DU
    from scanobjectnn_amd.pointnet2 import evaluate_scenennobjects as EV
    from scanobjectnn_amd.pointnet2 import train as TR
    log_dir = tmp_path / "log"
    log = TR.train(TR.parse_args(["--model", "spidercnn_cls_xyz", "--num_point", "512", "--batch_size", "16",
                                  "--max_epoch", "1", "--synthetic_clouds", "64", "--log_dir", str(log_dir)]))
    assert len(log) == 1 and np.isfinite(log[0]["mean_loss"])
    ckpt = log_dir / "model.pt"
    assert ckpt.exists()

    raw = synth_clouds(16, 576, seed=61) * 2.0 + 0.5
    labels = synth_labels(16, seed=61)
    np.savez(tmp_path / "test.npz", data=raw, label=labels)
    want = DU.normalize_data(DU.center_data(raw.copy()))
    cur, lab = DU.get_current_data_h5(want, labels, 512, rng=np.random.RandomState(0))
    sd = torch.load(ckpt, map_location="cpu")
    prefix = str(tmp_path / "model.ckpt")
    _indep_bundle(prefix, {k[len("graph."):]: v.numpy() for k, v in sd.items()})
    for path in (str(ckpt), prefix):
        args = EV.parse_args(["--model", "spidercnn_cls_xyz", "--num_point", "512", "--batch_size", "8",
                              "--model_path", path, "--test_file", str(tmp_path / "test.npz"),
                              "--dump_dir", str(tmp_path / "dump")])
        ev = EV.evaluate(args)
        assert np.array_equal(ev["label"], lab) and np.isfinite(ev["mean_loss"])
        net = Model(m.get_model, device=DEV, seed=0).build(torch.zeros((2, 512, 3), device=DEV))
        net.load_state_dict(sd)
        with torch.no_grad():
            by_hand = np.concatenate([net(torch.from_numpy(cur[i:i + 8]).float().to(DEV), is_training=False)
                                      .argmax(dim=1).cpu().numpy() for i in range(0, 16, 8)])
        assert np.array_equal(ev["pred"], by_hand)
