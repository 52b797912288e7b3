"""The float64 definitions of tests/spider_ref.py checked WITHOUT any kernel (no GPU marker): against explicit Python loops
on a tiny shape, against float64 autograd of the dense form (the expanded operand A built the way _ref_layer of
tests/test_spiderconv_gpu.py builds it), and the per-element bound of tests/edge_checks.py against an fp32 evaluation of
every definition, SEQUENTIAL in the header's order, on every case of tests/test_spider_paths_gpu.py -- the bounds must
hold for a correct fp32 implementation before any kernel is held to them.  Those runs print the relative RMS against
float64 that tests/spider_checks.RMS_BAR is derived from.  Last, the bound bites: one deliberately wrong restatement per
edge the GPU cases carry, each rejected by check_sum on the case that carries the edge."""
import numpy as np
import pytest
import torch

import spider_checks as K
import spider_ref as R

D = torch.float64
T = 5
F32 = torch.float32


def _show(report):
    for what, worst, rms in report:
        print("fp32 sequential %-40s worst err/bound %.3g  relative RMS %.3g" % (what, worst, rms))


# ------------------------------------------------------------------------------------------------------- against loops
TINY = (2, 5, 2, 3, 2)


def _phi_loop(d):
    x, y, z = (float(v) for v in d)
    return [x, y, z, x * y * z, x * y, y * z, x * z, x * x, y * y, z * z, x * x * y, x * y * y, x * x * z, x * z * z, y * y * z,
            y * z * z, x * x * x, y * y * y, z * z * z]


def test_taylor_against_loops():
    delta, theta, tbias, dg = K.taylor_inputs(11)
    ref, A, L = R.taylor_fwd(delta, theta, tbias)
    bwd = R.taylor_bwd(delta, dg)
    assert L == 20 and bwd["dtheta"][2] == 11 and bwd["dtbias"][2] == 11
    assert (delta[3] == 0).all() and (delta[0] != 0).all()
    dth, dthA = np.zeros((19, T)), np.zeros((19, T))
    for r in range(11):
        ph = _phi_loop(delta[r].double())
        for t in range(T):
            s, a = float(tbias[t]), abs(float(tbias[t]))
            for m in range(19):
                s += float(theta[m, t]) * ph[m]
                a += abs(float(theta[m, t]) * ph[m])
                dth[m, t] += ph[m] * float(dg[r, t])
                dthA[m, t] += abs(ph[m] * float(dg[r, t]))
            assert abs(ref[r, t].item() - s) < 1e-14 and abs(A[r, t].item() - a) < 1e-14
    assert np.allclose(bwd["dtheta"][0].numpy(), dth, rtol=1e-12, atol=1e-14)
    assert np.allclose(bwd["dtheta"][1].numpy(), dthA, rtol=1e-12, atol=1e-14)
    assert torch.allclose(bwd["dtbias"][0], dg.double().sum(0)) and torch.allclose(bwd["dtbias"][1], dg.double().abs().sum(0))


def test_contraction_against_loops():
    b, n, k, c, o = TINY
    feat, idx, g, w, bias, dy = K.conv_inputs(TINY)
    y, yA, L = R.conv_fwd(feat, idx, g, w, bias)
    wg, dgr = R.conv_wgrad(feat, idx, g, dy), R.conv_dgrad(feat, idx, g, w, dy)
    assert L == k * c * T + 1 and wg["dw"][2] == b * n and dgr["dfg"][2] == o + T and dgr["dg"][2] == o + c
    F, G, W, DY = feat.double().numpy(), g.double().numpy(), w.double().numpy(), dy.double().numpy()
    yl, yla = np.zeros((b, n, o)), np.zeros((b, n, o))
    dw, dwa = np.zeros((k * c * T, o)), np.zeros((k * c * T, o))
    dfg, dfga = np.zeros((b, n, k, c)), np.zeros((b, n, k, c))
    dgl, dgla = np.zeros((b, n, k, T)), np.zeros((b, n, k, T))
    for cl in range(b):
        for p in range(n):
            for oo in range(o):
                yl[cl, p, oo], yla[cl, p, oo] = float(bias[oo]), abs(float(bias[oo]))
            for j in range(k):
                src = int(idx[cl, p, j])                                   # a row of the SAME cloud
                for ch in range(c):
                    for t in range(T):
                        row = (j * c + ch) * T + t
                        a = F[cl, src, ch] * G[cl, p, j, t]
                        for oo in range(o):
                            yl[cl, p, oo] += a * W[row, oo]
                            yla[cl, p, oo] += abs(a * W[row, oo])
                            dw[row, oo] += a * DY[cl, p, oo]
                            dwa[row, oo] += abs(a * DY[cl, p, oo])
                        dA = sum(DY[cl, p, oo] * W[row, oo] for oo in range(o))
                        dAa = sum(abs(DY[cl, p, oo] * W[row, oo]) for oo in range(o))
                        dfg[cl, p, j, ch] += dA * G[cl, p, j, t]
                        dfga[cl, p, j, ch] += dAa * abs(G[cl, p, j, t])
                        dgl[cl, p, j, t] += dA * F[cl, src, ch]
                        dgla[cl, p, j, t] += dAa * abs(F[cl, src, ch])
    for got, want in ((y, yl), (yA, yla), (wg["dw"][0], dw), (wg["dw"][1], dwa), (dgr["dfg"][0], dfg), (dgr["dfg"][1], dfga),
                      (dgr["dg"][0], dgl), (dgr["dg"][1], dgla), (wg["db"][0], DY.sum((0, 1))),
                      (wg["db"][1], np.abs(DY).sum((0, 1)))):
        assert np.allclose(got.numpy(), want, rtol=1e-12, atol=1e-14)
    nob = R.conv_fwd(feat, idx, g, w, None)
    assert torch.allclose(nob[0], y - bias.double()) and torch.allclose(nob[1], yA - bias.double().abs())
    # the scatter
    dF, dFA, cnt = R.scatter_grouped(dgr["dfg"][0], idx, n)
    sl, sla, cl_ = np.zeros((b, n, c)), np.zeros((b, n, c)), np.zeros((b, n, 1))
    for cl in range(b):
        for p in range(n):
            for j in range(k):
                sl[cl, int(idx[cl, p, j])] += dfg[cl, p, j]
                sla[cl, int(idx[cl, p, j])] += np.abs(dfg[cl, p, j])
                cl_[cl, int(idx[cl, p, j])] += 1
    assert np.allclose(dF.numpy(), sl) and np.allclose(dFA.numpy(), sla) and np.array_equal(cnt.numpy(), cl_)
    assert (cnt > 1).any() and (cnt == 0).any() and not torch.equal(idx[0], idx[1])


def _gn_literal(x, gamma, beta, groups, eps):
    b, n, c = x.shape
    xg = x.reshape(b, n, groups, c // groups)
    var, mean = torch.var_mean(xg, dim=(1, 3), unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    z = ((xg - mean) * rstd).reshape(b, n, c) * gamma + beta
    return z, mean.reshape(b, groups), rstd.reshape(b, groups)


def test_group_norm_against_loops():
    shape = (2, 4, 6, 2)
    b, n, c, groups = shape
    cg = c // groups
    x, gamma, beta, dout = K.gn_inputs(shape)
    z, mean, rstd = _gn_literal(x.double(), gamma.double(), beta.double(), groups, K.EPS)
    out = torch.relu(z)
    f = R.group_norm_relu_fwd(x, gamma, beta, groups, K.EPS, mean, rstd, out)
    X = x.double().numpy()
    for cl in range(b):
        for gi in range(groups):
            vals = [X[cl, p, gi * cg + cc] for p in range(n) for cc in range(cg)]
            mu = sum(vals) / len(vals)
            va = sum((v - mu) ** 2 for v in vals) / len(vals)
            assert abs(f["mean"][0][cl, gi].item() - mu) < 1e-14 and abs(f["var"][0][cl, gi].item() - va) < 1e-14
            assert abs(f["mean"][1][cl, gi].item() - sum(abs(v) for v in vals) / len(vals)) < 1e-14
            assert abs(f["rstd"][cl, gi].item() - 1 / np.sqrt(va + K.EPS)) < 1e-9
            for p in range(n):
                for cc in range(cg):
                    ch = gi * cg + cc
                    zz = float(gamma[ch]) * (X[cl, p, ch] - mu) / np.sqrt(va + K.EPS) + float(beta[ch])
                    assert abs(f["z"][0][cl, p, ch].item() - zz) < 1e-9
                    assert abs(f["out"][0][cl, p, ch].item() - max(zz, 0.0)) < 1e-9
    assert f["mean"][2] == n * cg and not f["flips"].any() and f["flips_ok"]
    assert (f["out"][0][..., c - 1] == 0).all()                             # the gamma = 0, beta = 0 channel


# -------------------------------------------------------------------------------------------------- against autograd
def test_gradients_against_autograd_of_the_dense_form():
    b, n, k, c, o = shape = (2, 7, 3, 4, 6)
    feat, idx, g, w, bias, dy = K.conv_inputs(shape)
    delta, theta, tbias, _ = K.taylor_inputs(b * n * k)
    F, th, tb, W, bi = (t.double().requires_grad_() for t in (feat, theta, tbias, w, bias))
    d = delta.double()
    X, Y, Z = d[..., 0], d[..., 1], d[..., 2]
    phi = torch.stack([X, Y, Z, X * Y * Z, X * Y, Y * Z, X * Z, X * X, Y * Y, Z * Z, X * X * Y, X * Y * Y, X * X * Z,
                       X * Z * Z, Y * Y * Z, Y * Z * Z, X * X * X, Y * Y * Y, Z * Z * Z], -1)
    g64 = (phi @ th + tb).view(b, n, k, T)
    assert torch.allclose(R.taylor_fwd(delta, theta, tbias)[0].view(b, n, k, T), g64.detach())
    grouped = F[torch.arange(b).view(b, 1, 1), idx.long()]                  # (b, n, k, c)
    A = (grouped.unsqueeze(-1) * g64.unsqueeze(3)).reshape(b * n, k * c * T)
    y = (A @ W + bi).reshape(b, n, o)
    gs = g64.detach().float()                                             # the stored g the entry points are given
    g64s = gs.double().requires_grad_()
    A2 = (grouped.detach().unsqueeze(-1) * g64s.unsqueeze(3)).reshape(b * n, k * c * T)
    ys = (A2 @ W.detach() + bi.detach()).reshape(b, n, o)
    assert torch.allclose(R.conv_fwd(feat, idx, gs, w, bias)[0], ys.detach())
    ys.backward(dy.double())
    dgr = R.conv_dgrad(feat, idx, gs, w, dy)
    assert torch.allclose(dgr["dg"][0], g64s.grad, rtol=1e-10, atol=1e-12)
    tw = R.taylor_bwd(delta, g64s.grad)
    y.backward(dy.double())
    # with g exact (float64) the chain closes: dW, db, dF through the scatter, dtheta, dtbias
    wg = R.conv_wgrad(feat, idx, g64.detach(), dy)
    dg2 = R.conv_dgrad(feat, idx, g64.detach(), w, dy)
    assert torch.allclose(wg["dw"][0], W.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(wg["db"][0], bi.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(R.scatter_grouped(dg2["dfg"][0], idx, n)[0], F.grad, rtol=1e-10, atol=1e-12)
    tw2 = R.taylor_bwd(delta, dg2["dg"][0])
    assert torch.allclose(tw2["dtheta"][0], th.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(tw2["dtbias"][0], tb.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(tw["dtheta"][0], th.grad, rtol=1e-5, atol=1e-6)    # the stored g differs by its one rounding


@pytest.mark.parametrize("shape", [(2, 6, 12, 4), (2, 5, 8, 1), (1, 9, 16, 16)], ids=str)
def test_group_norm_backward_against_autograd(shape):
    b, n, c, groups = shape
    x, gamma, beta, dout = K.gn_inputs(shape)
    gamma[c - 1] = 0.7                                                    # autograd has no y > 0 rule for a dead channel
    x64, g64, b64 = (t.double().requires_grad_() for t in (x, gamma, beta))
    z, mean, rstd = _gn_literal(x64, g64, b64, groups, K.EPS)
    out = torch.relu(z)
    out.backward(dout.double())
    r = R.group_norm_relu_bwd(dout, x.double(), out.detach(), gamma, mean.detach(), rstd.detach(), groups)
    assert torch.allclose(r["dx"][0], x64.grad, rtol=1e-9, atol=1e-11)
    assert torch.allclose(r["dgamma"][0], g64.grad, rtol=1e-9, atol=1e-11)
    assert torch.allclose(r["dbeta"][0], b64.grad, rtol=1e-9, atol=1e-11)


# ------------------------------------------------------------------------------------------- fp32, sequential, in bound
def _phi32(delta):
    X, Y, Z = delta[:, 0], delta[:, 1], delta[:, 2]
    xx, yy, zz, xy, yz, xz = X * X, Y * Y, Z * Z, X * Y, Y * Z, X * Z
    return [X, Y, Z, xy * Z, xy, yz, xz, xx, yy, zz, xx * Y, xy * Y, xx * Z, xz * Z, yy * Z, yz * Z, xx * X, yy * Y, zz * Z]


def _seq(term, count, like):
    acc = torch.zeros_like(like)
    for i in range(count):
        acc += term(i)
    return acc


@pytest.mark.parametrize("rows", K.TAYLOR_ROWS)
def test_fp32_taylor_stays_inside_the_bound(rows):
    delta, theta, tbias, dg = K.taylor_inputs(rows)
    ph = _phi32(delta)
    s = tbias.expand(rows, T).clone()
    for m in range(19):
        s = s + ph[m].unsqueeze(1) * theta[m]
    report = []
    K.check_sum(s, R.taylor_fwd(delta, theta, tbias), "taylor_fwd g", report=report)
    terms = (torch.stack(ph + [torch.ones(rows)], 1).unsqueeze(2) * dg.unsqueeze(1)).contiguous()      # (rows, 20, T)
    acc = _seq(lambda r: terms[r], rows, terms[0])
    ref = R.taylor_bwd(delta, dg)
    K.check_sum(acc[:19], ref["dtheta"], "taylor_bwd dtheta", report=report)
    K.check_sum(acc[19], ref["dtbias"], "taylor_bwd dtbias", report=report)
    _show(report)


def _expanded32(feat, idx, g):
    b, n, k = idx.shape
    Fg = feat[torch.arange(b).view(b, 1, 1), idx.long()]
    return Fg, (Fg.unsqueeze(-1) * g.unsqueeze(3)).reshape(b * n, -1)


def fp32_conv(shape, what):
    """the three contractions in fp32, the operand A rounded as the kernels round it, every sum sequential"""
    b, n, k, c, o = shape
    feat, idx, g, w, bias, dy = K.conv_inputs(shape)
    Fg, A = _expanded32(feat, idx, g)
    P, Kd = A.shape
    dy2 = dy.reshape(P, o)
    out = {}
    if "fwd" in what:
        At = A.t().contiguous()
        out["y"] = (_seq(lambda kk: At[kk].unsqueeze(1) * w[kk], Kd, torch.zeros(P, o)) + bias).view(b, n, o)
    if "wgrad" in what:
        out["dw"] = _seq(lambda p: A[p].unsqueeze(1) * dy2[p], P, torch.zeros(Kd, o))
        out["db"] = _seq(lambda p: dy2[p], P, torch.zeros(o))
    if "dgrad" in what:
        wt, dyt = w.t().contiguous(), dy2.t().contiguous()
        dA = _seq(lambda oo: dyt[oo].unsqueeze(1) * wt[oo], o, torch.zeros(P, Kd)).view(b, n, k, c, T)
        out["dfg"] = _seq(lambda t: dA[..., t] * g[..., t].unsqueeze(3), T, torch.zeros(b, n, k, c))
        out["dg"] = _seq(lambda ch: dA[:, :, :, ch] * Fg[..., ch].unsqueeze(3), c, torch.zeros(b, n, k, T))
    return (feat, idx, g, w, bias, dy), out


@pytest.mark.parametrize("case", K.CONV_CASES, ids=K.conv_id)
def test_fp32_contraction_stays_inside_the_bound(case):
    shape = case[0]
    (feat, idx, g, w, bias, dy), got = fp32_conv(shape, ("fwd", "wgrad", "dgrad"))
    report = []
    K.check_sum(got["y"], R.conv_fwd(feat, idx, g, w, bias), "conv_fwd y %s" % (shape,), report=report)
    wg = R.conv_wgrad(feat, idx, g, dy)
    K.check_sum(got["dw"], wg["dw"], "conv_wgrad dw %s" % (shape,), report=report)
    K.check_sum(got["db"], wg["db"], "conv_wgrad db %s" % (shape,), report=report)
    dgr = R.conv_dgrad(feat, idx, g, w, dy)
    K.check_sum(got["dfg"], dgr["dfg"], "conv_dgrad dfg %s" % (shape,), report=report)
    K.check_sum(got["dg"], dgr["dg"], "conv_dgrad dg %s" % (shape,), report=report)
    if shape in K.END_TO_END:
        b, n, k, c, o = shape
        dfg = got["dfg"].reshape(-1, c)
        flat = (idx.long() + n * torch.arange(b).view(b, 1, 1)).reshape(-1)
        dF = torch.zeros(b * n, c)
        for r in range(flat.numel()):
            dF[flat[r]] += dfg[r]
        K.check_sum(dF.view(b, n, c), R.scatter_grouped(got["dfg"], idx, n), "scatter_grouped dF %s" % (shape,), report=report)
    _show(report)


def fp32_gn_fwd(x, gamma, beta, groups):
    b, n, c = x.shape
    cg = c // groups
    cnt = n * cg
    xe = x.view(b, n, groups, cg).permute(1, 3, 0, 2).reshape(cnt, b, groups).contiguous()     # element (p, cc) order
    mean = _seq(lambda e: xe[e], cnt, xe[0]) / cnt
    d = xe - mean
    var = _seq(lambda e: d[e] * d[e], cnt, xe[0]) / cnt
    rstd = 1.0 / torch.sqrt(var + torch.tensor(K.EPS, dtype=F32))
    xh = (x.view(b, n, groups, cg) - mean.view(b, 1, groups, 1)) * rstd.view(b, 1, groups, 1)
    z = gamma * xh.reshape(b, n, c) + beta
    return torch.relu(z), mean, var, rstd


def fp32_gn_bwd(dout, x, y, gamma, mean, rstd, groups):
    b, n, c = x.shape
    cg = c // groups
    cnt = n * cg
    gy = torch.where(y > 0, dout, torch.zeros(()))
    xh = ((x.view(b, n, groups, cg) - mean.view(b, 1, groups, 1)) * rstd.view(b, 1, groups, 1)).reshape(b, n, c)
    gyf, gxf = gy.reshape(b * n, c), (gy * xh).reshape(b * n, c)
    dbeta = _seq(lambda r: gyf[r], b * n, gyf[0])
    dgamma = _seq(lambda r: gxf[r], b * n, gyf[0])

    def elems(v):
        return v.view(b, n, groups, cg).permute(1, 3, 0, 2).reshape(cnt, b, groups).contiguous()
    t1, t2 = elems(gamma * gy), elems((gamma * gy) * xh)
    m1 = (_seq(lambda e: t1[e], cnt, t1[0]) / cnt).view(b, 1, groups, 1)
    m2 = (_seq(lambda e: t2[e], cnt, t1[0]) / cnt).view(b, 1, groups, 1)
    dx = rstd.view(b, 1, groups, 1) * (((gamma * gy).view(b, n, groups, cg) - m1) - xh.view(b, n, groups, cg) * m2)
    return dx.reshape(b, n, c), dgamma, dbeta, m1.view(b, groups), m2.view(b, groups)


@pytest.mark.parametrize("shape", K.GN_CASES, ids=str)
def test_fp32_group_norm_stays_inside_the_bound(shape):
    b, n, c, groups = shape
    x, gamma, beta, dout = K.gn_inputs(shape)
    out, mean, var, rstd = fp32_gn_fwd(x, gamma, beta, groups)
    f = R.group_norm_relu_fwd(x, gamma, beta, groups, K.EPS, mean, rstd, out)
    report = []
    K.check_sum(mean, f["mean"], "gn mean %s" % (shape,), report=report)
    K.check_sum(var, f["var"], "gn var %s" % (shape,), report=report)
    assert ((rstd.double() - f["rstd"]).abs() <= f["rstd_lim"]).all()
    K.check_sum(out, f["out"], "gn out %s" % (shape,), report=report)
    assert f["flips_ok"], int(f["flips"].sum())
    assert (out[..., c - 1] == 0).all() and (f["out"][0][..., c - 1] == 0).all()
    if shape in K.GN_CONST:
        cloud, grp, v = K.GN_CONST[shape]
        cg = c // groups
        assert (n * cg) & (n * cg - 1) == 0
        assert mean[cloud, grp].item() == v and var[cloud, grp].item() == 0.0
        assert rstd[cloud, grp].item() == (1.0 / torch.sqrt(torch.tensor(K.EPS, dtype=F32))).item()
        sl = slice(grp * cg, (grp + 1) * cg)
        assert torch.equal(out[cloud, :, sl], torch.relu(beta[sl]).expand(n, cg))
    dx, dgamma, dbeta, m1, m2 = fp32_gn_bwd(dout, x, out, gamma, mean, rstd, groups)
    r = R.group_norm_relu_bwd(dout, x, out, gamma, mean, rstd, groups)
    assert (r["gy"][..., c - 1] == 0).all()
    K.check_sum(dgamma, r["dgamma"], "gn dgamma %s" % (shape,), report=report)
    K.check_sum(dbeta, r["dbeta"], "gn dbeta %s" % (shape,), report=report)
    K.check_sum(m1, r["m1"], "gn m1 %s" % (shape,), report=report)
    K.check_sum(m2, r["m2"], "gn m2 %s" % (shape,), report=report)
    K.check_sum(dx, r["dx"], "gn dx %s" % (shape,), report=report)
    _show(report)


def test_mask_margin_is_a_condition():
    """a decision that differs from float64's with |z| beyond its bound is refused, however few there are"""
    shape = (2, 50, 112, 16)
    x, gamma, beta, dout = K.gn_inputs(shape)
    out, mean, var, rstd = fp32_gn_fwd(x, gamma, beta, shape[3])
    wrong = out.clone()
    pos = torch.nonzero(out > 0.5)[0]
    wrong[tuple(pos)] = 0.0                                               # one active element switched off
    f = R.group_norm_relu_fwd(x, gamma, beta, shape[3], K.EPS, mean, rstd, wrong)
    assert int(f["flips"].sum()) == 1 and not f["flips_ok"]


# ---------------------------------------------------------------------------------------------------- the bound bites
def _rejects(out, triple, what):
    with pytest.raises(AssertionError):
        K.check_sum(out, triple, what)


RAGGED, TAIL = (2, 300, 20, 40, 80), (3, 65, 7, 17, 48)


def test_a_dropped_row_tile_is_rejected():
    """rows >= 64 floor(n / 64) left zero: the one-row tail tile of n = 65"""
    feat, idx, g, w, bias, dy = K.conv_inputs(TAIL)
    ref = R.conv_fwd(feat, idx, g, w, bias)
    wrong = ref[0].clone()
    wrong[:, 64:] = 0
    _rejects(wrong, ref, "y")
    dgr = R.conv_dgrad(feat, idx, g, w, dy)
    for name in ("dfg", "dg"):
        wrong = dgr[name][0].clone()
        wrong[:, 64:] = 0
        _rejects(wrong, dgr[name], name)


def test_a_dropped_channel_tail_is_rejected():
    """c >= 16 floor(C / 16) dropped: channel 16 of C = 17, in all three contractions"""
    feat, idx, g, w, bias, dy = K.conv_inputs(TAIL)
    cut = feat.clone()
    cut[..., 16:] = 0
    _rejects(R.conv_fwd(cut, idx, g, w, bias)[0], R.conv_fwd(feat, idx, g, w, bias), "y")
    _rejects(R.conv_wgrad(cut, idx, g, dy)["dw"][0], R.conv_wgrad(feat, idx, g, dy)["dw"], "dw")
    dgr = R.conv_dgrad(feat, idx, g, w, dy)
    _rejects(R.conv_dgrad(cut, idx, g, w, dy)["dg"][0], dgr["dg"], "dg")
    wrong = dgr["dfg"][0].clone()
    wrong[..., 16:] = 0
    _rejects(wrong, dgr["dfg"], "dfg")


def test_a_swapped_weight_row_order_is_rejected():
    """the weight row read as (j T + t) C + c where it is (j C + c) T + t"""
    b, n, k, c, o = TAIL
    feat, idx, g, w, bias, dy = K.conv_inputs(TAIL)
    wsw = w.view(k, c, T, o).transpose(1, 2).reshape(k * c * T, o).contiguous()
    _rejects(R.conv_fwd(feat, idx, g, wsw, bias)[0], R.conv_fwd(feat, idx, g, w, bias), "y")
    wg = R.conv_wgrad(feat, idx, g, dy)
    _rejects(wg["dw"][0].view(k, c, T, o).transpose(1, 2).reshape(k * c * T, o), wg["dw"], "dw")
    dgr = R.conv_dgrad(feat, idx, g, w, dy)
    _rejects(R.conv_dgrad(feat, idx, g, wsw, dy)["dg"][0], dgr["dg"], "dg")


@pytest.mark.parametrize("shape,splits,occupied", [(TAIL, 4, 4), (RAGGED, 9, 5)])
def test_a_missing_split_is_rejected(shape, splits, occupied):
    """the rows of the last split that holds any (3 rows of 195; 88 of 600) missing from dW and db"""
    b, n, k, c, o = shape
    feat, idx, g, w, bias, dy = K.conv_inputs(shape)
    chunk = K.wgrad_chunk(b, n, splits)
    first = (occupied - 1) * chunk
    assert first < b * n <= occupied * chunk
    cut = dy.clone().view(b * n, o)
    cut[first:] = 0
    ref = R.conv_wgrad(feat, idx, g, dy)
    wrong = R.conv_wgrad(feat, idx, g, cut.view(b, n, o))
    _rejects(wrong["dw"][0], ref["dw"], "dw")
    _rejects(wrong["db"][0], ref["db"], "db")


def test_a_cloud_local_neighbour_index_is_rejected():
    """the weight gradient walks all b n rows and must add the cloud's base to idx: every cloud reading cloud 0's rows"""
    feat, idx, g, w, bias, dy = K.conv_inputs(TAIL)
    local = feat[0:1].expand_as(feat).contiguous()
    _rejects(R.conv_wgrad(local, idx, g, dy)["dw"][0], R.conv_wgrad(feat, idx, g, dy)["dw"], "dw")
    _rejects(R.conv_fwd(local, idx, g, w, bias)[0], R.conv_fwd(feat, idx, g, w, bias), "y")
    _rejects(R.conv_dgrad(local, idx, g, w, dy)["dg"][0], R.conv_dgrad(feat, idx, g, w, dy)["dg"], "dg")


def test_db_from_one_column_tile_is_rejected():
    feat, idx, g, w, bias, dy = K.conv_inputs(RAGGED)
    ref = R.conv_wgrad(feat, idx, g, dy)["db"]
    wrong = ref[0].clone()
    wrong[64:] = 0
    _rejects(wrong, ref, "db")


def test_a_taylor_backward_that_stops_at_the_grid_is_rejected():
    """256 blocks of 256 threads cover 65 536 rows; the 77 rows of the second trip missing"""
    rows = 65536 + 77
    delta, theta, tbias, dg = K.taylor_inputs(rows)
    ref = R.taylor_bwd(delta, dg)
    wrong = R.taylor_bwd(delta[:65536], dg[:65536])
    _rejects(wrong["dtheta"][0], ref["dtheta"], "dtheta")
    _rejects(wrong["dtbias"][0], ref["dtbias"], "dtbias")


@pytest.mark.parametrize("shape", [(3, 33, 48, 16), (2, 50, 112, 16)], ids=str)
def test_group_norm_sums_over_the_wrong_group_are_rejected(shape):
    b, n, c, groups = shape
    cg = c // groups
    x, gamma, beta, dout = K.gn_inputs(shape)
    out, mean, var, rstd = fp32_gn_fwd(x, gamma, beta, groups)
    f = R.group_norm_relu_fwd(x, gamma, beta, groups, K.EPS, mean, rstd, out)
    omean, _, _, _ = fp32_gn_fwd(x.roll(-cg, dims=2).contiguous(), gamma, beta, groups)       # group gi reads group gi + 1
    _rejects(omean, f["mean"], "mean")
    r = R.group_norm_relu_bwd(dout, x, out, gamma, mean, rstd, groups)
    wrong = R.group_norm_relu_bwd(dout.roll(-cg, dims=2), x.roll(-cg, dims=2), out.roll(-cg, dims=2), gamma.roll(-cg),
                                  mean.roll(-1, dims=1), rstd.roll(-1, dims=1), groups)
    _rejects(wrong["m1"][0] * 1.0, r["m1"], "m1")
    _rejects(wrong["dgamma"][0], r["dgamma"], "dgamma")


@pytest.mark.parametrize("shape", [(2, 300, 80, 16), (2, 40, 512, 2)], ids=str)
def test_dx_without_the_second_mean_is_rejected(shape):
    b, n, c, groups = shape
    x, gamma, beta, dout = K.gn_inputs(shape)
    out, mean, var, rstd = fp32_gn_fwd(x, gamma, beta, groups)
    r = R.group_norm_relu_bwd(dout, x, out, gamma, mean, rstd, groups)
    cg = c // groups
    ms, rs = mean.double().view(b, 1, groups, 1), rstd.double().view(b, 1, groups, 1)
    xhat = (x.double().view(b, n, groups, cg) - ms) * rs
    wrong = r["dx"][0] + (rs * xhat * r["m2"][0].view(b, 1, groups, 1)).reshape(b, n, c)
    _rejects(wrong, r["dx"], "dx")
