"""Float64 definitions of the per-cloud + per-point first conv (include/pcops.h "first conv of PointNet's segmentation
heads") and of the two models built on it, pointnet_seg and pointnet_partseg, written from the header and from the
reference's model files, not from scanobjectnn_amd/pointnet.  Plain torch on whatever device the inputs live on.

Every sum comes back as a triple (ref, A, L) as in tests/edge_ref.py and tests/tnet_ref.py: the float64 value, the magnitude
sum of its terms, and the length of the longest chain of roundings on an element -- what |out - ref| <= C (L + 4) 2^-24 A of
tests/edge_checks.py needs.  Each definition exists twice: as plain loops (`*_loops`) and in dense form.

Layout: X, dX (b n, k); Wx, dWx (k, c); Ctr, dCtr (b, c); Y, G (b n, c); p, q, t, pivot (c).  Row r belongs to cloud r // n.
Inputs are float32, widened, never re-rounded.

The chains (u = 2^-24):
  Y      k fused multiply-adds and the addition of Ctr: L = k + 1, A = |X| |Wx| + |Ctr|.
  S1     sum over a partial's rows of d = y - pivot.  d carries y's error, at most (k + 1 + 1) u A_d with A_d = A_y + |pivot| >=
         |d|; adding m of them in any order costs at most (m - 1) u sum |d| more, m <= rows_per_partial: L = k + 2 + m.
  S2     sum of d^2: each term's error is 2 |d| err(d) + u d^2 <= (2 (k + 2) + 1) u A_d^2, the sum adds (m - 1) u sum d^2:
         L = 2 k + 5 + m, A = sum A_d^2.
  D      p G + q Y + t as two fused multiply-adds: two roundings, A_D = |p| |G| + |q| |Y| + |t|.
  dX     c terms, each carrying D's two roundings, one more where a later pass adds to an earlier one: L = c + 3, A = A_D |Wx|^T.
  dWx    b n terms in ANY order (parts that hold no row add exact zeros): L = b n + 2, A = |X|^T A_D.
  dCtr   n terms per cloud: L = n + 2, A = sum A_D."""
import torch

D = torch.float64
BN_EPS = 1e-3


def _d(x):
    return x.to(D)


# ------------------------------------------------------------------------------------------------------------ dense forms
def fwd(b, n, X, Wx, Ctr):
    """Y[r] = X[r] Wx + Ctr[r // n]"""
    k, c = Wx.shape
    ctr = _d(Ctr).view(b, 1, c).expand(b, n, c).reshape(b * n, c)
    return _d(X) @ _d(Wx) + ctr, _d(X).abs() @ _d(Wx).abs() + ctr.abs(), k + 1


def stats(b, n, X, Wx, Ctr, pivot, rows_per_partial):
    """the shifted-moment partials [P][2][c], P = b ceil(n / rows_per_partial): partial cloud * ceil(n / rpp) + j holds the
    cloud's rows j rpp .. min(n, (j + 1) rpp) - 1; pivot None: zero.  -> (S1 triple, S2 triple)"""
    k, c = Wx.shape
    y, ay, _ = fwd(b, n, X, Wx, Ctr)
    piv = _d(pivot) if pivot is not None else torch.zeros(c, dtype=D, device=X.device)
    d, ad = (y - piv).view(b, n, c), (ay + piv.abs()).view(b, n, c)
    per = -(-n // rows_per_partial)
    pad = per * rows_per_partial - n
    if pad:
        z = torch.zeros(b, pad, c, dtype=D, device=X.device)
        d, ad = torch.cat([d, z], 1), torch.cat([ad, z], 1)
    d, ad = d.view(b * per, rows_per_partial, c), ad.view(b * per, rows_per_partial, c)
    m = min(n, rows_per_partial)
    return (d.sum(1), ad.sum(1), k + 2 + m), ((d * d).sum(1), (ad * ad).sum(1), 2 * k + 5 + m)


def dmat(G, Y, p, q, t):
    """D = p G + q Y + t and its magnitude"""
    return _d(p) * _d(G) + _d(q) * _d(Y) + _d(t), _d(p).abs() * _d(G).abs() + _d(q).abs() * _d(Y).abs() + _d(t).abs()


def bwd(b, n, G, Y, p, q, t, X, Wx):
    k, c = Wx.shape
    Dm, Ad = dmat(G, Y, p, q, t)
    X64, W64 = _d(X), _d(Wx)
    return {"dX": (Dm @ W64.t(), Ad @ W64.abs().t(), c + 3),
            "dWx": (X64.t() @ Dm, X64.abs().t() @ Ad, b * n + 2),
            "dCtr": (Dm.view(b, n, c).sum(1), Ad.view(b, n, c).sum(1), n + 2)}


# ------------------------------------------------------------------------------------------------------------ plain loops
def fwd_loops(b, n, X, Wx, Ctr, pivot, rows_per_partial):
    """-> Y, S1, S2 by walking clouds, rows and input channels"""
    k, c = Wx.shape
    per = -(-n // rows_per_partial)
    Y = torch.zeros(b * n, c, dtype=D)
    S1, S2 = torch.zeros(b * per, c, dtype=D), torch.zeros(b * per, c, dtype=D)
    piv = _d(pivot) if pivot is not None else torch.zeros(c, dtype=D)
    for cloud in range(b):
        for pt in range(n):
            r = cloud * n + pt
            y = _d(Ctr[cloud]).clone()
            for i in range(k):
                y += float(X[r, i]) * _d(Wx[i])
            Y[r] = y
            part = cloud * per + pt // rows_per_partial
            S1[part] += y - piv
            S2[part] += (y - piv) ** 2
    return Y, S1, S2


def bwd_loops(b, n, G, Y, p, q, t, X, Wx):
    k, c = Wx.shape
    dX, dWx, dCtr = torch.zeros(b * n, k, dtype=D), torch.zeros(k, c, dtype=D), torch.zeros(b, c, dtype=D)
    for cloud in range(b):
        for pt in range(n):
            r = cloud * n + pt
            drow = _d(p) * _d(G[r]) + _d(q) * _d(Y[r]) + _d(t)
            dCtr[cloud] += drow
            for i in range(k):
                dX[r, i] = (drow * _d(Wx[i])).sum()
                dWx[i] += float(X[r, i]) * drow
    return dX, dWx, dCtr


# -------------------------------------------------------------------------- float64 autograd of the layer behind a batch norm
def bn_backward_coeffs(Yv, Gm, gamma, eps=BN_EPS):
    """(p, q, t) with dY = p Gm + q Y + t for z = gamma (Y - mean) / sqrt(var + eps) + beta over the rows of Y, Gm = dL/dz:
    p = gamma rstd,  q = -p rstd^2 cov / 1,  t = -p (mean_g) - q mean   where mean_g = mean Gm, cov = mean Gm (Y - mean)"""
    mean = Yv.mean(0)
    var = ((Yv - mean) ** 2).mean(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    mg = Gm.mean(0)
    cov = (Gm * (Yv - mean)).mean(0)
    p = gamma * rstd
    q = -p * rstd * rstd * cov
    t = -p * mg - q * mean
    return p, q, t


# ----------------------------------------------------------------------------------------------------------- the two models
def params_from_state_dict(sd, device=None):
    """{TF variable name: float64 tensor} from a graph.Model state dict"""
    return {k.split("graph.", 1)[1]: v.detach().to(device=device, dtype=D).clone() for k, v in sd.items()}


def _bn(P, scope, x, training):
    flat = x.reshape(-1, x.shape[-1])
    if training:
        mean = flat.mean(0)
        var = ((flat - mean) ** 2).mean(0)
    else:
        mean, var = P[scope + '/bn/moving_mean'], P[scope + '/bn/moving_variance']
    return ((flat - mean) / torch.sqrt(var + BN_EPS) * P[scope + '/bn/gamma'] + P[scope + '/bn/beta']).reshape(x.shape)


def _layer(P, scope, x, training, bn=True, act=True):
    w = P[scope + '/weights']
    y = x @ w.reshape(-1, w.shape[-1]) + P[scope + '/biases']
    if bn:
        y = _bn(P, scope, y, training)
    return torch.relu(y) if act else y


def _tnet(P, scope, head, x, k, training):
    """transform_nets.py: tconv1..3 (64, 128, 1024), max over the points, tfc1, tfc2 (512, 256), then a (256, k k) product
    plus bias plus the identity"""
    t = x
    for name in ("tconv1", "tconv2", "tconv3"):
        t = _layer(P, "%s/%s" % (scope, name), t, training)
    t = t.amax(dim=1)
    for name in ("tfc1", "tfc2"):
        t = _layer(P, "%s/%s" % (scope, name), t, training)
    eye = torch.eye(k, dtype=t.dtype, device=t.device).flatten()
    return (t @ P["%s/%s/weights" % (scope, head)] + P["%s/%s/biases" % (scope, head)] + eye).reshape(-1, k, k)


def _front(points, P, training):
    """-> point_feat (B, N, 64), global_feat (B, 1024), feature transform (B, 64, 64)"""
    t1 = _tnet(P, "transform_net1", "transform_XYZ", points, 3, training)
    net = _layer(P, "conv2", _layer(P, "conv1", points @ t1, training), training)
    t2 = _tnet(P, "transform_net2", "transform_feat", net, 64, training)
    point_feat = net @ t2
    net = point_feat
    for i in (3, 4, 5):
        net = _layer(P, "conv%d" % i, net, training)
    return point_feat, net.amax(dim=1), t2


def _head(point_feat, global_feat, P, training):
    """conv6..9 on the CONCATENATION [point_feat | tiled global_feat], then conv10 without norm or activation"""
    b, n, _ = point_feat.shape
    net = torch.cat([point_feat, global_feat.view(b, 1, -1).expand(b, n, global_feat.shape[-1])], dim=-1)
    for i in (6, 7, 8, 9):
        net = _layer(P, "conv%d" % i, net, training)
    return _layer(P, "conv10", net, training, bn=False, act=False)


def pointnet_seg(points, P, training=False):
    """points (B, N, 3) float64 -> class_pred (B, 15), seg_pred (B, N, 2), transform; dropout is the identity"""
    point_feat, global_feat, t2 = _front(points, P, training)
    net = _layer(P, "fc2", _layer(P, "fc1", global_feat, training), training)
    class_pred = net @ P["fc3/weights"] + P["fc3/biases"]
    return class_pred, _head(point_feat, global_feat, P, training), t2


def pointnet_partseg(points, P, training=False):
    """points (B, N, 3) float64 -> seg_pred (B, N, 6), transform"""
    point_feat, global_feat, t2 = _front(points, P, training)
    return _head(point_feat, global_feat, P, training), t2


def ortho(t2, reg_weight):
    k = t2.shape[-1]
    diff = t2 @ t2.transpose(1, 2) - torch.eye(k, dtype=t2.dtype, device=t2.device)
    return 0.5 * reg_weight * (diff * diff).sum()


def seg_ce(seg_pred, gt):
    """mean over the clouds of the mean over the points of -log softmax(seg_pred)[gt]"""
    lp = torch.log_softmax(seg_pred, dim=-1)
    return -lp.gather(-1, gt.long().unsqueeze(-1)).squeeze(-1).mean(dim=1).mean()
