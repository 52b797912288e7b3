"""Float64 definitions of the 3DmFV-Net family (include/pcops.h "3DmFV-Net", the reference's get_3dmfv at
3DmFV-Net/utils/tf_util.py:578-652 and TF's conv3d / pooling semantics), written from those and from nothing in
scanobjectnn_amd/mfv3d.  Plain torch on whatever device the inputs live on.  Sums come back as triples (ref, A, L) as in
tests/spider_ref.py: the float64 value, the magnitude sum of the terms added into the element, and their number -- what
|out - ref| <= C (L + 4) 2^-24 A of tests/edge_checks.py needs.

Layouts are the LOGICAL ones of the reference: activations (B, R, R, R, C) channel-last, weights (k, k, k, Cin, Cout),
fv (B, 20, K).  The kernels' voxel-major buffers (R^3, B, C) are `to_vm` / `from_vm` of these.  A few definitions take a
switch that selects ONE WRONG restatement (padding counted in the average, pad-before in the max pool, unmirrored taps,
L2 norm over the wrong axis, sigma read as a variance): tests/test_mfv_ref_cpu.py shows that each is rejected."""
import math

import torch
import torch.nn.functional as F

D = torch.float64


def _d(x):
    return x.to(D)


def to_vm(x):
    """(B,R,R,R,C) -> (R^3,B,C) contiguous"""
    b, r, c = x.shape[0], x.shape[1], x.shape[4]
    return x.permute(1, 2, 3, 0, 4).reshape(r * r * r, b, c).contiguous()


def from_vm(xm, r):
    """(R^3,B,C) -> (B,R,R,R,C)"""
    _, b, c = xm.shape
    return xm.reshape(r, r, r, b, c).permute(3, 0, 1, 2, 4)


# ------------------------------------------------------------------------------------------------------- representation
def get_3dmfv(points, w, mu, sigma, dtype=D, l2_axis=-1, sigma_is_variance=False):
    """get_3dmfv as written, vectorised, evaluated in `dtype`: -> (B,20,K).  Diagonal normal density, Q = w p / sum_k w p,
    d_pi = (Q - w) / (sqrt(w) n), d_mu = Q z / (n sqrt(w)), d_sigma = Q (z^2 - 1) / (n sqrt(2 w)) reduced over the points to
    max, sum / max, min, sum; sign(x) sqrt|x|; x rsqrt(max(sum_k x^2, 1e-12)) per (cloud, row)."""
    pts, w, mu, sigma = (t.to(dtype) for t in (points, w, mu, sigma))
    if sigma_is_variance:
        sigma = torch.sqrt(sigma)      # WRONG: the argument read as a variance
    n = pts.shape[1]
    z = (pts.unsqueeze(2) - mu) / sigma
    p = torch.exp(-0.5 * (z * z).sum(-1)) / ((2.0 * math.pi) ** 1.5 * sigma.prod(-1))
    wp = p * w
    Q = wp / wp.sum(-1, keepdim=True)
    d_pi_all = (Q - w) / (torch.sqrt(w) * n)
    d_pi = torch.stack([d_pi_all.amax(1), d_pi_all.sum(1)], 1)
    d_mu_all = Q.unsqueeze(-1) * z
    d_sig_all = Q.unsqueeze(-1) * (z * z - 1.0)

    def red(a, scale):
        s = torch.cat([a.amax(1), a.amin(1), a.sum(1)], 2)       # (B,K,9)
        return (scale.unsqueeze(-1) * s).permute(0, 2, 1)

    d_mu = red(d_mu_all, 1.0 / (n * torch.sqrt(w)))
    d_sigma = red(d_sig_all, 1.0 / (n * torch.sqrt(2.0 * w)))

    def norm(d):
        d = torch.sign(d) * torch.sqrt(torch.abs(d))
        return d * torch.rsqrt(torch.clamp((d * d).sum(l2_axis, keepdim=True), min=1e-12))

    return torch.cat([norm(d_pi), norm(d_mu), norm(d_sigma)], 1)


def get_3dmfv_loops(points, w, mu, sigma):
    """the same definition as explicit Python loops over clouds, points, Gaussians and axes (tiny inputs only)"""
    B, N, _ = points.shape
    K = w.shape[0]
    pts, w_, mu_, sg = (t.double().tolist() for t in (points, w, mu, sigma))
    out = torch.zeros(B, 20, K, dtype=D)
    for b in range(B):
        rows = [[None] * K for _ in range(20)]
        acc = [[[] for _ in range(K)] for _ in range(7)]          # d_pi, d_mu xyz, d_sigma xyz per point
        for i in range(N):
            wp = []
            for k in range(K):
                q = sum(((pts[b][i][a] - mu_[k][a]) / sg[k][a]) ** 2 for a in range(3))
                dens = math.exp(-0.5 * q) / ((2 * math.pi) ** 1.5 * sg[k][0] * sg[k][1] * sg[k][2])
                wp.append(w_[k] * dens)
            tot = sum(wp)
            for k in range(K):
                Q = wp[k] / tot
                acc[0][k].append((Q - w_[k]) / (math.sqrt(w_[k]) * N))
                for a in range(3):
                    z = (pts[b][i][a] - mu_[k][a]) / sg[k][a]
                    acc[1 + a][k].append(Q * z)
                    acc[4 + a][k].append(Q * (z * z - 1.0))
        for k in range(K):
            rows[0][k], rows[1][k] = max(acc[0][k]), sum(acc[0][k])
            for fam, base, scale in ((1, 2, 1.0 / (N * math.sqrt(w_[k]))), (4, 11, 1.0 / (N * math.sqrt(2 * w_[k])))):
                for a in range(3):
                    v = acc[fam + a][k]
                    rows[base + a][k], rows[base + 3 + a][k], rows[base + 6 + a][k] = \
                        scale * max(v), scale * min(v), scale * sum(v)
        for r in range(20):
            pw = [math.copysign(math.sqrt(abs(v)), v) if v != 0 else 0.0 for v in rows[r]]
            nrm = 1.0 / math.sqrt(max(sum(v * v for v in pw), 1e-12))
            for k in range(K):
                out[b, r, k] = pw[k] * nrm
    return out


# ---------------------------------------------------------------------------------------------------------- convolution
def valid_taps(r, k):
    """(R,R,R) number of taps of a k^3 SAME kernel that fall inside the grid at each voxel"""
    h = k // 2
    per = torch.tensor([sum(1 for d in range(-h, h + 1) if 0 <= i + d < r) for i in range(r)])
    return per.view(r, 1, 1) * per.view(1, r, 1) * per.view(1, 1, r)


def _pad(x, h):
    return F.pad(x, (0, 0, h, h, h, h, h, h))


def conv3d_fwd(x, w, bias=None):
    """y[b,v] = bias + sum_t x[b, v + t - h] w[t] over the zero-padded grid (TF SAME, stride 1); L = in-grid taps * Cin + 1.
    -> (ref, A, L (1,R,R,R,1))"""
    b, r, cin = x.shape[0], x.shape[1], x.shape[4]
    k, cout = w.shape[0], w.shape[4]
    h = k // 2
    xp, w64 = _pad(_d(x), h), _d(w)
    ref = torch.zeros(b, r, r, r, cout, dtype=D, device=x.device)
    mag = torch.zeros_like(ref)
    for ta in range(k):
        for tb in range(k):
            for tc in range(k):
                sl = xp[:, ta:ta + r, tb:tb + r, tc:tc + r]
                ref += sl @ w64[ta, tb, tc]
                mag += sl.abs() @ w64[ta, tb, tc].abs()
    if bias is not None:
        ref, mag = ref + _d(bias), mag + _d(bias).abs()
    L = (valid_taps(r, k).to(x.device) * cin + 1).view(1, r, r, r, 1)
    return ref, mag, L


def conv3d_valid_chain(x, w, bias=None):
    """the per-voxel chain over the in-grid taps alone, no padded operand: the form the kernel is built on"""
    b, r = x.shape[0], x.shape[1]
    k, cout = w.shape[0], w.shape[4]
    h = k // 2
    x64, w64 = _d(x), _d(w)
    out = torch.zeros(b, r, r, r, cout, dtype=D, device=x.device)
    for va in range(r):
        for vb in range(r):
            for vc in range(r):
                acc = torch.zeros(b, cout, dtype=D, device=x.device) if bias is None else _d(bias).expand(b, cout).clone()
                for ta in range(max(0, h - va), min(k, r + h - va)):
                    for tb in range(max(0, h - vb), min(k, r + h - vb)):
                        for tc in range(max(0, h - vc), min(k, r + h - vc)):
                            acc = acc + x64[:, va + ta - h, vb + tb - h, vc + tc - h] @ w64[ta, tb, tc]
                out[:, va, vb, vc] = acc
    return out


def conv3d_dgrad(w, dy, mirrored=True):
    """dx[b,u] = sum_t dy[b, u - (t - h)] w[t]^T; L = in-grid taps * Cout.  mirrored=False is the WRONG restatement that
    reads dy[u + (t - h)].  -> (ref, A, L)"""
    b, r, cout = dy.shape[0], dy.shape[1], dy.shape[4]
    k, cin = w.shape[0], w.shape[3]
    h = k // 2
    dp, w64 = _pad(_d(dy), h), _d(w)
    ref = torch.zeros(b, r, r, r, cin, dtype=D, device=dy.device)
    mag = torch.zeros_like(ref)
    for ta in range(k):
        for tb in range(k):
            for tc in range(k):
                a, b_, c = (ta, tb, tc) if not mirrored else (k - 1 - ta, k - 1 - tb, k - 1 - tc)
                sl = dp[:, a:a + r, b_:b_ + r, c:c + r]
                ref += sl @ w64[ta, tb, tc].t()
                mag += sl.abs() @ w64[ta, tb, tc].abs().t()
    L = (valid_taps(r, k).to(dy.device) * cout).view(1, r, r, r, 1)
    return ref, mag, L


def tap_rows(r, k, b):
    """(k,k,k) number of rows (in-grid voxel, cloud) a tap's weight gradient sums"""
    h = k // 2
    per = torch.tensor([sum(1 for i in range(r) if 0 <= i + d < r) for d in range(-h, h + 1)])
    return per.view(k, 1, 1) * per.view(1, k, 1) * per.view(1, 1, k) * b


def conv3d_wgrad(x, dy, k):
    """dw[t] = sum_{b, v: v + t - h in grid} x[b, v + t - h]^T dy[b, v], L = rows of the tap; db = sum_{b,v} dy, L = B R^3.
    -> dict(dw=(ref, A, L (k,k,k,1,1)), db=(ref, A, L))"""
    b, r, cin = x.shape[0], x.shape[1], x.shape[4]
    cout = dy.shape[4]
    h = k // 2
    xp, d64 = _pad(_d(x), h), _d(dy).reshape(-1, cout)
    ref = torch.zeros(k, k, k, cin, cout, dtype=D, device=x.device)
    mag = torch.zeros_like(ref)
    for ta in range(k):
        for tb in range(k):
            for tc in range(k):
                sl = xp[:, ta:ta + r, tb:tb + r, tc:tc + r].reshape(-1, cin)
                ref[ta, tb, tc] = sl.t() @ d64
                mag[ta, tb, tc] = sl.abs().t() @ d64.abs()
    L = tap_rows(r, k, b).to(x.device).clamp_min(1).view(k, k, k, 1, 1)
    return {"dw": (ref, mag, L), "db": (d64.sum(0), d64.abs().sum(0), b * r * r * r)}


# ---------------------------------------------------------------------------------------------------------------- pools
def avg_pool3d_same(x, k=3, count_padding=False):
    """TF avg_pool3d, k^3 window, stride 1, SAME: the mean over the IN-GRID elements of the window.  count_padding=True is
    the WRONG restatement that divides by k^3."""
    b, r = x.shape[0], x.shape[1]
    h = k // 2
    xp = _pad(_d(x), h)
    s = torch.zeros_like(_d(x))
    for ta in range(k):
        for tb in range(k):
            for tc in range(k):
                s += xp[:, ta:ta + r, tb:tb + r, tc:tc + r]
    cnt = float(k ** 3) if count_padding else valid_taps(r, k).to(x.device).view(1, r, r, r, 1).to(D)
    return s / cnt


def pool_windows(x, pad_before=False):
    """the 2^3 stride-2 SAME windows of x (B,R,R,R,C): (B,R',R',R',C,8), R' = ceil(R / 2), padding -inf.  TF pads AFTER the
    data when the total padding is odd (5 -> windows {0,1} {2,3} {4}); pad_before=True is the WRONG restatement."""
    r = x.shape[1]
    p = (-r) % 2
    pad = (0, 0) + ((p, 0) if pad_before else (0, p)) * 3
    xp = F.pad(x, pad, value=float("-inf"))
    ro = (r + p) // 2
    w = xp.unfold(1, 2, 2).unfold(2, 2, 2).unfold(3, 2, 2)           # (B,R',R',R',C,2,2,2)
    return w.reshape(x.shape[0], ro, ro, ro, x.shape[4], 8)


def max_pool3d_same(x, arg=None, pad_before=False):
    """TF max_pool3d 2^3 stride 2 SAME.  arg (B,R',R',R',C) int64: the window slot to take instead of the maximum (a
    decision imposed from outside)"""
    win = pool_windows(x, pad_before)
    if arg is None:
        return win.amax(-1)
    return win.gather(-1, arg.unsqueeze(-1)).squeeze(-1)


def max_pool3d_arg(x):
    """the window slot of the (first) maximum: the decision max_pool3d_same(x, arg) imposes"""
    return pool_windows(x).argmax(-1)


# ------------------------------------------------------------------------------------------------------------ classifier
BN_EPS = 1e-3


def params_from_state_dict(sd, dtype=D, device="cpu"):
    """graph.Model state dict -> {reference variable name: tensor}"""
    return {k.split("graph.", 1)[1]: v.detach().to(device=device, dtype=dtype).clone() for k, v in sd.items()
            if k.startswith("graph.")}


def _bn(x2d, P, scope, training):
    if training:
        mean = x2d.mean(0)
        var = ((x2d - mean) ** 2).mean(0)
    else:
        mean, var = P[scope + "/bn/moving_mean"], P[scope + "/bn/moving_variance"]
    return (x2d - mean) / torch.sqrt(var + BN_EPS) * P[scope + "/bn/gamma"] + P[scope + "/bn/beta"]


def _relu(x, scope, masks):
    if masks is None:
        return torch.relu(x)
    return x * masks[scope].to(x.dtype)


def _conv_layer(x, P, scope, training, masks):
    w = P[scope + "/weights"]
    k = w.shape[0]
    if k == 1:
        y = x @ w[0, 0, 0] + P[scope + "/biases"]
    else:
        y = F.conv3d(x.permute(0, 4, 1, 2, 3), w.permute(4, 3, 0, 1, 2), P[scope + "/biases"], padding=k // 2)
        y = y.permute(0, 2, 3, 4, 1)
    y = _bn(y.reshape(-1, y.shape[-1]), P, scope, training).reshape(y.shape)
    return _relu(y, scope, masks)


def _inception(x, P, scope, training, masks):
    one = _conv_layer(x, P, scope + "_conv1", training, masks)
    three = _conv_layer(one, P, scope + "_conv2", training, masks)
    five = _conv_layer(one, P, scope + "_conv3", training, masks)
    avg = _conv_layer(avg_pool3d_same(x, 3), P, scope + "_conv4", training, masks)
    return torch.cat([one, three, five, avg], 4)


def mfv3d_net_cls(points, gmm, P, training, masks=None, pool_args=None):
    """the whole classifier (3DmFV-Net/models/3dmfv_net_cls.py:29-84) in the dtype of P, dropout left out.  masks: {scope:
    bool tensor} ReLU decisions to impose (x * mask instead of relu), pool_args: {scope: window slots} for the max pools."""
    w, mu, sigma = gmm
    dt = next(iter(P.values())).dtype
    b, K = points.shape[0], w.shape[0]
    res = int(round(K ** (1.0 / 3.0)))
    fv = get_3dmfv(points, w, mu, sigma, dtype=dt)
    net = fv.reshape(b, 20, res, res, res).permute(0, 2, 3, 4, 1)
    for i in (1, 2, 3):
        net = _inception(net, P, "inception%d" % i, training, masks)
    net = max_pool3d_same(net, None if pool_args is None else pool_args["maxpool4"])
    for i in (5, 6):
        net = _inception(net, P, "inception%d" % i, training, masks)
    net = max_pool3d_same(net, None if pool_args is None else pool_args["maxpool7"])
    net = net.reshape(b, -1)
    for scope in ("fc1", "fc2", "fc3"):
        net = _relu(_bn(net @ P[scope + "/weights"] + P[scope + "/biases"], P, scope, training), scope, masks)
    return net @ P["fc4/weights"] + P["fc4/biases"], fv
