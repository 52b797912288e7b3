"""Float64 definitions of PointNet's per-cloud feature transform and its orthogonality regulariser (include/pcops.h
"PointNet's per-cloud feature transform") and of the pointnet_cls_basic classifier, written from the header and from the
reference's description of the model, not from scanobjectnn_amd/pointnet.  Plain torch on whatever device the inputs live on.

Every sum comes back as a triple (ref, A, L) as in tests/edge_ref.py: the float64 value, the magnitude sum of its terms, and
the length of the longest chain of roundings on an element -- what |out - ref| <= C (L + 4) 2^-24 A of tests/edge_checks.py
needs.  Each definition exists twice: as plain loops (`*_loops`) and in dense form.

Layout: X, out, G, dX (b, n, k); T, dT (b, k, k).  Inputs are float32, widened, never re-rounded."""
import torch

D = torch.float64
BN_EPS = 1e-3


def _d(x):
    return x.to(D)


# ------------------------------------------------------------------------------------------------------------ dense forms
def fwd(X, T):
    """out[c][p][j] = sum_i X[c][p][i] T[c][i][j]; L = k"""
    return _d(X) @ _d(T), _d(X).abs() @ _d(T).abs(), T.shape[-1]


def bwd(X, T, G):
    """dX[c][p][i] = sum_j G[c][p][j] T[c][i][j] (L = k);  dT[c][i][j] = sum_p X[c][p][i] G[c][p][j] (L = n)"""
    X64, T64, G64 = _d(X), _d(T), _d(G)
    return {"dX": (G64 @ T64.transpose(1, 2), G64.abs() @ T64.abs().transpose(1, 2), T.shape[-1]),
            "dT": (X64.transpose(1, 2) @ G64, X64.abs().transpose(1, 2) @ G64.abs(), X.shape[1])}


def ortho(T, weight):
    """Gm = T T^T - I;  loss_parts[c] = weight / 2 sum Gm^2;  dT[c] = 2 weight Gm T.

    Gm: a k-term sum and the subtraction, magnitude A_G = |T| |T|^T + I, L = k.
    dT: a k-term sum of products of Gm, each carrying Gm's own error (k + 4) u A_G, so its magnitude sum is taken over A_G, not
    over |Gm| -- the cancellation in T T^T - I is what the operation is about, and the bound says so: A = 2 w A_G |T|, L = k
    (C = 2 covers the second k-term chain: (k + 4) u A_G |T| from Gm's error plus (k + 2) u |Gm| |T| <= the same again).
    loss_parts: to first order the error is w sum |Gm| err(Gm) plus the rounding of a k k-term sum of squares; in units of
    (L + 4) u with L = k that is A = w sum |Gm| A_G + (k k + 4) / (k + 4) (w / 2) sum Gm^2."""
    T64 = _d(T)
    k = T.shape[-1]
    eye = torch.eye(k, dtype=D, device=T.device)
    Gm = T64 @ T64.transpose(1, 2) - eye
    AG = T64.abs() @ T64.abs().transpose(1, 2) + eye
    half = 0.5 * weight * (Gm * Gm).sum(dim=(1, 2))
    loss = (half, weight * (Gm.abs() * AG).sum(dim=(1, 2)) + (k * k + 4.0) / (k + 4.0) * half, k)
    return {"Gm": (Gm, AG, k), "loss_parts": loss, "dT": (2 * weight * (Gm @ T64), 2 * weight * (AG @ T64.abs()), k)}


# ------------------------------------------------------------------------------------------------------------ plain loops
def fwd_loops(X, T):
    b, n, k = X.shape
    out = torch.zeros(b, n, k, dtype=D)
    for c in range(b):
        for p in range(n):
            for i in range(k):
                out[c, p] += float(X[c, p, i]) * _d(T[c, i])
    return out


def bwd_loops(X, T, G):
    b, n, k = X.shape
    dX, dT = torch.zeros(b, n, k, dtype=D), torch.zeros(b, k, k, dtype=D)
    for c in range(b):
        for p in range(n):
            for i in range(k):
                dX[c, p, i] = (_d(G[c, p]) * _d(T[c, i])).sum()
                dT[c, i] += float(X[c, p, i]) * _d(G[c, p])
    return dX, dT


def ortho_loops(T, weight):
    b, k, _ = T.shape
    loss, dT = torch.zeros(b, dtype=D), torch.zeros(b, k, k, dtype=D)
    for c in range(b):
        Gm = torch.zeros(k, k, dtype=D)
        for i in range(k):
            for i2 in range(k):
                Gm[i, i2] = (_d(T[c, i]) * _d(T[c, i2])).sum() - (1.0 if i == i2 else 0.0)
        for i in range(k):
            for i2 in range(k):
                loss[c] += 0.5 * weight * Gm[i, i2] ** 2
                dT[c, i] += 2 * weight * Gm[i, i2] * _d(T[c, i2])
    return loss, dT


# ------------------------------------------------------------------------------------------------------- pointnet_cls_basic
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


def _layer(P, scope, x, training):
    w = P[scope + '/weights']
    y = x @ w.reshape(-1, w.shape[-1]) + P[scope + '/biases']
    return torch.relu(_bn(P, scope, y, training))


def pointnet_cls_basic(points, P, training=False):
    """points (B, N, 3) float64 -> logits: conv1 ([1, 3] over the coordinates) .. conv5, max over the points, fc1, fc2, fc3;
    dropout is the identity (eval, or switched off by the caller)"""
    net = points
    for i in range(1, 6):
        net = _layer(P, 'conv%d' % i, net, training)
    net = net.amax(dim=1)
    net = _layer(P, 'fc2', _layer(P, 'fc1', net, training), training)
    return net @ P['fc3/weights'] + P['fc3/biases']
