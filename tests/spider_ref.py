"""Float64 definitions of the SpiderConv family (include/pcops.h "SpiderConv" and the comment block at the top of
csrc/spider.hip), written from those two and from nothing in spidercnn/spider_ops.py.  Plain torch on whatever device the
inputs live on.  Every sum comes back as a triple (ref, A, L) as in tests/edge_ref.py: the float64 value, the MAGNITUDE SUM
of the terms a kernel that follows the header really adds into the element, and the number of those terms -- what the
per-element bound  |out - ref| <= C (L + 4) 2^-24 A  of tests/edge_checks.py needs.

Layout: feat (b, n, c), idx (b, n, k) int32 with values in [0, n) PER CLOUD, g / dg (b, n, k, T), w (k c T, o) whose row is
(j c_ + c) T + t, y / dy (b, n, o), delta (rows, 3), theta (19, T).  Inputs are float32; they are widened, never
re-rounded.  Each entry point is defined on the fp32 tensors THAT entry point is given (the stored g, y, mean, rstd, dy),
so every kernel is judged alone and errors do not compound down the layer.
"""
import torch

from edge_checks import C_BOUND, U

D = torch.float64
T = 5
MONO = 19


def _d(x):
    return x.to(D)


def monomials(delta):
    """phi_m(delta), m in the header's order x y z xyz xy yz xz xx yy zz xxy xyy xxz xzz yyz yzz xxx yyy zzz: (..., 19)"""
    d = _d(delta)
    X, Y, Z = d[..., 0], d[..., 1], d[..., 2]
    return torch.stack([X, Y, Z, X * Y * Z, X * Y, Y * Z, X * Z, X * X, Y * Y, Z * Z, X * X * Y, X * Y * Y, X * X * Z,
                        X * Z * Z, Y * Y * Z, Y * Z * Z, X * X * X, Y * Y * Y, Z * Z * Z], -1)


# --------------------------------------------------------------------------------------------------------------- Taylor
def taylor_fwd(delta, theta, tbias):
    """g[r,t] = tbias[t] + sum_m theta[m,t] phi_m(delta[r]): 19 products and the bias, L = 20.  delta (rows, 3)."""
    terms = monomials(delta).unsqueeze(-1) * _d(theta)                   # (rows, 19, T)
    return terms.sum(-2) + _d(tbias), terms.abs().sum(-2) + _d(tbias).abs(), MONO + 1


def taylor_bwd(delta, dg):
    """dtheta[m,t] = sum_r phi_m(delta[r]) dg[r,t], dtbias[t] = sum_r dg[r,t]; L = rows.
    -> dict(dtheta=(ref, A, L), dtbias=(ref, A, L))"""
    phi, g64 = monomials(delta.reshape(-1, 3)), _d(dg).reshape(-1, T)
    rows = phi.shape[0]
    return {"dtheta": (phi.t() @ g64, phi.abs().t() @ g64.abs(), rows),
            "dtbias": (g64.sum(0), g64.abs().sum(0), rows)}


# ---------------------------------------------------------------------------------------------------------- contraction
def gather_feat(feat, idx):
    """F[idx[p,j]] with idx taken inside the cloud of p: (b, n, k, c) float64"""
    b = feat.shape[0]
    return _d(feat)[torch.arange(b, device=feat.device).view(b, 1, 1), idx.long()]


def expanded(feat, idx, g):
    """the expanded operand A[p,(j,c,t)] = F[idx[p,j],c] g[p,j,t]: (b n, k c T) float64, columns in the weight's row order"""
    b, n, k = idx.shape
    return (gather_feat(feat, idx).unsqueeze(-1) * _d(g).unsqueeze(3)).reshape(b * n, -1)


def conv_fwd(feat, idx, g, w, bias=None):
    """y[p,o] = bias[o] + sum_{j,c,t} F[idx[p,j],c] g[p,j,t] W[(j C + c) T + t, o]; L = k C T + 1.  -> (ref, A, L), (b, n, o)"""
    b, n, k = idx.shape
    Aop, W64 = expanded(feat, idx, g), _d(w)
    o = W64.shape[1]
    bz = _d(bias) if bias is not None else torch.zeros(o, dtype=D, device=w.device)
    ref = Aop @ W64 + bz
    mag = Aop.abs() @ W64.abs() + bz.abs()
    return ref.view(b, n, o), mag.view(b, n, o), Aop.shape[1] + 1


def conv_wgrad(feat, idx, g, dy):
    """dW[(j C + c) T + t, o] = sum_p F[idx[p,j],c] g[p,j,t] dY[p,o] over all b n rows, db[o] = sum_p dY[p,o]; L = b n.
    -> dict(dw=(ref, A, L), db=(ref, A, L))"""
    Aop = expanded(feat, idx, g)
    P = Aop.shape[0]
    dy64 = _d(dy).reshape(P, -1)
    return {"dw": (Aop.t() @ dy64, Aop.abs().t() @ dy64.abs(), P),
            "db": (dy64.sum(0), dy64.abs().sum(0), P)}


def conv_dgrad(feat, idx, g, w, dy):
    """dA[p,(j,c,t)] = sum_o dY[p,o] W[(j C + c) T + t, o], then
      dfg[p,j,c] = sum_t dA g[p,j,t]          A = sum_t |g| sum_o |dY W|,   L = O + T
      dg[p,j,t]  = sum_c dA F[idx[p,j],c]     A = sum_c |F| sum_o |dY W|,   L = O + C
    -> dict(dfg=(ref, A, L) (b, n, k, c), dg=(ref, A, L) (b, n, k, T))"""
    b, n, k = idx.shape
    c, o = feat.shape[2], w.shape[1]
    dy64, W64 = _d(dy).reshape(b * n, o), _d(w)
    dA = (dy64 @ W64.t()).view(b, n, k, c, T)
    dAa = (dy64.abs() @ W64.abs().t()).view(b, n, k, c, T)
    g64, Fg = _d(g).unsqueeze(3), gather_feat(feat, idx).unsqueeze(-1)
    return {"dfg": ((dA * g64).sum(-1), (dAa * g64.abs()).sum(-1), o + T),
            "dg": ((dA * Fg).sum(3), (dAa * Fg.abs()).sum(3), o + c)}


def scatter_grouped(dfg, idx, n):
    """dF[i] = sum over the (p, j) of the same cloud with idx[p,j] == i of dfg[p,j,:]; L = count_i.  -> (ref, A, L (b, n, 1))"""
    b, m, k, c = dfg.shape
    flat = (idx.long() + n * torch.arange(b, device=idx.device).view(b, 1, 1)).reshape(-1)

    def inv(v):
        out = torch.zeros(b * n, v.shape[-1], dtype=D, device=dfg.device)
        return out.index_add_(0, flat, v.reshape(b * m * k, -1)).view(b, n, -1)

    v = _d(dfg)
    return inv(v), inv(v.abs()), inv(torch.ones(b, m, k, 1, dtype=D, device=dfg.device))


# ------------------------------------------------------------------------------------------------------ group norm + ReLU
def _grouped(x, groups):
    b, n, c = x.shape
    return _d(x).view(b, n, groups, c // groups)


def group_norm_relu_fwd(x, gamma, beta, groups, eps, mean, rstd, out):
    """Group norm over the n points and c / groups contiguous channels of each (cloud, group), two-pass biased variance.
    mean, rstd, out: what the kernel STORED (fp32); each later quantity is defined on the stored value of the one before
    it, so a kernel whose sums are right is inside every bound whatever its order of summation:
      mean  = sum x / (n cg)                                 A = sum |x| / (n cg),   L = n cg
      var   = sum (x - mean_stored)^2 / (n cg)               A = var (no term is negative), L = n cg
      rstd  = 1 / sqrt(var + eps): no sum.  d rstd = -1/2 rstd d var / (var + eps), and the add, the root and the
              division round once each:  |rstd_stored - rstd| <= rstd (1/2 bound(var) / (var + eps) + 3 u)  ("rstd_lim")
      z     = gamma (x - mean_stored) rstd_stored + beta     A = |gamma (x - mean) rstd| + |beta|, L = 3 (the
              subtraction, the product with rstd, one fused multiply-add)
      out   = z mask, mask = [out_stored > 0]: the ReLU decision read back from the kernel (tests/decisions.py, DESIGN.md
              section 2).  Every element with (z > 0) != mask is reported in "flips"; such an element must have
              |z| <= the bound of z there ("flips_ok": a condition on each of them, not a count allowance).
    -> dict(mean, var, rstd, rstd_lim, z, out, mask, flips, flips_ok)"""
    b, n, c = x.shape
    cg = c // groups
    L = n * cg
    xg = _grouped(x, groups)
    m64 = xg.mean((1, 3))
    mA = xg.abs().mean((1, 3))
    ms = _d(mean).view(b, 1, groups, 1)
    var = ((xg - ms) ** 2).mean((1, 3))
    r64 = 1.0 / torch.sqrt(var + eps)
    rstd_lim = r64 * (0.5 * C_BOUND * (L + 4) * U * var / (var + eps) + 3 * U)
    rs = _d(rstd).view(b, 1, groups, 1)
    gm, bt = _d(gamma).view(1, 1, groups, cg), _d(beta).view(1, 1, groups, cg)
    lin = gm * (xg - ms) * rs
    z = (lin + bt).reshape(b, n, c)
    zA = (lin.abs() + bt.abs()).reshape(b, n, c)
    mask = out > 0
    flips = (z > 0) != mask
    zlim = C_BOUND * (3 + 4) * U * zA
    return {"mean": (m64, mA, L), "var": (var, var, L), "rstd": r64, "rstd_lim": rstd_lim, "z": (z, zA, 3),
            "out": (z * mask.to(D), zA, 3), "mask": mask, "flips": flips,
            "flips_ok": bool((z.abs()[flips] <= zlim[flips]).all())}


L_DX = 6


def group_norm_relu_bwd(dout, x, y, gamma, mean, rstd, groups):
    """On the GIVEN fp32 mean, rstd and y:  gy = dout [y > 0] (exact), xhat = (x - mean) rstd,
      dgamma[ch] = sum_{cloud, p} gy xhat       A = sum |gy xhat|,  L = b n
      dbeta[ch]  = sum_{cloud, p} gy            A = sum |gy|,       L = b n
      m1 = sum_group gamma gy / (n cg)          A1 = sum |gamma gy| / (n cg),        Lg = n cg
      m2 = sum_group gamma gy xhat / (n cg)     A2 = sum |gamma gy xhat| / (n cg),   Lg = n cg
      dx = rstd (gamma gy - m1 - xhat m2)
    First-order bound of dx.  The kernel forms dx from its own fp32 m1', m2' with |m1' - m1| <= C (Lg + 4) u A1 and
    |m2' - m2| <= C (Lg + 4) u A2 (their triples), and from there with L_DX = 6 roundings of its own: two in xhat, one in
    the fused gamma gy - m1', one in xhat m2', one in the subtraction, one in the product with rstd.  So
      |dx' - dx| <= rstd (|m1' - m1| + |xhat| |m2' - m2|) + L_DX u rstd (|gamma gy| + |m1| + |xhat m2|)
                 <= C u rstd [(Lg + 4) (A1 + |xhat| A2) + (L_DX + 4) (|gamma gy| + |m1| + |xhat m2|)]
                  = C (L_DX + 4) u A     with   A = rstd [|gamma gy| + |m1| + |xhat m2| + (Lg + 4) / (L_DX + 4) (A1 + |xhat| A2)],
    which is the triple (dx, A, L_DX): the long sums weigh only on the two means, not on the element's own term.
    -> dict(dgamma, dbeta, m1, m2, dx) of triples, gy (b, n, c) float64"""
    b, n, c = x.shape
    cg = c // groups
    Lg = n * cg
    ms, rs = _d(mean).view(b, 1, groups, 1), _d(rstd).view(b, 1, groups, 1)
    gy = torch.where(y > 0, _d(dout), torch.zeros((), dtype=D, device=x.device))
    xhat = (_grouped(x, groups) - ms) * rs
    gyg = gy.view(b, n, groups, cg)
    gm = _d(gamma).view(1, 1, groups, cg)
    t1, t2 = gm * gyg, gm * gyg * xhat
    m1, A1 = t1.mean((1, 3), keepdim=True), t1.abs().mean((1, 3), keepdim=True)
    m2, A2 = t2.mean((1, 3), keepdim=True), t2.abs().mean((1, 3), keepdim=True)
    dx = rs * (t1 - m1 - xhat * m2)
    dxA = rs.abs() * (t1.abs() + m1.abs() + (xhat * m2).abs() + (Lg + 4.0) / (L_DX + 4.0) * (A1 + xhat.abs() * A2))
    gx = gyg * xhat
    return {"dgamma": (gx.sum((0, 1)).reshape(c), gx.abs().sum((0, 1)).reshape(c), b * n),
            "dbeta": (gy.sum((0, 1)), gy.abs().sum((0, 1)), b * n),
            "m1": (m1.view(b, groups), A1.view(b, groups), Lg), "m2": (m2.view(b, groups), A2.view(b, groups), Lg),
            "dx": (dx.reshape(b, n, c), dxA.reshape(b, n, c), L_DX), "gy": gy}
