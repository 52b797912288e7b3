"""Float64 definitions of the EdgeConv family (include/pcops.h: pcops_edge_pool_*, the [Q | Ctr] forms, pcops_edge_first_*,
pcops_edge_weights_*), written from the header and from nothing in the product.  Plain torch on whatever device the inputs
live on.  Every sum comes back as a triple (ref, A, L): the float64 value, the MAGNITUDE SUM of the terms that are added
into the element (absolute values of the terms a kernel that follows the header's formulas really adds) and the number of
those terms -- what the per-element bound  |out - ref| <= C (L + 4) 2^-24 A  of tests/edge_checks.py needs.

Layout: Q (b, n, c), Ctr (b, m, c), idx (b, m, s) with values in [0, n); per-group tensors (b, m, c); per-channel vectors
(c).  Inputs are float32 (any strides); they are widened, never re-rounded, unless a definition says "stored": a stored
fp32 tensor (ysel, Y, the edge rows) is the float64 value rounded ONCE, which is exactly what one fp32 operation gives.
"""
import torch

D = torch.float64


def _d(x):
    return x.to(D)


def gather_rows(Q, idx):
    """Q[idx]: (b, m, s, c) float64"""
    b = Q.shape[0]
    return _d(Q)[torch.arange(b, device=Q.device).view(b, 1, 1), idx.long()]


def inverse_sum(vals, idx, n):
    """sum over the rows (g, s) with idx[g, s] == i of vals[b, g, s, :] -> (b, n, c)"""
    b, m, s, c = vals.shape
    flat = (idx.long() + n * torch.arange(b, device=idx.device).view(b, 1, 1)).reshape(-1)
    out = torch.zeros(b * n, c, dtype=vals.dtype, device=vals.device)
    out.index_add_(0, flat, vals.reshape(-1, c))
    return out.view(b, n, c)


def counts(idx, n):
    b = idx.shape[0]
    ones = torch.ones(idx.shape + (1,), dtype=D, device=idx.device)
    return inverse_sum(ones, idx, n)                                     # (b, n, 1)


# ------------------------------------------------------------------------------------------------------------- pooled layer
def pool_fwd(Q, Ctr, idx, gamma, pivot=None, relative=True):
    """pcops_edge_pool_fwd.  qsel = max over s where gamma >= 0 (-0.0 counts as >= 0: `gamma < 0` is false), min where
    gamma < 0; arg = the FIRST s attaining it; SQ = sum_s Q[idx]; statistics (sum y', sum y'^2) over all (b, m, s) with
    y' = Q[idx] + Ctr - pivot.
    relative: the sums are taken the way the header describes them, q' = q - Q[0,0,:] and c' = Ctr + Q[0,0,:] - pivot (the
    form with statistics); False: SQ summed from the rows themselves (the call without statistics).
    -> dict(qsel, arg, SQ=(ref, A, L), s1=(ref, A, L), s2=(ref, A, L))"""
    b, m, s = idx.shape
    c = Q.shape[-1]
    q = gather_rows(Q, idx)                                              # (b, m, s, c)
    up = ~(gamma < 0)                                                    # (c)
    v = torch.where(up, q, -q)
    ex, arg = v.max(dim=2)
    first = (v == ex.unsqueeze(2)).to(torch.uint8).argmax(dim=2)         # first slot of the extremum (argmax of a 0/1 mask)
    qsel = torch.where(up, ex, -ex)
    qz = _d(Q)[0, 0] if relative else torch.zeros(c, dtype=D, device=Q.device)
    dq = q - qz
    SQ = q.sum(2)
    SQ_A = dq.abs().sum(2) + s * qz.abs()
    pv = _d(pivot) if pivot is not None else torch.zeros(c, dtype=D, device=Q.device)
    y = q + _d(Ctr).unsqueeze(2) - pv
    cv = _d(Ctr) + (qz - pv)                                             # c'
    s1 = y.sum((0, 1, 2))
    s1_A = (s * cv.abs() + dq.abs().sum(2)).sum((0, 1))
    s2 = (y * y).sum((0, 1, 2))
    s2_A = ((dq * dq).sum(2) + 2 * cv.abs() * dq.abs().sum(2) + s * cv * cv).sum((0, 1))
    G = b * m
    return {"qsel": qsel, "arg": first.to(torch.uint8), "SQ": (SQ, SQ_A, s + 1),
            "s1": (s1, s1_A, G * (s + 1)), "s2": (s2, s2_A, G * (s + 2))}


def pool_out(qsel, Ctr, scale, shift):
    """pcops_edge_pool_out*: ysel = qsel + Ctr (stored: one fp32 add), out = relu(scale ysel + shift) on the STORED ysel.
    -> (out float64, unrounded; ysel float32)"""
    ysel = (_d(qsel) + _d(Ctr)).float()
    out = (_d(ysel) * _d(scale) + _d(shift)).clamp_min(0.0)
    return out, ysel


def pool_bwd(Q, Ctr, idx, gpool, ysel, SQ, arg, scale, shift, p, q, t):
    """pcops_edge_pool_bwd:  a = p gpool [scale ysel + shift > 0],  dCtr[g] = q (SQ + k Ctr) + k t + a,
    dQ[i] = cnt_i (q Q[i] + t) + q sum_{(g,s)->i} Ctr[g] + sum_{(g,s)->i, arg[g,c] == s} a[g,c].
    -> dict(dCtr=(ref, A, L), dQ=(ref, A, L (b, n, c)), cnt)"""
    b, m, s = idx.shape
    n = Q.shape[1]
    pd, qd, td = _d(p), _d(q), _d(t)
    on = (_d(ysel) * _d(scale) + _d(shift)) > 0
    a = torch.where(on, pd * _d(gpool), torch.zeros((), dtype=D, device=Q.device))       # (b, m, c)
    C64 = _d(Ctr)
    dCtr = qd * (_d(SQ) + s * C64) + s * td + a
    dCtr_A = qd.abs() * (_d(SQ).abs() + s * C64.abs()) + s * td.abs() + a.abs()
    cnt = counts(idx, n)                                                                 # (b, n, 1)
    sumc = inverse_sum(C64.unsqueeze(2).expand(b, m, s, -1), idx, n)
    sumc_A = inverse_sum(C64.abs().unsqueeze(2).expand(b, m, s, -1), idx, n)
    hit = arg.long().unsqueeze(2) == torch.arange(s, device=Q.device).view(1, 1, s, 1)   # (b, m, s, c)
    suma = inverse_sum(a.unsqueeze(2) * hit.to(D), idx, n)
    suma_A = inverse_sum(a.abs().unsqueeze(2) * hit.to(D), idx, n)
    nhit = inverse_sum((hit & (a != 0).unsqueeze(2)).to(D), idx, n)
    Q64 = _d(Q)
    dQ = qd * (cnt * Q64 + sumc) + cnt * td + suma
    dQ_A = qd.abs() * (cnt * Q64.abs() + sumc_A) + cnt * td.abs() + suma_A
    return {"dCtr": (dCtr, dCtr_A, 4), "dQ": (dQ, dQ_A, cnt + nhit + 2), "cnt": cnt}


# ------------------------------------------------------------------------------------- stored first layer of a gather stack
def tnet_fwd(Q, Ctr, idx, pivot=None):
    """pcops_sa_gather_fwd_ld: Y = Q[idx] + Ctr (stored: one fp32 add), statistics (sum y', sum y'^2), y' = Y - pivot, of
    the STORED rows.  -> dict(Y float32 (b, m, s, c), s1, s2)"""
    b, m, s = idx.shape
    c = Q.shape[-1]
    Y = (gather_rows(Q, idx) + _d(Ctr).unsqueeze(2)).float()
    pv = _d(pivot) if pivot is not None else torch.zeros(c, dtype=D, device=Q.device)
    y = _d(Y) - pv
    R = b * m * s
    return {"Y": Y, "s1": (y.sum((0, 1, 2)), y.abs().sum((0, 1, 2)), R), "s2": ((y * y).sum((0, 1, 2)), (y * y).sum((0, 1, 2)), R)}


def tnet_bwd(G, p, q, t, idx, Q, Ctr):
    """pcops_sa_scatter_bwd_ld:  dY = p G + q Y + t with Y = Q[idx] + Ctr;  dCtr[g] = sum_s dY,  dQ[i] = sum_{(g,s)->i} dY.
    G (b, m, s, c).  -> dict(dCtr=(ref, A, L), dQ=(ref, A, L))"""
    b, m, s = idx.shape
    n = Q.shape[1]
    pd, qd, td = _d(p), _d(q), _d(t)
    qg, C64, G64 = gather_rows(Q, idx), _d(Ctr).unsqueeze(2), _d(G)
    dY = pd * G64 + qd * (qg + C64) + td
    dYa = pd.abs() * G64.abs() + qd.abs() * (qg.abs() + C64.abs()) + td.abs()
    cnt = counts(idx, n)
    return {"dCtr": (dY.sum(2), dYa.sum(2), 2 * s + 3),
            "dQ": (inverse_sum(dY, idx, n), inverse_sum(dYa, idx, n), 2 * cnt + 3)}


# ------------------------------------------------------------------------------------------ first layer without a scatter
def edge_rows(xyz, idx):
    """e = [x_g | x_j - x_g], j = idx[g, s] (m == n): (b, m, s, 6) float32, the three differences one fp32 subtraction each"""
    b, m, s = idx.shape
    xg = _d(xyz).unsqueeze(2).expand(b, m, s, 3)
    xj = gather_rows(xyz, idx)
    return torch.cat([xg, xj - xg], dim=-1).float()


def first_layer(xyz, idx, Gm, W, bias, p, q, t, sumG, mean):
    """pcops_edge_first_moments / _wgrad / _layer_grads.  Gm (b m s, c) the masked gradient, W (6, c), bias (c) or None.
      moments (27): the 21 products e_i e_j (i <= j, row-major upper triangle) then the 6 sums, over all rows
      EtG (6, c) = E^T Gm
      dW (6, c) = p EtG + q (M W + S b) + t S,   dbias (c) = p sumG + q mean rows + t rows
    -> dict(rows (b m s, 6) float32, moments=(ref, A, L), EtG=(ref, A, L), dW=(ref, A), dbias=(ref, A))"""
    e32 = edge_rows(xyz, idx).reshape(-1, 6)
    e = _d(e32)
    R = e.shape[0]
    iu = torch.triu_indices(6, 6, device=e.device)
    prod = e[:, iu[0]] * e[:, iu[1]]                                     # (R, 21)
    mom = torch.cat([prod.sum(0), e.sum(0)])
    mom_A = torch.cat([prod.abs().sum(0), e.abs().sum(0)])
    G64 = _d(Gm)
    EtG = e.t() @ G64
    EtG_A = e.abs().t() @ G64.abs()
    M = torch.zeros(6, 6, dtype=D, device=e.device)
    M[iu[0], iu[1]] = prod.sum(0)
    M = M + M.t() - torch.diag(torch.diag(M))
    Ma = torch.zeros(6, 6, dtype=D, device=e.device)
    Ma[iu[0], iu[1]] = prod.abs().sum(0)
    Ma = Ma + Ma.t() - torch.diag(torch.diag(Ma))
    S, Sa = e.sum(0), e.abs().sum(0)
    pd, qd, td, W64 = _d(p), _d(q), _d(t), _d(W)
    bz = _d(bias) if bias is not None else torch.zeros_like(pd)
    dW = pd * EtG + qd * (M @ W64 + S.unsqueeze(1) * bz) + td * S.unsqueeze(1)
    dW_A = pd.abs() * EtG_A + qd.abs() * (Ma @ W64.abs() + Sa.unsqueeze(1) * bz.abs()) + td.abs() * Sa.unsqueeze(1)
    db = pd * _d(sumG) + qd * (_d(mean) * R) + td * R
    db_A = pd.abs() * _d(sumG).abs() + qd.abs() * _d(mean).abs() * R + td.abs() * R
    return {"rows": e32, "moments": (mom, mom_A, R), "EtG": (EtG, EtG_A, R), "dW": (dW, dW_A), "dbias": (db, db_A)}


def first_layer_from_partials(wpart, mpart, W, bias, p, q, t, sumG, mean, rows):
    """pcops_edge_first_layer_grads alone: the same dW / dbias from GIVEN fp32 partial rows wpart (P1, 6, c), mpart (P2, 27).
    -> (dW, dW_A, dbias, dbias_A), the magnitudes from the absolute values of the partials"""
    iu = torch.triu_indices(6, 6, device=wpart.device)

    def sym(v):
        M = torch.zeros(6, 6, dtype=D, device=v.device)
        M[iu[0], iu[1]] = v
        return M + M.t() - torch.diag(torch.diag(M))

    A, Aa = _d(wpart).sum(0), _d(wpart).abs().sum(0)
    mom, moma = _d(mpart).sum(0), _d(mpart).abs().sum(0)
    M, Ma, S, Sa = sym(mom[:21]), sym(moma[:21]), mom[21:], moma[21:]
    pd, qd, td = _d(p), _d(q), _d(t)
    bz = _d(bias) if bias is not None else torch.zeros_like(pd)
    dW = pd * A + qd * (M @ _d(W) + S.unsqueeze(1) * bz) + td * S.unsqueeze(1)
    dW_A = pd.abs() * Aa + qd.abs() * (Ma @ _d(W).abs() + Sa.unsqueeze(1) * bz.abs()) + td.abs() * Sa.unsqueeze(1)
    db = pd * _d(sumG) + qd * (_d(mean) * rows) + td * rows
    db_A = pd.abs() * _d(sumG).abs() + qd.abs() * _d(mean).abs() * rows + td.abs() * rows
    return dW, dW_A, db, db_A


# ----------------------------------------------------------------------------------------------- the concatenated weight
def edge_weights_fwd(W1, b1, kp):
    """W1 (2 c, cp) = [W_a ; W_b] -> Wcat (kp, 2 cp) = [W_b | W_a - W_b], rows c.. zero; bcat (2 cp) = [0 | b1]  (float32:
    copies and one fp32 subtraction)"""
    c, cp = W1.shape[0] // 2, W1.shape[1]
    Wa, Wb = _d(W1[:c]), _d(W1[c:])
    Wcat = torch.zeros(kp, 2 * cp, dtype=torch.float32, device=W1.device)
    Wcat[:c, :cp] = W1[c:]
    Wcat[:c, cp:] = (Wa - Wb).float()
    bcat = torch.zeros(2 * cp, dtype=torch.float32, device=W1.device)
    if b1 is not None:
        bcat[cp:] = b1
    return Wcat, bcat


def edge_weights_bwd(dWcat, dbcat, c):
    """dW_a = dWcat[:c, cp:], dW_b = dWcat[:c, :cp] - dWcat[:c, cp:], db1 = dbcat[cp:]  (float32)"""
    cp = dWcat.shape[1] // 2
    dWa = dWcat[:c, cp:]
    dWb = (_d(dWcat[:c, :cp]) - _d(dWcat[:c, cp:])).float()
    return torch.cat([dWa, dWb], dim=0), dbcat[cp:].clone()


# ------------------------------------------------------------------------------------------------- BN backward coefficients
def bn_bwd_coeffs(y, g, gamma, eps=1e-3):
    """training-mode BN over the rows of y (R, c) followed by anything whose gradient at the BN OUTPUT is g (R, c):
    dY = p g + q y + t with  p = gamma r,  q = -p mean(g xhat) r,  t = -p mean(g) - q mu   (r = rsqrt(var + eps))"""
    mu = y.mean(0)
    var = y.var(0, unbiased=False)
    r = torch.rsqrt(var + eps)
    xhat = (y - mu) * r
    pcoef = gamma * r
    qcoef = -pcoef * (g * xhat).mean(0) * r
    tcoef = -pcoef * g.mean(0) - qcoef * mu
    return pcoef, qcoef, tcoef
