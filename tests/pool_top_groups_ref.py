"""float64 restatement of pcops_mlp_dgrad_top_groups / pcops_mlp_wgrad_top_groups (pcops.h) from their arguments, and of
the small operands around them (pcops_mlp_pool_top_prep / _finish of csrc/pooltop_sparse.hip, the two K-sized products of
csrc/small_gemm.hip), in plain torch."""
import torch


def _d(t):
    return t.double()


def coefficients(gout, ysel, pool_scale, pool_shift, p):
    """cf [G][N] = p gout where relu(bn(ysel)) > 0, else 0 (pcops_mlp_pool_top_addend's coefficient)"""
    live = _d(ysel) * _d(pool_scale) + _d(pool_shift) > 0
    return torch.where(live, _d(p) * _d(gout), torch.zeros((), dtype=torch.float64, device=gout.device))


def _rows(argmax, S):
    """global row of every (group, channel): g S + argmax[g, c]"""
    G = argmax.shape[0]
    return torch.arange(G, device=argmax.device).view(G, 1) * S + argmax.long()


def dgrad_top_groups(S, Yprev, prev_scale, prev_shift, Mq, vconst, gout, ysel, argmax, pool_scale, pool_shift, p, Wt):
    """-> Gprev [M][Kp], and the two statistics' terms (dX, dX Yprev) whose column sums stats_partial adds up to"""
    z = _d(Yprev) * _d(prev_scale) + _d(prev_shift)
    X = torch.relu(z)
    cf = coefficients(gout, ysel, pool_scale, pool_shift, p)
    G, N = cf.shape
    addend = torch.zeros_like(X)
    addend.index_add_(0, _rows(argmax, S).reshape(-1), cf.reshape(-1, 1) * _d(Wt).repeat(G, 1))
    Gprev = (z > 0) * (X @ _d(Mq) + _d(vconst) + addend)
    return Gprev, (Gprev, Gprev * _d(Yprev))


def wgrad_top_groups(S, Yprev, prev_scale, prev_shift, gout, ysel, argmax, pool_scale, pool_shift, p):
    """-> gram = X^T X, xsum = X^T 1, Ssp [Kp][N] = X^T (p.G), cfsum [N] = 1^T (p.G)"""
    X = torch.relu(_d(Yprev) * _d(prev_scale) + _d(prev_shift))
    cf = coefficients(gout, ysel, pool_scale, pool_shift, p)
    G, N = cf.shape
    rows = _rows(argmax, S)
    Ssp = torch.zeros(X.shape[1], N, dtype=torch.float64, device=X.device)
    for g0 in range(0, G, 256):         # (G, N, Kp) float64 in slices
        r = rows[g0:g0 + 256]
        Ssp += torch.einsum("gc,gck->kc", cf[g0:g0 + 256], X[r.reshape(-1)].view(r.shape[0], N, -1))
    return X.t() @ X, X.sum(0), Ssp, cf.sum(0)


def prep(W, b, q, t):
    """pcops_mlp_pool_top_prep and the K x K product: Wt, Wq = W diag(q), u = q.b + t, v = W u, Mq = Wq W^T"""
    W, b, q, t = _d(W), _d(b), _d(q), _d(t)
    Wq, u = W * q, q * b + t
    return W.t().contiguous(), Wq, u, W @ u, Wq @ W.t()


def finish(M, W, b, q, t, Wq, u, gram, xsum, Ssp, cfsum):
    """pcops_mlp_pool_top_finish behind dW = gram Wq: dW = (gram Wq + Ssp) + xsum u^T, db = cfsum + q.(xsum^T W + M b) + M t"""
    W, b, q, t = _d(W), _d(b), _d(q), _d(t)
    dW = gram @ Wq + Ssp + torch.outer(xsum, u)
    db = cfsum + q * (xsum @ W + M * b) + M * t
    return dW, db
