"""The float64 restatement of the *_groups entry points (pool_top_groups_ref.py) against torch autograd of the layer itself,
and the planner's choice of the form."""
import torch

import pool_top_groups_ref as PR
from scanobjectnn_amd import fused_mlp

EPS = 1e-3


def _rel(got, want):
    return (got - want).abs().max().item() / want.abs().max().item()


def test_restatement_equals_autograd_of_the_layer():
    """train-mode BN of the layer below and of this layer, max over groups of 32 rows (first maximiser), 12 groups:
    the combined expressions of pcops.h with prep / finish restated give autograd's dX (under the ReLU mask of the layer
    below), dW and db to 1e-10 relative"""
    G, S, K, N = 12, 32, 64, 128
    M = G * S
    g = torch.Generator().manual_seed(1)
    f64 = dict(dtype=torch.float64, generator=g)
    Yprev = torch.randn(M, K, **f64)
    gam0, bet0 = 0.5 + torch.rand(K, **f64), 0.3 * torch.randn(K, **f64)
    gam0[::5] *= -1.0
    W = (torch.randn(K, N, **f64) / K ** 0.5).requires_grad_(True)
    b = (0.1 * torch.randn(N, **f64)).requires_grad_(True)
    gam, bet = 0.5 + torch.rand(N, **f64), 0.2 * torch.randn(N, **f64)
    gam[::3] *= -1.0
    go = torch.randn(G, N, **f64)

    # ---- the layer under autograd
    m0, v0 = Yprev.mean(0), Yprev.var(0, unbiased=False)
    psc = gam0 / torch.sqrt(v0 + EPS)
    psh = bet0 - m0 * psc
    z = (Yprev * psc + psh).requires_grad_(True)       # bn of the layer below: Gprev is the gradient at z
    X = torch.relu(z)
    Y = X @ W + b
    mean, var = Y.mean(0), Y.var(0, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + EPS)
    A = (Y - mean) * rstd * gam + bet
    pre, arg = A.view(G, S, N).max(1)                  # relu is monotone: the max of relu(A) sits where the max of A does
    out = torch.relu(pre)
    for gi in range(G):                                 # first maximiser
        assert torch.equal(arg[gi], (A.view(G, S, N)[gi] == pre[gi]).int().argmax(0))
    (out * go).sum().backward()

    # ---- dY = p.G + q.Y + t of the train-mode BN, from the pooled gradient alone
    sc = (gam * rstd).detach()
    sh = (bet - mean * sc).detach()
    ysel = torch.gather(Y.detach().view(G, S, N), 1, arg.view(G, 1, N)).view(G, N)
    gm = go * (ysel * sc + sh > 0)
    yhat = (ysel - mean.detach()) * rstd.detach()
    dgamma, dbeta = (gm * yhat).sum(0), gm.sum(0)
    p = sc
    q = -gam * rstd.detach() ** 2 * dgamma / M
    t = -sc * dbeta / M - q * mean.detach()

    Wd, bd = W.detach(), b.detach()
    Wt, Wq, u, v, Mq = PR.prep(Wd, bd, q, t)
    arg8 = arg.to(torch.uint8)
    Gprev, _ = PR.dgrad_top_groups(S, Yprev, psc, psh, Mq, v, go, ysel, arg8, sc, sh, p, Wt)
    gram, xsum, Ssp, cfsum = PR.wgrad_top_groups(S, Yprev, psc, psh, go, ysel, arg8, sc, sh, p)
    dW, db = PR.finish(M, Wd, bd, q, t, Wq, u, gram, xsum, Ssp, cfsum)
    for name, got, want in (("dX", Gprev, z.grad), ("dW", dW, W.grad)):
        r = _rel(got, want)
        print("%s relative error %.3e" % (name, r))
        assert r <= 1e-10, (name, r)
    # db: behind a train-mode BN the true value is zero (the terms cancel), so the error is taken relative to the terms
    r = (db - b.grad).abs().max().item() / cfsum.abs().max().item()
    print("db error relative to its terms %.3e (autograd's largest |db| %.3e)" % (r, b.grad.abs().max().item()))
    assert r <= 1e-10, r


def _sa1_plan(R):
    B, M, S = R // (512 * 32), 512, 32
    return fused_mlp.plan_stack(R=R, S=S, K0=None, widths=[64, 64, 128], pool=1, training=True, need_grad=True, need_dx=False,
                                sync=False, w_aligned=[False, True, True], has_b=[False, True, True], geom=(B, 2048, M),
                                present=["xyz", "wxyz", "bias"])


def test_planner_takes_the_groups_form_from_the_row_floor(monkeypatch):
    monkeypatch.setattr(fused_mlp, "POOL_TOP_GROUPS", True)
    top = _sa1_plan(262144).layers[-1]
    assert top.bwd == fused_mlp.B_TOP and not top.store_y and top.groups and top.fwd == fused_mlp.F_POOL
    small = _sa1_plan(65536).layers[-1]
    assert small.bwd in fused_mlp._ONEPASS and small.store_y and not small.groups
    monkeypatch.setattr(fused_mlp, "POOL_TOP_GROUPS", False)
    off = _sa1_plan(262144).layers[-1]
    assert off == small._replace(count=off.count) and off.bwd in fused_mlp._ONEPASS
