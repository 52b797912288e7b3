"""The float64 definitions of tests/edge_ref.py checked WITHOUT any kernel (no GPU marker): against naive Python loops,
against torch float64 autograd of the literal ops (gather -> training-mode BN -> ReLU -> max over s; the stored form
without the max; e W + b -> BN for the first layer), and the per-element bound of tests/edge_checks.py against an fp32
evaluation of the same sums in another order -- the bounds must hold for a correct fp32 implementation on every input
kind the GPU file uses, the 1e3-offset statistics included, before any kernel is held to them."""
import numpy as np
import pytest
import torch

import edge_checks as K
import edge_ref as R

D = torch.float64
B, N, S, C = 2, 9, 4, 4
EPS = 1e-3


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _tiny(kind, seed=0):
    g = _gen(seed)
    idx = K.make_graph(kind, B, N, N, S, g)
    QC = K.make_features(kind, B, N, N, C, g)
    Q, Ctr = QC[..., :C].contiguous(), QC[..., C:].contiguous()
    gamma = K.make_gamma(C, g)
    return g, idx, Q, Ctr, gamma


@pytest.mark.parametrize("kind", K.KINDS)
def test_graphs_are_what_they_say(kind):
    g = _gen(1)
    idx = K.make_graph(kind, B, 12, 12, 5, g)
    assert idx.dtype == torch.int32 and idx.shape == (B, 12, 5) and idx.min() >= 0 and idx.max() < 12
    cnt = R.counts(idx, 12).squeeze(-1)
    if kind == "hub":
        assert (cnt[:, 0] >= 12).all() and (cnt == 0).any()
    if kind == "dup":
        assert all(len(set(row.tolist())) < 5 for row in idx.view(-1, 5))
    if kind == "self":
        assert (idx == torch.arange(12).view(1, 12, 1)).all()


@pytest.mark.parametrize("kind", K.KINDS)
def test_pool_fwd_against_loops(kind):
    g, idx, Q, Ctr, gamma = _tiny(kind)
    pivot = 0.1 * torch.randn(C, generator=g)
    got = R.pool_fwd(Q, Ctr, idx, gamma, pivot)
    q, ct, pv = Q.double().numpy(), Ctr.double().numpy(), pivot.double().numpy()
    s1, s2 = np.zeros(C), np.zeros(C)
    for b in range(B):
        for m in range(N):
            for c in range(C):
                vals = [q[b, idx[b, m, s], c] for s in range(S)]
                up = not (gamma[c].item() < 0)                       # -0.0 is not < 0
                best, arg = vals[0], 0
                for s in range(1, S):
                    if (vals[s] > best) if up else (vals[s] < best):
                        best, arg = vals[s], s
                assert got["qsel"][b, m, c].item() == best and got["arg"][b, m, c].item() == arg
                assert abs(got["SQ"][0][b, m, c].item() - sum(vals)) < 1e-12
                for v in vals:
                    y = v + ct[b, m, c] - pv[c]
                    s1[c] += y
                    s2[c] += y * y
    assert np.allclose(got["s1"][0].numpy(), s1, rtol=1e-12, atol=1e-12)
    assert np.allclose(got["s2"][0].numpy(), s2, rtol=1e-12, atol=1e-12)
    if kind == "dup":                                                # ties happen, and the first slot is what decides them
        qg = R.gather_rows(Q, idx)
        v = torch.where(~(gamma < 0), qg, -qg)
        assert ((v == v.max(2, keepdim=True).values).sum(2) > 1).any()


def test_negative_zero_gamma_takes_the_maximum():
    g, idx, Q, Ctr, gamma = _tiny("knn")
    assert (gamma == 0).sum() == 2 and torch.signbit(gamma).any()
    got = R.pool_fwd(Q, Ctr, idx, gamma)
    qg = R.gather_rows(Q, idx)
    for c in torch.nonzero(gamma == 0).flatten().tolist():
        assert torch.equal(got["qsel"][..., c], qg[..., c].max(2).values)


def _literal_pool(Q, Ctr, idx, gamma, beta):
    y = R.gather_rows(Q, idx) + Ctr.unsqueeze(2)                         # (b, m, s, c)
    flat = y.reshape(-1, C)
    mu, var = flat.mean(0), flat.var(0, unbiased=False)
    z = (y - mu) * torch.rsqrt(var + EPS) * gamma + beta
    a = torch.relu(z)
    return a.max(dim=2).values, y, mu, var


@pytest.mark.parametrize("kind", K.KINDS)
def test_pool_bwd_against_autograd(kind):
    g, idx, Q32, Ctr32, gamma32 = _tiny(kind, seed=3)
    if kind == "dup":                                                    # autograd's max splits nothing but picks ANY tied slot:
        Q32 = Q32 + 1e-3 * torch.randn(Q32.shape, generator=g)           # keep the repeated neighbours, drop value ties
    Q, Ctr = Q32.double().requires_grad_(), Ctr32.double().requires_grad_()
    gamma, beta = gamma32.double(), 0.3 * torch.randn(C, generator=g).double()
    gamma = torch.where(gamma == 0, torch.full_like(gamma, 0.25), gamma)
    out, y, mu, var = _literal_pool(Q, Ctr, idx, gamma, beta)
    gpool = torch.randn(out.shape, generator=g).double()
    out.backward(gpool)
    # the same through the library's formulas: forward products, then (p, q, t) from the BN backward of the masked gradient
    f = R.pool_fwd(Q32, Ctr32, idx, gamma)
    r = torch.rsqrt(var.detach() + EPS)
    scale, shift = gamma * r, beta - gamma * r * mu.detach()
    ysel = f["qsel"] + Ctr32.double()                                    # float64 here: the algebra, not the storage
    on = (ysel * scale + shift) > 0
    gm = torch.where(on, gpool, torch.zeros((), dtype=D))                # gradient at the BN output, at the arg rows only
    rows = B * N * S
    xhat_sel = (ysel - mu.detach()) * r
    p = gamma * r
    q = -p * ((gm * xhat_sel).sum((0, 1)) / rows) * r
    t = -p * (gm.sum((0, 1)) / rows) - q * mu.detach()
    got = R.pool_bwd(Q32.double(), Ctr32.double(), idx, gpool, ysel, f["SQ"][0], f["arg"], scale, shift, p, q, t)
    assert torch.allclose(got["dCtr"][0], Ctr.grad, rtol=1e-9, atol=1e-11)
    assert torch.allclose(got["dQ"][0], Q.grad, rtol=1e-9, atol=1e-11)
    # and bn_bwd_coeffs is that derivation for a dense gradient
    gd = torch.zeros(B, N, S, C, dtype=D).scatter_(2, f["arg"].long().unsqueeze(2), gm.unsqueeze(2))
    p2, q2, t2 = R.bn_bwd_coeffs(y.detach().reshape(-1, C), gd.reshape(-1, C), gamma, EPS)
    assert torch.allclose(p2, p) and torch.allclose(q2, q, atol=1e-14) and torch.allclose(t2, t, atol=1e-14)


@pytest.mark.parametrize("kind", K.KINDS)
def test_tnet_against_loops_and_autograd(kind):
    g, idx, Q32, Ctr32, gamma32 = _tiny(kind, seed=5)
    pivot = 0.1 * torch.randn(C, generator=g)
    f = R.tnet_fwd(Q32, Ctr32, idx, pivot)
    for b in range(B):
        for m in range(N):
            for s in range(S):
                want = (Q32[b, idx[b, m, s]].double() + Ctr32[b, m].double()).float()
                assert torch.equal(f["Y"][b, m, s], want)
    yp = f["Y"].double().reshape(-1, C) - pivot.double()
    assert torch.allclose(f["s1"][0], yp.sum(0)) and torch.allclose(f["s2"][0], (yp * yp).sum(0))
    Q, Ctr = Q32.double().requires_grad_(), Ctr32.double().requires_grad_()
    gamma, beta = gamma32.double() + 0.3, 0.3 * torch.randn(C, generator=g).double()
    y = R.gather_rows(Q, idx) + Ctr.unsqueeze(2)
    flat = y.reshape(-1, C)
    z = (flat - flat.mean(0)) * torch.rsqrt(flat.var(0, unbiased=False) + EPS) * gamma + beta
    G = torch.randn(z.shape, generator=g).double()
    z.backward(G)
    p, q, t = R.bn_bwd_coeffs(flat.detach(), G, gamma, EPS)
    got = R.tnet_bwd(G.view(B, N, S, C), p, q, t, idx, Q32.double(), Ctr32.double())
    assert torch.allclose(got["dCtr"][0], Ctr.grad, rtol=1e-9, atol=1e-11)
    assert torch.allclose(got["dQ"][0], Q.grad, rtol=1e-9, atol=1e-11)
    # naive loops for the scatter
    dY = p * G.view(B, N, S, C) + q * y.detach() + t
    dq = torch.zeros(B, N, C, dtype=D)
    for b in range(B):
        for m in range(N):
            for s in range(S):
                dq[b, idx[b, m, s]] += dY[b, m, s]
    assert torch.allclose(got["dQ"][0], dq, rtol=1e-12, atol=1e-12)


def test_first_layer_against_loops_and_autograd():
    g = _gen(7)
    idx = K.make_graph("knn", B, N, N, S, g)
    xyz = torch.rand(B, N, 3, generator=g)
    W32 = torch.randn(6, C, generator=g)
    b32 = 0.1 * torch.randn(C, generator=g)
    e32 = R.edge_rows(xyz, idx)
    for b in range(B):
        for m in range(N):
            for s in range(S):
                want = torch.cat([xyz[b, m], xyz[b, idx[b, m, s]] - xyz[b, m]])      # fp32 subtraction
                assert torch.equal(e32[b, m, s], want)
    E = e32.double().reshape(-1, 6)
    W, bias = W32.double().requires_grad_(), b32.double().requires_grad_()
    gamma, beta = 0.5 + torch.rand(C, generator=g).double(), torch.zeros(C, dtype=D)
    y = E @ W + bias
    z = (y - y.mean(0)) * torch.rsqrt(y.var(0, unbiased=False) + EPS) * gamma + beta
    Gm = torch.randn(z.shape, generator=g).double()
    z.backward(Gm)
    p, q, t = R.bn_bwd_coeffs(y.detach(), Gm, gamma, EPS)
    got = R.first_layer(xyz, idx, Gm, W32, b32, p, q, t, Gm.sum(0), y.detach().mean(0))
    assert torch.allclose(got["dW"][0], W.grad, rtol=1e-9, atol=1e-11)
    assert torch.allclose(got["dbias"][0], bias.grad, rtol=1e-9, atol=1e-11)
    k = 0
    for i in range(6):
        for j in range(i, 6):
            assert abs(got["moments"][0][k].item() - (E[:, i] * E[:, j]).sum().item()) < 1e-12
            k += 1
    assert torch.allclose(got["moments"][0][21:], E.sum(0))
    assert torch.allclose(got["EtG"][0], E.t() @ Gm)
    # the partial-row form of the last kernel is the same map
    wpart = torch.stack([0.25 * got["EtG"][0].float()] * 4)
    mpart = torch.stack([0.5 * got["moments"][0].float()] * 2)
    dW2, _, db2, _ = R.first_layer_from_partials(wpart, mpart, W32, b32, p, q, t, Gm.sum(0), y.detach().mean(0), E.shape[0])
    assert torch.allclose(dW2, got["dW"][0], rtol=1e-5, atol=1e-5) and torch.allclose(db2, got["dbias"][0])


def test_edge_weights_maps():
    g = _gen(9)
    c, cp, kp = 3, 8, 5
    W1, b1 = torch.randn(2 * c, cp, generator=g), torch.randn(cp, generator=g)
    Wcat, bcat = R.edge_weights_fwd(W1, b1, kp)
    for r in range(kp):
        for j in range(cp):
            assert Wcat[r, j].item() == (W1[c + r, j].item() if r < c else 0.0)
            assert Wcat[r, cp + j].item() == ((W1[r, j] - W1[c + r, j]).item() if r < c else 0.0)
    assert torch.equal(bcat, torch.cat([torch.zeros(cp), b1]))
    assert torch.equal(R.edge_weights_fwd(W1, None, kp)[1], torch.zeros(2 * cp))
    # the backward map is the transpose of the forward one: <Wcat(W1), D> == <W1, dW1(D)>
    Dw, Db = torch.randn(kp, 2 * cp, generator=g), torch.randn(2 * cp, generator=g)
    dW1, db1 = R.edge_weights_bwd(Dw, Db, c)
    assert abs((Wcat.double() * Dw.double()).sum() - (W1.double() * dW1.double()).sum()) < 1e-5
    assert torch.equal(db1, Db[cp:])


def test_pool_out_definition():
    g = _gen(11)
    qsel, Ctr = torch.randn(5, C, generator=g), torch.randn(5, C, generator=g)
    sc, sh = torch.randn(C, generator=g), torch.randn(C, generator=g)
    out, ysel = R.pool_out(qsel, Ctr, sc, sh)
    assert torch.equal(ysel, qsel + Ctr)
    K.check_one_ulp(torch.relu(ysel * sc + sh), out, "pool_out in fp32")
    with pytest.raises(AssertionError):
        K.check_one_ulp(torch.relu(ysel * sc + sh) * (1 + 2.0 ** -21), out, "pool_out, 4 ulp off")


# -------------------------------------------------------------------------------------- the bounds, against fp32 on the CPU
def _sum32(x, dims):
    """an fp32 sum in an order no kernel uses: the terms in reverse, one after the other along the flattened dims"""
    x = x.float()
    keep = [d for d in range(x.dim()) if d not in dims]
    x = x.permute(*keep, *dims).reshape(*[x.shape[d] for d in keep], -1).flip(-1)
    return x.cumsum(-1, dtype=torch.float32)[..., -1]


CASES32 = [(kind, 0.0, True) for kind in K.KINDS] + [("knn", 1e3, True), ("knn", 0.0, False)]


@pytest.mark.parametrize("kind,offset,with_pivot", CASES32)
def test_bounds_hold_for_an_fp32_evaluation(kind, offset, with_pivot):
    b, n, s, c = 2, 96, 7, 8
    g = _gen(13)
    idx = K.make_graph(kind, b, n, n, s, g)
    QC = K.make_features(kind, b, n, n, c, g, offset=offset)
    Q, Ctr = QC[..., :c].contiguous(), QC[..., c:].contiguous()
    gamma = K.make_gamma(c, g)
    pivot = (2 * offset + 0.1 * torch.randn(c, generator=g)) if with_pivot else None
    f = R.pool_fwd(Q, Ctr, idx, gamma, pivot)
    bi = torch.arange(b).view(b, 1, 1)
    qg = Q[bi, idx.long()]                                               # fp32 (b, m, s, c)
    qz = Q[0, 0]
    dq = qg - qz
    sq = _sum32(dq, (2,))
    K.check_sum(torch.addcmul(sq, torch.full_like(sq, float(s)), qz.expand_as(sq)), f["SQ"], "SQ (fp32)")
    cv = Ctr + (qz - (pivot if pivot is not None else torch.zeros(c)))
    K.check_sum(_sum32(float(s) * cv + sq, (0, 1)), f["s1"], "sum y' (fp32)")
    sq2 = _sum32(dq * dq, (2,))
    K.check_sum(_sum32(cv * (float(s) * cv + 2 * sq) + sq2, (0, 1)), f["s2"], "sum y'^2 (fp32)")
    # the naive evaluation  sum (q + Ctr - pivot)^2  of the offset case loses what the shifted form keeps: the bound notices
    if offset:
        y = qg + Ctr.unsqueeze(2)
        with pytest.raises(AssertionError):
            K.check_sum(_sum32(y * y, (0, 1, 2)) - 2 * pivot * _sum32(y, (0, 1, 2)) + b * n * s * pivot * pivot, f["s2"], "naive")
    # backward
    sc, sh, p, q, t = (torch.randn(c, generator=g) for _ in range(5))
    gpool = torch.randn(b, n, c, generator=g)
    _, ysel = R.pool_out(f["qsel"].float(), Ctr, sc, sh)
    SQ32 = f["SQ"][0].float()
    bw = R.pool_bwd(Q, Ctr, idx, gpool, ysel, SQ32, f["arg"], sc, sh, p, q, t)
    a = torch.where(torch.addcmul(sh, ysel, sc) > 0, p * gpool, torch.zeros(()))
    K.check_sum(q * (float(s) * Ctr + SQ32) + (float(s) * t + a), bw["dCtr"], "dCtr (fp32)")
    hit = f["arg"].long().unsqueeze(2) == torch.arange(s).view(1, 1, s, 1)
    terms = (q * Ctr).unsqueeze(2) + a.unsqueeze(2) * hit.float()        # per entry: q Ctr[g] (+ a at the arg row)
    flat = (idx.long() + n * torch.arange(b).view(b, 1, 1)).reshape(-1)
    dq32 = torch.zeros(b * n, c).index_add_(0, flat.flip(0), terms.reshape(-1, c).flip(0)).view(b, n, c)
    cnt = bw["cnt"].float()
    K.check_sum(dq32 + cnt * (q * Q + t), bw["dQ"], "dQ (fp32)")
    # the stored form
    G = torch.randn(b, n, s, c, generator=g)
    tb = R.tnet_bwd(G, p, q, t, idx, Q, Ctr)
    dY = p * G + (q * (qg + Ctr.unsqueeze(2)) + t)
    K.check_sum(_sum32(dY, (2,)), tb["dCtr"], "T-Net dCtr (fp32)")
    K.check_sum(torch.zeros(b * n, c).index_add_(0, flat, dY.reshape(-1, c)).view(b, n, c), tb["dQ"], "T-Net dQ (fp32)")
    if not offset:
        tf = R.tnet_fwd(Q, Ctr, idx, pivot)
        yp = tf["Y"] - (pivot if pivot is not None else torch.zeros(c))
        K.check_sum(_sum32(yp, (0, 1, 2)), tf["s1"], "T-Net sum y' (fp32)")
        K.check_sum(_sum32(yp * yp, (0, 1, 2)), tf["s2"], "T-Net sum y'^2 (fp32)")


def test_first_layer_bounds_hold_in_fp32():
    b, n, s, c = 2, 64, 5, 8
    g = _gen(17)
    idx = K.make_graph("knn", b, n, n, s, g)
    xyz = torch.rand(b, n, 3, generator=g)
    Gm = torch.randn(b * n * s, c, generator=g)
    W, bias = torch.randn(6, c, generator=g), torch.randn(c, generator=g)
    p, q, t, sumG, mean = (torch.randn(c, generator=g) for _ in range(5))
    f = R.first_layer(xyz, idx, Gm, W, bias, p, q, t, sumG, mean)
    e = f["rows"].reshape(-1, 6)
    iu = torch.triu_indices(6, 6)
    mom32 = torch.cat([_sum32(e[:, iu[0]] * e[:, iu[1]], (0,)), _sum32(e, (0,))])
    K.check_sum(mom32, f["moments"], "moments (fp32)")
    K.check_sum(_sum32(e.unsqueeze(2) * Gm.unsqueeze(1), (0,)), f["EtG"], "E^T Gm (fp32)")


def test_check_sum_rejects_one_wrong_element():
    ref = torch.randn(4, 8, dtype=D)
    out = ref.float()
    K.check_sum(out, (ref, ref.abs(), 1), "exact")
    out[2, 3] += 1e-4
    with pytest.raises(AssertionError):
        K.check_sum(out, (ref, ref.abs(), 1), "one element off")
