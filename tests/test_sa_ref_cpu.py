"""The float64 definitions of tests/sa_ref.py checked WITHOUT any kernel (no GPU marker): against naive Python loops at a tiny
shape, against torch float64 autograd of the literal ops (gather + add for the forward; gather -> affine -> ReLU -> max over s
with the arg-max taken as given for the pooled form), the per-element bound against an fp32 evaluation of the same sums in
another order on every input kind tests/test_sa_paths_gpu.py uses -- a correct fp32 implementation must stay inside it before
any kernel is held to it --, the mask-margin condition of the pooled cases, the sensitivity of the bound (a reference with one
row dropped or doubled, a weight off by one, a row sent to the next point or one channel quad swapped must FAIL it at every
shape the GPU file uses), and the host model of pcops_rows_plan against loops."""
import numpy as np
import pytest
import torch

import sa_ref as R

D = torch.float64
ALL = ("Q", "Ctr", "xyz", "bias")
POOLED_SHAPES = ("cs64_tail", "cs32_c32", "cs16_c16", "cs8_c8", "pooled_s256", "fallback_c16", "split_c32", "split_c64",
                 "split_c256")
FWD_SHAPES = [(3, 70, 9, 20, 4), (3, 70, 9, 20, 64), (3, 70, 9, 20, 1024), (3, 70, 9, 48, 64), (2, 70, 3, 1100, 4),
              (2, 16, 4099, 2, 4), (2, 70, 64, 16, 64)]


def _case(name, seed=0):
    return R.scatter_case(name, "cpu", seed=seed)


def _tiny(compact=False):
    if compact:
        return R.make_case(2, 7, 3, 32, 8, "cpu", seed=3, cnt=[[32, 1, 17], [0, 16, 5]])
    return R.make_case(2, 7, 3, 5, 8, "cpu", seed=3, special=True)


# ------------------------------------------------------------------------------------------------------ loops, tiny shape
def test_layout_is_the_ball_query_one():
    cs = _tiny()
    idx, cnt = cs["idx"], cs["cnt"]
    assert (idx[0] == 5).all() and (idx != 6).all()                              # special: one owner, one unnamed point
    for b in range(1, 2):
        for j in range(3):
            assert (idx[b, j, int(cnt[b, j]):] == idx[b, j, 0]).all()            # padded rows repeat the first hit
    assert (cnt[:, 0] == 5).all() and (cnt[:, 1] == 1).all()
    assert idx[1, 0, 4] == idx[1, 0, 1]                                          # an exact duplicate row among the hits
    for k in ("p", "q", "t"):
        assert (cs[k] > 0).any() and (cs[k] < 0).any()


@pytest.mark.parametrize("compact", [False, True])
def test_forward_and_sums_against_loops(compact):
    cs = _tiny(compact)
    b, n, m, S, C = cs["b"], cs["n"], cs["m"], cs["S"], cs["C"]
    tab = R.row_table(cs, compact)
    Y, A, L = R.forward(cs, ALL, tab)
    assert L == 6
    pv = 0.3 * torch.randn(C, generator=torch.Generator().manual_seed(1))
    st = R.stats(Y, tab["wt"], tab["grp"] // 2, 3, 0, pv)
    mo = R.moments(R.offsets(cs, tab), tab["wt"], tab["grp"] // 2, 3, 0)
    xyz, ctr = cs["xyz"].numpy(), cs["new_xyz"].numpy()
    s1, s2, mom = np.zeros((3, C)), np.zeros((3, C)), np.zeros((3, 9))
    r = 0
    for g in range(b * m):
        cl = g // m
        c0 = max(int(cs["cnt"].view(-1)[g]), 1)
        keep = min(-(-c0 // 16), S // 16) * 16 if compact else S
        for s in range(keep):
            i = int(cs["idx"].view(b * m, S)[g, s])
            o = xyz[cl, i] - ctr[cl, g % m]                                      # fp32
            assert o.dtype == np.float32
            wt = (S - keep + 1) if (compact and s == 0) else 1
            assert tab["wt"][r].item() == wt and tab["grp"][r].item() == g and tab["pt"][r].item() == i
            for c in range(C):
                y = float(cs["Q"][cl, i, c]) + float(cs["Ctr"][cl, g % m, c]) + float(cs["bias"][c])
                a = abs(float(cs["Q"][cl, i, c])) + abs(float(cs["Ctr"][cl, g % m, c])) + abs(float(cs["bias"][c]))
                for k in range(3):
                    y += float(o[k]) * float(cs["Wxyz"][k, c])
                    a += abs(float(o[k]) * float(cs["Wxyz"][k, c]))
                assert abs(Y[r, c].item() - y) < 1e-12 and abs(A[r, c].item() - a) < 1e-12
                s1[g // 2, c] += wt * (y - float(pv[c]))
                s2[g // 2, c] += wt * (y - float(pv[c])) ** 2
            x, yy, z = (float(v) for v in o)
            mom[g // 2] += wt * np.array([x * x, x * yy, x * z, yy * yy, yy * z, z * z, x, yy, z])
            r += 1
    assert r == tab["R"]
    assert np.allclose(st[0][:, 0].numpy(), s1, rtol=1e-12, atol=1e-12)
    assert np.allclose(st[0][:, 1].numpy(), s2, rtol=1e-12, atol=1e-12)
    assert np.allclose(mo[0].numpy(), mom, rtol=1e-12, atol=1e-12)
    assert (st[1] >= st[0].abs() - 1e-12).all() and (mo[1] >= mo[0].abs() - 1e-12).all()
    tot = R.total(st)
    assert torch.equal(tot[0], st[0].sum(0)) and tot[0].shape == (2, C)


@pytest.mark.parametrize("pooled", [False, True])
@pytest.mark.parametrize("compact", [False, True])
def test_backward_against_loops(compact, pooled):
    cs = _tiny(compact)
    b, n, m, S, C = cs["b"], cs["n"], cs["m"], cs["S"], cs["C"]
    tab = R.row_table(cs, compact)
    Y = R.forward(cs, ALL, tab)[0].float().double()
    if pooled:
        gm, _ = R.pooled_gm(cs, tab, Y)
    else:
        gm = cs["G"][:tab["R"]].double()
    ref = R.backward(cs, tab, Y, gm, Lw=11)
    dQ, dC, dW, db = np.zeros((b * n, C)), np.zeros((b * m, C)), np.zeros((3, C)), np.zeros(C)
    cnt = np.zeros(b * n)
    o = R.offsets(cs, tab).double().numpy()
    for r in range(tab["R"]):
        g, s, i = int(tab["grp"][r]), int(tab["s"][r]), int(tab["pt"][r])
        cnt[(g // m) * n + i] += 1
        for c in range(C):
            y = Y[r, c].item()
            if pooled:
                hit = int(cs["argmax"][g, c]) == s and float(cs["psc"][c]) * y + float(cs["psh"][c]) > 0
                g_ = float(cs["gpool"][g, c]) if hit else 0.0
            else:
                g_ = float(cs["G"][r, c])
            d = float(cs["p"][c]) * g_ + tab["wt"][r].item() * (float(cs["q"][c]) * y + float(cs["t"][c]))
            dQ[(g // m) * n + i, c] += d
            dC[g, c] += d
            db[c] += d
            dW[:, c] += o[r] * d
    for k, want in (("dQ", dQ), ("dCtr", dC), ("dWxyz", dW), ("dbias", db)):
        assert np.allclose(ref[k][0].numpy(), want, rtol=1e-12, atol=1e-12), k
        assert (ref[k][1] >= ref[k][0].abs() - 1e-12).all()
    assert np.array_equal(ref["dQ"][2].view(-1).numpy(), cnt) and ref["dCtr"][2] == S and ref["dbias"][2] == 11


# ------------------------------------------------------------------------------------------------------------- autograd
def _literal_forward(cs, Q, Ctr, W, bias):
    b, n, m, S, C = cs["b"], cs["n"], cs["m"], cs["S"], cs["C"]
    li = cs["idx"].long().view(b, m * S, 1)
    Yq = torch.gather(Q, 1, li.expand(b, m * S, C)).view(b, m, S, C)
    o = (torch.gather(cs["xyz"], 1, li.expand(b, m * S, 3)).view(b, m, S, 3) - cs["new_xyz"].view(b, m, 1, 3)).double()
    return Yq + Ctr.view(b, m, 1, C) + o @ W + bias


def test_against_autograd():
    cs = _tiny()
    b, n, m, S, C = cs["b"], cs["n"], cs["m"], cs["S"], cs["C"]
    leaves = [cs[k].double().requires_grad_() for k in ("Q", "Ctr", "Wxyz", "bias")]
    Y = _literal_forward(cs, *leaves)
    tab = R.row_table(cs)
    Yd = R.forward(cs, ALL, tab)[0]
    assert torch.allclose(Y.detach().view(-1, C), Yd, rtol=1e-13, atol=1e-13)
    ref = R.backward(cs, tab, Yd, cs["G"].double(), Lw=1)
    gQ, gC, gW, gb = torch.autograd.grad((ref["d"].view(b, m, S, C) * Y).sum(), leaves)
    for got, k in ((gQ.view(-1, C), "dQ"), (gC.view(-1, C), "dCtr"), (gW, "dWxyz"), (gb, "dbias")):
        assert torch.allclose(got, ref[k][0], rtol=1e-12, atol=1e-12), k
    # pooled: out[g, c] = relu(psc Y + psh) at the given arg-max slot, upstream gradient gpool; with p = psc, q = t = 0 the
    # backward is exactly that chain
    leaves = [cs[k].double().requires_grad_() for k in ("Q", "Ctr", "Wxyz", "bias")]
    Y = _literal_forward(cs, *leaves)
    act = torch.relu(cs["psc"].double() * Y + cs["psh"].double())
    out = torch.gather(act, 2, cs["argmax"].long().view(b, m, 1, C)).squeeze(2)
    grads = torch.autograd.grad((cs["gpool"].double().view(b, m, C) * out).sum(), leaves)
    cp = dict(cs, p=cs["psc"], q=torch.zeros(C), t=torch.zeros(C))
    gm, clear = R.pooled_gm(cs, tab, Yd)
    assert clear and (gm != 0).any()
    ref = R.backward(cp, tab, Yd, gm, Lw=1)
    for got, k in zip(grads, ("dQ", "dCtr", "dWxyz", "dbias")):
        assert torch.allclose(got.reshape(ref[k][0].shape), ref[k][0], rtol=1e-12, atol=1e-12), k


# ----------------------------------------------------------------------------- a correct fp32 evaluation stays inside the bound
def _fp32_forward(cs, terms, tab):
    """bias and the coordinate term first, then Ctr, then Q: not the kernels' order"""
    C = cs["C"]
    y = torch.zeros(tab["R"], C)
    if "bias" in terms:
        y = y + cs["bias"]
    if "xyz" in terms:
        o = R.offsets(cs, tab)
        y = y + o[:, 2:3] * cs["Wxyz"][2] + o[:, 1:2] * cs["Wxyz"][1] + o[:, 0:1] * cs["Wxyz"][0]
    if "Ctr" in terms:
        y = y + cs["Ctr"].view(-1, C)[tab["grp"]]
    if "Q" in terms:
        y = y + cs["Q"].view(-1, C)[tab["dst"]]
    return y


def _partials(cs, tab, name):
    """(partial of every row, number of partials, L) of the weight-gradient sums as the kernel the GPU file runs at this
    shape forms them: 16 groups per workgroup (fallback), or a cloud's groups dealt to gsplit workgroups (LDS kernel)"""
    b, m, S = cs["b"], cs["m"], cs["S"]
    if name.startswith("fallback"):
        return tab["grp"] // 16, -(-b * m // 16), 16 * S + -(-b * m // 16)
    gsplit = 3 if name == "stream_gsplit3" else 1
    jper = -(-m // gsplit)
    return (tab["grp"] // m) * gsplit + (tab["grp"] % m) // jper, b * gsplit, jper * S + b * gsplit


def _fp32_backward(cs, tab, Y32, gm32, part, nparts):
    """every sum in fp32, rows taken last to first (index_add_ on the CPU adds in the order given), the weight gradients
    per partial and then over the partials"""
    b, n, m, C = cs["b"], cs["n"], cs["m"], cs["C"]
    d = cs["p"] * gm32 + tab["wt"].float().view(-1, 1) * (cs["q"] * Y32 + cs["t"])
    rev = torch.arange(tab["R"] - 1, -1, -1)
    d, dst, grp, part = d[rev], tab["dst"][rev], tab["grp"][rev], part[rev]
    o = R.offsets(cs, tab)[rev]
    dW = torch.stack([torch.zeros(nparts, C).index_add_(0, part, o[:, k:k + 1] * d).flip(0).cumsum(0)[-1] for k in range(3)])
    return {"dQ": torch.zeros(b * n, C).index_add_(0, dst, d), "dCtr": torch.zeros(b * m, C).index_add_(0, grp, d),
            "dWxyz": dW, "dbias": torch.zeros(nparts, C).index_add_(0, part, d).flip(0).cumsum(0)[-1]}


@pytest.mark.parametrize("name,form", [(c[0], f) for c in R.SCATTER_SHAPES for f in ("stored", "pooled", "rebuilt", "pooled_rebuilt")
                                       if not f.startswith("pooled") or c[0] in POOLED_SHAPES])
def test_fp32_backward_stays_inside_the_bound(name, form):
    cs = _case(name, seed=1)
    pooled, rebuilt = form.startswith("pooled"), form.endswith("rebuilt")
    tab = R.row_table(cs)
    terms = ("xyz", "bias") if rebuilt else ("Q", "xyz", "bias")
    Yd, Ay, Ly = R.forward(cs, terms, tab)
    if rebuilt:
        Y32 = _fp32_forward(cs, terms, tab)
    else:
        Y32 = Yd.float()
        Yd, Ay, Ly = Y32.double(), None, 0
    if pooled:
        gm, clear = R.pooled_gm(cs, tab, Yd)
        gm32, clear32 = R.pooled_gm(cs, tab, Y32.double())
        assert clear and clear32 and torch.equal(gm, gm32)
        gm32 = gm32.float()
    else:
        gm, gm32 = cs["G"].double(), cs["G"]
    part, nparts, Lw = _partials(cs, tab, name)
    ref = R.backward(cs, tab, Yd, gm, Ay, Ly, True, Lw)
    got = _fp32_backward(cs, tab, Y32, gm32, part, nparts)
    for k in ("dQ", "dCtr", "dWxyz", "dbias"):
        R.check(got[k], ref[k], "%s %s %s" % (name, form, k))


@pytest.mark.parametrize("pivot", [None, "near", "far"])
@pytest.mark.parametrize("shape", FWD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fp32_forward_and_statistics_stay_inside_the_bound(shape, pivot):
    cs = R.make_case(*shape, "cpu", seed=4)
    C, S = cs["C"], cs["S"]
    tab = R.row_table(cs)
    Yt = R.forward(cs, ALL, tab)
    Y32 = _fp32_forward(cs, ALL, tab)
    R.check(Y32, Yt, "Y")
    gpb = 8 if shape[0] * shape[2] >= 8192 else 1
    P = -(-shape[0] * shape[2] // gpb)
    owner = tab["grp"] // gpb
    pv = None if pivot is None else ((Yt[0].mean(0) + 0.1 * R.vec(C, torch.Generator().manual_seed(9)).double()).float()
                                     if pivot == "near" else torch.full((C,), 1e3))
    d = Y32 - (0 if pv is None else pv)
    rev = torch.arange(tab["R"] - 1, -1, -1)
    # a workgroup's 256 / (C / 4) row lanes take every RL-th row of a group and are then added: the kernel's structure, with
    # the rows of a lane and the lanes themselves taken last to first
    RL = 256 // (C // 4)
    lane = owner * RL + tab["s"] % RL
    by_lane = lambda v: torch.zeros(P * RL, C).index_add_(0, lane[rev], v[rev]).view(P, RL, C).flip(1).cumsum(1)[:, -1]   # noqa: E731
    got = torch.stack([by_lane(d), by_lane(d * d)], 1)
    L = gpb * S + P
    for st in (R.stats(Y32.double(), tab["wt"], owner, P, L, pv), R.stats(Yt[0], tab["wt"], owner, P, L, pv, Ay=Yt[1], Ly=Yt[2])):
        R.check(got, st, "stats per partial")
        R.check(got.cumsum(0)[-1], R.total(st), "stats summed")
    o = R.offsets(cs, tab)
    x, y, z = o[:, 0], o[:, 1], o[:, 2]
    t = torch.stack([x * x, x * y, x * z, y * y, y * z, z * z, x, y, z], 1)
    mo = R.moments(o, tab["wt"], owner, P, L)
    # the moments: one thread per staged row (256 of them), then the 256 partial sums
    ml = owner * 256 + ((tab["grp"] % gpb) * S + tab["s"]) % 256
    got = torch.zeros(P * 256, 9).index_add_(0, ml[rev], t[rev]).view(P, 256, 9).flip(1).cumsum(1)[:, -1]
    R.check(got, mo, "moments per partial")
    R.check(got.cumsum(0)[-1], R.total(mo), "moments summed")


@pytest.mark.parametrize("S", [32, 64])
def test_fp32_compacted_statistics_stay_inside_the_bound(S):
    cs = R.make_case(2, 70, 6, S, 64, "cpu", seed=8, cnt=[[S, 1, 16, 17, 0, 5], [0, S, 17, 16, 1, S - 1]])
    terms = ("Q", "xyz", "bias")
    tab, full = R.row_table(cs, True), R.row_table(cs)
    assert tab["R"] < full["R"]
    Y32 = _fp32_forward(cs, terms, tab)
    R.check(Y32, R.forward(cs, terms, tab), "Y")
    w = tab["wt"].float().view(-1, 1)
    got = torch.stack([torch.zeros(12, 64).index_add_(0, tab["grp"], w * Y32),
                       torch.zeros(12, 64).index_add_(0, tab["grp"], w * Y32 * Y32)], 1)
    R.check(got, R.stats(Y32.double(), tab["wt"], tab["grp"], 12, S + 12), "compacted stats")
    Yf = R.forward(cs, terms, full)
    R.check(got, R.stats(Yf[0], full["wt"], full["grp"], 12, S + 12, Ay=Yf[1], Ly=Yf[2]), "compacted stats against all rows")


@pytest.mark.parametrize("S", [32, 64])
def test_a_wrong_weight_breaks_the_compacted_statistics(S):
    cs = R.make_case(2, 70, 6, S, 64, "cpu", seed=8, cnt=[[S, 1, 16, 17, 0, 5], [0, S, 17, 16, 1, S - 1]])
    tab = R.row_table(cs, True)
    Yd = R.forward(cs, ("Q", "xyz", "bias"), tab)[0].float().double()
    st = R.stats(Yd, tab["wt"], tab["grp"], 12, S + 12)
    mo = R.moments(R.offsets(cs, tab), tab["wt"], tab["grp"], 12, S + 12)
    R.check(st[0].float(), st, "stats")
    r0 = int(torch.nonzero(tab["wt"] > 1)[0])                  # row 0 of a compacted group
    for w in (tab["wt"][r0].item() - 1, 1.0):                  # one copy too few / the weight forgotten
        wt = tab["wt"].clone()
        wt[r0] = w
        with pytest.raises(AssertionError):
            R.check(R.stats(Yd, wt, tab["grp"], 12, S + 12)[0].float(), st, "stats")
        with pytest.raises(AssertionError):
            R.check(R.moments(R.offsets(cs, tab), wt, tab["grp"], 12, S + 12)[0].float(), mo, "moments")


def test_fp32_cloud_bias_stays_inside_the_bound():
    g = torch.Generator().manual_seed(0)
    rows, rpg, C = 1536, 512, 64
    Q, Ctr, G = torch.randn(rows, C, generator=g), torch.randn(3, C, generator=g), torch.randn(rows, C, generator=g)
    p, q, t = R.vec(C, g), R.vec(C, g), R.vec(C, g, lo=0.1)
    pv = Q.mean(0) + 0.1
    ref = R.cloud_bias(Q, Ctr, rpg, G, p, q, t, pv)
    assert ref["Y"].dtype == torch.float32 and ref["stats"][0].shape == (6, 2, C)
    d = t + q * ref["Y"] + G * p
    R.check(d, ref["dQ"], "dQ")
    rev = torch.arange(rows - 1, -1, -1)
    R.check(torch.zeros(3, C).index_add_(0, (rev // rpg), d[rev]), ref["dCtr"], "dCtr")
    e = ref["Y"] - pv
    got = torch.stack([torch.zeros(6, C).index_add_(0, rev // 256, e[rev]), torch.zeros(6, C).index_add_(0, rev // 256, (e * e)[rev])], 1)
    R.check(got, ref["stats"], "stats")


# -------------------------------------------------------------------------------------------------------- the pooled mask
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("name", POOLED_SHAPES)
def test_mask_margin_holds(name, seed):
    cs = _case(name, seed=seed)
    tab = R.row_table(cs)
    for terms in (("Q", "xyz", "bias"), ("xyz", "bias"), ("Q", "bias")):
        gm, clear = R.pooled_gm(cs, tab, R.forward(cs, terms, tab)[0].float().double())
        assert clear and (gm != 0).any()


def test_mask_margin_is_a_condition():
    cs = _tiny()
    tab = R.row_table(cs)
    Y = R.forward(cs, ALL, tab)[0]
    g, c, s = 1, 2, int(cs["argmax"][1, 2])
    Y[g * cs["S"] + s, c] = -cs["psh"][c].double() / cs["psc"][c].double() * (1 + 2.0 ** -30)
    assert not R.pooled_gm(cs, tab, Y)[1]


# ------------------------------------------------------------------------------------------------------------ sensitivity
def _mutants(cs, tab, ref, Yd):
    """(name, outputs a wrong kernel of that kind would return, the outputs it gets wrong)"""
    b, n, m, C = cs["b"], cs["n"], cs["m"], cs["C"]
    r0 = tab["R"] // 2
    inner = cs["q"].double() * Yd[r0] + cs["t"].double()
    out = []
    for kind in ("dropped", "doubled", "weight", "next_point", "quad"):
        d, dst = ref["d"].clone(), tab["dst"].clone()
        wrong = ("dQ", "dCtr", "dWxyz", "dbias")
        if kind == "dropped":
            d[r0] = 0
        elif kind == "doubled":
            d[r0] *= 2
        elif kind == "weight":
            d[r0] += inner
        elif kind == "next_point":
            if b * n == 1:
                continue                                  # a single point: there is no other row to send it to
            dst[r0] = (dst[r0] + 1) % (b * n)
            wrong = ("dQ",)
        else:
            d[r0, 0:4], d[r0, 4:8] = ref["d"][r0, 4:8], ref["d"][r0, 0:4]
        o = R.offsets(cs, tab).double()
        got = {"dQ": torch.zeros(b * n, C, dtype=D).index_add_(0, dst, d),
               "dCtr": torch.zeros(b * m, C, dtype=D).index_add_(0, tab["grp"], d), "dWxyz": o.t() @ d, "dbias": d.sum(0)}
        out.append((kind, got, wrong))
    return out


@pytest.mark.parametrize("name", [c[0] for c in R.SCATTER_SHAPES])
def test_a_wrong_row_breaks_the_bound(name):
    cs = _case(name)
    tab = R.row_table(cs)
    Yd = R.forward(cs, ("Q", "xyz", "bias"), tab)[0].float().double()
    # the largest L any kernel is given at this shape: the loosest bound a mistake has to break
    Lw = max(cs["m"] * cs["S"] + cs["b"], 16 * cs["S"] + -(-cs["b"] * cs["m"] // 16))
    ref = R.backward(cs, tab, Yd, cs["G"].double(), None, 0, True, Lw)
    for k in ("dQ", "dCtr", "dWxyz", "dbias"):
        R.check(ref[k][0].float(), ref[k], k)                                     # the unmutated one passes
    for kind, got, wrong in _mutants(cs, tab, ref, Yd):
        for k in wrong:
            with pytest.raises(AssertionError):
                R.check(got[k].float(), ref[k], "%s %s %s" % (name, kind, k))


@pytest.mark.parametrize("shape", FWD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_a_wrong_row_breaks_the_forward_bounds(shape):
    cs = R.make_case(*shape, "cpu", seed=4)
    C, S = cs["C"], cs["S"]
    tab = R.row_table(cs)
    Yt = R.forward(cs, ALL, tab)
    gpb = 8 if shape[0] * shape[2] >= 8192 else 1
    P = -(-shape[0] * shape[2] // gpb)
    owner = tab["grp"] // gpb
    L = gpb * S + P
    r0 = tab["R"] // 2
    Yw = Yt[0].clone()
    Yw[r0] = Yt[0][(r0 + S) % tab["R"]]                                          # the next group's row (another centre)
    with pytest.raises(AssertionError):
        R.check(Yw.float(), Yt, "Y")
    Yq = Yt[0].clone()
    Yq[r0, 0:4] = Yt[0][r0, 0:4].flip(0)                                         # a quad in the wrong lane order
    with pytest.raises(AssertionError):
        R.check(Yq.float(), Yt, "Y")
    Y32 = Yt[0].float().double()
    st = R.stats(Y32, tab["wt"], owner, P, L)
    mo = R.moments(R.offsets(cs, tab), tab["wt"], owner, P, L)
    for kind in ("dropped", "doubled", "misattributed"):
        wt, own = tab["wt"].clone(), owner.clone()
        if kind == "dropped":
            wt[r0] = 0
        elif kind == "doubled":
            wt[r0] = 2
        else:
            own[tab["grp"] == tab["grp"][r0]] = (owner[r0] + 1) % P               # a whole group in the next partial row
        bad_st = R.stats(Y32, wt, own, P, L)[0].float()
        bad_mo = R.moments(R.offsets(cs, tab), wt, own, P, L)[0].float()
        with pytest.raises(AssertionError):
            R.check(bad_st, st, "stats per partial")
        with pytest.raises(AssertionError):
            R.check(bad_mo, mo, "moments per partial")
        if kind == "misattributed":                                               # ... which only the per-partial check sees
            R.check(bad_st.double().sum(0), R.total(st), "stats summed")
        else:
            with pytest.raises(AssertionError):
                R.check(bad_st.double().sum(0), R.total(st), "stats summed")


# ------------------------------------------------------------------------------------------------------ pcops_rows_plan
@pytest.mark.parametrize("S", [16, 64, 256])
def test_rows_plan_against_loops(S):
    vals = [0, 1, 15, 16, 17, S - 1, S, S + 3]
    cnt = torch.tensor(vals * 3 + [S, 0, 1], dtype=torch.int32)
    bs, rows, blocks = R.rows_plan(cnt, S)
    start, want = [0], []
    for g, c in enumerate(cnt.tolist()):
        nb = min(-(-max(c, 1) // 16), S // 16)
        assert R.blocks_of(cnt, S)[g].item() == nb
        for k in range(nb):
            w = np.float32(S - 16 * nb + 1 if k == 0 else 1)
            want.append([g, 16 * k, int(w.view(np.int32)), 0])
        start.append(start[-1] + nb)
    assert bs.tolist() == start and bs.dtype == torch.int32 and rows == 16 * start[-1]
    assert blocks.dtype == torch.int32 and blocks.tolist() == want
