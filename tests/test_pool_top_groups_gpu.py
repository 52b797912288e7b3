"""The algebraic backward of a pooled top layer over many small uncompacted groups (pcops.h: pcops_mlp_dgrad_top_groups,
pcops_mlp_wgrad_top_groups): both entry points against the float64 restatement of pool_top_groups_ref.py, to 2e-5 of the
largest element (statistics: 2e-5 of the sum of magnitudes), the bounds of test_pool_top_rows_gpu.py; then an SA1-shaped
stack at the planner's row floor with PCOPS_POOL_TOP_GROUPS 1 against 0."""
import pytest
import torch

import pool_top_groups_ref as PR
from scanobjectnn_amd import _lib, fused_mlp
from test_fused_mlp_gpu import make_layers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-3
REL = 2e-5
UNSUPPORTED = -4


def _close(name, got, want, rel=REL):
    scale = want.abs().max().item()
    err = (got.double() - want).abs().max().item()
    print("%-22s max err %.3e  largest element %.3e  ratio %.3e" % (name, err, scale, err / max(scale, 1e-300)))
    assert torch.isfinite(got).all(), name
    assert err <= rel * scale, (name, err, scale)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _inputs(S, Kp, N, G, seed):
    """Hand-made groups (where G has them): 0 every channel picks row 0, and X of that row is all <= 0; 1 every channel
    picks the last row; 2 every coefficient zero; 3 one live channel; 4 every channel picks row 5 (rows 4 and 6: none);
    5 row 7 has X <= 0 everywhere.  Every fifth prev_scale and every third pool_scale entry is negative."""
    g = torch.Generator().manual_seed(seed)
    M = G * S
    Yprev = torch.randn(M, Kp, generator=g).to(DEV)
    psc = ((0.5 + torch.rand(Kp, generator=g)) * (1.0 - 2.0 * (torch.arange(Kp) % 5 == 4))).to(DEV)
    psh = (0.3 * torch.randn(Kp, generator=g)).to(DEV)
    gout = torch.randn(G, N, generator=g).to(DEV)
    ysel = torch.randn(G, N, generator=g).to(DEV)
    arg = torch.randint(0, S, (G, N), generator=g).to(DEV)
    sc = ((0.5 + torch.rand(N, generator=g)) * (1.0 - 2.0 * (torch.arange(N) % 3 == 2))).to(DEV)
    sh = (0.2 * torch.randn(N, generator=g)).to(DEV)
    p = (0.5 + torch.rand(N, generator=g)).to(DEV)
    dead = -100.0 * torch.sign(sc)                                # relu(bn(ysel)) == 0
    arg[0] = 0
    Yprev[0] = -10.0 * torch.sign(psc)
    if G > 1:
        arg[1] = S - 1
    if G > 2:
        ysel[2] = dead
    if G > 5:
        ysel[3] = dead
        ysel[3, 7] = -dead[7]
        arg[4] = 5
        Yprev[5 * S + 7] = -10.0 * torch.sign(psc)
    Wt = (torch.randn(N, Kp, generator=g) / N ** 0.5).to(DEV)
    Mq = (torch.randn(Kp, Kp, generator=g) / Kp ** 0.5).to(DEV)
    v = (0.1 * torch.randn(Kp, generator=g)).to(DEV)
    return dict(Yprev=Yprev, psc=psc.contiguous(), psh=psh, gout=gout, ysel=ysel, arg=arg.to(torch.uint8).contiguous(),
                sc=sc.contiguous(), sh=sh, p=p, Wt=Wt, Mq=Mq, v=v)


def _dgrad(M, Kp, N, S, d):
    P = _lib.load().pcops_mlp_stats_rows(M)
    Gprev, part = _nan(M, Kp), _nan(P, 2, Kp)
    _lib.call("pcops_mlp_dgrad_top_groups", M, Kp, N, S, d["Yprev"].data_ptr(), d["psc"].data_ptr(), d["psh"].data_ptr(),
              d["Mq"].data_ptr(), d["v"].data_ptr(), d["gout"].data_ptr(), d["ysel"].data_ptr(), d["arg"].data_ptr(),
              d["sc"].data_ptr(), d["sh"].data_ptr(), d["p"].data_ptr(), d["Wt"].data_ptr(), Gprev.data_ptr(), part.data_ptr())
    return Gprev, part


def _wgrad(M, Kp, N, S, d):
    scratch = _nan(int(_lib.load().pcops_mlp_pool_top_groups_partial(M, Kp, N)))
    gram, xsum, Ssp, cfsum = _nan(Kp, Kp), _nan(Kp), _nan(Kp, N), _nan(N)
    _lib.call("pcops_mlp_wgrad_top_groups", M, Kp, N, S, d["Yprev"].data_ptr(), d["psc"].data_ptr(), d["psh"].data_ptr(),
              d["gout"].data_ptr(), d["ysel"].data_ptr(), d["arg"].data_ptr(), d["sc"].data_ptr(), d["sh"].data_ptr(),
              d["p"].data_ptr(), scratch.data_ptr(), gram.data_ptr(), xsum.data_ptr(), Ssp.data_ptr(), cfsum.data_ptr())
    return gram, xsum, Ssp, cfsum


# fewer groups than a tile holds, a ragged last tile, more tiles than workgroups (two tiles each at 67 and 515 groups of 32)
@pytest.mark.parametrize("G", [1, 3, 67, 515])
@pytest.mark.parametrize("S,Kp,N", [(32, 64, 128), (64, 64, 128), (32, 64, 256)])
def test_entry_points_against_float64(S, Kp, N, G):
    M = G * S
    d = _inputs(S, Kp, N, G, seed=S + N + G)
    Gprev, part = _dgrad(M, Kp, N, S, d)
    want_g, terms = PR.dgrad_top_groups(S, d["Yprev"], d["psc"], d["psh"], d["Mq"], d["v"], d["gout"], d["ysel"], d["arg"],
                                        d["sc"], d["sh"], d["p"], d["Wt"])
    _close("Gprev", Gprev, want_g)
    assert not Gprev[0].any()                                      # the row whose X is <= 0 everywhere: mask all zero
    assert torch.isfinite(part).all()
    sums = part.double().sum(0)
    for name, got_s, tm in (("stats sum dX", sums[0], terms[0]), ("stats sum dX Yprev", sums[1], terms[1])):
        err = (got_s - tm.sum(0)).abs().max().item()
        scale = tm.abs().sum(0).max().item()
        print("%-22s max err %.3e  sum of magnitudes %.3e" % (name, err, scale))
        assert err <= REL * scale, (name, err, scale)
    got_w = _wgrad(M, Kp, N, S, d)
    want_w = PR.wgrad_top_groups(S, d["Yprev"], d["psc"], d["psh"], d["gout"], d["ysel"], d["arg"], d["sc"], d["sh"], d["p"])
    for name, a, b in zip(("gram", "xsum", "Ssp", "cfsum"), got_w, want_w):
        _close(name, a, b)
    assert torch.equal(got_w[0], got_w[0].t())                     # mirrored, bit for bit
    # ---- a second call: the same bits
    Gprev2, part2 = _dgrad(M, Kp, N, S, d)
    assert torch.equal(Gprev, Gprev2) and torch.equal(part, part2)
    for a, b in zip(got_w, _wgrad(M, Kp, N, S, d)):
        assert torch.equal(a, b)
    torch.cuda.synchronize()


@pytest.mark.parametrize("M,Kp,N,S", [(262144, 128, 256, 32), (262144, 32, 128, 32), (262144, 64, 96, 32), (262144, 64, 288, 32),
                                      (262144, 64, 144, 32), (262144, 64, 128, 16), (262144, 64, 128, 48),
                                      (262144, 64, 128, 128), (262144 + 16, 64, 128, 32), (1 << 24, 64, 128, 32)])
def test_shapes_outside_the_set_are_refused(M, Kp, N, S):
    """PCOPS_ERR_UNSUPPORTED from both entry points before any pointer is looked at, 0 from the query"""
    lib = _lib.load()
    assert lib.pcops_mlp_pool_top_groups_supported(M, Kp, N, S) == 0
    assert lib.pcops_mlp_dgrad_top_groups(M, Kp, N, S, *([None] * 14), None) == UNSUPPORTED
    assert lib.pcops_mlp_wgrad_top_groups(M, Kp, N, S, *([None] * 14), None) == UNSUPPORTED


def test_query_has_the_row_floor_the_entry_points_do_not():
    lib = _lib.load()
    for S, N in ((32, 128), (64, 128), (32, 256)):
        assert lib.pcops_mlp_pool_top_groups_supported(262144, 64, N, S) == 1
        assert lib.pcops_mlp_pool_top_groups_supported(262144 - S, 64, N, S) == 0
        assert lib.pcops_mlp_pool_top_groups_supported(131072, 64, N, S) == 0


# ------------------------------------------------------------------------------------------------ the stack
def _sa1_stack(B=16, seed=0):
    from scanobjectnn_amd.pointnet2 import tf_grouping, tf_sampling
    from scanobjectnn_amd.synth import synth_clouds
    M, S, widths = 512, 32, [64, 64, 128]
    g = torch.Generator().manual_seed(seed)
    xyz = torch.from_numpy(synth_clouds(B, 2048, seed=seed + 3)).to(DEV)
    new_xyz = tf_sampling.gather_point(xyz, tf_sampling.farthest_point_sample(M, xyz))
    idx, _ = tf_grouping.query_ball_point(0.2, S, xyz, new_xyz)
    wxyz = torch.randn(3, widths[0], generator=g).to(DEV)
    bias = (0.1 * torch.randn(widths[0], generator=g)).to(DEV)
    go = torch.randn(B * M, widths[-1], generator=g).to(DEV)
    return dict(idx=idx, xyz=xyz, new_xyz=new_xyz, wxyz=wxyz, bias=bias, layers=make_layers(widths[0], widths, seed=seed + 1),
                go=go, R=B * M * S, N=widths[-1])


def _run(st, record):
    wxyz, bias = st["wxyz"].clone().requires_grad_(True), st["bias"].clone().requires_grad_(True)
    ls = [[t.clone().requires_grad_(True) for t in l[:4]] + [l[4].clone(), l[5].clone()] for l in st["layers"]]
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    hook = lambda name, phase, args: record.append((name, args)) if phase == "pre" else None     # noqa: E731
    _lib._hooks.append(hook)
    try:
        out = fused_mlp.gather_mlp_stack(st["idx"], True, True, 0.9, EPS, True, [tuple(l) for l in ls], xyz=st["xyz"],
                                         new_xyz=st["new_xyz"], wxyz=wxyz, bias=bias)
        out.backward(st["go"])
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
    finally:
        _lib._hooks.remove(hook)
    named = [("dwxyz", wxyz.grad), ("dbias", bias.grad)]
    named += [("L%d.%s" % (li, n), t.grad) for li, l in enumerate(ls) for ti, (n, t) in
              enumerate(zip(("dW", "db", "dgamma", "dbeta"), l[:4])) if not (li == 0 and ti < 2)]
    return out.detach().clone(), [n for n, _ in named], [t.clone() for _, t in named], peak


GROUPS = ("pcops_mlp_wgrad_top_groups", "pcops_mlp_dgrad_top_groups")


def test_sa1_stack_takes_the_groups_form_and_equals_the_one_pass_form(monkeypatch):
    """gather_mlp_stack on an SA1-shaped stack at the row floor (16 x 512 x 32 = 262 144 rows, coordinate-only first layer,
    widths 64-64-128), PCOPS_POOL_TOP_GROUPS 1 against 0: same forward bits, every gradient within 2e-4 * scale + 1e-6
    (the bound of the uncompacted comparison in test_fused_mlp_gpu.py), the two entry points on the call hook, the pooled
    forward called with Y = None, and a forward + backward peak lower by the size of Y at least."""
    st = _sa1_stack()
    assert st["R"] == 262144
    res = {}
    for mode in (True, False):
        monkeypatch.setattr(fused_mlp, "POOL_TOP_GROUPS", mode)
        rec = []
        res[mode] = _run(st, rec)
        called = [n for n, _ in rec]
        fwd = [a for n, a in rec if n == "pcops_mlp_gemm_fwd_pool"]
        assert len(fwd) == 1
        if mode:
            assert all(called.count(n) == 1 for n in GROUPS), called
            assert fwd[0][11] is None                               # Y: not stored
            assert "pcops_mlp_bwd_fused_gw" not in called and "pcops_mlp_pool_top_addend" not in called
            assert "pcops_mlp_bwd_fused_xyz_rows" in called         # (the layer below keeps its kernel)
        else:
            assert not set(GROUPS) & set(called) and fwd[0][11] is not None
    assert torch.equal(res[True][0], res[False][0])
    go_scale = st["go"].abs().max().item()
    for name, a, b in zip(res[True][1], res[True][2], res[False][2]):
        # the gradient of a bias in front of a batch norm (the first layer's too) is zero in exact arithmetic: both forms
        # return rounding noise there, judged on the scale of the upstream gradient as in test_fused_mlp_gpu.py
        scale = go_scale if name.endswith(".db") or name == "dbias" else b.abs().max().item()
        err = (a - b).abs().max().item()
        print("%-10s max diff %.3e  scale %.3e" % (name, err, scale))
        assert err <= 2e-4 * scale + 1e-6, (name, err, scale)
    ybytes = st["R"] * st["N"] * 4
    print("Y %.1f MB; forward + backward peak %.1f -> %.1f MB" % (ybytes / 1e6, res[False][3] / 1e6, res[True][3] / 1e6))
    assert res[False][3] - res[True][3] >= ybytes
