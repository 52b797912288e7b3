"""The algebraic backward of a pooled top layer over COMPACTED rows (pcops.h: pcops_mlp_gram_rows,
pcops_mlp_gemm_dgrad_top_rows, pcops_mlp_pool_top_addend_rows, pcops_mlp_pool_top_wsparse_rows, and
pcops_mlp_gemm_fwd_pool_rows without the Y store; the products in csrc/mlp.hip, the two sparse halves in
csrc/pooltop_sparse.hip).

Every entry point against a float64 restatement on row sets built by pcops_rows_plan from hand-made pts_cnt, to a
relative error of 2e-5 of the largest element (the bound test_bwd_fused_gpu.py holds the split-operand products to);
then the whole SA2-shaped stack with PCOPS_POOL_TOP_ROWS 1 against 0."""
import pytest
import torch

from scanobjectnn_amd import _lib, fused_mlp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-3
REL = 2e-5


def _close(name, got, want, rel=REL):
    scale = want.abs().max().item()
    err = (got.double() - want).abs().max().item()
    print("%-28s max err %.3e  largest element %.3e  ratio %.3e" % (name, err, scale, err / max(scale, 1e-300)))
    assert err <= rel * scale, (name, err, scale)


def _f(*shape):
    return torch.empty(shape, dtype=torch.float32, device=DEV)


class RowSet:
    """b x m groups of S slots with hand-made member counts: 1, 15, 16, 17, S - 1 and S members among them"""

    def __init__(self, S, G, seed):
        g = torch.Generator().manual_seed(seed)
        cnt = torch.randint(1, S + 1, (G,), generator=g, dtype=torch.int32)
        special = [1, 15, 16, 17, S - 1, S]
        for i, c in enumerate(special * 3):
            cnt[(i * 37) % G] = c
        cnt[G - 1] = 1
        cnt[0] = S
        self.S, self.G = S, G
        self.cnt = cnt.view(8, G // 8).to(DEV)
        self.rows = _lib.Rows(self.cnt, S)
        self.R = G * S                                            # uncompacted count: sizes every buffer
        self.n = self.rows.num_rows()
        bs = self.rows.block_start.long()
        self.first = 16 * bs[:-1]                                  # first compacted row of every group
        self.nrow = 16 * (bs[1:] - bs[:-1])                        # rows of every group
        want_rows = 16 * ((cnt.long() + 15) // 16)
        assert torch.equal(self.nrow.cpu(), want_rows) and self.n == int(want_rows.sum())
        w = torch.ones(self.n, dtype=torch.float64, device=DEV)
        w[self.first] = (S - self.nrow + 1).double()               # the copies left out, on the group's first row
        self.w = w
        assert abs(w.sum().item() - self.R) < 0.5


def _prev(rs, Kp, seed):
    """raw previous-layer activation (allocated at the uncompacted row count) and its BN coefficients; X in float64"""
    g = torch.Generator().manual_seed(seed)
    Yprev = torch.randn(rs.R, Kp, generator=g).to(DEV)
    psc = (0.5 + torch.rand(Kp, generator=g)).to(DEV) * (1.0 - 2.0 * (torch.arange(Kp, device=DEV) % 5 == 4))
    psh = (0.3 * torch.randn(Kp, generator=g)).to(DEV)
    X = torch.relu(Yprev[:rs.n].double() * psc.double() + psh.double())
    return Yprev, psc.contiguous(), psh, X


def _pool_inputs(rs, N, seed):
    """upstream gradient, selected raw values, arg-max rows (compacted numbering) and the pooled layer's coefficients.
    Group 0: every channel picks row 0, the weighted row.  Group 1: every coefficient zero.  Group 2: one channel alive."""
    g = torch.Generator().manual_seed(seed)
    G = rs.G
    gout = torch.randn(G, N, generator=g).to(DEV)
    ysel = torch.randn(G, N, generator=g).to(DEV)
    arg = (torch.rand(G, N, generator=g).to(DEV) * rs.nrow.view(G, 1).float()).long().clamp_(max=255)
    arg = torch.minimum(arg, rs.nrow.view(G, 1) - 1)
    sc = (0.5 + torch.rand(N, generator=g)).to(DEV)
    sh = (0.2 * torch.randn(N, generator=g)).to(DEV)
    p = (0.5 + torch.rand(N, generator=g)).to(DEV)
    arg[0] = 0
    ysel[1] = -100.0                                               # relu(bn(ysel)) == 0 everywhere: no coefficient
    ysel[2] = -100.0
    ysel[2, 7] = 1.0
    arg[3] = rs.nrow[3] - 1                                        # the last row of a group
    active = (ysel.double() * sc.double() + sh.double()) > 0
    cf = torch.where(active, p.double() * gout.double(), torch.zeros((), dtype=torch.float64, device=DEV))
    return gout, ysel, arg.to(torch.uint8).contiguous(), sc, sh, p, cf, arg


SHAPES = [(64, 128, 256), (128, 128, 256), (64, 64, 128), (128, 64, 128)]     # (S, Kp, N)


@pytest.mark.parametrize("S,Kp,N", SHAPES)
def test_entry_points_against_float64(S, Kp, N):
    lib = _lib.load()
    G = 65536 // S if S == 64 else 131072 // S
    rs = RowSet(S, G, seed=S + Kp)
    R, n = rs.R, rs.n
    assert lib.pcops_mlp_pool_top_rows_supported(R, Kp, N, S) == 1
    Yprev, psc, psh, X = _prev(rs, Kp, seed=3)
    gout, ysel, arg8, sc, sh, p, cf, arg = _pool_inputs(rs, N, seed=4)
    g = torch.Generator().manual_seed(5)
    rref = rs.rows.ref

    # ---- Gram matrix with row weights: X^T diag(w) X, X^T w
    splits = lib.pcops_mlp_wgrad_splits(R, Kp, Kp)
    scratch, gram, xsum = _f(splits * (Kp * Kp + Kp)), _f(Kp, Kp), _f(Kp)
    _lib.call("pcops_mlp_gram_rows", R, Kp, Yprev.data_ptr(), Kp, psc.data_ptr(), psh.data_ptr(), scratch.data_ptr(),
              gram.data_ptr(), xsum.data_ptr(), rref)
    _close("gram", gram, X.t() @ (X * rs.w.view(-1, 1)))
    _close("xsum", xsum, X.t() @ rs.w)

    # ---- addend: the rows of (p.G) W^T that are not zero, and the row -> slot map
    Wt = (torch.randn(N, Kp, generator=g) / N ** 0.5).to(DEV)
    addend, rowmap = _f(R, Kp).fill_(float("nan")), torch.full((R,), -7, dtype=torch.int32, device=DEV)
    _lib.call("pcops_mlp_pool_top_addend_rows", R, Kp, N, S, gout.data_ptr(), ysel.data_ptr(), arg8.data_ptr(),
              sc.data_ptr(), sh.data_ptr(), p.data_ptr(), Wt.data_ptr(), addend.data_ptr(), rowmap.data_ptr(), rref)
    rowof = (rs.first.view(G, 1) + arg).reshape(-1)               # compacted row of slot (g, a): 16 block_start[g] + a
    want_add = torch.zeros(n, Kp, dtype=torch.float64, device=DEV)
    want_add.index_add_(0, rowof, cf.reshape(-1, 1) * Wt.double().repeat(G, 1))
    hit = torch.zeros(n, dtype=torch.bool, device=DEV)
    hit[rowof[cf.reshape(-1) != 0]] = True
    rm = rowmap[:n].long()
    assert torch.equal(rm >= 0, hit), "rowmap: a slot exactly where a coefficient lands"
    assert int(rm.max()) < R and int(rm[~hit].max()) == -1 and int(rm[~hit].min()) == -1
    assert rm[hit].unique().numel() == int(hit.sum())             # every row its own slot
    got_add = torch.zeros(n, Kp, dtype=torch.float64, device=DEV)
    got_add[hit] = addend[rm[hit]].double()
    _close("addend", got_add, want_add)
    f0, f1 = int(rs.first[0]), int(rs.first[1])
    assert not hit[f1:f1 + int(rs.nrow[1])].any()                 # the all-zero group owns no slot
    assert int(hit[f0:f0 + int(rs.nrow[0])].sum()) == 1 and bool(hit[f0])     # everything on the weighted row

    # ---- data gradient: mask_prev . (w (X Mq + v) + addend[rowmap]) and its statistics
    Mq = (torch.randn(Kp, Kp, generator=g) / Kp ** 0.5).to(DEV)
    v = (0.1 * torch.randn(Kp, generator=g)).to(DEV)
    Gprev, part = _f(R, Kp), _f(lib.pcops_mlp_stats_rows(R), 2, Kp)
    _lib.call("pcops_mlp_gemm_dgrad_top_rows", R, Kp, Yprev.data_ptr(), psc.data_ptr(), psh.data_ptr(), Mq.data_ptr(),
              v.data_ptr(), addend.data_ptr(), addend.shape[0], rowmap.data_ptr(), Gprev.data_ptr(), part.data_ptr(), rref)
    mask = (Yprev[:n].double() * psc.double() + psh.double()) > 0
    want_g = mask * (rs.w.view(-1, 1) * (X @ Mq.double() + v.double()) + got_add)
    _close("Gprev", Gprev[:n], want_g)
    _close("Gprev first rows", Gprev[rs.first], want_g[rs.first])
    sums = part.double().sum(0)
    # the statistics' error is judged on the sum of magnitudes (they are sums of terms of either sign)
    for name, got_s, terms in (("stats sum dX", sums[0], want_g), ("stats sum dX Yprev", sums[1], want_g * Yprev[:n].double())):
        err = (got_s - terms.sum(0)).abs().max().item()
        scale = terms.abs().sum(0).max().item()
        print("%-28s max err %.3e  sum of magnitudes %.3e" % (name, err, scale))
        assert err <= REL * scale, (name, err, scale)

    # ---- sparse half of the weight gradient: X^T (p.G), 1^T (p.G)
    Ssp, cfsum = _f(Kp, N), _f(N)
    wpart = _f(int(lib.pcops_mlp_pool_top_wsparse_rows_partial(Kp, N)))
    _lib.call("pcops_mlp_pool_top_wsparse_rows", R, Kp, N, S, gout.data_ptr(), ysel.data_ptr(), arg8.data_ptr(),
              sc.data_ptr(), sh.data_ptr(), p.data_ptr(), Yprev.data_ptr(), psc.data_ptr(), psh.data_ptr(),
              Ssp.data_ptr(), cfsum.data_ptr(), wpart.data_ptr(), rref)
    want_s = torch.zeros(Kp, N, dtype=torch.float64, device=DEV)
    for g0 in range(0, G, 256):                                    # (G, N, Kp) float64 in slices
        rows_ = rowof.view(G, N)[g0:g0 + 256]
        want_s += torch.einsum("gc,gck->kc", cf[g0:g0 + 256], X[rows_.reshape(-1)].view(rows_.shape[0], N, Kp))
    _close("Ssp", Ssp, want_s)
    _close("cfsum", cfsum, cf.sum(0))
    torch.cuda.synchronize()


@pytest.mark.parametrize("S,Kp,N", [(64, 128, 256), (128, 64, 128)])
def test_rows_null_is_the_plain_entry_point(S, Kp, N):
    """rows == NULL: exactly the entry point without the suffix (bit for bit)"""
    lib = _lib.load()
    R = 65536
    g = torch.Generator().manual_seed(9)
    Yprev = torch.randn(R, Kp, generator=g).to(DEV)
    psc, psh = (0.5 + torch.rand(Kp, generator=g)).to(DEV), (0.3 * torch.randn(Kp, generator=g)).to(DEV)
    splits = lib.pcops_mlp_wgrad_splits(R, Kp, Kp)
    out = []
    for name, tail in (("pcops_mlp_gram", ()), ("pcops_mlp_gram_rows", (None,))):
        scratch, gram, xsum = _f(splits * (Kp * Kp + Kp)), _f(Kp, Kp), _f(Kp)
        _lib.call(name, R, Kp, Yprev.data_ptr(), Kp, psc.data_ptr(), psh.data_ptr(), scratch.data_ptr(), gram.data_ptr(),
                  xsum.data_ptr(), *tail)
        out.append((gram, xsum))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.parametrize("S,K,N", [(64, 128, 256), (128, 64, 128)])
def test_pooled_forward_without_the_store(S, K, N):
    """pcops_mlp_gemm_fwd_pool_rows with Y == NULL: block partials and statistics bit-identical to the storing call"""
    lib = _lib.load()
    rs = RowSet(S, 65536 // S if S == 64 else 131072 // S, seed=11)
    R = rs.R
    assert lib.pcops_mlp_gemm_fwd_pool_rows_supported(R, K, N) == 1
    Yprev, psc, psh, _ = _prev(rs, K, seed=12)
    g = torch.Generator().manual_seed(13)
    W = (torch.randn(K, N, generator=g) / K ** 0.5).to(DEV)
    b = (0.1 * torch.randn(N, generator=g)).to(DEV)
    gamma = ((0.5 + torch.rand(N, generator=g)) * (1.0 - 2.0 * (torch.arange(N) % 3 == 2))).to(DEV)
    piv = (0.1 * torch.randn(N, generator=g)).to(DEV)
    nbk = rs.rows.blocks.shape[0]
    res = []
    for store in (True, False):
        Y = _f(R, N) if store else None
        part = _f(lib.pcops_mlp_stats_rows(R), 2, N).fill_(float("nan"))
        ypart, ppart = _f(nbk, N).zero_(), torch.zeros((nbk, N), dtype=torch.uint8, device=DEV)
        _lib.call("pcops_mlp_gemm_fwd_pool_rows", R, K, N, Yprev.data_ptr(), K, psc.data_ptr(), psh.data_ptr(),
                  W.data_ptr(), b.data_ptr(), gamma.data_ptr(), Y.data_ptr() if store else None, part.data_ptr(),
                  piv.data_ptr(), ypart.data_ptr(), ppart.data_ptr(), rs.rows.ref)
        res.append((part, ypart, ppart))
    for a, c in zip(res[0], res[1]):
        assert torch.equal(a, c)
    assert torch.isfinite(res[1][0]).all()


def _sa2_stack(B, seed=0):
    from scanobjectnn_amd.pointnet2 import tf_grouping, tf_sampling
    from scanobjectnn_amd.synth import synth_clouds
    N, M, S, widths = 512, 128, 64, [128, 128, 256]
    g = torch.Generator().manual_seed(seed)
    xyz = torch.from_numpy(synth_clouds(B, N, seed=seed + 3)).to(DEV)
    new_xyz = tf_sampling.gather_point(xyz, tf_sampling.farthest_point_sample(M, xyz))
    idx, cnt = tf_grouping.query_ball_point(0.4, S, xyz, new_xyz)
    C1 = widths[0]
    Q = (0.5 * torch.randn(B, N, C1, generator=g)).to(DEV)
    wxyz = torch.randn(3, C1, generator=g).to(DEV)
    layers, cin = [], C1
    for w in widths:
        layers.append([(torch.randn(cin, w, generator=g) / cin ** 0.5).to(DEV), (0.1 * torch.randn(w, generator=g)).to(DEV),
                       ((0.5 + torch.rand(w, generator=g)) * (1.0 - 2.0 * (torch.arange(w) % 3 == 2))).to(DEV),
                       (0.2 * torch.randn(w, generator=g)).to(DEV), (0.1 * torch.randn(w, generator=g)).to(DEV),
                       (0.5 + torch.rand(w, generator=g)).to(DEV)])
        cin = w
    go = torch.randn(B * M, widths[-1], generator=g).to(DEV)
    return dict(idx=idx, cnt=cnt, xyz=xyz, new_xyz=new_xyz, Q=Q, wxyz=wxyz, layers=layers, go=go, R=B * M * S, N=widths[-1])


def _run(st, record=None):
    Q, wxyz = st["Q"].clone().requires_grad_(True), st["wxyz"].clone().requires_grad_(True)
    ls = [[t.clone().requires_grad_(True) for t in l[:4]] + [l[4].clone(), l[5].clone()] for l in st["layers"]]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    hook = (lambda name, phase, args: record.append((name, args)) if phase == "pre" else None) if record is not None else None
    if hook:
        _lib._hooks.append(hook)
    try:
        out = fused_mlp.gather_mlp_stack(st["idx"], True, True, 0.9, EPS, True, [tuple(l) for l in ls], Q=Q, xyz=st["xyz"],
                                         new_xyz=st["new_xyz"], wxyz=wxyz, pts_cnt=st["cnt"])
        assert out.grad_fn.rows is not None, "the stack was expected to run on compacted rows"
        torch.cuda.synchronize()
        peak_fwd = torch.cuda.max_memory_allocated() - base
        out.backward(st["go"])
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
    finally:
        if hook:
            _lib._hooks.remove(hook)
    grads = [Q.grad, wxyz.grad] + [t.grad for li, l in enumerate(ls) for ti, t in enumerate(l[:4]) if not (li == 0 and ti < 2)]
    names = ["dQ", "dwxyz"] + ["L%d.%s" % (li, n) for li in range(len(ls)) for ti, n in enumerate(("dW", "db", "dgamma", "dbeta"))
                               if not (li == 0 and ti < 2)]
    return out.detach().clone(), names, [t.clone() for t in grads], peak_fwd, peak


ALGEBRAIC = ("pcops_mlp_gemm_dgrad_top_rows", "pcops_mlp_gram_rows", "pcops_mlp_pool_top_addend_rows",
             "pcops_mlp_pool_top_wsparse_rows")


def test_sa2_stack_takes_the_rows_form_and_equals_the_plain_one(monkeypatch):
    """gather_mlp_stack at an SA2-shaped compacted stack, PCOPS_POOL_TOP_ROWS 1 against 0: same forward bits, every
    gradient within 2e-4 * scale + 1e-6 (the bound of the uncompacted comparison in test_fused_mlp_gpu.py), the four
    *_rows entry points on the call hook with the row set, the pooled forward called with Y = None.

    Memory: the forward peak falls by the whole of Y (R x 256 floats).  Over forward + backward the form gives part of
    it back -- the addend is R x 128 floats, half of Y, next to the Gram / sparse-half partial sums -- so that peak is
    asserted to fall by a quarter of Y at least; both figures are printed."""
    st = _sa2_stack(32)
    res = {}
    for mode in (True, False):
        monkeypatch.setattr(fused_mlp, "POOL_TOP_ROWS", mode)
        rec = []
        res[mode] = _run(st, rec)
        called = [n for n, _ in rec]
        fwd = [a for n, a in rec if n == "pcops_mlp_gemm_fwd_pool_rows"]
        assert len(fwd) == 1
        if mode:
            for want in ALGEBRAIC:
                hits = [a for n, a in rec if n == want]
                assert len(hits) == 1 and hits[0][-1] is not None, (want, called)
            assert fwd[0][10] is None                             # Y: not stored
            assert "pcops_mlp_gemm_dgrad_rows" in called          # (the layers below keep their kernels)
        else:
            assert not set(ALGEBRAIC) & set(called) and fwd[0][10] is not None
    assert torch.equal(res[True][0], res[False][0])
    go_scale = st["go"].abs().max().item()
    for name, a, b in zip(res[True][1], res[True][2], res[False][2]):
        scale = go_scale if name.endswith(".db") else b.abs().max().item()
        err = (a - b).abs().max().item()
        print("%-10s max diff %.3e  scale %.3e" % (name, err, scale))
        assert err <= 2e-4 * scale + 1e-6, (name, err, scale)
    ybytes = st["R"] * st["N"] * 4
    print("Y %.1f MB; forward peak %.1f -> %.1f MB; forward + backward peak %.1f -> %.1f MB" % (
        ybytes / 1e6, res[False][3] / 1e6, res[True][3] / 1e6, res[False][4] / 1e6, res[True][4] / 1e6))
    assert res[False][3] - res[True][3] >= 0.95 * ybytes
    assert res[False][4] - res[True][4] >= 0.25 * ybytes


def test_rows_form_is_deterministic():
    """two runs of the new path: bit-identical output and gradients (fixed-order sums, no float atomics).  The library's
    deterministic mode is on: outside it the scatter-add BELOW the stack (dQ, dwxyz: float atomics) differs between
    two runs of any path, the plain one included."""
    st = _sa2_stack(8, seed=2)
    _lib.set_deterministic(True)
    try:
        rec = []
        a = _run(st, rec)
        assert set(ALGEBRAIC) <= {n for n, _ in rec}
        b = _run(st)
    finally:
        _lib.set_deterministic(False)
    assert torch.equal(a[0], b[0])
    for name, x, y in zip(a[1], a[2], b[2]):
        assert torch.equal(x, y), name
