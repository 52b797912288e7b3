"""pcops_sa_scatter_bwd_rows, the chunked walk over the inverse index (csrc/gather.hip), held to a float64 reference element
by element in BOTH of its forms: the Y form (PCOPS_OPT_SCATTER_QFORM = 0, reads the rows of Y) and the Q form (= 1, the
default: Y = Q[idx] + offsets Wxyz + bias is a function of what the call was handed, so its rows are not read).

Y is made by the product's own pcops_sa_gather_fwd_rows from Q, Wxyz, bias, so both forms are given the same, consistent Y.
Reference: d[r] = p.G[r] + wt_r (q.Y[r] + t) in float64, scattered over idx (dQ) and reduced (dWxyz = sum o_r^T d[r],
dbias = sum d[r]); wt_r is 1 except on row 0 of a compacted group, which also stands for the copies left out.

Per-element bound, as in tests/test_gemm_plans_gpu.py:
    |out - ref| <= C (L + 8) 2^-24 sum|terms|,   C = 2
An fp32 sum of L terms in any order is within (L - 1) 2^-24 of the sum of their absolute values; a row's term is itself a
few roundings deep (the products with p, q, wt, the offset subtraction, and in the Q form the sums W_i, O_i and the moments
that replace Y), which the + 8 pays for.  sum|terms| is the same sum in float64 with absolute values taken term by term and
|Y| replaced by its parts |Q[i]| + sum_a |Wxyz[a]| |o_r[a]| + |bias|: the Q form's intermediates are those parts, not Y, so
one bound serves both forms.
  dQ[b, i]     : L = number of rows that name point i in cloud b.
  dWxyz, dbias : L = rows per partial + number of partials.  The walk deals 64-row (small problems: 16-row) chunks of the
                 sorted list round-robin to the waves of a persistent grid (1024 workgroups in the Y form, 768 in the Q
                 form), every workgroup writes one partial and a second kernel adds the partials.  A workgroup's partial is
                 therefore at most ceil(chunks / (768 * 4)) * 4 chunks deep (chunks counted on the uncompacted row
                 count, as the kernels do), and there are at most 1024 partials: L = that depth + 1024 covers both forms.
A dropped or doubled row, a wrong weight, a wrong point or group breaks the bound by orders of magnitude.

Each case also reads back which form ran (pcops_last_launch_plan: path 8, [1] = 1 for the Q form) and checks that a
point no row names gets a gradient row of exact zeros."""
import ctypes

import pytest
import torch

from scanobjectnn_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
C_BOUND = 2.0
KBLK = 16


def plan():
    out = (ctypes.c_int * 5)()
    assert _lib.load().pcops_last_launch_plan(out, 5) == 5
    return tuple(out)


def _p(t):
    return t.data_ptr() if t is not None else None


def _vec(n, g, lo=0.5):
    s = 1.0 - 2.0 * (torch.arange(n, device=DEV) % 3 == 1)
    return (lo + torch.rand(n, generator=g, device=DEV)) * s


def make_case(b, n, m, S, C, compact, has_xyz, has_bias, special, seed=0):
    """inputs of one call.  special: cloud 0 names ONE point in all of its rows (the longest possible list) and no cloud
    names point n - 1."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    hi = n - 1 if special else n
    idx = torch.randint(0, hi, (b, m, S), device=DEV, generator=g, dtype=torch.int32)
    # ball-query layout: a group has cnt hits, the rest of its S rows repeat the first
    cnt = torch.randint(1, S + 1, (b, m), device=DEV, generator=g, dtype=torch.int32)
    cnt[:, 0] = S
    if m > 1:
        cnt[:, 1] = 1
    pad = torch.arange(S, device=DEV).view(1, 1, S) >= cnt.unsqueeze(-1)
    idx = torch.where(pad, idx[:, :, :1].expand(b, m, S), idx).contiguous()
    if special:
        idx[0] = min(5, n - 2)
    xyz = torch.rand(b, n, 3, device=DEV, generator=g)
    new_xyz = torch.rand(b, m, 3, device=DEV, generator=g)
    Q = torch.randn(b, n, C, device=DEV, generator=g)
    Wxyz = torch.randn(3, C, device=DEV, generator=g) if has_xyz else None
    bias = torch.randn(C, device=DEV, generator=g) if has_bias else None
    rows = _lib.Rows(cnt, S) if compact else None
    R = rows.num_rows() if compact else b * m * S
    Gm = torch.randn(R, C, device=DEV, generator=g)
    p, q, t = _vec(C, g), _vec(C, g), _vec(C, g, lo=0.1)
    # the forward's own Y
    Y = torch.full((R, C), float("nan"), device=DEV)
    _lib.call("pcops_sa_gather_fwd_rows", b, n, m, S, C, Q.data_ptr(), None, _p(xyz if has_xyz else None),
              _p(new_xyz if has_xyz else None), _p(Wxyz), _p(bias), idx.data_ptr(), Y.data_ptr(), None, None, None, None,
              rows.ref if compact else None)
    torch.cuda.synchronize()
    assert torch.isfinite(Y).all()
    return dict(b=b, n=n, m=m, S=S, C=C, idx=idx, cnt=cnt, xyz=xyz, new_xyz=new_xyz, Q=Q, Wxyz=Wxyz, bias=bias, rows=rows, R=R,
                G=Gm, p=p, q=q, t=t, Y=Y, has_xyz=has_xyz, special=special)


def row_table(cs):
    """(group, point, weight) of every row of G / Y, in float64 / int64"""
    b, m, S = cs["b"], cs["m"], cs["S"]
    idx2 = cs["idx"].view(b * m, S).long()
    if cs["rows"] is None:
        r = torch.arange(b * m * S, device=DEV)
        grp, s = r // S, r % S
        wt = torch.ones(b * m * S, dtype=torch.float64, device=DEV)
    else:
        nb = cs["R"] // KBLK
        blk = cs["rows"].blocks[:nb]
        j = torch.arange(KBLK, device=DEV).view(1, KBLK)
        grp = blk[:, 0].long().view(nb, 1).expand(nb, KBLK).reshape(-1)
        s = (blk[:, 1].long().view(nb, 1) + j).reshape(-1)
        w = blk[:, 2].contiguous().view(torch.float32).double().view(nb, 1)
        wt = torch.where(j == 0, w.expand(nb, KBLK), torch.ones(nb, KBLK, dtype=torch.float64, device=DEV)).reshape(-1)
        # the compacted set must stand for every row of the call: the weights add up to the uncompacted row count
        assert wt.sum().item() == b * m * S
    return grp, idx2[grp, s], wt


def reference(cs):
    b, n, m, C = cs["b"], cs["n"], cs["m"], cs["C"]
    grp, pt, wt = row_table(cs)
    cloud = grp // m
    dst = cloud * n + pt
    pd, qd, td = cs["p"].double(), cs["q"].double(), cs["t"].double()
    Gd, Yd = cs["G"].double(), cs["Y"].double()
    d = pd * Gd + wt.view(-1, 1) * (qd * Yd + td)
    # |terms| with |Y| replaced by its parts
    parts = cs["Q"].view(b * n, C)[dst].double().abs()
    o = None
    if cs["has_xyz"]:
        o = (cs["xyz"].view(b * n, 3)[dst] - cs["new_xyz"].view(b * m, 3)[grp]).double()     # fp32 subtraction, as the kernels
        parts = parts + o.abs() @ cs["Wxyz"].double().abs()
    if cs["bias"] is not None:
        parts = parts + cs["bias"].double().abs()
    T = pd.abs() * Gd.abs() + wt.view(-1, 1) * (qd.abs() * parts + td.abs())
    ref = {"dQ": torch.zeros(b * n, C, dtype=torch.float64, device=DEV).index_add_(0, dst, d),
           "dbias": d.sum(0)}
    mag = {"dQ": torch.zeros(b * n, C, dtype=torch.float64, device=DEV).index_add_(0, dst, T),
           "dbias": T.sum(0)}
    if o is not None:
        ref["dWxyz"] = o.t() @ d
        mag["dWxyz"] = o.abs().t() @ T
    L = torch.bincount(dst, minlength=b * n).double().view(-1, 1)
    return ref, mag, L


def partial_depth(cs, ch):
    chunks = cs["b"] * ((cs["m"] * cs["S"] + ch - 1) // ch)
    return -(-chunks // (768 * 4)) * 4 * ch + 1024


def check(out, ref, mag, L, what):
    out = out.double()
    assert torch.isfinite(out).all(), "%s: non-finite output" % what
    err = (out - ref).abs()
    lim = C_BOUND * (L + 8) * U * mag + 1e-30
    worst = (err / lim).max().item()
    print("%s: worst err/bound %.3g, max |err| %.3g" % (what, worst, err.max().item()))
    bad = err > lim
    assert not bad.any(), "%s: %d elements outside the bound, worst err/bound %.3g at %s" % (
        what, int(bad.sum()), worst, tuple(torch.nonzero(bad)[0].tolist()))


def run_scatter(cs, qform):
    b, n, m, S, C = cs["b"], cs["n"], cs["m"], cs["S"], cs["C"]
    lib = _lib.load()
    dQ = torch.full((b, n, C), float("nan"), device=DEV)
    dW = torch.full((3, C), float("nan"), device=DEV) if cs["has_xyz"] else None
    db = torch.full((C,), float("nan"), device=DEV)
    wpart = torch.empty(lib.pcops_sa_scatter_rows(b, m) * 4 * C, device=DEV)
    wsp = torch.empty(int(lib.pcops_sa_scatter_workspace_bytes(b, n, m, S)) // 4, dtype=torch.int32, device=DEV)
    hx = cs["has_xyz"]
    prev = _lib.set_option(_lib.OPT_SCATTER_QFORM, qform)
    try:
        _lib.call("pcops_sa_scatter_bwd_rows", b, n, m, S, C, cs["G"].data_ptr(), cs["Y"].data_ptr(), cs["p"].data_ptr(),
                  cs["q"].data_ptr(), cs["t"].data_ptr(), None, None, None, None, cs["idx"].data_ptr(),
                  _p(cs["xyz"] if hx else None), _p(cs["new_xyz"] if hx else None), dQ.data_ptr(), None, wpart.data_ptr(),
                  _p(dW), db.data_ptr(), cs["Q"].data_ptr(), None, _p(cs["Wxyz"]), _p(cs["bias"]), wsp.data_ptr(),
                  cs["rows"].ref if cs["rows"] is not None else None)
        took = plan()
    finally:
        _lib.set_option(_lib.OPT_SCATTER_QFORM, prev)
    torch.cuda.synchronize()
    return dQ, dW, db, took


#        name                 b    n    m    S    C  compact xyz   bias  special
CASES = [
    ("bench_compacted",     256, 512, 128,  64, 128, True,  True,  False, False),
    ("bench_uncompacted",   256, 512, 128,  64, 128, False, True,  False, False),
    ("bench_special",       256, 512, 128,  64, 128, True,  True,  True,  True),
    ("ragged_compacted",      3,  70,   9,  16,  64, True,  True,  True,  True),
    ("ragged_uncompacted",    3,  70,   9,  16,  64, False, True,  True,  True),
    ("c32_small",             4, 300,  40,  32,  32, True,  True,  True,  True),
    ("c256_small",            4, 300,  40,  32, 256, True,  True,  True,  True),
    ("c32_chunks64",         64, 256,  64,  64,  32, True,  True,  True,  True),
    ("c64_chunks64",         64, 256,  64,  64,  64, False, True,  True,  True),
    ("c256_chunks64",        64, 256,  64,  64, 256, True,  True,  False, True),
    ("c512_blocks_of_256",    2, 100,  12,  16, 512, True,  True,  True,  True),
    ("no_xyz_compacted",      4, 300,  40,  32, 128, True,  False, True,  True),
    ("no_xyz_uncompacted",    4, 300,  40,  32, 128, False, False, False, True),
    ("no_xyz_chunks64",      64, 256,  64,  64, 128, True,  False, True,  True),
]


@pytest.mark.parametrize("qform", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_scatter_against_float64(case, qform):
    name, b, n, m, S, C, compact, has_xyz, has_bias, special = case
    cs = make_case(b, n, m, S, C, compact, has_xyz, has_bias, special)
    ref, mag, L = reference(cs)
    dQ, dW, db, took = run_scatter(cs, qform)
    ch = 16 if b * ((m * S + 63) // 64) < 4096 else 64
    assert took == (8, qform, ch, 0, 4 if compact else 0), "the switch did not select the form under test: %s" % (took,)
    what = "%s qform=%d" % (name, qform)
    check(dQ.view(b * n, C), ref["dQ"], mag["dQ"], L, what + " dQ")
    Lw = partial_depth(cs, ch)
    check(db, ref["dbias"], mag["dbias"], Lw, what + " dbias")
    if has_xyz:
        check(dW, ref["dWxyz"], mag["dWxyz"], Lw, what + " dWxyz")
    if special:
        assert L.view(b, n)[0].max().item() == (L.view(b, n)[0].sum().item())       # cloud 0: one point owns every row
        assert (L.view(b, n)[:, n - 1] == 0).all()
        last = dQ[:, n - 1]
        assert (last == 0).all() and not torch.signbit(last).any(), "%s: a point no row names must get exact zeros" % what


def test_deterministic_mode_keeps_the_owner_walk():
    """the Q form is an atomic walk: deterministic mode must not take it, whatever the switch says"""
    lib = _lib.load()
    cs = make_case(3, 70, 9, 16, 64, True, True, True, True)
    ref, mag, L = reference(cs)
    lib.pcops_set_deterministic(1)
    try:
        dQ, dW, db, took = run_scatter(cs, 1)
        dQ2, dW2, db2, _ = run_scatter(cs, 1)
    finally:
        lib.pcops_set_deterministic(0)
    assert took[0] == 9, took
    assert torch.equal(dQ, dQ2) and torch.equal(dW, dW2) and torch.equal(db, db2)
    check(dQ.view(-1, 64), ref["dQ"], mag["dQ"], L, "owner walk dQ")
