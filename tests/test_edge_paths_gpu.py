"""Every dispatch branch of the EdgeConv family (csrc/edgeconv.hip and its launchers at the end of csrc/gather.hip) held to
the float64 definitions of tests/edge_ref.py element by element, with the branch each case ran read back from the
library (pcops_last_launch_plan, path codes 10..13 of include/pcops.h).

The shape table is written from the launchers' predicates, not from the models' shapes: c < 64, m % 64 != 0 and s > 128
(generic forward), n on both sides of 2528 (LDS-resident slice / 64-group chunks over L2), s % 4 == 0 && s <= 20 against
everything else (prefetched / in-line indices), s on both sides of 20 (groups summed in one run / in blocks of 16), m > 256 (the one-group-ahead prefetch and its tail), m << ceil(log2 s) on
both sides of 65536 (inverse index staged as 16-bit codes or not), the LDS walk's byte budget, 2 m s < n, n > 2560 (global
atomics), deterministic mode (ordered owner pair), every lanes-per-row instance of the generic owner walk.  Four graphs
at every shape class (tests/edge_checks.make_graph): a kNN graph, a hub (one list of length >= m, half the points in
nobody's list), repeated neighbours with quantised features (ties: the FIRST slot must win) and idx[g, s] = g.  gamma has
mixed signs inside a float4, whole all-non-negative slices (both forward specialisations run in one call), one -0.0 and
one 0.0.  Statistics: with a pivot, without (NULL), not requested (stats_partial NULL, the eval call), and Q, Ctr with a
common offset of 1e3 and a pivot near 2e3 -- the cancellation the shifted moments exist for.

Memory contract of every case: outputs prefilled with NaN (0xFF for arg), guard bands on both sides of every output and
of the workspace bit-identical afterwards, rows of stats_partial beyond pcops_edge_pool_fwd_stats_rows() untouched; the
strided forms write dQ and dCtr into the two column halves of ONE (b, n, 2 c) buffer.

Bounds (tests/edge_checks.py): selections and single fp32 operations (arg, qsel, ysel, Y, edge rows, the weight maps) are
bit-exact; out of pcops_edge_pool_out* is one fmaf and a max, at most 1 ulp from the float64 value rounded once; every sum
is held to |out - ref| <= 2 (L + 4) 2^-24 A per element, L the number of terms and A the sum of the magnitudes of the
terms the header's formulas add (edge_ref returns both), beside a relative-RMS bar of 1e-6.  tests/test_edge_ref_cpu.py
shows on the CPU that an fp32 evaluation in another order stays inside these bounds on the same input kinds.
pcops_edge_first_layer_grads sums in double: with P1 + P2 <= 4096 partial rows and 16 further operations its double
arithmetic is within 4112 * 2^-53 < 2^-40 of the magnitude sum, and the one rounding of the result to fp32 adds at most
2^-24 |dW|: the bound is 2^-24 |ref| + 2^-40 A against the float64 map of the SAME fp32 partial rows.

Not reached here: the non-temporal store of ec_fwd_kernel<1> needs an output of 256 MB and more; it stays covered only by
test_tnet_edgeconv_stack_at_bench_size.  The opt-in one-walk backward (PCOPS_EDGECONV_BWD_FUSED=1, read once per process)
runs in a fresh child process.
"""
import ctypes
import os
import subprocess
import sys
import zlib

import pytest
import torch

import edge_checks as K
import edge_ref as R
from scanobjectnn_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = torch.float64
OK, BAD_SHAPE, UNSUPPORTED = 0, -2, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OBSERVED = set()          # the plan as reported; [2] of the forward paths (rows of statistics) is checked per case and left 0


def plan():
    out = (ctypes.c_int * 5)()
    assert _lib.load().pcops_last_launch_plan(out, 5) == 5
    return tuple(out)


def stream():
    return torch.cuda.current_stream().cuda_stream


def P(t):
    return t.data_ptr() if t is not None else None


def gen(*key):
    """a generator seeded by the case itself, so every case is the same run after run and alone"""
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(key).encode()))


def inputs(kind, b, n, m, s, c, ld, offset=0.0):
    """idx, Q, Ctr (views of one (b, n, 2 c) buffer when ld, dense copies otherwise), their row strides, gamma"""
    g = gen(kind, b, n, m, s, c)
    idx = K.make_graph(kind, b, n, m, s, g)
    QC = K.make_features(kind, b, n, m, c, g, offset=offset)
    if ld:
        assert n == m
        Q, Ctr, ldq = QC[..., :c], QC[..., c:], 2 * c
    else:
        Q, Ctr, ldq = QC[:, :n, :c].contiguous(), QC[:, :m, c:].contiguous(), c
    return g, idx, Q, Ctr, ldq, K.make_gamma(c, g)


def vec(g, c):
    return torch.randn(c, generator=g, device=DEV)


# ---------------------------------------------------------------------------------------------------------------- forward
STATS_MODES = ("pivot", "nopivot", "none", "offset")

# (branch [1], n, m, s, c, b, ld)
FWD_SHAPES = [
    (0, 50, 37, 5, 32, 2, False), (0, 40, 40, 3, 4, 2, False), (0, 64, 64, 129, 64, 2, False), (0, 70, 70, 6, 128, 2, False),
    (2, 128, 128, 20, 64, 2, False), (2, 320, 320, 8, 128, 2, False), (2, 100, 64, 4, 64, 2, False),
    (2, 64, 64, 1, 64, 2, False), (2, 64, 64, 7, 64, 2, False), (2, 64, 64, 21, 64, 2, False), (2, 64, 64, 24, 64, 2, False),
    (2, 64, 64, 128, 64, 2, False),
    (1, 2560, 64, 8, 64, 2, False), (1, 2560, 64, 7, 64, 2, False),
    (1, 2560, 64, 4, 128, 1, False),          # c = 128: a wave of ec_fwd_kernel is a 64-channel slice; the second is all >= 0
    (1, 2560, 64, 128, 64, 1, False),         # more than 20 neighbours on the chunk kernel: its blocked instance
    (2, 128, 128, 20, 64, 2, True), (1, 2560, 2560, 4, 64, 2, True),
    (2, 128, 128, 24, 64, 2, True), (1, 2560, 2560, 24, 64, 1, True),        # ... and the blocked instances, strided
]
FWD_CASES = [(sh, kind, STATS_MODES[(i + j) % 4]) for i, sh in enumerate(FWD_SHAPES) for j, kind in enumerate(K.KINDS)]


def _fwd_id(case):
    (k, n, m, s, c, b, ld), kind, mode = case
    return "%s%d_n%d_m%d_s%d_c%d-%s-%s" % ("ld" if ld else "k", k, n, m, s, c, kind, mode)


@pytest.mark.parametrize("case", FWD_CASES, ids=_fwd_id)
def test_pool_fwd(case):
    (kern, n, m, s, c, b, ld), kind, mode = case
    lib = _lib.load()
    off = 1e3 if mode == "offset" else 0.0
    g, idx, Q, Ctr, ldq, gamma = inputs(kind, b, n, m, s, c, ld, offset=off)
    pivot = None
    if mode in ("pivot", "offset"):
        pivot = 2 * off + 0.1 * vec(g, c)
    want_stats = mode != "none"
    rows = lib.pcops_edge_pool_fwd_stats_rows(b, n, m, s, c)
    assert 1 <= rows <= lib.pcops_edge_pool_stats_rows(b * m)
    SQ, qsel, arg = K.Out((b, m, c)), K.Out((b, m, c)), K.Out((b, m, c), dtype=torch.uint8)
    part = K.Out((lib.pcops_edge_pool_stats_rows(b * m) + 2, 2, c)) if want_stats else None
    if ld:
        rc = lib.pcops_edge_pool_fwd_ld(b, n, m, s, c, P(Q), ldq, P(Ctr), ldq, P(idx), P(gamma), SQ.ptr(), qsel.ptr(), arg.ptr(),
                                        part.ptr() if part else None, P(pivot), stream())
    else:
        rc = lib.pcops_edge_pool_fwd(b, n, m, s, c, P(Q), P(Ctr), P(idx), P(gamma), SQ.ptr(), qsel.ptr(), arg.ptr(),
                                     part.ptr() if part else None, P(pivot), stream())
    pl = plan()
    torch.cuda.synchronize()
    assert rc == OK
    blocked = 1 if kern != 0 and s > 20 else 0      # groups of more than 20: the instances that sum in blocks of 16
    assert pl == (10, kern, rows if want_stats else 0, blocked, 1 if ld else 0), pl
    OBSERVED.add((10, kern, 0, blocked, pl[4]))
    for o in (SQ, qsel, arg) + ((part,) if part else ()):
        assert o.guards_intact()
    ref = R.pool_fwd(Q, Ctr, idx, gamma, pivot, relative=want_stats)
    assert torch.equal(arg.t, ref["arg"]), "arg: %d differ" % int((arg.t != ref["arg"]).sum())
    assert K.bits_equal(qsel.t, ref["qsel"].float()) and torch.equal(qsel.t.double(), ref["qsel"])
    bi = torch.arange(b, device=DEV).view(b, 1, 1)
    picked = idx.long().gather(2, arg.t.long())                          # (b, m, c): the row each channel selected
    assert K.bits_equal(qsel.t, Q[bi, picked, torch.arange(c, device=DEV).view(1, 1, c)])
    K.check_sum(SQ.t, ref["SQ"], "SQ")
    if want_stats:
        assert K.bits_equal(part.t[rows:], part.initial()[rows:]), \
            "rows of stats_partial beyond the %d the query announces were written" % rows
        red = part.t[:rows].double().sum(0)
        K.check_sum(red[0], ref["s1"], "sum y'")
        K.check_sum(red[1], ref["s2"], "sum y'^2")


def test_pool_fwd_refusals():
    lib = _lib.load()
    g, idx, Q, Ctr, ldq, gamma = inputs("knn", 2, 64, 64, 4, 12, False)
    SQ, qsel, arg = K.Out((2, 64, 12)), K.Out((2, 64, 12)), K.Out((2, 64, 12), dtype=torch.uint8)
    rc = lib.pcops_edge_pool_fwd(2, 64, 64, 4, 12, P(Q), P(Ctr), P(idx), P(gamma), SQ.ptr(), qsel.ptr(), arg.ptr(), None, None,
                                 stream())
    torch.cuda.synchronize()
    assert rc == BAD_SHAPE                                               # 256 % (c / 4) != 0
    assert SQ.untouched() and qsel.untouched() and arg.untouched()


# -------------------------------------------------------------------------------------------------------------- pool_out
@pytest.mark.parametrize("c", [4, 64])
@pytest.mark.parametrize("form", ["dense", "ld", "ld2", "ld2_no_ysel"])
def test_pool_out(form, c):
    lib = _lib.load()
    G, ld2 = 300, 320
    g = gen("out", c)
    qs = torch.randn(G, c, generator=g, device=DEV)
    QC = torch.randn(G, 2 * c, generator=g, device=DEV)
    sc, sh = vec(g, c), vec(g, c)
    sc[c // 2] = 0.0
    out, ysel, out2 = K.Out((G, c)), K.Out((G, c)), K.Out((G, ld2))
    if form == "dense":
        Ctr = QC[:, c:].contiguous()
        rc = lib.pcops_edge_pool_out(G, c, P(qs), P(Ctr), P(sc), P(sh), out.ptr(), ysel.ptr(), stream())
    else:
        Ctr = QC[:, c:]
        ys = None if form == "ld2_no_ysel" else ysel.ptr()
        if form == "ld":
            rc = lib.pcops_edge_pool_out_ld(G, c, P(qs), P(Ctr), 2 * c, P(sc), P(sh), out.ptr(), ys, stream())
        else:
            rc = lib.pcops_edge_pool_out_ld2(G, c, P(qs), P(Ctr), 2 * c, P(sc), P(sh), out.ptr(), ys, out2.ptr() + 4 * 16,
                                             ld2, stream())
    torch.cuda.synchronize()
    assert rc == OK
    assert out.guards_intact() and ysel.guards_intact() and out2.guards_intact()
    want, want_ysel = R.pool_out(qs, Ctr, sc, sh)
    K.check_one_ulp(out.t, want, "out")
    if form == "ld2_no_ysel":
        assert ysel.untouched()
    else:
        assert K.bits_equal(ysel.t, want_ysel)
    if form.startswith("ld2"):
        # the layer's column block [16, 16 + c) of the wider tensor, nothing else of it
        assert K.bits_equal(out2.t[:, 16:16 + c], out.t)
        before = out2.initial()
        assert K.bits_equal(out2.t[:, :16], before[:, :16]) and K.bits_equal(out2.t[:, 16 + c:], before[:, 16 + c:])
    else:
        assert out2.untouched()


# --------------------------------------------------------------------------------------------------------------- backward
def _bwd_inputs(kind, b, n, m, s, c, ld):
    g, idx, Q, Ctr, ldq, gamma = inputs(kind, b, n, m, s, c, ld)
    f = R.pool_fwd(Q, Ctr, idx, gamma, relative=False)
    sc, sh = vec(g, c), vec(g, c)
    _, ysel = R.pool_out(f["qsel"].float(), Ctr, sc, sh)
    SQ = f["SQ"][0].float()
    gpool = torch.randn(b, m, c, generator=g, device=DEV)
    p, q, t = vec(g, c), vec(g, c), vec(g, c)
    return idx, Q, Ctr, ldq, gpool, ysel, SQ, f["arg"].contiguous(), sc, sh, p, q, t


def _workspace(b, n, m, s):
    nbytes = int(_lib.load().pcops_sa_scatter_workspace_bytes(b, n, m, s))
    return K.Out(((nbytes + 3) // 4,), dtype=torch.int32)


def _run_pool_bwd(kind, b, n, m, s, c, ld, report=None):
    lib = _lib.load()
    idx, Q, Ctr, ldq, gpool, ysel, SQ, arg, sc, sh, p, q, t = _bwd_inputs(kind, b, n, m, s, c, ld)
    wsp = _workspace(b, n, m, s)
    if ld:
        both = K.Out((b, n, 2 * c))
        rc = lib.pcops_edge_pool_bwd_ld(b, n, m, s, c, P(Q), ldq, P(Ctr), ldq, P(idx), P(gpool), P(ysel), P(SQ), P(arg), P(sc),
                                        P(sh), P(p), P(q), P(t), both.ptr(), 2 * c, both.ptr() + 4 * c, 2 * c, wsp.ptr(), stream())
        outs, dQ, dCtr = (both,), both.t[..., :c], both.t[..., c:]
    else:
        oq, oc = K.Out((b, n, c)), K.Out((b, m, c))
        rc = lib.pcops_edge_pool_bwd(b, n, m, s, c, P(Q), P(Ctr), P(idx), P(gpool), P(ysel), P(SQ), P(arg), P(sc), P(sh), P(p),
                                     P(q), P(t), oq.ptr(), oc.ptr(), wsp.ptr(), stream())
        outs, dQ, dCtr = (oq, oc), oq.t, oc.t
    pl = plan()
    torch.cuda.synchronize()
    assert rc == OK
    for o in outs + (wsp,):
        assert o.guards_intact()
    ref = R.pool_bwd(Q, Ctr, idx, gpool, ysel, SQ, arg, sc, sh, p, q, t)
    K.check_sum(dCtr, ref["dCtr"], "dCtr", report=report)
    K.check_sum(dQ, ref["dQ"], "dQ", report=report)
    return pl


# (plan [1], walk, staged, n, m, s, c, b, ld, deterministic)
BWD_SHAPES = [
    (3, 2, 1, 128, 128, 20, 64, 2, False, False), (3, 2, 1, 192, 192, 5, 128, 2, False, False),
    (3, 1, 1, 2048, 2048, 32, 64, 1, False, False),
    (3, 1, 0, 2112, 2112, 20, 64, 1, False, False),
    (1, 0, 0, 100, 100, 5, 32, 2, False, False), (1, 0, 0, 100, 100, 5, 64, 2, False, False),
    (1, 0, 0, 100, 100, 5, 128, 2, False, False), (1, 0, 0, 100, 100, 5, 256, 2, False, False),
    (1, 0, 0, 100, 100, 5, 512, 2, False, False), (1, 0, 0, 2560, 64, 4, 64, 2, False, False),
    (2, 0, 0, 100, 100, 5, 64, 2, False, True), (2, 0, 0, 2624, 40, 3, 64, 2, False, True),
    (0, 0, 0, 2624, 40, 3, 32, 2, False, False), (0, 0, 0, 2624, 40, 3, 256, 2, False, False),
    (3, 2, 1, 128, 128, 20, 64, 2, True, False), (3, 1, 0, 2112, 2112, 20, 64, 1, True, False),
]
BWD_CASES = [(sh, kind) for sh in BWD_SHAPES for kind in K.KINDS]


def _bwd_id(case):
    (k, walk, staged, n, m, s, c, b, ld, det), kind = case
    return "%s%d%d%d_n%d_m%d_s%d_c%d%s-%s" % ("ld" if ld else "k", k, walk, staged, n, m, s, c, "_det" if det else "", kind)


@pytest.mark.parametrize("case", BWD_CASES, ids=_bwd_id)
def test_pool_bwd(case):
    (k, walk, staged, n, m, s, c, b, ld, det), kind = case
    was = _lib.deterministic()
    if det:
        _lib.set_deterministic(True)
    try:
        pl = _run_pool_bwd(kind, b, n, m, s, c, ld)
    finally:
        _lib.set_deterministic(was)
    assert pl == (11, k, walk, staged, 1 if ld else 0), pl
    OBSERVED.add(pl)


def test_pool_bwd_without_groups_and_refusals():
    lib = _lib.load()
    idx, Q, Ctr, ldq, gpool, ysel, SQ, arg, sc, sh, p, q, t = _bwd_inputs("knn", 2, 64, 64, 4, 64, False)
    oq, oc, wsp = K.Out((2, 64, 64)), K.Out((2, 64, 64)), _workspace(2, 64, 64, 4)
    args = (P(Q), P(Ctr), P(idx), P(gpool), P(ysel), P(SQ), P(arg), P(sc), P(sh), P(p), P(q), P(t), oq.ptr(), oc.ptr(), wsp.ptr())
    rc = lib.pcops_edge_pool_bwd(0, 64, 64, 4, 64, *args, stream())      # G = 0: nothing to do, nothing written
    torch.cuda.synchronize()
    assert rc == OK and oq.untouched() and oc.untouched() and wsp.untouched()
    rc = lib.pcops_edge_pool_bwd(2, 64, 64, 4, 48, *args, stream())      # c = 48: no owner-walk instance
    torch.cuda.synchronize()
    assert rc == BAD_SHAPE and oq.untouched() and oc.untouched() and wsp.untouched()


def test_ld_forms_refuse_partial_chunks_and_deterministic_mode():
    """m % 64 != 0: every [Q | Ctr] entry point answers PCOPS_ERR_UNSUPPORTED and writes nothing; the query answers 0 in
    deterministic mode for a shape it otherwise takes"""
    lib = _lib.load()
    b, n, s, c = 2, 100, 4, 64
    idx, Q, Ctr, ldq, gpool, ysel, SQ, arg, sc, sh, p, q, t = _bwd_inputs("knn", b, n, n, s, c, True)
    gamma = K.make_gamma(c, gen("refuse"))
    assert lib.pcops_edge_ld_supported(b, n, n, s, c) == 0
    o1, o2, oa = K.Out((b, n, c)), K.Out((b, n, c)), K.Out((b, n, c), dtype=torch.uint8)
    part, both, wsp, Y = K.Out((8, 2, c)), K.Out((b, n, 2 * c)), _workspace(b, n, n, s), K.Out((b, n, s, c))
    G = torch.randn(b, n, s, c, device=DEV, generator=gen("refuse", 1))
    rcs = [
        lib.pcops_edge_pool_fwd_ld(b, n, n, s, c, P(Q), ldq, P(Ctr), ldq, P(idx), P(gamma), o1.ptr(), o2.ptr(), oa.ptr(), part.ptr(),
                                   None, stream()),
        lib.pcops_edge_pool_bwd_ld(b, n, n, s, c, P(Q), ldq, P(Ctr), ldq, P(idx), P(gpool), P(ysel), P(SQ), P(arg), P(sc), P(sh),
                                   P(p), P(q), P(t), both.ptr(), 2 * c, both.ptr() + 4 * c, 2 * c, wsp.ptr(), stream()),
        lib.pcops_sa_gather_fwd_ld(b, n, n, s, c, P(Q), ldq, P(Ctr), ldq, P(idx), Y.ptr(), part.ptr(), None, stream()),
        lib.pcops_sa_scatter_bwd_ld(b, n, n, s, c, P(G), P(p), P(q), P(t), P(idx), P(Q), ldq, P(Ctr), ldq, both.ptr(), 2 * c,
                                    both.ptr() + 4 * c, 2 * c, wsp.ptr(), stream()),
    ]
    torch.cuda.synchronize()
    assert rcs == [UNSUPPORTED] * 4
    for o in (o1, o2, oa, part, both, wsp, Y):
        assert o.untouched()
    assert lib.pcops_edge_ld_supported(2, 128, 128, 20, 64) == 1
    was = _lib.deterministic()
    _lib.set_deterministic(True)
    try:
        assert lib.pcops_edge_ld_supported(2, 128, 128, 20, 64) == 0
    finally:
        _lib.set_deterministic(was)
    assert lib.pcops_edge_ld_supported(2, 128, 128, 20, 64) == 1


# ------------------------------------------------------------------------------- the stored first layer of a gather stack
TNET_SHAPES = [(128, 128, 20, 64), (64, 64, 7, 128)]


@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("shape", TNET_SHAPES, ids=lambda sh: "n%d_m%d_s%d_c%d" % sh)
def test_sa_gather_fwd_ld(shape, kind):
    n, m, s, c = shape
    b = 2
    lib = _lib.load()
    g, idx, Q, Ctr, ldq, _ = inputs(kind, b, n, m, s, c, True)
    mode = STATS_MODES[K.KINDS.index(kind) % 3]
    pivot = 0.1 * vec(g, c) if mode == "pivot" else None
    rows = lib.pcops_sa_gather_fwd_stats_rows(b, n, m, s, c, 1, 1, 0, 0)
    Y = K.Out((b, m, s, c))
    part = K.Out((rows + 2, 2, c)) if mode != "none" else None
    rc = lib.pcops_sa_gather_fwd_ld(b, n, m, s, c, P(Q), ldq, P(Ctr), ldq, P(idx), Y.ptr(), part.ptr() if part else None,
                                    P(pivot), stream())
    pl = plan()
    torch.cuda.synchronize()
    assert rc == OK
    assert pl == (12, 0, rows if part else 0, 0, 1), pl
    OBSERVED.add((12, 0, 0, 0, 1))
    assert Y.guards_intact() and (part is None or part.guards_intact())
    ref = R.tnet_fwd(Q, Ctr, idx, pivot)
    assert K.bits_equal(Y.t, ref["Y"])
    if part:
        assert K.bits_equal(part.t[rows:], part.initial()[rows:])
        red = part.t[:rows].double().sum(0)
        K.check_sum(red[0], ref["s1"], "sum y'")
        K.check_sum(red[1], ref["s2"], "sum y'^2")


@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("shape", TNET_SHAPES, ids=lambda sh: "n%d_m%d_s%d_c%d" % sh)
def test_sa_scatter_bwd_ld(shape, kind):
    n, m, s, c = shape
    b = 2
    lib = _lib.load()
    g, idx, Q, Ctr, ldq, _ = inputs(kind, b, n, m, s, c, True)
    G = torch.randn(b, m, s, c, generator=g, device=DEV)
    G[:, :, 1::3] = 0.0                                                  # masked rows, as behind a ReLU
    p, q, t = vec(g, c), vec(g, c), vec(g, c)
    both, wsp = K.Out((b, n, 2 * c)), _workspace(b, n, m, s)
    rc = lib.pcops_sa_scatter_bwd_ld(b, n, m, s, c, P(G), P(p), P(q), P(t), P(idx), P(Q), ldq, P(Ctr), ldq, both.ptr(), 2 * c,
                                     both.ptr() + 4 * c, 2 * c, wsp.ptr(), stream())
    pl = plan()
    torch.cuda.synchronize()
    assert rc == OK
    assert pl == (13, 0, 1, 1, 1), pl
    OBSERVED.add(pl)
    assert both.guards_intact() and wsp.guards_intact()
    ref = R.tnet_bwd(G, p, q, t, idx, Q, Ctr)
    K.check_sum(both.t[..., c:], ref["dCtr"], "dCtr")
    K.check_sum(both.t[..., :c], ref["dQ"], "dQ")


# --------------------------------------------------------------------------------- the first layer without a scatter
@pytest.mark.parametrize("with_rows", [False, True], ids=["no_rows", "edge_rows"])
@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("c", [64, 128])
def test_edge_first_layer(c, kind, with_rows):
    lib = _lib.load()
    b, n, s = 2, 64, 20                                                  # 2560 rows: not a multiple of the 2048-workgroup grid
    g = gen("first", c, kind)
    idx = K.make_graph(kind, b, n, n, s, g)
    xyz = torch.rand(b, n, 3, generator=g, device=DEV)
    rows = b * n * s
    Gm = torch.randn(rows, c, generator=g, device=DEV)
    Gm[1::3] = 0.0
    W, bias = torch.randn(6, c, generator=g, device=DEV), (vec(g, c) if with_rows else None)
    p, q, t, sumG, mean = (vec(g, c) for _ in range(5))
    assert lib.pcops_edge_first_supported(b, n, n, s, c) == 1
    PR = lib.pcops_edge_first_rows()
    mpart, wpart = K.Out((PR, 27)), K.Out((PR, 6, c))
    e8 = K.Out((rows, 8)) if with_rows else None
    dW, db = K.Out((6, c)), K.Out((c,))
    rc = [lib.pcops_edge_first_moments(b, n, n, s, P(xyz), P(idx), mpart.ptr(), e8.ptr() if e8 else None, stream()),
          lib.pcops_edge_first_wgrad(b, n, n, s, c, P(Gm), P(xyz), P(idx), wpart.ptr(), stream()),
          lib.pcops_edge_first_layer_grads(PR, wpart.ptr(), PR, mpart.ptr(), c, P(W), P(bias), P(p), P(q), P(t), P(sumG), P(mean),
                                           rows, dW.ptr(), db.ptr() if with_rows else None, stream())]
    torch.cuda.synchronize()
    assert rc == [OK, OK, OK]
    for o in (mpart, wpart, dW, db) + ((e8,) if e8 else ()):
        assert o.guards_intact()
    ref = R.first_layer(xyz, idx, Gm, W, bias, p, q, t, sumG, mean)
    if e8:
        assert K.bits_equal(e8.t[:, :6], ref["rows"].reshape(rows, 6))
        assert not e8.t[:, 6:].any()                                     # the two pad floats are zeros
    else:
        assert db.untouched()
    K.check_sum(mpart.t.double().sum(0), ref["moments"], "edge moments")
    K.check_sum(wpart.t.double().sum(0), ref["EtG"], "E^T Gm")
    # the last kernel against the float64 map of the partial rows it was given
    dW2, dW2_A, db2, db2_A = R.first_layer_from_partials(wpart.t, mpart.t, W, bias, p, q, t, sumG, mean, rows)
    assert torch.isfinite(dW.t).all()
    assert ((dW.t.double() - dW2).abs() <= K.U * dW2.abs() + 2.0 ** -40 * dW2_A).all()
    if with_rows:
        assert ((db.t.double() - db2).abs() <= K.U * db2.abs() + 2.0 ** -40 * db2_A).all()
    # and the chain against the definition: the partial sums carry the fp32 error of `rows` terms, the last step next to none
    K.check_sum(dW.t, (ref["dW"][0], ref["dW"][1], rows), "dW")
    if with_rows:
        K.check_sum(db.t, (ref["dbias"][0], ref["dbias"][1], 3), "dbias")


# ------------------------------------------------------------------------------------------------- the concatenated weight
@pytest.mark.parametrize("with_bias", [False, True], ids=["b1_null", "b1"])
@pytest.mark.parametrize("shape", [(3, 64, 8), (64, 128, 64)], ids=lambda sh: "c%d_cp%d_kp%d" % sh)
def test_edge_weights(shape, with_bias):
    c, cp, kp = shape
    lib = _lib.load()
    g = gen("weights", c, cp)
    W1 = torch.randn(2 * c, cp, generator=g, device=DEV)
    b1 = vec(g, cp) if with_bias else None
    Wcat, bcat = K.Out((kp, 2 * cp)), K.Out((2 * cp,))
    rc = lib.pcops_edge_weights_fwd(c, cp, kp, P(W1), P(b1), Wcat.ptr(), bcat.ptr(), stream())
    torch.cuda.synchronize()
    assert rc == OK and Wcat.guards_intact() and bcat.guards_intact()
    wantW, wantb = R.edge_weights_fwd(W1, b1, kp)
    assert K.bits_equal(Wcat.t, wantW) and K.bits_equal(bcat.t, wantb)
    dWcat, dbcat = torch.randn(kp, 2 * cp, generator=g, device=DEV), vec(g, 2 * cp)
    dW1, db1 = K.Out((2 * c, cp)), K.Out((cp,))
    rc = lib.pcops_edge_weights_bwd(c, cp, P(dWcat), P(dbcat), dW1.ptr(), db1.ptr() if with_bias else None, stream())
    torch.cuda.synchronize()
    assert rc == OK and dW1.guards_intact() and db1.guards_intact()
    wantdW, wantdb = R.edge_weights_bwd(dWcat, dbcat, c)
    assert K.bits_equal(dW1.t, wantdW)
    assert K.bits_equal(db1.t, wantdb) if with_bias else db1.untouched()


# ------------------------------------------------------------------------------------------- the opt-in one-walk backward
def _fused_child():
    """runs in a fresh process with PCOPS_EDGECONV_BWD_FUSED=1 (the switch is read once): ec_bwd_lds_kernel, both forms"""
    for ld in (False, True):
        for kind in K.KINDS:
            pl = _run_pool_bwd(kind, 2, 128, 128, 20, 64, ld)
            assert pl == (11, 4, 0, 1, 1 if ld else 0), pl
    print("fused child ok")


def test_one_walk_backward_in_a_child_process():
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_edge_paths_gpu as T; T._fused_child()"
            % (os.path.join(ROOT, "tests"), ROOT))
    env = dict(os.environ, PCOPS_EDGECONV_BWD_FUSED="1")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "fused child ok" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])


# ------------------------------------------------------------------------------------------------ what ran, all together
# Every variant this file is written to reach, as the library reported it (include/pcops.h, path codes 10..13).  A dispatch
# change that retires one of them, or adds one no case lists, fails here and the table is updated on purpose.
EXPECTED = {
    (10, 0, 0, 0, 0), (10, 1, 0, 0, 0), (10, 2, 0, 0, 0), (10, 1, 0, 0, 1), (10, 2, 0, 0, 1),
    (10, 1, 0, 1, 0), (10, 2, 0, 1, 0), (10, 1, 0, 1, 1), (10, 2, 0, 1, 1),
    (11, 0, 0, 0, 0), (11, 1, 0, 0, 0), (11, 2, 0, 0, 0),
    (11, 3, 2, 1, 0), (11, 3, 1, 1, 0), (11, 3, 1, 0, 0), (11, 3, 2, 1, 1), (11, 3, 1, 0, 1),
    (12, 0, 0, 0, 1), (13, 0, 1, 1, 1),
}


def test_every_listed_variant_ran():
    assert OBSERVED == EXPECTED, "missing %s, unlisted %s" % (sorted(EXPECTED - OBSERVED), sorted(OBSERVED - EXPECTED))
