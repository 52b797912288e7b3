"""Every path of the two set-abstraction launchers of csrc/gather.hip that tests/test_sa_scatter_qform_gpu.py and
tests/test_xyz_stats_moments_gpu.py leave out, plus pcops_rows_plan and pcops_cloud_bias_fwd / _bwd, held element by element to
the float64 definitions of tests/sa_ref.py (bound and conventions there).  The C ABI is called directly; every output lives in
a guarded, NaN-prefilled buffer (edge_checks.Out); after every call the guards are checked, outputs the call was not handed
must be bit-untouched, and the branch is read back from pcops_last_launch_plan (paths 8, 9, 13..16 of include/pcops.h).
No environment variables, no child processes: workspace = NULL keeps a call off the inverse-index forms,
pcops_set_deterministic selects the owner walk.

L of the reductions (sa_ref.check: |out - ref| <= 2 (L + 8) 2^-24 A):
  dQ            rows naming the point (LDS atomics, global atomics or the walk: one term per row, any order)
  dCtr          S: a wave (LDS kernel) or a workgroup's row lanes (fallback) sum the S rows of a group
  dWxyz, dbias  rows per partial + partials.  LDS kernel: a workgroup owns ceil(m / gsplit) groups of one cloud, its 1024
                lanes each sum some of those rows and are then added; b gsplit partials, added by sum_rows_kernel.
                Fallback: 16 groups per workgroup, ceil(G / 16) partials.
  Y             the terms present (Q 1, Ctr 1, xyz 3, bias 1)
  statistics, moments   rows per workgroup (groups per workgroup x S) + P partial rows
  where the kernel rebuilds Y (RC) or never reads it (path 13) the reference's Y is the float64 one and L grows by Y's terms.

Which case runs which kernel instance (sa_scatter_lds_kernel<POOLED, CS, RC>):
  <0,64,0> lds[cs64_tail-direct]  budget[*] are <0,32,0> <0,16,0> <0,8,0> again    <1,64,0> lds[cs64_tail-pooled]
  <0,32,0> lds[cs32_c32-direct]   <0,16,0> lds[cs16_c16-direct]   <0,8,0> lds[cs8_c8-direct], smallest
  <1,32,0> lds[cs32_c32-pooled]   <1,16,0> lds[cs16_c16-pooled], pooled_s256      <1,8,0> lds[cs8_c8-pooled]
  <0,CS,1> lds[*-rebuilt]         <1,CS,1> lds[*-pooled_rebuilt]   for CS = 64, 32, 16, 8 by the same four shapes
  <0,64,0> with gsplit = 3: stream_gsplit3;  as the streaming pass of the split form: split[*-direct] (<0,32,0> at C = 32),
  <1,64,0> / <1,32,0>: split[*-pooled*]
sa_scatter_bwd_kernel<false>: fallback[fallback_c8], [fallback_c512], [fallback_stream];  <true>: fallback[fallback_c16]
sa_scatter_csr_kernel<LPR, true, 16> (the Y-only walk after the pooled streaming pass): split[*-pooled], split[*-pooled_dctr]
with LPR = 8, 16, 64 at C = 32, 64, 256;  <LPR, false, 16> after the unpooled streaming pass: split[*-direct]."""
import ctypes

import pytest
import torch

import sa_ref as R
from sa_ref import Out, bits_equal
from scanobjectnn_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, NULLP, BAD_SHAPE, BAD_ARG, UNSUPPORTED = 0, -1, -2, -3, -4
REPORT = []


def plan():
    out = (ctypes.c_int * 5)()
    assert _lib.load().pcops_last_launch_plan(out, 5) == 5
    return tuple(out)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return t.data_ptr() if t is not None else None


def case(name, seed=0, C=None):
    return R.scatter_case(name, DEV, seed=seed, C=C)


# ------------------------------------------------------------------------------------------------------------- scatter
def run_scatter(cs, outs, pooled=False, Y=None, fwd=(), xyz=True, ws=False, rows=None):
    """one call of pcops_sa_scatter_bwd_rows; returns (status, outputs, plan)"""
    lib = _lib.load()
    b, n, m, S, C = cs["b"], cs["n"], cs["m"], cs["S"], cs["C"]
    o = {"dQ": Out((b * n, C)), "dCtr": Out((b * m, C)), "dWxyz": Out((3, C)), "dbias": Out((C,)),
         "wpart": Out((lib.pcops_sa_scatter_rows(b, m) * 4 * C,)),
         "ws": Out((int(lib.pcops_sa_scatter_workspace_bytes(b, n, m, S)) // 4,), dtype=torch.int32)}
    ptr = lambda k: o[k].ptr() if k in outs else None                                   # noqa: E731
    wp = o["wpart"].ptr() if ("dWxyz" in outs or "dbias" in outs) else None
    src = lambda k: _p(cs[k]) if k in fwd else None                                      # noqa: E731
    status = lib.pcops_sa_scatter_bwd_rows(
        b, n, m, S, C, None if pooled else cs["G"].data_ptr(), _p(Y), cs["p"].data_ptr(), cs["q"].data_ptr(),
        cs["t"].data_ptr(), _p(cs["gpool"]) if pooled else None, _p(cs["argmax"]) if pooled else None,
        _p(cs["psc"]) if pooled else None, _p(cs["psh"]) if pooled else None, cs["idx"].data_ptr(),
        _p(cs["xyz"]) if xyz else None, _p(cs["new_xyz"]) if xyz and xyz != "no_centres" else None,
        ptr("dQ"), ptr("dCtr"), wp, ptr("dWxyz"), ptr("dbias"), src("Q"), src("Ctr"), src("Wxyz"), src("bias"),
        o["ws"].ptr() if ws else None, rows.ref if rows is not None else None, _stream())
    took = plan()
    torch.cuda.synchronize()
    for k, v in o.items():
        assert v.guards_intact(), "%s: guard band overwritten" % k
        if k in ("dQ", "dCtr", "dWxyz", "dbias") and (k not in outs or status != OK):
            assert v.untouched(), "%s was written by a call that must not write it" % k
    if not ws:
        assert o["ws"].untouched()
    return status, o, took


def scatter_ref(cs, terms, stored, pooled, Lw, with_xyz=True):
    """(Y to hand the kernel or None, reference triples).  stored: the kernel reads the fp32 Y, which is then the reference's
    own; otherwise it rebuilds Y from `terms` and the reference is the float64 forward"""
    tab = R.row_table(cs)
    Yf = R.forward(cs, terms, tab)
    if stored:
        Y32 = Yf[0].float()
        Yd, Ay, Ly = Y32.double(), None, 0
    else:
        Y32, (Yd, Ay, Ly) = None, Yf
    if pooled:
        gm, clear = R.pooled_gm(cs, tab, Yd)
        assert clear, "the inputs put a ReLU decision of an arg-max element on the edge: choose another seed"
    else:
        gm = cs["G"].double()
    return Y32, R.backward(cs, tab, Yd, gm, Ay, Ly, with_xyz, Lw)


def check_scatter(o, ref, outs, cs, what):
    for k in outs:
        R.check(o[k].t, ref[k], "%s %s" % (what, k), report=REPORT)
    if "dQ" in outs and cs["special"]:
        b, n = cs["b"], cs["n"]
        L = ref["dQ"][2].view(b, n)
        assert (L[:, n - 1] == L.min()).all()
        last = o["dQ"].t.view(b, n, -1)[:, n - 1]
        assert (last == 0).all() and not torch.signbit(last).any(), "%s: a point no row names must get exact +0" % what


def lw_lds(cs, gsplit):
    return -(-cs["m"] // gsplit) * cs["S"] + cs["b"] * gsplit


def lw_fallback(cs):
    return 16 * cs["S"] + -(-cs["b"] * cs["m"] // 16)


ALL4 = ("dQ", "dCtr", "dWxyz", "dbias")
CS_OF = {"cs64_tail": 64, "cs32_c32": 32, "cs16_c16": 16, "cs8_c8": 8}


@pytest.mark.parametrize("form", ["direct", "pooled", "rebuilt", "pooled_rebuilt"])
@pytest.mark.parametrize("name", list(CS_OF))
def test_lds(name, form):
    """plan 14 by channel count: stored Y with fwd_Q handed over / pooled with dQ resident in LDS / Y rebuilt (RC)"""
    cs = case(name, seed=1)
    pooled, rc = form.startswith("pooled"), form.endswith("rebuilt")
    if rc:
        outs, terms, fwd = ("dCtr", "dWxyz", "dbias"), ("xyz", "bias"), ("Wxyz", "bias")
    else:
        outs, terms, fwd = ALL4, ("Q", "xyz", "bias"), ("Q",)
    Y, ref = scatter_ref(cs, terms, not rc, pooled, lw_lds(cs, 1))
    status, o, took = run_scatter(cs, outs, pooled=pooled, Y=Y, fwd=fwd)
    assert status == OK and took == (14, CS_OF[name], int(pooled), int(rc), 1), took
    check_scatter(o, ref, outs, cs, "14 lds %s %s" % (name, form))


@pytest.mark.parametrize("name,xyz,cs_want", [("budget_cs32", True, 32), ("budget_cs16", True, 16), ("budget_cs8", False, 8)])
def test_lds_slice_narrowed_by_budget(name, xyz, cs_want):
    """C = 64 but the cloud's dQ slice (+ xyz) only fits LDS at a narrower slice: several slices per cloud"""
    cs = case(name)
    Y, ref = scatter_ref(cs, ("Q",), True, False, None)
    status, o, took = run_scatter(cs, ("dQ",), Y=Y, xyz=xyz)
    assert status == OK and took == (14, cs_want, 0, 0, 1), took
    check_scatter(o, ref, ("dQ",), cs, "14 lds " + name)


def test_lds_pooled_every_argmax_byte():
    """S = 256: arg-max values 0, 127, 128, 255 in each byte lane of the packed quad"""
    cs = case("pooled_s256")
    S = cs["S"]
    cs["argmax"][0, 0:4] = torch.tensor([0, 127, 128, 255], dtype=torch.uint8, device=DEV)
    cs["argmax"][1, 4:8] = torch.tensor([255, 128, 127, 0], dtype=torch.uint8, device=DEV)
    cs["psh"][:8] = 0.25
    tab = R.row_table(cs)
    Y32 = R.forward(cs, ("Q", "bias"), tab)[0].float()
    planted = [(0, c, int(cs["argmax"][0, c])) for c in range(4)] + [(1, c, int(cs["argmax"][1, c])) for c in range(4, 8)]
    for g, c, s in planted:                                   # the planted rows pass the ReLU: their gradient must arrive
        Y32[g * S + s, c] = 2.0 * torch.sign(cs["psc"][c])
    gm, clear = R.pooled_gm(cs, tab, Y32.double())
    assert clear
    assert all(gm[g * S + s, c] == cs["gpool"][g, c].double() for g, c, s in planted)
    ref = R.backward(cs, tab, Y32.double(), gm, None, 0, False, None)
    outs = ("dQ", "dCtr")
    status, o, took = run_scatter(cs, outs, pooled=True, Y=Y32, xyz=False)
    assert status == OK and took == (14, 16, 1, 0, 1), took
    check_scatter(o, ref, outs, cs, "14 lds pooled_s256")


def test_lds_streaming_gsplit():
    """no feature gradient: a cloud's groups dealt to 3 workgroups (14 + 14 + 12), 9 clouds (a second round of 8)"""
    cs = case("stream_gsplit3")
    outs = ("dCtr", "dWxyz", "dbias")
    Y, ref = scatter_ref(cs, ("Q", "xyz", "bias"), True, False, lw_lds(cs, 3))
    status, o, took = run_scatter(cs, outs, Y=Y)
    assert status == OK and took == (14, 64, 0, 0, 3), took
    check_scatter(o, ref, outs, cs, "14 lds stream_gsplit3")


def test_lds_smallest():
    cs = case("smallest")
    Y, ref = scatter_ref(cs, ("Q", "xyz", "bias"), True, False, lw_lds(cs, 1))
    status, o, took = run_scatter(cs, ALL4, Y=Y, fwd=("Q",))
    assert status == OK and took == (14, 8, 0, 0, 1), took
    check_scatter(o, ref, ALL4, cs, "14 lds smallest")


@pytest.mark.parametrize("name,pooled,outs", [
    ("fallback_c8", False, ALL4), ("fallback_c16", True, ("dQ", "dCtr")), ("fallback_c512", False, ALL4),
    ("fallback_stream", False, ("dCtr", "dWxyz", "dbias"))])
def test_fallback(name, pooled, outs):
    """plan 15: clouds too large for an LDS slice.  Padded rows (they repeat the group's first index) leave as one atomic"""
    cs = case(name)
    assert (cs["cnt"] < cs["S"]).any()
    Y, ref = scatter_ref(cs, ("Q", "xyz", "bias"), True, pooled, lw_fallback(cs))
    status, o, took = run_scatter(cs, outs, pooled=pooled, Y=Y)
    assert status == OK and took == (15, 0, int(pooled), 0, 0), took
    check_scatter(o, ref, outs, cs, "15 fallback " + name)


@pytest.mark.parametrize("form", ["direct", "pooled", "pooled_dctr"])
@pytest.mark.parametrize("name,cs0", [("split_c32", 32), ("split_c64", 64), ("split_c256", 64)])
def test_split(name, cs0, form):
    """workspace given: LDS streaming pass (dCtr, dWxyz / dbias, pooled arg-row atomics into dQ), then the chunked walk"""
    cs = case(name, seed=2)
    pooled = form != "direct"
    outs = ("dQ",) if form == "pooled" else ALL4
    Y, ref = scatter_ref(cs, ("Q", "xyz", "bias"), True, pooled, lw_lds(cs, 1))
    status, o, took = run_scatter(cs, outs, pooled=pooled, Y=Y, ws=True)
    assert status == OK and took == (8, 0, 16, cs0, 0), took
    check_scatter(o, ref, outs, cs, "8 split %s %s" % (name, form))


def test_split_deterministic():
    lib = _lib.load()
    cs = case("split_c64", seed=2)
    Y, ref = scatter_ref(cs, ("Q", "xyz", "bias"), True, False, lw_lds(cs, 1))
    lib.pcops_set_deterministic(1)
    try:
        status, o, took = run_scatter(cs, ALL4, Y=Y, ws=True)
        status2, o2, took2 = run_scatter(cs, ALL4, Y=Y, ws=True)
        # no ordered variant of the pooled arg-row atomics: refused, nothing written
        statusp, _, _ = run_scatter(cs, ("dQ",), pooled=True, Y=Y, ws=True)
    finally:
        lib.pcops_set_deterministic(0)
    assert status == OK and status2 == OK and took == took2 == (9, 0, 0, 64, 0), (took, took2)
    assert statusp == UNSUPPORTED
    for k in ALL4:
        assert bits_equal(o[k].t, o2[k].t), "%s differs between two deterministic runs" % k
    check_scatter(o, ref, ALL4, cs, "9 owner split")


def test_q_plus_ctr_form():
    """path 13 (a shape ec_bwd_supported accepts: 64 | m, 64 | c, 2 m s >= n); deterministic mode must not take it"""
    lib = _lib.load()
    cs = case("q_plus_ctr", seed=3)
    outs = ("dQ", "dCtr")
    tab = R.row_table(cs)
    Yd, Ay, Ly = R.forward(cs, ("Q", "Ctr"), tab)
    ref = R.backward(cs, tab, Yd, cs["G"].double(), Ay, Ly, False, None)
    Y = Yd.float()
    status, o, took = run_scatter(cs, outs, Y=Y, fwd=("Q", "Ctr"), xyz=False, ws=True)
    assert status == OK and took[0] == 13 and took[4] == 0, took
    check_scatter(o, ref, outs, cs, "13 q+ctr")
    lib.pcops_set_deterministic(1)
    try:
        status, o, took = run_scatter(cs, outs, Y=Y, fwd=("Q", "Ctr"), xyz=False, ws=True)
    finally:
        lib.pcops_set_deterministic(0)
    assert status == OK and took == (9, 0, 0, 64, 0), took
    check_scatter(o, ref, outs, cs, "9 owner q+ctr")


def test_scatter_refusals():
    cs = case("split_c64")
    tab = R.row_table(cs)
    Y = R.forward(cs, ("Q",), tab)[0].float()
    rows = _lib.Rows(cs["cnt"], cs["S"])
    assert run_scatter(cs, ("dQ",), pooled=True, Y=Y, ws=True, rows=rows)[0] == UNSUPPORTED
    assert run_scatter(cs, ("dQ", "dCtr"), Y=Y, ws=True, rows=rows)[0] == UNSUPPORTED
    assert run_scatter(cs, ("dQ",), Y=Y, ws=False, rows=rows)[0] == UNSUPPORTED
    assert run_scatter(cs, ("dQ",), Y=Y, xyz="no_centres")[0] == NULLP
    c96 = case("split_c64", C=96)
    assert run_scatter(c96, ("dQ",), Y=R.forward(c96, ("Q",), R.row_table(c96))[0].float())[0] == BAD_SHAPE
    big = R.make_case(1, 10, 1, 257, 8, DEV)
    big["argmax"].clamp_(max=255)
    assert run_scatter(big, ("dQ",), pooled=True, Y=R.forward(big, ("Q",), R.row_table(big))[0].float())[0] == BAD_SHAPE


# ------------------------------------------------------------------------------------------------------------- forward
def run_gather(cs, terms, want, pivot=None, rows=None):
    lib = _lib.load()
    b, n, m, S, C = cs["b"], cs["n"], cs["m"], cs["S"], cs["C"]
    P = lib.pcops_sa_gather_stats_rows(b * m)
    o = {"Y": Out((b * m * S, C)), "off4": Out((b * m * S, 4)), "stats": Out((P, 2, C)), "moments": Out((P, 9))}
    ptr = lambda k: o[k].ptr() if k in want else None                                   # noqa: E731
    src = lambda k: _p(cs[k]) if k in terms else None                                   # noqa: E731
    hx = "xyz" in terms
    status = lib.pcops_sa_gather_fwd_rows(
        b, n, m, S, C, src("Q"), src("Ctr"), _p(cs["xyz"]) if hx else None, _p(cs["new_xyz"]) if hx else None,
        src("Wxyz") if not hx else _p(cs["Wxyz"]), src("bias"), cs["idx"].data_ptr(), ptr("Y"), ptr("off4"), ptr("stats"),
        _p(pivot), ptr("moments"), rows.ref if rows is not None else None, _stream())
    took = plan()
    torch.cuda.synchronize()
    for k, v in o.items():
        assert v.guards_intact(), "%s: guard band overwritten" % k
        if k not in want or status != OK:
            assert v.untouched(), "%s was written by a call that must not write it" % k
    return status, o, took, P


def check_gather(cs, terms, want, o, P, gpb, what, pivot=None, compact=False):
    S = cs["S"]
    tab = R.row_table(cs, compact)
    Rn = tab["R"]
    Yt = R.forward(cs, terms, tab)
    owner = tab["grp"] // gpb
    L = gpb * S + P
    if "Y" in want:
        R.check(o["Y"].t[:Rn], Yt, what + " Y", report=REPORT)
        assert bits_equal(o["Y"].t[Rn:], o["Y"].initial()[Rn:]), what + ": a dropped row was written"
    if "off4" in want:
        off = torch.cat([R.offsets(cs, tab), torch.zeros(Rn, 1, device=DEV)], 1)
        assert bits_equal(o["off4"].t[:Rn], off), what + ": off4 is not the fp32 subtraction"
        assert bits_equal(o["off4"].t[Rn:], o["off4"].initial()[Rn:]), what + ": off4 of a dropped row was written"
    if "stats" in want:
        if "Y" in want:
            st = R.stats(o["Y"].t[:Rn].double(), tab["wt"], owner, P, L, pivot)
        else:
            st = R.stats(Yt[0], tab["wt"], owner, P, L, pivot, Ay=Yt[1], Ly=Yt[2])
        R.check(o["stats"].t, st, what + " stats per partial", report=REPORT)
        R.check(o["stats"].t.double().sum(0), R.total(st), what + " stats summed", report=REPORT)
    if "moments" in want:
        mo = R.moments(R.offsets(cs, tab), tab["wt"], owner, P, L)
        R.check(o["moments"].t, mo, what + " moments per partial", report=REPORT)
        R.check(o["moments"].t.double().sum(0), R.total(mo), what + " moments summed", report=REPORT)


def near_pivot(cs, terms):
    Y = R.forward(cs, terms, R.row_table(cs))[0]
    return (Y.mean(0) + 0.1 * R.vec(cs["C"], torch.Generator(device=DEV).manual_seed(9)).double()).float()


TERM_SETS = [("Q",), ("Q", "Ctr", "xyz"), ("xyz", "bias"), ("Q", "xyz", "bias"), ("Q", "Ctr", "xyz", "bias")]


@pytest.mark.parametrize("C", [4, 64, 1024])
@pytest.mark.parametrize("terms", TERM_SETS, ids=["+".join(t) for t in TERM_SETS])
def test_gather_all_outputs(terms, C):
    cs = R.make_case(3, 70, 9, 20, C, DEV, seed=4, special=True)
    want = ("Y", "stats") + (("off4", "moments") if "xyz" in terms else ())
    pv = near_pivot(cs, terms)
    status, o, took, P = run_gather(cs, terms, want, pivot=pv)
    assert status == OK and took == (16, 1, P, 0, 0) and P == 27, took
    check_gather(cs, terms, want, o, P, 1, "16 gather %s C=%d" % ("+".join(terms), C), pivot=pv)


@pytest.mark.parametrize("want,pivot", [(("Y",), None), (("off4",), None), (("stats",), None), (("stats",), "near"),
                                        (("stats",), "far"), (("Y", "stats"), "far"), (("stats", "moments"), "near"),
                                        (("Y", "moments"), None)],
                         ids=["Y", "off4", "stats", "stats_pivot", "stats_far", "Y_stats_far", "stats_moments", "Y_moments"])
def test_gather_each_output_alone(want, pivot):
    terms = ("Q", "xyz", "bias")
    cs = R.make_case(3, 70, 9, 20, 64, DEV, seed=5, special=True)
    pv = None if pivot is None else (near_pivot(cs, terms) if pivot == "near" else torch.full((64,), 1e3, device=DEV))
    status, o, took, P = run_gather(cs, terms, want, pivot=pv)
    assert status == OK and took == (16, 1, P if "stats" in want else 0, 0, 0), took
    check_gather(cs, terms, want, o, P, 1, "16 gather alone " + "+".join(want) + " " + str(pivot), pivot=pv)


def test_gather_stays_off_the_edgeconv_kernel():
    """{Q, Ctr, xyz} at a shape the EdgeConv forward accepts ({Q, Ctr} alone goes there: path 12)"""
    terms = ("Q", "Ctr", "xyz")
    cs = R.make_case(2, 70, 64, 16, 64, DEV, seed=6)
    status, o, took, P = run_gather(cs, terms, ("Y", "stats"))
    assert status == OK and took == (16, 1, 128, 0, 0), took
    check_gather(cs, terms, ("Y", "stats"), o, P, 1, "16 gather q+ctr+xyz")
    status, o, took, P = run_gather(cs, ("Q", "Ctr"), ("Y",))
    assert status == OK and took[0] == 12, took


@pytest.mark.parametrize("shape,gpb", [((3, 70, 9, 48, 64), 1), ((2, 70, 3, 1100, 4), 1), ((2, 16, 4099, 2, 4), 8)],
                         ids=["S48", "S1100", "G8198"])
def test_gather_staging_and_groups_per_workgroup(shape, gpb):
    """21 groups per staging chunk / one group per chunk with staging sized by S / 8 groups per workgroup, the last partial"""
    terms = ("Q", "Ctr", "xyz", "bias")
    cs = R.make_case(*shape, DEV, seed=7)
    want = ("Y", "off4", "stats", "moments")
    pv = near_pivot(cs, terms)
    status, o, took, P = run_gather(cs, terms, want, pivot=pv)
    assert status == OK and took == (16, gpb, P, 0, 0) and P == -(-shape[0] * shape[2] // gpb), took
    check_gather(cs, terms, want, o, P, gpb, "16 gather %s" % (shape,), pivot=pv)


@pytest.mark.parametrize("S", [32, 64])
def test_gather_compacted(S):
    cnt = [[S, 1, 16, 17, 0, 5], [0, S, 17, 16, 1, S - 1]]
    cs = R.make_case(2, 70, 6, S, 64, DEV, seed=8, cnt=cnt)
    rows = _lib.Rows(cs["cnt"], S)
    bs, nrows, blocks = R.rows_plan(cs["cnt"], S)
    assert rows.num_rows() == nrows < 2 * 6 * S and torch.equal(rows.block_start, bs)
    terms = ("Q", "xyz", "bias")
    want = ("Y", "off4", "stats", "moments")
    pv = near_pivot(cs, terms)
    status, o, took, P = run_gather(cs, terms, want, pivot=pv, rows=rows)
    assert status == OK and took == (16, 1, P, 0, 4), took
    check_gather(cs, terms, want, o, P, 1, "16 gather compacted S=%d" % S, pivot=pv, compact=True)
    # the row-0 weights enter the sums: the compacted statistics are those of all b m S rows
    full = R.row_table(cs)
    Yf = R.forward(cs, terms, full)
    st = R.stats(Yf[0], full["wt"], full["grp"], P, S + P, pv, Ay=Yf[1], Ly=Yf[2])
    R.check(o["stats"].t, st, "16 gather compacted S=%d stats against all rows" % S, report=REPORT)


def test_gather_moments_route_plan():
    """statistics only, arithmetic first layer: with PCOPS_OPT_XYZ_STATS_MOMENTS = 1 the two sums come from the nine moments
    (tests/test_xyz_stats_moments_gpu.py holds the numbers of that route)"""
    cs = R.make_case(3, 70, 9, 20, 64, DEV, seed=4)
    status, o, took, P = run_gather(cs, ("xyz", "bias"), ("stats", "moments"))
    assert status == OK and took == (16, 1, P, 0, 0), took           # the option's default: the generic kernel
    check_gather(cs, ("xyz", "bias"), ("stats", "moments"), o, P, 1, "16 gather stats only, arithmetic layer")
    prev = _lib.set_option(_lib.OPT_XYZ_STATS_MOMENTS, 1)
    try:
        status, o, took, P = run_gather(cs, ("xyz", "bias"), ("stats", "moments"))
    finally:
        _lib.set_option(_lib.OPT_XYZ_STATS_MOMENTS, prev)
    assert status == OK and took == (16, 1, P, 1, 0), took


# ------------------------------------------------------------------------------------------------------- pcops_rows_plan
@pytest.mark.parametrize("S", [16, 64, 256])
@pytest.mark.parametrize("G", [1, 1023, 1025, 4096, 4097, 8190, 65536, 65537])
def test_rows_plan_is_the_host_model(G, S):
    lib = _lib.load()
    gen = torch.Generator(device=DEV).manual_seed(G + S)
    vals = torch.tensor([0, 1, 15, 16, 17, S - 1, S, S + 3], dtype=torch.int32, device=DEV)
    cnt = vals[torch.randint(0, 8, (G,), device=DEV, generator=gen)].contiguous()
    nmax = int(lib.pcops_rows_max_blocks(1, G, S))
    blocks, bstart, rows = Out((nmax, 4), dtype=torch.int32), Out((G + 1,), dtype=torch.int32), Out((1,), dtype=torch.int32)
    status = lib.pcops_rows_plan(1, G, S, cnt.data_ptr(), blocks.ptr(), bstart.ptr(), rows.ptr(), _stream())
    torch.cuda.synchronize()
    assert status == OK and blocks.guards_intact() and bstart.guards_intact() and rows.guards_intact()
    bs, nrows, want = R.rows_plan(cnt, S)
    assert torch.equal(bstart.t, bs) and rows.t.item() == nrows
    nb = nrows // 16
    assert torch.equal(blocks.t[:nb], want), "a RowBlock differs (g, s0, weight bits, pad)"
    assert torch.equal(blocks.t[nb:], blocks.initial()[nb:]), "blocks past the total were written"


# ------------------------------------------------------------------------------------------- pcops_cloud_bias_fwd / _bwd
def _cloud_case(rpg, groups, C, seed=0):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    rows = rpg * groups
    kw = dict(device=DEV, generator=gen)
    return dict(Q=torch.randn(rows, C, **kw), Ctr=torch.randn(groups, C, **kw), G=torch.randn(rows, C, **kw),
                p=R.vec(C, gen), q=R.vec(C, gen), t=R.vec(C, gen, lo=0.1))


@pytest.mark.parametrize("C", [4, 64, 1024])
@pytest.mark.parametrize("groups", [2, 3])
@pytest.mark.parametrize("rpg", [256, 512])
def test_cloud_bias(rpg, groups, C):
    lib = _lib.load()
    c = _cloud_case(rpg, groups, C)
    rows = rpg * groups
    P = lib.pcops_cloud_bias_rows(rows)
    assert P == rows // 256
    what = "cloud bias rpg=%d groups=%d C=%d" % (rpg, groups, C)
    for pivot in (None, (c["Q"].mean(0) + 0.1 * R.vec(C, torch.Generator(device=DEV).manual_seed(1))).contiguous()):
        ref = R.cloud_bias(c["Q"], c["Ctr"], rpg, c["G"], c["p"], c["q"], c["t"], pivot)
        Y, st = Out((rows, C)), Out((P, 2, C))
        assert lib.pcops_cloud_bias_fwd(rows, rpg, C, c["Q"].data_ptr(), c["Ctr"].data_ptr(), Y.ptr(), st.ptr(), _p(pivot),
                                        _stream()) == OK
        torch.cuda.synchronize()
        assert Y.guards_intact() and st.guards_intact()
        assert bits_equal(Y.t, ref["Y"]), what + ": Y is not the fp32 sum"
        R.check(st.t, ref["stats"], what + " stats per partial", report=REPORT)
        R.check(st.t.double().sum(0), R.total(ref["stats"]), what + " stats summed", report=REPORT)
    # without statistics: Y alone
    Y2, st2 = Out((rows, C)), Out((P, 2, C))
    assert lib.pcops_cloud_bias_fwd(rows, rpg, C, c["Q"].data_ptr(), c["Ctr"].data_ptr(), Y2.ptr(), None, None, _stream()) == OK
    torch.cuda.synchronize()
    assert bits_equal(Y2.t, ref["Y"]) and Y2.guards_intact() and st2.untouched()
    for with_dq in (True, False):
        dQ, dC, part = Out((rows, C)), Out((groups, C)), Out((P, C))
        assert lib.pcops_cloud_bias_bwd(rows, rpg, C, c["G"].data_ptr(), ref["Y"].data_ptr(), c["p"].data_ptr(),
                                        c["q"].data_ptr(), c["t"].data_ptr(), dQ.ptr() if with_dq else None, dC.ptr(),
                                        part.ptr(), _stream()) == OK
        torch.cuda.synchronize()
        assert dQ.guards_intact() and dC.guards_intact() and part.guards_intact()
        if with_dq:
            R.check(dQ.t, ref["dQ"], what + " dQ", report=REPORT)
        else:
            assert dQ.untouched()
        R.check(dC.t, ref["dCtr"], what + " dCtr", report=REPORT)


def test_cloud_bias_refusals():
    lib = _lib.load()
    for rows, rpg, C, off in [(256, 128, 64, 0), (768, 512, 64, 0), (512, 256, 96, 0), (512, 256, 64, 1)]:
        c = _cloud_case(rpg, max(rows // rpg, 1), C)
        Q = torch.randn(rows + 1, C, device=DEV).view(-1)[off:off + rows * C]
        assert Q.data_ptr() % 16 == (4 if off else 0)
        Y, st, dQ, dC, part = Out((rows, C)), Out((rows // 256 + 1, 2, C)), Out((rows, C)), Out((4, C)), Out((8, C))
        assert lib.pcops_cloud_bias_fwd(rows, rpg, C, Q.data_ptr(), c["Ctr"].data_ptr(), Y.ptr(), st.ptr(), None,
                                        _stream()) == UNSUPPORTED
        assert lib.pcops_cloud_bias_bwd(rows, rpg, C, Q.data_ptr(), Q.data_ptr(), c["p"].data_ptr(), c["q"].data_ptr(),
                                        c["t"].data_ptr(), dQ.ptr(), dC.ptr(), part.ptr(), _stream()) == UNSUPPORTED
        torch.cuda.synchronize()
        assert all(v.untouched() for v in (Y, st, dQ, dC, part))


def test_zz_report():
    """prints the worst err / bound and relative RMS per path, as recorded in DESIGN.md (run with -s)"""
    worst = {}
    for what, w, rms in REPORT:
        key = " ".join(what.split(" ")[:2])
        a, b = worst.get(key, ((0.0, ""), (0.0, "")))
        worst[key] = (max(a, (w, what)), max(b, (rms, what)))
    for key in sorted(worst):
        (w, ww), (r, rw) = worst[key]
        print("SA-PATHS %-12s worst err/bound %.3g (%s)   relative RMS %.3g (%s)" % (key, w, ww, r, rw))
    assert all(w[0] <= 1.0 for w, _ in worst.values())
