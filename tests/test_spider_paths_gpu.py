"""Every kernel path of the SpiderConv family (csrc/spider.hip) held to the float64 definitions of tests/spider_ref.py
element by element, through the C ABI (_lib.call), each entry point on the fp32 tensors it is given.

Memory contract of every case: every output (and every workspace) lies in a tests/edge_checks.Out buffer -- NaN prefill,
guard bands on both sides bit-identical afterwards -- so a store past n, O, C or K, or a slot a kernel should have written
and did not, shows.  Every case runs twice and must be bit-identical: the file promises fixed-order sums everywhere.

Bounds: every sum is held to |out - ref| <= 2 (L + 4) 2^-24 A per element (edge_checks.check_sum, constants unchanged)
beside the family's relative-RMS bar of tests/spider_checks.py; copies, NULL-argument twins and decisions are bit-exact.
tests/test_spider_ref_cpu.py shows without a GPU that a sequential fp32 evaluation stays inside these bounds on the same
inputs and that one wrong restatement per edge below falls outside them.

What each case reaches, kernel by kernel (shapes are b, n, k, C, O; T = 5):

conv_fwd_kernel -- grid (ceil(n / 64), ceil(O / 64), b)
  1, 40, 5, 3, 16        one partial row tile (rows 40..63 masked), C < 16 (13 zero channels in the K block), O = 16 (three
                         of four 16-column slices of the tile masked)
  2, 64, 1, 16, 64       whole tiles only, k = 1, C = 16 exactly (one full K block, no tail)
  3, 65, 7, 17, 48       one-row tail tile, channel tail of 1 in a second K block, O = 48
  2, 300, 20, 40, 80     ragged rows, an 8-channel tail in a third K block, a second column tile of 16 columns
  1, 130, 20, 256, 256   C = 256 (16 K blocks per neighbour), 25 601 terms per element
  1, 70, 64, 5, 32       k = 64;      1, 96, 3, 256, 512   O = 512 (eight column tiles)
  bias == NULL on every case: bit-identical to a zero bias.  b = 0: OK, output untouched.
conv_wgrad_kernel / wgrad_reduce_kernel -- grid (k ceil(C / 16), ceil(O / 64), splits); the split count is read back from
pcops_spider_conv_wgrad_workspace_bytes and asserted per case
  1, 40, 5, 3, 16        splits == 1 because b n <= 64: dw and db stored directly, no reduce launch, workspace NULL
  1, 130, 20, 256, 256   splits == 1 because the grid already has >= 1024 workgroups, over three 64-row steps
  2, 64, 1, 16, 64       2 splits of one whole tile each;   1, 70, 64, 5, 32 and 1, 96, 3, 256, 512: 2 splits, ragged second
  3, 65, 7, 17, 48       4 splits of 64 rows: the tiles straddle the cloud boundaries at rows 65 and 130 (global neighbour
                         row = (p / n) n + idx), the last split holds 3 rows
  2, 300, 20, 40, 80     9 splits, 5 hold rows: the four trailing ones must store zeros (the workspace is NaN-prefilled)
  2, 520, 4, 3, 16       the cap of 16 splits, 7 of them empty
  dbias == NULL on every case: dw bit-identical.  b = 0: dw and dbias zeroed.
conv_dgrad_kernel -- grid (ceil(n / 64), k, b): the same row, channel and column edges as the forward (O = 16: one masked
  64-column step; O = 80 and 512: two and eight steps); dfeat_grouped == NULL on every case: dg bit-identical, and per
  element in the first-layer form of the end-to-end test.  b = 0: OK, outputs untouched.
taylor_fwd_kernel / taylor_bwd_partial_kernel / taylor_bwd_final_kernel -- rows given directly
  1, 255, 256, 257       one thread; one block less one thread, exactly one block, one block and one thread
  65 536                 the capped grid of 256 x 256 exactly full, one trip each
  65 536 + 77            a ragged second trip of the grid-stride loop that only 77 threads take
  3 * 65 536 + 5         several trips
  rows = 0: forward untouched, dtheta and dtbias zeroed.  delta has rows that are exactly zero, dg a non-zero mean.
gn_fwd_kernel / gn_bwd_kernel / gn_bwd_final_kernel -- (b, n, C, groups)
  2, 70, 16, 16          cg = 1;      3, 33, 48, 16   cg = 3, nact = 255;      2, 50, 112, 16   cg = 7, nact = 252
  2, 300, 80, 16         cg = 5;      2, 40, 512, 2   cg = 256, the limit;     2, 130, 256, 16  the model's last layer
  1, 9, 16, 1            one group, n cg = 144 < 256: idle threads in both reductions
  2, 32, 32, 4           cg = 8, n cg = 256: one (cloud, group) constant -- mean exact, var = 0, rstd = 1 / sqrt(eps)
  every case: gamma of either sign, one channel with gamma = 0 and beta = 0 (output exactly 0, gy = 0 by the y > 0 rule),
  the ReLU decision read back from the output and every decision that differs from float64's held to |z| <= bound(z).
  b = 0: dgamma and dbeta zeroed.
End to end (3, 65, 7, 17, 48 and 1, 40, 5, 3, 16; with and without deterministic mode; with and without a feature
gradient): spider_ops.spider_conv forward and backward bit-identical to the entry points called one by one, each gradient
per element; dF through scatter_grouped is bit-identical in deterministic mode (the ordered owner walk) and held to the
scatter's own triple in both modes -- outside deterministic mode the scatter may add in any order.
"""
import pytest
import torch

import spider_checks as K
import spider_ref as R
from scanobjectnn_amd import _lib
from scanobjectnn_amd.spidercnn import spider_ops as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 5


def P(t):
    return t.data_ptr() if t is not None else None


def OP(o):
    return o.ptr() if o is not None else None


def _done(*outs):
    torch.cuda.synchronize()
    for o in outs:
        if o is not None:
            assert o.guards_intact()


def _ws(nbytes):
    assert nbytes % 4 == 0
    return K.Out((nbytes // 4,), device=DEV) if nbytes else None


# --------------------------------------------------------------------------------------------- the entry points, guarded
def conv_fwd(shape, feat, idx, g, w, bias):
    b, n, k, c, o = shape
    y = K.Out((max(b, 1), n, o), device=DEV)
    _lib.call("pcops_spider_conv_fwd", b, n, c, k, T, o, P(feat), P(idx), P(g), P(w), P(bias), y.ptr())
    _done(y)
    return y


def conv_wgrad(shape, feat, idx, g, dy, want_db=True):
    b, n, k, c, o = shape
    dw, db = K.Out((k * c * T, o), device=DEV), K.Out((o,), device=DEV)
    ws = _ws(_lib.load().pcops_spider_conv_wgrad_workspace_bytes(b, n, c, k, T, o))
    _lib.call("pcops_spider_conv_wgrad", b, n, c, k, T, o, P(feat), P(idx), P(g), P(dy), dw.ptr(),
              db.ptr() if want_db else None, OP(ws))
    _done(dw, db, ws)
    if not want_db:
        assert db.untouched()
    return dw, db


def conv_dgrad(shape, feat, idx, g, w, dy, want_dfg=True):
    b, n, k, c, o = shape
    dfg, dg = K.Out((max(b, 1), n, k, c), device=DEV), K.Out((max(b, 1), n, k, T), device=DEV)
    _lib.call("pcops_spider_conv_dgrad", b, n, c, k, T, o, P(feat), P(idx), P(g), P(w), P(dy),
              dfg.ptr() if want_dfg else None, dg.ptr())
    _done(dfg, dg)
    if not want_dfg:
        assert dfg.untouched()
    return dfg, dg


def taylor_fwd(rows, delta, theta, tbias):
    g = K.Out((max(rows, 1), T), device=DEV)
    _lib.call("pcops_spider_taylor_fwd", rows, T, P(delta), P(theta), P(tbias), g.ptr())
    _done(g)
    return g


def taylor_bwd(rows, delta, dg):
    dtheta, dtbias = K.Out((19, T), device=DEV), K.Out((T,), device=DEV)
    ws = _ws(_lib.load().pcops_spider_taylor_bwd_workspace_bytes(rows, T))
    _lib.call("pcops_spider_taylor_bwd", rows, T, P(delta), P(dg), dtheta.ptr(), dtbias.ptr(), OP(ws))
    _done(dtheta, dtbias, ws)
    return dtheta, dtbias


def gn_fwd(shape, x, gamma, beta):
    b, n, c, groups = shape
    y, mean, rstd = K.Out((b, n, c), device=DEV), K.Out((b, groups), device=DEV), K.Out((b, groups), device=DEV)
    _lib.call("pcops_group_norm_relu_fwd", b, n, c, groups, K.EPS, P(x), P(gamma), P(beta), y.ptr(), mean.ptr(), rstd.ptr())
    _done(y, mean, rstd)
    return y, mean, rstd


def gn_bwd(shape, dout, x, y, gamma, mean, rstd):
    b, n, c, groups = shape
    dx, dgamma, dbeta = K.Out((max(b, 1), n, c), device=DEV), K.Out((c,), device=DEV), K.Out((c,), device=DEV)
    ws = _ws(_lib.load().pcops_group_norm_relu_workspace_bytes(b, c))
    _lib.call("pcops_group_norm_relu_bwd", b, n, c, groups, P(dout), P(x), P(y), P(gamma), P(mean), P(rstd), dx.ptr(),
              dgamma.ptr(), dbeta.ptr(), OP(ws))
    _done(dx, dgamma, dbeta, ws)
    return dx, dgamma, dbeta


def _twice(fn, *args, **kw):
    """the call made twice into fresh buffers: bit-identical results, the first returned"""
    first, second = fn(*args, **kw), fn(*args, **kw)
    for a, b_ in zip(first, second) if isinstance(first, tuple) else ((first, second),):
        assert K.bits_equal(a.t, b_.t)
    return first


# ----------------------------------------------------------------------------------------------------------- contraction
@pytest.mark.parametrize("case", K.CONV_CASES, ids=K.conv_id)
def test_contraction(case):
    shape, splits, occupied = case
    b, n, k, c, o = shape
    feat, idx, g, w, bias, dy = K.conv_inputs(shape, DEV)
    nbytes = _lib.load().pcops_spider_conv_wgrad_workspace_bytes(b, n, c, k, T, o)
    per_split = (k * c * T * o + o) * 4
    assert nbytes % per_split == 0 and (nbytes // per_split if nbytes else 1) == splits
    assert -(-(b * n) // K.wgrad_chunk(b, n, splits)) == occupied
    report = []

    y = _twice(conv_fwd, shape, feat, idx, g, w, bias)
    K.check_sum(y.t, R.conv_fwd(feat, idx, g, w, bias), "y", report=report)
    y0 = conv_fwd(shape, feat, idx, g, w, None)
    assert K.bits_equal(y0.t, conv_fwd(shape, feat, idx, g, w, torch.zeros_like(bias)).t)
    K.check_sum(y0.t, R.conv_fwd(feat, idx, g, w, None), "y without bias", report=report)

    dw, db = _twice(conv_wgrad, shape, feat, idx, g, dy)
    ref = R.conv_wgrad(feat, idx, g, dy)
    K.check_sum(dw.t, ref["dw"], "dw", report=report)
    K.check_sum(db.t, ref["db"], "db", report=report)
    dw0, _ = conv_wgrad(shape, feat, idx, g, dy, want_db=False)
    assert K.bits_equal(dw0.t, dw.t)

    dfg, dg = _twice(conv_dgrad, shape, feat, idx, g, w, dy)
    ref = R.conv_dgrad(feat, idx, g, w, dy)
    K.check_sum(dfg.t, ref["dfg"], "dfg", report=report)
    K.check_sum(dg.t, ref["dg"], "dg", report=report)
    _, dg0 = conv_dgrad(shape, feat, idx, g, w, dy, want_dfg=False)
    assert K.bits_equal(dg0.t, dg.t)
    for what, worst, rms in report:
        print("%s %-16s worst err/bound %.3g  relative RMS %.3g" % (shape, what, worst, rms))


def test_no_clouds():
    """b = 0: forward and data gradient return OK and touch nothing; the weight gradient, the group-norm backward and the
    Taylor backward zero their sums"""
    shape = (0, 40, 5, 3, 16)
    feat, idx, g, w, bias, dy = K.conv_inputs((1,) + shape[1:], DEV)
    assert conv_fwd(shape, feat, idx, g, w, bias).untouched()
    dfg, dg = conv_dgrad(shape, feat, idx, g, w, dy)
    assert dfg.untouched() and dg.untouched()
    assert _lib.load().pcops_spider_conv_wgrad_workspace_bytes(0, 40, 3, 5, T, 16) == 0
    dw, db = conv_wgrad(shape, feat, idx, g, dy)
    assert (dw.t == 0).all() and (db.t == 0).all()
    dw, _ = conv_wgrad(shape, feat, idx, g, dy, want_db=False)
    assert (dw.t == 0).all()
    x, gamma, beta, dout = K.gn_inputs((1, 9, 16, 1), DEV)
    dx, dgamma, dbeta = gn_bwd((0, 9, 16, 1), dout, x, x, gamma, None, None)
    assert dx.untouched() and (dgamma.t == 0).all() and (dbeta.t == 0).all()
    delta, theta, tbias, dgt = K.taylor_inputs(1, DEV)
    assert taylor_fwd(0, delta, theta, tbias).untouched()
    dtheta, dtbias = taylor_bwd(0, delta, dgt)
    assert (dtheta.t == 0).all() and (dtbias.t == 0).all()


# ---------------------------------------------------------------------------------------------------------------- Taylor
@pytest.mark.parametrize("rows", K.TAYLOR_ROWS)
def test_taylor(rows):
    delta, theta, tbias, dg = K.taylor_inputs(rows, DEV)
    assert _lib.load().pcops_spider_taylor_bwd_workspace_bytes(rows, T) == min(256, -(-rows // 256)) * 400
    report = []
    g = _twice(taylor_fwd, rows, delta, theta, tbias)
    K.check_sum(g.t, R.taylor_fwd(delta, theta, tbias), "g", report=report)
    dtheta, dtbias = _twice(taylor_bwd, rows, delta, dg)
    ref = R.taylor_bwd(delta, dg)
    K.check_sum(dtheta.t, ref["dtheta"], "dtheta", report=report)
    K.check_sum(dtbias.t, ref["dtbias"], "dtbias", report=report)
    for what, worst, rms in report:
        print("rows %d %-8s worst err/bound %.3g  relative RMS %.3g" % (rows, what, worst, rms))


# ------------------------------------------------------------------------------------------------------------ group norm
@pytest.mark.parametrize("shape", K.GN_CASES, ids=str)
def test_group_norm(shape):
    """The shape (2, 32, 32, 4) has one (cloud, group) whose 256 = 2^8 values all equal 1.5: every thread holds one value,
    every partial sum of the tree is 1.5 times a power of two, so the fp32 sums for that group are exact and mean = 1.5 to
    the last bit; every deviation is then 0, var = 0, rstd = 1 / sqrt(eps) and out = relu(beta) exactly."""
    b, n, c, groups = shape
    cg = c // groups
    x, gamma, beta, dout = K.gn_inputs(shape, DEV)
    report = []
    y, mean, rstd = _twice(gn_fwd, shape, x, gamma, beta)
    f = R.group_norm_relu_fwd(x, gamma, beta, groups, K.EPS, mean.t, rstd.t, y.t)
    K.check_sum(mean.t, f["mean"], "mean", report=report)
    assert torch.isfinite(rstd.t).all()
    over = (rstd.t.double() - f["rstd"]).abs() / f["rstd_lim"]
    assert (over <= 1).all(), "rstd: worst err/bound %.3g" % over.max().item()
    K.check_sum(y.t, f["out"], "out", report=report)
    assert (y.t >= 0).all()
    assert f["flips_ok"], "%d decisions differ from float64's, not all of them ties" % int(f["flips"].sum())
    assert (y.t[..., c - 1] == 0).all()                                   # gamma = 0, beta = 0
    if shape in K.GN_CONST:
        cloud, grp, v = K.GN_CONST[shape]
        assert (n * cg) & (n * cg - 1) == 0
        sl = slice(grp * cg, (grp + 1) * cg)
        assert (x[cloud, :, sl] == v).all()
        assert mean.t[cloud, grp].item() == v
        assert (f["var"][0][cloud, grp] == 0).all()                       # about the stored mean: every deviation is 0
        assert torch.equal(y.t[cloud, :, sl], torch.relu(beta[sl]).expand(n, cg))

    dx, dgamma, dbeta = _twice(gn_bwd, shape, dout, x, y.t, gamma, mean.t, rstd.t)
    r = R.group_norm_relu_bwd(dout, x, y.t, gamma, mean.t, rstd.t, groups)
    assert (r["gy"][..., c - 1] == 0).all()
    K.check_sum(dgamma.t, r["dgamma"], "dgamma", report=report)
    K.check_sum(dbeta.t, r["dbeta"], "dbeta", report=report)
    K.check_sum(dx.t, r["dx"], "dx", report=report)
    assert dbeta.t[c - 1].item() == 0 and dgamma.t[c - 1].item() == 0
    for what, worst, rms in report:
        print("%s %-8s worst err/bound %.3g  relative RMS %.3g" % (shape, what, worst, rms))


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("first_layer", [False, True], ids=["inner", "first"])
@pytest.mark.parametrize("det", [True, False], ids=["deterministic", "default"])
@pytest.mark.parametrize("shape", K.END_TO_END, ids=K.conv_id)
def test_layer_is_its_entry_points(shape, det, first_layer):
    b, n, k, c, o = shape
    groups = 16
    gshape = (b, n, o, groups)
    feat, idx, _, w, bias, _ = K.conv_inputs(shape, DEV)
    delta, theta, tbias, _ = K.taylor_inputs(b * n * k, DEV)
    delta = delta.view(b, n, k, 3)
    _, gamma, beta, dout = K.gn_inputs(gshape, DEV)
    prev = _lib.deterministic()
    _lib.set_deterministic(det)
    try:
        fl = feat.clone().requires_grad_(not first_layer)
        leaves = [t.clone().requires_grad_(True) for t in (theta, tbias, w, bias, gamma, beta)]
        res = S.spider_conv(fl, idx, delta, *leaves, groups, eps=K.EPS)
        res.backward(dout)
        # the same, entry point by entry point
        g = taylor_fwd(b * n * k, delta, theta, tbias).t.view(b, n, k, T)
        y = conv_fwd(shape, feat, idx, g, w, bias).t
        out, mean, rstd = (v.t for v in gn_fwd(gshape, y, gamma, beta))
        assert K.bits_equal(res.detach(), out)
        dy, dgamma, dbeta = (v.t for v in gn_bwd(gshape, dout, y, out, gamma, mean, rstd))
        dw, db = (v.t for v in conv_wgrad(shape, feat, idx, g, dy))
        dfg, dg = conv_dgrad(shape, feat, idx, g, w, dy, want_dfg=not first_layer)
        dtheta, dtbias = (v.t for v in taylor_bwd(b * n * k, delta, dg.t))
        for name, leaf, got in zip(("dtheta", "dtbias", "dW", "db", "dgamma", "dbeta"), leaves,
                                   (dtheta, dtbias, dw, db, dgamma, dbeta)):
            assert K.bits_equal(leaf.grad, got), name
        tw, wg = R.taylor_bwd(delta, dg.t), R.conv_wgrad(feat, idx, g, dy)
        gn = R.group_norm_relu_bwd(dout, y, out, gamma, mean, rstd, groups)
        for name, got, triple in (("dtheta", dtheta, tw["dtheta"]), ("dtbias", dtbias, tw["dtbias"]), ("dW", dw, wg["dw"]),
                                  ("db", db, wg["db"]), ("dgamma", dgamma, gn["dgamma"]), ("dbeta", dbeta, gn["dbeta"]),
                                  ("dy", dy, gn["dx"]), ("dg", dg.t, R.conv_dgrad(feat, idx, g, w, dy)["dg"])):
            # db = the column sums of dy, and the sum of a group-norm gradient over a group is zero in exact arithmetic:
            # with one channel per group (O = 16) the reference of db is pure cancellation
            K.check_sum(got, triple, name, rms=not (name == "db" and o == groups))
        if first_layer:
            assert fl.grad is None
        else:
            K.check_sum(dfg.t, R.conv_dgrad(feat, idx, g, w, dy)["dfg"], "dfg")
            triple = R.scatter_grouped(dfg.t, idx, n)
            K.check_sum(fl.grad, triple, "dF of the layer")
            dF = S.scatter_grouped(dfg.t, idx, n)
            K.check_sum(dF, triple, "dF through scatter_grouped")
            if det:
                assert K.bits_equal(fl.grad, dF)
    finally:
        _lib.set_deterministic(prev)
