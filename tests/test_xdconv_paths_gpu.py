"""The wide-channel path of the X-Conv contraction (csrc/xconv.hip, PCOPS_OPT_XCONV_CHANNEL_GROUPS): beyond 256 channels the
forward and the data gradient spread the 16-channel tiles over a second grid axis, at most 8 tiles per group.  Through the
C ABI, per wide case of tests/xdconv_checks.py:

  * pcops_xconv_channel_groups is the mirrored rule, and 1 with the option off; pcops_xconv_dgrad_workspace_bytes is
    groups b p K K 4 bytes, and 0 with the option off and for every case of xconv_checks.CASES
  * out, dlifted and dfts_grouped: BIT-IDENTICAL between the option on and off (channels never mix, the arithmetic per
    element is the one-group kernel's), and inside the per-element bound and the relative-RMS bar against float64
  * dX of pcops_xconv_dgrad_ws: the groups' partial sums added in ascending order -- inside the bound and the bar, the same
    bits on two calls; every slice of the NaN-prefilled workspace written whole; its slices add up to dX bit for bit
  * pcops_xconv_dgrad (the entry point without workspace) runs one group whatever the option says: the bits of _ws with
    the option off; and on every case of xconv_checks.CASES _ws is bit-identical to it with a NULL workspace
  * dfts_grouped == NULL is honoured; every output and the workspace lie in guard-banded buffers whose guards stay intact

Bounds: |out - ref| <= 2 (L + 4) 2^-24 A per element with the L of tests/test_xconv_paths_gpu.py (2 K, c + dm, K + dm), beside
the bar of tests/xdconv_checks.py (twice the worst sequential-fp32 value on these very inputs, measured without a GPU by
tests/test_xdconv_ref_cpu.py).  The option is restored after every test."""
import pytest
import torch

import xconv_checks as XC
import xconv_ref as R
import xdconv_checks as K
from scanobjectnn_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def P(t):
    return t.data_ptr() if t is not None else None


@pytest.fixture(autouse=True)
def _restore_option():
    was = _lib.get_option(_lib.OPT_XCONV_CHANNEL_GROUPS)
    yield
    _lib.set_option(_lib.OPT_XCONV_CHANNEL_GROUPS, was)


def _done(*outs):
    torch.cuda.synchronize()
    for o in outs:
        if o is not None:
            assert o.guards_intact()


def fwd(shape, lifted, fts, idx, X, wd):
    b, n, p, k, c1, c2, dm = shape
    out = K.Out((b, p, (c1 + c2) * dm), device=DEV)
    _lib.call("pcops_xconv_fwd", *shape, P(lifted), P(fts), P(idx), P(X), P(wd), out.ptr())
    _done(out)
    return out


def dgrad_ws(shape, lifted, fts, idx, X, wd, dout, want_dfg=True):
    """pcops_xconv_dgrad_ws with the workspace the library asks for -> dX, dlifted, dfg, workspace (None with one group)"""
    b, n, p, k, c1, c2, dm = shape
    dX, dl = K.Out((b, p, k, k), device=DEV), K.Out((b, p, k, c1), device=DEV)
    dfg = K.Out((b, p, k, max(c2, 1)), device=DEV)
    nbytes = _lib.load().pcops_xconv_dgrad_workspace_bytes(*shape)
    ws = K.Out((nbytes // 4,), device=DEV) if nbytes else None
    _lib.call("pcops_xconv_dgrad_ws", *shape, P(lifted), P(fts), P(idx), P(X), P(wd), P(dout), dX.ptr(), dl.ptr(),
              dfg.ptr() if want_dfg and c2 else None, ws.ptr() if ws else None)
    _done(dX, dl, dfg, ws)
    if not (want_dfg and c2):
        assert dfg.untouched()
    return dX, dl, dfg, ws


def dgrad_plain(shape, lifted, fts, idx, X, wd, dout):
    b, n, p, k, c1, c2, dm = shape
    dX, dl = K.Out((b, p, k, k), device=DEV), K.Out((b, p, k, c1), device=DEV)
    dfg = K.Out((b, p, k, max(c2, 1)), device=DEV)
    _lib.call("pcops_xconv_dgrad", *shape, P(lifted), P(fts), P(idx), P(X), P(wd), P(dout), dX.ptr(), dl.ptr(),
              dfg.ptr() if c2 else None)
    _done(dX, dl, dfg)
    return dX, dl, dfg


@pytest.mark.parametrize("shape", K.WIDE_CASES, ids=K.case_id)
def test_wide_contraction(shape):
    b, n, p, k, c1, c2, dm = shape
    lib = _lib.load()
    lifted, fts, idx, X, wd, dout = K.inputs(shape, DEV)
    groups, _ = K.channel_groups(c1 + c2)
    assert groups > 1
    report = []

    # ---- the option off: one group everywhere, no workspace
    _lib.set_option(_lib.OPT_XCONV_CHANNEL_GROUPS, 0)
    assert lib.pcops_xconv_channel_groups(*shape) == 1 and lib.pcops_xconv_dgrad_workspace_bytes(*shape) == 0
    out1 = fwd(shape, lifted, fts, idx, X, wd)
    dX1, dl1, dfg1, ws1 = dgrad_ws(shape, lifted, fts, idx, X, wd, dout)
    assert ws1 is None

    # ---- the option on
    _lib.set_option(_lib.OPT_XCONV_CHANNEL_GROUPS, 1)
    assert lib.pcops_xconv_channel_groups(*shape) == groups
    assert lib.pcops_xconv_dgrad_workspace_bytes(*shape) == groups * b * p * k * k * 4
    out = fwd(shape, lifted, fts, idx, X, wd)
    K.check_sum(out.t, R.fwd(lifted, fts, idx, X, wd), "out", report=report)
    assert K.bits_equal(out.t, out1.t)

    dX, dl, dfg, ws = dgrad_ws(shape, lifted, fts, idx, X, wd, dout)
    ref = R.dgrad(lifted, fts, idx, X, wd, dout)
    K.check_sum(dX.t, ref["dX"], "dX", report=report)
    K.check_sum(dl.t, ref["dlifted"], "dlifted", report=report)
    assert K.bits_equal(dl.t, dl1.t)
    if c2:
        K.check_sum(dfg.t, ref["dfg"], "dfts_grouped", report=report)
        assert K.bits_equal(dfg.t, dfg1.t)
    K.check_sum(dX1.t, ref["dX"], "dX, one group", report=report)

    # every group wrote its whole slice, and dX is the slices added in ascending order
    part = ws.t.view(groups, b, p, k, k)
    assert torch.isfinite(part).all()
    acc = torch.zeros_like(part[0])
    for g in range(groups):
        acc = acc + part[g]
    assert K.bits_equal(acc, dX.t)

    # the same bits on a second call
    dX2, dl2, dfg2, _ = dgrad_ws(shape, lifted, fts, idx, X, wd, dout)
    assert K.bits_equal(dX2.t, dX.t) and K.bits_equal(dl2.t, dl.t) and K.bits_equal(dfg2.t, dfg.t)
    assert K.bits_equal(fwd(shape, lifted, fts, idx, X, wd).t, out.t)

    # dfts_grouped == NULL: the other two keep their bits, the buffer is untouched (asserted in dgrad_ws)
    if c2:
        dX0, dl0, _, _ = dgrad_ws(shape, lifted, fts, idx, X, wd, dout, want_dfg=False)
        assert K.bits_equal(dX0.t, dX.t) and K.bits_equal(dl0.t, dl.t)

    # the entry point without workspace runs one group whatever the option says
    dXp, dlp, dfgp = dgrad_plain(shape, lifted, fts, idx, X, wd, dout)
    assert K.bits_equal(dXp.t, dX1.t) and K.bits_equal(dlp.t, dl1.t) and K.bits_equal(dfgp.t, dfg1.t)
    for what, worst, rms in report:
        print("%s %-13s worst err/bound %.3g  relative RMS %.3g" % (shape, what, worst, rms))


@pytest.mark.parametrize("shape", XC.CASES, ids=K.case_id)
def test_one_group_cases_take_the_old_launch(shape):
    """c <= 256: one group and no workspace whatever the option says; _ws with a NULL workspace is pcops_xconv_dgrad"""
    lib = _lib.load()
    tensors = K.inputs(shape, DEV)
    want = dgrad_plain(shape, *tensors)
    for option in (1, 0):
        _lib.set_option(_lib.OPT_XCONV_CHANNEL_GROUPS, option)
        assert lib.pcops_xconv_channel_groups(*shape) == 1 == K.channel_groups(shape[4] + shape[5], option)[0]
        assert lib.pcops_xconv_dgrad_workspace_bytes(*shape) == 0
        dX, dl, dfg, ws = dgrad_ws(shape, *tensors)
        assert ws is None
        assert K.bits_equal(dX.t, want[0].t) and K.bits_equal(dl.t, want[1].t) and K.bits_equal(dfg.t, want[2].t)


def test_queries_answer_zero_where_the_launchers_refuse():
    lib = _lib.load()
    for shape in XC.UNSUPPORTED + [(0, 20, 17, 16, 96, 480, 1)]:
        assert lib.pcops_xconv_channel_groups(*shape) == 0 and lib.pcops_xconv_dgrad_workspace_bytes(*shape) == 0
    # a wide shape without its workspace is a NULL-pointer error before any launch, and writes nothing
    shape = K.WIDE_CASES[0]
    b, n, p, k, c1, c2, dm = shape
    lifted, fts, idx, X, wd, dout = K.inputs(shape, DEV)
    dX, dl, dfg = K.Out((b, p, k, k), device=DEV), K.Out((b, p, k, c1), device=DEV), K.Out((b, p, k, c2), device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.pcops_xconv_dgrad_ws(*shape, P(lifted), P(fts), P(idx), P(X), P(wd), P(dout), dX.ptr(), dl.ptr(), dfg.ptr(),
                                    None, stream) == -1
    torch.cuda.synchronize()
    assert dX.untouched() and dl.untouched() and dfg.untouched()


def test_autograd_function_takes_the_wide_path():
    """xconv_ops.dgrad calls the _ws form: the Function's gradients on the decoder's widest shape equal the ABI's bits"""
    from scanobjectnn_amd.pointcnn import xconv_ops
    shape = (2, 20, 17, 16, 96, 480, 1)
    lifted, fts, idx, X, wd, dout = K.inputs(shape, DEV)
    calls = []
    hook = lambda name, phase, args: calls.append(name) if phase == "pre" else None  # noqa: E731
    _lib._hooks.append(hook)
    try:
        leaves = [t.clone().requires_grad_(True) for t in (lifted, X)]
        xconv_ops.xconv_contract(leaves[0], fts, idx, leaves[1], wd).backward(dout)
    finally:
        _lib._hooks.remove(hook)
    assert "pcops_xconv_dgrad_ws" in calls and "pcops_xconv_dgrad" not in calls
    dX, dl, _, _ = dgrad_ws(shape, lifted, fts, idx, X, wd, dout)
    assert K.bits_equal(leaves[1].grad, dX.t) and K.bits_equal(leaves[0].grad, dl.t)
