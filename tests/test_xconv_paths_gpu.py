"""Every kernel path of the X-Conv contraction (csrc/xconv.hip) held to the float64 definitions of tests/xconv_ref.py element
by element, through the C ABI (_lib.call), each entry point on the fp32 tensors it is given.

Memory contract of every case: every output and every workspace lies in a tests/edge_checks.Out buffer -- NaN prefill, guard
bands on both sides bit-identical afterwards -- so a store past p, K, c or dm, or a slot a kernel should have written and did
not, shows.  Every case runs twice and must be bit-identical: the file promises fixed-order sums everywhere.

Bounds: |out - ref| <= 2 (L + 4) 2^-24 A per element (edge_checks.check_sum, constants unchanged) beside the family's
relative-RMS bar of tests/xconv_checks.py.  tests/test_xconv_ref_cpu.py shows without a GPU that a sequential fp32 evaluation
stays inside these bounds on the same inputs and that one wrong restatement per edge falls outside them.

What each case reaches (b, n, p, K, c1, c2, dm) -- forward and data gradient: a wave per point, 16 points per workgroup, 16
channels per MFMA tile, K zero-padded to 16:
  1, 33, 33, 8, 24, 0, 4     no fts (NULL fts and idx); dm = 4; a third workgroup that holds one point; an 8-channel tail tile
  2, 40, 17, 12, 12, 48, 2   K = 12: four padded rows and columns of X, padded rows of wd in LDS; the lifted / fts boundary
                             at channel 12 inside the first tile; c = 60: a 12-channel tail; p != n; a workgroup that
                             straddles the two clouds (points 16..31 of 34)
  3, 20, 20, 16, 48, 192, 2  K = 16 exactly: no padding anywhere; c = 240: 15 whole tiles, 30 720 bytes of wd in LDS
  1, 9, 5, 1, 3, 5, 1        K = 1 (15 padded rows); dm = 1; c = 8: one half-empty tile
  2, 64, 64, 5, 16, 16, 3    odd K; whole tiles and whole workgroups only; dm = 3
  dfts_grouped == NULL on every case with fts: dX and dlifted bit-identical, the buffer untouched.  b = 0: OK, untouched.
Weight gradient: grid (channel tiles, splits); the split count is read back from pcops_xconv_wgrad_splits, the workspace size
from pcops_xconv_wgrad_workspace_bytes, and both are asserted per case -- see WGRAD_CASES of tests/xconv_checks.py: one split
(direct store, workspace NULL) at one point and at five, then 2, 4, 8, 16, 32 and the cap of 64, four of them with trailing
splits that hold no point and must store zeros into the NaN-prefilled workspace, one whose count the channel tiles cap.
b = 0: dwd zeroed.  Unsupported shapes: PCOPS_ERR_UNSUPPORTED from all three launchers and the two queries answer 0, nothing
written.
"""
import pytest
import torch

import xconv_checks as K
import xconv_ref as R
from scanobjectnn_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_UNSUPPORTED = -4      # PCOPS_ERR_UNSUPPORTED of include/pcops.h


def P(t):
    return t.data_ptr() if t is not None else None


def _done(*outs):
    torch.cuda.synchronize()
    for o in outs:
        if o is not None:
            assert o.guards_intact()


def fwd(shape, lifted, fts, idx, X, wd):
    b, n, p, k, c1, c2, dm = shape
    out = K.Out((max(b, 1), p, (c1 + c2) * dm), device=DEV)
    _lib.call("pcops_xconv_fwd", *shape, P(lifted), P(fts), P(idx), P(X), P(wd), out.ptr())
    _done(out)
    return out


def dgrad(shape, lifted, fts, idx, X, wd, dout, want_dfg=True):
    b, n, p, k, c1, c2, dm = shape
    dX, dl = K.Out((max(b, 1), p, k, k), device=DEV), K.Out((max(b, 1), p, k, c1), device=DEV)
    dfg = K.Out((max(b, 1), p, k, max(c2, 1)), device=DEV)
    _lib.call("pcops_xconv_dgrad", *shape, P(lifted), P(fts), P(idx), P(X), P(wd), P(dout), dX.ptr(), dl.ptr(),
              dfg.ptr() if want_dfg and c2 else None)
    _done(dX, dl, dfg)
    if not (want_dfg and c2):
        assert dfg.untouched()
    return dX, dl, dfg


def wgrad(shape, lifted, fts, idx, X, dout):
    b, n, p, k, c1, c2, dm = shape
    dwd = K.Out((k, c1 + c2, dm), device=DEV)
    nbytes = _lib.load().pcops_xconv_wgrad_workspace_bytes(*shape)
    ws = K.Out((nbytes // 4,), device=DEV) if nbytes else None
    _lib.call("pcops_xconv_wgrad", *shape, P(lifted), P(fts), P(idx), P(X), P(dout), dwd.ptr(), ws.ptr() if ws else None)
    _done(dwd, ws)
    return dwd, ws


def _twice(fn, *args, **kw):
    """the call made twice into fresh buffers: bit-identical results, the first returned"""
    first, second = fn(*args, **kw), fn(*args, **kw)
    for a, b_ in zip(first, second) if isinstance(first, tuple) else ((first, second),):
        if a is not None:
            assert K.bits_equal(a.t, b_.t)
    return first


def _check_wgrad(shape, splits, occupied, tensors, report):
    b, n, p, k, c1, c2, dm = shape
    lifted, fts, idx, X, wd, dout = tensors
    lib = _lib.load()
    assert lib.pcops_xconv_wgrad_splits(*shape) == splits
    assert lib.pcops_xconv_wgrad_workspace_bytes(*shape) == (splits * k * (c1 + c2) * dm * 4 if splits > 1 else 0)
    assert -(-(b * p) // K.wgrad_chunk(b, p, splits)) == occupied
    dwd, ws = _twice(wgrad, shape, lifted, fts, idx, X, dout)
    K.check_sum(dwd.t, R.wgrad(lifted, fts, idx, X, wd.shape, dout), "dwd", report=report)
    if ws is not None:
        part = ws.t.view(splits, -1)
        assert torch.isfinite(part).all()                                  # every split wrote its whole slice ...
        assert (part[occupied:] == 0).all() and (part[:occupied] != 0).any(dim=1).all()      # ... the empty ones zeros


@pytest.mark.parametrize("shape", K.CASES, ids=K.case_id)
def test_contraction(shape):
    tensors = K.inputs(shape, DEV)
    lifted, fts, idx, X, wd, dout = tensors
    report = []
    out = _twice(fwd, shape, lifted, fts, idx, X, wd)
    K.check_sum(out.t, R.fwd(lifted, fts, idx, X, wd), "out", report=report)

    dX, dl, dfg = _twice(dgrad, shape, lifted, fts, idx, X, wd, dout)
    ref = R.dgrad(lifted, fts, idx, X, wd, dout)
    K.check_sum(dX.t, ref["dX"], "dX", report=report)
    K.check_sum(dl.t, ref["dlifted"], "dlifted", report=report)
    if fts is not None:
        K.check_sum(dfg.t, ref["dfg"], "dfts_grouped", report=report)
        dX0, dl0, _ = dgrad(shape, lifted, fts, idx, X, wd, dout, want_dfg=False)
        assert K.bits_equal(dX0.t, dX.t) and K.bits_equal(dl0.t, dl.t)

    splits, occupied = next((s, o) for sh, s, o in K.WGRAD_CASES if sh == shape)
    _check_wgrad(shape, splits, occupied, tensors, report)
    for what, worst, rms in report:
        print("%s %-13s worst err/bound %.3g  relative RMS %.3g" % (shape, what, worst, rms))


@pytest.mark.parametrize("case", [c for c in K.WGRAD_CASES if c[0] not in K.CASES], ids=K.case_id)
def test_wgrad_splits(case):
    shape, splits, occupied = case
    report = []
    _check_wgrad(shape, splits, occupied, K.inputs(shape, DEV), report)
    print("%s dwd worst err/bound %.3g  relative RMS %.3g" % (shape, report[0][1], report[0][2]))


def test_no_clouds():
    shape = (0, 40, 17, 12, 12, 48, 2)
    lifted, fts, idx, X, wd, dout = K.inputs((1,) + shape[1:], DEV)
    assert fwd(shape, lifted, fts, idx, X, wd).untouched()
    assert all(o.untouched() for o in dgrad(shape, lifted, fts, idx, X, wd, dout))
    assert _lib.load().pcops_xconv_wgrad_splits(*shape) == 0 and _lib.load().pcops_xconv_wgrad_workspace_bytes(*shape) == 0
    dwd, _ = wgrad(shape, lifted, fts, idx, X, dout)
    assert (dwd.t == 0).all()


@pytest.mark.parametrize("shape", K.UNSUPPORTED, ids=K.case_id)
def test_unsupported_shapes_write_nothing(shape):
    b, n, p, k, c1, c2, dm = shape
    lib = _lib.load()
    assert lib.pcops_xconv_supported(k, c1, c2, dm) == 0
    assert lib.pcops_xconv_wgrad_splits(*shape) == 0 and lib.pcops_xconv_wgrad_workspace_bytes(*shape) == 0
    lifted, fts, idx, X, wd, dout = K.inputs(shape, DEV)
    stream = torch.cuda.current_stream().cuda_stream
    c = c1 + c2
    out, dX, dl = K.Out((b, p, c * dm), device=DEV), K.Out((b, p, k, k), device=DEV), K.Out((b, p, k, c1), device=DEV)
    dfg, dwd = K.Out((b, p, k, c2), device=DEV), K.Out((k, c, dm), device=DEV)
    ws = K.Out((64 * k * c * dm,), device=DEV)
    assert lib.pcops_xconv_fwd(*shape, P(lifted), P(fts), P(idx), P(X), P(wd), out.ptr(), stream) == ERR_UNSUPPORTED
    assert lib.pcops_xconv_dgrad(*shape, P(lifted), P(fts), P(idx), P(X), P(wd), P(dout), dX.ptr(), dl.ptr(), dfg.ptr(),
                                 stream) == ERR_UNSUPPORTED
    assert lib.pcops_xconv_wgrad(*shape, P(lifted), P(fts), P(idx), P(X), P(dout), dwd.ptr(), ws.ptr(),
                                 stream) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(o.untouched() for o in (out, dX, dl, dfg, dwd, ws))
    assert "outside the range" in _lib.strerror(ERR_UNSUPPORTED)
