"""Every kernel path of PointNet's per-cloud transform and its regulariser (csrc/tnet.hip) held to the float64 definitions
of tests/tnet_ref.py element by element, through the C ABI (_lib.call), each entry point on the fp32 tensors it is given.

Memory contract of every case: every output and every workspace lies in a tests/edge_checks.Out buffer -- NaN prefill, guard
bands on both sides bit-identical afterwards -- so a store past n or past the 64 columns, or a slot a kernel should have
written and did not, shows.  Every case runs twice and must be bit-identical: the file promises fixed-order sums everywhere,
with and without the library's deterministic mode.

Bounds: |out - ref| <= 2 (L + 4) 2^-24 A per element (edge_checks.check_sum, constants unchanged) beside the family's
relative-RMS bar of tests/tnet_checks.py; L = 64 for out, dX and the regulariser, L = n for dT.  tests/test_tnet_ref_cpu.py
shows without a GPU that a sequential fp32 evaluation stays inside these bounds on the same inputs and that one wrong
restatement per edge falls outside them.

What each case reaches (b, n) -- forward: 16 points per wave step, 128 per workgroup; backward: 64 points per step, a split a
whole number of steps: see CASES and SPLIT_CASES of tests/tnet_checks.py.  The split count is read back from
pcops_transformk_bwd_splits, the workspace size from pcops_transformk_workspace_bytes, and both are asserted per case: one
split (direct store, workspace NULL), then 2, 4, 8 and the cap of 16, three of them with trailing splits that hold no point
and must store zeros into the NaN-prefilled workspace, one whose count the number of clouds caps.  dX == NULL on every case:
dT bit-identical, the buffer untouched.  Unsupported shapes: PCOPS_ERR_UNSUPPORTED from every launcher, the queries answer 0,
nothing written."""
import pytest
import torch

import tnet_checks as K
import tnet_ref as R
from scanobjectnn_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_UNSUPPORTED = -4      # PCOPS_ERR_UNSUPPORTED of include/pcops.h
W = 2.0 ** -10


def _done(*outs):
    torch.cuda.synchronize()
    for o in outs:
        if o is not None:
            assert o.guards_intact()


def fwd(shape, X, T):
    b, n = shape
    out = K.Out((b, n, 64), device=DEV)
    _lib.call("pcops_transformk_fwd", b, n, 64, X.data_ptr(), T.data_ptr(), out.ptr())
    _done(out)
    return out


def bwd(shape, X, T, G, want_dx=True):
    b, n = shape
    dX, dT = K.Out((b, n, 64), device=DEV), K.Out((b, 64, 64), device=DEV)
    nbytes = _lib.load().pcops_transformk_workspace_bytes(b, n, 64)
    ws = K.Out((nbytes // 4,), device=DEV) if nbytes else None
    _lib.call("pcops_transformk_bwd", b, n, 64, X.data_ptr(), T.data_ptr(), G.data_ptr(), dX.ptr() if want_dx else None,
              dT.ptr(), ws.ptr() if ws else None)
    _done(dX, dT, ws)
    if not want_dx:
        assert dX.untouched()
    return dX, dT, ws


def ortho(T, weight):
    b = T.shape[0]
    parts, dT = K.Out((b,), device=DEV), K.Out((b, 64, 64), device=DEV)
    _lib.call("pcops_ortho_reg", b, 64, T.data_ptr(), float(weight), parts.ptr(), dT.ptr())
    _done(parts, dT)
    return parts, dT


def _twice(fn, *args, **kw):
    """the call made twice into fresh buffers: bit-identical results, the first returned"""
    first, second = fn(*args, **kw), fn(*args, **kw)
    for a, b_ in zip(first, second) if isinstance(first, tuple) else ((first, second),):
        if a is not None:
            assert K.bits_equal(a.t, b_.t)
    return first


def _check_bwd(shape, splits, occupied, report):
    b, n = shape
    lib = _lib.load()
    assert lib.pcops_transformk_supported(b, n, 64) == 1
    assert lib.pcops_transformk_bwd_splits(b, n, 64) == splits == K.bwd_splits(b, n)
    assert lib.pcops_transformk_workspace_bytes(b, n, 64) == (b * splits * 64 * 64 * 4 if splits > 1 else 0)
    assert -(-n // K.bwd_chunk(n, splits)) == occupied
    X, T, G = K.inputs(shape, DEV)
    dX, dT, ws = _twice(bwd, shape, X, T, G)
    ref = R.bwd(X, T, G)
    K.check_sum(dX.t, ref["dX"], "dX", report=report)
    K.check_sum(dT.t, ref["dT"], "dT", report=report)
    assert (ws is None) == (splits == 1)
    if ws is not None:
        part = ws.t.view(b, splits, -1)
        assert torch.isfinite(part).all()                                  # every split wrote its whole slice ...
        assert (part[:, occupied:] == 0).all() and (part[:, :occupied] != 0).any(dim=2).all()      # ... the empty ones zeros
    _, dT0, _ = bwd(shape, X, T, G, want_dx=False)                         # dX == NULL
    assert K.bits_equal(dT0.t, dT.t)
    # the same bits in the library's deterministic mode
    prev = _lib.deterministic()
    _lib.set_deterministic(True)
    try:
        dXd, dTd, _ = bwd(shape, X, T, G)
    finally:
        _lib.set_deterministic(prev)
    assert K.bits_equal(dXd.t, dX.t) and K.bits_equal(dTd.t, dT.t)


@pytest.mark.parametrize("shape", K.CASES, ids=K.case_id)
def test_transform(shape):
    X, T, G = K.inputs(shape, DEV)
    report = []
    out = _twice(fwd, shape, X, T)
    K.check_sum(out.t, R.fwd(X, T), "out", report=report)
    splits, occupied = next(((s, o) for sh, s, o in K.SPLIT_CASES if sh == shape),
                            (K.bwd_splits(*shape), -(-shape[1] // K.bwd_chunk(shape[1], K.bwd_splits(*shape)))))
    _check_bwd(shape, splits, occupied, report)
    for what, worst, rms in report:
        print("%s %-4s worst err/bound %.3g  relative RMS %.3g" % (shape, what, worst, rms))


@pytest.mark.parametrize("case", [c for c in K.SPLIT_CASES if c[0] not in K.CASES], ids=K.case_id)
def test_backward_splits(case):
    shape, splits, occupied = case
    report = []
    X, T, _ = K.inputs(shape, DEV)
    K.check_sum(_twice(fwd, shape, X, T).t, R.fwd(X, T), "out", report=report)
    _check_bwd(shape, splits, occupied, report)
    for what, worst, rms in report:
        print("%s %-4s worst err/bound %.3g  relative RMS %.3g" % (shape, what, worst, rms))


@pytest.mark.parametrize("case", K.ORTHO_CASES, ids=K.case_id)
def test_regulariser(case):
    T = K.ortho_inputs(case, DEV)
    report = []
    parts, dT = _twice(ortho, T, W)
    ref = R.ortho(T, W)
    K.check_sum(parts.t, ref["loss_parts"], "loss_parts", report=report)
    K.check_sum(dT.t, ref["dT"], "dT", report=report)
    if case[0] > 1:                                                       # clouds do not leak into each other
        one, dT1 = ortho(T[1:2].contiguous(), W)
        assert K.bits_equal(one.t, parts.t[1:2]) and K.bits_equal(dT1.t, dT.t[1:2])
    for what, worst, rms in report:
        print("%s %-10s worst err/bound %.3g  relative RMS %.3g" % (case, what, worst, rms))


@pytest.mark.parametrize("shape", K.UNSUPPORTED, ids=K.case_id)
def test_unsupported_shapes_write_nothing(shape):
    b, n, k = shape
    lib = _lib.load()
    assert lib.pcops_transformk_supported(b, n, k) == 0
    assert lib.pcops_transformk_bwd_splits(b, n, k) == 0 and lib.pcops_transformk_workspace_bytes(b, n, k) == 0
    stream = torch.cuda.current_stream().cuda_stream
    rows = max(n, 1)
    X = torch.ones(b, rows, k, device=DEV)
    T = torch.ones(b, k, k, device=DEV)
    out, dX, dT = K.Out((b, rows, k), device=DEV), K.Out((b, rows, k), device=DEV), K.Out((b, k, k), device=DEV)
    ws, parts = K.Out((16 * b * k * k,), device=DEV), K.Out((b,), device=DEV)
    assert lib.pcops_transformk_fwd(b, n, k, X.data_ptr(), T.data_ptr(), out.ptr(), stream) == ERR_UNSUPPORTED
    assert lib.pcops_transformk_bwd(b, n, k, X.data_ptr(), T.data_ptr(), X.data_ptr(), dX.ptr(), dT.ptr(), ws.ptr(),
                                    stream) == ERR_UNSUPPORTED
    if k != 64:
        assert lib.pcops_ortho_reg(b, k, T.data_ptr(), 0.001, parts.ptr(), dT.ptr(), stream) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(o.untouched() for o in (out, dX, dT, ws, parts))
