"""Every kernel path of the 3DmFV-Net family (csrc/mfv.hip) held to the float64 definitions of tests/mfv_ref.py, through the
C ABI (_lib.call), each entry point on the fp32 tensors it is given.

Memory contract of every case: every output and every workspace lies in a tests/edge_checks.Out buffer -- NaN prefill, guard
bands on both sides bit-identical afterwards -- so a store out of range, or a slot a kernel should have written and did not,
shows.  Every case runs twice and must be bit-identical: the file promises fixed-order sums, no float atomics.

Bars (tests/mfv_checks.py, measured by tests/test_mfv_ref_cpu.py): the representation within four times the worst fp32
evaluation of its definition (max-abs and relative RMS); every convolution sum within |out - ref| <= 2 (L + 4) 2^-24 A per
element (edge_checks.check_sum, unchanged) beside the family's relative-RMS bar.

What each case reaches.
fv_partial_kernel / fv_finish_kernel -- grid (ceil(N / 512), B); 64 points per LDS tile; Gaussians tid and tid + 256
  1, 1, 8          one point: one tile of one point, max = min = sum, 248 idle threads
  2, 7, 8          few points
  3, 65, 27        one point past a 64-point tile; point 0 of cloud 0 exactly on a mean
  2, 300, 125      K no multiple of 64; the cloud scaled by 1.5 and shifted by 0.2, much of it outside the grid
  1, 1025, 512     one point past the second chunk (three chunks folded in ascending order), both Gaussians of every thread
  2, 100, 10       non-cubic K, non-uniform w, anisotropic sigma
  both layouts: (B, 20, K) and the voxel-major (K, B, 20), bit-identical up to the permutation.  K = 513: unsupported.
conv3d_fwd_kernel -- grid (ceil(B / 64), ceil(Cout / 64), R^3); also the data gradient (conv3d_flip_kernel + the same kernel
with Cin and Cout exchanged, so Cout' up to 512 and Cin' down to 32)
conv3d_wgrad_kernel / wgrad_reduce_kernel -- grid (k^3 ceil(Cin / 64), ceil(Cout / 64), splits); the split count of every
case is read back from pcops_conv3d_wgrad_splits and asserted: 1 (direct store, workspace NULL), 2, 4, 8, 16
  1, 3, 5, 64, 32       kernel wider than the grid
  3, 2, 5, 64, 32       the 2^3 grid behind the first max pool of the 27-Gaussian model: taps no voxel can use store zeros
  3, 3, 3, 64, 32       a few clouds on the small grid
  65, 5, 3, 64, 32      one row past a tile at every voxel
  2, 5, 5, 128, 64      5^3 kernel on the 5^3 grid
  4, 8, 3, 128, 64      the 8^3 grid
  2, 4, 5, 256, 128     the 4^3 grid, 5^3 kernel
  1, 5, 5, 512, 256     widest layer
  bias == NULL and dbias == NULL twins; B = 0.  Unsupported shapes return PCOPS_ERR_UNSUPPORTED and write nothing.
"""
import pytest
import torch

import mfv_checks as K
import mfv_ref as R
from scanobjectnn_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNSUPPORTED = -4


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


def _twice(fn, *args, **kw):
    first, second = fn(*args, **kw), fn(*args, **kw)
    for a, b_ in zip(first, second) if isinstance(first, tuple) else ((first, second),):
        assert K.bits_equal(a.t, b_.t)
    return first


# ------------------------------------------------------------------------------------------------------- representation
def fv_fwd(case, pts, w, mu, sigma, voxel_major=False):
    b, n, k = case
    fv = K.Out((k, b, 20) if voxel_major else (b, 20, k), device=DEV)
    nbytes = _lib.load().pcops_fv3d_workspace_bytes(b, n, k)
    assert nbytes == b * -(-n // 512) * 20 * k * 4                       # chunk partials only: nothing of size N K
    ws = _ws(nbytes)
    _lib.call("pcops_fv3d_fwd", b, n, k, 1 if voxel_major else 0, P(pts), P(w), P(mu), P(sigma), fv.ptr(), OP(ws))
    _done(fv, ws)
    return fv


@pytest.mark.parametrize("case", K.FV_CASES, ids=str)
def test_representation(case):
    pts, w, mu, sigma = K.fv_inputs(case, DEV)
    want = R.get_3dmfv(pts, w, mu, sigma)
    fv = _twice(fv_fwd, case, pts, w, mu, sigma)
    assert torch.isfinite(fv.t).all()
    a, r = K.fv_errors(fv.t, want)
    print("%s get_3dmfv max-abs %.3g (bar %.3g)  relative RMS %.3g (bar %.3g)" % (case, a, K.FV_MAXABS_BAR, r, K.FV_RMS_BAR))
    assert a <= K.FV_MAXABS_BAR and r <= K.FV_RMS_BAR
    vm = _twice(fv_fwd, case, pts, w, mu, sigma, voxel_major=True)
    assert K.bits_equal(vm.t.permute(1, 2, 0), fv.t)


def test_representation_unsupported():
    pts, w, mu, sigma = K.fv_inputs((1, 16, 8), DEV)
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    for b, n, k in K.FV_UNSUPPORTED:
        fv, ws = K.Out((b, 20, k), device=DEV), K.Out((1024,), device=DEV)
        assert lib.pcops_fv3d_workspace_bytes(b, n, k) == 0
        assert lib.pcops_fv3d_fwd(b, n, k, 0, P(pts), P(w), P(mu), P(sigma), fv.ptr(), ws.ptr(), stream) == UNSUPPORTED
        torch.cuda.synchronize()
        assert fv.untouched() and ws.untouched()
    fv = K.Out((1, 20, 8), device=DEV)
    assert lib.pcops_fv3d_fwd(1, 0, 8, 0, P(pts), P(w), P(mu), P(sigma), fv.ptr(), fv.ptr(), stream) == -2     # N = 0
    assert lib.pcops_fv3d_fwd(0, 16, 8, 0, None, None, None, None, None, None, stream) == 0                    # no clouds
    torch.cuda.synchronize()
    assert fv.untouched()


# ---------------------------------------------------------------------------------------------------------- convolution
def conv_fwd(shape, xm, w, bias):
    b, r, k, cin, cout = shape
    y = K.Out((r ** 3, max(b, 1), cout), device=DEV)
    _lib.call("pcops_conv3d_fwd", b, r, k, cin, cout, P(xm), P(w), P(bias), y.ptr())
    _done(y)
    return y


def conv_dgrad(shape, w, dym):
    b, r, k, cin, cout = shape
    dx = K.Out((r ** 3, max(b, 1), cin), device=DEV)
    nbytes = _lib.load().pcops_conv3d_dgrad_workspace_bytes(b, r, k, cin, cout)
    assert nbytes == (k ** 3 * cin * cout * 4 if b else 0)
    ws = _ws(nbytes)
    _lib.call("pcops_conv3d_dgrad", b, r, k, cin, cout, P(w), P(dym), dx.ptr(), OP(ws))
    _done(dx, ws)
    return dx


def conv_wgrad(shape, xm, dym, want_db=True):
    b, r, k, cin, cout = shape
    dw, db = K.Out((k, k, k, cin, cout), device=DEV), K.Out((cout,), device=DEV)
    ws = _ws(_lib.load().pcops_conv3d_wgrad_workspace_bytes(b, r, k, cin, cout))
    _lib.call("pcops_conv3d_wgrad", b, r, k, cin, cout, P(xm), P(dym), dw.ptr(), db.ptr() if want_db else None, OP(ws))
    _done(dw, db, ws)
    if not want_db:
        assert db.untouched()
    return dw, db


@pytest.mark.parametrize("case", K.CONV_CASES, ids=K.conv_id)
def test_convolution(case):
    shape, splits = case
    b, r, k, cin, cout = shape
    x, w, bias, dy = K.conv_inputs(shape, DEV)
    xm, dym = R.to_vm(x), R.to_vm(dy)
    lib = _lib.load()
    assert lib.pcops_conv3d_wgrad_splits(b, r, k, cin, cout) == splits
    nbytes = lib.pcops_conv3d_wgrad_workspace_bytes(b, r, k, cin, cout)
    assert nbytes == (splits * (k ** 3 * cin * cout + cout) * 4 if splits > 1 else 0)
    report = []

    y = _twice(conv_fwd, shape, xm, w, bias)
    K.check_sum(R.from_vm(y.t, r), R.conv3d_fwd(x, w, bias), "y", report=report)
    y0 = conv_fwd(shape, xm, w, None)
    assert K.bits_equal(y0.t, conv_fwd(shape, xm, w, torch.zeros_like(bias)).t)
    K.check_sum(R.from_vm(y0.t, r), R.conv3d_fwd(x, w, None), "y without bias", report=report)

    dx = _twice(conv_dgrad, shape, w, dym)
    K.check_sum(R.from_vm(dx.t, r), R.conv3d_dgrad(w, dy), "dx", report=report)

    dw, db = _twice(conv_wgrad, shape, xm, dym)
    ref = R.conv3d_wgrad(x, dy, k)
    K.check_sum(dw.t, ref["dw"], "dw", report=report)
    K.check_sum(db.t, ref["db"], "db", report=report)
    dw0, _ = conv_wgrad(shape, xm, dym, want_db=False)
    assert K.bits_equal(dw0.t, dw.t)
    if r == 2 and k == 5:                                                   # offsets of +-2 reach no voxel of a 2^3 grid
        assert (dw.t[0] == 0).all() and (dw.t[:, :, 4] == 0).all()
    for what, worst, rms in report:
        print("%s %-16s worst err/bound %.3g  relative RMS %.3g" % (shape, what, worst, rms))


def test_convolution_no_clouds_and_unsupported():
    shape = (0, 3, 3, 64, 32)
    x, w, bias, dy = K.conv_inputs((1,) + shape[1:], DEV)
    xm, dym = R.to_vm(x), R.to_vm(dy)
    assert conv_fwd(shape, xm, w, bias).untouched() and conv_dgrad(shape, w, dym).untouched()
    dw, db = conv_wgrad(shape, xm, dym)
    assert (dw.t == 0).all() and (db.t == 0).all()
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    for b, r, k, cin, cout in K.CONV_UNSUPPORTED:
        out, ws = K.Out((1 << 16,), device=DEV), K.Out((1024,), device=DEV)
        assert lib.pcops_conv3d_wgrad_workspace_bytes(b, r, k, cin, cout) == 0
        assert lib.pcops_conv3d_dgrad_workspace_bytes(b, r, k, cin, cout) == 0
        assert lib.pcops_conv3d_wgrad_splits(b, r, k, cin, cout) == 0
        assert lib.pcops_conv3d_fwd(b, r, k, cin, cout, P(xm), P(w), P(bias), out.ptr(), stream) == UNSUPPORTED
        assert lib.pcops_conv3d_dgrad(b, r, k, cin, cout, P(w), P(dym), out.ptr(), ws.ptr(), stream) == UNSUPPORTED
        assert lib.pcops_conv3d_wgrad(b, r, k, cin, cout, P(xm), P(dym), out.ptr(), out.ptr(), ws.ptr(), stream) == UNSUPPORTED
        torch.cuda.synchronize()
        assert out.untouched() and ws.untouched()
