"""The 3DmFV kernels of libpcops (csrc/mfv.hip): the representation in one pass with nothing of size N K in memory, and the
k^3 SAME convolutions of the inception trunk on VOXEL-MAJOR activations (R^3, B, C), where the B rows of a voxel share one
list of in-grid taps and a tap outside the grid costs nothing.  PCOPS_MFV_NATIVE=0 selects the torch forms below
(broadcast algebra, F.conv3d): the A/B baseline, and the only form that runs off the GPU."""
import math
import os

import torch
import torch.nn.functional as F

from .. import _lib

FV_ROWS = 20
FV_MAX_K = 512
CONV_MAX_R = 8


def native_enabled():
    """PCOPS_MFV_NATIVE=0: the torch forms (the A/B baseline); read at every call"""
    return os.environ.get("PCOPS_MFV_NATIVE", "1") != "0"


def _ws(nbytes, dev):
    return torch.empty(max(int(nbytes), 4) // 4 + 1, dtype=torch.float32, device=dev)


# ------------------------------------------------------------------------------------------------------- representation
def fv3d_supported(b, n, k):
    return n >= 1 and 1 <= k <= FV_MAX_K and b <= 65535


def fv3d(points, w, mu, sigma, voxel_major=False):
    """points (B,N,3), w (K), mu (K,3), sigma (K,3) -> fv (B,20,K), or (K,B,20) with voxel_major.  No gradient: the points
    are data and the mixture is a constant (3DmFV-Net/train.py:278-283 feeds both)."""
    b, n, _ = points.shape
    k = w.shape[0]
    if not fv3d_supported(b, n, k):
        raise _lib.PcopsError("3DmFV kernel: B = %d, N = %d, K = %d is outside what csrc/mfv.hip is built for (N >= 1, "
                              "1 <= K <= %d); PCOPS_MFV_NATIVE=0 selects the torch form" % (b, n, k, FV_MAX_K))
    points = _lib.check(points.detach(), torch.float32, "points", 3)
    w = _lib.check(w.detach(), torch.float32, "w", 1)
    mu = _lib.check(mu.detach(), torch.float32, "mu", 2)
    sigma = _lib.check(sigma.detach(), torch.float32, "sigma", 2)
    fv = torch.empty((k, b, FV_ROWS) if voxel_major else (b, FV_ROWS, k), dtype=torch.float32, device=points.device)
    ws = _ws(_lib.load().pcops_fv3d_workspace_bytes(b, n, k), points.device)
    _lib.call("pcops_fv3d_fwd", b, n, k, 1 if voxel_major else 0, points.data_ptr(), w.data_ptr(), mu.data_ptr(),
              sigma.data_ptr(), fv.data_ptr(), ws.data_ptr())
    return fv


def fv3d_torch(points, w, mu, sigma):
    """get_3dmfv as written (tf_util.py:578-652) in broadcast algebra, any device and dtype: -> (B,20,K).  Materialises
    (B,N,K,3) tensors like the reference does."""
    n = points.shape[1]
    z = (points.unsqueeze(2) - mu) / sigma                                        # (B,N,K,3)
    p = torch.exp(-0.5 * (z * z).sum(-1)) / ((2.0 * math.pi) ** 1.5 * sigma.prod(-1))
    wp = p * w
    Q = wp / wp.sum(-1, keepdim=True)                                            # (B,N,K)
    d_pi_all = (Q - w) / (torch.sqrt(w) * n)
    d_pi = torch.stack([d_pi_all.amax(1), d_pi_all.sum(1)], dim=1)                # (B,2,K)
    Qd = Q.unsqueeze(-1)

    def stats(a, scale):                                                          # (B,N,K,3) -> (B,9,K)
        s = torch.cat([a.amax(1), a.amin(1), a.sum(1)], dim=2)                   # (B,K,9)
        return (scale.unsqueeze(-1) * s).permute(0, 2, 1)

    d_mu = stats(Qd * z, 1.0 / (n * torch.sqrt(w)))
    d_sigma = stats(Qd * (z * z - 1.0), 1.0 / (n * torch.sqrt(2.0 * w)))

    def normalise(d):
        d = torch.sign(d) * torch.sqrt(torch.abs(d))
        return d * torch.rsqrt(torch.clamp((d * d).sum(-1, keepdim=True), min=1e-12))

    return torch.cat([normalise(d_pi), normalise(d_mu), normalise(d_sigma)], dim=1)


# ---------------------------------------------------------------------------------------------------------- convolution
def conv3d_supported(r, k, cin, cout):
    """the shapes csrc/mfv.hip is built for (include/pcops.h "3DmFV-Net")"""
    return 1 <= r <= CONV_MAX_R and k in (3, 5) and cin % 16 == 0 and cout % 16 == 0 and 16 <= cin <= 512 and \
        16 <= cout <= 512


def conv3d_fwd(x, w, bias, r):
    """x (R^3,B,Cin) voxel-major, w (k,k,k,Cin,Cout), bias (Cout) or None -> y (R^3,B,Cout)"""
    v, b, cin = x.shape
    k, cout = w.shape[0], w.shape[4]
    y = torch.empty((v, b, cout), dtype=torch.float32, device=x.device)
    _lib.call("pcops_conv3d_fwd", b, r, k, cin, cout, x.data_ptr(), w.data_ptr(), _lib.ptr(bias), y.data_ptr())
    return y


def conv3d_dgrad(w, dy, r):
    """-> dx (R^3,B,Cin): the forward kernel on the mirrored, transposed weights"""
    v, b, cout = dy.shape
    k, cin = w.shape[0], w.shape[3]
    dx = torch.empty((v, b, cin), dtype=torch.float32, device=dy.device)
    ws = _ws(_lib.load().pcops_conv3d_dgrad_workspace_bytes(b, r, k, cin, cout), dy.device)
    _lib.call("pcops_conv3d_dgrad", b, r, k, cin, cout, w.data_ptr(), dy.data_ptr(), dx.data_ptr(), ws.data_ptr())
    return dx


def conv3d_wgrad(x, dy, k, r, need_bias=True):
    """-> dw (k,k,k,Cin,Cout), dbias (Cout) or None; split partials added in ascending order"""
    v, b, cin = x.shape
    cout = dy.shape[2]
    dw = torch.empty((k, k, k, cin, cout), dtype=torch.float32, device=dy.device)
    db = torch.empty(cout, dtype=torch.float32, device=dy.device) if need_bias else None
    ws = _ws(_lib.load().pcops_conv3d_wgrad_workspace_bytes(b, r, k, cin, cout), dy.device)
    _lib.call("pcops_conv3d_wgrad", b, r, k, cin, cout, x.data_ptr(), dy.data_ptr(), dw.data_ptr(), _lib.ptr(db),
              ws.data_ptr())
    return dw, db


class Conv3dFn(torch.autograd.Function):
    """(x (R^3,B,Cin), w (k,k,k,Cin,Cout), bias (Cout)) -> (R^3,B,Cout)"""

    @staticmethod
    def forward(ctx, x, w, bias, r):
        ctx.save_for_backward(x, w)
        ctx.r = r
        return conv3d_fwd(x, w, bias, r)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        dx = conv3d_dgrad(w, dy, ctx.r) if ctx.needs_input_grad[0] else None
        dw, db = conv3d_wgrad(x, dy, w.shape[0], ctx.r, need_bias=ctx.needs_input_grad[2])
        return dx, dw, db, None


def conv3d(x, w, bias):
    """x (R,R,R,B,Cin) contiguous (voxel-major), w (k,k,k,Cin,Cout), bias (Cout) -> (R,R,R,B,Cout).  Shapes outside
    conv3d_supported() raise before any launch (there is no silent fall-back to the torch form)."""
    r, b, cin = x.shape[0], x.shape[3], x.shape[4]
    k, cout = w.shape[0], w.shape[4]
    if not (x.shape[1] == r and x.shape[2] == r and w.shape[1] == k and w.shape[2] == k and w.shape[3] == cin
            and conv3d_supported(r, k, cin, cout)):
        raise _lib.PcopsError(
            "conv3d kernels: grid %s, kernel %s, Cin = %d, Cout = %d is outside what csrc/mfv.hip is built for (cubic grid "
            "R <= %d, k^3 with k in {3, 5}, Cin and Cout multiples of 16 up to 512); PCOPS_MFV_NATIVE=0 selects the torch "
            "form" % (tuple(x.shape[:3]), tuple(w.shape[:3]), cin, cout, CONV_MAX_R))
    x = _lib.check(x, torch.float32, "x", 5)
    y = Conv3dFn.apply(x.view(r * r * r, b, cin), w.contiguous(), bias.contiguous(), r)
    return y.view(r, r, r, b, cout)


def conv3d_torch(x, w, bias):
    """the same convolution through F.conv3d: x (B,D,H,W,Cin) -> (B,D,H,W,Cout), stride 1, SAME (odd kernels)"""
    kd, kh, kw = w.shape[:3]
    y = F.conv3d(x.permute(0, 4, 1, 2, 3), w.permute(4, 3, 0, 1, 2), bias, padding=(kd // 2, kh // 2, kw // 2))
    return y.permute(0, 2, 3, 4, 1)
