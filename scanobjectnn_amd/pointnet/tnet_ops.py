"""PointNet's learned feature transform and its regulariser on libpcops (csrc/tnet.hip).

`apply_feature_transform(net, transform)` is `tf.matmul(net, transform)` of pointnet/models/pointnet_cls.py:47 -- (B, N, K)
features times a DIFFERENT (K, K) matrix per cloud -- and `ortho_regulariser(transform, reg_weight)` is
`reg_weight * tf.nn.l2_loss(T T^T - I)` of :86-91.  Both run one launch per direction for CUDA fp32 tensors of a shape the
library supports (K = 64); anything else, and everything with PCOPS_POINTNET_NATIVE=0, is the torch expression."""
import os

import torch

from .. import _lib


def native_enabled():
    """PCOPS_POINTNET_NATIVE=0: the transform and the regulariser as the torch expressions; read at every call"""
    return os.environ.get("PCOPS_POINTNET_NATIVE", "1") != "0"


class _TransformK(torch.autograd.Function):
    """net (B, N, K) x transform (B, K, K) on pcops_transformk_fwd / _bwd.  The output is an ordinary tensor: it may feed any
    number of consumers, autograd adds their gradients before backward runs."""

    @staticmethod
    def forward(ctx, x, T):
        x, T = x.contiguous(), T.contiguous()
        b, n, k = x.shape
        out = torch.empty_like(x)
        _lib.call("pcops_transformk_fwd", b, n, k, x.data_ptr(), T.data_ptr(), out.data_ptr())
        ctx.save_for_backward(x, T)
        return out

    @staticmethod
    def backward(ctx, g):
        x, T = ctx.saved_tensors
        b, n, k = x.shape
        g = g.contiguous()
        dT = torch.empty_like(T)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        nbytes = int(_lib.load().pcops_transformk_workspace_bytes(b, n, k))
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device) if nbytes else None
        _lib.call("pcops_transformk_bwd", b, n, k, x.data_ptr(), T.data_ptr(), g.data_ptr(), _lib.ptr(dx), dT.data_ptr(),
                  _lib.ptr(ws))
        return dx, dT


class _OrthoReg(torch.autograd.Function):
    """transform (B, K, K) -> reg_weight * sum_b l2_loss(T_b T_b^T - I): loss and gradient from the one launch of
    pcops_ortho_reg; the B per-cloud parts are added by one `sum`"""

    @staticmethod
    def forward(ctx, T, weight):
        T = T.contiguous()
        b, k, _ = T.shape
        parts = torch.empty(b, dtype=torch.float32, device=T.device)
        dT = torch.empty_like(T)
        _lib.call("pcops_ortho_reg", b, k, T.data_ptr(), float(weight), parts.data_ptr(), dT.data_ptr())
        ctx.save_for_backward(dT)
        return parts.sum()

    @staticmethod
    def backward(ctx, g):
        (dT,) = ctx.saved_tensors
        return dT * g, None


def _native(x, k):
    return native_enabled() and x.is_cuda and x.dtype == torch.float32 and k == x.shape[-1]


def apply_feature_transform(net, transform):
    """tf.matmul(net, transform): net (B, N, K), transform (B, K, K) -> (B, N, K)"""
    if (net.dim() == 3 and transform.dim() == 3 and _native(net, transform.shape[-1]) and transform.is_cuda
            and transform.dtype == torch.float32 and tuple(transform.shape) == (net.shape[0], net.shape[2], net.shape[2])
            and _lib.load().pcops_transformk_supported(net.shape[0], net.shape[1], net.shape[2])):
        return _TransformK.apply(net, transform)
    return torch.matmul(net, transform)


def ortho_regulariser_torch(transform, reg_weight):
    k = transform.shape[1]
    mat_diff = torch.matmul(transform, transform.transpose(1, 2)) - torch.eye(k, device=transform.device, dtype=transform.dtype)
    return 0.5 * (mat_diff * mat_diff).sum() * reg_weight


def ortho_regulariser(transform, reg_weight):
    """reg_weight * l2_loss(T T^T - I) summed over the clouds (tf.nn.l2_loss = sum(x^2) / 2); transform (B, K, K)"""
    if (transform.dim() == 3 and transform.shape[1] == transform.shape[2] and _native(transform, transform.shape[1])
            and 1 <= transform.shape[0] <= 65535
            and _lib.load().pcops_transformk_supported(transform.shape[0], 1, transform.shape[1])):
        return _OrthoReg.apply(transform, reg_weight)
    return ortho_regulariser_torch(transform, reg_weight)
