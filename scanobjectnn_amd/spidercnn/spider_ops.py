"""SpiderConv on libpcops (csrc/spider.hip): one autograd Function per layer -- Taylor weights, the contraction over
(neighbour, channel, Taylor channel), group norm and ReLU.  The expanded operand A[p,(j,c,t)] = F[idx[p,j],c] g[p,j,t]
of the reference (SpiderCNN/utils/tf_util.py:219-223) exists only tile by tile in LDS; the Function saves F, idx,
delta, g, the pre-norm output and its statistics."""
import torch

from .. import _lib

TAYLOR_CHANNELS = 5


def _ws(nbytes, dev):
    return torch.empty(max(int(nbytes), 4) // 4 + 1, dtype=torch.float32, device=dev)


def taylor_fwd(delta, theta, tbias):
    """delta (B,N,k,3), theta (19,T), tbias (T) -> g (B,N,k,T)"""
    b, n, k, _ = delta.shape
    t = theta.shape[1]
    g = torch.empty((b, n, k, t), dtype=torch.float32, device=delta.device)
    _lib.call("pcops_spider_taylor_fwd", b * n * k, t, delta.data_ptr(), theta.data_ptr(), tbias.data_ptr(),
              g.data_ptr())
    return g


def taylor_bwd(delta, dg):
    """-> dtheta (19,T), dtbias (T), summed in a fixed order"""
    rows, t = delta.numel() // 3, dg.shape[-1]
    dtheta = torch.empty((19, t), dtype=torch.float32, device=dg.device)
    dtbias = torch.empty(t, dtype=torch.float32, device=dg.device)
    ws = _ws(_lib.load().pcops_spider_taylor_bwd_workspace_bytes(rows, t), dg.device)
    _lib.call("pcops_spider_taylor_bwd", rows, t, delta.data_ptr(), dg.data_ptr(), dtheta.data_ptr(), dtbias.data_ptr(),
              ws.data_ptr())
    return dtheta, dtbias


def conv_fwd(feat, idx, g, w, bias):
    """feat (B,N,C), idx (B,N,k), g (B,N,k,T), w (k C T, O), bias (O) -> y (B,N,O)"""
    b, n, c = feat.shape
    k, t, o = idx.shape[2], g.shape[3], w.shape[1]
    y = torch.empty((b, n, o), dtype=torch.float32, device=feat.device)
    _lib.call("pcops_spider_conv_fwd", b, n, c, k, t, o, feat.data_ptr(), idx.data_ptr(), g.data_ptr(), w.data_ptr(),
              _lib.ptr(bias), y.data_ptr())
    return y


def conv_wgrad(feat, idx, g, dy):
    """-> dw (k C T, O), dbias (O)"""
    b, n, c = feat.shape
    k, t, o = idx.shape[2], g.shape[3], dy.shape[2]
    dw = torch.empty((k * c * t, o), dtype=torch.float32, device=dy.device)
    db = torch.empty(o, dtype=torch.float32, device=dy.device)
    ws = _ws(_lib.load().pcops_spider_conv_wgrad_workspace_bytes(b, n, c, k, t, o), dy.device)
    _lib.call("pcops_spider_conv_wgrad", b, n, c, k, t, o, feat.data_ptr(), idx.data_ptr(), g.data_ptr(), dy.data_ptr(),
              dw.data_ptr(), db.data_ptr(), ws.data_ptr())
    return dw, db


def conv_dgrad(feat, idx, g, w, dy, need_dfeat=True):
    """-> dfeat_grouped (B,N,k,C) or None, dg (B,N,k,T)"""
    b, n, c = feat.shape
    k, t, o = idx.shape[2], g.shape[3], w.shape[1]
    dfg = torch.empty((b, n, k, c), dtype=torch.float32, device=dy.device) if need_dfeat else None
    dg = torch.empty((b, n, k, t), dtype=torch.float32, device=dy.device)
    _lib.call("pcops_spider_conv_dgrad", b, n, c, k, t, o, feat.data_ptr(), idx.data_ptr(), g.data_ptr(), w.data_ptr(),
              dy.data_ptr(), _lib.ptr(dfg), dg.data_ptr())
    return dfg, dg


def group_norm_relu_fwd(x, gamma, beta, groups, eps=1e-6):
    """x (B,N,C) -> relu(group_norm(x)), mean (B,G), rstd (B,G)"""
    b, n, c = x.shape
    y = torch.empty_like(x)
    mean = torch.empty((b, groups), dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    _lib.call("pcops_group_norm_relu_fwd", b, n, c, groups, eps, x.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
              y.data_ptr(), mean.data_ptr(), rstd.data_ptr())
    return y, mean, rstd


def group_norm_relu_bwd(dout, x, y, gamma, mean, rstd, groups):
    """-> dx (B,N,C), dgamma (C), dbeta (C)"""
    b, n, c = x.shape
    dx = torch.empty_like(x)
    dgamma = torch.empty(c, dtype=torch.float32, device=x.device)
    dbeta = torch.empty_like(dgamma)
    ws = _ws(_lib.load().pcops_group_norm_relu_workspace_bytes(b, c), x.device)
    _lib.call("pcops_group_norm_relu_bwd", b, n, c, groups, dout.data_ptr(), x.data_ptr(), y.data_ptr(),
              gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
              ws.data_ptr())
    return dx, dgamma, dbeta


scatter_grouped = _lib.scatter_grouped      # (dfeat_grouped (B,N,k,C), idx, n) -> dfeat (B,N,C); shared with X-Conv


class SpiderConvFn(torch.autograd.Function):
    """(feat, idx, delta, theta (19,T), tbias (T), w (k C T, O), bias (O), gamma (O), beta (O)) -> (B,N,O)"""

    @staticmethod
    def forward(ctx, feat, idx, delta, theta, tbias, w, bias, gamma, beta, groups, eps):
        g = taylor_fwd(delta, theta, tbias)
        y = conv_fwd(feat, idx, g, w, bias)
        out, mean, rstd = group_norm_relu_fwd(y, gamma, beta, groups, eps)
        ctx.save_for_backward(feat, idx, delta, g, w, gamma, y, out, mean, rstd)
        ctx.groups = groups
        ctx.need_dfeat = ctx.needs_input_grad[0]
        return out

    @staticmethod
    def backward(ctx, dout):
        feat, idx, delta, g, w, gamma, y, out, mean, rstd = ctx.saved_tensors
        dy, dgamma, dbeta = group_norm_relu_bwd(dout.contiguous(), y, out, gamma, mean, rstd, ctx.groups)
        dw, dbias = conv_wgrad(feat, idx, g, dy)
        dfg, dg = conv_dgrad(feat, idx, g, w, dy, need_dfeat=ctx.need_dfeat)
        dtheta, dtbias = taylor_bwd(delta, dg)
        dfeat = scatter_grouped(dfg, idx, feat.shape[1]) if dfg is not None else None
        return dfeat, None, None, dtheta, dtbias, dw, dbias, dgamma, dbeta, None, None


def supported(c, k, t, o, groups):
    """the shapes csrc/spider.hip is built for (include/pcops.h "SpiderConv")"""
    return 1 <= k <= 64 and t == TAYLOR_CHANNELS and 1 <= c <= 256 and o % 16 == 0 and 16 <= o <= 512 and \
        groups > 0 and o % groups == 0 and o // groups <= 256


def spider_conv(feat, idx, delta, theta, tbias, w, bias, gamma, beta, groups, eps=1e-6):
    """One SpiderConv layer with group norm and ReLU on the native kernels; all tensors on the MI355X.  Shapes outside
    supported() raise before any launch (there is no silent fall-back to the torch form)."""
    c, k, t, o = feat.shape[-1], idx.shape[-1], theta.shape[-1], w.shape[-1]
    if not supported(c, k, t, o, groups):
        raise _lib.PcopsError(
            "SpiderConv kernels: C = %d, k = %d, T = %d, O = %d, %d groups is outside what csrc/spider.hip is built for "
            "(1 <= C <= 256, 1 <= k <= 64, T = 5, O %% 16 == 0 and 16 <= O <= 512, O / groups <= 256); "
            "PCOPS_SPIDER_NATIVE=0 selects the dense torch form" % (c, k, t, o, groups))
    feat = _lib.check(feat, torch.float32, "feat", 3)
    idx = _lib.check(idx, torch.int32, "idx", 3)
    delta = _lib.check(delta, torch.float32, "delta", 4)
    theta, tbias, w = theta.contiguous(), tbias.contiguous(), w.contiguous()
    return SpiderConvFn.apply(feat, idx, delta, theta, tbias, w, bias.contiguous(), gamma.contiguous(),
                              beta.contiguous(), int(groups), float(eps))
