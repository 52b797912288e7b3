"""The X-Conv contraction on libpcops (csrc/xconv.hip): gather + concat + X-transform + the depthwise (1, K) filter of one
X-Conv layer as one autograd Function.  With Fin[q,k,:] = concat(lifted[q,k,:], fts[idx[q,k],:]):

    out[b, p, ch dm + m] = sum_k' wd[k',ch,m] sum_k X[b,p,k',k] Fin[b,p,k,ch]

Neither Fin nor X Fin exists in memory on the native route; the Function saves its five inputs only.
PCOPS_XCONV_NATIVE=0 selects `xconv_torch`, the dense torch form -- the comparison form, and the only one that runs off
the GPU."""
import os

import torch

from .. import _lib


def native_enabled():
    """PCOPS_XCONV_NATIVE=0: the dense torch form; read at every layer build"""
    return os.environ.get("PCOPS_XCONV_NATIVE", "1") != "0"


def gather_rows(x, idx):
    """x (B,N,C), idx (B,P,K) -> x[b, idx[b,p,k], :] (B,P,K,C)"""
    b = x.shape[0]
    return x[torch.arange(b, device=x.device).view(b, 1, 1), idx.long()]


def xconv_torch(lifted, fts, idx, X, wd):
    """lifted (B,P,K,c1), fts (B,N,c2) or None, idx (B,P,K), X (B,P,K,K), wd (K,c,dm) -> (B,P,c dm), any device / dtype"""
    fin = lifted if fts is None else torch.cat([lifted, gather_rows(fts, idx)], dim=-1)
    t = torch.matmul(X, fin)                                              # (B,P,K,c): fts_X of the reference
    b, p = t.shape[:2]
    return torch.einsum('bpkc,kcm->bpcm', t, wd).reshape(b, p, -1)        # TF's depthwise order c * dm + m


def _dims(lifted, fts, X, wd):
    b, p, k, c1 = lifted.shape
    c2 = 0 if fts is None else fts.shape[2]
    n = p if fts is None else fts.shape[1]
    return b, n, p, k, c1, c2, wd.shape[2]


def fwd(lifted, fts, idx, X, wd):
    dims = _dims(lifted, fts, X, wd)
    b, _, p, _, c1, c2, dm = dims
    out = torch.empty((b, p, (c1 + c2) * dm), dtype=torch.float32, device=lifted.device)
    _lib.call("pcops_xconv_fwd", *dims, lifted.data_ptr(), _lib.ptr(fts), _lib.ptr(idx), X.data_ptr(), wd.data_ptr(),
              out.data_ptr())
    return out


def dgrad(lifted, fts, idx, X, wd, dout, need_dfts=True):
    """-> dX (B,P,K,K), dlifted (B,P,K,c1), dfts_grouped (B,P,K,c2) or None; a layer of more than 256 channels runs in
    pcops_xconv_channel_groups groups whose partial dX sums meet in a workspace (PCOPS_XCONV_GROUPS=0: one group)"""
    dims = _dims(lifted, fts, X, wd)
    b, _, p, k, c1, c2, _ = dims
    dX, dl = torch.empty_like(X), torch.empty_like(lifted)
    dfg = torch.empty((b, p, k, c2), dtype=torch.float32, device=X.device) if need_dfts and c2 else None
    nbytes = int(_lib.load().pcops_xconv_dgrad_workspace_bytes(*dims))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=X.device) if nbytes else None
    _lib.call("pcops_xconv_dgrad_ws", *dims, lifted.data_ptr(), _lib.ptr(fts), _lib.ptr(idx), X.data_ptr(), wd.data_ptr(),
              dout.data_ptr(), dX.data_ptr(), dl.data_ptr(), _lib.ptr(dfg), _lib.ptr(ws))
    return dX, dl, dfg


def wgrad(lifted, fts, idx, X, wd, dout):
    """-> dwd (K,c,dm), the same bits on every call"""
    dims = _dims(lifted, fts, X, wd)
    dwd = torch.empty_like(wd)
    nbytes = int(_lib.load().pcops_xconv_wgrad_workspace_bytes(*dims))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=X.device) if nbytes else None
    _lib.call("pcops_xconv_wgrad", *dims, lifted.data_ptr(), _lib.ptr(fts), _lib.ptr(idx), X.data_ptr(), dout.data_ptr(),
              dwd.data_ptr(), _lib.ptr(ws))
    return dwd


class XConvFn(torch.autograd.Function):
    """(lifted, fts | None, idx | None, X, wd) -> (B,P,c dm)"""

    @staticmethod
    def forward(ctx, lifted, fts, idx, X, wd):
        ctx.save_for_backward(lifted, fts, idx, X, wd)
        return fwd(lifted, fts, idx, X, wd)

    @staticmethod
    def backward(ctx, dout):
        lifted, fts, idx, X, wd = ctx.saved_tensors
        need = ctx.needs_input_grad
        dout = dout.contiguous()
        dX = dl = dfts = dwd = None
        if need[4]:
            dwd = wgrad(lifted, fts, idx, X, wd, dout)
        if need[0] or need[1] or need[3]:
            dX, dl, dfg = dgrad(lifted, fts, idx, X, wd, dout, need_dfts=need[1])
            if dfg is not None:
                dfts = _lib.scatter_grouped(dfg, idx, fts.shape[1])
        return (dl if need[0] else None), dfts, None, (dX if need[3] else None), dwd


def supported(k, c1, c2, dm):
    """pcops_xconv_supported: the shapes csrc/xconv.hip is built for (include/pcops.h "X-Conv contraction")"""
    return bool(_lib.load().pcops_xconv_supported(int(k), int(c1), int(c2), int(dm)))


def xconv_contract(lifted, fts, idx, X, wd):
    """The contraction of one X-Conv layer.  Native unless PCOPS_XCONV_NATIVE=0; a shape outside supported() raises
    before any launch -- there is no silent fall-back to the torch form."""
    if not native_enabled():
        return xconv_torch(lifted, fts, idx, X, wd)
    k, c1, dm = lifted.shape[2], lifted.shape[3], wd.shape[2]
    c2 = 0 if fts is None else fts.shape[2]
    if not supported(k, c1, c2, dm):
        raise _lib.PcopsError(
            "X-Conv kernels: K = %d, c1 = %d, c2 = %d, depth multiplier %d is outside what csrc/xconv.hip is built for "
            "(1 <= K <= 16, c1 >= 1, 1 <= dm <= 4, (c1 + c2) dm <= 960); PCOPS_XCONV_NATIVE=0 selects the dense torch form"
            % (k, c1, c2, dm))
    lifted = _lib.check(lifted, torch.float32, "lifted", 4)
    X = _lib.check(X, torch.float32, "X", 4)
    wd = _lib.check(wd, torch.float32, "wd", 3)
    if fts is not None:
        fts = _lib.check(fts, torch.float32, "fts", 3)
        idx = _lib.check(idx, torch.int32, "idx", 3)
    else:
        idx = None
    return XConvFn.apply(lifted, fts, idx, X, wd)
