"""3DmFV-Net layers -- mirror of `3DmFV-Net/utils/tf_util.py`: get_3dmfv (:578-652), conv3d (:254-311), max_pool3d
(:406-429), avg_pool3d (:432-455), fully_connected (:314-351), dropout (:554-575), with the reference's signatures and
variable names (`weights`, `biases`, `bn/beta`, `bn/gamma`; the moving statistics as `bn/moving_mean`, `bn/moving_variance`).
Batch norm is the EMA / tf.nn.moments flavour of `dgcnn/tf_util.py` (:458-495 is the same template): biased variance,
eps 1e-3.

Every layer takes and returns the reference's logical shape (B, D, H, W, C).  The trunk's activations are kept VOXEL-MAJOR
in memory -- (D, H, W, B, C) contiguous, handed on as a permuted view -- so that the k^3 convolutions see the B rows of a
voxel as one contiguous tile (mfv_ops.py) and no transpose sits between two layers; a tensor in any other layout is
rearranged once on entry.

PCOPS_MFV_NATIVE=0 selects the torch forms (broadcast algebra, F.conv3d, torch batch norm): the A/B baseline, any device."""
import torch
import torch.nn.functional as F

from .. import fused_mlp
from ..dgcnn import tf_util as _dg
from ..graph import constant_initializer, get_variable, variable_scope
from ..pointnet2.tf_util import _dense, _variable_with_weight_decay, dropout, relu  # noqa: F401
from . import mfv_ops
from .mfv_ops import native_enabled  # noqa: F401

BN_EPS = _dg.BN_EPS


def voxel_major(x):
    """(B,D,H,W,C) in any layout -> (D,H,W,B,C) contiguous; free when x already is a voxel-major view"""
    return x.permute(1, 2, 3, 0, 4).contiguous()


def from_voxel_major(xm):
    """(D,H,W,B,C) contiguous -> the logical (B,D,H,W,C) view of it"""
    return xm.permute(3, 0, 1, 2, 4)


def concat(values, axis=4):
    """tf.concat over the channel axis of (B,D,H,W,C) tensors, result voxel-major"""
    if axis not in (4, -1):
        return torch.cat(values, dim=axis)
    return from_voxel_major(torch.cat([voxel_major(v) for v in values], dim=4))


def _native(x):
    return native_enabled() and x.is_cuda and x.dtype == torch.float32


def get_3dmfv(points, w, mu, sigma, flatten=True):
    """points (B,N,3), w (K), mu (K,3), sigma (K,3) standard deviations -> the 3DmFV representation: (B, 20 K) with
    flatten, else (B,20,K), rows d_pi max, sum; d_mu max xyz, min xyz, sum xyz; d_sigma max xyz, min xyz, sum xyz.
    No gradient flows into any argument (data and constants in the reference).  On the native path one pass of
    pcops_fv3d_fwd with nothing of size N K in memory; with flatten=False the result is a view of the voxel-major
    (K,B,20) buffer, so the model's reshape + transpose to (B,res,res,res,20) costs nothing."""
    if native_enabled() and points.is_cuda:
        if flatten:
            return mfv_ops.fv3d(points, w, mu, sigma).reshape(points.shape[0], -1)
        return mfv_ops.fv3d(points, w, mu, sigma, voxel_major=True).permute(1, 2, 0)
    with torch.no_grad():
        fv = mfv_ops.fv3d_torch(points, w.to(points), mu.to(points), sigma.to(points))
    return fv.reshape(points.shape[0], -1) if flatten else fv


def _bn_relu_rows(rows, c, is_training, bn_decay, activation_fn):
    """batch norm (scope 'bn') + activation over (rows, C).  Native: pcops_fc_bn_fwd / _bwd (csrc/head.hip), one launch
    per direction, up to fused_mlp.FC_BN_MAX_ROWS rows; beyond that, and in the torch form, dgcnn/tf_util's batch norm."""
    if _native(rows) and activation_fn in (relu, None) and fused_mlp.fc_batch_norm_supported(rows):
        with variable_scope('bn'):
            beta = get_variable('beta', [c], constant_initializer(0.0))
            gamma = get_variable('gamma', [c], constant_initializer(1.0))
            mov_mean = get_variable('moving_mean', [c], constant_initializer(0.0), trainable=False)
            mov_var = get_variable('moving_variance', [c], constant_initializer(1.0), trainable=False)
        decay = float(bn_decay) if bn_decay is not None else 0.9
        return fused_mlp.fc_batch_norm(rows, gamma, beta, mov_mean, mov_var, is_training, decay, BN_EPS, False,
                                       activation_fn is relu)
    out = _dg._bn(rows, is_training, bn_decay, 'bn', False)
    return activation_fn(out) if activation_fn is not None else out


def conv3d(inputs, num_output_channels, kernel_size, scope, stride=[1, 1, 1], padding='SAME', use_xavier=True,
           stddev=1e-3, weight_decay=0.0, activation_fn=relu, bn=False, bn_decay=None, is_training=None):
    """tf_util.py:254-311.  inputs (B,D,H,W,C); stride 1, SAME.  [1,1,1] kernels with bn + relu run as one fused MLP stack
    over the flattened rows (fused_mlp.mlp_stack, the path of conv2d_stack); k^3 kernels run on pcops_conv3d_fwd / _dgrad /
    _wgrad (cubic grids up to 8^3, k in {3, 5}, channels multiples of 16 up to 512 -- anything else raises) followed by the
    layer's batch norm + ReLU (_bn_relu_rows)."""
    if list(stride) != [1, 1, 1] or padding != 'SAME':
        raise NotImplementedError("conv3d: only stride [1,1,1] with SAME padding is used by the model")
    kd, kh, kw = kernel_size
    with variable_scope(scope):
        b, d, h, w_, cin = inputs.shape
        cout = num_output_channels
        kernel = _variable_with_weight_decay('weights', [kd, kh, kw, cin, cout], stddev=stddev,
                                             wd=weight_decay or None, use_xavier=use_xavier)
        biases = get_variable('biases', [cout], constant_initializer(0.0))
        native = _native(inputs)
        if (kd, kh, kw) == (1, 1, 1):
            xm = voxel_major(inputs)
            rows = xm.view(-1, cin)
            if native and bn and activation_fn is relu and fused_mlp.fused_supported(rows, [cout], True, True):
                with variable_scope('bn'):
                    beta = get_variable('beta', [cout], constant_initializer(0.0))
                    gamma = get_variable('gamma', [cout], constant_initializer(1.0))
                    mm = get_variable('moving_mean', [cout], constant_initializer(0.0), trainable=False)
                    mv = get_variable('moving_variance', [cout], constant_initializer(1.0), trainable=False)
                decay = bn_decay if bn_decay is not None else 0.9
                out = fused_mlp.mlp_stack(rows, 1, False, is_training, decay, BN_EPS, False,
                                          [(kernel.view(cin, cout), biases, gamma, beta, mm, mv)])
                return from_voxel_major(out.view(d, h, w_, b, cout))
            out = _dense(rows, kernel.view(cin, cout), biases)
        elif native:
            out = mfv_ops.conv3d(voxel_major(inputs), kernel, biases).view(-1, cout)
        else:
            out = voxel_major(mfv_ops.conv3d_torch(inputs, kernel, biases)).view(-1, cout)
        if bn:
            out = _bn_relu_rows(out, cout, is_training, bn_decay, activation_fn)
        elif activation_fn is not None:
            out = activation_fn(out)
        return from_voxel_major(out.view(d, h, w_, b, cout))


def fully_connected(inputs, num_outputs, scope, use_xavier=True, stddev=1e-3, weigth_decay=0.0, activation_fn=relu,
                    bn=False, bn_decay=None, is_training=None):
    """tf_util.py:314-351 (the reference spells the keyword `weigth_decay`): the fused FC + BN head of dgcnn/tf_util.py"""
    return _dg.fully_connected(inputs, num_outputs, scope, use_xavier=use_xavier, stddev=stddev,
                               weight_decay=weigth_decay, activation_fn=activation_fn, bn=bn, bn_decay=bn_decay,
                               is_training=is_training)


def _pool_view(inputs):
    """(B,D,H,W,C) -> (1, B C, D, H, W) over the voxel-major buffer (channels-last for torch's pooling)"""
    b, d, h, w_, c = inputs.shape
    return voxel_major(inputs).view(d, h, w_, b * c).permute(3, 0, 1, 2).unsqueeze(0)


def _pool_result(out, b, c):
    _, _, d, h, w_ = out.shape
    return from_voxel_major(out.squeeze(0).permute(1, 2, 3, 0).reshape(d, h, w_, b, c))


def max_pool3d(inputs, kernel_size, scope, stride=[2, 2, 2], padding='VALID'):
    """tf_util.py:406-429.  TF's SAME pads AFTER the data when the padding is odd (5 -> 3 with windows {0,1} {2,3} {4},
    3 -> 2): torch's ceil_mode, which lets the last window run off the end."""
    if list(kernel_size) != list(stride):
        raise NotImplementedError("max_pool3d: only kernel_size == stride is used by the model")
    with variable_scope(scope):
        b, c = inputs.shape[0], inputs.shape[4]
        out = F.max_pool3d(_pool_view(inputs), tuple(kernel_size), tuple(stride), ceil_mode=(padding == 'SAME'))
        return _pool_result(out, b, c)


def avg_pool3d(inputs, kernel_size, scope, stride=[2, 2, 2], padding='VALID'):
    """tf_util.py:432-455.  TF's SAME average divides by the number of IN-GRID elements of the window
    (count_include_pad=False)."""
    with variable_scope(scope):
        b, c = inputs.shape[0], inputs.shape[4]
        if padding == 'SAME':
            if list(stride) != [1, 1, 1] or any(k % 2 == 0 for k in kernel_size):
                raise NotImplementedError("avg_pool3d SAME: only odd kernels with stride 1 are used by the model")
            # window sums over the zero-padded grid divided by the in-grid count (torch's own padded pooling refuses a
            # grid smaller than the kernel: the 2^3 grid behind the first max pool of the 27-Gaussian model)
            x = _pool_view(inputs)
            pad = [k // 2 for k in reversed(kernel_size) for _ in (0, 1)]
            ones = torch.ones((1, 1) + tuple(x.shape[2:]), dtype=x.dtype, device=x.device)
            count = F.avg_pool3d(F.pad(ones, pad), tuple(kernel_size), 1, divisor_override=1)
            out = F.avg_pool3d(F.pad(x, pad), tuple(kernel_size), 1, divisor_override=1) / count
        else:
            out = F.avg_pool3d(_pool_view(inputs), tuple(kernel_size), tuple(stride))
        return _pool_result(out, b, c)
