"""The head PointNet's two segmentation models share (pointnet/models/pointnet_seg.py:81-100, pointnet_partseg.py:66-85): a
conv stack on concat([point_feat (B, N, 1, 64) | global feature tiled over the points (1024)]).

`conv2d_stack_point_cloud` evaluates it WITHOUT the concatenation.  The first conv is linear,
    [x_bn | c_b] W + bias = x_bn W_x + (c_b W_c + bias),        W = [W_x ; W_c], rows 0..63 / 64..1087
(the per-point rows come FIRST here -- the opposite of dgcnn_bga's head, dgcnn/tf_util.conv2d_stack_cloud_point), so the
per-cloud part is one (B, 1024) product and the per-point part is 64 deep.  Routes, in this order:
  1. `pcops_cloud_point_*` (csrc/cloudpoint.hip): the 64-deep product inside the first layer's streaming pass, forward and
     backward -- the (B N, 512) product and its gradient never exist.  PCOPS_CLOUD_POINT_FUSED=0 switches it off.
  2. Q = X W_x through `fused_mlp.rows_linear`, then the cloud-bias arm of the fused stack (the route of dgcnn_bga's head).
  3. where the fused stack does not take the shape, and on the CPU: the plain conv2d layers on the concatenation.
The variables are the ones `conv2d(..., scope=scopes[i])` creates on the 1088-wide input, whichever route runs."""
import torch

from .. import fused_mlp
from ..dgcnn import tf_util

# Rows (B N) from which route 1 is taken; below it route 2.  Measured (profiles/pointnet_seg_bench.txt):
# at B = 256, N = 2048 (524 288 rows) the step takes the same time on either route and 1.5 GB less memory on route 1; at
# B = 32, N = 1024 (32 768 rows) the step is 0.5 ms of 5.6 slower on route 1.  The bound is the geometric mean of the two sizes.
POINT_FUSED_MIN_ROWS = 131072


def stack_ok(per_point, widths):
    """the fused stack takes this head at all (routes 1 and 2)"""
    b, n = per_point.shape[0], per_point.shape[1]
    return (tf_util.fused_ok(per_point, widths) and b * n >= 8192 and n <= 16384 and per_point.shape[-1] % 4 == 0)


def point_fused(b, n, cx, c1):
    """route 1 runs for this shape: the switch, the size policy and the library's own predicate"""
    return b * n >= POINT_FUSED_MIN_ROWS and fused_mlp.cloud_point_fused_supported(b, n, cx, c1)


def conv2d_stack_point_cloud(per_point, per_cloud, widths, scopes, is_training, bn_decay):
    """len(widths) x conv2d([1,1], bn, relu) on concat([per_point | per_cloud broadcast over the points], -1).
    per_point (B, N, 1, Cx) | (B, N, Cx), per_cloud (B, Cc) -> (B, N, 1, widths[-1])"""
    b, n = per_point.shape[0], per_point.shape[1]
    cx, cc = per_point.shape[-1], per_cloud.shape[-1]
    per_cloud = per_cloud.reshape(b, cc)
    if not stack_ok(per_point, widths):
        net = torch.cat([per_point.reshape(b, n, 1, cx), per_cloud.view(b, 1, 1, cc).expand(b, n, 1, cc)], dim=-1)
        for width, scope in zip(widths, scopes):
            net = tf_util.conv2d(net, width, [1, 1], padding='VALID', stride=[1, 1], bn=True, is_training=is_training,
                                 scope=scope, bn_decay=bn_decay)
        return net
    layers = tf_util._pn2._stack_variables(cx + cc, widths, list(scopes), 1e-3, None, True, ('moving_mean', 'moving_variance'))
    w1, b1 = layers[0][0], layers[0][1]
    w_x, w_c = fused_mlp.split_rows(w1, cx)                 # (one concatenation as their gradient)
    ctr = fused_mlp.small_linear(per_cloud, w_c, b1).view(b, 1, widths[0])
    from ..pointnet2.pointnet_util import _whole_cloud_group
    _, idx = _whole_cloud_group(b, n, per_point.device)
    decay = bn_decay if bn_decay is not None else 0.9
    if point_fused(b, n, cx, widths[0]):
        out = fused_mlp.gather_mlp_stack(idx, False, is_training, decay, tf_util.BN_EPS, False, layers, Ctr=ctr,
                                         identity_idx=True, point=(per_point.reshape(b, n, cx), w_x))
    else:
        q = fused_mlp.rows_linear(per_point.reshape(b * n, cx), w_x).view(b, n, widths[0])
        out = fused_mlp.gather_mlp_stack(idx, False, is_training, decay, tf_util.BN_EPS, False, layers, Q=q, Ctr=ctr,
                                         identity_idx=True)
    return out.view(b, n, 1, widths[-1])
