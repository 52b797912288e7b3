"""PointCNN layers -- mirror of `PointCNN/pointfly.py`: dense :342, conv2d :332, depthwise_conv2d :318,
separable_conv2d :305, batch_normalization :298, knn_indices_general :163, get_xforms :75, augment :94.

Every layer is linear -> ELU -> batch norm, without a bias when a norm follows.  The norm is
tf.layers.batch_normalization(momentum=0.99, epsilon=1e-3) over every axis but the last.  Variables carry the names and
layouts TensorFlow gives them (`<name>/kernel`, `<name>/depthwise_weights`, `<name>/depthwise_kernel`,
`<name>/pointwise_kernel`, `<name>_bn/gamma`, ...), so tf_checkpoint.py round-trips them name for name.
Convolutions are the (1, K) VALID kernels over the neighbour axis X-Conv uses: inputs (B, P, K, C) -> (B, P, 1, C')."""
import torch
import torch.nn.functional as F

from ..graph import constant_initializer, get_variable, glorot_normal_initializer, variable_scope
from . import xconv_ops

elu = F.elu
BN_MOMENTUM = 0.99
BN_EPS = 1e-3


def batch_normalization(data, is_training, name):
    """Training: batch mean and biased variance.  The moving variance is fed the unbiased batch variance for 4-D inputs
    (TensorFlow takes its fused kernel there) and the biased one otherwise (an assumption)."""
    c = data.shape[-1]
    with variable_scope(name):
        gamma = get_variable('gamma', [c], constant_initializer(1.0))
        beta = get_variable('beta', [c], constant_initializer(0.0))
        moving_mean = get_variable('moving_mean', [c], constant_initializer(0.0), trainable=False)
        moving_var = get_variable('moving_variance', [c], constant_initializer(1.0), trainable=False)
    flat = data.reshape(-1, c)
    if is_training:
        var, mean = torch.var_mean(flat, dim=0, unbiased=False)
        rows = flat.shape[0]
        with torch.no_grad():
            bessel = rows / max(rows - 1, 1) if data.dim() == 4 else 1.0
            moving_mean.mul_(BN_MOMENTUM).add_(mean.detach(), alpha=1.0 - BN_MOMENTUM)
            moving_var.mul_(BN_MOMENTUM).add_(var.detach() * bessel, alpha=1.0 - BN_MOMENTUM)
    else:
        mean, var = moving_mean, moving_var
    scale = gamma * torch.rsqrt(var + BN_EPS)
    return (flat * scale + (beta - mean * scale)).reshape(data.shape)


def _finish(out, name, is_training, with_bn, activation):
    if activation is not None:
        out = activation(out)
    return batch_normalization(out, is_training, name + '_bn') if with_bn else out


def dense(input, output, name, is_training, with_bn=True, activation=elu):
    cin = input.shape[-1]
    with variable_scope(name):
        kernel = get_variable('kernel', [cin, output], glorot_normal_initializer())
        bias = None if with_bn else get_variable('bias', [output], constant_initializer(0.0))
    out = torch.matmul(input, kernel)
    if bias is not None:
        out = out + bias
    return _finish(out, name, is_training, with_bn, activation)


def _check_kernel(input, kernel_size):
    if tuple(kernel_size) != (1, input.shape[2]):
        raise NotImplementedError("pointfly: only the (1, K) VALID kernel over the K neighbours is mirrored, got %s on %s"
                                  % (tuple(kernel_size), tuple(input.shape)))


def conv2d(input, output, name, is_training, kernel_size, with_bn=True, activation=elu):
    _check_kernel(input, kernel_size)
    b, p, k, cin = input.shape
    with variable_scope(name):
        kernel = get_variable('kernel', [1, k, cin, output], glorot_normal_initializer())
        bias = None if with_bn else get_variable('bias', [output], constant_initializer(0.0))
    out = torch.matmul(input.reshape(b, p, k * cin), kernel.reshape(k * cin, output)).view(b, p, 1, output)
    if bias is not None:
        out = out + bias
    return _finish(out, name, is_training, with_bn, activation)


def _depthwise(input, kernel):
    """input (B,P,K,C), kernel (1,K,C,dm) -> (B,P,1,C dm), output channel c * dm + m (TensorFlow's order)"""
    b, p, _, c = input.shape
    return torch.einsum('bpkc,kcm->bpcm', input, kernel[0]).reshape(b, p, 1, -1)


def depthwise_conv2d(input, depth_multiplier, name, is_training, kernel_size, with_bn=True, activation=elu):
    """tf.contrib.layers.separable_conv2d(num_outputs=None): the depthwise half alone, variable `depthwise_weights`"""
    _check_kernel(input, kernel_size)
    k, c = input.shape[2], input.shape[3]
    with variable_scope(name):
        kernel = get_variable('depthwise_weights', [1, k, c, depth_multiplier], glorot_normal_initializer())
        bias = None if with_bn else get_variable('biases', [c * depth_multiplier], constant_initializer(0.0))
    out = _depthwise(input, kernel)
    if bias is not None:
        out = out + bias
    return _finish(out, name, is_training, with_bn, activation)


def separable_conv2d_variables(name, k, channels, output, depth_multiplier, with_bn=True):
    """the variables of tf.layers.separable_conv2d with a (1, k) kernel: depthwise_kernel, pointwise_kernel, bias | None"""
    with variable_scope(name):
        dk = get_variable('depthwise_kernel', [1, k, channels, depth_multiplier], glorot_normal_initializer())
        pk = get_variable('pointwise_kernel', [1, 1, channels * depth_multiplier, output], glorot_normal_initializer())
        bias = None if with_bn else get_variable('bias', [output], constant_initializer(0.0))
    return dk, pk, bias


def pointwise_finish(mid, pk, bias, name, is_training, with_bn=True, activation=elu):
    """the pointwise half on the depthwise output mid (B, P, c dm), then bias | ELU and norm: (B, P, 1, output)"""
    out = torch.matmul(mid, pk.view(pk.shape[2], pk.shape[3])).unsqueeze(2)
    if bias is not None:
        out = out + bias
    return _finish(out, name, is_training, with_bn, activation)


def separable_conv2d(input, output, name, is_training, kernel_size, depth_multiplier=1, with_bn=True, activation=elu):
    """tf.layers.separable_conv2d: depthwise (1, K) then pointwise"""
    _check_kernel(input, kernel_size)
    dk, pk, bias = separable_conv2d_variables(name, input.shape[2], input.shape[3], output, depth_multiplier, with_bn)
    return pointwise_finish(_depthwise(input, dk).squeeze(2), pk, bias, name, is_training, with_bn, activation)


# ------------------------------------------------------------------------------------------------------------ neighbours
def knn_indices_general(queries, points, k, sort=True, unique=True):
    """queries (B,P,3), points (B,N,3) -> the k nearest points of every query, nearest first: (B,P,k) int32.
    `unique` has no effect, as in the reference (prepare_for_unique_top_k :142 discards its result).  The ranking is the
    difference form sum_c (p_c - q_c)^2 that pcops_knn_point pins, not the reference's r_A - 2 A B^T + r_B: the two differ
    only where distances tie to rounding.  Off the GPU, where only the comparison form
    (PCOPS_XCONV_NATIVE=0) runs, the same form is ranked in torch."""
    if xconv_ops.native_enabled() or queries.is_cuda:
        from ..pointnet2.tf_grouping import knn_point
        return knn_point(k, points.contiguous(), queries.contiguous())[1]
    d = sum((queries[:, :, None, c] - points[:, None, :, c]) ** 2 for c in range(points.shape[2]))
    return torch.topk(d, k, dim=2, largest=False, sorted=True).indices.int()


# ---------------------------------------------------------------------------------------------------------- augmentation
def _draw(param, method, num, generator, device, centre):
    """`num` draws of rotation_angle / scaling_factor (:53-72): 'u' uniform in centre +- param, 'g' a normal of standard
    deviation param clipped at three of them"""
    if isinstance(param, (list, tuple)):
        raise NotImplementedError("pointfly.get_xforms: a list of choices per axis is not mirrored")
    if method == 'u':
        return centre + float(param) * (2.0 * torch.rand(num, generator=generator, device=device) - 1.0)
    if method == 'g':
        g = torch.randn(num, generator=generator, device=device).clamp_(-3.0, 3.0)
        return centre + float(param) * g
    raise ValueError("pointfly.get_xforms: method %r" % (method,))


def rotation_matrices(rx, ry, rz):
    """euler2mat(rx, ry, rz, 'rxyz'): rotating axes x, then y, then z -- R = Rx(rx) Ry(ry) Rz(rz); (num, 3, 3)"""
    def rot(a, i, j):
        m = torch.eye(3, device=a.device, dtype=a.dtype).repeat(a.shape[0], 1, 1)
        m[:, i, i], m[:, j, j] = torch.cos(a), torch.cos(a)
        m[:, i, j], m[:, j, i] = -torch.sin(a), torch.sin(a)
        return m
    return rot(rx, 1, 2) @ rot(ry, 2, 0) @ rot(rz, 0, 1)


def get_xforms(xform_num, rotation_range=(0, 0, 0, 'u'), scaling_range=(0.0, 0.0, 0.0, 'u'), order='rxyz',
               generator=None, device=None):
    """-> xforms, rotations (xform_num, 3, 3).  The reference multiplies the scaling matrix diag(s) and the rotation
    ELEMENTWISE (`scaling * rotation` on NumPy arrays, :89), so the transform it applies is diag(s_i R_ii) -- a
    per-axis scaling by s_i R_ii, no rotation.  Restated as computed, not as intended."""
    if order != 'rxyz':
        raise NotImplementedError("pointfly.get_xforms: rotation order %r" % (order,))
    angles = [_draw(rotation_range[i], rotation_range[3], xform_num, generator, device, 0.0) for i in range(3)]
    rotations = rotation_matrices(*angles)
    scales = torch.stack([_draw(scaling_range[i], scaling_range[3], xform_num, generator, device, 1.0)
                          for i in range(3)], dim=1)
    return torch.diag_embed(scales) * rotations, rotations


def augment(points, xforms, range=None):
    """points (B,N,3) @ xforms (B,3,3), plus a clipped normal jitter of scale `range`; range None or 0.0 adds nothing"""
    out = torch.matmul(points, xforms)
    if not range:
        return out
    jitter = float(range) * torch.randn_like(out)
    return out + jitter.clamp_(-5 * float(range), 5 * float(range))

