"""PointNet with a per-point background mask -- mirror of `pointnet/models/pointnet_seg.py` (placeholder_inputs :15-21,
get_model :24-108, get_loss :111-134): the PointNet member of the BGA family.  The front end is `pointnet_cls.get_model`'s; the
mask branch runs conv6..9 through `seg_ops.conv2d_stack_point_cloud` (csrc/cloudpoint.hip on the GPU) and conv10 as a plain
conv2d -- the same variables on every route."""
import torch

from .. import fused_mlp
from ..graph import variable_scope
from ..dgcnn import tf_util      # the BN flavour of `pointnet/utils/tf_util.py` (see pointnet_cls.py)
from .seg_ops import conv2d_stack_point_cloud
from .tnet_ops import apply_feature_transform, ortho_regulariser
from .transform_nets import feature_transform_net, input_transform_net

NUM_CLASSES = 15
BACKGROUND_CLASS = -1


def placeholder_inputs(batch_size, num_point, device=None):
    pointclouds_pl = torch.zeros((batch_size, num_point, 3), dtype=torch.float32, device=device)
    labels_pl = torch.zeros((batch_size,), dtype=torch.int32, device=device)
    mask_pl = torch.zeros((batch_size, num_point), dtype=torch.int32, device=device)
    return pointclouds_pl, labels_pl, mask_pl


def get_model(point_cloud, is_training, bn_decay=None):
    """point_cloud (B,N,3) -> class_pred (B,15), seg_pred (B,N,2), end_points {'transform': (B,64,64)}"""
    batch_size, num_point = point_cloud.shape[0], point_cloud.shape[1]
    end_points = {}
    with variable_scope('transform_net1'):
        transform = input_transform_net(point_cloud, is_training, bn_decay, K=3)
    fused = point_cloud.is_cuda and tf_util.fused_ok(point_cloud, [64, 128, 1024])
    input_image = tf_util.apply_transform(point_cloud, transform).unsqueeze(-1)  # (B,N,3,1); pcops_transform3 on the GPU
    net = tf_util.conv2d(input_image, 64, [1, 3], padding='VALID', stride=[1, 1], bn=True,
                         is_training=is_training, scope='conv1', bn_decay=bn_decay)
    if fused:
        net = tf_util.conv2d_stack(net, [64], ['conv2'], is_training, bn_decay)
    else:
        net = tf_util.conv2d(net, 64, [1, 1], padding='VALID', stride=[1, 1], bn=True,
                             is_training=is_training, scope='conv2', bn_decay=bn_decay)
    with variable_scope('transform_net2'):
        transform = feature_transform_net(net, is_training, bn_decay, K=64)
    end_points['transform'] = transform
    point_feat = apply_feature_transform(net.squeeze(2), transform).unsqueeze(2)    # feeds conv3 AND the head below
    if fused:
        # conv3..5 + maxpool as one fused stack: the (B, N, 1024) activation never exists
        global_feat = tf_util.conv2d_stack_global_max(point_feat, [64, 128, 1024], ['conv3', 'conv4', 'conv5'], is_training,
                                                      bn_decay)
    else:
        net = point_feat
        for i, width in zip((3, 4, 5), (64, 128, 1024)):
            net = tf_util.conv2d(net, width, [1, 1], padding='VALID', stride=[1, 1], bn=True,
                                 is_training=is_training, scope='conv%d' % i, bn_decay=bn_decay)
        global_feat = tf_util.max_pool2d(net, [num_point, 1], padding='VALID', scope='maxpool')

    # branch for obj label
    net = global_feat.reshape(batch_size, -1)
    net = tf_util.fully_connected(net, 512, bn=True, is_training=is_training, scope='fc1', bn_decay=bn_decay)
    net = tf_util.dropout(net, keep_prob=0.7, is_training=is_training, scope='dp1')
    net = tf_util.fully_connected(net, 256, bn=True, is_training=is_training, scope='fc2', bn_decay=bn_decay)
    net = tf_util.dropout(net, keep_prob=0.7, is_training=is_training, scope='dp2')
    class_pred = tf_util.fully_connected(net, NUM_CLASSES, activation_fn=None, scope='fc3')

    # for mask segmentation
    # concat([point_feat, tiled global_feat]) -> conv6..9 without the concatenation (seg_ops: the 64-deep per-point product
    # inside the first layer's pass, the 1024 per-cloud channels as one row per cloud)
    net = conv2d_stack_point_cloud(point_feat, global_feat.reshape(batch_size, -1), [512, 256, 128, 128],
                                   ['conv6', 'conv7', 'conv8', 'conv9'], is_training, bn_decay)
    net = tf_util.conv2d(net, 2, [1, 1], padding='VALID', stride=[1, 1], activation_fn=None, scope='conv10')
    seg_pred = net.squeeze(2)   # BxNxC
    return class_pred, seg_pred, end_points


def _seg_loss(seg_pred, gt):
    """mean over the clouds of the mean over a cloud's points; every cloud has n points: the mean of all rows"""
    b, n, c = seg_pred.shape
    return fused_mlp.softmax_cross_entropy(seg_pred.reshape(b * n, c), gt.reshape(b * n))


def get_loss(class_pred, seg_pred, gt_label, gt_mask, end_points, seg_weight=0.5, reg_weight=0.001):
    """(1 - seg_weight) CE(class) + seg_weight CE(mask) + reg_weight * l2_loss(T T^T - I); returns (total, classify, seg)"""
    classify_loss = fused_mlp.softmax_cross_entropy(class_pred, gt_label)
    seg_loss = _seg_loss(seg_pred, gt_mask)
    mat_diff_loss = ortho_regulariser(end_points['transform'], reg_weight)
    total_loss = (1 - seg_weight) * classify_loss + seg_weight * seg_loss + mat_diff_loss
    return total_loss, classify_loss, seg_loss
