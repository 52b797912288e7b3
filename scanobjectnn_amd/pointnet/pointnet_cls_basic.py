"""PointNet without the T-Nets -- mirror of `pointnet/models/pointnet_cls_basic.py` (get_model :17-60, get_loss :63-69):
conv1..5, the max over the points, fc1, fc2, dp1, fc3 and plain cross-entropy.

The reference hard-codes 40 outputs (ModelNet40) and takes no `num_class`, so its own ScanObjectNN trainer cannot call it;
here `get_model` takes `num_class=15` like its sibling `pointnet_cls`.

On the GPU conv2..5 and the max run as fused conv stacks (the (B, N, 1024) activation never exists); on the CPU layer by
layer -- the same variables either way."""
import torch

from .. import fused_mlp
from ..dgcnn import tf_util      # the `tf.nn.moments` + EMA batch-norm flavour, as in pointnet_cls

NUM_CLASSES = 15


def placeholder_inputs(batch_size, num_point, device=None):
    pointclouds_pl = torch.zeros((batch_size, num_point, 3), dtype=torch.float32, device=device)
    labels_pl = torch.zeros((batch_size,), dtype=torch.int32, device=device)
    return pointclouds_pl, labels_pl


def get_model(point_cloud, is_training, bn_decay=None, num_class=NUM_CLASSES):
    """point_cloud (B,N,3) -> logits (B,num_class), end_points {}"""
    batch_size, num_point = point_cloud.shape[0], point_cloud.shape[1]
    end_points = {}
    input_image = point_cloud.unsqueeze(-1)                                    # (B,N,3,1)
    # conv1 is a [1, 3] kernel over the coordinates (weights [1, 3, 1, 64]): a dense layer in front of the fused stack
    net = tf_util.conv2d(input_image, 64, [1, 3], padding='VALID', stride=[1, 1], bn=True,
                         is_training=is_training, scope='conv1', bn_decay=bn_decay)
    widths, scopes = [64, 64, 128, 1024], ['conv2', 'conv3', 'conv4', 'conv5']
    if point_cloud.is_cuda and tf_util.fused_ok(net, widths):
        net = tf_util.conv2d_stack_global_max(net, widths, scopes, is_training, bn_decay)
    else:
        for width, scope in zip(widths, scopes):
            net = tf_util.conv2d(net, width, [1, 1], padding='VALID', stride=[1, 1], bn=True,
                                 is_training=is_training, scope=scope, bn_decay=bn_decay)
        net = tf_util.max_pool2d(net, [num_point, 1], padding='VALID', scope='maxpool')
    net = net.reshape(batch_size, -1)
    net = tf_util.fully_connected(net, 512, bn=True, is_training=is_training, scope='fc1', bn_decay=bn_decay)
    net = tf_util.fully_connected(net, 256, bn=True, is_training=is_training, scope='fc2', bn_decay=bn_decay)
    net = tf_util.dropout(net, keep_prob=0.7, is_training=is_training, scope='dp1')
    net = tf_util.fully_connected(net, num_class, activation_fn=None, scope='fc3')
    return net, end_points


def get_loss(pred, label, end_points=None):
    """mean softmax cross-entropy; on the GPU one launch per direction (pcops_softmax_ce)"""
    return fused_mlp.softmax_cross_entropy(pred, label)
