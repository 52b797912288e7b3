"""3DmFV-Net classifier -- mirror of `3DmFV-Net/models/3dmfv_net_cls.py` (placeholder_inputs :13-26, get_model :29-84,
inception_module :86-102, get_loss :106-115).  The mixture is a constant of the model (`train.py:278-283` feeds it with
every batch): `model_fn` binds it, so that the trainer and the evaluation see the (point_cloud, is_training, bn_decay)
signature of the other families."""
import numpy as np
import torch
import torch.nn.functional as F

from .. import provider
from ..graph import get_default_graph
from . import tf_util
from .gmm import get_3d_grid_gmm


def placeholder_inputs(batch_size, n_points, gmm, device=None):
    """gmm: the (w, mu, sigma) triple of gmm.get_3d_grid_gmm -> points, labels, w, mu, sigma (zeros / the mixture)"""
    w, mu, sigma = gmm
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device=device)  # noqa: E731
    points = torch.zeros((batch_size, n_points, mu.shape[1]), dtype=torch.float32, device=device)
    labels = torch.zeros((batch_size,), dtype=torch.int32, device=device)
    return points, labels, t(w), t(mu), t(sigma)


def get_model(points, w, mu, sigma, is_training, bn_decay=None, weigth_decay=0.005, add_noise=False, num_classes=40):
    """points (B,N,3), the mixture w (K), mu (K,3), sigma (K,3) with K a cube -> (logits (B,num_classes), fv (B,20,K))"""
    batch_size = points.shape[0]
    n_gaussians = w.shape[0]
    res = int(np.round(np.power(n_gaussians, 1.0 / 3.0)))
    if res ** 3 != n_gaussians:
        raise ValueError("the classifier reads the %d Gaussians as a cubic grid; %d is no cube" % (n_gaussians, n_gaussians))

    fv = tf_util.get_3dmfv(points, w, mu, sigma, flatten=False)
    if add_noise and is_training:
        fv = fv + 0.01 * torch.randn_like(fv)

    grid_fisher = fv.reshape(batch_size, -1, res, res, res).permute(0, 2, 3, 4, 1)

    net = inception_module(grid_fisher, n_filters=64, kernel_sizes=[3, 5], is_training=is_training, bn_decay=bn_decay,
                           scope='inception1')
    net = inception_module(net, n_filters=128, kernel_sizes=[3, 5], is_training=is_training, bn_decay=bn_decay,
                           scope='inception2')
    net = inception_module(net, n_filters=256, kernel_sizes=[3, 5], is_training=is_training, bn_decay=bn_decay,
                           scope='inception3')
    net = tf_util.max_pool3d(net, [2, 2, 2], scope='maxpool4', stride=[2, 2, 2], padding='SAME')
    net = inception_module(net, n_filters=256, kernel_sizes=[3, 5], is_training=is_training, bn_decay=bn_decay,
                           scope='inception5')
    net = inception_module(net, n_filters=512, kernel_sizes=[3, 5], is_training=is_training, bn_decay=bn_decay,
                           scope='inception6')
    net = tf_util.max_pool3d(net, [2, 2, 2], scope='maxpool7', stride=[2, 2, 2], padding='SAME')

    net = net.reshape(batch_size, -1)

    net = tf_util.fully_connected(net, 1024, bn=True, is_training=is_training, scope='fc1', bn_decay=bn_decay,
                                  weigth_decay=weigth_decay)
    net = tf_util.dropout(net, keep_prob=0.7, is_training=is_training, scope='dp1')
    net = tf_util.fully_connected(net, 256, bn=True, is_training=is_training, scope='fc2', bn_decay=bn_decay,
                                  weigth_decay=weigth_decay)
    net = tf_util.dropout(net, keep_prob=0.7, is_training=is_training, scope='dp2')
    net = tf_util.fully_connected(net, 128, bn=True, is_training=is_training, scope='fc3', bn_decay=bn_decay,
                                  weigth_decay=weigth_decay)
    net = tf_util.dropout(net, keep_prob=0.7, is_training=is_training, scope='dp3')
    net = tf_util.fully_connected(net, num_classes, activation_fn=None, scope='fc4', is_training=is_training,
                                  weigth_decay=weigth_decay)
    return net, fv


def inception_module(input, n_filters=64, kernel_sizes=[3, 5], is_training=None, bn_decay=None, scope='inception'):
    one_by_one = tf_util.conv3d(input, n_filters, [1, 1, 1], scope=scope + '_conv1', stride=[1, 1, 1], padding='SAME',
                                bn=True, bn_decay=bn_decay, is_training=is_training)
    three_by_three = tf_util.conv3d(one_by_one, int(n_filters / 2), [kernel_sizes[0]] * 3, scope=scope + '_conv2',
                                    stride=[1, 1, 1], padding='SAME', bn=True, bn_decay=bn_decay, is_training=is_training)
    five_by_five = tf_util.conv3d(one_by_one, int(n_filters / 2), [kernel_sizes[1]] * 3, scope=scope + '_conv3',
                                  stride=[1, 1, 1], padding='SAME', bn=True, bn_decay=bn_decay, is_training=is_training)
    average_pooling = tf_util.avg_pool3d(input, [kernel_sizes[0]] * 3, scope=scope + '_avg_pool', stride=[1, 1, 1],
                                         padding='SAME')
    average_pooling = tf_util.conv3d(average_pooling, n_filters, [1, 1, 1], scope=scope + '_conv4', stride=[1, 1, 1],
                                     padding='SAME', bn=True, bn_decay=bn_decay, is_training=is_training)
    return tf_util.concat([one_by_one, three_by_three, five_by_five, average_pooling], axis=4)


def get_loss(pred, label, end_points=None):
    """mean sparse softmax cross entropy (:106-115).  The weight-decay terms that `_variable_with_weight_decay` collects
    are NOT part of it: the reference's train.py minimises get_loss(pred, labels) alone (:173-188), so --weight_decay
    changes nothing there, and nothing here."""
    return F.cross_entropy(pred, label.long())


def bind(gmm, device=None, weigth_decay=0.005):
    """-> get_model(point_cloud, is_training, bn_decay=None, num_class=15) with the mixture bound (what graph.Model takes)"""
    w, mu, sigma = (torch.as_tensor(np.asarray(a), dtype=torch.float32, device=device) for a in gmm)

    def bound(point_cloud, is_training, bn_decay=None, num_class=15):
        get_default_graph().end_points.pop("losses", None)      # this call's weight-decay terms only (collected, never added)
        return get_model(point_cloud[:, :, :3], w.to(point_cloud.device), mu.to(point_cloud.device),
                         sigma.to(point_cloud.device), is_training, bn_decay=bn_decay, weigth_decay=weigth_decay,
                         num_classes=num_class)
    return bound


def model_fn(args, device=None):
    """the classifier for the trainer's / the evaluation's flags: --num_gaussians (grid subdivisions per axis, 5),
    --gmm_variance (0.04), --gmm_type (grid), --weight_decay (0.0)"""
    gmm_type = getattr(args, "gmm_type", "grid")
    if gmm_type != "grid":
        raise NotImplementedError("--gmm_type %s: only the grid mixture is built; the learned (EM) mixture of the "
                                  "reference (utils.get_gmm) is out of scope" % gmm_type)
    n = int(getattr(args, "num_gaussians", 5))
    gmm = get_3d_grid_gmm([n, n, n], float(getattr(args, "gmm_variance", 0.04)))
    return bind(gmm, device=device, weigth_decay=float(getattr(args, "weight_decay", 0.0)))


# `augment` below as a recipe of the device-resident feed (device_feed.py, pcops_feed_batch): the same three steps and constants
DEVICE_FEED_RECIPE = {"recipe": 2, "smin": 0.66, "smax": 1.5, "tval": 0.2, "sigma": 0.01, "clip": 0.05}


def augment(batch, generator=None):
    """the model's training augmentation (3DmFV-Net/train.py:25,263-274): scale, translate, jitter -- no rotation"""
    batch = provider.scale_point_cloud(batch, smin=0.66, smax=1.5, generator=generator)
    batch = provider.translate_point_cloud(batch, tval=0.2, generator=generator)
    return provider.jitter_point_cloud(batch, sigma=0.01, clip=0.05, generator=generator)
