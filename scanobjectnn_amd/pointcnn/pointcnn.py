"""X-Conv and the PointCNN trunks -- mirror of `PointCNN/pointcnn.py` (xconv :10-52, PointCNN :55-159, PointCNN_SEG
:161-277, whose encoder loop is the classifier's and is shared here).

The hot path of xconv -- gather_nd of the previous features, the concat with the lifted coordinates, the matmul with the
X-transform and the depthwise half of fts_conv -- is one contraction (xconv_ops.xconv_contract, csrc/xconv.hip); the
dense lifts, the X_0 / X_1 / X_2 chain, the pointwise half, ELU and batch norm are torch expressions (pointfly.py)."""
import math

import torch

from . import pointfly as pf
from . import xconv_ops


def fts_conv(lifted, fts, indices, X, C, name, is_training, depth_multiplier):
    """pf.separable_conv2d(X @ concat(lifted, fts[indices]), C, name, is_training, (1, K), depth_multiplier) without its
    input ever formed: the layer's own two variables, the fused contraction (gather, concat, X-transform, depthwise half)
    in their place, then the pointwise half, ELU and the norm.  -> (N, P, 1, C)"""
    K = lifted.shape[2]
    channels = lifted.shape[3] + (0 if fts is None else fts.shape[2])
    dk, pk, bias = pf.separable_conv2d_variables(name, K, channels, C, depth_multiplier)
    mid = xconv_ops.xconv_contract(lifted.contiguous(), fts, indices if fts is not None else None, X.contiguous(),
                                   dk[0].contiguous())
    return pf.pointwise_finish(mid, pk, bias, name, is_training)


def xconv(pts, fts, qrs, tag, N, K, D, P, C, C_pts_fts, is_training, with_X_transformation, depth_multiplier,
          sorting_method=None, with_global=False):
    """pts (N,n,3), fts (N,n,C_prev) or None, qrs (N,P,3) -> (N,P,C) (+ C // 4 global channels in front)"""
    if K * D > pts.shape[1]:
        raise ValueError("%s: K * D = %d neighbours of %d points" % (tag, K * D, pts.shape[1]))
    indices_dilated = pf.knn_indices_general(qrs, pts, K * D, True)
    indices = indices_dilated[:, :, ::D].contiguous()                     # (N,P,K): every D-th of the K D nearest
    if sorting_method is not None:
        raise NotImplementedError("PointCNN sorting_method %r: only None is built" % (sorting_method,))

    nn_pts_local = xconv_ops.gather_rows(pts, indices) - qrs.unsqueeze(2)  # (N,P,K,3)
    nn_fts_from_pts_0 = pf.dense(nn_pts_local, C_pts_fts, tag + 'nn_fts_from_pts_0', is_training)
    nn_fts_from_pts = pf.dense(nn_fts_from_pts_0, C_pts_fts, tag + 'nn_fts_from_pts', is_training)

    if with_X_transformation:
        X_0 = pf.conv2d(nn_pts_local, K * K, tag + 'X_0', is_training, (1, K))
        X_1 = pf.depthwise_conv2d(X_0.reshape(N, -1, K, K), K, tag + 'X_1', is_training, (1, K))
        X_2 = pf.depthwise_conv2d(X_1.reshape(N, -1, K, K), K, tag + 'X_2', is_training, (1, K), activation=None)
        X = X_2.reshape(N, -1, K, K)
    else:                                                                 # fts_X = nn_fts_input: the identity transform
        X = torch.eye(K, dtype=pts.dtype, device=pts.device).expand(N, qrs.shape[1], K, K)

    fts_conv_3d = fts_conv(nn_fts_from_pts, fts, indices, X, C, tag + 'fts_conv', is_training, depth_multiplier).squeeze(2)

    if with_global:
        fts_global_0 = pf.dense(qrs, C // 4, tag + 'fts_global_0', is_training)
        fts_global = pf.dense(fts_global_0, C // 4, tag + 'fts_global', is_training)
        return torch.cat([fts_global, fts_conv_3d], dim=-1)
    return fts_conv_3d


def sample(pts, P, sampling, tag):
    """the P representative points of a layer (:92-104)"""
    if sampling == 'random':                                              # the clouds arrive shuffled: the first P points
        return pts[:, :P].contiguous()
    if sampling == 'fps':
        from ..pointnet2.tf_sampling import farthest_point_sample, gather_point
        return gather_point(pts.contiguous(), farthest_point_sample(P, pts.contiguous()))
    if sampling == 'ids':
        raise NotImplementedError("%ssampling 'ids' (inverse density sampling) is out of scope; use 'random' or 'fps'" % tag)
    raise ValueError("%sunknown sampling method %r" % (tag, sampling))


def fc_stack(fts, fc_params, name, is_training):
    """dense + dropout per row of fc_params, the layers named name.format(i) -> [fts, fc_0, fc_1, ...]"""
    layers = [fts]
    for layer_idx, layer_param in enumerate(fc_params):
        fc = pf.dense(layers[-1], layer_param['C'], name.format(layer_idx), is_training)
        # tf.layers.dropout(rate): `rate` of the units are DROPPED (0.8 on the last layer keeps a fifth)
        layers.append(torch.nn.functional.dropout(fc, float(layer_param['dropout_rate']), bool(is_training)))
    return layers


class Encoder:
    """the X-Conv layers of `xconv_params` (:68-131, and again :173-234): layer_pts / layer_fts, entry 0 the input"""

    def __init__(self, points, features, is_training, setting):
        xconv_params = setting.xconv_params
        if features is not None:
            raise NotImplementedError("PointCNN: extra per-point features are out of scope (use_extra_features = False)")
        N = points.shape[0]
        self.layer_pts = [points]
        self.layer_fts = [None]

        for layer_idx, layer_param in enumerate(xconv_params):
            tag = 'xconv_' + str(layer_idx + 1) + '_'
            K, D, P, C, links = (layer_param[k] for k in ('K', 'D', 'P', 'C', 'links'))
            if setting.sampling != 'random' and links:
                raise ValueError("flexible links are supported only when random sampling is used")

            pts = self.layer_pts[-1]
            fts = self.layer_fts[-1]
            if P == -1 or (layer_idx > 0 and P == xconv_params[layer_idx - 1]['P']):
                qrs = pts
            else:
                qrs = sample(pts, P, setting.sampling, tag)
            self.layer_pts.append(qrs)

            if layer_idx == 0:
                C_pts_fts = C // 2 if fts is None else C // 4
                depth_multiplier = 4
            else:
                C_prev = xconv_params[layer_idx - 1]['C']
                C_pts_fts = C_prev // 4
                depth_multiplier = math.ceil(C / C_prev)
            with_global = (setting.with_global and layer_idx == len(xconv_params) - 1)
            fts_xconv = xconv(pts, fts, qrs, tag, N, K, D, qrs.shape[1], C, C_pts_fts, is_training,
                              setting.with_X_transformation, depth_multiplier, setting.sorting_method, with_global)
            fts_list = [self.layer_fts[link][:, :qrs.shape[1]] for link in links if self.layer_fts[link] is not None]
            self.layer_fts.append(torch.cat(fts_list + [fts_xconv], dim=-1) if fts_list else fts_xconv)



class PointCNN(Encoder):
    def __init__(self, points, features, is_training, setting):
        Encoder.__init__(self, points, features, is_training, setting)
        self.fc_layers = fc_stack(self.layer_fts[-1], setting.fc_params, 'fc{:d}', is_training)


class PointCNN_SEG(Encoder):
    """mirror of :161-277: the encoder, the classification head on its last features, the X-DeConv decoder back up to the
    input points, the segmentation head.  An X-DeConv layer is xconv() from the points of encoder layer pts_layer_idx onto
    those of qrs_layer_idx with depth multiplier 1 and no global branch, then concat with the encoder's features at the
    query points and a dense layer."""

    def __init__(self, points, features, is_training, setting):
        Encoder.__init__(self, points, features, is_training, setting)
        xconv_params = setting.xconv_params
        N = points.shape[0]
        self.fc_layers_classification = fc_stack(self.layer_fts[-1], setting.fc_params_classification, 'fc_class_{:d}',
                                                 is_training)

        for layer_idx, layer_param in enumerate(getattr(setting, 'xdconv_params', [])):
            tag = 'xdconv_' + str(layer_idx + 1) + '_'
            K, D, pts_layer_idx, qrs_layer_idx = (layer_param[k] for k in ('K', 'D', 'pts_layer_idx', 'qrs_layer_idx'))

            pts = self.layer_pts[pts_layer_idx + 1]
            fts = self.layer_fts[pts_layer_idx + 1] if layer_idx == 0 else self.layer_fts[-1]
            qrs = self.layer_pts[qrs_layer_idx + 1]
            fts_qrs = self.layer_fts[qrs_layer_idx + 1]
            C = xconv_params[qrs_layer_idx]['C']
            C_pts_fts = xconv_params[pts_layer_idx]['C'] // 4
            fts_xdconv = xconv(pts, fts, qrs, tag, N, K, D, qrs.shape[1], C, C_pts_fts, is_training,
                               setting.with_X_transformation, 1, setting.sorting_method)
            fts_concat = torch.cat([fts_xdconv, fts_qrs], dim=-1)
            self.layer_pts.append(qrs)
            self.layer_fts.append(pf.dense(fts_concat, C, tag + 'fts_fuse', is_training))

        self.fc_layers_segmentation = fc_stack(self.layer_fts[-1], setting.fc_params_segmentation, 'fc_seg_{:d}', is_training)
