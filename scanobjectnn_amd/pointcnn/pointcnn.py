"""X-Conv and the PointCNN trunk -- mirror of `PointCNN/pointcnn.py` (xconv :10-52, PointCNN :55-159).

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


class PointCNN:
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

        self.fc_layers = [self.layer_fts[-1]]
        for layer_idx, layer_param in enumerate(setting.fc_params):
            fc = pf.dense(self.fc_layers[-1], layer_param['C'], 'fc{:d}'.format(layer_idx), is_training)
            # tf.layers.dropout(rate): `rate` of the units are DROPPED (0.8 on the last layer keeps a fifth)
            self.fc_layers.append(torch.nn.functional.dropout(fc, float(layer_param['dropout_rate']), bool(is_training)))
