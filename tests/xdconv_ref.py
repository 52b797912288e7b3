"""Float64 restatement of PointCNN's background-aware model (PointCNN_SEG + Net of the reference, setting
pointcnn_seg/object_dataset_x3) with the neighbour indices as an input, built on tests/xconv_ref.xconv_layer and written from
PointCNN's description of the X-DeConv layer, not from scanobjectnn_amd/pointcnn.

An X-DeConv layer is an X-Conv layer whose source points `pts` and query points `qrs` are two stages of the ENCODER (rows
(K, D, pts_layer_idx, qrs_layer_idx)): depth multiplier 1, no global branch, its output concatenated IN FRONT of the encoder's
own features at the query points, then one dense layer back to that stage's width.  The first X-DeConv reads the encoder's
features of stage pts_layer_idx; every later one reads the previous X-DeConv's fused output.

`wrong` names one deliberate mistake per decoder edge (tests/test_xdconv_ref_cpu.py shows each is rejected):
  'swapped'   pts_layer_idx and qrs_layer_idx exchanged
  'front'     the encoder's features concatenated in front of the X-DeConv output instead of behind it
  'stage'     the first X-DeConv fed the encoder's features of the stage before pts_layer_idx"""
import math

import torch

import xconv_ref as R


def encoder(points, P, setting, training, indices):
    """-> (pts_l, fts_l): per stage the points and the features, entry 0 the input cloud (no features); the classifier's
    loop of xconv_ref.pointcnn_cls"""
    pts_l, fts_l = [points], [None]
    params = setting.xconv_params
    for li, lp in enumerate(params):
        K, Pn, C = lp['K'], lp['P'], lp['C']
        pts, fts = pts_l[-1], fts_l[-1]
        qrs = pts if (Pn == -1 or (li > 0 and Pn == params[li - 1]['P'])) else pts[:, :Pn]
        if li == 0:
            c_pts, dm = C // 2, 4
        else:
            c_pts, dm = params[li - 1]['C'] // 4, math.ceil(C / params[li - 1]['C'])
        out = R.xconv_layer(P, 'xconv_%d_' % (li + 1), pts, fts, qrs, indices[li], K, C, c_pts, dm, training,
                            setting.with_X_transformation, setting.with_global and li == len(params) - 1)
        links = [fts_l[link][:, :qrs.shape[1]] for link in lp['links'] if fts_l[link] is not None]
        pts_l.append(qrs)
        fts_l.append(torch.cat(links + [out], dim=-1) if links else out)
    return pts_l, fts_l


def _head(P, name, x, rows, training):
    for i in range(len(rows)):
        x = R._dense(P, name % i, x, training)
    return x


def pointcnn_seg(points, P, setting, training, indices, wrong=None):
    """points (B, N, 3) float64, P: float64 variables by TF name, indices: per X-Conv layer and then per X-DeConv layer the
    (B, P_l, K) neighbour indices (already dilated) -> (classification logits (B, P_last, num_class), segmentation logits
    (B, N, 2)).  Dropout is the identity here; sampling 'random'; no mean over the points in either mode."""
    params = setting.xconv_params
    pts_l, fts_l = encoder(points, P, setting, training, indices)
    cls = _head(P, 'fc_class_%d', fts_l[-1], setting.fc_params_classification, training)
    cls = cls @ P['logits_classification/kernel'] + P['logits_classification/bias']

    fused = None
    for di, dp in enumerate(setting.xdconv_params):
        src, dst = dp['pts_layer_idx'], dp['qrs_layer_idx']
        if wrong == 'swapped':
            src, dst = dst, src
        first = fts_l[src + 1] if wrong != 'stage' else fts_l[src]
        fts = first if fused is None else fused
        C = params[dst]['C']
        out = R.xconv_layer(P, 'xdconv_%d_' % (di + 1), pts_l[src + 1], fts, pts_l[dst + 1], indices[len(params) + di],
                            dp['K'], C, params[src]['C'] // 4, 1, training, setting.with_X_transformation, False)
        skip = fts_l[dst + 1]
        both = torch.cat([skip, out] if wrong == 'front' else [out, skip], dim=-1)
        fused = R._dense(P, 'xdconv_%d_fts_fuse' % (di + 1), both, training)
    seg = _head(P, 'fc_seg_%d', fused, setting.fc_params_segmentation, training)
    return cls, seg @ P['logits_segmentation/kernel'] + P['logits_segmentation/bias']


def _ce(logits, target):
    """-log softmax(logits)[target] per row, (..., C) and (...) -> (...)"""
    return -(torch.log_softmax(logits, dim=-1).gather(-1, target.long().unsqueeze(-1)).squeeze(-1))


def loss(cls, seg, label, mask, seg_weight, wrong=None):
    """(total, classify, seg) of train_seg.py:137-146: the class cross entropy with the label repeated over the points,
    averaged over all of them; per cloud the mean mask cross entropy, averaged over the clouds.  wrong = 'sum': the mask
    term as the sum over a cloud's points instead of their mean"""
    classify = _ce(cls, label.view(-1, 1).expand(cls.shape[:2])).mean()
    per_cloud = _ce(seg, mask).sum(dim=1) if wrong == 'sum' else _ce(seg, mask).mean(dim=1)
    seg_loss = per_cloud.mean()
    return (1 - seg_weight) * classify + seg_weight * seg_loss, classify, seg_loss
