"""Settings of the PointCNN models -- the numbers of `PointCNN/pointcnn_cls/modelnet_x3_l4.py`, its 40-class twin
`modelnet40_expt.py` and `PointCNN/pointcnn_seg/object_dataset_x3.py` as plain namespaces.  `as_setting` takes any object with the same attributes,
so tests build much smaller ones."""
import math
from types import SimpleNamespace

_XCONV = ('K', 'D', 'P', 'C', 'links')
_XDCONV = ('K', 'D', 'pts_layer_idx', 'qrs_layer_idx')
_FC = ('C', 'dropout_rate')
REQUIRED = ('xconv_params', 'with_global', 'sampling', 'with_X_transformation', 'sorting_method')
# ... and the heads: `fc_params` (the classifier) or the two split lists of the BGA model
HEADS = (('fc_params',), ('fc_params_classification', 'fc_params_segmentation'))
DEFAULTS = dict(num_class=15, sample_num=1024, batch_size=32, num_epochs=400, learning_rate_base=0.01, decay_steps=8000,
                decay_rate=0.5, learning_rate_min=1e-6, weight_decay=1e-5, jitter=0.0, jitter_val=0.0,
                rotation_range=[0, math.pi, 0, 'u'], rotation_range_val=[0, 0, 0, 'u'], rotation_order='rxyz',
                scaling_range=[0.1, 0.1, 0.1, 'g'], scaling_range_val=[0, 0, 0, 'u'], optimizer='adam', epsilon=1e-2,
                data_dim=6, use_extra_features=False)


def xconv_params(rows):
    return [dict(zip(_XCONV, r)) for r in rows]


def xdconv_params(rows):
    return [dict(zip(_XDCONV, r)) for r in rows]


def fc_params(rows):
    return [dict(zip(_FC, r)) for r in rows]


def make(**kw):
    """a setting: DEFAULTS (the trainer's numbers of modelnet_x3_l4, which object_dataset_x3 repeats) overridden by kw"""
    return as_setting(SimpleNamespace(**dict(DEFAULTS, **kw)))


def as_setting(obj):
    """`obj` itself after checking that it carries what the trunk reads; trainer numbers it lacks come from DEFAULTS"""
    missing = [a for a in REQUIRED if not hasattr(obj, a)]
    if not any(all(hasattr(obj, a) for a in heads) for heads in HEADS):
        missing.append("fc_params (or fc_params_classification and fc_params_segmentation)")
    if missing:
        raise AttributeError("PointCNN setting lacks %s" % ", ".join(missing))
    for k, v in DEFAULTS.items():
        if not hasattr(obj, k):
            setattr(obj, k, v)
    return obj


_x = 3
_ENCODER_X3 = [(8, 1, -1, 16 * _x, []),
               (12, 2, 384, 32 * _x, []),
               (16, 2, 128, 64 * _x, []),
               (16, 3, 128, 128 * _x, [])]
modelnet_x3_l4 = make(
    xconv_params=xconv_params(_ENCODER_X3),
    fc_params=fc_params([(128 * _x, 0.0), (64 * _x, 0.8)]),
    with_global=True, sampling='random', with_X_transformation=True, sorting_method=None)

# the ModelNet40 experiment (train on synthetic, test on real): modelnet_x3_l4 with 40 classes, nothing else differs
modelnet40_expt = make(**dict(vars(modelnet_x3_l4), num_class=40))

object_dataset_x3 = make(
    xconv_params=xconv_params(_ENCODER_X3),
    xdconv_params=xdconv_params([(16, 6, 3, 3),
                                 (16, 6, 3, 2),
                                 (12, 6, 2, 1),
                                 (8, 6, 1, 0),
                                 (8, 4, 0, 0)]),
    fc_params_classification=fc_params([(128 * _x, 0.0), (64 * _x, 0.8)]),
    fc_params_segmentation=fc_params([(32 * _x, 0.0), (32 * _x, 0.5)]),
    with_global=True, sampling='random', with_X_transformation=True, sorting_method=None, data_dim=3)

SETTINGS = {"modelnet_x3_l4": modelnet_x3_l4, "modelnet40_expt": modelnet40_expt, "object_dataset_x3": object_dataset_x3}
# the setting a model takes when --setting is left out
MODEL_DEFAULT = {"pointcnn_cls": "modelnet_x3_l4", "pointcnn_seg": "object_dataset_x3"}
# the models that take --num_class from their setting when it is left out (pointcnn_seg keeps the command line's default,
# like its other flags)
NUM_CLASS_FROM_SETTING = frozenset({"pointcnn_cls"})


def get(name):
    if name not in SETTINGS:
        raise KeyError("--setting %s: known settings are %s" % (name, ", ".join(sorted(SETTINGS))))
    return SETTINGS[name]
