"""PointCNN classifier -- mirror of `PointCNN/pointcnn_cls.py` (Net :10-16) with the loss, the metrics and the trainer
numbers of `PointCNN/train.py` (:132-171, :254-276) under the setting `pointcnn_cls/modelnet_x3_l4.py`.

Training returns per-point logits (B, P_last, num_class); evaluation averages the last FC layer over the points first and
returns (B, 1, num_class).  Accuracy and votes are taken on `class_scores`: the softmax summed over the point axis."""
import torch
import torch.nn.functional as F

from . import pointfly as pf
from . import settings
from .pointcnn import PointCNN

NUM_CLASSES = 15


def get_model(point_cloud, is_training, bn_decay=None, setting=settings.modelnet_x3_l4, num_class=NUM_CLASSES):
    """point_cloud (B,N,3+) -> logits (B, P_last | 1, num_class).  bn_decay is accepted and unused: the norm's momentum
    is the constant 0.99 of pointfly.batch_normalization."""
    setting = settings.as_setting(setting)
    net = PointCNN(point_cloud[:, :, :3].contiguous(), None, is_training, setting)
    fc = net.fc_layers[-1]
    if not is_training:
        fc = fc.mean(dim=1, keepdim=True)
    return pf.dense(fc, num_class, 'logits', is_training, with_bn=False, activation=None)


def get_loss(pred, label):
    """the label tiled over the point axis, mean sparse softmax cross entropy (train.py:138-140)"""
    b, p, c = pred.shape
    return F.cross_entropy(pred.reshape(b * p, c), label.long().view(b, 1).expand(b, p).reshape(-1))


def class_scores(logits):
    """(B,P,C) -> (B,C): the softmax summed over the points (train.py:135,271: np.sum(probs, axis=1))"""
    return torch.softmax(logits, dim=-1).sum(dim=1)


def regularization_loss(net, weight_decay):
    """weight_decay * sum ||v||^2 / 2 over every kernel AND every batch-norm gamma and beta (each carries an
    l2_regularizer(scale=1.0) in pointfly.py; train.py:164); the bias of the logits layer carries none"""
    terms = [(p * p).sum() for name, p in net.named_parameters() if not name.endswith('/bias')]
    return 0.5 * float(weight_decay) * torch.stack(terms).sum()


def learning_rate(step, base, decay_steps, decay_rate, lr_min):
    """max(base * rate^floor(step / decay_steps), lr_min), counted in STEPS (train.py:160-162)"""
    return max(base * decay_rate ** (int(step) // int(decay_steps)), lr_min)


def setting_of(args):
    """--setting, or the setting of --model when the flag is left out (settings.MODEL_DEFAULT)"""
    return settings.get(getattr(args, "setting", None) or
                        settings.MODEL_DEFAULT.get(getattr(args, "model", None), "modelnet_x3_l4"))


def flag_defaults(args):
    """the trainer flags this model takes from its setting when the command line leaves them out (train.py:76-77)"""
    s = setting_of(args)
    return {"learning_rate": s.learning_rate_base, "decay_step": s.decay_steps, "decay_rate": s.decay_rate,
            "batch_size": s.batch_size, "max_epoch": s.num_epochs}


class Trainer:
    """What pointnet2/train.py takes from this model instead of its own defaults, bound to the flags: the lr schedule from
    --learning_rate / --decay_step / --decay_rate (the setting's values where the command line left them out: parse_args
    has resolved them) with the setting's floor, Adam's epsilon, the regulariser and the augmentation of --setting."""

    def __init__(self, args):
        self.setting = s = setting_of(args)
        given = lambda name, default: default if getattr(args, name, None) is None else getattr(args, name)  # noqa: E731
        self.base = float(given("learning_rate", s.learning_rate_base))
        self.decay_steps = int(given("decay_step", s.decay_steps))
        self.decay_rate = float(given("decay_rate", s.decay_rate))
        self.adam_epsilon = float(s.epsilon)

    def learning_rate(self, step):
        return learning_rate(step, self.base, self.decay_steps, self.decay_rate, self.setting.learning_rate_min)

    def regularization_loss(self, net):
        return regularization_loss(net, self.setting.weight_decay)

    def augment(self, batch, generator=None):
        return augment(batch, generator=generator, setting=self.setting)


def trainer(args):
    return Trainer(args)


def bind(setting, model=None):
    """get_model (or another model of the family with the same signature) under `setting`"""
    model = model or get_model

    def bound(point_cloud, is_training, bn_decay=None, num_class=NUM_CLASSES):
        return model(point_cloud, is_training, bn_decay=bn_decay, setting=setting, num_class=num_class)
    return bound


def model_fn(args, device=None):
    """the classifier for --setting (modelnet_x3_l4)"""
    return bind(setting_of(args))


def augment(batch, generator=None, setting=settings.modelnet_x3_l4):
    """the training augmentation of train.py:254-265: batch @ xforms (get_xforms under the setting's ranges), and a
    jitter that is 0.0 in the setting and so adds nothing"""
    s = setting
    xforms, _ = pf.get_xforms(batch.shape[0], rotation_range=s.rotation_range, scaling_range=s.scaling_range,
                              order=s.rotation_order, generator=generator, device=batch.device)
    return pf.augment(batch, xforms, s.jitter)
