"""PointCNN's background-aware model -- mirror of `PointCNN/pointcnn_seg.py` (Net :9-19) on `PointCNN_SEG`, with the losses
of `PointCNN/train_seg.py:137-146` under the setting `pointcnn_seg/object_dataset_x3.py`.

Both heads are per point: classification logits (B, P_last, num_class) on the encoder's last representatives and mask logits
(B, N, 2) on the input points, which the X-DeConv decoder reaches again.  Unlike the classifier's Net there is no mean over
the points at evaluation.  Accuracy and votes of the class head are taken on `class_scores`, as for the classifier; the
trainer numbers, the augmentation and the regulariser are the classifier's (TRAINER_FROM), read from this model's setting."""
import torch.nn.functional as F

from . import pointfly as pf
from . import settings
from .pointcnn import PointCNN_SEG
from .pointcnn_cls import NUM_CLASSES, augment, bind, class_scores, setting_of  # noqa: F401
from .pointcnn_cls import get_loss as classification_loss

# pointnet2/train.py takes this model's trainer numbers -- Adam's epsilon, the lr schedule in steps with the setting's
# floor, the regulariser, the augmentation -- from the classifier's `trainer` hook, bound to THIS model's setting.  The
# module defines no `trainer` and no `flag_defaults` of its own: --learning_rate, --decay_step, --decay_rate, --batch_size
# and --max_epoch keep the trainer's defaults when the command line leaves them out (only pointcnn_cls reads them from
# its setting), so the reference's numbers are given on the command line.
TRAINER_FROM = "scanobjectnn_amd.pointcnn.pointcnn_cls"


def get_model(point_cloud, is_training, bn_decay=None, setting=settings.object_dataset_x3, num_class=NUM_CLASSES):
    """point_cloud (B,N,3+) -> (classification logits (B, P_last, num_class), segmentation logits (B, N, 2)).  bn_decay is
    accepted and unused, as in pointcnn_cls."""
    setting = settings.as_setting(setting)
    net = PointCNN_SEG(point_cloud[:, :, :3].contiguous(), None, is_training, setting)
    classification_logits = pf.dense(net.fc_layers_classification[-1], num_class, 'logits_classification', is_training,
                                     with_bn=False, activation=None)
    segmentation_logits = pf.dense(net.fc_layers_segmentation[-1], 2, 'logits_segmentation', is_training, with_bn=False,
                                   activation=None)
    return classification_logits, segmentation_logits


def get_loss(class_logits, seg_logits, label, mask, seg_weight=0.5):
    """-> (total, classify_loss, seg_loss): the label tiled over the point axis (:138-140), the mean over the clouds of each
    cloud's mean mask cross entropy (:143-144), total = (1 - w) classify + w seg (:146)"""
    classify_loss = classification_loss(class_logits, label)
    b, n, c = seg_logits.shape
    per_point = F.cross_entropy(seg_logits.reshape(b * n, c), mask.reshape(b * n).long(), reduction='none').view(b, n)
    seg_loss = per_point.mean(dim=1).mean()
    return (1 - seg_weight) * classify_loss + seg_weight * seg_loss, classify_loss, seg_loss


def model_fn(args, device=None):
    """the model for --setting (object_dataset_x3)"""
    return bind(setting_of(args), get_model)
