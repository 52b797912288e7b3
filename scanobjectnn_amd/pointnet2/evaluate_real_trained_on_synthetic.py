"""Train on synthetic, test on real -- the caller `evaluate_real_trained_on_synthetic.py` that each of the reference's six
model folders ships, once for every family here: a classifier trained on ModelNet40 (`--num_class 40`) is evaluated on
ScanObjectNN clouds through `class_maps.MODELNET_TO_OBJECTDATASET`.  bag, bin, box and pillow have no ModelNet40 class
and are dropped from the test set; a prediction outside the fourteen mapped ModelNet40 classes is wrong ("NA").

  python -m scanobjectnn_amd.pointnet2.evaluate_real_trained_on_synthetic --model pointnet2_cls_ssg \
         --model_path log/model.pt | log/model.ckpt --test_file test_objectdataset.npz | .h5 [--num_votes 12]
  ... --model pointcnn_cls                       (--setting modelnet40_expt, as in the reference, unless given)

Outputs under --dump_dir [dump_real_trained_on_synthetic/]: log_evaluate.txt, pred_label.txt, confusion.csv (15 x 40).
`--num_votes` is honoured (several of the reference's copies parse it and then run one vote; at the default of 1 there is
no difference).  Protocol and the other deviations: `cross_domain.py`."""
from . import cross_domain

DIRECTION = cross_domain.REAL_ON_SYNTHETIC


def parse_args(argv=None):
    return cross_domain.parse_args(argv, DIRECTION, doc=__doc__)


def evaluate(args):
    """-> scores (K',40), label (K', ScanObjectNN), pred (K', ModelNet40), accuracy, avg_class_acc, per_class, confusion, ..."""
    return cross_domain.evaluate(args, DIRECTION)


if __name__ == "__main__":
    evaluate(parse_args())
