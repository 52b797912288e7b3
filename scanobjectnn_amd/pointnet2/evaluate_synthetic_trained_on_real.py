"""Train on real, test on synthetic -- the caller `evaluate_synthetic_trained_on_real.py` that each of the reference's six
model folders ships, once for every family here: a classifier trained on ScanObjectNN (`--num_class 15`) is evaluated on
ModelNet40 clouds.  Only the fourteen ModelNet40 classes with a ScanObjectNN counterpart are tested; a prediction is
correct when the label is one of the ModelNet40 classes it stands for (chair <- chair, bench, stool).

  python -m scanobjectnn_amd.pointnet2.evaluate_synthetic_trained_on_real --model pointnet2_cls_ssg \
         --model_path log/model.pt | log/model.ckpt --test_file modelnet40_test.npz | .h5 [--num_votes 12]

A single ModelNet40 file is read as .npz (arrays `data` (K,N,3), `label` (K,)), or as .h5 where h5py is installed.
Outputs under --dump_dir [dump_synthetic_trained_on_real/]: log_evaluate.txt, pred_label.txt, confusion.csv (40 x 15).
`--num_votes` is honoured (several of the reference's copies parse it and then run one vote; at the default of 1 there is
no difference).  Protocol and the other deviations: `cross_domain.py`."""
from . import cross_domain

DIRECTION = cross_domain.SYNTHETIC_ON_REAL


def parse_args(argv=None):
    return cross_domain.parse_args(argv, DIRECTION, doc=__doc__)


def evaluate(args):
    """-> scores (K',15), label (K', ModelNet40), pred (K', ScanObjectNN), accuracy, avg_class_acc, per_class, confusion, ..."""
    return cross_domain.evaluate(args, DIRECTION)


if __name__ == "__main__":
    evaluate(parse_args())
