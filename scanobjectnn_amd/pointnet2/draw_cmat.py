"""Confusion matrix of the same-domain evaluation -- the caller `pointnet2/draw_cmat.py` (one copy per model folder in the
reference): the evaluation of `evaluate_scenennobjects` with its flags, reached by calling it, then the confusion matrix of
its predictions, row-normalised (`:204-211`: every row divided by its sum, an empty row left as zeros by `nan_to_num`).

  python -m scanobjectnn_amd.pointnet2.draw_cmat --model pointnet2_cls_ssg --model_path log/model.pt \
         --test_file test.npz [--num_votes 12] [--dump_dir confusion_matrix/]

Writes `matrix.csv` (one row per true class, `%.17g`) next to the evaluation's own outputs, and `matrix.pdf` (`:213-228`)
when matplotlib imports; without it only the plot is skipped.

Deviation: the matrix is always --num_class x --num_class (15 x 15) by label index.  The reference's sklearn call shrinks
it to the classes that occur among labels and predictions and then labels 15 ticks, which shifts the names once a class
is absent."""
import os
import sys

import numpy as np

from . import evaluate_scenennobjects as EV

DUMP_DIR = "confusion_matrix/"                     # :39


def confusion_counts(pred, label, num_classes=EV.NUM_CLASSES):
    """(num_classes, num_classes) raw counts: rows the true class, columns the predicted class"""
    mat = np.zeros((num_classes, num_classes), dtype=np.int64)
    np.add.at(mat, (np.asarray(label, dtype=np.int64), np.asarray(pred, dtype=np.int64)), 1)
    return mat


def row_normalised(counts):
    """every row divided by its sum; a class that never occurs keeps a row of zeros"""
    counts = np.asarray(counts, dtype=np.float64)
    total = counts.sum(axis=1, keepdims=True)
    return np.divide(counts, total, out=np.zeros_like(counts), where=total > 0)


def parse_args(argv=None):
    """the flags of `evaluate_scenennobjects`, with this script's --dump_dir default"""
    argv = list(sys.argv[1:] if argv is None else argv)
    if not any(a == "--dump_dir" or a.startswith("--dump_dir=") for a in argv):
        argv += ["--dump_dir", DUMP_DIR]
    return EV.parse_args(argv)


def plot(mat, names, path):
    """matrix.pdf; False when matplotlib is not installed"""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        return False
    fig, ax = plt.subplots(figsize=(8, 8))
    im = ax.imshow(mat, interpolation="nearest", cmap="Blues", vmin=0.0, vmax=1.0)
    fig.colorbar(im, ax=ax, fraction=0.046)
    ticks = np.arange(len(names))
    ax.set_xticks(ticks)
    ax.set_yticks(ticks)
    ax.set_xticklabels(names, rotation=90)
    ax.set_yticklabels(names)
    ax.set_xlabel("predicted")
    ax.set_ylabel("true")
    fig.tight_layout()
    fig.savefig(path)
    plt.close(fig)
    return True


def draw(args):
    ev = EV.evaluate(args)
    mat = row_normalised(confusion_counts(ev["pred"], ev["label"], args.num_class))
    np.savetxt(os.path.join(args.dump_dir, "matrix.csv"), mat, fmt="%.17g", delimiter=",")     # reads back exactly
    names = [l.rstrip() for l in open(args.shape_names)] if args.shape_names else \
        (EV.SHAPE_NAMES if args.num_class == 15 else ["class%d" % i for i in range(args.num_class)])
    plotted = plot(mat, names[:args.num_class], os.path.join(args.dump_dir, "matrix.pdf"))
    return dict(ev, matrix=mat, plotted=plotted)


if __name__ == "__main__":
    draw(parse_args())
