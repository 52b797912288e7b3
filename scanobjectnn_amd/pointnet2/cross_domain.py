"""Cross-domain evaluation -- the reference README's "Generalization of real vs synthetic": a ModelNet40-trained
classifier tested on ScanObjectNN (`evaluate_real_trained_on_synthetic.py`, which each of its six model folders ships) and
a ScanObjectNN-trained one tested on ModelNet40 (`evaluate_synthetic_trained_on_real.py`), both through the class maps
of `class_maps.py`.  One implementation for every family here, selected by `--model`.

The protocol (`pointnet2/evaluate_real_trained_on_synthetic.py:143-259`, `evaluate_synthetic_trained_on_real.py:143-263`):
the test set is sampled and shuffled as in the same-domain evaluation, the clouds whose label has no counterpart in the
other domain are dropped BEFORE batching, whole batches are scored with the votes summed, and a prediction counts as
correct when it maps onto the label.  Per-class counters live in the 15 ScanObjectNN slots in both directions.  The
metric functions work on host arrays and take any callable as the model, so they run without a GPU.

Deviations from the reference:
  * `--num_votes` is honoured for every family.  Several of the reference's copies parse it and then run one vote; at the
    default of 1 there is no difference.
  * no loss is computed: the labels live in the other label space (a ModelNet label up to 39 is no target for a 15-class
    loss), and the reference has the line that logs it commented out.
  * a confusion matrix of raw counts (`confusion.csv`) with a fixed size, test-set classes by model classes.
  * fewer surviving clouds than one batch: a SystemExit that says so, where the reference divides by zero.
"""
import argparse
import importlib
import os

import numpy as np
import torch

from .. import data_utils
from ..class_maps import (MODELNET_SHAPE_NAMES, MODELNET_TO_OBJECTDATASET, OBJECTDATASET_SHAPE_NAMES,
                          OBJECTDATASET_TO_MODELNET)
from .evaluate_scenennobjects import load_test_set, restore, split_output, vote_logits

REAL_ON_SYNTHETIC = "real_trained_on_synthetic"        # a 40-class model on ScanObjectNN clouds
SYNTHETIC_ON_REAL = "synthetic_trained_on_real"        # a 15-class model on ModelNet40 clouds
NUM_OBJECTDATASET, NUM_MODELNET = len(OBJECTDATASET_SHAPE_NAMES), len(MODELNET_SHAPE_NAMES)
# per direction: the model's label space and class count, the test set's, and PointCNN's setting when --setting is left out
DIRECTIONS = {
    REAL_ON_SYNTHETIC: dict(model_classes=NUM_MODELNET, test_classes=NUM_OBJECTDATASET, test_keys=OBJECTDATASET_TO_MODELNET,
                            setting={"pointcnn_cls": "modelnet40_expt"}),
    SYNTHETIC_ON_REAL: dict(model_classes=NUM_OBJECTDATASET, test_classes=NUM_MODELNET, test_keys=MODELNET_TO_OBJECTDATASET,
                            setting={"pointcnn_cls": "modelnet_x3_l4"})}


def _direction(direction):
    if direction not in DIRECTIONS:
        raise ValueError("direction %r: one of %s" % (direction, ", ".join(sorted(DIRECTIONS))))
    return DIRECTIONS[direction]


def _too_few(what):
    return SystemExit("cross-domain evaluation: %s; nothing to average over (lower --batch_size, or check that the test "
                      "file's labels are in the test domain's label space)" % what)


def select_mapped(data, labels, direction):
    """-> (data, labels) of the clouds whose label has a counterpart in the other domain, order preserved.  Runs BEFORE
    batching (`evaluate_real_trained_on_synthetic.py:156-170`), so the dropped clouds do not thin out the batches."""
    labels = np.asarray(labels).reshape(-1)
    keep = np.isin(labels, sorted(_direction(direction)["test_keys"]))
    return np.asarray(data)[keep], labels[keep]


@torch.no_grad()
def vote_scores(net, data, batch_size, num_votes=1, device="cuda:0", scores_fn=None):
    """(K', C): the scores of every cloud of the K' = (K // batch_size) * batch_size whole batches, summed over `num_votes`
    rotations about the up axis -- the forward of `evaluate_scenennobjects.eval_one_epoch` (its `vote_logits`,
    `split_output` and the model module's optional `class_scores` hook as `scores_fn`), without loss and labels."""
    if scores_fn is None:
        scores_fn = lambda logits: logits                              # noqa: E731
    num_batches = len(data) // batch_size
    if num_batches == 0:
        raise _too_few("%d clouds are left after the class filter, fewer than one batch of %d" % (len(data), batch_size))
    out = []
    for b in range(num_batches):
        pts = torch.as_tensor(data[b * batch_size:(b + 1) * batch_size], dtype=torch.float32, device=device)
        out.append(vote_logits(lambda p: scores_fn(split_output(net(p.contiguous(), is_training=False))[0]), pts,
                               num_votes).cpu().numpy())
    return np.concatenate(out)


def _lut(mapping, size):
    lut = np.full(size, -1, dtype=np.int64)
    for k, v in mapping.items():
        lut[k] = v
    return lut


def _summary(pred, pred_slot, label_slot, lines, confusion):
    """the shared tail: `pred_slot` / `label_slot` are the prediction and the label as ScanObjectNN indices (-1: a
    prediction without counterpart, which is seen and wrong)"""
    correct = pred_slot == label_slot
    seen_class = np.bincount(label_slot, minlength=NUM_OBJECTDATASET)
    correct_class = np.bincount(label_slot[correct], minlength=NUM_OBJECTDATASET)
    occurs = seen_class > 0
    per_class = np.where(occurs, correct_class / np.maximum(seen_class, 1), -1.0)
    return {"pred": pred, "total_seen": int(len(pred)), "total_correct": int(correct.sum()),
            "accuracy": float(correct.sum()) / len(pred), "avg_class_acc": float(per_class[occurs].mean()),
            "per_class": per_class, "seen_class": seen_class, "correct_class": correct_class, "lines": lines,
            "confusion": confusion}


def _checked(scores, labels, num_model, num_test):
    scores, labels = np.asarray(scores), np.asarray(labels).reshape(-1).astype(np.int64)
    if len(labels) == 0:
        raise _too_few("no cloud was scored")
    if scores.shape != (len(labels), num_model):
        raise ValueError("scores %s for %d labels: expected (%d, %d)" % (scores.shape, len(labels), len(labels), num_model))
    if labels.min() < 0 or labels.max() >= num_test:
        raise ValueError("labels outside 0..%d" % (num_test - 1))
    pred = scores.argmax(axis=1)                                # the first maximiser
    confusion = np.zeros((num_test, num_model), dtype=np.int64)
    np.add.at(confusion, (labels, pred), 1)
    return labels, pred, confusion


def summarize_real_on_synthetic(scores40, labels15):
    """a 40-class model on ScanObjectNN labels (`evaluate_real_trained_on_synthetic.py:199-259`): the prediction is mapped
    to ScanObjectNN and compared with the label; one without counterpart is seen and wrong ("NA" in pred_label.txt).
    -> accuracy, avg_class_acc (mean over the classes that were seen), per_class (15, -1 where never seen), pred,
    seen_class / correct_class (15), lines ("<mapped prediction | NA>, <label>"), confusion (15 x 40 raw counts)."""
    labels, pred, confusion = _checked(scores40, labels15, NUM_MODELNET, NUM_OBJECTDATASET)
    mapped = _lut(MODELNET_TO_OBJECTDATASET, NUM_MODELNET)[pred]
    names = OBJECTDATASET_SHAPE_NAMES
    lines = ["%s, %s" % (names[m] if m >= 0 else "NA", names[l]) for m, l in zip(mapped, labels)]
    return _summary(pred, mapped, labels, lines, confusion)


def summarize_synthetic_on_real(scores15, labels40):
    """a 15-class model on ModelNet40 labels (`evaluate_synthetic_trained_on_real.py:199-263`): correct when the label is
    one of the ModelNet classes the prediction stands for, which is to say when the label maps onto the prediction (the
    inverse map is derived from the forward one).  Counters are indexed by the MAPPED label; every label must be mapped
    (`select_mapped`).  lines: "<prediction>, <mapped label>", both ScanObjectNN names; confusion: 40 x 15 raw counts."""
    labels, pred, confusion = _checked(scores15, labels40, NUM_OBJECTDATASET, NUM_MODELNET)
    slot = _lut(MODELNET_TO_OBJECTDATASET, NUM_MODELNET)[labels]
    if (slot < 0).any():
        raise ValueError("ModelNet40 label %d has no ScanObjectNN counterpart: filter with select_mapped first"
                         % labels[slot < 0][0])
    has_counterpart = np.isin(pred, sorted(OBJECTDATASET_TO_MODELNET))
    names = OBJECTDATASET_SHAPE_NAMES
    lines = ["%s, %s" % (names[p], names[s]) for p, s in zip(pred, slot)]
    return _summary(pred, np.where(has_counterpart, pred, -1), slot, lines, confusion)


SUMMARIES = {REAL_ON_SYNTHETIC: summarize_real_on_synthetic, SYNTHETIC_ON_REAL: summarize_synthetic_on_real}


def confusion_csv(confusion, direction):
    """header row of the model's class names, then one row per true class of the test set: its name, then the counts"""
    model_names, test_names = (MODELNET_SHAPE_NAMES, OBJECTDATASET_SHAPE_NAMES) if direction == REAL_ON_SYNTHETIC else \
        (OBJECTDATASET_SHAPE_NAMES, MODELNET_SHAPE_NAMES)
    rows = ["true\\pred," + ",".join(model_names)]
    rows += ["%s,%s" % (name, ",".join(str(int(c)) for c in row)) for name, row in zip(test_names, confusion)]
    return "\n".join(rows) + "\n"


# ---- the two command lines ------------------------------------------------------------------------------------------
def parse_args(argv, direction, doc=None):
    """the flags of the reference's scripts (`:27-45`); --num_class and --dump_dir default per direction"""
    from .train import MODELS, _flag, add_model_flags, resolve_model_flags
    d = _direction(direction)
    p = argparse.ArgumentParser(description=doc or __doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--gpu", type=int, default=0, help="GPU to use (:28)")
    p.add_argument("--model", default="pointnet2_cls_ssg", choices=sorted(MODELS))            # :29
    p.add_argument("--batch_size", type=int, default=1)                                       # :30
    p.add_argument("--num_point", type=int, default=1024)                                     # :31
    p.add_argument("--model_path", default="log/model.ckpt",
                   help="model.pt of this package, or the prefix of a TensorFlow tensor bundle (:33)")
    p.add_argument("--dump_dir", default="dump_%s/" % direction)                              # :34
    p.add_argument("--with_bg", type=_flag, default=True)                                     # :35
    p.add_argument("--norm", type=_flag, default=True)                                        # :36
    p.add_argument("--center_data", type=_flag, default=True)                                 # :37
    p.add_argument("--num_class", type=int, default=None,
                   help="classes of the MODEL [%d; pointcnn_cls: its setting's]" % d["model_classes"])    # :38
    p.add_argument("--test_file", default="", help=".npz / .h5 / pickled split list of the OTHER domain (:40); synthetic "
                   "clouds with labels over its %d classes if empty" % d["test_classes"])
    p.add_argument("--data_path", default="", help="root of the raw objects_bin/ files for pickled split lists")
    p.add_argument("--normal", action="store_true", help="accepted for CLI compatibility (:42); never read")
    p.add_argument("--num_votes", type=int, default=1, help="honoured for every family (:43)")
    p.add_argument("--visu", type=_flag, default=False, help="accepted (:44); image / ply dumps are out of scope")
    p.add_argument("--synthetic_clouds", type=int, default=256)
    add_model_flags(p)
    return resolve_model_flags(p.parse_args(argv), num_class=d["model_classes"], setting=d["setting"])


def evaluate(args, direction):
    from ..graph import Model
    from .train import ALL_MASK_MODELS, MODELS, model_fn
    d = _direction(direction)
    if not torch.cuda.is_available() or not 0 <= args.gpu < torch.cuda.device_count():
        raise RuntimeError("--gpu %d: no such device (%d visible)" % (args.gpu, torch.cuda.device_count()))
    dev = torch.device("cuda", args.gpu)
    torch.cuda.set_device(dev)
    if args.model in ALL_MASK_MODELS or args.model.endswith("_partseg"):
        raise SystemExit("evaluate_%s.py evaluates classifiers; the background-aware models have their own command line, "
                         "as in the reference: python -m scanobjectnn_amd.pointnet2.evaluate_seg_scenennobjects (part "
                         "models: python -m scanobjectnn_amd.pointnet2.evaluate_partseg)" % direction)
    if args.num_class != d["model_classes"]:
        raise SystemExit("evaluate_%s.py maps the %d classes of its model's domain; --num_class %d%s has no class map"
                         % (direction, d["model_classes"], args.num_class,
                            " (--setting %s)" % args.setting if args.model == "pointcnn_cls" else ""))
    mod = importlib.import_module(MODELS[args.model])
    os.makedirs(args.dump_dir, exist_ok=True)
    log_f = open(os.path.join(args.dump_dir, "log_evaluate.txt"), "w")
    log_f.write(str(args) + "\n")

    def log_string(s):
        log_f.write(s + "\n")
        log_f.flush()
        print(s)

    rng = np.random.RandomState(0)                 # `np.random.seed(0)` (:73): the same two shuffles as the reference
    # the test set's labels live in the OTHER domain's label space: synthetic ones are drawn there
    data, labels = load_test_set(argparse.Namespace(**dict(vars(args), num_class=d["test_classes"])))
    kw = {"num_class": args.num_class} if args.num_class != 15 else {}
    net = Model(model_fn(mod, args, dev), device=dev, seed=0, **kw).build(torch.zeros((2, args.num_point, 3), device=dev))
    info = restore(net, args.model_path)
    log_string("Model restored. (%s, %d variables)" % (info["format"], info["loaded"]))
    if isinstance(data, list):
        cur, lab = data_utils.get_current_data(data, labels, args.num_point, rng=rng)     # :148
    else:
        cur, lab = data_utils.get_current_data_h5(data, labels, args.num_point, rng=rng)  # :146
    lab = np.squeeze(lab)
    log_string("%s %s" % (cur.shape, lab.shape))                                          # :153-154
    cur, lab = select_mapped(cur, lab, direction)
    log_string("%s %s" % (cur.shape, lab.shape))                                          # :165-166
    scores = vote_scores(net, cur, args.batch_size, num_votes=args.num_votes, device=dev,
                         scores_fn=getattr(mod, "class_scores", None))
    lab = lab[:len(scores)]
    ev = SUMMARIES[direction](scores, lab)
    with open(os.path.join(args.dump_dir, "pred_label.txt"), "w") as fout:                 # :227
        fout.write("".join(line + "\n" for line in ev["lines"]))
    with open(os.path.join(args.dump_dir, "confusion.csv"), "w") as fout:
        fout.write(confusion_csv(ev["confusion"], direction))
    log_string("total seen: %d" % ev["total_seen"])
    log_string("eval accuracy: %f" % ev["accuracy"])
    log_string("eval avg class acc: %f" % ev["avg_class_acc"])
    for name, acc in zip(OBJECTDATASET_SHAPE_NAMES, ev["per_class"]):
        log_string("%10s:\t%0.3f" % (name, acc))
    log_f.close()
    return dict(ev, scores=scores, label=lab)
