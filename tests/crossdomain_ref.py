"""Restatement of the two cross-domain metric loops (`pointnet2/evaluate_real_trained_on_synthetic.py:156-259`,
`evaluate_synthetic_trained_on_real.py:156-263`) as plain per-cloud Python loops over dicts, independent of the
vectorised product code in `scanobjectnn_amd/pointnet2/cross_domain.py` and of `class_maps.py`: the maps are derived here
from the two name fixtures under tests/golden/ plus the six aliases.

The `wrong_*` functions are one wrong restatement per rule; the tests show that the comparison tells them apart."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALIASES = {"bookshelf": "shelf", "dresser": "cabinet", "wardrobe": "cabinet", "monitor": "display", "bench": "chair",
           "stool": "chair"}


def read_names(filename):
    with open(os.path.join(GOLDEN, filename)) as f:
        return [line.rstrip() for line in f if line.strip()]


MODELNET_NAMES = read_names("shape_names_modelnet.txt")
OBJECT_NAMES = read_names("shape_names_ext.txt")


def derive_forward():
    """ModelNet40 index -> ScanObjectNN index: the class of the same name, or of the alias"""
    fwd = {}
    for i, name in enumerate(MODELNET_NAMES):
        name = ALIASES.get(name, name)
        if name in OBJECT_NAMES:
            fwd[i] = OBJECT_NAMES.index(name)
    return fwd


def derive_inverse(fwd):
    inv = {}
    for m in sorted(fwd):
        inv.setdefault(fwd[m], []).append(m)
    return inv


M2O = derive_forward()
O2M = derive_inverse(M2O)


def filter_mapped(data, labels, direction):
    keys = O2M if direction == "real_trained_on_synthetic" else M2O
    kept = [i for i in range(len(labels)) if int(labels[i]) in keys]
    return [data[i] for i in kept], [int(labels[i]) for i in kept]


def whole_batches(n, batch_size):
    return (n // batch_size) * batch_size


def _first_argmax(row):
    best = 0
    for j in range(1, len(row)):
        if row[j] > row[best]:
            best = j
    return best


def _finish(total_seen, total_correct, seen_class, correct_class, lines, confusion, average_over_all=False):
    if total_seen == 0:
        raise SystemExit("no cloud to evaluate")
    seen_counts = [seen_class[c] for c in range(15) if seen_class[c] != 0]
    correct_counts = [correct_class[c] for c in range(15) if seen_class[c] != 0]
    ratios = np.array(correct_counts) / np.array(seen_counts, dtype=np.float64)
    avg = float(ratios.sum() / 15.0) if average_over_all else float(np.mean(ratios))
    per_class = [correct_class[c] / float(seen_class[c]) if seen_class[c] else -1.0 for c in range(15)]
    return {"total_seen": total_seen, "accuracy": total_correct / float(total_seen), "avg_class_acc": avg,
            "per_class": per_class, "lines": lines, "confusion": confusion}


def real_on_synthetic(scores40, labels15, skip_unmapped=False, average_over_all=False):
    """40-class scores against ScanObjectNN labels"""
    total_seen = total_correct = 0
    seen_class = {c: 0 for c in range(15)}
    correct_class = {c: 0 for c in range(15)}
    lines = []
    confusion = [[0] * 40 for _ in range(15)]
    for row, label in zip(scores40, labels15):
        label = int(label)
        pred = _first_argmax(row)
        confusion[label][pred] += 1
        if skip_unmapped and pred not in M2O:                   # WRONG on purpose: the cloud is not even seen
            continue
        total_seen += 1
        seen_class[label] += 1
        if pred in M2O:
            mapped = M2O[pred]
            if mapped == label:
                total_correct += 1
                correct_class[label] += 1
            lines.append("%s, %s" % (OBJECT_NAMES[mapped], OBJECT_NAMES[label]))
        else:
            lines.append("NA, %s" % OBJECT_NAMES[label])
    return _finish(total_seen, total_correct, seen_class, correct_class, lines, confusion, average_over_all)


def synthetic_on_real(scores15, labels40, index_by_raw_label=False):
    """15-class scores against (mapped) ModelNet40 labels"""
    total_seen = total_correct = 0
    slots = 40 if index_by_raw_label else 15
    seen_class = {c: 0 for c in range(slots)}
    correct_class = {c: 0 for c in range(slots)}
    lines = []
    confusion = [[0] * 15 for _ in range(40)]
    for row, label in zip(scores15, labels40):
        label = int(label)
        pred = _first_argmax(row)
        confusion[label][pred] += 1
        slot = label if index_by_raw_label else M2O[label]      # raw label: WRONG on purpose
        total_seen += 1
        seen_class[slot] += 1
        if pred in O2M and label in O2M[pred]:
            total_correct += 1
            correct_class[slot] += 1
        lines.append("%s, %s" % (OBJECT_NAMES[pred], OBJECT_NAMES[M2O[label]]))
    if index_by_raw_label:                                      # fold into what a 15-row table would print
        seen_class = {c: seen_class[c] for c in range(15)}
        correct_class = {c: correct_class[c] for c in range(15)}
    return _finish(total_seen, total_correct, seen_class, correct_class, lines, confusion)


def run(direction, predict_batch, data, labels, batch_size, filter_after_batching=False, **wrong):
    """the whole protocol on host data: filter, whole batches, scores of `predict_batch(list of clouds) -> rows`, summary.
    filter_after_batching: WRONG on purpose -- the batches are cut from the unfiltered set and thinned afterwards."""
    summary = real_on_synthetic if direction == "real_trained_on_synthetic" else synthetic_on_real
    if filter_after_batching:
        n = whole_batches(len(labels), batch_size)
        data, labels = filter_mapped(list(data[:n]), list(labels[:n]), direction)
        scores = [r for lo in range(0, len(labels), batch_size) for r in predict_batch(data[lo:lo + batch_size])]
        return summary(scores, labels, **wrong), labels
    data, labels = filter_mapped(data, labels, direction)
    n = whole_batches(len(labels), batch_size)
    scores = []
    for lo in range(0, n, batch_size):
        scores.extend(predict_batch(data[lo:lo + batch_size]))
    return summary(scores, labels[:n], **wrong), labels[:n]
