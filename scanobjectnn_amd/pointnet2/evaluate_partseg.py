"""Evaluation of the part-segmentation models -- the caller `pointnet/evaluate_partseg.py` restated (`pointnet2/
evaluate_partseg.py` is the same script on `pointnet2_cls_partseg`): its command line (`:20-37`), the restore (`:104`), the
loop (`:117-192`: ONE random point subset and cloud order from `np.random.seed(0)`, whole batches, the loss of every batch
weighted by its size) and what it reports (`:186-192`): total seen, mean loss, `seg accuracy = correct points / (seen clouds *
points)`, the mean accuracy over the part classes that occur, and the accuracy per part (-1 for a part that never occurs).
Output: `dump_dir/log_evaluate.txt`.  The reference's vote loop feeds the unrotated cloud at every vote; it runs one.  Visual
dumps (`--visu`, `--visu_mask`) are out of scope; the flags are accepted.

  python -m scanobjectnn_amd.pointnet2.evaluate_partseg --model pointnet_partseg --num_point 1024 --batch_size 32 \
         --model_path log/model.pt --test_file test_parts.h5

`--model` is `pointnet_partseg` or `pointnet2_cls_partseg`.  `--model_path`: this package's `model.pt`, or the prefix of a
TensorFlow tensor bundle (as evaluate_scenennobjects).
"""
import argparse
import importlib
import os

import numpy as np
import torch

from .. import data_utils
from .evaluate_scenennobjects import _host, restore, split_output

NUM_CLASSES = 6
# training_data/part_labels/chair_parts.txt (part id order)
PART_NAMES = ["background", "head", "back", "arm", "base", "seat"]


def part_models():
    from .train import MODELS
    return sorted(m for m in MODELS if m.endswith("_partseg"))


@torch.no_grad()
def eval_parts(net, data, parts, batch_size, device="cuda:0", num_classes=NUM_CLASSES, loss_fn=None):
    """net: graph.Model of a part model -> seg_pred (B,N,C) or (seg_pred, end_points); data (K,N,3), parts (K,N).  Whole
    batches only.  loss_fn(seg_pred, parts, end_points) -> the loss of one batch, accumulated as loss * batch (`:155`)."""
    parts = _host(parts)
    seen_c = np.zeros(num_classes, dtype=np.int64)
    corr_c = np.zeros(num_classes, dtype=np.int64)
    total_seen, total_correct, loss_sum = 0, 0, 0.0
    for b in range(data.shape[0] // batch_size):
        sl = slice(b * batch_size, (b + 1) * batch_size)
        pts = torch.as_tensor(data[sl], dtype=torch.float32, device=device)
        gt = np.asarray(parts[sl])
        seg_pred, end_points = split_output(net(pts.contiguous(), is_training=False))
        if loss_fn is not None:
            loss_sum += float(loss_fn(seg_pred, torch.as_tensor(gt.astype(np.int64), device=device), end_points)) * batch_size
        pred = seg_pred.argmax(dim=2).cpu().numpy()
        total_correct += int((pred == gt).sum())
        total_seen += batch_size
        for c in range(num_classes):
            seen_c[c] += int((gt == c).sum())
            corr_c[c] += int(((gt == c) & (pred == c)).sum())
    occurs = seen_c > 0
    part_accs = np.where(occurs, corr_c / np.maximum(seen_c, 1), -1.0)
    return {"total_seen": total_seen, "mean_loss": loss_sum / max(total_seen, 1),
            "seg_accuracy": total_correct / (float(max(total_seen, 1)) * data.shape[1]),
            "avg_class_acc": float(part_accs[occurs].mean()) if occurs.any() else 0.0, "per_part": part_accs.tolist()}


def parse_args(argv=None):
    from .train import _flag
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--gpu", type=int, default=0, help="GPU to use (:21)")
    p.add_argument("--model", default="pointnet_partseg", choices=part_models())                # :22
    p.add_argument("--batch_size", type=int, default=1)                                       # :23
    p.add_argument("--num_point", type=int, default=1024)                                     # :24
    p.add_argument("--model_path", default="log/model.ckpt",
                   help="model.pt of this package, or the prefix of a TensorFlow tensor bundle (:26)")
    p.add_argument("--dump_dir", default="dump/")                                             # :27
    p.add_argument("--with_bg", type=_flag, default=True)                                     # :28
    p.add_argument("--norm", type=_flag, default=True)                                        # :29
    p.add_argument("--center_data", type=_flag, default=True)                                 # :30
    p.add_argument("--test_file", default="", help=".npz / .h5 with data, label, parts (:34); synthetic clouds if empty")
    p.add_argument("--visu_mask", type=_flag, default=False, help="accepted (:36); mask dumps are out of scope")
    p.add_argument("--visu", type=_flag, default=False, help="accepted (:37); image dumps are out of scope")
    p.add_argument("--synthetic_clouds", type=int, default=256)
    return p.parse_args(argv)


def load_test_set(args):
    """(:68-74): load with part labels, centre, normalise on the host exactly like the reference"""
    if not args.test_file:
        from ..synth import synth_clouds, synth_labels
        data = synth_clouds(args.synthetic_clouds, max(args.num_point, 2048), seed=2)
        labels = synth_labels(args.synthetic_clouds, 2)
        parts = (np.floor((data[:, :, 1] + 1.0) * 3.0).clip(0, 5)).astype(np.int32)    # six height bands, as the trainer's
    elif args.test_file.endswith(".npz"):
        data, labels, parts = data_utils.load_npz(args.test_file, "parts")
    else:
        data, labels, parts = data_utils.load_parts_h5(args.test_file)
    if args.center_data:
        data = data_utils.center_data(data)
    if args.norm:
        data = data_utils.normalize_data(data)
    return data, np.asarray(labels).reshape(-1), parts


def evaluate(args):
    from ..graph import Model
    from .train import MODELS
    if not torch.cuda.is_available() or not 0 <= args.gpu < torch.cuda.device_count():
        raise RuntimeError("--gpu %d: no such device (%d visible)" % (args.gpu, torch.cuda.device_count()))
    dev = torch.device("cuda", args.gpu)
    torch.cuda.set_device(dev)
    mod = importlib.import_module(MODELS[args.model])
    os.makedirs(args.dump_dir, exist_ok=True)
    log_f = open(os.path.join(args.dump_dir, "log_evaluate.txt"), "w")
    log_f.write(str(args) + "\n")

    def log_string(s):
        log_f.write(s + "\n")
        log_f.flush()
        print(s)

    rng = np.random.RandomState(0)                 # `np.random.seed(0)` (:63)
    data, labels, parts = load_test_set(args)
    net = Model(mod.get_model, device=dev, seed=0).build(torch.zeros((2, args.num_point, 3), device=dev))
    info = restore(net, args.model_path)
    log_string("Model restored. (%s, %d variables)" % (info["format"], info["loaded"]))
    cur, _lab, cur_parts = data_utils.get_current_data_parts_h5(data, labels, parts, args.num_point, rng=rng)   # :128

    def loss_fn(seg_pred, gt, end_points):
        return mod.get_loss(seg_pred, gt) if end_points is None else mod.get_loss(seg_pred, gt, end_points)

    ev = eval_parts(net, cur, np.squeeze(cur_parts), args.batch_size, device=dev, loss_fn=loss_fn)
    log_string("total seen: %d" % ev["total_seen"])
    log_string("eval mean loss: %f" % ev["mean_loss"])
    log_string("eval seg accuracy: %f" % ev["seg_accuracy"])
    log_string("eval avg class acc: %f" % ev["avg_class_acc"])
    for i, name in enumerate(PART_NAMES):
        log_string("%10s:\t%0.3f" % (name, ev["per_part"][i]))
    log_f.close()
    return ev


if __name__ == "__main__":
    evaluate(parse_args())
