"""Training loop -- restates the step semantics of `pointnet2/train.py:136-171,218-261` (`train_seg.py` for the BGA
models, `train_partseg.py` for part segmentation) with the reference's flag names (`train.py:25-46`), data-parallel
over the GPUs of one node.

  python -m scanobjectnn_amd.pointnet2.train --model pointnet2_cls_ssg --num_point 2048 --batch_size 256 \
         --max_epoch 1 [--train_file x.npz --test_file y.npz]          (synthetic clouds when no file is given)
  python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m scanobjectnn_amd.pointnet2.train ...
  python -m scanobjectnn_amd.pointnet2.train --model pointnet_seg --batch_size 32 --num_point 1024 \
         --train_file train_withmask.h5 --test_file test_withmask.h5   (`pointnet/train_seg.py:33-35`: its batch and points)
  python -m scanobjectnn_amd.pointnet2.train --model pointnet_partseg --batch_size 32 --num_point 1024 \
         --train_file train_parts.h5 --test_file test_parts.h5         (`pointnet/train_partseg.py`)

Input pipeline, all on the device: the loaded set is uploaded ONCE, centred and normalised there
(`train.py:100-106` does it on the host: `data_utils.center_data`, `normalize_data`), the per-epoch point subset /
cloud order (`data_utils.get_current_data_h5`) is an index gather on the resident tensor, and rotate + jitter
(`provider.py:34-52,189-200`) run per batch on the device.
Per step: forward (training BN, dropout) -> loss -> backward -> ONE all-reduce of the flat gradient bucket ->
Adam / momentum with the staircase lr; bn_decay follows the reference schedule.  Loss and accuracy are accumulated
on the device and read ONCE per epoch (no per-step host synchronisation).  `--graph` (single rank, the families listed in
`captured_step.py`): that step is captured once as a HIP graph and replayed, with the input pipeline above staying outside
the graph; evaluation, checkpoints and everything else are the same either way.  `--device_feed` (`device_feed.py`): that
input pipeline as ONE launch per step on the resident set -- raw `.bin` split lists included, which then live on the device --
with counter-based random numbers; under `--graph` the launch is part of the captured step.  A checkpoint (`model.pt`, variables under
the reference's TF scope names) is written every epoch after the BN moving statistics were made rank 0's.
"""
import argparse
import importlib
import json
import os
import time

import numpy as np
import torch

from .. import captured_step as CS, data_utils, device_feed as DF, dist as D, provider
from .. import train_util as TU
from ..graph import Model
from ..synth import synth_clouds, synth_labels, synth_masks
from . import evaluate_scenennobjects as EV

MODELS = {"pointnet2_cls_ssg": "scanobjectnn_amd.pointnet2.pointnet2_cls_ssg",
          "pointnet2_cls_bga": "scanobjectnn_amd.pointnet2.pointnet2_cls_bga",
          "pointnet2_cls_msg": "scanobjectnn_amd.pointnet2.pointnet2_cls_msg",
          "pointnet2_cls_partseg": "scanobjectnn_amd.pointnet2.pointnet2_cls_partseg",
          "dgcnn": "scanobjectnn_amd.dgcnn.dgcnn", "dgcnn_bga": "scanobjectnn_amd.dgcnn.dgcnn_bga",
          "spidercnn_cls_xyz": "scanobjectnn_amd.spidercnn.spidercnn_cls_xyz",
          "3dmfv_net_cls": "scanobjectnn_amd.mfv3d.mfv3d_net_cls",
          "pointcnn_cls": "scanobjectnn_amd.pointcnn.pointcnn_cls",
          "pointcnn_seg": "scanobjectnn_amd.pointcnn.pointcnn_seg",
          "pointnet_cls": "scanobjectnn_amd.pointnet.pointnet_cls",
          "pointnet_cls_basic": "scanobjectnn_amd.pointnet.pointnet_cls_basic",
          "pointnet_seg": "scanobjectnn_amd.pointnet.pointnet_seg",
          "pointnet_partseg": "scanobjectnn_amd.pointnet.pointnet_partseg"}
# the models that predict a per-point foreground mask beside the class (the reference's train_seg.py trainers)
MASK_MODELS = frozenset(m for m in MODELS if m.endswith("_bga")) | {"pointcnn_seg"}
# ... whose get_model also returns end points that their get_loss takes (pointnet/train_seg.py: the transform regulariser)
MASK_MODELS_END_POINTS = frozenset({"pointnet_seg"})
ALL_MASK_MODELS = MASK_MODELS | MASK_MODELS_END_POINTS
# flags a model may take from its own setting when the command line leaves them out (the module's flag_defaults);
# for every other model these are the defaults
FLAG_DEFAULTS = {"max_epoch": 250, "batch_size": 16, "learning_rate": 0.001, "decay_step": 200000, "decay_rate": 0.7}


def add_model_flags(p):
    """flags of one family that the trainer and the evaluation share (3DmFV-Net/train.py:49-54)"""
    p.add_argument("--weight_decay", type=float, default=0.0,
                   help="3dmfv_net_cls: handed to the FC layers as in the reference, whose loss never adds the collected terms")
    p.add_argument("--gmm_type", default="grid", help="3dmfv_net_cls: grid (learn, the EM mixture, is out of scope and raises)")
    p.add_argument("--num_gaussians", type=int, default=5, help="3dmfv_net_cls: grid subdivisions per axis (5: 125 Gaussians)")
    p.add_argument("--gmm_variance", type=float, default=0.04, help="3dmfv_net_cls: variance of every grid Gaussian")
    p.add_argument("--setting", default=None, help="pointcnn_cls / pointcnn_seg: the setting (PointCNN/train.py:41) "
                   "[the model's own: modelnet_x3_l4 / object_dataset_x3; modelnet40_expt: modelnet_x3_l4 with 40 classes].  "
                   "pointcnn_cls takes the flags it is not given from its setting, --num_class included; pointcnn_seg keeps this file's defaults: give --learning_rate 0.01 --decay_step 8000 "
                   "--decay_rate 0.5 --batch_size 32 --max_epoch 400 for object_dataset_x3's numbers")


def resolve_model_flags(args, num_class=15, setting=None):
    """--setting left out: the model's own setting (modelnet_x3_l4 for every model that reads none); `setting`: a command
    line's own {model: setting} defaults, looked up first.  --num_class left out: the class count of the setting for the
    models that take it from there (pointcnn_cls), `num_class` for every other model."""
    from ..pointcnn import settings as S
    if args.setting is None:
        args.setting = (setting or {}).get(args.model) or S.MODEL_DEFAULT.get(args.model, "modelnet_x3_l4")
    if getattr(args, "num_class", num_class) is None:
        args.num_class = S.get(args.setting).num_class if args.model in S.NUM_CLASS_FROM_SETTING else num_class
    return args


def own_trainer(mod, args):
    """the trainer numbers a model brings instead of this file's defaults (PointCNN: Adam's epsilon, the lr schedule in
    steps, the regulariser, the augmentation): the module's own `trainer` hook, or the hook of the module that its
    TRAINER_FROM names -- pointcnn_seg trains with pointcnn_cls's and defines none of its own; None for every other model"""
    if hasattr(mod, "trainer"):
        return mod.trainer(args)
    if hasattr(mod, "TRAINER_FROM"):
        return importlib.import_module(mod.TRAINER_FROM).trainer(args)
    return None


def model_fn(mod, args, dev):
    """the get_model(point_cloud, is_training, bn_decay, **kw) graph.Model takes: the module's own, or what the module
    binds from the flags (3DmFV-Net: the mixture is an input of its get_model)"""
    return mod.model_fn(args, dev) if hasattr(mod, "model_fn") else mod.get_model


def _flag(v):
    """the reference declares its switches as `default = True` without a type, so ANY string on the command line
    is truthy there; typed properly here"""
    if isinstance(v, bool):
        return v
    if v.lower() in ("1", "true", "yes", "y", "t"):
        return True
    if v.lower() in ("0", "false", "no", "n", "f"):
        return False
    raise argparse.ArgumentTypeError("expected a boolean, got %r" % (v,))


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gpu", type=int, default=0, help="GPU to use when not launched by torchrun (train.py:26)")
    p.add_argument("--model", default="pointnet2_cls_ssg", choices=sorted(MODELS))
    p.add_argument("--log_dir", default="log")
    p.add_argument("--with_bg", type=_flag, default=True, help="keep background points of raw .bin objects (:30)")
    p.add_argument("--norm", type=_flag, default=True, help="divide every cloud by its max L2 norm (:31)")
    p.add_argument("--center_data", type=_flag, default=True, help="subtract every cloud's centroid (:32)")
    p.add_argument("--num_class", type=int, default=None, help="[15; pointcnn_cls: its setting's]")    # :33
    p.add_argument("--num_point", type=int, default=1024)           # :38
    p.add_argument("--max_epoch", type=int, default=None, help="[250]")             # :39
    p.add_argument("--batch_size", type=int, default=None, help="GLOBAL batch, split over the ranks [16]")
    p.add_argument("--learning_rate", type=float, default=None, help="[0.001]")
    p.add_argument("--momentum", type=float, default=0.9)           # :41
    p.add_argument("--optimizer", default="adam", choices=["adam", "momentum"])   # :42
    p.add_argument("--decay_step", type=int, default=None, help="[200000]")
    p.add_argument("--decay_rate", type=float, default=None, help="[0.7]")
    p.add_argument("--normal", action="store_true", help="accepted for CLI compatibility (:46); the reference never reads it")
    p.add_argument("--seg_weight", type=float, default=0.5)         # train_seg.py:35 (typed properly)
    p.add_argument("--train_file", default="")
    p.add_argument("--test_file", default="")
    p.add_argument("--data_path", default="", help="root of the raw objects_bin/ files for pickled split lists")
    p.add_argument("--synthetic_clouds", type=int, default=2048)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--sync_bn", action="store_true", help="BN statistics of the global batch (all-reduced)")
    p.add_argument("--no_augment", action="store_true", help="skip rotate + jitter (tests / debugging)")
    p.add_argument("--deterministic", action="store_true",
                   help="bit-reproducible backward passes: ordered owner sums instead of float atomics (slower)")
    p.add_argument("--graph", action="store_true",
                   help="capture one training step as a HIP graph and replay it every step (captured_step.py); a run that "
                   "cannot be captured says why in one line and trains eagerly")
    p.add_argument("--device_feed", action="store_true",
                   help="build every step's batch on the device in one launch (device_feed.py): selection, labels, mask and "
                   "the augmentation, with counter-based random numbers; raw .bin sets then live on the device and may train "
                   "under --graph.  A run it cannot feed says why in one line and trains on the host-fed path")
    add_model_flags(p)
    args = resolve_model_flags(p.parse_args(argv))
    mod = importlib.import_module(MODELS[args.model])
    own = mod.flag_defaults(args) if hasattr(mod, "flag_defaults") else {}
    for name, default in FLAG_DEFAULTS.items():
        if getattr(args, name) is None:
            setattr(args, name, own.get(name, default))
    return args


def _load(path, with_mask, num, n_pts, seed, args):
    """-> (data (K,n,3) f32 | list of ragged clouds, labels, mask | None) on the host, NOT yet centred / normalised"""
    if with_mask == "parts":            # part segmentation: per-point part ids 0..5 (`train_partseg.py:93-94`)
        if path:
            return data_utils.load_npz(path, "parts") if path.endswith(".npz") else data_utils.load_parts_h5(path)
        data = synth_clouds(num, max(n_pts, 2048), seed=seed)
        parts = (np.floor((data[:, :, 1] + 1.0) * 3.0).clip(0, 5)).astype(np.int32)   # six height bands
        return data, synth_labels(num, seed), parts
    if path:
        if path.endswith(".npz"):
            arrs = data_utils.load_npz(path, with_mask)
        elif ".h5" in path:                                     # train.py:91-99
            arrs = data_utils.load_withmask_h5(path) if with_mask else data_utils.load_h5(path)
        else:                                                   # pickled split list + raw .bin objects
            if with_mask:
                raise ValueError("%s: pickled split lists of raw .bin objects carry no per-point masks; the mask / part "
                                 "models need an .h5 / .npz file with a 'mask' / 'parts' array" % path)
            arrs = data_utils.load_data(path, n_pts, with_bg_pl=args.with_bg, data_path=args.data_path)
        if with_mask:
            return arrs[0], arrs[1], data_utils.convert_to_binary_mask(arrs[2])
        return arrs[0], arrs[1], None
    data = synth_clouds(num, max(n_pts, 2048), seed=seed)
    return data, synth_labels(num, seed), synth_masks(num, data.shape[1], seed) if with_mask else None


def prepare_set(data, labels, mask, args, dev):
    """upload once; centre + normalise ON THE DEVICE exactly as `train.py:100-106` does on the host.  Ragged sets
    (raw .bin objects) are preprocessed per cloud on the host, as the reference's in-place loops do."""
    if isinstance(data, list):
        if args.center_data:
            data = [pc - pc.mean(axis=0, dtype=np.float32) for pc in data]
        if args.norm:
            data = [pc / np.sqrt((pc * pc).sum(axis=-1, dtype=np.float32)).max() for pc in data]
        return data, np.asarray(labels), mask
    x = torch.as_tensor(np.ascontiguousarray(data, dtype=np.float32), device=dev)
    if args.center_data:
        x = data_utils.center_data_device(x)
    if args.norm:
        x = data_utils.normalize_data_device(x)
    lab = torch.as_tensor(np.asarray(labels).reshape(-1).astype(np.int64), device=dev)
    m = None
    if mask is not None:
        mask = np.asarray(mask)
        m = torch.as_tensor((mask.reshape(mask.shape[0], -1) if mask.ndim == 3 else mask).astype(np.int64), device=dev)
    return x, lab, m


def epoch_view(data, labels, mask, num_point, rng, dev):
    """this epoch's (clouds, labels, mask) on the device: ONE random point subset shared by all clouds + a random
    cloud order (`data_utils.get_current_data_h5 / _withmask_h5 / _parts_h5`), as an index gather on the resident set"""
    if isinstance(data, list):                                  # ragged: per-cloud subsets on the host, then upload
        cur, lab = data_utils.get_current_data(data, labels, num_point, rng=rng)
        return (torch.as_tensor(cur, dtype=torch.float32, device=dev),
                torch.as_tensor(lab.astype(np.int64), device=dev), None)
    idx_pts, idx = data_utils.epoch_indices(data.shape[0], data.shape[1], num_point, rng)
    ip = torch.as_tensor(idx_pts, device=dev)
    ic = torch.as_tensor(idx, device=dev)
    cur = data.index_select(1, ip).index_select(0, ic)
    msk = mask.index_select(1, ip).index_select(0, ic) if mask is not None else None
    return cur, labels.index_select(0, ic), msk


def train(args, state=None):
    """-> the epoch records; `state`: a dict that receives the run's model, flat parameters, optimiser and last epoch's
    running sums"""
    rank, world, local = D.init_from_env()
    if world == 1:
        if not 0 <= args.gpu < torch.cuda.device_count():
            raise RuntimeError("--gpu %d: no such device (%d visible)" % (args.gpu, torch.cuda.device_count()))
        local = args.gpu
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    D.SYNC_BN = bool(args.sync_bn)
    if args.deterministic:
        from scanobjectnn_amd import _lib
        _lib.set_deterministic(True)
    mod = importlib.import_module(MODELS[args.model])
    partseg = args.model.endswith("_partseg")
    with_mask = "parts" if partseg else args.model in ALL_MASK_MODELS
    per_rank = args.batch_size // world
    rng = np.random.RandomState(args.seed)          # same stream on every rank -> same epoch order
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed + 1000 + rank)
    train_data, train_lab, train_mask = prepare_set(
        *_load(args.train_file, with_mask, args.synthetic_clouds, args.num_point, 1, args), args, dev)
    test_data, test_lab, test_mask = prepare_set(
        *_load(args.test_file, with_mask, max(args.batch_size, 256), args.num_point, 2, args), args, dev)

    example = torch.zeros((2, args.num_point, 3), device=dev)
    kw = {"num_class": args.num_class} if args.num_class != 15 else {}
    net = Model(model_fn(mod, args, dev), device=dev, seed=args.seed, **kw).build(example)
    fp = TU.FlatParams(net).enable_overlap(world)        # N > 1: gradient ranges travel while the backward pass runs
    D.broadcast_(fp.flat)
    own = own_trainer(mod, args)                                   # a model with trainer numbers of its own (PointCNN)
    opt = TU.make_optimizer(args.optimizer, fp, args.momentum, **({"epsilon": own.adam_epsilon} if own else {}))
    augment = own.augment if own else getattr(mod, "augment", None)
    scores = getattr(mod, "class_scores", lambda logits: logits)     # what argmax and the votes are taken on
    step = 0
    if rank == 0:
        os.makedirs(args.log_dir, exist_ok=True)
    log = []
    lo, hi = D.shard_range(args.batch_size, rank, world)

    def step_body(x, y, m, bn_decay, tot, update):
        """forward, loss, backward, gradient collection, the optimiser (`update`) and the epoch's running sums: one training
        step, which is also what --graph captures"""
        fp.begin_step()
        out = net(x, is_training=True, bn_decay=bn_decay)
        if partseg:
            seg_pred, end_points = EV.split_output(out)     # pointnet_partseg: (seg_pred, end_points)
            loss = mod.get_loss(seg_pred, m) if end_points is None else mod.get_loss(seg_pred, m, end_points)
        elif with_mask:
            if args.model in MASK_MODELS_END_POINTS:
                loss = mod.get_loss(out[0], out[1], y, m, out[2], seg_weight=args.seg_weight)[0]
            else:
                loss = mod.get_loss(out[0], out[1], y, m, seg_weight=args.seg_weight)[0]
        else:
            logits, end_points = EV.split_output(out)      # SpiderCNN returns bare logits
            loss = EV.model_loss(mod, logits, y, end_points)
        if own:                                                   # minimised, not reported (PointCNN/train.py:171)
            (loss + own.regularization_loss(net)).backward()
        else:
            loss.backward()
        fp.collect_mean(world)
        update()
        with torch.no_grad():
            tot[0] += loss.detach()
            if partseg:                      # point accuracy (`train_partseg.py:237-241`)
                tot[1] += (seg_pred.argmax(dim=2) == m).sum()
                tot[2] += per_rank * args.num_point
            else:
                tot[1] += (scores(EV.split_output(out)[0]).argmax(dim=1) == y).sum()
                tot[2] += per_rank

    feed = test_feed = None                          # --device_feed: the step's batch from one launch on the resident set
    if getattr(args, "device_feed", False):
        why = DF.refusal(args, mod, own, dev.type)        # decided here, before anything runs
        if why is not None:
            print("--device_feed refused, training on the host-fed path: %s" % why, flush=True)
            args.device_feed = False                      # (what captured_step.refusal reads below)
        else:
            recipe, consts = DF.recipe_of(args, mod)
            feed = DF.DeviceFeed(train_data, train_lab, train_mask, args.num_point, per_rank, args.seed + 1000, recipe,
                                 consts, dev)
            if isinstance(test_data, list):               # a ragged evaluation set: its epoch views come from a feed as well
                test_feed = DF.DeviceFeed(test_data, test_lab, None, args.num_point, 1, args.seed + 2000, 0, consts, dev)
    captured = None                                  # --graph: the step as one captured HIP graph, built at the first batch
    use_graph = bool(getattr(args, "graph", False))
    if use_graph:
        why = CS.refusal(args, world, os.environ)         # decided here, never by catching a capture that failed
        if why is not None:
            print("--graph refused, training eagerly: %s" % why, flush=True)
            use_graph = False
    for epoch in range(args.max_epoch):
        if feed is not None:                                       # the host draws the epoch's order (and shared point list)
            feed.begin_epoch(rng, epoch)
            nb = feed.K // args.batch_size
        else:
            cur, lab, msk = epoch_view(train_data, train_lab, train_mask, args.num_point, rng, dev)
            nb = cur.shape[0] // args.batch_size
        t0 = time.time()
        tot = torch.zeros(3, dtype=torch.float64, device=dev)      # loss sum, correct, seen -- read once per epoch
        if captured is not None:
            tot = captured.tot.zero_()                             # ... accumulated inside the graph
        for b in range(nb):
            if own:                                                   # the model's schedule (PointCNN: in steps) on the same flags
                lr = own.learning_rate(step)
            else:
                lr = TU.get_learning_rate(step, args.batch_size, args.learning_rate, args.decay_step, args.decay_rate)
            bn_decay = TU.get_bn_decay(step, args.batch_size, float(args.decay_step))
            if feed is not None:                # x, y, m from one launch: this rank's first cloud by its position in the order
                batch = (b * args.batch_size + lo, step)
                x = y = m = None
            else:
                sl = slice(b * args.batch_size + lo, b * args.batch_size + hi)
                x = cur[sl]
                if not args.no_augment and augment is not None:           # a family with its own augmentation (3DmFV-Net)
                    x = augment(x, generator=gen)
                elif not args.no_augment:
                    x = provider.jitter_point_cloud(provider.rotate_point_cloud(x, generator=gen), generator=gen)
                x = x.contiguous()
                y = lab[sl]
                m = msk[sl] if with_mask else None
            if use_graph:
                if captured is None:
                    captured = CS.CapturedStep(step_body, net, fp, opt, x, y, m, feed=feed)
                    tot = captured.tot
                captured.step(x, y, m, lr, bn_decay, batch=batch if feed is not None else None)
            else:
                if feed is not None:
                    feed.set_batch(*batch)
                    x, y, m = feed.launch()
                step_body(x, y, m, bn_decay, tot, lambda: opt.step(lr))
            step += 1
        if D.dist.is_initialized() and world > 1:
            D.dist.all_reduce(tot)
            tot[0] /= world
        loss_sum, correct, seen = (float(v) for v in tot.tolist())            # the epoch's only host sync
        D.broadcast_buffers_(net)                # per-rank BN moving statistics -> rank 0's, before eval / checkpoint
        # the reference draws a FRESH point subset and cloud order for every evaluation from the same global stream
        # as the training epochs (`train.py:275`: get_current_data_h5 on TEST_DATA) -- same here, same `rng`
        if test_feed is not None:                # ragged: the order from `rng`, every cloud's subset from the feed's permutation
            test_feed.begin_epoch(rng, epoch)
            td, tl, tm = test_feed.epoch_view()
        else:
            td, tl, tm = epoch_view(test_data, test_lab, test_mask, args.num_point, rng, dev)
        if partseg:
            ev = EV.eval_partseg_one_epoch(net, td, tm, per_rank, device=dev)
        elif with_mask:
            ev = EV.eval_seg_one_epoch(net, td, tl, tm, per_rank, device=dev, scores_fn=scores)
        else:
            ev = EV.eval_one_epoch(net, td, tl, per_rank, device=dev, num_classes=args.num_class, scores_fn=scores)
        rec = {"epoch": epoch, "mean_loss": loss_sum / max(nb, 1), "train_acc": correct / max(seen, 1),
               "eval_acc": ev["accuracy"], "eval_avg_class_acc": ev["avg_class_acc"],
               "clouds_per_s": nb * args.batch_size / (time.time() - t0),
               "graph": use_graph, "captures": captured.captures if captured is not None else 0}
        if "seg_accuracy" in ev:                 # BGA models: the mask accuracy of `train_seg.py:330`
            rec["eval_seg_acc"] = ev["seg_accuracy"]
        log.append(rec)
        if rank == 0:
            print(json.dumps(rec), flush=True)
            torch.save(net.state_dict(), os.path.join(args.log_dir, "model.pt"))
    if state is not None:                        # what a test compares between two runs
        state.update(net=net, fp=fp, opt=opt, tot=tot.clone(), captures=captured.captures if captured is not None else 0)
    if captured is not None:
        captured.release()
    return log


if __name__ == "__main__":
    train(parse_args())
