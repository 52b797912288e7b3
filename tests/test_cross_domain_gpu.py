"""Cross-domain evaluation on the GPU: every classifier family built at 40 classes and driven through the two command
lines, a checkpoint evaluated in a label space it was not trained in, the reference's batch of 1, the trainer's
`--num_class 40` checkpoints (state dict and TensorFlow bundle) and `draw_cmat`.

Every comparison is exact: the command line's scores are the same eval-mode forward on the same input as a direct call of
the restored model, and every metric and output file is what the per-cloud loops of tests/crossdomain_ref.py compute
from those scores."""
import importlib
import math
import os

import numpy as np
import pytest
import torch

import crossdomain_ref as R
from scanobjectnn_amd import data_utils as DU
from scanobjectnn_amd import provider
from scanobjectnn_amd.graph import Model
from scanobjectnn_amd.pointnet2 import evaluate_real_trained_on_synthetic as E1
from scanobjectnn_amd.pointnet2 import evaluate_scenennobjects as EV
from scanobjectnn_amd.pointnet2 import evaluate_synthetic_trained_on_real as E2
from scanobjectnn_amd.pointnet2 import train as T
from scanobjectnn_amd.synth import synth_clouds

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D1, D2 = "real_trained_on_synthetic", "synthetic_trained_on_real"
CLI = {D1: E1, D2: E2}
MODEL_CLASSES = {D1: 40, D2: 15}
REF_SUMMARY = {D1: R.real_on_synthetic, D2: R.synthetic_on_real}


def _num_point(model):
    return 1024 if model == "pointcnn_cls" else 512          # PointCNN's setting samples 1024


def _model_flags(model):
    return ["--model", model] + (["--setting", "modelnet40_expt"] if model == "pointcnn_cls" else [])


def _test_file(path, direction, n_clouds, n_pts, seed=41):
    """clouds that the command line still has to centre and normalise; labels walk through the test domain's whole label
    space (15: every label once, so bag, bin, box and pillow are dropped; 40: every fifth label from bench on), so the
    filter drops some and a partial batch remains"""
    raw = synth_clouds(n_clouds, n_pts + 64, seed=seed) * 2.0 + 0.7
    i = np.arange(n_clouds)
    labels = (i % 15 if direction == D1 else (3 + 5 * i) % 40).astype(np.int32)
    np.savez(path, data=raw, label=labels)
    return raw, labels


def _net(model, args, seed, num_class):
    mod = importlib.import_module(T.MODELS[model])
    kw = {"num_class": num_class} if num_class != 15 else {}
    net = Model(T.model_fn(mod, args, torch.device(DEV)), device=DEV, seed=seed, **kw)
    return mod, net.build(torch.zeros((2, args.num_point, 3), device=DEV))


def _by_hand(model, args, direction, raw, labels):
    """the protocol restated: centre, normalise, RandomState(0) subset and order, filter BEFORE batching, whole batches,
    the restored model called directly on every rotated batch, votes summed in order"""
    data = DU.normalize_data(DU.center_data(raw.copy()))
    cur, lab = DU.get_current_data_h5(data, labels, args.num_point, rng=np.random.RandomState(0))
    keys = R.O2M if direction == D1 else R.M2O
    keep = [i for i in range(len(lab)) if int(lab[i]) in keys]
    assert 0 < len(keep) < len(lab)                              # the filter dropped some, not all
    cur, lab = cur[keep], lab[keep]
    n = (len(lab) // args.batch_size) * args.batch_size
    mod, net = _net(model, args, seed=7, num_class=args.num_class)          # other initial values than the checkpoint's
    info = EV.restore(net, args.model_path)
    assert not info["missing"] and not info["unexpected"]
    scores_fn = getattr(mod, "class_scores", lambda logits: logits)
    scores = []
    with torch.no_grad():
        for lo in range(0, n, args.batch_size):
            pts = torch.as_tensor(cur[lo:lo + args.batch_size], dtype=torch.float32, device=DEV)
            total = None
            for v in range(args.num_votes):
                rot = provider.rotate_point_cloud_by_angle(pts, v / float(args.num_votes) * math.pi * 2).contiguous()
                out = scores_fn(EV.split_output(net(rot, is_training=False))[0])
                total = out if total is None else total + out
            scores.append(total.cpu().numpy())
    return np.concatenate(scores), lab[:n]


def _check(ev, dump, direction, want_scores, want_lab):
    n_model, n_test = MODEL_CLASSES[direction], MODEL_CLASSES[D2 if direction == D1 else D1]
    assert np.array_equal(ev["label"], want_lab) and len(want_lab) > 0
    assert ev["scores"].shape == (len(want_lab), n_model) and ev["scores"].dtype == want_scores.dtype
    assert np.array_equal(ev["scores"], want_scores)                          # bit for bit
    assert np.isfinite(ev["scores"]).all() and np.ptp(ev["scores"]) > 0
    ref = REF_SUMMARY[direction](ev["scores"], ev["label"])
    print("accuracy %r avg_class_acc %r seen %d" % (ev["accuracy"], ev["avg_class_acc"], len(want_lab)))
    assert ev["accuracy"] == ref["accuracy"] and ev["avg_class_acc"] == ref["avg_class_acc"]
    assert list(ev["per_class"]) == ref["per_class"]
    assert ev["confusion"].tolist() == ref["confusion"] and ev["confusion"].shape == (n_test, n_model)
    assert ev["pred"].tolist() == [int(np.argmax(row)) for row in ev["scores"]]
    assert open(os.path.join(dump, "pred_label.txt")).read().splitlines() == ref["lines"]
    rows = [r.split(",") for r in open(os.path.join(dump, "confusion.csv")).read().splitlines()]
    model_names, test_names = (R.MODELNET_NAMES, R.OBJECT_NAMES) if direction == D1 else (R.OBJECT_NAMES, R.MODELNET_NAMES)
    assert rows[0][1:] == model_names and [r[0] for r in rows[1:]] == test_names
    assert [[int(c) for c in r[1:]] for r in rows[1:]] == ref["confusion"]
    log = open(os.path.join(dump, "log_evaluate.txt")).read()
    table = ["%10s:\t%0.3f" % (name, acc) for name, acc in zip(R.OBJECT_NAMES, ref["per_class"])]
    for key in ["Model restored.", "total seen: %d" % len(want_lab), "eval accuracy: %f" % ref["accuracy"],
                "eval avg class acc: %f" % ref["avg_class_acc"], "\n".join(table)]:
        assert key in log, key
    assert "mean loss" not in log                                 # no loss in a foreign label space
    assert log.splitlines()[0].startswith("Namespace(") and "num_class=%d" % n_model in log.splitlines()[0]      # the flags


def _run(model, direction, tmp_path, n_clouds=16, batch_size=4, num_votes=2, model_path=None):
    n_pts = _num_point(model)
    raw, labels = _test_file(tmp_path / "test.npz", direction, n_clouds, n_pts)
    dump = str(tmp_path / ("dump_" + direction))
    flags = _model_flags(model) if direction == D1 else ["--model", model]
    argv = flags + ["--num_point", str(n_pts), "--batch_size", str(batch_size), "--num_votes", str(num_votes),
                    "--test_file", str(tmp_path / "test.npz"), "--dump_dir", dump,
                    "--model_path", model_path or str(tmp_path / "model.pt")]
    args = CLI[direction].parse_args(argv)
    assert args.num_class == MODEL_CLASSES[direction]
    if model_path is None:                       # an untrained model as the checkpoint
        _, net = _net(model, args, seed=0, num_class=args.num_class)
        torch.save(net.state_dict(), tmp_path / "model.pt")
        del net
    ev = CLI[direction].evaluate(args)
    want_scores, want_lab = _by_hand(model, args, direction, raw, labels)
    _check(ev, dump, direction, want_scores, want_lab)
    return ev, args


@pytest.mark.parametrize("model", ["pointnet2_cls_ssg", "dgcnn", "pointnet_cls", "spidercnn_cls_xyz", "pointcnn_cls",
                                   "3dmfv_net_cls"])
def test_real_trained_on_synthetic_every_family(model, tmp_path):
    ev, _ = _run(model, D1, tmp_path)
    assert len(ev["label"]) == 8 and set(ev["label"].tolist()) <= set(R.O2M)          # 11 of 16 kept, two whole batches


@pytest.mark.parametrize("model", ["pointnet2_cls_ssg", "pointcnn_cls", "3dmfv_net_cls"])
def test_synthetic_trained_on_real(model, tmp_path):
    ev, args = _run(model, D2, tmp_path)
    assert len(ev["label"]) == 8 and set(ev["label"].tolist()) <= set(R.M2O)          # 10 of 16 kept
    assert args.setting == "modelnet_x3_l4"


def test_batch_of_one_single_vote(tmp_path):
    """the reference's defaults: --batch_size 1 --num_votes 1"""
    n_pts = 512
    raw = synth_clouds(8, n_pts + 64, seed=43) * 2.0 + 0.7
    labels = ((2 * np.arange(8) + 1) % 15).astype(np.int32)                    # bin, cabinet, desk, door, table, pillow, sofa, bag
    np.savez(tmp_path / "test.npz", data=raw, label=labels)
    dump = str(tmp_path / "dump")
    args = E1.parse_args(["--num_point", str(n_pts), "--test_file", str(tmp_path / "test.npz"), "--dump_dir", dump,
                          "--model_path", str(tmp_path / "model.pt")])
    assert (args.batch_size, args.num_votes, args.model, args.num_class) == (1, 1, "pointnet2_cls_ssg", 40)
    _, net = _net(args.model, args, seed=0, num_class=40)
    torch.save(net.state_dict(), tmp_path / "model.pt")
    ev = E1.evaluate(args)
    want_scores, want_lab = _by_hand(args.model, args, D1, raw, labels)
    assert len(want_lab) == 5
    _check(ev, dump, D1, want_scores, want_lab)


def _train_file(path, n_clouds, n_pts, n_labels, seed):
    np.savez(path, data=synth_clouds(n_clouds, n_pts + 64, seed=seed) * 1.5 + 0.2,
             label=((7 * np.arange(n_clouds) + 1) % n_labels).astype(np.int32))


def test_trainer_checkpoint_and_tf_bundle(tmp_path):
    """train.py --num_class 40 for two steps on 40-label clouds -> model.pt -> evaluate_real_trained_on_synthetic; the same
    from a TensorFlow bundle of that checkpoint"""
    from scanobjectnn_amd import tf_checkpoint
    _train_file(tmp_path / "train40.npz", 16, 512, 40, seed=45)
    log_dir = tmp_path / "log"
    targs = T.parse_args(["--model", "pointnet2_cls_ssg", "--num_class", "40", "--num_point", "512", "--batch_size", "8",
                          "--max_epoch", "1", "--train_file", str(tmp_path / "train40.npz"),
                          "--test_file", str(tmp_path / "train40.npz"), "--log_dir", str(log_dir)])
    log = T.train(targs)
    assert len(log) == 1 and np.isfinite(log[0]["mean_loss"]) and log[0]["mean_loss"] > 0
    sd = torch.load(log_dir / "model.pt", map_location="cpu")
    assert tuple(sd["graph.fc3/biases"].shape) == (40,)
    (tmp_path / "pt").mkdir()
    ev, args = _run("pointnet2_cls_ssg", D1, tmp_path / "pt", model_path=str(log_dir / "model.pt"))
    _, net = _net("pointnet2_cls_ssg", args, seed=3, num_class=40)
    net.load_state_dict(sd)
    tf_checkpoint.save_tf_checkpoint(net, str(tmp_path / "model.ckpt"))
    assert os.path.exists(str(tmp_path / "model.ckpt") + ".index")
    (tmp_path / "tf").mkdir()
    ev_tf, _ = _run("pointnet2_cls_ssg", D1, tmp_path / "tf", model_path=str(tmp_path / "model.ckpt"))
    assert "Model restored. (tf-bundle" in open(tmp_path / "tf" / ("dump_" + D1) / "log_evaluate.txt").read()
    assert np.array_equal(ev_tf["scores"], ev["scores"]) and ev_tf["accuracy"] == ev["accuracy"]


def test_pointcnn_trainer_takes_40_classes_from_the_setting(tmp_path):
    _train_file(tmp_path / "train40.npz", 16, 512, 40, seed=46)
    targs = T.parse_args(["--model", "pointcnn_cls", "--setting", "modelnet40_expt", "--num_point", "512", "--batch_size", "8",
                          "--max_epoch", "1", "--train_file", str(tmp_path / "train40.npz"),
                          "--test_file", str(tmp_path / "train40.npz"), "--log_dir", str(tmp_path / "log")])
    assert targs.num_class == 40
    log = T.train(targs)
    assert len(log) == 1 and np.isfinite(log[0]["mean_loss"]) and log[0]["mean_loss"] > 0
    sd = torch.load(tmp_path / "log" / "model.pt", map_location="cpu")
    assert tuple(sd["graph.logits/kernel"].shape) == (192, 40) and tuple(sd["graph.logits/bias"].shape) == (40,)
    mod, net = _net("pointcnn_cls", targs, seed=1, num_class=40)
    net.load_state_dict(sd)
    x = torch.from_numpy(synth_clouds(2, 512, seed=47)).to(DEV)
    with torch.no_grad():
        assert net(x, is_training=True).shape[::2] == (2, 40)                  # (B, P_last, 40) per-point logits
        assert mod.class_scores(net(x, is_training=False)).shape == (2, 40)


@pytest.mark.parametrize("model", ["pointnet2_cls_msg", "dgcnn", "pointnet_cls", "pointnet_cls_basic", "spidercnn_cls_xyz",
                                   "3dmfv_net_cls"])
def test_every_other_classifier_trains_and_evaluates_at_40_classes(model, tmp_path):
    """the rest of train.MODELS' classifiers: two steps at --num_class 40 on labels up to 39, then the cross-domain command line
    on the trainer's checkpoint (pointnet2_cls_ssg and pointcnn_cls: the two tests above)"""
    _train_file(tmp_path / "train40.npz", 8, 512, 40, seed=48)
    targs = T.parse_args(["--model", model, "--num_class", "40", "--num_point", "512", "--batch_size", "4", "--max_epoch", "1",
                          "--train_file", str(tmp_path / "train40.npz"), "--test_file", str(tmp_path / "train40.npz"),
                          "--log_dir", str(tmp_path / "log")])
    log = T.train(targs)
    assert len(log) == 1 and np.isfinite(log[0]["mean_loss"]) and log[0]["mean_loss"] > 0
    ev, _ = _run(model, D1, tmp_path, model_path=str(tmp_path / "log" / "model.pt"))
    assert ev["scores"].shape == (8, 40)


def test_draw_cmat(tmp_path):
    from scanobjectnn_amd.pointnet2 import draw_cmat
    _, net = _net("pointnet2_cls_ssg", EV.parse_args(["--num_point", "512"]), seed=0, num_class=15)
    torch.save(net.state_dict(), tmp_path / "model.pt")
    flags = ["--num_point", "512", "--batch_size", "4", "--num_votes", "2", "--synthetic_clouds", "16",
             "--model_path", str(tmp_path / "model.pt")]
    out = draw_cmat.draw(draw_cmat.parse_args(flags + ["--dump_dir", str(tmp_path / "cmat")]))
    ev = EV.evaluate(EV.parse_args(flags + ["--dump_dir", str(tmp_path / "dump")]))
    assert np.array_equal(out["pred"], ev["pred"]) and np.array_equal(out["label"], ev["label"]) and len(ev["pred"]) == 16
    mat = np.loadtxt(tmp_path / "cmat" / "matrix.csv", delimiter=",")
    assert mat.shape == (15, 15)
    counts = [[0] * 15 for _ in range(15)]
    for p, l in zip(ev["pred"], ev["label"]):
        counts[int(l)][int(p)] += 1
    for row, got in zip(counts, mat):
        total = sum(row)
        assert got.tolist() == [c / float(total) if total else 0.0 for c in row]
        # a row of c_i / total, each rounded once (half an ulp of a value <= 1), summed in 14 additions that each round
        # a value <= 1 again: within 15 * 2^-52 of 1 -- or exactly 0 for a class that never occurs
        assert abs(got.sum() - 1.0) <= 15 * 2.0 ** -52 if total else got.sum() == 0.0
    assert any(sum(r) == 0 for r in counts) and any(sum(r) > 0 for r in counts)
    assert os.path.exists(tmp_path / "cmat" / "pred_label.txt")             # the evaluation's own outputs, by calling it
    assert os.path.exists(tmp_path / "cmat" / "matrix.pdf") == out["plotted"]
