"""Cross-domain evaluation on the host: the class maps against the two name fixtures, the two metric summaries against
hand-computed cases and against the per-cloud loops of tests/crossdomain_ref.py (exact equality of every number, line and
matrix entry), `vote_scores` with a stub model, the command lines' defaults, and one wrong restatement per rule that the
comparison has to reject."""
import math

import numpy as np
import pytest
import torch

import crossdomain_ref as R
from scanobjectnn_amd import class_maps as CM
from scanobjectnn_amd.pointnet2 import cross_domain as CD

D1, D2 = CD.REAL_ON_SYNTHETIC, CD.SYNTHETIC_ON_REAL
SUMMARY = {D1: CD.summarize_real_on_synthetic, D2: CD.summarize_synthetic_on_real}


def _one_hot_scores(pred, width):
    s = np.zeros((len(pred), width), dtype=np.float32)
    s[np.arange(len(pred)), pred] = 1.0
    return s


def _same(ev, ref):
    """every number, line and confusion entry of the product summary equals the loops'"""
    assert ev["total_seen"] == ref["total_seen"]
    assert ev["accuracy"] == ref["accuracy"]
    assert ev["avg_class_acc"] == ref["avg_class_acc"]
    assert list(ev["per_class"]) == ref["per_class"]
    assert ev["lines"] == ref["lines"]
    assert ev["confusion"].tolist() == ref["confusion"]


def _differs(ev, ref):
    return (ev["total_seen"] != ref["total_seen"] or ev["accuracy"] != ref["accuracy"]
            or ev["avg_class_acc"] != ref["avg_class_acc"] or list(ev["per_class"]) != ref["per_class"]
            or ev["lines"] != ref["lines"])


# ---- the maps ------------------------------------------------------------------------------------------------------
def test_maps_against_the_name_fixtures():
    from scanobjectnn_amd.pointnet2 import evaluate_scenennobjects as EV
    assert CM.MODELNET_SHAPE_NAMES == R.MODELNET_NAMES and len(R.MODELNET_NAMES) == 40
    assert CM.MODELNET_SHAPE_NAMES[0] == "airplane" and CM.MODELNET_SHAPE_NAMES[39] == "xbox"
    assert CM.OBJECTDATASET_SHAPE_NAMES is EV.SHAPE_NAMES and EV.SHAPE_NAMES == R.OBJECT_NAMES      # imported, not copied
    assert CM.MODELNET_TO_OBJECTDATASET == R.M2O and len(CM.MODELNET_TO_OBJECTDATASET) == 14
    by_name = {CM.MODELNET_SHAPE_NAMES[m]: EV.SHAPE_NAMES[o] for m, o in CM.MODELNET_TO_OBJECTDATASET.items()}
    assert by_name == {"bed": "bed", "bookshelf": "shelf", "chair": "chair", "desk": "desk", "door": "door",
                       "dresser": "cabinet", "wardrobe": "cabinet", "monitor": "display", "bench": "chair",
                       "stool": "chair", "sink": "sink", "sofa": "sofa", "table": "table", "toilet": "toilet"}
    inv = CM.OBJECTDATASET_TO_MODELNET
    assert len(inv) == 11 and inv == R.O2M
    assert sorted(m for ms in inv.values() for m in ms) == sorted(CM.MODELNET_TO_OBJECTDATASET)
    for o, ms in inv.items():
        assert isinstance(ms, list) and all(CM.MODELNET_TO_OBJECTDATASET[m] == o for m in ms)
    name = EV.SHAPE_NAMES.index
    assert {CM.MODELNET_SHAPE_NAMES[m] for m in inv[name("chair")]} == {"chair", "bench", "stool"}
    assert {CM.MODELNET_SHAPE_NAMES[m] for m in inv[name("cabinet")]} == {"dresser", "wardrobe"}
    assert not {name("bag"), name("bin"), name("box"), name("pillow")} & set(inv)
    assert list(CM.OBJECTDATASET_TO_COMBINED) == sorted(inv) and list(CM.OBJECTDATASET_TO_COMBINED.values()) == list(range(11))


# ---- hand-computed cases -------------------------------------------------------------------------------------------
def test_hand_case_real_trained_on_synthetic():
    labels = np.array([4, 4, 3, 0, 11, 10, 5])
    data = np.arange(7, dtype=np.float32).reshape(7, 1, 1) * np.ones((1, 2, 3), dtype=np.float32)
    kept, lab = CD.select_mapped(data, labels, D1)
    assert lab.tolist() == [4, 4, 3, 10, 5] and kept[:, 0, 0].tolist() == [0, 1, 2, 5, 6]      # bag and pillow dropped
    lab = lab[:(len(lab) // 2) * 2]
    assert lab.tolist() == [4, 4, 3, 10]
    ev = CD.summarize_real_on_synthetic(_one_hot_scores([8, 3, 0, 2], 40), lab)
    assert ev["accuracy"] == 0.75 and ev["total_seen"] == 4 and ev["pred"].tolist() == [8, 3, 0, 2]
    want = [-1.0] * 15
    want[3], want[4], want[10] = 0.0, 1.0, 1.0                    # cabinet, chair, bed
    assert list(ev["per_class"]) == want
    assert ev["avg_class_acc"] == 2.0 / 3.0
    assert ev["lines"] == ["chair, chair", "chair, chair", "NA, cabinet", "bed, bed"]
    assert ev["confusion"].shape == (15, 40) and ev["confusion"].sum() == 4
    assert ev["confusion"][4, 8] == 1 and ev["confusion"][4, 3] == 1 and ev["confusion"][3, 0] == 1 and ev["confusion"][10, 2] == 1
    _same(ev, R.real_on_synthetic(_one_hot_scores([8, 3, 0, 2], 40), lab))


def test_hand_case_synthetic_trained_on_real():
    labels = np.array([8, 32, 3, 0, 38, 14, 30])
    data = np.zeros((7, 2, 3), dtype=np.float32)
    _, lab = CD.select_mapped(data, labels, D2)
    assert lab.tolist() == [8, 32, 3, 38, 14, 30]                 # airplane dropped
    lab = lab[:(len(lab) // 3) * 3]
    assert len(lab) == 6
    scores = _one_hot_scores([4, 4, 9, 3, 0, 13], 15)
    ev = CD.summarize_synthetic_on_real(scores, lab)
    assert ev["total_seen"] == 6 and ev["total_correct"] == 4 and ev["accuracy"] == 4 / 6.0
    want = [-1.0] * 15
    want[3], want[4], want[13] = 0.5, 2 / 3.0, 1.0                # cabinet, chair, sofa
    assert list(ev["per_class"]) == want
    assert ev["avg_class_acc"] == 13.0 / 18.0
    assert ev["lines"] == ["chair, chair", "chair, chair", "table, chair", "cabinet, cabinet", "bag, cabinet", "sofa, sofa"]
    assert ev["confusion"].shape == (40, 15) and ev["confusion"][32, 4] == 1 and ev["confusion"][14, 0] == 1
    _same(ev, R.synthetic_on_real(scores, lab))
    with pytest.raises(ValueError, match="select_mapped"):
        CD.summarize_synthetic_on_real(_one_hot_scores([0], 15), np.array([0]))       # airplane: not filtered


# ---- random cases against the loops --------------------------------------------------------------------------------
def _random_case(direction, seed, k=200, label_pool=None):
    rng = np.random.default_rng(seed)
    n_test, n_model = (15, 40) if direction == D1 else (40, 15)
    labels = rng.choice(label_pool, k) if label_pool is not None else rng.integers(0, n_test, k)
    data = rng.standard_normal((k, 4, 3)).astype(np.float32)
    w = rng.standard_normal((12, n_model)).astype(np.float32)
    return data, labels.astype(np.int32), w


def _stub_predict(w):
    """scores as a fixed function of the cloud alone"""
    def predict_batch(clouds):
        x = np.asarray(clouds, dtype=np.float32).reshape(len(clouds), -1)
        return list(np.tanh(x) @ w)
    return predict_batch


def _product(direction, predict_batch, data, labels, batch_size):
    cur, lab = CD.select_mapped(data, labels, direction)
    n = (len(lab) // batch_size) * batch_size
    if n == 0:
        raise SystemExit("too few")
    scores = np.array([r for lo in range(0, n, batch_size) for r in predict_batch(cur[lo:lo + batch_size])])
    return SUMMARY[direction](scores, lab[:n]), lab[:n]


@pytest.mark.parametrize("direction", [D1, D2])
@pytest.mark.parametrize("batch_size", [1, 4, 7, 32])
def test_random_cases_equal_the_loops(direction, batch_size):
    data, labels, w = _random_case(direction, seed=batch_size)
    ev, lab = _product(direction, _stub_predict(w), data, labels, batch_size)
    ref, ref_lab = R.run(direction, _stub_predict(w), list(data), list(labels), batch_size)
    assert lab.tolist() == ref_lab and 0 < len(lab) < 200 and len(lab) % batch_size == 0
    if batch_size in (7, 32):
        kept = int(np.isin(labels, list(R.O2M if direction == D1 else R.M2O)).sum())
        assert kept % batch_size != 0 and len(lab) == kept - kept % batch_size         # a partial batch was dropped
    _same(ev, ref)
    assert len(ev["lines"]) == len(lab) and ev["confusion"].sum() == len(lab)
    assert (ev["per_class"] == -1).sum() == 15 - len(set(lab.tolist() if direction == D1 else [R.M2O[l] for l in lab.tolist()]))


@pytest.mark.parametrize("direction", [D1, D2])
def test_argmax_tie_takes_the_first_index(direction):
    n_model = 40 if direction == D1 else 15
    # chair / chair, bench / table: the tie between a right and a wrong class is decided by the index order
    lab = np.array([4, 4, 4]) if direction == D1 else np.array([8, 8, 8])
    right, wrong_lo, wrong_hi = (8, 0, 39) if direction == D1 else (4, 0, 14)
    scores = np.zeros((3, n_model), dtype=np.float32)
    scores[0, [wrong_lo, right]] = 2.0            # the wrong class comes first
    scores[1, [right, wrong_hi]] = 2.0            # the right class comes first
    scores[2, :] = 1.0                            # all equal: index 0
    ev = SUMMARY[direction](scores, lab)
    assert ev["pred"].tolist() == [wrong_lo, right, 0] and ev["total_correct"] == 1
    _same(ev, (R.real_on_synthetic if direction == D1 else R.synthetic_on_real)(scores, lab))


@pytest.mark.parametrize("direction", [D1, D2])
def test_a_mapped_class_that_never_occurs(direction):
    pool = [3, 4, 0, 11] if direction == D1 else [8, 32, 0, 38]          # two mapped slots only (cabinet, chair)
    data, labels, w = _random_case(direction, seed=5, label_pool=pool)
    ev, lab = _product(direction, _stub_predict(w), data, labels, 4)
    ref, _ = R.run(direction, _stub_predict(w), list(data), list(labels), 4)
    _same(ev, ref)
    assert [i for i in range(15) if ev["per_class"][i] != -1] == [3, 4]
    assert ev["avg_class_acc"] == float(np.mean(ev["per_class"][[3, 4]]))


@pytest.mark.parametrize("direction", [D1, D2])
def test_no_mapped_cloud_raises_system_exit(direction):
    pool = [0, 1, 2, 11] if direction == D1 else [0, 1, 5, 39]
    data, labels, w = _random_case(direction, seed=6, k=20, label_pool=pool)
    cur, lab = CD.select_mapped(data, labels, direction)
    assert cur.shape == (0, 4, 3) and lab.shape == (0,)
    with pytest.raises(SystemExit, match="fewer than one batch"):
        CD.vote_scores(lambda x, is_training: x.sum(dim=1), cur, 1, device="cpu")
    with pytest.raises(SystemExit):
        SUMMARY[direction](np.zeros((0, 40 if direction == D1 else 15), dtype=np.float32), lab)
    with pytest.raises(SystemExit):
        R.run(direction, _stub_predict(w), list(data), list(labels), 1)
    # some clouds survive, but fewer than one batch
    data, labels, w = _random_case(direction, seed=7, k=20, label_pool=pool + [4 if direction == D1 else 8])
    cur, lab = CD.select_mapped(data, labels, direction)
    assert 0 < len(lab) < 16
    with pytest.raises(SystemExit, match="fewer than one batch of 16"):
        CD.vote_scores(lambda x, is_training: x.sum(dim=1), cur, 16, device="cpu")


# ---- vote_scores with a stub net -----------------------------------------------------------------------------------
class _Stub:
    """a fixed function of its input; records every call"""

    def __init__(self, as_tuple):
        self.calls, self.as_tuple = [], as_tuple
        self.w = torch.linspace(-1.0, 1.0, 3 * 5, dtype=torch.float32).reshape(3, 5)

    def __call__(self, x, is_training):
        assert is_training is False and x.is_contiguous() and x.dtype == torch.float32
        self.calls.append(x.clone())
        out = torch.tanh(x @ self.w + x[..., :1])              # (B,N,5): not rotation invariant
        return (out, {"end": 1}) if self.as_tuple else out


@pytest.mark.parametrize("with_scores_fn", [False, True])
def test_vote_scores_with_a_stub_net(with_scores_fn):
    from scanobjectnn_amd import provider
    data = np.random.default_rng(3).standard_normal((11, 6, 3)).astype(np.float32)
    net = _Stub(as_tuple=not with_scores_fn)
    # without a hook the net returns (B,C) logits and end points; with one, bare per-point values that the hook reduces
    if with_scores_fn:
        scores_fn = lambda o: torch.softmax(o, dim=-1).sum(dim=1)          # noqa: E731
        inner = net
    else:
        scores_fn = None
        inner = lambda x, is_training: (net(x, is_training)[0].sum(dim=1), {"end": 1})     # noqa: E731
    got = CD.vote_scores(inner, data, 4, num_votes=3, device="cpu", scores_fn=scores_fn)
    assert got.shape == (8, 5) and got.dtype == np.float32                     # 11 // 4 whole batches
    assert len(net.calls) == 2 * 3
    want = []
    for b in range(2):
        pts = torch.from_numpy(data[4 * b:4 * b + 4])
        total = None
        for v in range(3):
            rot = provider.rotate_point_cloud_by_angle(pts, v / 3.0 * 2 * math.pi)
            assert torch.equal(net.calls[3 * b + v], rot)                      # the angles: vote / num_votes * 2 pi
            o = torch.tanh(rot @ net.w + rot[..., :1])
            o = torch.softmax(o, dim=-1).sum(dim=1) if with_scores_fn else o.sum(dim=1)
            total = o if total is None else total + o
        want.append(total.numpy())
    assert np.array_equal(got, np.concatenate(want))
    assert not np.array_equal(got, 3 * CD.vote_scores(inner, data, 4, num_votes=1, device="cpu", scores_fn=scores_fn))
    one = CD.vote_scores(inner, data, 11, num_votes=1, device="cpu", scores_fn=scores_fn)
    assert one.shape == (11, 5)


# ---- command lines -------------------------------------------------------------------------------------------------
def test_command_line_defaults():
    from scanobjectnn_amd.pointnet2 import evaluate_real_trained_on_synthetic as E1, evaluate_synthetic_trained_on_real as E2
    a = E1.parse_args([])
    assert (a.gpu, a.model, a.batch_size, a.num_point, a.model_path, a.dump_dir, a.num_class, a.test_file, a.normal,
            a.num_votes, a.visu, a.with_bg, a.norm, a.center_data) == \
        (0, "pointnet2_cls_ssg", 1, 1024, "log/model.ckpt", "dump_real_trained_on_synthetic/", 40, "", False, 1, False,
         True, True, True)
    b = E2.parse_args([])
    assert (b.model, b.batch_size, b.num_point, b.dump_dir, b.num_class, b.num_votes) == \
        ("pointnet2_cls_ssg", 1, 1024, "dump_synthetic_trained_on_real/", 15, 1)
    c = E1.parse_args(["--model", "3dmfv_net_cls", "--num_gaussians", "3", "--gmm_variance", "0.1", "--num_votes", "12",
                       "--visu", "true", "--normal", "--batch_size", "8", "--norm", "no"])
    assert (c.num_gaussians, c.gmm_variance, c.num_votes, c.visu, c.normal, c.batch_size, c.norm, c.num_class) == \
        (3, 0.1, 12, True, True, 8, False, 40)
    # PointCNN: the reference's own default setting per direction, and the class count from the setting
    p1, p2 = E1.parse_args(["--model", "pointcnn_cls"]), E2.parse_args(["--model", "pointcnn_cls"])
    assert (p1.setting, p1.num_class, p2.setting, p2.num_class) == ("modelnet40_expt", 40, "modelnet_x3_l4", 15)
    assert E1.parse_args(["--model", "pointcnn_cls", "--setting", "modelnet_x3_l4"]).num_class == 15
    assert E1.parse_args(["--model", "pointcnn_cls", "--setting", "modelnet_x3_l4", "--num_class", "40"]).num_class == 40
    assert E1.parse_args(["--model", "dgcnn"]).setting == "modelnet_x3_l4"             # read by no other model


def test_setting_modelnet40_expt_and_the_fall_back():
    from scanobjectnn_amd.pointcnn import pointcnn_cls, settings as S
    from scanobjectnn_amd.pointnet2 import draw_cmat, evaluate_scenennobjects as EV, evaluate_seg_scenennobjects as EVS, train
    s40, s15 = S.get("modelnet40_expt"), S.get("modelnet_x3_l4")
    assert s40.num_class == 40 and s15.num_class == 15 and s40 is not s15
    assert {k: v for k, v in vars(s40).items() if k != "num_class"} == {k: v for k, v in vars(s15).items() if k != "num_class"}
    for parse in (train.parse_args, EV.parse_args, draw_cmat.parse_args):
        a = parse(["--model", "pointcnn_cls", "--setting", "modelnet40_expt"])
        assert (a.setting, a.num_class) == ("modelnet40_expt", 40)
        assert pointcnn_cls.setting_of(a) is s40
        assert parse(["--model", "pointcnn_cls", "--setting", "modelnet40_expt", "--num_class", "15"]).num_class == 15
        # as before: the model's own setting, 15 classes, and an explicit --num_class for every model
        assert (parse(["--model", "pointcnn_cls"]).setting, parse(["--model", "pointcnn_cls"]).num_class) == ("modelnet_x3_l4", 15)
        assert parse([]).num_class == 15 and parse(["--model", "dgcnn", "--num_class", "40"]).num_class == 40
        assert parse(["--model", "dgcnn", "--setting", "modelnet40_expt"]).num_class == 15      # read by pointcnn_cls only
    a = train.parse_args(["--model", "pointcnn_cls", "--setting", "modelnet40_expt"])
    assert (a.learning_rate, a.decay_step, a.decay_rate, a.batch_size, a.max_epoch) == (0.01, 8000, 0.5, 32, 400)
    assert train.parse_args(["--model", "pointcnn_seg"]).setting == "object_dataset_x3"
    assert train.parse_args(["--model", "pointcnn_seg"]).num_class == 15
    assert EVS.parse_args(["--model", "pointcnn_seg"]).setting == "object_dataset_x3"
    assert draw_cmat.parse_args([]).dump_dir == "confusion_matrix/" and draw_cmat.parse_args(["--dump_dir", "x"]).dump_dir == "x"


def test_mask_and_part_models_are_refused(monkeypatch):
    from scanobjectnn_amd.pointnet2 import evaluate_real_trained_on_synthetic as E1, evaluate_synthetic_trained_on_real as E2
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    for E in (E1, E2):
        for model in ("pointnet2_cls_bga", "pointcnn_seg", "pointnet_seg", "pointnet_partseg"):
            with pytest.raises(SystemExit, match="evaluate_seg_scenennobjects"):
                E.evaluate(E.parse_args(["--model", model]))
    with pytest.raises(SystemExit, match="no class map"):
        E1.evaluate(E1.parse_args(["--num_class", "15"]))


def test_draw_cmat_matrix_pieces():
    from scanobjectnn_amd.pointnet2 import draw_cmat
    counts = draw_cmat.confusion_counts([0, 1, 1, 14, 0], [0, 0, 1, 14, 0])
    assert counts.shape == (15, 15) and counts[0, 0] == 2 and counts[0, 1] == 1 and counts.sum() == 5
    m = draw_cmat.row_normalised(counts)
    assert m[0, 0] == 2 / 3.0 and m[0, 1] == 1 / 3.0 and m[1, 1] == 1.0 and m[14, 14] == 1.0
    assert not m[2:14].any() and np.isfinite(m).all()                 # classes that never occur: rows of zeros


# ---- one wrong restatement per rule --------------------------------------------------------------------------------
def test_the_comparison_rejects_one_wrong_restatement_per_rule():
    # (1) the filter applied after batching: other clouds make it into the whole batches
    data, labels, w = _random_case(D1, seed=11)
    ev, lab = _product(D1, _stub_predict(w), data, labels, 32)
    ref, ref_lab = R.run(D1, _stub_predict(w), list(data), list(labels), 32, filter_after_batching=True)
    assert lab.tolist() != ref_lab and _differs(ev, ref)
    # (2) unmapped predictions skipped instead of counted wrong
    scores = np.tanh(data.reshape(200, -1)) @ w
    assert not np.isin(scores.argmax(1), list(R.M2O)).all()
    cur, lab = CD.select_mapped(scores, labels, D1)
    ev = CD.summarize_real_on_synthetic(cur, lab)
    _same(ev, R.real_on_synthetic(cur, lab))
    assert _differs(ev, R.real_on_synthetic(cur, lab, skip_unmapped=True))
    # (3) the average over 15 instead of over the seen classes (eleven at the most are ever seen)
    wrong = R.real_on_synthetic(cur, lab, average_over_all=True)
    assert ev["avg_class_acc"] != wrong["avg_class_acc"] and ev["accuracy"] == wrong["accuracy"]
    # (4) direction 2: per-class counters indexed by the raw ModelNet label
    data, labels, w = _random_case(D2, seed=12)
    scores = np.tanh(data.reshape(200, -1)) @ w
    cur, lab = CD.select_mapped(scores, labels, D2)
    ev = CD.summarize_synthetic_on_real(cur, lab)
    _same(ev, R.synthetic_on_real(cur, lab))
    wrong = R.synthetic_on_real(cur, lab, index_by_raw_label=True)
    assert list(ev["per_class"]) != wrong["per_class"] and ev["accuracy"] == wrong["accuracy"]
