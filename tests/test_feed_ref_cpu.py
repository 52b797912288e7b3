"""The device-resident feed without a GPU: the restatement of tests/feed_ref.py against known answers and statistics, the
error bar of tests/feed_checks.py against an fp32 evaluation and against one wrong restatement per edge, the launcher's
argument checks, and the two refusal functions."""
import argparse
import ctypes
import os

import numpy as np
import pytest

import feed_checks as FC
import feed_ref as R


# ------------------------------------------------------------------------------------------------------------ the generator
@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox_known_answers(counter, key, want):
    assert " ".join("%08x" % w for w in R.philox(*counter, key)) == want


def test_philox_broadcasts_and_the_key_is_the_seed_split():
    one = [R.philox(7, 3, j, R.TAG_JIT, R.key_of(FC.SEED)) for j in range(5)]
    assert np.array_equal(R.philox(7, 3, np.arange(5), R.TAG_JIT, R.key_of(FC.SEED)), np.stack(one))
    assert R.key_of(FC.SEED) == (0x90ABCDEF, 0x12345678)
    assert len({R.TAG_CLOUD, R.TAG_JIT, R.TAG_PERM}) == 3


def test_header_fixes_the_tags():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pcops.h")).read()
    for name, tag in (("CLOUD", R.TAG_CLOUD), ("JIT", R.TAG_JIT), ("PERM", R.TAG_PERM)):
        assert "#define PCOPS_FEED_TAG_%s" % name in text and ("0x%08xu" % tag) in text


def test_uniform_is_exact_in_fp32_and_open():
    w = np.array([0, 0x1ff, 0x200, 0x80000000, 0xffffffff], dtype=np.uint32)
    u = R.uniform(w)
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
    assert u.min() == 2.0 ** -24 and u.max() == 1.0 - 2.0 ** -24


def test_normals_mean_and_variance():
    """10^6 restated normals: mean within 4 sigma / sqrt(N), variance within 4 sqrt(2 / N)"""
    n = 333334
    z = R.normals(R.philox(5, 9, np.arange(n), R.TAG_JIT, R.key_of(FC.SEED))).reshape(-1)
    assert z.size >= 10 ** 6
    assert abs(z.mean()) <= 4.0 / np.sqrt(z.size)
    assert abs(z.var() - 1.0) <= 4.0 * np.sqrt(2.0 / z.size)
    for k in range(3):                                                    # each of the three outputs on its own as well
        assert abs(z[k::3].mean()) <= 4.0 / np.sqrt(n) and abs(z[k::3].var() - 1.0) <= 4.0 * np.sqrt(2.0 / n)


# ---------------------------------------------------------------------------------------------------------- the permutation
@pytest.mark.parametrize("ni", [1, 2, 3, 64, 65, 1024, 1025, 2049, 70001])
def test_permutation_is_a_bijection(ni):
    for cloud, epoch in ((0, 0), (3, 7)):
        p = R.perm(ni, R.perm_keys(1234, cloud, epoch))
        assert p.min() == 0 and p.max() == ni - 1 and np.unique(p).size == ni
        assert np.array_equal(R.perm(ni, R.perm_keys(1234, cloud, epoch), min(ni, 33)), p[:33])     # a prefix is a prefix


def test_permutation_known_answer_and_what_moves_it():
    keys = R.perm_keys(1234, 5, 7)
    p = R.perm(1500, keys, 8)
    assert p.tolist() == PERM_1500_FIRST8, p.tolist()
    assert not np.array_equal(R.perm(1500, R.perm_keys(1234, 5, 8), 8), p)        # the epoch
    assert not np.array_equal(R.perm(1500, R.perm_keys(1234, 6, 7), 8), p)        # the cloud
    assert not np.array_equal(R.perm(1500, R.perm_keys(1235, 5, 7), 8), p)        # the seed
    wrong = R.perm(1500, keys, wrong="swapped_half")
    assert np.unique(wrong).size == 1500 and not np.array_equal(wrong[:8], p)      # still a bijection, not this one


PERM_1500_FIRST8 = [1328, 1322, 315, 1057, 1079, 1295, 1120, 151]      # recorded from the restatement: pins it against drift


@pytest.mark.parametrize("ni", [1025, 1500, 3000, 20000])
def test_inclusion_counts_are_those_of_a_shuffle(ni):
    """seed 1234, epoch 7, clouds 0..2999: how often each source point is among the first 1024 and the first 64 outputs.
    Measured with this file's tags: z between -1.79 and +1.97 in seven of the eight cases and +3.54 for the first 64 of
    20 000 points; the same statistic at other epochs between -0.81 and +2.96 (sixteen cases), for NumPy's shuffle between
    -1.56 and +1.41 (six cases)."""
    clouds = 3000
    c1024, c64 = np.zeros(ni), np.zeros(ni)
    for c in range(clouds):
        p = R.perm(ni, R.perm_keys(1234, c, 7), 1024)
        assert np.unique(p).size == 1024
        c1024[p] += 1
        c64[p[:64]] += 1
    for take, counts in ((1024, c1024), (64, c64)):
        z = FC.inclusion_z(counts, clouds, take, ni)
        print("n_i = %d, first %d: z = %+.2f" % (ni, take, z))
        assert abs(z) <= 4.0


# ------------------------------------------------------------------------------------------------------ recipes and the bar
def test_bar_is_the_sum_of_its_terms():
    assert FC.bar(0) == 0.0
    assert 1.5e-6 < FC.bar(1) < 2.0e-6 and 5e-7 < FC.bar(2) < 8e-7
    assert FC.bar(1, sigma=0.1) > FC.bar(1)


@pytest.mark.parametrize("recipe", [1, 2])
@pytest.mark.parametrize("case", FC.RECIPE_CASES, ids=lambda c: "%s-n%d-first%d" % c[:3])
def test_fp32_evaluation_lands_below_the_bar(case, recipe):
    S, order, mode, idx, want = FC.recipe_case(*case, recipe=recipe)
    got = FC.recipe_case(*case, recipe=recipe, dtype=np.float32)[4]
    assert got[0].dtype == np.float32
    err, ok = FC.bar_excess(got, want, FC.bar(recipe))
    print("recipe %d %s: fp32 against float64 %.3g, bar %.3g" % (recipe, case, err, FC.bar(recipe)))
    assert ok, (err, FC.bar(recipe))
    assert np.abs(want[0]).max() <= (1.0 if recipe == 1 else 1.5 + 0.2) + 0.05      # the magnitudes the bar assumes


@pytest.mark.parametrize("recipe, wrong", [(r, w) for r in (1, 2) for w in FC.WRONG[r]])
def test_a_wrong_restatement_lands_above_the_bar(recipe, wrong):
    for case in FC.RECIPE_CASES:
        if wrong == "local_row" and case[2] == 0:
            continue                                   # row and global position coincide at first = 0
        want = FC.recipe_case(*case, recipe=recipe)[4]
        got = FC.recipe_case(*case, recipe=recipe, wrong=wrong)[4]
        err, ok = FC.bar_excess(got, want, FC.bar(recipe))
        assert not ok and err > 100 * FC.bar(recipe), (case, err)


def test_a_swapped_feistel_half_fails_the_exact_check():
    for n in FC.RAGGED_N:
        S, order = FC.ragged_set(n), FC.order_of(6)
        want = R.feed_batch(S, order, 0, 6, n, 1, None, 0, 2, FC.SEED, 0, False)
        assert FC.exact_mismatch(R.feed_batch(S, order, 0, 6, n, 1, None, 0, 2, FC.SEED, 0, False), want) is None
        got = R.feed_batch(S, order, 0, 6, n, 1, None, 0, 2, FC.SEED, 0, False, wrong="swapped_half")
        assert FC.exact_mismatch(got, want) is not None


def test_restated_batch_row_guard_and_split():
    """rows past the end are zeros with label -1; B = 6 is three launches of B = 2; step moves the augmentation only, the
    epoch moves the selection"""
    n, S, order = 33, FC.ragged_set(33), FC.order_of(6)
    x, y, m = R.feed_batch(S, order, 4, 3, n, 1, None, 1, 2, FC.SEED, 1, False)
    assert y[2] == -1 and not x[2].any() and not m[2].any() and y[0] == S["labels"][order[4]]
    whole = R.feed_batch(S, order, 0, 6, n, 1, None, 1, 2, FC.SEED, 1, False)
    parts = [R.feed_batch(S, order, f, 2, n, 1, None, 1, 2, FC.SEED, 1, False) for f in (0, 2, 4)]
    assert FC.exact_mismatch(tuple(np.concatenate(p) for p in zip(*parts)), whole) is None
    other_step = R.feed_batch(S, order, 0, 6, n, 1, None, 2, 2, FC.SEED, 1, False)
    assert np.array_equal(other_step[2], whole[2]) and not np.array_equal(other_step[0], whole[0])
    other_epoch = R.feed_batch(S, order, 0, 6, n, 1, None, 1, 3, FC.SEED, 1, False)
    assert not np.array_equal(other_epoch[2], whole[2])


# ------------------------------------------------------------------------------------------- the launcher's argument checks
def test_launcher_argument_checks_without_gpu():
    from scanobjectnn_amd import _lib
    lib = _lib.load()
    F, LL, U64 = ctypes.c_float, ctypes.c_longlong, ctypes.c_ulonglong
    I, P = ctypes.c_int, ctypes.c_void_p
    assert _lib.SIGNATURES["pcops_feed_batch"] == ([I, LL, I, I, I, I, LL] + [P] * 7 + [U64] + [F] * 5 + [P] * 3, True)
    assert _lib.SIGNATURES["pcops_feed_set_params"] == ([I, I, I, P], True)

    def batch(K=5, ntot=70, B=3, n=33, mode=0, recipe=0, min_points=70, ptrs=(None,) * 10, clip=0.05, smin=0.66, smax=1.5):
        pts, offsets, labels, side, order, idx, params, x, y, m = ptrs
        return lib.pcops_feed_batch(K, LL(ntot), B, n, mode, recipe, LL(min_points), pts, offsets, labels, side, order, idx,
                                    params, U64(1), F(0.01), F(clip), F(smin), F(smax), F(0.2), x, y, m, None)
    assert batch() == -1                                   # null pointers
    assert batch(B=0) == 0                                 # a no-op before any pointer is looked at
    assert batch(n=71) == -2 and batch(n=130) == -2        # n > min_points
    assert batch(min_points=71) == -2                      # a dense set has no cloud larger than ntot
    assert batch(K=0) == -2 and batch(n=0) == -2 and batch(B=-1) == -2 and batch(ntot=0) == -2
    assert batch(mode=2) == -3 and batch(recipe=3) == -3 and batch(recipe=1, clip=0.0) == -3
    assert batch(recipe=2, smin=2.0) == -3
    assert batch(B=65536) == -4
    fake = ctypes.c_void_p(64)                             # never dereferenced: every call below ends at a check
    assert batch(ptrs=(fake, fake) + (None,) * 8) == -3    # mode 0 on a ragged set
    assert batch(mode=1, ptrs=(fake,) + (None,) * 9) == -1
    assert lib.pcops_feed_set_params(0, 0, 0, None, None) == -1


# ------------------------------------------------------------------------------------------------------------ the refusals
def _args(**kw):
    base = dict(model="pointnet2_cls_ssg", no_augment=False, train_file="", device_feed=True, sync_bn=False)
    return argparse.Namespace(**dict(base, **kw))


class _Own:
    def augment(self, batch, generator=None):
        return batch


class _Mod:
    pass


def test_device_feed_refusal_every_reason():
    from scanobjectnn_amd import device_feed as DF
    from scanobjectnn_amd.mfv3d import mfv3d_net_cls
    assert DF.refusal(_args(), _Mod, None, "cuda") is None
    assert DF.refusal(_args(model="3dmfv_net_cls"), mfv3d_net_cls, None, "cuda") is None
    assert DF.recipe_of(_args(), _Mod)[0] == 1 and DF.recipe_of(_args(no_augment=True), _Mod)[0] == 0
    rec = DF.recipe_of(_args(model="3dmfv_net_cls"), mfv3d_net_cls)
    assert rec[0] == 2 and rec[1] == {"sigma": 0.01, "clip": 0.05, "smin": 0.66, "smax": 1.5, "tval": 0.2}
    why = DF.refusal(_args(), _Mod, None, "cpu")
    assert why and "\n" not in why and "cpu" in why.lower()
    why = DF.refusal(_args(model="pointcnn_cls"), _Mod, _Own(), "cuda")
    assert why and "\n" not in why and "augmentation of its own" in why

    class Unknown:                                     # a module-level augment that names no recipe
        @staticmethod
        def augment(batch, generator=None):
            return batch
    why = DF.refusal(_args(), Unknown, None, "cuda")
    assert why and "\n" not in why and "recipe" in why
    assert DF.refusal(_args(no_augment=True), Unknown, None, "cuda") is None      # nothing to restate without augmentation


def test_bin_refusal_of_the_captured_step_is_lifted_by_the_flag_only():
    from scanobjectnn_amd import captured_step as CS
    a = _args(train_file="split/train_files.pkl", device_feed=False)
    why = CS.refusal(a, 1, {})
    assert why == "split/train_files.pkl: a list of raw .bin objects is a ragged set sampled on the host every epoch"
    del a.device_feed                                  # a namespace from before the flag existed
    assert CS.refusal(a, 1, {}) == why
    assert CS.refusal(_args(train_file="split/train_files.pkl"), 1, {}) is None
    # everything else is as it was, with the flag and without
    for flag in (True, False):
        assert CS.refusal(_args(device_feed=flag), 2, {}) is not None
        assert "PCOPS_SYNC" in CS.refusal(_args(device_feed=flag), 1, {"PCOPS_SYNC": "1"})
        assert "--sync_bn" in CS.refusal(_args(device_feed=flag, sync_bn=True), 1, {})
        assert "not on the list" in CS.refusal(_args(device_feed=flag, model="spidercnn_cls_xyz"), 1, {})
        assert CS.refusal(_args(device_feed=flag, train_file="a.npz"), 1, {}) is None


def test_device_feed_host_side_on_the_cpu():
    """what DeviceFeed decides on the host, no device involved: the concatenation of a ragged list and its offsets, and the
    epoch draws -- the dense draw is data_utils.epoch_indices on the trainer's stream, call for call"""
    from scanobjectnn_amd import data_utils, device_feed as DF
    clouds, labels, _ = FC.ball_clouds([40, 33, 90], 3)
    pts, offsets, lab = DF.concat_ragged(clouds, labels)
    assert pts.shape == (163, 3) and pts.dtype == np.float32 and offsets.tolist() == [0, 40, 73, 163]
    assert np.array_equal(pts[40:73], clouds[1]) and lab.dtype == np.int64 and lab.tolist() == list(labels)
    a, b = np.random.RandomState(4), np.random.RandomState(4)
    idx_pts, order = DF.epoch_draw(b, 7, 70, 33, dense=True)
    want_pts, want_order = data_utils.epoch_indices(7, 70, 33, a)
    assert np.array_equal(idx_pts, want_pts) and np.array_equal(order, want_order)
    assert a.randint(1 << 30) == b.randint(1 << 30)                # the stream is where the host path leaves it
    idx_pts, order = DF.epoch_draw(b, 7, 0, 33, dense=False)
    assert idx_pts is None and sorted(order.tolist()) == list(range(7))
