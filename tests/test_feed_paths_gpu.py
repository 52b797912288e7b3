"""pcops_feed_batch on the GPU, path by path, against the restatement of tests/feed_ref.py: every case is launched twice
into guard-banded outputs -- the two results equal bit for bit, the bands untouched -- and compared exactly (selection,
labels, side values, recipe 0) or within the derived bar of tests/feed_checks.py (recipes 1 and 2).

Measured on the MI355X (each recipe case prints its figure): largest |kernel - float64| 1.11e-7 for recipe 1 (bar 1.72e-6)
and 1.27e-7 for recipe 2 (bar 5.77e-7)."""
import numpy as np
import pytest
import torch

import feed_checks as FC
import feed_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
X_FILL, Y_FILL, M_FILL = -777.0, -555, -333


class Launch:
    """one set on the device and the launches into guard-banded outputs"""

    def __init__(self, S, dense):
        self.S, self.dense = S, dense
        t = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=DEV)   # noqa: E731
        self.pts, self.labels, self.side = t(S["pts"], torch.float32), t(S["labels"], torch.int64), t(S["side"], torch.int64)
        self.offsets = None if dense else t(S["offsets"], torch.int64)
        self.params = torch.zeros(4, dtype=torch.int32, device=DEV)

    def status(self, order, first, B, n, mode, idx, step, epoch, recipe, with_side=True, min_points=None, nulls=(), **kw):
        """(status, x, y, m as NumPy, or None where the launch was given none) of one launch; `nulls`: argument names
        passed as NULL"""
        from scanobjectnn_amd import _lib
        lib = _lib.load()
        c = {k: float(np.float32(v)) for k, v in dict(R.RECIPE_CONSTS, **kw).items()}
        x = torch.full((GUARD + B * n * 3 + GUARD,), X_FILL, dtype=torch.float32, device=DEV)
        y = torch.full((GUARD + B + GUARD,), Y_FILL, dtype=torch.int64, device=DEV)
        m = torch.full((GUARD + B * n + GUARD,), M_FILL, dtype=torch.int64, device=DEV)
        o = torch.as_tensor(np.asarray(order), dtype=torch.int32, device=DEV)
        ip = None if idx is None else torch.as_tensor(np.asarray(idx), dtype=torch.int32, device=DEV)
        _lib.call("pcops_feed_set_params", first, step, epoch, self.params.data_ptr())
        side = self.side if with_side else None
        ptrs = {"pts": self.pts.data_ptr(), "offsets": _lib.ptr(self.offsets), "labels": self.labels.data_ptr(),
                "side": _lib.ptr(side), "order": o.data_ptr(), "idx_pts": _lib.ptr(ip), "params": self.params.data_ptr(),
                "x": x[GUARD:].data_ptr(), "y": y[GUARD:].data_ptr(), "m": m[GUARD:].data_ptr()}
        for name in nulls:
            ptrs[name] = None
        stream = torch.cuda.current_stream().cuda_stream
        st = lib.pcops_feed_batch(self.S["K"], self.S["ntot"] if self.dense else 0, B, n, mode, recipe,
                                  self.S["min_points"] if min_points is None else min_points, ptrs["pts"], ptrs["offsets"],
                                  ptrs["labels"], ptrs["side"], ptrs["order"], ptrs["idx_pts"], ptrs["params"], FC.SEED,
                                  c["sigma"], c["clip"], c["smin"], c["smax"], c["tval"], ptrs["x"], ptrs["y"], ptrs["m"], stream)
        torch.cuda.synchronize()
        xs, ys, ms = x.cpu().numpy(), y.cpu().numpy(), m.cpu().numpy()
        for buf, fill in ((xs, X_FILL), (ys, Y_FILL), (ms, M_FILL)):
            assert (buf[:GUARD] == fill).all() and (buf[buf.size - GUARD:] == fill).all(), "a guard band was written"
        return st, xs[GUARD:-GUARD].reshape(B, n, 3), ys[GUARD:-GUARD], ms[GUARD:-GUARD].reshape(B, n)

    def twice(self, *a, **kw):
        """the launch's (x, y, m) after two launches that agree bit for bit; m is None without side values"""
        st1, x1, y1, m1 = self.status(*a, **kw)
        st2, x2, y2, m2 = self.status(*a, **kw)
        assert st1 == 0 and st2 == 0
        assert np.array_equal(x1.view(np.uint32), x2.view(np.uint32)) and np.array_equal(y1, y2) and np.array_equal(m1, m2)
        if kw.get("with_side", True) and self.S["side"] is not None:
            return x1, y1, m1
        assert (m1 == M_FILL).all()                      # no side values: m is not touched
        return x1, y1, None


_SETS = {}


def launch_of(kind, *key):
    """sets are built and uploaded once and shared"""
    if (kind,) + key not in _SETS:
        S = FC.dense_set(*key) if kind == "dense" else FC.ragged_set(*key)
        _SETS[(kind,) + key] = Launch(S, kind == "dense")
    return _SETS[(kind,) + key]


# ------------------------------------------------------------------------------------------------ selection, bit for bit
@pytest.mark.parametrize("N, n, first", FC.DENSE_CASES)
def test_dense_shared_list_is_index_select(N, n, first):
    L = launch_of("dense", 5, N)
    idx, order = FC.shared_indices(N, n), FC.order_of(5)
    got = L.twice(order, first, 3, n, 0, idx, 0, 0, 0)
    data = L.pts.view(5, N, 3)
    ip, ic = torch.as_tensor(idx, device=DEV).long(), torch.as_tensor(order, device=DEV).long()
    cur = data.index_select(1, ip).index_select(0, ic)                      # train.epoch_view's gather
    msk = L.side.view(5, N).index_select(1, ip).index_select(0, ic)
    lab = L.labels.index_select(0, ic)
    rows = min(3, 5 - first)
    assert np.array_equal(got[0][:rows].view(np.uint32), cur[first:first + rows].cpu().numpy().view(np.uint32))
    assert np.array_equal(got[1][:rows], lab[first:first + rows].cpu().numpy())
    assert np.array_equal(got[2][:rows], msk[first:first + rows].cpu().numpy())
    assert FC.exact_mismatch(got, R.feed_batch(L.S, order, first, 3, n, 0, idx, 0, 0, FC.SEED, 0, True)) is None
    assert rows == 3 or ((got[1][rows:] == -1).all() and not got[0][rows:].any() and not got[2][rows:].any())


def test_dense_n_beyond_the_cloud_is_refused():
    """n = 130 on clouds of 70 points: PCOPS_ERR_BAD_SHAPE, nothing written"""
    L = launch_of("dense", 5, 70)
    st, x, y, m = L.status(FC.order_of(5), 0, 3, 130, 0, np.zeros(130, dtype=np.int32), 0, 0, 0)
    assert st == -2 and (x == X_FILL).all() and (y == Y_FILL).all() and (m == M_FILL).all()


@pytest.mark.parametrize("n", FC.RAGGED_N)
@pytest.mark.parametrize("first", [0, 2])
def test_ragged_permutation_gather(n, first):
    """every cloud size of the table in one launch (B = K = 6): n, n + 1, 2 n - 1, 1024, 1025, 70001 points"""
    L = launch_of("ragged", n)
    order = FC.order_of(6)
    got = L.twice(order, first, 6, n, 1, None, 0, 2, 0)
    want = R.feed_batch(L.S, order, first, 6, n, 1, None, 0, 2, FC.SEED, 0, False)
    assert FC.exact_mismatch(got, want) is None
    for r in range(6 - first):                                    # the side values name cloud and point: all distinct
        assert np.unique(got[2][r]).size == n


def test_dense_set_under_the_permutation():
    """mode 1 on a dense set (NULL offsets)"""
    L = launch_of("dense", 5, 140)
    order = FC.order_of(5)
    got = L.twice(order, 1, 3, 130, 1, None, 0, 4, 0)
    assert FC.exact_mismatch(got, R.feed_batch(L.S, order, 1, 3, 130, 1, None, 0, 4, FC.SEED, 0, True)) is None


# ---------------------------------------------------------------------------------------------------------------- recipes
@pytest.mark.parametrize("recipe", [1, 2])
@pytest.mark.parametrize("case", FC.RECIPE_CASES, ids=lambda c: "%s-n%d-first%d" % c[:3])
def test_recipes_within_the_bar(case, recipe):
    kind, n, first, B = case
    S, order, mode, idx, want = FC.recipe_case(*case, recipe=recipe)
    L = launch_of(kind, *((5, S["ntot"]) if kind == "dense" else (n,)))
    got = L.twice(order, first, B, n, mode, idx, 3, 2, recipe)
    err, ok = FC.bar_excess(got, want, FC.bar(recipe))
    print("recipe %d %s: kernel against float64 %.3g, bar %.3g" % (recipe, case, err, FC.bar(recipe)))
    assert ok, (err, FC.bar(recipe))
    plain = L.twice(order, first, B, n, mode, idx, 3, 2, 0)
    assert np.array_equal(plain[2], got[2]) and not np.array_equal(plain[0], got[0])      # same points, moved


def test_batch_of_six_is_three_batches_of_two():
    for kind, recipe in (("ragged", 1), ("ragged", 2), ("dense", 1)):
        L = launch_of(kind, *((5, 140) if kind == "dense" else (33,)))
        K = L.S["K"]
        order, n = FC.order_of(K), 33
        mode, idx = (0, FC.shared_indices(140, n)) if kind == "dense" else (1, None)
        whole = L.twice(order, 0, 6, n, mode, idx, 5, 1, recipe)
        parts = [L.twice(order, f, 2, n, mode, idx, 5, 1, recipe) for f in (0, 2, 4)]
        joined = tuple(np.concatenate(p) for p in zip(*parts))
        assert np.array_equal(joined[0].view(np.uint32), whole[0].view(np.uint32))
        assert np.array_equal(joined[1], whole[1]) and np.array_equal(joined[2], whole[2])
        if K == 5:                                               # the dense set: row 5 is past the end in both
            assert whole[1][5] == -1 and not whole[0][5].any() and not whole[2][5].any()


def test_rows_past_the_end_and_step_and_epoch():
    L = launch_of("ragged", 33)
    order, n = FC.order_of(6), 33
    x, y, m = L.twice(order, 4, 5, n, 1, None, 1, 2, 1)
    assert (y[2:] == -1).all() and not x[2:].any() and not m[2:].any() and (y[:2] >= 0).all() and x[:2].any()
    x, y, m = L.twice(order, 6, 2, n, 1, None, 1, 2, 1)           # the whole launch past the end
    assert (y == -1).all() and not x.any() and not m.any()
    a = L.twice(order, 0, 6, n, 1, None, 1, 2, 1)
    b = L.twice(order, 0, 6, n, 1, None, 2, 2, 1)                 # another step: the same points, other draws
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[1], b[1]) and not np.array_equal(a[0], b[0])
    c = L.twice(order, 0, 6, n, 1, None, 1, 3, 1)                 # another epoch: other points
    assert not np.array_equal(a[2], c[2]) and np.array_equal(a[1], c[1])


def test_statuses_write_nothing():
    L = launch_of("ragged", 33)
    order, n = FC.order_of(6), 33
    untouched = lambda x, y, m: (x == X_FILL).all() and (y == Y_FILL).all() and (m == M_FILL).all()      # noqa: E731
    got = L.twice(order, 0, 3, n, 1, None, 0, 0, 0, with_side=False)          # side == NULL: x and y, m untouched
    want = R.feed_batch(dict(L.S, side=None), order, 0, 3, n, 1, None, 0, 0, FC.SEED, 0, False)
    assert FC.exact_mismatch(got, want) is None
    st, x, y, m = L.status(order, 0, 0, n, 1, None, 0, 0, 0)                  # B == 0 (the views are empty, the bands checked)
    assert st == 0
    st, *out = L.status(order, 0, 3, 34, 1, None, 0, 0, 0)                    # n > min_points (the smallest cloud has 33)
    assert st == -2 and untouched(*out)
    for name in ("pts", "labels", "order", "params", "x", "y"):
        st, *out = L.status(order, 0, 3, n, 1, None, 0, 0, 0, nulls=(name,))
        assert st == -1 and untouched(*out), name
    st, *out = L.status(order, 0, 3, n, 0, None, 0, 0, 0)                     # the shared list on a ragged set
    assert st == -3 and untouched(*out)
    D = launch_of("dense", 5, 70)
    st, *out = D.status(FC.order_of(5), 0, 3, n, 0, None, 0, 0, 0)            # mode 0 without its list
    assert st == -1 and untouched(*out)


def test_set_params_writes_four_ints_only():
    from scanobjectnn_amd import _lib
    buf = torch.full((GUARD + 4 + GUARD,), 99, dtype=torch.int32, device=DEV)
    _lib.call("pcops_feed_set_params", 7, -3, 11, buf[GUARD:].data_ptr())
    assert buf[GUARD:GUARD + 4].tolist() == [7, -3, 11, 0]
    assert (buf[:GUARD] == 99).all().item() and (buf[GUARD + 4:] == 99).all().item()


# ------------------------------------------------------------------------------------------------------- the host wrapper
def test_device_feed_object_dense_and_ragged():
    """DeviceFeed on both kinds of set: a dense unaugmented epoch is train.epoch_view's, batch by batch and bit for bit (the
    same draws from the same stream); a ragged epoch_view is the restated permutation's gather in the drawn order, and it
    leaves the step's parameters as they were"""
    import argparse
    from scanobjectnn_amd import device_feed as DF
    from scanobjectnn_amd.pointnet2 import train as T
    S = FC.dense_set(7, 70)
    data = torch.as_tensor(S["pts"], device=DEV).view(7, 70, 3)
    lab, msk = torch.as_tensor(S["labels"], device=DEV), torch.as_tensor(S["side"], device=DEV).view(7, 70)
    feed = DF.DeviceFeed(data, lab, msk, 33, 2, 5, 0, DF.NO_CONSTS, DEV)
    ra, rb = np.random.RandomState(3), np.random.RandomState(3)
    for epoch in range(2):
        cur, cl, cm = T.epoch_view(data, lab, msk, 33, ra, DEV)
        feed.begin_epoch(rb, epoch)
        for b in range(4):                                       # the fourth batch holds one cloud and one row past the end
            feed.set_batch(2 * b, 10 * epoch + b)
            x, y, m = feed.launch()
            rows = min(2, 7 - 2 * b)
            assert torch.equal(x[:rows], cur[2 * b:2 * b + rows]) and torch.equal(y[:rows], cl[2 * b:2 * b + rows])
            assert torch.equal(m[:rows], cm[2 * b:2 * b + rows])
            assert rows == 2 or (y[1].item() == -1 and not x[1].any().item())
    assert DF.recipe_of(argparse.Namespace(no_augment=True), T)[0] == 0

    clouds, labels, _ = FC.ball_clouds([40, 33, 90, 1500], 3)
    feed = DF.DeviceFeed(clouds, labels, None, 33, 2, 77, 1, dict(DF.NO_CONSTS, **DF.JITTER), DEV)
    rng = np.random.RandomState(9)
    feed.begin_epoch(rng, 4)
    feed.set_batch(2, 6)
    before = feed.params.clone()
    x, y, m = feed.epoch_view()
    assert m is None and torch.equal(feed.params, before) and before.tolist() == [2, 6, 4, 0]
    order = feed.order.cpu().numpy()
    assert sorted(order.tolist()) == [0, 1, 2, 3]
    want = R.feed_batch(R.make_set(clouds, labels), order, 0, 4, 33, 1, None, 0, 4, 77, 0, False)
    assert np.array_equal(x.cpu().numpy(), want[0].astype(np.float32)) and np.array_equal(y.cpu().numpy(), want[1])
    with pytest.raises(ValueError):
        DF.DeviceFeed(clouds, labels, None, 34, 2, 77, 0, DF.NO_CONSTS, DEV)
