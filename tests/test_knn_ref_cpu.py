"""tests/knn_ref.py (the kNN graph in exact arithmetic, and the band of the contract) against the CPU oracle, which restates
the library's fp32 contract: the definition that tests/test_knn_paths_gpu.py holds the kernels to is first held to the
oracle here, on every input family of tests/knn_checks.py at the smallest n its kernels take.

  * O.pairwise_distance lies within band of dist64;
  * O.knn_graph passes check_lists;
  * undecided_share is under its cap (families built from exact ties are exempt: there the oracle decides);
  * check_lists has teeth: a k-th neighbour swapped for the (k + 3)-th on a well-separated cloud, and a repeated index, fail.

Worst |O.pairwise_distance - dist64| / band, measured on the oracle (not on the code under test), at the shapes below
(n = 33 for c = 3, 16, 64, 128; the last column c = 64 at n = 256, the fp16 kernel's smallest cloud):
  family      c = 3     c = 16    c = 64    c = 128   c = 64, n = 256
  gauss       0.28      0.09      0.05      0.02      0.05
  offset      0.17      0.14      0.07      0.05      0.10
  lattice     0         0         0         0         0        (every product and sum exact in fp32)
  few         0.17      0.07      0.05      0.02      0.02
  line        0         0         0         0         0.21     (exact until j^2 |e|^2 outgrows 24 bits)
  line_rev    0         0         0         0         0.21
  huge / subnormal_mix (c = 64, n = 256): 0.05 / 0.05
Undecided shares of the families not built from ties, same shapes: gauss 0.030 at n = 33 (1 / 33: the k-th candidate itself
and nothing else), 0.004 at n = 256; offset 0.035-0.048 at n = 33, 0.008 at n = 256; huge 0.004, subnormal_mix 0.004.
Tie families, for the record (exempt): lattice 0.02-0.23, few 0.24-0.25, line 0.008-0.042.
"""
import numpy as np
import pytest
import torch

import knn_checks as K
import knn_ref as R
from oracle import oracle as O

SHAPES = [(33, 3, 20), (33, 16, 20), (33, 64, 32), (33, 128, 32), (256, 64, 20)]      # n, c, k


def _held(x, k, ties, label):
    adj = O.pairwise_distance(x)
    ratio = R.contract_ratio(x, adj)
    share = R.undecided_share(x, k)
    print("%s contract / band %.3g  undecided share %.4f" % (label, ratio, share))
    assert ratio <= 1.0
    assert R.check_lists(x, O.knn_graph(x, k), k) == x.shape[0] * x.shape[1]
    if not ties:
        assert share <= K.share_cap(x.shape[1])
    return adj


@pytest.mark.parametrize("n,c,k", SHAPES, ids=str)
@pytest.mark.parametrize("family", K.FAMILIES)
def test_oracle_follows_the_definition(family, n, c, k):
    x = K.cloud(family, 2, n, c)
    adj = _held(x, k, family in K.TIES, "%s n=%d c=%d k=%d" % (family, n, c, k))
    if family == "offset":
        assert (adj < 0).any() and (adj == 0).any()                   # the family is what it claims to be
    if family == "lattice":
        assert np.array_equal(adj.astype(np.float64), R.dist64(x).numpy())


@pytest.mark.parametrize("name", K.F16_EDGE_INPUTS)
def test_oracle_follows_the_definition_on_the_fp16_edge_inputs(name):
    _held(K.edge_input(name), 20, False, name)


def test_line_is_the_worst_case_it_claims_to_be():
    """for the last query of the descending line every later candidate is nearer than all before it"""
    x = K.cloud("line", 1, 40, 3)
    d = R.dist64(x)[0, -1]
    assert (d[1:] < d[:-1]).all()
    d = R.dist64(K.cloud("line_rev", 1, 40, 3))[0, 0]
    assert (d[1:-1] > d[:-2]).all()


def test_check_lists_has_teeth():
    n, c, k = 64, 3, 20
    x = K.cloud("gauss", 2, n, c)
    d = R.dist64(x)
    order = d.argsort(dim=2, stable=True)
    good = order[:, :, :k].clone()
    assert R.check_lists(x, good, k) == 2 * n
    # well separated: the k-th and the (k + 3)-th neighbour of the chosen query are more than two bands apart
    gap = (d.gather(2, order[:, :, k + 2:k + 3]) - d.gather(2, order[:, :, k - 1:k])).squeeze(2) - 2 * R.band(x).amax(dim=2)
    q = int(gap[1].argmax())
    assert gap[1, q] > 0
    swapped = good.clone()
    swapped[1, q, k - 1] = order[1, q, k + 2]
    with pytest.raises(AssertionError, match="provably farther"):
        R.check_lists(x, swapped, k)
    repeated = good.clone()
    repeated[0, 5, 7] = repeated[0, 5, 2]
    with pytest.raises(AssertionError, match="repeat"):
        R.check_lists(x, repeated, k)
    outside = good.clone()
    outside[0, 0, 0] = n
    with pytest.raises(AssertionError, match="outside"):
        R.check_lists(x, outside, k)
    outside[0, 0, 0] = -1
    with pytest.raises(AssertionError, match="outside"):
        R.check_lists(x, outside, k)
    with pytest.raises(AssertionError):
        R.check_lists(x, good[:, :-1], k)                             # a query left out


def test_undecided_share_counts_what_it_says():
    x = np.zeros((1, 4, 1), np.float32)
    x[0, :, 0] = [0.0, 1.0, 2.0, 4.0]
    assert R.undecided_share(x, 2) == pytest.approx(5 / 16)           # the k-th of each query; query 1 has a tie at its k-th
    assert R.undecided_share(torch.from_numpy(x), 1) == pytest.approx(4 / 16)
