"""Every kernel of scanobjectnn_amd/csrc/knn.hip, variant by variant, through the C ABI (_lib.call on raw pointers), held to
  * the path the library reports for exactly those arguments (pcops_knn_graph_path: 3|16 fp16 filter, 2|16 fp32 MFMA,
    1 generic, 0 no kernel for the width),
  * the CPU oracle, bit for bit (np.array_equal), and
  * the operation itself: tests/knn_ref.py check_lists -- k distinct indices in range, none provably farther in float64 than
    a point left out.  It is vacuous only for the pairs within two bands of the k-th distance; on every input not built from
    exact ties their share is asserted under knn_checks.share_cap (0.05; 1 / n from n = 20 down, where the k-th candidate
    alone is that much).  Tie families (lattice, few, line) are exempt: there bit-equality with the oracle decides.

Memory contract of every case: every output lives in a tests/edge_checks.Out buffer -- int32 prefilled with -1, float32
with NaN, guard bands on both sides bit-identical afterwards -- so a store out of range, or a row a kernel should have
written and did not (a -1 fails check_lists), shows.  Every case runs twice and must be bit-identical.  b = 2 unless noted:
cloud 1 starts n c floats after cloud 0.  "misaligned": x starts one float past a 16-byte boundary inside a larger buffer.

What each case reaches (the tables are tests/knn_checks.py; families rotate over gauss, offset, lattice, few, line, line_rev).
knn_mfma_kernel<CP, KL> -- path 2|16; 128 queries per workgroup, 128-row candidate chunks, 32-row tiles, two half-waves per
query; CP = 4, 16, 64, 128 for c <= CP, KL = 20 for k <= 20, else 32 (k <= 32)
  every (CP, KL) at one c (3, 16, 63, 128):
    KL = 20  (n, k) = (1, 1) (2, 2) (2, 1) (19, 19) (20, 19) (20, 20) (21, 20), n = 31, 33, 127, 128, 129, 257 at k = 20
    KL = 32  (n, k) = (21, 21) (22, 21) (31, 21) (31, 31) (32, 32) (33, 32), n = 127, 128, 129, 257 at k = 32
             n == k: each half-list holds about k / 2 finite entries and value((KL + 1) / 2 - 1) sits on the boundary
  every c at n = 129, k = 20 and 32: CP = 4: 1, 3, 4; 16: 5, 15, 16; 64: 17, 63, 64; 128: 65, 127, 128
    c == CP aligned: the 16-byte `vec` loads; c == CP misaligned: the scalar loads (one case per CP and KL)
  every k at n = 129: 1, 2, 19, 20 (KL = 20), 21, 22, 31, 32 (KL = 32)
  b = 9, n = 129, c = 3, k = 20 and 32: xcd_cloud_part with more clouds than XCDs
  c = 64, n = 257, k = 20 misaligned: the path flips from 3|16 (asserted for the aligned twin) to 2|16: <64, 20>
  c = 64, n = 256 and 300, k = 20 and 19 with PCOPS_OPT_KNN_F16_PREFILTER = 0 (restored in finally): 2|16, <64, 20>
  seeded (pcops_knn_graph_seeded called directly): n = 129, c = 3, 16, 64, 128 (every CP), k = 1, 19, 20 (KL = 20) and
    21, 31, 32 (KL = 32); hints: the true graph, the graph of perturbed features, random permutations, the k farthest,
    one index k times, a repeated pair at positions 0 and 1 (two half-waves), 0 and 2, k - 3 and k - 1 (one half-wave),
    an index of -1, an index of n: bit-identical to the unseeded call and to the oracle; the first three hints on a lattice
    FOUND HERE: (129, 3, 19) with the true graph whose last entry is -1 (every CP and KL, and the fp16 kernel, failed
    alike): a row that only ONE of a query's two lanes saw as invalid -- an index out of range, or a repeat inside one
    half-wave -- was still trusted by the other lane, which then dropped the k-th neighbour.  Fixed in csrc/knn.hip.
knn_f16_kernel<20> -- path 3|16; c = 64, n >= 256, k <= 20, x 16-byte aligned; 256 queries per workgroup of 512 threads
  n = 256, 257, 385, 513 x k = 1, 19, 20, all six families; few and line also at n = 257, k = 20
  n = 256, k = 20: features beyond the fp16 range (the filter switches itself off), fp16-subnormal mix
  seeded: n = 257, k = 1, 19, 20, every hint
knn_graph_kernel<C, TJ> -- path 1 (k > 32, ignores a seed); TJ = 128 for C <= 32, else 64
  c = 3 -> C = 4, 8 -> 8, 9 -> 16, 32 -> 32, 33 -> 64, 128 -> 128, each at k = 33 and n = 33, 100, 257
    (n = 257: the 256-thread block drops to 192 for C = 4, 8, 16, to 128 for C = 32, to 64 for C = 64 and 128)
  c = 3, k = 123 and c = 128, k = 63 at n = 257: the largest k whose lists fit 64 KB of LDS at 64 threads, one per TJ;
    k = 124 and k = 64: PCOPS_ERR_UNSUPPORTED, nn_idx untouched
  c = 16, k = 40, n = 257 misaligned; a seed at (257, 16, 33): bit 16 of the path clear, the same graph
  c = 129: path 0, PCOPS_ERR_UNSUPPORTED, untouched; the Python wrapper raises PcopsError
  b = 0: PCOPS_OK, nothing written; k = 0 and k = n + 1: PCOPS_ERR_BAD_ARGUMENT
pairwise_distance_kernel -- c = 1, 32, 33, 65 (32-channel chunks) x n = 63, 64, 65 (64 x 64 tiles): bit-equal to the oracle,
  within band of dist64
knn_topk_kernel -- rows = 1, 64, 65 x n = 64, 65, 130 x k = 1, 20, 95 on matrices with exact ties; k = 96: unsupported
edge_feature_kernel<4> -- c = 4, 64 aligned;  <1> -- c = 3, 5, 13, and c = 4 misaligned;  k = 1;
  b n k c = 16 640 x 256 (8, 2048, 20, 13): the grid-stride loop runs
edge_feature_grad_kernel<false> (atomics) and <true> + pcops_scatter_rows_sorted -- the same graphs, among them `hub` (point
  0 in every list, the second half of the points in none); k = 0; deterministic mode: the atomic form is unsupported
"""
import numpy as np
import pytest
import torch

import knn_checks as K
import knn_ref as R
from edge_checks import make_graph
from oracle import oracle as O
from scanobjectnn_amd import _lib
from scanobjectnn_amd.dgcnn import tf_util as dg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def P(t):
    return t.data_ptr() if t is not None else None


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, misaligned=False):
    """the array on the device, 16-byte aligned or starting one float past such a boundary inside a larger buffer"""
    a = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.empty(a.numel() + 8, dtype=a.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    t = buf[1:1 + a.numel()] if misaligned else buf[:a.numel()]
    t = t.view(a.shape)
    t.copy_(a)
    assert t.data_ptr() % 16 == (4 if misaligned else 0) and t.is_contiguous()
    return t


def _done(*outs):
    torch.cuda.synchronize()
    for o in outs:
        assert o.guards_intact()


def graph(x, k, seed=None):
    b, n, c = x.shape
    nn = K.Out((b, n, k), dtype=torch.int32, device=DEV)
    if seed is None:
        _lib.call("pcops_knn_graph", b, n, c, k, P(x), nn.ptr())
    else:
        _lib.call("pcops_knn_graph_seeded", b, n, c, k, P(x), P(seed), nn.ptr())
    _done(nn)
    return nn


def graph_twice(x, k, seed=None):
    first, second = graph(x, k, seed), graph(x, k, seed)
    assert torch.equal(first.t, second.t)
    return first.t


def path_of(x, k):
    b, n, c = x.shape
    return int(_lib.load().pcops_knn_graph_path(b, n, c, k, P(x)))


def held(xh, x, k, path, ties):
    """path, exactness, definition; returns the oracle's graph"""
    assert path_of(x, k) == path
    nn = graph_twice(x, k)
    want = O.knn_graph(xh, k)
    got = nn.cpu().numpy()
    share = R.undecided_share(x, k)
    print("n %d c %d k %d path %d undecided share %.4f" % (xh.shape[1], xh.shape[2], k, path, share))
    np.testing.assert_array_equal(got, want)
    assert R.check_lists(x, nn, k) == xh.shape[0] * xh.shape[1]
    if not ties:
        assert share <= K.share_cap(xh.shape[1])
    return want


def run_case(case):
    fam, b, n, c, k, mis, path = case
    xh = K.cloud(fam, b, n, c)
    held(xh, _dev(xh, mis), k, path, fam in K.TIES)
    return xh


# ---------------------------------------------------------------------------------------------------------- fused graph
@pytest.mark.parametrize("case", K.MFMA_CASES, ids=K.case_id)
def test_mfma_kernel(case):
    fam, b, n, c, k, mis, path = case
    xh = run_case(case)
    if c == 64 and n >= 256 and k <= 20 and mis:                        # the aligned twin would take the fp16 kernel
        assert path_of(_dev(xh), k) == K.F16


@pytest.mark.parametrize("case", K.NO_PREFILTER_CASES, ids=K.case_id)
def test_mfma_kernel_without_the_prefilter(case):
    fam, b, n, c, k, mis, path = case
    xh = K.cloud(fam, b, n, c)
    x = _dev(xh)
    assert path_of(x, k) == K.F16
    prev = _lib.set_option(_lib.OPT_KNN_F16_PREFILTER, 0)
    try:
        held(xh, x, k, path, fam in K.TIES)
    finally:
        _lib.set_option(_lib.OPT_KNN_F16_PREFILTER, prev)
    assert path_of(x, k) == K.F16


@pytest.mark.parametrize("case", K.F16_CASES, ids=K.case_id)
def test_f16_kernel(case):
    run_case(case)


@pytest.mark.parametrize("name", K.F16_EDGE_INPUTS)
def test_f16_kernel_edge_inputs(name):
    xh = K.edge_input(name)
    held(xh, _dev(xh), 20, K.F16, False)


@pytest.mark.parametrize("case", K.GENERIC_CASES, ids=K.case_id)
def test_generic_kernel(case):
    run_case(case)


@pytest.mark.parametrize("n,c,k,path", K.SEEDED_CASES, ids=str)
def test_seeded(n, c, k, path):
    """whatever the hint, the seeded call gives the unseeded graph and the oracle's, bit for bit"""
    rng = np.random.default_rng(100 * c + k)
    xh = K.cloud("gauss", 2, n, c, seed=1)
    x = _dev(xh)
    want = held(xh, x, k, path, False)
    d64 = R.dist64(x).cpu().numpy()
    for kind in K.HINTS:
        if (kind == "pair_0_1" and k < 2) or (kind in ("pair_0_2", "pair_last") and k < 3):
            continue
        seed = K.hint(kind, xh, k, want, d64, rng)
        assert seed.shape == want.shape and seed.dtype == np.int32
        got = graph_twice(x, k, _dev(seed)).cpu().numpy()
        assert np.array_equal(got, want), "hint %s: %d rows differ" % (kind, int((got != want).any(axis=2).sum()))
    # the same hints on a tie-ridden cloud: the bound must keep every tie the unseeded scan keeps
    lh = K.cloud("lattice", 2, n, c, seed=1)
    lx = _dev(lh)
    lwant = held(lh, lx, k, path, True)
    for kind in ("exact", "perturbed", "random"):
        got = graph_twice(lx, k, _dev(K.hint(kind, lh, k, lwant, R.dist64(lx).cpu().numpy(), rng))).cpu().numpy()
        assert np.array_equal(got, lwant), "lattice, hint %s" % kind


def test_seed_on_the_generic_path_is_ignored():
    """k = 33 runs knn_graph_kernel, which takes no seed: bit 16 of the path is clear and the graph is the same"""
    rng = np.random.default_rng(33)
    xh = K.cloud("gauss", 2, 257, 16)
    x = _dev(xh)
    assert path_of(x, 33) == K.GENERIC and not path_of(x, 33) & 16
    want = held(xh, x, 33, K.GENERIC, False)
    for kind in ("random", "farthest", "minus_one", "index_n"):
        seed = K.hint(kind, xh, 33, want, R.dist64(x).cpu().numpy(), rng)
        assert np.array_equal(graph_twice(x, 33, _dev(seed)).cpu().numpy(), want)


def test_graph_unsupported_and_argument_errors():
    lib = _lib.load()
    for n, c, k, path in K.GENERIC_UNSUPPORTED:
        xh = K.cloud("gauss", 2, n, c)
        x = _dev(xh)
        assert path_of(x, k) == path
        nn = K.Out((2, n, k), dtype=torch.int32, device=DEV)
        seed = _dev(np.zeros((2, n, k), np.int32))
        assert lib.pcops_knn_graph(2, n, c, k, P(x), nn.ptr(), _stream()) == K.UNSUPPORTED
        assert lib.pcops_knn_graph_seeded(2, n, c, k, P(x), P(seed), nn.ptr(), _stream()) == K.UNSUPPORTED
        torch.cuda.synchronize()
        assert nn.untouched()
    with pytest.raises(_lib.PcopsError):
        dg.knn_graph(_dev(K.cloud("gauss", 2, 64, 129)), k=20)
    xh = K.cloud("gauss", 2, 40, 3)
    x = _dev(xh)
    nn = K.Out((2, 40, 20), dtype=torch.int32, device=DEV)
    assert lib.pcops_knn_graph(0, 40, 3, 20, P(x), nn.ptr(), _stream()) == K.OK               # no clouds
    assert lib.pcops_knn_graph(0, 40, 3, 20, None, None, _stream()) == K.OK
    assert lib.pcops_knn_graph(2, 40, 3, 0, P(x), nn.ptr(), _stream()) == K.BAD_ARGUMENT
    assert lib.pcops_knn_graph(2, 40, 3, 41, P(x), nn.ptr(), _stream()) == K.BAD_ARGUMENT
    assert lib.pcops_knn_graph_seeded(2, 40, 3, 41, P(x), nn.ptr(), nn.ptr(), _stream()) == K.BAD_ARGUMENT
    torch.cuda.synchronize()
    assert nn.untouched()


# ---------------------------------------------------------------------------------------------------- materialised pair
def pairwise(x):
    b, n, c = x.shape
    adj = K.Out((b, n, n), device=DEV)
    _lib.call("pcops_pairwise_distance", b, n, c, P(x), adj.ptr())
    _done(adj)
    return adj


@pytest.mark.parametrize("b,n,c", K.PAIRWISE_CASES, ids=str)
@pytest.mark.parametrize("family", ["gauss", "offset"])
def test_pairwise_distance(family, b, n, c):
    xh = K.cloud(family, b, n, c)
    x = _dev(xh)
    adj, again = pairwise(x), pairwise(x)
    assert K.bits_equal(adj.t, again.t)
    assert torch.isfinite(adj.t).all()
    np.testing.assert_array_equal(adj.t.cpu().numpy(), O.pairwise_distance(xh))
    ratio = R.contract_ratio(x, adj.t)
    print("%s n %d c %d contract / band %.3g" % (family, n, c, ratio))
    assert ratio <= 1.0


def _topk_matrix(rows, n, rng):
    """rows of a distance-like matrix quantised to a few values: exact ties in every row; row 0 constant, the last row
    descending (every later candidate nearer than all before it)"""
    adj = (rng.integers(0, 12, (rows, n)) * 0.25 - 1.0).astype(np.float32)
    adj[0] = 0.5
    adj[-1] = -np.arange(n, dtype=np.float32)
    if rows > 2:
        adj[1] = rng.standard_normal(n).astype(np.float32)
    return adj


def topk(adj, rows, n, k):
    nn = K.Out((rows, k), dtype=torch.int32, device=DEV)
    _lib.call("pcops_knn_topk", rows, n, k, P(adj), nn.ptr())
    _done(nn)
    return nn


@pytest.mark.parametrize("rows,n,k", K.TOPK_CASES, ids=str)
def test_knn_topk(rows, n, k):
    rng = np.random.default_rng(rows * 1000 + n + k)
    ah = _topk_matrix(rows, n, rng)
    adj = _dev(ah)
    nn, again = topk(adj, rows, n, k), topk(adj, rows, n, k)
    assert torch.equal(nn.t, again.t)
    got = nn.t.cpu().numpy()
    np.testing.assert_array_equal(got, np.argsort(ah.astype(np.float64), axis=1, kind="stable")[:, :k])   # ties -> lower index
    np.testing.assert_array_equal(got, O.knn(ah[None], k)[0])


def test_knn_topk_unsupported_and_argument_errors():
    lib = _lib.load()
    adj = _dev(_topk_matrix(65, 130, np.random.default_rng(0)))
    nn = K.Out((65, 96), dtype=torch.int32, device=DEV)
    assert lib.pcops_knn_topk(65, 130, 96, P(adj), nn.ptr(), _stream()) == K.UNSUPPORTED
    assert lib.pcops_knn_topk(65, 130, 0, P(adj), nn.ptr(), _stream()) == K.BAD_ARGUMENT
    assert lib.pcops_knn_topk(65, 130, 131, P(adj), nn.ptr(), _stream()) == K.BAD_ARGUMENT
    assert lib.pcops_knn_topk(0, 130, 20, P(adj), nn.ptr(), _stream()) == K.OK
    torch.cuda.synchronize()
    assert nn.untouched()


# -------------------------------------------------------------------------------------------------------- edge features
def _edge_inputs(case):
    kind, b, n, c, k, mis, vec = case
    gen = torch.Generator(device=DEV)
    gen.manual_seed(n * 31 + c)
    idx = make_graph(kind, b, n, n, k, gen)
    x = _dev(torch.randn(b, n, c, generator=gen, device=DEV).cpu().numpy(), mis)
    go = torch.randn(b, n, k, 2 * c, generator=gen, device=DEV)
    return idx, x, go


def _grad_reference(idx, go, b, n, c, k):
    """float64 scatter: grad_x[b, i] = sum_s (ga - gb)[b, i, s] + sum over (i', s) with idx[b, i', s] == i of gb[b, i', s];
    A the sum of the magnitudes of the addends, L the addends of the row (its in-degree) + k"""
    ga, gb = go[..., :c].double(), go[..., c:].double()
    flat = (idx.long() + n * torch.arange(b, device=idx.device).view(b, 1, 1)).reshape(-1)
    ref = (ga - gb).sum(dim=2).reshape(b * n, c).index_add(0, flat, gb.reshape(-1, c))
    A = (ga.abs() + gb.abs()).sum(dim=2).reshape(b * n, c).index_add(0, flat, gb.abs().reshape(-1, c))
    deg = torch.zeros(b * n, dtype=torch.float64, device=idx.device).index_add(
        0, flat, torch.ones(flat.numel(), dtype=torch.float64, device=idx.device))
    return ref.view(b, n, c), A.view(b, n, c), (deg + k).view(b, n, 1), deg.view(b, n)


@pytest.mark.parametrize("case", K.EDGE_CASES, ids=str)
def test_edge_feature_and_gradients(case):
    kind, b, n, c, k, mis, vec = case
    idx, x, go = _edge_inputs(case)
    assert (x.data_ptr() % 16 == 0 and c % 4 == 0) == (vec == 4)

    def fwd():
        out = K.Out((b, n, k, 2 * c), device=DEV)
        assert out.ptr() % 16 == 0
        _lib.call("pcops_edge_feature", b, n, c, k, P(x), P(idx), out.ptr())
        _done(out)
        return out

    out, again = fwd(), fwd()
    assert K.bits_equal(out.t, again.t)
    xi = x.view(b, n, 1, c).expand(b, n, k, c)
    xj = x.reshape(b * n, c)[(idx.long() + n * torch.arange(b, device=DEV).view(b, 1, 1)).reshape(-1)].view(b, n, k, c)
    assert K.bits_equal(out.t, torch.cat([xi, xj - xi], dim=3))               # one fp32 subtraction: exact agreement
    np.testing.assert_array_equal(out.t.cpu().numpy(), O.get_edge_feature(x.cpu().numpy(), idx.cpu().numpy(), k))

    ref, A, L, deg = _grad_reference(idx, go, b, n, c, k)
    if kind == "hub":
        assert (deg[:, 0] >= n).all() and (deg[:, (n + 1) // 2:] == 0).all()  # everybody's neighbour; nobody's
    gx = K.Out((b, n, c), device=DEV)
    _lib.call("pcops_edge_feature_grad", b, n, c, k, P(go), P(idx), gx.ptr())
    _done(gx)
    K.check_sum(gx.t, (ref, A, L), "grad_x (atomics)")

    def ordered():
        g = K.Out((b, n, c), device=DEV)
        _lib.call("pcops_edge_feature_grad_central", b, n, c, k, P(go), g.ptr())
        _done(g)
        _lib.scatter_rows_sorted(idx.view(b, n * k), None, n, out=g.t, c=c, ld=2 * c, src_ptr=go.data_ptr() + 4 * c)
        _done(g)
        return g

    g1, g2 = ordered(), ordered()
    assert K.bits_equal(g1.t, g2.t)
    K.check_sum(g1.t, (ref, A, L), "grad_x (central + ordered scatter)")


def test_edge_feature_gradient_edges():
    case = ("knn", 2, 33, 4, 5, False, 4)
    kind, b, n, c, k, mis, vec = case
    idx, x, go = _edge_inputs(case)
    lib = _lib.load()
    gx = K.Out((b, n, c), device=DEV)
    was = _lib.deterministic()
    _lib.set_deterministic(True)
    try:                                                                      # atomics are refused in deterministic mode
        assert lib.pcops_edge_feature_grad(b, n, c, k, P(go), P(idx), gx.ptr(), _stream()) == K.UNSUPPORTED
        torch.cuda.synchronize()
        assert gx.untouched()
    finally:
        _lib.set_deterministic(was)
    # k = 0: the gradient is all zeros, nothing else is written, no other pointer is read
    for fn, args in (("pcops_edge_feature_grad", (None, None)), ("pcops_edge_feature_grad_central", (None,))):
        g0 = K.Out((b, n, c), device=DEV)
        _lib.call(fn, b, n, c, 0, *args, g0.ptr())
        _done(g0)
        assert (g0.t == 0).all()
    out = K.Out((b, n, 1, 2 * c), device=DEV)
    _lib.call("pcops_edge_feature", b, n, c, 0, P(x), P(idx), out.ptr())
    _lib.call("pcops_edge_feature", 0, n, c, k, None, None, None)
    torch.cuda.synchronize()
    assert out.untouched()
