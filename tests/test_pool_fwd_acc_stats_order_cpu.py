"""The summation order of the pooled forward's statistics, restated in numpy float32.

The transposing epilogue of gemm_ws_kernel sums a 32 x 128 tile in four 32-column passes: in pass h lane l owns the column
quad 4 (l % 8) of columns 32 h .. and the rows rho + 8 j, rho = l / 8, j = 0 .. 3 ascending, tile after tile; the waves'
closing reduction is shfl_xor 32, 16, 8 on the lane number, i.e. rho ^ 4, 2, 1.  The kernel that stores no Y sums on the
accumulator registers: acc[nt][v] of lane l is row (v & 3) + 8 (v >> 2) + 4 (l >> 5), column 32 nt + (l & 31), the sums
S[nt][i] run over acc[nt][i + 4 j], j ascending, and the closing tree is t_i = S[nt][i] + (lane ^ 32's), (t0 + t2) + (t1 + t3).

Both are walked here over the same tiles, every chain in its own order (the lanes side by side as array axes); first and
second moment must come out bit for bit equal -- ragged last tile, block weights on tile rows 0 and 16, values over six
decades -- and two near misses (rows in plain ascending order, the tree as (t0 + t1) + (t2 + t3)) must NOT."""
import numpy as np
import pytest

F = np.float32
NT = 4


def _fma(a, b, c):
    """fmaf(a, b, c) on float32 arrays: the product is exact in float64; the float64 sum is rounded TO ODD (TwoSum gives the
    sign of what round-to-nearest dropped), and a round-to-odd 53-bit value rounds to 24 bits like the exact one"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (e != 0.0) & even
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F)


def test_fma_restatement_rounds_once():
    # 1 + 2^-24 (a tie of the float32 grid) plus a product far below it: fused rounds up, the twice-rounded sum does not
    a, b, c = np.array([F(2.0 ** -30)]), np.array([F(2.0 ** -30)]), np.array([np.float64(1.0 + 2.0 ** -24)])
    got = _fma(a, b, c)          # (c is not a float32 here on purpose: the addend's width is not what is under test)
    assert got[0] == F(1.0 + 2.0 ** -23)
    assert (a.astype(np.float64) * b.astype(np.float64) + c).astype(F)[0] == F(1.0)


def _tiles(ntile, rows_last, seed, decades):
    g = np.random.default_rng(seed)
    mag = 10.0 ** g.uniform(-decades / 2.0, decades / 2.0, size=(ntile, 32, 32 * NT))
    t = (g.standard_normal((ntile, 32, 32 * NT)) * mag).astype(F)
    return t, [32] * (ntile - 1) + [rows_last]


def _add(S1, S2, o, w, live):
    """one step of every chain: S1 += w o, S2 = fmaf(w o, o, S2) where `live` (w None: the unweighted form)"""
    wo = o if w is None else (w * o).astype(F)
    return np.where(live, (S1 + wo).astype(F), S1), np.where(live, _fma(wo, o, S2), S2)


def transposed(tiles, rem, weights):
    """[2][128] as the transposing epilogue and its shfl_xor 32, 16, 8 tree leave them (one wave).
    State [pass h][rho = lane / 8][column of the pass = 4 (lane % 8) + e]"""
    s1 = np.zeros((NT, 8, 32), F)
    s2 = np.zeros((NT, 8, 32), F)
    rho = np.arange(8)
    for t, tile in enumerate(tiles):
        for j in range(4):
            rows = rho + 8 * j
            o = tile[rows].reshape(8, NT, 32).transpose(1, 0, 2)
            live = (rows < rem[t])[None, :, None]
            w = None
            if weights is not None and j % 2 == 0:         # the step's first row (lanes 0 .. 7) opens a 16-row block
                w = np.ones((1, 8, 1), F)
                w[0, 0, 0] = weights[2 * t + j // 2]
            s1, s2 = _add(s1, s2, o, w, live)
    for x in (4, 2, 1):                                    # shfl_xor 32, 16, 8 of the lane number
        s1 = (s1 + s1[:, rho ^ x]).astype(F)
        s2 = (s2 + s2[:, rho ^ x]).astype(F)
    return np.stack([s1[:, 0].reshape(-1), s2[:, 0].reshape(-1)])


def from_accumulators(tiles, rem, weights, ascending_rows=False, tree="02_13"):
    """[2][128] from the accumulator layout.  State [nt][half = lane >> 5][i][lane & 31]; the two keyword arguments build
    the near misses"""
    S1 = np.zeros((NT, 2, 4, 32), F)
    S2 = np.zeros((NT, 2, 4, 32), F)
    half, ii = np.arange(2)[:, None], np.arange(4)[None, :]
    for t, tile in enumerate(tiles):
        for j in range(4):
            rows = ii + 8 * j + 4 * half                                        # [half][i]: register v = i + 4 j
            o = tile[rows.reshape(-1)].reshape(2, 4, NT, 32).transpose(2, 0, 1, 3)
            live = (rows < rem[t])[None, :, :, None]
            w = None
            if weights is not None and j % 2 == 0:                              # tile rows 0 / 16: lanes 0 .. 31, i = 0
                w = np.ones((1, 2, 4, 1), F)
                w[0, 0, 0, 0] = weights[2 * t + j // 2]
            if not ascending_rows:
                S1, S2 = _add(S1, S2, o, w, live)
            else:                                                               # ONE chain per lane and column block
                for i in range(4):
                    S1[:, :, 0], S2[:, :, 0] = _add(S1[:, :, 0], S2[:, :, 0], o[:, :, i], None if w is None else w[:, :, i],
                                                    live[:, :, i])
    out = []
    for S in (S1, S2):
        t = (S[:, 0] + S[:, 1]).astype(F)                                       # lane + (lane ^ 32): [nt][i][32]
        if tree == "02_13":
            r = ((t[:, 0] + t[:, 2]).astype(F) + (t[:, 1] + t[:, 3]).astype(F)).astype(F)
        else:
            r = ((t[:, 0] + t[:, 1]).astype(F) + (t[:, 2] + t[:, 3]).astype(F)).astype(F)
        out.append(r.reshape(-1))
    return np.stack(out)


def _weights(ntile, rem_last, seed):
    """block weights: 1 + the copies a compacted group leaves out (1 .. 49); the block beyond the last clamped to the last"""
    g = np.random.default_rng(seed)
    w = g.integers(1, 50, size=2 * ntile).astype(F)
    nblk = 2 * (ntile - 1) + (rem_last + 15) // 16
    w[nblk:] = w[nblk - 1]
    return w


CASES = [  # tiles, rows of the last tile, weighted, decades
    (37, 32, False, 6.0), (37, 17, False, 6.0), (5, 32, True, 6.0), (37, 9, True, 6.0), (3, 16, True, 2.0), (1, 1, True, 6.0),
]


@pytest.fixture(scope="module")
def walked():
    out = {}
    for c in CASES:
        ntile, last, weighted, dec = c
        tiles, rem = _tiles(ntile, last, seed=ntile * 100 + last, decades=dec)
        w = _weights(ntile, last, seed=7) if weighted else None
        out[c] = (tiles, rem, w, transposed(tiles, rem, w))
    return out


@pytest.mark.parametrize("case", CASES)
def test_accumulator_order_equals_the_transposed_order(walked, case):
    tiles, rem, w, want = walked[case]
    got = from_accumulators(tiles, rem, w)
    assert np.isfinite(want).all() and (want[1] > 0).all()
    assert got.tobytes() == want.tobytes(), "moments differ in %d of %d places" % ((got != want).sum(), got.size)


def test_row_classes_of_both_layouts_are_the_same_chains():
    """the mapping itself: (rho, column) of the transposed pass is the registers acc[nt][i + 4 j] of lane
    32 (rho >> 2) + column % 32 with i = rho & 3, and the shuffles pair the row classes the tree says"""
    for lane in range(64):
        rho, q = lane // 8, lane % 8
        for j in range(4):
            for e in range(4):
                col = 4 * q + e
                l2, i = 32 * (rho >> 2) + col, rho & 3
                v = i + 4 * j
                assert (v & 3) + 8 * (v >> 2) + 4 * (l2 >> 5) == rho + 8 * j and (l2 & 31) == col
    for off, x in ((32, 4), (16, 2), (8, 1)):
        assert all(((lane ^ off) // 8) == ((lane // 8) ^ x) for lane in range(64))


def test_plain_ascending_rows_is_rejected(walked):
    tiles, rem, w, want = walked[CASES[0]]
    got = from_accumulators(tiles, rem, w, ascending_rows=True)
    assert (got[0] != want[0]).sum() > 64 and (got[1] != want[1]).sum() > 64


def test_the_other_tree_is_rejected(walked):
    tiles, rem, w, want = walked[CASES[0]]
    got = from_accumulators(tiles, rem, w, tree="01_23")
    assert (got[0] != want[0]).sum() > 16 and (got[1] != want[1]).sum() > 16
