"""pcops_mlp_pool_top_addend_rows under PCOPS_OPT_POOL_TOP_ROWS_PIPELINED = 1 (pooltop_sparse.hip pool_top_addend_rows_pipe_kernel: a
wave per group, the row's hits as ballots, the next row's W^T reads in flight) against the kernel it replaces (option 0)
and against float64 (2e-5 of the largest element, the bound of that file's _close), on the row sets and pool inputs of test_pool_top_rows_gpu.py.

The contract is "the same bits": per row and column both kernels run one fmaf chain over the row's hits in ascending channel
order from 0, so rowmap is equal, the addend is bit-identical on the hit rows and untouched (still NaN) on every other row.
All four (S, Kp, N) shapes take the new kernel under option 1 (pcops.h).

Group counts.  The new kernel runs min(ceil(G / 16), 256) workgroups of 16 waves, a wave per group and trip of its persistent
loop, so a wave takes a second group only beyond 4096 groups: 8 (one workgroup, half of its waves without a group), 1032 (64
full workgroups and one with 8 of 16 waves busy; the former kernel's 4-group rounds end ragged there), that file's own count,
4104 (256 x 16 + 8: eight waves take a second group, every other wave's prefetch for the second trip lies beyond G) and 8208
(two full trips and a ragged third: the next group's triple and the block_start pair two groups ahead are both in use).

Hit patterns on top of that file's three (everything on the weighted row, no coefficient, one coefficient; group 3 puts
everything on its last row): group 4 carries exactly 1, 2, 3, 4 and 5 hits on the rows 3 .. 7 (one, two and three of them
inside one 64-channel word: the slot and the loop behind it), the channels 31, 32, 63, 64 and N - 1 together on row 9 and
once more, one per row, on the rows 10 .. 14 of group 6.

The comparison is not empty: some row carries >= 8 hits, and more than half of all rows are hit.  At G = 8 the latter cannot
hold -- that file's four special groups own 176 of the 288 rows (S = 64) and three hit rows, and this file's two own 32 and
11 -- so there the hit rows of every constructed group are asserted exactly (1, 0, 1, 1, 6, 5) and the two groups of random
picks to a quarter of their rows (64 live channels over 128 rows leave 39 % of them hit at the sparsest shape)."""
import pytest
import torch

from scanobjectnn_amd import _lib
from test_pool_top_rows_gpu import SHAPES, RowSet, _close, _f, _pool_inputs, _run, _sa2_stack

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _inputs(rs, N, seed):
    """_pool_inputs plus the patterns of the module docstring; cf recomputed in float64"""
    gout, ysel, arg8, sc, sh, p, _, arg = _pool_inputs(rs, N, seed)
    assert int(rs.nrow[4]) >= 16 and int(rs.nrow[6]) >= 16
    ysel[4] = -100.0
    ysel[6] = -100.0
    rows_of = {3: [5], 4: [6, 70], 5: [7, 8, 9], 6: [10, 71, 72, 73], 7: [11, 12, 13, 14, 15], 9: [31, 32, 63, 64, N - 1]}
    for r, chans in rows_of.items():
        for c in chans:
            ysel[4, c] = 10.0
            arg[4, c] = r
    for r, c in zip(range(10, 15), (31, 32, 63, 64, N - 1)):
        ysel[6, c] = 10.0
        arg[6, c] = r
    active = (ysel.double() * sc.double() + sh.double()) > 0
    cf = torch.where(active, p.double() * gout.double(), torch.zeros((), dtype=torch.float64, device=DEV))
    assert bool(active[4].sum() == 20) and bool(active[6].sum() == 5) and bool((gout[4:7] != 0).all())
    return gout, ysel, arg.to(torch.uint8).contiguous(), sc, sh, p, cf, arg


def _addend(rs, Kp, N, pin, Wt, opt):
    gout, ysel, arg8, sc, sh, p, _, _ = pin
    addend = _f(rs.R, Kp).fill_(float("nan"))
    rowmap = torch.full((rs.R,), -7, dtype=torch.int32, device=DEV)
    prev = _lib.set_option(_lib.OPT_POOL_TOP_ROWS_PIPELINED, opt)
    try:
        _lib.call("pcops_mlp_pool_top_addend_rows", rs.R, Kp, N, rs.S, gout.data_ptr(), ysel.data_ptr(), arg8.data_ptr(),
                  sc.data_ptr(), sh.data_ptr(), p.data_ptr(), Wt.data_ptr(), addend.data_ptr(), rowmap.data_ptr(), rs.rows.ref)
    finally:
        _lib.set_option(_lib.OPT_POOL_TOP_ROWS_PIPELINED, prev)
    torch.cuda.synchronize()
    return addend, rowmap


@pytest.mark.parametrize("G", [8, 1032, None, 4104, 8208])
@pytest.mark.parametrize("S,Kp,N", SHAPES)
def test_pipelined_addend_gives_the_former_bits(S, Kp, N, G):
    if G is None:
        G = 65536 // S if S == 64 else 131072 // S
    rs = RowSet(S, G, seed=S + Kp)
    n = rs.n
    pin = _inputs(rs, N, seed=4)
    cf, arg = pin[6], pin[7]
    g = torch.Generator().manual_seed(5)
    Wt = (torch.randn(N, Kp, generator=g) / N ** 0.5).to(DEV)

    # ---- the CPU side: which rows are hit, and how often
    rowof = (rs.first.view(G, 1) + arg).reshape(-1)
    live = cf.reshape(-1) != 0
    per_row = torch.bincount(rowof[live], minlength=n)
    hit = per_row > 0
    f4 = int(rs.first[4])
    assert per_row[f4 + 3:f4 + 8].tolist() == [1, 2, 3, 4, 5] and int(per_row[f4 + 9]) == 5
    f6 = int(rs.first[6])
    assert per_row[f6 + 10:f6 + 15].tolist() == [1, 1, 1, 1, 1] and int(per_row[f6:f6 + int(rs.nrow[6])].sum()) == 5
    f3 = int(rs.first[3])
    assert bool(hit[f3 + int(rs.nrow[3]) - 1]), "a hit on a group's last row"
    assert int(per_row.max()) >= 8, "some row carries >= 8 hits"
    print("S %d Kp %d N %d G %d: %d rows, %d hit, deepest row %d hits" % (S, Kp, N, G, n, int(hit.sum()), int(per_row.max())))
    if G == 8:                                                     # see the module docstring
        per_group = [int(hit[int(rs.first[i]):int(rs.first[i]) + int(rs.nrow[i])].sum()) for i in range(G)]
        assert [per_group[i] for i in (0, 1, 2, 3, 4, 6)] == [1, 0, 1, 1, 6, 5], per_group
        assert all(4 * per_group[i] >= int(rs.nrow[i]) for i in (5, 7)), per_group
    else:
        assert 2 * int(hit.sum()) > n, "more than half of all rows are hit"

    a0, m0 = _addend(rs, Kp, N, pin, Wt, 0)
    a1, m1 = _addend(rs, Kp, N, pin, Wt, 1)
    a2, m2 = _addend(rs, Kp, N, pin, Wt, 1)
    assert torch.equal(m0, m1), "rowmap"
    rm = m1[:n].long()
    assert torch.equal(rm >= 0, hit) and torch.equal(rm[hit], torch.nonzero(hit).view(-1)) and bool((rm[~hit] == -1).all())
    assert bool((m1[n:] == -7).all())
    for name, a in (("former kernel", a0), ("pipelined", a1)):
        assert bool(torch.isnan(a[:n][~hit]).all()) and bool(torch.isnan(a[n:]).all()), name + ": a row without a hit is not written"
    assert bool(torch.isfinite(a1[:n][hit]).all())
    assert torch.equal(a0[:n][hit], a1[:n][hit]), "the former kernel's bits"
    assert torch.equal(a1[:n][hit], a2[:n][hit]) and torch.equal(m1, m2), "two runs of the pipelined kernel"
    want = torch.zeros(n, Kp, dtype=torch.float64, device=DEV)
    want.index_add_(0, rowof, cf.reshape(-1, 1) * Wt.double().repeat(G, 1))
    got = torch.zeros(n, Kp, dtype=torch.float64, device=DEV)
    got[hit] = a1[:n][hit].double()
    _close("addend, pipelined", got, want)


def test_sa2_stack_with_the_pipelined_addend_against_the_former():
    """gather_mlp_stack at the SA2-shaped compacted stack of test_pool_top_rows_gpu.py, the option 1 against 0, in the
    library's deterministic mode: every kernel above the scatter is the same arithmetic under both values, so the forward
    and every gradient are bit-identical."""
    st = _sa2_stack(8, seed=2)
    res = {}
    _lib.set_deterministic(True)
    try:
        for opt in (1, 0):
            prev = _lib.set_option(_lib.OPT_POOL_TOP_ROWS_PIPELINED, opt)
            try:
                rec = []
                res[opt] = _run(st, rec)
                assert len([name for name, _ in rec if name == "pcops_mlp_pool_top_addend_rows"]) == 1
            finally:
                _lib.set_option(_lib.OPT_POOL_TOP_ROWS_PIPELINED, prev)
    finally:
        _lib.set_deterministic(False)
    assert torch.equal(res[1][0], res[0][0])
    for name, x, y in zip(res[1][1], res[1][2], res[0][2]):
        assert torch.equal(x, y), name
