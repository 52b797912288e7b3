"""pcops_mlp_gram_rows on the bf16 matrix pipe with split operands (PCOPS_OPT_GRAM_SPLIT_BF16, mlp.hip gram_rows_bf3_kernel)
and the software-pipelined pcops_mlp_pool_top_wsparse_rows (PCOPS_OPT_POOL_TOP_ROWS_PIPELINED, pooltop_sparse.hip pool_top_wsparse_rows_pipe_kernel)
against float64 and against the kernels they replace, on the row sets of test_pool_top_rows_gpu.py (hand-made member
counts 1, 15, 16, 17, S - 1, S; the all-zero, the one-live-channel and the everything-on-the-weighted-row group), then
the SA2-shaped stack of that file with both options on against both off.

pcops_mlp_pool_top_addend_rows has ONE form under either value of PCOPS_OPT_POOL_TOP_ROWS_PIPELINED (its rewrite was not
built), so there is nothing to compare for it here; test_pool_top_rows_gpu.py pins it against float64.

Kp = 128 takes the split form.  Kp = 64 KEEPS the fp32 kernel under either value of the option (pcops.h): the test pins that
as "same bits, pipe 0".

The bound on the Gram matrix is the one test_pool_top_rows_gpu.py holds every entry point to: 2e-5 of the largest element.
The column sums are the producers' fp32 sums in the order of the fp32 kernel: bit-identical between the two option values."""
import pytest
import torch

from scanobjectnn_amd import _lib
from test_pool_top_rows_gpu import REL, RowSet, _close, _f, _pool_inputs, _prev, _run, _sa2_stack

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOTH = (_lib.OPT_GRAM_SPLIT_BF16, _lib.OPT_POOL_TOP_ROWS_PIPELINED)


def _gram_rows(lib, rs, Kp, Yprev, psc, psh, opt):
    splits = lib.pcops_mlp_wgrad_splits(rs.R, Kp, Kp)
    scratch, gram, xsum = _f(splits * (Kp * Kp + Kp)).fill_(float("nan")), _f(Kp, Kp), _f(Kp)
    prev = _lib.set_option(_lib.OPT_GRAM_SPLIT_BF16, opt)
    try:
        _lib.call("pcops_mlp_gram_rows", rs.R, Kp, Yprev.data_ptr(), Kp, psc.data_ptr(), psh.data_ptr(), scratch.data_ptr(),
                  gram.data_ptr(), xsum.data_ptr(), rs.rows.ref)
        pipe = int(lib.pcops_last_launch_pipe())
    finally:
        _lib.set_option(_lib.OPT_GRAM_SPLIT_BF16, prev)
    torch.cuda.synchronize()
    return gram, xsum, pipe


@pytest.mark.parametrize("S,Kp", [(64, 128), (128, 128)])
def test_split_gram_against_float64_and_the_fp32_kernel(S, Kp):
    lib = _lib.load()
    G = 65536 // S if S == 64 else 131072 // S
    rs = RowSet(S, G, seed=S + Kp)
    Yprev, psc, psh, X = _prev(rs, Kp, seed=3)
    want = X.t() @ (X * rs.w.view(-1, 1))
    scale = want.abs().max().item()
    g0, x0, pipe0 = _gram_rows(lib, rs, Kp, Yprev, psc, psh, 0)
    g1, x1, pipe1 = _gram_rows(lib, rs, Kp, Yprev, psc, psh, 1)
    e0 = (g0.double() - want).abs().max().item()
    e1 = (g1.double() - want).abs().max().item()
    print("gram S %d Kp %d: largest element %.3e   fp32 kernel max err %.3e (ratio %.3e)   split operands max err %.3e (ratio %.3e)"
          % (S, Kp, scale, e0, e0 / scale, e1, e1 / scale))
    assert pipe0 == 0 and pipe1 == 1
    assert torch.isfinite(g1).all()
    assert e1 <= REL * scale, ("split gram", e1, scale)
    assert e0 <= REL * scale, ("fp32 gram", e0, scale)
    assert torch.equal(g1, g1.t()), "the lower triangle is the mirror of the upper one"
    assert torch.equal(x0, x1), "column sums: the fp32 sums of the other form, bit for bit"
    # fixed-order sums, no atomics: a second run of the split form gives the same bits
    g2, x2, _ = _gram_rows(lib, rs, Kp, Yprev, psc, psh, 1)
    assert torch.equal(g1, g2) and torch.equal(x1, x2)


@pytest.mark.parametrize("S,Kp", [(64, 64), (128, 64)])
def test_kp64_keeps_the_fp32_kernel(S, Kp):
    lib = _lib.load()
    G = 65536 // S if S == 64 else 131072 // S
    rs = RowSet(S, G, seed=S + Kp)
    Yprev, psc, psh, _ = _prev(rs, Kp, seed=3)
    g0, x0, pipe0 = _gram_rows(lib, rs, Kp, Yprev, psc, psh, 0)
    g1, x1, pipe1 = _gram_rows(lib, rs, Kp, Yprev, psc, psh, 1)
    assert pipe0 == 0 and pipe1 == 0
    assert torch.equal(g0, g1) and torch.equal(x0, x1)


def _sparse_halves(lib, rs, Kp, N, Yprev, psc, psh, pin, opt):
    """the sparse half of the weight gradient under one value of PCOPS_OPT_POOL_TOP_ROWS_PIPELINED"""
    gout, ysel, arg8, sc, sh, p, _, _ = pin
    R, S = rs.R, rs.S
    Ssp, cfsum = _f(Kp, N), _f(N)
    wpart = _f(int(lib.pcops_mlp_pool_top_wsparse_rows_partial(Kp, N))).fill_(float("nan"))
    prev = _lib.set_option(_lib.OPT_POOL_TOP_ROWS_PIPELINED, opt)
    try:
        _lib.call("pcops_mlp_pool_top_wsparse_rows", R, Kp, N, S, gout.data_ptr(), ysel.data_ptr(), arg8.data_ptr(),
                  sc.data_ptr(), sh.data_ptr(), p.data_ptr(), Yprev.data_ptr(), psc.data_ptr(), psh.data_ptr(),
                  Ssp.data_ptr(), cfsum.data_ptr(), wpart.data_ptr(), rs.rows.ref)
    finally:
        _lib.set_option(_lib.OPT_POOL_TOP_ROWS_PIPELINED, prev)
    torch.cuda.synchronize()
    return Ssp, cfsum


@pytest.mark.parametrize("S,Kp,N", [(64, 128, 256), (128, 128, 256), (64, 64, 128), (128, 64, 128)])
def test_pipelined_sparse_halves(S, Kp, N):
    """wsparse: Ssp and cfsum of the pipelined kernel against float64 at 2e-5 of the largest element, two runs bit-identical
    (both widths take the new kernel), and -- same partition, same fmaf chains -- the former kernel's bits."""
    lib = _lib.load()
    G = 65536 // S if S == 64 else 131072 // S
    rs = RowSet(S, G, seed=S + Kp)
    Yprev, psc, psh, X = _prev(rs, Kp, seed=3)
    pin = _pool_inputs(rs, N, seed=4)
    cf, arg = pin[6], pin[7]
    s0, c0 = _sparse_halves(lib, rs, Kp, N, Yprev, psc, psh, pin, 0)
    s1, c1 = _sparse_halves(lib, rs, Kp, N, Yprev, psc, psh, pin, 1)
    s2, c2 = _sparse_halves(lib, rs, Kp, N, Yprev, psc, psh, pin, 1)
    rowof = (rs.first.view(G, 1) + arg).reshape(-1)
    want_s = torch.zeros(Kp, N, dtype=torch.float64, device=DEV)
    for g0 in range(0, G, 256):
        rows_ = rowof.view(G, N)[g0:g0 + 256]
        want_s += torch.einsum("gc,gck->kc", cf[g0:g0 + 256], X[rows_.reshape(-1)].view(rows_.shape[0], N, Kp))
    _close("Ssp, former kernel", s0, want_s)
    _close("Ssp, pipelined", s1, want_s)
    _close("cfsum, pipelined", c1, cf.sum(0))
    assert torch.equal(s1, s2) and torch.equal(c1, c2), "two runs of the pipelined kernel"
    assert torch.equal(s0, s1) and torch.equal(c0, c1), "the former kernel's bits"


def test_sa2_stack_with_both_options_against_neither():
    """gather_mlp_stack at the SA2-shaped compacted stack of test_pool_top_rows_gpu.py, PCOPS_OPT_GRAM_SPLIT_BF16 and
    PCOPS_OPT_POOL_TOP_ROWS_PIPELINED both 1 against both 0: same forward bits, every gradient within 2e-4 * scale + 1e-6 (the bound of that file), and two runs with the option
    on in deterministic mode bit-identical."""
    st = _sa2_stack(32)
    res = {}
    for opt in (1, 0):
        prev = [_lib.set_option(o, opt) for o in BOTH]
        try:
            rec = []
            res[opt] = _run(st, rec)
            for want in ("pcops_mlp_gram_rows", "pcops_mlp_pool_top_wsparse_rows", "pcops_mlp_pool_top_addend_rows"):
                assert len([n for n, _ in rec if n == want]) == 1, want
        finally:
            for o, v in zip(BOTH, prev):
                _lib.set_option(o, v)
    assert torch.equal(res[1][0], res[0][0])
    go_scale = st["go"].abs().max().item()
    for name, a, b in zip(res[1][1], res[1][2], res[0][2]):
        scale = go_scale if name.endswith(".db") else b.abs().max().item()
        err = (a - b).abs().max().item()
        print("%-10s max diff %.3e  scale %.3e" % (name, err, scale))
        assert err <= 2e-4 * scale + 1e-6, (name, err, scale)
    _lib.set_deterministic(True)
    prev = [_lib.set_option(o, 1) for o in BOTH]
    try:
        a, b = _run(st), _run(st)
    finally:
        for o, v in zip(BOTH, prev):
            _lib.set_option(o, v)
        _lib.set_deterministic(False)
    assert torch.equal(a[0], b[0])
    for name, x, y in zip(a[1], a[2], b[2]):
        assert torch.equal(x, y), name
