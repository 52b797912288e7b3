"""The pooled forward with and without the Y store, case by case (tests/test_pool_fwd_acc_stats_gpu.py).  The test imports
this module and runs the cases in its own process; PCOPS_POOL_FWD_ACC_STATS is read once per process, so it also runs

    python tests/pool_fwd_acc_stats_child.py OUT.pt

with PCOPS_POOL_FWD_ACC_STATS=0 in the environment and compares: OUT.pt holds {case name: record}, a record being the
outputs of every call of the case on the CPU next to pcops_last_launch_acc_stats() and pcops_last_launch_plan() behind it.

Outputs live between guard bands and start as NaN (bytes: 0xEE), so a value the kernel did not write, or one it wrote
outside, shows."""
import ctypes as C
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

from scanobjectnn_amd import _lib  # noqa: E402

DEV = "cuda:0"
GUARD = 1024


class Out:
    """n elements of dtype between two guard bands; payload NaN (uint8: 0xEE), guards 12345 (uint8: 0xA5)"""

    def __init__(self, shape, dtype=torch.float32):
        n = 1
        for s in shape:
            n *= s
        self.n, self.shape = n, shape
        self.base = torch.empty(n + 2 * GUARD, dtype=dtype, device=DEV)
        self.guard = 12345.0 if dtype == torch.float32 else 0xA5
        self.base.fill_(self.guard)
        self.t = self.base[GUARD:GUARD + n].view(shape)
        self.t.fill_(float("nan") if dtype == torch.float32 else 0xEE)

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return bool((self.base[:GUARD] == self.guard).all()) and bool((self.base[GUARD + self.n:] == self.guard).all())


def flag():
    return int(_lib.load().pcops_last_launch_acc_stats())


def plan():
    out = (C.c_int * 5)()
    assert _lib.load().pcops_last_launch_plan(out, 5) == 5
    return tuple(out)


def _layer(K, N, seed, pro=True):
    """weights, bias, gamma (every third negative), pivot and the previous layer's BN coefficients of a K -> N layer"""
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(K, N, generator=g) / K ** 0.5).to(DEV)
    b = (0.1 * torch.randn(N, generator=g)).to(DEV)
    gamma = ((0.5 + torch.rand(N, generator=g)) * (1.0 - 2.0 * (torch.arange(N) % 3 == 2))).to(DEV)
    piv = (0.1 * torch.randn(N, generator=g)).to(DEV)
    sc = ((0.5 + torch.rand(K, generator=g)) * (1.0 - 2.0 * (torch.arange(K) % 5 == 4))).to(DEV).contiguous()
    sh = (0.3 * torch.randn(K, generator=g)).to(DEV)
    return W, b, gamma.contiguous(), piv, (sc if pro else None), (sh if pro else None)


# ---- uncompacted pcops_mlp_gemm_fwd_pool.  (name, M, K, N, S, pivot given, pro_scale given, PCOPS_OPT_GEMM_SPLIT_BF16, variant expected)
POOL_CASES = []
for _name, _M, _K, _N, _S in (("flagship_tile", 65536, 64, 128, 32), ("two_tile_groups", 16384, 64, 128, 64),
                              ("two_column_blocks", 16384, 128, 256, 32), ("ragged_k48_n116", 8192, 48, 116, 32)):
    for _piv in (True, False):
        POOL_CASES.append(("%s_%s" % (_name, "pivot" if _piv else "nopivot"), _M, _K, _N, _S, _piv, True, 1, True))
# every other plan keeps its kernel
POOL_CASES += [
    ("keeps_n64", 16384, 64, 64, 32, True, True, 1, False),
    ("keeps_n96", 16384, 64, 96, 32, True, True, 1, False),
    ("keeps_k320_streamed", 16384, 320, 128, 32, True, True, 1, False),
    ("keeps_s20", 160 * 55, 64, 128, 20, True, True, 1, False),
    ("keeps_plain_operand", 16384, 64, 128, 32, True, False, 1, False),
    ("keeps_fp32_pipe", 16384, 64, 128, 32, True, True, 0, False),
]
NEW_PLAN = (2, 1, 128, 0, 1)


def run_pool(case):
    """the storing call, then the call with Y == NULL: {"store": ..., "nostore": ...}, each (flag, plan, part, ysel, argsel)"""
    name, M, K, N, S, use_piv, pro, opt, _ = case
    lib = _lib.load()
    assert lib.pcops_mlp_gemm_fwd_pool_supported(M, K, N, S) == 1, name
    g = torch.Generator().manual_seed(M + K + N + S)
    X = torch.randn(M, K, generator=g).to(DEV)
    W, b, gamma, piv, sc, sh = _layer(K, N, seed=K * 1000 + N, pro=pro)
    P = lib.pcops_mlp_stats_rows(M)
    rec = {}
    prev = _lib.set_option(_lib.OPT_GEMM_SPLIT_BF16, opt)
    try:
        for which in ("store", "nostore"):
            Y = Out((M, N)) if which == "store" else None
            part, ysel, argsel = Out((P, 2, N)), Out((M // S, N)), Out((M // S, N), torch.uint8)
            _lib.call("pcops_mlp_gemm_fwd_pool", M, K, N, S, X.data_ptr(), K, _lib.ptr(sc), _lib.ptr(sh), W.data_ptr(),
                      b.data_ptr(), gamma.data_ptr(), Y.ptr() if Y is not None else None, part.ptr(),
                      piv.data_ptr() if use_piv else None, ysel.ptr(), argsel.ptr())
            f, pl = flag(), plan()
            torch.cuda.synchronize()
            outs = [part, ysel, argsel] + ([Y] if Y is not None else [])
            assert all(o.guards_intact() for o in outs), "%s %s: a write outside an output" % (name, which)
            assert torch.isfinite(part.t).all() and torch.isfinite(ysel.t).all(), "%s %s: an output not written" % (name, which)
            assert int(argsel.t.max()) < S, "%s %s: an arg row outside its group (or not written)" % (name, which)
            rec[which] = (f, pl, part.t.cpu(), ysel.t.cpu(), argsel.t.cpu())
    finally:
        _lib.set_option(_lib.OPT_GEMM_SPLIT_BF16, prev)
    return rec


# ---- compacted pcops_mlp_gemm_fwd_pool_rows.  (name, S, G, K, N, seed)
ROWS_CASES = [("rows_128_256", 64, 1024, 128, 256, 21), ("rows_64_128", 64, 1024, 64, 128, 22)]


class RowSet:
    """G groups of S slots with the member counts of test_pool_top_rows_gpu.RowSet (1, 15, 16, 17, S - 1 and S among them),
    one count moved by 16 where needed so that the compacted row count is 16 mod 32: the last tile is ragged and its second
    block index is clamped to the last block"""

    def __init__(self, S, G, seed):
        g = torch.Generator().manual_seed(seed)
        cnt = torch.randint(1, S + 1, (G,), generator=g, dtype=torch.int32)
        for i, c in enumerate([1, 15, 16, 17, S - 1, S] * 3):
            cnt[(i * 37) % G] = c
        cnt[G - 1] = 1
        cnt[0] = S
        rows = lambda: int((16 * ((cnt.long() + 15) // 16)).sum())        # noqa: E731
        if rows() % 32 == 0:
            cnt[5] = cnt[5] + 16 if cnt[5] <= S - 16 else cnt[5] - 16
        assert rows() % 32 == 16
        self.S, self.G, self.R = S, G, G * S
        self.rows = _lib.Rows(cnt.view(8, G // 8).to(DEV), S)
        self.n = self.rows.num_rows()
        assert self.n == rows()
        self.nblk = self.n // 16
        w = self.rows.blocks[:self.nblk, 2].contiguous().view(torch.float32)
        assert (w > 1.0).any() and (w >= 1.0).all(), "block weights above 1 must be present"


def run_rows(case):
    """the storing call, then two calls with Y == NULL: (flag, plan, part, ypart, ppart) each"""
    name, S, G, K, N, seed = case
    lib = _lib.load()
    rs = RowSet(S, G, seed)
    R = rs.R
    assert lib.pcops_mlp_gemm_fwd_pool_rows_supported(R, K, N) == 1
    g = torch.Generator().manual_seed(seed + 1)
    X = torch.randn(R, K, generator=g).to(DEV)
    W, b, gamma, piv, sc, sh = _layer(K, N, seed=seed + 2)
    P = lib.pcops_mlp_stats_rows(R)
    nbk = rs.rows.blocks.shape[0]
    rec = {"rows": rs.n}
    for which in ("store", "nostore", "nostore2"):
        Y = Out((R, N)) if which == "store" else None
        part, ypart, ppart = Out((P, 2, N)), Out((nbk, N)), Out((nbk, N), torch.uint8)
        _lib.call("pcops_mlp_gemm_fwd_pool_rows", R, K, N, X.data_ptr(), K, sc.data_ptr(), sh.data_ptr(), W.data_ptr(),
                  b.data_ptr(), gamma.data_ptr(), Y.ptr() if Y is not None else None, part.ptr(), piv.data_ptr(), ypart.ptr(),
                  ppart.ptr(), rs.rows.ref)
        f, pl = flag(), plan()
        torch.cuda.synchronize()
        outs = [part, ypart, ppart] + ([Y] if Y is not None else [])
        assert all(o.guards_intact() for o in outs), "%s %s: a write outside an output" % (name, which)
        assert torch.isfinite(part.t).all() and torch.isfinite(ypart.t[:rs.nblk]).all(), "%s %s: an output not written" % (name, which)
        assert int(ppart.t[:rs.nblk].max()) < S
        rec[which] = (f, pl, part.t.cpu(), ypart.t.cpu(), ppart.t.cpu())
    return rec


def run_all():
    out = {}
    for c in POOL_CASES:
        out[c[0]] = run_pool(c)
    for c in ROWS_CASES:
        out[c[0]] = run_rows(c)
    return out


def main(argv):
    res = run_all()
    torch.save(res, argv[0])
    print("pool fwd acc stats child ok (PCOPS_POOL_FWD_ACC_STATS=%s)" % os.environ.get("PCOPS_POOL_FWD_ACC_STATS", "unset"))


if __name__ == "__main__":
    main(sys.argv[1:])
