"""The pooled forward that stores no Y takes its statistics from the accumulator registers (gemm_ws_kernel VAR 5 | 16,
DESIGN.md section 4.31): same kernel walk, same arithmetic, the transposed epilogue's summation order -- so every output is
bit for bit the storing call's, which still runs the transposing kernel.

* uncompacted pcops_mlp_gemm_fwd_pool, storing call against Y == NULL in one process: all pcops_mlp_stats_rows(M)
  statistics rows, ysel and argsel equal; NaN-prefilled outputs between guard bands; every third gamma negative; with and
  without stat_pivot; pcops_last_launch_acc_stats() 0 after the storing call and 1 after the other; the plan tuple
  (2, 1, 128, 0, 1) for both.  Shapes: the flagship's tile, a group of two tiles, two column blocks and two K chunks, a padded
  K step with a ragged column block and fewer tile owners than statistics rows.
* compacted pcops_mlp_gemm_fwd_pool_rows: block weights above 1, a row count that is 16 mod 32 (ragged last tile, last block
  shared by clamp), (K, N) = (128, 256) and (64, 128): statistics, ypart, ppart equal; two Y == NULL calls the same bits.
* N = 64, N = 96, K = 320 (streamed weights), S = 20, pro_scale == NULL and PCOPS_OPT_GEMM_SPLIT_BF16 = 0 keep their
  kernels: the flag stays 0 and Y == NULL still gives the storing call's bits.
* a child process with PCOPS_POOL_FWD_ACC_STATS=0: the flag is 0 everywhere and every output of every case above is bit-equal
  to this process's."""
import os
import subprocess
import sys

import pytest
import torch

import pool_fwd_acc_stats_child as CH

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b):
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


_cache = {}


def _record(case, run):
    if case[0] not in _cache:
        _cache[case[0]] = run(case)
    return _cache[case[0]]


NEW = [c for c in CH.POOL_CASES if c[-1]]
KEEP = [c for c in CH.POOL_CASES if not c[-1]]


@pytest.mark.parametrize("case", NEW, ids=[c[0] for c in NEW])
def test_uncompacted_without_the_store_equals_the_storing_call(case):
    rec = _record(case, CH.run_pool)
    (f0, p0, *out0), (f1, p1, *out1) = rec["store"], rec["nostore"]
    assert (f0, f1) == (0, 1), "the storing call keeps the transposing kernel, the other takes the new variant"
    assert p0 == CH.NEW_PLAN and p1 == CH.NEW_PLAN
    for name, a, b in zip(("stats rows", "ysel", "argsel"), out0, out1):
        assert same_bits(a, b), "%s: %s differs in %d places" % (case[0], name, int((a != b).sum()))


@pytest.mark.parametrize("case", CH.ROWS_CASES, ids=[c[0] for c in CH.ROWS_CASES])
def test_compacted_without_the_store_equals_the_storing_call(case):
    rec = _record(case, CH.run_rows)
    assert rec["rows"] % 32 == 16
    flags = [rec[k][0] for k in ("store", "nostore", "nostore2")]
    assert flags == [0, 1, 1]
    assert rec["store"][1] == rec["nostore"][1] and rec["store"][1][:4] == CH.NEW_PLAN[:4]
    for other in ("nostore", "nostore2"):
        for name, a, b in zip(("stats rows", "ypart", "ppart"), rec["store"][2:], rec[other][2:]):
            assert same_bits(a, b), "%s %s: %s differs in %d places" % (case[0], other, name, int((a != b).sum()))


@pytest.mark.parametrize("case", KEEP, ids=[c[0] for c in KEEP])
def test_every_other_plan_keeps_its_kernel(case):
    rec = _record(case, CH.run_pool)
    assert rec["store"][0] == 0 and rec["nostore"][0] == 0
    pl = rec["store"][1]
    print(case[0], "plan", pl)
    assert pl == rec["nostore"][1] and pl[0] == 2
    # the case is what its name says: (field of the plan tuple, value) -- the plain operand shares the tuple and differs
    # in the kernel's operand mode alone
    field, value = {"keeps_n64": (2, 64), "keeps_n96": (2, 96), "keeps_k320_streamed": (3, 1), "keeps_s20": (4, 3),
                    "keeps_plain_operand": (2, 128), "keeps_fp32_pipe": (1, 0)}[case[0]]
    assert pl[field] == value, (case[0], pl)
    for name, a, b in zip(("stats rows", "ysel", "argsel"), rec["store"][2:], rec["nostore"][2:]):
        assert same_bits(a, b), "%s: %s differs" % (case[0], name)


def test_switched_off_in_a_child_process_gives_the_same_bits(tmp_path):
    out = str(tmp_path / "off.pt")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pool_fwd_acc_stats_child.py"), out], cwd=ROOT,
                         env=dict(os.environ, PCOPS_POOL_FWD_ACC_STATS="0"), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-1500:] + run.stderr[-2500:]
    assert "pool fwd acc stats child ok (PCOPS_POOL_FWD_ACC_STATS=0)" in run.stdout
    off = torch.load(out)
    for case in CH.POOL_CASES:
        here = _record(case, CH.run_pool)
        for which in ("store", "nostore"):
            assert off[case[0]][which][0] == 0, "%s %s: the new variant ran in the child" % (case[0], which)
            assert off[case[0]][which][1] == here[which][1]
            for a, b in zip(off[case[0]][which][2:], here[which][2:]):
                assert same_bits(a, b), (case[0], which)
    for case in CH.ROWS_CASES:
        here = _record(case, CH.run_rows)
        assert off[case[0]]["rows"] == here["rows"]
        for which in ("store", "nostore", "nostore2"):
            assert off[case[0]][which][0] == 0 and off[case[0]][which][1] == here[which][1]
            for a, b in zip(off[case[0]][which][2:], here[which][2:]):
                assert same_bits(a, b), (case[0], which)
