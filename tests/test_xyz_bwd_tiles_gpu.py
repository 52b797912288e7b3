"""pcops_mlp_bwd_fused_xyz_rows at K = N = 64, uncompacted rows, dense G: the all-wave tile kernel of csrc/xyz_bwd_tiles.hip
(the default; PCOPS_BWD_XYZ_TILES=0 gives bwd_fused_kernel back), called through the C ABI and held to the float64 restatement
of tests/xyz_bwd_ref.py: 2e-5 of the largest element of dW, of db, and of each summed statistics row (the bar of
tests/test_pool_top_groups*_gpu.py).  The mask inputs are exact in fp32 (tests/test_xyz_bwd_ref_cpu.py), so no ReLU decision
may differ from the reference's.  Row counts around a tile edge, hand-made sets, NaN-prefilled outputs with guard bands, two
calls the same bits, the plan tuple; the 64 -> 128 form, compacted rows and the switched-off child process keep the old kernel,
whose error on the same inputs is printed beside the new kernel's."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import xyz_bwd_ref as XR
from edge_checks import Out, bits_equal
from scanobjectnn_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 2e-5
K = XR.K
PLAN_TILES = (17, 2, 64, 0, 0)       # pcops_last_launch_plan(): the tile kernel, both halves on split operands
PLAN_OLD = (3, 1, 64, 0, 0)          # bwd_fused_kernel: split dX half, fp32 dW half
CASES = ["65536,1,random", "65537,2,random", "65599,3,random", "65601,4,random",
         "65536,5,masks_off", "65536,6,masks_on", "65536,7,t_only", "65536,8,zero_rows", "65536,9,decades"]


def _device_inputs(M, N, seed, kind="random"):
    return {k: v.to(DEV) for k, v in XR.make_inputs(M, N, seed, kind).items()}


def _plan():
    out = (ctypes.c_int * 5)()
    assert _lib.load().pcops_last_launch_plan(out, 5) == 5
    return tuple(out)


def _call(d, M, N, rows=None):
    """one call on NaN-prefilled outputs between guard bands; the buffers are sized as the caller sizes them"""
    lib = _lib.load()
    groups = int(lib.pcops_mlp_bwd_fused_groups(M, K, N, 0, 0))
    assert groups == 256
    o = {"partial": Out((groups * (K * N + N),), device=DEV), "dW": Out((K, N), device=DEV), "db": Out((N,), device=DEV),
         "st": Out((groups, 2, K), device=DEV), "xs": Out((groups, 3, K), device=DEV)}
    _lib.call("pcops_mlp_bwd_fused_xyz_rows", M, K, N, d["off4"].data_ptr(), d["xyzw"].data_ptr(), d["asc"].data_ptr(),
              d["ash"].data_ptr(), d["G"].data_ptr(), d["Y"].data_ptr(), d["p"].data_ptr(), d["q"].data_ptr(), d["t"].data_ptr(),
              None, None, 1, d["W"].data_ptr(), o["partial"].ptr(), o["dW"].ptr(), o["db"].ptr(), o["st"].ptr(), o["xs"].ptr(),
              rows)
    plan, pipe = _plan(), int(lib.pcops_last_launch_pipe())
    torch.cuda.synchronize()
    for name, buf in o.items():
        assert buf.guards_intact(), "%s: written outside the buffer" % name
    for name in ("dW", "db", "st", "xs"):
        assert torch.isfinite(o[name].t).all(), "%s: a row was not written (or is not finite)" % name
    r = {name: buf.t.clone() for name, buf in o.items() if name != "partial"}
    r["plan"], r["pipe"] = plan, pipe
    return r


def _errors(r, ref):
    """-> {what: (max error, largest element of the reference)} of dW, db and the five summed statistics rows"""
    got = {"dW": r["dW"].double(), "db": r["db"].double(), "gp": r["st"].double().sum(0)[0], "gpy": r["st"].double().sum(0)[1]}
    want = {k: ref[k].to(got["dW"].device) for k in ("dW", "db", "gp", "gpy")}
    for i, name in enumerate(("off_x", "off_y", "off_z")):
        got[name] = r["xs"].double().sum(0)[i]
        want[name] = ref["off"][i].to(got["dW"].device)
    return {k: ((got[k] - want[k]).abs().max().item(), want[k].abs().max().item()) for k in got}


def _hold(errs, what):
    for k, (err, scale) in errs.items():
        assert err <= REL * scale, "%s %s: max error %.3e, largest element %.3e (bound %.1e of it)" % (what, k, err, scale, REL)


@pytest.fixture(scope="module")
def old(tmp_path_factory):
    """every case on bwd_fused_kernel: a child process with PCOPS_BWD_XYZ_TILES=0 (the child only sets that variable)"""
    out = str(tmp_path_factory.mktemp("xyz_bwd") / "old.pt")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "xyz_bwd_tiles_child.py"), out] + CASES, cwd=ROOT,
                         env=dict(os.environ, PCOPS_BWD_XYZ_TILES="0"), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-1500:] + run.stderr[-2500:]
    assert "xyz bwd tiles child ok (PCOPS_BWD_XYZ_TILES=0)" in run.stdout
    return torch.load(out)


@pytest.mark.parametrize("case", CASES)
def test_tile_kernel_against_float64(case, old):
    M, seed, kind = case.split(",")
    M, seed = int(M), int(seed)
    d = _device_inputs(M, 64, seed, kind)
    ref = XR.reference(d)
    r = _call(d, M, 64)
    assert r["plan"] == PLAN_TILES and r["pipe"] == 1, "the call did not take the tile kernel (is PCOPS_BWD_XYZ_TILES set?)"
    o_dW, o_db, o_st, o_xs, o_plan, o_pipe = old[case]
    assert tuple(o_plan) == PLAN_OLD and o_pipe == 2, "the child did not take bwd_fused_kernel"
    e_new = _errors(r, ref)
    e_old = _errors({"dW": o_dW, "db": o_db, "st": o_st, "xs": o_xs}, {k: v.cpu() for k, v in ref.items()})
    for k in e_new:
        scale = max(e_new[k][1], 1e-300)
        print("%-22s %-6s largest %.3e   err/largest: tiles %.3e   bwd_fused_kernel %.3e" % (
            case, k, e_new[k][1], e_new[k][0] / scale, e_old[k][0] / scale))
    _hold(e_new, case)
    _hold(e_old, case + " (PCOPS_BWD_XYZ_TILES=0)")
    if kind == "masks_off":
        assert not r["dW"].any() and not r["st"].any() and not r["xs"].any(), "a closed mask let something through"
        assert r["db"].abs().min().item() > 0
    # the two kernels against each other: at most the bound
    _hold(_errors(r, {"dW": o_dW.double(), "db": o_db.double(), "gp": o_st.double().sum(0)[0], "gpy": o_st.double().sum(0)[1],
                      "off": o_xs.double().sum(0)}), case + " against the child")
    again = _call(d, M, 64)
    for name in ("dW", "db", "st", "xs"):
        assert bits_equal(r[name], again[name]), "%s: two calls, different bits" % name


def test_wider_layer_keeps_the_old_kernel():
    M = 65536
    d = _device_inputs(M, 128, 31)
    r = _call(d, M, 128)
    assert r["plan"][0] == 3 and r["plan"][2] == 128, r["plan"]
    _hold(_errors(r, XR.reference(d)), "64 -> 128")


def test_compacted_rows_keep_the_old_kernel():
    """a row set whose groups are all full compacts to itself (every weight 1): the restatement holds as it stands"""
    S, G = 32, 2048
    M = S * G
    d = _device_inputs(M, 64, 32)
    rows = _lib.Rows(torch.full((1, G), S, dtype=torch.int32, device=DEV), S)
    assert rows.num_rows() == M
    r = _call(d, M, 64, rows.ref)
    assert r["plan"][0] == 3 and r["plan"][4] == 4, r["plan"]
    _hold(_errors(r, XR.reference(d)), "compacted rows")
