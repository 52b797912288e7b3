"""pcops_mlp_bwd_tiles_rows (csrc/bwd_tiles128.hip): the one-pass backward of a 128 -> 128 layer on the all-wave tile kernel, called
through the C ABI and held to the float64 restatement of tests/bwd_tiles_ref.py: every output -- dW, db, Gprev, the two summed
statistics rows -- within 2e-5 of the largest element of its reference (the bound of tests/test_xyz_bwd_tiles_gpu.py).  The mask
inputs are exact in fp32 (bwd_tiles_ref.make_inputs), so no ReLU decision may differ from the reference's.  Uncompacted rows
around the tile edges and a compacted set whose device row count is below the allocated one; NaN-prefilled outputs between guard
bands, two calls the same bits, the plan tuple; the error of the two-kernel path (pcops_mlp_gemm_dgrad_rows +
pcops_mlp_wgrad_rows) on the same inputs is printed beside the new kernel's.  Then the stack: the planner's arm at 524 288 rows
against the split arm, and a child process with PCOPS_BWD_TILES128=0."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import bwd_tiles_ref as BR
from edge_checks import Out, bits_equal
from scanobjectnn_amd import _lib, fused_mlp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 2e-5
EPS = 1e-3
K = BR.K
CASES = ["u,64,1,random", "u,100,2,random", "u,8192,3,random", "u,8200,4,random", "u,8200,5,masks_off", "u,8200,6,masks_on",
         "u,8200,7,pq_zero", "u,8200,8,decades", "c,12800,9,random", "c,12800,10,masks_off", "c,12800,11,masks_on",
         "c,12800,12,pq_zero", "c,12800,13,decades"]
NAMES = ("dW", "db", "Gprev", "gp", "gpy")


def _plan():
    out = (ctypes.c_int * 5)()
    assert _lib.load().pcops_last_launch_plan(out, 5) == 5
    return tuple(out)


@pytest.fixture(scope="module")
def rowset():
    """200 groups of 64 slots (12 800 allocated rows): group 0 has 5 members (ONE block, weight 49), 114 groups 40 members
    (three blocks, weight 17), 85 groups 20 members (two blocks, weight 33) -- 513 blocks, 8 208 rows = 16 mod 64"""
    cnt = torch.tensor([5] + [40] * 114 + [20] * 85, dtype=torch.int32, device=DEV).view(1, 200)
    rows = _lib.Rows(cnt, 64)
    n = rows.num_rows()
    assert n == 8208 and n % 64 == 16 and n < rows.full_rows == 12800
    w = BR.block_row_weights(rows.blocks, rows.full_rows)
    bs = rows.block_start.cpu()
    assert bs[1] - bs[0] == 1                                        # the single-block group
    assert w[0] == 49 and w[16] == 17 and w[32] == 1 and (w[:n] > 1).sum() == 200
    assert all(w[16 * int(b)] > 1 for b in bs[:-1])                  # the weights above 1 sit on group-first rows
    return rows, w, n


def _inputs(case):
    _, M, seed, kind = case.split(",")
    return {k: v.to(DEV) for k, v in BR.make_inputs(int(M), int(seed), kind).items()}


def _call(d, M, rows=None, n=None):
    """one call on NaN-prefilled outputs between guard bands; n: the rows that exist (the device row count)"""
    lib = _lib.load()
    n = M if n is None else n
    groups = int(lib.pcops_mlp_bwd_tiles_groups(M, K, K))
    assert groups == min(256, (M + 31) // 32)
    o = {"partial": Out((groups * (K * K + K),), device=DEV), "dW": Out((K, K), device=DEV), "db": Out((K,), device=DEV),
         "Gprev": Out((M, K), device=DEV), "st": Out((groups, 2, K), device=DEV)}
    _lib.call("pcops_mlp_bwd_tiles_rows", M, K, K, d["Yprev"].data_ptr(), d["asc"].data_ptr(), d["ash"].data_ptr(),
              d["G"].data_ptr(), d["Y"].data_ptr(), d["p"].data_ptr(), d["q"].data_ptr(), d["t"].data_ptr(), d["W"].data_ptr(),
              o["partial"].ptr(), o["dW"].ptr(), o["db"].ptr(), o["Gprev"].ptr(), o["st"].ptr(), rows)
    plan, pipe = _plan(), int(lib.pcops_last_launch_pipe())
    torch.cuda.synchronize()
    for name, buf in o.items():
        assert buf.guards_intact(), "%s: written outside the buffer" % name
    for name in ("partial", "dW", "db", "st"):
        assert torch.isfinite(o[name].t).all(), "%s: an element was not written (or is not finite)" % name
    assert torch.isfinite(o["Gprev"].t[:n]).all(), "Gprev: a row was not written (or is not finite)"
    assert torch.isnan(o["Gprev"].t[n:]).all(), "Gprev: a row behind the row count was written"
    r = {name: o[name].t.clone() for name in ("dW", "db", "st")}
    r["Gprev"] = o["Gprev"].t[:n].clone()
    r["plan"], r["pipe"] = plan, pipe
    return r


def _two_kernels(d, M, rows=None, n=None):
    """the same layer through pcops_mlp_gemm_dgrad_rows and pcops_mlp_wgrad_rows"""
    lib = _lib.load()
    n = M if n is None else n
    f = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=DEV)      # noqa: E731
    Wt, Gprev, dW, db = f(K, K), f(M, K), f(K, K), f(K)
    P = int(lib.pcops_mlp_stats_rows(M))
    st = f(P, 2, K)
    scratch = f(int(lib.pcops_mlp_wgrad_splits(M, K, K)) * (K * K + K))
    _lib.call("pcops_mlp_transpose", K, K, d["W"].data_ptr(), Wt.data_ptr())
    _lib.call("pcops_mlp_gemm_dgrad_rows", M, K, K, d["G"].data_ptr(), d["Y"].data_ptr(), d["p"].data_ptr(), d["q"].data_ptr(),
              d["t"].data_ptr(), None, None, 1, None, None, Wt.data_ptr(), d["Yprev"].data_ptr(), d["asc"].data_ptr(),
              d["ash"].data_ptr(), Gprev.data_ptr(), st.data_ptr(), rows)
    _lib.call("pcops_mlp_wgrad_rows", M, K, K, d["Yprev"].data_ptr(), K, d["asc"].data_ptr(), d["ash"].data_ptr(),
              d["G"].data_ptr(), d["Y"].data_ptr(), d["p"].data_ptr(), d["q"].data_ptr(), d["t"].data_ptr(), None, None, 1, None,
              None, scratch.data_ptr(), dW.data_ptr(), db.data_ptr(), rows)
    torch.cuda.synchronize()
    return {"dW": dW, "db": db, "st": st, "Gprev": Gprev[:n].clone()}


def _errors(r, ref):
    """-> {what: (max error, largest element of the reference)}"""
    got = {"dW": r["dW"].double(), "db": r["db"].double(), "Gprev": r["Gprev"].double(), "gp": r["st"].double().sum(0)[0],
           "gpy": r["st"].double().sum(0)[1]}
    return {k: ((got[k] - ref[k]).abs().max().item(), ref[k].abs().max().item()) for k in NAMES}


def _hold(errs, what):
    for k, (err, scale) in errs.items():
        assert err <= REL * scale, "%s %s: max error %.3e, largest element %.3e (bound %.1e of it)" % (what, k, err, scale, REL)


@pytest.mark.parametrize("case", CASES)
def test_tile_kernel_against_float64(case, rowset):
    form, M, _, kind = case.split(",")
    M = int(M)
    d = _inputs(case)
    rows, w, n = (rowset[0].ref, rowset[1].to(DEV), rowset[2]) if form == "c" else (None, None, M)
    ref = BR.reference(d, w, n)
    r = _call(d, M, rows, n)
    assert r["plan"] == (18, 2, 128, 0, 4 if form == "c" else 0) and r["pipe"] == 1, (r["plan"], r["pipe"])
    e_new, e_two = _errors(r, ref), _errors(_two_kernels(d, M, rows, n), ref)
    for k in NAMES:
        scale = max(e_new[k][1], 1e-300)
        print("%-22s %-6s largest %.3e   err/largest: tiles %.3e   two kernels %.3e" % (
            case, k, e_new[k][1], e_new[k][0] / scale, e_two[k][0] / scale))
    _hold(e_new, case)
    if kind == "masks_off":
        assert not r["dW"].any() and not r["Gprev"].any() and not r["st"].any(), "a closed mask let something through"
        assert r["db"].abs().min().item() > 0
    again = _call(d, M, rows, n)
    for name in ("dW", "db", "st", "Gprev"):
        assert bits_equal(r[name], again[name]), "%s: two calls, different bits" % name


def test_query_and_refusals():
    lib = _lib.load()
    q = lib.pcops_mlp_bwd_tiles_groups
    assert q(64, 128, 128) == 2 and q(63, 128, 128) == 0 and q(2097152, 128, 128) == 256
    assert q(1 << 22, 128, 128) == 0                                  # M * 512 bytes = 2^31
    assert q((1 << 22) - 1, 128, 128) == 256
    assert q(65536, 64, 128) == 0 and q(65536, 128, 64) == 0 and q(65536, 128, 256) == 0
    d = _inputs("u,64,1,random")
    o = torch.zeros(64 * K + 2 * (K * K + K) + 4, device=DEV)
    args = lambda G: (64, K, K, d["Yprev"].data_ptr(), d["asc"].data_ptr(), d["ash"].data_ptr(), G, d["Y"].data_ptr(),   # noqa: E731
                      d["p"].data_ptr(), d["q"].data_ptr(), d["t"].data_ptr(), d["W"].data_ptr(), o.data_ptr(), o.data_ptr(),
                      o.data_ptr(), o.data_ptr(), o.data_ptr(), None, None)
    assert lib.pcops_mlp_bwd_tiles_rows(*args(d["G"].data_ptr() + 4)) == -4       # a misaligned operand
    assert lib.pcops_mlp_bwd_tiles_rows(*args(None)) == -1
    torch.cuda.synchronize()
    assert not o.any()


# ------------------------------------------------------------------------------------------------ the stack
def sa2_stack(B=64, seed=0):
    """an SA2-shaped stack: B clouds x 128 groups x 64 slots over 512 points with 128 features, widths 128-128-256, ball-query
    padding compacted (64 clouds: 524 288 allocated rows, the planner's floor for the tile arm)"""
    from scanobjectnn_amd.pointnet2 import tf_grouping, tf_sampling
    from scanobjectnn_amd.synth import synth_clouds
    from test_fused_mlp_gpu import make_layers
    M, S, widths = 128, 64, [128, 128, 256]
    g = torch.Generator().manual_seed(seed)
    xyz = torch.from_numpy(synth_clouds(B, 512, seed=seed + 3)).to(DEV)
    new_xyz = tf_sampling.gather_point(xyz, tf_sampling.farthest_point_sample(M, xyz))
    idx, cnt = tf_grouping.query_ball_point(0.4, S, xyz, new_xyz)
    Q = torch.randn(B, 512, widths[0], generator=g).to(DEV)
    wxyz = torch.randn(3, widths[0], generator=g).to(DEV)
    go = torch.randn(B * M, widths[-1], generator=g).to(DEV)
    return dict(idx=idx, cnt=cnt, xyz=xyz, new_xyz=new_xyz, Q=Q, wxyz=wxyz, layers=make_layers(widths[0], widths, seed=seed + 1),
                go=go, R=B * M * S)


def run_stack(st):
    """-> (output, names, gradients, names of the launches), in deterministic mode"""
    Q, wxyz = st["Q"].clone().requires_grad_(True), st["wxyz"].clone().requires_grad_(True)
    ls = [[t.clone().requires_grad_(True) for t in l[:4]] + [l[4].clone(), l[5].clone()] for l in st["layers"]]
    rec = []
    hook = lambda name, phase, args: rec.append(name) if phase == "pre" else None     # noqa: E731
    _lib._hooks.append(hook)
    was = _lib.deterministic()
    _lib.set_deterministic(True)        # the first layer's scatter-add in a fixed order: two runs of one arm give the same bits
    try:
        out = fused_mlp.gather_mlp_stack(st["idx"], True, True, 0.9, EPS, True, [tuple(l) for l in ls], Q=Q, xyz=st["xyz"],
                                         new_xyz=st["new_xyz"], wxyz=wxyz, pts_cnt=st["cnt"])
        out.backward(st["go"])
        torch.cuda.synchronize()
    finally:
        _lib.set_deterministic(was)
        _lib._hooks.remove(hook)
    named = [("dQ", Q.grad), ("dwxyz", wxyz.grad)]
    named += [("L%d.%s" % (li, n), t.grad) for li, l in enumerate(ls) for ti, (n, t) in
              enumerate(zip(("dW", "db", "dgamma", "dbeta"), l[:4])) if not (li == 0 and ti < 2)]
    return out.detach().clone(), [n for n, _ in named], [t.clone() for _, t in named], rec


TWO = ("pcops_mlp_wgrad_rows", "pcops_mlp_gemm_dgrad_rows")


@pytest.fixture(scope="module")
def stack_runs():
    """the stack on the tile arm (the default) and on the split arm (the planner's floor out of reach)"""
    st = sa2_stack()
    assert st["R"] == 524288 == fused_mlp.TILES_MIN_ROWS
    tiles = run_stack(st)
    floor = fused_mlp.TILES_MIN_ROWS
    fused_mlp.TILES_MIN_ROWS = 1 << 62
    try:
        split = run_stack(st)
    finally:
        fused_mlp.TILES_MIN_ROWS = floor
    return st, tiles, split


def test_stack_takes_the_tile_arm_and_equals_the_split_arm(stack_runs):
    """same forward bits, every gradient within 2e-4 * scale + 1e-6 (the bound of the stack comparisons in
    tests/test_pool_top_groups_gpu.py), the new entry point once on the call hook in place of the middle layer's two"""
    st, tiles, split = stack_runs
    assert tiles[3].count("pcops_mlp_bwd_tiles_rows") == 1 and "pcops_mlp_bwd_tiles_rows" not in split[3]
    for n in TWO:
        assert split[3].count(n) == tiles[3].count(n) + 1, (n, tiles[3], split[3])
    assert torch.equal(tiles[0], split[0])
    go_scale = st["go"].abs().max().item()
    for name, a, b in zip(tiles[1], tiles[2], split[2]):
        # the gradient of a bias in front of a batch norm is zero in exact arithmetic: rounding noise on both sides, judged on
        # the scale of the upstream gradient
        scale = go_scale if name.endswith(".db") else b.abs().max().item()
        err = (a - b).abs().max().item()
        print("%-10s max diff %.3e  scale %.3e" % (name, err, scale))
        assert err <= 2e-4 * scale + 1e-6, (name, err, scale)


def test_switched_off_the_query_is_zero_and_the_stack_is_the_split_arm(stack_runs, tmp_path):
    """a child process with PCOPS_BWD_TILES128=0 (the switch is read once per process): the query answers 0, the stack takes the
    split arm and gives the bits the split arm gives here"""
    _, _, split = stack_runs
    out = str(tmp_path / "off.pt")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bwd_tiles128_child.py"), out], cwd=ROOT,
                         env=dict(os.environ, PCOPS_BWD_TILES128="0"), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-1500:] + run.stderr[-2500:]
    assert "bwd tiles128 child ok (PCOPS_BWD_TILES128=0)" in run.stdout
    off = torch.load(out)
    assert off["query"] == 0 and "pcops_mlp_bwd_tiles_rows" not in off["launches"]
    assert off["launches"] == split[3]
    assert bits_equal(off["out"], split[0].cpu())
    for name, a, b in zip(split[1], off["grads"], split[2]):
        assert bits_equal(a, b.cpu()), "%s: the switched-off stack is not the split arm bit for bit" % name
