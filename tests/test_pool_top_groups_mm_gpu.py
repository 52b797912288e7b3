"""pcops_mlp_dgrad_top_groups at N = 128 with the tile's addend as a product on the 16-bit matrix pipe
(dgrad_top_groups_mm_kernel, the default; PCOPS_POOL_TOP_GROUPS_MM=0 gives the addend walk back): against the float64
restatement of pool_top_groups_ref.py to the bound of test_pool_top_groups_gpu.py -- 2e-5 of the largest element of Gprev and
of each statistics row -- at the shapes and hand-made groups of the walk's worst and the product's edge cases; NaN-prefilled
outputs with rows to spare behind M; two calls the same bits; N = 256 and the option-off N = 128 against the walk in a child
process (the bits of the walk at N = 128 as recorded from the kernel this one stands beside:
tests/golden/pool_top_groups_walk_bits.json); an SA1-shaped stack at the planner's floor against the one-pass arm."""
import json
import os
import subprocess
import sys

import pytest
import torch

import pool_top_groups_mm_child as CH
import pool_top_groups_ref as PR
from scanobjectnn_amd import _lib, fused_mlp
from test_pool_top_groups_gpu import GROUPS, _inputs, _run, _sa1_stack

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 2e-5
KP, N = 64, 128
PIPE_SPLIT, PIPE_FP32 = 1, 0       # pcops_last_launch_pipe(): split bf16 operands (the product form) / fp32 (the walk)
SPARE = 64                       # rows allocated behind M, and one statistics row behind the last: they stay NaN
WALK_CASES = ["32,256,67,1", "64,256,35,2", "32,128,67,3", "64,128,35,4"]


def _dgrad(S, G, d, n=N):
    """one call on NaN-prefilled outputs with room to spare; -> Gprev [M], stats [P], what lies behind them, the pipe"""
    M = G * S
    P = _lib.load().pcops_mlp_stats_rows(M)
    Gprev = torch.full((M + SPARE, KP), float("nan"), dtype=torch.float32, device=DEV)
    part = torch.full((P + 1, 2, KP), float("nan"), dtype=torch.float32, device=DEV)
    _lib.call("pcops_mlp_dgrad_top_groups", M, KP, n, S, d["Yprev"].data_ptr(), d["psc"].data_ptr(), d["psh"].data_ptr(),
              d["Mq"].data_ptr(), d["v"].data_ptr(), d["gout"].data_ptr(), d["ysel"].data_ptr(), d["arg"].data_ptr(),
              d["sc"].data_ptr(), d["sh"].data_ptr(), d["p"].data_ptr(), d["Wt"].data_ptr(), Gprev.data_ptr(), part.data_ptr())
    pipe = int(_lib.load().pcops_last_launch_pipe())
    torch.cuda.synchronize()
    assert torch.isnan(Gprev[M:]).all() and torch.isnan(part[P:]).all(), "written past the end"
    return Gprev[:M], part[:P], pipe


def _reference(S, d):
    return PR.dgrad_top_groups(S, d["Yprev"], d["psc"], d["psh"], d["Mq"], d["v"], d["gout"], d["ysel"], d["arg"], d["sc"],
                               d["sh"], d["p"], d["Wt"])


def _check(S, G, d, want=None):
    """the product form against float64 (2e-5 of the largest element of Gprev, and of each statistics row), every element in
    range written, a second call the same bits; -> (Gprev, stats)"""
    Gprev, part, pipe = _dgrad(S, G, d)
    assert pipe == PIPE_SPLIT, "N = 128 did not take the product form (is PCOPS_POOL_TOP_GROUPS_MM set?)"
    want_g, terms = want if want is not None else _reference(S, d)
    assert torch.isfinite(Gprev).all() and torch.isfinite(part).all()
    scale = want_g.abs().max().item()
    err = (Gprev.double() - want_g).abs().max().item()
    print("Gprev              max err %.3e  largest element %.3e  ratio %.3e" % (err, scale, err / max(scale, 1e-300)))
    assert err <= REL * scale, ("Gprev", err, scale)
    sums = part.double().sum(0)
    for name, got_s, tm in (("stats sum dX", sums[0], terms[0]), ("stats sum dX Yprev", sums[1], terms[1])):
        want_s = tm.sum(0)
        err, scale = (got_s - want_s).abs().max().item(), want_s.abs().max().item()
        print("%-18s max err %.3e  largest element %.3e  ratio %.3e" % (name, err, scale, err / max(scale, 1e-300)))
        assert err <= REL * scale, (name, err, scale)
    Gprev2, part2, _ = _dgrad(S, G, d)
    assert torch.equal(Gprev, Gprev2) and torch.equal(part, part2)
    return Gprev, part


# 1 group: fewer tiles than workgroups; odd counts at S = 32: a half-filled last tile; 515: several tiles per workgroup
# through both register sets
@pytest.mark.parametrize("G", [1, 3, 67, 515])
@pytest.mark.parametrize("S", [32, 64])
def test_product_form_against_float64(S, G):
    d = _inputs(S, KP, N, G, seed=S + N + G)
    Gprev, _ = _check(S, G, d)
    assert not Gprev[0].any()                                      # (_inputs: X of row 0 is <= 0 everywhere)


def _live(d):
    """ysel with relu(bn(ysel)) > 0 on every channel: cf = p gout everywhere"""
    return 100.0 * torch.sign(d["sc"]).expand_as(d["ysel"]).contiguous()


@pytest.mark.parametrize("S", [32, 64])
def test_every_channel_on_one_row(S):
    """every group's 128 channels pick ONE row (row 7, the last row, row 0 in turn): the heaviest row, the walk's worst case"""
    G = 6
    d = _inputs(S, KP, N, G, seed=11 + S)
    d["ysel"] = _live(d)
    for g in range(G):
        d["arg"][g] = (7, S - 1, 0)[g % 3]
    _check(S, G, d)


def test_channels_spread_over_every_row():
    """S = 64: channel c picks row (c + 5 g) % 64 -- every row of a group is hit, by two channels each (128 channels cannot
    pick 128 different rows of 64), and a fragment's eight channels lie on eight different rows"""
    S, G = 64, 5
    d = _inputs(S, KP, N, G, seed=23)
    d["ysel"] = _live(d)
    for g in range(G):
        d["arg"][g] = ((torch.arange(N) + 5 * g) % S).to(torch.uint8).to(DEV)
    _check(S, G, d)


@pytest.mark.parametrize("S", [32, 64])
def test_argmax_past_the_group_and_dead_coefficients_leave_the_dense_part(S):
    """every argmax >= S (S, ..., 255), then every cf == 0 through ReLU-negative ysel: the addend is zero either way, the
    result is the dense part (float64 of it: gout = 0), and the two runs agree bit for bit"""
    G = 5
    d = _inputs(S, KP, N, G, seed=31 + S)
    dense = dict(d, gout=torch.zeros_like(d["gout"]))
    want = _reference(S, dense)
    past = dict(d, ysel=_live(d))
    past["arg"] = (S + (torch.arange(G * N).view(G, N) * 5) % (256 - S)).to(torch.uint8).to(DEV)
    assert past["arg"].min().item() >= S and past["arg"].max().item() == 255
    g_past, p_past = _check(S, G, past, want)
    dead = dict(d, ysel=-_live(d))
    g_dead, p_dead = _check(S, G, dead, want)
    assert torch.equal(g_past, g_dead) and torch.equal(p_past, p_dead)


@pytest.mark.parametrize("S", [32, 64])
def test_coefficients_over_nine_decades_in_one_group(S):
    """cf from 1e-6 to 1e3 in magnitude, both signs, in each group (the small pieces of the split matter next to the large
    terms of the same row): the same 2e-5 of the largest element"""
    G = 4
    d = _inputs(S, KP, N, G, seed=41 + S)
    d["ysel"] = _live(d)
    g = torch.Generator().manual_seed(5)
    for gi in range(G):
        mag = torch.logspace(-6, 3, N)[torch.randperm(N, generator=g)]
        sign = 1.0 - 2.0 * torch.randint(0, 2, (N,), generator=g)
        d["gout"][gi] = (mag * sign).to(DEV) / d["p"]
    d["arg"][1] = 3                                                # ... and all nine decades on one row
    _check(S, G, d)


def _child(tmp_path, env, cases):
    out = str(tmp_path / "walk.pt")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pool_top_groups_mm_child.py"), out] + cases, cwd=ROOT,
                         env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-1500:] + run.stderr[-2500:]
    assert "pool top groups child ok" in run.stdout
    return torch.load(out)


def test_wider_layers_and_the_option_keep_the_walk(tmp_path):
    """a child process with PCOPS_POOL_TOP_GROUPS_MM=0 runs the walk at N = 256 and N = 128, S = 32 and 64.  N = 256 here
    (option at its default) gives the child's bits; the child's N = 128 bits are the recorded bits of the walk; and N = 128
    here takes the product form (its difference from the walk is printed; both are held to float64 above)."""
    walk = _child(tmp_path, {"PCOPS_POOL_TOP_GROUPS_MM": "0"}, WALK_CASES)
    with open(os.path.join(ROOT, "tests", "golden", "pool_top_groups_walk_bits.json")) as f:
        recorded = json.load(f)
    for case in WALK_CASES:
        S, n, G, seed = (int(v) for v in case.split(","))
        w_g, w_p, w_pipe = walk[case]
        assert w_pipe == PIPE_FP32, case
        Gprev, part, pipe = _dgrad(S, G, _inputs(S, KP, n, G, seed), n)
        if n == 256:
            assert pipe == PIPE_FP32, case
            assert torch.equal(Gprev.cpu(), w_g) and torch.equal(part.cpu(), w_p), case
        else:
            assert pipe == PIPE_SPLIT, case
            assert recorded[case] == {"Gprev": CH.digest(w_g), "stats": CH.digest(w_p)}, case
            print("%s product form against the walk: max diff %.3e of %.3e" % (case, (Gprev.cpu() - w_g).abs().max().item(),
                                                                                w_g.abs().max().item()))


def test_sa1_stack_on_the_product_form_equals_the_one_pass_form(monkeypatch):
    """gather_mlp_stack on the SA1-shaped stack of test_pool_top_groups_gpu.py at the planner's floor (262 144 rows): the
    *_groups arm, whose data gradient is the product form here, against the one-pass arm: same forward bits, every gradient
    within 2e-4 * scale + 1e-6"""
    st = _sa1_stack()
    assert st["R"] == 262144
    res, pipes = {}, []
    hook = lambda name, phase, args: (name == "pcops_mlp_dgrad_top_groups" and phase == "post" and       # noqa: E731
                                      pipes.append(int(_lib.load().pcops_last_launch_pipe())))
    _lib._hooks.append(hook)
    try:
        for mode in (True, False):
            monkeypatch.setattr(fused_mlp, "POOL_TOP_GROUPS", mode)
            rec = []
            res[mode] = _run(st, rec)
            called = [n for n, _ in rec]
            assert all(called.count(n) == (1 if mode else 0) for n in GROUPS), called
    finally:
        _lib._hooks.remove(hook)
    assert pipes == [PIPE_SPLIT]
    assert torch.equal(res[True][0], res[False][0])
    go_scale = st["go"].abs().max().item()
    for name, a, b in zip(res[True][1], res[True][2], res[False][2]):
        scale = go_scale if name.endswith(".db") or name == "dbias" else b.abs().max().item()
        err = (a - b).abs().max().item()
        print("%-10s max diff %.3e  scale %.3e" % (name, err, scale))
        assert err <= 2e-4 * scale + 1e-6, (name, err, scale)
