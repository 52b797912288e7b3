"""The float64 restatement of pcops_mlp_bwd_tiles_rows (tests/bwd_tiles_ref.py) held to float64 autograd of the layer at 1e-10,
two wrong restatements of the block weights rejected, and the planner's choice of the arm at its row floor and below it with
the launches stubbed (tests/stack_trace.py)."""
import torch

import bwd_tiles_ref as BR
import stack_trace as ST
from scanobjectnn_amd import fused_mlp

TOL = 1e-10


def _weights(M, seed):
    """weights above 1 on some rows that open a 16-row block, as a compacted row set has them"""
    g = torch.Generator().manual_seed(seed)
    w = torch.ones(M)
    first = torch.arange(0, M, 16)
    pick = first[torch.rand(first.numel(), generator=g) < 0.5]
    w[pick] = torch.randint(2, 50, (pick.numel(),), generator=g).float()
    return w


def _rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)


def _autograd(d, w, rows):
    """the layer's gradients by float64 autograd, the upstream dY built independently of the restatement: row by row"""
    n = d["Yprev"].shape[0] if rows is None else rows
    D = torch.float64
    dY = torch.empty(n, BR.K, dtype=D)
    for r in range(n):
        dense = d["q"].to(D) * d["Y"][r].to(D) + d["t"].to(D)
        dY[r] = d["p"].to(D) * d["G"][r].to(D) + (1.0 if w is None else float(w[r])) * dense
    dW, dX = BR.layer_autograd(d["Yprev"][:n], d["asc"], d["ash"], dY, d["W"])
    # the gradient with respect to Yprev is a_scale . Gprev: the masked data gradient in front of the batch norm's scale
    return dY, dW, dX


def _check(d, w, rows):
    ref = BR.reference(d, w, rows)
    dY, dW, dX = _autograd(d, w, rows)
    n = dY.shape[0]
    asc = d["asc"].double()
    assert ref["Gprev"].shape == (n, BR.K)
    assert _rel(ref["dW"], dW) <= TOL
    assert _rel(ref["db"], dY.sum(0)) <= TOL
    assert _rel(ref["Gprev"] * asc, dX) <= TOL
    nz = asc != 0
    assert _rel((ref["gp"] * asc)[nz], dX.sum(0)[nz]) <= TOL
    assert _rel((ref["gpy"] * asc)[nz], (dX * d["Yprev"][:n].double()).sum(0)[nz]) <= TOL
    return ref


def test_restatement_equals_float64_autograd():
    for M, seed, kind in [(64, 1, "random"), (100, 2, "random"), (208, 3, "decades"), (96, 4, "pq_zero")]:
        _check(BR.make_inputs(M, seed, kind), None, None)


def test_restatement_with_block_weights_equals_float64_autograd():
    d = BR.make_inputs(272, 5)
    w = _weights(272, 6)
    assert (w > 1).sum() >= 3
    _check(d, w, None)
    _check(d, w, 208)          # a device row count below the allocated one: the rows behind it do not exist
    d["G"][208:] = float("nan")
    ref = _check(d, w, 208)
    assert all(torch.isfinite(v).all() for v in ref.values())


def test_masks_off_and_on():
    d = BR.make_inputs(96, 7, "masks_off")
    ref = BR.reference(d)
    assert not ref["dW"].any() and not ref["Gprev"].any() and not ref["gp"].any() and not ref["gpy"].any()
    assert ref["db"].abs().min().item() > 0
    d = BR.make_inputs(96, 8, "masks_on")
    ref = BR.reference(d)
    dY = d["p"].double() * d["G"].double() + d["q"].double() * d["Y"].double() + d["t"].double()
    assert _rel(ref["Gprev"], dY @ d["W"].double().t()) <= TOL


def test_wrong_restatements_are_rejected():
    """the weight belongs to q Y + t alone, and the statistics are those of the weighted dY: both mistakes are far outside 1e-10"""
    d = BR.make_inputs(272, 9)
    w = _weights(272, 10)
    args = (d["Yprev"], d["asc"], d["ash"], d["G"], d["Y"], d["p"], d["q"], d["t"], d["W"], w)
    ref = BR.bwd_tiles(*args)
    _, dW, dX = _autograd(d, w, None)
    on_g = BR.wrong_weight_on_g(*args)
    assert _rel(on_g["dW"], dW) > 1e-3 and _rel(on_g["Gprev"] * d["asc"].double(), dX) > 1e-3
    unw = BR.wrong_stats_unweighted(*args)
    assert _rel(unw["dW"], dW) <= TOL                      # (only its statistics are wrong)
    assert _rel(unw["gp"], ref["gp"]) > 1e-6 and _rel(unw["gpy"], ref["gpy"]) > 1e-6
    asc = d["asc"].double()
    nz = asc != 0
    assert _rel((unw["gp"] * asc)[nz], dX.sum(0)[nz]) > 1e-6


def test_block_row_weights_reads_the_table():
    blocks = torch.zeros(3, 4, dtype=torch.int32)
    blocks[:, 2] = torch.tensor([49.0, 1.0, 17.0]).view(torch.int32)
    w = BR.block_row_weights(blocks, 40)
    assert w[0] == 49 and w[16] == 1 and w[32] == 17 and w.sum() == 37 + 49 + 1 + 17


def _sa2_plan(B):
    """the plan of an SA2-shaped stack (B clouds x 128 groups x 64 slots, widths 128-128-256, compacted rows), launches stubbed"""
    run = ST.gather(B, 512, 128, 64, [128, 128, 256], True, "q_xyz", "train", compact=True)
    with ST.patched(fused_mlp, TRACE=[]), ST.stubbed() as log:
        nodes = fused_mlp.TRACE
        run("cpu", lambda: None)
    assert len(plans := [n.plan for n in nodes if hasattr(n, "plan")]) == 1
    return plans[0], [launch[0] for launch in log]


def test_planner_takes_the_tile_arm_from_the_row_floor():
    plan, names = _sa2_plan(64)                  # 524 288 allocated rows: the planner's floor
    mid = plan.layers[1]
    assert mid.bwd == fused_mlp.B_ONEPASS_TILES and mid.count > 0 and mid.store_y and plan.layers[0].store_y
    assert names.count("pcops_mlp_bwd_tiles_rows") == 1
    assert "pcops_mlp_wgrad_rows" not in names and "pcops_mlp_gemm_dgrad_rows" not in names
    # 262 144 (the SA2 stack of tests/test_pool_top_rows_gpu.py) and 65 536 (the stored trace of sa2_rows): the split arm
    for clouds in (32, 8):
        plan, names = _sa2_plan(clouds)
        assert plan.layers[1].bwd == fused_mlp.B_SPLIT
        assert "pcops_mlp_bwd_tiles_rows" not in names
        assert names.count("pcops_mlp_wgrad_rows") == 1 and names.count("pcops_mlp_gemm_dgrad_rows") == 1
