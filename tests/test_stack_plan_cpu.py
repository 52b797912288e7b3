"""fused_mlp's stack plan against the launch traces stored in tests/golden/stack_traces.json.gz (tests/stack_trace.py;
recorded on the commit before the plan existed): every stack calls the same entry points in the same order with the same
scalars and the same pointers NULL -- on CPU tensors, with the launches replaced by a recorder.  Which buffer goes into
which slot, and the values, are the float64 GPU tests' business."""
import pytest

import stack_trace as ST
from scanobjectnn_amd import fused_mlp

GOLDEN = ST.load_golden()
# position of Y among the arguments of the forward entry points that store a layer's output
Y_ARG = {"pcops_sa_gather_fwd_ld": 10, "pcops_cloud_bias_fwd": 5, "pcops_sa_gather_fwd_rows": 12, "pcops_mlp_gemm_fwd": 9,
         "pcops_mlp_gemm_fwd_xyz_rows": 9, "pcops_mlp_gemm_fwd_pool_rows": 10, "pcops_mlp_gemm_fwd_rows": 9,
         "pcops_mlp_gemm_fwd_pool": 11}


def test_the_stored_cases_are_the_cases():
    assert sorted(GOLDEN) == sorted(ST.CASES)
    assert all(name in GOLDEN for name in ST.GPU_CASES)


@pytest.mark.parametrize("name", sorted(ST.CASES))
def test_trace_equals_the_stored_one(name):
    trace, nodes, _ = ST.run_case(name)
    want = GOLDEN[name]
    for half, got, ref in zip(("forward", "backward"), trace, want):
        assert [launch[0] for launch in got] == [launch[0] for launch in ref], half
        for g, r in zip(got, ref):
            assert g == r, (half, g, r)
    # the saved plan's "Y stored" bits are the Y pointers of the forward launches, layer by layer
    for node in nodes:
        if not isinstance(node.saved, fused_mlp.StackSaved):
            continue
        stored = [launch[1 + Y_ARG[launch[0]]] for launch in trace[0] if launch[0] in Y_ARG]
        assert stored == [int(lp.store_y) for lp in node.plan.layers]
        assert stored == [int(y is not None) for y in node.saved.Ys]


def test_the_misaligned_weight_refuses_the_one_pass_backward():
    names = [launch[0] for launch in ST.run_case("misaligned/81920_20_64_64-128_1")[0][1]]
    assert "pcops_mlp_wgrad_rows" in names and not any(n.startswith("pcops_mlp_bwd_fused") for n in names)
    aligned = [launch[0] for launch in GOLDEN["dense/81920_20_64_64-128_1"][1]]
    assert any(n.startswith("pcops_mlp_bwd_fused") for n in aligned)


def test_edge_rows_are_stored_only_where_the_backward_reduces_them():
    """one decision: the forward of a direct EdgeConv stack stores the edge rows exactly when the layer above takes the
    one-pass edge form -- also where only the weight's address refuses that form"""
    for misaligned, want in ((None, True), (1, False)):
        with ST.patched(fused_mlp, TRACE=[]), ST.stubbed() as log:
            ST.edge(8, 1024, 20, [64, 128], True, misaligned=misaligned)("cpu", lambda: None)
            plan = fused_mlp.TRACE[0].plan
        names = [launch[0] for launch in log]
        moments = [launch for launch in log if launch[0] == "pcops_edge_first_moments"]
        assert plan.edge_rows == want and moments[0][-1] == int(want)
        assert ("pcops_mlp_bwd_fused_edge" in names) == want and ("pcops_edge_first_wgrad" in names) != want


def test_no_backward_is_planned_where_none_can_happen():
    _, nodes, _ = ST.run_case("rep/sa2_rows_nograd")
    assert nodes == []                       # (nothing is kept either)
    plan = fused_mlp.plan_stack(R=8192, S=64, K0=131, widths=[128, 128, 256], pool=1, training=False, need_grad=False,
                                need_dx=False, sync=False, w_aligned=[True] * 3, has_b=[True] * 3)
    assert [lp.bwd for lp in plan.layers] == ["", "", ""] and not plan.pool_top
