"""pcops_mlp_bwd_fused_xyz_rows in a process of its own (tests/test_xyz_bwd_tiles_gpu.py): PCOPS_BWD_XYZ_TILES is read once per
process, so the test runs bwd_fused_kernel (`=0`) here and its own process keeps the default.

    python tests/xyz_bwd_tiles_child.py OUT.pt M,seed,kind [M,seed,kind ...]

The inputs of a case are xyz_bwd_ref.make_inputs(M, 64, seed, kind); OUT.pt holds {case: (dW, db, stats_partial, xyz_stats,
plan, pipe)} on the CPU, plan and pipe being pcops_last_launch_plan() / pcops_last_launch_pipe() behind the call."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(argv):
    from test_xyz_bwd_tiles_gpu import _call, _device_inputs
    out = {}
    for case in argv[1:]:
        M, seed, kind = case.split(",")
        r = _call(_device_inputs(int(M), 64, int(seed), kind), int(M), 64)
        out[case] = (r["dW"].cpu(), r["db"].cpu(), r["st"].cpu(), r["xs"].cpu(), r["plan"], r["pipe"])
        print("%s plan %s pipe %d" % (case, r["plan"], r["pipe"]))
    torch.save(out, argv[0])
    print("xyz bwd tiles child ok (PCOPS_BWD_XYZ_TILES=%s)" % os.environ.get("PCOPS_BWD_XYZ_TILES", "unset"))


if __name__ == "__main__":
    main(sys.argv[1:])
