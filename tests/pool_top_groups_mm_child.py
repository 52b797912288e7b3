"""pcops_mlp_dgrad_top_groups in a process of its own (tests/test_pool_top_groups_mm_gpu.py): PCOPS_POOL_TOP_GROUPS_MM is
read once per process, so the test runs the walk (`=0`) here and its own process keeps the default.

    python tests/pool_top_groups_mm_child.py OUT.pt S,N,G,seed [S,N,G,seed ...]

The inputs of a case are test_pool_top_groups_gpu._inputs(S, 64, N, G, seed); OUT.pt holds {case: (Gprev, stats_partial,
pipe)} on the CPU, pipe being pcops_last_launch_pipe() behind the call.  `digest()` is the SHA-256 of a tensor's bytes, what
tests/golden/pool_top_groups_walk_bits.json records."""
import hashlib
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

KP = 64


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run_case(S, N, G, seed):
    from scanobjectnn_amd import _lib
    from test_pool_top_groups_gpu import _dgrad, _inputs
    d = _inputs(S, KP, N, G, seed)
    Gprev, part = _dgrad(G * S, KP, N, S, d)
    torch.cuda.synchronize()
    return Gprev.cpu(), part.cpu(), int(_lib.load().pcops_last_launch_pipe())


def main(argv):
    out = {}
    for case in argv[1:]:
        S, N, G, seed = (int(v) for v in case.split(","))
        out[case] = run_case(S, N, G, seed)
        print("%s pipe %d Gprev %s stats %s" % (case, out[case][2], digest(out[case][0]), digest(out[case][1])))
    torch.save(out, argv[0])
    print("pool top groups child ok (PCOPS_POOL_TOP_GROUPS_MM=%s)" % os.environ.get("PCOPS_POOL_TOP_GROUPS_MM", "unset"))


if __name__ == "__main__":
    main(sys.argv[1:])
