"""The SA2-shaped stack of tests/test_bwd_tiles128_gpu.py in a process of its own: PCOPS_BWD_TILES128 is read once per process, so
the test runs the switched-off library here and its own process keeps the default.

    python tests/bwd_tiles128_child.py OUT.pt

OUT.pt holds {"query": pcops_mlp_bwd_tiles_groups(524288, 128, 128), "out", "grads", "launches"} on the CPU."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(argv):
    from scanobjectnn_amd import _lib
    from test_bwd_tiles128_gpu import run_stack, sa2_stack
    query = int(_lib.load().pcops_mlp_bwd_tiles_groups(524288, 128, 128))
    out, _, grads, launches = run_stack(sa2_stack())
    torch.save({"query": query, "out": out.cpu(), "grads": [g.cpu() for g in grads], "launches": launches}, argv[0])
    print("bwd tiles128 child ok (PCOPS_BWD_TILES128=%s)" % os.environ.get("PCOPS_BWD_TILES128", "unset"))


if __name__ == "__main__":
    main(sys.argv[1:])
