"""Writes tests/golden/stack_traces.json.gz: the launch trace of every case of tests/stack_trace.py (see there), as the
package found FIRST on the path produces them -- run it with the parent commit's tree in front to pin a refactor:

    PYTHONPATH=<parent worktree, library built> python tests/golden/make_stack_traces.py [output file]

Only the public entry points of fused_mlp are used.  Compact JSON (no whitespace, 0 / 1 for booleans), gzip with a zero
time stamp: the same traces give the same bytes."""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.append(os.path.dirname(HERE))                 # tests/
sys.path.append(os.path.dirname(os.path.dirname(HERE)))  # the repository (behind whatever PYTHONPATH names)

import stack_trace as ST  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else ST.GOLDEN
    traces = {name: ST.run_case(name)[0] for name in ST.CASES}
    data = json.dumps(traces, separators=(",", ":"), sort_keys=True).encode()
    with open(out, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as z:
        z.write(data)
    print("%d cases, %d launches, %d bytes of JSON, %d bytes stored; package: %s"
          % (len(traces), sum(len(t[0]) + len(t[1]) for t in traces.values()), len(data), os.path.getsize(out),
             os.path.dirname(ST.fused_mlp.__file__)))


if __name__ == "__main__":
    main()
