"""What the per-model A/B timing tools (bench_spidercnn, bench_mfv3d, bench_pointcnn, bench_pointnet) share: the event-timed
median, the launch counter, the per-entry-point event hook, one fresh child process per run, the report with its `# raw`
records, the numbers of a summary line and the reader of rocprofv3's kernel_stats.csv.  Each tool keeps its workload, its
configurations and its sentences.  torch is imported by the functions that run on the GPU, never by importing this module."""
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEWS = {"view", "reshape", "detach", "alias", "expand", "slice", "select", "t", "transpose", "unsqueeze", "squeeze",
         "as_strided", "empty", "empty_like", "empty_strided", "_unsafe_view", "permute", "split", "unbind", "narrow",
         "set_", "lift_fresh", "sym_size", "sym_stride", "sym_numel", "sym_storage_offset", "is_same_size", "new_empty"}


def timed(fn, warmup, steps, inner=1):
    """(median over `steps` windows of `inner` calls each, in ms per call; peak MB allocated over them)"""
    import torch
    for _ in range(warmup * inner):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / inner)
    return statistics.median(times), torch.cuda.max_memory_allocated() / 2 ** 20


def count_launches(fn):
    """[dispatched aten operators that compute, libpcops calls] of one fn()"""
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode
    from scanobjectnn_amd import _lib
    count = [0, 0]

    class Log(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if str(func).split(".")[1] not in VIEWS:
                count[0] += 1
            return func(*args, **(kwargs or {}))

    def hook(name, phase, a):
        if phase == "pre":
            count[1] += 1
    _lib._hooks.append(hook)
    try:
        with torch.autograd.set_multithreading_enabled(False), Log():       # backward runs under the mode too
            fn()
    finally:
        _lib._hooks.remove(hook)
    torch.cuda.synchronize()
    return count


def time_entry_points(step, prefixes, shape_len):
    """[(name, shape, ms)] of every libpcops call of one step() whose name starts with one of `prefixes`, HIP events around
    each launch; the shape is the call's first shape_len(name) integer arguments"""
    import torch
    from scanobjectnn_amd import _lib
    calls = []

    def hook(name, phase, a):
        if not name.startswith(prefixes):
            return
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        if phase == "pre":
            calls.append([name, a[:shape_len(name)], ev, None])
        else:
            calls[-1][3] = ev
    _lib._hooks.append(hook)
    try:
        step()
        torch.cuda.synchronize()
    finally:
        _lib._hooks.remove(hook)
    return [(name, [int(v) for v in shape], e0.elapsed_time(e1)) for name, shape, e0, e1 in calls]


def emit(res):
    print("RESULT " + json.dumps(res), flush=True)


def run_child(script, child_argv, env_overlay, timeout):
    """(the last RESULT record, seconds taken) of one fresh child process, which has ended when this returns.  A child that
    fails or reports nothing ends the caller (SystemExit), and one that outlasts `timeout` raises TimeoutExpired: whatever
    the cause, nothing is started on the GPU after a run that went wrong."""
    t0 = time.time()
    out = subprocess.run([sys.executable, script] + child_argv, env=dict(os.environ, **env_overlay), cwd=ROOT,
                         capture_output=True, text=True, timeout=timeout)
    found = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
    if out.returncode != 0 or not found:
        print("child %s %s %s (exit %d): %s" % (" ".join(child_argv), env_overlay, "failed" if out.returncode else
                                                 "printed no RESULT", out.returncode, out.stderr[-2000:]), flush=True)
        raise SystemExit(1)
    return json.loads(found[-1][7:]), time.time() - t0


class Report:
    """the lines of one invocation, printed as they come and written with the raw records at the end"""

    def __init__(self):
        self.lines = []

    def say(self, s):
        print(s, flush=True)
        self.lines.append(s)

    def write(self, path, results):
        """given a path, the lines and the raw records they were made from"""
        if path:
            with open(path, "w") as f:
                f.write("\n".join(self.lines) + "\n")
                f.write("# raw\n" + "\n".join(json.dumps(r) for r in results) + "\n")

    @staticmethod
    def append(path, lines):
        """print the lines of a --kernel_stats summary and, given a path, add them to that report"""
        print("\n".join(lines))
        if path:
            with open(path, "a") as f:
                f.write("\n".join(lines) + "\n")


def split_on_off(records, key):
    """the records whose fields equal `key`'s, as (switch on, switch off): `on` where the parent noted which switch it
    alternated, else `native`"""
    sel = [r for r in records if all(r[k] == v for k, v in key.items())]
    return [r for r in sel if r.get("on", r["native"])], [r for r in sel if not r.get("on", r["native"])]


def median(records, field="ms"):
    return statistics.median(r[field] for r in records)


def per_round(records):
    return " ".join("%.3f" % r["ms"] for r in records)


def spread(on, off):
    """the larger of the two sides' max - min, of two lists of numbers"""
    return max(max(on) - min(on), max(off) - min(off))


def peak_mb(on, off):
    return max(r["max_memory_allocated_mb"] for r in on), max(r["max_memory_allocated_mb"] for r in off)


def launches(on, off):
    """aten + libpcops launches of the last round's call, each side"""
    return on[-1]["aten_ops"] + on[-1]["pcops_calls"], off[-1]["aten_ops"] + off[-1]["pcops_calls"]


def kernel_stats_rows(directory, sub, required=False):
    """the rows of the last DIR/sub/**/*kernel_stats.csv (rocprofv3 --kernel-trace --stats) as dicts; without one [], or the
    end of the run where the summary cannot do without it"""
    files = sorted(glob.glob(os.path.join(directory, sub, "**", "*kernel_stats.csv"), recursive=True))
    if not files and required:
        raise SystemExit("no kernel_stats.csv under %s/%s" % (directory, sub))
    if not files:
        return []
    with open(files[-1]) as f:
        return list(csv.DictReader(f))


def add_common_args(parser, steps, warmup, windows=False):
    """the flags every tool has; `windows`: a run times windows of several calls, not single calls"""
    parser.add_argument("--child", action="store_true")
    parser.add_argument("--steps", type=int, default=steps, help="timed windows per run" if windows else None)
    parser.add_argument("--warmup", type=int, default=warmup, help="untimed windows first" if windows else None)
    parser.add_argument("--rounds", type=int, default=2)
    parser.add_argument("--child_timeout", type=int, default=300)
    parser.add_argument("--out", default="")
