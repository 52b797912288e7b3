"""The per-model A/B timing tools (tools/bench_{pointnet,pointcnn,spidercnn,mfv3d}.py over tools/ab_bench.py), pinned without a
GPU: the raw records that each committed profile holds, handed back in order where a child process would have produced them,
must give that profile's header, per-run lines and summary again, line for line; the run order, the child-process protocol,
the kernel-trace reader and both sides of every verdict sentence are checked on hand-made inputs."""
import argparse
import ast
import importlib.util
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
# (tool, argv, profile, raw records, summary lines)
REPLAYS = [("bench_pointnet", [], "pointnet_bench.txt", 24, 6),
           ("bench_pointcnn", ["--model", "pointcnn_seg", "--steps", "5", "--inner_step", "5", "--inner_layer", "200"],
            "pointcnn_seg_bench.txt", 36, 9),
           ("bench_spidercnn", [], "spidercnn_bench.txt", 8, 60),
           ("bench_mfv3d", ["--rounds", "2", "--steps", "10", "--warmup", "3"], "mfv3d_bench.txt", 12, 67)]
ELAPSED = re.compile(r"  \(\d+ s\)$")


def _load(name):
    if TOOLS not in sys.path:
        sys.path.insert(0, TOOLS)                      # the tools import ab_bench as scripts do, from their own directory
    spec = importlib.util.spec_from_file_location(name, os.path.join(TOOLS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _args(tool, argv, monkeypatch):
    """the tool's own parse of argv: what main() hands to parent()"""
    got = []
    with monkeypatch.context() as m:
        m.setattr(tool, "parent", got.append)
        tool.main(argv)
    return got[0]


def _profile(name):
    """(header, per-run lines, summary lines, raw records as lines) of a committed profile"""
    lines = open(os.path.join(ROOT, "profiles", name)).read().split("\n")
    head = next(i for i, l in enumerate(lines) if l.startswith("# tools/bench_"))
    blank, raw = lines.index(""), lines.index("# raw")
    records = []
    for l in lines[raw + 1:]:
        if not l.startswith("{"):
            break
        records.append(l)
    return lines[head], lines[head + 1:blank], lines[blank + 1:raw], records


@pytest.mark.parametrize("name,argv,profile,n_records,n_summary", REPLAYS, ids=[r[2] for r in REPLAYS])
def test_profile_replays(name, argv, profile, n_records, n_summary, monkeypatch, tmp_path):
    tool = _load(name)
    header, runs, summary, raw = _profile(profile)
    assert (len(raw), len(summary)) == (n_records, n_summary)
    args = _args(tool, argv, monkeypatch)
    pending, calls = [json.loads(l) for l in raw], []

    def fake_run_child(script, child_argv, env_overlay, timeout):
        rec = pending.pop(0)
        calls.append((child_argv, env_overlay, rec))
        return {k: v for k, v in rec.items() if k not in ("switch", "on")}, 0.0     # the parent adds these two itself
    monkeypatch.setattr(tool.ab_bench, "run_child", fake_run_child)
    out = tmp_path / "out.txt"
    tool.main(argv + ["--out", str(out)])
    assert not pending and len(calls) == n_records
    written = out.read_text().split("\n")
    assert written[0] == header == tool.header(args)
    assert [ELAPSED.sub("", l) for l in written[1:1 + n_records]] == [ELAPSED.sub("", l) for l in runs]
    assert all(ELAPSED.search(l) for l in runs) and all(l.endswith("  (0 s)") for l in written[1:1 + n_records])
    assert written[1 + n_records] == ""
    assert written[2 + n_records:2 + n_records + n_summary] == summary
    assert written[2 + n_records + n_summary:] == ["# raw"] + raw + [""]
    # summarise alone, on the records as the parent kept them, is the same pure function of them
    assert tool.summarise([json.loads(l) for l in raw], args) == summary

    # the run order: every config `rounds` times, the switch on and then off, with the config's own child arguments
    expected = [(child_argv, overlay, key, value) for child_argv, overlay, key in tool.configs(args)
                for _ in range(args.rounds) for value in ("1", "0")]
    assert len(expected) == n_records
    for (child_argv, overlay, key, value), (got_argv, got_overlay, rec) in zip(expected, calls):
        assert got_argv == child_argv and child_argv[0] == "--child"
        assert {k: rec[k] for k in key} == key
        assert rec.get("on", rec["native"]) == (value == "1")
        if name == "bench_pointcnn":
            assert overlay == {"PCOPS_XCONV_NATIVE": "1", "PCOPS_XCONV_GROUPS": "1"}      # both pinned, then one alternates
            assert got_overlay == dict(overlay, **{key["switch"]: value})
            assert rec["native"] == (got_overlay["PCOPS_XCONV_NATIVE"] == "1")
            assert rec["groups"] == int(got_overlay["PCOPS_XCONV_GROUPS"])
        else:
            assert overlay == {} and list(got_overlay.values()) == [value]
    if name == "bench_pointcnn":
        assert [c[2]["switch"] for c in tool.configs(args)] == ["PCOPS_XCONV_NATIVE"] * 6 + ["PCOPS_XCONV_GROUPS"] * 3


def test_shared_module_imports_no_torch():
    tree = ast.parse(open(os.path.join(TOOLS, "ab_bench.py")).read())
    top = [a.name for n in tree.body if isinstance(n, ast.Import) for a in n.names]
    top += [n.module for n in tree.body if isinstance(n, ast.ImportFrom)]
    assert top and not [m for m in top if m.split(".")[0] in ("torch", "scanobjectnn_amd", "numpy")]


def test_run_child_takes_last_result_and_stops_at_a_failure(capsys):
    ab_bench = _load("ab_bench")
    good = "import os; print('RESULT {\"v\": 1}'); print('noise'); print('RESULT {\"v\": \"%s\"}' % os.environ['AB_BENCH_TEST'])"
    res, seconds = ab_bench.run_child("-c", [good], {"AB_BENCH_TEST": "two"}, 60)
    assert res == {"v": "two"} and seconds >= 0.0
    for bad, said in (("import sys; sys.stderr.write('went wrong'); sys.exit(3)", "failed (exit 3): went wrong"),
                      ("pass", "printed no RESULT (exit 0)")):
        started = []
        with pytest.raises(SystemExit) as stop:
            for code in (good, bad, good):                # a caller's loop: nothing may start after the child that failed
                started.append(code)
                ab_bench.run_child("-c", [code], {"AB_BENCH_TEST": "x"}, 60)
        assert stop.value.code == 1 and started == [good, bad]
        assert said in capsys.readouterr().out


def test_entry_point_hook_is_removed_when_the_step_raises():
    from scanobjectnn_amd import _lib
    ab_bench = _load("ab_bench")
    before = list(_lib._hooks)

    def step():
        assert len(_lib._hooks) == len(before) + 1
        raise RuntimeError("step failed")
    with pytest.raises(RuntimeError, match="step failed"):
        ab_bench.time_entry_points(step, ("pcops_",), lambda name: 2)
    assert _lib._hooks == before


STATS = """"Name","Calls","TotalDurationNs","AverageNs","Percentage","MinNs","MaxNs","StdDev"
"void (anonymous namespace)::tnet_apply_fwd_kernel<64>(float const*, float const*, float*, int)",100,5000000,50000.0,50.0,40000,60000,1.0
"void (anonymous namespace)::xconv_dgrad_kernel<12, 2>(xconv_args)",100,2500000,25000.0,25.0,20000,30000,1.0
"xconv_fwd_kernel<12, 2>(xconv_args)",50,1500000,30000.0,15.0,29000,31000,1.0
"xconv_reduce_kernel(float const*, float*, int)",25,500000,20000.0,5.0,19000,21000,1.0
"void at::native::vectorized_elementwise_kernel<4, at::native::FillFunctor<float>>(int, at::native::FillFunctor<float>)",24,480000,20000.0,4.8,19000,21000,1.0
"tnet_ortho_kernel(float const*, float*, float*, int, float)",100,20000,200.0,0.2,100,300,1.0
"""


def test_kernel_stats_readers(tmp_path, capsys):
    traces = tmp_path / "traces"
    deep = traces / "transform_b32_n1024_native1" / "host" / "1234"
    deep.mkdir(parents=True)
    (deep / "p_kernel_stats.csv").write_text(STATS)
    (traces / "empty_run").mkdir()
    ab_bench = _load("ab_bench")
    rows = ab_bench.kernel_stats_rows(str(traces), "transform_b32_n1024_native1")
    assert len(rows) == 6 and rows[3]["Name"].startswith("xconv_reduce_kernel(") and rows[3]["Calls"] == "25"
    assert ab_bench.kernel_stats_rows(str(traces), "empty_run") == []

    out = tmp_path / "report.txt"
    out.write_text("kept\n")
    _load("bench_pointnet").kernel_stats(argparse.Namespace(kernel_stats=str(traces), out=str(out)))
    run = "transform_b32_n1024_native1       "
    expected = ["", "# kernel times: rocprofv3 --kernel-trace --stats, one run per launcher, size and form; us per launch.  The "
                "transform moves 3 b n 256 bytes forward + backward reads and 2 b n 256 bytes of writes.",
                run + " %-90s calls   100  avg     50.0 us  min     40.0 us" % "tnet_apply_fwd_kernel<64>",
                run + " %-90s calls   100  avg     25.0 us  min     20.0 us" % "xconv_dgrad_kernel<12, 2>",
                run + " %-90s calls    50  avg     30.0 us  min     29.0 us" % "xconv_fwd_kernel<12, 2>",
                run + " %-90s calls    25  avg     20.0 us  min     19.0 us" % "xconv_reduce_kernel",
                run + " %-90s calls   100  avg      0.2 us  min      0.1 us" % "tnet_ortho_kernel",
                run + " all of the above per call of the loop: 95.2 us"]       # the fill kernel (24 calls < 100 / 4) is setup
    assert capsys.readouterr().out == "\n".join(expected) + "\n"
    assert out.read_text() == "kept\n" + "\n".join(expected) + "\n"

    pointcnn = _load("bench_pointcnn")
    assert pointcnn._trace_rows(str(traces), "transform_b32_n1024_native1") == {
        "dgrad_kernel<12, 2>": (100, 25.0, 20.0), "fwd_kernel<12, 2>": (50, 30.0, 29.0), "reduce_kernel": (25, 20.0, 19.0)}
    with pytest.raises(SystemExit, match="no kernel_stats.csv under"):
        pointcnn._trace_rows(str(traces), "empty_run")


def _pointnet_records(on, off):
    """two rounds of every bench_pointnet config with the given ms per round on each side"""
    return [{"what": what, "native": native, "batch": b, "num_point": n, "ms": ms, "max_memory_allocated_mb": 1.0,
             "window_ms": ms, "aten_ops": 1, "pcops_calls": 1}
            for what in ("step", "transform", "ortho") for b, n in ((32, 1024), (256, 2048))
            for r in range(2) for native, ms in ((True, on[r]), (False, off[r]))]


def test_spread_and_verdicts_are_strict(monkeypatch):
    ab_bench = _load("ab_bench")
    assert ab_bench.spread([1.0, 2.0], [2.5, 2.5]) == 1.0 and ab_bench.spread([3.0, 3.0], [1.0, 1.25, 0.5]) == 0.75
    pointnet = _load("bench_pointnet")
    args = _args(pointnet, [], monkeypatch)
    # medians 1.5 and 2.5: the difference is the spread (1.0) exactly, which is not more than the spread
    for line in pointnet.summarise(_pointnet_records([1.0, 2.0], [2.5, 2.5]), args):
        assert "torch - native = 1.000 ms, spread between rounds 1.000 ms: within the spread; ratio 1.67;" in line
    for line in pointnet.summarise(_pointnet_records([2.5, 2.5], [1.0, 2.0]), args):
        assert "torch - native = -1.000 ms, spread between rounds 1.000 ms: within the spread; ratio 0.60;" in line
    for line in pointnet.summarise(_pointnet_records([1.0, 2.0], [2.5, 2.75]), args):
        assert "torch - native = 1.125 ms, spread between rounds 1.000 ms: more than the spread; ratio 1.75;" in line
    for line in pointnet.summarise(_pointnet_records([2.5, 2.75], [1.0, 2.0]), args):
        assert "torch - native = -1.125 ms, spread between rounds 1.000 ms: more than the spread; ratio 0.57;" in line

    pointcnn = _load("bench_pointcnn")
    args = _args(pointcnn, ["--model", "pointcnn_seg"], monkeypatch)
    at = pointcnn._groups_verdict(0, "fwd", [1.0, 2.0], [2.5, 2.5], args)
    assert at.startswith("xdconv_1 fwd  : groups 1.0 2.0 us, one group 2.5 2.5 us; one group - groups = 1.0 us, spread between "
                         "rounds 1.0 us: NOT lower by more than the spread; with groups ")
    over = pointcnn._groups_verdict(1, "dgrad", [1.0, 2.0], [2.5, 2.75], args)
    assert over.startswith("xdconv_2 dgrad: groups 1.0 2.0 us, one group 2.5 2.8 us; one group - groups = 1.1 us, spread between "
                           "rounds 1.0 us: LOWER by more than the spread; with groups ")
    slower = pointcnn._groups_verdict(1, "dgrad", [2.5, 2.75], [1.0, 2.0], args)
    assert "one group - groups = -1.1 us, spread between rounds 1.0 us: NOT lower by more than the spread;" in slower
