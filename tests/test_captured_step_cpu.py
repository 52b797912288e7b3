"""The host side of `--graph` (scanobjectnn_amd/captured_step.py), without a GPU: the entry point that reads Adam's step size
from device memory is declared, bound and checks its arguments before any launch; the rule that asks for a new capture is
a pure function of the schedule values; the refusals are decided from the flags, the world size and the environment."""
import argparse
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_binding_maps_the_device_lr_adam():
    from scanobjectnn_amd import _lib
    LL, P, F = ctypes.c_longlong, ctypes.c_void_p, ctypes.c_float
    text = open(os.path.join(ROOT, "include", "pcops.h")).read()
    assert "int pcops_adam_step_dev(long long n, float *p, const float *g, float *m, float *v, float beta1, float beta2," in text
    assert _lib.SIGNATURES["pcops_adam_step_dev"] == ([LL, P, P, P, P, F, F, P, F], True)
    assert _lib.SIGNATURES["pcops_adam_step"] == ([LL, P, P, P, P, F, F, F, F], True)        # the by-value form has not moved
    assert _lib.ABI_VERSION == 4 and _lib.load().pcops_abi_version() == 4


def test_device_lr_adam_checks_its_arguments_before_any_launch():
    """n % 4 != 0 -> shape error; a null p, g, m, v or lr_t -> pointer error; n == 0 -> ok (no pointer is looked at)"""
    from scanobjectnn_amd import _lib
    lib = _lib.load()
    b1, b2, eps = ctypes.c_float(0.9), ctypes.c_float(0.999), ctypes.c_float(1e-8)
    buf = (ctypes.c_float * 8)()                      # host memory: only ever compared against NULL, never launched on
    ok = ctypes.cast(buf, ctypes.c_void_p)

    def call(n, p, g, m, v, lr):
        return lib.pcops_adam_step_dev(ctypes.c_longlong(n), p, g, m, v, b1, b2, lr, eps, None)

    assert call(6, ok, ok, ok, ok, ok) == -2
    assert call(-4, ok, ok, ok, ok, ok) == -2
    assert call(0, None, None, None, None, None) == 0
    for hole in range(5):
        ptrs = [ok] * 5
        ptrs[hole] = None
        assert call(8, *ptrs) == -1, hole
    assert "null" in _lib.strerror(-1)


def _capture_steps(optimizer, batch, base_lr, decay_step, decay_rate, nsteps):
    from scanobjectnn_amd import captured_step as CS, train_util as TU
    captured, steps = None, []
    for s in range(nsteps):
        wanted = CS.baked_values(optimizer, TU.get_learning_rate(s, batch, base_lr, decay_step, decay_rate),
                                 TU.get_bn_decay(s, batch, float(decay_step)))
        if CS.needs_capture(captured, wanted):
            steps.append(s)
            captured = wanted
    return steps


def test_recapture_rule_follows_the_schedules():
    from scanobjectnn_amd import train_util as TU
    seen, changes = [], []
    for s in range(400):
        d = TU.get_bn_decay(s, 16, 32.0)
        if not seen or seen[-1] != d:
            seen.append(d)
            changes.append(s)
    assert seen == [0.5, 0.75, 0.875, 0.9375, 0.96875, 0.984375, 0.99]
    assert changes == [0, 2, 4, 6, 8, 10, 12]
    # Adam: lr travels through device memory, so only bn_decay asks for a capture
    assert _capture_steps("adam", 16, 0.001, 32, 0.7, 400) == [0, 2, 4, 6, 8, 10, 12]
    # momentum bakes lr too: every staircase step of lr (every second step, until the 1e-5 floor holds it) asks as well
    lr_changes = [s for s in range(400) if s == 0 or TU.get_learning_rate(s, 16, 0.001, 32, 0.7) !=
                  TU.get_learning_rate(s - 1, 16, 0.001, 32, 0.7)]
    assert lr_changes[:9] == [0, 2, 4, 6, 8, 10, 12, 14, 16] and lr_changes[-1] == 26          # 0.001 * 0.7^13 < 1e-5
    assert _capture_steps("momentum", 16, 0.001, 32, 0.7, 400) == lr_changes
    assert len(lr_changes) > 7


def test_recapture_rule_is_a_function_of_the_values_alone():
    from scanobjectnn_amd import captured_step as CS
    assert CS.needs_capture(None, (0.5,))
    assert not CS.needs_capture((0.5,), (0.5,)) and CS.needs_capture((0.5,), (0.75,))
    assert CS.baked_values("adam", 0.001, 0.5) == CS.baked_values("adam", 0.0007, 0.5) == (0.5,)
    assert CS.baked_values("momentum", 0.001, 0.5) == (0.5, 0.001) != CS.baked_values("momentum", 0.0007, 0.5)


def _args(**kw):
    base = dict(model="pointnet2_cls_ssg", sync_bn=False, train_file="")
    base.update(kw)
    return argparse.Namespace(**base)


def test_refusals_are_decided_from_flags_world_and_environment():
    from scanobjectnn_amd import captured_step as CS
    for model in ("pointnet2_cls_ssg", "dgcnn", "pointcnn_cls", "pointnet_cls"):
        assert CS.refusal(_args(model=model), 1, {}) is None, model
        assert CS.refusal(_args(model=model, train_file="train.h5"), 1, {"PCOPS_SYNC": "0"}) is None
        assert CS.refusal(_args(model=model, train_file="train.npz"), 1, {}) is None
    assert tuple(CS.VERIFIED_MODELS) == ("pointnet2_cls_ssg", "dgcnn", "pointcnn_cls", "pointnet_cls")
    assert "ranks" in CS.refusal(_args(), 2, {})
    assert "PCOPS_SYNC" in CS.refusal(_args(), 1, {"PCOPS_SYNC": "1"})
    assert "sync_bn" in CS.refusal(_args(sync_bn=True), 1, {})
    assert "ragged" in CS.refusal(_args(train_file="training_objectdataset.pickle"), 1, {})
    assert "PCOPS_FUSED_ADAM" in CS.refusal(_args(), 1, {"PCOPS_FUSED_ADAM": "0"})
    from scanobjectnn_amd.pointnet2 import train as T
    for model in sorted(set(T.MODELS) - set(CS.VERIFIED_MODELS)):
        why = CS.refusal(_args(model=model), 1, {})
        assert why is not None and model in why and "\n" not in why, model


def test_graph_flag_parses_and_defaults_to_off():
    from scanobjectnn_amd.pointnet2 import train as T
    assert T.parse_args([]).graph is False
    assert T.parse_args(["--graph", "--model", "pointcnn_cls"]).graph is True


def test_committed_graph_step_report_follows_from_its_raw_records():
    """profiles/graph_step_ab.txt: the summary lines are what tools/bench_graph_step.py makes of the raw records kept below
    them, one eager and one graph record per configuration and round"""
    import importlib.util
    import json
    import sys
    tools = os.path.join(ROOT, "tools")
    sys.path.insert(0, tools)
    try:
        spec = importlib.util.spec_from_file_location("bench_graph_step", os.path.join(tools, "bench_graph_step.py"))
        tool = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(tool)
    finally:
        sys.path.remove(tools)
    lines = open(os.path.join(ROOT, "profiles", "graph_step_ab.txt")).read().splitlines()
    blank, raw = lines.index(""), lines.index("# raw")
    records = [json.loads(l) for l in lines[raw + 1:] if l]
    args = argparse.Namespace(steps=8, warmup=2, inner=10, rounds=2)
    assert len(records) == 2 * 2 * len(tool.CONFIGS) and sum(r["on"] for r in records) == len(records) // 2
    assert all(r["pcops_calls"] == 0 and r["captures"] == 1 for r in records if r["on"])
    assert all(r["pcops_calls"] > 0 for r in records if not r["on"])
    assert lines[blank + 1:raw] == tool.summarise(records, args)
    assert lines[1:blank] == [tool.run_line(r, i // 2 % 2, float(l.rsplit("(", 1)[1].split(" s)")[0]))
                              for i, (r, l) in enumerate(zip(records, lines[1:blank]))]
