"""Launch traces of the fused stacks (fused_mlp.FusedMLPStack / EdgeConvPool): which entry points a forward + backward
calls, in which order, with which scalars and which pointers NULL.  libpcops's shape queries are host code, so with the
launches themselves replaced by a recorder a whole stack runs on CPU tensors in milliseconds -- every decision the host
code takes shows in the trace, none of the values do.

A trace is [forward launches, backward launches]; a launch is [name, arg, ...] with, per argument and by its type in
include/pcops.h, 0 / 1 for a NULL / non-NULL pointer and the value for a scalar.  pcops_small_gemm_pair is
[name, [M, K, N, M, K, N], [the other fields of both problems, pointers as 0 / 1]] -- the first list is what a
`_lib._hooks` hook sees of it.

CASES maps a name to a function (dev, between) -> outputs that runs ONE stack through the public entry points of fused_mlp; on a
CPU device its inputs are uninitialised (nothing reads them), on the GPU they are random and valid.
tests/golden/make_stack_traces.py stores the traces, tests/test_stack_plan_cpu.py / _gpu.py compare against them.
"""
import contextlib
import gzip
import itertools
import json
import os

import torch

from scanobjectnn_amd import _lib, fused_mlp
from scanobjectnn_amd import dist as _dist

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stack_traces.json.gz")
PAIR = "pcops_small_gemm_pair"
FLAGS = ("POOL_TOP", "POOL_TOP_ROWS", "BWD_FUSED", "FUSE_POOL_ROWS", "EDGE_DIRECT_FUSED", "STAT_PIVOT", "TAIL_FOLD")


def encode(name, args):
    types = _lib.SIGNATURES[name][0]
    assert len(types) == len(args), name
    out = [name]
    for t, a in zip(types, args):
        if t is _lib._P:
            out.append(0 if (a is None or (isinstance(a, int) and a == 0)) else 1)
        elif t is _lib._F:
            out.append(float(a))
        else:
            out.append(int(a))
    return out


def _encode_pair(p0, p1):
    rest = []
    for p in (p0, p1):      # (M, K, N, A, lda, transA, B, ldb, transB, bias, C, ldc, colsum)
        rest += [int(p[3] is not None), int(p[4]), int(p[5]), int(p[6] is not None), int(p[7]), int(p[8]),
                 int(p[9] is not None), int(p[10] is not None), int(p[11]), int(p[12] is not None)]
    return [PAIR, [int(v) for v in tuple(p0[:3]) + tuple(p1[:3])], rest]


@contextlib.contextmanager
def stubbed():
    """the launches of _lib replaced by a recorder (nothing reaches the library but its shape queries); yields the list
    the launches are appended to"""
    log = []
    saved = _lib.call, _lib.small_gemm_pair
    _lib.call = lambda name, *args: log.append(encode(name, args))
    _lib.small_gemm_pair = lambda p0, p1: log.append(_encode_pair(p0, p1))
    try:
        yield log
    finally:
        _lib.call, _lib.small_gemm_pair = saved


@contextlib.contextmanager
def hooked():
    """the same record from a `_lib._hooks` hook of real launches (of pcops_small_gemm_pair: the name and the six sizes)"""
    log = []

    def hook(name, phase, args):
        if phase == "pre":
            log.append([PAIR, [int(v) for v in args]] if name == PAIR else encode(name, args))
    _lib._hooks.append(hook)
    try:
        yield log
    finally:
        _lib._hooks.remove(hook)


def hook_view(trace):
    """what hooked() sees of a stored trace"""
    return [[launch[:2] if launch[0] == PAIR else launch for launch in half] for half in trace]


@contextlib.contextmanager
def patched(obj, **attrs):
    old = {k: getattr(obj, k) for k in attrs}
    for k, v in attrs.items():
        setattr(obj, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(obj, k, v)


def load_golden():
    with gzip.open(GOLDEN, "rt") as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------ inputs
def _t(dev, *shape):
    if torch.device(dev).type == "cpu":
        return torch.empty(shape, dtype=torch.float32)
    return torch.randn(shape, dtype=torch.float32, device=dev)


def _layers(dev, k0, widths, grad=True, misaligned=None):
    layers, cin = [], k0
    for li, w in enumerate(widths):
        if li == misaligned:        # a weight 4 bytes off the 16-byte alignment the one-pass backward needs
            W = _t(dev, cin * w + 1)[1:].view(cin, w)
        else:
            W = _t(dev, cin, w) / max(cin, 1) ** 0.5
        mv = _t(dev, w).abs() + 0.5
        layer = [W, 0.1 * _t(dev, w), 1.0 + 0.1 * _t(dev, w), 0.1 * _t(dev, w), 0.1 * _t(dev, w), mv]
        for t in layer[:4]:
            t.requires_grad_(grad)
        layers.append(tuple(layer))
        cin = w
    return layers


def _idx(dev, B, M, S, N, identity=False):
    if identity:
        return torch.arange(S, dtype=torch.int32, device=dev).view(1, 1, S).expand(B, 1, S).contiguous()
    if torch.device(dev).type == "cpu":
        return torch.empty((B, M, S), dtype=torch.int32)
    return torch.randint(0, N, (B, M, S), dtype=torch.int32, device=dev)


def _finish(out, mode, between):
    """between() where the forward has ended, then the backward of the stack's output(s) unless the mode has none;
    returns the outputs"""
    outs = out if isinstance(out, tuple) else (out,)
    between()
    if mode != "nograd":
        torch.autograd.backward(list(outs), [_t(o.device, *o.shape) for o in outs])
    return outs


def _mode_ctx(mode):
    return torch.no_grad() if mode == "nograd" else contextlib.nullcontext()


# mode: "train" | "eval" (gradient through frozen statistics) | "nograd" (eval, no autograd) | "noinput" (training, the
# stack's input needs no gradient)
def dense(R, S, K0, widths, pool, mode="train", misaligned=None):
    def run(dev, between):
        x = _t(dev, R, K0).requires_grad_(mode in ("train", "eval"))
        layers = _layers(dev, K0, widths, mode != "nograd", misaligned)
        with _mode_ctx(mode):
            out = fused_mlp.mlp_stack(x, S, pool, mode in ("train", "noinput"), 0.9, 1e-3, True, layers)
        return _finish(out, mode, between)
    return run


def gather(B, N, M, S, widths, pool, form, mode="train", compact=False, identity=False):
    """form: q_ctr | xyz_bias | q_xyz (tests/test_fused_mlp_gpu.py); compact: with a pts_cnt (compacted rows where the
    policy takes them); identity: idx = 0..N-1 with M = 1, S = N (group_all)"""
    def run(dev, between):
        C1 = widths[0]
        g = mode in ("train", "eval")
        Q = _t(dev, B, N, C1).requires_grad_(g) if form != "xyz_bias" else None
        Ctr = _t(dev, B, M, C1).requires_grad_(mode != "nograd") if form == "q_ctr" else None
        xyz = _t(dev, B, N, 3) if form != "q_ctr" else None
        new_xyz = _t(dev, B, M, 3) if form != "q_ctr" else None
        wxyz = _t(dev, 3, C1).requires_grad_(mode != "nograd") if form != "q_ctr" else None
        bias = _t(dev, C1).requires_grad_(mode != "nograd") if form == "xyz_bias" else None
        idx = _idx(dev, B, M, S, N, identity)
        cnt = None
        if compact:     # any count in [1, S]: the trace does not depend on it
            cnt = torch.full((B, M), S // 3 + 1, dtype=torch.int32, device=dev)
            if torch.device(dev).type != "cpu":
                cnt = torch.randint(1, S + 1, (B, M), dtype=torch.int32, device=dev)
        layers = _layers(dev, C1, widths, mode != "nograd")
        with _mode_ctx(mode):
            out = fused_mlp.gather_mlp_stack(idx, pool, mode in ("train", "noinput"), 0.9, 1e-3, True, layers, Q=Q, Ctr=Ctr,
                                             xyz=xyz, new_xyz=new_xyz, wxyz=wxyz, bias=bias, identity_idx=identity,
                                             pts_cnt=cnt)
        return _finish(out, mode, between)
    return run


def edge(B, N, k, widths, direct, mode="train", cat=False, misaligned=None):
    """an EdgeConv stack on the [Q | Ctr] product; direct: its input needs no gradient (pcops_edge_first_*);
    cat: a single pooled layer that also stores its block of a concatenation (EdgeConvPool)"""
    def run(dev, between):
        C1 = widths[0]
        layers = _layers(dev, 6, widths, mode != "nograd", misaligned)
        idx = _idx(dev, B, N, k, N)
        QC = _t(dev, B, N, 2 * C1)
        kw = {}
        if direct:
            w1, b1 = layers[0][0], layers[0][1]
            kw["direct"] = (_t(dev, B, N, 3), w1, b1)
        else:
            QC.requires_grad_(mode in ("train", "eval"))
        if cat:
            kw["cat_slot"] = (fused_mlp.CatBuffer((B, N, 3 * C1), dev), C1)
        with _mode_ctx(mode):
            out = fused_mlp.gather_mlp_stack(idx, True, mode in ("train", "noinput"), 0.9, 1e-3, False, layers, QC=QC, **kw)
        return _finish(out, mode, between)
    return run


def with_flags(run, **flags):
    def wrapped(dev, between):
        with patched(fused_mlp, **flags):
            return run(dev, between)
    return wrapped


def with_gram_wgrad(run):
    """the opt-in Gram form of the one-pass backward's weight gradient (pcops.h PCOPS_OPT_BWD_FUSED_GRAM_WGRAD)"""
    def wrapped(dev, between):
        prev = _lib.set_option(_lib.OPT_BWD_FUSED_GRAM_WGRAD, 1)
        try:
            return run(dev, between)
        finally:
            _lib.set_option(_lib.OPT_BWD_FUSED_GRAM_WGRAD, prev)
    return wrapped


def with_sync_bn(run):
    """SyncBN on one rank: the exchange hands the rank's own partials back"""
    def wrapped(dev, between):
        with patched(_dist, sync_bn_active=lambda: True, allreduce_stat_partials=lambda part, rows, pivot=None: (part, rows)):
            return run(dev, between)
    return wrapped


DENSE = [  # CASES of tests/test_fused_mlp_gpu.py
    (512 * 32, 32, 3, [64, 64, 128], True), (128 * 64, 64, 131, [128, 128, 256], True),
    (4 * 128, 128, 259, [256, 512, 1024], True), (1000, 1, 384, [256, 128], False), (777, 1, 128, [128], False),
    (130 * 20, 20, 6, [64], True), (1024 * 32 * 2, 32, 3, [64, 64, 128], True), (512 * 64 + 37, 1, 128, [128, 256], False),
    (128 * 64 * 4, 64, 132, [128, 128, 256], True), (40000, 1, 256, [64], False), (400 * 96, 96, 64, [64, 128], True),
    (130 * 256, 256, 32, [128, 64], True), (1100 * 32, 32, 16, [32, 32], True), (256 * 128, 128, 260, [256, 512, 1024], True),
    (33000, 1, 320, [1024, 64], False), (64 * 256, 256, 320, [1024], True), (48 * 256, 256, 128, [1024], True),
    (4096 * 20, 20, 64, [64, 128], True), (2048 * 16, 16, 32, [64, 64], True), (1024 * 48, 48, 32, [64, 128], True),
    (3000 * 11, 11, 64, [128], True), (1024 * 32 * 2 + 64, 32, 32, [64, 96, 128], True), (70000 + 19, 1, 64, [96, 128], False),
    (2048 * 16, 16, 64, [96, 128], True), (2048 * 20, 20, 32, [128, 128], True), (1100 * 48, 48, 16, [96, 128], True),
]
GATHER = [  # GATHER_CASES
    (4, 256, 64, 32, [64, 64, 128], True), (3, 100, 37, 16, [128, 128, 256], True), (2, 128, 128, 20, [64], True),
    (2, 90, 30, 8, [32, 32, 64], True), (2, 64, 16, 4, [64, 128], False), (8, 512, 256, 32, [64, 64, 128], True),
    (4, 512, 128, 64, [64, 128], False), (3, 700, 130, 96, [32, 64, 64], True), (2, 1024, 168, 128, [64, 96, 128], True),
]
COMPACT = [  # COMPACT_CASES without the radius (the trace does not depend on the counts)
    (8, 512, 128, 64, [128, 128, 256], "q_xyz"), (4, 1024, 256, 64, [64, 64, 128], "xyz_bias"),
    (8, 600, 100, 48, [64, 128], "q_xyz"), (2, 2048, 128, 128, [32, 64, 128], "xyz_bias"),
    (8, 512, 256, 64, [64, 64, 128], "q_xyz"), (4, 1024, 128, 128, [64, 96, 128], "xyz_bias"),
    (4, 1024, 128, 64, [64, 96], "q_xyz"), (8, 512, 128, 64, [128, 128], "q_xyz"),
]
# eight shapes that between them reach every backward arm: algebraic top layer on compacted rows + one-pass rows form;
# arithmetic first layer + one-pass xyz form; direct edge + one-pass edge forms; [Q | Ctr] scatter + Gram one-pass;
# cloud-bias + separate wgrad / dgrad of wide layers; algebraic top layer on plain rows + the dense first layer's dgrad;
# an unpooled dense stack; the arithmetic coordinate-only first layer under an unpooled output
REPRESENTATIVE = {
    "sa2_rows": lambda mode: gather(8, 512, 128, 64, [128, 128, 256], True, "q_xyz", mode, compact=True),
    "sa1_xyz_rows": lambda mode: gather(4, 1024, 256, 64, [64, 64, 128], True, "xyz_bias", mode, compact=True),
    "edge_direct": lambda mode: edge(8, 1024, 20, [64, 128], True, mode),
    "edge_qc": lambda mode: edge(8, 1024, 20, [64, 128], False, mode),
    "group_all": lambda mode: gather(8, 256, 1, 256, [256, 512, 1024], False, "q_ctr", mode, identity=True),
    "dense_pool_top": lambda mode: dense(128 * 64 * 4, 64, 132, [128, 128, 256], True, mode),
    "dense_plain": lambda mode: dense(512 * 64 + 37, 1, 128, [128, 256], False, mode),
    "xyz_unpooled": lambda mode: gather(4, 512, 128, 64, [64, 128], False, "xyz_bias", mode),
}


def _name(kind, *parts):
    return kind + "/" + "_".join("-".join(str(v) for v in p) if isinstance(p, (list, tuple)) else str(p) for p in parts)


def _cases():
    c = {}
    for R, S, K0, widths, pool in DENSE:        # (the three pool-top shapes are among them)
        c[_name("dense", R, S, K0, widths, int(pool))] = dense(R, S, K0, widths, pool)
    for B, N, M, S, widths, pool in GATHER:
        for form in ("q_ctr", "xyz_bias", "q_xyz"):
            c[_name("gather", B, N, M, S, widths, int(pool), form)] = gather(B, N, M, S, widths, pool, form)
    for B, N, M, S, widths, form in COMPACT:
        c[_name("compact", B, N, M, S, widths, form)] = gather(B, N, M, S, widths, True, form, compact=True)
    for widths in ([64], [128], [64, 128]):     # the [Q | Ctr] stacks of test_edge_conv_stack_one_gemm_matches_two
        c[_name("edge_qc", 8, 1024, 20, widths)] = edge(8, 1024, 20, widths, False)
    for B, N, k, widths in ((8, 1024, 20, [64, 128]), (4, 2048, 20, [64, 128]), (8, 1024, 16, [128, 64, 64])):
        c[_name("edge_direct", B, N, k, widths)] = edge(B, N, k, widths, True)
    for C in (64, 128):
        c[_name("edge_pool", C, "two_operand")] = gather(8, 1024, 1024, 20, [C], True, "q_ctr")
        c[_name("edge_pool", C, "qc")] = edge(8, 1024, 20, [C], False)
        c[_name("edge_pool", C, "qc_cat")] = edge(8, 1024, 20, [C], False, cat=True)
    # whole clouds as one group each; 256 points per cloud and more take the streaming forms (pcops_cloud_bias_*)
    for (B, N), pool in itertools.product(((16, 128), (8, 256)), (False, True)):
        run = gather(B, N, 1, N, [256, 512, 1024], pool, "q_ctr", identity=True)
        c[_name("group_all", B, N, int(pool))] = run
        c[_name("group_all", B, N, int(pool), "no_cloud_bias")] = with_flags(run, CLOUD_BIAS=False)
        c[_name("group_all", B, N, int(pool), "no_tail_fold")] = with_flags(run, TAIL_FOLD=False)
    for name, make in REPRESENTATIVE.items():
        for mode in ("train", "eval", "nograd", "noinput"):
            c[_name("rep", name, mode)] = make(mode)
        for flag in FLAGS:
            c[_name("rep", name, "no_" + flag)] = with_flags(make("train"), **{flag: False})
    c["misaligned/81920_20_64_64-128_1"] = dense(4096 * 20, 20, 64, [64, 128], True, misaligned=1)
    for name in ("edge_direct", "edge_qc", "dense_pool_top", "sa2_rows"):     # ... pcops_mlp_bwd_fused_gw / _edge_gw
        c[_name("gram_wgrad", name)] = with_gram_wgrad(REPRESENTATIVE[name]("train"))
    c[_name("gram_wgrad", "dense", 4096 * 20, 20, 64, [64, 128])] = with_gram_wgrad(dense(4096 * 20, 20, 64, [64, 128], True))
    c["sync_bn/dense"] = with_sync_bn(dense(512 * 32, 32, 3, [64, 64, 128], True))
    c["sync_bn/gather_xyz"] = with_sync_bn(gather(8, 512, 256, 32, [64, 64, 128], True, "xyz_bias"))
    c["sync_bn/edge_pool"] = with_sync_bn(edge(8, 1024, 20, [64], False))
    return c


CASES = _cases()
# the cases tests/test_stack_plan_gpu.py runs on the device
GPU_CASES = [
    _name("dense", 4096 * 20, 20, 64, [64, 128], 1), _name("dense", 64 * 256, 256, 320, [1024], 1),
    _name("dense", 128 * 64 * 4, 64, 132, [128, 128, 256], 1),
    _name("compact", 8, 512, 128, 64, [128, 128, 256], "q_xyz"), _name("compact", 4, 1024, 256, 64, [64, 64, 128], "xyz_bias"),
    _name("edge_direct", 8, 1024, 20, [64, 128]), _name("edge_direct", 8, 1024, 16, [128, 64, 64]),
    _name("edge_pool", 64, "qc_cat"), _name("group_all", 16, 128, 0),
]


def run_case(name, dev="cpu", recorder=stubbed):
    """([forward launches, backward launches], the autograd nodes fused_mlp.TRACE received, the outputs) of one case"""
    assert not any(k.startswith("PCOPS_") and k != "PCOPS_LIB" for k in os.environ), "the stored traces are the default switches'"
    mark = []
    with patched(fused_mlp, TRACE=[]), recorder() as log:
        nodes = fused_mlp.TRACE
        outs = CASES[name](dev, lambda: mark.append(len(log)))
    return [log[:mark[0]], log[mark[0]:]], [n for n in nodes if hasattr(n, "saved")], outs
