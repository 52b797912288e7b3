"""ctypes binding of libpcops.so (the C ABI of include/pcops.h).

The product path is HIP-only: there is NO CPU fallback.  A missing library, a CPU
tensor or a non-zero status raises immediately (the CPU restatement under oracle/ is
test infrastructure and is never imported from here).
"""
import ctypes as C
import os
import re
import weakref

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PCOPS_LIB") or os.path.join(_HERE, "libpcops.so")      # PCOPS_LIB: A/B runs of two builds

_I, _F, _P, _U64, _LL = C.c_int, C.c_float, C.c_void_p, C.c_ulonglong, C.c_longlong
ABI_VERSION = 4      # pcops_abi_version() of the library this binding matches (include/pcops.h), checked in load()

HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "pcops.h")


class PcopsError(RuntimeError):
    pass


_SCALARS = {"int": _I, "float": _F, "long long": _LL, "unsigned long long": _U64}


def _ctype(decl, fn):
    """ctypes type of one parameter or return type of include/pcops.h: any pointer is a c_void_p, a scalar is looked
    up with and then without a trailing parameter name; anything else is refused (a guessed width would pass the wrong
    arguments silently)"""
    if "*" in decl:
        return _P
    words = [w for w in decl.split() if w != "const"]
    for ws in (words, words[:-1]):
        if " ".join(ws) in _SCALARS:
            return _SCALARS[" ".join(ws)]
    raise PcopsError("include/pcops.h: no ctypes mapping for '%s' in the declaration of %s" % (decl, fn))


def parse_header(text):
    """(SIGNATURES, PLAIN) from the text of include/pcops.h: every `ret pcops_name(args);` outside comments,
    preprocessor lines and typedefs.  SIGNATURES: name -> (argtypes without the trailing stream, True) for the entry
    points whose last parameter is a pcops_stream_t (they return a status); PLAIN: name -> (argtypes, restype)."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    text = re.sub(r"\btypedef\b[^;{]*\{[^}]*\}[^;]*;", " ", text)      # struct / enum bodies
    text = re.sub(r"\btypedef\b[^;{]*;", " ", text)
    signatures, plain = {}, {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split()).lstrip("} ")                      # (the closing brace of extern "C")
        if not stmt:
            continue
        m = re.fullmatch(r"(.*?)\b(pcops_\w+) ?\((.*)\)", stmt)
        if not m:
            raise PcopsError("include/pcops.h: cannot read the declaration '%s'" % stmt)
        ret, name, params = m.group(1).strip(), m.group(2), [a.strip() for a in m.group(3).split(",")]
        if params == ["void"] or params == [""]:
            params = []
        has_stream = bool(params) and params[-1].split()[0] == "pcops_stream_t"
        argtypes = [_ctype(a, name) for a in (params[:-1] if has_stream else params)]
        if ret == "void":
            restype = None
        elif ret.replace(" ", "") == "constchar*":
            restype = C.c_char_p
        elif "*" in ret:
            raise PcopsError("include/pcops.h: no ctypes mapping for the return type '%s' of %s" % (ret, name))
        else:
            restype = _ctype(ret, name)
        if has_stream:
            if restype is not _I:
                raise PcopsError("include/pcops.h: %s takes a stream but does not return a status" % name)
            signatures[name] = (argtypes, True)
        else:
            plain[name] = (argtypes, restype)
    return signatures, plain


# name -> (argtypes without the trailing stream, has_stream)  /  name -> (argtypes, restype): read from the header, the
# one place an entry point's signature is written down
with open(HEADER_PATH) as _f:
    SIGNATURES, PLAIN = parse_header(_f.read())


class GemmProblem(C.Structure):
    """pcops_gemm_problem_t: one product C = op(A) op(B) + bias (+ column sums of op(B)) of pcops_small_gemm_pair"""
    _fields_ = [("M", C.c_int), ("K", C.c_int), ("N", C.c_int), ("A", C.c_void_p), ("lda", C.c_int), ("transA", C.c_int),
                ("B", C.c_void_p), ("ldb", C.c_int), ("transB", C.c_int), ("bias", C.c_void_p), ("C", C.c_void_p),
                ("ldc", C.c_int), ("colsum", C.c_void_p)]


def small_gemm_pair(p0, p1):
    """two independent small products in one launch; p = (M, K, N, A, lda, transA, B, ldb, transB, bias, C, ldc, colsum) with device
    pointers as integers or None"""
    arr = (GemmProblem * 2)(GemmProblem(*p0), GemmProblem(*p1))
    lib = load()
    stream = torch.cuda.current_stream().cuda_stream
    shape = tuple(int(v) for v in p0[:3]) + tuple(int(v) for v in p1[:3])     # what a profiling hook sees of the launch
    for h in _hooks:
        h("pcops_small_gemm_pair", "pre", shape)
    status = lib.pcops_small_gemm_pair(arr, stream)
    for h in _hooks:
        h("pcops_small_gemm_pair", "post", shape)
    if status != 0:
        raise PcopsError("pcops_small_gemm_pair failed: %s (status %d)" % (strerror(status), status))


class RowsT(C.Structure):
    """pcops_rows_t: device pointers of a compacted row set (blocks, block_start, rows)"""
    _fields_ = [("blocks", C.c_void_p), ("block_start", C.c_void_p), ("rows", C.c_void_p)]


class Rows:
    """A compacted row set of one grouped stack (pcops.h "compacted rows"): owns the three device buffers and the
    host-side struct the *_rows entry points take."""
    by_struct = weakref.WeakValueDictionary()

    def __init__(self, pts_cnt, nsample):
        b, m = pts_cnt.shape
        lib = load()
        nb = int(lib.pcops_rows_max_blocks(b, m, int(nsample)))
        dev = pts_cnt.device
        self.blocks = torch.empty((nb, 4), dtype=torch.int32, device=dev)
        self.block_start = torch.empty(b * m + 1, dtype=torch.int32, device=dev)
        self.rows = torch.empty(1, dtype=torch.int32, device=dev)
        call("pcops_rows_plan", b, m, int(nsample), pts_cnt.data_ptr(), self.blocks.data_ptr(),
             self.block_start.data_ptr(), self.rows.data_ptr())
        self.struct = RowsT(self.blocks.data_ptr(), self.block_start.data_ptr(), self.rows.data_ptr())
        self.full_rows = b * m * int(nsample)
        Rows.by_struct[id(self.struct)] = self          # lets a profiling hook find the owner of a byref() argument

    def num_rows(self):
        """rows actually computed (device -> host copy: profiling / tests only)"""
        return int(self.rows.item())

    @property
    def ref(self):
        return C.byref(self.struct)


_lib = None


def load():
    """dlopen libpcops.so; raises if it has not been built (python __graft_entry__.py)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PcopsError(
            "libpcops.so is missing (%s). Build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C scanobjectnn_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (argtypes, _) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = list(argtypes) + [_P]
        fn.restype = _I
    for name, (argtypes, restype) in PLAIN.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = restype
    got = int(lib.pcops_abi_version())
    if got != ABI_VERSION:
        # the signatures are the header's, not the library's: a stale or newer library would take the wrong arguments
        # SILENTLY (round 3 inserted stat_pivot mid-signature in five entry points) -- refuse it instead
        raise PcopsError("%s reports ABI version %d, this binding is written for %d: rebuild it "
                         "(make -C scanobjectnn_amd/csrc)" % (LIB_PATH, got, ABI_VERSION))
    _lib = lib
    return lib


def strerror(status):
    return load().pcops_strerror(int(status)).decode()


def ptr(t):
    """device pointer of a tensor that already passed check()"""
    return t.data_ptr() if t is not None else None


def check(t, dtype, name, ndim=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise PcopsError("%s is on %s: pcops ops run on the MI355X only (no CPU fallback)"
                         % (name, t.device))
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if ndim is not None and t.dim() != ndim:
        raise ValueError("%s must have rank %d, got shape %s" % (name, ndim, tuple(t.shape)))
    return t.contiguous()


OPT_GEMM_SPLIT_BF16, OPT_WGRAD_SPLIT_BF16, OPT_BWD_FUSED_DX_SPLIT_BF16, OPT_KNN_F16_PREFILTER = 1, 2, 3, 4
OPT_DGRAD_SPLIT_BF16, OPT_BWD_FUSED_GRAM_WGRAD = 5, 6            # round 6
OPT_SCATTER_QFORM = 7                                            # pcops_sa_scatter_bwd(_rows): Q form of the chunked walk
OPT_XYZ_STATS_MOMENTS = 8                                        # pcops_sa_gather_fwd(_rows): arithmetic first layer's statistics
OPT_GRAM_SPLIT_BF16 = 9                                          # pcops_mlp_gram_rows at Kp == 128: split operands on the bf16 pipe
OPT_POOL_TOP_ROWS_PIPELINED = 10                                 # pcops_mlp_pool_top_wsparse_rows: software-pipelined kernel
OPT_XCONV_CHANNEL_GROUPS = 11                                    # pcops_xconv_fwd / _dgrad_ws: channel tiles of a wide layer over the grid


def set_option(option, value):
    """pcops_set_option (pcops.h "Arithmetic options"); returns the previous value"""
    prev = int(load().pcops_set_option(int(option), int(value)))
    if prev < 0:
        raise PcopsError("pcops_set_option(%d, %d): %s" % (option, value, strerror(prev)))
    return prev


def get_option(option):
    return int(load().pcops_get_option(int(option)))


def set_deterministic(on=True):
    """Bit-reproducible backward passes (pcops.h "deterministic backward passes"): every scatter-add is taken by one
    owner in ascending row order.  Process-wide; PCOPS_DETERMINISTIC=1 in the environment sets it at load time."""
    load().pcops_set_deterministic(1 if on else 0)


def deterministic():
    return bool(load().pcops_get_deterministic())


def scatter_rows_sorted_supported(rows, ndst):
    """the launcher's own predicate (LDS-resident counting sort: ndst <= 19 968, rows < 2^30): callers that may use
    the atomic form instead ask before choosing the ordered one"""
    return bool(load().pcops_scatter_rows_sorted_supported(int(rows), int(ndst)))


def scatter_rows_sorted(idx, src, ndst, div=1, w=None, out=None, c=None, ld=None, src_ptr=None):
    """out (B, ndst, C) = ordered scatter-add of the rows of src (pcops_scatter_rows_sorted).  idx (B, rows) int32;
    src (B, rows / div, C) unless c / ld / src_ptr describe a strided view; out given -> accumulate."""
    b, rows = idx.shape[0], idx[0].numel()
    if not scatter_rows_sorted_supported(rows, ndst):
        raise PcopsError("ordered scatter-add (deterministic backward): %d destination points per cloud, the limit is "
                         "%d (the per-cloud counting sort lives in LDS); rows %d must stay below 2^30.  Switch "
                         "deterministic mode off for clouds this large." % (ndst, load().pcops_scatter_rows_sorted_max_ndst(), rows))
    if c is None:
        c, ld = src.shape[-1], src.shape[-1]
    acc = out is not None
    if out is None:
        out = torch.empty((b, ndst, c), dtype=torch.float32, device=idx.device)
    ws = torch.empty(int(load().pcops_scatter_rows_workspace_bytes(b, rows, ndst)) // 8 + 1, dtype=torch.int64,
                     device=idx.device)
    call("pcops_scatter_rows_sorted", b, rows, ndst, c, div, ld, idx.data_ptr(), ptr(w),
         src_ptr if src_ptr is not None else src.data_ptr(), out.data_ptr(), 1 if acc else 0, ws.data_ptr())
    return out


def scatter_grouped(dfg, idx, n):
    """dfeat (B,N,C) = the scatter-add of dfeat_grouped (B,M,k,C) through idx (B,M,k) (pcops_group_point_grad's
    contract; the ordered owner walk in deterministic mode).  Shared by the SpiderConv and X-Conv backward passes."""
    b, m, k, c = dfg.shape
    if deterministic():
        return scatter_rows_sorted(idx.view(b, m * k), dfg.view(b, m * k, c), n)
    out = torch.empty((b, n, c), dtype=torch.float32, device=dfg.device)
    call("pcops_group_point_grad", b, n, c, m, k, dfg.data_ptr(), idx.data_ptr(), out.data_ptr())
    return out


_SYNC_EVERY_CALL = os.environ.get("PCOPS_SYNC", "0") == "1"
_hooks = []  # profiling hooks: callables (name, phase, args) with phase in {"pre", "post"}


def call(name, *args):
    """Invoke a stream-taking entry point on torch's current HIP stream."""
    lib = load()
    stream = torch.cuda.current_stream().cuda_stream
    for h in _hooks:
        h(name, "pre", args)
    status = getattr(lib, name)(*args, stream)
    for h in _hooks:
        h(name, "post", args)
    if _SYNC_EVERY_CALL and status == 0:      # debugging aid (PCOPS_SYNC=1): a device fault is reported at its launch
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            raise PcopsError("%s: device fault (%s)" % (name, e))
    if status != 0:
        raise PcopsError("%s failed: %s (status %d)" % (name, strerror(status), status))
