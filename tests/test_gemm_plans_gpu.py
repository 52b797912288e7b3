"""Every variant of the MLP product kernels (csrc/mlp.hip: ws_plan / launch_gemm / wgrad_impl / bwd_fused_launch) held to a
float64 reference element by element, with the variant each case ran read back from the library (pcops_last_launch_plan).

The case table is written from the plan rules, not from the models' shapes: both sides of M = 8192 (tiled / wave-stream),
K % 8 and K against 192 / 256 (weights resident or streamed), N in the bands <= 64, 65..96, > 96 (64-, 96-, 128-column
tiles), strided and misaligned operands, ragged row tails, whole-tile / s4 / arbitrary pooling groups, every value of each
per-call option.  Each case also checks the memory contract no model-level test sees: outputs are prefilled with NaN and
must come back finite (all pcops_mlp_stats_rows(M) rows of stats_partial included: rows a kernel does not emit are zeroed),
guard bands before and after every output must come back bit-identical, and the padding columns of a strided input are NaN.

Per-element bound.  The operand is formed the way the kernel forms it (fp32 fmaf), the product is taken in float64, and for
every output element
    |out - ref| <= C * (L + 4) * 2^-24 * (|A| @ |B|)_ij + tiny
with L the length of the sum.  An fp32 sum of L products in any order is within (L - 1) 2^-24 of sum |a b|; the three-piece
bf16 split represents each factor to 2^-24 relative and drops products of that order, which adds at most 2 units per term,
covered by the + 4.  The second unit of C = 2 pays for the operands torch cannot round exactly like the kernel's fmaf
(the prologue relu(fma(x, s, b)) is formed in float64 and rounded once, which may differ from the fmaf by one unit; the data
gradient p.G + q.Y + t is bounded with |A| built from the absolute values of its terms).  A dropped row, a swapped column
block or a wrong group breaks the bound by orders of magnitude; a missing split piece (2^-16 relative) breaks the
relative-RMS bar kept beside it.
"""
import ctypes

import pytest
import torch

from scanobjectnn_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
C_BOUND = 2.0
RMS_BAR = 1e-6            # relative RMS against float64; the kernels measure 5e-8 .. 5e-7 (pcops.h ARITHMETIC notes)
GUARD = 64                # floats of guard band on each side of an output
PATTERN = 0x5A5A5A5A      # guard bit pattern (a finite float no kernel writes by chance)
OK, UNSUPPORTED = 0, -4

# variant tuples (pcops.h pcops_last_launch_plan): (path, split, bn, wst, pool)
OBSERVED = {"fwd": set(), "fwd_pool": set(), "dgrad": set(), "wgrad": set(), "bwd_fused": set()}


def plan():
    out = (ctypes.c_int * 5)()
    assert _lib.load().pcops_last_launch_plan(out, 5) == 5
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- buffers
class Out:
    """an output inside a larger buffer at a 16-byte-aligned offset (+ off floats), guard bands filled with PATTERN,
    the output itself with NaN (0xff for bytes)"""

    def __init__(self, shape, dtype=torch.float32, off=0):
        n = 1
        for s in shape:
            n *= s
        self.n, self.lo = n, GUARD + off
        self.base = torch.empty(n + 2 * GUARD + off, dtype=dtype, device=DEV)
        if dtype == torch.float32:
            self.base.view(torch.int32).fill_(PATTERN)
        else:
            self.base.fill_(0xA5)
        self.t = self.base[self.lo:self.lo + n].view(*shape)
        self.t.fill_(float("nan") if dtype == torch.float32 else 0xFF)
        self.ref = self.base.clone()

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        a, b = self.base, self.ref
        if a.dtype == torch.float32:
            a, b = a.view(torch.int32), b.view(torch.int32)
        return torch.equal(a[:self.lo], b[:self.lo]) and torch.equal(a[self.lo + self.n:], b[self.lo + self.n:])

    def untouched(self):
        a, b = self.base, self.ref
        if a.dtype == torch.float32:
            a, b = a.view(torch.int32), b.view(torch.int32)
        return torch.equal(a, b)


def placed(t, off):
    """a copy of t starting `off` floats past a 16-byte boundary"""
    base = torch.empty(t.numel() + 4, dtype=t.dtype, device=DEV)
    v = base[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _rand(g, *shape):
    return torch.randn(*shape, generator=g, device=g.device).to(DEV)


def _vec(n, g, lo=0.5, neg=True):
    s = (1.0 - 2.0 * (torch.arange(n, device=g.device) % 3 == 1)) if neg else 1.0
    return ((lo + torch.rand(n, generator=g, device=g.device)) * s).to(DEV)


def check_elementwise(out, ref, bound, what):
    out = out.double()
    assert torch.isfinite(out).all(), "%s: non-finite output" % what
    err = (out - ref).abs()
    lim = C_BOUND * bound + 1e-30
    bad = err > lim
    assert not bad.any(), "%s: %d elements outside the bound, worst err/bound %.3g at %s" % (
        what, int(bad.sum()), (err / lim).max().item(), tuple(torch.nonzero(bad)[0].tolist()))
    rms = ((err ** 2).mean().sqrt() / (ref ** 2).mean().sqrt().clamp_min(1e-300)).item()
    assert rms <= RMS_BAR, "%s: relative RMS %.3g" % (what, rms)


def with_option(opt, value, fn):
    prev = _lib.set_option(opt, value)
    try:
        return fn()
    finally:
        _lib.set_option(opt, prev)


def prologue(X, sc, sh):
    """A = relu(fmaf(x, s, b)) as the kernel forms it (float64 product, one rounding), and |A|'s bound: |x s| + |b| where
    the pre-activation is not clearly negative (a fmaf that rounds across 0 then stays inside the bound)"""
    x = X.double()
    pre = x * sc.double() + sh.double()
    A = pre.float().double().clamp_min(0.0)
    mag = (x * sc.double()).abs() + sh.double().abs()
    Aabs = torch.where(pre > -4 * U * mag, mag, torch.zeros_like(mag))
    return A, Aabs


def dy_operand(M, K, G, Y, p, q, t, gpool=None, argmax=None, S=1):
    """dY = p.G + q.Y + t (G dense, or the pooled rows: gpool[g, c] at row g S + argmax[g, c]) and its |terms| bound"""
    Gd = G.double() if gpool is None else None
    if gpool is not None:
        ng = M // S
        Gd = torch.zeros(ng, S, K, dtype=torch.float64, device=DEV)
        Gd.scatter_(1, argmax.long().unsqueeze(1), gpool.double().unsqueeze(1))
        Gd = Gd.view(M, K)
    pd, qd, td = p.double(), q.double(), t.double()
    dY = pd * Gd + qd * Y.double() + td
    dYabs = pd.abs() * Gd.abs() + qd.abs() * Y.double().abs() + td.abs()
    return dY, dYabs


# ---------------------------------------------------------------------------------------------------------------- forward
# (name, M, K, N, ldx, off_X, off_W, off_Y, prologue, stats, pivot)
FWD_CASES = [
    ("tiled_below_8192", 8191, 64, 64, 64, 0, 0, 0, True, True, True),
    ("ws_at_8192", 8192, 64, 64, 64, 0, 0, 0, True, True, False),
    ("k8_tail1", 8192 + 32 * 7 + 1, 8, 64, 8, 0, 0, 0, True, True, True),
    ("k40_n32_tail17", 8192 + 17, 40, 32, 40, 0, 0, 0, False, True, False),
    ("n68_bn96", 9000 + 31 - 9000 % 32, 96, 68, 96, 0, 0, 0, True, True, True),
    ("n96", 8192 + 1, 64, 96, 64, 0, 0, 0, True, False, False),
    ("n100_bn128", 8192 + 17, 128, 100, 128, 0, 0, 0, True, True, True),
    ("k128_n128", 8192 + 31, 128, 128, 128, 0, 0, 0, False, True, False),
    ("k192_n132", 8192 + 17, 192, 132, 192, 0, 0, 0, True, True, True),
    ("k200_stream", 8192 + 1, 200, 128, 200, 0, 0, 0, True, True, False),
    ("k256_n256", 8192 + 31, 256, 256, 256, 0, 0, 0, True, True, True),
    ("k264_n64", 8192 + 17, 264, 64, 264, 0, 0, 0, True, True, False),
    ("k320_n4", 8192, 320, 4, 320, 0, 0, 0, False, True, True),
    ("k1024_n1024", 8192 + 17, 1024, 1024, 1024, 0, 0, 0, True, True, False),
    ("k132_large_m", 65536 + 1, 132, 64, 132, 0, 0, 0, True, True, True),
    ("ldx72", 8192 + 17, 64, 128, 72, 0, 0, 0, True, True, False),
    ("ldx66_odd", 8192 + 17, 64, 64, 66, 0, 0, 0, True, True, False),
    ("x_off1", 8192 + 1, 64, 128, 64, 1, 0, 0, True, True, False),
    ("w_off1_k64", 8192 + 1, 64, 128, 64, 0, 1, 0, True, True, False),
    ("w_off1_k264", 8192 + 1, 264, 64, 264, 0, 1, 0, True, True, False),
    ("y_off1", 8192 + 17, 64, 64, 64, 0, 0, 1, True, True, False),
]


def _fwd_run(case, opt):
    name, M, K, N, ldx, ox, ow, oy, pro, stats, pivot = case
    g = torch.Generator(device=DEV).manual_seed(M * 7 + K * 3 + N)
    lib = _lib.load()
    Xs = _rand(g, M, ldx)
    if ldx > K:
        Xs[:, K:] = float("nan")                       # padding columns are never read
    X = placed(Xs, ox)
    W = placed((_rand(g, K, N) / K ** 0.5), ow)
    bias = (0.1 * _rand(g, N))
    sc, sh = (_vec(K, g), 0.3 * _rand(g, K)) if pro else (None, None)
    piv = (0.05 * _rand(g, N)) if pivot else None
    P = lib.pcops_mlp_stats_rows(M)
    Y = Out((M, N), off=oy)
    part = Out((P, 2, N)) if stats else None

    def go():
        rc = lib.pcops_mlp_gemm_fwd(M, K, N, X.data_ptr(), ldx, sc.data_ptr() if pro else None,
                                    sh.data_ptr() if pro else None, W.data_ptr(), bias.data_ptr(), Y.ptr(),
                                    part.ptr() if stats else None, piv.data_ptr() if pivot else None,
                                    torch.cuda.current_stream().cuda_stream)
        return rc, plan()

    rc, pl = with_option(_lib.OPT_GEMM_SPLIT_BF16, opt, go)
    assert rc == OK
    torch.cuda.synchronize()
    Xk = Xs[:, :K]
    if pro:
        A, Aabs = prologue(Xk, sc, sh)
    else:
        A, Aabs = Xk.double(), Xk.double().abs()
    Wd = W.double()
    ref = A @ Wd + bias.double()
    bound = (K + 4) * U * (Aabs @ Wd.abs() + bias.double().abs())
    check_elementwise(Y.t, ref, bound, "fwd %s opt %d" % (name, opt))
    assert Y.guards_intact(), "fwd %s: a write outside Y" % name
    if stats:
        assert torch.isfinite(part.t).all(), "fwd %s: stats rows not written / zeroed" % name
        assert part.guards_intact(), "fwd %s: a write outside stats_partial" % name
        Yd = Y.t.double() - (piv.double() if pivot else 0.0)
        for which, val in ((0, Yd), (1, Yd * Yd)):
            got = part.t[:, which].double().sum(0)
            want = val.sum(0)
            lim = 3e-5 * val.abs().sum(0) + 1e-30
            assert ((got - want).abs() <= lim).all(), "fwd %s: statistics %d" % (name, which)
    return pl


# the variant ws_plan gives each case under option 0 / 1 / 2 of PCOPS_OPT_GEMM_SPLIT_BF16
FWD_EXPECT = {
    "tiled_below_8192": [(1, 0, 0, 0, 0), (1, 0, 0, 0, 0), (1, 0, 0, 0, 0)],
    "ws_at_8192":       [(2, 0, 64, 0, 0), (2, 1, 64, 0, 0), (2, 1, 64, 0, 0)],
    "k8_tail1":         [(2, 0, 64, 0, 0), (2, 1, 64, 0, 0), (2, 1, 64, 0, 0)],
    "k40_n32_tail17":   [(2, 0, 64, 0, 0), (2, 1, 64, 0, 0), (2, 1, 64, 0, 0)],
    "n68_bn96":         [(2, 0, 96, 0, 0), (2, 1, 96, 0, 0), (2, 1, 96, 0, 0)],
    "n96":              [(2, 0, 96, 0, 0), (2, 1, 96, 0, 0), (2, 1, 96, 0, 0)],
    "n100_bn128":       [(2, 0, 128, 0, 0), (2, 1, 128, 0, 0), (2, 1, 128, 0, 0)],
    "k128_n128":        [(2, 0, 128, 0, 0), (2, 1, 128, 0, 0), (2, 1, 128, 0, 0)],
    "k192_n132":        [(2, 0, 128, 1, 0), (2, 1, 128, 1, 0), (2, 0, 128, 1, 0)],
    "k200_stream":      [(2, 0, 128, 1, 0), (2, 1, 128, 1, 0), (2, 0, 128, 1, 0)],
    "k256_n256":        [(2, 0, 128, 1, 0), (2, 1, 128, 1, 0), (2, 0, 128, 1, 0)],
    "k264_n64":         [(2, 0, 64, 1, 0), (2, 1, 64, 0, 0), (2, 1, 64, 0, 0)],
    "k320_n4":          [(2, 0, 64, 1, 0), (2, 1, 64, 1, 0), (2, 0, 64, 1, 0)],
    "k1024_n1024":      [(2, 0, 128, 1, 0), (2, 1, 128, 1, 0), (2, 0, 128, 1, 0)],
    "k132_large_m":     [(1, 0, 0, 0, 0), (1, 0, 0, 0, 0), (1, 0, 0, 0, 0)],
    "ldx72":            [(2, 0, 128, 0, 0), (2, 1, 128, 0, 0), (2, 1, 128, 0, 0)],
    "ldx66_odd":        [(1, 0, 0, 0, 0), (1, 0, 0, 0, 0), (1, 0, 0, 0, 0)],
    "x_off1":           [(1, 0, 0, 0, 0), (1, 0, 0, 0, 0), (1, 0, 0, 0, 0)],
    "w_off1_k64":       [(2, 0, 128, 0, 0), (2, 1, 128, 0, 0), (2, 1, 128, 0, 0)],
    "w_off1_k264":      [(1, 0, 0, 0, 0), (1, 0, 0, 0, 0), (1, 0, 0, 0, 0)],
    "y_off1":           [(1, 0, 0, 0, 0), (1, 0, 0, 0, 0), (1, 0, 0, 0, 0)],
}


@pytest.mark.parametrize("opt", [0, 1, 2])
@pytest.mark.parametrize("case", FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_fwd(case, opt):
    pl = _fwd_run(case, opt)
    OBSERVED["fwd"].add(pl)
    assert pl == FWD_EXPECT[case[0]][opt], (case[0], opt, pl)


# ---------------------------------------------------------------------------------------------------------- pooled forward
# (name, M, K, N, S, prologue, store Y) -- whole tiles (S % 32 == 0), s4 groups (S % 4 == 0, lcm(S, 32) <= 256), refused S
POOL_CASES = [
    ("s32", 32 * 300, 64, 128, 32, True, True),
    ("s64_noY", 64 * 140, 128, 64, 64, True, False),
    ("s256", 256 * 33, 64, 96, 256, True, True),
    ("s12", 96 * 90, 64, 64, 12, True, True),
    ("s16", 32 * 260, 40, 128, 16, True, True),
    ("s20_noY", 160 * 55, 64, 128, 20, False, False),
    ("s48", 96 * 90, 96, 68, 48, True, True),
    ("s36_refused", 288 * 30, 64, 64, 36, True, True),
    ("s10_refused", 10 * 900, 64, 64, 10, True, True),
]
POOL_EXPECT = {
    "s32":         [(2, 0, 128, 0, 1), (2, 1, 128, 0, 1), (2, 1, 128, 0, 1)],
    "s64_noY":     [(2, 0, 64, 0, 1), (2, 1, 64, 0, 1), (2, 1, 64, 0, 1)],
    "s256":        [(2, 0, 96, 0, 1), (2, 1, 96, 0, 1), (2, 1, 96, 0, 1)],
    "s12":         [None, (2, 1, 64, 0, 3), (2, 1, 64, 0, 3)],
    "s16":         [None, (2, 1, 128, 0, 3), (2, 1, 128, 0, 3)],
    "s20_noY":     [None, (2, 1, 128, 0, 3), (2, 1, 128, 0, 3)],
    "s48":         [None, (2, 1, 96, 0, 3), (2, 1, 96, 0, 3)],
    "s36_refused": [None, None, None],
    "s10_refused": [None, None, None],
}


def _tied_rows(X, S):
    """duplicated rows inside every group: even groups are S copies of their first row (every row ties), odd groups repeat
    rows 0 and 1 at S - 1 and S / 2 -- the arg row must be the FIRST that attains the extreme"""
    ng = X.shape[0] // S
    Xg = X.view(ng, S, -1)
    Xg[0::2] = Xg[0::2, :1].clone()
    Xg[1::2, S - 1] = Xg[1::2, 0]
    Xg[1::2, S // 2] = Xg[1::2, 1]
    return X


def _pool_run(case, opt):
    name, M, K, N, S, pro, storeY = case
    g = torch.Generator(device=DEV).manual_seed(M + 11 * S + N)
    lib = _lib.load()
    X = _tied_rows(_rand(g, M, K), S)
    W = _rand(g, K, N) / K ** 0.5
    bias = 0.1 * _rand(g, N)
    gamma = _vec(N, g)                                 # every third channel negative: its group MINIMUM is selected
    sc, sh = (_vec(K, g), 0.3 * _rand(g, K)) if pro else (None, None)
    ng = M // S
    P = lib.pcops_mlp_stats_rows(M)
    Y = Out((M, N)) if storeY else None
    part = Out((P, 2, N))
    ysel, argsel = Out((ng, N)), Out((ng, N), dtype=torch.uint8)
    supported = lib.pcops_mlp_gemm_fwd_pool_supported(M, K, N, S)

    def go():
        rc = lib.pcops_mlp_gemm_fwd_pool(M, K, N, S, X.data_ptr(), K, sc.data_ptr() if pro else None,
                                         sh.data_ptr() if pro else None, W.data_ptr(), bias.data_ptr(), gamma.data_ptr(),
                                         Y.ptr() if storeY else None, part.ptr(), None, ysel.ptr(), argsel.ptr(),
                                         torch.cuda.current_stream().cuda_stream)
        return rc, plan(), lib.pcops_mlp_gemm_fwd_pool_supported(M, K, N, S)

    rc, pl, supported = with_option(_lib.OPT_GEMM_SPLIT_BF16, opt, go)
    torch.cuda.synchronize()
    outs = [o for o in (Y, part, ysel, argsel) if o is not None]
    if not supported:
        assert rc == UNSUPPORTED, (name, opt, rc)
        assert all(o.untouched() for o in outs), "fwd_pool %s: refused, yet wrote" % name
        return None
    assert rc == OK, (name, opt, rc)
    assert all(o.guards_intact() for o in outs), "fwd_pool %s: a write outside an output" % name
    A, Aabs = prologue(X, sc, sh) if pro else (X.double(), X.double().abs())
    ref = A @ W.double() + bias.double()
    bound = (K + 4) * U * (Aabs @ W.double().abs() + bias.double().abs())
    am = argsel.t.long()
    assert (am < S).all(), "fwd_pool %s: arg row outside its group" % name
    rows = am + (torch.arange(ng, device=DEV) * S).unsqueeze(1)
    if storeY:
        check_elementwise(Y.t, ref, bound, "fwd_pool %s opt %d" % (name, opt))
        Yg = Y.t.view(ng, S, N)
        assert torch.equal(ysel.t, torch.gather(Y.t, 0, rows)), "fwd_pool %s: ysel is not Y at the arg row" % name
        ext = torch.where(gamma >= 0, Yg.max(1).values, Yg.min(1).values)
        first = (Yg == ext.unsqueeze(1)).to(torch.int32).argmax(1)          # the FIRST row attaining it (ties)
        assert torch.equal(am, first.long()), "fwd_pool %s: not the first extreme row" % name
        Ysum = Y.t.double()
    else:
        # no Y to judge on: the selected value is the reference's at the arg row, and no row of the group is beyond it
        check_elementwise(ysel.t, torch.gather(ref, 0, rows), torch.gather(bound, 0, rows), "fwd_pool ysel %s" % name)
        refg, bg = ref.view(ng, S, N), C_BOUND * bound.view(ng, S, N)
        sel = torch.gather(ref, 0, rows).unsqueeze(1)
        slack = 2 * bg.max(1, keepdim=True).values + 1e-30
        beyond = torch.where(gamma >= 0, refg > sel + slack, refg < sel - slack)
        assert not beyond.any(), "fwd_pool %s: a row beyond the selected extreme" % name
        Ysum = ref
    assert torch.isfinite(part.t).all(), "fwd_pool %s: stats rows not written / zeroed" % name
    for which, val in ((0, Ysum), (1, Ysum * Ysum)):
        got, want = part.t[:, which].double().sum(0), val.sum(0)
        lim = 3e-5 * val.abs().sum(0) + (0 if storeY else 4 * C_BOUND * (bound * (Ysum.abs() + 1)).sum(0))
        assert ((got - want).abs() <= lim + 1e-30).all(), "fwd_pool %s: statistics %d" % (name, which)
    return pl


@pytest.mark.parametrize("opt", [0, 1, 2])
@pytest.mark.parametrize("case", POOL_CASES, ids=[c[0] for c in POOL_CASES])
def test_fwd_pool(case, opt):
    pl = _pool_run(case, opt)
    want = POOL_EXPECT[case[0]][opt]
    if pl is not None:
        OBSERVED["fwd_pool"].add(pl)
    assert pl == want, (case[0], opt, pl)


# ----------------------------------------------------------------------------------------------------------- data gradient
# (name, M, K = dY columns, Nout, masked, S (0: dense G), G offset in floats)
DGRAD_CASES = [
    ("tiled_8191", 8191, 64, 64, True, 0, 0),
    ("k64_n128_plain", 8192 + 17, 64, 128, False, 0, 0),
    ("k128_n64", 8192 + 1, 128, 64, True, 0, 0),
    ("k96_n96", 8192 + 31, 96, 96, True, 0, 0),
    ("k256_n128", 8192 + 17, 256, 128, True, 0, 0),
    ("k192_n68_plain", 8192 + 1, 192, 68, False, 0, 0),
    ("k264_n64", 8192 + 17, 264, 64, True, 0, 0),
    ("k200_n100", 8192 + 31, 200, 100, True, 0, 0),
    ("k1024_n132_plain", 8192 + 1, 1024, 132, False, 0, 0),
    ("k8_n32", 8192 + 17, 8, 32, True, 0, 0),
    ("k132_large_m", 65536 + 1, 132, 64, True, 0, 0),
    ("g_off1", 8192 + 17, 64, 64, True, 0, 1),
    ("pool32", 32 * 300, 128, 64, True, 32, 0),
    ("pool64_plain", 64 * 140, 64, 128, False, 64, 0),
    ("pool256", 256 * 33, 64, 64, True, 256, 0),
    ("pool20", 20 * 450, 128, 96, True, 20, 0),
    ("pool12_plain", 12 * 700, 64, 64, False, 12, 0),
    ("pool48", 48 * 180, 256, 128, True, 48, 0),
    ("pool8_tiled", 8 * 1100, 64, 64, True, 8, 0),
]
DGRAD_EXPECT = {
    "tiled_8191":       [(1, 0, 0, 0, 0), (1, 0, 0, 0, 0), (1, 0, 0, 0, 0)],
    "k64_n128_plain":   [(2, 0, 128, 0, 0), (2, 0, 128, 0, 0), (2, 0, 128, 0, 0)],
    "k128_n64":         [(2, 0, 64, 0, 0), (2, 1, 64, 0, 0), (2, 1, 64, 0, 0)],
    "k96_n96":          [(2, 0, 96, 0, 0), (2, 0, 96, 0, 0), (2, 0, 96, 0, 0)],
    "k256_n128":        [(2, 0, 64, 1, 0), (2, 1, 64, 0, 0), (2, 0, 64, 1, 0)],
    "k192_n68_plain":   [(2, 0, 96, 1, 0), (2, 0, 96, 1, 0), (2, 0, 96, 1, 0)],
    "k264_n64":         [(2, 0, 64, 1, 0), (2, 0, 64, 1, 0), (2, 0, 64, 1, 0)],
    "k200_n100":        [(2, 0, 64, 1, 0), (2, 0, 64, 1, 0), (2, 0, 64, 1, 0)],
    "k1024_n132_plain": [(2, 0, 128, 1, 0), (2, 0, 128, 1, 0), (2, 0, 128, 1, 0)],
    "k8_n32":           [(2, 0, 64, 0, 0), (2, 0, 64, 0, 0), (2, 0, 64, 0, 0)],
    "k132_large_m":     [(1, 0, 0, 0, 0), (1, 0, 0, 0, 0), (1, 0, 0, 0, 0)],
    "g_off1":           [(1, 0, 0, 0, 0), (1, 0, 0, 0, 0), (1, 0, 0, 0, 0)],
    "pool32":           [(2, 0, 64, 0, 1), (2, 1, 64, 0, 1), (2, 1, 64, 0, 1)],
    "pool64_plain":     [(2, 0, 128, 0, 1), (2, 0, 128, 0, 1), (2, 0, 128, 0, 1)],
    "pool256":          [(2, 0, 64, 0, 1), (2, 0, 64, 0, 1), (2, 0, 64, 0, 1)],
    "pool20":           [(2, 0, 96, 0, 2), (2, 1, 96, 0, 2), (2, 1, 96, 0, 2)],
    "pool12_plain":     [(2, 0, 64, 0, 2), (2, 0, 64, 0, 2), (2, 0, 64, 0, 2)],
    "pool48":           [(2, 0, 64, 1, 2), (2, 1, 64, 0, 2), (2, 0, 64, 1, 2)],
    "pool8_tiled":      [(1, 0, 0, 0, 2), (1, 0, 0, 0, 2), (1, 0, 0, 0, 2)],
}


def _masked_prev(g, M, Nout):
    """Yprev with every pre-activation relu(sc Yprev + sh) at least 1e-3 away from 0 (the mask does not depend on rounding)"""
    sc, sh = _vec(Nout, g), 0.3 * _rand(g, Nout)
    pre = (0.002 + torch.rand(M, Nout, generator=g, device=g.device).to(DEV)) * torch.where(_rand(g, M, Nout) > 0, 1.0, -1.0)
    Yprev = ((pre.double() - sh.double()) / sc.double()).float()
    assert ((Yprev.double() * sc.double() + sh.double()).abs() > 1e-3).all()
    return Yprev, sc, sh


def _pooled_grad(g, M, K, S):
    gpool = _rand(g, M // S, K)
    gpool[torch.rand(M // S, K, generator=g, device=g.device).to(DEV) < 0.3] = 0.0
    argmax = torch.randint(0, S, (M // S, K), generator=g, device=g.device, dtype=torch.int32).to(torch.uint8).to(DEV)
    return gpool, argmax


def _dgrad_run(case, opt):
    name, M, K, Nout, masked, S, og = case
    g = torch.Generator(device=DEV).manual_seed(M * 5 + K + Nout)
    lib = _lib.load()
    Y = _rand(g, M, K)
    p, q, t = _vec(K, g), 0.1 * _vec(K, g), 0.05 * _rand(g, K)
    Wt = _rand(g, K, Nout) / K ** 0.5
    if S:
        G, (gpool, argmax) = None, _pooled_grad(g, M, K, S)
    else:
        G, gpool, argmax = placed(_rand(g, M, K), og), None, None
    Yprev, sc, sh = _masked_prev(g, M, Nout) if masked else (None, None, None)
    P = lib.pcops_mlp_stats_rows(M)
    Gprev = Out((M, Nout))
    part = Out((P, 2, Nout)) if masked else None

    def ptr(x):
        return None if x is None else x.data_ptr()

    def go():
        rc = lib.pcops_mlp_gemm_dgrad(M, K, Nout, ptr(G), Y.data_ptr(), p.data_ptr(), q.data_ptr(), t.data_ptr(),
                                      ptr(gpool), ptr(argmax), S if S else 1, p.data_ptr() if S else None,
                                      p.data_ptr() if S else None, Wt.data_ptr(), ptr(Yprev), ptr(sc), ptr(sh),
                                      Gprev.ptr(), part.ptr() if masked else None,
                                      torch.cuda.current_stream().cuda_stream)
        return rc, plan()

    rc, pl = with_option(_lib.OPT_DGRAD_SPLIT_BF16, opt, go)
    assert rc == OK, (name, opt, rc)
    torch.cuda.synchronize()
    dY, dYabs = dy_operand(M, K, G, Y, p, q, t, gpool, argmax, S if S else 1)
    ref = dY @ Wt.double()
    bound = (K + 4 + 2) * U * (dYabs @ Wt.double().abs())
    if masked:
        mask = (Yprev.double() * sc.double() + sh.double()) > 0
        ref, bound = ref * mask, bound * mask
    check_elementwise(Gprev.t, ref, bound, "dgrad %s opt %d" % (name, opt))
    assert Gprev.guards_intact(), "dgrad %s: a write outside Gprev" % name
    if masked:
        assert torch.isfinite(part.t).all(), "dgrad %s: stats rows not written / zeroed" % name
        assert part.guards_intact(), "dgrad %s: a write outside stats_partial" % name
        Gd = Gprev.t.double()
        for which, val in ((0, Gd), (1, Gd * Yprev.double())):
            got, want = part.t[:, which].double().sum(0), val.sum(0)
            assert ((got - want).abs() <= 3e-5 * val.abs().sum(0) + 1e-30).all(), "dgrad %s: statistics %d" % (name, which)
    return pl


@pytest.mark.parametrize("opt", [0, 1, 2])
@pytest.mark.parametrize("case", DGRAD_CASES, ids=[c[0] for c in DGRAD_CASES])
def test_dgrad(case, opt):
    pl = _dgrad_run(case, opt)
    OBSERVED["dgrad"].add(pl)
    assert pl == DGRAD_EXPECT[case[0]][opt], (case[0], opt, pl)


# --------------------------------------------------------------------------------------------------------- weight gradient
# (name, M, K, N, ldx, prologue, S)
WGRAD_CASES = [
    ("legacy_8191", 8191, 64, 64, 64, True, 0),
    ("k64_n64", 8192 + 17, 64, 64, 64, True, 0),
    ("k64_n256_plain", 8192 + 1, 64, 256, 64, False, 0),
    ("k128_n128", 32768 + 31, 128, 128, 128, True, 0),
    ("k96_n100", 32768 + 1, 96, 100, 96, True, 0),
    ("k132_n68", 32768 + 17, 132, 68, 132, True, 0),
    ("k66_ldx66", 8192 + 17, 66, 64, 66, False, 0),
    ("ldx72", 8192 + 17, 64, 128, 72, True, 0),
    ("pool32", 32 * 1100, 128, 128, 128, True, 32),
    ("pool20", 20 * 1700, 64, 128, 64, True, 20),
    ("pool12_plain", 12 * 800, 64, 64, 64, False, 12),
    ("pool8_legacy", 8 * 1000, 64, 64, 64, True, 8),
]
WGRAD_EXPECT = {
    "legacy_8191":    [(7, 0, 128, 0, 0), (7, 0, 128, 0, 0)],
    "k64_n64":        [(6, 0, 64, 0, 0), (6, 0, 64, 0, 0)],
    "k64_n256_plain": [(5, 0, 256, 0, 0), (5, 0, 256, 0, 0)],
    "k128_n128":      [(6, 0, 128, 0, 0), (4, 1, 128, 0, 0)],
    "k96_n100":       [(6, 0, 128, 0, 0), (4, 1, 128, 0, 0)],
    "k132_n68":       [(6, 0, 128, 0, 0), (4, 1, 128, 0, 0)],
    "k66_ldx66":      [(7, 0, 128, 0, 0), (7, 0, 128, 0, 0)],
    "ldx72":          [(6, 0, 128, 0, 0), (6, 0, 128, 0, 0)],
    "pool32":         [(5, 0, 128, 0, 1), (4, 1, 128, 0, 1)],
    "pool20":         [(5, 0, 128, 0, 2), (5, 0, 128, 0, 2)],
    "pool12_plain":   [(5, 0, 64, 0, 2), (5, 0, 64, 0, 2)],
    "pool8_legacy":   [(7, 0, 128, 0, 2), (7, 0, 128, 0, 2)],
}


def _wgrad_run(case, opt):
    name, M, K, N, ldx, pro, S = case
    g = torch.Generator(device=DEV).manual_seed(M * 3 + K + N)
    lib = _lib.load()
    Xs = _rand(g, M, ldx)
    if ldx > K:
        Xs[:, K:] = float("nan")
    sc, sh = (_vec(K, g), 0.3 * _rand(g, K)) if pro else (None, None)
    Y = _rand(g, M, N)
    p, q, t = _vec(N, g), 0.1 * _vec(N, g), 0.05 * _rand(g, N)
    if S:
        G, (gpool, argmax) = None, _pooled_grad(g, M, N, S)
    else:
        G, gpool, argmax = _rand(g, M, N), None, None
    splits = lib.pcops_mlp_wgrad_splits(M, K, N)
    scratch = torch.empty(splits * (K * N + N), device=DEV)
    dW, db = Out((K, N)), Out((N,))

    def ptr(x):
        return None if x is None else x.data_ptr()

    def go():
        rc = lib.pcops_mlp_wgrad(M, K, N, Xs.data_ptr(), ldx, ptr(sc), ptr(sh), ptr(G), Y.data_ptr(), p.data_ptr(),
                                 q.data_ptr(), t.data_ptr(), ptr(gpool), ptr(argmax), S if S else 1,
                                 p.data_ptr() if S else None, p.data_ptr() if S else None, scratch.data_ptr(), dW.ptr(),
                                 db.ptr(), torch.cuda.current_stream().cuda_stream)
        return rc, plan()

    rc, pl = with_option(_lib.OPT_WGRAD_SPLIT_BF16, opt, go)
    assert rc == OK, (name, opt, rc)
    torch.cuda.synchronize()
    Xk = Xs[:, :K]
    A, Aabs = prologue(Xk, sc, sh) if pro else (Xk.double(), Xk.double().abs())
    dY, dYabs = dy_operand(M, N, G, Y, p, q, t, gpool, argmax, S if S else 1)
    check_elementwise(dW.t, A.t() @ dY, (M + 4 + 2) * U * (Aabs.t() @ dYabs), "wgrad dW %s opt %d" % (name, opt))
    check_elementwise(db.t, dY.sum(0), (M + 4 + 2) * U * dYabs.sum(0), "wgrad db %s opt %d" % (name, opt))
    assert dW.guards_intact() and db.guards_intact(), "wgrad %s: a write outside dW / db" % name
    return pl


@pytest.mark.parametrize("opt", [0, 1])
@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_wgrad(case, opt):
    pl = _wgrad_run(case, opt)
    OBSERVED["wgrad"].add(pl)
    assert pl == WGRAD_EXPECT[case[0]][opt], (case[0], opt, pl)


# One case per arm of the weight-gradient dispatch (wgrad_launch: family x tile x operand mode x resolved dY mode) that takes
# uncompacted rows and a read operand and that no other test of the suite launches, at the smallest rows the planners admit
# (8 192 for the producer/consumer plan, 32 768 for the split-operand plan), widths from {64, 96, 128, 320}, groups of 32
# (whole tiles) and 20 rows.  Names: pc<tk><tn> the producer/consumer tile (k96: its 96 x 32 consumer layout), bf3 the
# split-operand kernel (which takes a shape under option 1 only: under option 0 the case runs the kernel of its first tuple).
# (name, M, K, N, ldx, prologue, S)
WGRAD_ARM_CASES = [
    ("pc11_plain_s32", 8192, 64, 64, 64, False, 32),
    ("pc11_plain_s20", 8200, 64, 64, 64, False, 20),
    ("pc12_plain_s32", 8192, 64, 128, 64, False, 32),
    ("pc14_bn_s32", 8192, 64, 320, 64, True, 32),
    ("pc14_bn_s20", 8200, 64, 320, 64, True, 20),
    ("pc14_plain_s32", 8192, 64, 320, 64, False, 32),
    ("pc14_plain_s20", 8200, 64, 320, 64, False, 20),
    ("pc21_bn_s20", 8200, 128, 64, 128, True, 20),
    ("pc21_plain_s32", 8192, 128, 64, 128, False, 32),
    ("pc21_plain_s20", 8200, 128, 64, 128, False, 20),
    ("pc22k96_bn_s32", 8192, 96, 128, 96, True, 32),
    ("pc22k96_bn_s20", 8200, 96, 128, 96, True, 20),
    ("pc22k96_plain_s32", 8192, 96, 128, 96, False, 32),
    ("pc22k96_plain_s20", 8200, 96, 128, 96, False, 20),
    ("pc22_bn_s20", 8200, 128, 128, 128, True, 20),
    ("pc22_plain_s32", 8192, 128, 128, 128, False, 32),
    ("pc22_plain_s20", 8200, 128, 128, 128, False, 20),
    ("pc24_bn_s32", 8192, 128, 320, 128, True, 32),
    ("pc24_bn_s20", 8200, 128, 320, 128, True, 20),
    ("pc24_plain_s20", 8200, 128, 320, 128, False, 20),
    ("pc14_bn_dy", 8192, 64, 320, 64, True, 0),
    ("bf3_plain_s32", 32768, 128, 128, 128, False, 32),
    ("bf3_plain_s16", 32768, 128, 128, 128, False, 16),
]
WGRAD_ARM_EXPECT = {
    "pc11_plain_s32": [(5, 0, 64, 0, 1), (5, 0, 64, 0, 1)],
    "pc11_plain_s20": [(5, 0, 64, 0, 2), (5, 0, 64, 0, 2)],
    "pc12_plain_s32": [(5, 0, 128, 0, 1), (5, 0, 128, 0, 1)],
    "pc14_bn_s32": [(5, 0, 256, 0, 1), (5, 0, 256, 0, 1)],
    "pc14_bn_s20": [(5, 0, 256, 0, 2), (5, 0, 256, 0, 2)],
    "pc14_plain_s32": [(5, 0, 256, 0, 1), (5, 0, 256, 0, 1)],
    "pc14_plain_s20": [(5, 0, 256, 0, 2), (5, 0, 256, 0, 2)],
    "pc21_bn_s20": [(5, 0, 64, 0, 2), (5, 0, 64, 0, 2)],
    "pc21_plain_s32": [(5, 0, 64, 0, 1), (5, 0, 64, 0, 1)],
    "pc21_plain_s20": [(5, 0, 64, 0, 2), (5, 0, 64, 0, 2)],
    "pc22k96_bn_s32": [(5, 0, 128, 0, 1), (5, 0, 128, 0, 1)],
    "pc22k96_bn_s20": [(5, 0, 128, 0, 2), (5, 0, 128, 0, 2)],
    "pc22k96_plain_s32": [(5, 0, 128, 0, 1), (5, 0, 128, 0, 1)],
    "pc22k96_plain_s20": [(5, 0, 128, 0, 2), (5, 0, 128, 0, 2)],
    "pc22_bn_s20": [(5, 0, 128, 0, 2), (5, 0, 128, 0, 2)],
    "pc22_plain_s32": [(5, 0, 128, 0, 1), (5, 0, 128, 0, 1)],
    "pc22_plain_s20": [(5, 0, 128, 0, 2), (5, 0, 128, 0, 2)],
    "pc24_bn_s32": [(5, 0, 256, 0, 1), (5, 0, 256, 0, 1)],
    "pc24_bn_s20": [(5, 0, 256, 0, 2), (5, 0, 256, 0, 2)],
    "pc24_plain_s20": [(5, 0, 256, 0, 2), (5, 0, 256, 0, 2)],
    "pc14_bn_dy": [(5, 0, 256, 0, 0), (5, 0, 256, 0, 0)],
    "bf3_plain_s32": [(5, 0, 128, 0, 1), (4, 1, 128, 0, 1)],
    "bf3_plain_s16": [(5, 0, 128, 0, 2), (4, 1, 128, 0, 2)],
}


# (the option decides nothing below 32 768 rows: those cases run under its default only)
WGRAD_ARM_RUNS = [(c, o) for c in WGRAD_ARM_CASES for o in ((0, 1) if c[1] >= 32768 else (1,))]


@pytest.mark.parametrize("case,opt", WGRAD_ARM_RUNS, ids=["%s-%d" % (c[0], o) for c, o in WGRAD_ARM_RUNS])
def test_wgrad_arms(case, opt):
    pl = _wgrad_run(case, opt)
    OBSERVED["wgrad"].add(pl)
    assert pl == WGRAD_ARM_EXPECT[case[0]][opt], (case[0], opt, pl)


# ------------------------------------------------------------------------ one-pass backward: the queries and the launchers
# Each launcher of the family has a query; where the query answers > 0 the launcher must take the shape and compute what
# the two-kernel path computes, where it answers 0 the launcher must refuse and write nothing.  (Before the edge forms had
# a query of their own, pcops_mlp_bwd_fused_gw_groups said yes to S = 32 / 64 and pcops_mlp_bwd_fused_edge_gw refused.)
BF_K, BF_N, BF_M = (48, 64, 68), (64, 96, 128, 132), (65535, 65536)
BF_S = (0, 10, 11, 20, 32, 64, 255, 256)
BF_FORMS = ("plain", "gw", "edge", "edge_gw")


def _bf_query(lib, form, M, K, N, S):
    if form == "plain":
        return lib.pcops_mlp_bwd_fused_groups(M, K, N, S, 1 if S else 0)
    if form == "gw":
        return lib.pcops_mlp_bwd_fused_gw_groups(M, K, N, S)
    return lib.pcops_mlp_bwd_fused_edge_groups(M, K, N, S, 1 if form == "edge_gw" else 0)


def _bf_case(lib, form, M, K, N, S, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    groups = _bf_query(lib, form, M, K, N, S)
    pooled = S > 0
    Yprev, sc, sh = _masked_prev(g, M, K)
    W = _rand(g, K, N) / K ** 0.5
    bias = 0.1 * _rand(g, N)
    A, Aabs = prologue(Yprev, sc, sh)
    if form in ("gw", "edge_gw"):
        Y = (A @ W.double() + bias.double()).float()        # the Gram form substitutes Y = X W + bias: the layer's own output
    else:
        Y = _rand(g, M, N)
    p, q, t = _vec(N, g), 0.1 * _vec(N, g), 0.05 * _rand(g, N)
    ng = (M + S - 1) // S if pooled else 0
    if pooled:
        gpool = _rand(g, ng, N)
        gpool[torch.rand(ng, N, generator=g, device=DEV) < 0.3] = 0.0
        argmax = torch.randint(0, S, (ng, N), generator=g, device=DEV, dtype=torch.int32)
        argmax[-1] = argmax[-1] % (M - (ng - 1) * S)          # the last (partial) group's arg rows lie inside M
        argmax = argmax.to(torch.uint8).to(DEV)
        G = None
    else:
        gpool = argmax = None
        G = _rand(g, M, N)
    edge = form in ("edge", "edge_gw")
    E = _rand(g, M, 8) if edge else None
    nparts = max(groups, 1)
    scratch = torch.empty(nparts * (K * N + N + K * K + K), device=DEV)
    dW, db = Out((K, N)), Out((N,))
    Gprev = None if edge else Out((M, K))
    stats = Out((nparts, 2, K))
    estats = Out((nparts, 6, K)) if edge else None

    def ptr(x):
        return None if x is None else x.data_ptr()

    st = torch.cuda.current_stream().cuda_stream
    common = (M, K, N, Yprev.data_ptr(), sc.data_ptr(), sh.data_ptr())
    pool_args = (Y.data_ptr(), p.data_ptr(), q.data_ptr(), t.data_ptr(), ptr(gpool), ptr(argmax), S)
    if form == "plain":
        rc = lib.pcops_mlp_bwd_fused(*common, ptr(G), *pool_args[:4], ptr(gpool), ptr(argmax), S if S else 1,
                                     W.data_ptr(), scratch.data_ptr(), dW.ptr(), db.ptr(), Gprev.ptr(), stats.ptr(), st)
    elif form == "gw":
        rc = lib.pcops_mlp_bwd_fused_gw(*common, *pool_args, W.data_ptr(), bias.data_ptr(), scratch.data_ptr(), dW.ptr(),
                                        db.ptr(), Gprev.ptr(), stats.ptr(), st)
    elif form == "edge":
        rc = lib.pcops_mlp_bwd_fused_edge(*common, *pool_args, W.data_ptr(), scratch.data_ptr(), dW.ptr(), db.ptr(),
                                          stats.ptr(), E.data_ptr(), estats.ptr(), st)
    else:
        rc = lib.pcops_mlp_bwd_fused_edge_gw(*common, *pool_args, W.data_ptr(), bias.data_ptr(), scratch.data_ptr(),
                                             dW.ptr(), db.ptr(), stats.ptr(), E.data_ptr(), estats.ptr(), st)
    pl = plan()
    torch.cuda.synchronize()
    outs = [o for o in (dW, db, Gprev, stats, estats) if o is not None]
    what = "%s M=%d K=%d N=%d S=%d" % (form, M, K, N, S)
    if groups == 0:
        assert rc == UNSUPPORTED, "%s: the query says no, the launcher returned %d" % (what, rc)
        assert all(o.untouched() for o in outs), "%s: refused, yet wrote" % what
        return None
    assert rc == OK, "%s: the query says %d groups, the launcher returned %d" % (what, groups, rc)
    assert all(o.guards_intact() for o in outs), "%s: a write outside an output" % what
    if pooled:
        Gd = torch.zeros(ng, S, N, dtype=torch.float64, device=DEV)
        Gd.scatter_(1, argmax.long().unsqueeze(1), gpool.double().unsqueeze(1))
        Gd = Gd.view(ng * S, N)[:M]
    else:
        Gd = G.double()
    pd, qd, td = p.double(), q.double(), t.double()
    dY = pd * Gd + qd * Y.double() + td
    dYabs = pd.abs() * Gd.abs() + qd.abs() * Y.double().abs() + td.abs()
    mask = (Yprev.double() * sc.double() + sh.double()) > 0
    Gm = (dY @ W.double().t()) * mask
    Gm_bound = (N + 6) * U * (dYabs @ W.double().abs().t()) * mask
    # the Gram form evaluates X^T (q.Y) as (X^T X) W diag(q): its bound is that product's magnitude
    yabs = (Aabs @ W.double().abs() + bias.double().abs()) if form in ("gw", "edge_gw") else Y.double().abs()
    dW_bound = (M + 6 + K) * U * (Aabs.t() @ (pd.abs() * Gd.abs() + qd.abs() * yabs + td.abs()))
    check_elementwise(dW.t, A.t() @ dY, dW_bound, "%s dW" % what)
    check_elementwise(db.t, dY.sum(0), (M + 6) * U * dYabs.sum(0), "%s db" % what)
    if Gprev is not None:
        check_elementwise(Gprev.t, Gm, Gm_bound, "%s Gprev" % what)
        Gs = Gprev.t.double()
    else:
        Gs = Gm
    assert torch.isfinite(stats.t).all(), "%s: stats rows" % what
    for which, val in ((0, Gs), (1, Gs * Yprev.double())):
        got, want = stats.t[:, which].double().sum(0), val.sum(0)
        assert ((got - want).abs() <= 3e-5 * val.abs().sum(0) + 1e-30).all(), "%s: statistics %d" % (what, which)
    if edge:
        # E^T Gm of the first EdgeConv layer below: the six edge channels of the rows (the two pad floats are not read)
        assert torch.isfinite(estats.t).all(), "%s: edge_stats" % what
        want = E[:, :6].double().t() @ Gm
        lim = 1e-5 * (E[:, :6].double().abs().t() @ Gm.abs()) + 1e-30
        assert ((estats.t.double().sum(0) - want).abs() <= lim).all(), "%s: edge_stats" % what
    return pl


@pytest.mark.parametrize("dx", [0, 1, 2])
@pytest.mark.parametrize("gram", [0, 1])
def test_bwd_fused_query_and_launcher_agree(gram, dx):
    lib = _lib.load()
    p0 = _lib.set_option(_lib.OPT_BWD_FUSED_GRAM_WGRAD, gram)
    p1 = _lib.set_option(_lib.OPT_BWD_FUSED_DX_SPLIT_BF16, dx)
    try:
        n = 0
        for M in BF_M:
            for K in BF_K:
                for N in BF_N:
                    for S in BF_S:
                        for form in BF_FORMS:
                            if form != "plain" and S == 0:
                                continue                  # the pooled-only forms take no dense gradient
                            accepted = _bf_query(lib, form, M, K, N, S) > 0
                            # numbers for every accepted shape; the refusals are cheap, the full grid is walked
                            pl = _bf_case(lib, form, M, K, N, S, seed=M + K * 7 + N * 13 + S)
                            assert (pl is not None) == accepted
                            if pl is not None:
                                OBSERVED["bwd_fused"].add(pl)
                                n += 1
        assert n > 0
    finally:
        _lib.set_option(_lib.OPT_BWD_FUSED_DX_SPLIT_BF16, p1)
        _lib.set_option(_lib.OPT_BWD_FUSED_GRAM_WGRAD, p0)


def test_edge_query_refuses_whole_tiles_with_the_gram_option():
    """the bug the grid above found: with the Gram option on, the non-edge query accepted S = 32 / 64 while the edge launcher
    refuses every S % 32 == 0; the edge forms now answer for themselves (fused_mlp asks the query of the launcher it calls).
    Through fused_mlp this never raised: the direct first-layer EdgeConv path only builds the edge rows where the edge query
    accepts, so a stack with k = 32 takes pcops_mlp_bwd_fused_gw and no edge form -- the fix is pinned here and by the grid."""
    lib = _lib.load()
    p0 = _lib.set_option(_lib.OPT_BWD_FUSED_GRAM_WGRAD, 1)
    try:
        for S in (32, 64):
            assert lib.pcops_mlp_bwd_fused_gw_groups(1 << 22, 64, 128, S) == 256
            assert lib.pcops_mlp_bwd_fused_edge_groups(1 << 22, 64, 128, S, 1) == 0
            assert lib.pcops_mlp_bwd_fused_edge_groups(1 << 22, 64, 128, S, 0) == 0
        assert lib.pcops_mlp_bwd_fused_edge_groups(1 << 22, 64, 128, 20, 1) == 256
    finally:
        _lib.set_option(_lib.OPT_BWD_FUSED_GRAM_WGRAD, p0)


# ------------------------------------------------------------------------------------------ outputs larger than 4 GiB
def _sample_rows(M):
    """first and last tiles, the rows around the 2^31- and 2^32-byte offsets of a 128-float row (and of a 64-float one),
    the ragged tail, and a spread in between"""
    rows = set(range(0, 64)) | set(range(M - 96, M))
    for row_bytes in (256, 512):
        for edge in (1 << 31, 1 << 32):
            r = edge // row_bytes
            rows |= set(range(max(r - 40, 0), min(r + 40, M)))
    rows |= set(range(0, M, M // 1500))
    return torch.tensor(sorted(rows), device=DEV)


def test_forward_and_data_gradient_past_4gib():
    lib = _lib.load()
    M, K, N = (1 << 23) + 77, 64, 128
    g = torch.Generator(device=DEV).manual_seed(5)
    X = torch.randn(M, K, device=DEV, generator=g)
    W = torch.randn(K, N, device=DEV, generator=g) / K ** 0.5
    bias = 0.1 * torch.randn(N, device=DEV, generator=g)
    sc, sh = torch.rand(K, device=DEV, generator=g) + 0.5, 0.3 * torch.randn(K, device=DEV, generator=g)
    rows = _sample_rows(M)
    st = torch.cuda.current_stream().cuda_stream
    Y = Out((M, N))                                        # 4.3 GB
    P = lib.pcops_mlp_stats_rows(M)
    part = Out((P, 2, N))
    assert lib.pcops_mlp_gemm_fwd(M, K, N, X.data_ptr(), K, sc.data_ptr(), sh.data_ptr(), W.data_ptr(), bias.data_ptr(),
                                  Y.ptr(), part.ptr(), None, st) == OK
    fplan = plan()
    torch.cuda.synchronize()
    assert fplan[0] == 2
    A, Aabs = prologue(X[rows], sc, sh)
    check_elementwise(Y.t[rows], A @ W.double() + bias.double(),
                      (K + 4) * U * (Aabs @ W.double().abs() + bias.double().abs()), "fwd past 4 GiB")
    assert Y.guards_intact() and part.guards_intact() and torch.isfinite(part.t).all()
    assert torch.isfinite(Y.t[-4096:]).all()
    del X
    # the data gradient of the same layer: dY (M, 128) from G and the stored Y, Gprev (M, 64) masked by a layer below
    G = torch.randn(M, N, device=DEV, generator=g)
    p, q, t = torch.rand(N, device=DEV, generator=g) + 0.5, 0.1 * torch.randn(N, device=DEV, generator=g), \
        0.05 * torch.randn(N, device=DEV, generator=g)
    Wt = W.t().contiguous()
    Gprev = Out((M, K))
    assert lib.pcops_mlp_gemm_dgrad(M, N, K, G.data_ptr(), Y.ptr(), p.data_ptr(), q.data_ptr(), t.data_ptr(), None,
                                    None, 1, None, None, Wt.data_ptr(), None, None, None, Gprev.ptr(), None, st) == OK
    torch.cuda.synchronize()
    dY, dYabs = dy_operand(len(rows), N, G[rows], Y.t[rows], p, q, t)
    check_elementwise(Gprev.t[rows], dY @ Wt.double(), (N + 6) * U * (dYabs @ Wt.double().abs()), "dgrad past 4 GiB")
    assert Gprev.guards_intact() and torch.isfinite(Gprev.t[-4096:]).all()
    # a plain dgrad takes 8 M x 128 floats of dY through 32-bit offsets: the last rows are the ones a clamp would lose
    tail = torch.arange(M - 2048, M, device=DEV)
    dY, dYabs = dy_operand(len(tail), N, G[tail], Y.t[tail], p, q, t)
    check_elementwise(Gprev.t[tail], dY @ Wt.double(), (N + 6) * U * (dYabs @ Wt.double().abs()), "dgrad tail")


# --------------------------------------------------------------------------------------------------------------- coverage
# every variant each launcher reached over the tables above; a plan change that adds, removes or re-routes a branch fails
# here and the lists are updated on purpose.  (path, split, bn, wst, pool) as in pcops.h pcops_last_launch_plan.
EXPECT_VARIANTS = {
    "fwd": [
        (1, 0, 0, 0, 0), (2, 0, 64, 0, 0), (2, 0, 64, 1, 0), (2, 0, 96, 0, 0), (2, 0, 128, 0, 0), (2, 0, 128, 1, 0),
        (2, 1, 64, 0, 0), (2, 1, 64, 1, 0), (2, 1, 96, 0, 0), (2, 1, 128, 0, 0), (2, 1, 128, 1, 0),
    ],
    "fwd_pool": [
        (2, 0, 64, 0, 1), (2, 0, 96, 0, 1), (2, 0, 128, 0, 1), (2, 1, 64, 0, 1), (2, 1, 64, 0, 3), (2, 1, 96, 0, 1),
        (2, 1, 96, 0, 3), (2, 1, 128, 0, 1), (2, 1, 128, 0, 3),
    ],
    "dgrad": [
        (1, 0, 0, 0, 0), (1, 0, 0, 0, 2), (2, 0, 64, 0, 0), (2, 0, 64, 0, 1), (2, 0, 64, 0, 2), (2, 0, 64, 1, 0),
        (2, 0, 64, 1, 2), (2, 0, 96, 0, 0), (2, 0, 96, 0, 2), (2, 0, 96, 1, 0), (2, 0, 128, 0, 0), (2, 0, 128, 0, 1),
        (2, 0, 128, 1, 0), (2, 1, 64, 0, 0), (2, 1, 64, 0, 1), (2, 1, 64, 0, 2), (2, 1, 96, 0, 2),
    ],
    "wgrad": [
        (4, 1, 128, 0, 0), (4, 1, 128, 0, 1), (5, 0, 64, 0, 2), (5, 0, 128, 0, 1), (5, 0, 128, 0, 2),
        (5, 0, 256, 0, 0), (6, 0, 64, 0, 0), (6, 0, 128, 0, 0), (7, 0, 128, 0, 0), (7, 0, 128, 0, 2),
        (4, 1, 128, 0, 2), (5, 0, 64, 0, 1), (5, 0, 256, 0, 1), (5, 0, 256, 0, 2),          # test_wgrad_arms
    ],
    "bwd_fused": [
        (3, 0, 64, 0, 0), (3, 0, 64, 0, 1), (3, 0, 64, 0, 2), (3, 0, 128, 0, 0), (3, 0, 128, 0, 1), (3, 0, 128, 0, 2),
        (3, 1, 64, 0, 0), (3, 1, 64, 0, 1), (3, 1, 64, 0, 2), (3, 1, 64, 0, 9), (3, 1, 64, 0, 10), (3, 1, 128, 0, 0),
        (3, 1, 128, 0, 1), (3, 1, 128, 0, 2), (3, 1, 128, 0, 9), (3, 1, 128, 0, 10), (3, 2, 128, 0, 0),
        (3, 2, 128, 0, 1), (3, 2, 128, 0, 2),
    ],
}


def test_every_listed_variant_ran():
    """runs last in the module (pytest keeps file order): the set of variants observed per launcher is the list"""
    for k, want in EXPECT_VARIANTS.items():
        assert OBSERVED[k] == set(want), (k, sorted(OBSERVED[k] - set(want)), sorted(set(want) - OBSERVED[k]))
