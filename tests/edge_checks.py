"""Shared pieces of the EdgeConv reference tests (tests/test_edge_ref_cpu.py, tests/test_edge_paths_gpu.py): the guarded
output buffer and the per-element bound of tests/test_gemm_plans_gpu.py, and the graphs / inputs both files build.
Nothing here touches the library; everything takes the device it should live on."""
import torch

U = 2.0 ** -24
C_BOUND = 2.0
RMS_BAR = 1e-6            # relative RMS against float64, kept beside every per-element bound
GUARD = 64                # elements of guard band on each side of an output
PATTERN = 0x5A5A5A5A      # guard bit pattern (a finite float no kernel writes by chance)


class Out:
    """an output inside a larger buffer, guard bands filled with PATTERN (0xA5 for bytes), the output itself with NaN
    (0xFF for bytes, -1 for int32)"""

    def __init__(self, shape, dtype=torch.float32, device="cuda:0"):
        n = 1
        for s in shape:
            n *= s
        self.n, self.lo = n, GUARD
        self.base = torch.empty(n + 2 * GUARD, dtype=dtype, device=device)
        if dtype == torch.float32:
            self.base.view(torch.int32).fill_(PATTERN)
        elif dtype == torch.int32:
            self.base.fill_(PATTERN)
        else:
            self.base.fill_(0xA5)
        self.t = self.base[self.lo:self.lo + n].view(*shape)
        self.t.fill_(float("nan") if dtype == torch.float32 else (0xFF if dtype == torch.uint8 else -1))
        self.ref = self.base.clone()

    def ptr(self):
        return self.t.data_ptr()

    def initial(self):
        """the output as it was handed over (the prefill), in the output's shape"""
        return self.ref[self.lo:self.lo + self.n].view(self.t.shape)

    def _bits(self):
        a, b = self.base, self.ref
        if a.dtype == torch.float32:
            a, b = a.view(torch.int32), b.view(torch.int32)
        return a, b

    def guards_intact(self):
        a, b = self._bits()
        return torch.equal(a[:self.lo], b[:self.lo]) and torch.equal(a[self.lo + self.n:], b[self.lo + self.n:])

    def untouched(self):
        a, b = self._bits()
        return torch.equal(a, b)


def bits_equal(a, b):
    """bit-identical float32 tensors (NaN patterns included)"""
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check_sum(out, triple, what, tiny=1e-30, report=None):
    """|out - ref| <= C (L + 4) 2^-24 A + tiny for every element, and the relative-RMS bar.  L: a number or a tensor that
    broadcasts against ref."""
    ref, A, L = triple
    out = out.double()
    assert out.shape == ref.shape, "%s: shape %s against %s" % (what, tuple(out.shape), tuple(ref.shape))
    assert torch.isfinite(out).all(), "%s: non-finite output" % what
    err = (out - ref).abs()
    lim = C_BOUND * (L + 4) * U * A + tiny
    worst = (err / lim).max().item()
    rms = ((err ** 2).mean().sqrt() / (ref ** 2).mean().sqrt().clamp_min(1e-300)).item()
    if report is not None:
        report.append((what, worst, rms))
    bad = err > lim
    assert not bad.any(), "%s: %d elements outside the bound, worst err/bound %.3g at %s" % (
        what, int(bad.sum()), worst, tuple(torch.nonzero(bad)[0].tolist()))
    assert rms <= RMS_BAR, "%s: relative RMS %.3g" % (what, rms)


def check_one_ulp(out, ref64, what):
    """a single fp32 operation whose float64 twin may round twice: at most one unit in the last place of the float64 value
    rounded once (non-negative values: the ordering of the bit patterns is the ordering of the floats)"""
    want = ref64.float()
    assert torch.isfinite(out).all(), "%s: non-finite output" % what
    assert (out >= 0).all() and (want >= 0).all()
    a = (out + 0.0).contiguous().view(torch.int32).long()
    b = (want + 0.0).contiguous().view(torch.int32).long()
    d = (a - b).abs().max().item()
    assert d <= 1, "%s: %d units in the last place" % (what, d)


# --------------------------------------------------------------------------------------------------------------- graphs
KINDS = ("knn", "hub", "dup", "self")


def make_graph(kind, b, n, m, s, gen):
    """idx (b, m, s) int32 with values in [0, n), built with torch alone.
    knn : cdist + topk of a small random cloud (the m centres are its first m points, or random ones when m > n)
    hub : a kNN graph over the first half of the points only, whose slot 0 is point 0 everywhere -- one list of length
          >= m, the second half of the points in nobody's list
    dup : every group repeats one neighbour two or three times
    self: idx[g, s] = g (mod n)"""
    dev = gen.device
    if kind == "self":
        return (torch.arange(m, device=dev) % n).view(1, m, 1).expand(b, m, s).contiguous().int()
    x = torch.rand(b, n, 3, generator=gen, device=dev)
    ctr = x[:, :m] if m <= n else torch.rand(b, m, 3, generator=gen, device=dev)
    d = torch.cdist(ctr, x)
    if kind == "hub" and (n + 1) // 2 >= s:
        d[:, :, (n + 1) // 2:] = float("inf")
    if s <= n:
        idx = d.topk(s, dim=2, largest=False).indices
    else:                                                                # more slots than points: wrap the ranking around
        idx = d.argsort(dim=2)[:, :, torch.arange(s, device=dev) % n]
    idx = idx.contiguous()
    if kind == "hub":
        idx[:, :, 0] = 0
    elif kind == "dup" and s >= 2:
        rep = 2 + (torch.arange(m, device=dev) % 2)                      # 2 or 3 copies
        src = torch.arange(m, device=dev) % s
        for r in range(1, 3):
            dst = (src + 1 + 2 * r) % s                                  # not adjacent: ties across the unrolled loads
            sel = (rep > r).view(1, m).expand(b, m)
            val = idx.gather(2, src.view(1, m, 1).expand(b, m, 1)).squeeze(2)
            cur = idx.gather(2, dst.view(1, m, 1).expand(b, m, 1)).squeeze(2)
            idx.scatter_(2, dst.view(1, m, 1).expand(b, m, 1), torch.where(sel, val, cur).unsqueeze(2))
    return idx.int()


def make_gamma(c, gen):
    """mixed signs inside a float4 in the first channels, all non-negative from channel 16 to 31 (a 16-channel slice) and,
    with c >= 128, from channel 64 to 127 (a 64-channel slice): one call then runs both the signed and the
    all-non-negative specialisation of the forward kernels; one -0.0 and one 0.0"""
    dev = gen.device
    g = 0.5 + torch.rand(c, generator=gen, device=dev)
    g[torch.arange(c, device=dev) % 3 == 1] *= -1.0
    if c >= 32:
        g[16:32] = g[16:32].abs()
        g[17], g[18] = -0.0, 0.0
    else:
        g[0], g[c - 1] = -0.0, 0.0
    if c >= 128:
        g[64:128] = g[64:128].abs()                                      # a whole 64-channel slice (a wave of ec_fwd_kernel)
    return g


def make_features(kind, b, n, m, c, gen, offset=0.0):
    """Q (b, n, 2 c) whose column halves are Q and Ctr for the strided forms; the dense forms take contiguous copies.
    `dup` quantises Q to a few values so that ties of the extremum are common and the first slot is really decided."""
    dev = gen.device
    QC = torch.randn(b, max(n, m), 2 * c, generator=gen, device=dev)
    if kind == "dup":
        QC[..., :c] = (QC[..., :c] * 1.5).round() / 2.0
    if offset:
        QC += offset
    return QC
