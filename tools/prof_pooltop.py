"""Per-call HIP-event timings of the algebraic top-layer backward (fused_mlp._pool_top_backward) against the plain
dgrad + wgrad it replaces, at the benchmark shapes; then SA2's compacted case: pcops_mlp_gram_rows (csrc/mlp.hip),
pcops_mlp_pool_top_wsparse_rows and pcops_mlp_pool_top_addend_rows (csrc/pooltop_sparse.hip) alone, HIP events around the entry point, under both
values of PCOPS_OPT_GRAM_SPLIT_BF16 / PCOPS_OPT_POOL_TOP_ROWS_PIPELINED (DESIGN.md sections 4.21, 4.23).
python tools/prof_pooltop.py [--rows-only]"""
import collections
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scanobjectnn_amd import _lib, fused_mlp  # noqa: E402

DEV = "cuda:0"
SHAPES = [("SSG SA3", 256 * 128, 128, 256, [256, 512, 1024]), ("DGCNN agg", 256 * 2048, 256, 320, [1024]),
          ("DGCNN tconv3", 256 * 2048, 256, 128, [1024]),
          # SA2 without row compaction: 32 768 groups of 64 (the compacted stack runs the *_rows forms of the same launches)
          ("SSG SA2", 256 * 128 * 64, 64, 132, [128, 128, 256])]


def layers(k0, widths):
    g = torch.Generator().manual_seed(k0)
    out, k = [], k0
    for n in widths:
        out.append([(torch.randn(k, n, generator=g) / k ** 0.5).to(DEV).requires_grad_(True),
                    (torch.randn(n, generator=g) * 0.1).to(DEV).requires_grad_(True),
                    (1 + 0.1 * torch.randn(n, generator=g)).to(DEV).requires_grad_(True),
                    (0.1 * torch.randn(n, generator=g)).to(DEV).requires_grad_(True),
                    torch.zeros(n, device=DEV), torch.ones(n, device=DEV)])
        k = n
    return out


class Timer:
    def __init__(self):
        self.t = collections.OrderedDict()
        self.open = None

    def __call__(self, name, phase, args):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        if phase == "pre":
            self.open = ev
        else:
            self.t.setdefault(name, []).append((self.open, ev))

    def report(self):
        torch.cuda.synchronize()
        tot = 0.0
        for k, v in self.t.items():
            ms = sum(a.elapsed_time(b) for a, b in v) / len(v)
            tot += ms * 1e3
            print("    %-34s x%d %8.1f us" % (k, len(v), ms * 1e3))
        print("    sum %.1f us" % tot)


def rows_case(reps=20):
    """SSG SA2 over compacted rows: 32 768 groups of 24 .. 64 members in S = 64 slots, Kp = 128, N = 256"""
    lib = _lib.load()
    S, Kp, N, G = 64, 128, 256, 32768
    g = torch.Generator().manual_seed(1)
    cnt = torch.randint(24, 65, (G,), generator=g, dtype=torch.int32)
    rows = _lib.Rows(cnt.view(256, 128).to(DEV), S)
    R = G * S
    print("SSG SA2, compacted: %d rows of %d, S %d, %d -> %d" % (rows.num_rows(), R, S, Kp, N))
    Yprev = torch.randn(R, Kp, generator=g).to(DEV)
    psc, psh = (0.5 + torch.rand(Kp, generator=g)).to(DEV), (0.3 * torch.randn(Kp, generator=g)).to(DEV)
    splits = lib.pcops_mlp_wgrad_splits(R, Kp, Kp)
    scratch, gram, xsum = (torch.empty(n, device=DEV) for n in (splits * (Kp * Kp + Kp), Kp * Kp, Kp))
    gout, ysel = torch.randn(G, N, generator=g).to(DEV), torch.randn(G, N, generator=g).to(DEV)
    nrow = 16 * ((cnt.long() + 15) // 16)
    arg8 = (torch.rand(G, N, generator=g) * nrow.view(G, 1)).long().clamp_(max=255).to(torch.uint8).to(DEV)
    sc, sh, p = ((0.5 + torch.rand(N, generator=g)).to(DEV), (0.2 * torch.randn(N, generator=g)).to(DEV),
                 (0.5 + torch.rand(N, generator=g)).to(DEV))
    Ssp, cfsum = torch.empty(Kp, N, device=DEV), torch.empty(N, device=DEV)
    wpart = torch.empty(int(lib.pcops_mlp_pool_top_wsparse_rows_partial(Kp, N)), device=DEV)

    def gram_call():
        _lib.call("pcops_mlp_gram_rows", R, Kp, Yprev.data_ptr(), Kp, psc.data_ptr(), psh.data_ptr(), scratch.data_ptr(),
                  gram.data_ptr(), xsum.data_ptr(), rows.ref)

    def ws_call():
        _lib.call("pcops_mlp_pool_top_wsparse_rows", R, Kp, N, S, gout.data_ptr(), ysel.data_ptr(), arg8.data_ptr(),
                  sc.data_ptr(), sh.data_ptr(), p.data_ptr(), Yprev.data_ptr(), psc.data_ptr(), psh.data_ptr(),
                  Ssp.data_ptr(), cfsum.data_ptr(), wpart.data_ptr(), rows.ref)

    Wt = (torch.randn(N, Kp, generator=g) / N ** 0.5).to(DEV)
    addend, rowmap = torch.empty(R, Kp, device=DEV), torch.empty(R, dtype=torch.int32, device=DEV)

    def addend_call():
        _lib.call("pcops_mlp_pool_top_addend_rows", R, Kp, N, S, gout.data_ptr(), ysel.data_ptr(), arg8.data_ptr(),
                  sc.data_ptr(), sh.data_ptr(), p.data_ptr(), Wt.data_ptr(), addend.data_ptr(), rowmap.data_ptr(), rows.ref)

    def timeit(f):
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        ts.sort()
        return ts[0], ts[len(ts) // 2], ts[-1]

    for label, option, f in (("gram_rows (gram + partial sum + mirror)", _lib.OPT_GRAM_SPLIT_BF16, gram_call),
                             ("wsparse_rows (walk + partial sum)", _lib.OPT_POOL_TOP_ROWS_PIPELINED, ws_call),
                             ("addend_rows", _lib.OPT_POOL_TOP_ROWS_PIPELINED, addend_call)):
        prev = _lib.get_option(option)
        try:
            for value in (0, 1, 0, 1):
                _lib.set_option(option, value)
                print("    %-42s option %d: min %6.1f median %6.1f max %6.1f us" % ((label, value) + timeit(f)))
        finally:
            _lib.set_option(option, prev)


for name, R, S, k0, widths in ([] if "--rows-only" in sys.argv else SHAPES):
    x = torch.randn(R, k0, device=DEV).requires_grad_(True)
    ls = layers(k0, widths)
    for mode in (True, False):
        fused_mlp.POOL_TOP = mode
        for it in range(3):
            out = fused_mlp.mlp_stack(x, S, True, True, 0.9, 1e-3, True, [tuple(l) for l in ls])
            go = torch.randn_like(out)
            tm = Timer()
            if it == 2:
                _lib._hooks.append(tm)
            out.backward(go)
            if it == 2:
                _lib._hooks.remove(tm)
                print("%s rows %d S %d %d -> %s  %s" % (name, R, S, k0, widths, "algebraic" if mode else "plain"))
                tm.report()

rows_case()
