"""Micro-benchmark of pcops_sa_scatter_bwd on the SSG / DGCNN shapes (runs on the GPU box).
The first block feeds random Y (the Y-reading forms); the second is SSG's SA2 call as the model issues it -- compacted
rows, Y made by pcops_sa_gather_fwd_rows from Q, Wxyz -- under both values of PCOPS_OPT_SCATTER_QFORM.
usage: bench_scatter.py [reps]"""
import sys
import os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from scanobjectnn_amd import _lib

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
dev = "cuda:0"
lib = _lib.load()
CASES = [  # b, n, m, S, C, has_dq, has_xyz, pooled
    (256, 512, 128, 64, 128, True, True, False),    # SSG SA2
    (256, 512, 128, 64, 128, False, True, False),   # ... streaming part only
    (256, 512, 128, 64, 128, True, False, False),   # ... no coordinate term
    (256, 2048, 512, 32, 64, False, True, False),   # SSG SA1 (no features)
    (256, 2048, 512, 32, 64, True, True, False),    # SA1 with features
    (64, 2048, 2048, 20, 64, True, False, True),    # EdgeConv, single pooled layer
]
for (b, n, m, S, C, has_dq, has_xyz, pooled) in CASES:
    g = torch.Generator(device=dev).manual_seed(1)
    R = b * m * S
    Y = torch.randn(R, C, device=dev, generator=g)
    G = torch.randn(R, C, device=dev, generator=g)
    idx = torch.randint(0, n, (b, m, S), device=dev, generator=g, dtype=torch.int32)
    xyz = torch.rand(b, n, 3, device=dev, generator=g)
    new_xyz = torch.rand(b, m, 3, device=dev, generator=g)
    p, q, t = (torch.randn(C, device=dev, generator=g) for _ in range(3))
    gpool = torch.randn(b * m, C, device=dev, generator=g)
    argmax = torch.randint(0, S, (b * m, C), device=dev, generator=g, dtype=torch.int32).to(torch.uint8)
    dQ = torch.empty(b, n, C, device=dev) if has_dq else None
    dCtr = torch.empty(b, m, C, device=dev) if not has_xyz else None
    wpart = torch.empty(lib.pcops_sa_scatter_rows(b, m) * 4 * C, device=dev)
    dW, db = torch.empty(3, C, device=dev), torch.empty(C, device=dev)
    wsp = torch.empty(int(lib.pcops_sa_scatter_workspace_bytes(b, n, m, S)) // 4, dtype=torch.int32, device=dev)
    P = lambda x: x.data_ptr() if x is not None else None

    def run():
        _lib.call("pcops_sa_scatter_bwd", b, n, m, S, C, None if pooled else G.data_ptr(), Y.data_ptr(), p.data_ptr(),
                  q.data_ptr(), t.data_ptr(), gpool.data_ptr() if pooled else None, argmax.data_ptr() if pooled else None,
                  p.data_ptr() if pooled else None, q.data_ptr() if pooled else None, idx.data_ptr(),
                  P(xyz) if has_xyz else None, P(new_xyz) if has_xyz else None, P(dQ), P(dCtr), wpart.data_ptr(),
                  dW.data_ptr() if has_xyz else None, db.data_ptr(), None, None, None, None, wsp.data_ptr())
    run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    by = 4 * R * C * (1 if pooled else 2)
    print("b=%d n=%d m=%d S=%d C=%d dq=%d xyz=%d pooled=%d : %8.1f us  %6.0f GB/s (Y,G reads)" % (
        b, n, m, S, C, has_dq, has_xyz, pooled, ms * 1e3, by / ms / 1e6))


# ---- SSG SA2 as the model calls it: consistent Q / Wxyz / Y, compacted rows, the Y form against the Q form
def sa2_case(b=256, n=512, m=128, S=64, C=128, compact=True, fill=0.7):
    g = torch.Generator(device=dev).manual_seed(2)
    idx = torch.randint(0, n, (b, m, S), device=dev, generator=g, dtype=torch.int32)
    # ball-query layout: cnt hits per group, the remaining rows repeat the first (what compaction drops)
    cnt = (torch.rand(b, m, device=dev, generator=g) * fill * S).to(torch.int32).clamp_(1, S)
    pad = torch.arange(S, device=dev).view(1, 1, S) >= cnt.unsqueeze(-1)
    idx = torch.where(pad, idx[:, :, :1].expand(b, m, S), idx).contiguous()
    rows = _lib.Rows(cnt, S) if compact else None
    R = rows.num_rows() if compact else b * m * S
    xyz = torch.rand(b, n, 3, device=dev, generator=g)
    new_xyz = torch.rand(b, m, 3, device=dev, generator=g)
    Q = torch.randn(b, n, C, device=dev, generator=g)
    W = torch.randn(3, C, device=dev, generator=g)
    G = torch.randn(R, C, device=dev, generator=g)
    p, q, t = (torch.randn(C, device=dev, generator=g) for _ in range(3))
    Y = torch.empty(R, C, device=dev)
    rref = rows.ref if compact else None
    _lib.call("pcops_sa_gather_fwd_rows", b, n, m, S, C, Q.data_ptr(), None, xyz.data_ptr(), new_xyz.data_ptr(), W.data_ptr(),
              None, idx.data_ptr(), Y.data_ptr(), None, None, None, None, rref)
    dQ = torch.empty(b, n, C, device=dev)
    wpart = torch.empty(lib.pcops_sa_scatter_rows(b, m) * 4 * C, device=dev)
    dW = torch.empty(3, C, device=dev)
    wsp = torch.empty(int(lib.pcops_sa_scatter_workspace_bytes(b, n, m, S)) // 4, dtype=torch.int32, device=dev)

    def run():
        _lib.call("pcops_sa_scatter_bwd_rows", b, n, m, S, C, G.data_ptr(), Y.data_ptr(), p.data_ptr(), q.data_ptr(),
                  t.data_ptr(), None, None, None, None, idx.data_ptr(), xyz.data_ptr(), new_xyz.data_ptr(), dQ.data_ptr(),
                  None, wpart.data_ptr(), dW.data_ptr(), None, Q.data_ptr(), None, W.data_ptr(), None, wsp.data_ptr(), rref)
    out = {}
    for form in (0, 1, 0, 1):
        prev = _lib.set_option(_lib.OPT_SCATTER_QFORM, form)
        try:
            run()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                run()
            e1.record()
            torch.cuda.synchronize()
        finally:
            _lib.set_option(_lib.OPT_SCATTER_QFORM, prev)
        us = e0.elapsed_time(e1) / reps * 1e3
        out[form] = (dQ.clone(), dW.clone())
        by = 4 * R * C * (1 if form else 2)
        print("SA2 b=%d n=%d m=%d S=%d C=%d rows=%d (%s) %s form : %8.1f us  %6.0f GB/s (%s)  [memset + index build + walk + reduce]" % (
            b, n, m, S, C, R, "compacted" if compact else "all rows", "Q" if form else "Y", us, by / us / 1e3,
            "G reads" if form else "Y,G reads"))
    rel = lambda a, r: ((a - r).abs().max() / r.abs().max()).item()
    print("    Q form against Y form: dQ max rel diff %.3g, dWxyz %.3g" % (rel(out[1][0], out[0][0]), rel(out[1][1], out[0][1])))


sa2_case(compact=True)
sa2_case(compact=False)
