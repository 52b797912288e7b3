"""tools/phase_prof.py for the two pooled forwards of the flagship step as the step calls them -- Y == NULL, stat_pivot given:
SA1's 64 -> 128 over 4 194 304 rows in groups of 32, SA2's 128 -> 256 over a compacted row set of 256 x 128 groups of 64 slots.
Needs a -DPCOPS_PHASE_PROF build of the library (see tools/phase_prof.py):
    PCOPS_LIB=scanobjectnn_amd/libpcops_prof.so python tools/phase_prof_pool.py [label]
Per launch: shader cycles per 32-row tile and wave in staging, the k-step loop (next to the 32 cycles per
v_mfma_f32_32x32x16_bf16 its matrix instructions occupy the pipe) and everything behind the loop; profiles/pool_fwd_acc_stats_ab.txt."""
import ctypes as C
import os
import sys
label = sys.argv[1] if len(sys.argv) > 1 else ""
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from scanobjectnn_amd import _lib
lib = _lib.load()
lib.pcops_debug_phase_prof.argtypes = [C.POINTER(C.c_ulonglong)]
dev = "cuda:0"
flag = getattr(lib, "pcops_last_launch_acc_stats", None)


def prof(name, fn, mfma_per_tile, reps=5):
    buf = (C.c_ulonglong * 8)()
    fn()
    fn()
    lib.pcops_debug_phase_prof(buf)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    lib.pcops_debug_phase_prof(buf)
    us = s.elapsed_time(e) / reps * 1e3
    st, mf, ep, tot, tiles, waves = (buf[i] / reps for i in range(6))
    print("%-6s %-40s acc_stats %s %7.0f us | cycles per tile and wave: stage %6.0f  matrix loop %6.0f (pipe %5d)  epilogue %6.0f  sum %6.0f | "
          "wave total %9.0f, tiles/wave %.1f, accounted %.2f"
          % (label, name, flag() if flag else "-", us, st / tiles, mf / tiles, mfma_per_tile * 32, ep / tiles,
             (st + mf + ep) / tiles, tot / waves, tiles / waves, (st + mf + ep) / tot), flush=True)


def vec(n, g):
    return (torch.randn(n, generator=g) * 0.1 + 1.0).to(dev)


g = torch.Generator().manual_seed(0)
# SA1: 64 -> 128, S = 32, 4 194 304 rows
M, K, N, S = 4194304, 64, 128, 32
X = torch.randn(M, K, device=dev)
W = (torch.randn(K, N, generator=g) / K ** 0.5).to(dev)
b, sc, sh, gam, piv = vec(N, g), vec(K, g), vec(K, g), vec(N, g), (0.1 * torch.randn(N, generator=g)).to(dev)
part = torch.empty(lib.pcops_mlp_stats_rows(M), 2, N, device=dev)
ys = torch.empty(M // S, N, device=dev)
ps = torch.empty(M // S, N, dtype=torch.uint8, device=dev)
prof("SA1 fwd_pool 4194304 64->128 S=32",
     lambda: _lib.call("pcops_mlp_gemm_fwd_pool", M, K, N, S, X.data_ptr(), K, sc.data_ptr(), sh.data_ptr(), W.data_ptr(),
                       b.data_ptr(), gam.data_ptr(), None, part.data_ptr(), piv.data_ptr(), ys.data_ptr(), ps.data_ptr()),
     6 * (K // 16) * 4)
del X, ys, ps
torch.cuda.empty_cache()

# SA2: 128 -> 256 over compacted rows (256 clouds x 128 groups x 64 slots)
S, K, N = 64, 128, 256
cnt = torch.randint(1, S + 1, (256, 128), generator=g, dtype=torch.int32)
cnt[torch.rand(256, 128, generator=g) < 0.2] = S
rows = _lib.Rows(cnt.to(dev), S)
R = 256 * 128 * S
print("%-6s SA2 compacted rows: %d of %d" % (label, rows.num_rows(), R), flush=True)
X = torch.randn(R, K, device=dev)
W = (torch.randn(K, N, generator=g) / K ** 0.5).to(dev)
b, sc, sh, gam, piv = vec(N, g), vec(K, g), vec(K, g), vec(N, g), (0.1 * torch.randn(N, generator=g)).to(dev)
part = torch.empty(lib.pcops_mlp_stats_rows(R), 2, N, device=dev)
nbk = rows.blocks.shape[0]
yp = torch.empty(nbk, N, device=dev)
pp = torch.empty(nbk, N, dtype=torch.uint8, device=dev)
prof("SA2 fwd_pool_rows 128->256 compacted",
     lambda: _lib.call("pcops_mlp_gemm_fwd_pool_rows", R, K, N, X.data_ptr(), K, sc.data_ptr(), sh.data_ptr(), W.data_ptr(),
                       b.data_ptr(), gam.data_ptr(), None, part.data_ptr(), piv.data_ptr(), yp.data_ptr(), pp.data_ptr(), rows.ref),
     6 * (K // 16) * 4)
torch.cuda.synchronize()
