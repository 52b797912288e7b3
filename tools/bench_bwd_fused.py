"""micro-benchmark of the one-pass backward (pcops_mlp_bwd_fused) against its Gram-form weight gradient
(pcops_mlp_bwd_fused_gw) at SA1's pooled top layer (4.19 M rows, 64 -> 128, groups of 32) and the T-Net's (10.5 M, groups of 20):
python tools/bench_bwd_fused.py [reps]   -- sustained loops of `reps` launches each, alternating.
`python tools/bench_bwd_fused.py [reps] tiles`: SA2's middle layer instead (2.10 M allocated rows, 128 -> 128, about 1.42 M after
compaction) -- pcops_mlp_gemm_dgrad_rows + pcops_mlp_wgrad_rows against pcops_mlp_bwd_tiles_rows on the same inputs."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from scanobjectnn_amd import _lib
lib = _lib.load()
_lib.set_option(_lib.OPT_BWD_FUSED_GRAM_WGRAD, 1)     # (opt-in: DESIGN.md section 4.16)
dev = "cuda:0"
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30


def vec(n):
    return torch.randn(n, device=dev) * 0.1 + 1.0


def timeit(fn):
    global reps
    fn(); torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def tiles128():
    B, Mg, S, K = 256, 128, 64, 128
    M = B * Mg * S
    cnt = torch.randint(9, S + 1, (B, Mg), device=dev, dtype=torch.int32)
    rows = _lib.Rows(cnt, S)
    Yp, Gm = torch.randn(M, K, device=dev), torch.randn(M, K, device=dev)
    W = torch.randn(K, K, device=dev) / K ** 0.5
    asc, ash, p, q, t = vec(K), vec(K) * 0.1, vec(K), vec(K) * 0.01, vec(K) * 0.01
    Y = torch.empty(M, K, device=dev)
    for r0 in range(0, M, 1 << 20):
        Y[r0:r0 + (1 << 20)] = torch.relu(Yp[r0:r0 + (1 << 20)] * asc + ash) @ W
    groups, P = lib.pcops_mlp_bwd_tiles_groups(M, K, K), lib.pcops_mlp_stats_rows(M)
    scratch = torch.empty(max(groups, lib.pcops_mlp_wgrad_splits(M, K, K)) * (K * K + K), device=dev)
    dW, db, Gprev, Wt = torch.empty(K, K, device=dev), torch.empty(K, device=dev), torch.empty(M, K, device=dev), torch.empty(K, K, device=dev)
    part = torch.zeros(max(groups, P), 2, K, device=dev)
    ptrs = [x.data_ptr() for x in (p, q, t)]

    def two():
        _lib.call("pcops_mlp_wgrad_rows", M, K, K, Yp.data_ptr(), K, asc.data_ptr(), ash.data_ptr(), Gm.data_ptr(), Y.data_ptr(),
                  *ptrs, None, None, 1, None, None, scratch.data_ptr(), dW.data_ptr(), db.data_ptr(), rows.ref)
        _lib.call("pcops_mlp_transpose", K, K, W.data_ptr(), Wt.data_ptr())
        _lib.call("pcops_mlp_gemm_dgrad_rows", M, K, K, Gm.data_ptr(), Y.data_ptr(), *ptrs, None, None, 1, None, None,
                  Wt.data_ptr(), Yp.data_ptr(), asc.data_ptr(), ash.data_ptr(), Gprev.data_ptr(), part.data_ptr(), rows.ref)

    def one():
        _lib.call("pcops_mlp_bwd_tiles_rows", M, K, K, Yp.data_ptr(), asc.data_ptr(), ash.data_ptr(), Gm.data_ptr(), Y.data_ptr(),
                  *ptrs, W.data_ptr(), scratch.data_ptr(), dW.data_ptr(), db.data_ptr(), Gprev.data_ptr(), part.data_ptr(), rows.ref)
    n = rows.num_rows()
    two(); d0, g0 = dW.clone(), Gprev[:n].clone()
    one(); d1, g1 = dW.clone(), Gprev[:n].clone()
    print("M=%d (%d rows): max |dW_tiles - dW| / max|dW| = %.3e, Gprev %.3e" % (
        M, n, float((d1 - d0).abs().max() / d0.abs().max()), float((g1 - g0).abs().max() / g0.abs().max())))
    for rnd in range(4):
        print("   two kernels %8.1f us   tiles %8.1f us" % (timeit(two), timeit(one)), flush=True)
    print("   distinct bytes %.2f GB: %.2f TB/s in the tile kernel's time" % (n * K * 16 / 1e9, n * K * 16 / timeit(one) / 1e6))


if sys.argv[2:3] == ["tiles"]:
    tiles128()
    sys.exit(0)

for (M, K, N, S) in [(4194304, 64, 128, 32), (10485760, 64, 128, 20)]:
    G = M // S
    Yp = torch.randn(M, K, device=dev)
    W = torch.randn(K, N, device=dev) / K ** 0.5; b = torch.randn(N, device=dev) * 0.1
    asc, ash, p, q, t = vec(K), vec(K) * 0.1, vec(N), vec(N) * 0.01, vec(N) * 0.01
    Y = torch.empty(M, N, device=dev)
    for r0 in range(0, M, 1 << 20):     # the layer's own forward: Y = relu(bn(Yprev)) W + b
        Y[r0:r0 + (1 << 20)] = torch.addmm(b, torch.relu(Yp[r0:r0 + (1 << 20)] * asc + ash), W)
    gp = torch.randn(G, N, device=dev); am = torch.randint(0, S, (G, N), device=dev, dtype=torch.int32).to(torch.uint8)
    groups = lib.pcops_mlp_bwd_fused_groups(M, K, N, S, 1)
    scratch = torch.empty(groups * (K * N + N + K * K + K), device=dev)
    dW, db, Gprev = torch.empty(K, N, device=dev), torch.empty(N, device=dev), torch.empty(M, K, device=dev)
    part = torch.empty(groups, 2, K, device=dev)
    f0 = lambda: _lib.call("pcops_mlp_bwd_fused", M, K, N, Yp.data_ptr(), asc.data_ptr(), ash.data_ptr(), None, Y.data_ptr(),
                           p.data_ptr(), q.data_ptr(), t.data_ptr(), gp.data_ptr(), am.data_ptr(), S, W.data_ptr(),
                           scratch.data_ptr(), dW.data_ptr(), db.data_ptr(), Gprev.data_ptr(), part.data_ptr())
    f1 = lambda: _lib.call("pcops_mlp_bwd_fused_gw", M, K, N, Yp.data_ptr(), asc.data_ptr(), ash.data_ptr(), Y.data_ptr(),
                           p.data_ptr(), q.data_ptr(), t.data_ptr(), gp.data_ptr(), am.data_ptr(), S, W.data_ptr(), b.data_ptr(),
                           scratch.data_ptr(), dW.data_ptr(), db.data_ptr(), Gprev.data_ptr(), part.data_ptr())
    f0(); d0 = dW.clone(); f1(); d1 = dW.clone()
    print("M=%d S=%d: max |dW_gw - dW| / max|dW| = %.3e" % (M, S, float((d1 - d0).abs().max() / d0.abs().max())))
    for rnd in range(3):
        print("   plain %8.1f us   gram form %8.1f us" % (timeit(f0), timeit(f1)), flush=True)
    # sustained (0.5 s each) with the shader clock and socket power the chip holds meanwhile (bench.py's hwmon poller)
    import bench
    keep = reps
    for label, fn in (("plain", f0), ("gram form", f1), ("plain", f0), ("gram form", f1)):
        reps = max(30, int(0.5e6 / max(timeit(fn), 1.0)))
        with bench.ClockPoller() as poller:
            us = timeit(fn)
        c = poller.summary() or {}
        print("   sustained %-9s %8.1f us   sclk %6.0f MHz   %6.0f W   (%d launches)" % (
            label, us, c.get("sclk_mhz", float("nan")), c.get("power_w", float("nan")), reps), flush=True)
    reps = keep
    del Yp, Y, Gprev
    torch.cuda.empty_cache()
