"""float64 restatement of pcops_mlp_bwd_tiles_rows (the one-pass backward of a 128 -> 128 layer  Y = relu(bn(Yprev)) W + b,
csrc/bwd_tiles128.hip), block weights of a compacted row set included, and the inputs tests/test_bwd_tiles_ref_cpu.py and
tests/test_bwd_tiles128_gpu.py share.  Plain torch, nothing of the library; the fp32 inputs are computed on in float64.

    z  = Yprev a_scale + a_shift        X = max(z, 0)        m = z > 0
    dY = p G + w (q Y + t)              w [rows]: the block's weight on the row that opens a 16-row block, 1 elsewhere
    dW = X^T dY     db = 1^T dY     Gprev = m . (dY W^T)     sums over the rows: Gprev, Gprev Yprev

The weight multiplies the dense part q Y + t only (the row stands for the sum of the gradients of its w dropped twins, whose
upstream gradient is the one row's G); the statistics are the plain sums of the Gprev that this weighted dY gives.  Only the
first `rows` rows exist (the device row count of a compacted set): the others are neither read nor written.
"""
import torch

K = 128
KINDS = ("random", "masks_off", "masks_on", "pq_zero", "decades")


def bwd_tiles(Yprev, a_scale, a_shift, G, Y, p, q, t, W, w=None, rows=None):
    """-> dict(dW [K][N], db [N], Gprev [rows][K], gp [K], gpy [K]), float64, on the inputs' device"""
    d = torch.float64
    n = Yprev.shape[0] if rows is None else int(rows)
    yp = Yprev[:n].to(d)
    z = yp * a_scale.to(d) + a_shift.to(d)
    X = z.clamp_min(0.0)
    dense = q.to(d) * Y[:n].to(d) + t.to(d)
    if w is not None:
        dense = dense * w[:n].to(d).unsqueeze(1)
    dY = p.to(d) * G[:n].to(d) + dense
    Gp = (dY @ W.to(d).t()) * (z > 0).to(d)
    return {"dW": X.t() @ dY, "db": dY.sum(0), "Gprev": Gp, "gp": Gp.sum(0), "gpy": (Gp * yp).sum(0)}


def wrong_weight_on_g(Yprev, a_scale, a_shift, G, Y, p, q, t, W, w, rows=None):
    """a WRONG restatement: the weight on p G as well (dY = w (p G + q Y + t))"""
    return bwd_tiles(Yprev, a_scale, a_shift, G.double() * w.double().unsqueeze(1), Y, p, q, t, W, w, rows)


def wrong_stats_unweighted(Yprev, a_scale, a_shift, G, Y, p, q, t, W, w, rows=None):
    """a WRONG restatement: dW, db and Gprev as they are, the statistics from the Gprev of an unweighted dY"""
    r = bwd_tiles(Yprev, a_scale, a_shift, G, Y, p, q, t, W, w, rows)
    u = bwd_tiles(Yprev, a_scale, a_shift, G, Y, p, q, t, W, None, rows)
    r["gp"], r["gpy"] = u["gp"], u["gpy"]
    return r


def layer_autograd(Yprev, a_scale, a_shift, dY, W):
    """float64 autograd of  Y = relu(Yprev a_scale + a_shift) W  under the upstream gradient dY -> (dW, dYprev)"""
    d = torch.float64
    yp = Yprev.to(d).clone().requires_grad_(True)
    Wd = W.to(d).clone().requires_grad_(True)
    Yl = torch.relu(yp * a_scale.to(d) + a_shift.to(d)) @ Wd
    Yl.backward(dY.to(d))
    return Wd.grad, yp.grad


def block_row_weights(blocks, M):
    """w [M] of a compacted row set from its block table (n, 4) int32 -- (group, row in group, weight as float bits, 0) per
    16-row block: the weight sits on the block's first row"""
    w = torch.ones(M, dtype=torch.float32)
    bw = blocks[:, 2].contiguous().view(torch.float32).cpu()
    nb = min(bw.numel(), (M + 15) // 16)
    w[0:16 * nb:16] = bw[:nb]
    return w


def make_inputs(M, seed, kind="random"):
    """CPU fp32 inputs.  Yprev, a_scale and a_shift are multiples of 2^-6 of magnitude at most 2: z is a multiple of 2^-12 below
    8, exact in fp32, so the ReLU decision of an fp32 kernel is the float64 one whatever its operation order.  Channel 5 has
    a_shift = 0 and every seventh row Yprev = 0: exact zeros of z.  G, Y, p, q, t, W are random."""
    assert kind in KINDS
    g = torch.Generator().manual_seed(seed)
    q6 = lambda *shape: torch.randint(-128, 129, shape, generator=g).float() / 64.0
    rn = lambda *shape: torch.randn(*shape, generator=g)
    d = {"Yprev": q6(M, K), "asc": q6(K), "ash": q6(K)}
    d["ash"][5] = 0.0
    d["Yprev"][::7] = 0.0
    d["G"], d["Y"] = rn(M, K), rn(M, K)
    d["p"], d["q"], d["t"] = 1.0 + 0.1 * rn(K), 0.01 * rn(K), 0.01 * rn(K)
    d["W"] = rn(K, K) / 8.0
    if kind == "masks_off":
        d["asc"].fill_(0.0)
        d["ash"].fill_(-1.0)
    elif kind == "masks_on":
        d["asc"].fill_(0.0)
        d["ash"].fill_(1.0)
    elif kind == "pq_zero":
        d["p"].fill_(0.0)
        d["q"].fill_(0.0)
    elif kind == "decades":
        mag = torch.logspace(-6, 3, M)[torch.randperm(M, generator=g)]
        d["G"] *= mag.unsqueeze(1)
    return d


def reference(d, w=None, rows=None):
    return bwd_tiles(d["Yprev"], d["asc"], d["ash"], d["G"], d["Y"], d["p"], d["q"], d["t"], d["W"], w, rows)
