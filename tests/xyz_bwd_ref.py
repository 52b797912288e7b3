"""float64 restatement of pcops_mlp_bwd_fused_xyz_rows on uncompacted rows with a dense upstream gradient (the one-pass backward of
the layer above the arithmetic first layer), and the inputs tests/test_xyz_bwd_ref_cpu.py and tests/test_xyz_bwd_tiles_gpu.py
share.  Plain torch, nothing of the library; every function takes the fp32 inputs and computes in float64.

    y1 = b + dx w0 + dy w1 + dz w2          z = y1 a_scale + a_shift        X1 = max(z, 0)       m1 = z > 0
    dY = p G + q Y + t                      dW = X1^T dY                    db = 1^T dY          Gp = m1 . (dY W^T)
    sums: Gp, Gp y1 and off_i Gp (i = x, y, z) over the rows
"""
import torch

K = 64
KINDS = ("random", "masks_off", "masks_on", "t_only", "zero_rows", "decades")


def xyz_bwd(off4, xyzw, a_scale, a_shift, G, Y, p, q, t, W):
    """-> dict(dW [K][N], db [N], gp [K], gpy [K], off [3][K]), float64, on the inputs' device"""
    d = torch.float64
    off = off4[:, :3].to(d)
    w, b = xyzw[:3].to(d), xyzw[3].to(d)
    y1 = off @ w + b
    z = y1 * a_scale.to(d) + a_shift.to(d)
    X1 = z.clamp_min(0.0)
    dY = p.to(d) * G.to(d) + q.to(d) * Y.to(d) + t.to(d)
    Gp = (dY @ W.to(d).t()) * (z > 0).to(d)
    return {"dW": X1.t() @ dY, "db": dY.sum(0), "gp": Gp.sum(0), "gpy": (Gp * y1).sum(0), "off": off.t() @ Gp}


def z_fp32(d):
    """z evaluated in fp32, one operation at a time (no operation of it rounds on the inputs of make_inputs: any order and
    any fusing give these bits)"""
    off, xw = d["off4"], d["xyzw"]
    y1 = xw[3].expand(off.shape[0], -1).clone()
    for i in range(3):
        y1 = torch.addcmul(y1, off[:, i:i + 1], xw[i:i + 1])
    return torch.addcmul(d["ash"].expand_as(y1), y1, d["asc"].expand_as(y1))


def z_fp64(d):
    off, xw = d["off4"].double(), d["xyzw"].double()
    return (off[:, :3] @ xw[:3] + xw[3]) * d["asc"].double() + d["ash"].double()


def make_inputs(M, N, seed, kind="random"):
    """CPU fp32 inputs.  off4 (its x, y, z), w0..2, b, a_scale and a_shift are multiples of 2^-6 of magnitude at most 2:
    y1 is then a multiple of 2^-12 below 16 and z a multiple of 2^-18 below 32 -- both exact in fp32, so the ReLU decision
    of an fp32 kernel is the float64 one whatever its operation order.  Channel 5 has b = a_shift = 0 and every seventh row
    zero offsets: exact zeros of z.  G, Y, p, q, t, W are random."""
    assert kind in KINDS
    g = torch.Generator().manual_seed(seed)
    q6 = lambda *shape: torch.randint(-128, 129, shape, generator=g).float() / 64.0
    rn = lambda *shape: torch.randn(*shape, generator=g)
    d = {"off4": q6(M, 4), "xyzw": q6(4, K), "asc": q6(K), "ash": q6(K)}
    d["xyzw"][3, 5] = 0.0
    d["ash"][5] = 0.0
    d["off4"][::7, :3] = 0.0
    d["G"], d["Y"] = rn(M, N), rn(M, N)
    d["p"], d["q"], d["t"] = 1.0 + 0.1 * rn(N), 0.01 * rn(N), 0.01 * rn(N)
    d["W"] = rn(K, N) / 8.0
    if kind == "masks_off":
        d["asc"].fill_(0.0)
        d["ash"].fill_(-1.0)
    elif kind == "masks_on":
        d["asc"].fill_(0.0)
        d["ash"].fill_(1.0)
    elif kind == "t_only":
        d["p"].fill_(0.0)
        d["q"].fill_(0.0)
        d["t"] = 0.5 + rn(N).abs()
    elif kind == "zero_rows":
        d["off4"][1::2] = 0.0
    elif kind == "decades":
        mag = torch.logspace(-6, 3, M)[torch.randperm(M, generator=g)]
        d["G"] *= mag.unsqueeze(1)
    return d


def reference(d):
    return xyz_bwd(d["off4"], d["xyzw"], d["asc"], d["ash"], d["G"], d["Y"], d["p"], d["q"], d["t"], d["W"])
