"""Float64 definitions of what the set-abstraction gather / scatter launchers of csrc/gather.hip compute
(pcops_sa_gather_fwd_rows, pcops_sa_scatter_bwd_rows, pcops_rows_plan, pcops_cloud_bias_fwd / _bwd), in plain torch, on
whatever device the inputs live on, without a library call.  tests/test_sa_ref_cpu.py holds them against loops and autograd,
tests/test_sa_paths_gpu.py holds the kernels against them.

Every sum comes as a triple (ref, A, L): the float64 value, the same sum with absolute values taken term by term, and the
number of terms.  check() is the project's per-element bound  |out - ref| <= 2 (L + 8) 2^-24 A  with the relative-RMS bar of
tests/edge_checks.py beside it: an fp32 sum of L terms in any order is within (L - 1) 2^-24 of A, and the + 8 pays for the few
roundings inside one term (the products with p, q, wt, the offset subtraction, the fused multiply-adds of the coordinate term).

Forward   Y[b,j,s,:] = Q[b,idx] + Ctr[b,j] + (xyz[b,idx] - new_xyz[b,j]) Wxyz + bias, every term optional; the offset
          subtraction in fp32 as the kernels do it, then promoted.  L = the terms present (Q 1, Ctr 1, xyz 3, bias 1).
Backward  d[r,c] = p gm + wt (q Y + t);  gm = G[r,c], or pooled: gpool[g,c] [argmax[g,c] == s and psc Y + psh > 0].
          dQ[b,i] = sum of d over the rows naming i (L = their number), dCtr[g] = sum_s d (L = S), dWxyz = sum_r o_r^T d,
          dbias = sum_r d (L = rows per partial + number of partials, given by the caller who knows the kernel).
          Where the reference's Y is the float64 one rather than the fp32 tensor the kernel read (Y rebuilt or never stored),
          |Y| in A is the sum of the absolute parts and L is raised by the forward's term count.
Compacted rows (pcops.h "compacted rows"): a group with cnt hits keeps its first 16 nb rows, nb = min(ceil(max(cnt, 1) / 16),
          S / 16); wt is 1 except on row 0 of the group, which carries S - 16 nb + 1 (itself and the copies left out)."""
import torch

from edge_checks import Out, bits_equal, check_sum  # noqa: F401  (re-exported: the test files take them from here)

KBLK = 16
D = torch.float64


def check(out, triple, what, report=None):
    """|out - ref| <= 2 (L + 8) 2^-24 A and the relative-RMS bar (check_sum's own constant is L + 4)"""
    ref, A, L = triple
    check_sum(out, (ref, A, L + 4), what, report=report)


def vec(n, gen, lo=0.5):
    """mixed signs inside every float4: channel 1 mod 3 negative"""
    dev = gen.device
    s = 1.0 - 2.0 * (torch.arange(n, device=dev) % 3 == 1)
    return (lo + torch.rand(n, generator=gen, device=dev)) * s


# --------------------------------------------------------------------------------------------------------------- inputs
def make_case(b, n, m, S, C, device, seed=0, special=False, cnt=None):
    """every input either launcher can take, in the ball-query layout: a group has cnt hits, the rest of its S rows repeat
    the first.  Group 0 of every cloud is full, group 1 has one hit; with S >= 3 every other group names one point twice
    (exact duplicate rows).  special: cloud 0 names ONE point in all of its rows and no cloud names point n - 1.
    cnt: the hit counts, where a case needs particular ones."""
    gen = torch.Generator(device=device).manual_seed(seed)
    kw = dict(device=device, generator=gen)
    hi = n - 1 if special else n
    idx = torch.randint(0, hi, (b, m, S), dtype=torch.int32, **kw)
    if cnt is None:
        cnt = torch.randint(1, S + 1, (b, m), dtype=torch.int32, **kw)
        cnt[:, 0] = S
        if m > 1:
            cnt[:, 1] = 1
    else:
        cnt = torch.as_tensor(cnt, dtype=torch.int32, device=device).view(b, m)
    if S >= 3:
        idx[:, ::2, S - 1] = idx[:, ::2, 1]
    pad = torch.arange(S, device=device).view(1, 1, S) >= cnt.unsqueeze(-1)
    idx = torch.where(pad, idx[:, :, :1].expand(b, m, S), idx).contiguous()
    if special:
        idx[0] = min(5, n - 2)
    cs = dict(b=b, n=n, m=m, S=S, C=C, idx=idx, cnt=cnt, special=special)
    cs["xyz"] = torch.rand(b, n, 3, **kw)
    cs["new_xyz"] = torch.rand(b, m, 3, **kw)
    cs["Q"] = torch.randn(b, n, C, **kw)
    cs["Ctr"] = torch.randn(b, m, C, **kw)
    cs["Wxyz"] = torch.randn(3, C, **kw)
    cs["bias"] = torch.randn(C, **kw)
    cs["G"] = torch.randn(b * m * S, C, **kw)
    cs["p"], cs["q"], cs["t"] = vec(C, gen), vec(C, gen), vec(C, gen, lo=0.1)
    cs["gpool"] = torch.randn(b * m, C, **kw)
    cs["argmax"] = torch.randint(0, S, (b * m, C), dtype=torch.int32, **kw).to(torch.uint8)
    cs["psc"], cs["psh"] = vec(C, gen), 0.5 * torch.randn(C, **kw)
    return cs


# ---------------------------------------------------------------------------------------------- pcops_rows_plan, on the host
def blocks_of(cnt, S):
    cnt = cnt.reshape(-1).long()
    return torch.minimum((cnt.clamp_min(1) + KBLK - 1) // KBLK, torch.full_like(cnt, S // KBLK))


def rows_plan(cnt, S):
    """block_start (G + 1) int32, rows, blocks (total, 4) int32 = (g, s0, bits of the fp32 weight, 0)"""
    nb = blocks_of(cnt, S)
    G, dev = nb.numel(), nb.device
    bs = torch.zeros(G + 1, dtype=torch.long, device=dev)
    bs[1:] = torch.cumsum(nb, 0)
    total = int(bs[-1])
    g = torch.repeat_interleave(torch.arange(G, device=dev), nb)
    k = torch.arange(total, device=dev) - bs[g]
    w = torch.where(k == 0, (S - KBLK * nb[g] + 1).float(), torch.ones(total, device=dev))
    blocks = torch.stack([g.int(), (KBLK * k).int(), w.contiguous().view(torch.int32), torch.zeros_like(g).int()], 1)
    return bs.int(), KBLK * total, blocks.contiguous()


def row_table(cs, compact=False):
    """one entry per row of Y / G as the launchers lay them out: group, sample slot, cloud-global point, weight"""
    b, n, m, S = cs["b"], cs["n"], cs["m"], cs["S"]
    dev = cs["idx"].device
    idx2 = cs["idx"].view(b * m, S).long()
    if not compact:
        r = torch.arange(b * m * S, device=dev)
        grp, s = r // S, r % S
        wt = torch.ones(b * m * S, dtype=D, device=dev)
    else:
        _, rows, blocks = rows_plan(cs["cnt"], S)
        nb = rows // KBLK
        j = torch.arange(KBLK, device=dev).view(1, KBLK)
        grp = blocks[:, 0].long().view(nb, 1).expand(nb, KBLK).reshape(-1)
        s = (blocks[:, 1].long().view(nb, 1) + j).reshape(-1)
        w = blocks[:, 2].contiguous().view(torch.float32).double().view(nb, 1)
        wt = torch.where(j == 0, w.expand(nb, KBLK), torch.ones(nb, KBLK, dtype=D, device=dev)).reshape(-1)
        assert wt.sum().item() == b * m * S           # the compacted set stands for every row of the call
    pt = idx2[grp, s]
    return dict(grp=grp, s=s, pt=pt, dst=(grp // m) * n + pt, wt=wt, R=grp.numel())


# -------------------------------------------------------------------------------------------------------------- forward
TERM_COUNT = {"Q": 1, "Ctr": 1, "xyz": 3, "bias": 1}


def offsets(cs, tab):
    """(R, 3) fp32: the subtraction as the kernels do it"""
    return cs["xyz"].view(-1, 3)[tab["dst"]] - cs["new_xyz"].view(-1, 3)[tab["grp"]]


def forward(cs, terms, tab):
    """(Y, A, L) over the rows of tab"""
    C, dev = cs["C"], cs["idx"].device
    Y = torch.zeros(tab["R"], C, dtype=D, device=dev)
    A = torch.zeros_like(Y)
    if "Q" in terms:
        v = cs["Q"].view(-1, C)[tab["dst"]].double()
        Y, A = Y + v, A + v.abs()
    if "Ctr" in terms:
        v = cs["Ctr"].view(-1, C)[tab["grp"]].double()
        Y, A = Y + v, A + v.abs()
    if "xyz" in terms:
        o = offsets(cs, tab).double()
        Y, A = Y + o @ cs["Wxyz"].double(), A + o.abs() @ cs["Wxyz"].double().abs()
    if "bias" in terms:
        v = cs["bias"].double()
        Y, A = Y + v, A + v.abs()
    return Y, A, sum(TERM_COUNT[k] for k in terms)


def _by_owner(v, owner, P):
    return torch.zeros(P, v.shape[1], dtype=D, device=v.device).index_add_(0, owner, v)


def stats(Yd, wt, owner, P, L, pivot=None, Ay=None, Ly=0):
    """shifted sums per partial row: [P][2][C] triples (s1 = sum wt (y - pv), s2 = sum wt (y - pv)^2).  owner: the
    workgroup of every row.  Yd: the float64 of what the kernel wrote; or, with Ay (the forward's absolute parts) and Ly (its
    term count), the float64 forward itself, whose rounding the bound then has to pay for."""
    pv = torch.zeros(Yd.shape[1], dtype=D, device=Yd.device) if pivot is None else pivot.double()
    w = wt.view(-1, 1)
    d = Yd - pv
    mag = d.abs() if Ay is None else Ay + pv.abs()
    ref = torch.stack([_by_owner(w * d, owner, P), _by_owner(w * d * d, owner, P)], 1)
    A = torch.stack([_by_owner(w * mag, owner, P), _by_owner(w * mag * mag, owner, P)], 1)
    Lt = torch.tensor([L + Ly, L + 2 * Ly], dtype=D, device=Yd.device).view(1, 2, 1)
    return ref, A, Lt


def moments(o32, wt, owner, P, L):
    """the nine offset moments per partial row, [P][9]: xx xy xz yy yz zz | x y z, weighted like the statistics"""
    o = o32.double()
    x, y, z = o[:, 0], o[:, 1], o[:, 2]
    t = torch.stack([x * x, x * y, x * z, y * y, y * z, z * z, x, y, z], 1) * wt.view(-1, 1)
    return _by_owner(t, owner, P), _by_owner(t.abs(), owner, P), L


def total(triple):
    """the sum over the partial rows of a per-partial triple"""
    ref, A, L = triple
    return ref.sum(0), A.sum(0), L[0] if torch.is_tensor(L) and L.dim() == 3 else L


# ------------------------------------------------------------------------------------------------------------- backward
def pooled_gm(cs, tab, Yd):
    """(gm, margin_ok): the pooled dY selector of every row, and whether every arg-max element's ReLU decision is clear of
    the edge, |psc y + psh| >= 2^-20 (|psc y| + |psh|) -- fp32 and float64 then decide alike"""
    am = cs["argmax"].long()[tab["grp"]]
    at = am == tab["s"].view(-1, 1)
    a, h = cs["psc"].double() * Yd, cs["psh"].double()
    clear = (a + h).abs() >= 2.0 ** -20 * (a.abs() + h.abs())
    gm = torch.where(at & (a + h > 0), cs["gpool"].double()[tab["grp"]], torch.zeros_like(Yd))
    return gm, bool(clear[at].all())


def backward(cs, tab, Yd, gm, Ay=None, Ly=0, with_xyz=True, Lw=None):
    """dict of triples: dQ (b n, C), dCtr (G, C), dWxyz (3, C), dbias (C), and the row terms d.
    Yd: float64 of the fp32 Y the kernel reads; or the float64 forward with its absolute parts Ay and term count Ly."""
    b, n, m, S, C = cs["b"], cs["n"], cs["m"], cs["S"], cs["C"]
    dev = Yd.device
    pd, qd, td = cs["p"].double(), cs["q"].double(), cs["t"].double()
    w = tab["wt"].view(-1, 1)
    d = pd * gm + w * (qd * Yd + td)
    T = pd.abs() * gm.abs() + w * (qd.abs() * (Yd.abs() if Ay is None else Ay) + td.abs())
    z = lambda r: torch.zeros(r, C, dtype=D, device=dev)                                     # noqa: E731
    cnt = torch.bincount(tab["dst"], minlength=b * n).double().view(-1, 1)
    out = {"d": d, "T": T,
           "dQ": (z(b * n).index_add_(0, tab["dst"], d), z(b * n).index_add_(0, tab["dst"], T), cnt + Ly),
           "dCtr": (z(b * m).index_add_(0, tab["grp"], d), z(b * m).index_add_(0, tab["grp"], T), S + Ly)}
    if Lw is not None:
        out["dbias"] = (d.sum(0), T.sum(0), Lw + Ly)
        if with_xyz:
            o = offsets(cs, tab).double()
            out["dWxyz"] = (o.t() @ d, o.abs().t() @ T, Lw + Ly)
    return out


# ------------------------------------------------------------------------------------------- pcops_cloud_bias_fwd / _bwd
def cloud_bias(Q, Ctr, rpg, G, p, q, t, pivot=None, rows_per_partial=256):
    """Y = Q + Ctr[r / rpg] (one fp32 addition: the kernel's Y is bit-equal to it), its statistics per 256-row partial, and
    the backward dQ = p G + q Y + t (L = 3), dCtr[g] = sum of its rows (L = rpg)"""
    rows, C = Q.shape
    dev = Q.device
    Y32 = Q + Ctr[torch.arange(rows, device=dev) // rpg]
    P = rows // rows_per_partial
    owner = torch.arange(rows, device=dev) // rows_per_partial
    st = stats(Y32.double(), torch.ones(rows, dtype=D, device=dev), owner, P, rows_per_partial + P, pivot)
    d = p.double() * G.double() + q.double() * Y32.double() + t.double()
    T = p.double().abs() * G.double().abs() + q.double().abs() * Y32.double().abs() + t.double().abs()
    grp = torch.arange(rows, device=dev) // rpg
    ng = rows // rpg
    dC = (torch.zeros(ng, C, dtype=D, device=dev).index_add_(0, grp, d),
          torch.zeros(ng, C, dtype=D, device=dev).index_add_(0, grp, T), rpg)
    return dict(Y=Y32, stats=st, dQ=(d, T, 3), dCtr=dC)


# --------------------------------------------------------------------------- the shapes tests/test_sa_paths_gpu.py runs
#              name              b     n    m    S    C  special
SCATTER_SHAPES = [
    ("cs64_tail",              3,    70,   9,  20,  64, True),
    ("cs32_c32",               3,    70,   9,  20,  32, True),
    ("cs16_c16",               3,    70,   9,   5,  16, True),
    ("cs8_c8",                 3,    70,   9,   3,   8, True),
    ("budget_cs32",            2,  1024,   5,   7,  64, True),
    ("budget_cs16",            2,  2048,   5,   7,  64, True),
    ("budget_cs8",             1,  3000,   5,   7,  64, False),
    ("pooled_s256",            1,   300,   2, 256,  16, False),
    ("stream_gsplit3",         9,    70,  40,  16, 128, True),
    ("smallest",               1,     1,   1,   1,   8, False),
    ("fallback_c8",            2,  5000,   3,   5,   8, True),
    ("fallback_c16",           2,  5000,   3,   5,  16, True),
    ("fallback_c512",          1,  5000,   3,   5, 512, False),
    ("fallback_stream",        1, 14000,   3,   5,  64, False),
    ("split_c32",              3,    70,   9,  16,  32, True),
    ("split_c64",              3,    70,   9,  16,  64, True),
    ("split_c256",             3,    70,   9,  16, 256, True),
    ("q_plus_ctr",             2,    70,  64,  16,  64, True),
]

# hit counts where the default (group 0 full, group 1 a single hit, the rest random) will not do.  pooled_s256 is ONE cloud of two
# 256-row groups: a single-hit group would hand one point a 256-term fp32 sum that carries the whole tensor's norm, and the
# expected relative error of such a sum taken in sequence, sqrt(256 / 3) 2^-24 = 5.5e-7 with a spread of a few times that, sits
# on the relative-RMS bar -- the per-element bound holds there either way, the bar would be decided by the order of the atomics
SCATTER_CNT = {"pooled_s256": [[256, 249]]}


def scatter_case(name, device, seed=0, C=None):
    b, n, m, S, c, special = {k[0]: k[1:] for k in SCATTER_SHAPES}[name]
    return make_case(b, n, m, S, C or c, device, seed=seed, special=special, cnt=SCATTER_CNT.get(name))
