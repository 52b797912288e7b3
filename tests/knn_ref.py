"""The kNN graph held to the operation itself: the k nearest points in exact arithmetic (float64 from the fp32 inputs), and
the band inside which a fp32 evaluation of the library's arithmetic contract may move a distance.  Plain torch, no library
calls; numpy arrays and tensors on any device are taken as they are.

Contract (scanobjectnn_amd/csrc/knn.hip, oracle/pcops_oracle.c):  D_ij = (s_i + (-2 inner_ij)) + s_j  with inner and s c-term
fmaf chains from +0.  Against the exact D64_ij = sum_l (x_il - x_jl)^2 = s_i - 2 inner_ij + s_j:
  * a c-term fmaf chain is within gamma_c = c u / (1 - c u) of its exact value relative to the sum of the magnitudes of its
    terms (u = 2^-24): |fl(s_i) - s_i| <= gamma_c s_i, and by Cauchy-Schwarz and AM-GM
    |fl(inner) - inner| <= gamma_c sum_l |x_il x_jl| <= gamma_c sqrt(s_i s_j) <= gamma_c (s_i + s_j) / 2;
  * the three inputs of the two additions therefore carry at most gamma_c (s_i + (s_i + s_j) + s_j) = 2 gamma_c (s_i + s_j);
  * each of the two additions rounds once, on a magnitude of at most s_i + 2 sqrt(s_i s_j) + s_j <= 2 (s_i + s_j) (plus the
    perturbations above): 2 x 2 u (s_i + s_j) (1 + O(c u));
  * in all (2 c + 4) u (s_i + s_j) (1 + O(c u)) <= 2 (c + 3) u (s_i + s_j) for c <= 128  --  the band.
Two lists that both follow the contract to within the band can only differ in pairs whose exact distance lies within two
bands of the exact k-th distance: those pairs are `undecided`, and for them (only) check_lists is vacuous.
"""
import torch

U = 2.0 ** -24
UNDECIDED_CAP = 0.05      # share of (query, candidate) pairs a case not built from exact ties may leave undecided


def _x64(x):
    x = torch.as_tensor(x)
    assert x.dtype == torch.float32 and x.dim() == 3
    return x.double()


def dist64(x):
    """D64[b, i, j] = sum_l (x_il - x_jl)^2 in float64, one channel at a time (nothing of size n n c)"""
    x = _x64(x)
    b, n, c = x.shape
    d = torch.zeros(b, n, n, dtype=torch.float64, device=x.device)
    for l in range(c):
        col = x[:, :, l]
        d += (col[:, :, None] - col[:, None, :]) ** 2
    return d


def band(x):
    """2 (c + 3) 2^-24 (s_i + s_j), s the float64 squared norms"""
    x = _x64(x)
    s = (x * x).sum(dim=2)
    return 2.0 * (x.shape[2] + 3) * U * (s[:, :, None] + s[:, None, :])


def check_lists(x, nn, k):
    """every query of every cloud: k distinct indices in [0, n), and no selected candidate provably farther than an
    unselected one: max over selected (D64 - band) <= min over unselected (D64 + band).  Returns the number of queries."""
    x = torch.as_tensor(x)
    nn = torch.as_tensor(nn).to(x.device).long()
    b, n, c = x.shape
    assert tuple(nn.shape) == (b, n, k), "lists of shape %s for %s" % (tuple(nn.shape), (b, n, k))
    bad = (nn < 0) | (nn >= n)
    assert not bad.any(), "%d indices outside [0, %d), first at %s: %d" % (
        int(bad.sum()), n, tuple(torch.nonzero(bad)[0].tolist()), int(nn[bad][0]))
    srt = nn.sort(dim=2).values
    rep = (srt[:, :, 1:] == srt[:, :, :-1]).any(dim=2)
    assert not rep.any(), "%d queries repeat an index, first (cloud, query) %s" % (
        int(rep.sum()), tuple(torch.nonzero(rep)[0].tolist()))
    d, bd = dist64(x), band(x)
    sel = torch.zeros(b, n, n, dtype=torch.bool, device=d.device)
    sel.scatter_(2, nn, True)
    inf = torch.tensor(float("inf"), dtype=torch.float64, device=d.device)
    far_sel = torch.where(sel, d - bd, -inf).amax(dim=2)
    near_unsel = torch.where(sel, inf, d + bd).amin(dim=2)              # n == k: nothing unselected, +inf
    wrong = far_sel > near_unsel
    assert not wrong.any(), "%d queries select a point provably farther than one they leave out, first (cloud, query) %s: " \
        "selected D64 - band %.9g > unselected D64 + band %.9g" % (
            int(wrong.sum()), tuple(torch.nonzero(wrong)[0].tolist()), far_sel[wrong][0].item(), near_unsel[wrong][0].item())
    return b * n


def undecided_share(x, k):
    """share of (query, candidate) pairs with |D64 - k-th smallest D64 of the query| <= 2 band"""
    d, bd = dist64(x), band(x)
    kth = d.kthvalue(k, dim=2).values
    return ((d - kth[:, :, None]).abs() <= 2.0 * bd).double().mean().item()


def contract_ratio(x, adj):
    """worst |adj - D64| / band over the pairs with a positive band (a fp32 evaluation of the contract against the band)"""
    d, bd = dist64(x), band(x)
    err = (torch.as_tensor(adj).to(d.device).double() - d).abs()
    zero = bd == 0
    assert (err[zero] == 0).all()
    return (err[~zero] / bd[~zero]).max().item() if (~zero).any() else 0.0
