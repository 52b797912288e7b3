"""Batch statistics of a first layer that is arithmetic in the offsets (y_c = w_c . o + b_c, never stored), taken from the
nine offset moments (PCOPS_OPT_XYZ_STATS_MOMENTS = 1) or summed over the rebuilt outputs (= 0, the default), both against
the float64 batch mean / variance.

pcops_sa_gather_fwd_rows is called directly with Y = Q = Ctr = NULL; the shifted sums it writes are finalised here the way
pcops_mlp_bn_finalize does (rows added in float64, mean = pivot + s1 / R, var = s2 / R - (s1 / R)^2).  Bar, as in
tests/test_bn_shifted_moments_gpu.py: with a WARM pivot (within a standard deviation of the batch mean) the moments are
right to 1e-6 relative -- the mean relative to max(|mean|, std), since a channel's mean may be zero -- at the shape of the
benchmark's SA1 layer, on all rows and on compacted rows, and with |mean| = 30 std.  off4 and the moment partials must not
depend on the switch at all.

The |mean| = 30 std cases have 65 536 rows and the 128-row case (one group per workgroup, eight partial rows) keeps a small
bias: the form that sums rebuilt outputs rounds every y to fp32 first, an error of 2^-24 |mean| / std = 1.8e-6 standard
deviations per row at |mean| = 30 std, which is above the bar for a single row and only averages below it over thousands
(measured on 128 rows at 30 std: 3.8e-6 on the variance for that form, 1.6e-7 from the moments)."""
import pytest
import torch

from scanobjectnn_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 1e-6


def _inputs(b, n, m, S, C, big, compact, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    idx = torch.randint(0, n, (b, m, S), device=DEV, generator=g, dtype=torch.int32)
    cnt = torch.randint(1, S + 1, (b, m), device=DEV, generator=g, dtype=torch.int32)
    pad = torch.arange(S, device=DEV).view(1, 1, S) >= cnt.unsqueeze(-1)
    idx = torch.where(pad, idx[:, :, :1].expand(b, m, S), idx).contiguous()      # ball-query layout: the tail repeats row 0
    xyz = torch.rand(b, n, 3, device=DEV, generator=g)
    new_xyz = torch.rand(b, m, 3, device=DEV, generator=g)
    W = torch.randn(3, C, device=DEV, generator=g)
    sign = 1.0 - 2.0 * (torch.arange(C, device=DEV) % 2)
    # std of o . w is ~ 0.7 for offsets in (-1, 1)^3: |mean| = 30 std in the `big` case
    bias = (big * 0.7 * sign * (1.0 + 0.1 * torch.rand(C, device=DEV, generator=g))) if big else \
        0.1 * torch.randn(C, device=DEV, generator=g)
    rows = _lib.Rows(cnt, S) if compact else None
    return idx, xyz, new_xyz, W, bias, rows


def _truth(b, n, m, S, idx, xyz, new_xyz, W, bias):
    ii = (idx.long() + (torch.arange(b, device=DEV) * n).view(b, 1, 1)).view(-1)
    o = (xyz.view(b * n, 3)[ii].view(b * m, S, 3) - new_xyz.view(b * m, 1, 3)).view(-1, 3)      # fp32, as the forward
    y = o.double() @ W.double() + bias.double()
    var, mean = torch.var_mean(y, dim=0, unbiased=False)
    return mean, var


def _run(b, n, m, S, C, idx, xyz, new_xyz, W, bias, rows, pivot, switch):
    lib = _lib.load()
    R = rows.num_rows() if rows is not None else b * m * S
    P = lib.pcops_sa_gather_fwd_stats_rows(b, n, m, S, C, 0, 0, 1, int(rows is not None))
    stats = torch.full((P, 2, C), float("nan"), device=DEV)
    mom = torch.full((lib.pcops_sa_gather_stats_rows(b * m), 9), float("nan"), device=DEV)
    off4 = torch.full((R, 4), float("nan"), device=DEV)
    prev = _lib.set_option(_lib.OPT_XYZ_STATS_MOMENTS, switch)
    try:
        _lib.call("pcops_sa_gather_fwd_rows", b, n, m, S, C, None, None, xyz.data_ptr(), new_xyz.data_ptr(), W.data_ptr(),
                  bias.data_ptr(), idx.data_ptr(), None, off4.data_ptr(), stats.data_ptr(), pivot.data_ptr(), mom.data_ptr(),
                  rows.ref if rows is not None else None)
    finally:
        _lib.set_option(_lib.OPT_XYZ_STATS_MOMENTS, prev)
    torch.cuda.synchronize()
    return stats, mom, off4


CASES = [  # name, b, n, m, S, C, big, compact
    ("bench_sa1", 256, 2048, 512, 32, 64, 0.0, False),
    ("bench_sa1_compacted", 256, 2048, 512, 32, 64, 0.0, True),
    ("mean_30_std", 8, 512, 256, 32, 64, 30.0, False),
    ("mean_30_std_compacted", 8, 512, 256, 32, 128, 30.0, True),
    ("few_groups", 2, 64, 4, 16, 32, 0.0, False),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_statistics_of_the_arithmetic_first_layer(case):
    name, b, n, m, S, C, big, compact = case
    idx, xyz, new_xyz, W, bias, rows = _inputs(b, n, m, S, C, big, compact, seed=b + C)
    mean, var = _truth(b, n, m, S, idx, xyz, new_xyz, W, bias)
    std = var.sqrt()
    if big:
        assert (mean.abs() / std).min().item() > 10.0           # the regime under test
    g = torch.Generator(device=DEV).manual_seed(7)
    pivot = (mean + 0.7 * std * torch.randn(C, device=DEV, generator=g).double()).float()      # warm
    Rf = float(b * m * S)
    got = {}
    for switch in (0, 1):
        stats, mom, off4 = _run(b, n, m, S, C, idx, xyz, new_xyz, W, bias, rows, pivot, switch)
        assert torch.isfinite(stats).all() and torch.isfinite(mom).all() and torch.isfinite(off4).all()
        tail_zero = stats.shape[0] == 1 or bool((stats[1:] == 0).all())
        if stats.shape[0] > 1:
            assert tail_zero == bool(switch), "%s: the switch did not select the form under test" % name
        s = stats.double().sum(0)
        bm = pivot.double() + s[0] / Rf
        bv = s[1] / Rf - (s[0] / Rf) ** 2
        em = ((bm - mean).abs() / torch.maximum(mean.abs(), std)).max().item()
        ev = ((bv - var).abs() / var).max().item()
        print("%s switch=%d: mean err %.3g (rel. to max(|mean|, std)), var rel err %.3g" % (name, switch, em, ev))
        got[switch] = (em, ev, mom, off4)
    assert torch.equal(got[0][2], got[1][2]) and torch.equal(got[0][3], got[1][3]), "off4 / moments depend on the switch"
    for switch in (0, 1):
        assert got[switch][0] <= BAR and got[switch][1] <= BAR, "%s switch=%d: %r" % (name, switch, got[switch][:2])
