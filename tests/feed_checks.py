"""What the feed's CPU and GPU tests share: the case tables, the synthetic sets, the error bar and the comparisons."""
import numpy as np

import feed_ref as R

SEED = 0x1234567890ABCDEF          # both key words non-zero
EPS = 2.0 ** -24                   # unit roundoff of fp32 (half the spacing at 1)
ULPS = 4                           # "a few ulp" for sinf / cosf / logf of any implementation under test (the device library
                                   # documents 1 to 2; NumPy's float32 loops stay under 4)


def bar(recipe, **kw):
    """Absolute bound on |fp32 result - float64 restatement| per coordinate, for input points inside the unit ball.  Derived
    from the statements of the recipe, every fp32 operation contributing its rounding (EPS relative):

    angle      theta = fl(fl(2 pi) u), theta <= 2 pi: the constant's and the product's rounding,  d_theta = 2 pi 2 EPS
    cos / sin  of the rounded angle, values <= 1 (spacing there <= EPS):                           d_trig  = d_theta + ULPS EPS
    rotation   x c - z s with x^2 + z^2 <= 1, so |x| + |z| <= sqrt 2; two products and one sum of values <= 1:
                                                                                                  sqrt 2 d_trig + 3 EPS
    normal     r = sqrt(-2 ln u), u >= 2^-24, so r <= sqrt(48 ln 2) = 5.77; logf is ULPS ulp RELATIVE (2 EPS each), the
               factor -2 is exact, the root halves a relative error and rounds once: rel_r = ULPS EPS + EPS;
               z = r cos(a):  d_z = r_max (d_trig + rel_r + EPS)
    jitter     min(max(sigma z, -clip), clip), the product's rounding on a value that matters only below clip:
                                                                                                  sigma d_z + EPS clip
    scale      s = smin + fl(fl(smax - smin) u): d_s = 2 EPS span + EPS S, S = max(|smin|, |smax|); t = fl((2 u - 1) tval),
               2 u - 1 exact: d_t = EPS tval; v s + t with |v| <= 1: d_s + EPS S + d_t + EPS (S + tval)
    last sum   v' + jitter, |result| <= top = 1 + clip (recipe 1) or S + tval + clip (recipe 2, at most 1.75 with the
               model's constants):                                                                EPS top

    Measured in fp32 over every case of RECIPE_CASES, NumPy on the CPU and the kernel on the MI355X alike: recipe 1 at most
    1.11e-7 against a bar of 1.72e-6, recipe 2 at most 1.27e-7 against 5.77e-7."""
    if recipe == 0:
        return 0.0
    c = {k: float(np.float32(v)) for k, v in dict(R.RECIPE_CONSTS, **kw).items()}
    d_theta = 2.0 * np.pi * 2.0 * EPS
    d_trig = d_theta + ULPS * EPS
    r_max = np.sqrt(48.0 * np.log(2.0))
    d_z = r_max * (d_trig + (ULPS * EPS + EPS) + EPS)
    jit = c["sigma"] * d_z + EPS * c["clip"]
    if recipe == 1:
        return np.sqrt(2.0) * d_trig + 3.0 * EPS + jit + EPS * (1.0 + c["clip"])
    S, span = max(abs(c["smin"]), abs(c["smax"])), c["smax"] - c["smin"]
    d_s, d_t = 2.0 * EPS * span + EPS * S, EPS * c["tval"]
    return d_s + EPS * S + d_t + EPS * (S + c["tval"]) + jit + EPS * (S + c["tval"] + c["clip"])


# ---- sets --------------------------------------------------------------------------------------------------------------
def ball_clouds(sizes, seed):
    """clouds of the given sizes inside the unit ball (centred, largest norm 1, as the trainer prepares them), distinct
    labels, and a per-point side value that names its cloud and point"""
    rng = np.random.RandomState(seed)
    clouds, side = [], []
    for i, s in enumerate(sizes):
        p = rng.standard_normal((s, 3)).astype(np.float32)
        if s > 1:
            p = p - p.mean(axis=0, dtype=np.float32)
        p = p / max(np.sqrt((p * p).sum(axis=-1, dtype=np.float32)).max(), np.float32(1e-6))
        clouds.append(p.astype(np.float32))
        side.append(np.arange(s, dtype=np.int64) + 1000003 * (i + 1))
    labels = 100 + 7 * np.arange(len(sizes))
    return clouds, labels, side


def dense_set(K, N, seed=11):
    return R.make_set(*ball_clouds([N] * K, seed))


def ragged_sizes(n):
    return [n, n + 1, 2 * n - 1, 1024, 1025, 70001]


def ragged_set(n, seed=12):
    return R.make_set(*ball_clouds(ragged_sizes(n), seed))


def shared_indices(N, n, seed=5):
    """the point list and cloud order data_utils.epoch_indices would draw"""
    rng = np.random.RandomState(seed)
    idx = np.arange(N)
    rng.shuffle(idx)
    return idx[:n].astype(np.int32)


def order_of(K, seed=6):
    rng = np.random.RandomState(seed)
    o = np.arange(K)
    rng.shuffle(o)
    return o.astype(np.int32)


# dense, mode 0, recipe 0 (K = 5, B = 3): (N, n, first).  N = 70 for every n it can hold; n = 130 on 70 points is the
# launcher's BAD_SHAPE case and runs on N = 140 here; n = 300 crosses the 256-point workgroup
DENSE_CASES = [(70, n, first) for n in (1, 33, 64, 65) for first in (0, 2)] + \
              [(140, 130, first) for first in (0, 2)] + [(310, 300, first) for first in (0, 2)]
# ragged, mode 1, recipe 0: n (cloud sizes ragged_sizes(n)); 300 crosses the 256-point workgroup
RAGGED_N = (33, 130, 300)
# recipes 1 and 2: (kind, n, first, B); first = 2 makes the global position differ from the row
RECIPE_CASES = [(kind, n, first, 3) for kind in ("dense", "ragged") for n in (33, 130) for first in (0, 2)] + \
               [("ragged", 300, 2, 3)]
WRONG = {1: ("rot_sign", "jitter_first", "local_row"), 2: ("scale_after_translation", "local_row")}


def recipe_case(kind, n, first, B, recipe, step=3, epoch=2, dtype=np.float64, wrong=None):
    """the restated batch of one RECIPE_CASES entry, and the launch's arguments"""
    if kind == "dense":
        S, mode, idx = dense_set(5, 140 if n <= 140 else n + 10), 0, None
        idx = shared_indices(S["ntot"], n)
    else:
        S, mode, idx = ragged_set(n), 1, None
    order = order_of(S["K"])
    want = R.feed_batch(S, order, first, B, n, mode, idx, step, epoch, SEED, recipe, kind == "dense", dtype=dtype, wrong=wrong)
    return S, order, mode, idx, want


# ---- comparisons -------------------------------------------------------------------------------------------------------
def exact_mismatch(got, want):
    """None when (x, y, m) equal bit for bit, else what differs"""
    for name, g, w in zip("xym", got, want):
        if (g is None) != (w is None):
            return "%s: one side has none" % name
        if g is not None and not np.array_equal(np.asarray(g), np.asarray(w).astype(np.asarray(g).dtype)):
            return "%s differs" % name
    return None


def bar_excess(got, want, bound):
    """(largest |got.x - want.x|, whether it is inside the bound AND y and m are equal)"""
    err = float(np.abs(np.asarray(got[0], dtype=np.float64) - np.asarray(want[0], dtype=np.float64)).max())
    same = np.array_equal(got[1], want[1]) and ((got[2] is None and want[2] is None) or np.array_equal(got[2], want[2]))
    return err, bool(err <= bound and same)


# ---- inclusion statistics ----------------------------------------------------------------------------------------------
def inclusion_z(counts, clouds, take, ni):
    """normal score of the finite-population-corrected chi-square of per-point inclusion counts: every point is in a cloud's
    first `take` outputs with p = take / ni; over `clouds` independent clouds a count has variance clouds p (1 - p), and
    since every cloud's inclusions sum to `take` exactly, sum (count - mean)^2 / (clouds p (1 - p)) has ni - 1 degrees of
    freedom, each with the factor ni / (ni - 1) of sampling without replacement; z = (X - dof) / sqrt(2 dof)"""
    p = take / ni
    x2 = ((counts - clouds * p) ** 2).sum() / (clouds * p * (1.0 - p)) * (ni - 1) / ni
    dof = ni - 1
    return (x2 - dof) / np.sqrt(2.0 * dof)
