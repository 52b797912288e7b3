"""Shared pieces of the kNN reference tests (tests/test_knn_ref_cpu.py, tests/test_knn_paths_gpu.py): the input families,
the case tables and the hints of the seeded entry point.  Numpy only, seeded; nothing here touches the library.

Path codes of pcops_knn_graph_path: F16 = 3|16 (knn_f16_kernel<20>), MFMA = 2|16 (knn_mfma_kernel<CP, KL>), GENERIC = 1
(knn_graph_kernel<C, TJ>, ignores a seed), 0 = no kernel for the width."""
import numpy as np

from edge_checks import Out, bits_equal, check_sum  # noqa: F401  (one import for the GPU file)

F16, MFMA, GENERIC, NONE = 3 | 16, 2 | 16, 1, 0
OK, BAD_SHAPE, BAD_ARGUMENT, UNSUPPORTED = 0, -2, -3, -4

FAMILIES = ("gauss", "offset", "lattice", "few", "line", "line_rev")
TIES = ("lattice", "few", "line", "line_rev")      # built from exact ties: exempt from the undecided cap, the oracle decides


def cloud(family, b, n, c, seed=0):
    """(b, n, c) float32.
    gauss    : standard normal
    offset   : standard normal, + 50 on the first min(c, 3) channels; from 8 points on, point 5 repeats point 2 and points
               6 and 7 are one ulp above or below it, channel by channel: contract distances that are exactly zero and
               NEGATIVE
    lattice  : {0, .5, 1}^c
    few      : 4 distinct points, repeated in turn
    line     : x_j = -j h e, h = 2^-4, e a fixed direction of multiples of 1/8 (exactly representable, so the two
               candidates at equal steps either side of a query tie exactly in float64); for the far half of the queries
               every later candidate is nearer than all before it
    line_rev : the same points in descending index order"""
    rng = np.random.default_rng(1000 * seed + 7 * n + c)
    if family == "gauss":
        x = rng.standard_normal((b, n, c))
    elif family == "offset":
        x = rng.standard_normal((b, n, c)).astype(np.float32)
        x[:, :, :min(c, 3)] += np.float32(50.0)
        def near(src):                                                  # one ulp up or down, channel by channel
            up = rng.random(src.shape) < 0.5
            return np.where(up, np.nextafter(src, np.float32(np.inf)), np.nextafter(src, np.float32(-np.inf)))
        if n >= 8:
            x[:, 5] = x[:, 2]
            x[:, 6], x[:, 7] = near(x[:, 2]), near(x[:, 2])
    elif family == "lattice":
        x = rng.integers(0, 3, (b, n, c)) * 0.5
    elif family == "few":
        x = rng.standard_normal((b, 4, c))[:, np.arange(n) % 4]
    elif family in ("line", "line_rev"):
        e = rng.integers(-8, 9, (b, 1, c)) / 8.0
        e[:, :, 0] = 1.0
        j = np.arange(n) if family == "line" else np.arange(n)[::-1]
        x = -j.reshape(1, n, 1) * (2.0 ** -4) * e
    else:
        raise ValueError(family)
    return np.ascontiguousarray(x, dtype=np.float32)


def share_cap(n):
    """the k-th candidate of a query is itself undecided: 1 / n of the pairs whatever the input.  From n = 20 down that
    alone is the 0.05 cap, and the condition becomes: nothing but the k-th itself"""
    return max(0.05, 1.0 / n)


# ------------------------------------------------------------------------------------------------ graph cases
# (family, b, n, c, k, misaligned, path)
C_MAIN = {4: 3, 16: 16, 64: 63, 128: 128}
C_ALL = {4: (1, 3, 4), 16: (5, 15, 16), 64: (17, 63, 64), 128: (65, 127, 128)}
K_ALL = {20: (1, 2, 19, 20), 32: (21, 22, 31, 32)}


def _mfma_cases():
    out, f = [], 0

    def add(n, c, k, mis=False, b=2, family=None):
        nonlocal f
        fam = family or FAMILIES[f % len(FAMILIES)]
        f += 1
        if n < 33 and fam == "offset":    # its four near-duplicates are one undecided cluster: over the cap in so small a cloud
            fam = "gauss"
        out.append((fam, b, n, c, k, mis, MFMA))

    for cp in (4, 16, 64, 128):
        cm = C_MAIN[cp]
        # KL = 20: every n edge at one c
        add(1, cm, 1), add(2, cm, 2), add(2, cm, 1), add(19, cm, 19), add(20, cm, 19), add(20, cm, 20), add(21, cm, 20)
        for n in (31, 33, 127, 128, 129, 257):
            add(n, cm, 20)
        # KL = 32: n == k, k + 1 at the smallest and the largest k, then the tile and chunk edges
        add(21, cm, 21), add(22, cm, 21), add(31, cm, 21), add(31, cm, 31), add(32, cm, 32), add(33, cm, 32)
        for n in (127, 128, 129, 257):
            add(n, cm, 32)
        for kl in (20, 32):
            for c in C_ALL[cp]:                                       # every c at n = 129
                if c != cm:
                    add(129, c, kl)
            add(129, cp, kl, mis=True)                                # c == CP off a 16-byte boundary: the scalar loads
            for k in K_ALL[kl][:-1]:                                  # every k at n = 129
                add(129, cm, k)
    add(129, 3, 20, b=9, family="gauss")                              # more clouds than XCDs
    add(129, 3, 32, b=9, family="line")
    add(257, 64, 20, mis=True, family="gauss")                        # c = 64, n >= 256 off a 16-byte boundary: not the fp16 kernel
    return out


MFMA_CASES = _mfma_cases()
NO_PREFILTER_CASES = [("gauss", 2, 256, 64, 20, False, MFMA), ("line", 2, 300, 64, 20, False, MFMA),
                      ("offset", 2, 300, 64, 19, False, MFMA)]       # with PCOPS_OPT_KNN_F16_PREFILTER = 0
F16_CASES = [(FAMILIES[(3 * i + j) % 6], 2, n, 64, k, False, F16)
             for i, n in enumerate((256, 257, 385, 513)) for j, k in enumerate((1, 19, 20))]
F16_CASES += [(fam, 2, 257, 64, 20, False, F16) for fam in ("few", "line")]       # the rotation has them at k = 1 and 19 only
F16_EDGE_INPUTS = ("huge", "subnormal_mix")                          # at (2, 256, 64, 20)
# knn_graph_kernel<C, TJ>: (family, b, n, c, k, misaligned, path); block size the launcher ends with in the docstring table
GENERIC_CASES = [(FAMILIES[(i + j) % 6], 2, n, c, 33, False, GENERIC)
                 for i, c in enumerate((3, 8, 9, 32, 33, 128)) for j, n in enumerate((33, 100, 257))]
GENERIC_CASES += [("gauss", 2, 257, 3, 123, False, GENERIC), ("lattice", 2, 257, 128, 63, False, GENERIC),
                  ("line", 2, 257, 16, 40, True, GENERIC)]
GENERIC_UNSUPPORTED = [(257, 3, 124, GENERIC), (257, 128, 64, GENERIC), (64, 129, 20, NONE), (64, 129, 33, NONE)]   # n, c, k, path


def edge_input(name, b=2, n=256, c=64):
    """the edge inputs of tests/test_knn_gpu.py's fp16-filter test, at the kernel's smallest n"""
    rng = np.random.default_rng(17)
    if name == "huge":
        return (rng.standard_normal((b, n, c)) * 3.0e5).astype(np.float32)        # beyond the fp16 range: the filter is off
    tiny = rng.uniform(3.0e-5, 6.0e-5, (b, n, c))
    small = rng.uniform(2.0e-3, 1.0e-2, (b, n, c))
    return np.where(rng.random((b, n, c)) < 0.5, tiny, small).astype(np.float32)


def case_id(case):
    fam, b, n, c, k, mis, path = case
    return "%s-b%d-n%d-c%d-k%d%s" % (fam, b, n, c, k, "-misaligned" if mis else "")


# ------------------------------------------------------------------------------------------------ seeded cases
# (n, c, k, path): every (CP, KL) of knn_mfma_kernel and the fp16 kernel, at even and odd k and at k = 1
SEEDED_CASES = [(129, c, k, MFMA) for c in (3, 16, 64, 128) for k in (1, 19, 20, 21, 31, 32)]
SEEDED_CASES += [(257, 64, k, F16) for k in (1, 19, 20)]
HINTS = ("exact", "perturbed", "random", "farthest", "one_index", "pair_0_1", "pair_0_2", "pair_last", "minus_one", "index_n")


def hint(kind, x, k, want, d64, rng):
    """(b, n, k) int32.  want: the true graph; d64: float64 distances (b, n, n) as numpy"""
    b, n, c = x.shape
    perm = np.stack([np.stack([rng.permutation(n)[:k] for _ in range(n)]) for _ in range(b)]).astype(np.int32)
    if kind == "exact":              # the true graph itself: the tightest valid bound, only the margin keeps the k-th
        return want.astype(np.int32).copy()
    if kind == "perturbed":          # the graph of slightly different features (DGCNN: the previous layer's)
        y = (x + 0.05 * np.abs(x).max() * rng.standard_normal(x.shape)).astype(np.float32)
        dy = ((y[:, :, None, :].astype(np.float64) - y[:, None, :, :]) ** 2).sum(-1)
        return np.argsort(dy, axis=2, kind="stable")[:, :, :k].astype(np.int32)
    if kind == "random":
        return perm
    if kind == "farthest":
        return np.argsort(-d64, axis=2, kind="stable")[:, :, :k].astype(np.int32)
    if kind == "one_index":          # the nearest point, k times: names one point, bounds nothing
        return np.repeat(want[:, :, :1], k, axis=2).astype(np.int32)
    s = want.astype(np.int32).copy()  # the true neighbours: the tightest bound there is, were the row valid
    if kind == "pair_0_1":           # positions 0 and 1 go to different half-waves
        s[:, ::2, 1] = s[:, ::2, 0]
    elif kind == "pair_0_2":         # positions 0 and 2 go to the same half-wave (only ONE of the two lanes sees the repeat)
        s[:, ::2, 2] = s[:, ::2, 0]
    elif kind == "pair_last":        # positions k - 1 and k - 3, one half-wave: the row names k - 1 points and NOT the k-th;
        s[:, ::2, k - 1] = s[:, ::2, k - 3]                   # trusted, its bound is the (k - 1)-th distance
    elif kind == "minus_one":
        s[:, ::2, 0] = -1
        s[:, 1::4, k - 1] = -1
    elif kind == "index_n":
        s[:, ::2, k // 2] = n
        s[:, 1::4, 0] = n
    else:
        raise ValueError(kind)
    return s


# ------------------------------------------------------------------------------------------------ materialised pair
PAIRWISE_CASES = [(2, n, c) for c in (1, 32, 33, 65) for n in (63, 64, 65)]
TOPK_CASES = [(rows, n, k) for rows in (1, 64, 65) for n in (64, 65, 130) for k in (1, 20, 95) if k <= n]

# ------------------------------------------------------------------------------------------------ edge features
# (graph kind of edge_checks.make_graph, b, n, c, k, misaligned, VEC the launcher takes)
EDGE_CASES = [("knn", 2, 65, 3, 5, False, 1), ("hub", 2, 65, 4, 5, False, 4), ("hub", 2, 65, 4, 5, True, 1),
              ("dup", 2, 33, 64, 20, False, 4), ("knn", 1, 50, 4, 1, False, 4), ("self", 3, 40, 5, 1, False, 1),
              ("hub", 8, 2048, 13, 20, False, 1)]                    # the last: b n k c = 16 640 x 256, the grid-stride loop runs
