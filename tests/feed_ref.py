"""NumPy restatement of the device-resident feed (include/pcops.h "Device-resident feed", scanobjectnn_amd/csrc/feed.hip):
Philox4x32-10, the uniform and normal maps, the per-cloud Feistel permutation and the three recipes.  Float64 by default
(`dtype=np.float32` evaluates the same statements in fp32, one rounding per operation, as the kernel does).  `wrong=`
switches ONE statement to a plausible mistake, for the tests that show the checks notice it:
  "rot_sign"                 the transposed rotation (x c + z s, -x s + z c)
  "jitter_first"             jitter before the rotation
  "scale_after_translation"  (v + t) s instead of v s + t
  "local_row"                the row inside the launch instead of g = first + r in the counters
  "swapped_half"             the Feistel network started from (R, L)
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
TAG_CLOUD, TAG_JIT, TAG_PERM = 0x434c4f55, 0x4a495454, 0x5045524d        # include/pcops.h PCOPS_FEED_TAG_*
MASK = np.uint64(0xffffffff)
S32 = np.uint64(32)
RECIPE_CONSTS = {"sigma": 0.01, "clip": 0.05, "smin": 0.66, "smax": 1.5, "tval": 0.2}


def philox(c0, c1, c2, c3, key):
    """Philox4x32-10 of the counters (arrays broadcast against each other) under key (k0, k1) -> (..., 4) uint32"""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(v).astype(np.uint64) & MASK for v in (c0, c1, c2, c3)])
    k0, k1 = int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def key_of(seed):
    return int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff


def uniform(w):
    """((w >> 9) + 0.5) 2^-23 in float64 (exact in fp32 as well)"""
    return ((np.asarray(w, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def normals(w, dtype=np.float64):
    """(..., 4) words -> (..., 3) Box-Muller normals z0, z1, z2"""
    u = uniform(w).astype(dtype)
    two_pi = dtype(2.0 * np.pi)
    r0, a0 = np.sqrt(dtype(-2.0) * np.log(u[..., 0])), two_pi * u[..., 1]
    r2, a2 = np.sqrt(dtype(-2.0) * np.log(u[..., 2])), two_pi * u[..., 3]
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r2 * np.cos(a2)], axis=-1)


# ---- the permutation ---------------------------------------------------------------------------------------------------
def feistel_f(v, k, w):
    v = (v ^ np.uint64(k)) & MASK
    v = (v * np.uint64(0x9E3779B1)) & MASK
    v = v ^ (v >> np.uint64(15))
    v = (v * np.uint64(0x85EBCA6B)) & MASK
    v = v ^ (v >> np.uint64(13))
    return v & np.uint64((1 << w) - 1)


def perm_keys(seed, cloud, epoch):
    return [int(k) for t in (0, 1) for k in philox(cloud, epoch, t, TAG_PERM, key_of(seed))]


def network(x, bits, keys, wrong=None):
    """one pass of the 8-round unbalanced Feistel network over [0, 2^bits)"""
    a = bits // 2
    b = bits - a
    x = np.asarray(x, dtype=np.uint64)
    L, R = x >> np.uint64(b), x & np.uint64((1 << b) - 1)
    wl, wr = a, b
    if wrong == "swapped_half":
        L, R = x & np.uint64((1 << a) - 1), x >> np.uint64(a)
    for r in range(8):
        L, R = R, L ^ feistel_f(R, keys[r], wl)
        wl, wr = wr, wl
    return (L << np.uint64(b)) | R


def perm(ni, keys, count=None, wrong=None):
    """perm(0), ..., perm(count - 1) of a cloud of ni points (count: ni), int64"""
    bits = max(int(ni - 1).bit_length(), 2)
    cur = np.arange(ni if count is None else count, dtype=np.uint64)
    out = np.zeros(cur.shape, dtype=np.int64)
    todo = np.arange(cur.size)
    while todo.size:
        cur = network(cur, bits, keys, wrong)
        done = cur < np.uint64(ni)
        out[todo[done]] = cur[done].astype(np.int64)
        todo, cur = todo[~done], cur[~done]
    return out


# ---- the batch ---------------------------------------------------------------------------------------------------------
def make_set(clouds, labels, side=None):
    """a list of (n_i, 3) float32 clouds (equal sizes: also usable as a dense set) -> the arrays the launch takes"""
    sizes = np.array([c.shape[0] for c in clouds], dtype=np.int64)
    S = {"K": len(clouds), "pts": np.ascontiguousarray(np.concatenate(clouds, axis=0), dtype=np.float32),
         "offsets": np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), "labels": np.asarray(labels, dtype=np.int64),
         "side": None if side is None else np.concatenate(side).astype(np.int64), "min_points": int(sizes.min()),
         "ntot": int(sizes[0]) if (sizes == sizes[0]).all() else 0}
    return S


def consts(dtype, **kw):
    """the recipe constants as the launch passes them (float) in the arithmetic's type"""
    c = dict(RECIPE_CONSTS, **kw)
    return {k: dtype(np.float32(v)) for k, v in c.items()}


def jitter(v, g, step, seed, C, dtype):
    z = normals(philox(g, step, np.arange(v.shape[0]), TAG_JIT, key_of(seed)), dtype)
    return v + np.clip(C["sigma"] * z, -C["clip"], C["clip"])


def augment(v, g, step, seed, recipe, C, dtype=np.float64, wrong=None):
    """one cloud's (n, 3) points through the recipe; g: the cloud's global position in the epoch's order"""
    v = v.astype(dtype)
    if recipe == 0:
        return v
    d0 = uniform(philox(g, step, 0, TAG_CLOUD, key_of(seed))).astype(dtype)
    if recipe == 1:
        if wrong == "jitter_first":
            v = jitter(v, g, step, seed, C, dtype)
        theta = dtype(2.0 * np.pi) * d0[0]
        c, s = np.cos(theta), np.sin(theta)
        if wrong == "rot_sign":
            s = -s
        v = np.stack([v[:, 0] * c - v[:, 2] * s, v[:, 1], v[:, 0] * s + v[:, 2] * c], axis=1)
        return v if wrong == "jitter_first" else jitter(v, g, step, seed, C, dtype)
    d1 = uniform(philox(g, step, 1, TAG_CLOUD, key_of(seed))).astype(dtype)
    scale = C["smin"] + (C["smax"] - C["smin"]) * d0[:3]
    shift = (dtype(2.0) * d1[:3] - dtype(1.0)) * C["tval"]
    v = (v + shift) * scale if wrong == "scale_after_translation" else v * scale + shift
    return jitter(v, g, step, seed, C, dtype)


def select(S, c, n, mode, idx_pts, epoch, seed, dense, wrong=None):
    """(first point of cloud c, the n source points the output points read)"""
    base = c * S["ntot"] if dense else int(S["offsets"][c])
    ni = S["ntot"] if dense else int(S["offsets"][c + 1]) - base
    src = np.asarray(idx_pts[:n], dtype=np.int64) if mode == 0 else perm(ni, perm_keys(seed, c, epoch), n, wrong)
    return base, src


def feed_batch(S, order, first, B, n, mode, idx_pts, step, epoch, seed, recipe, dense, dtype=np.float64, wrong=None, **kw):
    """-> x (B, n, 3) dtype, y (B) int64, m (B, n) int64 or None, as pcops_feed_batch defines them"""
    C = consts(dtype, **kw)
    x, y = np.zeros((B, n, 3), dtype=dtype), np.full(B, -1, dtype=np.int64)
    m = None if S["side"] is None else np.zeros((B, n), dtype=np.int64)
    for r in range(B):
        g = first + r
        if g >= S["K"]:
            continue
        c = int(order[g])
        base, src = select(S, c, n, mode, idx_pts, epoch, seed, dense, wrong)
        x[r] = augment(S["pts"][base + src], r if wrong == "local_row" else g, step, seed, recipe, C, dtype, wrong)
        y[r] = S["labels"][c]
        if m is not None:
            m[r] = S["side"][base + src]
    return x, y, m
