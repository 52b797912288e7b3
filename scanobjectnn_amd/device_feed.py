"""`--device_feed`: the trainer's input side as ONE libpcops launch per step (`pcops_feed_batch`, csrc/feed.hip; DESIGN.md
section 4.33).  The set lives on the device -- a dense (K, N, 3) tensor, or the raw `.bin` objects of a pickled split list
concatenated once with their offsets -- and the launch picks the step's clouds and their points, gathers labels and the
per-point mask / parts, and applies the augmentation recipe.  Its random numbers are counter-based (Philox4x32-10 keyed by
the seed, counted by epoch, step, position in the epoch's order and output point), NOT `torch.Generator`'s: an augmented
run with the flag draws other rotations and jitter than the run without it, while `--no_augment` on a dense set feeds the
very batches of the host path, bit for bit.  Nothing in the launch changes from step to step but four integers in device
memory (`pcops_feed_set_params`), so a captured step (`captured_step.py`) holds the launch as its first node.

What the host still draws, with the trainer's `rng`: the epoch's cloud order and, for a dense set, the ONE point list all
clouds share (`data_utils.epoch_indices`, call for call what `train.epoch_view` draws).  A ragged set's per-cloud subsets
are the kernel's: the first n outputs of a keyed permutation of every cloud, in place of one NumPy shuffle per cloud."""
import numpy as np
import torch

from . import _lib, data_utils

# recipe 1's constants are provider.jitter_point_cloud's defaults; recipe 2's are named by the model (DEVICE_FEED_RECIPE)
JITTER = {"sigma": 0.01, "clip": 0.05}
NO_CONSTS = {"sigma": 0.0, "clip": 1.0, "smin": 1.0, "smax": 1.0, "tval": 0.0}


def recipe_of(args, mod):
    """(recipe, constants) of pcops_feed_batch for this run: 0 the gather alone (--no_augment), 1 rotate + jitter (the
    trainer's default augmentation), or what the model names in DEVICE_FEED_RECIPE beside an `augment` of its own
    (3DmFV-Net: 2, scale + translate + jitter); None for a model whose `augment` names none"""
    if getattr(args, "no_augment", False):
        return 0, dict(NO_CONSTS)
    if hasattr(mod, "augment"):
        named = getattr(mod, "DEVICE_FEED_RECIPE", None)
        return None if named is None else (int(named["recipe"]), dict(NO_CONSTS, **{k: v for k, v in named.items() if k != "recipe"}))
    return 1, dict(NO_CONSTS, **JITTER)


def refusal(args, mod, own, device=None):
    """None when `--device_feed` may feed this run, else the reason (one line) why it trains on the host-fed path.  Pure:
    decided from the flags, the model's module, its trainer hook and the device's type before anything runs."""
    device = device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu")
    if str(device).split(":")[0] != "cuda":
        return "the run is on the %s: the feed is a HIP kernel and there is no CPU restatement of it in the product" % str(device).upper()
    if own is not None and hasattr(own, "augment"):
        return ("--model %s trains with an augmentation of its own (its trainer hook's), which the feed's recipes do not restate"
                % args.model)
    if recipe_of(args, mod) is None:
        return "--model %s has an augment of its own and names no feed recipe for it (DEVICE_FEED_RECIPE)" % args.model
    return None


def concat_ragged(clouds, labels):
    """a list of (n_i, 3) clouds -> (all points (P, 3) float32, offsets (K + 1) int64, labels (K) int64) on the host"""
    sizes = np.array([pc.shape[0] for pc in clouds], dtype=np.int64)
    pts = np.ascontiguousarray(np.concatenate([np.asarray(pc, dtype=np.float32)[:, :3] for pc in clouds], axis=0))
    return pts, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), np.asarray(labels).reshape(-1).astype(np.int64)


def epoch_draw(rng, num_clouds, num_total_points, num_points, dense):
    """the epoch's host draws -> (shared point list | None, cloud order).  Dense: data_utils.epoch_indices, the two
    shuffles of `train.epoch_view`; ragged: the cloud order alone"""
    if dense:
        return data_utils.epoch_indices(num_clouds, num_total_points, num_points, rng)
    order = np.arange(num_clouds)
    rng.shuffle(order)
    return None, order


class DeviceFeed:
    """data: (K, N, 3) float32 device tensor with labels (K) and mask (K, N) | None as `train.prepare_set` returns them, or
    its list of centred / normalised ragged arrays with their labels (uploaded here, once).  batch: the rows one launch of
    this rank builds; seed: the Philox key; recipe, consts: `recipe_of`."""

    def __init__(self, data, labels, mask, num_point, batch, seed, recipe, consts, device):
        self.dev = torch.device(device)
        self.n, self.batch, self.seed, self.recipe, self.consts = int(num_point), int(batch), int(seed), int(recipe), dict(consts)
        if isinstance(data, list):
            pts, offsets, lab = concat_ragged(data, labels)
            self.dense, self.ntot = False, 0
            self.min_points = int(np.diff(offsets).min())
            if int(np.diff(offsets).max()) >= 2 ** 31:
                raise ValueError("a cloud of 2^31 points or more")
            self.pts = torch.as_tensor(pts, device=self.dev)
            self.offsets = torch.as_tensor(offsets, device=self.dev)
            self.labels = torch.as_tensor(lab, device=self.dev)
            self.side = None
            self.K = len(data)
        else:
            self.dense, (self.K, self.ntot) = True, (int(data.shape[0]), int(data.shape[1]))
            self.min_points = self.ntot
            self.pts = _lib.check(data, torch.float32, "data", 3)
            self.offsets = None
            self.labels = _lib.check(labels, torch.int64, "labels", 1)
            self.side = _lib.check(mask, torch.int64, "mask", 2) if mask is not None else None
        if self.n > self.min_points:
            raise ValueError("cloud with %d < %d points" % (self.min_points, self.n))
        self.mode = 0 if self.dense else 1
        self.order = torch.zeros(self.K, dtype=torch.int32, device=self.dev)
        self.idx_pts = torch.zeros(self.n, dtype=torch.int32, device=self.dev) if self.dense else None
        self.params = torch.zeros(4, dtype=torch.int32, device=self.dev)
        self.x = torch.zeros((self.batch, self.n, 3), dtype=torch.float32, device=self.dev)
        self.y = torch.zeros(self.batch, dtype=torch.int64, device=self.dev)
        self.m = torch.zeros((self.batch, self.n), dtype=torch.int64, device=self.dev) if self.side is not None else None
        self.epoch = 0

    def begin_epoch(self, rng, epoch):
        """draw the epoch's cloud order (and, dense, its shared point list) with the trainer's rng and upload them"""
        idx_pts, order = epoch_draw(rng, self.K, self.ntot, self.n, self.dense)
        self.order.copy_(torch.as_tensor(np.asarray(order).astype(np.int32)))
        if idx_pts is not None:
            self.idx_pts.copy_(torch.as_tensor(np.asarray(idx_pts).astype(np.int32)))
        self.epoch = int(epoch)

    def set_batch(self, first, step):
        """the next launch builds the rows whose positions in the epoch's order start at `first`, with `step`'s draws: the
        three integers into device memory, as the arguments of an ordinary launch on the current stream"""
        _lib.call("pcops_feed_set_params", int(first), int(step), self.epoch, self.params.data_ptr())

    def _launch(self, rows, recipe, x, y, m):
        c = self.consts
        _lib.call("pcops_feed_batch", self.K, self.ntot, rows, self.n, self.mode, recipe, self.min_points,
                  self.pts.data_ptr(), _lib.ptr(self.offsets), self.labels.data_ptr(), _lib.ptr(self.side),
                  self.order.data_ptr(), _lib.ptr(self.idx_pts), self.params.data_ptr(), self.seed, float(c["sigma"]),
                  float(c["clip"]), float(c["smin"]), float(c["smax"]), float(c["tval"]), x.data_ptr(), y.data_ptr(),
                  _lib.ptr(m))

    def launch(self):
        """fill the static x, y, m from the parameters in device memory: the launch a captured step replays"""
        self._launch(self.batch, self.recipe, self.x, self.y, self.m)
        return self.x, self.y, self.m

    def epoch_view(self):
        """the whole epoch in one launch, unaugmented: (clouds (K, n, 3), labels (K), mask | None) in the epoch's order --
        what `data_utils.get_current_data` builds on the host for a ragged set.  The step's parameters are put back."""
        x = torch.empty((self.K, self.n, 3), dtype=torch.float32, device=self.dev)
        y = torch.empty(self.K, dtype=torch.int64, device=self.dev)
        m = torch.empty((self.K, self.n), dtype=torch.int64, device=self.dev) if self.side is not None else None
        saved = self.params.clone()
        for lo in range(0, self.K, 65535):                       # a launch takes at most 65 535 rows
            hi = min(self.K, lo + 65535)
            self.set_batch(lo, 0)
            self._launch(hi - lo, 0, x[lo:hi], y[lo:hi], m[lo:hi] if m is not None else None)
        self.params.copy_(saved)
        return x, y, m
