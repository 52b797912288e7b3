"""`--graph`: one training step -- forward, loss, backward, gradient collection, optimiser, metric accumulation -- captured
ONCE as a HIP graph and replayed every step, so that the host issues one graph launch where the eager step issues some
hundreds to thousands of kernel launches.  (`graph.py` is the TF1-style variable store; this
module is the captured step.)

What makes the step capturable: it has no host synchronisation, libpcops allocates nothing and takes torch's current
stream (`_lib.call`), and the one value that changes on every step and entered a kernel by value, Adam's lr_t, is read
from device memory by `pcops_adam_step_dev` (`train_util.TFAdam.set_lr` fills it ahead of every replay, on the same
stream; the fill carries the value as a launch argument).  What stays outside the graph: the epoch's index gather, batch
slicing and augmentation (the trainer's own generator), which copy into the static inputs held here.

Values baked into a capture: `bn_decay` (the BN moving-average updates take it as a Python number) and, for the
momentum optimiser, `lr`.  Both are staircases that move rarely; `needs_capture` asks for a new capture when one of them
changes, and a re-capture frees the previous graph and its memory pool first.

Before every capture the step runs eagerly on the capture stream (WARMUP_STEPS times) so that every lazily built cache --
stack plans, `pointnet_util._whole_cloud_group`, `fused_mlp._unit_coef`, `Rows` buffers, the library's once-per-process
function attributes -- exists before a launch could be recorded instead of run; parameters, optimiser moments, BN moving
statistics, the running sums, Adam's `t` and the device's random state are then put back, so a captured run is step for
step the eager run.

Whether a run may be captured is decided BEFORE anything is captured, by `refusal`, a pure function of the flags, the
world size and the environment -- never by catching a failed capture.
"""
import torch

from . import train_util as TU

# the families whose captured step is held to their eager step, bit for bit, by tests/test_captured_step_gpu.py
VERIFIED_MODELS = ("pointnet2_cls_ssg", "dgcnn", "pointcnn_cls", "pointnet_cls")
WARMUP_STEPS = 2


def refusal(args, world, environ):
    """None when `--graph` may capture this run, else the reason (one line) why it trains eagerly instead"""
    if world > 1:
        return ("%d ranks: the overlapped gradient all-reduce runs on side streams, and a graph with parallel branches "
                "is out of scope" % world)
    if environ.get("PCOPS_SYNC", "0") == "1":
        return "PCOPS_SYNC=1 synchronises the device after every libpcops call, which a capture cannot contain"
    if environ.get("PCOPS_FUSED_ADAM", "1") == "0":
        return "PCOPS_FUSED_ADAM=0 takes Adam's step size by value in torch operators; only pcops_adam_step_dev reads it from the device"
    if getattr(args, "sync_bn", False):
        return "--sync_bn exchanges the batch statistics between ranks inside the forward pass"
    path = getattr(args, "train_file", "") or ""
    if path and not path.endswith(".npz") and ".h5" not in path and not getattr(args, "device_feed", False):
        return "%s: a list of raw .bin objects is a ragged set sampled on the host every epoch" % path
    if args.model not in VERIFIED_MODELS:
        return ("--model %s is not on the list of families whose captured step is verified against their eager step (%s)"
                % (args.model, ", ".join(VERIFIED_MODELS)))
    return None


def baked_values(optimizer, lr, bn_decay):
    """the schedule values a capture holds as constants: bn_decay, and lr for the momentum optimiser (Adam's step size is
    read from device memory)"""
    return (float(bn_decay),) if optimizer == "adam" else (float(bn_decay), float(lr))


def needs_capture(captured, wanted):
    """does a step whose baked values are `wanted` need a new capture, `captured` being those of the graph at hand (None:
    there is none yet)"""
    return captured is None or tuple(captured) != tuple(wanted)


class CapturedStep:
    """body(x, y, m, bn_decay, tot, update): one training step on the static inputs, adding its loss / correct / seen to
    `tot` and calling `update()` where the optimiser steps.  x (B,N,3) float32, y the labels, m the per-point mask or
    parts (None for a classifier): examples that give the static buffers their shapes and dtypes.
    feed (device_feed.DeviceFeed, optional): the static inputs are the feed's buffers and its launch is the first node of the
    captured body; x, y, m are then not read, and `step` moves the feed's parameters instead of copying a batch in."""

    def __init__(self, body, net, fp, opt, x, y, m=None, feed=None):
        self.net, self.fp, self.opt, self.feed = net, fp, opt, feed
        self.body = body if feed is None else self._fed(body)
        dev = fp.flat.device
        self.adam = isinstance(opt, TU.TFAdam)
        if self.adam:
            opt.enable_device_lr()
        if feed is not None:
            self.x, self.y, self.m = feed.x, feed.y, feed.m
        else:
            self.x, self.y = torch.zeros_like(x, device=dev), torch.zeros_like(y, device=dev)
            self.m = torch.zeros_like(m, device=dev) if m is not None else None
        self.tot = torch.zeros(3, dtype=torch.float64, device=dev)      # loss sum, correct, seen: accumulated in the graph
        self.stream = torch.cuda.Stream(dev)                             # warm-up and capture: one stream, a linear graph
        self.graph = None
        self.baked = None
        self.captures = 0

    def _fed(self, body):
        """the feed's launch, then the step: it reads its parameters from device memory and changes none of them, so the
        warm-up steps leave them as they found them"""
        def fed(x, y, m, bn_decay, tot, update):
            self.feed.launch()
            body(x, y, m, bn_decay, tot, update)
        return fed

    def _state(self):
        """every tensor a step changes that the next step reads"""
        moments = [self.opt.m, self.opt.v] if self.adam else [self.opt.accum]
        return [self.fp.flat] + moments + list(self.net.buffers()) + [self.tot]

    def _update(self, lr, captured):
        if not self.adam:
            self.opt.step(lr)                            # TFMomentum: torch operators with lr baked into them
            return
        if not captured:
            self.opt.set_lr(lr)
        self.opt.step_from_device_lr()

    def release(self):
        """free the graph at hand and the memory pool it replays in"""
        if self.graph is None:
            return
        torch.cuda.current_stream().synchronize()        # the last replay has left the pool
        self.graph.reset()
        self.graph = None
        torch.cuda.empty_cache()

    def capture(self, lr, bn_decay):
        self.release()
        dev = self.fp.flat.device
        state = self._state()
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            saved = [t.clone() for t in state]
            t, rng = getattr(self.opt, "t", None), torch.cuda.get_rng_state(dev)
            for _ in range(WARMUP_STEPS):
                self.body(self.x, self.y, self.m, bn_decay, self.tot, lambda: self._update(lr, False))
            for dst, src in zip(state, saved):
                dst.copy_(src)
            if self.adam:
                self.opt.t = t
            torch.cuda.set_rng_state(rng, dev)
            del saved
        torch.cuda.current_stream().wait_stream(self.stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=self.stream):
            self.body(self.x, self.y, self.m, bn_decay, self.tot, lambda: self._update(lr, True))
        self.graph = graph
        self.captures += 1

    def step(self, x, y, m, lr, bn_decay, batch=None):
        """one training step on (x, y, m): into the static inputs, a new capture where the schedule asks for one, Adam's
        step size into its device scalar, one replay.  With a feed: batch = (first, step) into the feed's parameters, ahead
        of a capture's warm-up steps as well, and no copy"""
        if self.feed is not None:
            self.feed.set_batch(*batch)
        else:
            self.x.copy_(x)
            self.y.copy_(y)
            if self.m is not None:
                self.m.copy_(m)
        wanted = baked_values("adam" if self.adam else "momentum", lr, bn_decay)
        if needs_capture(self.baked, wanted):
            self.capture(lr, bn_decay)
            self.baked = wanted
        if self.adam:
            self.opt.set_lr(lr)
        self.graph.replay()
