"""``torch.autograd.Function`` wrappers around the C ABI (``native.py`` / ``include/ctvae_hip.h``).

Conventions
-----------
* Activations are plain contiguous NHWC tensors ``[B,H,W,C]`` inside this module; the model layer
  (``models/``) exposes them as logical-NCHW ``permute(0,3,1,2)`` views (= torch channels_last).
* Weights are parameters whose *memory* is the packed ``[kh*kw][Ci][Co]`` layout while their logical
  shape/strides are PyTorch's (``models/packing.py``); kernels receive ``param.data_ptr()``.
* Parameter gradients are written by the wgrad kernels straight into ``param.grad`` (same packed memory
  layout, accumulate semantics like autograd); ``backward`` therefore returns ``None`` for parameters.
  DDP hooks on parameters do not fire -- use ``ctvae_amd.ddp.GradBucketAllReduce``.
* No op here has a PyTorch/CPU fallback: a missing library or a CPU tensor raises.
"""
import math
import weakref
from dataclasses import dataclass

import torch
from torch.autograd import Function

from . import native

ACT_NONE, ACT_LRELU, ACT_RELU, ACT_TANH = 0, 1, 2, 3
CONV, CONVT = 0, 1
CONV_FLAT = CONV | 0x100   # CTVAE_W_CI_TAP: nn.Linear over torch.flatten(NCHW [B,ci,k,k]) run as a k x k conv of the NHWC tensor
BN_MOMENTUM, BN_EPS = 0.1, 1e-5      # nn.BatchNorm2d defaults (vanilla_vae.py:30)


@dataclass(frozen=True)
class ConvSpec:
    kind: int          # CONV / CONVT
    ci: int
    co: int
    k: int
    stride: int = 1
    pad: int = 0
    out_pad: int = 0
    act: int = ACT_NONE

    def out_hw(self, h, w):
        if self.kind in (CONV, CONV_FLAT):
            return (h + 2 * self.pad - self.k) // self.stride + 1, (w + 2 * self.pad - self.k) // self.stride + 1
        return ((h - 1) * self.stride - 2 * self.pad + self.k + self.out_pad,
                (w - 1) * self.stride - 2 * self.pad + self.k + self.out_pad)

    def geom(self, B, H, W):
        """The ten integers by which every convolution entry point of the C ABI names a layer, in its order."""
        return (self.kind, B, H, W, self.ci, self.co, self.k, self.stride, self.pad, self.out_pad)


def _req_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("ctvae HIP kernels need device tensors (there is no CPU fallback on the product path)")


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def grad_target(p):
    """(tensor to write the gradient into, accumulate flag).  Allocates p.grad with p's memory layout if absent."""
    blk = getattr(p, "_grad_block", None)
    if blk is not None:
        blk.written = True                 # FlatAdam's block activity: a gradient kernel wrote the block since zero_grad
    if p.grad is None:
        p.grad = torch.empty_strided(p.shape, p.stride(), dtype=p.dtype, device=p.device)
        return p.grad, 0
    if p.grad.stride() != p.stride():
        raise RuntimeError("parameter .grad does not share the packed layout of the parameter")
    if blk is not None and blk.fresh:      # zero_grad(lazy=True) (models/packing.py): first writer of the block overwrites
        blk.fresh = False
        return p.grad, 0
    return p.grad, 1


def _grad_targets(p, q):
    """grad_target of two parameters one kernel call writes (q may be None) under ONE accumulate flag: (gp, gq, accumulate).
    Where only one of them is fresh it is materialised as zeros and both accumulate.  p is asked first: the first asker
    consumes a lazily zeroed block's flag."""
    gp, acc = grad_target(p)
    if q is None:
        return gp, None, acc
    gq, accq = grad_target(q)
    if accq != acc:
        (gp if acc == 0 else gq).zero_()
        acc = 1
    return gp, gq, acc


# ---------------------------------------------------------------------------------------------------
# low level launch helpers (no autograd)
# ---------------------------------------------------------------------------------------------------
_geom_answers = {}


def _geom_query(name, geom, *extra, tag=None):
    """What the library's query entry point ``name`` answers for one layer geometry, name(*geom, *extra), asked once.
    tag: library state the answer depends on besides its arguments."""
    key = (name, geom, extra, tag)
    v = _geom_answers.get(key)
    if v is None:
        v = _geom_answers[key] = getattr(native.load(), name)(*geom, *extra)
    return v


def wino_filter_floats(spec: ConvSpec, B, H, W, ws_numel) -> int:
    """Size of the Winograd filter hand-over buffer of this layer (0: its forward / data gradient are not both Winograd)."""
    return int(_geom_query("ctvae_conv_wino_filter_floats", spec.geom(B, H, W), ws_numel * 4, tag=native.winograd_enabled()))


def _coef_ptrs(in_coef, ci):
    """(scale, shift) pointers into a [2][Ci] (or longer) coefficient block; (None, None) without one."""
    if in_coef is None:
        return None, None
    p = in_coef.data_ptr()
    return p, p + 4 * ci


def conv_forward_raw(x, w, b, spec: ConvSpec, add=None, act=None, in_coef=None, in_act=ACT_NONE, wino_out=None, wino_ready=None):
    """in_coef [2][Ci]: read act_in(x*scale+shift) instead of x (lazy BatchNorm apply, image-side layers only).
    wino_out: buffer of wino_filter_floats() floats that receives the data gradient's Winograd filters.
    wino_ready: the forward's transformed filters, made ahead of time for the current weights (WinoFilterCache)."""
    B, H, W, _ = x.shape
    ho, wo = spec.out_hw(H, W)
    y = torch.empty((B, ho, wo, spec.co), dtype=torch.float32, device=x.device)
    ws = native.workspace(x.device)
    g = spec.geom(B, H, W)
    native.call("ctvae_conv_forward", g[0], x.data_ptr(), w.data_ptr(), native.ptr(b), native.ptr(add), y.data_ptr(),
                *g[1:], spec.act if act is None else act, *_coef_ptrs(in_coef, spec.ci), in_act,
                native.ptr(wino_out), native.ptr(wino_ready), ws.data_ptr(), ws.numel() * 4)
    return y


# ---------------------------------------------------------------------------------------------------
# Winograd filters of a whole step in one launch
# ---------------------------------------------------------------------------------------------------
_param_epoch = [0]


def bump_param_epoch():
    """Parameters may have changed by means torch does not see (the Adam kernel writes through raw pointers), or a new step
    begins (zero_grad): transformed filters made before this are not trusted any more."""
    _param_epoch[0] += 1


class _WinoFilterCache:
    """Both transformed filter sets of every 3x3 stride-1 layer that runs Winograd, refreshed by ONE launch per training step
    (ctvae_wino_filters_batch) instead of a launch per layer: the first Winograd layer of a forward pass that finds its
    entry stale (another parameter epoch -- see bump_param_epoch -- or another tensor version) refreshes EVERY registered
    entry whose weight is alive.  Used only for forward passes that will be differentiated (training); anything else keeps the
    per-layer transform.  Entries die with their weight (weak references)."""

    def __init__(self):
        self.entries = {}          # id(weight) -> dict(ref, uf, ub, epoch, version, ci, co)

    def filters(self, w, spec, n_floats):
        """(forward filters, data-gradient filters) valid for w as it is now."""
        e = self.entries.get(id(w))
        if e is None or e["ref"]() is not w or e["uf"].numel() != n_floats or e["uf"].device != w.device:
            e = self.entries[id(w)] = dict(ref=weakref.ref(w), uf=torch.empty(n_floats, dtype=torch.float32, device=w.device),
                                           ub=torch.empty(n_floats, dtype=torch.float32, device=w.device), epoch=-1, version=-1,
                                           ci=spec.ci, co=spec.co)
        if e["epoch"] != _param_epoch[0] or e["version"] != w._version:
            self.refresh(w.device)
        return e["uf"], e["ub"]

    def refresh(self, device):
        import ctypes as C
        live = []
        for k in list(self.entries):
            e = self.entries[k]
            w = e["ref"]()
            if w is None:
                del self.entries[k]
            elif w.device == device and (e["epoch"] != _param_epoch[0] or e["version"] != w._version):
                live.append((e, w))
        if not live:
            return
        n = len(live)
        native.call("ctvae_wino_filters_batch", n, (C.c_void_p * n)(*[w.data_ptr() for _, w in live]),
                    (C.c_void_p * n)(*[e["uf"].data_ptr() for e, _ in live]), (C.c_void_p * n)(*[e["ub"].data_ptr() for e, _ in live]),
                    (C.c_int * n)(*[e["ci"] for e, _ in live]), (C.c_int * n)(*[e["co"] for e, _ in live]))
        for e, w in live:
            e["epoch"], e["version"] = _param_epoch[0], w._version


wino_cache = _WinoFilterCache()
_WINO_BATCH = True     # False: one filter-transform launch per layer (tests compare the two)


def _wino_filters_for(ctx_needs_grad, w, spec, B, H, W_):
    """(ready forward filters or None, buffer for / holding the data-gradient filters or None) for a Winograd layer."""
    n = wino_filter_floats(spec, B, H, W_, native.workspace(w.device).numel()) if ctx_needs_grad else 0
    if not n:
        return None, None
    if _WINO_BATCH and spec.ci % 32 == 0 and spec.co % 32 == 0:
        uf, ub = wino_cache.filters(w, spec, n)
        return uf, ub
    return None, torch.empty(n, dtype=torch.float32, device=w.device)


def conv_dgrad_raw(dy, w, spec: ConvSpec, in_hw, add=None, mask=None, mask_act=ACT_NONE, wino_filters=None):
    B = dy.shape[0]
    H, W = in_hw
    dx = torch.empty((B, H, W, spec.ci), dtype=torch.float32, device=dy.device)
    ws = native.workspace(dy.device)
    # this data gradient owns the whole workspace (conv_backward_raw asks with half of it)
    if wino_filters is not None and wino_filter_floats(spec, B, H, W, ws.numel()) != wino_filters.numel():
        wino_filters = None        # made for another row count or Winograd setting: the data gradient picks its own kernel and filters
    g = spec.geom(B, H, W)
    native.call("ctvae_conv_dgrad", g[0], dy.data_ptr(), w.data_ptr(), native.ptr(add), native.ptr(mask), mask_act,
                dx.data_ptr(), *g[1:], native.ptr(wino_filters), ws.data_ptr(), ws.numel() * 4)
    return dx


def _stamp(t):
    """Identity of a tensor as it is now: a hand-over is honoured only for the tensor it was made for, untouched since."""
    return t.data_ptr(), t._version, tuple(t.shape)


def _same(t, stamp):
    return stamp is not None and _stamp(t) == stamp


class BNLink:
    """Hand-over between a train-mode ConvBNAct layer and the layer that consumes its output ``a``.

    The consumer's data-gradient kernel produces g_a; given the BatchNorm's y/mean/invstd/gamma/beta it also emits the
    per-tile backward sums (ctvae_conv_backward), which the BatchNorm's own backward then takes instead of running a
    separate pass over (g_a, y).  The sums are only used when the gradient tensor that arrives is exactly the one the
    dgrad wrote (same storage pointer, same version counter): if autograd summed several contributions, or anything
    modified it in place, the BatchNorm falls back to its own pass."""
    __slots__ = ("y", "mean", "invstd", "gamma", "beta", "act", "part", "rows", "coef", "g", "slices", "sole", "g_hold")

    def __init__(self, y, mean, invstd, gamma, beta, act):
        self.y, self.mean, self.invstd, self.gamma, self.beta, self.act = y, mean, invstd, gamma, beta, act
        self.sole = False       # set by model code (mark_sole_consumer): the layer's output has exactly one consumer
        self.g_hold = None      # the placeholder of publish_lazy, kept alive until take_lazy (its address is not recycled meanwhile)
        self.part = None
        self.rows = 0
        self.coef = None
        self.slices = None
        self.g = None           # _stamp of the gradient tensor the published sums / slices belong to

    def publish_lazy(self, g, slices, n, geom):
        """Small layers (ctvae_conv_backward_lazy): the consumer's data gradient ran split-K and left its n raw slices
        (channel-major, rows in that launch's own order: geom = its ConvSpec.geom) in ``slices``; ``g`` is a placeholder that
        was never written -- the BatchNorm's backward sums the slices itself (ctvae_bn_backward_fused).  Nothing else may
        consume g: take_lazy raises if another tensor arrives."""
        self.slices = (slices, n, geom)
        self.g_hold = g
        self.part, self.rows, self.coef = None, 0, None
        self.g = _stamp(g)

    def take_lazy(self, g):
        """(slices, n, geom) when the consumer left its data gradient as raw slices, else None.  One use only."""
        sl, self.slices = self.slices, None
        self.g_hold = None
        if sl is None:
            return None
        if not _same(g, self.g):
            raise RuntimeError("BNLink: the consumer left its data gradient as split-K slices for this BatchNorm's backward pass "
                               "(sole consumer of the layer's output), but a different gradient tensor arrived")
        return sl

    def publish(self, g, part, rows, coef=None):
        """coef [7][C]: the consumer's finishing launch already ran this BatchNorm's backward finalize on the sums
        (ctvae_conv_backward bn_coef_out)."""
        self.part, self.rows, self.coef = part, rows, coef
        self.g = _stamp(g)

    def take(self, g):
        """(part, rows, coef) when ``g`` is the tensor the sums were computed for, else (None, 0, None).  One use only."""
        part, rows, coef = self.part, self.rows, self.coef
        self.part, self.rows, self.coef = None, 0, None
        if part is None or not _same(g, self.g):
            return None, 0, None
        return part, rows, coef


class ActLink:
    """Hand-over between a producer whose output r = act(pre) ends in a fused activation (ConvBNActConvAct: final_layer's
    Tanh) and the consumer that claimed the link offered for r (offer_out_act_link / claim_out_act_link: the reconstruction
    loss).  The consumer's backward multiplies by act'(r) itself and says so (publish_done), so the tensor that arrives at
    the producer's backward is already the gradient w.r.t. its pre-activation and the separate activation-backward pass is
    skipped.  The producer checks that it received exactly that tensor; anything else cannot be repaired and raises."""
    __slots__ = ("act", "g", "done", "out_ref", "out_ver")

    def __init__(self, act):
        self.act = act
        self.done = False
        self.g = None           # _stamp of the gradient tensor that carries the activation derivative
        self.out_ref = self.out_ver = None

    def publish_done(self, g):
        self.done = True
        self.g = _stamp(g)

    def take(self, g):
        """True when ``g`` already carries the activation derivative.  One use only."""
        done, self.done = self.done, False
        if not done:
            return False
        if not _same(g, self.g):
            raise RuntimeError("ActLink: the activation backward was folded into the consumer's backward pass (it claimed "
                               "the link), but a different gradient tensor arrived")
        return True


# Output-activation links OFFERED by a producer instead of promised by model code: the producer registers the tensor it hands
# out (final_layer's Tanh output r), and the one consumer that knows how to fold act'(r) into its own backward pass -- the
# reconstruction loss, which reads r anyway -- claims the link in its forward.  If nobody claims it, or the loss is not
# asked for that gradient, the producer runs its activation backward as usual; if the loss folded it but a different
# gradient tensor arrives (r had a second consumer), ActLink.take raises.  Keyed by address, not hung on the tensor as a tag: r
# crosses the public NCHW boundary as a permuted view between final_layer and the loss -- another tensor object, the same memory.
_out_act_links = {}


def offer_out_act_link(out, act):
    link = ActLink(act)
    link.out_ref, link.out_ver = weakref.ref(out), out._version
    if len(_out_act_links) > 8:
        for k in [k for k, l in _out_act_links.items() if l.out_ref() is None]:
            del _out_act_links[k]
    _out_act_links[out.data_ptr()] = link
    return link


def claim_out_act_link(t):
    """The link offered for exactly this tensor (same storage, shape and version, producer's tensor still alive), else None."""
    link = _out_act_links.pop(t.data_ptr(), None)
    if link is None:
        return None
    o = link.out_ref()
    if o is None or o.data_ptr() != t.data_ptr() or tuple(o.shape) != tuple(t.shape) or o._version != link.out_ver:
        return None
    return link


# Gradients handed on as raw split-K slices (pixel-major) to an element-wise consumer that sums them while it reads: the producer
# (conv_backward_raw, asked by a layer whose input tensor is tagged grad_slices_ok) offers the placeholder it returns, the consumer's
# backward (GaussianLatent, _ToNHWC, LinearToNHWC) claims it.  The tag is a promise of model code that the tensor's gradient goes to
# that consumer and nowhere else: the placeholder is never written.  A broken promise raises -- a tensor at an offered address that
# is not the untouched placeholder (claim_lazy_grad), more offers than a pass can have open (offer_lazy_grad), an offer nobody
# claimed because autograd summed the placeholder into another tensor for a second consumer (kernels.backward, after the pass).
_lazy_grads = {}


def offer_lazy_grad(g, slices, n):
    if len(_lazy_grads) >= 16:
        raise RuntimeError("offer_lazy_grad: 16 gradient placeholders are on offer unclaimed (backward passes outside kernels.backward?)")
    # the entry keeps the placeholder alive: its address is not recycled.  Size, not shape as in _stamp: it arrives as a reshape's view
    _lazy_grads[g.data_ptr()] = (slices, n, g._version, g.numel(), g)


def claim_lazy_grad(g):
    """(slices, n) if ``g`` is a placeholder on offer; None if nothing is on offer at its address (an ordinary gradient).  A tensor
    at an offered address that is not the untouched placeholder (written since, another size, not contiguous) is misuse: raises."""
    e = _lazy_grads.pop(g.data_ptr(), None)
    if e is not None and (e[2] != g._version or e[3] != g.numel() or not g.is_contiguous()):
        raise RuntimeError("claim_lazy_grad: a gradient left as split-K slices arrived as something else than its untouched placeholder")
    return e and (e[0], e[1])


class _Tag:
    """What a tensor's producer or model code hands to the ONE layer that consumes it.  Hangs on the tensor object (tag / tag_of);
    a view is another object and carries nothing unless model code says so (carry_tag)."""
    __slots__ = ("bn_link", "lazy_bn", "fwd_slices", "grad_slices_ok")

    def __init__(self):
        self.bn_link = None            # BNLink: the tensor is the output of a train-mode ConvBNAct
        self.lazy_bn = None            # (coef [2][C], act): the tensor holds the raw conv output, its consumer applies BatchNorm + act on load
        self.fwd_slices = None         # (slices, n, bias, _stamp): the tensor is an unwritten placeholder for bias + the sum of the slices
        self.grad_slices_ok = False    # model code: the tensor's gradient goes to ONE backward that can sum split-K slices (_lazy_grads)


_NO_TAG = _Tag()


def tag(t):
    """The tag of ``t``, created if absent: for writing."""
    if not hasattr(t, "_ctvae_tag"):
        t._ctvae_tag = _Tag()
    return t._ctvae_tag


def tag_of(t):
    """The tag of ``t`` for reading (a shared empty one if it has none)."""
    return getattr(t, "_ctvae_tag", _NO_TAG)


def carry_tag(src, view):
    """Model code hands ``view`` (a reshape of src) on in src's place, so src's one consumer is the view's.  Slices are stamped anew."""
    tg = tag_of(src)
    if view is not src and (tg.fwd_slices is not None or tg.grad_slices_ok):
        tag(view).grad_slices_ok = tg.grad_slices_ok
        tag(view).fwd_slices = tg.fwd_slices and tg.fwd_slices[:3] + (_stamp(view),)
    return view


def _handovers_in(x):
    """(bn_link, lazy_bn, grad_slices_ok) of a layer's input: the first two describe memory, so only a contiguous x (_c keeps it) has them."""
    tg, c = tag_of(x), x.is_contiguous()
    return tg.bn_link if c else None, tg.lazy_bn if c else None, tg.grad_slices_ok


def check_fwd_slices(t, fs):
    """fs = (slices, n, bias, stamp) handed over next to the placeholder t, or None.  Slices made for another tensor raise."""
    if fs is not None and not (t.is_contiguous() and _same(t, fs[3])):
        raise RuntimeError("forward split-K slices came with a tensor that is not the untouched placeholder they were made for")
    return fs


def grad_slices_ok(t):
    """Model code: the gradient w.r.t. ``t`` is consumed by ONE backward that can sum split-K slices (see _lazy_grads)."""
    tag(t).grad_slices_ok = True
    return t


def bn_apply_is_separate(spec, B, H, W) -> bool:
    """Does a training ConvBNAct of this geometry run its BatchNorm apply as a launch of its own (ctvae_conv_bn_act_apply_is_separate)?
    Only then is it worth handing the consumer the raw tensor: applying on load costs the consumer's tile kernels ~4 vector
    instructions per element next to their f32 MFMAs (+10-16 % per launch, measured)."""
    ws = native.workspace(torch.device("cuda", torch.cuda.current_device()))
    return bool(_geom_query("ctvae_conv_bn_act_apply_is_separate", spec.geom(B, H, W), ws.numel() * 4))


def lazy_bn_input_supported(spec, B, H, W) -> bool:
    """Can a train-mode ConvBNAct layer of this geometry read its input through the previous block's BatchNorm + activation
    (forward tile kernel and weight-gradient kernel both transform on load: ctvae_conv_input_transform_supported)?"""
    return input_transform_supported(spec, B, H, W)      # (the tile kernels form max(t, slope*t): LeakyReLU / ReLU / none)


def mark_sole_consumer(x):
    """Model code promises that x -- the output of a train-mode ConvBNAct block -- is read by exactly ONE consumer (the next
    block of a chain: blocks.Chain, or the one layer the model hands it to).  That consumer may then leave its data gradient as
    split-K slices for the BatchNorm's backward launch to sum (BNLink.publish_lazy): the gradient tensor in between is never
    written, so a second consumer would add garbage -- BNLink.take_lazy raises if anything but the placeholder arrives."""
    link = tag_of(x).bn_link
    if link is not None:
        link.sole = True
    return x


def _dy_bn_args(dy_bn):
    """The weight gradient's dy_bn_y, dy_bn_coef, dy_bn_act, gy_out arguments of dy_bn = (y, coef, act, gy_out or None)."""
    return (dy_bn[0].data_ptr(), dy_bn[1].data_ptr(), dy_bn[2], native.ptr(dy_bn[3])) if dy_bn is not None else (None, None, 0, None)


def _bn_commit_args(bn_commit):
    """bn_dgamma, bn_dbeta, bn_accumulate of bn_commit = (dgamma, dbeta, accumulate)."""
    return (bn_commit[0].data_ptr(), bn_commit[1].data_ptr(), bn_commit[2]) if bn_commit is not None else (None, None, 0)


def _bn_rider_args(bn, part, rows, coef, bn_commit):
    """The paired backward's BatchNorm rider: bn_y, bn_mean, bn_invstd, bn_gamma, bn_beta, bn_act of the BNLink ``bn`` below the
    layer, its bn_part / bn_part_rows sums table, bn_coef_out and _bn_commit_args.  bn None: no rider, nothing commits."""
    cg, cb, cacc = _bn_commit_args(bn_commit)
    if bn is None:
        return (None, None, None, None, None, 0, None, rows, None, None, None, cacc)
    return (native.ptr(bn.y), native.ptr(bn.mean), native.ptr(bn.invstd), native.ptr(bn.gamma), native.ptr(bn.beta), bn.act,
            part.data_ptr(), rows, coef.data_ptr(), cg, cb, cacc)


def conv_wgrad_raw(x, dy, w_param, b_param, spec: ConvSpec, in_coef=None, in_act=ACT_NONE, dy_bn=None, bn_commit=None,
                   recompute=None):
    """dy_bn = (y, coef[5][Co], act, gy_out): dy is g_a of the BatchNorm behind this layer; g_y is formed on load and
    written to gy_out (ctvae_conv_wgrad dy_bn_*).  gy_out None + bn_commit = (dgamma, dbeta, accumulate): the layer with no
    data gradient (encoder.0) -- g_y is never written and the kernel commits the BatchNorm's parameter gradients.
    recompute = (w2, spec2) with dy_bn: dy is the 3-channel gradient of the picture-side conv spec2 behind that BatchNorm and the
    kernel forms g_a itself (ctvae_conv_wgrad_recompute, where conv_recompute_supported)."""
    B, H, W, _ = x.shape
    ws = native.workspace(x.device)
    gw, gb, acc = _grad_targets(w_param, b_param)
    g = spec.geom(B, H, W)
    if recompute is not None:
        native.call("ctvae_conv_wgrad_recompute", g[0], x.data_ptr(), dy.data_ptr(), recompute[0].data_ptr(), gw.data_ptr(),
                    native.ptr(gb), *g[1:], acc, *_coef_ptrs(in_coef, spec.ci), in_act, *_dy_bn_args(dy_bn),
                    *_conv2_args(recompute[1]), ws.data_ptr(), ws.numel() * 4)
        return
    native.call("ctvae_conv_wgrad", g[0], x.data_ptr(), dy.data_ptr(), gw.data_ptr(), native.ptr(gb), *g[1:], acc,
                *_coef_ptrs(in_coef, spec.ci), in_act, *_dy_bn_args(dy_bn), *_bn_commit_args(bn_commit),
                ws.data_ptr(), ws.numel() * 4)


_PAIR = True     # a layer's weight and data gradients share one call (ctvae_conv_backward); tests read the plan it implies


def _conv_backward_lazy(x, dy, w_param, gw, gb, acc, spec, in_coef, in_act, pixel_major):
    """ctvae_conv_backward_lazy where the data gradient of this geometry splits K: the weight (+ bias) gradient, and the data
    gradient left as n raw slices -- channel-major for a BatchNorm's backward launch (pixel_major 0), pixel-major for an
    element-wise consumer (1).  Returns (slices, n), or None where that form does not apply and nothing was launched."""
    B, H, W, _ = x.shape
    ws = native.workspace(x.device)
    g = spec.geom(B, H, W)
    n = _geom_query("ctvae_conv_backward_lazy_slices", g, 0 if pixel_major else 1, ws.numel() * 4)
    if n <= 1:
        return None
    slices = torch.empty(n * B * H * W * spec.ci, dtype=torch.float32, device=dy.device)
    native.call("ctvae_conv_backward_lazy", g[0], x.data_ptr(), dy.data_ptr(), w_param.data_ptr(), gw.data_ptr(), native.ptr(gb),
                slices.data_ptr(), *g[1:], acc, *_coef_ptrs(in_coef, spec.ci), in_act, pixel_major, ws.data_ptr(), ws.numel() * 4)
    return slices, n


def conv_backward_raw(x, dy, w_param, b_param, spec: ConvSpec, link=None, mask=None, mask_act=ACT_NONE, wino_filters=None,
                      in_coef=None, in_act=ACT_NONE, dy_bn=None, bn_commit=None, grad_slices=False, recompute=None):
    """ctvae_conv_backward: weight (+bias) gradient into ``.grad`` and the data gradient of one layer in one call (the
    two GEMMs share a launch when both run their 64x64 tile kernels).  ``link``: BNLink of the layer that produced x --
    its BatchNorm-backward sums come out of the data gradient's epilogues and its finalize rides in this call's finishing
    launch.  in_coef / in_act / dy_bn: the weight gradient's options of conv_wgrad_raw.  bn_commit = (dgamma, dbeta,
    accumulate): the rider also commits that BatchNorm's parameter gradients (only where no apply launch follows).
    recompute = (w2, spec2), with dy_bn and without mask / Winograd filters: as in conv_wgrad_raw (ctvae_conv_backward_recompute)."""
    B, H, W, _ = x.shape
    ws = native.workspace(x.device)
    g = spec.geom(B, H, W)
    # each GEMM of the paired call owns half the workspace (conv_dgrad_raw asks with all of it)
    if wino_filters is not None and wino_filter_floats(spec, B, H, W, ws.numel() // 2) != wino_filters.numel():
        # the forward pass ran Winograd over more rows than this backward pass sees (companion rows: x and y through one launch,
        # only x differentiated), or under another Winograd setting: the data gradient picks its own kernel and filters
        wino_filters = None
    gw, gb, acc = _grad_targets(w_param, b_param)
    dx = torch.empty((B, H, W, spec.ci), dtype=torch.float32, device=dy.device)
    if (link is not None and link.sole and tuple(link.y.shape) == (B, H, W, spec.ci) and mask is None and wino_filters is None
            and dy_bn is None and bn_commit is None):
        lazy = _conv_backward_lazy(x, dy, w_param, gw, gb, acc, spec, in_coef, in_act, 0)
        if lazy is not None:
            # small layer: the data gradient stays n raw split-K slices, summed by the BatchNorm's own backward launch
            link.publish_lazy(dx, *lazy, g)
            return dx
    if grad_slices and link is None and mask is None and wino_filters is None and dy_bn is None and bn_commit is None:
        lazy = _conv_backward_lazy(x, dy, w_param, gw, gb, acc, spec, in_coef, in_act, 1)
        if lazy is not None:
            # the consumer of this gradient sums split-K slices itself (offer_lazy_grad): no finish launch, dx is a placeholder
            offer_lazy_grad(dx, *lazy)
            return dx
    part, rows = None, 0
    if link is not None and tuple(link.y.shape) == (B, H, W, spec.ci):
        rows = max(_geom_query("ctvae_conv_backward_bn_rows", g, ws.numel() * 4), 0)    # (halves the workspace itself)
        if rows > 0:
            part = torch.empty(rows * spec.ci * 2, dtype=torch.float32, device=dy.device)
    bn = link if part is not None else None
    coef = torch.empty(7 * spec.ci, dtype=torch.float32, device=dy.device) if bn is not None else None   # the finalize rides along
    rider = _bn_rider_args(bn, part, rows, coef, bn_commit)
    if recompute is not None:
        native.call("ctvae_conv_backward_recompute", g[0], x.data_ptr(), dy.data_ptr(), recompute[0].data_ptr(), w_param.data_ptr(),
                    gw.data_ptr(), native.ptr(gb), dx.data_ptr(), *g[1:], acc, *rider,
                    *_coef_ptrs(in_coef, spec.ci), in_act, *_dy_bn_args(dy_bn), *_conv2_args(recompute[1]),
                    ws.data_ptr(), ws.numel() * 4)
    else:
        native.call("ctvae_conv_backward", g[0], x.data_ptr(), dy.data_ptr(), w_param.data_ptr(), gw.data_ptr(), native.ptr(gb),
                    dx.data_ptr(), *g[1:], acc, native.ptr(mask), mask_act, native.ptr(wino_filters), *rider,
                    *_coef_ptrs(in_coef, spec.ci), in_act, *_dy_bn_args(dy_bn), ws.data_ptr(), ws.numel() * 4)
    if bn is not None:
        bn.publish(dx, part, rows, coef)
    return dx


def _conv2_args(spec2: ConvSpec):
    """kind2, Co2, k2, stride2, pad2, out_pad2: how the ..._recompute entry points name the picture-side conv behind a layer."""
    return (spec2.kind, spec2.co, spec2.k, spec2.stride, spec2.pad, spec2.out_pad)


def conv_recompute_supported(spec: ConvSpec, spec2: ConvSpec, B, H, W) -> bool:
    """ctvae_conv_recompute_supported: can this layer's weight-gradient kernel form g_a itself from the 3-channel gradient of the
    picture-side conv spec2 that reads this layer's output through a BatchNorm (the final block)?"""
    return spec2.ci == spec.co and bool(_geom_query("ctvae_conv_recompute_supported", spec.geom(B, H, W), *_conv2_args(spec2)))


def conv_backward_nodx_raw(x, dy, w_param, b_param, spec: ConvSpec, link, in_coef, in_act, bn_commit):
    """ctvae_conv_backward_nodx: conv_backward_raw of the picture-side conv behind the BatchNorm ``link`` (x is its raw y, read
    through in_coef) without the data gradient tensor.  Returns the finalized [7][Ci] coefficient block of that BatchNorm, or None
    where this form does not apply and nothing was launched (the data gradient's pass could not emit the sums)."""
    B, H, W, _ = x.shape
    ws = native.workspace(x.device)
    g = spec.geom(B, H, W)
    rows = max(_geom_query("ctvae_conv_backward_bn_rows", g, ws.numel() * 4), 0)
    if rows <= 0 or tuple(link.y.shape) != (B, H, W, spec.ci) or in_coef is None:
        return None
    gw, gb, acc = _grad_targets(w_param, b_param)
    part = torch.empty(rows * spec.ci * 2, dtype=torch.float32, device=dy.device)
    coef = torch.empty(7 * spec.ci, dtype=torch.float32, device=dy.device)
    native.call("ctvae_conv_backward_nodx", g[0], x.data_ptr(), dy.data_ptr(), w_param.data_ptr(), gw.data_ptr(), native.ptr(gb),
                *g[1:], acc, *_bn_rider_args(link, part, rows, coef, bn_commit),
                *_coef_ptrs(in_coef, spec.ci), in_act, ws.data_ptr(), ws.numel() * 4)
    return coef


def wgrad_then_dgrad(x, g, w_param, b_param, spec, need_dgrad, link=None, wino_filters=None, in_coef=None, in_act=ACT_NONE,
                     grad_slices=False):
    """Weight gradient (accumulated straight into ``.grad``) and data gradient of one layer, on the launch stream.  Each GEMM
    launch already covers every CU, so nothing is gained by overlapping the two; what does pay is ONE launch for both GEMMs
    (ctvae_conv_backward / conv_bwd_pair_kernel)."""
    if need_dgrad:
        return conv_backward_raw(x, g, w_param, b_param, spec, link=link, wino_filters=wino_filters, in_coef=in_coef, in_act=in_act,
                                 grad_slices=grad_slices)
    conv_wgrad_raw(x, g, w_param, b_param, spec, in_coef=in_coef, in_act=in_act)
    return None


def act_backward_raw(g_out, out, act):
    if act == ACT_NONE:
        return g_out
    g_in = torch.empty_like(out)
    native.call("ctvae_act_backward", g_out.data_ptr(), out.data_ptr(), g_in.data_ptr(), out.numel(), act)
    return g_in


def permute_raw(x, B, C, P, to_nhwc):
    out = torch.empty(x.numel(), dtype=torch.float32, device=x.device)
    native.call("ctvae_permute", x.data_ptr(), out.data_ptr(), B, C, P, 1 if to_nhwc else 0)
    return out


# ---------------------------------------------------------------------------------------------------
# layout boundary
# ---------------------------------------------------------------------------------------------------
class _ToNHWC(Function):
    """Logical NCHW contiguous -> NHWC contiguous (HIP permute)."""

    @staticmethod
    def forward(ctx, x):
        B, C, H, W = x.shape
        ctx.dims = (B, C, H, W)
        return permute_raw(_c(x), B, C, H * W, True).view(B, H, W, C)

    @staticmethod
    def backward(ctx, g):
        B, C, H, W = ctx.dims
        lazy = claim_lazy_grad(g)
        if lazy is not None:
            # the gradient arrives as split-K slices of the consumer's data gradient: summed while the layout changes
            out = torch.empty((B, C, H, W), dtype=torch.float32, device=g.device)
            native.call("ctvae_splitk_permute", lazy[0].data_ptr(), lazy[1], out.data_ptr(), B, C, H * W)
            return out
        return permute_raw(_c(g), B, C, H * W, False).view(B, C, H, W)


class LinearToNHWC(Function):
    """``decoder_input(z).view(-1, C, h, w)`` (vanilla_vae.py:101-102) handed to the decoder as the NHWC tensor [B, h, w, C] by ONE
    launch: the Linear's GEMM stores output feature c*P + p at column p*C + c (ctvae_linear_pixmajor_forward) instead of a layout
    launch behind it.  Backward is what ConvAct + _ToNHWC did: the gradient goes back to the Linear's own feature order (summing
    the consumer's split-K slices on the way when it arrives as slices), then the Linear's paired backward launch."""

    @staticmethod
    def supported(B, ci, C, P, device):
        return bool(_geom_query("ctvae_linear_pixmajor_supported", (B, ci, C, P), native.workspace(device).numel() * 4))

    @staticmethod
    def forward(ctx, x, w, b, spec, C, h, wd):
        _req_cuda(x, w)
        x = _c(x)
        B = x.shape[0]
        ctx.link_in, _, ctx.x_slices_ok = _handovers_in(x)
        ctx.spec, ctx.w, ctx.b, ctx.dims = spec, w, b, (B, C, h, wd)
        ws = native.workspace(x.device)
        y = torch.empty((B, h, wd, C), dtype=torch.float32, device=x.device)
        native.call("ctvae_linear_pixmajor_forward", x.data_ptr(), w.data_ptr(), native.ptr(b), y.data_ptr(), B, spec.ci, C, h * wd,
                    spec.act, ws.data_ptr(), ws.numel() * 4)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * 7
        (x,) = ctx.saved_tensors
        B, C, h, wd = ctx.dims
        spec = ctx.spec
        if spec.act != ACT_NONE:
            raise RuntimeError("LinearToNHWC: a fused activation is not differentiated here (decoder_input has none)")
        lazy = claim_lazy_grad(g)
        if lazy is not None:       # split-K slices of the consumer's data gradient: summed while the layout changes
            g_flat = torch.empty((B, 1, 1, C * h * wd), dtype=torch.float32, device=g.device)
            native.call("ctvae_splitk_permute", lazy[0].data_ptr(), lazy[1], g_flat.data_ptr(), B, C, h * wd)
        else:
            g_flat = permute_raw(_c(g), B, C, h * wd, False).view(B, 1, 1, C * h * wd)
        g_x = wgrad_then_dgrad(x, g_flat, ctx.w, ctx.b, spec, ctx.needs_input_grad[0], ctx.link_in, None, grad_slices=ctx.x_slices_ok)
        return g_x, None, None, None, None, None, None


class _ToNCHW(Function):
    """NHWC contiguous -> NCHW contiguous."""

    @staticmethod
    def forward(ctx, x):
        B, H, W, C = x.shape
        ctx.dims = (B, C, H, W)
        return permute_raw(_c(x), B, C, H * W, False).view(B, C, H, W)

    @staticmethod
    def backward(ctx, g):
        B, C, H, W = ctx.dims
        return permute_raw(_c(g), B, C, H * W, True).view(B, H, W, C)


def to_nhwc(x_nchw):
    """Accept a logical [B,C,H,W] tensor, return the NHWC-contiguous [B,H,W,C] tensor (zero-copy for channels_last)."""
    _req_cuda(x_nchw)
    if x_nchw.dtype != torch.float32:
        raise RuntimeError("ctvae kernels are fp32 (parity target 1e-4, SURVEY.md §7)")
    v = x_nchw.permute(0, 2, 3, 1)
    if v.is_contiguous():
        return v
    if x_nchw.is_contiguous():
        return _ToNHWC.apply(x_nchw)
    return v.contiguous()


def to_nchw_view(x_nhwc):
    return x_nhwc.permute(0, 3, 1, 2)


def staging_like(batch):
    """Static input buffer for hipGraph replay of steps on batches like ``batch``: an image batch ([B,C,H,W] fp32 on the
    device) gets channels_last memory -- the layout the encoder reads -- so that the per-step hand-over ``stage_batch`` IS the
    NCHW -> NHWC conversion instead of a copy followed by one."""
    if batch.is_cuda and batch.dim() == 4 and batch.dtype == torch.float32:
        return torch.empty_like(batch, memory_format=torch.channels_last)
    return torch.empty_like(batch)


def stage_batch(dst, src):
    """dst <- src for a buffer from ``staging_like``: one ctvae_permute launch for an NCHW-contiguous source and a
    channels_last buffer (what a DataLoader hands over / what the step reads), a plain copy otherwise."""
    if (src.is_cuda and src.dim() == 4 and src.dtype == torch.float32 and src.shape == dst.shape and src.is_contiguous()
            and dst.permute(0, 2, 3, 1).is_contiguous() and not dst.is_contiguous()):
        B, C, H, W = src.shape
        native.call("ctvae_permute", src.data_ptr(), dst.data_ptr(), B, C, H * W, 1)
        torch.autograd.graph.increment_version(dst)     # written through a raw pointer: caches keyed on (tensor, version) must see it
    else:
        dst.copy_(src, non_blocking=True)
    return dst


# ---------------------------------------------------------------------------------------------------
# Companion rows: a second batch that rides through the same launches without taking part in autograd
# ---------------------------------------------------------------------------------------------------
# CT-MCQ-VAE encodes two images per sample (ct_mcq_vae.py:536-539, 565-566): x, whose encoder pass is trained, and y, of which
# only the code indices are used (no backward).  The encoder has no BatchNorm, so its layers treat rows independently: the
# layer Functions below take y as ``aux`` and, when aux directly follows x in memory, run ONE launch over both (twice the
# rows per launch instead of twice the launches: Winograd / tile kernels at 128 images leave half the chip idle).  Only x is
# an autograd input; the aux output is marked non-differentiable and the saved tensors are the x rows.
def adjacent_rows(x, aux):
    """The [Bx+Ba, ...] tensor that x and aux form when aux starts where x ends in the same allocation, else None."""
    if (aux is None or not x.is_contiguous() or not aux.is_contiguous() or x.shape[1:] != aux.shape[1:] or x.dtype != aux.dtype
            or x.untyped_storage().data_ptr() != aux.untyped_storage().data_ptr()
            or x.data_ptr() + x.numel() * x.element_size() != aux.data_ptr()):
        return None
    return torch.as_strided(x.detach(), (x.shape[0] + aux.shape[0],) + tuple(x.shape[1:]), x.stride(), x.storage_offset())


def to_nhwc_pair(x_nchw, y_nchw):
    """NHWC tensors of two same-shaped logical [B,C,H,W] batches in ONE buffer (x rows first), one launch each."""
    _req_cuda(x_nchw, y_nchw)
    if x_nchw.shape != y_nchw.shape or x_nchw.dtype != torch.float32 or y_nchw.dtype != torch.float32 or x_nchw.requires_grad:
        return to_nhwc(x_nchw), to_nhwc(y_nchw)
    B, C, H, W = x_nchw.shape
    buf = torch.empty((2 * B, H, W, C), dtype=torch.float32, device=x_nchw.device)
    for half, src in ((buf[:B], x_nchw), (buf[B:], y_nchw)):
        if src.is_contiguous():
            native.call("ctvae_permute", src.data_ptr(), half.data_ptr(), B, C, H * W, 1)
        else:
            half.copy_(src.permute(0, 2, 3, 1))
    return buf[:B], buf[B:]


def _with_aux(x, aux, fn):
    """fn(rows) for x and aux: one call on the combined rows when they are adjacent, else one call each."""
    both = adjacent_rows(x, aux)
    if both is not None:
        out = fn(both)
        outs = out if isinstance(out, tuple) else (out,)
        B = x.shape[0]
        return tuple(o[:B] for o in outs), tuple(o[B:] for o in outs)
    ox, oa = fn(x), fn(aux)
    return (ox if isinstance(ox, tuple) else (ox,)), (oa if isinstance(oa, tuple) else (oa,))


# ---------------------------------------------------------------------------------------------------
# conv / linear (+ bias + residual + activation)
# ---------------------------------------------------------------------------------------------------
_flat_specs = {}


def flatten_linear(h, w, b, out_features, lazy_slices=False):
    """nn.Linear(C*k*k, out_features) applied to torch.flatten(h_nchw, start_dim=1), for the NHWC tensor h [B,k,k,C] -> [B, out]
    (vanilla_vae.py:87-91 and every model built on that encoder).  k = 2 with 32-aligned widths: a 2x2 stride-2 convolution
    straight on the NHWC tensor over the Linear layer's own [in][out] block (CONV_FLAT) -- no layout copies, and the data
    gradient comes back NHWC with the BatchNorm-backward sums of the layer below in its epilogue.  Anything else: the NCHW copy
    and a 1x1 GEMM.  lazy_slices: returns (out, fwd_slices) for GaussianLatent only, which sums the GEMM's split-K slices itself."""
    B, k, k2, C = h.shape
    key = (k, k2, C, out_features)
    spec = _flat_specs.get(key)
    if spec is None:
        if k == 2 and k2 == 2 and C % 32 == 0 and out_features % 32 == 0:
            spec = ConvSpec(CONV_FLAT, C, out_features, 2, 2, 0)
        else:
            spec = ConvSpec(CONV, C * k * k2, out_features, 1)
        _flat_specs[key] = spec
    if spec.kind == CONV_FLAT:
        y = ConvAct.apply(h, w, b, None, spec, None, lazy_slices)
        out = carry_tag(y, y.view(B, -1))
    else:
        out = ConvAct.apply(_ToNCHW.apply(h).view(B, 1, 1, -1), w, b, None, spec).view(B, -1)
    return (out, tag_of(out).fwd_slices) if lazy_slices else out


class ConvAct(Function):
    """y = act(conv(x, w) + b + add).  Conv2d/ConvTranspose2d/Linear forward, dgrad and wgrad on HIP."""

    @staticmethod
    def forward(ctx, x, w, b, add, spec, aux=None, lazy_slices=False):
        """aux: companion rows (see above); returns (y, y_aux) then.  lazy_slices (model code: the ONE consumer of y sums split-K
        slices itself, e.g. GaussianLatent): where the launch splits K, y is an unwritten placeholder and the raw slices (no bias)
        hang on its tag (fwd_slices) for the caller of .apply to pass on."""
        _req_cuda(x, w)
        ctx.link_in, _, ctx.x_slices_ok = _handovers_in(x)
        ctx.wino_u = None
        ctx.spec, ctx.w, ctx.b, ctx.has_add = spec, w, b, add is not None
        if lazy_slices and aux is None and add is None and spec.act == ACT_NONE and x.is_contiguous():
            B, H, W_, _ = x.shape
            ws = native.workspace(x.device)
            g = spec.geom(B, H, W_)
            n = _geom_query("ctvae_conv_forward_lazy_slices", g, ws.numel() * 4)
            if n > 1:
                ho, wo = spec.out_hw(H, W_)
                y = torch.empty((B, ho, wo, spec.co), dtype=torch.float32, device=x.device)
                slices = torch.empty(n * y.numel(), dtype=torch.float32, device=x.device)
                native.call("ctvae_conv_forward_lazy", g[0], x.data_ptr(), w.data_ptr(), slices.data_ptr(), *g[1:],
                            ws.data_ptr(), ws.numel() * 4)
                ctx.save_for_backward(x, None)
                tag(y).fwd_slices = (slices, n, b, _stamp(y))
                return y
        x = _c(x)
        add_c = _c(add) if add is not None else None
        if aux is not None:
            if add is not None:
                raise RuntimeError("ConvAct: companion rows and a residual operand together are not supported")
            rows = adjacent_rows(x, _c(aux))
            Bt = rows.shape[0] if rows is not None else x.shape[0]
            ready, ctx.wino_u = _wino_filters_for(ctx.needs_input_grad[0], w, spec, Bt, x.shape[1], x.shape[2])
            first = [True]

            def run(t):
                wo, first[0] = (ctx.wino_u if (first[0] and ready is None) else None), False
                return conv_forward_raw(t, w, b, spec, None, wino_out=wo, wino_ready=ready)
            (y,), (y_aux,) = _with_aux(x, _c(aux), run)
            ctx.save_for_backward(x, y if spec.act != ACT_NONE else None)
            ctx.mark_non_differentiable(y_aux)
            ctx.set_materialize_grads(False)        # else backward is handed a zero-filled tensor for y_aux: a fill per layer
            return y, y_aux
        ready = None
        if add is None:
            ready, ctx.wino_u = _wino_filters_for(ctx.needs_input_grad[0], w, spec, x.shape[0], x.shape[1], x.shape[2])
        y = conv_forward_raw(x, w, b, spec, add_c, wino_out=None if ready is not None else ctx.wino_u, wino_ready=ready)
        ctx.save_for_backward(x, y if spec.act != ACT_NONE else None)
        return y

    @staticmethod
    def backward(ctx, g_y, *_g_aux):
        if g_y is None:
            return (None,) * 7
        spec = ctx.spec
        x, y = ctx.saved_tensors
        g_y = _c(g_y)
        g_pre = g_y if spec.act == ACT_NONE else act_backward_raw(g_y, y, spec.act)
        g_x = wgrad_then_dgrad(x, g_pre, ctx.w, ctx.b, spec, ctx.needs_input_grad[0], ctx.link_in, ctx.wino_u,
                               grad_slices=ctx.x_slices_ok)
        g_add = g_pre if (ctx.has_add and ctx.needs_input_grad[3]) else None
        return g_x, None, None, g_add, None, None, None


class ResBlock(Function):
    """out = post_act(x + Conv1x1(ReLU(Conv3x3(x)))), both convs bias-free: ResidualLayer (vq_vae.py:57-70) as ONE autograd
    node.  As two ConvAct nodes the input x has two consumers (the 3x3 conv and the skip), and autograd adds their
    gradients with a launch of its own per block; here the skip gradient enters the 3x3 conv's data gradient as the
    ``add`` operand of its epilogue (direct and Winograd kernels alike), and the ReLU derivative is the ``mask`` operand of
    the 1x1 conv's data gradient."""

    @staticmethod
    def forward(ctx, x, w3, w1, spec3, spec1, aux=None):
        """aux: companion rows (see adjacent_rows); returns (out, out_aux) then."""
        _req_cuda(x, w3, w1)
        x = _c(x)
        ctx.wino_u = None
        ctx.specs = (spec3, spec1)
        ctx.w = (w3, w1)
        rows = adjacent_rows(x, _c(aux)) if aux is not None else None
        Bt = rows.shape[0] if rows is not None else x.shape[0]
        ready, ctx.wino_u = _wino_filters_for(ctx.needs_input_grad[0], w3, spec3, Bt, x.shape[1], x.shape[2])
        if aux is not None:
            first = [True]

            def run(t):
                wo, first[0] = (ctx.wino_u if (first[0] and ready is None) else None), False
                h_ = conv_forward_raw(t, w3, None, spec3, wino_out=wo, wino_ready=ready)
                return h_, conv_forward_raw(h_, w1, None, spec1, t)
            (h, out), (_h_aux, out_aux) = _with_aux(x, _c(aux), run)
            ctx.save_for_backward(x, h, out if spec1.act != ACT_NONE else None)
            ctx.mark_non_differentiable(out_aux)
            ctx.set_materialize_grads(False)
            return out, out_aux
        h = conv_forward_raw(x, w3, None, spec3, wino_out=None if ready is not None else ctx.wino_u, wino_ready=ready)
        out = conv_forward_raw(h, w1, None, spec1, x)
        ctx.save_for_backward(x, h, out if spec1.act != ACT_NONE else None)
        return out

    @staticmethod
    def backward(ctx, g_out, *_g_aux):
        if g_out is None:
            return (None,) * 6
        spec3, spec1 = ctx.specs
        w3, w1 = ctx.w
        x, h, out = ctx.saved_tensors
        g_out = _c(g_out)
        g_pre = act_backward_raw(g_out, out, spec1.act) if spec1.act != ACT_NONE else g_out
        g_h = conv_backward_raw(h, g_pre, w1, None, spec1, mask=h, mask_act=spec3.act)
        conv_wgrad_raw(x, g_h, w3, None, spec3)
        g_x = None
        if ctx.needs_input_grad[0]:
            g_x = conv_dgrad_raw(g_h, w3, spec3, (x.shape[1], x.shape[2]), add=g_pre, wino_filters=ctx.wino_u)
        return g_x, None, None, None, None, None


def _conv_bn_act_forward(x, params, running, training, spec, bn_act, lazy_in, want_a, want_coef):
    """ctvae_conv_bn_act_forward: y = conv(x, w) + b and the BatchNorm2d (+ activation) behind it.  params = (w, b, gamma,
    beta); running = (running_mean, running_var, num_batches_tracked); lazy_in = (coef, act) of an input that is read through
    the previous block's BatchNorm, or None.  want_a: the activated tensor is written; want_coef: the [2][C] scale | shift
    block is, for a consumer that applies it on load.  Returns y, a, coef, save_mean, save_invstd."""
    w, b, gamma, beta = params
    running_mean, running_var, num_batches_tracked = running
    B, H, W, _ = x.shape
    ho, wo = spec.out_hw(H, W)
    C = spec.co
    y = torch.empty((B, ho, wo, C), dtype=torch.float32, device=x.device)
    a = torch.empty_like(y) if want_a else None
    coef = torch.empty(2 * C, dtype=torch.float32, device=x.device) if want_coef else None
    save_mean = torch.empty(C, dtype=torch.float32, device=x.device)
    save_invstd = torch.empty(C, dtype=torch.float32, device=x.device)
    ws = native.workspace(x.device)
    in_coef, in_act = lazy_in if lazy_in is not None else (None, ACT_NONE)
    g = spec.geom(B, H, W)
    native.call("ctvae_conv_bn_act_forward", g[0], x.data_ptr(), w.data_ptr(), native.ptr(b), gamma.data_ptr(),
                beta.data_ptr(), native.ptr(running_mean), native.ptr(running_var), BN_MOMENTUM, BN_EPS,
                1 if training else 0, bn_act, y.data_ptr(), native.ptr(a), save_mean.data_ptr(), save_invstd.data_ptr(),
                native.ptr(coef), native.ptr(num_batches_tracked) if training else None, *g[1:],
                *_coef_ptrs(in_coef, spec.ci), in_act, ws.data_ptr(), ws.numel() * 4)
    return y, a, coef, save_mean, save_invstd


def _bn_backward(g_a, y, bn, bn_act, g_y, grads, part=None, rows=0, coef_out=None, coef_in=None):
    """ctvae_bn_backward over y [B,H,W,C].  bn = (gamma, beta, save_mean, save_invstd); grads = (dgamma, dbeta, accumulate).
    g_y None: the apply pass is left to the weight-gradient kernel, which reads coef_out.  part / rows: the sums the consumer's
    data gradient emitted; coef_in: the [7][C] block of a finalize that already ran (BNLink.take)."""
    gamma, beta, save_mean, save_invstd = bn
    gg, gbt, acc = grads
    B, H, W, C = y.shape
    ws = native.workspace(y.device)
    native.call("ctvae_bn_backward", g_a.data_ptr(), beta.data_ptr(), y.data_ptr(), B * H * W, C, gamma.data_ptr(),
                save_mean.data_ptr(), save_invstd.data_ptr(), bn_act, native.ptr(g_y), gg.data_ptr(), gbt.data_ptr(), acc,
                native.ptr(part), rows, native.ptr(coef_out), native.ptr(coef_in), ws.data_ptr(), ws.numel() * 4)


class ConvBNAct(Function):
    """a = act(BatchNorm2d(conv(x, w) + b)) with train-mode batch statistics (vanilla_vae.py:25-35,47-75)."""

    @staticmethod
    def forward(ctx, x, w, b, gamma, beta, running_mean, running_var, training, spec, bn_act, num_batches_tracked=None,
                lazy_out=False):
        """lazy_out (model code, blocks.Chain: the ONE consumer of the output applies BatchNorm + activation while it loads):
        the returned tensor holds the raw conv output y and is tagged lazy_bn = (coef [2][C], act); the stand-alone apply launch and
        the activated tensor do not exist.  An input tagged that way is read through its own coefficients.  Training tags bn_link."""
        _req_cuda(x, w, gamma)
        ctx.link_in, lazy_in, ctx.x_slices_ok = _handovers_in(x)
        x = _c(x)
        y, a, coef, save_mean, save_invstd = _conv_bn_act_forward(
            x, (w, b, gamma, beta), (running_mean, running_var, num_batches_tracked), training, spec, bn_act, lazy_in,
            want_a=not lazy_out, want_coef=lazy_out)
        ctx.spec, ctx.bn_act, ctx.training = spec, bn_act, training
        ctx.params = (w, b, gamma, beta)
        ctx.lazy_in = lazy_in
        ctx.save_for_backward(x, y, save_mean, save_invstd)
        out = y if lazy_out else a             # lazy_out: the output IS the raw conv output (also saved above for backward)
        ctx.link_out = tag(out).bn_link = BNLink(y, save_mean, save_invstd, gamma, beta, bn_act) if training else None
        tag(out).lazy_bn = (coef, bn_act) if lazy_out else None
        return out

    @staticmethod
    def backward(ctx, g_a):
        if not ctx.training:
            raise RuntimeError("backward through eval-mode BatchNorm is not supported on the HIP path")
        spec = ctx.spec
        w, b, gamma, beta = ctx.params
        x, y, save_mean, save_invstd = ctx.saved_tensors
        g_a = _c(g_a)
        in_coef, in_act = ctx.lazy_in if ctx.lazy_in is not None else (None, ACT_NONE)
        gg, gbt, accg = _grad_targets(gamma, beta)
        lazy = ctx.link_out.take_lazy(g_a) if ctx.link_out is not None else None
        if lazy is not None:
            # g_a was never materialised: the consumer's split-K slices are summed here, with the sums, the finalize and the apply
            g_y = torch.empty_like(y)
            native.call("ctvae_bn_backward_fused", lazy[0].data_ptr(), lazy[1], *lazy[2], y.data_ptr(), gamma.data_ptr(),
                        beta.data_ptr(), save_mean.data_ptr(), save_invstd.data_ptr(), ctx.bn_act, g_y.data_ptr(), gg.data_ptr(),
                        gbt.data_ptr(), accg)
        else:
            part, rows, coef = ctx.link_out.take(g_a) if ctx.link_out is not None else (None, 0, None)
            if coef is not None:
                part, rows = None, 0         # finalized by the consumer's finishing launch: apply + commit only
                if not ctx.needs_input_grad[0] and wgrad_bn_apply_mode(spec, x.shape[0], x.shape[1], x.shape[2]) == 2:
                    # the first layer of the encoder: no data gradient follows, so g_y is only the weight gradient's operand --
                    # formed on load from (g_a, y, coef); the apply launch and its 33 MB output are not needed
                    conv_wgrad_raw(x, g_a, w, b, spec, dy_bn=(y, coef, ctx.bn_act, None), bn_commit=(gg, gbt, accg))
                    return (None,) * 12
            g_y = torch.empty_like(y)
            _bn_backward(g_a, y, (gamma, beta, save_mean, save_invstd), ctx.bn_act, g_y, (gg, gbt, accg), part, rows, coef_in=coef)
        g_x = wgrad_then_dgrad(x, g_y, w, b, spec, ctx.needs_input_grad[0], ctx.link_in, in_coef=in_coef, in_act=in_act,
                               grad_slices=ctx.x_slices_ok)
        return (g_x,) + (None,) * 11


def input_transform_supported(spec: ConvSpec, B, H, W) -> bool:
    """Can this layer apply the previous block's BatchNorm + activation while loading (ctvae_conv_forward in_scale)?"""
    return bool(_geom_query("ctvae_conv_input_transform_supported", spec.geom(B, H, W)))


def wgrad_bn_apply_mode(spec: ConvSpec, B, H, W) -> int:
    """ctvae_conv_wgrad_bn_apply_supported: 0 no; 1 the weight-gradient kernel applies the BatchNorm backward on load and writes
    g_y for the data gradient (final_layer.0); 2 it applies it on load and nothing is written (encoder.0: no data gradient)."""
    return int(_geom_query("ctvae_conv_wgrad_bn_apply_supported", spec.geom(B, H, W)))


def wgrad_bn_apply_supported(spec: ConvSpec, B, H, W) -> bool:
    """Can this layer's weight-gradient kernel apply the BatchNorm backward on load and hand g_y on (ctvae_conv_wgrad dy_bn_*)?"""
    return wgrad_bn_apply_mode(spec, B, H, W) == 1


class ConvBNActConvAct(Function):
    """r = act2(conv2(act(BN(conv1(x))))) for an image-side conv2 (3 output channels): the reference's final_layer
    nn.Sequential(ConvTranspose2d, BatchNorm2d, LeakyReLU, Conv2d, Tanh) (vanilla_vae.py:64-75) as ONE autograd node.

    The BatchNorm output is never written: conv1 leaves y and the per-channel affine, conv2's forward and weight
    gradient apply affine + LeakyReLU while staging their input tiles, conv2's data gradient emits the BatchNorm's
    backward sums.  On the 64x64x32 activations of this block that removes two full passes over 134 MB per step.
    Backward, where conv_recompute_supported: conv2's data gradient g_a is not written either -- conv1's weight-gradient kernel
    forms it again per tile from the 3-channel gradient (ctvae_conv_backward_nodx, ctvae_conv_backward_recompute)."""

    @staticmethod
    def forward(ctx, x, w1, b1, gamma, beta, running_mean, running_var, num_batches_tracked, w2, b2, training, spec1, spec2, bn_act):
        _req_cuda(x, w1, w2, gamma)
        ctx.link_in, ctx.lazy_in, _ = _handovers_in(x)
        x = _c(x)
        y1, _, coef, save_mean, save_invstd = _conv_bn_act_forward(
            x, (w1, b1, gamma, beta), (running_mean, running_var, num_batches_tracked), training, spec1, bn_act, ctx.lazy_in,
            want_a=False, want_coef=True)
        r = conv_forward_raw(y1, w2, b2, spec2, in_coef=coef, in_act=bn_act)
        ctx.act_out = offer_out_act_link(r, spec2.act) if (training and spec2.act != ACT_NONE) else None
        ctx.specs, ctx.bn_act, ctx.training = (spec1, spec2), bn_act, training
        ctx.params = (w1, b1, gamma, beta, w2, b2)
        ctx.save_for_backward(x, y1, r, coef, save_mean, save_invstd)
        return r

    @staticmethod
    def backward(ctx, g_r):
        if not ctx.training:
            raise RuntimeError("backward through eval-mode BatchNorm is not supported on the HIP path")
        spec1, spec2 = ctx.specs
        w1, b1, gamma, beta, w2, b2 = ctx.params
        x, y1, r, coef, save_mean, save_invstd = ctx.saved_tensors
        g_r = _c(g_r)
        if ctx.act_out is not None and ctx.act_out.take(g_r):
            g_pre = g_r                                          # the loss's backward pass already applied act'(r)
        else:
            g_pre = act_backward_raw(g_r, r, spec2.act) if spec2.act != ACT_NONE else g_r
        C = y1.shape[3]
        bn = (gamma, beta, save_mean, save_invstd)
        link = BNLink(y1, save_mean, save_invstd, gamma, beta, ctx.bn_act)
        grads = _grad_targets(gamma, beta)
        lazy = wgrad_bn_apply_supported(spec1, x.shape[0], x.shape[1], x.shape[2])
        g_y = torch.empty_like(y1)
        in_coef, in_act = ctx.lazy_in if ctx.lazy_in is not None else (None, ACT_NONE)
        if lazy and conv_recompute_supported(spec1, spec2, x.shape[0], x.shape[1], x.shape[2]):
            # g_a [B,2H,2W,32] is never allocated: conv2's backward runs without its data gradient's stores, and conv1's
            # weight-gradient kernel forms g_a again, tile by tile, from the 3-channel g_pre (same values, bit for bit)
            c7 = conv_backward_nodx_raw(y1, g_pre, w2, b2, spec2, link, coef, ctx.bn_act, grads)
            if c7 is not None:
                dy_bn, rc = (y1, c7, ctx.bn_act, g_y), (w2, spec2)
                if ctx.needs_input_grad[0]:
                    g_x = conv_backward_raw(x, g_pre, w1, b1, spec1, link=ctx.link_in, dy_bn=dy_bn, in_coef=in_coef, in_act=in_act,
                                            recompute=rc)
                else:
                    conv_wgrad_raw(x, g_pre, w1, b1, spec1, dy_bn=dy_bn, in_coef=in_coef, in_act=in_act, recompute=rc)
                    g_x = None
                return (g_x,) + (None,) * 13
        # conv2's weight gradient, its data gradient (which emits the BatchNorm's backward sums) and the BatchNorm's
        # finalize in one call: the finalize rides in the slab-reduction launch (the link is local to this node, so the
        # rider commits d gamma / d beta itself when no apply launch follows)
        g_a = conv_backward_raw(y1, g_pre, w2, b2, spec2, link=link, in_coef=coef, in_act=ctx.bn_act,
                                bn_commit=grads if lazy else None)
        part, rows, c7 = link.take(g_a)
        if c7 is None:
            # the rider declined (no sums from the data gradient): the BatchNorm's own launch finalizes
            bcoef = torch.empty(5 * C, dtype=torch.float32, device=x.device) if lazy else None
            _bn_backward(g_a, y1, bn, ctx.bn_act, None if lazy else g_y, grads, part, rows, coef_out=bcoef)
        elif lazy:
            bcoef = c7                                           # rows 0-4 are the coefficients the weight-gradient kernel reads
        else:
            _bn_backward(g_a, y1, bn, ctx.bn_act, g_y, grads, coef_in=c7)
        if lazy:
            # the weight-gradient kernel turns g_a into g_y on load and leaves g_y behind for the data gradient
            if ctx.needs_input_grad[0]:
                g_x = conv_backward_raw(x, g_a, w1, b1, spec1, link=ctx.link_in, dy_bn=(y1, bcoef, ctx.bn_act, g_y),
                                        in_coef=in_coef, in_act=in_act)
            else:
                conv_wgrad_raw(x, g_a, w1, b1, spec1, dy_bn=(y1, bcoef, ctx.bn_act, g_y), in_coef=in_coef, in_act=in_act)
                g_x = None
        else:
            g_x = wgrad_then_dgrad(x, g_y, w1, b1, spec1, ctx.needs_input_grad[0], ctx.link_in, in_coef=in_coef, in_act=in_act)
        return (g_x,) + (None,) * 13


class ActFn(Function):
    """Standalone activation (nn.LeakyReLU sites mcq_vae.py:185,216)."""

    @staticmethod
    def forward(ctx, x, act, aux=None):
        _req_cuda(x)
        x = _c(x)
        ctx.act = act

        def run(t):
            o = torch.empty_like(t)
            native.call("ctvae_act_forward", t.data_ptr(), o.data_ptr(), t.numel(), act)
            return o
        if aux is not None:
            (out,), (out_aux,) = _with_aux(x, _c(aux), run)
            ctx.save_for_backward(out)
            ctx.mark_non_differentiable(out_aux)
            ctx.set_materialize_grads(False)
            return out, out_aux
        out = run(x)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, g, *_g_aux):
        if g is None:
            return None, None, None
        (out,) = ctx.saved_tensors
        return act_backward_raw(_c(g), out, ctx.act), None, None


# ---------------------------------------------------------------------------------------------------
# Gaussian reparameterisation and losses
# ---------------------------------------------------------------------------------------------------
def _rows(t):
    """(tensor, row stride) for a 2-D tensor whose rows are contiguous (column slices of a wider matrix allowed)."""
    if t.dim() != 2 or t.stride(1) != 1:
        t = t.contiguous()
    return t, t.stride(0)


class SplitHeads(Function):
    """[B,2L] fused fc_mu|fc_var output -> (mu, log_var) views; backward gathers both gradients with one
    kernel instead of two zero-fills, two strided copies and an add."""

    @staticmethod
    def forward(ctx, heads, L):
        ctx.L = L
        return heads[:, :L], heads[:, L:]

    @staticmethod
    def backward(ctx, g_mu, g_lv):
        if g_mu is None:
            g_mu = torch.zeros_like(g_lv)
        if g_lv is None:
            g_lv = torch.zeros_like(g_mu)
        return torch.cat([g_mu, g_lv], dim=1), None


class Reparameterize(Function):
    """z = eps * exp(0.5*logvar) + mu (vanilla_vae.py:107-117), noise injectable."""

    @staticmethod
    def forward(ctx, mu, logvar, eps):
        _req_cuda(mu, logvar, eps)
        mu_, mrs = _rows(mu)
        lv_, lrs = _rows(logvar)
        eps = _c(eps)
        B, L = mu.shape
        z = torch.empty((B, L), dtype=torch.float32, device=mu.device)
        native.call("ctvae_reparam_forward", mu_.data_ptr(), mrs, lv_.data_ptr(), lrs, eps.data_ptr(), z.data_ptr(), B, L)
        ctx.save_for_backward(lv_, eps)
        ctx.lrs = lrs
        return z

    @staticmethod
    def backward(ctx, g_z):
        lv_, eps = ctx.saved_tensors
        g_z = _c(g_z)
        B, L = g_z.shape
        g_mu = torch.empty_like(g_z)
        g_lv = torch.empty_like(g_z)
        native.call("ctvae_reparam_backward", g_z.data_ptr(), lv_.data_ptr(), ctx.lrs, eps.data_ptr(), g_mu.data_ptr(),
                    g_lv.data_ptr(), B, L)
        return g_mu, g_lv, None


class GaussianLatent(Function):
    """(mu, log_var, z) from the fused fc_mu | fc_var output heads [B,2L] as ONE autograd node (vanilla_vae.py:85-92,107-122):
    mu / log_var are views of heads, z = eps*exp(0.5*log_var) + mu.  eps None: N(0,1) drawn in the kernel from ``rng`` (a device
    uint64 pair: Philox key and stream position, advanced by the backward launch).  Backward forms g_heads in one launch;
    as separate SplitHeads / Reparameterize nodes autograd adds the KL and the reparameterisation contributions to mu and
    log_var with a launch each and concatenates with a third."""

    @staticmethod
    def forward(ctx, heads, eps, rng, fwd_slices=None):
        _req_cuda(heads)
        fs = check_fwd_slices(heads, fwd_slices)    # what flatten_linear(lazy_slices=True) returned next to heads: heads not written yet
        heads = _c(heads)
        B, L2 = heads.shape
        L = L2 // 2
        eps_in = _c(eps) if eps is not None else None
        if eps_in is None and rng is None:
            raise RuntimeError("GaussianLatent: either eps or the rng state is needed")
        eps_out = torch.empty((B, L), dtype=torch.float32, device=heads.device)
        z = torch.empty((B, L), dtype=torch.float32, device=heads.device)
        native.call("ctvae_gauss_latent_forward", heads.data_ptr(), native.ptr(eps_in), native.ptr(rng) if eps_in is None else None,
                    eps_out.data_ptr(), z.data_ptr(), B, L, fs[0].data_ptr() if fs else None, fs[1] if fs else 0,
                    native.ptr(fs[2]) if fs else None)
        ctx.save_for_backward(heads, eps_out)
        ctx.rng = rng if eps_in is None else None
        ctx.set_materialize_grads(False)
        return heads[:, :L], heads[:, L:], z

    @staticmethod
    def backward(ctx, g_mu, g_lv, g_z):
        heads, eps = ctx.saved_tensors
        B, L2 = heads.shape
        g_mu = _c(g_mu) if g_mu is not None else None
        g_lv = _c(g_lv) if g_lv is not None else None
        lazy = claim_lazy_grad(g_z) if g_z is not None else None
        g_z = _c(g_z) if g_z is not None else None
        g_heads = torch.empty_like(heads)
        native.call("ctvae_gauss_latent_backward", native.ptr(g_mu), native.ptr(g_lv), lazy[0].data_ptr() if lazy else native.ptr(g_z),
                    heads.data_ptr(), eps.data_ptr(), g_heads.data_ptr(), native.ptr(ctx.rng), B, L2 // 2, lazy[1] if lazy else 0)
        return g_heads, None, None, None


def _scalar_outputs(ctx, out):
    """The 4-vector a loss kernel wrote, handed out as four 0-dim views.  Callers index the returned tuple, so no autograd
    select node sits between the loss and this Function: indexing a tensor output (out[0]) made ``loss.backward()`` build
    zeros[4] and copy the root gradient into it -- two launches per step for nothing.  Only the first carries gradient."""
    o = out.unbind(0)
    ctx.mark_non_differentiable(*o[1:])
    ctx.set_materialize_grads(False)
    return o


class VAELoss(Function):
    """out = [loss, mse, kld, -kld]: mse = F.mse_loss(recons, x); kld as vanilla_vae.py:143; loss = mse + M_N*kld (+ extra).
    recons/x are same-layout contiguous tensors.  Only out[0] carries gradient."""

    @staticmethod
    def forward(ctx, recons, x, mu, logvar, extra, M_N, logcosh_alpha=0.0):
        """logcosh_alpha > 0: the reconstruction term is LogCoshVAE's (logcosh_vae.py:141-150) instead of the MSE;
        logcosh_alpha == L2L1 (-1): SWAE's F.mse_loss + F.l1_loss (swae.py:121-125), no KL term."""
        _req_cuda(recons, x)
        recons, x = _c(recons), _c(x)
        if recons.shape != x.shape:
            raise RuntimeError("mse_loss: shape mismatch")
        out = torch.empty(4, dtype=torch.float32, device=recons.device)
        ws = native.workspace(recons.device)
        pre = None
        if mu is not None:
            mu_, mrs = _rows(mu)
            lv_, lrs = _rows(logvar)
            B, L = mu.shape
        else:
            mu_, lv_, mrs, lrs, B, L = None, None, 0, 0, 0, 0
        if logcosh_alpha < 0.0:
            if mu is not None:
                raise RuntimeError("l2 + l1 reconstruction term: no KL term")
            native.call("ctvae_l2l1_loss_forward", recons.data_ptr(), x.data_ptr(), recons.numel(), native.ptr(extra), out.data_ptr(),
                        ws.data_ptr(), ws.numel() * 4)
        elif logcosh_alpha > 0.0:
            if extra is not None:
                raise RuntimeError("log-cosh loss: no extra term")
            native.call("ctvae_logcosh_loss_forward", recons.data_ptr(), x.data_ptr(), recons.numel(), float(logcosh_alpha),
                        native.ptr(mu_), mrs, native.ptr(lv_), lrs, B, L, float(M_N), out.data_ptr(), ws.data_ptr(), ws.numel() * 4)
        else:
            if mu is not None and ctx.needs_input_grad[0] and ctx.needs_input_grad[2] and ctx.needs_input_grad[3]:
                # the gradients for a unit upstream gradient come out of the same pass (ctvae_loss_forward_grad); backward hands
                # them over as they are when the loss is the root of the pass (kernels.backward), else it runs its own kernel
                ctx.act_link = claim_out_act_link(recons)
                ract = ctx.act_link.act if ctx.act_link is not None else ACT_NONE
                pre = (torch.empty_like(recons), torch.empty((B, L), dtype=torch.float32, device=recons.device),
                       torch.empty((B, L), dtype=torch.float32, device=recons.device))
                native.call("ctvae_loss_forward_grad", recons.data_ptr(), x.data_ptr(), recons.numel(), mu_.data_ptr(), mrs, lv_.data_ptr(),
                            lrs, B, L, float(M_N), native.ptr(extra), out.data_ptr(), pre[0].data_ptr(), pre[1].data_ptr(),
                            pre[2].data_ptr(), ract, ws.data_ptr(), ws.numel() * 4)
            else:
                native.call("ctvae_loss_forward", recons.data_ptr(), x.data_ptr(), recons.numel(), native.ptr(mu_), mrs, native.ptr(lv_),
                            lrs, B, L, float(M_N), native.ptr(extra), out.data_ptr(), ws.data_ptr(), ws.numel() * 4)
        ctx.pre = pre
        ctx.save_for_backward(recons, x, mu_, lv_)
        ctx.meta = (mrs, lrs, B, L, float(M_N), tuple(extra.shape) if extra is not None else None)
        ctx.logcosh_alpha = float(logcosh_alpha)
        if pre is None:
            ctx.act_link = claim_out_act_link(recons) if ctx.needs_input_grad[0] else None
        return _scalar_outputs(ctx, out)

    @staticmethod
    def backward(ctx, g_loss, *_unused):
        recons, x, mu_, lv_ = ctx.saved_tensors
        mrs, lrs, B, L, M_N, has_extra = ctx.meta
        if g_loss is None:
            return (None,) * 7
        if ctx.pre is not None and _is_cached_root(g_loss):
            # the loss is the root of this backward pass (kernels.backward): the forward pass has written these gradients
            g_r, g_mu, g_lv = ctx.pre
            if ctx.act_link is not None:
                ctx.act_link.publish_done(g_r)
            g_extra = g_loss.reshape(has_extra) if (has_extra is not None and ctx.needs_input_grad[4]) else None
            return g_r, None, g_mu, g_lv, g_extra, None, None
        g_loss = _c(g_loss.reshape(1))               # d/d loss; mse and kld outputs are reported detached
        want_r = ctx.needs_input_grad[0]
        want_kl = mu_ is not None and (ctx.needs_input_grad[2] or ctx.needs_input_grad[3])
        g_r = torch.empty_like(recons) if want_r else None
        link = ctx.act_link if want_r else None
        ract = link.act if link is not None else ACT_NONE        # recons = act(pre): hand back the gradient w.r.t. pre
        g_mu = g_lv = None
        if want_kl:
            g_mu = torch.empty((B, L), dtype=torch.float32, device=recons.device)
            g_lv = torch.empty((B, L), dtype=torch.float32, device=recons.device)
        if want_r and want_kl:      # the usual case: both gradients in one launch
            native.call("ctvae_loss_backward", recons.data_ptr(), x.data_ptr(), g_loss.data_ptr(), g_r.data_ptr(), recons.numel(),
                        ctx.logcosh_alpha, mu_.data_ptr(), mrs, lv_.data_ptr(), lrs, g_mu.data_ptr(), g_lv.data_ptr(), B, L, M_N, ract)
        else:
            if want_r:
                if ctx.logcosh_alpha < 0.0:
                    native.call("ctvae_l2l1_backward", recons.data_ptr(), x.data_ptr(), g_loss.data_ptr(), g_r.data_ptr(), recons.numel(),
                                ract)
                elif ctx.logcosh_alpha > 0.0:
                    native.call("ctvae_logcosh_backward", recons.data_ptr(), x.data_ptr(), g_loss.data_ptr(), g_r.data_ptr(),
                                recons.numel(), ctx.logcosh_alpha, ract)
                else:
                    native.call("ctvae_mse_backward", recons.data_ptr(), x.data_ptr(), g_loss.data_ptr(), g_r.data_ptr(), recons.numel(),
                                ract)
            if want_kl:
                native.call("ctvae_kl_backward", mu_.data_ptr(), mrs, lv_.data_ptr(), lrs, g_loss.data_ptr(), g_mu.data_ptr(),
                            g_lv.data_ptr(), B, L, M_N)
        if link is not None:
            link.publish_done(g_r)
        g_extra = g_loss.reshape(has_extra) if (has_extra is not None and ctx.needs_input_grad[4]) else None
        return g_r, None, g_mu, g_lv, g_extra, None, None


FREE_BITS_MAX_L = 1024                  # what ctvae_freebits_kl_forward_grad covers


class FreeBitsKL(Function):
    """out = [w * sum_d f_d, sum_d m_d, sum_d f_d, #floored]: the Gaussian KL term with free bits (Kingma et al. 2016, eq. 15) and
    a weight read from device memory (csrc/klfloor.hip).  m_d is the batch mean of dimension d's KL, f_d = m_d
    where m_d > free_bits (or is not finite), else free_bits; w = scale * w_dev[0].  ``w_dev`` is a 1-element
    fp32 device tensor whose ADDRESS the launch takes: a captured launch reads the value it holds at replay.  Only out[0] carries
    gradient, to mu and log_var; the gradients for a unit upstream gradient come out of the forward launch."""

    @staticmethod
    def forward(ctx, mu, log_var, w_dev, scale, free_bits):
        _req_cuda(mu, log_var, w_dev)
        if mu.dim() != 2 or mu.shape != log_var.shape or mu.dtype != torch.float32 or log_var.dtype != torch.float32:
            raise RuntimeError(f"free_bits_kl: mu / log_var must be fp32 [B, L] of one shape, got {tuple(mu.shape)} {mu.dtype}, "
                               f"{tuple(log_var.shape)} {log_var.dtype}")
        if w_dev.dtype != torch.float32 or w_dev.numel() != 1:
            raise RuntimeError("free_bits_kl: the weight is one fp32 element on the device")
        B, L = mu.shape
        if B < 1 or not 1 <= L <= FREE_BITS_MAX_L:
            raise RuntimeError(f"free_bits_kl: B >= 1 and 1 <= L <= {FREE_BITS_MAX_L}, got B = {B}, L = {L}")
        mu_, mrs = _rows(mu)
        lv_, lrs = _rows(log_var)
        out = torch.empty(4, dtype=torch.float32, device=mu.device)
        want = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        pre = (torch.empty((B, L), dtype=torch.float32, device=mu.device),
               torch.empty((B, L), dtype=torch.float32, device=mu.device)) if want else None
        ws = native.workspace(mu.device)
        native.call("ctvae_freebits_kl_forward_grad", mu_.data_ptr(), mrs, lv_.data_ptr(), lrs, B, L, w_dev.data_ptr(), float(scale),
                    float(free_bits), out.data_ptr(), native.ptr(pre[0]) if want else None, native.ptr(pre[1]) if want else None,
                    ws.data_ptr(), ws.numel() * 4)
        ctx.pre = pre
        return _scalar_outputs(ctx, out)

    @staticmethod
    def backward(ctx, g, *_unused):
        if g is None or ctx.pre is None:
            return (None,) * 5
        g_mu, g_lv = ctx.pre
        if not _is_cached_root(g):                    # the rare path: an upstream gradient other than kernels.backward's one
            g_mu, g_lv = g_mu * g, g_lv * g
        return g_mu, g_lv, None, None, None


def free_bits_term(mu, log_var, kwargs, scale=1.0):
    """The KL side of a served model's ``loss_function`` under ``kld_schedule`` / ``kld_free_bits``: FreeBitsKL's four scalars
    when ``kwargs['M_N']`` is a device tensor or ``kwargs`` has ``free_bits``; None for a float ``M_N`` alone (the caller then runs
    exactly what it ran before).  scale: the model's host constant in front of M_N * KL."""
    M_N, has_floor = kwargs['M_N'], 'free_bits' in kwargs
    if not torch.is_tensor(M_N):
        if not has_floor:
            return None
        M_N = torch.full((1,), float(M_N), dtype=torch.float32, device=mu.device)
    return FreeBitsKL.apply(mu, log_var, M_N, scale, kwargs['free_bits'] if has_floor else 0.0)


class GumbelSoftmax(Function):
    """s = softmax((z + g)/temp, dim=-1), g = -log(-log(u + eps) + eps): CategoricalVAE.reparameterize
    (cat_vae.py:118-132) with the uniform draws injectable.  z, u: [..., Q]."""

    @staticmethod
    def forward(ctx, z, u, temp, eps):
        _req_cuda(z, u)
        if z.shape != u.shape:
            raise RuntimeError("gumbel_softmax: logits / uniform shape mismatch")
        z, u = _c(z), _c(u)
        Q = z.shape[-1]
        s = torch.empty_like(z)
        native.call("ctvae_gumbel_softmax_forward", z.data_ptr(), u.data_ptr(), s.data_ptr(), z.numel() // Q, Q, float(temp), float(eps))
        ctx.save_for_backward(s)
        ctx.temp = float(temp)
        return s

    @staticmethod
    def backward(ctx, g_s):
        (s,) = ctx.saved_tensors
        g_s = _c(g_s)
        Q = s.shape[-1]
        g_z = torch.empty_like(s)
        native.call("ctvae_gumbel_softmax_backward", g_s.data_ptr(), s.data_ptr(), g_z.data_ptr(), s.numel() // Q, Q, ctx.temp)
        return g_z, None, None, None


class CatKL(Function):
    """kld = mean_b sum_{d,q} p (log(p + eps) - log(1/Q + eps)), p = softmax(q, -1) (cat_vae.py:147,160-167).  q: [B,D,Q]."""

    @staticmethod
    def forward(ctx, q, eps):
        _req_cuda(q)
        q = _c(q)
        B, Q = q.shape[0], q.shape[-1]
        log_prior = math.log(1.0 / Q + eps)
        out = torch.empty(1, dtype=torch.float32, device=q.device)
        ws = native.workspace(q.device)
        native.call("ctvae_cat_kl_forward", q.data_ptr(), q.numel() // Q, Q, B, float(eps), log_prior, out.data_ptr(),
                    ws.data_ptr(), ws.numel() * 4)
        ctx.save_for_backward(q)
        ctx.meta = (B, Q, float(eps), log_prior)
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        (q,) = ctx.saved_tensors
        B, Q, eps, log_prior = ctx.meta
        g = _c(g.reshape(1))
        g_q = torch.empty_like(q)
        native.call("ctvae_cat_kl_backward", q.data_ptr(), g.data_ptr(), g_q.data_ptr(), q.numel() // Q, Q, B, eps, log_prior)
        return g_q, None


class IWLoss(Function):
    """out = [loss, mean lp, mean kld, -mean kld] of the importance-weighted objective (iwae.py:126-155, miwae.py:130-163):
    recons [R,...] (R = B*M*S rows, same per-image layout as x [B,...]), mu / logvar [R,L], S samples per group.
    Only out[0] carries gradient (through both the softmax weights and the log-weights, as in the reference)."""

    @staticmethod
    def forward(ctx, recons, x, mu, logvar, S, M_N):
        _req_cuda(recons, x, mu, logvar)
        recons, x, mu, logvar = _c(recons), _c(x), _c(mu), _c(logvar)
        R, B = recons.shape[0], x.shape[0]
        n = recons.numel() // R
        if R % B or x.numel() != B * n or mu.shape[0] != R or mu.shape != logvar.shape:
            raise RuntimeError("iw_loss: shape mismatch")
        L = mu.numel() // R
        dev = recons.device
        rows = torch.empty(3, R, dtype=torch.float32, device=dev)      # lp, kld, coef
        out = torch.empty(4, dtype=torch.float32, device=dev)
        native.call("ctvae_iw_loss_forward", recons.data_ptr(), x.data_ptr(), n, R, R // B, mu.data_ptr(), logvar.data_ptr(), L,
                    int(S), float(M_N), rows[0].data_ptr(), rows[1].data_ptr(), rows[2].data_ptr(), out.data_ptr())
        ctx.save_for_backward(recons, x, mu, logvar, rows)
        ctx.meta = (n, R, R // B, L, float(M_N))
        return _scalar_outputs(ctx, out)

    @staticmethod
    def backward(ctx, g_loss, *_unused):
        recons, x, mu, logvar, rows = ctx.saved_tensors
        n, R, rep, L, M_N = ctx.meta
        if g_loss is None:
            return (None,) * 6
        g_loss = _c(g_loss.reshape(1))
        g_r = torch.empty_like(recons) if ctx.needs_input_grad[0] else None
        g_mu = g_lv = None
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            g_mu, g_lv = torch.empty_like(mu), torch.empty_like(logvar)
        native.call("ctvae_iw_loss_backward", recons.data_ptr(), x.data_ptr(), n, R, rep, mu.data_ptr(), logvar.data_ptr(), L, M_N,
                    rows[2].data_ptr(), g_loss.data_ptr(), native.ptr(g_r), native.ptr(g_mu), native.ptr(g_lv))
        return g_r, None, g_mu, g_lv, None, None


class MMD(Function):
    """out = [mmd, K(p,p), K(z,z), K(p,z)] of WAE_MMD / InfoVAE (wae_mmd.py:120-203): z, prior [N,D]; kind 'imq' | 'rbf';
    c = 2*D*latent_var.  Only out[0] carries gradient, and only towards z (the prior draws are constants)."""

    @staticmethod
    def forward(ctx, z, prior, kind, c, w_pp, w_zz, w_pz):
        _req_cuda(z, prior)
        z, prior = _c(z), _c(prior)
        if z.dim() != 2 or z.shape != prior.shape:
            raise RuntimeError("mmd: z / prior must be [N,D] of one shape")
        if kind not in ("imq", "rbf"):
            raise ValueError('Undefined kernel type.')
        N, D = z.shape
        out = torch.empty(4, dtype=torch.float32, device=z.device)
        grad = torch.empty_like(z)
        ws = native.workspace(z.device)
        native.call("ctvae_mmd_forward", z.data_ptr(), prior.data_ptr(), N, D, 0 if kind == "imq" else 1, float(c), 1e-7,
                    float(w_pp), float(w_zz), float(w_pz), out.data_ptr(), grad.data_ptr(), ws.data_ptr(), ws.numel() * 4)
        ctx.save_for_backward(grad)
        return _scalar_outputs(ctx, out)

    @staticmethod
    def backward(ctx, g_mmd, *_unused):
        (grad,) = ctx.saved_tensors
        return (grad * g_mmd if g_mmd is not None else None), None, None, None, None, None, None


L2L1 = -1.0      # VAELoss(..., logcosh_alpha=L2L1): squared + absolute error

_kl_dummy = {}


class GaussKL(Function):
    """mean_b(-0.5 * sum_d(1 + logvar - mu^2 - exp(logvar))): the Gaussian KL term on its own (hvae.py:213-222 forms three of
    them) through the loss kernels: reconstruction operands of four zeros, M_N = 1, so out = {kld, 0, kld, -kld}."""

    @staticmethod
    def forward(ctx, mu, logvar):
        _req_cuda(mu, logvar)
        mu_, mrs = _rows(mu)
        lv_, lrs = _rows(logvar)
        B, L = mu.shape
        z4 = _kl_dummy.get(mu.device)
        if z4 is None:
            z4 = _kl_dummy[mu.device] = torch.zeros(4, dtype=torch.float32, device=mu.device)
        out = torch.empty(4, dtype=torch.float32, device=mu.device)
        ws = native.workspace(mu.device)
        native.call("ctvae_loss_forward", z4.data_ptr(), z4.data_ptr(), 4, mu_.data_ptr(), mrs, lv_.data_ptr(), lrs, B, L, 1.0, None,
                    out.data_ptr(), ws.data_ptr(), ws.numel() * 4)
        ctx.save_for_backward(mu_, lv_)
        ctx.meta = (mrs, lrs, B, L)
        return out[2].clone()

    @staticmethod
    def backward(ctx, g):
        mu_, lv_ = ctx.saved_tensors
        mrs, lrs, B, L = ctx.meta
        g = _c(g.reshape(1))
        g_mu = torch.empty((B, L), dtype=torch.float32, device=mu_.device)
        g_lv = torch.empty((B, L), dtype=torch.float32, device=mu_.device)
        native.call("ctvae_kl_backward", mu_.data_ptr(), mrs, lv_.data_ptr(), lrs, g.data_ptr(), g_mu.data_ptr(), g_lv.data_ptr(), B, L, 1.0)
        return g_mu, g_lv


class LadderMerge(Function):
    """(z, kl) of one LVAE rung (lvae.py:166-204; csrc/ladder.hip): merge of the bottom-up (mu_e, lv_e) and top-down (mu_t, lv_t)
    Gaussians, reparameterised sample with eps, kl [B] between the merged and the bottom-up Gaussian."""

    @staticmethod
    def forward(ctx, mu_e, lv_e, mu_t, lv_t, eps):
        _req_cuda(mu_e, lv_e, mu_t, lv_t, eps)
        mu_e, lv_e, mu_t, lv_t, eps = (_c(t) for t in (mu_e, lv_e, mu_t, lv_t, eps))
        B, D = mu_e.shape
        z = torch.empty_like(mu_e)
        kl = torch.empty(B, dtype=torch.float32, device=mu_e.device)
        native.call("ctvae_ladder_merge_forward", mu_e.data_ptr(), lv_e.data_ptr(), mu_t.data_ptr(), lv_t.data_ptr(), eps.data_ptr(),
                    B, D, z.data_ptr(), kl.data_ptr())
        ctx.save_for_backward(mu_e, lv_e, mu_t, lv_t, eps)
        ctx.set_materialize_grads(False)
        return z, kl

    @staticmethod
    def backward(ctx, gz, gkl):
        mu_e, lv_e, mu_t, lv_t, eps = ctx.saved_tensors
        if gz is None and gkl is None:
            return (None,) * 5
        B, D = mu_e.shape
        gz = _c(gz) if gz is not None else None
        gkl = _c(gkl) if gkl is not None else None
        outs = [torch.empty_like(mu_e) for _ in range(4)]
        native.call("ctvae_ladder_merge_backward", native.ptr(gz), native.ptr(gkl), mu_e.data_ptr(), lv_e.data_ptr(), mu_t.data_ptr(),
                    lv_t.data_ptr(), eps.data_ptr(), B, D, *[o.data_ptr() for o in outs])
        return outs[0], outs[1], outs[2], outs[3], None


class GammaReparam(Function):
    """z = h(alpha + Bs, h^-1(alpha + Bs, zhat)) / beta: GammaVAE.reparameterize (gamma_vae.py:108-149) with the draw
    zhat ~ Gamma(alpha + Bs, 1) given.  csrc/gamma.hip."""

    @staticmethod
    def forward(ctx, alpha, beta, zhat, shape_b):
        _req_cuda(alpha, beta, zhat)
        alpha, beta, zhat = _c(alpha), _c(beta), _c(zhat)
        z = torch.empty_like(alpha)
        native.call("ctvae_gamma_reparam_forward", alpha.data_ptr(), beta.data_ptr(), zhat.data_ptr(), float(shape_b), z.data_ptr(),
                    alpha.numel())
        ctx.save_for_backward(alpha, beta, zhat)
        ctx.shape_b = float(shape_b)
        return z

    @staticmethod
    def backward(ctx, g):
        alpha, beta, zhat = ctx.saved_tensors
        g = _c(g)
        ga, gb = torch.empty_like(alpha), torch.empty_like(alpha)
        native.call("ctvae_gamma_reparam_backward", g.data_ptr(), alpha.data_ptr(), beta.data_ptr(), zhat.data_ptr(), ctx.shape_b,
                    ga.data_ptr(), gb.data_ptr(), alpha.numel())
        return ga, gb, None, None


class GammaKL(Function):
    """mean_b sum_d [I(c,d,c,d) - I(1/alpha, beta, c, d)], c = 1/prior_alpha, d = prior_beta (gamma_vae.py:151-171)."""

    @staticmethod
    def forward(ctx, alpha, beta, prior_alpha, prior_beta):
        _req_cuda(alpha, beta)
        alpha, beta = _c(alpha), _c(beta)
        B, D = alpha.shape
        out = torch.empty(1, dtype=torch.float32, device=alpha.device)
        ws = native.workspace(alpha.device)
        native.call("ctvae_gamma_kl_forward", alpha.data_ptr(), beta.data_ptr(), B, D, float(prior_alpha), float(prior_beta),
                    out.data_ptr(), ws.data_ptr(), ws.numel() * 4)
        ctx.save_for_backward(alpha, beta)
        ctx.prior = (float(prior_alpha), float(prior_beta))
        return out[0]

    @staticmethod
    def backward(ctx, g):
        alpha, beta = ctx.saved_tensors
        B, D = alpha.shape
        g = _c(g.reshape(1))
        ga, gb = torch.empty_like(alpha), torch.empty_like(alpha)
        native.call("ctvae_gamma_kl_backward", g.data_ptr(), alpha.data_ptr(), beta.data_ptr(), B, D, ctx.prior[0], ctx.prior[1],
                    ga.data_ptr(), gb.data_ptr())
        return ga, gb, None, None


class Sigmoid(Function):
    """nn.Sigmoid behind GammaVAE's final conv (gamma_vae.py:78) as an elementwise pair."""

    @staticmethod
    def forward(ctx, x):
        _req_cuda(x)
        x = _c(x)
        y = torch.empty_like(x)
        native.call("ctvae_sigmoid_forward", x.data_ptr(), y.data_ptr(), x.numel())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        g = _c(g)
        gx = torch.empty_like(y)
        native.call("ctvae_sigmoid_backward", g.data_ptr(), y.data_ptr(), gx.data_ptr(), y.numel())
        return gx


class TCDecomp(Function):
    """(mi, tc, kld) of BetaTCVAE's KL decomposition (betatc_vae.py:128-199; csrc/tcvae.hip): z, mu, logvar [B,D] (D <= 32),
    log_iw [B,B] the log importance weights.  All three outputs carry gradient."""

    @staticmethod
    def forward(ctx, z, mu, logvar, log_iw):
        _req_cuda(z, mu, logvar, log_iw)
        z, mu, logvar, log_iw = (_c(t) for t in (z, mu, logvar, log_iw))
        B, D = z.shape
        if mu.shape != z.shape or logvar.shape != z.shape or tuple(log_iw.shape) != (B, B):
            raise RuntimeError("tc decomposition: shapes")
        out = torch.empty(3, dtype=torch.float32, device=z.device)
        lse_s = torch.empty(B, dtype=torch.float32, device=z.device)
        lse_d = torch.empty((B, D), dtype=torch.float32, device=z.device)
        ws = native.workspace(z.device)
        native.call("ctvae_tc_forward", z.data_ptr(), mu.data_ptr(), logvar.data_ptr(), log_iw.data_ptr(), B, D, out.data_ptr(),
                    lse_s.data_ptr(), lse_d.data_ptr(), ws.data_ptr(), ws.numel() * 4)
        ctx.save_for_backward(z, mu, logvar, log_iw, lse_s, lse_d)
        ctx.set_materialize_grads(False)
        return out.unbind(0)

    @staticmethod
    def backward(ctx, g_mi, g_tc, g_kld):
        z, mu, logvar, log_iw, lse_s, lse_d = ctx.saved_tensors
        if g_mi is None and g_tc is None and g_kld is None:
            return None, None, None, None
        zero = torch.zeros((), dtype=torch.float32, device=z.device)
        g3 = torch.stack([(g if g is not None else zero).reshape(()).to(torch.float32) for g in (g_mi, g_tc, g_kld)])
        B, D = z.shape
        dz, dmu, dlv = torch.empty_like(z), torch.empty_like(z), torch.empty_like(z)
        native.call("ctvae_tc_backward", z.data_ptr(), mu.data_ptr(), logvar.data_ptr(), log_iw.data_ptr(), lse_s.data_ptr(),
                    lse_d.data_ptr(), g3.data_ptr(), B, D, dz.data_ptr(), dmu.data_ptr(), dlv.data_ptr())
        return dz, dmu, dlv, None


class VampKL(Function):
    """VampVAE's KL term (vampvae.py:140-171): -(E_log_p - E_log_q) with the VampPrior mixture over the K pseudo-input
    posteriors.  z, mu, logvar [B,D]; prior_mu, prior_logvar [K,D].  csrc/vamp.hip, both directions."""

    @staticmethod
    def forward(ctx, z, mu, logvar, pmu, plv):
        _req_cuda(z, mu, logvar, pmu, plv)
        z, mu, logvar, pmu, plv = (_c(t) for t in (z, mu, logvar, pmu, plv))
        B, D = z.shape
        Kc = pmu.shape[0]
        if mu.shape != z.shape or logvar.shape != z.shape or pmu.shape != (Kc, D) or plv.shape != (Kc, D):
            raise RuntimeError("vamp kl: shapes")
        out = torch.empty(3, dtype=torch.float32, device=z.device)
        wgt = torch.empty((B, Kc), dtype=torch.float32, device=z.device)
        ws = native.workspace(z.device)
        native.call("ctvae_vamp_kl_forward", z.data_ptr(), mu.data_ptr(), logvar.data_ptr(), pmu.data_ptr(), plv.data_ptr(), B, D, Kc,
                    out.data_ptr(), wgt.data_ptr(), ws.data_ptr(), ws.numel() * 4)
        ctx.save_for_backward(z, mu, logvar, pmu, plv, wgt)
        return out[0].clone()

    @staticmethod
    def backward(ctx, g):
        z, mu, logvar, pmu, plv, wgt = ctx.saved_tensors
        B, D = z.shape
        Kc = pmu.shape[0]
        g = _c(g.reshape(1))
        dz, dmu, dlv = torch.empty_like(z), torch.empty_like(z), torch.empty_like(z)
        dpm, dpl = torch.empty_like(pmu), torch.empty_like(pmu)
        native.call("ctvae_vamp_kl_backward", z.data_ptr(), mu.data_ptr(), logvar.data_ptr(), pmu.data_ptr(), plv.data_ptr(),
                    wgt.data_ptr(), g.data_ptr(), B, D, Kc, dz.data_ptr(), dmu.data_ptr(), dlv.data_ptr(), dpm.data_ptr(), dpl.data_ptr())
        return dz, dmu, dlv, dpm, dpl


class SWD(Function):
    """Sliced Wasserstein distance of SWAE.compute_swd (swae.py:150-178): z, prior [N,D]; proj [S,D] unit directions; p the
    exponent; weight = reg_weight.  One launch projects, sorts both sets per direction and leaves d swd / d z (csrc/swd.hip)."""

    @staticmethod
    def forward(ctx, z, prior, proj, p, weight):
        _req_cuda(z, prior, proj)
        z, prior, proj = _c(z), _c(prior), _c(proj)
        if z.dim() != 2 or z.shape != prior.shape or proj.dim() != 2 or proj.shape[1] != z.shape[1]:
            raise RuntimeError("swd: z / prior must be [N,D] of one shape and proj [S,D]")
        N, D = z.shape
        S = proj.shape[0]
        out = torch.empty(1, dtype=torch.float32, device=z.device)
        grad = torch.empty_like(z)
        ws = native.workspace(z.device)
        native.call("ctvae_swd_forward", z.data_ptr(), prior.data_ptr(), proj.data_ptr(), N, D, S, float(p), float(weight),
                    out.data_ptr(), grad.data_ptr(), ws.data_ptr(), ws.numel() * 4)
        ctx.save_for_backward(grad)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None, None, None


class DIPLoss(Function):
    """DIP-VAE II regulariser of dip_vae.py:147-159 on mu / log_var [B,D] (csrc/dip.hip) -> 0-dim tensor."""

    @staticmethod
    def forward(ctx, mu, logvar, lambda_diag, lambda_offdiag):
        _req_cuda(mu, logvar)
        mu_, mrs = _rows(mu)
        lv_, lrs = _rows(logvar)
        B, D = mu.shape
        n = native.load().ctvae_dip_state_floats(B, D)
        state = torch.empty(n, dtype=torch.float32, device=mu.device)
        native.call("ctvae_dip_forward", mu_.data_ptr(), mrs, lv_.data_ptr(), lrs, B, D, float(lambda_diag), float(lambda_offdiag),
                    state.data_ptr())
        ctx.save_for_backward(state)
        ctx.dims = (B, D)
        return state[B * D + D * D + 3 * D].clone()

    @staticmethod
    def backward(ctx, g):
        (state,) = ctx.saved_tensors
        B, D = ctx.dims
        g = _c(g.reshape(1))
        g_mu = torch.empty((B, D), dtype=torch.float32, device=state.device)
        g_lv = torch.empty((B, D), dtype=torch.float32, device=state.device)
        native.call("ctvae_dip_backward", state.data_ptr(), g.data_ptr(), g_mu.data_ptr(), g_lv.data_ptr(), B, D)
        return g_mu, g_lv, None, None


_ones = {}


def _is_cached_root(g):
    """Is g the cached ones tensor kernels.backward() hands to autograd as the root gradient (value 1 by construction)?"""
    one = _ones.get((g.device, g.dtype, tuple(g.shape)))
    return one is not None and g.data_ptr() == one.data_ptr()


class capture_graph:
    """``torch.cuda.graph(g, **kw)`` with Python's cyclic garbage collector switched off for the duration of the capture.
    torch collects once before it begins the capture; a collection that the capture's own allocations trigger in the middle
    can destroy device objects of an earlier owner (another model's graphs and pools) while the stream is capturing -- under
    the capture's global mode that is an illegal call, and it ends in ``Fatal Python error: Aborted`` from a destructor."""

    def __init__(self, graph, **kwargs):
        self._cm = torch.cuda.graph(graph, **kwargs)
        self._was = False

    def __enter__(self):
        import gc
        self._was = gc.isenabled()
        if _DEFER_REDUCE and torch.cuda.is_available():
            _defer_arena_for(torch.device("cuda", torch.cuda.current_device()))   # never from inside the capture (its private pool)
        r = self._cm.__enter__()      # synchronizes, collects, empties the cache, begins the capture
        gc.disable()
        return r

    def __exit__(self, *exc):
        import gc
        try:
            return self._cm.__exit__(*exc)
        finally:
            if self._was:
                gc.enable()


_DEFER_REDUCE = True     # kernels.backward defers the slab reductions to one launch (False: plain loss.backward(); tests assert it is on)
_DEFER_ARENA_BYTES = 2048 << 20     # slab arena of the deferred weight-gradient reductions: 2 GB of the 288
_defer_arena = {}


def _defer_arena_for(device):
    """The slab arena of deferred weight-gradient reductions on this device: 2 GB of the 288, allocated once, outside any graph
    capture (capture_graph makes sure of that: an arena first requested inside a capture would live in that graph's pool)."""
    arena = _defer_arena.get(device)
    if arena is None:
        arena = _defer_arena[device] = torch.empty(_DEFER_ARENA_BYTES // 4, dtype=torch.float32, device=device)
    return arena


def backward(loss):
    """``loss.backward()`` with the root gradient taken from a cached ones tensor: autograd otherwise fills a fresh
    ``ones_like(loss)`` on every call (one launch per step; the harness and bench.py call this).

    The slab reductions behind the weight-gradient kernels are deferred to the end of the pass (ctvae_defer_begin / _flush:
    their slabs go into a 2 GB arena, one launch reduces all of them) -- a parameter gradient is complete when this returns.
    Raises after the pass if a gradient placeholder on offer (_lazy_grads) was not claimed: the gradients of this pass are garbage."""
    key = (loss.device, loss.dtype, tuple(loss.shape))
    one = _ones.get(key)
    if one is None:
        one = _ones[key] = torch.ones_like(loss)
    _lazy_grads.clear()            # placeholders of an earlier pass that nobody claimed (a pass cut short) are not valid in this one
    if not (_DEFER_REDUCE and loss.is_cuda):
        loss.backward(gradient=one)
    else:
        arena = _defer_arena_for(loss.device)
        lib = native.load()
        native.check(lib.ctvae_defer_begin(arena.data_ptr(), arena.numel() * 4), "ctvae_defer_begin")
        try:
            loss.backward(gradient=one)
        finally:
            native.check(lib.ctvae_defer_flush(native.stream_ptr()), "ctvae_defer_flush")
    if _lazy_grads:
        _lazy_grads.clear()
        raise RuntimeError("kernels.backward: a gradient left as split-K slices was never claimed (its tensor had a second consumer)")


class PairMLP(Function):
    """out[b,i,j] = sigmoid(b2 + sum_h w2[h] * leaky_relu(u[b,i,h] + v[b,j,h])): the all-pairs tail of
    ``CausalTransition.graph_discovers[k]`` (ct_mcq_vae.py:86-95,147-151) without the [B,N,N,H] intermediates.
    w2 [H] / b2 [1]: one scorer for the batch; w2 [B,H] / b2 [B]: one scorer per sample (per-action discoverers)."""

    SLOPE = 0.01   # nn.LeakyReLU() default

    @staticmethod
    def forward(ctx, u, v, w2, b2):
        _req_cuda(u, v, w2)
        B, N, H = u.shape
        per_sample = w2.dim() == 2
        if per_sample and (tuple(w2.shape) != (B, H) or b2.numel() != B):
            raise RuntimeError("PairMLP: per-sample scorer needs w2 [B,H] and b2 [B]")
        u, v = _c(u), _c(v)
        w2 = _c(w2) if per_sample else _c(w2.reshape(-1))
        b2 = _c(b2.reshape(-1))
        out = torch.empty((B, N, N), dtype=torch.float32, device=u.device)
        native.call("ctvae_pair_mlp_forward", u.data_ptr(), v.data_ptr(), H, w2.data_ptr(), b2.data_ptr(), out.data_ptr(),
                    B, N, H, PairMLP.SLOPE, 1 if per_sample else 0, None)
        ctx.save_for_backward(u, v, w2, out)
        ctx.per_sample = per_sample
        return out

    @staticmethod
    def backward(ctx, g):
        u, v, w2, out = ctx.saved_tensors
        B, N, H = u.shape
        g = _c(g)
        du, dv = torch.empty_like(u), torch.empty_like(v)
        dw2p = torch.empty((B, H), dtype=torch.float32, device=u.device)
        db2p = torch.empty(B, dtype=torch.float32, device=u.device)
        native.call("ctvae_pair_mlp_backward", u.data_ptr(), v.data_ptr(), H, w2.data_ptr(), out.data_ptr(), g.data_ptr(),
                    du.data_ptr(), dv.data_ptr(), H, dw2p.data_ptr(), db2p.data_ptr(), B, N, H, PairMLP.SLOPE,
                    1 if ctx.per_sample else 0, None)
        if ctx.per_sample:
            return du, dv, dw2p, db2p
        return du, dv, dw2p.sum(0), db2p.sum().reshape(1)


class GATScore(Function):
    """S[b,h,r,c] = sum_k att[h,k] * leaky_relu(xl[b,r,h,k] + xr[b,c,h,k] + attr[b,r,c]*we[h,k], slope): GATv2 attention
    logits on a batch of dense graphs (ct_mcq_vae.py:103-114) without the [B,N,N,C]-per-head intermediates."""

    @staticmethod
    def forward(ctx, xl, xr, attr, we, att, slope):
        _req_cuda(xl, xr, attr, we, att)
        xl, xr, attr, we, att = _c(xl), _c(xr), _c(attr), _c(we), _c(att)
        B, N, H, C = xl.shape
        out = torch.empty((B, H, N, N), dtype=torch.float32, device=xl.device)
        native.call("ctvae_gat_score", 0, xl.data_ptr(), xr.data_ptr(), attr.data_ptr(), we.data_ptr(), att.data_ptr(),
                    out.data_ptr(), B, N, H, C, float(slope))
        ctx.save_for_backward(xl, xr, attr, we, att)
        ctx.slope = float(slope)
        return out

    @staticmethod
    def backward(ctx, g):
        xl, xr, attr, we, att = ctx.saved_tensors
        B, N, H, C = xl.shape
        g = _c(g)
        dxl, dxr = torch.empty_like(xl), torch.empty_like(xr)
        dattp = torch.empty((B, H, C), dtype=torch.float32, device=xl.device)
        dwep = torch.empty((B, H, C), dtype=torch.float32, device=xl.device)
        native.call("ctvae_gat_score_backward", xl.data_ptr(), xr.data_ptr(), attr.data_ptr(), we.data_ptr(), att.data_ptr(),
                    g.data_ptr(), dxl.data_ptr(), dxr.data_ptr(), dattp.data_ptr(), dwep.data_ptr(), B, N, H, C, ctx.slope)
        dattr = None
        if ctx.needs_input_grad[2]:
            t = torch.empty((B, H, N, N), dtype=torch.float32, device=xl.device)
            native.call("ctvae_gat_score", 1, xl.data_ptr(), xr.data_ptr(), attr.data_ptr(), we.data_ptr(), att.data_ptr(),
                        t.data_ptr(), B, N, H, C, ctx.slope)
            dattr = (g * t).sum(1)
        return dxl, dxr, dattr, dwep.sum(0), dattp.sum(0), None


def banked(params) -> bool:
    """True when the same-shaped contiguous tensors lie back to back in memory (FlatParamMixin places a module bank so)."""
    p0 = params[0]
    n = p0.numel() * p0.element_size()
    return all(p.is_contiguous() and p.shape == p0.shape and p.data_ptr() == p0.data_ptr() + k * n for k, p in enumerate(params))


_flat_buffers = []     # [(weakref(flat parameter buffer), weakref(flat gradient buffer))] of the live FlatParamMixin models
_alias_given = {}


def register_flat_buffers(flat, gflat):
    _flat_buffers[:] = [(f, g) for f, g in _flat_buffers if f() is not None and g() is not None]
    _flat_buffers.append((weakref.ref(flat), weakref.ref(gflat)))


_alias_epoch = [-1, -1]   # parameter epoch of the last zero_grad; ... of the last zero_grad that also cleared the torch-level span


def note_zero_grad(prezeroed):
    """FlatParamMixin.zero_grad (after its epoch bump): gradient aliases may be handed out until the epoch moves again (an
    optimizer step without a zero_grad behind it leaves .grad attached, and a kernel writing into the memory autograd is about to
    add to would double the gradient); prezeroed: the whole autograd-managed span of the gradient buffer was cleared in one fill."""
    _alias_epoch[0] = _param_epoch[0]
    _alias_epoch[1] = _param_epoch[0] if prezeroed else -1


def alias_prezeroed():
    return _alias_epoch[1] == _param_epoch[0]


def flat_grad_alias(t):
    """For a contiguous tensor t that lies in a model's flat PARAMETER buffer (a bank of autograd-managed parameters): a fresh
    view of the same range of the flat GRADIENT buffer, for the gradient kernel to write into -- autograd then attaches slices
    of it as the parameters' .grad and gather_torch_grads() has nothing to copy (CT-MCQ-VAE: two multi-tensor copies of 21 and
    18 us per step).  Only in the epoch a zero_grad opened, and once per range: a second writer gets None and a tensor of its
    own, which autograd adds to the first."""
    if t is None or not t.is_contiguous() or _alias_epoch[0] != _param_epoch[0]:
        return None
    for fr, gr in _flat_buffers:
        f, g = fr(), gr()
        if f is None or g is None or f.device != t.device:
            continue
        off = t.data_ptr() - f.data_ptr()
        if off >= 0 and off % 4 == 0 and off + 4 * t.numel() <= 4 * f.numel():
            if _alias_given.get(t.data_ptr()) == _param_epoch[0]:
                return None
            _alias_given[t.data_ptr()] = _param_epoch[0]
            return g.as_strided(tuple(t.shape), tuple(t.stride()), off // 4)
    return None


class BankView(Function):
    """The G same-shaped parameters of a module bank (back to back in memory, see ``banked``) as ONE [G, *shape] tensor
    without a copy; backward hands every parameter its slice of the bank's gradient (views, no copies either)."""

    @staticmethod
    def forward(ctx, *params):
        p0 = params[0]
        if not banked(params):
            raise RuntimeError("BankView: the parameters are not laid out as one bank")
        n = p0.numel()
        return p0.detach().as_strided((len(params),) + tuple(p0.shape), (n,) + tuple(p0.stride()))

    @staticmethod
    def backward(ctx, g):
        return tuple(g[k] for k in range(g.shape[0]))


def glinear_ok(K, N, *lds):
    return K % 4 == 0 and N % 4 == 0 and all(l % 4 == 0 for l in lds)


class GroupLinear(Function):
    """y[b, m, s*N + n] = sum_k x[b, m, k] * W_s[group_s[b]][n][koff_s + k] + bias_s[group_s[b]][n] on blocks of 64 rows per
    sample (csrc/glinear.hip).  x [B,64,K]; spec: per segment (koff, group) with group an int32 [B] tensor or None (everybody
    uses matrix 0); wb: per segment the bank W [G,N,ldw >= koff+K] and its bias [G,N] or None.  Several segments may name the
    same bank: its gradient then arrives once, at the first of them."""

    @staticmethod
    def forward(ctx, x, K, N, spec, *wb):
        import ctypes as C
        _req_cuda(x, *[t for t in wb if t is not None])
        x = _c(x)
        B, M, ldx = x.shape
        nseg = len(spec)
        if M != 64 or ldx != K or len(wb) != 2 * nseg or not 1 <= nseg <= 4:
            raise RuntimeError("GroupLinear: needs x [B,64,K] and (bank, bias) per segment, 1..4 segments")
        Ws, bs, gs = [], [], []
        for s, (koff, grp) in enumerate(spec):
            W, b = wb[2 * s], wb[2 * s + 1]
            if W.dim() != 3 or W.shape[1] != N or W.stride(2) != 1 or koff + K > W.shape[2] or (b is not None and not b.is_contiguous()):
                raise RuntimeError("GroupLinear: bank must be [G,N,ldw] with unit inner stride")
            if grp is not None and (grp.dtype != torch.int32 or grp.numel() != B or not grp.is_contiguous()):
                raise RuntimeError("GroupLinear: group ids must be a contiguous int32 [B] tensor")
            Ws.append(W)
            bs.append(b)
            gs.append(grp)
        for s in range(nseg):            # segments of one bank share one gradient tensor (backward): one bias bank per weight bank
            for t in range(s):
                if Ws[t].data_ptr() == Ws[s].data_ptr() and bs[t] is not None and bs[s] is not None and bs[t].data_ptr() != bs[s].data_ptr():
                    raise RuntimeError("GroupLinear: segments that name the same weight bank must name the same bias bank")
        y = torch.empty((B, 64, nseg * N), dtype=torch.float32, device=x.device)
        ctx.host = (
            (C.c_void_p * nseg)(*[W.data_ptr() + 4 * spec[s][0] for s, W in enumerate(Ws)]),
            (C.c_int * nseg)(*[W.stride(1) for W in Ws]),
            (C.c_int64 * nseg)(*[W.stride(0) for W in Ws]),
            (C.c_void_p * nseg)(*[native.ptr(b) for b in bs]),
            (C.c_int * nseg)(*[(b.shape[-1] if b is not None else 0) for b in bs]),
            (C.c_void_p * nseg)(*[native.ptr(g) for g in gs]),
        )
        h = ctx.host
        native.call("ctvae_glinear_forward", x.data_ptr(), ldx, K, nseg, N, h[0], h[1], h[2], h[3], h[4], h[5], y.data_ptr(),
                    nseg * N, B)
        ctx.save_for_backward(x, *[t for t in Ws], *[g for g in gs if g is not None])
        ctx.meta = (K, N, nseg, tuple(k for k, _ in spec), tuple(g is not None for g in gs), tuple(b is not None for b in bs))
        ctx.bias_banks = bs
        return y

    @staticmethod
    def backward(ctx, g):
        K, N, nseg, koffs, has_g, has_b = ctx.meta
        saved = ctx.saved_tensors
        x, Ws = saved[0], saved[1:1 + nseg]
        grp_it = iter(saved[1 + nseg:])
        gs = [next(grp_it) if hg else None for hg in has_g]
        g = _c(g)
        B = x.shape[0]
        h = ctx.host
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            native.call("ctvae_glinear_dgrad", g.data_ptr(), nseg * N, nseg, N, h[0], h[1], h[2], h[5], dx.data_ptr(), K, K, B)
        ws = native.workspace(x.device)
        # Segments that name the SAME bank (the discoverers' first layers: columns 0..D-1 / D..2D-1, matrix 0 for everybody and
        # matrix 1 + action per sample) write into ONE gradient tensor per bank, zero-filled once and accumulated into by each
        # segment's launch; the first segment's input slot carries it, the others return None.  (As separate tensors autograd
        # added them: a fill per segment and an add per extra segment over 5 MB each.)
        grads = [None] * (2 * nseg)
        shared = {}
        for s in range(nseg):
            W = Ws[s]
            G = W.shape[0]
            if not ctx.needs_input_grad[4 + 2 * s]:
                continue
            key = (W.data_ptr(), tuple(W.shape), tuple(W.stride()))
            ent = shared.get(key)
            users = [t for t in range(nseg) if Ws[t].data_ptr() == W.data_ptr() and ctx.needs_input_grad[4 + 2 * t]]
            # a segment that covers its bank completely (all columns, every group) WRITES it: when that is the bank's first
            # user -- with its bias, if the bank has one -- there is no zero fill; everybody after it accumulates
            whole = (ent is None and koffs[s] == 0 and W.shape[2] == K and (gs[s] is not None or G == 1)
                     and (has_b[s] or not any(has_b[t] for t in users)))
            if ent is None:
                dW = flat_grad_alias(W)              # the bank's own range of the flat gradient buffer, where there is one
                if dW is None:
                    dW = (torch.empty_like if whole else torch.zeros_like)(W, memory_format=torch.contiguous_format)
                elif not whole and not alias_prezeroed():
                    dW.zero_()
                db = None
                if any(has_b[t] for t in users):
                    bt = next(ctx.bias_banks[t] for t in users if has_b[t])
                    db = flat_grad_alias(bt) if tuple(bt.shape) == (G, N) else None
                    if db is None:
                        db = (torch.empty if whole else torch.zeros)((G, N), dtype=torch.float32, device=x.device)
                    elif not whole and not alias_prezeroed():
                        db.zero_()
                ent = shared[key] = (dW, db)
                grads[2 * s] = dW
                if db is not None:           # the bias gradient goes to the first segment of this bank that has a bias input
                    t = next(t for t in range(nseg) if Ws[t].data_ptr() == W.data_ptr() and has_b[t])
                    grads[2 * t + 1] = db
            dW, db = ent
            Gk = G if gs[s] is not None else 1        # no group ids: only matrix 0 is used
            native.call("ctvae_glinear_wgrad", x.data_ptr(), K, K, g.data_ptr(), nseg * N, s * N, N, native.ptr(gs[s]), Gk, B,
                        dW.data_ptr() + 4 * koffs[s], dW.stride(1), native.ptr(db) if has_b[s] else None, 0 if whole else 1,
                        ws.data_ptr(), ws.numel() * 4)
        return (dx, None, None, None) + tuple(grads)


class PairScores(Function):
    """Edge scores of every ordered node pair for the all-sample discoverer 0 and (grp given) the discoverer of each sample's
    action, from the projections uv [B,64,nd*2*H] = [u0 | v0 | u_a | v_a] (GroupLinear), reading the scorer bank w2 [G,H] / b2 [G]
    in place: out [nd,B,64,64], out[d][b,i,j] = sigmoid(b2 + sum_h w2[h] * lrelu(u[b,i,h] + v[b,j,h])) (csrc/pairmlp.hip;
    ct_mcq_vae.py:86-95,147-151)."""

    @staticmethod
    def forward(ctx, uv, w2, b2, grp, H):
        _req_cuda(uv, w2, b2)
        uv, w2, b2 = _c(uv), _c(w2), _c(b2)
        B, N, ld = uv.shape
        nd = 2 if grp is not None else 1
        if N != 64 or ld != nd * 2 * H or w2.shape[-1] != H:
            raise RuntimeError("PairScores: uv must be [B,64,nd*2*H]")
        out = torch.empty((nd, B, 64, 64), dtype=torch.float32, device=uv.device)
        p = uv.data_ptr()
        native.call("ctvae_pair_mlp_forward", p, p + 4 * H, ld, w2.data_ptr(), b2.data_ptr(), out[0].data_ptr(), B, 64, H,
                    PairMLP.SLOPE, 0, None)
        if nd == 2:
            native.call("ctvae_pair_mlp_forward", p + 8 * H, p + 12 * H, ld, w2.data_ptr(), b2.data_ptr(), out[1].data_ptr(), B, 64,
                        H, PairMLP.SLOPE, 1, grp.data_ptr())
        ctx.save_for_backward(uv, w2, b2, grp, out)
        ctx.H = H
        return out

    @staticmethod
    def backward(ctx, g):
        uv, w2, b2, grp, out = ctx.saved_tensors
        H = ctx.H
        B, _, ld = uv.shape
        nd = out.shape[0]
        G = w2.shape[0]
        g = _c(g)
        d_uv = torch.empty_like(uv)
        dw2p = torch.empty((nd, B, H), dtype=torch.float32, device=uv.device)
        db2p = torch.empty((nd, B), dtype=torch.float32, device=uv.device)
        p, d = uv.data_ptr(), d_uv.data_ptr()
        native.call("ctvae_pair_mlp_backward", p, p + 4 * H, ld, w2.data_ptr(), out[0].data_ptr(), g[0].data_ptr(), d, d + 4 * H, ld,
                    dw2p[0].data_ptr(), db2p[0].data_ptr(), B, 64, H, PairMLP.SLOPE, 0, None)
        # per-sample partials -> rows of the scorer bank: discoverer 0 takes every sample, discoverer grp[b] sample b (in order,
        # no atomics; as torch ops this was one_hot^T @ parts plus the fills / casts / cats around it)
        dw2 = flat_grad_alias(w2) if tuple(w2.shape) == (G, H) else None
        db2 = flat_grad_alias(b2) if tuple(b2.shape) == (G,) else None
        if dw2 is None:
            dw2 = torch.empty((G, H), dtype=torch.float32, device=uv.device)
        if db2 is None:
            db2 = torch.empty((G,), dtype=torch.float32, device=uv.device)
        native.call("ctvae_group_rowsum", dw2p[0].data_ptr(), 0, 1, B, H, H, None, G, dw2.data_ptr(), 0)
        native.call("ctvae_group_rowsum", db2p[0].data_ptr(), 0, 1, B, 1, 1, None, G, db2.data_ptr(), 0)
        if nd == 2:
            native.call("ctvae_pair_mlp_backward", p + 8 * H, p + 12 * H, ld, w2.data_ptr(), out[1].data_ptr(), g[1].data_ptr(),
                        d + 8 * H, d + 12 * H, ld, dw2p[1].data_ptr(), db2p[1].data_ptr(), B, 64, H, PairMLP.SLOPE, 1, grp.data_ptr())
            native.call("ctvae_group_rowsum", dw2p[1].data_ptr(), 0, 1, B, H, H, grp.data_ptr(), G, dw2.data_ptr(), 1)
            native.call("ctvae_group_rowsum", db2p[1].data_ptr(), 0, 1, B, 1, 1, grp.data_ptr(), G, db2.data_ptr(), 1)
        return d_uv, dw2, db2, None, None


class GATLayer(Function):
    """One GATv2Conv layer on B dense graphs over the 64 latent nodes (csrc/gatlayer.hip; ct_mcq_vae.py:103-114): scores,
    masked softmax over the sources and the alpha-weighted aggregation in one launch.

    xlr [B,64,2*Hs*C]: lin_l(x) of the Hs head slots, then lin_r(x) (one GEMM output); adj [B,64,64] weighted adjacency
    (adj[b,r,c] != 0: edge r -> c); we / att [H,C], bias [H*C]; head_map int32 [B,Hs] or None (slot == head).
    Returns act(out) [B,64,Hs*C]."""

    @staticmethod
    def forward(ctx, xlr, adj, we, att, bias, head_map, Hs, C, slope, act):
        _req_cuda(xlr, adj, we, att, bias)
        xlr, adj, we, att, bias = _c(xlr), _c(adj), _c(we), _c(att), _c(bias)
        B, N, ld = xlr.shape
        if N != 64 or ld != 2 * Hs * C or tuple(adj.shape) != (B, 64, 64):
            raise RuntimeError("GATLayer: needs xlr [B,64,2*Hs*C] and adj [B,64,64]")
        if head_map is not None:
            head_map = _c(head_map.to(torch.int32))
            if tuple(head_map.shape) != (B, Hs):
                raise RuntimeError("GATLayer: head_map must be [B,Hs]")
        out = torch.empty((B, 64, Hs * C), dtype=torch.float32, device=xlr.device)
        alpha = torch.empty((B, Hs, 64, 64), dtype=torch.float32, device=xlr.device)
        native.call("ctvae_gat_layer_forward", xlr.data_ptr(), xlr.data_ptr() + 4 * Hs * C, ld, adj.data_ptr(), we.data_ptr(),
                    att.data_ptr(), bias.data_ptr(), native.ptr(head_map), out.data_ptr(), Hs * C, alpha.data_ptr(), B, Hs, C,
                    float(slope), int(act))
        ctx.save_for_backward(xlr, adj, we, att, bias, head_map, out, alpha)
        ctx.meta = (Hs, C, float(slope), int(act))
        return out

    @staticmethod
    def backward(ctx, g):
        xlr, adj, we, att, bias, head_map, out, alpha = ctx.saved_tensors
        Hs, C, slope, act = ctx.meta
        B, _, ld = xlr.shape
        H = we.shape[0]
        g = _c(g)
        dev = xlr.device
        scratch = torch.empty((2, B, Hs, 64, 64), dtype=torch.float32, device=dev)
        d_xlr = torch.empty_like(xlr)
        parts = torch.empty((3, B * Hs, C), dtype=torch.float32, device=dev)
        dadj = torch.empty_like(adj) if ctx.needs_input_grad[1] else None
        native.call("ctvae_gat_layer_backward", xlr.data_ptr(), xlr.data_ptr() + 4 * Hs * C, ld, adj.data_ptr(), we.data_ptr(),
                    att.data_ptr(), bias.data_ptr(), native.ptr(head_map), out.data_ptr(), Hs * C, alpha.data_ptr(), g.data_ptr(),
                    scratch[0].data_ptr(), scratch[1].data_ptr(), d_xlr.data_ptr(), d_xlr.data_ptr() + 4 * Hs * C, ld,
                    parts[0].data_ptr(), parts[1].data_ptr(), parts[2].data_ptr(), native.ptr(dadj), 0, B, Hs, C, slope, act)
        if head_map is None:
            red = parts.view(3, B, Hs * C).sum(1).view(3, H, C)
        else:   # per-head sums of the per-(sample, slot) partials, in row order (deterministic, no atomics): one launch
            red = torch.empty((3, H, C), dtype=torch.float32, device=dev)
            native.call("ctvae_group_rowsum", parts.data_ptr(), B * Hs * C, 3, B * Hs, C, C, head_map.data_ptr(), H, red.data_ptr(), 0)
        return d_xlr, dadj, red[2], red[1], red[0].reshape(-1), None, None, None, None, None


class CTActionReg(Function):
    """beta * adjacency_KL_loss(adj) + delta * graph_size_loss(graph) + epsilon * positive_trial_loss(adj) of
    CausalTransition.forward_action (ct_mcq_vae.py:275,314-323) in one launch each way (csrc/ctmisc.hip).  adj, graph [B,64,64];
    uni [B,4096]: the uniform draws behind the KL target softmax(rand)."""

    @staticmethod
    def forward(ctx, adj, graph, uni, beta, delta, epsilon):
        _req_cuda(adj, graph, uni)
        adj, graph, uni = _c(adj), _c(graph), _c(uni)
        B, N, _ = adj.shape
        part = torch.empty((B, 4), dtype=torch.float32, device=adj.device)
        ctx.coef = (float(beta) / B, float(delta) / B, float(epsilon) / B)
        native.call("ctvae_ct_reg_forward", adj.data_ptr(), graph.data_ptr(), uni.data_ptr(), part.data_ptr(), ctx.coef[0],
                    ctx.coef[1], ctx.coef[2], B, N)
        ctx.save_for_backward(adj, graph, uni, part)
        return part[:, 3].sum()

    @staticmethod
    def backward(ctx, g):
        adj, graph, uni, part = ctx.saved_tensors
        B, N, _ = adj.shape
        g = _c(g.reshape(1))
        d_adj, d_graph = torch.empty_like(adj), torch.empty_like(graph)
        native.call("ctvae_ct_reg_backward", adj.data_ptr(), graph.data_ptr(), uni.data_ptr(), part.data_ptr(), g.data_ptr(),
                    ctx.coef[0], ctx.coef[1], ctx.coef[2], d_adj.data_ptr(), d_graph.data_ptr(), B, N)
        return d_adj, d_graph, None, None, None, None


class BlendSoftmax(Function):
    """softmax_d(y[..., 0, :] * (1 - mask) + y[..., 1, :] * mask) (two head slots) or softmax_d(y[..., 0, :]) (one): the tail of
    CausalTransition._compute_y (ct_mcq_vae.py:226-228).  y [B,S,Hs,D], mask [B,S,1] or None -> [B,S,D]."""

    @staticmethod
    def forward(ctx, y, mask):
        _req_cuda(y)
        y = _c(y)
        B, S, Hs, D = y.shape
        m = _c(mask.reshape(B * S)) if mask is not None else None
        probs = torch.empty((B, S, D), dtype=torch.float32, device=y.device)
        native.call("ctvae_ct_blend_softmax_forward", y.data_ptr(), native.ptr(m), probs.data_ptr(), B * S, Hs, D)
        ctx.save_for_backward(y, m, probs)
        ctx.mask_shape = tuple(mask.shape) if mask is not None else None
        return probs

    @staticmethod
    def backward(ctx, g):
        y, m, probs = ctx.saved_tensors
        B, S, Hs, D = y.shape
        g = _c(g)
        dy = torch.empty_like(y)
        dm = torch.empty(B * S, dtype=torch.float32, device=y.device) if (m is not None and ctx.needs_input_grad[1]) else None
        native.call("ctvae_ct_blend_softmax_backward", g.data_ptr(), probs.data_ptr(), y.data_ptr(), native.ptr(m), dy.data_ptr(),
                    native.ptr(dm), B * S, Hs, D)
        return dy, (dm.view(ctx.mask_shape) if dm is not None else None)


class LatentCE(Function):
    """F.cross_entropy(log(clamp(p, 1e-4)), target) over node rows (latent_CrossEntropy_loss, ct_mcq_vae.py:306-311).
    probs [R,D] rows contiguous, target int64 [R]."""

    @staticmethod
    def forward(ctx, probs, target):
        _req_cuda(probs, target)
        probs, target = _c(probs), _c(target)
        R, D = probs.shape
        rows = torch.empty(R, dtype=torch.float32, device=probs.device)
        native.call("ctvae_ct_latent_ce_forward", probs.data_ptr(), target.data_ptr(), rows.data_ptr(), R, D)
        ctx.save_for_backward(probs, target)
        return rows.mean()

    @staticmethod
    def backward(ctx, g):
        probs, target = ctx.saved_tensors
        R, D = probs.shape
        g = _c(g.reshape(1))
        d = torch.empty_like(probs)
        native.call("ctvae_ct_latent_ce_backward", probs.data_ptr(), target.data_ptr(), g.data_ptr(), d.data_ptr(), R, D)
        return d, None


class CTMask(Function):
    """CausalTransition._compute_mask (ct_mcq_vae.py:117-127) in one launch each way (csrc/ctmisc.hip): x [B,64,64] (one-hot
    latent, no gradient), action [B,A], pe [64,64], keep [B,64,64] or None (dropout keep mask of the positional encoding),
    W [64,A+64] / bias [64] (mask.0), expo [B,64,2] exponential draws -> straight-through sample [B,64]."""

    @staticmethod
    def forward(ctx, x, action, pe, keep, scale, W, bias, expo):
        _req_cuda(x, action, pe, W, bias, expo)
        x, action, pe, W, bias, expo = _c(x), _c(action), _c(pe), _c(W), _c(bias), _c(expo)
        keep = _c(keep) if keep is not None else None
        B, S, D = x.shape
        A = action.shape[1]
        dev = x.device
        inter = torch.empty((B, S, D), dtype=torch.float32, device=dev)
        psoft = torch.empty((3, B, S), dtype=torch.float32, device=dev)      # p, sample, soft
        native.call("ctvae_ct_mask_forward", x.data_ptr(), action.data_ptr(), pe.data_ptr(), native.ptr(keep), float(scale),
                    W.data_ptr(), bias.data_ptr(), expo.data_ptr(), B, S, D, A, inter.data_ptr(), psoft[0].data_ptr(),
                    psoft[1].data_ptr(), psoft[2].data_ptr())
        ctx.save_for_backward(x, action, pe, keep, inter, psoft)
        ctx.scale = float(scale)
        return psoft[1]

    @staticmethod
    def backward(ctx, g):
        x, action, pe, keep, inter, psoft = ctx.saved_tensors
        B, S, D = x.shape
        A = action.shape[1]
        g = _c(g)
        dWp = torch.empty((B, A + D, D), dtype=torch.float32, device=x.device)
        dbp = torch.empty((B, D), dtype=torch.float32, device=x.device)
        native.call("ctvae_ct_mask_backward", x.data_ptr(), action.data_ptr(), pe.data_ptr(), native.ptr(keep), ctx.scale,
                    inter.data_ptr(), psoft[0].data_ptr(), psoft[2].data_ptr(), g.data_ptr(), B, S, D, A, dWp.data_ptr(), dbp.data_ptr())
        return None, None, None, None, None, dWp.sum(0).t(), dbp.sum(0), None


class PosEncode(Function):
    """(x + pe) * keep * scale: PositionalEncoding.forward (ct_mcq_vae.py:33-38) with the dropout mask given; x [B,S,D],
    pe [S,D], keep [B,S,D] or None."""

    @staticmethod
    def forward(ctx, x, pe, keep, scale):
        _req_cuda(x, pe)
        x, pe = _c(x), _c(pe)
        keep = _c(keep) if keep is not None else None
        if x.numel() % pe.numel() or pe.numel() % 4 or (keep is not None and keep.shape != x.shape):
            raise RuntimeError("PosEncode: shapes")
        out = torch.empty_like(x)
        native.call("ctvae_ct_posenc_forward", x.data_ptr(), pe.data_ptr(), native.ptr(keep), float(scale), out.data_ptr(), x.numel(),
                    pe.numel())
        ctx.save_for_backward(keep)
        ctx.scale = float(scale)
        return out

    @staticmethod
    def backward(ctx, g):
        (keep,) = ctx.saved_tensors
        if keep is None:
            return g, None, None, None
        g = _c(g)
        gx = torch.empty_like(g)
        native.call("ctvae_ct_posenc_backward", g.data_ptr(), keep.data_ptr(), ctx.scale, gx.data_ptr(), g.numel())
        return gx, None, None, None


def one_hot_f32(inds, N):
    """F.one_hot(inds, N).float() in one launch; inds int64 (any shape) -> [..., N] float32."""
    _req_cuda(inds)
    inds = _c(inds)
    if inds.dtype != torch.int64 or N % 4:
        return torch.nn.functional.one_hot(inds, N).to(torch.float32)
    out = torch.empty(tuple(inds.shape) + (N,), dtype=torch.float32, device=inds.device)
    native.call("ctvae_one_hot", inds.data_ptr(), inds.numel(), N, out.data_ptr())
    return out


class MaskBlend(Function):
    """adj = s[0] * (1 - mask) + s[1] * mask (CausalTransition._compute_adj, ct_mcq_vae.py:153): s [2,B,64,64] the scores of
    discoverer 0 and of each sample's own discoverer (PairScores), mask [B,64,1]; one launch each way (csrc/ctmisc.hip)."""

    @staticmethod
    def forward(ctx, s, mask):
        _req_cuda(s, mask)
        s, mask = _c(s), _c(mask)
        if s.dim() != 4 or s.shape[0] != 2 or s.shape[-1] != 64 or mask.numel() * 64 != s[0].numel():
            raise RuntimeError("MaskBlend: needs s [2,B,64,64] and one mask value per row of 64")
        out = torch.empty_like(s[0])
        native.call("ctvae_ct_blend_forward", s[0].data_ptr(), s[1].data_ptr(), mask.data_ptr(), out.data_ptr(), mask.numel())
        ctx.save_for_backward(s, mask)
        return out

    @staticmethod
    def backward(ctx, g):
        s, mask = ctx.saved_tensors
        g = _c(g)
        gs = torch.empty_like(s)
        gm = torch.empty_like(mask)
        native.call("ctvae_ct_blend_backward", g.data_ptr(), s[0].data_ptr(), s[1].data_ptr(), mask.data_ptr(), gs[0].data_ptr(),
                    gs[1].data_ptr(), gm.data_ptr(), mask.numel())
        return gs, gm


class CTSample(Function):
    """Straight-through Bernoulli(p) from exponential draws expo [...,2] (what F.gumbel_softmax draws: Gumbel = -log E;
    ct_mcq_vae.py:180-183) -> sample, and with ``weighted`` also p * sample (weighted_graph, :244,271) from the same launch."""

    @staticmethod
    def forward(ctx, p, expo, weighted):
        _req_cuda(p, expo)
        p, expo = _c(p), _c(expo)
        out = torch.empty_like(p)
        soft = torch.empty_like(p)
        w = torch.empty_like(p) if weighted else None
        native.call("ctvae_ct_sample_forward", p.data_ptr(), expo.data_ptr(), out.data_ptr(), soft.data_ptr(), native.ptr(w), p.numel())
        ctx.save_for_backward(p, soft, out)
        ctx.set_materialize_grads(False)
        return (out, w) if weighted else out

    @staticmethod
    def backward(ctx, g_s, g_w=None):
        p, soft, out = ctx.saved_tensors
        if g_s is None and g_w is None:
            return None, None, None
        g_s = _c(g_s) if g_s is not None else None
        g_w = _c(g_w) if g_w is not None else None
        gp = torch.empty_like(p)
        native.call("ctvae_ct_sample_backward", native.ptr(g_s), native.ptr(g_w), p.data_ptr(), soft.data_ptr(), out.data_ptr(),
                    gp.data_ptr(), p.numel())
        return gp, None, None


class GumbelBernoulliST(Function):
    """Straight-through Bernoulli(p) sample via hard 2-class Gumbel-softmax (ct_mcq_vae.py:177-183); noise [...,2]."""

    @staticmethod
    def forward(ctx, p, noise):
        _req_cuda(p, noise)
        p, noise = _c(p), _c(noise)
        out = torch.empty_like(p)
        soft = torch.empty_like(p)
        native.call("ctvae_gumbel_st_forward", p.data_ptr(), noise.data_ptr(), out.data_ptr(), soft.data_ptr(), p.numel())
        ctx.save_for_backward(p, soft)
        return out

    @staticmethod
    def backward(ctx, g):
        p, soft = ctx.saved_tensors
        g = _c(g)
        gp = torch.empty_like(p)
        native.call("ctvae_gumbel_st_backward", g.data_ptr(), p.data_ptr(), soft.data_ptr(), gp.data_ptr(), p.numel())
        return gp, None


# ---------------------------------------------------------------------------------------------------
# vector quantiser
# ---------------------------------------------------------------------------------------------------
def vq_compute_inds(latents_nhwc, codebooks, K, C):
    """latents [B,H,W,D] -> int64 [B,C,H,W] (mcq_vae.py:26-39,100-110).  No gradient (arg-min)."""
    _req_cuda(latents_nhwc)
    lat = _c(latents_nhwc.detach())
    B, H, W, D = lat.shape
    inds = torch.empty((B, C, H, W), dtype=torch.int64, device=lat.device)
    native.call("ctvae_vq_inds", lat.data_ptr(), codebooks[0].data_ptr(), inds.data_ptr(), B, H * W, D, K, C)
    return inds


class VQLookup(Function):
    """(quantized [B,H,W,D], vq_loss scalar) = compute_latents(latents, inds) (mcq_vae.py:41-64,112-127)."""

    @staticmethod
    def forward(ctx, latents, inds, beta, K, C, *codebooks):
        _req_cuda(latents, inds)
        lat = _c(latents)
        inds = _c(inds)
        B, H, W, D = lat.shape
        q = torch.empty_like(lat)
        vq_loss = torch.empty((), dtype=torch.float32, device=lat.device)
        ws = native.workspace(lat.device)
        native.call("ctvae_vq_lookup", lat.data_ptr(), codebooks[0].data_ptr(), inds.data_ptr(), q.data_ptr(),
                    vq_loss.data_ptr(), float(beta), B, H * W, D, K, C, ws.data_ptr(), ws.numel() * 4)
        ctx.meta = (float(beta), K, C)
        ctx.codebooks = codebooks
        ctx.save_for_backward(lat, inds)
        return q, vq_loss

    @staticmethod
    def backward(ctx, g_q, g_vq):
        lat, inds = ctx.saved_tensors
        beta, K, C = ctx.meta
        B, H, W, D = lat.shape
        g_q = _c(g_q) if g_q is not None else None
        g_vq = _c(g_vq) if g_vq is not None else None
        g_lat = torch.empty_like(lat) if ctx.needs_input_grad[0] else None
        cb0 = ctx.codebooks[0]
        dcb = None
        acc = 0
        if g_vq is not None and cb0.requires_grad:
            flags = [grad_target(cb) for cb in ctx.codebooks]
            if any(f[1] != flags[0][1] for f in flags):
                for (gt, a) in flags:
                    if a == 0:
                        gt.zero_()
                acc = 1
            else:
                acc = flags[0][1]
            dcb = flags[0][0]
            for i in range(1, C):
                if flags[i][0].data_ptr() != dcb.data_ptr() + i * cb0.numel() * 4:
                    raise RuntimeError("codebook gradients must be stored back to back (flat gradient buffer)")
        ws = native.workspace(lat.device)
        native.call("ctvae_vq_backward", native.ptr(g_q), native.ptr(g_vq), lat.data_ptr(), cb0.data_ptr(), inds.data_ptr(),
                    native.ptr(g_lat), native.ptr(dcb), acc, beta, B, H * W, D, K, C, ws.data_ptr(), ws.numel() * 4)
        return (g_lat, None, None, None, None) + (None,) * len(ctx.codebooks)


class VQLookupEMA(Function):
    """``VQLookup`` for EMA codebooks (exp_params.codebook_ema_decay): vq_loss = beta * sum_c mse_c, the commitment term alone
    (ctvae_vq_lookup_commit), and no codebook gradient -- the backward pass is ctvae_vq_backward's null-``d_codebooks`` path, so
    the codebooks' block of the flat gradient buffer is never asked for and stays an absent block.  The quantised latents and the
    latent gradient are bit for bit ``VQLookup``'s."""

    @staticmethod
    def forward(ctx, latents, inds, beta, K, C, *codebooks):
        _req_cuda(latents, inds)
        lat = _c(latents)
        inds = _c(inds)
        B, H, W, D = lat.shape
        q = torch.empty_like(lat)
        vq_loss = torch.empty((), dtype=torch.float32, device=lat.device)
        ws = native.workspace(lat.device)
        native.call("ctvae_vq_lookup_commit", lat.data_ptr(), codebooks[0].data_ptr(), inds.data_ptr(), q.data_ptr(),
                    vq_loss.data_ptr(), float(beta), B, H * W, D, K, C, ws.data_ptr(), ws.numel() * 4)
        ctx.meta = (float(beta), K, C)
        ctx.codebooks = codebooks
        ctx.save_for_backward(lat, inds)
        return q, vq_loss

    @staticmethod
    def backward(ctx, g_q, g_vq):
        lat, inds = ctx.saved_tensors
        beta, K, C = ctx.meta
        B, H, W, D = lat.shape
        g_q = _c(g_q) if g_q is not None else None
        g_vq = _c(g_vq) if g_vq is not None else None
        g_lat = torch.empty_like(lat) if ctx.needs_input_grad[0] else None
        if g_lat is not None:
            ws = native.workspace(lat.device)
            native.call("ctvae_vq_backward", native.ptr(g_q), native.ptr(g_vq), lat.data_ptr(), ctx.codebooks[0].data_ptr(),
                        inds.data_ptr(), g_lat.data_ptr(), None, 0, beta, B, H * W, D, K, C, ws.data_ptr(), ws.numel() * 4)
        return (g_lat, None, None, None, None) + (None,) * len(ctx.codebooks)


# ---------------------------------------------------------------------------------------------------
# flat fused Adam
# ---------------------------------------------------------------------------------------------------
_mssim_host = None


def _mssim_host_arrays():
    """(window, weights) as HOST float arrays for ctvae_mssim_*: the window exactly as the reference builds it
    (mssim_vae.py:203-206: exp(+(x - 5)^2 / (2 * 1.5^2)) in float32, normalised), the level weights of mssim_vae.py:252."""
    global _mssim_host
    if _mssim_host is None:
        import ctypes
        from math import exp
        k = torch.tensor([exp((x - 11 // 2) ** 2 / (2 * 1.5 ** 2)) for x in range(11)])
        k = (k / k.sum()).float()
        win = (ctypes.c_float * 11)(*[float(v) for v in k])
        wts = (ctypes.c_float * 5)(0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
        _mssim_host = (win, wts)
    return _mssim_host


class MSSIMLoss(Function):
    """MSSIM.forward (mssim_vae.py:250-279) of NHWC pictures [B,64,64,C]: 1 - prod of the level powers, five SSIM levels with
    the reference's 11-tap window; the gradient goes to the first picture only (the second is the input image)."""

    @staticmethod
    def forward(ctx, recons, target):
        _req_cuda(recons, target)
        r, x = _c(recons), _c(target)
        B, H, W, C = r.shape
        if tuple(x.shape) != (B, H, W, C) or H != 64 or W != 64:
            raise RuntimeError("MSSIMLoss: NHWC pictures of 64 x 64 pixels (five levels down to 4 x 4, mssim_vae.py:255-266)")
        win, wts = _mssim_host_arrays()
        lib = native.load()
        part = torch.empty(int(lib.ctvae_mssim_part_floats(B, C)), dtype=torch.float32, device=r.device)
        out = torch.empty(11, dtype=torch.float32, device=r.device)          # [0] loss, [1..10] per-level coefficients
        native.call("ctvae_mssim_forward", r.data_ptr(), x.data_ptr(), win, wts, part.data_ptr(), out.data_ptr(),
                    out.data_ptr() + 4, B, C, H, W)
        ctx.save_for_backward(r, x, out)
        return out[0].clone()

    @staticmethod
    def backward(ctx, g):
        r, x, out = ctx.saved_tensors
        B, H, W, C = r.shape
        win, _ = _mssim_host_arrays()
        g_r = torch.empty_like(r)
        native.call("ctvae_mssim_backward", r.data_ptr(), x.data_ptr(), win, out.data_ptr() + 4, _c(g).data_ptr(), g_r.data_ptr(),
                    B, C, H, W)
        return g_r, None


def adam_state(head, device):
    """The device state of ctvae_adam_step: head = [step, lr, beta1, beta2, eps, weight_decay, beta1^step, beta2^step], followed
    by the kernel's zeroed ticket counters (ctvae_adam_state_floats() floats in all).  On the CPU (the gloo tests run a test
    double of the kernel): just the head."""
    dev = torch.device(device)
    if dev.type != "cuda":
        return torch.tensor(head, dtype=torch.float32, device=dev)
    st = torch.zeros(int(native.load().ctvae_adam_state_floats()), dtype=torch.float32, device=dev)
    st[:8] = torch.tensor(head, dtype=torch.float32)
    return st


def adam_step(flat_params, flat_grads, exp_avg, exp_avg_sq, state, grad_scale=1.0):
    _req_cuda(flat_params, flat_grads)
    bump_param_epoch()
    native.call("ctvae_adam_step", flat_params.data_ptr(), flat_grads.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                state.data_ptr(), flat_params.numel(), float(grad_scale))


CLIP_ALGORITHMS = {"norm": 0, "value": 1}          # CTVAE_CLIP_NORM / CTVAE_CLIP_VALUE


def grad_clip_workspace(device):
    """The partial sums of ctvae_adam_step_clipped's norm pass (ctvae_grad_clip_workspace_floats() floats).  On the CPU (the
    gloo tests run a test double of the kernel): an empty tensor."""
    dev = torch.device(device)
    if dev.type != "cuda":
        return torch.zeros(0, dtype=torch.float32, device=dev)
    return torch.zeros(int(native.load().ctvae_grad_clip_workspace_floats()), dtype=torch.float32, device=dev)


def adam_step_clipped(flat_params, flat_grads, exp_avg, exp_avg_sq, state, grad_scale, algorithm, clip_val, workspace=None,
                      norm_out=None):
    """adam_step on the gradient clipped as torch.nn.utils.clip_grad_norm_ (algorithm "norm": the pre-clip norm of
    flat_grads * grad_scale goes to norm_out, a one-float device tensor) or clip_grad_value_ ("value") would clip it."""
    _req_cuda(flat_params, flat_grads)
    bump_param_epoch()
    native.call("ctvae_adam_step_clipped", flat_params.data_ptr(), flat_grads.data_ptr(), exp_avg.data_ptr(),
                exp_avg_sq.data_ptr(), state.data_ptr(), flat_params.numel(), float(grad_scale), CLIP_ALGORITHMS[algorithm],
                float(clip_val), native.ptr(workspace), native.ptr(norm_out))


CLIP_OFF = 2                                       # CTVAE_ADAM_NO_CLIP
ABSENT_GRAD_MODES = ("zero", "skip", "skip_until_first")


class AdamBlockTable:
    """Device side of FlatAdam's block table (``absent_grad`` "skip" / "skip_until_first", ctvae_adam_step_blocks): sorted int32
    ``lo`` / ``hi`` offsets of the blocks inside the optimizer's slice of ``n`` floats, ``hit_index`` (a bank member's word of
    the hit vector, -1 for every other block), ``state`` [nb, 4] = (step, beta1^step, beta2^step, seen) per block and the
    ``active`` flags the step fills and reads."""

    def __init__(self, ranges, hit_index, n, nhits, device):
        prev = 0
        for lo, hi in ranges:
            if not prev <= lo < hi <= n:
                raise ValueError(f"block table: [{lo}, {hi}) is empty, overlaps its predecessor or leaves the {n} floats")
            prev = hi
        if not ranges or n >= 2 ** 31 or len(hit_index) != len(ranges) or any(h >= nhits for h in hit_index):
            raise ValueError("block table: needs at least one block, fewer than 2^31 floats and one hit index per block")
        dev = torch.device(device)
        self.nb, self.n, self.nhits = len(ranges), int(n), int(nhits)
        self.lo = torch.tensor([r[0] for r in ranges], dtype=torch.int32, device=dev)
        self.hi = torch.tensor([r[1] for r in ranges], dtype=torch.int32, device=dev)
        self.hit_index = torch.tensor(list(hit_index), dtype=torch.int32, device=dev)
        self.hits = torch.zeros(max(self.nhits, 1), dtype=torch.int32, device=dev)
        self.state = torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float32, device=dev).repeat(self.nb, 1)
        self.active = torch.zeros(self.nb, dtype=torch.int32, device=dev)


def adam_mark_members(hits, group=None):
    """Forward side of a parameter bank: member 0 and every member ``group`` (int32 [B]) names were used in this step."""
    _req_cuda(hits, group)
    native.call("ctvae_adam_mark_members", hits.data_ptr(), hits.numel(), native.ptr(group), 0 if group is None else group.numel())


def adam_block_flags_local(table, present):
    """First half of adam_step_blocks' flags for a step whose flags are reduced across ranks: table.active[b] = present[b],
    for a bank member and its hit word -- this rank's gradients alone, whatever the blocks' history.  Consumes the hit words."""
    _req_cuda(table.active, present)
    if present.numel() != table.nb or present.dtype != torch.int32:
        raise ValueError("adam_block_flags_local: present is one int32 word per block of the table")
    native.call("ctvae_adam_block_flags_local", present.data_ptr(), table.hit_index.data_ptr(), table.hits.data_ptr(), table.nhits,
                table.active.data_ptr(), table.nb)


def adam_block_flags_finish(table, mode):
    """Second half, on the reduced table.active in place: "skip_until_first" adds the blocks that have stepped before.  After
    it adam_step_blocks runs with ``flags_final=True``."""
    if mode not in ABSENT_GRAD_MODES[1:]:
        raise ValueError("adam_block_flags_finish: mode is 'skip' or 'skip_until_first'")
    _req_cuda(table.active)
    native.call("ctvae_adam_block_flags_finish", table.state.data_ptr(), table.active.data_ptr(), table.nb,
                1 if mode == "skip_until_first" else 0)


def adam_step_blocks(flat_params, flat_grads, exp_avg, exp_avg_sq, state, table, present, mode, grad_scale=1.0, algorithm=None,
                     clip_val=None, workspace=None, norm_out=None, flags_final=False):
    """adam_step / adam_step_clipped (algorithm None / "norm" / "value") on the blocks of ``table`` that have a gradient in this
    step, every block under its own step counter; the others keep parameter, moments and counter.  present: int32 [nb] device
    tensor, what the host knows of the blocks' gradients; a bank member also needs its hit word (adam_mark_members).
    mode: "skip" or "skip_until_first".  flags_final: table.active already holds the step's flags (adam_block_flags_local, the
    caller's reduction, adam_block_flags_finish); the flags launch is left out and ``present`` is not read (may be None)."""
    if not flat_params.is_cuda:
        raise RuntimeError(f"FlatAdam absent_grad={mode!r} needs device tensors: the block-aware step (ctvae_adam_step_blocks) "
                           "is a HIP kernel, there is no CPU fallback and no CPU test double of it")
    _req_cuda(flat_grads, table.active if flags_final else present)
    if mode not in ABSENT_GRAD_MODES[1:] or flat_params.numel() != table.n or (not flags_final and present.numel() != table.nb):
        raise ValueError("adam_step_blocks: mode is 'skip' or 'skip_until_first'; table and present flags must fit the buffers")
    bump_param_epoch()
    if not flags_final:
        native.call("ctvae_adam_block_flags", present.data_ptr(), table.hit_index.data_ptr(), table.hits.data_ptr(), table.nhits,
                    table.state.data_ptr(), table.active.data_ptr(), table.nb, 1 if mode == "skip_until_first" else 0)
    native.call("ctvae_adam_step_blocks", flat_params.data_ptr(), flat_grads.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                state.data_ptr(), flat_params.numel(), float(grad_scale), CLIP_OFF if algorithm is None else CLIP_ALGORITHMS[algorithm],
                0.0 if clip_val is None else float(clip_val), native.ptr(workspace), native.ptr(norm_out), table.lo.data_ptr(),
                table.hi.data_ptr(), table.state.data_ptr(), table.active.data_ptr(), table.nb)


GRAD_ACCUM_MODES = {"store": 0, "add": 1, "finish": 2}          # CTVAE_ACCUM_STORE / _ADD / _FINISH


def grad_accumulate(acc, grads, mode):
    """One micro-batch of a gradient-accumulation window (ctvae_grad_accumulate), on two equally long fp32 vectors: "store"
    acc = grads, "add" acc += grads, "finish" grads = acc + grads (the window's sum lands in the gradient buffer, acc stays)."""
    _req_cuda(acc, grads)
    if acc.numel() != grads.numel() or acc.dtype != torch.float32 or grads.dtype != torch.float32 \
            or not (acc.is_contiguous() and grads.is_contiguous()):
        raise ValueError("grad_accumulate: acc and grads are contiguous fp32 vectors of one length")
    native.call("ctvae_grad_accumulate", acc.data_ptr(), grads.data_ptr(), acc.numel(), GRAD_ACCUM_MODES[mode])


def grad_accumulator_like(grads):
    """A zeroed accumulator for ``grads`` (a slice of the flat gradient buffer) that sits at the same offset from a 16-byte
    boundary as the slice does, so that grad_accumulate runs its 16-byte loop on both."""
    n = grads.numel()
    buf = torch.zeros(n + 3, dtype=torch.float32, device=grads.device)
    shift = ((grads.data_ptr() - buf.data_ptr()) // 4) % 4
    return buf[shift:shift + n]


def _same_fp32_vectors(what, a, b):
    _req_cuda(a, b)
    if a.numel() != b.numel() or a.dtype != torch.float32 or b.dtype != torch.float32 \
            or not (a.is_contiguous() and b.is_contiguous()):
        raise ValueError(f"{what}: both arguments are contiguous fp32 vectors of one length")


def ema_update(ema, params, one_minus_decay):
    """One step of a weight average (ctvae_ema_update): ema = fmaf(one_minus_decay, params - ema, ema) per element; ``params`` is
    read only.  one_minus_decay: a float inside (0, 1), handed to the launch by value."""
    _same_fp32_vectors("ema_update", ema, params)
    native.call("ctvae_ema_update", ema.data_ptr(), params.data_ptr(), ema.numel(), float(one_minus_decay))


def buffer_swap(a, b):
    """Exchange the contents of two equally long fp32 vectors word for word (ctvae_buffer_swap).  The caller bumps the parameter
    epoch when one of them holds parameters."""
    _same_fp32_vectors("buffer_swap", a, b)
    native.call("ctvae_buffer_swap", a.data_ptr(), b.data_ptr(), a.numel())


# ---------------------------------------------------------------------------------------------------
# codebook usage and dead-code restarts (csrc/vqusage.hip; optim.CodebookUsage)
# ---------------------------------------------------------------------------------------------------
VQ_USAGE_MAX_K, VQ_USAGE_MAX_WORDS = 512, 8192      # what ctvae_vq_usage covers: K <= 512 and C * K <= 8192 (its LDS histogram)


def vq_usage_supported(K, C):
    return 1 <= K <= VQ_USAGE_MAX_K and C >= 1 and C * K <= VQ_USAGE_MAX_WORDS


def _req_dense(what, name, t, dtype):
    if not torch.is_tensor(t) or t.dtype != dtype:
        raise ValueError(f"{what}: {name} must be a {dtype} tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be contiguous")


def vq_usage_pass_indices() -> int:
    """The indices one turn of the usage kernel's grid covers; a longer index tensor runs its grid-stride loop."""
    return int(native.load().ctvae_vq_usage_pass_indices())


def _vq_usage_args(what, inds, counts, invalid):
    """The checks of ``vq_usage`` and its launch arguments (inds, counts, invalid, B, C, HW, K)."""
    for name, t in (("inds", inds), ("counts", counts), ("invalid", invalid)):
        _req_dense(what, name, t, torch.int64)
    if inds.dim() < 3 or counts.dim() != 2 or invalid.numel() != 1 or inds.size(1) != counts.size(0) or inds.numel() == 0:
        raise ValueError(f"{what}: inds [B, C, ...] {tuple(inds.shape)}, counts [C, K] {tuple(counts.shape)} and invalid [1] "
                         f"{tuple(invalid.shape)} do not fit together")
    C, K = counts.shape
    if not vq_usage_supported(K, C):
        raise ValueError(f"{what}: num_embeddings K={K} with C={C} codebooks is not covered: the kernel needs 1 <= K <= "
                         f"{VQ_USAGE_MAX_K} and C * K <= {VQ_USAGE_MAX_WORDS}")
    _req_cuda(inds, counts, invalid)
    B = inds.size(0)
    return inds.data_ptr(), counts.data_ptr(), invalid.data_ptr(), B, C, inds.numel() // (B * C), K


def _vq_pool_fill_args(what, latents_nhwc, pool):
    """The checks of ``vq_pool_fill`` and its launch arguments (latents, pool, P, D, R)."""
    for name, t in (("latents", latents_nhwc), ("pool", pool)):
        _req_dense(what, name, t, torch.float32)
    if pool.dim() != 2 or latents_nhwc.dim() < 2 or latents_nhwc.size(-1) != pool.size(1) or latents_nhwc.numel() == 0 \
            or pool.numel() == 0:
        raise ValueError(f"{what}: latents [..., D] {tuple(latents_nhwc.shape)} and pool [R, D] {tuple(pool.shape)} do not "
                         "fit together")
    _req_cuda(latents_nhwc, pool)
    R, D = pool.shape
    return latents_nhwc.data_ptr(), pool.data_ptr(), latents_nhwc.numel() // D, D, R


def vq_usage(inds, counts, invalid):
    """counts[c][k] += the number of entries of inds[:, c] equal to k (ctvae_vq_usage).  inds: int64 [B, C, ...] as
    ``vq_compute_inds`` returns it; counts: int64 [C, K]; invalid: one int64 word that counts the indices outside [0, K).  A wrong
    dtype or shape, a non-contiguous tensor or a (K, C) outside ``vq_usage_supported`` raises a ValueError that names it, before
    any launch."""
    native.call("ctvae_vq_usage", *_vq_usage_args("vq_usage", inds, counts, invalid))


def vq_pool_fill(latents_nhwc, pool) -> int:
    """The first min(P, R) rows of the NHWC latents [..., D] (P rows) into the front of ``pool`` [R, D], word for word
    (ctvae_vq_pool_fill); returns that row count, which the host knows from the shapes alone."""
    args = _vq_pool_fill_args("vq_pool_fill", latents_nhwc, pool)
    native.call("ctvae_vq_pool_fill", *args)
    return min(args[2], args[4])


def vq_usage_pool_fill(inds, counts, invalid, latents_nhwc, pool) -> int:
    """``vq_usage`` and ``vq_pool_fill`` in one launch (ctvae_vq_usage_pool_fill): what a training forward issues.  Everything
    is checked before the launch; returns the pool rows filled."""
    what = "vq_usage_pool_fill"
    args = _vq_pool_fill_args(what, latents_nhwc, pool)
    native.call("ctvae_vq_usage_pool_fill", *_vq_usage_args(what, inds, counts, invalid), *args)
    return min(args[2], args[4])


def _restart_entries(what, entries, C, K, valid_rows):
    """The (c, k, row) list as a host int64 [n, 3] tensor, every entry inside its range (K None: k is not checked)."""
    ent = torch.as_tensor(entries, dtype=torch.int64, device="cpu").reshape(-1, 3)
    if ent.numel():
        hi = torch.tensor([C, K if K is not None else (1 << 62), valid_rows], dtype=torch.int64)
        bad = ((ent < 0) | (ent >= hi)).any(dim=1).nonzero()
        if bad.numel():
            c, k, row = ent[int(bad[0])].tolist()
            raise ValueError(f"{what}: entry {int(bad[0])} (c={c}, k={k}, row={row}) is out of range: c < {C}, "
                             + (f"k < {K}, " if K is not None else "") + f"row < {valid_rows} valid pool rows")
    return ent


def _restart_shapes(what, pool, valid_rows, C, Dc):
    _req_dense(what, "pool", pool, torch.float32)
    if pool.dim() != 2 or not 0 <= valid_rows <= pool.size(0) or C - 1 + Dc > pool.size(1):
        raise ValueError(f"{what}: pool [R, D] {tuple(pool.shape)} does not hold {valid_rows} valid rows of C - 1 + Dc = "
                         f"{C - 1 + Dc} channels")


def vq_restart_gather(entries, pool, valid_rows, C, Dc):
    """rows[i] = pool[row_i][c_i : c_i + Dc) for the (c, k, row) entries (ctvae_vq_restart_gather): a new fp32 [n, Dc] tensor --
    the first half of a data-parallel restart, whose rows rank 0 then broadcasts."""
    _restart_shapes("vq_restart_gather", pool, valid_rows, C, Dc)
    ent = _restart_entries("vq_restart_gather", entries, C, None, valid_rows)
    _req_cuda(pool)
    rows = torch.empty((ent.size(0), Dc), dtype=torch.float32, device=pool.device)
    if ent.size(0):
        dev_ent = ent.to(pool.device)
        native.call("ctvae_vq_restart_gather", dev_ent.data_ptr(), ent.size(0), pool.data_ptr(), int(valid_rows), pool.size(1), C, Dc,
                    rows.data_ptr())
    return rows


def vq_restart(entries, pool, valid_rows, codebooks, exp_avg, exp_avg_sq, rows=None):
    """Restart the listed codes (ctvae_vq_restart).  entries: (c, k, row) triples, a list or a host int64 [n, 3] tensor;
    codebooks / exp_avg / exp_avg_sq: fp32 [C, K, Dc] views of the flat parameter buffer and of the two Adam moments at the same
    offsets.  For every entry E_c[k][:] = pool[row][c : c + Dc) -- the channels codebook c is compared against -- or, with
    ``rows`` ([n, Dc], ``vq_restart_gather``'s), = rows[i]; both moments of those elements become 0.  Everything is checked on
    the host before the launch: a wrong dtype, a non-contiguous tensor or an entry out of range raises a ValueError that names
    it and nothing is written.  No entries: no launch.  The caller bumps the parameter epoch."""
    what = "vq_restart"
    for name, t in (("codebooks", codebooks), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        _req_dense(what, name, t, torch.float32)
    if codebooks.dim() != 3 or exp_avg.shape != codebooks.shape or exp_avg_sq.shape != codebooks.shape:
        raise ValueError(f"{what}: codebooks, exp_avg and exp_avg_sq are [C, K, Dc] tensors of one shape, got "
                         f"{tuple(codebooks.shape)}, {tuple(exp_avg.shape)}, {tuple(exp_avg_sq.shape)}")
    C, K, Dc = codebooks.shape
    if rows is None:
        _restart_shapes(what, pool, valid_rows, C, Dc)
        ent = _restart_entries(what, entries, C, K, valid_rows)
    else:
        _req_dense(what, "rows", rows, torch.float32)
        ent = _restart_entries(what, entries, C, K, 1 << 62)
        if tuple(rows.shape) != (ent.size(0), Dc):
            raise ValueError(f"{what}: rows must be [n, Dc] = {(ent.size(0), Dc)}, got {tuple(rows.shape)}")
    if len({tuple(e) for e in ent[:, :2].tolist()}) != ent.size(0):
        raise ValueError(f"{what}: a code (c, k) is listed twice")
    _req_cuda(codebooks, exp_avg, exp_avg_sq, rows if rows is not None else pool)
    if ent.size(0) == 0:
        return
    dev_ent = ent.to(codebooks.device)
    D = pool.size(1) if rows is None else C - 1 + Dc      # (with rows the pool's width is not read: the least the launcher accepts)
    native.call("ctvae_vq_restart", dev_ent.data_ptr(), ent.size(0), native.ptr(pool if rows is None else None),
                int(valid_rows) if rows is None else 0, D, native.ptr(rows), codebooks.data_ptr(), exp_avg.data_ptr(),
                exp_avg_sq.data_ptr(), C, K, Dc)


# ---------------------------------------------------------------------------------------------------
# EMA codebooks (csrc/vqema.hip; optim.CodebookEMA)
# ---------------------------------------------------------------------------------------------------
VQ_EMA_MAX_K, VQ_EMA_MAX_C, VQ_EMA_MAX_DC = 16384, 8, 256      # what ctvae_vq_ema_stats / ctvae_vq_ema_update cover


def vq_ema_supported(K, C, Dc):
    return 1 <= K <= VQ_EMA_MAX_K and 1 <= C <= VQ_EMA_MAX_C and 1 <= Dc <= VQ_EMA_MAX_DC


def _vq_ema_accumulators(what, acc_n, acc_s):
    """The checks both EMA wrappers make of the window accumulators; returns (C, K, Dc)."""
    _req_dense(what, "acc_n", acc_n, torch.int64)
    _req_dense(what, "acc_s", acc_s, torch.float32)
    if acc_n.dim() != 2 or acc_s.dim() != 3 or tuple(acc_s.shape[:2]) != tuple(acc_n.shape) or acc_s.numel() == 0:
        raise ValueError(f"{what}: acc_n [C, K] {tuple(acc_n.shape)} and acc_s [C, K, Dc] {tuple(acc_s.shape)} do not fit "
                         "together")
    C, K, Dc = acc_s.shape
    if not vq_ema_supported(K, C, Dc):
        raise ValueError(f"{what}: K={K}, C={C}, Dc={Dc} is not covered: the kernels need 1 <= K <= {VQ_EMA_MAX_K}, C <= "
                         f"{VQ_EMA_MAX_C} and Dc <= {VQ_EMA_MAX_DC}")
    return C, K, Dc


def vq_ema_stats(latents_nhwc, inds, acc_n, acc_s, invalid):
    """The EMA statistics of one micro-batch, added to the window accumulators (ctvae_vq_ema_stats): acc_n[c][k] += the number of
    positions with inds[:, c] == k, acc_s[c][k][d] += the sum of latents[p][c + d] over those positions (the slice quirk).
    latents: fp32 [..., D] NHWC with D = C * Dc; inds: int64 [B, C, ...] as ``vq_compute_inds`` returns it; acc_n int64 [C, K],
    acc_s fp32 [C, K, Dc], invalid one int64 word (indices outside [0, K)).  A wrong dtype or shape, a non-contiguous tensor or
    an uncovered (K, C, Dc) raises a ValueError that names it, before any launch."""
    what = "vq_ema_stats"
    C, K, Dc = _vq_ema_accumulators(what, acc_n, acc_s)
    _req_dense(what, "latents", latents_nhwc, torch.float32)
    _req_dense(what, "inds", inds, torch.int64)
    _req_dense(what, "invalid", invalid, torch.int64)
    if inds.dim() < 3 or inds.size(1) != C or inds.numel() == 0 or invalid.numel() != 1 or latents_nhwc.dim() < 2 \
            or latents_nhwc.size(-1) != C * Dc or latents_nhwc.numel() // (C * Dc) * C != inds.numel():
        raise ValueError(f"{what}: latents [..., D = {C * Dc}] {tuple(latents_nhwc.shape)}, inds [B, C = {C}, ...] "
                         f"{tuple(inds.shape)} and invalid [1] {tuple(invalid.shape)} do not fit together")
    _req_cuda(latents_nhwc, inds, acc_n, acc_s, invalid)
    B = inds.size(0)
    ws = native.workspace(latents_nhwc.device)
    native.call("ctvae_vq_ema_stats", latents_nhwc.data_ptr(), inds.data_ptr(), acc_n.data_ptr(), acc_s.data_ptr(),
                invalid.data_ptr(), B, inds.numel() // (B * C), C * Dc, K, C, ws.data_ptr(), ws.numel() * 4)


def vq_ema_update(codebooks, N, M, acc_n, acc_s, decay, eps):
    """The EMA codebook update behind an optimizer step (ctvae_vq_ema_update): N = decay N + (1 - decay) acc_n, M likewise from
    acc_s, E = M / Ntilde with the Laplace-smoothed cluster sizes, every code overwritten, the accumulators zeroed in the same
    launch.  codebooks / M / acc_s: fp32 [C, K, Dc]; N fp32 [C, K]; acc_n int64 [C, K]; decay in (0, 1) and eps > 0 are handed
    over by value (as fp32).  Checked before the launch like ``vq_ema_stats``.  The caller bumps the parameter epoch."""
    what = "vq_ema_update"
    C, K, Dc = _vq_ema_accumulators(what, acc_n, acc_s)
    for name, t in (("codebooks", codebooks), ("N", N), ("M", M)):
        _req_dense(what, name, t, torch.float32)
    if tuple(codebooks.shape) != (C, K, Dc) or tuple(M.shape) != (C, K, Dc) or tuple(N.shape) != (C, K):
        raise ValueError(f"{what}: codebooks {tuple(codebooks.shape)} and M {tuple(M.shape)} must be [C, K, Dc] = {(C, K, Dc)}, "
                         f"N {tuple(N.shape)} [C, K]")
    if isinstance(decay, bool) or not 0.0 < float(decay) < 1.0 or isinstance(eps, bool) or not float(eps) > 0.0:
        raise ValueError(f"{what}: decay {decay!r} must lie in (0, 1) and eps {eps!r} above 0")
    _req_cuda(codebooks, N, M, acc_n, acc_s)
    native.call("ctvae_vq_ema_update", codebooks.data_ptr(), N.data_ptr(), M.data_ptr(), acc_n.data_ptr(), acc_s.data_ptr(),
                C, K, Dc, float(decay), float(eps))


def adam_flags_window(window, table, mode):
    """The block-activity words of one micro-batch (table.active, after adam_block_flags_local) against the window's
    (ctvae_adam_flags_window): "store" window = active, "add" window = max(window, active), "finish" active = max(window,
    active) -- what adam_block_flags_finish and adam_step_blocks(flags_final=True) then read."""
    _req_cuda(window, table.active)
    if window.numel() != table.nb or window.dtype != torch.int32:
        raise ValueError("adam_flags_window: window is one int32 word per block of the table")
    native.call("ctvae_adam_flags_window", window.data_ptr(), table.active.data_ptr(), table.nb, GRAD_ACCUM_MODES[mode])


# ---------------------------------------------------------------------------------------------------
# gradient tracking: per-parameter norms and histograms from the flat gradient buffer (csrc/gradstat.hip)
# ---------------------------------------------------------------------------------------------------
GRAD_HIST_BINS = 64
_GUARD_WORD = 0x5A5A5A5A


def _guarded(sizes, guard, device):
    """One int32 buffer holding regions of ``sizes`` words, each between ``guard`` words of _GUARD_WORD (the first region starts
    on an 8-byte boundary); returns the buffer and the regions' (lo, hi)."""
    guard = (int(guard) + 1) // 2 * 2
    spans, cur = [], guard
    for n in sizes:
        spans.append((cur, cur + n))
        cur += n + guard
    raw = torch.full((max(cur, 1),), _GUARD_WORD, dtype=torch.int32, device=device)
    for lo, hi in spans:
        raw[lo:hi] = 0
    return raw, spans


def _guards_intact(raw, spans):
    keep = torch.ones(raw.numel(), dtype=torch.bool)
    for lo, hi in spans:
        keep[lo:hi] = False
    return bool((raw.cpu()[keep] == _GUARD_WORD).all())


class GradSegmentTable:
    """Device side of the gradient-tracking kernels (ctvae_grad_segment_stats / _hist), everything allocated once: the segment
    descriptors ``segments`` = [(base, rows, period, col_lo, width)] inside a gradient range of ``n`` floats (the elements
    base + r * period + col_lo + c; FlatParamMixin.grad_segments, offsets relative to the range), the chunk list made from them
    (``chunk_seg``, ``chunk_first``, ``seg_chunk_begin``: every segment's rows * width elements in pieces of
    ctvae_grad_segment_chunk_floats()), the per-chunk partials and the outputs.  The outputs are regions of ONE int32 buffer,
    ``raw``, so that ``fetch()`` is one device-to-host copy: ``out_sum`` float64 [nseg, 2] (sum |v|^p, max |v|), ``out_range``
    float32 [nseg, 2] (finite min, max), ``out_bad`` int32 [nseg] (non-finite count), ``out_hist`` int32 [nseg, 64] and
    ``out_flags`` int32 [nflags] (the caller's block flags, copied along).  guard: words of a fixed pattern around every region of
    the outputs and the partials (``guards_intact()``).  On the CPU the table can be built and inspected; the launches cannot run
    there."""

    def __init__(self, segments, n, device, nflags=0, guard=0):
        segs = [tuple(int(v) for v in s) for s in segments]
        if not segs or n >= 2 ** 40 or nflags < 0:
            raise ValueError("segment table: needs at least one segment")
        spans = []
        for base, rows, period, col_lo, width in segs:
            first, end = base + col_lo, base + (rows - 1) * period + col_lo + width
            if min(base, col_lo) < 0 or rows < 1 or width < 1 or (rows > 1 and col_lo + width > period) or end > n:
                raise ValueError(f"segment table: segment {(base, rows, period, col_lo, width)} is malformed or leaves the {n} floats")
            spans.append((first, end, base, rows, period, col_lo, width))
        spans.sort()
        for a, b in zip(spans, spans[1:]):
            if a[1] > b[0] and not (a[2:5] == b[2:5] and a[5] + a[6] <= b[5]):
                raise ValueError(f"segment table: segments {a[2:]} and {b[2:]} overlap")
        chunk = int(native.load().ctvae_grad_segment_chunk_floats())
        chunk_seg, chunk_first, begin = [], [], [0]
        for s, (_, rows, _, _, width) in enumerate(segs):
            for first in range(0, rows * width, chunk):
                chunk_seg.append(s)
                chunk_first.append(first)
            begin.append(len(chunk_seg))
        dev = torch.device(device)
        self.nseg, self.n, self.nflags, self.nchunks, self.chunk = len(segs), int(n), int(nflags), len(chunk_seg), chunk
        self.segments = torch.tensor(segs, dtype=torch.int64, device=dev)
        self.chunk_seg = torch.tensor(chunk_seg, dtype=torch.int32, device=dev)
        self.chunk_first = torch.tensor(chunk_first, dtype=torch.int64, device=dev)
        self.seg_chunk_begin = torch.tensor(begin, dtype=torch.int32, device=dev)
        ns, nc = self.nseg, self.nchunks
        self.raw, self._spans = _guarded([4 * ns, 2 * ns, ns, GRAD_HIST_BINS * ns, self.nflags], guard, dev)
        self.ws, self._ws_spans = _guarded([2 * nc, 3 * nc, nc], guard, dev)
        self.out_sum, self.out_range, self.out_bad, self.out_hist, self.out_flags = self._views(self.raw)
        (a, b), (c, d), (e, f) = self._ws_spans
        self.part_sum, self.part_f, self.part_bad = self.ws[a:b].view(torch.float64), self.ws[c:d].view(torch.float32), self.ws[e:f]

    def _views(self, raw):
        (a, b), (c, d), (e, f), (g, h), (i, j) = self._spans
        return (raw[a:b].view(torch.float64).view(self.nseg, 2), raw[c:d].view(torch.float32).view(self.nseg, 2), raw[e:f],
                raw[g:h].view(self.nseg, GRAD_HIST_BINS), raw[i:j])

    def fetch(self):
        """The outputs on the host, by ONE device-to-host copy: (sum [nseg, 2] float64, range [nseg, 2] float32, bad [nseg],
        hist [nseg, 64], flags [nflags])."""
        return self._views(self.raw.cpu())

    def guards_intact(self) -> bool:
        return _guards_intact(self.raw, self._spans) and _guards_intact(self.ws, self._ws_spans)


def _grad_segment_args(table, grads):
    _req_cuda(grads, table.raw)
    if grads.dtype != torch.float32 or grads.dim() != 1 or not grads.is_contiguous() or grads.numel() != table.n:
        raise ValueError(f"gradient tracking: grads is the contiguous fp32 range of {table.n} floats the table was built for")


def grad_segment_stats(table, grads, scale=1.0, norm_type=2.0, flags=None):
    """ctvae_grad_segment_stats: for every segment of ``table`` over v = fl32(grads * scale): sum |v|^norm_type in double and
    max |v| (``out_sum``), finite min / max (``out_range``), the non-finite count (``out_bad``); zeroes ``out_hist``.  Two launches.
    flags: int32 [table.nflags] device words copied into ``out_flags`` by the second launch.  norm_type travels as fp32."""
    _grad_segment_args(table, grads)
    norm_type = float(norm_type)
    if not norm_type > 0:
        raise ValueError(f"gradient tracking: norm_type {norm_type!r} must be > 0 (inf: the largest magnitude)")
    if (flags is None) != (table.nflags == 0) or (flags is not None and (flags.dtype != torch.int32 or flags.numel() != table.nflags
                                                                         or not flags.is_cuda or not flags.is_contiguous())):
        raise ValueError(f"gradient tracking: flags is {table.nflags} contiguous int32 device words (None for 0)")
    native.call("ctvae_grad_segment_stats", grads.data_ptr(), table.n, float(scale), norm_type, table.segments.data_ptr(),
                table.nseg, table.chunk_seg.data_ptr(), table.chunk_first.data_ptr(), table.seg_chunk_begin.data_ptr(),
                table.nchunks, table.part_sum.data_ptr(), table.part_f.data_ptr(), table.part_bad.data_ptr(),
                table.out_sum.data_ptr(), table.out_range.data_ptr(), table.out_bad.data_ptr(), table.out_hist.data_ptr(),
                native.ptr(flags), table.out_flags.data_ptr() if table.nflags else None, table.nflags)


def grad_segment_hist(table, grads, scale=1.0):
    """ctvae_grad_segment_hist, behind grad_segment_stats with the same ``grads`` and ``scale``: the finite values of every
    segment into the 64 bins between its finished min and max (torch.histc's rule on the CPU, in fp32).  One launch."""
    _grad_segment_args(table, grads)
    native.call("ctvae_grad_segment_hist", grads.data_ptr(), table.n, float(scale), table.segments.data_ptr(), table.nseg,
                table.chunk_seg.data_ptr(), table.chunk_first.data_ptr(), table.nchunks, table.out_range.data_ptr(),
                table.out_hist.data_ptr())


# ---------------------------------------------------------------------------------------------------
# latent usage of the Gaussian models (csrc/latentstat.hip; latentstats.LatentStats)
# ---------------------------------------------------------------------------------------------------
LATENT_MAX_L = 1024                      # what ctvae_latent_accumulate covers: cov_sum is L * L doubles
LATENT_STATE = (("kl_sum", torch.float64, 1), ("mu_sum", torch.float64, 1), ("sig2_sum", torch.float64, 1),
                ("cov_sum", torch.float64, 2), ("nonfinite", torch.int32, 1), ("rows", torch.int32, 0))


def _latent_rows(t, L):
    """A [B, L] fp32 tensor as (tensor to keep alive, row pitch in floats): its own memory when the columns are unit-stride and
    the rows at least L floats apart -- a column half of a [B, 2L] heads tensor, a slice of an expanded view -- else a
    contiguous copy."""
    B = t.size(0)
    if (L > 1 and t.stride(1) != 1) or (B > 1 and t.stride(0) < L):
        t = t.contiguous()
    return t, (t.stride(0) if B > 1 else L)


def latent_accumulate(mu, log_var, state):
    """The rows of mu, log_var (fp32 [B, L] device tensors, detached here) added into ``state`` (ctvae_latent_accumulate): a dict
    of contiguous device tensors ``kl_sum``, ``mu_sum``, ``sig2_sum`` (float64 [L]), ``cov_sum`` (float64 [L, L]), ``nonfinite``
    (int32 [L]) and ``rows`` (int32 [1]).  One launch, no copy of a unit-stride input, no host synchronisation.  A CPU tensor is
    a RuntimeError (there is no CPU fallback); a wrong dtype or shape raises a ValueError that names it, before any launch."""
    what = "latent_accumulate"
    for name, t in (("mu", mu), ("log_var", log_var)):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2:
            raise ValueError(f"{what}: {name} must be a torch.float32 [B, L] tensor, got "
                             f"{getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))}")
    if mu.shape != log_var.shape:
        raise ValueError(f"{what}: mu {tuple(mu.shape)} and log_var {tuple(log_var.shape)} must have one shape")
    B, L = mu.shape
    if not 1 <= L <= LATENT_MAX_L:
        raise ValueError(f"{what}: latent_dim L={L} is not covered: the kernel needs 1 <= L <= {LATENT_MAX_L}")
    for name, dtype, rank in LATENT_STATE:
        t = state.get(name)
        _req_dense(what, name, t, dtype)
        if tuple(t.shape) != ((1,) if rank == 0 else (L,) * rank):
            raise ValueError(f"{what}: {name} must be {[1] if rank == 0 else [L] * rank} for L={L}, got {tuple(t.shape)}")
    _req_cuda(mu, log_var, *(state[name] for name, _, _ in LATENT_STATE))
    if B == 0:
        return
    m, pm = _latent_rows(mu.detach(), L)
    v, pv = _latent_rows(log_var.detach(), L)
    native.call("ctvae_latent_accumulate", m.data_ptr(), pm, v.data_ptr(), pv, B, L, *(state[name].data_ptr() for name, _, _ in LATENT_STATE))


# ---------------------------------------------------------------------------------------------------
# reconstruction quality per image (csrc/reconstat.hip; reconstats.ReconStats)
# ---------------------------------------------------------------------------------------------------
RECON_MIN_S, RECON_MAX_S = 11, 64        # what ctvae_recon_record covers: one 11-tap window at least, the LDS ring's width at most
RECON_MAX_K = 32                         # slots of the worst set
RECON_COLUMNS = ("mse", "mae", "max_err", "ssim")


def recon_consts(data_range: float):
    """The 13 doubles ``ctvae_recon_record`` reads on the host: the window of Wang et al. 2004, g[t] ~ exp(-(t-5)^2 / (2 * 1.5^2))
    normalised to sum 1, then C1 = (0.01 R)^2 and C2 = (0.03 R)^2.  Python floats: float64."""
    import ctypes
    import math
    R = float(data_range)
    if not (R > 0 and R < float("inf")):
        raise ValueError(f"recon_stats_range must be a finite number > 0, got {data_range!r}")
    g = [math.exp(-((t - 5) ** 2) / (2.0 * 1.5 ** 2)) for t in range(11)]
    total = math.fsum(g)
    return (ctypes.c_double * 13)(*[v / total for v in g], (0.01 * R) ** 2, (0.03 * R) ** 2)


def _recon_nhwc(what, name, x):
    """The NHWC memory under a logical [B, C, S, S] fp32 device tensor: its own when the channels-last view is contiguous, else
    a contiguous copy."""
    if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 4:
        raise ValueError(f"{what}: {name} must be a torch.float32 [B, C, S, S] tensor, got "
                         f"{getattr(x, 'dtype', type(x).__name__)} {tuple(getattr(x, 'shape', ()))}")
    v = x.detach().permute(0, 2, 3, 1)
    return v if v.is_contiguous() else v.contiguous()


def _recon_pair(what, recons, target):
    a, b = _recon_nhwc(what, "recons", recons), _recon_nhwc(what, "target", target)
    if a.shape != b.shape:
        raise ValueError(f"{what}: recons {tuple(recons.shape)} and target {tuple(target.shape)} must have one shape")
    B, S, S2, C = a.shape
    if S != S2 or not RECON_MIN_S <= S <= RECON_MAX_S or C < 1:
        raise ValueError(f"{what}: pictures [B, C, S, S] need {RECON_MIN_S} <= S <= {RECON_MAX_S} and C >= 1, got "
                         f"{tuple(recons.shape)}")
    return a, b, B, S, C


def _recon_rows(what, records, flags, row0, B):
    _req_dense(what, "records", records, torch.float64)
    _req_dense(what, "flags", flags, torch.int32)
    cap = flags.numel()
    if records.dim() != 2 or tuple(records.shape) != (cap, 4) or flags.dim() != 1:
        raise ValueError(f"{what}: records [capacity, 4] and flags [capacity] do not fit: {tuple(records.shape)}, {tuple(flags.shape)}")
    row0 = int(row0)
    if row0 < 0 or row0 + B > cap:
        raise ValueError(f"{what}: rows [{row0}, {row0 + B}) leave the capacity {cap}")
    return row0, cap


def recon_record(recons, target, consts, records, flags, row0):
    """``ctvae_recon_record``: the per-image mse, mae, max_err and ssim of the pairs (recons, target) -- logical [B, C, S, S] fp32
    device tensors, read as the NHWC memory underneath (a contiguous copy where it is not one) -- into rows [row0, row0 + B) of
    ``records`` (float64 [capacity, 4]) and ``flags`` (int32 [capacity]).  ``consts``: ``recon_consts(R)``.  One launch, no host
    synchronisation.  Returns the two NHWC tensors (``recon_worst`` reads the same memory)."""
    what = "recon_record"
    a, b, B, S, C = _recon_pair(what, recons, target)
    row0, cap = _recon_rows(what, records, flags, row0, B)
    _req_cuda(a, b, records, flags)
    if B:
        native.call("ctvae_recon_record", a.data_ptr(), b.data_ptr(), B, S, C, consts, records.data_ptr(), flags.data_ptr(), row0, cap)
    return a, b


def recon_worst_state(K, S, C, device):
    """One side of the worst set's ping-pong state, empty: ``ssim`` float64 [K], ``row`` int32 [K] (-1: empty), ``a`` / ``b`` fp32
    [K, S, S, C] (NHWC), ``source`` int32 [K]."""
    K = int(K)
    if not 1 <= K <= RECON_MAX_K:
        raise ValueError(f"recon_worst_state: 1 <= K <= {RECON_MAX_K}, got {K}")
    return {"ssim": torch.zeros(K, dtype=torch.float64, device=device), "row": torch.full((K,), -1, dtype=torch.int32, device=device),
            "a": torch.zeros(K, S, S, C, dtype=torch.float32, device=device), "b": torch.zeros(K, S, S, C, dtype=torch.float32, device=device),
            "source": torch.full((K,), -1, dtype=torch.int32, device=device)}


def recon_worst(old, new, records, flags, row0, a_nhwc, b_nhwc):
    """``ctvae_recon_worst`` behind ``recon_record`` of the same batch: the K worst of ``old``'s slots and the batch's rows into
    ``new`` (two ``recon_worst_state`` sides, never the same one).  a_nhwc, b_nhwc: what ``recon_record`` returned.  Two launches."""
    what = "recon_worst"
    if old is new or any(old[k].data_ptr() == new[k].data_ptr() for k in ("ssim", "row", "a", "b")):
        raise ValueError(f"{what}: old and new must be the two sides of the state, nothing is merged in place")
    K, S, _, C = old["a"].shape
    for side in (old, new):
        for k, dtype in (("ssim", torch.float64), ("row", torch.int32), ("a", torch.float32), ("b", torch.float32), ("source", torch.int32)):
            _req_dense(what, k, side[k], dtype)
        if tuple(side["a"].shape) != (K, S, S, C) or tuple(side["b"].shape) != (K, S, S, C) or side["ssim"].numel() != K \
                or side["row"].numel() != K or side["source"].numel() != K:
            raise ValueError(f"{what}: the two sides must be recon_worst_state(K, S, C) of one K, S, C")
    for name, t in (("a_nhwc", a_nhwc), ("b_nhwc", b_nhwc)):
        _req_dense(what, name, t, torch.float32)
        if t.dim() != 4 or tuple(t.shape[1:]) != (S, S, C) or t.size(0) != a_nhwc.size(0):
            raise ValueError(f"{what}: {name} must be [B, {S}, {S}, {C}] NHWC, got {tuple(t.shape)}")
    B = a_nhwc.size(0)
    row0, cap = _recon_rows(what, records, flags, row0, B)
    _req_cuda(a_nhwc, b_nhwc, records, flags, *old.values(), *new.values())
    native.call("ctvae_recon_worst", old["ssim"].data_ptr(), old["row"].data_ptr(), old["a"].data_ptr(), old["b"].data_ptr(),
                records.data_ptr(), flags.data_ptr(), row0, B, cap, a_nhwc.data_ptr(), b_nhwc.data_ptr(), S, C, K,
                new["ssim"].data_ptr(), new["row"].data_ptr(), new["a"].data_ptr(), new["b"].data_ptr(), new["source"].data_ptr())


# ---------------------------------------------------------------------------------------------------
# a Gaussian-mixture latent prior fitted by EM (csrc/gmm.hip; latentprior.GaussianMixturePrior)
# ---------------------------------------------------------------------------------------------------
GMM_MAX_D, GMM_MAX_K = 256, 64           # what the ctvae_gmm_* entry points cover


def _gmm_dims(what, X, K, name="X"):
    """(N, D) of a [N, D] fp32 tensor after the checks every ctvae_gmm_* wrapper shares."""
    if not torch.is_tensor(X) or X.dtype != torch.float32 or X.dim() != 2:
        raise ValueError(f"{what}: {name} must be a torch.float32 [N, D] tensor, got "
                         f"{getattr(X, 'dtype', type(X).__name__)} {tuple(getattr(X, 'shape', ()))}")
    if not X.is_contiguous():
        raise ValueError(f"{what}: {name} must be contiguous")
    N, D = X.shape
    if not 1 <= D <= GMM_MAX_D:
        raise ValueError(f"{what}: D={D} is not covered: the kernels need 1 <= D <= {GMM_MAX_D}")
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= GMM_MAX_K:
        raise ValueError(f"{what}: K={K!r} is not covered: the kernels need 1 <= K <= {GMM_MAX_K}")
    return N, D


def _gmm_param(what, name, t, shape, dtype=torch.float32):
    _req_dense(what, name, t, dtype)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} must be {list(shape)}, got {list(t.shape)}")


def gmm_estep(X, log_w, mu, P, log_det_half, full=True):
    """``ctvae_gmm_estep``: X fp32 [N, D] and the mixture as the host prepared it -- ``log_w`` [K], ``mu`` [K, D], ``P`` ([K, D, D]
    the inverse lower Cholesky factors for ``full``, [K, D] = 1 / sqrt(var) else), ``log_det_half`` [K], all fp32 on the device.
    Returns ``(r [N, K] fp32, ll [N] fp32, nonfinite [N] int32)``.  One launch, no host synchronisation.  A CPU tensor is a
    RuntimeError (there is no CPU fallback); a wrong dtype, shape, D or K raises a ValueError that names it, before any launch."""
    what = "gmm_estep"
    K = int(log_w.numel()) if torch.is_tensor(log_w) else 0
    N, D = _gmm_dims(what, X, K)
    _gmm_param(what, "log_w", log_w, (K,))
    _gmm_param(what, "mu", mu, (K, D))
    _gmm_param(what, "P", P, (K, D, D) if full else (K, D))
    _gmm_param(what, "log_det_half", log_det_half, (K,))
    _req_cuda(X, log_w, mu, P, log_det_half)
    r = torch.empty(N, K, dtype=torch.float32, device=X.device)
    ll = torch.empty(N, dtype=torch.float32, device=X.device)
    bad = torch.empty(N, dtype=torch.int32, device=X.device)
    if N:
        native.call("ctvae_gmm_estep", X.data_ptr(), N, D, K, 1 if full else 0, log_w.data_ptr(), mu.data_ptr(), P.data_ptr(),
                    log_det_half.data_ptr(), r.data_ptr(), ll.data_ptr(), bad.data_ptr())
    return r, ll, bad


def gmm_mstep_slabs(N, D, K, full=True) -> int:
    """The number of row slabs ``ctvae_gmm_mstep`` splits N rows into."""
    return int(native.load().ctvae_gmm_mstep_slabs(int(N), int(D), int(K), 1 if full else 0))


def gmm_mstep(X, r, nonfinite, means, full=True, ws=None):
    """``ctvae_gmm_mstep``: the float64 sums of one M step, centred at ``means`` (fp32 [K, D]): ``(Nk [K], S1 [K, D], S2)`` with S2
    [K, D, D] for ``full`` and [K, D] else, float64 device tensors.  ``r`` fp32 [N, K] and ``nonfinite`` int32 [N] (or None) are
    ``gmm_estep``'s.  ``ws``: a float64 device tensor to reuse as scratch (at least ``ctvae_gmm_mstep_workspace_bytes`` / 8
    elements; None: allocated here).  Three launches (two for diag), no host synchronisation.  N < K is a ValueError."""
    what = "gmm_mstep"
    K = int(means.size(0)) if torch.is_tensor(means) and means.dim() == 2 else 0
    N, D = _gmm_dims(what, X, K)
    _gmm_param(what, "means", means, (K, D))
    _gmm_param(what, "r", r, (N, K))
    if nonfinite is not None:
        _gmm_param(what, "nonfinite", nonfinite, (N,), torch.int32)
    if N < K:
        raise ValueError(f"{what}: {N} rows cannot carry K={K} components: the M step needs N >= K")
    _req_cuda(X, r, nonfinite, means)
    need = int(native.load().ctvae_gmm_mstep_workspace_bytes(N, D, K, 1 if full else 0))
    if ws is None:
        ws = torch.empty(need // 8, dtype=torch.float64, device=X.device)
    else:
        _req_dense(what, "ws", ws, torch.float64)
        _req_cuda(ws)
        if ws.numel() * 8 < need:
            raise ValueError(f"{what}: ws holds {ws.numel() * 8} bytes, {need} are needed")
    Nk = torch.empty(K, dtype=torch.float64, device=X.device)
    S1 = torch.empty(K, D, dtype=torch.float64, device=X.device)
    S2 = torch.empty((K, D, D) if full else (K, D), dtype=torch.float64, device=X.device)
    native.call("ctvae_gmm_mstep", X.data_ptr(), r.data_ptr(), native.ptr(nonfinite), N, D, K, 1 if full else 0, means.data_ptr(),
                Nk.data_ptr(), S1.data_ptr(), S2.data_ptr(), ws.data_ptr(), ws.numel() * 8)
    return Nk, S1, S2


def gmm_sample(u, eps, cdf, mu, L, full=True):
    """``ctvae_gmm_sample``: ``u`` fp32 [n] in [0, 1), ``eps`` fp32 [n, D], ``cdf`` float64 [K], ``mu`` fp32 [K, D], ``L`` fp32
    ([K, D, D] lower Cholesky factors for ``full``, [K, D] = sqrt(var) else).  Returns ``(z [n, D] fp32, k [n] int32)``: row i is
    ``mu_k + L_k eps[i]`` for the first k whose cdf exceeds u[i].  One launch; the kernel holds no random state."""
    what = "gmm_sample"
    K = int(cdf.numel()) if torch.is_tensor(cdf) else 0
    n, D = _gmm_dims(what, eps, K, name="eps")
    _gmm_param(what, "u", u, (n,))
    _gmm_param(what, "cdf", cdf, (K,), torch.float64)
    _gmm_param(what, "mu", mu, (K, D))
    _gmm_param(what, "L", L, (K, D, D) if full else (K, D))
    _req_cuda(u, eps, cdf, mu, L)
    z = torch.empty(n, D, dtype=torch.float32, device=eps.device)
    k = torch.empty(n, dtype=torch.int32, device=eps.device)
    if n:
        native.call("ctvae_gmm_sample", u.data_ptr(), eps.data_ptr(), n, D, K, 1 if full else 0, cdf.data_ptr(), mu.data_ptr(),
                    L.data_ptr(), z.data_ptr(), k.data_ptr())
    return z, k


# ---------------------------------------------------------------------------------------------------
# test log-likelihood by importance sampling (csrc/loglik.hip; loglik.ImportanceLogLik)
# ---------------------------------------------------------------------------------------------------
LOGLIK_STATE = ("m", "s", "s2", "t", "n")          # the columns of the merge state


def loglik_consts(sigma, P, device=None):
    """The two doubles ``ctvae_loglik_rows`` reads from device memory, computed on the host in float64: ``1 / (2 sigma^2)`` and
    ``(P / 2) log(2 pi sigma^2)`` of the observation model N(decode(z), sigma^2 I) over P elements."""
    import math
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float)) or not (sigma > 0 and sigma < float("inf")):
        raise ValueError(f"loglik_consts: sigma must be a finite number > 0, got {sigma!r}")
    if isinstance(P, bool) or not isinstance(P, int) or P < 1:
        raise ValueError(f"loglik_consts: P must be an integer of at least 1, got {P!r}")
    s2 = float(sigma) * float(sigma)
    if not (s2 > 0 and 1.0 / (2.0 * s2) < float("inf")):
        raise ValueError(f"loglik_consts: sigma^2 leaves float64 for sigma={sigma!r}")
    return torch.tensor([1.0 / (2.0 * s2), 0.5 * P * math.log(2.0 * math.pi * s2)], dtype=torch.float64,
                        device="cuda" if device is None else device)


def loglik_latent(mu, log_var, eps):
    """``ctvae_loglik_latent``: ``mu``, ``log_var`` fp32 [B, L] and ``eps`` fp32 [B, S, L], all contiguous.  Returns ``(z [B * S, L]
    fp32, a [B * S] float64)``: ``z = mu + expf(0.5f * log_var) * eps`` and ``a = log p(z) - log q(z|x)``, formed in float64 from
    the stored z.  One launch.  A CPU tensor is a RuntimeError; a wrong dtype or shape raises a ValueError that names it."""
    what = "loglik_latent"
    for name, t, rank in (("mu", mu, 2), ("log_var", log_var, 2), ("eps", eps, 3)):
        _req_dense(what, name, t, torch.float32)
        if t.dim() != rank:
            raise ValueError(f"{what}: {name} must be {'[B, L]' if rank == 2 else '[B, S, L]'}, got {tuple(t.shape)}")
    B, S, L = eps.shape
    if tuple(mu.shape) != (B, L) or tuple(log_var.shape) != (B, L) or S < 1 or L < 1:
        raise ValueError(f"{what}: mu {tuple(mu.shape)}, log_var {tuple(log_var.shape)} and eps {tuple(eps.shape)} must be [B, L], "
                         f"[B, L] and [B, S, L] with S >= 1 and L >= 1")
    _req_cuda(mu, log_var, eps)
    z = torch.empty(B * S, L, dtype=torch.float32, device=eps.device)
    a = torch.empty(B * S, dtype=torch.float64, device=eps.device)
    if B:
        native.call("ctvae_loglik_latent", mu.data_ptr(), log_var.data_ptr(), eps.data_ptr(), B, S, L, z.data_ptr(), a.data_ptr())
    return z, a


def loglik_memory_formats(t):
    """The dense memory formats a logical [N, C, H, W] tensor lies in: a subset of ("nchw", "nhwc") -- both for C == 1 or
    H * W == 1, none for anything strided."""
    return tuple(name for name, v in (("nchw", t), ("nhwc", t.permute(0, 2, 3, 1))) if v.is_contiguous())


def loglik_rows(xhat, x, S, a, consts):
    """``ctvae_loglik_rows``: ``xhat`` logical [B * S, C, H, W] fp32 (the decoded rows), ``x`` logical [B, C, H, W] fp32 (the
    images), read where they lie: both must be dense in the same memory format, NCHW-contiguous or channels-last (the decoder's
    NCHW view over NHWC memory); any other pairing is a ValueError, nothing is copied.  ``a`` float64 [B * S] (``loglik_latent``'s)
    or None for 0; ``consts``: ``loglik_consts(sigma, P)``.  Returns ``lw`` float64 [B * S].  One launch."""
    what = "loglik_rows"
    for name, t in (("xhat", xhat), ("x", x)):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 4:
            raise ValueError(f"{what}: {name} must be a torch.float32 [N, C, H, W] tensor, got "
                             f"{getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))}")
    if isinstance(S, bool) or not isinstance(S, int) or S < 1:
        raise ValueError(f"{what}: S must be an integer of at least 1, got {S!r}")
    B = x.size(0)
    if tuple(xhat.shape) != (B * S,) + tuple(x.shape[1:]) or x[0].numel() < 1:
        raise ValueError(f"{what}: xhat {tuple(xhat.shape)} must be [B * S, C, H, W] for x {tuple(x.shape)} and S={S}")
    xhat, x = xhat.detach(), x.detach()
    fh, fx = loglik_memory_formats(xhat), loglik_memory_formats(x)
    if not set(fh) & set(fx):
        say = lambda f: " / ".join({"nchw": "NCHW-contiguous", "nhwc": "channels-last"}[k] for k in f) or "not dense"
        raise ValueError(f"{what}: xhat is {say(fh)} and x is {say(fx)}: both must be dense in the same memory format "
                         f"(NCHW-contiguous or channels-last); nothing is copied here")
    R, P = B * S, x[0].numel()
    if a is not None:
        _req_dense(what, "a", a, torch.float64)
        if tuple(a.shape) != (R,):
            raise ValueError(f"{what}: a must be [{R}], got {list(a.shape)}")
    _req_dense(what, "consts", consts, torch.float64)
    if tuple(consts.shape) != (2,):
        raise ValueError(f"{what}: consts must be loglik_consts(sigma, P), two doubles, got {list(consts.shape)}")
    _req_cuda(xhat, x, a, consts)
    lw = torch.empty(R, dtype=torch.float64, device=xhat.device)
    if R:
        native.call("ctvae_loglik_rows", xhat.data_ptr(), x.data_ptr(), B, S, P, native.ptr(a), consts.data_ptr(), lw.data_ptr())
    return lw


def loglik_state(capacity, device):
    """An empty merge state: ``(state float64 [capacity, 5], flags int32 [capacity])``; the columns are ``LOGLIK_STATE`` -- m = -inf,
    the rest 0."""
    state = torch.zeros(int(capacity), len(LOGLIK_STATE), dtype=torch.float64, device=device)
    state[:, 0] = float("-inf")
    return state, torch.zeros(int(capacity), dtype=torch.int32, device=device)


def loglik_merge(lw, S, state, flags, row0):
    """``ctvae_loglik_merge``: the chunk's log-weights ``lw`` float64 [B * S] into rows [row0, row0 + B) of ``state`` (float64
    [capacity, 5]) and ``flags`` (int32 [capacity]), one at a time in sample order.  One launch, no host synchronisation."""
    what = "loglik_merge"
    _req_dense(what, "lw", lw, torch.float64)
    _req_dense(what, "state", state, torch.float64)
    _req_dense(what, "flags", flags, torch.int32)
    if isinstance(S, bool) or not isinstance(S, int) or S < 1:
        raise ValueError(f"{what}: S must be an integer of at least 1, got {S!r}")
    if lw.dim() != 1 or lw.numel() % S:
        raise ValueError(f"{what}: lw must be [B * S] for S={S}, got {list(lw.shape)}")
    cap = flags.numel()
    if flags.dim() != 1 or tuple(state.shape) != (cap, len(LOGLIK_STATE)):
        raise ValueError(f"{what}: state [capacity, {len(LOGLIK_STATE)}] and flags [capacity] do not fit: {tuple(state.shape)}, "
                         f"{tuple(flags.shape)}")
    B, row0 = lw.numel() // S, int(row0)
    if row0 < 0 or row0 + B > cap:
        raise ValueError(f"{what}: rows [{row0}, {row0 + B}) leave the capacity {cap}")
    _req_cuda(lw, state, flags)
    if B:
        native.call("ctvae_loglik_merge", lw.data_ptr(), B, S, state.data_ptr(), flags.data_ptr(), row0, cap)


# ---------------------------------------------------------------------------------------------------
# interpolated Markov code prior (csrc/codeprior.hip; codeprior.MarkovCodePrior)
# ---------------------------------------------------------------------------------------------------
CODE_PRIOR_EXPERTS = ("uniform", "position", "left", "up", "previous")
CODE_PRIOR_TABLES = ("pos", "left", "up", "prev")
CODE_PRIOR_MAX_K = 512
CODE_PRIOR_MAX_TOTAL = 1 << 53               # a row total must stay below: it is converted to float64 exactly


def code_prior_sample_max_history() -> int:
    """The W * C the sampler covers: the row of context codes it keeps in LDS."""
    return int(native.load().ctvae_code_prior_sample_max_history())


def _cp_tensor(what, name, t, dtype, shape=None):
    """A dense device tensor of ``dtype`` (and ``shape``), or a ValueError that names the argument."""
    if not torch.is_tensor(t) or t.dtype != dtype:
        raise ValueError(f"{what}: {name} must be a {dtype} tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} must be {list(shape)}, got {list(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be contiguous")
    if not t.is_cuda:
        raise ValueError(f"{what}: {name} must be a device tensor (there is no CPU fallback)")


def _cp_grid(what, name, inds):
    """(B, C, H, W) of an int64 index grid [B, C, H, W] with no empty extent."""
    _cp_tensor(what, name, inds, torch.int64)
    if inds.dim() != 4 or inds.numel() == 0:
        raise ValueError(f"{what}: {name} must be [B, C, H, W] with no empty extent, got {list(inds.shape)}")
    if inds.numel() >= 1 << 31:
        raise ValueError(f"{what}: {name} holds {inds.numel()} tokens, one launch covers fewer than 2^31")
    return tuple(inds.shape)


def code_prior_limits(what, K, C, H, W):
    for name, v in (("K", K), ("C", C), ("H", H), ("W", W)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{what}: {name} must be an integer, got {v!r}")
    if not 1 <= K <= CODE_PRIOR_MAX_K:
        raise ValueError(f"{what}: K must lie in 1..{CODE_PRIOR_MAX_K}, got {K}")
    for name, v in (("C", C), ("H", H), ("W", W)):
        if v < 1:
            raise ValueError(f"{what}: {name} must be at least 1, got {v}")


def _cp_tables(what, tables, C, H, W, device):
    """The checks of the four count tables ``(pos, left, up, prev)``; returns K."""
    if not isinstance(tables, (tuple, list)) or len(tables) != 4:
        raise ValueError(f"{what}: tables must be the four tensors (pos, left, up, prev)")
    pos = tables[0]
    if not torch.is_tensor(pos) or pos.dim() != 3:
        raise ValueError(f"{what}: pos must be [C, H*W, K], got {list(getattr(pos, 'shape', ()))}")
    K = int(pos.size(2))
    code_prior_limits(what, K, C, H, W)
    shapes = ((C, H * W, K),) + ((C, K + 1, K),) * 3
    for name, t, shape in zip(CODE_PRIOR_TABLES, tables, shapes):
        _cp_tensor(what, name, t, torch.int64, shape)
        if t.device != device:
            raise ValueError(f"{what}: {name} lies on {t.device}, not on {device}")
    return K


def _cp_totals(what, totals, C, H, W, K, device):
    if not isinstance(totals, (tuple, list)) or len(totals) != 4:
        raise ValueError(f"{what}: totals must be the four tensors (pos_tot, left_tot, up_tot, prev_tot)")
    shapes = ((C, H * W),) + ((C, K + 1),) * 3
    for name, t, shape in zip(CODE_PRIOR_TABLES, totals, shapes):
        _cp_tensor(what, name + "_tot", t, torch.int64, shape)
        if t.device != device:
            raise ValueError(f"{what}: {name}_tot lies on {t.device}, not on {device}")
    top = torch.stack([t.max() for t in totals])           # one read for the four tables
    low = torch.stack([t.min() for t in totals])
    top, low = top.tolist(), low.tolist()
    for name, hi, lo in zip(CODE_PRIOR_TABLES, top, low):
        if hi >= CODE_PRIOR_MAX_TOTAL or lo < 0:
            raise ValueError(f"{what}: {name}_tot must lie in [0, 2^53), got a row total of {hi if hi >= CODE_PRIOR_MAX_TOTAL else lo}")


def _cp_lambda(what, lam, C, device):
    _cp_tensor(what, "lambda", lam, torch.float64, (C, len(CODE_PRIOR_EXPERTS)))
    if lam.device != device:
        raise ValueError(f"{what}: lambda lies on {lam.device}, not on {device}")


def code_prior_tables(K, C, H, W, device):
    """Zeroed ``(pos [C, H*W, K], left, up, prev [C, K+1, K])`` int64 tables and the ``invalid`` word."""
    code_prior_limits("code_prior_tables", K, C, H, W)
    z = lambda *s: torch.zeros(*s, dtype=torch.int64, device=device)
    return (z(C, H * W, K), z(C, K + 1, K), z(C, K + 1, K), z(C, K + 1, K)), z(1)


def code_prior_totals(tables):
    """The row totals of the four tables: exact int64 sums."""
    return tuple(t.sum(dim=2) for t in tables)


def code_prior_count(inds, tables, invalid):
    """``ctvae_code_prior_count``: every token of ``inds`` (int64 [B, C, H, W], as ``vq_compute_inds`` returns it) is added to the
    four int64 tables ``(pos [C, H*W, K], left, up, prev [C, K+1, K])``; a token whose own code or a context code lies outside
    [0, K) adds 1 to ``invalid`` (one int64 word) instead.  A wrong dtype, shape, device or contiguity is a ValueError that names
    the argument, before any launch."""
    what = "code_prior_count"
    B, C, H, W = _cp_grid(what, "inds", inds)
    K = _cp_tables(what, tables, C, H, W, inds.device)
    _cp_tensor(what, "invalid", invalid, torch.int64)
    if invalid.numel() != 1 or invalid.device != inds.device:
        raise ValueError(f"{what}: invalid must be one int64 word on {inds.device}, got {list(invalid.shape)} on {invalid.device}")
    native.call("ctvae_code_prior_count", inds.data_ptr(), *(t.data_ptr() for t in tables), invalid.data_ptr(), B, C, H, W, K)


def code_prior_score(inds, tables, totals, lam):
    """``ctvae_code_prior_score``: ``(logp float64 [B, C], resp float64 [B, C, 5], bad int32 [B])`` of ``inds`` int64 [B, C, H, W]
    under the tables, their row ``totals`` (int64, below 2^53) and ``lam`` float64 [C, 5]."""
    what = "code_prior_score"
    B, C, H, W = _cp_grid(what, "inds", inds)
    K = _cp_tables(what, tables, C, H, W, inds.device)
    _cp_totals(what, totals, C, H, W, K, inds.device)
    _cp_lambda(what, lam, C, inds.device)
    J = len(CODE_PRIOR_EXPERTS)
    logp = torch.empty(B, C, dtype=torch.float64, device=inds.device)
    resp = torch.empty(B, C, J, dtype=torch.float64, device=inds.device)
    bad = torch.empty(B, dtype=torch.int32, device=inds.device)
    native.call("ctvae_code_prior_score", inds.data_ptr(), *(t.data_ptr() for t in tables), *(t.data_ptr() for t in totals),
                lam.data_ptr(), logp.data_ptr(), resp.data_ptr(), bad.data_ptr(), B, C, H, W, K)
    return logp, resp, bad


def code_prior_sample(tables, totals, lam, u, H, W):
    """``ctvae_code_prior_sample``: int64 ``inds`` [n, C, H, W] from ``u`` float64 [n, H*W, C, 2] in [0, 1)."""
    what = "code_prior_sample"
    _cp_tensor(what, "u", u, torch.float64)
    if u.dim() != 4 or u.size(3) != 2 or u.numel() == 0:
        raise ValueError(f"{what}: u must be [n, H*W, C, 2] with no empty extent, got {list(u.shape)}")
    n, HW, C = int(u.size(0)), int(u.size(1)), int(u.size(2))
    for name, v in (("H", H), ("W", W)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"{what}: {name} must be an integer of at least 1, got {v!r}")
    if H * W != HW:
        raise ValueError(f"{what}: u must be [n, H*W, C, 2] for H={H}, W={W}, got {list(u.shape)}")
    if u.numel() // 2 >= 1 << 31:
        raise ValueError(f"{what}: u asks for {u.numel() // 2} tokens, one launch covers fewer than 2^31")
    K = _cp_tables(what, tables, C, H, W, u.device)
    if W * C > code_prior_sample_max_history():
        raise ValueError(f"{what}: W * C = {W * C} is not covered: the sampler keeps a row of at most "
                         f"{code_prior_sample_max_history()} context codes")
    _cp_totals(what, totals, C, H, W, K, u.device)
    _cp_lambda(what, lam, C, u.device)
    if u.data_ptr() % 16:
        raise ValueError(f"{what}: u must start on a 16-byte boundary")
    inds = torch.empty(n, C, H, W, dtype=torch.int64, device=u.device)
    native.call("ctvae_code_prior_sample", *(t.data_ptr() for t in tables), *(t.data_ptr() for t in totals), lam.data_ptr(),
                u.data_ptr(), inds.data_ptr(), n, C, H, W, K)
    return inds


def code_prior_embed(inds, codebooks):
    """``ctvae_code_prior_embed``: fp32 NHWC [n, H, W, C * Dc] with code ``c`` in channels [c * Dc, (c + 1) * Dc), a copy of the rows
    of ``codebooks`` -- fp32 [C, K, Dc], or the list of C [K, Dc] weights stored back to back that
    ``MultipleCodebookVectorQuantizer._codebooks()`` checks."""
    what = "code_prior_embed"
    n, C, H, W = _cp_grid(what, "inds", inds)
    if isinstance(codebooks, (tuple, list)):
        if len(codebooks) != C:
            raise ValueError(f"{what}: codebooks holds {len(codebooks)} codebooks, inds has C={C}")
        for i, w in enumerate(codebooks):
            _cp_tensor(what, f"codebooks[{i}]", w, torch.float32, tuple(codebooks[0].shape))
            if w.dim() != 2 or w.data_ptr() != codebooks[0].data_ptr() + i * codebooks[0].numel() * 4:
                raise ValueError(f"{what}: codebooks[{i}] must be [K, Dc] and stored back to back with the others")
        K, Dc = codebooks[0].shape
        first = codebooks[0]
    else:
        _cp_tensor(what, "codebooks", codebooks, torch.float32)
        if codebooks.dim() != 3 or codebooks.size(0) != C or codebooks.numel() == 0:
            raise ValueError(f"{what}: codebooks must be [C={C}, K, Dc], got {list(codebooks.shape)}")
        _, K, Dc = codebooks.shape
        first = codebooks
    if first.device != inds.device:
        raise ValueError(f"{what}: codebooks lies on {first.device}, not on {inds.device}")
    out = torch.empty(n, H, W, C * Dc, dtype=torch.float32, device=inds.device)
    native.call("ctvae_code_prior_embed", inds.data_ptr(), first.data_ptr(), out.data_ptr(), n, C, H, W, int(K), int(Dc))
    return out
