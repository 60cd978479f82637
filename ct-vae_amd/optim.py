"""Flat fused Adam (+ ExponentialLR) over a model's packed parameter buffer.

Same update rule as ``torch.optim.Adam(lr, weight_decay)`` with default betas/eps, which is what the
reference's harness builds (experiment.py:158-160); the schedule is ``ExponentialLR(gamma)`` stepped once
per epoch (experiment.py:173-175).  One kernel launch per step for the whole model, hyper-parameters and the
step counter live in a small device tensor so the launch is hipGraph-capturable.

Parameters without a gradient (``absent_grad``, ``exp_params.adam_absent_grad``).  torch keeps a step counter per parameter
and does not touch a parameter whose ``.grad`` is None.  That matters only where a parameter receives NO gradient in some steps
-- in this repository CT-MCQ-VAE's per-action ``graph_discovers`` whose action is absent from a batch, ``ct_layer.mask`` in
base-mode steps, the decoder in causal-mode steps; VanillaVAE / MCQ-VAE, where every parameter gets a gradient every step,
step identically under all three values (tests/test_ct_gpu.py pins their 3-step trajectory):
* ``"zero"`` (the default): ONE step counter for the whole buffer, and every element is updated every step.  A parameter
  without a gradient sees a zero gradient: its first moment decays, it keeps drifting by its momentum, its bias correction
  follows the global count.  The plain ``ctvae_adam_step`` / ``ctvae_adam_step_clipped`` launches, no block table.
* ``"skip"``: a block without a gradient is not touched in that step -- parameter, both moments and its own step counter stay,
  no weight decay.  ``torch.optim.Adam`` with ``zero_grad(set_to_none=True)``, current torch's default and what the CPU oracle
  runs.
* ``"skip_until_first"``: a block is frozen until its first gradient, where its counter starts; from then on it steps every
  step, with a zero gradient when none arrived.  torch 1.12.1 under Lightning 1.6.5 (the reference's pinned stack), whose
  ``zero_grad()`` keeps zero tensors.
The two skip modes run ``ctvae_adam_step_blocks`` over a block table built once from the model's layout
(``FlatParamMixin.adam_blocks``, clipped to the slice): one block per kernel-managed storage block (active when a gradient
kernel wrote it since ``zero_grad``), per torch-level parameter (active when autograd produced its ``.grad``) and per member
of a module bank (active when the bank was used AND the forward marked the member on the device: scorer 0, and scorer 1 + i
iff some sample has action i); alignment gaps belong to no block and are never written.  What the host knows travels as a
device word per block, constant per captured step signature (checked at capture), the rest is decided on the device, so a
replayed hipGraph steps correctly.  Data-parallel training (``step(reduce_flags=...)``) follows torch DDP with
``find_unused_parameters=True``: the flags are formed from this rank's gradients alone, MAX-reduced across ranks, and only then
does "skip_until_first" add the blocks that have stepped before -- a block steps on EVERY rank, with the gradient's mean, iff
it got a gradient on at least one (a rank where it got none contributes its zeros), so the per-block state stays the same on
all ranks while they run different modes in one step.  ``ct_layer.a_dense`` never has a non-zero gradient
(its node has no outgoing edge) and never steps here; torch hands it an all-zero gradient and would apply weight decay to it.

Deviation from ``torch.optim.Adam`` in every mode (documented, not pinned by a fixture):
* beta1^t / beta2^t are accumulated in fp32 on the device (state[6..7], or per block); torch computes them in double on the
  host.  After 10^4 steps the relative difference of the bias corrections is < 1e-4 (beta2^t has decayed to 4.5e-5 by then).

Gradient clipping (Lightning's ``gradient_clip_val`` / ``gradient_clip_algorithm``, which the reference's YAMLs hand to the
Trainer): ``clip_val`` None or <= 0 is off, and the step is the plain Adam launch.  Otherwise the step clips the optimizer's
slice of the gradient after the DDP scale and before the weight decay, on the device and without a host sync:
``"norm"`` = ``torch.nn.utils.clip_grad_norm_(max_norm=clip_val)`` (one extra launch, the squared-norm pass; the pre-clip
norm is left in the device tensor ``grad_norm``), ``"value"`` = ``clip_grad_value_(clip_val)`` (folded into the Adam launch).
Non-finite norms behave as in torch: NaN makes every updated element NaN, inf clips everything to zero.

Gradient accumulation (Lightning's ``accumulate_grad_batches: k``, ``FlatAdam(accumulate=k)``; k = 1 allocates and launches
nothing).  ``zero_grad`` still runs before every micro-batch; the sum of a window's gradients lives in a buffer of its own, the
size of the optimizer's slice.  ``stash()`` takes a micro-batch that does not end its window into that buffer (one
``ctvae_grad_accumulate`` launch: "store" for the first, "add" after it), ``step()`` ends the window: a "finish" launch leaves
stashed sum + current gradients in the flat gradient buffer, and the exchange, the clip and the Adam kernels run on it as on a
single batch's -- so clipping and weight decay apply once per window, and ``grad_norm`` is the norm of the gradient that is
stepped.  The caller folds 1 / k into ``grad_scale`` next to 1 / world (also for an epoch's incomplete last window: Lightning
divides every loss by k).  In the skip modes a block is active in the window's step iff it was active in at least one
micro-batch, by host pattern and device hit words as in a single step: every stash forms its micro-batch's flags
(``adam_block_flags_local``, which consumes the hit words) and merges them into the window's (``ctvae_adam_flags_window``); the
step merges its own, reduces them across ranks if asked to, and only then does "skip_until_first" add the blocks that have
stepped before.  ``accumulation_schedule`` / ``with_window_ends`` say which batches of an epoch end a window.

Weight average (``exp_params.ema_decay``; ``WeightEMA`` beside ``FlatAdam``, ``ema_settings`` its validator): an exponential
moving average of the optimizer's slice of the flat parameter buffer in a buffer of its own, one ``ctvae_ema_update`` launch per
optimizer step and one ``ctvae_buffer_swap`` launch to exchange it with the live weights for evaluation (csrc/ema.hip).  The
reference keeps no such average: what it computes is defined here.  Without the key nothing is allocated or launched.

Codebook usage (``exp_params.codebook_stats`` / ``codebook_restart_every``; ``CodebookUsage`` beside ``WeightEMA``,
``codebook_settings`` its validator): how often every code of a quantising model is chosen, counted by ``ctvae_vq_usage`` from the
index tensors the quantiser computes anyway (csrc/vqusage.hip; integer atomics, exact), the statistics of a counts tensor
(``codebook_stats`` / ``codebook_record``: perplexity, usage, dead codes, float64 on the host), and dead-code restarts: the dead
list (``codebook_dead_list``), the draw of pool rows (``codebook_restart_rows``) and the ``ctvae_vq_restart`` launch that writes
the codes and zeroes their Adam moments.  The reference has neither: what they compute is defined here.  Without the keys nothing
is allocated or launched.

EMA codebooks (``exp_params.codebook_ema_decay`` / ``codebook_ema_eps``; ``CodebookEMA`` beside ``CodebookUsage``,
``codebook_ema_settings`` its validator): the codebooks of a quantising model as running means of the latents assigned to each
code (van den Oord et al. 2017, appendix A.1) instead of optimizer-trained weights -- window statistics by ``ctvae_vq_ema_stats``
per micro-batch, one ``ctvae_vq_ema_update`` launch behind every optimizer step (csrc/vqema.hip; no float atomics).  The reference
has no such update: what it computes is defined here.  Without the key nothing is allocated or launched.
"""
import contextlib
import math
import struct

import torch

from . import kernels as K


def clip_settings(clip_val, algorithm=None):
    """Validated ``(clip_val, algorithm)`` with Lightning 1.6.5's rules: the value is a number or None, and None or <= 0 means
    no clipping (returned as None); the algorithm is "norm" (the default) or "value", in any letter case."""
    algo = "norm" if algorithm is None else algorithm
    if not isinstance(algo, str) or algo.lower() not in K.CLIP_ALGORITHMS:
        raise ValueError(f"gradient_clip_algorithm {algorithm!r} is invalid: allowed are 'norm' and 'value'")
    if clip_val is None:
        return None, algo.lower()
    if isinstance(clip_val, bool) or not isinstance(clip_val, (int, float)) or math.isnan(clip_val):
        raise TypeError(f"gradient_clip_val must be a number, got {clip_val!r}")
    return (float(clip_val) if clip_val > 0 else None), algo.lower()


ACCUMULATE_KEY = "accumulate_grad_batches"


def accumulate_setting(value):
    """Validated ``accumulate_grad_batches``: an integer k >= 1, None meaning 1.  A bool, a float, a number below 1 or a dict
    (Lightning's per-epoch schedule, which is not supported) raises a ValueError that names the key."""
    if value is None:
        return 1
    if isinstance(value, dict):
        raise ValueError(f"{ACCUMULATE_KEY} {value!r} is invalid: a per-epoch schedule {{epoch: k}} is not supported, give one "
                         "integer >= 1")
    if isinstance(value, bool) or not isinstance(value, int) or value < 1:
        raise ValueError(f"{ACCUMULATE_KEY} {value!r} is invalid: it must be an integer >= 1")
    return int(value)


def with_window_ends(batches, k):
    """``(batch, ends_window)`` over one epoch's iterable of batches, by Lightning 1.6.5's rule: batch i (counted from 0 in every
    epoch) ends a window, i.e. is followed by the optimizer step, when (i + 1) % k == 0 or it is the epoch's last batch.  The
    loader's length need not be known: the generator looks one batch ahead."""
    it = iter(batches)
    try:
        cur = next(it)
    except StopIteration:
        return
    i = 0
    for nxt in it:
        yield cur, (i + 1) % k == 0
        cur, i = nxt, i + 1
    yield cur, True


def accumulation_schedule(n_batches, k):
    """``with_window_ends``' rule for an epoch of ``n_batches`` batches: one bool per batch, True where a window ends."""
    return [ends for _, ends in with_window_ends(range(n_batches), k)]


def absent_grad_setting(value):
    """Validated ``absent_grad`` (module docstring); None means the default, "zero"."""
    v = "zero" if value is None else value
    if not isinstance(v, str) or v not in K.ABSENT_GRAD_MODES:
        raise ValueError(f"adam_absent_grad {value!r} is invalid: allowed are 'zero', 'skip' and 'skip_until_first'")
    return v


class FlatAdam:
    def __init__(self, model, lr, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8, params_slice=None, clip_val=None,
                 clip_algorithm="norm", absent_grad="zero", accumulate=1):
        self.model = model
        self.accumulate = accumulate_setting(accumulate)
        self.acc = self.window_flags = None         # the window's gradient sum / block flags: exist only when accumulate > 1
        self.stashed = 0                            # micro-batches of the current window in `acc`
        self._merge_flags = False                   # finish_window() ran: the coming step merges the window's block flags
        flat = model.flat_params
        self.slice = params_slice if params_slice is not None else slice(0, flat.numel())
        n = flat[self.slice].numel()
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=flat.device)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=flat.device)
        self.state = K.adam_state([0.0, lr, betas[0], betas[1], eps, weight_decay, 1.0, 1.0], flat.device)
        self.lr = lr
        self.clip_val, self.clip_algorithm = clip_settings(clip_val, clip_algorithm)
        self.clip_ws = self.grad_norm = None        # grad_norm: pre-clip norm of the last step (norm mode), on the device
        if self.clip_val is not None and self.clip_algorithm == "norm":
            self.clip_ws = K.grad_clip_workspace(flat.device)
            self.grad_norm = torch.zeros((), dtype=torch.float32, device=flat.device)
        self.absent_grad = absent_grad_setting(absent_grad)
        self.blocks = self.table = self.host_pattern = None
        if self.absent_grad != "zero":
            self._build_block_table(n, flat.device)
        if self.accumulate > 1:
            self.acc = K.grad_accumulator_like(model._flat_grads[self.slice])    # (flat_params above built both buffers)
            if self.table is not None:
                self.window_flags = torch.zeros_like(self.table.active)

    # -- block table (absent_grad "skip" / "skip_until_first") ---------------------------------------------
    def _build_block_table(self, n, device):
        """self.blocks: [(lo, hi, kind, ref, member)] of model.adam_blocks() clipped to the slice, offsets relative to it;
        self.table: its device side.  Every bank module gets its words of the hit vector (``member_hits``)."""
        start = int(self.slice.start or 0)
        blocks = []
        for lo, hi, kind, ref, member in self.model.adam_blocks():
            lo, hi = max(lo - start, 0), min(hi - start, n)
            if lo < hi:
                blocks.append((lo, hi, kind, ref, member))
        blocks.sort(key=lambda b: b[0])
        banks, base, hit_index = {}, 0, []
        for _, _, kind, ref, member in blocks:
            if kind == "bank":
                banks.setdefault(id(ref[0]), [ref[0], 0])
                banks[id(ref[0])][1] = max(banks[id(ref[0])][1], member + 1)
        for ent in banks.values():
            ent.append(base)
            base += ent[1]
        for _, _, kind, ref, member in blocks:
            hit_index.append(banks[id(ref[0])][2] + member if kind == "bank" else -1)
        self.blocks = blocks
        self.table = K.AdamBlockTable([(b[0], b[1]) for b in blocks], hit_index, n, base, device)
        self._patterns = {}
        if self.table.hits.is_cuda:          # (on the CPU the table can be built and inspected; the step itself is a HIP kernel)
            for mod, count, off in banks.values():
                mod.member_hits = self.table.hits[off:off + count]

    def _host_pattern(self):
        """What the host knows of this step's gradients, one 0 / 1 per block (a bank member: whether its bank was used)."""
        out = []
        for _, _, kind, ref, _ in self.blocks:
            if kind == "kernel":
                out.append(int(ref.written))
            elif kind == "torch":
                out.append(int(self.model.torch_grad_present(ref)))
            elif kind == "bank":
                out.append(int(self.model.torch_grad_present(ref[1])))
            else:                            # a caller's own record: ref() -> bool
                out.append(int(bool(ref())))
        return tuple(out)

    def current_pattern(self):
        """The host-known activity ``step()`` would use now (skip modes), for a caller that hands it back later as ``pattern``."""
        self.model.gather_torch_grads()
        return self._host_pattern()

    def block_steps(self):
        """Per-block step counts (device, float), in the order of ``blocks``."""
        return self.table.state[:, 0]

    def set_lr(self, lr):
        self.lr = lr
        self.state[1:2].fill_(lr)

    def _present(self, pattern, device):
        """The device words of the host-known activity ``pattern`` (None: the model's current one); sets ``host_pattern``."""
        pat = self._host_pattern() if pattern is None else tuple(pattern)
        present = self._patterns.get(pat)
        if present is None:
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FlatAdam: the step being captured has gradients for other blocks than every eager step "
                                   "before it; a captured step's host-known activity must be constant")
            present = self._patterns[pat] = torch.tensor(pat, dtype=torch.int32, device=device)
        self.host_pattern = pat
        return present

    def stash(self, pattern=None):
        """Gradient accumulation (``accumulate`` > 1): add the current micro-batch's gradients to the window's sum instead of
        stepping.  One ``grad_accumulate`` launch over the slice ("store" for a window's first micro-batch, "add" after it); in
        the skip modes also this micro-batch's block flags (``adam_block_flags_local``, which consumes the hit words) and their
        merge into the window's (``adam_flags_window``).  The micro-batch that ends the window is not stashed: ``step()`` adds
        the sum to it.  pattern: as in ``step``."""
        if self.acc is None:
            raise RuntimeError("FlatAdam.stash: this optimizer was built without gradient accumulation (accumulate=1)")
        self.model.gather_torch_grads()
        mode = "store" if self.stashed == 0 else "add"
        K.grad_accumulate(self.acc, self.model.flat_grads[self.slice], mode)
        if self.absent_grad != "zero":
            K.adam_block_flags_local(self.table, self._present(pattern, self.acc.device))
            K.adam_flags_window(self.window_flags, self.table, mode)
        self.stashed += 1

    def finish_window(self):
        """The "finish" ``grad_accumulate`` launch of a window with stashed micro-batches: stashed sum + current gradients, left
        in the flat gradient buffer.  ``step()`` runs it itself; a caller that exchanges the gradients in front of the step
        (data-parallel training without block flags) calls it before the exchange.  Nothing without a stash."""
        self.model.gather_torch_grads()
        if self.stashed:
            K.grad_accumulate(self.acc, self.model.flat_grads[self.slice], "finish")
            self.stashed, self._merge_flags = 0, True

    def step(self, grad_scale=1.0, reduce_flags=None, pattern=None):
        """reduce_flags (skip modes only; data-parallel training): a callable that MAX-reduces the int32 [nb] flags tensor it
        is handed across ranks, in place and ordered on the current stream.  The step then runs local flags -> reduce_flags ->
        finish -> update, so that a block steps on every rank iff it got a gradient on at least one.  pattern: the host-known
        activity to use instead of the model's current one (a replayed captured step: the host still holds whatever the last
        step that ran Python left).

        After ``stash()`` calls the step ends their window: the "finish" ``grad_accumulate`` launch first leaves stashed sum +
        current gradients in the flat gradient buffer, where the exchange (``reduce_flags`` is called behind it), the clip pass
        and the Adam kernels find it as they find a single batch's; in the skip modes the flags run local -> window merge ->
        [reduce_flags] -> finish, so a block steps iff some micro-batch of the window had a gradient for it.  The caller folds
        the window's 1 / k into ``grad_scale``.  Without a stash the step issues no accumulation launch."""
        self.finish_window()
        p, g = self.model.flat_params[self.slice], self.model.flat_grads[self.slice]
        window, self._merge_flags = self._merge_flags, False
        if self.absent_grad != "zero":
            present = self._present(pattern, p.device)
            split = window or reduce_flags is not None
            if split:
                K.adam_block_flags_local(self.table, present)
                if window:
                    K.adam_flags_window(self.window_flags, self.table, "finish")
                if reduce_flags is not None:
                    reduce_flags(self.table.active)
                K.adam_block_flags_finish(self.table, self.absent_grad)
            K.adam_step_blocks(p, g, self.exp_avg, self.exp_avg_sq, self.state, self.table, present, self.absent_grad, grad_scale,
                               None if self.clip_val is None else self.clip_algorithm, self.clip_val, self.clip_ws, self.grad_norm,
                               flags_final=split)
        elif self.clip_val is None:
            K.adam_step(p, g, self.exp_avg, self.exp_avg_sq, self.state, grad_scale)
        else:
            K.adam_step_clipped(p, g, self.exp_avg, self.exp_avg_sq, self.state, grad_scale, self.clip_algorithm, self.clip_val,
                                self.clip_ws, self.grad_norm)

    def zero_grad(self, set_to_none=False):
        self.model.zero_grad()

    def state_dict(self):
        sd = {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "state": self.state}
        if self.absent_grad != "zero":       # (the default's state layout is what it was)
            sd["absent_grad"] = self.absent_grad
            sd["block_state"] = self.table.state      # [nb, 4]: step, beta1^step, beta2^step, seen
        return sd

    def load_state_dict(self, sd):
        theirs = sd.get("absent_grad", "zero")
        if theirs != self.absent_grad:
            raise RuntimeError(f"optimizer state was written under adam_absent_grad={theirs!r}, this run uses "
                               f"{self.absent_grad!r}: the step counters of the two do not translate")
        if self.absent_grad != "zero":
            if tuple(sd["block_state"].shape) != tuple(self.table.state.shape):
                raise RuntimeError("optimizer state has another block table than this model")
            self.table.state.copy_(sd["block_state"])
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.state[:8].copy_(sd["state"][:8])      # (states saved before the ticket word existed have 8 entries)


EMA_DECAY_KEY, EMA_WARMUP_KEY, EMA_EVAL_KEY = "ema_decay", "ema_warmup", "ema_eval"


def _fp32(x: float) -> float:
    """x rounded to the nearest fp32 value (what a ``float`` kernel argument receives)."""
    return struct.unpack("f", struct.pack("f", x))[0]


def ema_settings(decay, warmup=None, eval=None):
    """Validated ``(ema_decay, ema_warmup, ema_eval)``.  ``decay`` None means off: (None, False, False), and then neither of the
    other two may be set.  Otherwise ``decay`` is a float with 0 < d < 1 whose 1 - d is still below 1 in fp32 (the kernel's
    argument); ``warmup`` (None: False) and ``eval`` (None: True) are real bools.  Anything else -- a bool, a string or an int as
    the decay, a value outside the range, a number where a bool belongs -- raises a ValueError that names the key."""
    for key, v in ((EMA_WARMUP_KEY, warmup), (EMA_EVAL_KEY, eval)):
        if v is not None and not isinstance(v, bool):
            raise ValueError(f"{key} {v!r} is invalid: it must be true or false")
        if v is not None and decay is None:
            raise ValueError(f"{key} is set without {EMA_DECAY_KEY}: there is no weight average to apply it to")
    if decay is None:
        return None, False, False
    if isinstance(decay, bool) or not isinstance(decay, float) or not 0.0 < decay < 1.0 or not 0.0 < _fp32(1.0 - decay) < 1.0:
        raise ValueError(f"{EMA_DECAY_KEY} {decay!r} is invalid: it must be a float with 0 < {EMA_DECAY_KEY} < 1")
    return float(decay), bool(warmup), True if eval is None else eval


def ema_decay_at(decay: float, warmup: bool, t: int) -> float:
    """The decay of update ``t`` (counted from 1): ``decay``, or with warm-up min(decay, (1 + t) / (10 + t)) -- 2/11 at the
    first update, so that a young average follows the weights instead of its starting point."""
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


class WeightEMA:
    """An exponential moving average of the weights an optimizer steps (``exp_params.ema_decay``), kept by HIP kernels of its
    own on the flat buffer (csrc/ema.hip): ``update()`` is one ``ctvae_ema_update`` launch, ema += (1 - decay) * (p - ema), and
    ``swap()`` one ``ctvae_buffer_swap`` launch that exchanges the average with the live weights -- captured steps hold the flat
    buffer's addresses, so evaluating with the average means exchanging contents, not pointers.

    What is averaged.  The optimizer's whole slice of ``model.flat_params``, element by element, in the buffer's own packed
    order: alignment gaps and bank padding (constant zeros) are averaged along with the rest, which is harmless and keeps the
    kernel free of tables.  Under ``adam_absent_grad`` "skip" / "skip_until_first" a block that did not step is still averaged:
    its parameter did not move, so its average keeps approaching it (and stays on it once it is there: the kernel's arithmetic
    form leaves ema == p exactly p).  BatchNorm running statistics are buffers, not parameters, and are not averaged.

    The buffer sits at the slice's offset from a 16-byte boundary (``K.grad_accumulator_like``), so both kernels run their 16-byte
    loop, and starts as a copy of the slice.  ``updates`` counts the launches on the host; the decay of update t is
    ``decay_at(t)``, and 1 - decay is formed in double precision and rounded to fp32 once, as the launch's by-value argument."""

    def __init__(self, optimizer, decay, warmup=False):
        self.decay, self.warmup, _ = ema_settings(decay, bool(warmup), None)
        if self.decay is None:
            raise ValueError(f"{EMA_DECAY_KEY} is None: no weight average is wanted, build no WeightEMA")
        self.opt = optimizer
        live = self.live
        self.buffer = K.grad_accumulator_like(live)
        self.buffer.copy_(live)
        self.updates = 0
        self.swapped = False           # the average is in the flat buffer right now (between swap() and swap())

    @property
    def live(self):
        """The optimizer's slice of the model's flat parameter buffer."""
        return self.opt.model.flat_params[self.opt.slice]

    def decay_at(self, t: int) -> float:
        return ema_decay_at(self.decay, self.warmup, t)

    def update(self):
        if self.swapped:
            raise RuntimeError("WeightEMA.update: the average is swapped in; the flat buffer does not hold the live weights")
        K.ema_update(self.buffer, self.live, _fp32(1.0 - self.decay_at(self.updates + 1)))
        self.updates += 1

    def swap(self):
        """Exchange the average with the live slice.  The parameter epoch moves: cached Winograd filters and whatever else is
        keyed on it were made from the other values."""
        K.buffer_swap(self.buffer, self.live)
        self.swapped = not self.swapped
        K.bump_param_epoch()

    @contextlib.contextmanager
    def swapped_in(self):
        """The model computes with the averaged weights inside; the live ones come back on exit, also when the body raises."""
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    def state_dict(self, buffer=True):
        """buffer=False: the checkpoint's ``"ema"`` entry, plain numbers only -- the buffer travels as weights there."""
        sd = {"decay": self.decay, "warmup": self.warmup, "updates": int(self.updates)}
        return {**sd, "buffer": self.buffer} if buffer else sd

    def load_state_dict(self, sd):
        if float(sd["decay"]) != self.decay or bool(sd["warmup"]) != self.warmup:
            raise RuntimeError(f"weight average was kept under {EMA_DECAY_KEY}={sd['decay']!r}, {EMA_WARMUP_KEY}={sd['warmup']!r}, "
                               f"this run uses {self.decay!r}, {self.warmup!r}")
        if "buffer" in sd:
            if sd["buffer"].numel() != self.buffer.numel():
                raise RuntimeError("weight average covers another parameter range than this optimizer's slice")
            self.buffer.copy_(sd["buffer"])
        self.updates = int(sd["updates"])


CODEBOOK_STATS_KEY, CODEBOOK_EVERY_KEY = "codebook_stats", "codebook_restart_every"
CODEBOOK_MIN_KEY, CODEBOOK_POOL_KEY = "codebook_restart_min_count", "codebook_restart_pool"
CODEBOOK_POOL_DEFAULT = 1024


def codebook_settings(stats=None, every=None, min_count=None, pool=None):
    """Validated ``(codebook_stats, codebook_restart_every, codebook_restart_min_count, codebook_restart_pool)``.  ``stats``: a
    real bool (None: False).  ``every``: an integer >= 1, None meaning no restarts -- returned as (stats, None, None, None), and
    then neither of the other two may be set.  ``min_count`` (None: 1) and ``pool`` (None: 1024): integers >= 1.  Anything else
    -- a bool, a float or a string where an integer belongs, a number below 1 -- raises a ValueError that names the key."""
    if stats is not None and not isinstance(stats, bool):
        raise ValueError(f"{CODEBOOK_STATS_KEY} {stats!r} is invalid: it must be true or false")

    def integer(key, v):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"{key} {v!r} is invalid: it must be an integer >= 1")
        return int(v)

    if every is None:
        for key, v in ((CODEBOOK_MIN_KEY, min_count), (CODEBOOK_POOL_KEY, pool)):
            if v is not None:
                raise ValueError(f"{key} is set without {CODEBOOK_EVERY_KEY}: there are no restarts to apply it to")
        return bool(stats), None, None, None
    return (bool(stats), integer(CODEBOOK_EVERY_KEY, every), integer(CODEBOOK_MIN_KEY, 1 if min_count is None else min_count),
            integer(CODEBOOK_POOL_KEY, CODEBOOK_POOL_DEFAULT if pool is None else pool))


def codebook_stats(counts):
    """Per-codebook usage statistics of an integer counts tensor [C, K], in float64 on the host: a list of C dicts with
    ``perplexity`` = exp(-sum p ln p) over p = counts / total (the terms with p = 0 left out), ``usage`` = the fraction of
    codes with count > 0, ``dead`` = the number of codes with count 0 and ``total``.  A codebook that was never asked (total 0)
    reports perplexity None and usage 0.0: nothing in the result is NaN."""
    c = torch.as_tensor(counts).detach().cpu().to(torch.float64)
    out = []
    for row in c:
        total = float(row.sum())
        used = row[row > 0]
        perplexity = None
        if total > 0:
            p = used / total
            perplexity = float(torch.exp(-(p * torch.log(p)).sum()))
        out.append({"perplexity": perplexity, "usage": float(used.numel()) / row.numel(), "dead": int(row.numel() - used.numel()),
                    "total": int(total)})
    return out


def codebook_record(counts, prefix):
    """``codebook_stats`` as log entries: ``<prefix>codebook_perplexity_<i>`` / ``_usage_<i>`` / ``_dead_<i>`` per codebook i and
    the unsuffixed means over codebooks (the perplexity's over the codebooks that have one; None when none has)."""
    st = codebook_stats(counts)
    rec = {}
    for i, s in enumerate(st):
        for k in ("perplexity", "usage", "dead"):
            rec[f"{prefix}codebook_{k}_{i}"] = s[k]
    known = [s["perplexity"] for s in st if s["perplexity"] is not None]
    rec[f"{prefix}codebook_perplexity"] = sum(known) / len(known) if known else None
    rec[f"{prefix}codebook_usage"] = sum(s["usage"] for s in st) / len(st)
    rec[f"{prefix}codebook_dead"] = sum(s["dead"] for s in st) / len(st)
    return rec


def codebook_dead_list(counts, min_count=1):
    """The dead codes of a window: every (c, k) with counts[c][k] < min_count, in (c, k) order."""
    c = torch.as_tensor(counts).detach().cpu()
    return [(int(i), int(j)) for i, j in (c < int(min_count)).nonzero().tolist()]


def codebook_restart_seed(manual_seed, ordinal) -> int:
    """Seed of restart number ``ordinal`` (counted from 0) of a run seeded with ``manual_seed``."""
    return (int(manual_seed or 0) * 1_000_003 + int(ordinal)) * 2 + 1          # (odd: never a seed of sample_images / the metrics)


def codebook_restart_rows(manual_seed, ordinal, n_dead, valid_rows):
    """The pool row of each of ``n_dead`` dead codes, in list order: ONE ``randperm`` over the ``valid_rows`` valid pool rows
    from a CPU generator of its own seeded with ``codebook_restart_seed``, consumed in order and wrapping around when there are
    more dead codes than rows.  No global or device generator moves."""
    if n_dead == 0:
        return []
    if valid_rows < 1:
        raise ValueError("codebook restart: the pool holds no latent rows yet")
    gen = torch.Generator(device="cpu")
    gen.manual_seed(codebook_restart_seed(manual_seed, ordinal))
    perm = torch.randperm(int(valid_rows), generator=gen).tolist()
    return [perm[i % valid_rows] for i in range(n_dead)]


def quantizer_codebooks(vq_layer):
    """(the quantiser's codebooks as ONE fp32 [C, K, Dc] view of their storage, D) for the two quantiser classes of
    models/mcq_vae.py: C codebooks stored back to back (``_codebooks()`` checks it), or the single embedding; D is the width of
    the latents the quantiser reads."""
    if hasattr(vq_layer, "quantizers"):
        ws = vq_layer._codebooks()
        C, (Kc, Dc) = len(ws), ws[0].shape
        return ws[0].detach().as_strided((C, Kc, Dc), (Kc * Dc, Dc, 1)), C * Dc
    w = vq_layer.embedding.weight
    if not w.is_contiguous():
        raise RuntimeError("the codebook is not stored row by row")
    return w.detach().unsqueeze(0), w.size(1)


def codebook_offset(vq_layer, optimizer):
    """Offset of a quantiser's codebooks inside the optimizer's slice of the flat parameter buffer; None when they lie outside."""
    cb, _ = quantizer_codebooks(vq_layer)
    flat = optimizer.model.flat_params
    lo = (cb.data_ptr() - flat.data_ptr()) // 4 - int(optimizer.slice.start or 0)
    n = flat[optimizer.slice].numel()
    return lo if 0 <= lo and lo + cb.numel() <= n else None


class CodebookUsage:
    """How often every code of a model's quantiser is chosen (``exp_params.codebook_stats`` / ``codebook_restart_every``), counted
    by HIP kernels of its own (csrc/vqusage.hip) from the index tensors the quantiser computes anyway.

    ``observe`` is what the experiment sets as the quantiser's ``usage_observer``: one launch per index search --
    ``ctvae_vq_usage`` (``counts += histogram``; exact integers) or, with a pool, ``ctvae_vq_usage_pool_fill``, which also keeps
    the first min(P, R) latent rows of the search as restart candidates.  It takes pointers and shapes only, so inside a captured
    training step it replays correctly; every buffer is allocated here, outside any capture.  ``counts`` and the ``invalid`` word (indices outside
    [0, K): none, unless the latents hold NaN) are one int64 buffer, so ``read()`` is one device-to-host copy.

    ``valid_rows``: how many pool rows hold latents of the LAST search, known on the host from shapes alone -- the smallest
    min(P, R) of all searches so far (every fill overwrites at least that many rows).  A replayed step runs no Python, but every
    signature has run eagerly before its capture, so the value is the same in captured and eager runs.

    ``restart`` (with a pool): the dead codes of a window, counts < min_count in (c, k) order, get pool rows drawn by
    ``codebook_restart_rows`` and are overwritten by ``ctvae_vq_restart``, E_c[k] = pool[row][c : c + Dc), with both Adam
    moments of those elements zeroed.  ``reduce`` / ``broadcast`` (data-parallel runs): one SUM all-reduce of the counts, so a
    code used on any rank is alive, and one broadcast of rank 0's gathered rows, so every rank writes the same values."""

    def __init__(self, vq_layer, pool_rows=None):
        self.vq = vq_layer
        cb, self.D = quantizer_codebooks(vq_layer)
        self.C, self.K, self.Dc = cb.shape
        if not K.vq_usage_supported(self.K, self.C):
            raise ValueError(f"codebook usage: num_embeddings {self.K} with {self.C} codebooks is not covered by the usage kernel "
                             f"(K <= {K.VQ_USAGE_MAX_K}, C * K <= {K.VQ_USAGE_MAX_WORDS})")
        self.words = torch.zeros(self.C * self.K + 1, dtype=torch.int64, device=cb.device)
        self.counts, self.invalid = self.words[:-1].view(self.C, self.K), self.words[-1:]
        self.pool = torch.zeros((int(pool_rows), self.D), dtype=torch.float32, device=cb.device) if pool_rows else None
        self.valid_rows = None          # no search has filled the pool yet

    def observe(self, inds, latents_nhwc):
        if self.pool is None:
            K.vq_usage(inds, self.counts, self.invalid)
            return
        lat = latents_nhwc.detach()
        rows = K.vq_usage_pool_fill(inds, self.counts, self.invalid, lat if lat.is_contiguous() else lat.contiguous(), self.pool)
        self.valid_rows = rows if self.valid_rows is None else min(self.valid_rows, rows)

    def read(self):
        """(counts [C, K], invalid) on the host: one copy."""
        w = self.words.cpu()
        return w[:-1].view(self.C, self.K), int(w[-1])

    def zero(self):
        self.words.zero_()

    def restart(self, optimizer, min_count, manual_seed, ordinal, reduce=None, broadcast=None):
        """One restart behind an optimizer step (class docstring); returns (host counts of the window, dead list, rows).  The
        counts are zeroed and the parameter epoch moves."""
        if reduce is not None:
            reduce(self.words)
        counts, _ = self.read()
        dead = codebook_dead_list(counts, min_count)
        rows = codebook_restart_rows(manual_seed, ordinal, len(dead), self.valid_rows or 0)
        if dead:
            entries = [(c, k, r) for (c, k), r in zip(dead, rows)]
            cb, m, v = self.codebook_views(optimizer)
            if broadcast is None:
                K.vq_restart(entries, self.pool, self.valid_rows, cb, m, v)
            else:
                gathered = K.vq_restart_gather(entries, self.pool, self.valid_rows, self.C, self.Dc)
                broadcast(gathered)
                K.vq_restart(entries, None, 0, cb, m, v, rows=gathered)
        K.bump_param_epoch()
        self.zero()
        return counts, dead, rows

    def codebook_offset(self, optimizer):
        return codebook_offset(self.vq, optimizer)

    def codebook_views(self, optimizer):
        """The codebooks and the two Adam moments of the same elements as [C, K, Dc] views."""
        cb, _ = quantizer_codebooks(self.vq)
        lo = self.codebook_offset(optimizer)
        if lo is None:
            raise RuntimeError("the codebooks lie outside the optimizer's slice")
        return cb, optimizer.exp_avg[lo:lo + cb.numel()].view(cb.shape), optimizer.exp_avg_sq[lo:lo + cb.numel()].view(cb.shape)


CODEBOOK_EMA_DECAY_KEY, CODEBOOK_EMA_EPS_KEY = "codebook_ema_decay", "codebook_ema_eps"
CODEBOOK_EMA_EPS_DEFAULT = 1e-5


def codebook_ema_settings(decay, eps=None):
    """Validated ``(codebook_ema_decay, codebook_ema_eps)``, both rounded to fp32 once (what the update launch receives).
    ``decay`` None means off: (None, None), and then ``eps`` may not be set.  Otherwise ``decay`` is a float with 0 < d < 1 that is
    still inside (0, 1) in fp32, and ``eps`` (None: 1e-5) a finite float > 0 that is still > 0 in fp32.  Anything else -- a bool,
    an int or a string, a value outside the range -- raises a ValueError that names the key."""
    if decay is None:
        if eps is not None:
            raise ValueError(f"{CODEBOOK_EMA_EPS_KEY} is set without {CODEBOOK_EMA_DECAY_KEY}: there is no codebook average to "
                             "apply it to")
        return None, None
    if isinstance(decay, bool) or not isinstance(decay, float) or not 0.0 < decay < 1.0 or not 0.0 < _fp32(decay) < 1.0:
        raise ValueError(f"{CODEBOOK_EMA_DECAY_KEY} {decay!r} is invalid: it must be a float with 0 < {CODEBOOK_EMA_DECAY_KEY} < 1")
    if eps is None:
        eps = CODEBOOK_EMA_EPS_DEFAULT
    if isinstance(eps, bool) or not isinstance(eps, float) or not 0.0 < eps < 3.0e38 or not _fp32(eps) > 0.0:
        raise ValueError(f"{CODEBOOK_EMA_EPS_KEY} {eps!r} is invalid: it must be a float > 0")
    return _fp32(decay), _fp32(eps)


def codebook_ema_serves(model) -> bool:
    """Whether ``model`` is one of the quantising models the EMA codebook update is defined for (MCQVAE, VQVAE, CTMCQVAE: a
    ``vq_layer`` quantiser with an ``ema`` switch)."""
    vq = getattr(model, "vq_layer", None)
    return vq is not None and hasattr(vq, "ema_observer") and hasattr(vq, "ema")


class CodebookEMA:
    """Exponential-moving-average codebooks (``exp_params.codebook_ema_decay``; van den Oord et al. 2017, appendix A.1), kept by
    HIP kernels of their own (csrc/vqema.hip).  The reference has no such update: what it computes is defined here.

    State per codebook c and code k, fp32 and hidden (not part of ``state_dict`` of the model): ``N[c][k]``, starting at 1, and
    ``M[c][k][:]``, starting at E_c[k] -- "one observation at the current value".  Window accumulators: ``acc_n`` (int64) and
    ``acc_s`` (fp32), plus an ``invalid`` word (indices outside [0, K)); acc_n and invalid are one int64 buffer and acc_s one fp32
    buffer; a data-parallel update hands the counts and the sums to ``reduce`` at once (``ddp.all_reduce_codebook_ema``: one
    collective).

    ``observe`` is what the experiment sets as the quantiser's ``ema_observer``: one ``ctvae_vq_ema_stats`` call per index search
    of a training micro-batch, acc += the batch's counts and sums (source channel c + d, the slice quirk).  Pointers and shapes
    only, so it replays inside a captured step; every buffer is allocated here, outside any capture.

    ``update`` runs eagerly behind an optimizer step: [``reduce(ints, floats)``: SUM over ranks,] then ONE launch,
    N <- g N + (1-g) acc_n, M <- g M + (1-g) acc_s, n = sum_k N_k, Nt_k = (N_k + eps) / (n + K eps) * n, E_k <- M_k / Nt_k for
    every code -- whatever the optimizer did to E is overwritten -- and the accumulators back to zero.  The parameter epoch
    moves.  ``reset_codes`` gives restarted codes N = 1 and M = their new row."""

    def __init__(self, vq_layer, decay, eps=None):
        self.decay, self.eps = codebook_ema_settings(decay, eps)
        if self.decay is None:
            raise ValueError(f"{CODEBOOK_EMA_DECAY_KEY} is None: no codebook average is wanted, build no CodebookEMA")
        self.vq = vq_layer
        cb, self.D = quantizer_codebooks(vq_layer)
        self.C, self.K, self.Dc = cb.shape
        if not K.vq_ema_supported(self.K, self.C, self.Dc):
            raise ValueError(f"{CODEBOOK_EMA_DECAY_KEY}: num_embeddings {self.K} with {self.C} codebooks of width {self.Dc} is not "
                             f"covered by the EMA kernels (K <= {K.VQ_EMA_MAX_K}, C <= {K.VQ_EMA_MAX_C}, Dc <= {K.VQ_EMA_MAX_DC})")
        dev = cb.device
        self.N = torch.ones((self.C, self.K), dtype=torch.float32, device=dev)
        self.M = cb.detach().clone().contiguous()
        self.words = torch.zeros(self.C * self.K + 1, dtype=torch.int64, device=dev)
        self.acc_n, self.invalid = self.words[:-1].view(self.C, self.K), self.words[-1:]
        self.acc_s = torch.zeros((self.C, self.K, self.Dc), dtype=torch.float32, device=dev)
        self.observed = self.updates = 0       # calls so far (host counters; a replayed step runs no Python and is not counted)

    def codebooks(self):
        return quantizer_codebooks(self.vq)[0]

    def restart_from_codebooks(self):
        """N = 1, M = the codebooks as they stand, empty window: the state of a fresh run (``load_weights_only``)."""
        self.N.fill_(1.0)
        self.M.copy_(self.codebooks())
        self.words.zero_()
        self.acc_s.zero_()

    def observe(self, inds, latents_nhwc):
        lat = latents_nhwc.detach()
        K.vq_ema_stats(lat if lat.is_contiguous() else lat.contiguous(), inds, self.acc_n, self.acc_s, self.invalid)
        self.observed += 1

    def update(self, reduce=None):
        if reduce is not None:
            reduce(self.words[:-1], self.acc_s)      # (the invalid word stays this rank's own count)
        K.vq_ema_update(self.codebooks(), self.N, self.M, self.acc_n, self.acc_s, self.decay, self.eps)
        K.bump_param_epoch()
        self.updates += 1

    def reset_codes(self, entries, rows=None):
        """Restarted codes: for every entry (c, k[, ...]) N[c][k] = 1 and M[c][k] = rows[i], or with ``rows`` None the code's
        current codebook row (what ``ctvae_vq_restart`` has just written)."""
        ent = torch.as_tensor([[int(e[0]), int(e[1])] for e in entries], dtype=torch.int64).reshape(-1, 2)
        if ent.numel() == 0:
            return
        if bool(((ent < 0) | (ent >= torch.tensor([self.C, self.K]))).any()):
            raise ValueError("CodebookEMA.reset_codes: an entry (c, k) is out of range")
        ent = ent.to(self.N.device)
        c, k = ent[:, 0], ent[:, 1]
        new = self.codebooks()[c, k] if rows is None else torch.as_tensor(rows, dtype=torch.float32).to(self.M.device)
        if tuple(new.shape) != (ent.size(0), self.Dc):
            raise ValueError(f"CodebookEMA.reset_codes: rows must be [n, Dc] = {(ent.size(0), self.Dc)}, got {tuple(new.shape)}")
        self.M[c, k] = new
        self.N[c, k] = 1.0

    def cluster_sizes(self):
        """(min_k N, max_k N) per codebook on the host: one copy."""
        n = self.N.detach().cpu()
        return n.min(dim=1).values.tolist(), n.max(dim=1).values.tolist()

    def state_dict(self):
        return {"decay": float(self.decay), "eps": float(self.eps), "N": self.N.detach().cpu().clone(),
                "M": self.M.detach().cpu().clone(), "acc_n": self.acc_n.detach().cpu().clone(),
                "acc_s": self.acc_s.detach().cpu().clone(), "invalid": int(self.invalid.cpu())}

    def load_state_dict(self, sd):
        if float(sd["decay"]) != self.decay:
            raise RuntimeError(f"codebook average was kept under {CODEBOOK_EMA_DECAY_KEY}={sd['decay']!r}, this run uses "
                               f"{self.decay!r}")
        if float(sd["eps"]) != self.eps:
            raise RuntimeError(f"codebook average was kept under {CODEBOOK_EMA_EPS_KEY}={sd['eps']!r}, this run uses {self.eps!r}")
        for name, t in (("N", self.N), ("M", self.M), ("acc_n", self.acc_n), ("acc_s", self.acc_s)):
            if tuple(sd[name].shape) != tuple(t.shape):
                raise RuntimeError(f"codebook average: checkpoint's {name} {tuple(sd[name].shape)} does not fit this model's "
                                   f"codebooks {tuple(t.shape)}")
        for name, t in (("N", self.N), ("M", self.M), ("acc_n", self.acc_n), ("acc_s", self.acc_s)):
            t.copy_(sd[name])
        self.invalid.fill_(int(sd.get("invalid", 0)))


TRACK_NORM_KEY = "track_grad_norm"
WATCH_KEY, WATCH_FREQ_KEY = "watch_gradients", "watch_log_freq"


def track_grad_norm_setting(value):
    """Validated ``track_grad_norm`` with Lightning 1.6.5's rule: None or -1 is off (returned as None); a number > 0, or
    ``'inf'`` / ``inf``, is the norm type (returned as a float).  A bool, 0, any other negative number, NaN or any other string
    raises a ValueError that names the key."""
    if value is None:
        return None
    if isinstance(value, str):
        if value != "inf":
            raise ValueError(f"{TRACK_NORM_KEY} {value!r} is invalid: it must be a number > 0, 'inf' or -1 (off)")
        return math.inf
    if isinstance(value, bool) or not isinstance(value, (int, float)) or math.isnan(value):
        raise ValueError(f"{TRACK_NORM_KEY} {value!r} is invalid: it must be a number > 0, 'inf' or -1 (off)")
    if value == -1:
        return None
    if value <= 0:
        raise ValueError(f"{TRACK_NORM_KEY} {value!r} is invalid: it must be a number > 0, 'inf' or -1 (off)")
    return float(value)


def watch_settings(watch, log_freq=None):
    """Validated ``(watch_gradients, watch_log_freq)``: a bool (None: False) and an integer >= 1 (None: 500, wandb's
    ``watch(log_freq=500)`` of the reference's run.py).  Anything else raises a ValueError that names the key."""
    if watch is not None and not isinstance(watch, bool):
        raise ValueError(f"{WATCH_KEY} {watch!r} is invalid: it must be true or false")
    if log_freq is None:
        log_freq = 500
    if isinstance(log_freq, bool) or not isinstance(log_freq, int) or log_freq < 1:
        raise ValueError(f"{WATCH_FREQ_KEY} {log_freq!r} is invalid: it must be an integer >= 1")
    return bool(watch), int(log_freq)


def grad_norm_key(norm_type) -> str:
    """Lightning's key stem: ``grad_<float(p)>_norm`` (``grad_2.0_norm``, ``grad_inf_norm``)."""
    return f"grad_{float(norm_type)}_norm"


def histc_bins(values, lo, hi, bins=K.GRAD_HIST_BINS):
    """The bin of every entry of the float32 numpy array ``values`` (finite, inside [lo, hi]) by the rule the histogram kernel
    restates from ``torch.histc`` on the CPU, carried out in fp32: min((long)((v - lo) / (hi - lo) * bins), bins - 1), with
    lo == hi widened to lo - 1, hi + 1 and a quotient that is not a number counted in bin 0.  The kernel's reference in the tests."""
    import numpy as np
    lo, hi = np.float32(lo), np.float32(hi)
    if lo == hi:
        lo, hi = np.float32(lo - np.float32(1)), np.float32(hi + np.float32(1))
    with np.errstate(all="ignore"):
        q = ((values.astype(np.float32) - lo) / np.float32(hi - lo) * np.float32(bins)).astype(np.float32)
    out = np.zeros(q.shape, dtype=np.int64)
    ok = q >= 0                                     # (NaN: False)
    out[ok] = np.minimum(q[ok], np.float32(bins - 1)).astype(np.int64)
    return out


class GradientTracker:
    """Per-parameter gradient norms (Lightning 1.6.5's ``track_grad_norm``) and 64-bin gradient histograms (wandb's
    ``watch(log="gradients")``) of the gradient an optimizer step was handed, read from the flat gradient buffer by the HIP
    kernels of csrc/gradstat.hip: two launches for the norms, a third for the histograms, ONE device-to-host copy.

    What is measured.  ``record()`` is called eagerly behind the optimizer step of a batch that ends a window.  No Adam kernel
    writes the gradient (``ctvae_adam_step``, ``_clipped`` and ``_blocks`` all take it as ``const float*``; the clip factor is
    applied in registers), so by then the optimizer's slice of the flat buffer still holds exactly what was stepped, before any
    scale: the batch's gradient, the DDP sum, or the window's sum.  With ``scale`` = the step's ``grad_scale`` (1 / (world * k))
    the kernels see the averaged PRE-CLIP gradient -- where Lightning's ``_track_grad_norm`` sits: behind accumulation and the DDP
    average, in front of the clip.  wandb hooks every micro-batch's local gradient instead; this records the gradient that is
    stepped (a deliberate difference).

    Which parameters.  The named parameters whose segment (``FlatParamMixin.grad_segments``) lies inside the optimizer's slice:
    with ``update_parameters`` only that range is exchanged and stepped, so only it is tracked -- Lightning walks every module
    parameter and would report the frozen ones too (as whatever their stale ``.grad`` holds).  In the two ``absent_grad`` skip modes
    a parameter whose Adam block's ``active`` word was 0 in the step is left out of both records (Lightning: ``p.grad is None``);
    the words travel in the same copy.  Under "zero" every parameter is reported.

    Parity.  The norm record restates ``pytorch_lightning.utilities.grads.grad_norm`` of 1.6.5 (keys ``grad_<p>_norm/<name>``
    with the LightningModule's ``model.`` prefix, ``grad_<p>_norm_total`` = the p-norm of the per-parameter norms, every value
    rounded to 4 decimals) and the histogram record wandb's ``log_tensor_stats`` (finite values only, 64 bins between their min
    and max); neither package is installed, so both parities are UNPINNED.  The norm type travels to the kernel as fp32 and the
    root is taken with the same value.  NaN in a gradient gives a NaN norm, as ``torch.norm`` does."""

    def __init__(self, optimizer, norm_type=None, watch=False, watch_log_freq=None):
        self.opt = optimizer
        self.norm_type = track_grad_norm_setting(norm_type)
        self.watch, self.watch_log_freq = watch_settings(watch, watch_log_freq)
        self.table = self.names = self.block_of = None
        if not self.enabled:
            return
        model = optimizer.model
        model.flat_params                                  # (flattens on first use: both buffers exist from here on)
        grads = model._flat_grads[optimizer.slice]
        start, n = int(optimizer.slice.start or 0), grads.numel()
        names, segs = [], []
        for name, base, rows, period, col_lo, width in model.grad_segments():
            first, end = base + col_lo, base + (rows - 1) * period + col_lo + width
            if start <= first and end <= start + n:
                names.append(name)
                segs.append((base - start, rows, period, col_lo, width))
        if not segs:
            raise ValueError("gradient tracking: no named parameter lies inside the optimizer's slice")
        self.names = names
        if optimizer.absent_grad != "zero":            # the Adam block that holds each segment's first element
            self.block_of = []
            for (base, _, _, col_lo, _) in segs:
                first = base + col_lo
                hit = [i for i, b in enumerate(optimizer.blocks) if b[0] <= first < b[1]]
                if len(hit) != 1:
                    raise RuntimeError(f"gradient tracking: offset {first} of the slice lies in {len(hit)} Adam blocks")
                self.block_of.append(hit[0])
        nflags = 0 if self.block_of is None else optimizer.table.nb
        self.table = K.GradSegmentTable(segs, n, grads.device, nflags=nflags)

    @property
    def enabled(self) -> bool:
        return self.norm_type is not None or self.watch

    def due(self, step: int, log_every: int):
        """(norms, histograms) wanted for optimizer step ``step`` (counted from 0): norms where the training scalars are logged,
        histograms every ``watch_log_freq`` steps."""
        return (self.norm_type is not None and step % log_every == 0, self.watch and step % self.watch_log_freq == 0)

    def measure(self, scale: float, hist: bool):
        """The launches and the one copy.  Returns (names, present, sum [nseg, 2], range [nseg, 2], bad [nseg], hist [nseg, 64])
        on the host; present[i]: whether segment i's Adam block stepped (always True under absent_grad "zero")."""
        opt = self.opt
        g = opt.model._flat_grads[opt.slice]           # (not ``flat_grads``: behind the step the buffer is complete as it is)
        p = self.norm_type if self.norm_type is not None else 2.0
        K.grad_segment_stats(self.table, g, scale, p, opt.table.active if self.block_of is not None else None)
        if hist:
            K.grad_segment_hist(self.table, g, scale)
        s, r, bad, h, flags = self.table.fetch()
        if self.block_of is None:
            present = [True] * len(self.names)
        else:
            fl = flags.tolist()
            present = [fl[b] != 0 for b in self.block_of]
        return self.names, present, s, r, bad, h

    def norm_record(self, names, present, sums):
        """Lightning's ``grad_norm`` dict from the kernels' sums: per-parameter norms, their p-norm as the total, 4 decimals."""
        p = self.norm_type
        stem = grad_norm_key(p)
        p32 = p if math.isinf(p) else float(torch.tensor(p, dtype=torch.float32))
        norms = []
        rec = {}
        for i, name in enumerate(names):
            if not present[i]:
                continue
            total, amax = float(sums[i, 0]), float(sums[i, 1])
            v = amax if math.isinf(p) else (math.sqrt(total) if p32 == 2.0 else (total if p32 == 1.0 else total ** (1.0 / p32)))
            norms.append(v)
            rec[f"{stem}/model.{name}"] = round(v, 4)
        if norms:
            if any(math.isnan(v) for v in norms):
                tot = math.nan
            elif math.isinf(p):
                tot = max(norms)
            elif any(math.isinf(v) for v in norms):
                tot = math.inf
            elif p32 == 2.0:
                tot = math.sqrt(math.fsum(v * v for v in norms))
            else:
                tot = math.fsum(v ** p32 for v in norms) ** (1.0 / p32)
            rec[f"{stem}_total"] = round(tot, 4)
        return rec

    @staticmethod
    def hist_record(names, present, rng, bad, hist):
        rec = {}
        for i, name in enumerate(names):
            if not present[i]:
                continue
            lo, hi = float(rng[i, 0]), float(rng[i, 1])
            none = not lo <= hi                            # +inf, -inf: the segment holds no finite value
            rec[f"gradients/{name}"] = {"min": None if none else lo, "max": None if none else hi,
                                        "counts": [int(c) for c in hist[i].tolist()], "nonfinite": int(bad[i])}
        return rec

    def record(self, step: int, log_every: int, scale: float):
        """What is due at optimizer step ``step``: (norm record or None, histogram record or None), without the ``step`` and
        ``lr-Adam`` entries the caller adds.  Launches, copies and allocates nothing when nothing is due."""
        want_norm, want_hist = self.due(step, log_every) if self.enabled else (False, False)
        if not (want_norm or want_hist):
            return None, None
        names, present, sums, rng, bad, hist = self.measure(scale, want_hist)
        return (self.norm_record(names, present, sums) if want_norm else None,
                self.hist_record(names, present, rng, bad, hist) if want_hist else None)


class ExponentialLR:
    """lr_epoch = lr0 * gamma**epoch (torch.optim.lr_scheduler.ExponentialLR), stepped once per epoch."""

    def __init__(self, optimizer: FlatAdam, gamma: float):
        self.opt, self.gamma, self.base_lr, self.epoch = optimizer, gamma, optimizer.lr, 0

    def step(self):
        self.epoch += 1
        self.opt.set_lr(self.base_lr * self.gamma ** self.epoch)
