"""Data-parallel gradient exchange: all-reduce over the model's flat gradient buffer.

Replaces what the reference gets implicitly from Lightning's ``DDPStrategy`` -> torch
``DistributedDataParallel`` (run.py:99): gradient buckets only, no model sharding,
per-rank BatchNorm statistics (no SyncBN in the reference).  Because parameters and gradients are single
flat fp32 buffers, the exchange is a handful of large RCCL all-reduces (xGMI is point-to-point: few big
messages beat 48 small ones) issued asynchronously (the process group's own stream) as soon as the corresponding
part of the backward pass has been issued; ``1/world`` is folded into the optimizer's ``grad_scale``.

Backend "nccl" is RCCL on ROCm; "gloo" works on CPU tensors for the 2-rank unit tests.
"""
import torch
import torch.distributed as dist


def codebook_ema_reduce(words, sums, all_reduce_sum):
    """The reduce plumbing of ``GradBucketAllReduce.all_reduce_codebook_ema`` on any tensors (host tensors under gloo): pack the
    int64 ``words`` and the fp32 ``sums`` into one float64 buffer, hand it to ``all_reduce_sum`` (in place), unpack in place."""
    nw = words.numel()
    buf = torch.cat([words.reshape(-1).to(torch.float64), sums.reshape(-1).to(torch.float64)])
    all_reduce_sum(buf)
    words.copy_(buf[:nw].to(torch.int64).view_as(words))
    sums.copy_(buf[nw:].to(torch.float32).view_as(sums))


class GradBucketAllReduce:
    def __init__(self, model, process_group=None, bucket_bytes=32 << 20, broadcast_from=0, force=False):
        """force: issue the collectives even in a 1-rank group (rehearsal of the N>1 call pattern on one GPU)."""
        self.model = model
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        self.active = self.world > 1 or (force and dist.is_initialized())
        self.bucket_elems = max(1, bucket_bytes // 4)
        self.range = None
        self.accumulate = 1        # VAEXperiment sets its accumulate_grad_batches here (all_reduce_range)
        if self.active and broadcast_from is not None:
            self.broadcast_parameters(broadcast_from)

    # C3: parameters (and buffers) from rank 0 once at construction
    def broadcast_parameters(self, src=0):
        dist.broadcast(self.model.flat_params, src, group=self.pg)
        from . import kernels as K
        K.bump_param_epoch()                 # cached Winograd filters were made from the old values
        for b in self.model.buffers():
            if b.is_floating_point():
                dist.broadcast(b, src, group=self.pg)

    def restrict(self, flat_slice):
        """Exchange only flat_grads[flat_slice]: the harness calls this when it optimises one sub-module
        (``update_parameters``, experiment.py:156-160) -- the other gradients are never applied, so they need not travel."""
        self.range = flat_slice

    def buckets(self):
        g = self.model.flat_grads
        if self.range is not None:
            g = g[self.range]
        n = g.numel()
        out, off = [], 0
        while off < n:
            e = min(n, off + self.bucket_elems)
            out.append(g[off:e])
            off = e
        return out

    def all_reduce(self, async_op=False):
        """SUM all-reduce of every bucket (division by world size is the caller's grad_scale).  The process group runs
        collectives on its own stream behind the current one; with async_op the current stream waits only in wait()."""
        if not self.active:
            return []
        if hasattr(self.model, "gather_torch_grads"):
            self.model.gather_torch_grads()            # autograd-produced gradients into the flat buffer first
        if not async_op:   # stream-ordered, no work objects: measured 0.09 ms per step cheaper than async + wait
            for b in self.buckets():
                dist.all_reduce(b, op=dist.ReduceOp.SUM, group=self.pg)
            return []
        return [dist.all_reduce(b, op=dist.ReduceOp.SUM, group=self.pg, async_op=True) for b in self.buckets()]

    def all_reduce_range(self, lo, hi, async_op=True):
        """Asynchronous SUM all-reduce of flat_grads[lo:hi] (bucketed), ordered behind everything issued so far on the
        current stream.  Returns the work handles for wait().  Refused under gradient accumulation: a range of ONE
        micro-batch's gradients would travel while the window's sum is still being formed (SplitBackward's overlap)."""
        if self.accumulate > 1:
            raise RuntimeError(f"all_reduce_range (SplitBackward's ranged exchange) is not available with accumulate_grad_batches="
                               f"{self.accumulate}: the gradients are exchanged once per window, after its last micro-batch")
        if not self.active or hi <= lo:
            return []
        if hasattr(self.model, "gather_torch_grads"):
            self.model.gather_torch_grads()
        g = self.model.flat_grads
        parts, off = [], lo
        while off < hi:
            e = min(hi, off + self.bucket_elems)
            parts.append(g[off:e])
            off = e
        # async_op: the process group runs the collective on its own stream, ordered behind the current stream; the
        # current stream only waits when wait() is called.  (Wrapping this in an extra communication stream costs two more
        # cross-stream waits per call -- measured 0.15 ms per step on MI355X.)
        if not async_op:
            for b in parts:
                dist.all_reduce(b, op=dist.ReduceOp.SUM, group=self.pg)
            return []
        return [dist.all_reduce(b, op=dist.ReduceOp.SUM, group=self.pg, async_op=True) for b in parts]

    def all_reduce_flags(self, flags):
        """MAX all-reduce, in place, of FlatAdam's int32 [nb] block-activity flags (``FlatAdam.step(reduce_flags=...)``): a
        block counts as active everywhere when some rank has a gradient for it.  One small collective, stream-ordered like the
        gradient buckets; the optimizer issues it before them, so that it travels while they are being queued."""
        if self.active:
            dist.all_reduce(flags, op=dist.ReduceOp.MAX, group=self.pg)

    def all_reduce_counts(self, counts):
        """SUM all-reduce, in place, of the int64 codebook usage counts (``optim.CodebookUsage.restart``): a code is dead only
        when no rank chose it often enough.  One small collective per restart, stream-ordered."""
        if self.active:
            dist.all_reduce(counts, op=dist.ReduceOp.SUM, group=self.pg)

    def all_reduce_codebook_ema(self, words, sums):
        """ONE SUM all-reduce, in place, of the window accumulators of ``optim.CodebookEMA``: the int64 counts and the fp32
        sums travel as one float64 buffer -- integers below 2^53 and fp32 values are exact in it, the
        ranks' shares are added in float64 and the sums rounded back to fp32 once, so every rank ends with the same bits (and a
        group of one rank with the bits it had)."""
        if self.active:
            codebook_ema_reduce(words, sums, lambda t: dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.pg))

    def broadcast_rows(self, rows, src=0):
        """Rank ``src``'s gathered restart rows to every rank, in place: the pools differ from rank to rank, the restarted codes
        must not."""
        if self.active:
            dist.broadcast(rows, src, group=self.pg)

    def wait(self, works):
        for w in works:
            w.wait()

    @property
    def grad_scale(self):
        return 1.0 / self.world

    def reduce_scalars(self, values: dict) -> dict:
        """C4: one fused all-reduce(mean) for all logged scalars instead of one per key."""
        keys = sorted(values)
        if self.world == 1 or not keys:
            return dict(values)
        t = torch.stack([values[k].detach().float().reshape(()) for k in keys])
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.pg)
        t /= self.world
        return {k: t[i] for i, k in enumerate(keys)}


class SplitBackward:
    """VanillaVAE training step cut at the latent z, so that the decoder-side gradient buckets travel over xGMI while
    the encoder's backward still runs (DDP's bucket/backward overlap, SURVEY.md §8e, without autograd hooks: parameter
    gradients are written by the wgrad kernels, not by AccumulateGrad nodes).

        stage1: encode -> reparameterize -> decode(z as a fresh leaf) -> loss; backward restricted to {z, decoder params}
        stage2: backward of (loss via mu/log_var, z with the gradient stage1 left on the leaf) restricted to encoder params

    Both stages are hipGraph-capturable; the flat gradient buffer is laid out in registration order, so the two sides
    are the contiguous ranges [0, split) and [split, n)."""

    DECODER_SIDE = ("decoder_input", "decoder", "final_layer")

    def __init__(self, model):
        self.model = model
        names = [n for n, _ in model.named_parameters()]
        dec = lambda n: n.split(".")[0] in self.DECODER_SIDE
        self.dec_params = [p for n, p in model.named_parameters() if dec(n)]
        self.enc_params = [p for n, p in model.named_parameters() if not dec(n)]
        if not self.dec_params or not self.enc_params or not hasattr(model, "reparameterize"):
            raise ValueError("SplitBackward needs a VanillaVAE-like model (encode / reparameterize / decode)")
        base = model.flat_params.data_ptr()
        lo = min((p.data_ptr() - base) // 4 for p in self.dec_params)
        hi_enc = max((p.data_ptr() - base) // 4 + p.numel() for p in self.enc_params)
        if hi_enc > lo:
            raise ValueError("encoder- and decoder-side parameters are not two contiguous ranges of the flat buffer")
        self.split = int(lo)
        self.total = model.flat_params.numel()
        self._loss = self._z = self._z_leaf = None
        del names

    def stage1(self, x, eps=None, **loss_kwargs):
        m = self.model
        mu, log_var = m.encode(x)
        z = m.reparameterize(mu, log_var, eps)
        z_leaf = z.detach().requires_grad_(True)
        recon = m.decode(z_leaf)
        losses = m.loss_function(recon, x, mu, log_var, **loss_kwargs)
        loss = losses["loss"]
        torch.autograd.backward([loss], inputs=[z_leaf] + self.dec_params, retain_graph=True)
        self._loss, self._z, self._z_leaf = loss, z, z_leaf
        return losses

    def stage2(self):
        torch.autograd.backward([self._loss, self._z], [None, self._z_leaf.grad], inputs=self.enc_params)
