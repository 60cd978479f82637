"""Lightning-free counterpart of the reference's training harness (experiment.py:17-187).

``VAEXperiment`` keeps the reference's step semantics: batch unpacking ``(real_img, labels, *options)``,
``model(real_img, labels=..., **options)``, ``loss_function(*results, M_N=kld_weight)`` for training and
``M_N=1.0`` with a ``val_`` key prefix for validation, Adam(lr=LR, weight_decay) + ExponentialLR(gamma)
over ``model.parameters()`` or ``getattr(model, update_parameters).parameters()``, with the Trainer's gradient clipping
(``gradient_clip_val`` / ``gradient_clip_algorithm``, see optim.py) in front of the step; ``exp_params.adam_absent_grad``
("zero", the default; "skip"; "skip_until_first") chooses what the step does to parameters without a gradient (optim.py; under
a DDP gradient exchange the two skip modes MAX-reduce their per-block activity flags across ranks, ``ddp_step``).  What changes is the
machinery: one flat fused Adam launch, one bucketed RCCL all-reduce, and scalars fetched with ONE device
-> host copy every ``log_every`` steps instead of one ``.item()`` sync per key per step (experiment.py:95-96).

``accumulate_grad_batches`` (the Trainer key of that name, an integer k >= 1; 1 is the path above, launch for launch): Lightning
1.6.5's gradient accumulation.  The batch index counts from 0 in every epoch; batch i ends a window when (i + 1) % k == 0 or it
is the epoch's last batch (``fit()`` looks one batch ahead, so the loader's batches must not share storage), and the optimizer
steps there, on (sum of the window's gradients) / k -- divided by k, not by the window's length, in an incomplete last window
too.  No window state crosses an epoch boundary.  ``zero_grad`` runs before every micro-batch; BatchNorm statistics, the models'
loss-call counters and the in-kernel noise advance per micro-batch; clipping and weight decay apply once per window
(``FlatAdam.stash`` / ``step``, optim.py).  ``global_step`` counts optimizer steps, a training record is logged on a window's last
micro-batch (its own un-normalised losses) when ``global_step % log_every == 0``, ``train_images`` counts every image.  Captured
steps end behind ``gather_torch_grads()`` when k > 1, as they do under DDP, and the stash or step launches follow the replay
eagerly: one graph per signature serves every position in a window.  Under DDP a micro-batch inside a window issues no
collective at all; the one that ends it sends the merged block flags (skip modes) and the window's sum, and steps with
``grad_scale = 1 / (world * k)``.  ``ddp.SplitBackward``'s ranged exchange is refused in this mode.

The step's tail.  ``finish_batch`` follows every backward pass, captured, eager or accumulated: the stash or the step (nothing
when Adam was part of the captured body), and behind a batch that ends its window ``_after_optimizer_step``, "the tail" below:
``track_gradients()`` (the flat buffer still holds what was stepped), ``codebook_update()`` (it overwrites the codebooks Adam
moved), ``ema_update()`` (the weight average sees the codebook the step ends with), ``codebook_restart()`` (a restarted code gets
N = 1 and M = its row; the weight average goes on towards the new row), then ``global_step += 1``: all four see the number of
the step that ran.  The tail is eager, never captured (decays are by-value kernel arguments, which a captured launch would
freeze; the dead list is formed on the host), and runs once per optimizer step, so once per accumulation window.

The validation order.  ``_validate`` arms every report the run has (a context each: reset or rebuilt, then observing; disarmed
in a ``finally``), runs the validation steps, and collects in the key order of the epoch record: the steps' means,
``write_graphs``, ``write_codebook_stats``, ``write_latent_stats``, ``write_recon_stats``, ``write_prior``, ``write_loglik``,
``validation_metrics``, and last ``sample_images``.  The reports are eager like all of validation, make their one device-to-host copy behind the steps, are rank
0's own rows (no collective) and, under ``ema_eval``, describe the averaged weights; a ``validation_step`` outside ``_validate``
observes nothing.

``val_metric`` (a ``metrics.MetricSet``): the reference recomputes the disentanglement metrics inside EVERY validation batch
and lets Lightning average the copies (experiment.py:72-74).  That is a cost, not a semantic -- the metric does not read the
batch -- so ``fit()`` computes it ONCE per validation epoch, after the validation batches, on rank 0 only and without a
collective, seeded from ``manual_seed`` and the epoch; the results join the epoch record and the JSONL log under ``val_``.

``val_sampling`` with a ``sample_dir`` (the reference's ``sample_images``, experiment.py:114-150, which Lightning calls at the end
of every validation epoch): ``fit(..., test_batches=...)`` then writes three PNG grids per epoch from the FIRST test batch --
``Inputs/inputs_<name>_Epoch_<e>.png``, ``Reconstructions/recons_<name>_Epoch_<e>.png`` (``model.generate``) and
``Samples/sample_<name>_Epoch_<e>.png`` (``model.sample``; skipped when the model raises ``Warning``, as VQVAE does) -- with
``imagegrid.save_image(normalize=True, nrow=12)``, on rank 0 only and without a collective.  Differences from the reference: it
samples ``min(32, rows of the test batch)`` images with that many of the batch's labels (``ConditionalVAE.sample(32,
labels=<whole batch>)`` cannot concatenate unless the batch has 32 rows); a per-row ``mode`` list, which the transition loaders
hand out, is passed on as its one mode, so that ``CTMCQVAE.generate``'s causal -> action remap sees it.  The call leaves the
run as it found it: eval mode and ``no_grad`` (no BatchNorm statistics, no in-kernel noise state, no parameter epoch move), its
``torch.randn`` draws come from generators seeded from ``manual_seed`` and the epoch, and torch's CPU / device generator states
are put back afterwards.

``val_graphs`` (CT-MCQ-VAE only; ``exp_params.val_graphs`` in run.py): during every validation epoch a
``causalgraph.GraphStats`` is the ``graph_observer`` of the model's causal-transition layer, so the validation steps' own
launches leave their per-sample adjacencies and intervention masks in per-group sums (group 0: base mode, group 1 + a: action a;
the causal-mode batches' hypothesised actions are not observed).  Afterwards rank 0 writes
``Graphs/adjacency_<name>_Epoch_<e>.png`` -- the mean adjacency of every group that had rows, group 0 first, one tile each --
and ``Graphs/mask_<name>_Epoch_<e>.png`` -- the mean mask of every action that had rows as an h x w picture -- under
``sample_dir``, and adds ``val_graph_edges_<group>``, the mean number of edges above 0.5 per graph, to the epoch record and the
JSONL log.  The captured training steps never see the observer, and it draws nothing: the run's trajectory is the same with
and without it.

``track_grad_norm`` (Lightning's Trainer flag: a norm type > 0 or 'inf'; None / -1 off) and ``watch_gradients`` with
``watch_log_freq`` (the reference's ``wb_logger.watch(model, log_freq=500)``, run.py:55; off by default): gradient tracking by
``optim.GradientTracker``, which ``track_gradients()`` drives first in the tail (above), and only on tracking steps: the norm
record joins ``log_file`` where the training scalars are logged (``global_step % log_every == 0``), the histogram record goes to
``grad_log_file`` every ``watch_log_freq`` optimizer steps.  No Adam kernel writes the gradient, so at that point the optimizer's
slice of the flat buffer holds exactly what was stepped, before any scale; with the step's ``grad_scale`` 1 / (world * k) the
tracker sees the averaged pre-clip gradient, where Lightning's ``_track_grad_norm`` sits.  Rank 0 measures and writes (three
launches, one device-to-host copy); the other ranks build no tracker.  The run ends bit for bit as it does without tracking;
without both keys there is no tracker, no launch and no key.

``exp_params.ema_decay`` (a float, 0 < d < 1; absent: off) with ``ema_warmup`` (default false) and ``ema_eval`` (default true): an
exponential moving average of the weights the optimizer steps, kept by ``optim.WeightEMA`` on the optimizer's slice of the flat
parameter buffer.  ``ema_update()`` is part of the tail (above), on every rank without a collective: the stepped parameters are
identical on all ranks, so the averages are too.  With ``ema_eval`` all of ``_validate`` runs with the averaged weights swapped
into the flat buffer (``WeightEMA.swapped_in``): the epoch record's ``val_*`` values, and what run.py chooses by them, describe
the averaged weights; BatchNorm running statistics and all random streams are the live ones, and the live weights come back
bit for bit, so the run trains exactly as it does without the key.  ``state_dict()`` carries ``"ema": {decay, warmup, updates}``
(``WeightEMA.state_dict(buffer=False)``); the buffer itself travels as weights (``ema_model_state_dict`` /
``load_ema_model_state_dict``, the checkpoint's ``ema_state_dict``).  Without ``ema_decay`` there is no buffer, no launch and no entry.

``exp_params.codebook_stats`` (a bool) and ``exp_params.codebook_restart_every`` (an integer N >= 1; with
``codebook_restart_min_count``, default 1, and ``codebook_restart_pool``, default 1024): codebook usage of the models with a
``vq_layer`` quantiser, by ``optim.CodebookUsage`` as the quantiser's ``usage_observer``.  The validation counter (rank 0 only) is
one of the reports of ``_validate`` (above): it observes the validation steps alone and adds ``val_codebook_perplexity_<i>`` /
``_usage_<i>`` / ``_dead_<i>`` and their means to the epoch record and the JSONL log; ``sample_images``, ``validation_metrics``,
rollouts and the tools run without an observer.  The training counter observes the training batches of ``fit()``: its launch is
part of the forward, inside the captured body when the step is captured and identical in eager steps, once per micro-batch.
``codebook_restart()`` closes the tail (above) of the optimizer step that makes ``global_step`` a multiple of N (its docstring
has the sequence); the weight average is not special-cased, and the per-block Adam counters of the skip modes are untouched.
``state_dict()`` carries ``"codebook": {every, min_count, pool, counts, ordinal, restarted, valid_rows}``; a full resume restores
it and refuses other ``every`` / ``min_count``.  Refused when the experiment is built: either key on a model without such a
quantiser, and restarts when ``update_parameters`` leaves the codebooks outside the optimizer's slice.  Without the keys there
is no buffer, no launch, no log key and no entry.

``exp_params.codebook_ema_decay`` (a float, 0 < g < 1; absent: off) with ``codebook_ema_eps`` (default 1e-5): EMA codebooks (van den
Oord et al. 2017, appendix A.1) for the models with a ``vq_layer`` quantiser, by ``optim.CodebookEMA``.  With the key the
quantiser's ``ema`` is set for good -- ``VQ_Loss`` is the commitment term alone, beta / (1 + beta) of the value without the key, in
training and validation records alike, and no codebook gradient is formed: the codebooks' block of the flat gradient buffer is an
absent block -- and ``CodebookEMA.observe`` is its ``ema_observer`` around the training batches of ``fit()`` only
(``_counting_training_codes``): one statistics call per index search, part of the forward, inside the captured body when the step
is captured.  ``codebook_update()`` is part of the tail (above).  Under DDP the window accumulators are SUM-reduced first:
one small collective per optimizer step, none inside a window, and all ranks hold the same N, M and codebooks.  Records on
logging steps: ``codebook_ema_min_cluster[_<i>]`` / ``codebook_ema_max_cluster[_<i>]``.  ``state_dict()`` carries ``"codebook_ema":
{decay, eps, N, M, acc_n, acc_s, invalid}``; a full resume restores it and refuses another decay or eps, or a checkpoint
without the entry.  Refused when the experiment is built: the key on another model, and the key when ``update_parameters`` leaves
the codebooks outside the optimizer's slice.  Without the key there is no buffer, no launch, no log key and no entry.

``exp_params.latent_stats`` (a bool): latent usage of the models with a Gaussian posterior (``BaseVAE.gaussian_posterior``), by
``latentstats.LatentStats`` on rank 0, a report of ``_validate`` (above).  Armed, it is zeroed and every ``validation_step`` hands
it the batch's ``mu`` / ``log_var`` views (one ``ctvae_latent_accumulate`` launch); ``write_latent_stats`` adds
``val_latent_kl_total`` / ``_active_units`` / ``_collapsed`` / ``_mean_abs_corr`` / ``_gaussian_tc`` / ``_nonfinite`` / ``_rows`` to the
epoch record and the JSONL log (what is undefined is left out), and with a ``sample_dir`` writes
``Latents/latent_stats_<name>_Epoch_<e>.npz`` and ``Latents/corr_<name>_Epoch_<e>.png``.  It draws nothing and writes no model
state, so training is bit for bit the same with and without it.  Refused when the experiment is built: the key on a model
whose hook returns None.  Without the key there is no buffer, no launch, no file and no log key.

``exp_params.kld_schedule`` (a mapping: linear warm-up or cyclical annealing of the KL weight) and ``exp_params.kld_free_bits`` (a
float >= 0, nats per latent dimension): ``klcontrol.KLControl`` (its module docstring has the definitions), on the models whose
training loss is recon + c * M_N * KL.  The run owns one persistent 1-element device tensor; ``write_kl_weight()`` puts
w(``global_step``) into it in front of every training step -- eagerly, also in front of a replay, one fill and only when the value
changed -- and the step hands ``loss_function`` ``M_N=<that tensor>`` and ``free_bits=lambda``: the loss launch
(``kernels.FreeBitsKL``) reads the weight from device memory, so a captured step follows the schedule (a by-value ``M_N`` is
frozen at capture).  Every micro-batch of an accumulation window uses the window's weight; every rank computes the same weight
from ``global_step``, the batch mean under the floor is over the rank's own rows, and no collective is added.  Training records
gain ``kld_weight`` (the host's value, no copy), ``KLD_free_bits`` and ``KLD_floored_dims``; validation (``M_N = 1.0``) is untouched.
``state_dict()`` carries ``"kl": {schedule, free_bits}``; a full resume under other values is refused by name, the weight itself
needs no state.  Refused when the experiment is built: either key on another model.  Without the keys there is no buffer, no
launch, no log key and no entry.

``exp_params.sample_prior`` (a mapping with ``type: gmm``; ``latentprior.prior_setting``): a Gaussian-mixture prior fitted to the
validation codes of the models in ``latentprior.PRIOR_MODELS``, on rank 0, a report of ``_validate``.  Armed, the code buffer
(``latentprior.CodeBuffer``) is cleared and every ``validation_step`` hands it the batch's ``mu`` view (``codes: sample``: ``mu +
exp(0.5 log_var) * eps`` with eps from a generator of the report's own), one device-to-device copy; ``write_prior`` fits the rows
with an even ordinal (``latentprior.GaussianMixturePrior``, csrc/gmm.hip), holds out the odd ones and adds
``val_prior_mixture_loglik`` / ``_standard_loglik`` / ``_iterations`` / ``_rows`` / ``_nonfinite`` to the epoch record (a refused fit:
``val_prior_error``) and, with a ``sample_dir``, ``Priors/latent_prior_<name>_Epoch_<e>.npz``; with ``val_sampling``
``sample_mixture_images`` writes ``Samples/sample_mixture_<name>_Epoch_<e>.png`` from a generator of its own next to the unchanged
``sample_<name>_...png``.  It adds nothing to checkpoints and moves no random stream.
``exp_params.recon_stats`` (a bool; with ``recon_stats_range``, the data range R, a float > 0, default 1.0, and ``recon_stats_worst``,
an integer 0 <= K <= 32, default 8): the reconstruction quality per validation image, by ``reconstats.ReconStats`` on rank 0,
a report of ``_validate`` (above).  Armed, it is reset and every ``validation_step`` hands it the pair
``BaseVAE.reconstruction_pair`` returns (one ``ctvae_recon_record`` launch, and the two of ``ctvae_recon_worst`` when K > 0);
``write_recon_stats`` adds ``val_recon_psnr`` / ``_ssim`` / ``_mae`` / ``_max_err`` / ``_psnr_p05`` / ``_ssim_p05`` / ``_psnr_min`` /
``_ssim_min`` / ``_rows`` / ``_nonfinite`` / ``_exact`` to the epoch record and the JSONL log (what has no image to stand on is left
out), and with a ``sample_dir`` writes ``Recon/recon_stats_<name>_Epoch_<e>.npz`` and, for K > 0,
``Recon/worst_<name>_Epoch_<e>.png``.  CT-MCQ-VAE has two accumulators, keyed by the batch's mode: its keys and file stems carry
``_base`` / ``_action`` (in action mode the target is ``input_y``), and causal batches, which have no picture pair, feed none.  It
draws nothing and writes no model state, so training is bit for bit the same with and without it.  Refused when the
experiment is built: a bad value, a dependent key without the main one, and IWAE / MIWAE, whose ``forward`` hands out
[B, S, C, H, W] samples.  Without the key there is no buffer, no launch, no file and no log key.
``exp_params.val_loglik`` (a mapping with ``samples``, an int in 1..4096, ``sigma``, a float > 0, and the optional ``chunk``;
``loglik.loglik_setting``): the marginal log-likelihood of every validation image by importance sampling under N(decode(z),
sigma^2 I), for the models in ``loglik.LOGLIK_MODELS``, by ``loglik.ImportanceLogLik`` on rank 0, a report of ``_validate``.  Armed,
it is reset and every ``validation_step`` hands it the batch's images (``results[1]``) and ``gaussian_posterior(results)``: per
chunk one ``torch.randn`` from a generator of the report's own, seeded from ``epoch_seed(e)``, ``ctvae_loglik_latent``, the
decoder on ``batch * chunk`` rows, ``ctvae_loglik_rows`` and ``ctvae_loglik_merge`` (csrc/loglik.hip), no host synchronisation;
``write_loglik`` makes the one copy and adds ``val_loglik`` / ``_elbo`` / ``_gap`` / ``_ess`` / ``_rows`` / ``_nonfinite`` to the epoch
record and the JSONL log (what has no image to stand on is left out) and, with a ``sample_dir``,
``Loglik/loglik_<name>_Epoch_<e>.npz``.  The decoder runs in eval mode under ``no_grad``: it writes no model state, moves no other
random stream and adds nothing to checkpoints, so training is bit for bit the same with and without it.  Refused when the
experiment is built: a bad value, ``sigma: mse`` (the command's alone) and any other model.  Without the key there is no buffer,
no launch, no file and no log key.
``exp_params.code_prior`` (a mapping with ``type: markov`` and the optional ``em_iters`` / ``uniform_floor``;
``codeprior.code_prior_setting``): an interpolated Markov prior over the code grids of the models in
``codeprior.CODE_PRIOR_MODELS``, on rank 0 with no collective, a report of ``_validate``.  Armed, the index buffer
(``codeprior.CodeGridBuffer``) is cleared and the quantiser's ``usage_observer`` hands it the indices of every validation search --
chained behind ``codebook_stats``' observer when that is armed too, so both see every search; ``write_code_prior`` counts the rows
with an even ordinal (``ctvae_code_prior_count``), fits lambda on the odd ones (``ctvae_code_prior_score`` per EM round) and reports
THOSE rows: ``val_code_prior_nats`` / ``_bits`` / ``_uniform_nats`` / ``_nats_<c>`` / ``_weight_<expert>`` / ``_rows`` / ``_invalid`` (fewer
than 2 rows: ``val_code_prior_error``) and, with a ``sample_dir``, ``Priors/code_prior_<name>_Epoch_<e>.npz``; with ``val_sampling``
``sample_code_prior_images`` writes ``Samples/sample_code_prior_<name>_Epoch_<e>.png`` from a generator of its own, seeded from
``epoch_seed(e)``, next to the unchanged ``sample_<name>_...png``.  It adds nothing to checkpoints, moves no random stream and
writes no model state, so training is bit for bit the same with and without it.  Refused when the experiment is built: a bad
value and any other model.  Without the key there is no buffer, no launch, no file and no log key.
"""
import contextlib
import json
import os
import time

import torch

from . import causalgraph, codeprior, imagegrid
from . import kernels as K
from .ddp import GradBucketAllReduce
from .evalrun import eval_mode, seeded_torch_rng, unpack_batch
from .klcontrol import KLControl, kl_settings, needs_served_model, serves as kl_serves
from .latentprior import (PRIOR_DIR, CodeBuffer, GaussianMixturePrior, draw_codes, needs_supported_model, prior_setting,
                          prior_supported)
from .latentstats import (LATENT_DIR, LatentStats, has_gaussian_posterior, latent_stats_setting, needs_gaussian_posterior,
                          record as latent_record, write_files as write_latent_files)
from . import loglik
from .reconstats import (RECON_DIR, ReconStats, recon_settings, record as recon_record, refuses_model as recon_refuses_model,
                         summarize as recon_summarize, write_files as write_recon_files)
from .optim import (CodebookEMA, CodebookUsage, ExponentialLR, FlatAdam, GradientTracker, WeightEMA, absent_grad_setting,
                    accumulate_setting, clip_settings, codebook_ema_serves, codebook_ema_settings, codebook_offset,
                    codebook_record, codebook_settings, ema_settings, track_grad_norm_setting, watch_settings, with_window_ends)


def _graph_key(real_img, kwargs):
    """Key of a capturable step: the batch's shape plus, per option, a tensor's shape / dtype or the (one-per-batch) mode name.
    None when an option is neither (such a step stays eager)."""
    items = []
    for k in sorted(kwargs):
        v = kwargs[k]
        if torch.is_tensor(v):
            items.append((k, tuple(v.shape), v.dtype))
        elif k == "mode" and isinstance(v, (str, list)):
            items.append((k, v[0] if isinstance(v, list) else v))
        else:
            return None
    return (tuple(real_img.shape), real_img.dtype, tuple(items))


class _GraphedTrainStep:
    """zero_grad + forward + loss + backward (+ Adam when there is neither a gradient exchange nor gradient accumulation: with
    either, what follows the gradients runs eagerly behind the replay) of one batch signature, captured once into a hipGraph
    and replayed: ~130 launches per VanillaVAE step -- ~400 per CT-MCQ-VAE step -- are host-bound when
    issued eagerly (VanillaVAE bs=256: 3.5 vs 1.8 ms; CT-MCQ-VAE at the YAML's 16 pairs per GPU: 7.5 vs 3.4 ms).
    The first WARM batches of a signature run eagerly as ordinary training steps; capture itself executes nothing, so the
    training trajectory is exactly the eager one.  A signature = input shape + the shapes of the tensor options (input_y,
    action) + the mode (datasets/transition.py hands out one mode per batch): the CT-MCQ-VAE modes each get their own graph
    (none of them reads a device value on the host any more)."""

    WARM = 3

    def __init__(self, exp, real_img, kwargs):
        self.exp = exp
        self.x = K.staging_like(real_img)            # channels_last: the hand-over below is the layout conversion too
        self.static = {k: torch.empty_like(v) for k, v in kwargs.items() if torch.is_tensor(v)}
        self.const = {k: v for k, v in kwargs.items() if not torch.is_tensor(v)}
        self.seen = 0
        self.graph = None
        self.losses = None
        self.pattern = None       # FlatAdam's host-known block activity of this signature's steps (absent_grad skip modes)

    def _body(self):
        exp = self.exp
        exp.model.zero_grad(lazy=True)            # no fill launch: first writers overwrite, settle_grads() fills what nobody wrote
        opts = {**self.static, **self.const}
        labels = opts.pop("labels", None)         # ConditionalVAE reads them (cvae.py:123); a static buffer like every tensor option
        results = exp.forward(self.x, labels=labels, **opts)
        losses = exp.model.loss_function(*results, **exp.loss_options(), optimizer_idx=0, batch_idx=0)
        K.backward(losses['loss'])
        # inside the capture: the fills of unwritten blocks AND the copies of autograd-produced gradients (CT layer: a_dense, mask,
        # positional encoding, the GATv2 vectors) into the flat buffer belong to the replayed step.  Left to ddp.all_reduce() /
        # optimizer.step() outside the graph they would run once -- after the capture step Python sees p.grad already attached to
        # its flat view and copies nothing, while every replay rewrites the graph-pool tensors autograd produced: from the second
        # replay on those parameters would be exchanged and stepped with a zero gradient
        exp.model.gather_torch_grads()
        if exp.ddp is None and exp.accumulate == 1:
            exp.optimizer.step()
            pat = exp.optimizer.host_pattern
            if pat is not None:              # constant per signature: a replay repeats the capture step's launches and flags
                if self.pattern is not None and pat != self.pattern:
                    raise RuntimeError("steps of one graph signature got gradients for different parameter blocks: "
                                       f"{sum(a != b for a, b in zip(pat, self.pattern))} blocks differ")
                self.pattern = pat
        elif exp.optimizer.absent_grad != "zero":
            # the step itself is eager (run()), so eager steps of one signature may differ; what a REPLAY's step needs is the
            # activity of the launches it repeats, the capture step's -- the host's own record is by then the last Python-run
            # step's, maybe another signature's
            self.pattern = exp.optimizer.current_pattern()
        # detached: a live loss keeps the step's autograd graph -- and with it the AccumulateGrad nodes of the parameters
        # torch accumulates itself (the CT layer's banks), bound to the stream they were made on -- alive into the next
        # signature's capture, where running them on that other stream ends the capture with a fault
        return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in losses.items()}

    def run(self, real_img, kwargs=None, ends_window=True):
        """ends_window (gradient accumulation only): whether this micro-batch is followed by the optimizer step."""
        exp = self.exp
        in_graph = exp.ddp is None and exp.accumulate == 1       # Adam is part of the body
        K.stage_batch(self.x, real_img)
        for k, t in self.static.items():
            t.copy_(kwargs[k], non_blocking=True)
        exp.write_kl_weight()              # eager, in front of the capture and of every replay: the body reads the device scalar
        if self.graph is None and self.seen >= self.WARM:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with K.capture_graph(g):
                self.losses = self._body()
            self.graph = g
        if self.graph is not None:
            self.graph.replay()
            if in_graph:
                K.bump_param_epoch()       # the replayed Adam launch changed the parameters behind Python's back
            losses = self.losses
        else:
            losses = self._body()
        self.seen += 1
        exp.finish_batch(ends_window, self.pattern, stepped=in_graph)      # eager, behind the replay
        return losses


class VAEXperiment:

    SAMPLE_DIRS = ("Inputs", "Reconstructions", "Samples")
    GRAPH_DIR = "Graphs"
    MASK_CELL = 16             # pixels per latent position in the mask sheet (the adjacency sheet: causalgraph's 4 per edge)

    def __init__(self, vae_model, params: dict, ddp: GradBucketAllReduce = None, log_every: int = 50, log_file=None,
                 gradient_clip_val=None, gradient_clip_algorithm=None, val_metric=None, val_sampling: bool = False,
                 sample_dir=None, run_name=None, val_graphs: bool = False, accumulate_grad_batches=None, track_grad_norm=None,
                 watch_gradients: bool = False, watch_log_freq=None, grad_log_file=None):
        self.accumulate = accumulate_setting(accumulate_grad_batches)
        self._log_train = True      # training_step logs; fit() clears it for micro-batches that do not end their window
        self.val_metric = val_metric
        self.val_graphs = bool(val_graphs)
        if self.val_graphs:
            from .models.ct_mcq_vae import CTMCQVAE
            if not isinstance(vae_model, CTMCQVAE):
                raise ValueError(f"val_graphs needs a CTMCQVAE (the graphs are its causal-transition layer's), got "
                                 f"{type(vae_model).__name__}")
            if vae_model.ct_layer.action_dim < 2 or vae_model.ct_layer.action_dim % 2:
                raise ValueError(f"val_graphs names its groups as factors in two directions: action_dim must be even and at least "
                                 f"2, got {vae_model.ct_layer.action_dim}")
        self.val_sampling, self.sample_dir = bool(val_sampling), sample_dir
        self.run_name = run_name if run_name is not None else type(vae_model).__name__
        self.gradient_clip_val, self.gradient_clip_algorithm = clip_settings(gradient_clip_val, gradient_clip_algorithm)
        self.model = vae_model
        self.params = params
        self.ddp = ddp
        if absent_grad_setting(params.get("adam_absent_grad")) != "zero" and ddp is not None and not hasattr(ddp, "all_reduce_flags"):
            raise ValueError(f"adam_absent_grad={params['adam_absent_grad']!r} is not available with this DDP gradient exchange: "
                             "it cannot reduce the per-block activity flags across ranks (no all_reduce_flags), and ranks must "
                             "not step differently")
        self.curr_device = None
        self.log_every = log_every
        self.log_file = log_file
        self.global_step = 0
        self.optimizer, self.scheduler = self.configure_optimizers()
        if ddp is not None and "update_parameters" in params:
            ddp.restrict(self.optimizer.slice)
        if ddp is not None and self.accumulate > 1:
            ddp.accumulate = self.accumulate      # (the exchange refuses ranged, SplitBackward-style calls from now on)
        self._graphed = {}          # (shape, dtype) -> _GraphedTrainStep
        # gradient tracking (optim.GradientTracker): validated on every rank, built on rank 0 only -- the others launch nothing
        self.grad_log_file = grad_log_file
        self.last_grad_norms = self.last_grad_hists = None      # the records of the last tracking step (also without log files)
        self.grad_tracker = self._build_tracker(track_grad_norm, watch_gradients, watch_log_freq)
        # weight average (optim.WeightEMA): on every rank -- the stepped parameters are the same everywhere, so are the averages
        decay, warmup, self.ema_eval = ema_settings(params.get("ema_decay"), params.get("ema_warmup"), params.get("ema_eval"))
        self.ema = WeightEMA(self.optimizer, decay, warmup) if decay is not None else None
        self._build_codebook_usage(params)
        self._build_codebook_ema(params)
        # latent usage (latentstats.LatentStats): validated on every rank, built on rank 0 only
        self.latent_stats = latent_stats_setting(params.get("latent_stats"))
        self.val_latents = None
        if self.latent_stats:
            if not has_gaussian_posterior(vae_model):
                raise ValueError(needs_gaussian_posterior(vae_model))
            if self._rank0():
                self.val_latents = LatentStats(vae_model.latent_dim, next(vae_model.parameters()).device)
        # sample prior (latentprior.GaussianMixturePrior): validated on every rank, the code buffer on rank 0 only
        self.sample_prior = prior_setting(params.get("sample_prior"))
        self.val_prior = None                   # the epoch's validation codes (latentprior.CodeBuffer)
        self.last_prior = None                  # the mixture the last validation epoch fitted (None: none, or the fit was refused)
        if self.sample_prior is not None:
            if not prior_supported(vae_model):
                raise ValueError(needs_supported_model(vae_model))
            if self._rank0():
                self.val_prior = CodeBuffer(vae_model.latent_dim, next(vae_model.parameters()).device)
        # test log-likelihood by importance sampling (loglik.ImportanceLogLik): validated on every rank, built on rank 0 only
        self.loglik_cfg = loglik.loglik_setting(params.get("val_loglik"))
        self.val_loglik = None
        if self.loglik_cfg is not None:
            if not loglik.loglik_supported(vae_model):
                raise ValueError("val_loglik: " + loglik.needs_supported_model(vae_model))
            if self._rank0():
                cfg = self.loglik_cfg      # (pixels None: the first batch says how many elements an image has)
                self.val_loglik = loglik.ImportanceLogLik(vae_model.latent_dim, None, cfg["sigma"], cfg["samples"], cfg["chunk"],
                                                          next(vae_model.parameters()).device)
        # code prior (codeprior.MarkovCodePrior): validated on every rank, the index buffer on rank 0 only
        self.code_prior = codeprior.code_prior_setting(params.get("code_prior"))
        self.val_code_prior = None              # the epoch's validation indices (codeprior.CodeGridBuffer)
        self.last_code_prior = None             # the prior the last validation epoch fitted (None: none, or too few rows)
        if self.code_prior is not None:
            if not codeprior.prior_supported(vae_model):
                raise ValueError(codeprior.needs_supported_model(vae_model))
            if self._rank0():
                self.val_code_prior = codeprior.CodeGridBuffer(next(vae_model.parameters()).device)
        # reconstruction quality (reconstats.ReconStats): validated on every rank, built on rank 0 only; CT-MCQ-VAE gets one
        # accumulator per picture mode
        self.recon_stats, self.recon_range, self.recon_worst = recon_settings(params)
        self.val_recon = None                   # {key suffix: ReconStats}; "" for every model but CT-MCQ-VAE
        self._val_observers = []                # what validation_step hands its results: empty outside _validate()
        if self.recon_stats:
            why = recon_refuses_model(vae_model)
            if why is not None:
                raise ValueError(why)
            if self._rank0():
                from .models.ct_mcq_vae import CTMCQVAE
                dev = next(vae_model.parameters()).device
                suffixes = ("_base", "_action") if isinstance(vae_model, CTMCQVAE) else ("",)
                self.val_recon = {sfx: ReconStats(dev, self.recon_range, self.recon_worst) for sfx in suffixes}
        # KL weight schedule / free bits (klcontrol.KLControl): on every rank, the same weight from global_step
        schedule, free_bits = kl_settings(params)
        self.kl = None
        if schedule is not None or free_bits is not None:
            if not kl_serves(vae_model):
                raise ValueError(needs_served_model("kld_schedule" if schedule is not None else "kld_free_bits",
                                                    type(vae_model).__name__ + (f" with loss_type {vae_model.loss_type!r}"
                                                                                if hasattr(vae_model, "loss_type") else "")))
            self.kl = KLControl(schedule, free_bits, params['kld_weight'], next(vae_model.parameters()).device)

    def forward(self, input, **kwargs):
        return self.model(input, **kwargs)

    # -- steps (experiment.py:44-74) ---------------------------------------------------------------------
    def training_step(self, batch, batch_idx, optimizer_idx=0):
        real_img, labels, kwargs = unpack_batch(batch)
        self.curr_device = real_img.device
        results = self.forward(real_img, labels=labels, **kwargs)
        self.write_kl_weight()
        train_loss = self.model.loss_function(*results, **self.loss_options(), optimizer_idx=optimizer_idx, batch_idx=batch_idx)
        if self._log_train:
            self.log_all(train_loss, batch_size=real_img.size(0), validation=False)
        return train_loss['loss']

    # -- KL weight schedule and free bits (exp_params.kld_schedule / kld_free_bits; klcontrol.KLControl) --------------
    def write_kl_weight(self):
        """Called eagerly in front of every training step, also in front of a captured step's replay: w(``global_step``) into the
        device scalar, one fill and only when the value differs from the last one written.  Nothing without the keys."""
        if self.kl is not None:
            self.kl.write(self.global_step)

    def loss_options(self):
        """What a training step hands ``loss_function`` for the KL weight: the float ``kld_weight``, or under the keys the device
        scalar and the floor."""
        if self.kl is None:
            return {"M_N": self.params['kld_weight']}
        return {"M_N": self.kl.tensor, "free_bits": self.kl.floor}

    def validation_step(self, batch, batch_idx, optimizer_idx=0):
        real_img, labels, kwargs = unpack_batch(batch)
        self.curr_device = real_img.device
        with torch.no_grad():
            results = self.forward(real_img, labels=labels, **kwargs)
            val_loss = self.model.loss_function(*results, M_N=1.0, optimizer_idx=optimizer_idx, batch_idx=batch_idx)
            for observe in self._val_observers:        # launches only: nothing comes back to the host before the epoch ends
                observe(results)
        return self.log_all(val_loss, batch_size=real_img.size(0), validation=True, force=True)

    def metric_func(self, x):
        x = x.to(next(self.model.parameters()).device)
        x = self.model.encode(x)[0]
        return x.reshape(x.size(0), -1)

    def validation_metrics(self, epoch: int) -> dict:
        """The ``val_metric`` results of one validation epoch under the ``val_`` prefix (also one JSONL line); {} without a
        metric or off rank 0.  The metric's own generator is seeded per epoch; no torch generator and no model state moves."""
        if self.val_metric is None or not self._rank0():
            return {}
        res = self.val_metric.compute(self.metric_func, model=self.model, seed=self.epoch_seed(epoch))
        return self._write_epoch_record({"val_" + k: v for k, v in res.items()})

    def _rank0(self):
        return self.ddp is None or not torch.distributed.is_initialized() or torch.distributed.get_rank() == 0

    def _active_ddp(self):
        """The gradient exchange when it has a process group to send on (the codebook collectives go through it), else None."""
        return self.ddp if self.ddp is not None and getattr(self.ddp, "active", False) else None

    def epoch_seed(self, epoch: int) -> int:
        """Seed of what validation draws in an epoch: the metric's generator, the ``sample_images`` draws."""
        return int(self.params.get('manual_seed', 0) or 0) * 1_000_003 + int(epoch)

    def _write_record(self, rec: dict, gradients: bool = False):
        """One JSONL line to ``log_file`` (gradients: to ``grad_log_file``), flushed; nothing without the file."""
        file = self.grad_log_file if gradients else self.log_file
        if file is not None:
            file.write(json.dumps(rec) + "\n")
            file.flush()

    def _write_epoch_record(self, rec: dict) -> dict:
        """A validation report's part of the epoch record, also as one JSONL line with the step behind its keys; returns it."""
        self._write_record({**rec, "step": self.global_step})
        return rec

    def sample_images(self, test_batch, epoch: int) -> list:
        """experiment.py:114-150 on one test batch ``(input, labels, *options)``: the input, ``model.generate`` and
        ``model.sample`` grids of this epoch under ``sample_dir`` (module docstring).  Returns the paths written."""
        test_input, test_label, kwargs = unpack_batch(test_batch)
        dev = next(self.model.parameters()).device
        test_input = test_input.to(dev)
        if torch.is_tensor(test_label):
            test_label = test_label.to(dev)
        kwargs = dict(kwargs)
        if isinstance(kwargs.get("mode"), list):
            kwargs["mode"] = kwargs["mode"][0]
        for d in self.SAMPLE_DIRS:
            os.makedirs(os.path.join(self.sample_dir, d), exist_ok=True)

        def path(d, stem):
            return os.path.join(self.sample_dir, d, f"{stem}_{self.run_name}_Epoch_{epoch}.png")

        written = []

        def save(img, p):
            imagegrid.save_image(img, p, normalize=True, nrow=12)
            written.append(p)

        with eval_mode(self.model), seeded_torch_rng(self.epoch_seed(epoch), dev):
            save(test_input, path("Inputs", "inputs"))
            save(self.model.generate(test_input, labels=test_label, **kwargs), path("Reconstructions", "recons"))
            try:
                n = min(32, test_input.size(0))
                labels = test_label[:n] if torch.is_tensor(test_label) else test_label
                save(self.model.sample(n, dev, labels=labels, **kwargs), path("Samples", "sample"))
            except Warning:
                pass
        return written

    def write_graphs(self, stats, epoch: int) -> dict:
        """What ``val_graphs`` leaves of one validation epoch (module docstring): the two sheets under ``sample_dir`` (when there
        is one, and only for groups that had rows) and the ``val_graph_edges_<group>`` scalars, which also go to the JSONL
        log.  One device -> host copy."""
        res = stats.result()
        summary = causalgraph.summarize(res)
        rec = {f"val_graph_edges_{k}": v["edges"] for k, v in summary.items() if v["edges"] is not None}
        if self.sample_dir is not None:
            d = os.path.join(self.sample_dir, self.GRAPH_DIR)
            seen = [g for g in range(stats.G) if res["rows"][g] > 0]
            masked = [g for g in range(1, stats.G) if res["mask_rows"][g] > 0]
            if seen or masked:
                os.makedirs(d, exist_ok=True)
            if seen:
                causalgraph.save_heatmaps(res["adjacency_mean"][seen], os.path.join(d, f"adjacency_{self.run_name}_Epoch_{epoch}.png"))
            if masked and res["hw"] is not None:
                h, w = res["hw"]
                causalgraph.save_heatmaps(res["mask_mean"][masked].reshape(len(masked), -1, w),
                                          os.path.join(d, f"mask_{self.run_name}_Epoch_{epoch}.png"), cell=self.MASK_CELL)
        return self._write_epoch_record(rec) if rec else rec

    def log_all(self, losses: dict, batch_size, validation: bool = False, force: bool = False, step=None):
        """Scalar tensors only (strings are dropped like experiment.py:93-106; the reference logs the 2-D ``ct_adjacency`` /
        ``ct_mask`` batch means as images, here ``val_graphs`` writes them per action instead); one fused all-reduce over
        ranks (sync_dist=True) and one D2H copy.  step: the optimizer step the record is of (None: ``global_step``)."""
        step = self.global_step if step is None else step
        if not force and (step % self.log_every) != 0:
            return None
        prefix = "val_" if validation else ""
        scal = {prefix + k: v for k, v in losses.items()
                if isinstance(v, torch.Tensor) and (v.dim() == 0 or (v.dim() == 1 and v.size(0) == 1))}
        if self.ddp is not None:
            scal = self.ddp.reduce_scalars(scal)
        keys = sorted(scal)
        vals = torch.stack([scal[k].detach().float().reshape(()) for k in keys]).cpu().tolist() if keys else []
        rec = dict(zip(keys, vals))
        if self.kl is not None and not validation:
            rec["kld_weight"] = self.kl.weight(step)      # the host's value of the step that ran: no copy
        rec["step"] = step
        self._write_record(rec)
        return rec

    # -- optimisation (experiment.py:152-187) ---------------------------------------------------------------
    def configure_optimizers(self):
        sl = None
        if "update_parameters" in self.params:
            sl = self.model.flat_range(self.params["update_parameters"])
        opt = FlatAdam(self.model, lr=self.params['LR'], weight_decay=self.params.get('weight_decay', 0.0), params_slice=sl,
                       clip_val=self.gradient_clip_val, clip_algorithm=self.gradient_clip_algorithm,
                       absent_grad=absent_grad_setting(self.params.get("adam_absent_grad")), accumulate=self.accumulate)
        sched = None
        if self.params.get('scheduler_gamma') is not None:
            sched = ExponentialLR(opt, self.params['scheduler_gamma'])
        return opt, sched

    # -- full resume (run.py:85-101: trainer_params.resume_from_checkpoint hands Lightning the optimizer, scheduler, epoch) ------
    def state_dict(self):
        """Everything beside the model's own state_dict that a run needs to continue exactly where it stopped: FlatAdam's
        moments and device state vector (step, lr, betas, eps, weight decay, beta^t), the scheduler's epoch, the global step
        and the random streams (torch CPU / device generators, the in-kernel Philox state of the latent noise).  Plain tensors
        and numbers only, so ``torch.load(..., weights_only=True)`` reads it back."""
        opt = self.optimizer.state_dict()
        sd = {"global_step": int(self.global_step),
              "optimizer": {"exp_avg": opt["exp_avg"].detach().cpu(), "exp_avg_sq": opt["exp_avg_sq"].detach().cpu(),
                            "state": opt["state"][:8].detach().cpu(), "lr": float(self.optimizer.lr),
                            "slice": [int(self.optimizer.slice.start or 0), int(self.optimizer.slice.stop)]},
              "torch_rng": torch.get_rng_state()}
        if "block_state" in opt:           # adam_absent_grad skip modes: per-block step, beta^step and seen flag
            sd["optimizer"].update(absent_grad=opt["absent_grad"], block_state=opt["block_state"].detach().cpu())
        if self.scheduler is not None:
            sd["scheduler"] = {"epoch": int(self.scheduler.epoch), "base_lr": float(self.scheduler.base_lr),
                               "gamma": float(self.scheduler.gamma)}
        dev = next(self.model.parameters()).device
        if dev.type == "cuda":
            sd["device_rng"] = torch.cuda.get_rng_state(dev)
        rng = getattr(self.model, "_rng_state", None)
        if rng is not None:
            sd["model_rng"] = rng.detach().cpu()
        if self.ema is not None:           # (the buffer itself travels as weights: the checkpoint's ema_state_dict, run.py)
            sd["ema"] = self.ema.state_dict(buffer=False)
        if self.codebook is not None:      # (the pool does not travel: the next forward refills it before a restart can read it)
            cb = self.codebook
            sd["codebook"] = {"every": int(self.codebook_every), "min_count": int(self.codebook_min_count),
                              "pool": int(cb.pool.size(0)), "counts": cb.read()[0].clone(), "ordinal": int(self.codebook_ordinal),
                              "restarted": int(self.codebook_restarted),
                              "valid_rows": -1 if cb.valid_rows is None else int(cb.valid_rows)}
        if self.kl is not None:            # (the weight itself is a function of global_step)
            sd["kl"] = self.kl.state_dict()
        if self.codebook_ema is not None:
            sd["codebook_ema"] = self.codebook_ema.state_dict()
        return sd

    def load_state_dict(self, sd):
        """Inverse of state_dict(), in place (captured steps, if any, keep pointing at the same buffers)."""
        if self.kl is not None:            # (a run without the keys ignores the entry)
            why = self.kl.mismatch(sd.get("kl"))
            if why is not None:
                raise RuntimeError(f"{why} (exp_params.kld_schedule / kld_free_bits differ)")
        o = sd["optimizer"]
        if [int(self.optimizer.slice.start or 0), int(self.optimizer.slice.stop)] != [int(v) for v in o["slice"]]:
            raise RuntimeError("checkpoint optimizes another parameter range than this run (update_parameters differs)")
        if o.get("absent_grad", "zero") != self.optimizer.absent_grad:
            raise RuntimeError(f"checkpoint was written under adam_absent_grad={o.get('absent_grad', 'zero')!r}, this run uses "
                               f"{self.optimizer.absent_grad!r} (exp_params.adam_absent_grad differs)")
        self.optimizer.load_state_dict(o)
        self.optimizer.lr = float(o["lr"])
        if self.scheduler is not None and "scheduler" in sd:
            self.scheduler.epoch = int(sd["scheduler"]["epoch"])
            self.scheduler.base_lr = float(sd["scheduler"]["base_lr"])
        self.global_step = int(sd["global_step"])
        torch.set_rng_state(sd["torch_rng"].cpu())
        dev = next(self.model.parameters()).device
        if "device_rng" in sd and dev.type == "cuda":
            torch.cuda.set_rng_state(sd["device_rng"].cpu(), dev)
        if "model_rng" in sd:
            self.model._rng_state = sd["model_rng"].to(dev)
        if self.ema is not None:           # (a run without the key ignores the entry; run.py refuses a checkpoint without it)
            if "ema" not in sd:
                raise RuntimeError("checkpoint holds no weight average (trainer['ema']), this run keeps one (exp_params.ema_decay)")
            self.ema.load_state_dict(sd["ema"])
        if self.codebook is not None:      # (a run without the key ignores the entry)
            self._load_codebook_state(sd.get("codebook"))
        if self.codebook_ema is not None:  # (likewise)
            if "codebook_ema" not in sd:
                raise RuntimeError("checkpoint holds no codebook average (trainer['codebook_ema']), this run keeps one "
                                   "(exp_params.codebook_ema_decay)")
            self.codebook_ema.load_state_dict(sd["codebook_ema"])
            if not self._rank0():          # (the accumulators are rank 0's own rows; the other ranks' share of the window starts over)
                self.codebook_ema.words.zero_()
                self.codebook_ema.acc_s.zero_()
        K.bump_param_epoch()

    def ddp_step(self, pattern=None):
        """Gradient exchange + optimizer step of a data-parallel run (1 / world folded into the step).  In the skip modes the
        step first forms this rank's block flags; their MAX all-reduce goes out from inside the step (``reduce_flags``) with
        the gradient buckets right behind it, so the small collective is under way before the large ones are queued.
        pattern: see FlatAdam.step (a replayed captured step hands over its capture step's).  Under gradient accumulation this
        is the step of the micro-batch that ends a window: the window's sum is finished into the flat gradient buffer before
        the buckets travel, the merged flags before theirs do, and 1 / k joins 1 / world in ``grad_scale``."""
        ddp, opt = self.ddp, self.optimizer
        scale = ddp.grad_scale / self.accumulate
        if opt.absent_grad == "zero":
            if self.accumulate > 1:
                opt.finish_window()
            ddp.all_reduce()
            opt.step(grad_scale=scale)
            return

        def flags_then_grads(flags):
            ddp.all_reduce_flags(flags)
            ddp.all_reduce()

        opt.step(grad_scale=scale, reduce_flags=flags_then_grads, pattern=pattern)

    def window_step(self, ends_window, pattern=None):
        """What follows a micro-batch's backward pass under gradient accumulation (``accumulate`` > 1).  A micro-batch inside
        its window is stashed (``FlatAdam.stash``: no collective, no step).  The one that ends the window steps on (stashed sum
        + its own gradients) / k -- divided by k, not by the window's length, also in an epoch's incomplete last window, as
        Lightning divides every loss by k -- with clipping and weight decay applied once, to that gradient."""
        if not ends_window:
            self.optimizer.stash(pattern)
        elif self.ddp is not None:
            self.ddp_step(pattern)
        else:
            self.optimizer.step(grad_scale=1.0 / self.accumulate, pattern=pattern)

    def finish_batch(self, ends_window=True, pattern=None, stepped=False):
        """What follows every backward pass of training, captured or eager: the stash or the step -- ``window_step`` under
        gradient accumulation, ``ddp_step`` with a gradient exchange, else the plain step; none of them when the captured body
        has ``stepped`` already -- and, where the batch ends its window, the step's tail.  pattern: see ``FlatAdam.step``."""
        if stepped:
            pass
        elif self.accumulate > 1:
            self.window_step(ends_window, pattern)
        elif self.ddp is not None:
            self.ddp_step(pattern)
        else:
            self.optimizer.step()
        if ends_window:
            self._after_optimizer_step()

    def _after_optimizer_step(self):
        """The tail of every optimizer step, eager also behind a replay, in the order the module docstring gives the reasons
        for; ``global_step`` names the step that ran until the last line."""
        self.track_gradients()
        self.codebook_update()
        self.ema_update()
        self.codebook_restart()
        self.global_step += 1

    def optimizer_step(self):
        """One optimizer step on the gradients in the flat buffer (under gradient accumulation: the end of a window)."""
        self.finish_batch()

    # -- gradient tracking (trainer_params.track_grad_norm, exp_params.watch_gradients; optim.GradientTracker) -----
    def _build_tracker(self, track_grad_norm, watch_gradients, watch_log_freq):
        """The tracker of this run, or None: the settings are validated on every rank, the tracker (its tables and output
        buffers) is built on rank 0 only and only when a key is set -- the other ranks launch nothing."""
        norm_type = track_grad_norm_setting(track_grad_norm)
        watch, freq = watch_settings(watch_gradients, watch_log_freq)
        if (norm_type is None and not watch) or not self._rank0():
            return None
        return GradientTracker(self.optimizer, norm_type, watch, freq)

    def track_gradients(self):
        """First in the step's tail (``_after_optimizer_step``).  On a step where a record is due (norms: where the training
        scalars are logged; histograms: every ``watch_log_freq`` steps) rank 0 measures the stepped gradient -- the optimizer's
        slice of the flat buffer times the step's ``grad_scale`` 1 / (world * k) -- and writes ``{"grad_<p>_norm/model.<name>":
        ..., "grad_<p>_norm_total": ..., "lr-Adam": lr, "step": s}`` to the metrics log and ``{"step": s, "gradients/<name>":
        {"min", "max", "counts", "nonfinite"}, ...}`` to the gradient log.  On every other step, and without a tracker, nothing
        is launched or allocated."""
        tr = self.grad_tracker
        if tr is None:
            return
        scale = (self.ddp.grad_scale if self.ddp is not None else 1.0) / self.accumulate
        norms, hists = tr.record(self.global_step, self.log_every, scale)
        if norms is not None:
            self.last_grad_norms = norms = {**norms, "lr-Adam": float(self.optimizer.lr), "step": self.global_step}   # (unrounded)
            self._write_record(norms)
        if hists is not None:
            self.last_grad_hists = hists = {"step": self.global_step, **hists}
            self._write_record(hists, gradients=True)

    # -- weight average (exp_params.ema_decay / ema_warmup / ema_eval; optim.WeightEMA) ------------------------------
    def ema_update(self):
        """In the step's tail: one ``ctvae_ema_update`` launch on every rank, no collective.  Nothing without ``ema_decay``."""
        if self.ema is not None:
            self.ema.update()

    def ema_weights(self):
        """A context inside which the model holds the averaged weights (``WeightEMA.swapped_in``); without a weight average it
        does nothing."""
        return self.ema.swapped_in() if self.ema is not None else contextlib.nullcontext()

    def ema_model_state_dict(self):
        """The model's ``state_dict()`` with the averaged weights in place of the live ones, on the host: a checkpoint's
        ``ema_state_dict`` without its ``model.`` prefix.  Entries outside the optimizer's slice equal the live ones."""
        with self.ema.swapped_in():
            return {k: v.detach().cpu().contiguous() for k, v in self.model.state_dict().items()}

    def load_ema_model_state_dict(self, sd, strict=True):
        """Inverse of ``ema_model_state_dict()``: ``sd`` is read into the average's buffer through the model's own
        ``load_state_dict`` while the average is swapped in; the live weights come back untouched."""
        live = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        with self.ema.swapped_in():
            self.model.load_state_dict(sd, strict=strict)
        self.model.load_state_dict(live)          # (what lies outside the slice -- BatchNorm statistics among it -- stays live)

    # -- codebook usage (exp_params.codebook_stats / codebook_restart_every; optim.CodebookUsage) --------------------
    def _build_codebook_usage(self, params):
        """The usage counters of this run: ``codebook`` (training window, pool and restarts; on every rank) under
        ``codebook_restart_every``, ``val_codebook`` (validation; rank 0 only) under ``codebook_stats``; both None without the
        keys.  Refused by name: either key on a model without a ``vq_layer`` quantiser, and restarts when the codebooks lie
        outside the optimizer's slice (``update_parameters``) -- Adam would never step a restarted code."""
        stats, every, min_count, pool = codebook_settings(params.get("codebook_stats"), params.get("codebook_restart_every"),
                                                          params.get("codebook_restart_min_count"),
                                                          params.get("codebook_restart_pool"))
        self.codebook_stats, self.codebook_every, self.codebook_min_count = stats, every, min_count
        self.codebook = self.val_codebook = None
        self.codebook_ordinal = self.codebook_restarted = 0      # restarts so far (the draw's seed), codes restarted so far
        self.last_codebook_restart = None                        # the record of the last restart (also without a log file)
        if not stats and every is None:
            return
        vq = getattr(self.model, "vq_layer", None)
        if vq is None or not hasattr(vq, "usage_observer"):
            key = "codebook_restart_every" if every is not None else "codebook_stats"
            raise ValueError(f"{key} needs a model with a vq_layer quantiser (MCQVAE, VQVAE, CTMCQVAE), got "
                             f"{type(self.model).__name__}")
        if every is not None:
            self.codebook = CodebookUsage(vq, pool)
            if self.codebook.codebook_offset(self.optimizer) is None:
                raise ValueError(f"codebook_restart_every cannot restart codes the optimizer does not step: update_parameters="
                                 f"{params.get('update_parameters')!r} leaves the codebooks outside the optimizer's slice "
                                 "(codebook_stats stays available)")
        if stats and self._rank0():
            self.val_codebook = CodebookUsage(vq)

    # -- EMA codebooks (exp_params.codebook_ema_decay / codebook_ema_eps; optim.CodebookEMA) ---------------------------
    def _build_codebook_ema(self, params):
        """``codebook_ema`` (on every rank), or None without the key.  Refused by name: a bad value, the key on a model without
        a ``vq_layer`` quantiser, and the key when ``update_parameters`` leaves the codebooks outside the optimizer's slice -- the
        user asked for those weights to stand still, the condition under which restarts are refused.  With the key the
        quantiser's ``ema`` is set for good: the commitment-only loss is a property of the run, validation included."""
        decay, eps = codebook_ema_settings(params.get("codebook_ema_decay"), params.get("codebook_ema_eps"))
        self.codebook_ema = None
        self.last_codebook_ema = None           # the cluster-size record of the last logging step (also without a log file)
        if decay is None:
            return
        if not codebook_ema_serves(self.model):
            raise ValueError(f"codebook_ema_decay needs a model with a vq_layer quantiser (MCQVAE, VQVAE, CTMCQVAE), got "
                             f"{type(self.model).__name__}")
        vq = self.model.vq_layer
        ema = CodebookEMA(vq, decay, eps)
        if codebook_offset(vq, self.optimizer) is None:
            raise ValueError(f"codebook_ema_decay cannot move codebooks the optimizer does not step: update_parameters="
                             f"{params.get('update_parameters')!r} leaves the codebooks outside the optimizer's slice")
        self.codebook_ema = vq.ema = ema

    def codebook_update(self):
        """In the step's tail, in front of ``ema_update()``: [DDP: one SUM all-reduce of the window accumulators,] one
        ``ctvae_vq_ema_update`` launch, a parameter-epoch bump.  On the steps that log training scalars one
        JSONL line ``{"codebook_ema_min_cluster_<i>": min_k N, "codebook_ema_max_cluster_<i>": max_k N, ...,
        "codebook_ema_min_cluster": ..., "codebook_ema_max_cluster": ..., "step": s}`` (rank 0, one device-to-host copy).
        Nothing without ``codebook_ema_decay``."""
        ema = self.codebook_ema
        if ema is None:
            return
        ddp = self._active_ddp()
        ema.update(reduce=ddp.all_reduce_codebook_ema if ddp is not None else None)
        if self.global_step % self.log_every == 0 and self._rank0():
            lo, hi = ema.cluster_sizes()
            rec = {}
            for i in range(ema.C):
                rec[f"codebook_ema_min_cluster_{i}"], rec[f"codebook_ema_max_cluster_{i}"] = lo[i], hi[i]
            rec["codebook_ema_min_cluster"], rec["codebook_ema_max_cluster"] = min(lo), max(hi)
            rec["step"] = self.global_step
            self.last_codebook_ema = rec
            self._write_record(rec)

    @contextlib.contextmanager
    def _counting_training_codes(self):
        """The training counter is the quantiser's ``usage_observer`` inside (around the training batches of ``fit()`` only:
        validation, ``sample_images``, the metrics and the tools count nothing here), and so is ``CodebookEMA.observe`` its
        ``ema_observer``; nothing without restarts and EMA codebooks."""
        if self.codebook is None and self.codebook_ema is None:
            yield
            return
        vq = self.model.vq_layer
        if self.codebook is not None:
            vq.usage_observer = self.codebook.observe
        if self.codebook_ema is not None:      # the EMA statistics are training-only as well (the loss form is the run's)
            vq.ema_observer = self.codebook_ema.observe
        try:
            yield
        finally:
            vq.usage_observer = None
            vq.ema_observer = None

    def codebook_restart(self):
        """Last in the step's tail.  Every ``codebook_restart_every`` optimizer steps: [DDP: one SUM all-reduce of the counts,]
        one device-to-host copy, the dead list, the draw from a CPU generator of its own, the restart launch [DDP: on rank 0's
        rows, one broadcast], a parameter-epoch bump, counts back to zero and one JSONL line ``{"codebook_restarts": n,
        "codebook_restarts_<i>": ..., "codebook_perplexity_<i>": ..., "codebook_usage_<i>": ..., "step": s}`` over the window
        that ended.  On every other step, and without the key, nothing."""
        cb = self.codebook
        if cb is None or (self.global_step + 1) % self.codebook_every != 0:
            return
        ddp = self._active_ddp()
        counts, dead, _ = cb.restart(self.optimizer, self.codebook_min_count, self.params.get("manual_seed", 0), self.codebook_ordinal,
                                     reduce=ddp.all_reduce_counts if ddp is not None else None,
                                     broadcast=ddp.broadcast_rows if ddp is not None else None)
        if self.codebook_ema is not None:      # a restarted code is one observation at its new row
            self.codebook_ema.reset_codes(dead)
        self.codebook_ordinal += 1
        self.codebook_restarted += len(dead)
        rec = {"codebook_restarts": len(dead)}
        for i in range(cb.C):
            rec[f"codebook_restarts_{i}"] = sum(1 for c, _ in dead if c == i)
        rec.update({k: v for k, v in codebook_record(counts, "").items() if "_dead" not in k and k[-1].isdigit()})
        rec["step"] = self.global_step
        self.last_codebook_restart = rec
        if self._rank0():
            self._write_record(rec)

    def write_codebook_stats(self, usage) -> dict:
        """What ``codebook_stats`` leaves of one validation epoch: ``val_codebook_perplexity_<i>`` / ``_usage_<i>`` / ``_dead_<i>``
        per codebook and their unsuffixed means, computed in float64 on the host from one copy of the counts; also one JSONL
        line.  An index outside [0, K) (NaN latents) is reported as ``val_codebook_invalid``."""
        counts, invalid = usage.read()
        rec = codebook_record(counts, "val_")
        if invalid:
            rec["val_codebook_invalid"] = invalid
        return self._write_epoch_record(rec)

    def write_latent_stats(self, latents, epoch: int) -> dict:
        """What ``latent_stats`` leaves of one validation epoch: the ``val_latent_*`` scalars (``latentstats.summarize``, float64 on
        the host from one copy of the accumulators; the undefined ones are left out), also as one JSONL line, and with a
        ``sample_dir`` and at least two rows ``Latents/latent_stats_<name>_Epoch_<e>.npz`` and ``Latents/corr_<name>_Epoch_<e>.png``."""
        res = latents.result()
        rec = latent_record(res)
        if self.sample_dir is not None and "cov" in res:
            d = os.path.join(self.sample_dir, LATENT_DIR)
            os.makedirs(d, exist_ok=True)
            write_latent_files(res, os.path.join(d, f"latent_stats_{self.run_name}_Epoch_{epoch}.npz"),
                               os.path.join(d, f"corr_{self.run_name}_Epoch_{epoch}.png"))
        return self._write_epoch_record(rec)

    def write_prior(self, codes, epoch: int) -> dict:
        """What ``sample_prior`` leaves of one validation epoch.  The rows of ``codes`` (a ``latentprior.CodeBuffer``) with an even
        ordinal are fitted, the rows with an odd ordinal are held out: ``val_prior_mixture_loglik`` and
        ``val_prior_standard_loglik`` are the mean log-likelihoods, in nats, of the finite held-out rows under the mixture and
        under N(0, I) (left out when there is no such row), ``val_prior_iterations``, ``val_prior_rows`` (the finite rows
        fitted) and ``val_prior_nonfinite`` (the non-finite rows of both halves); also one JSONL line, and with a ``sample_dir``
        ``Priors/latent_prior_<name>_Epoch_<e>.npz``.  A refused fit -- too few rows, a covariance that is not positive definite --
        leaves ``val_prior_error``, a string, in place of all that, and the epoch goes on."""
        cfg = self.sample_prior
        X = codes.view()
        fitted, held = X[0::2].contiguous(), X[1::2].contiguous()
        prior = GaussianMixturePrior(codes.D, cfg["components"], cfg["covariance"], cfg["reg_covar"], codes.device)
        self.last_prior = None
        try:
            info = prior.fit(fitted, seed=self.epoch_seed(epoch), max_iter=cfg["max_iter"], tol=cfg["tol"])
        except ValueError as e:
            return self._write_epoch_record({"val_prior_error": str(e)})
        self.last_prior = prior
        rec = {}
        ll, bad = prior.log_prob(held)
        mix = prior.mean_over_finite(ll, bad)
        if mix is not None:
            rec["val_prior_mixture_loglik"] = mix
            rec["val_prior_standard_loglik"] = prior.mean_over_finite(*prior.standard_log_prob(held))
        rec.update(val_prior_iterations=info["iterations"], val_prior_rows=info["rows"],
                   val_prior_nonfinite=info["nonfinite"] + int(bad.sum()))
        if self.sample_dir is not None:
            d = os.path.join(self.sample_dir, PRIOR_DIR)
            os.makedirs(d, exist_ok=True)
            prior.save(os.path.join(d, f"latent_prior_{self.run_name}_Epoch_{epoch}.npz"))
        return self._write_epoch_record(rec)

    def sample_mixture_images(self, n: int, epoch: int):
        """``Samples/sample_mixture_<name>_Epoch_<e>.png`` next to ``sample_images``' prior samples: ``n`` draws from the mixture
        this epoch fitted, decoded.  The draws come from a generator of their own: no other random stream moves.  Returns the
        path, or None when this epoch fitted no mixture."""
        if self.last_prior is None:
            return None
        dev = next(self.model.parameters()).device
        g = torch.Generator(device=dev)
        g.manual_seed(self.epoch_seed(epoch))
        os.makedirs(os.path.join(self.sample_dir, "Samples"), exist_ok=True)
        p = os.path.join(self.sample_dir, "Samples", f"sample_mixture_{self.run_name}_Epoch_{epoch}.png")
        with eval_mode(self.model), torch.no_grad():
            z, _ = self.last_prior.sample(n, g)
            imagegrid.save_image(self.model.decode(z), p, normalize=True, nrow=12)
        return p

    def write_code_prior(self, grids, epoch: int) -> dict:
        """What ``code_prior`` leaves of one validation epoch.  The rows of ``grids`` (a ``codeprior.CodeGridBuffer``) with an even
        ordinal are counted, lambda is fitted on the rows with an odd ordinal, and THOSE rows are reported (the weights have seen
        them; ``fit_code_prior``'s test-split number is the clean one): ``val_code_prior_nats`` (mean nats per code),
        ``val_code_prior_bits``, ``val_code_prior_uniform_nats`` (ln K), ``val_code_prior_nats_<c>`` per codebook,
        ``val_code_prior_weight_<expert>`` (the mean over the codebooks), ``val_code_prior_rows`` (the rows counted) and
        ``val_code_prior_invalid``; also one JSONL line, and with a ``sample_dir`` ``Priors/code_prior_<name>_Epoch_<e>.npz``.  Fewer
        than 2 rows leave ``val_code_prior_error``, a string, in place of all that, and the epoch goes on."""
        cfg = self.code_prior
        X = grids.view()
        self.last_code_prior = None
        if X.size(0) < 2:
            return self._write_epoch_record({"val_code_prior_error": f"a code prior needs at least 2 rows (one to count, one to "
                                                                     f"fit the weights on), got {X.size(0)}"})
        prior = codeprior.MarkovCodePrior(int(self.model.num_embeddings), *grids.shape, grids.device)
        try:
            codeprior.fit_halves(prior, X, cfg["em_iters"], cfg["uniform_floor"])
        except ValueError as e:
            return self._write_epoch_record({"val_code_prior_error": str(e)})
        self.last_code_prior = prior
        rec = codeprior.record(prior.summary(X[1::2].contiguous()), prior.rows, prior.invalid)
        if self.sample_dir is not None:
            d = os.path.join(self.sample_dir, codeprior.CODE_PRIOR_DIR)
            os.makedirs(d, exist_ok=True)
            prior.save(os.path.join(d, f"code_prior_{self.run_name}_Epoch_{epoch}.npz"))
        return self._write_epoch_record(rec)

    def sample_code_prior_images(self, n: int, epoch: int):
        """``Samples/sample_code_prior_<name>_Epoch_<e>.png`` next to ``sample_images``' own samples: ``n`` ancestral draws from the
        prior this epoch fitted, decoded.  The draws come from a generator of their own: no other random stream moves.  Returns
        the path, or None when this epoch fitted no prior."""
        if self.last_code_prior is None:
            return None
        g = torch.Generator(device=self.last_code_prior.device)
        g.manual_seed(self.epoch_seed(epoch))
        os.makedirs(os.path.join(self.sample_dir, "Samples"), exist_ok=True)
        p = os.path.join(self.sample_dir, "Samples", f"sample_code_prior_{self.run_name}_Epoch_{epoch}.png")
        with torch.no_grad():
            inds = self.last_code_prior.sample(n, g)
            imagegrid.save_image(self.last_code_prior.decode_samples(self.model, inds), p, normalize=True, nrow=12)
        return p

    def write_recon_stats(self, accumulators, epoch: int) -> dict:
        """What ``recon_stats`` leaves of one validation epoch: per accumulator one copy, the ``val_recon_*`` scalars
        (``reconstats.summarize``; what has no image to stand on is left out), also as one JSONL line, and with a ``sample_dir`` and
        at least one row ``Recon/recon_stats_<name>[_<mode>]_Epoch_<e>.npz`` and, with a worst set,
        ``Recon/worst_<name>[_<mode>]_Epoch_<e>.png``."""
        rec = {}
        for sfx, acc in accumulators.items():
            res = acc.result()
            rec.update(recon_record(recon_summarize(res["records"], res["flags"], acc.R), suffix=sfx))
            if self.sample_dir is not None and len(res["flags"]):
                d = os.path.join(self.sample_dir, RECON_DIR)
                os.makedirs(d, exist_ok=True)
                write_recon_files(res, os.path.join(d, f"recon_stats_{self.run_name}{sfx}_Epoch_{epoch}.npz"),
                                  os.path.join(d, f"worst_{self.run_name}{sfx}_Epoch_{epoch}.png") if acc.K > 0 else None)
        return self._write_epoch_record(rec)

    def write_loglik(self, acc, epoch: int) -> dict:
        """What ``val_loglik`` leaves of one validation epoch: one copy of the importance sampler's state, finished on the host in
        float64; ``val_loglik`` (mean nats per image), ``val_loglik_elbo``, ``val_loglik_gap``, ``val_loglik_ess`` -- over the images
        without a non-finite log-weight, left out when there is none -- ``val_loglik_rows`` and ``val_loglik_nonfinite``; also one
        JSONL line, and with a ``sample_dir`` and at least one row ``Loglik/loglik_<name>_Epoch_<e>.npz``."""
        res = acc.result()
        rec = loglik.record(loglik.summarize(res, acc.P or 1))
        if self.sample_dir is not None and len(res["nonfinite"]):
            d = os.path.join(self.sample_dir, loglik.LOGLIK_DIR)
            os.makedirs(d, exist_ok=True)
            loglik.write_file(res, os.path.join(d, f"loglik_{self.run_name}_Epoch_{epoch}.npz"))
        return self._write_epoch_record(rec)

    def _load_codebook_state(self, entry):
        """Full resume under ``codebook_restart_every``: the window's counts, the restart ordinal and the total come back, so a
        run resumed inside a window continues bit for bit; other ``every`` / ``min_count`` than the checkpoint's are refused."""
        if entry is None:
            raise RuntimeError("checkpoint holds no codebook usage (trainer['codebook']), this run restarts dead codes "
                               "(exp_params.codebook_restart_every)")
        if int(entry["every"]) != self.codebook_every or int(entry["min_count"]) != self.codebook_min_count:
            raise RuntimeError(f"checkpoint counted its codes under codebook_restart_every={entry['every']!r}, "
                               f"codebook_restart_min_count={entry['min_count']!r}, this run uses {self.codebook_every!r}, "
                               f"{self.codebook_min_count!r}")
        cb = self.codebook
        if tuple(entry["counts"].shape) != tuple(cb.counts.shape):
            raise RuntimeError("checkpoint's codebook counts have another shape than this model's codebooks")
        cb.zero()
        if self._rank0():                  # (the counts are rank 0's own rows; the other ranks' share of the window starts over)
            cb.counts.copy_(entry["counts"])
        valid = int(entry.get("valid_rows", -1))
        cb.valid_rows = None if valid < 0 else min(valid, cb.pool.size(0))
        self.codebook_ordinal, self.codebook_restarted = int(entry["ordinal"]), int(entry["restarted"])

    # -- validation reports: contexts armed around the validation steps, each yielding what writes its part of the epoch record --
    @contextlib.contextmanager
    def _graph_report(self, epoch):
        ct = self.model.ct_layer
        stats = causalgraph.GraphStats(ct.action_dim + 1, causalgraph.model_nodes(self.model), next(self.model.parameters()).device)
        ct.graph_observer = stats.observe
        try:
            yield lambda: self.write_graphs(stats, epoch)
        finally:
            ct.graph_observer = None

    @contextlib.contextmanager
    def _codebook_report(self, epoch):
        self.val_codebook.zero()
        self.model.vq_layer.usage_observer = self.val_codebook.observe
        try:
            yield lambda: self.write_codebook_stats(self.val_codebook)
        finally:
            self.model.vq_layer.usage_observer = None

    @contextlib.contextmanager
    def _observing_results(self, observe):
        """``validation_step`` hands ``observe`` every step's results inside."""
        self._val_observers.append(observe)
        try:
            yield
        finally:
            self._val_observers.remove(observe)

    @contextlib.contextmanager
    def _latent_report(self, epoch):
        self.val_latents.zero()
        with self._observing_results(lambda results: self.val_latents.observe(*self.model.gaussian_posterior(results))):
            yield lambda: self.write_latent_stats(self.val_latents, epoch)

    @contextlib.contextmanager
    def _recon_report(self, epoch):
        for acc in self.val_recon.values():
            acc.reset()

        def observe(results):        # CT-MCQ-VAE feeds the accumulator of the batch's mode, every other model the only one
            pair = self.model.reconstruction_pair(results)
            if pair is not None:
                self.val_recon["" if "" in self.val_recon else "_" + results[4]["mode"]].observe(*pair)

        with self._observing_results(observe):
            yield lambda: self.write_recon_stats(self.val_recon, epoch)

    @contextlib.contextmanager
    def _prior_report(self, epoch):
        """The codes of every validation batch -- views the step already holds -- are copied into the code buffer."""
        self.val_prior.clear()
        g = None
        if self.sample_prior["codes"] == "sample":     # a generator of the report's own: no other random stream moves
            g = torch.Generator(device=self.val_prior.device)
            g.manual_seed(self.epoch_seed(epoch))

        def observe(results):
            self.val_prior.append(draw_codes(*self.model.gaussian_posterior(results), self.sample_prior["codes"], g))

        with self._observing_results(observe):
            yield lambda: self.write_prior(self.val_prior, epoch)

    @contextlib.contextmanager
    def _loglik_report(self, epoch):
        """Every validation batch's images and posteriors -- tensors the step already holds -- feed the importance sampler."""
        acc = self.val_loglik
        acc.reset()
        g = torch.Generator(device=acc.device)         # a generator of the report's own: no other random stream moves
        g.manual_seed(self.epoch_seed(epoch))
        decode = loglik.decoder_of(self.model)

        def observe(results):
            mu, log_var = self.model.gaussian_posterior(results)
            acc.add_batch(loglik.images_for(self.model, results[1]), mu, log_var, decode, g)

        with self._observing_results(observe):
            yield lambda: self.write_loglik(acc, epoch)

    @contextlib.contextmanager
    def _code_prior_report(self, epoch):
        """The indices of every validation search -- a tensor the quantiser already holds -- are copied into the index buffer.
        The observer that is already set (``codebook_stats``') keeps seeing every search, before this one."""
        self.val_code_prior.clear()
        vq = self.model.vq_layer
        before = vq.usage_observer

        def observe(inds, latents):
            if before is not None:
                before(inds, latents)
            self.val_code_prior.append(inds)

        vq.usage_observer = observe
        try:
            yield lambda: self.write_code_prior(self.val_code_prior, epoch)
        finally:
            vq.usage_observer = before

    def _val_reports(self):
        """The reports this run has on this rank, in the order of their keys in the epoch record."""
        reports = ((self._graph_report, self.val_graphs and self._rank0()), (self._codebook_report, self.val_codebook is not None),
                   (self._latent_report, self.val_latents is not None), (self._recon_report, self.val_recon is not None),
                   (self._prior_report, self.val_prior is not None), (self._loglik_report, self.val_loglik is not None),
                   (self._code_prior_report, self.val_code_prior is not None))         # (behind _codebook_report: it chains)
        return [report for report, on in reports if on]

    def _validate(self, epoch, val_batches, test_batches):
        """The validation part of one epoch of ``fit()``: the validation steps' means, what the armed reports write,
        ``validation_metrics`` and ``sample_images``; returns what joins the epoch record."""
        self.model.eval()
        sums, cnt = {}, 0
        with contextlib.ExitStack() as armed:
            writers = [armed.enter_context(report(epoch)) for report in self._val_reports()]
            for i, batch in enumerate(val_batches()):
                r = self.validation_step(batch, i)
                for k, v in r.items():
                    if k != "step":
                        sums[k] = sums.get(k, 0.0) + v
                cnt += 1
        rec = {k: v / max(cnt, 1) for k, v in sums.items()}
        for write in writers:
            rec.update(write())
        rec.update(self.validation_metrics(epoch))
        if self.val_sampling and self.sample_dir is not None and test_batches is not None and self._rank0():
            first = next(iter(test_batches()), None)
            if first is not None:
                self.sample_images(first, epoch)
                if self.val_prior is not None:
                    self.sample_mixture_images(min(32, unpack_batch(first)[0].size(0)), epoch)
                if self.val_code_prior is not None:
                    self.sample_code_prior_images(min(32, unpack_batch(first)[0].size(0)), epoch)
        return rec

    def fit(self, train_batches, val_batches=None, max_epochs=1, on_epoch_end=None, start_epoch=0, test_batches=None):
        """train_batches / val_batches / test_batches: callables returning an iterable of batches for one epoch.  start_epoch:
        first epoch to run (a resumed run continues at the checkpoint's epoch + 1; max_epochs counts from 0 as Lightning's
        does).  test_batches: with ``val_sampling`` and a ``sample_dir``, rank 0 reads its first batch after every validation
        epoch for ``sample_images``."""
        history = []
        for epoch in range(start_epoch, max_epochs):
            self.model.train()
            t0 = time.time()
            k = self.accumulate
            # k > 1: the batch index counts from 0 in every epoch, and the epoch's last batch ends its window whatever its index
            # (one batch of look-ahead: the loader is an iterable) -- no window state crosses an epoch boundary
            stream = ((b, True) for b in train_batches()) if k == 1 else with_window_ends(train_batches(), k)
            with self._counting_training_codes():
                n = self._train_epoch(stream)
            if self.scheduler is not None:
                self.scheduler.step()                      # Lightning steps ExponentialLR once per epoch
            rec = {"epoch": epoch, "train_images": n, "epoch_seconds": time.time() - t0}
            if val_batches is not None:
                # ema_eval: everything validation computes -- losses, graphs, metrics, sample sheets -- sees the averaged weights
                with self.ema_weights() if self.ema_eval else contextlib.nullcontext():
                    rec.update(self._validate(epoch, val_batches, test_batches))
            history.append(rec)
            if on_epoch_end is not None:
                on_epoch_end(epoch, rec)
        return history

    def _train_epoch(self, stream):
        """The training batches of one epoch of ``fit()``: ``stream`` yields (batch, ends_window); returns the images seen."""
        n = 0
        for i, (batch, ends) in enumerate(stream):
            real_img, _labels, kwargs = unpack_batch(batch)
            # graph_safe = False: the model's step depends on host state that changes per call (e.g. BetaVAE type 'B':
            # the capacity C follows the loss-call counter), so a captured step would freeze it
            if getattr(self.model, 'uses_labels', False) and torch.is_tensor(_labels):
                kwargs = {**kwargs, "labels": _labels.to(real_img.device)}      # part of the step's signature and inputs
            key = _graph_key(real_img, kwargs) if (self.params.get('hipgraph', True) and real_img.is_cuda
                                                   and getattr(self.model, 'graph_safe', True)) else None
            if key is not None:
                gs = self._graphed.get(key)
                if gs is None:
                    gs = self._graphed[key] = _GraphedTrainStep(self, real_img, kwargs)
                self.curr_device = real_img.device
                losses = gs.run(real_img, kwargs, ends)
                if ends:                               # the record of the step that just ran: global_step has moved on
                    self.log_all(losses, batch_size=real_img.size(0), validation=False, step=self.global_step - 1)
            else:
                self.model.zero_grad(lazy=True)
                self._log_train = ends                 # a record per optimizer step, with the losses of its last micro-batch
                try:
                    loss = self.training_step(batch, i)
                finally:
                    self._log_train = True
                K.backward(loss)
                self.model.settle_grads()
                self.finish_batch(ends)
            n += batch[0].size(0)
        return n
