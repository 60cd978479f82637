"""Entry point mirroring the reference's ``run.py`` (run.py:21-110): ``python -m ctvae_amd.run -c configs/vae.yaml``.

Consumes the reference's YAML layout unchanged (model_params / data_params / exp_params / trainer_params /
logging_params; ``model_params`` is splatted into ``vae_models[name]``), with the tolerances of SURVEY N4:
``find_unused_parameters`` optional, ``gpus`` int or list, ``dataset_name`` defaults to a synthetic source.
One process per GPU (launch with ``python -m torch.distributed.run``); Lightning / wandb are not required.
Checkpoints: top-k on ``val_Reconstruction_Loss`` + ``last.ckpt`` with ``state_dict`` keys prefixed ``model.``
so they interchange with the reference's (run.py:85-97), plus a ``trainer`` entry (optimizer moments, scheduler, epoch, global
step, random streams) for ``trainer_params.resume_from_checkpoint`` without ``load_weights_only`` (run.py:85-101: full resume).
``trainer_params.gradient_clip_val`` / ``gradient_clip_algorithm`` clip the gradients before every optimizer step as the
Lightning Trainer does (configs/gammavae.yaml); without them the step is unchanged.
``trainer_params.accumulate_grad_batches: k`` (an integer >= 1; Lightning's ``{epoch: k}`` schedule is refused) steps the
optimizer once per window of k batches on the window's gradient sum / k (experiment.py, optim.py); absent or 1 changes nothing.
``exp_params.metrics`` (run.py:64-76; "MIG", "FactorVaeScore") with ``data_params.hbm_factor_sizes`` (the sizes of the
ground-truth factor grid the ``hbm_images`` rows enumerate row-major) adds the disentanglement metrics to every validation epoch.
``exp_params.val_sampling: true`` (the reference's run.py hard-wires it on; here it defaults to false) writes the input,
reconstruction and sample PNG grids of the first test batch after every validation epoch into ``Inputs/``, ``Reconstructions/``
and ``Samples/`` of the run's log directory, named after ``logging_params.name`` (experiment.py: ``sample_images``).
``exp_params.val_graphs: true`` (CT-MCQ-VAE only) writes the mean learned adjacency per action and the mean intervention mask
per action after every validation epoch into ``Graphs/`` of the log directory and adds ``val_graph_edges_<group>`` to the epoch
records (experiment.py: ``val_graphs``); with several ranks they show rank 0's own validation rows.
``trainer_params.track_grad_norm`` (Lightning's flag: a number > 0 or 'inf' is the norm type, -1 or absent is off; a bool, 0 or
anything else is refused by name) adds one line ``{"grad_<p>_norm/model.<name>": ..., "grad_<p>_norm_total": ..., "lr-Adam": lr,
"step": s}`` to ``metrics_rank0.jsonl`` on every step whose training scalars are logged (the reference's ``LearningRateMonitor``
rides along as ``lr-Adam``).  ``exp_params.watch_gradients: true`` (the reference's run.py:55 hard-wires
``wb_logger.watch(model, log_freq=500)``; here it defaults to false) with ``exp_params.watch_log_freq`` (an integer >= 1, default
500) writes one line of 64-bin per-parameter gradient histograms to ``gradients_rank0.jsonl`` every ``watch_log_freq`` optimizer
steps.  Both read the gradient that is stepped, from the flat buffer, by HIP kernels (optim.py: ``GradientTracker``); without
the keys no file, no key and no launch is added.
``exp_params.ema_decay`` (a float, 0 < d < 1) with ``ema_warmup`` (default false) and ``ema_eval`` (default true) keeps an
exponential moving average of the optimized weights and, under ``ema_eval``, validates with it -- so the top-k choice on
``val_Reconstruction_Loss`` is made on the averaged weights (experiment.py, optim.py: ``WeightEMA``).  ``state_dict`` stays the live
weights; the checkpoint gains ``ema_state_dict`` (the same keys, the averaged weights) and ``trainer['ema']``.  A full resume under
the key needs both, written under the same decay and warm-up; ``load_weights_only`` starts the average from the loaded weights; a
run without the key ignores them.  A refused value is a SystemExit that names ``exp_params.<key>``.
``exp_params.codebook_stats: true`` adds per-codebook usage statistics (``val_codebook_perplexity_<i>`` / ``_usage_<i>`` /
``_dead_<i>`` and their means) to every validation epoch of a quantising model (MCQVAE, VQVAE, CTMCQVAE);
``exp_params.codebook_restart_every: N`` (with ``codebook_restart_min_count``, default 1, and ``codebook_restart_pool``, default
1024) counts usage during training and every N optimizer steps overwrites the codes chosen fewer than ``min_count`` times with
encoder outputs of the last batch, zeroing their Adam moments (experiment.py, optim.py: ``CodebookUsage``).  The checkpoint
gains ``trainer['codebook']``; a full resume under the key continues the window bit for bit and refuses other ``every`` /
``min_count``; ``load_weights_only`` starts a fresh window; a run without the key ignores the entry.  Restarts are refused when
``update_parameters`` leaves the codebooks outside the optimizer's slice.
``exp_params.codebook_ema_decay: g`` (a float, 0 < g < 1; with ``codebook_ema_eps``, default 1e-5) trains the codebooks of a
quantising model by the exponential-moving-average update of van den Oord et al. 2017, appendix A.1, instead of the optimizer
(experiment.py, optim.py: ``CodebookEMA``): ``VQ_Loss`` becomes the commitment term alone, training records gain
``codebook_ema_min_cluster_<i>`` / ``codebook_ema_max_cluster_<i>``, and the checkpoint gains ``trainer['codebook_ema']``; a full
resume under the key continues bit for bit and refuses another decay or eps, ``load_weights_only`` starts from the loaded
codebooks, a run without the key ignores the entry.  Refused like the restarts under ``update_parameters``; a refused value or
model is a SystemExit that names ``exp_params.codebook_ema_decay`` / ``codebook_ema_eps``.
``exp_params.latent_stats: true`` adds the latent usage of a model with a Gaussian posterior to every validation epoch:
``val_latent_kl_total`` / ``_active_units`` / ``_collapsed`` / ``_mean_abs_corr`` / ``_gaussian_tc`` / ``_nonfinite`` / ``_rows`` in the
epoch records and ``metrics_rank0.jsonl``, and ``Latents/latent_stats_<name>_Epoch_<e>.npz`` (per-dimension KL, mean, variance and
covariance of the posterior means) with ``Latents/corr_<name>_Epoch_<e>.png`` in the log directory (experiment.py,
latentstats.py); ``python -m ctvae_amd.latent_stats`` does the same for a checkpoint and adds the traversal picture.  Anything but
a bool, and the key on a model without such a posterior, is a SystemExit that names it.
``exp_params.kld_schedule`` anneals the KL weight over the optimizer steps s -- ``{type: linear, warmup_steps: N, start: a}``:
``kld_weight * (a + (1 - a) * min(1, s / N))``; ``{type: cyclical, cycle_steps: M, ratio: r, cycles: n}``: ``kld_weight * min(1,
((s mod M) / M) / r)``, constant ``kld_weight`` from step n * M on (``cycles`` absent: for ever) -- and ``exp_params.kld_free_bits:
lambda`` (nats per latent dimension, >= 0) floors the batch-mean KL of every dimension at lambda, switching off the KL gradient
of the dimensions under it (klcontrol.py, experiment.py).  They serve VanillaVAE and its aliases, TwoStageVAE, ConditionalVAE,
MSSIMVAE, LogCoshVAE and BetaVAE with ``loss_type: 'H'``; the training records gain ``kld_weight``, ``KLD_free_bits`` and
``KLD_floored_dims``, validation is unchanged, and the checkpoint gains ``trainer['kl']``: a full resume under other settings is
refused, ``load_weights_only`` starts the schedule at step 0, a run without the keys ignores the entry.  A refused value or model
is a SystemExit that names ``exp_params.kld_schedule`` or ``exp_params.kld_free_bits``.
``exp_params.sample_prior: {type: gmm}`` (with ``components``, 1..64, default 10; ``covariance``, full | diag; ``max_iter``, default 50;
``tol``, default 1e-3; ``reg_covar``, default 1e-6; ``codes``, mean | sample) fits a Gaussian-mixture prior to the validation codes of
every validation epoch (experiment.py, latentprior.py): ``val_prior_mixture_loglik`` / ``_standard_loglik`` / ``_iterations`` /
``_rows`` / ``_nonfinite`` in the epoch records and ``metrics_rank0.jsonl``, ``Priors/latent_prior_<name>_Epoch_<e>.npz`` and, with
``val_sampling``, ``Samples/sample_mixture_<name>_Epoch_<e>.png`` in the log directory; ``python -m ctvae_amd.fit_prior`` does the same
for a checkpoint over the training split.  A refused value or model is a SystemExit that names ``exp_params.sample_prior``.
``exp_params.code_prior: {type: markov}`` (with ``em_iters``, an int >= 1, default 20, and ``uniform_floor``, a float inside (0, 1),
default 1e-3) fits an interpolated Markov prior to the validation code grids of MCQVAE / VQVAE in every validation epoch
(experiment.py, codeprior.py): ``val_code_prior_nats`` / ``_bits`` / ``_uniform_nats`` / ``_nats_<c>`` / ``_weight_<expert>`` / ``_rows`` /
``_invalid`` in the epoch records and ``metrics_rank0.jsonl``, ``Priors/code_prior_<name>_Epoch_<e>.npz`` and, with ``val_sampling``,
``Samples/sample_code_prior_<name>_Epoch_<e>.png`` in the log directory; ``python -m ctvae_amd.fit_code_prior`` does the same for a
checkpoint over the training split and scores the test split.  A refused value or model is a SystemExit that names
``exp_params.code_prior``.
``exp_params.recon_stats: true`` (with ``recon_stats_range``, the data range R of the pictures, a float > 0, default 1.0, and
``recon_stats_worst``, an integer 0 <= K <= 32, default 8) adds the reconstruction quality per validation image to every validation
epoch: ``val_recon_psnr`` / ``_ssim`` / ``_mae`` / ``_max_err``, the 5th percentiles and minima ``_psnr_p05`` / ``_ssim_p05`` / ``_psnr_min``
/ ``_ssim_min`` and the counts ``_rows`` / ``_nonfinite`` / ``_exact`` in the epoch records and ``metrics_rank0.jsonl``, and
``Recon/recon_stats_<name>_Epoch_<e>.npz`` (the per-image values) with ``Recon/worst_<name>_Epoch_<e>.png`` (the K worst targets over
their reconstructions) in the log directory (experiment.py, reconstats.py); CT-MCQ-VAE reports its base and action batches apart,
under ``_base`` / ``_action``.  ``python -m ctvae_amd.recon_stats`` does the same for a checkpoint.  The top-k checkpoints are still
chosen by ``val_Reconstruction_Loss``.  A bad value, a dependent key without ``recon_stats``, and IWAE / MIWAE are a SystemExit
that names ``exp_params.recon_stats`` (or the dependent key).
``exp_params.val_loglik: {samples: K, sigma: s}`` (``samples`` an int, 1..4096; ``sigma`` a float > 0, the observation model
N(decode(z), sigma^2 I); optionally ``chunk``, an int in 1..K, default min(K, 64)) estimates the marginal log-likelihood of every
validation image by importance sampling, K draws from its posterior (the IWAE bound; experiment.py, loglik.py, csrc/loglik.hip):
``val_loglik`` (mean nats per image), ``val_loglik_elbo``, ``val_loglik_gap``, ``val_loglik_ess``, ``val_loglik_rows`` and
``val_loglik_nonfinite`` in the epoch records and ``metrics_rank0.jsonl``, and ``Loglik/loglik_<name>_Epoch_<e>.npz`` (the per-image
values) in the log directory.  It serves ``loglik.LOGLIK_MODELS``; ``python -m ctvae_amd.log_likelihood`` does the same for a
checkpoint over the test split with up to 65536 samples, and alone knows ``sigma: mse``.  A refused value or model is a SystemExit
that names ``exp_params.val_loglik``.
"""
import argparse
import json
import os

import torch
import torch.distributed as dist
import yaml

from . import filler
from .ddp import GradBucketAllReduce
from .experiment import VAEXperiment
from .models import vae_models
from .optim import accumulate_setting, codebook_settings, ema_settings, track_grad_norm_setting, watch_settings


class SyntheticData:
    """Synthetic stand-in for dataset.py's VAEDataset with the reference's batch contracts: plain datasets
    yield (X, labels); T-datasets yield (X, labels, {"action", "input_y", "mode"}) with one mode per batch."""

    def __init__(self, data_params, model_params, device, rank=0, world=1, steps_per_epoch=8, seed=0):
        self.p, self.mp, self.dev, self.rank, self.world = data_params, model_params, device, rank, world
        self.steps, self.seed = steps_per_epoch, seed
        name = data_params.get("dataset_name", "synthetic")
        self.transition = name.startswith("T")
        self.action_dim = model_params.get("action_dim", 12)

    def _batches(self, bs, base_seed):
        img = self.p.get("patch_size", 64)
        for i in range(self.steps):
            s = base_seed + 7919 * i + 104729 * self.rank          # each rank takes its own rows of the global batch
            if self.transition:
                x, y, a = filler.synthetic_pairs(s, bs, self.action_dim, img)
                mode = ["base", "action", "causal"][i % 3]
                opts = {"mode": [mode] * bs}
                if mode != "base":
                    opts.update({"action": a.to(self.dev), "input_y": y.to(self.dev)})
                yield (x.to(self.dev), torch.zeros(bs, device=self.dev), opts)
            else:
                x, _ = filler.synthetic_batch(s, bs, img=img)
                yield (x.to(self.dev), torch.zeros(bs, device=self.dev))

    def train(self):
        return self._batches(self.p["train_batch_size"], self.seed)

    def val(self):
        return self._batches(self.p["val_batch_size"], self.seed + 1_000_003)

    def test(self):
        """dataset.py:145-166: batches of the validation kind at val_batch_size (their own draws)."""
        return self._batches(self.p["val_batch_size"], self.seed + 2_000_003)


class HbmData:
    """Real data, resident in HBM (ctvae_amd.data): ``data_params.hbm_images`` names a ``.npy`` uint8 array [N,H,W,3] (the
    decoded dataset, converted once); ``hbm_names`` optionally a text file with one item name per row (default: the row
    number, which is what the disent datasets use, disent_dataset.py:56).  Splits come from
    ``<data_path>/<folder>/list_eval_partition.txt`` (row id, item index, split code; disent_dataset.py:70-80) when it
    exists.  ``T*`` datasets read ``<data_path>/<folder>/variation_attrs_<V>.txt`` (transition.py:111-125) with
    V = action_dim / 2 and yield mode-pure (x, labels, options) batches; others yield (x, labels).  Train batches are
    shuffled and sharded over the ranks; validation uses split ``test`` like dataset.py:88-93."""

    FOLDERS = {"TCeleba": "celeba", "TShapes3D": "3dshapes", "TCars3D": "cars3d", "TDSprites": "dsprites",
               "TSmallNORB": "smallnorb", "TSprites": "sprites"}

    def __init__(self, data_params, model_params, device, rank=0, world=1, seed=0):
        import numpy as np
        from . import data as D
        self.D, self.p, self.dev, self.rank, self.world, self.seed = D, data_params, device, rank, world, seed
        name = data_params.get("dataset_name", "")
        self.transition = name.startswith("T")
        self.folder = os.path.join(data_params.get("data_path", "."), self.FOLDERS.get(name, name.lower().lstrip("t")))
        imgs = torch.from_numpy(np.load(data_params["hbm_images"], mmap_mode="c", allow_pickle=False))
        self.store = D.HbmImageStore(imgs, device, crop=data_params.get("crop_size", 148), size=data_params.get("patch_size", 64))
        if data_params.get("hbm_names"):
            all_names = [l.strip() for l in open(data_params["hbm_names"]) if l.strip()]
        else:
            all_names = [str(i) for i in range(len(self.store))]
        part = os.path.join(self.folder, "list_eval_partition.txt")
        self.split_rows = {}
        if os.path.exists(part):
            import csv
            rows = list(csv.reader(open(part)))[1:]
            for code, split in ((0, "train"), (1, "valid"), (2, "test")):
                self.split_rows[split] = [int(r[1]) for r in rows if int(r[2]) == code]
        else:
            self.split_rows = {s: list(range(len(all_names))) for s in ("train", "valid", "test")}
        self.all_names = all_names
        self.V = int(model_params.get("action_dim", 12)) // 2
        self.epoch = 0

    def _loader(self, split, batch_size, shuffle):
        D = self.D
        rows = torch.tensor(self.split_rows[split], dtype=torch.int64)
        names = [self.all_names[i] for i in self.split_rows[split]]
        store = self.store
        if self.transition:
            table = D.TransitionTable(os.path.join(self.folder, f"variation_attrs_{self.V}.txt"), names, self.V, split)
            sampler = D.TransitionBatchSampler(table, batch_size, shuffle=shuffle, drop_last=True, limit=self.p.get("limit"),
                                               rank=self.rank, world=self.world, seed=self.seed)
            sampler.set_epoch(self.epoch)
            rows_dev = rows.to(self.dev)
            for batch in sampler:
                mode, xr, yr, act = table.resolve_batch(batch)
                x = store.fetch(rows_dev[xr.to(self.dev)])
                opts = {"mode": [mode] * len(batch)}
                if mode != "base":
                    opts.update({"input_y": store.fetch(rows_dev[yr.to(self.dev)]), "action": act.to(self.dev)})
                yield x, torch.zeros(len(batch), device=self.dev), opts
        else:
            g = torch.Generator().manual_seed(self.seed + 7919 * (self.epoch + 1))
            order = rows[torch.randperm(len(rows), generator=g)] if shuffle else rows
            order = D.shard_rows(order, self.rank, self.world)      # same number of batches on every rank
            for i in range(0, len(order), batch_size):
                r = order[i:i + batch_size]
                yield store.fetch(r), torch.zeros(len(r), device=self.dev)

    def train(self):
        self.epoch += 1
        return self._loader("train", self.p["train_batch_size"], True)

    def val(self):
        return self._loader("test", self.p["val_batch_size"], False)

    def test(self):
        """dataset.py:145-166: the validation split again at val_batch_size, shuffled; T-datasets mode-pure with drop_last."""
        return self._loader("test", self.p["val_batch_size"], True)


def model_weights(state: dict) -> dict:
    """A checkpoint's ``state_dict`` / ``ema_state_dict`` (keys ``model.<name>``, as ``on_epoch_end`` writes them) as the model's own."""
    return {k[6:]: v for k, v in state.items() if k.startswith("model.")}


def build_val_metric(config, data):
    """``exp_params.metrics`` -> a MetricSet over the whole store (the reference hands it ``_full_data``), sized as run.py:72-76;
    None without the key.  A metric that cannot run is a SystemExit with the reason."""
    names = config['exp_params'].get('metrics')
    if not names:
        return None
    from . import metrics as M
    dp = config['data_params']
    if not isinstance(data, HbmData):
        raise SystemExit("exp_params.metrics needs ground-truth factors: synthetic data has none (set data_params.hbm_images)")
    if not dp.get('hbm_factor_sizes'):
        raise SystemExit("exp_params.metrics needs data_params.hbm_factor_sizes (the sizes of the factor grid hbm_images enumerates)")
    try:
        dataset = M.FactorData(data.store, M.FactorGrid(dp['hbm_factor_sizes']))
        return M.MetricSet(list(names), dataset, batch_size=dp['val_batch_size'], num_train=dp['train_batch_size'] * 20,
                           num_test=dp['train_batch_size'] * 10, seed=config['exp_params'].get('manual_seed', 0) or 0)
    except ValueError as e:
        raise SystemExit(f"exp_params.metrics: {e}")


def trainer_accumulate(trainer_params) -> int:
    """``trainer_params.accumulate_grad_batches`` as the k of VAEXperiment (absent: 1); a value that is not an integer >= 1
    -- a bool, a float, Lightning's ``{epoch: k}`` schedule -- is a SystemExit that names the key."""
    try:
        return accumulate_setting(trainer_params.get('accumulate_grad_batches'))
    except ValueError as e:
        raise SystemExit(f"trainer_params.{e}")


def trainer_track_grad_norm(trainer_params):
    """``trainer_params.track_grad_norm`` as VAEXperiment's norm type (None: off); a refused value is a SystemExit that names
    the key."""
    try:
        return track_grad_norm_setting(trainer_params.get('track_grad_norm'))
    except ValueError as e:
        raise SystemExit(f"trainer_params.{e}")


def exp_watch_gradients(exp_params):
    """``exp_params.watch_gradients`` / ``watch_log_freq`` as ``(watch, log_freq)``; a refused value is a SystemExit that names
    the key."""
    try:
        return watch_settings(exp_params.get('watch_gradients'), exp_params.get('watch_log_freq'))
    except ValueError as e:
        raise SystemExit(f"exp_params.{e}")


def exp_ema(exp_params):
    """``exp_params.ema_decay`` / ``ema_warmup`` / ``ema_eval`` as ``(decay, warmup, eval)`` (decay None: off); a refused value is
    a SystemExit that names the key."""
    try:
        return ema_settings(exp_params.get('ema_decay'), exp_params.get('ema_warmup'), exp_params.get('ema_eval'))
    except ValueError as e:
        raise SystemExit(f"exp_params.{e}")


def check_ema_checkpoint(ckpt, path, decay, warmup):
    """Full resume of a run that keeps a weight average: the checkpoint must hold the average (``ema_state_dict``) and its
    settings (``trainer['ema']``), written under this run's decay and warm-up; otherwise a SystemExit names the key and the path."""
    ema = ckpt.get("trainer", {}).get("ema")
    if "ema_state_dict" not in ckpt or ema is None:
        raise SystemExit(f"exp_params.ema_decay is set, but {path} holds no weight average (no 'ema_state_dict' / trainer['ema']): "
                         "it was written by a run without the key; set trainer_params.load_weights_only to start the average "
                         "from its weights")
    if float(ema["decay"]) != decay or bool(ema["warmup"]) != warmup:
        raise SystemExit(f"exp_params.ema_decay / ema_warmup are {decay!r} / {warmup!r}, but {path} kept its weight average under "
                         f"{ema['decay']!r} / {ema['warmup']!r}")


VQ_MODELS = ("MCQVAE", "VQVAE", "CTMCQVAE")        # the served models with a ``vq_layer`` quantiser


def exp_codebook(config):
    """``exp_params.codebook_stats`` / ``codebook_restart_every`` / ``codebook_restart_min_count`` / ``codebook_restart_pool`` as
    ``(stats, every, min_count, pool)`` (every None: no restarts).  A refused value, either feature on a model that does not
    quantise, and restarts under an ``update_parameters`` other than ``vq_layer`` (the optimizer would not step the codebooks) are
    a SystemExit that names the key."""
    ep = config['exp_params']
    try:
        stats, every, min_count, pool = codebook_settings(ep.get('codebook_stats'), ep.get('codebook_restart_every'),
                                                          ep.get('codebook_restart_min_count'), ep.get('codebook_restart_pool'))
    except ValueError as e:
        raise SystemExit(f"exp_params.{e}")
    name = config['model_params'].get('name')
    if (stats or every is not None) and name not in VQ_MODELS:
        key = 'codebook_restart_every' if every is not None else 'codebook_stats'
        raise SystemExit(f"exp_params.{key} needs a model with a vq_layer quantiser ({', '.join(VQ_MODELS)}), model_params.name "
                         f"is {name!r}")
    if every is not None and ep.get('update_parameters') not in (None, 'vq_layer'):
        raise SystemExit(f"exp_params.codebook_restart_every cannot restart codes the optimizer does not step: "
                         f"exp_params.update_parameters is {ep.get('update_parameters')!r} (codebook_stats stays available)")
    return stats, every, min_count, pool


def exp_codebook_ema(config):
    """``exp_params.codebook_ema_decay`` / ``codebook_ema_eps`` as ``(decay, eps)``, rounded to fp32 (decay None: off).  A refused
    value, the key on a model that does not quantise, and the key under an ``update_parameters`` other than ``vq_layer`` (the user
    asked for the codebooks to stand still) are a SystemExit that names the key."""
    from .optim import codebook_ema_settings
    ep = config['exp_params']
    try:
        decay, eps = codebook_ema_settings(ep.get('codebook_ema_decay'), ep.get('codebook_ema_eps'))
    except ValueError as e:
        raise SystemExit(f"exp_params.{e}")
    if decay is None:
        return None, None
    name = config['model_params'].get('name')
    if name not in VQ_MODELS:
        raise SystemExit(f"exp_params.codebook_ema_decay needs a model with a vq_layer quantiser ({', '.join(VQ_MODELS)}), "
                         f"model_params.name is {name!r}")
    if ep.get('update_parameters') not in (None, 'vq_layer'):
        raise SystemExit(f"exp_params.codebook_ema_decay cannot move codebooks the optimizer does not step: "
                         f"exp_params.update_parameters is {ep.get('update_parameters')!r}")
    return decay, eps


def check_codebook_ema_checkpoint(ckpt, path, decay, eps):
    """Full resume of a run with EMA codebooks: the checkpoint must hold ``trainer['codebook_ema']``, written under this run's
    decay and eps; otherwise a SystemExit names the key and the path."""
    entry = ckpt.get("trainer", {}).get("codebook_ema")
    if entry is None:
        raise SystemExit(f"exp_params.codebook_ema_decay is set, but {path} holds no codebook average (no trainer['codebook_ema']): "
                         "it was written by a run without the key; set trainer_params.load_weights_only to start the average "
                         "from its weights")
    if float(entry["decay"]) != decay:
        raise SystemExit(f"exp_params.codebook_ema_decay is {decay!r}, but {path} kept its codebook average under "
                         f"{entry['decay']!r}")
    if float(entry["eps"]) != eps:
        raise SystemExit(f"exp_params.codebook_ema_eps is {eps!r}, but {path} kept its codebook average under {entry['eps']!r}")


def exp_latent_stats(config) -> bool:
    """``exp_params.latent_stats`` as a bool (absent: False).  Anything but a bool, and the key on a model without a Gaussian
    posterior, are a SystemExit that names the key."""
    from . import latentstats
    try:
        on = latentstats.latent_stats_setting(config['exp_params'].get('latent_stats'))
    except ValueError as e:
        raise SystemExit(f"exp_params.{e}")
    name = config['model_params'].get('name')
    cls = vae_models.get(name)
    if on and (cls is None or not latentstats.has_gaussian_posterior(cls)):
        raise SystemExit(f"exp_params.{latentstats.needs_gaussian_posterior(cls, name=repr(name))} (model_params.name)")
    return on


def exp_sample_prior(config):
    """``exp_params.sample_prior`` as None (absent: off) or the complete mapping (``latentprior.prior_setting``).  A refused value
    and a model the mixture does not serve are a SystemExit that names the key."""
    from . import latentprior
    try:
        cfg = latentprior.prior_setting(config['exp_params'].get('sample_prior'))
    except ValueError as e:
        raise SystemExit(f"exp_params.{e}")
    name = config['model_params'].get('name')
    cls = vae_models.get(name)
    if cfg is not None and (cls is None or not latentprior.prior_supported(cls)):
        raise SystemExit(f"exp_params.{latentprior.needs_supported_model(cls, name=repr(name))} (model_params.name)")
    return cfg


def exp_code_prior(config):
    """``exp_params.code_prior`` as None (absent: off) or the complete mapping (``codeprior.code_prior_setting``).  A refused value
    and a model the prior does not serve are a SystemExit that names the key."""
    from . import codeprior
    try:
        cfg = codeprior.code_prior_setting(config['exp_params'].get('code_prior'))
    except ValueError as e:
        raise SystemExit(f"exp_params.{e}")
    name = config['model_params'].get('name')
    cls = vae_models.get(name)
    if cfg is not None and (cls is None or not codeprior.prior_supported(cls)):
        raise SystemExit(f"exp_params.{codeprior.needs_supported_model(cls, name=repr(name))} (model_params.name)")
    return cfg


def exp_val_loglik(config):
    """``exp_params.val_loglik`` as None (absent: off) or the complete mapping (``loglik.loglik_setting``).  A refused value and a
    model the estimate does not serve are a SystemExit that names the key."""
    from . import loglik
    try:
        cfg = loglik.loglik_setting(config['exp_params'].get('val_loglik'))
    except ValueError as e:
        raise SystemExit(f"exp_params.{e}")
    name = config['model_params'].get('name')
    cls = vae_models.get(name)
    if cfg is not None and (cls is None or not loglik.loglik_supported(cls)):
        raise SystemExit(f"exp_params.val_loglik: {loglik.needs_supported_model(cls, name=repr(name))} (model_params.name)")
    return cfg


def exp_recon_stats(config) -> tuple:
    """``exp_params.recon_stats`` / ``recon_stats_range`` / ``recon_stats_worst`` as ``(on, R, K)``.  A refused value, a dependent key
    without the main one, and a model that hands out several reconstructions per image (IWAE, MIWAE) are a SystemExit that
    names the key."""
    from . import reconstats
    try:
        on, R, K = reconstats.recon_settings(config['exp_params'])
    except ValueError as e:
        raise SystemExit(f"exp_params.{e}")
    name = config['model_params'].get('name')
    cls = vae_models.get(name)
    if on:
        why = f"recon_stats: model_params.name {name!r} is not a model" if cls is None else reconstats.refuses_model(cls, name=repr(name))
        if why is not None:
            raise SystemExit(f"exp_params.{why} (model_params.name)")
    return on, R, K


def exp_kl(config):
    """``exp_params.kld_schedule`` / ``kld_free_bits`` as ``(schedule, free_bits)`` (both None: off).  A refused value, and either key
    on a model whose loss is not recon + c * M_N * KL (BetaVAE's default ``loss_type: 'B'`` among them), are a SystemExit that
    names the key."""
    from . import klcontrol
    ep = config['exp_params']
    try:
        schedule, free_bits = klcontrol.kl_settings(ep)
    except ValueError as e:
        raise SystemExit(f"exp_params.{e}")
    if schedule is None and free_bits is None:
        return None, None
    mp = config['model_params']
    name = mp.get('name')
    cls = vae_models.get(name)
    if cls is None or not klcontrol.serves(cls, loss_type=mp.get('loss_type', 'B')):
        key = 'kld_schedule' if schedule is not None else 'kld_free_bits'
        what = repr(name) + (f" with loss_type {mp.get('loss_type', 'B')!r}" if cls is not None and cls.__name__ == "BetaVAE" else "")
        raise SystemExit(f"exp_params.{klcontrol.needs_served_model(key, what)} (model_params.name)")
    return schedule, free_bits


def check_kl_checkpoint(ckpt, path, schedule, free_bits):
    """Full resume of a run under ``kld_schedule`` / ``kld_free_bits``: the checkpoint must hold ``trainer['kl']``, written under the
    same settings; otherwise a SystemExit names the key and the path."""
    from . import klcontrol
    why = klcontrol.KLControl(schedule, free_bits, 0.0, "cpu").mismatch(ckpt.get("trainer", {}).get("kl"))
    if why is not None:
        raise SystemExit(f"exp_params.kld_schedule / kld_free_bits: {why} ({path}); set trainer_params.load_weights_only to start at "
                         "step 0 from its weights")


def check_codebook_checkpoint(ckpt, path, every, min_count):
    """Full resume of a run that restarts dead codes: the checkpoint must hold ``trainer['codebook']``, written under this run's
    ``every`` and ``min_count``; otherwise a SystemExit names the key and the path."""
    entry = ckpt.get("trainer", {}).get("codebook")
    if entry is None:
        raise SystemExit(f"exp_params.codebook_restart_every is set, but {path} holds no codebook usage (no trainer['codebook']): "
                         "it was written by a run without the key; set trainer_params.load_weights_only to start a fresh window "
                         "from its weights")
    if int(entry["every"]) != every or int(entry["min_count"]) != min_count:
        raise SystemExit(f"exp_params.codebook_restart_every / codebook_restart_min_count are {every!r} / {min_count!r}, but {path} "
                         f"counted its codes under {entry['every']!r} / {entry['min_count']!r}")


def main(argv=None):
    ap = argparse.ArgumentParser(description='MI355X runner for the ct-vae models')
    ap.add_argument('--config', '-c', dest="filename", metavar='FILE', default='configs/vae.yaml')
    ap.add_argument('--steps-per-epoch', type=int, default=8, help="synthetic data: batches per epoch")
    ap.add_argument('--max-epochs', type=int, default=None)
    args = ap.parse_args(argv)
    with open(args.filename) as f:
        config = yaml.safe_load(f)
    ema_decay, ema_warmup, _ = exp_ema(config['exp_params'])
    _, restart_every, restart_min_count, _ = exp_codebook(config)
    cb_ema_decay, cb_ema_eps = exp_codebook_ema(config)    # refused here too; VAEXperiment reads the keys itself
    exp_latent_stats(config)                 # refused here, before a device is touched; VAEXperiment reads the key itself
    kl_schedule, kl_free_bits = exp_kl(config)             # likewise
    recon_on, _, _ = exp_recon_stats(config)               # likewise
    exp_sample_prior(config)                               # likewise
    exp_val_loglik(config)                                 # likewise
    exp_code_prior(config)                                 # likewise

    rank =int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    gpus = config.get('trainer_params', {}).get('gpus', 1)
    use_gpu = (len(gpus) if isinstance(gpus, (list, tuple)) else int(gpus)) != 0
    if not (use_gpu and torch.cuda.is_available()):
        raise SystemExit("ctvae_amd runs on MI355X GPUs only: the hot path has no CPU fallback (use the reference for gpus: [])")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=dev)

    seed = config['exp_params'].get('manual_seed', 0)
    torch.manual_seed(seed)                                           # seed_everything (run.py:48)
    mp = dict(config['model_params'])
    model = vae_models[mp['name']](**mp).to(dev)
    val_graphs = bool(config['exp_params'].get('val_graphs', False))
    if val_graphs:
        from .models.ct_mcq_vae import CTMCQVAE
        if not isinstance(model, CTMCQVAE):
            raise SystemExit(f"exp_params.val_graphs needs a CTMCQVAE, model_params.name is {mp['name']!r}")
    # trainer_params.resume_from_checkpoint (run.py:85-101): with load_weights_only the reference loads the model's weights
    # (strict=False) and drops the key; without it the path is splatted into the Lightning Trainer, which restores optimizer,
    # scheduler, epoch and global step and continues -- the "trainer" entry of our checkpoints carries exactly that state
    ckpt_path = config['trainer_params'].get('resume_from_checkpoint')
    weights_only = bool(config['trainer_params'].get('load_weights_only'))
    ckpt = None
    if ckpt_path:
        ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=True)
        if ema_decay is not None and not weights_only:
            check_ema_checkpoint(ckpt, ckpt_path, ema_decay, ema_warmup)
        if restart_every is not None and not weights_only:
            check_codebook_checkpoint(ckpt, ckpt_path, restart_every, restart_min_count)
        if cb_ema_decay is not None and not weights_only:
            check_codebook_ema_checkpoint(ckpt, ckpt_path, cb_ema_decay, cb_ema_eps)
        if (kl_schedule is not None or kl_free_bits is not None) and not weights_only:
            check_kl_checkpoint(ckpt, ckpt_path, kl_schedule, kl_free_bits)
        model.load_state_dict(model_weights(ckpt['state_dict']), strict=not weights_only)
    ddp = GradBucketAllReduce(model) if world > 1 else None
    log_dir = os.path.join(config['logging_params'].get('save_dir', 'logs/'), config['logging_params'].get('name', mp['name']))
    os.makedirs(os.path.join(log_dir, "checkpoints"), exist_ok=True)
    log_file = open(os.path.join(log_dir, f"metrics_rank{rank}.jsonl"), "a") if rank == 0 else None
    tp = config['trainer_params']
    accumulate = trainer_accumulate(tp)
    track_norm = trainer_track_grad_norm(tp)
    watch, watch_freq = exp_watch_gradients(config['exp_params'])
    grad_log_file = open(os.path.join(log_dir, f"gradients_rank{rank}.jsonl"), "a") if rank == 0 and watch else None
    val_sampling = bool(config['exp_params'].get('val_sampling', False))
    if val_sampling and rank == 0:
        for d in VAEXperiment.SAMPLE_DIRS:
            os.makedirs(os.path.join(log_dir, d), exist_ok=True)
    if val_graphs and rank == 0:
        os.makedirs(os.path.join(log_dir, VAEXperiment.GRAPH_DIR), exist_ok=True)
    if recon_on and rank == 0:
        from .reconstats import RECON_DIR
        os.makedirs(os.path.join(log_dir, RECON_DIR), exist_ok=True)
    exp = VAEXperiment(model, config['exp_params'], ddp=ddp, log_file=log_file, gradient_clip_val=tp.get('gradient_clip_val'),
                       gradient_clip_algorithm=tp.get('gradient_clip_algorithm'), val_sampling=val_sampling, sample_dir=log_dir,
                       run_name=config['logging_params'].get('name', mp['name']), val_graphs=val_graphs,
                       accumulate_grad_batches=accumulate, track_grad_norm=track_norm, watch_gradients=watch,
                       watch_log_freq=watch_freq, grad_log_file=grad_log_file)
    if config['data_params'].get('hbm_images'):
        data = HbmData(config['data_params'], mp, dev, rank, world, seed)
    else:
        data = SyntheticData(config['data_params'], mp, dev, rank, world, args.steps_per_epoch, seed)

    exp.val_metric = build_val_metric(config, data)

    start_epoch = 0
    if ckpt is not None and not weights_only:
        if "trainer" not in ckpt:
            raise SystemExit(f"{ckpt_path} holds weights only (no 'trainer' entry: optimizer moments, scheduler, epoch); "
                             "set trainer_params.load_weights_only to start a new run from its weights")
        exp.load_state_dict(ckpt["trainer"])
        if exp.ema is not None:                                       # the average's buffer travels as weights
            exp.load_ema_model_state_dict(model_weights(ckpt['ema_state_dict']))
        start_epoch = int(ckpt["epoch"]) + 1
        if hasattr(data, "epoch"):
            data.epoch = start_epoch                                  # the shuffling order follows the epoch
    best = []

    def on_epoch_end(epoch, rec):
        if rank != 0:
            return
        print(json.dumps(rec), flush=True)
        state = {"state_dict": {"model." + k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()},
                 "epoch": epoch, "global_step": exp.global_step, "trainer": exp.state_dict()}
        if exp.ema is not None:                                       # the same keys, the averaged weights inside the slice
            state["ema_state_dict"] = {"model." + k: v for k, v in exp.ema_model_state_dict().items()}
        torch.save(state, os.path.join(log_dir, "checkpoints", "last.ckpt"))
        score = rec.get("val_Reconstruction_Loss")
        if score is not None:                                         # ModelCheckpoint(save_top_k=2, monitor=val_Reconstruction_Loss)
            path = os.path.join(log_dir, "checkpoints", f"epoch={epoch}.ckpt")
            torch.save(state, path)
            best.append((score, path))
            best.sort()
            for _, p in best[2:]:
                if os.path.exists(p):
                    os.remove(p)
            del best[2:]

    epochs = args.max_epochs or config['trainer_params'].get('max_epochs', 1)
    hist = exp.fit(data.train, data.val, max_epochs=epochs, on_epoch_end=on_epoch_end, start_epoch=start_epoch,
                   test_batches=data.test if val_sampling else None)
    if world > 1:
        dist.destroy_process_group()
    return hist


if __name__ == "__main__":
    main()
