"""CPU: the paths of VAEXperiment that every run feature shares -- what follows a backward pass (``finish_batch`` and the
step's tail), the validation reports of ``_validate`` (armed, disarmed also when something raises, written in order), the step
``log_all`` logs, and the bytes of every kind of JSONL record.  No kernel runs: the optimizer, the gradient exchange, the tail
methods, the model's forward and the record sources are replaced by recorders and stubs."""
import contextlib
import io
import itertools
from types import SimpleNamespace

import pytest
import torch

SMALL_MCQ = dict(in_channels=3, embedding_dim=16, hidden_dims=[8, 16], num_embeddings=8, img_size=64, codebooks=1, beta=0.25)
PARAMS = {"LR": 1e-3, "kld_weight": 1.0, "manual_seed": 3}
TAIL = ["track_gradients", "codebook_update", "ema_update", "codebook_restart"]


def _exp(params=None, **kw):
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    torch.manual_seed(0)
    return VAEXperiment(vae_models["MCQVAE"](**SMALL_MCQ), dict(PARAMS, **(params or {})), **kw)


def _record_calls(exp):
    """Recorders in place of the optimizer's step and stash, ``ddp_step`` and the four tail methods: (name, global_step at the
    call, keyword arguments) in call order."""
    calls = []

    def recorder(name):
        return lambda *a, **k: calls.append((name, exp.global_step, a, k))

    exp.optimizer.step, exp.optimizer.stash, exp.ddp_step = recorder("step"), recorder("stash"), recorder("ddp_step")
    for name in TAIL:
        setattr(exp, name, recorder(name))
    return calls


def _expected_first(accumulate, ends, stepped, ddp):
    """What follows the backward pass in front of the tail: nothing when the captured body stepped; inside a window the stash;
    else the exchange's step or the plain one."""
    if stepped:
        return []
    if accumulate > 1 and not ends:
        return ["stash"]
    return ["ddp_step" if ddp else "step"]


@pytest.mark.parametrize("accumulate,ends,stepped,ddp", list(itertools.product((1, 3), (True, False), (False, True), (False, True))))
def test_finish_batch_sequence(accumulate, ends, stepped, ddp):
    exp = _exp(ddp=SimpleNamespace(grad_scale=0.5, active=False) if ddp else None, accumulate_grad_batches=accumulate)
    calls = _record_calls(exp)
    exp.global_step = 4
    exp.finish_batch(ends, "pat", stepped=stepped)
    assert [c[0] for c in calls] == _expected_first(accumulate, ends, stepped, ddp) + (TAIL if ends else [])
    assert all(c[1] == 4 for c in calls), "the tail sees the number of the step that ran"
    assert exp.global_step == (5 if ends else 4)
    if not stepped:
        name, _, a, k = calls[0]
        if name == "stash":
            assert a == ("pat",)
        elif name == "ddp_step":
            assert a == ("pat",)
        elif accumulate > 1:
            assert k == {"grad_scale": 1.0 / 3, "pattern": "pat"}
        else:
            assert a == () and k == {}


@pytest.mark.parametrize("accumulate,ddp", list(itertools.product((1, 3), (False, True))))
def test_optimizer_step_is_finish_batch_at_a_window_end(accumulate, ddp):
    seqs = []
    for call in (lambda e: e.optimizer_step(), lambda e: e.finish_batch()):
        exp = _exp(ddp=SimpleNamespace(grad_scale=0.5, active=False) if ddp else None, accumulate_grad_batches=accumulate)
        calls = _record_calls(exp)
        call(exp)
        assert exp.global_step == 1
        seqs.append([(c[0], c[2], c[3]) for c in calls])
    assert seqs[0] == seqs[1]
    assert [c[0] for c in seqs[0]] == ["ddp_step" if ddp else "step"] + TAIL


def test_active_ddp():
    assert _exp()._active_ddp() is None
    for ddp, active in ((SimpleNamespace(grad_scale=1.0), False), (SimpleNamespace(grad_scale=1.0, active=False), False),
                        (SimpleNamespace(grad_scale=1.0, active=True), True)):
        assert (_exp(ddp=ddp)._active_ddp() is ddp) == active


# -- validation reports ------------------------------------------------------------------------------------------------------
BATCH = (torch.zeros(2, 3, 4, 4), torch.zeros(2))


def _stub_model(exp, pairs):
    """The model's part of ``validation_step`` without a kernel; ``pairs`` counts the calls of ``reconstruction_pair``."""
    exp.forward = lambda x, **kw: [x, x]
    exp.model.loss_function = lambda *r, **kw: {"loss": torch.tensor(1.5)}

    def reconstruction_pair(results):
        pairs.append(results)
        return None            # (a batch without a picture pair: the accumulators get nothing)

    exp.model.reconstruction_pair = reconstruction_pair


def _report_exp():
    exp = _exp({"codebook_stats": True, "recon_stats": True})
    assert exp.val_codebook is not None and list(exp.val_recon) == [""]
    exp.val_recon = {"": SimpleNamespace(reset=lambda: None)}          # (the real accumulator has no CPU form)
    exp.write_codebook_stats = lambda usage: {"val_codebook_x": 1.0}
    exp.write_recon_stats = lambda acc, epoch: {"val_recon_x": 2.0}
    exp.validation_metrics = lambda epoch: {"val_m": 3.0}
    return exp


def _assert_disarmed(exp, pairs):
    assert exp.model.vq_layer.usage_observer is None
    assert exp._val_observers == []
    del pairs[:]
    exp.validation_step(BATCH, 0)
    assert pairs == [], "a validation_step outside _validate observes nothing"


def test_validate_arms_runs_disarms_and_writes_in_order():
    exp, pairs, seen = _report_exp(), [], []
    _stub_model(exp, pairs)
    step = exp.validation_step

    def validation_step(batch, i):
        seen.append((exp.model.vq_layer.usage_observer is not None, len(exp._val_observers)))
        return step(batch, i)

    exp.validation_step = validation_step
    rec = exp._validate(0, lambda: [BATCH, BATCH], None)
    assert seen == [(True, 1), (True, 1)] and len(pairs) == 2
    assert list(rec.items()) == [("val_loss", 1.5), ("val_codebook_x", 1.0), ("val_recon_x", 2.0), ("val_m", 3.0)]
    exp.validation_step = step
    _assert_disarmed(exp, pairs)


def test_validate_disarms_when_a_write_raises():
    exp, pairs, fake = _report_exp(), [], []
    _stub_model(exp, pairs)

    @contextlib.contextmanager
    def report(epoch):
        def write():
            raise RuntimeError("the write failed")

        fake.append("armed")
        try:
            yield write
        finally:
            fake.append("disarmed")

    reports = exp._val_reports()
    exp._val_reports = lambda: reports + [report]
    exp.validation_step = lambda batch, i: {"val_loss": 1.0, "step": 0}
    with pytest.raises(RuntimeError, match="the write failed"):
        exp._validate(0, lambda: [BATCH], None)
    assert fake == ["armed", "disarmed"]
    del exp.validation_step
    _assert_disarmed(exp, pairs)


def test_validate_disarms_when_an_observer_raises():
    exp, pairs, fake = _report_exp(), [], []
    _stub_model(exp, pairs)

    def observe(results):
        raise RuntimeError("the observer failed")

    @contextlib.contextmanager
    def report(epoch):
        with exp._observing_results(observe):
            fake.append(len(exp._val_observers))
            yield lambda: {}

    reports = exp._val_reports()
    exp._val_reports = lambda: reports + [report]
    with pytest.raises(RuntimeError, match="the observer failed"):
        exp._validate(0, lambda: [BATCH], None)
    assert fake == [2] and len(pairs) == 1       # the run's own recon observer came first, in the real validation_step
    _assert_disarmed(exp, pairs)


# -- records -----------------------------------------------------------------------------------------------------------------
def test_log_all_logs_the_step_it_is_given():
    exp = _exp(log_every=5, log_file=io.StringIO())
    exp.global_step = 3
    exp.kl = SimpleNamespace(weight=lambda step: step / 4)
    losses = {"loss": torch.tensor(1.5), "Reconstruction_Loss": torch.tensor([2.0]), "name": "dropped", "map": torch.zeros(2, 2)}
    assert exp.log_all(losses, 4, step=7) is None and exp.log_all(losses, 4) is None
    assert exp.log_file.getvalue() == ""
    rec = exp.log_all(losses, 4, step=10)
    assert rec == {"Reconstruction_Loss": 2.0, "loss": 1.5, "kld_weight": 2.5, "step": 10}
    assert exp.log_file.getvalue() == '{"Reconstruction_Loss": 2.0, "loss": 1.5, "kld_weight": 2.5, "step": 10}\n'
    assert exp.global_step == 3
    exp.global_step = 5                     # without a step: global_step, as before
    exp.log_all(losses, 4, validation=True)
    assert exp.log_file.getvalue().splitlines()[1] == '{"val_Reconstruction_Loss": 2.0, "val_loss": 1.5, "step": 5}'
    exp.log_all(losses, 4, validation=True, force=True, step=8)
    assert exp.log_file.getvalue().splitlines()[2] == '{"val_Reconstruction_Loss": 2.0, "val_loss": 1.5, "step": 8}'


def _last_line(f):
    return f.getvalue().splitlines()[-1]


def test_every_record_kind_byte_for_byte(monkeypatch):
    from ctvae_amd import causalgraph, experiment as E
    exp = _exp({"codebook_stats": True}, log_every=1, log_file=io.StringIO(), grad_log_file=io.StringIO())
    log, exp.global_step = exp.log_file, 6
    # validation_metrics: the metric's results under val_, seeded per epoch
    seeds = []
    exp.val_metric = SimpleNamespace(compute=lambda f, model, seed: seeds.append(seed) or {"mig": 0.25, "fvs": 0.5})
    assert exp.validation_metrics(2) == {"val_mig": 0.25, "val_fvs": 0.5}
    assert _last_line(log) == '{"val_mig": 0.25, "val_fvs": 0.5, "step": 6}'
    assert seeds == [3 * 1_000_003 + 2] and exp.epoch_seed(2) == seeds[0]
    # write_graphs: skipped when no group had rows
    monkeypatch.setattr(causalgraph, "summarize", lambda res: {"base": {"edges": 1.5}, "f0+": {"edges": None}})
    assert exp.write_graphs(SimpleNamespace(result=lambda: {}), 0) == {"val_graph_edges_base": 1.5}
    assert _last_line(log) == '{"val_graph_edges_base": 1.5, "step": 6}'
    n = len(log.getvalue())
    monkeypatch.setattr(causalgraph, "summarize", lambda res: {"base": {"edges": None}})
    assert exp.write_graphs(SimpleNamespace(result=lambda: {}), 0) == {} and len(log.getvalue()) == n
    # track_gradients: the norms with the rate and the step behind them, the histograms with the step in front
    exp.grad_tracker = SimpleNamespace(record=lambda step, every, scale: ({"grad_2.0_norm_total": 1.0}, {"gradients/w": {"min": 0.0}}))
    exp.track_gradients()
    assert _last_line(log) == '{"grad_2.0_norm_total": 1.0, "lr-Adam": 0.001, "step": 6}'
    assert exp.grad_log_file.getvalue() == '{"step": 6, "gradients/w": {"min": 0.0}}\n'
    # codebook_update
    exp.codebook_ema = SimpleNamespace(C=2, update=lambda reduce=None: None, cluster_sizes=lambda: ([1.0, 0.5], [2.0, 3.0]))
    exp.codebook_update()
    assert _last_line(log) == ('{"codebook_ema_min_cluster_0": 1.0, "codebook_ema_max_cluster_0": 2.0, "codebook_ema_min_cluster_1": 0.5, '
                               '"codebook_ema_max_cluster_1": 3.0, "codebook_ema_min_cluster": 0.5, "codebook_ema_max_cluster": 3.0, '
                               '"step": 6}')
    # codebook_restart (on the step that makes global_step a multiple of N)
    monkeypatch.setattr(E, "codebook_record", lambda counts, prefix: {prefix + "codebook_perplexity_0": 4.0, prefix + "codebook_usage_0": 0.5,
                                                                     prefix + "codebook_dead_0": 4, prefix + "codebook_perplexity": 4.0})
    exp.codebook_ema = SimpleNamespace(reset_codes=lambda dead: None)
    exp.codebook, exp.codebook_every = SimpleNamespace(C=1, restart=lambda *a, **k: (None, [(0, 2), (0, 5)], None)), 7
    exp.codebook_restart()
    assert _last_line(log) == '{"codebook_restarts": 2, "codebook_restarts_0": 2, "codebook_perplexity_0": 4.0, "codebook_usage_0": 0.5, "step": 6}'
    assert (exp.codebook_ordinal, exp.codebook_restarted) == (1, 2)
    # the three reports of a validation epoch
    assert exp.write_codebook_stats(SimpleNamespace(read=lambda: (None, 3))) == {
        "val_codebook_perplexity_0": 4.0, "val_codebook_usage_0": 0.5, "val_codebook_dead_0": 4, "val_codebook_perplexity": 4.0,
        "val_codebook_invalid": 3}
    assert _last_line(log) == ('{"val_codebook_perplexity_0": 4.0, "val_codebook_usage_0": 0.5, "val_codebook_dead_0": 4, '
                               '"val_codebook_perplexity": 4.0, "val_codebook_invalid": 3, "step": 6}')
    monkeypatch.setattr(E, "latent_record", lambda res: {"val_latent_kl_total": 9.0, "val_latent_rows": 8})
    assert exp.write_latent_stats(SimpleNamespace(result=lambda: {}), 0) == {"val_latent_kl_total": 9.0, "val_latent_rows": 8}
    assert _last_line(log) == '{"val_latent_kl_total": 9.0, "val_latent_rows": 8, "step": 6}'
    monkeypatch.setattr(E, "recon_summarize", lambda records, flags, R: None)
    monkeypatch.setattr(E, "recon_record", lambda summary, suffix: {f"val_recon_psnr{suffix}": 30.0})
    accs = {sfx: SimpleNamespace(R=1.0, K=0, result=lambda: {"records": None, "flags": []}) for sfx in ("_base", "_action")}
    assert exp.write_recon_stats(accs, 0) == {"val_recon_psnr_base": 30.0, "val_recon_psnr_action": 30.0}
    assert _last_line(log) == '{"val_recon_psnr_base": 30.0, "val_recon_psnr_action": 30.0, "step": 6}'
    assert len(log.getvalue().splitlines()) == 8 and exp.global_step == 6


def test_ema_checkpoint_entry_is_the_average_own():
    exp = _exp({"ema_decay": 0.99, "ema_warmup": True})
    entry = exp.state_dict()["ema"]
    assert entry == {"decay": 0.99, "warmup": True, "updates": 0} and list(entry) == ["decay", "warmup", "updates"]
    assert [type(v) for v in entry.values()] == [float, bool, int]
    assert entry == exp.ema.state_dict(buffer=False) and set(exp.ema.state_dict()) == set(entry) | {"buffer"}
    exp.ema.load_state_dict(entry)


def test_codebook_offset_serves_any_quantiser():
    from ctvae_amd.optim import codebook_offset
    exp = _exp({"codebook_restart_every": 3, "codebook_ema_decay": 0.9})
    lo = codebook_offset(exp.model.vq_layer, exp.optimizer)
    assert lo is not None and lo == exp.codebook.codebook_offset(exp.optimizer)
    with pytest.raises(ValueError, match="codebook_ema_decay cannot move codebooks the optimizer does not step: update_parameters="
                                         "'decoder' leaves the codebooks outside the optimizer's slice"):
        _exp({"codebook_ema_decay": 0.9, "update_parameters": "decoder"})
