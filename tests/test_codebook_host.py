"""Host side of codebook usage and dead-code restarts (``exp_params.codebook_stats`` / ``codebook_restart_every`` /
``codebook_restart_min_count`` / ``codebook_restart_pool``; optim.CodebookUsage): the settings validator, the statistics against
NumPy, the dead list and the draw, and the refusals of the experiment, the runner and a resume.  No GPU: nothing here launches a
kernel.  Perplexity is float64 on both sides over at most 512 terms: relative 1e-12."""
import json
import math
import os

import numpy as np
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(in_channels=3, embedding_dim=16, hidden_dims=[8, 16], num_embeddings=8, img_size=64, codebooks=4, beta=0.25)
PARAMS = {"LR": 1e-3, "weight_decay": 0.0, "kld_weight": 1.0, "manual_seed": 11}


def _mcq(**over):
    from ctvae_amd.models import vae_models
    torch.manual_seed(7)
    cfg = dict(CFG, **over)
    return vae_models["MCQVAE"](**dict(cfg, hidden_dims=list(cfg["hidden_dims"])))


# ---- settings ----------------------------------------------------------------------------------------------
def test_settings_accepts():
    from ctvae_amd.optim import codebook_settings
    assert codebook_settings() == (False, None, None, None)
    assert codebook_settings(True) == (True, None, None, None)
    assert codebook_settings(False, 100) == (False, 100, 1, 1024)           # min_count defaults to 1, the pool to 1024 rows
    assert codebook_settings(True, 1, 3, 7) == (True, 1, 3, 7)


@pytest.mark.parametrize("bad", [1, 0, "true", 0.5, [True]])
def test_settings_refuses_stats_by_name(bad):
    from ctvae_amd.optim import codebook_settings
    with pytest.raises(ValueError, match="codebook_stats"):
        codebook_settings(bad)


@pytest.mark.parametrize("bad", [True, False, 2.0, "2", 0, -1, [2]])
def test_settings_refuses_the_integers_by_name(bad):
    from ctvae_amd.optim import codebook_settings
    with pytest.raises(ValueError, match="codebook_restart_every"):
        codebook_settings(None, bad)
    with pytest.raises(ValueError, match="codebook_restart_min_count"):
        codebook_settings(None, 2, bad)
    with pytest.raises(ValueError, match="codebook_restart_pool"):
        codebook_settings(None, 2, None, bad)


def test_settings_refuses_dependent_keys_alone():
    from ctvae_amd.optim import codebook_settings
    with pytest.raises(ValueError, match="codebook_restart_min_count.*without codebook_restart_every"):
        codebook_settings(True, None, 2)
    with pytest.raises(ValueError, match="codebook_restart_pool.*without codebook_restart_every"):
        codebook_settings(None, None, None, 64)


# ---- statistics --------------------------------------------------------------------------------------------
def _numpy_stats(counts):
    out = []
    for row in np.asarray(counts, dtype=np.float64):
        total = row.sum()
        if total == 0:
            out.append((None, 0.0, len(row)))
            continue
        p = row[row > 0] / total
        out.append((float(np.exp(-(p * np.log(p)).sum())), float((row > 0).sum()) / len(row), int((row == 0).sum())))
    return out


def test_statistics_match_numpy():
    from ctvae_amd.optim import codebook_record, codebook_stats
    g = torch.Generator().manual_seed(5)
    counts = torch.randint(0, 1000, (5, 512), generator=g)
    counts[1] = 0                                   # a codebook that was never asked
    counts[2] = 0
    counts[2, 17] = 12345                           # one code takes everything: perplexity 1
    counts[3] = 3                                   # uniform: perplexity K
    counts[4, ::2] = 0
    st = codebook_stats(counts)
    ref = _numpy_stats(counts.numpy())
    for s, (perp, usage, dead) in zip(st, ref):
        if perp is None:
            assert s["perplexity"] is None
        else:
            assert abs(s["perplexity"] - perp) <= 1e-12 * perp, (s["perplexity"], perp)
        assert s["usage"] == usage and s["dead"] == dead
    assert st[1] == {"perplexity": None, "usage": 0.0, "dead": 512, "total": 0}
    assert abs(st[2]["perplexity"] - 1.0) <= 1e-12 and st[2]["dead"] == 511
    assert abs(st[3]["perplexity"] - 512.0) <= 512e-12 and st[3]["usage"] == 1.0
    assert st[4]["dead"] >= 256
    rec = codebook_record(counts, "val_")
    assert rec["val_codebook_perplexity_1"] is None and rec["val_codebook_usage_1"] == 0.0 and rec["val_codebook_dead_1"] == 512
    known = [r[0] for r in ref if r[0] is not None]
    assert abs(rec["val_codebook_perplexity"] - sum(known) / 4) <= 1e-12 * 512
    assert rec["val_codebook_usage"] == sum(r[1] for r in ref) / 5 and rec["val_codebook_dead"] == sum(r[2] for r in ref) / 5
    text = json.dumps(rec)                          # null, never NaN
    assert "NaN" not in text and "null" in text
    assert all(v is None or math.isfinite(v) for v in rec.values())
    empty = codebook_record(torch.zeros(2, 4, dtype=torch.int64), "")
    assert empty["codebook_perplexity"] is None and empty["codebook_usage"] == 0.0 and "NaN" not in json.dumps(empty)


# ---- the dead list and the draw ----------------------------------------------------------------------------
def test_dead_list_is_in_c_k_order():
    from ctvae_amd.optim import codebook_dead_list
    counts = torch.tensor([[0, 5, 1, 0], [2, 2, 2, 2], [9, 0, 0, 1]])
    assert codebook_dead_list(counts) == [(0, 0), (0, 3), (2, 1), (2, 2)]
    assert codebook_dead_list(counts, 2) == [(0, 0), (0, 2), (0, 3), (2, 1), (2, 2), (2, 3)]
    assert codebook_dead_list(counts, 3) == [(0, 0), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (2, 3)]
    assert codebook_dead_list(torch.ones(2, 3, dtype=torch.int64)) == []


def test_draw_is_one_randperm_per_seed_and_ordinal():
    from ctvae_amd.optim import codebook_restart_rows, codebook_restart_seed
    cpu = torch.get_rng_state()
    rows = codebook_restart_rows(11, 0, 5, 100)
    assert torch.equal(torch.get_rng_state(), cpu), "the global generator moved"
    gen = torch.Generator().manual_seed(codebook_restart_seed(11, 0))
    assert rows == torch.randperm(100, generator=gen)[:5].tolist()
    assert rows == codebook_restart_rows(11, 0, 5, 100) and len(set(rows)) == 5
    assert rows[:3] == codebook_restart_rows(11, 0, 3, 100)                 # consumed in list order
    assert rows != codebook_restart_rows(11, 1, 5, 100) and rows != codebook_restart_rows(12, 0, 5, 100)
    assert codebook_restart_rows(11, 0, 0, 0) == []
    with pytest.raises(ValueError, match="pool"):
        codebook_restart_rows(11, 0, 1, 0)


def test_draw_wraps_around_when_dead_codes_outnumber_rows():
    from ctvae_amd.optim import codebook_restart_rows, codebook_restart_seed
    rows = codebook_restart_rows(3, 2, 11, 4)
    perm = torch.randperm(4, generator=torch.Generator().manual_seed(codebook_restart_seed(3, 2))).tolist()
    assert sorted(perm) == [0, 1, 2, 3]
    assert rows == [perm[i % 4] for i in range(11)]


# ---- the experiment ----------------------------------------------------------------------------------------
def test_experiment_builds_nothing_without_the_keys():
    from ctvae_amd.experiment import VAEXperiment
    m = _mcq()
    exp = VAEXperiment(m, dict(PARAMS))
    assert exp.codebook is None and exp.val_codebook is None and "codebook" not in exp.state_dict()
    assert m.vq_layer.usage_observer is None
    exp.codebook_restart()                          # nothing to do, nothing launched


def test_experiment_objects_on_the_host():
    from ctvae_amd.experiment import VAEXperiment
    m = _mcq()
    exp = VAEXperiment(m, dict(PARAMS, codebook_stats=True, codebook_restart_every=3, codebook_restart_pool=10))
    cb = exp.codebook
    assert (cb.C, cb.K, cb.Dc, cb.D) == (4, 8, 4, 16)
    assert tuple(cb.counts.shape) == (4, 8) and cb.counts.dtype == torch.int64 and tuple(cb.pool.shape) == (10, 16)
    assert exp.val_codebook is not None and exp.val_codebook.pool is None
    assert m.vq_layer.usage_observer is None        # attached inside fit() only
    views = cb.codebook_views(exp.optimizer)
    ws = [q.embedding.weight for q in m.vq_layer.quantizers]
    assert views[0].data_ptr() == ws[0].data_ptr() and tuple(views[0].shape) == (4, 8, 4)
    assert torch.equal(views[0][2], ws[2].detach())
    lo = cb.codebook_offset(exp.optimizer)
    assert views[1].data_ptr() == exp.optimizer.exp_avg[lo:].data_ptr() and views[2].data_ptr() == exp.optimizer.exp_avg_sq[lo:].data_ptr()
    sd = exp.state_dict()["codebook"]
    assert {k: v for k, v in sd.items() if k != "counts"} == {"every": 3, "min_count": 1, "pool": 10, "ordinal": 0,
                                                              "restarted": 0, "valid_rows": -1}
    assert torch.equal(sd["counts"], torch.zeros(4, 8, dtype=torch.int64))
    with exp._counting_training_codes():
        assert m.vq_layer.usage_observer == cb.observe
    assert m.vq_layer.usage_observer is None
    with pytest.raises(ZeroDivisionError):
        with exp._counting_training_codes():
            1 / 0
    assert m.vq_layer.usage_observer is None
    # a single-codebook quantiser (VQVAE's class) is one [1, K, D] codebook
    from ctvae_amd.models import vae_models
    from ctvae_amd.optim import CodebookUsage
    v = vae_models["VQVAE"](in_channels=3, embedding_dim=16, num_embeddings=32, hidden_dims=[8, 16], img_size=64)
    u = CodebookUsage(v.vq_layer, 4)
    assert (u.C, u.K, u.Dc, u.D) == (1, 32, 16, 16)


def test_experiment_refuses_by_name():
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    vanilla = vae_models["VanillaVAE"](in_channels=3, latent_dim=16)
    with pytest.raises(ValueError, match="codebook_stats.*vq_layer.*VanillaVAE"):
        VAEXperiment(vanilla, dict(PARAMS, codebook_stats=True))
    with pytest.raises(ValueError, match="codebook_restart_every.*vq_layer.*VanillaVAE"):
        VAEXperiment(vanilla, dict(PARAMS, codebook_restart_every=5))
    with pytest.raises(ValueError, match="codebook_restart_min_count"):
        VAEXperiment(_mcq(), dict(PARAMS, codebook_restart_min_count=2))
    with pytest.raises(ValueError, match="codebook_restart_every"):
        VAEXperiment(_mcq(), dict(PARAMS, codebook_restart_every=2.0))
    with pytest.raises(ValueError, match="num_embeddings 1024"):
        VAEXperiment(_mcq(num_embeddings=1024), dict(PARAMS, codebook_stats=True))
    # restarts need the codebooks inside the optimizer's slice; the statistics do not
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "ct_mcq_vae.yaml")))
    torch.manual_seed(3)
    ct = vae_models["CTMCQVAE"](**cfg["model_params"])
    ep = dict(cfg["exp_params"])
    assert ep["update_parameters"] == "ct_layer"
    with pytest.raises(ValueError, match="codebook_restart_every.*update_parameters='ct_layer'"):
        VAEXperiment(ct, dict(ep, codebook_restart_every=10))
    exp = VAEXperiment(ct, dict(ep, codebook_stats=True))
    assert exp.codebook is None and exp.val_codebook is not None
    del ep["update_parameters"]
    assert VAEXperiment(ct, dict(ep, codebook_restart_every=10)).codebook is not None


def test_resume_refuses_mismatched_settings():
    from ctvae_amd.experiment import VAEXperiment
    a = VAEXperiment(_mcq(), dict(PARAMS, codebook_restart_every=3, codebook_restart_min_count=2))
    a.codebook.counts.copy_(torch.arange(32).view(4, 8))
    a.codebook.valid_rows = 9
    a.codebook_ordinal, a.codebook_restarted = 4, 17
    sd = a.state_dict()
    b = VAEXperiment(_mcq(), dict(PARAMS, codebook_restart_every=3, codebook_restart_min_count=2, codebook_restart_pool=8))
    b.load_state_dict(sd)                           # (another pool size is no obstacle: the pool does not travel)
    assert torch.equal(b.codebook.counts, a.codebook.counts) and (b.codebook_ordinal, b.codebook_restarted) == (4, 17)
    assert b.codebook.valid_rows == 8
    for other in ({"codebook_restart_every": 4, "codebook_restart_min_count": 2}, {"codebook_restart_every": 3}):
        with pytest.raises(RuntimeError, match="codebook_restart_every"):
            VAEXperiment(_mcq(), dict(PARAMS, **other)).load_state_dict(sd)
    plain = VAEXperiment(_mcq(), dict(PARAMS)).state_dict()
    with pytest.raises(RuntimeError, match="codebook_restart_every"):
        VAEXperiment(_mcq(), dict(PARAMS, codebook_restart_every=3)).load_state_dict(plain)
    VAEXperiment(_mcq(), dict(PARAMS)).load_state_dict(sd)         # a run without the key ignores the entry


# ---- the runner --------------------------------------------------------------------------------------------
def _config(tmp_path, name, exp=None, **trainer):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", name)))
    cfg["trainer_params"].update(trainer)
    cfg["exp_params"].update(exp or {})
    cfg["logging_params"]["save_dir"] = str(tmp_path / "logs")
    p = tmp_path / name
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_runner_refuses_by_name(tmp_path):
    """Bad values, a model that does not quantise and restarts under ``update_parameters: ct_layer`` leave run.main as a
    SystemExit naming exp_params.<key>, before a device or a file is touched."""
    from ctvae_amd import run
    for key, bad in (("codebook_stats", 1), ("codebook_restart_every", True), ("codebook_restart_every", 0),
                     ("codebook_restart_every", 2.5), ("codebook_restart_every", "10")):
        with pytest.raises(SystemExit, match=rf"exp_params\.{key}"):
            run.main(["-c", _config(tmp_path, "mcq_vae.yaml", exp={key: bad})])
    with pytest.raises(SystemExit, match=r"exp_params\.codebook_restart_min_count"):
        run.main(["-c", _config(tmp_path, "mcq_vae.yaml", exp={"codebook_restart_every": 5, "codebook_restart_min_count": 0})])
    with pytest.raises(SystemExit, match=r"exp_params\.codebook_restart_pool.*without codebook_restart_every"):
        run.main(["-c", _config(tmp_path, "mcq_vae.yaml", exp={"codebook_restart_pool": 64})])
    with pytest.raises(SystemExit, match=r"exp_params\.codebook_stats.*vq_layer.*VanillaVAE"):
        run.main(["-c", _config(tmp_path, "vae.yaml", exp={"codebook_stats": True})])
    with pytest.raises(SystemExit, match=r"exp_params\.codebook_restart_every.*vq_layer.*VanillaVAE"):
        run.main(["-c", _config(tmp_path, "vae.yaml", exp={"codebook_restart_every": 5})])
    with pytest.raises(SystemExit, match=r"exp_params\.codebook_restart_every.*update_parameters.*ct_layer"):
        run.main(["-c", _config(tmp_path, "ct_mcq_vae.yaml", exp={"codebook_restart_every": 5})])
    assert not (tmp_path / "logs").exists()
    cfg = yaml.safe_load(open(_config(tmp_path, "ct_mcq_vae.yaml", exp={"codebook_stats": True})))
    assert run.exp_codebook(cfg) == (True, None, None, None)                # the statistics stay allowed there


def test_resume_check_refuses_by_name():
    from ctvae_amd.run import check_codebook_checkpoint
    good = {"state_dict": {}, "trainer": {"codebook": {"every": 4, "min_count": 1}}}
    check_codebook_checkpoint(good, "a.ckpt", 4, 1)
    for ckpt in ({"state_dict": {}, "trainer": {}}, {"state_dict": {}}):
        with pytest.raises(SystemExit, match=r"exp_params\.codebook_restart_every.*a\.ckpt"):
            check_codebook_checkpoint(ckpt, "a.ckpt", 4, 1)
    with pytest.raises(SystemExit, match=r"exp_params\.codebook_restart_every.*a\.ckpt"):
        check_codebook_checkpoint(good, "a.ckpt", 5, 1)
    with pytest.raises(SystemExit, match=r"exp_params\.codebook_restart_every.*a\.ckpt"):
        check_codebook_checkpoint(good, "a.ckpt", 4, 2)


def test_config_shows_the_keys_commented_out():
    text = open(os.path.join(ROOT, "configs", "mcq_vae.yaml")).read()
    assert "# codebook_stats: true" in text and "# codebook_restart_every:" in text
    ep = yaml.safe_load(text)["exp_params"]
    assert not any(k.startswith("codebook") for k in ep)
