"""Host side of the weight average (``exp_params.ema_decay``, optim.WeightEMA): the settings validator, the decay schedule, the
runner's refusals and the ``--ema`` flag of the two checkpoint tools.  No GPU: nothing here launches a kernel."""
import os

import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ema_settings_accepts():
    from ctvae_amd.optim import ema_settings
    assert ema_settings(None, None, None) == (None, False, False)
    assert ema_settings(0.999) == (0.999, False, True)                    # ema_warmup defaults to false, ema_eval to true
    assert ema_settings(0.5, True, False) == (0.5, True, False)
    assert ema_settings(0.5, False, True) == (0.5, False, True)
    d, w, e = ema_settings(1e-3, None, None)
    assert d == 1e-3 and w is False and e is True


@pytest.mark.parametrize("bad", [True, False, "0.999", 1, 0, 0.0, 1.0, -0.5, 1.5, float("nan"), float("inf"), [0.5]])
def test_ema_settings_refuses_the_decay_by_name(bad):
    from ctvae_amd.optim import ema_settings
    with pytest.raises(ValueError, match="ema_decay"):
        ema_settings(bad, None, None)


def test_ema_settings_refuses_the_flags_by_name():
    from ctvae_amd.optim import ema_settings
    for bad in (1, 0, "true", 0.5):
        with pytest.raises(ValueError, match="ema_warmup"):
            ema_settings(0.9, bad, None)
        with pytest.raises(ValueError, match="ema_eval"):
            ema_settings(0.9, None, bad)
    for v in (True, False):                                                # set without ema_decay: refused by the flag's name
        with pytest.raises(ValueError, match="ema_warmup.*without ema_decay"):
            ema_settings(None, v, None)
        with pytest.raises(ValueError, match="ema_eval.*without ema_decay"):
            ema_settings(None, None, v)


def test_decay_at():
    from ctvae_amd.optim import ema_decay_at
    for t in (1, 2, 10, 10 ** 6):
        assert ema_decay_at(0.999, False, t) == 0.999
    assert ema_decay_at(0.999, True, 1) == 2 / 11
    assert ema_decay_at(0.999, True, 2) == 3 / 12
    assert ema_decay_at(0.999, True, 10) == 11 / 20
    assert ema_decay_at(0.999, True, 10 ** 6) == 0.999                     # (1 + t) / (10 + t) = 0.99999100...: the cap holds
    assert ema_decay_at(0.5, True, 1) == 2 / 11 and ema_decay_at(0.5, True, 10) == 0.5


def test_weight_ema_object_on_the_host():
    """What needs no kernel: the buffer is a copy of the optimizer's slice at its 16-byte phase, ``decay_at`` follows the
    settings, and the state round-trips."""
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    m = vae_models["VanillaVAE"](in_channels=3, latent_dim=16)
    params = {"LR": 0.005, "weight_decay": 0.0, "kld_weight": 0.00025}
    plain = VAEXperiment(m, dict(params))
    assert plain.ema is None and plain.ema_eval is False and "ema" not in plain.state_dict()
    exp = VAEXperiment(m, dict(params, ema_decay=0.999, ema_warmup=True))
    ema = exp.ema
    live = m.flat_params[exp.optimizer.slice]
    assert exp.ema_eval is True and ema.updates == 0
    assert ema.buffer.data_ptr() != live.data_ptr() and torch.equal(ema.buffer, live)
    assert ema.buffer.data_ptr() % 16 == live.data_ptr() % 16
    assert [ema.decay_at(t) for t in (1, 2, 10, 10 ** 6)] == [2 / 11, 3 / 12, 11 / 20, 0.999]
    assert exp.state_dict()["ema"] == {"decay": 0.999, "warmup": True, "updates": 0}
    sd = ema.state_dict()
    assert set(sd) == {"decay", "warmup", "updates", "buffer"}
    other = VAEXperiment(vae_models["VanillaVAE"](in_channels=3, latent_dim=16), dict(params, ema_decay=0.999, ema_warmup=True)).ema
    other.load_state_dict({**sd, "updates": 7})
    assert other.updates == 7 and torch.equal(other.buffer, ema.buffer)
    with pytest.raises(RuntimeError, match="ema_decay"):
        other.load_state_dict({**sd, "decay": 0.99})
    with pytest.raises(ValueError, match="ema_warmup"):
        VAEXperiment(m, dict(params, ema_warmup=True))
    with pytest.raises(ValueError, match="ema_decay"):
        VAEXperiment(m, dict(params, ema_decay=1))


def _config(tmp_path, name, exp=None, **trainer):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", name)))
    cfg["trainer_params"].update(trainer)
    cfg["exp_params"].update(exp or {})
    cfg["logging_params"]["save_dir"] = str(tmp_path / "logs")
    p = tmp_path / name
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_runner_refuses_by_name(tmp_path):
    """Bad values leave run.main as a SystemExit naming exp_params.<key>, before a device or a file is touched."""
    from ctvae_amd import run
    for bad in (True, "0.9", 1, 0.0, 1.0, 2.5):
        with pytest.raises(SystemExit, match=r"exp_params\.ema_decay"):
            run.main(["-c", _config(tmp_path, "vae.yaml", exp={"ema_decay": bad})])
    with pytest.raises(SystemExit, match=r"exp_params\.ema_warmup"):
        run.main(["-c", _config(tmp_path, "vae.yaml", exp={"ema_decay": 0.9, "ema_warmup": 1})])
    with pytest.raises(SystemExit, match=r"exp_params\.ema_eval"):
        run.main(["-c", _config(tmp_path, "vae.yaml", exp={"ema_decay": 0.9, "ema_eval": "yes"})])
    with pytest.raises(SystemExit, match=r"exp_params\.ema_warmup.*without ema_decay"):
        run.main(["-c", _config(tmp_path, "vae.yaml", exp={"ema_warmup": True})])
    with pytest.raises(SystemExit, match=r"exp_params\.ema_eval.*without ema_decay"):
        run.main(["-c", _config(tmp_path, "vae.yaml", exp={"ema_eval": False})])
    assert not (tmp_path / "logs").exists()


def test_resume_check_refuses_by_name():
    """Full resume under the key: a checkpoint without the average, or one kept under other settings, names the key and the path."""
    from ctvae_amd.run import check_ema_checkpoint
    good = {"state_dict": {}, "ema_state_dict": {}, "trainer": {"ema": {"decay": 0.9, "warmup": False, "updates": 3}}}
    check_ema_checkpoint(good, "a.ckpt", 0.9, False)
    for ckpt in ({"state_dict": {}, "trainer": {}}, {"state_dict": {}, "ema_state_dict": {}, "trainer": {}},
                 {"state_dict": {}, "trainer": {"ema": good["trainer"]["ema"]}}, {"state_dict": {}}):
        with pytest.raises(SystemExit, match=r"exp_params\.ema_decay.*a\.ckpt"):
            check_ema_checkpoint(ckpt, "a.ckpt", 0.9, False)
    with pytest.raises(SystemExit, match=r"exp_params\.ema_decay.*a\.ckpt"):
        check_ema_checkpoint(good, "a.ckpt", 0.99, False)
    with pytest.raises(SystemExit, match=r"exp_params\.ema_decay.*a\.ckpt"):
        check_ema_checkpoint(good, "a.ckpt", 0.9, True)


def test_tools_refuse_ema_without_the_entry(tmp_path):
    from ctvae_amd import apply_action, causal_graph
    ckpt = tmp_path / "plain.ckpt"
    torch.save({"state_dict": {}, "epoch": 0}, ckpt)
    cfg = _config(tmp_path, "ct_mcq_vae.yaml")
    for tool in (apply_action, causal_graph):
        with pytest.raises(SystemExit, match=r"--ema.*plain\.ckpt.*ema_state_dict"):
            tool.main(["-c", cfg, "--checkpoint", str(ckpt), "--ema"])
