"""CPU: what the checkpoint commands share -- ctvae_amd/evalrun.py (the reading of a batch, the ``.npz`` writer) and the front end
ctvae_amd/tool.py, through each of the five commands: the refusals every command words alike, and the torch generator left alone."""
import importlib
import io
import os

import numpy as np
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAUSSIAN = ("VanillaVAE, BetaVAE, LogCoshVAE, DIPVAE, MSSIMVAE, TwoStageVAE, VampVAE, IWAE, MIWAE, InfoVAE, JointVAE, BetaTCVAE, "
            "ConditionalVAE")
PRIOR = "VanillaVAE, BetaVAE, LogCoshVAE, DIPVAE, MSSIMVAE, TwoStageVAE, InfoVAE, VampVAE, BetaTCVAE"
# command: (its own config, a config it does not serve, the model name in that one, the reason it gives)
COMMANDS = {
    "apply_action": ("ct_mcq_vae.yaml", "vae.yaml", None, "model_params.name is 'VanillaVAE': actions exist only in a CTMCQVAE"),
    "causal_graph": ("ct_mcq_vae.yaml", "vae.yaml", None, "model_params.name is 'VanillaVAE': causal graphs exist only in a CTMCQVAE"),
    "latent_stats": ("vae.yaml", "mcq_vae.yaml", None,
                     f"model_params.name is 'MCQVAE': latent_stats needs a model with a Gaussian posterior ({GAUSSIAN}), got 'MCQVAE'"),
    "recon_stats": ("vae.yaml", "vae.yaml", "IWAE",
                    "model_params.name: recon_stats needs one reconstruction per image: 'IWAE' hands out [B, S, C, H, W] samples "
                    "(IWAE, MIWAE are not served)"),
    "fit_prior": ("vae.yaml", "mcq_vae.yaml", None,
                  "model_params.name is 'MCQVAE': sample_prior needs a model with a Gaussian posterior whose decoder takes "
                  f"[n, latent_dim] latents alone ({PRIOR}), got 'MCQVAE'"),
}


def _config(tmp_path, name, model_name=None, **trainer):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", name)))
    cfg["trainer_params"].update(trainer)
    if model_name is not None:
        cfg["model_params"]["name"] = model_name
    cfg["logging_params"]["save_dir"] = str(tmp_path / "logs")
    p = tmp_path / name
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def _refusal(command, argv) -> str:
    """The message ``main(argv)`` of the command ends with; torch's CPU generator is where it was."""
    main = importlib.import_module("ctvae_amd." + command).main
    before = torch.get_rng_state()
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert torch.equal(torch.get_rng_state(), before)
    return str(e.value)


@pytest.mark.parametrize("command", list(COMMANDS))
def test_every_command_refuses_alike_and_writes_nothing(command, tmp_path):
    own, other, other_name, reason = COMMANDS[command]
    missing = str(tmp_path / "missing.ckpt")
    assert _refusal(command, ["-c", _config(tmp_path, own)]) == \
        f"{command}: no checkpoint: give --checkpoint or set trainer_params.resume_from_checkpoint"
    assert _refusal(command, ["-c", _config(tmp_path, own), "--checkpoint", missing]) == f"{command}: checkpoint {missing} does not exist"
    assert _refusal(command, ["-c", _config(tmp_path, own, resume_from_checkpoint=missing)]) == \
        f"{command}: checkpoint {missing} does not exist"
    plain = tmp_path / "plain.ckpt"
    torch.save({"state_dict": {}, "epoch": 0}, plain)
    assert _refusal(command, ["-c", _config(tmp_path, own), "--checkpoint", str(plain), "--ema"]) == \
        f"{command}: --ema: checkpoint {plain} holds no ema_state_dict (it was written without exp_params.ema_decay)"
    assert _refusal(command, ["-c", _config(tmp_path, other, model_name=other_name)]) == f"{command}: {reason}"
    assert not os.path.exists(tmp_path / "logs")                    # nothing was written


@pytest.mark.parametrize("command", list(COMMANDS))
def test_the_last_host_refusal_leaves_the_generator_alone(command, tmp_path, monkeypatch):
    """As far as a host goes: a checkpoint that holds what ``--ema`` asks for is read, then the machine without a GPU is refused."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    both = tmp_path / "both.ckpt"
    torch.save({"state_dict": {}, "ema_state_dict": {}, "epoch": 0}, both)
    torch.manual_seed(4711)
    for flags in ([], ["--ema"]):
        assert _refusal(command, ["-c", _config(tmp_path, COMMANDS[command][0]), "--checkpoint", str(both)] + flags) == \
            f"{command}: ctvae_amd runs on MI355X GPUs only: the hot path has no CPU fallback"
    assert not os.path.exists(tmp_path / "logs")


def test_unpack_batch_and_batch_mode():
    from ctvae_amd.evalrun import batch_mode, unpack_batch

    class Labelled:
        uses_labels = True

    class Plain:
        uses_labels = False

    x, flat, column = torch.zeros(3, 2), torch.tensor([4, 5, 6]), torch.tensor([[4], [5], [6]])
    opts = {"mode": ["action"] * 3, "action": torch.eye(3)}
    assert unpack_batch((x, flat)) == (x, flat, {}) and unpack_batch([x, None]) == (x, None, {})
    got = unpack_batch((x, flat, opts))
    assert got[0] is x and got[1] is flat and got[2] is opts
    assert unpack_batch((x, flat, opts, "more"))[2] is opts
    for third in (None, "base", [("mode", "base")], 3):
        assert unpack_batch((x, flat, third)) == (x, flat, {})
    # one label per image becomes one class column only for a model that uses labels; without a model nothing is reshaped
    assert unpack_batch((x, flat))[1] is flat and unpack_batch((x, flat), None)[1] is flat
    assert unpack_batch((x, flat), Plain())[1] is flat and unpack_batch((x, flat), object())[1] is flat
    got = unpack_batch((x, flat, opts), Labelled())
    assert got[1].shape == (3, 1) and torch.equal(got[1], column) and got[2] is opts
    assert unpack_batch((x, column), Labelled())[1] is column                       # 2-D labels are left alone
    wide = torch.zeros(3, 40)
    assert unpack_batch((x, wide), Labelled())[1] is wide
    assert unpack_batch((x, None), Labelled())[1] is None and unpack_batch((x, [4, 5, 6]), Labelled())[1] == [4, 5, 6]
    with pytest.raises(ValueError):
        unpack_batch((x,))

    assert batch_mode({"mode": "causal"}) == "causal" and batch_mode({"mode": "causal"}, "base") == "causal"
    assert batch_mode({"mode": ["action", "action"]}) == "action" and batch_mode({"mode": ("base",)}, "causal") == "base"
    assert batch_mode({"mode": []}) is None and batch_mode({"mode": []}, "base") is None and batch_mode({"mode": ()}) is None
    assert batch_mode({}) is None and batch_mode({"action": 1}) is None
    assert batch_mode({}, "base") == "base" and batch_mode({}, default="base") == "base"


def test_npz_bytes_are_reproducible_and_load():
    from ctvae_amd import evalrun
    arrays = {"adjacency_mean": np.arange(8.0).reshape(2, 2, 2), "rows": np.array([3, 0])}
    data = evalrun.npz_bytes(arrays)
    assert data == evalrun.npz_bytes(arrays)
    back = np.load(io.BytesIO(data))
    assert sorted(back.files) == ["adjacency_mean", "rows"]
    assert np.array_equal(back["adjacency_mean"], arrays["adjacency_mean"]) and back["rows"].tolist() == [3, 0]
