"""CPU: the float64 NumPy restatement of the code prior (tests/codeprior_checks.py) against hand-made tables and a known chain, and
every host-side refusal of ``exp_params.code_prior``: ``codeprior.code_prior_setting``, the unserved models, ``run.exp_code_prior``
and the ``fit_code_prior`` command."""
import importlib
import math
import os

import numpy as np
import pytest
import torch
import yaml

from . import codeprior_checks as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement is self-consistent ------------------------------------------------------------------------------------------
def _forced_tables(K, C, H, W):
    """Every row of every table has ONE non-zero code: position p -> (p + c) % K, context row r -> (r + 1 + c) % K (the
    boundary row K included)."""
    tables = R.empty_tables(K, C, H, W)
    for c in range(C):
        for p in range(H * W):
            tables[0][c, p, (p + c) % K] = 3
        for t in tables[1:]:
            for r in range(K + 1):
                t[c, r, (r + 1 + c) % K] = 2 + r
    return tables


@pytest.mark.parametrize("expert", [1, 2, 3, 4])
def test_forced_tables_sample_the_forced_sequence_and_score_it_zero(expert):
    K, C, H, W = 5, 2, 3, 4
    tables = _forced_tables(K, C, H, W)
    lam = np.zeros((C, R.J))
    lam[:, expert] = 1.0
    u = np.random.default_rng(expert).random((2, H * W, C, 2))
    got = R.sample(tables, lam, u, H, W)
    want = np.empty((C, H, W), dtype=np.int64)
    for p in range(H * W):
        h, w = divmod(p, W)
        for c in range(C):
            if expert == 1:
                want[c, h, w] = (p + c) % K
            else:
                ctx = {2: want[c, h, w - 1] if w > 0 else K,            # the boundary rows at w = 0, h = 0 and c = 0
                       3: want[c, h - 1, w] if h > 0 else K,
                       4: want[c - 1, h, w] if c > 0 else K}[expert]
                want[c, h, w] = (ctx + 1 + c) % K
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want)      # whatever the uniforms are
    logp, resp, bad, _, _ = R.score(got, tables, lam, K)
    assert np.array_equal(logp, np.zeros((2, C))) and not bad.any()           # log 1 = 0 exactly
    assert np.array_equal(resp[:, :, expert], np.full((2, C), float(H * W)))


def test_contexts_use_the_boundary_symbol():
    K = 7
    inds = np.arange(2 * 2 * 3).reshape(1, 2, 2, 3) % K
    pos, left, up, prev = R.contexts(inds, K)
    assert (left[..., 0] == K).all() and np.array_equal(left[..., 1:], inds[..., :-1])
    assert (up[:, :, 0] == K).all() and np.array_equal(up[:, :, 1:], inds[:, :, :-1])
    assert (prev[:, 0] == K).all() and np.array_equal(prev[:, 1:], inds[:, :-1])
    assert np.array_equal(pos[0, 1], np.arange(6).reshape(2, 3))


def test_a_zero_total_row_scores_and_samples_as_uniform():
    K, C, H, W = 6, 1, 1, 2
    tables = R.empty_tables(K, C, H, W)                     # every row is empty
    lam = np.array([[0.0, 0.25, 0.25, 0.25, 0.25]])
    inds = np.array([[[[4, 1]]]])
    logp, resp, _, _, _ = R.score(inds, tables, lam, K)
    assert abs(logp[0, 0] - 2 * math.log(1.0 / K)) < 1e-15
    assert np.allclose(resp[0, 0], [0.0, 0.5, 0.5, 0.5, 0.5], rtol=0, atol=1e-15)
    u = np.array([[[[0.3, 0.0]], [[0.9, np.nextafter(1.0, 0.0)]]]])
    assert R.sample(tables, lam, u, H, W).ravel().tolist() == [0, K - 1]
    u[0, :, 0, 1] = [0.5, 1.0 / 3.0]
    assert R.sample(tables, lam, u, H, W).ravel().tolist() == [3, int(np.floor((1.0 / 3.0) * 6.0))]


def test_counts_totals_and_invalid():
    K = 4
    inds = np.array([[[[0, 1], [2, 3]]], [[[1, 9], [1, 1]]]])                # image 1 holds a 9 at (0, 1)
    tables, invalid = R.count(inds, K)
    # the 9 itself, and its lower neighbour (1, 1) whose upper context it is: 2 tokens left out; (1, 0) has left = 1: fine
    assert invalid == 2
    assert all(int(t.sum()) == 8 - 2 for t in tables)
    assert tables[1][0, K, 0] == 1 and tables[1][0, K, 2] == 1 and tables[1][0, K, 1] == 2      # left boundary rows
    assert tables[2][0, 0, 2] == 1 and tables[2][0, 1, 3] == 1 and tables[2][0, 1, 1] == 1      # up
    assert tables[3][0, K].tolist() == tables[0][0].sum(axis=0).tolist()                        # C = 1: all previous are K
    again, invalid2 = R.count(inds, K, tables)
    assert invalid2 == 2 and all(np.array_equal(a, 2 * t) for a, t in zip(again, tables))


def test_pick_expert_boundaries():
    lam = np.array([0.25, 0.25, 0.0, 0.25, 0.25])
    assert R.pick_expert(0.0, lam) == 0 and R.pick_expert(np.nextafter(0.25, 0), lam) == 0
    assert R.pick_expert(0.25, lam) == 1                       # u1 on the boundary belongs to the next expert
    assert R.pick_expert(0.5, lam) == 3                        # the empty expert 2 is never picked
    assert R.pick_expert(np.nextafter(1.0, 0), lam) == 4
    assert R.pick_expert(0.9, np.array([0.5, 0.0, 0.0, 0.0, 0.0])) == R.J - 1      # none qualifies


# ---- a known first-order chain ---------------------------------------------------------------------------------------------------
CHAIN = dict(K=16, C=2, H=4, W=8, stay=0.7)


@pytest.fixture(scope="module")
def chain():
    x = R.chain_fixture(20251, 192, **CHAIN)
    K = CHAIN["K"]
    tables, invalid = R.count(x[0::2], K)
    lam = R.em(x[1::2], tables, K, 20, 1e-3)
    return x, tables, lam, invalid


def test_em_keeps_lambda_a_distribution_with_the_floor(chain):
    _, _, lam, invalid = chain
    assert invalid == 0
    assert np.allclose(lam.sum(axis=1), 1.0, rtol=0, atol=1e-14) and (lam >= 0).all()
    assert (lam[:, 0] >= 1e-3 * (1 - 1e-12)).all()
    assert (lam.argmax(axis=1) == 2).all()                      # the structure is the left neighbour's


def test_held_out_nats_are_clearly_below_ln_k(chain):
    """The chain's conditional entropy: the first column is uniform (ln 16 = 2.77), every other repeats its left neighbour with
    probability 0.7 + 0.3 / 16, i.e. 1.36 nats; the column mean is 1.54.  The prior, fitted on 96 grids and scored on fresh
    ones, must come within half a nat of that -- far below ln K."""
    x, tables, lam, _ = chain
    K, stay = CHAIN["K"], CHAIN["stay"]
    fresh = R.chain_fixture(777, 64, **CHAIN)
    nats = R.nats_per_code(fresh, tables, lam, K)
    p_same = stay + (1 - stay) / K
    p_other = (1 - stay) / K
    h_cond = -(p_same * math.log(p_same) + (K - 1) * p_other * math.log(p_other))
    truth = (math.log(K) + (CHAIN["W"] - 1) * h_cond) / CHAIN["W"]
    print(f"held-out nats per code {nats:.4f}, the chain's entropy rate {truth:.4f}, ln K {math.log(K):.4f}")
    assert truth <= nats + 0.02 and nats < truth + 0.5 < math.log(K) - 0.5


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_setting_defaults_and_absent():
    from ctvae_amd.codeprior import code_prior_setting
    assert code_prior_setting(None) is None
    assert code_prior_setting({"type": "markov"}) == {"type": "markov", "em_iters": 20, "uniform_floor": 1e-3}
    assert code_prior_setting({"type": "markov", "em_iters": 3, "uniform_floor": 0.5}) == \
        {"type": "markov", "em_iters": 3, "uniform_floor": 0.5}


BAD_SETTINGS = [
    (True, "code_prior must be a mapping with type: markov, got True"),
    ("markov", "code_prior must be a mapping with type: markov, got 'markov'"),
    ({}, "code_prior.type must be markov, got None"),
    ({"type": "pixelcnn"}, "code_prior.type must be markov, got 'pixelcnn'"),
    ({"type": "markov", "order": 2}, "code_prior has unknown field(s) order; known: type, em_iters, uniform_floor"),
    ({"type": "markov", "em_iters": 2.0}, "code_prior.em_iters must be an integer of at least 1, got 2.0"),
    ({"type": "markov", "em_iters": True}, "code_prior.em_iters must be an integer of at least 1, got True"),
    ({"type": "markov", "em_iters": 0}, "code_prior.em_iters must be an integer of at least 1, got 0"),
    ({"type": "markov", "uniform_floor": 0.0}, "code_prior.uniform_floor must be a float inside (0, 1), got 0.0"),
    ({"type": "markov", "uniform_floor": 1.0}, "code_prior.uniform_floor must be a float inside (0, 1), got 1.0"),
    ({"type": "markov", "uniform_floor": 1}, "code_prior.uniform_floor must be a float inside (0, 1), got 1"),
    ({"type": "markov", "uniform_floor": "small"}, "code_prior.uniform_floor must be a float inside (0, 1), got 'small'"),
    ({"type": "markov", "uniform_floor": float("nan")}, "code_prior.uniform_floor must be a float inside (0, 1), got nan"),
]


@pytest.mark.parametrize("value,message", BAD_SETTINGS)
def test_setting_refusals_name_the_field(value, message):
    from ctvae_amd import run
    from ctvae_amd.codeprior import code_prior_setting
    with pytest.raises(ValueError) as e:
        code_prior_setting(value)
    assert str(e.value) == message
    with pytest.raises(SystemExit) as e:
        run.exp_code_prior({"exp_params": {"code_prior": value}, "model_params": {"name": "MCQVAE"}})
    assert str(e.value) == "exp_params." + message


def test_unserved_models_are_refused_by_name():
    from ctvae_amd import codeprior, run
    from ctvae_amd.models import vae_models
    assert codeprior.CODE_PRIOR_MODELS == ("MCQVAE", "VQVAE")
    on = {"type": "markov"}
    for name in ("MCQVAE", "VQVAE"):
        assert codeprior.prior_supported(vae_models[name])
        assert run.exp_code_prior({"exp_params": {"code_prior": on}, "model_params": {"name": name}})["em_iters"] == 20
    served = {vae_models[n] for n in codeprior.CODE_PRIOR_MODELS}
    for name, cls in vae_models.items():
        if cls in served:
            continue
        assert not codeprior.prior_supported(cls)
        with pytest.raises(SystemExit) as e:
            run.exp_code_prior({"exp_params": {"code_prior": on}, "model_params": {"name": name}})
        msg = str(e.value)
        assert msg.startswith("exp_params.code_prior ") and repr(name) in msg and msg.endswith("(model_params.name)")
        if cls.__name__ == "CTMCQVAE":
            assert "does not serve CTMCQVAE" in msg and "causal-transition layer" in msg and "out of scope" in msg
        else:
            assert "needs a quantising model" in msg and "MCQVAE, VQVAE" in msg
    with pytest.raises(SystemExit) as e:
        run.exp_code_prior({"exp_params": {"code_prior": on}, "model_params": {"name": "NoSuchVAE"}})
    assert "'NoSuchVAE'" in str(e.value)


def test_run_reads_an_absent_key_as_none():
    from ctvae_amd import run
    for name in ("mcq_vae.yaml", "vae.yaml", "ct_mcq_vae.yaml"):
        cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", name)))
        assert "code_prior" not in cfg["exp_params"]
        assert run.exp_code_prior(cfg) is None


def test_grid_buffer_grows_by_doubling():
    from ctvae_amd.codeprior import CodeGridBuffer
    buf = CodeGridBuffer("cpu", capacity=2)
    assert buf.view().size(0) == 0 and buf.shape is None
    rows = torch.arange(5 * 2 * 3 * 3, dtype=torch.int64).reshape(5, 2, 3, 3)
    buf.append(rows[:1])
    buf.append(rows[1:2])
    assert buf._buf.size(0) == 2
    buf.append(rows[2:])
    assert buf._buf.size(0) == 8 and buf.rows == 5 and buf.shape == (2, 3, 3) and torch.equal(buf.view(), rows)
    with pytest.raises(ValueError, match=r"CodeGridBuffer.append takes int64 indices \[B, 2, 3, 3\]"):
        buf.append(rows[:, :1])
    with pytest.raises(ValueError, match="CodeGridBuffer.append takes int64"):
        buf.append(rows.float())
    single = CodeGridBuffer("cpu")
    single.append(rows[:, 0])                                   # VQVAE's [B, H, W] gets its codebook axis
    assert single.shape == (1, 3, 3)
    buf.clear()
    assert buf.view().size(0) == 0


def test_prior_limits_are_refused_by_name():
    from ctvae_amd.codeprior import MarkovCodePrior
    for args, word in (((0, 1, 2, 2), "K must lie in 1..512"), ((513, 1, 2, 2), "K must lie in 1..512"),
                       ((8, 0, 2, 2), "C must be at least 1"), ((8, 1, 0, 2), "H must be at least 1"),
                       ((8, 1, 2, 0), "W must be at least 1"), ((8.0, 1, 2, 2), "K must be an integer")):
        with pytest.raises(ValueError, match=word):
            MarkovCodePrior(*args, device="cpu")
    p = MarkovCodePrior(8, 1, 2, 2, device="cpu")
    with pytest.raises(RuntimeError, match="count or load the tables first"):
        p.state_dict()
    with pytest.raises(RuntimeError, match="GPU only"):
        p.count(torch.zeros(1, 1, 2, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"count takes inds \[B, 1, 2, 2\]"):
        p.count(torch.zeros(1, 2, 2, 2, dtype=torch.int64))


# ---- the command: the five refusals every checkpoint command words alike (tests/test_tool_host.py) ---------------------------------
COMMAND = "fit_code_prior"
REASON = ("model_params.name is 'VanillaVAE': code_prior needs a quantising model whose decoder takes the quantised grid alone "
          "(MCQVAE, VQVAE), got 'VanillaVAE'")


def _config(tmp_path, name, **trainer):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", name)))
    cfg["trainer_params"].update(trainer)
    cfg["logging_params"]["save_dir"] = str(tmp_path / "logs")
    p = tmp_path / name
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def _refusal(argv) -> str:
    main = importlib.import_module("ctvae_amd." + COMMAND).main
    before = torch.get_rng_state()
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert torch.equal(torch.get_rng_state(), before)
    return str(e.value)


def test_the_command_refuses_like_the_others_and_writes_nothing(tmp_path):
    own = "mcq_vae.yaml"
    missing = str(tmp_path / "missing.ckpt")
    assert _refusal(["-c", _config(tmp_path, own)]) == \
        f"{COMMAND}: no checkpoint: give --checkpoint or set trainer_params.resume_from_checkpoint"
    assert _refusal(["-c", _config(tmp_path, own), "--checkpoint", missing]) == f"{COMMAND}: checkpoint {missing} does not exist"
    assert _refusal(["-c", _config(tmp_path, own, resume_from_checkpoint=missing)]) == \
        f"{COMMAND}: checkpoint {missing} does not exist"
    plain = tmp_path / "plain.ckpt"
    torch.save({"state_dict": {}, "epoch": 0}, plain)
    assert _refusal(["-c", _config(tmp_path, own), "--checkpoint", str(plain), "--ema"]) == \
        f"{COMMAND}: --ema: checkpoint {plain} holds no ema_state_dict (it was written without exp_params.ema_decay)"
    assert _refusal(["-c", _config(tmp_path, "vae.yaml")]) == f"{COMMAND}: {REASON}"
    ct = _refusal(["-c", _config(tmp_path, "ct_mcq_vae.yaml")])
    assert ct.startswith(f"{COMMAND}: model_params.name is 'CTMCQVAE': code_prior does not serve CTMCQVAE") and "out of scope" in ct
    assert not os.path.exists(tmp_path / "logs")


def test_the_commands_own_flags_are_refused_by_name(tmp_path):
    cfg = _config(tmp_path, "mcq_vae.yaml")
    assert _refusal(["-c", cfg, "--em-iters", "0"]) == f"{COMMAND}: --em-iters must be an integer of at least 1, got 0"
    assert _refusal(["-c", cfg, "--uniform-floor", "1.5"]) == f"{COMMAND}: --uniform-floor must be a float inside (0, 1), got 1.5"
    assert _refusal(["-c", cfg, "--rows", "1"]) == f"{COMMAND}: --rows must be at least 2, got 1"
    assert _refusal(["-c", cfg, "--samples", "0"]) == f"{COMMAND}: --samples must be at least 1, got 0"
    assert not os.path.exists(tmp_path / "logs")


def test_the_last_host_refusal_leaves_the_generator_alone(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    both = tmp_path / "both.ckpt"
    torch.save({"state_dict": {}, "ema_state_dict": {}, "epoch": 0}, both)
    torch.manual_seed(4711)
    for flags in ([], ["--ema"]):
        assert _refusal(["-c", _config(tmp_path, "mcq_vae.yaml"), "--checkpoint", str(both)] + flags) == \
            f"{COMMAND}: ctvae_amd runs on MI355X GPUs only: the hot path has no CPU fallback"
    assert not os.path.exists(tmp_path / "logs")
