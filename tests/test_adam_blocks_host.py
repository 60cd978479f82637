"""CPU: FlatAdam's block table (absent_grad "skip" / "skip_until_first"), the ``exp_params.adam_absent_grad`` key on its way
through VAEXperiment and a checkpoint, and -- with the CPU oracle -- the rule by which tests/test_adam_blocks_ct_gpu.py expects
CT-MCQ-VAE's ``ct_layer`` parameters to have a gradient or none in each mode."""
import os

import pytest
import torch
import yaml

from ctvae_amd import filler
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 12


def _ct_cfg():
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "ct_mcq_vae.yaml")))["model_params"]
    cfg["action_dim"] = A
    cfg["hidden_dims"] = list(cfg["hidden_dims"])
    return cfg


def _ct_model():
    from ctvae_amd.models import vae_models
    torch.manual_seed(3)
    return vae_models["CTMCQVAE"](**_ct_cfg())


def _param_floats(model, params):
    """Flat-buffer offsets of every element of the given parameters (packed weights are strided views)."""
    flat = model.flat_params
    idx = torch.arange(flat.numel())
    out = torch.zeros(flat.numel(), dtype=torch.bool)
    for p in params:
        off = (p.data_ptr() - flat.data_ptr()) // 4
        out[idx.as_strided(p.size(), p.stride(), off).reshape(-1)] = True
    return out


def _check_table(model, opt, params):
    start, stop = int(opt.slice.start or 0), int(opt.slice.stop)
    prev = 0
    covered = torch.zeros(stop - start, dtype=torch.bool)
    for lo, hi, kind, ref, member in opt.blocks:
        assert prev <= lo < hi <= stop - start, (lo, hi, prev)          # sorted, disjoint, inside the slice
        covered[lo:hi] = True
        prev = hi
    assert opt.table.lo.tolist() == [b[0] for b in opt.blocks] and opt.table.hi.tolist() == [b[1] for b in opt.blocks]
    assert opt.table.lo.dtype == torch.int32 and tuple(opt.table.state.shape) == (len(opt.blocks), 4)
    assert opt.table.state.tolist() == [[0.0, 1.0, 1.0, 0.0]] * len(opt.blocks)
    owned = _param_floats(model, params)[start:stop]
    assert bool(covered[owned].all()), "a parameter element lies in no block"
    return covered, owned


def test_block_table_of_ctmcqvae_ct_layer():
    from ctvae_amd.optim import FlatAdam
    m = _ct_model()
    sl = m.flat_range("ct_layer")
    opt = FlatAdam(m, lr=1e-3, params_slice=sl, absent_grad="skip")
    named = {k: p for k, p in m.named_parameters() if k.startswith("ct_layer.")}
    covered, owned = _check_table(m, opt, named.values())
    # every parameter of ct_layer is torch-level and contiguous: the blocks are exactly the parameters' floats -- the padding
    # behind the [13] bias bank and every alignment gap belong to no block
    assert torch.equal(covered, owned)
    assert int((~covered).sum()) > 0, "the slice has no gap: the [13]-float bias bank should be padded to 16"
    lo_of = {(p.data_ptr() - m.flat_params.data_ptr()) // 4 - sl.start: k for k, p in named.items()}
    assert sorted(lo_of) == [b[0] for b in opt.blocks] and all(named[lo_of[b[0]]].numel() == b[1] - b[0] for b in opt.blocks)
    bank = [(lo_of[b[0]], b[4]) for b in opt.blocks if b[2] == "bank"]
    assert len(bank) == 4 * (A + 1)
    for name, member in bank:                                  # one entry per scorer and bank, under the scorer's index
        assert name.startswith(f"ct_layer.graph_discovers.{member}."), (name, member)
    assert sorted(opt.table.hit_index[opt.table.hit_index >= 0].tolist()) == sorted(list(range(A + 1)) * 4)
    assert all(b[2] == "torch" for b in opt.blocks if "graph_discovers" not in lo_of[b[0]])
    # the whole model: the conv / codebook storage blocks join as kernel-managed blocks, one per _GradBlock
    full = FlatAdam(m, lr=1e-3, absent_grad="skip_until_first")
    _check_table(m, full, list(m.parameters()))
    assert [(b[0], b[1]) for b in full.blocks if b[2] == "kernel"] == [(g.lo, g.hi) for g in m._grad_blocks]


def test_block_table_of_vanilla_vae():
    from ctvae_amd.models import vae_models
    from ctvae_amd.optim import FlatAdam
    torch.manual_seed(0)
    m = vae_models["VanillaVAE"](in_channels=3, latent_dim=128)
    opt = FlatAdam(m, lr=1e-3, absent_grad="skip")
    _check_table(m, opt, list(m.parameters()))
    assert all(b[2] == "kernel" for b in opt.blocks) and len(opt.blocks) == len(m._grad_blocks)
    assert [(b[0], b[1]) for b in opt.blocks] == [(g.lo, g.hi) for g in m._grad_blocks]
    mu, var = m.fc_mu.weight._grad_block, m.fc_var.weight._grad_block
    assert mu is var                                            # the two heads are one GEMM, one block
    assert opt.table.hit_index.tolist() == [-1] * len(opt.blocks) and opt.table.nhits == 0
    # the record behind a kernel-managed block's activity: set by the gradient kernels' grad_target, cleared by zero_grad
    from ctvae_amd import kernels as K
    for lazy in (False, True):
        m.zero_grad(lazy=lazy)
        assert not any(g.written for g in m._grad_blocks)
        K.grad_target(m.fc_mu.weight)
        assert [g for g in m._grad_blocks if g.written] == [mu]
        m.gather_torch_grads()
        assert opt._host_pattern() == tuple(int(b[3] is mu) for b in opt.blocks)


def test_configure_optimizers_honours_adam_absent_grad():
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.optim import FlatAdam, absent_grad_setting
    m = _ct_model()
    base = {"LR": 1e-3, "kld_weight": 1.0, "update_parameters": "ct_layer"}
    exp = VAEXperiment(m, base)
    assert exp.optimizer.absent_grad == "zero" and exp.optimizer.table is None and m.ct_layer.graph_discovers.member_hits is None
    assert set(exp.optimizer.state_dict()) == {"exp_avg", "exp_avg_sq", "state"}
    assert set(exp.state_dict()["optimizer"]) == {"exp_avg", "exp_avg_sq", "state", "lr", "slice"}
    for mode in ("zero", "skip", "skip_until_first"):
        exp = VAEXperiment(m, dict(base, adam_absent_grad=mode))
        assert exp.optimizer.absent_grad == mode and (exp.optimizer.table is not None) == (mode != "zero")
    for bad in ("none", "Skip", "", 0, True):
        with pytest.raises(ValueError, match="'zero', 'skip' and 'skip_until_first'"):
            VAEXperiment(m, dict(base, adam_absent_grad=bad))
        with pytest.raises(ValueError, match="'zero', 'skip' and 'skip_until_first'"):
            FlatAdam(m, lr=1e-3, absent_grad=bad)
    assert absent_grad_setting(None) == "zero"
    # together with a gradient exchange the skip modes are refused when the experiment is built, the default is not
    class NoExchange:
        def restrict(self, sl):
            self.range = sl
    for mode in ("skip", "skip_until_first"):
        with pytest.raises(ValueError, match="DDP"):
            VAEXperiment(m, dict(base, adam_absent_grad=mode), ddp=NoExchange())
    VAEXperiment(m, dict(base, adam_absent_grad="zero"), ddp=NoExchange())
    # no CPU step, and no CPU test double of it: refused by name
    exp = VAEXperiment(m, dict(base, adam_absent_grad="skip"))
    with pytest.raises(RuntimeError, match="absent_grad='skip'.*no CPU"):
        exp.optimizer.step()


def test_yaml_round_trip_and_checkpoint_modes(tmp_path):
    """The key in a YAML as run.py reads it -> VAEXperiment -> checkpoint's trainer entry -> torch.load(weights_only=True) ->
    a run of the same mode; a run of another mode refuses it; a checkpoint without the key is a "zero" checkpoint."""
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "ct_mcq_vae.yaml")))
    assert "adam_absent_grad" not in cfg["exp_params"]
    cfg["exp_params"]["adam_absent_grad"] = "skip_until_first"
    path = tmp_path / "ct.yaml"
    path.write_text(yaml.safe_dump(cfg))
    config = yaml.safe_load(open(path))
    mp = dict(config["model_params"])
    torch.manual_seed(config["exp_params"].get("manual_seed", 0))
    model = vae_models[mp["name"]](**mp)
    exp = VAEXperiment(model, config["exp_params"])
    opt = exp.optimizer
    assert opt.absent_grad == "skip_until_first"
    sl = model.flat_range(config["exp_params"]["update_parameters"])
    assert (opt.slice.start, opt.slice.stop) == (sl.start, sl.stop) and opt.table.n == sl.stop - sl.start
    opt.table.state[:, 0] = torch.arange(opt.table.nb, dtype=torch.float32)      # something to carry
    opt.table.state[::2, 3] = 1.0
    torch.save({"trainer": exp.state_dict()}, tmp_path / "last.ckpt")
    trainer = torch.load(tmp_path / "last.ckpt", map_location="cpu", weights_only=True)["trainer"]
    assert trainer["optimizer"]["absent_grad"] == "skip_until_first"
    again = VAEXperiment(model, config["exp_params"])
    again.load_state_dict(trainer)
    assert torch.equal(again.optimizer.table.state, opt.table.state)
    for other in ("zero", "skip"):
        with pytest.raises(RuntimeError, match="adam_absent_grad"):
            VAEXperiment(model, dict(config["exp_params"], adam_absent_grad=other)).load_state_dict(trainer)
    zero = VAEXperiment(model, {k: v for k, v in config["exp_params"].items() if k != "adam_absent_grad"})
    old = zero.state_dict()
    assert "absent_grad" not in old["optimizer"] and "block_state" not in old["optimizer"]
    zero.load_state_dict(old)                                    # checkpoints without the key load under "zero" as before
    with pytest.raises(RuntimeError, match="adam_absent_grad"):
        again.load_state_dict(old)


# ---- the activity rule, on the CPU oracle --------------------------------------------------------------
SEQUENCE = [("base", None), ("action", [0, 3, 0, 3]), ("causal", [1, 5, 2, 9]), ("action", [3, 7, 7, 3]), ("base", None),
            ("action", [0, 0, 0, 0])]


def expected_active(name, mode, actions):
    """Whether the ct_layer parameter ``name`` (without the prefix) gets a gradient in a step of ``mode`` whose samples carry
    the action ids ``actions`` -- from the mode and the action list alone (tests/test_adam_blocks_ct_gpu.py uses the same
    rule): the mask network only where an intervention is formed (action and causal mode); scorer 0 always, scorer 1 + i iff
    action i occurs -- causal mode tries every action on every sample; a_dense never (its node has no outgoing edge);
    everything else always."""
    if name.startswith("a_dense."):
        return False
    if name.startswith("mask."):
        return mode != "base"
    if name.startswith("graph_discovers."):
        k = int(name.split(".")[1])
        if k == 0 or mode == "causal":
            return True
        return mode == "action" and (k - 1) in actions
    return True


@pytest.mark.parametrize("mode,actions", [SEQUENCE[0], SEQUENCE[1], SEQUENCE[2]], ids=["base", "action", "causal"])
def test_oracle_gradients_follow_the_activity_rule(mode, actions):
    """oracle/causal_cpu.ctmcq_step on 4 pairs: exactly the parameters the rule calls inactive come back with no or an
    all-zero gradient.  (The oracle evaluates scorer 1 + argmax(action) under a zero mask in base mode and feeds a_dense's
    node into a graph it has no edge into: all-zero gradients where the reference has none / zeros.)"""
    from oracle import causal_cpu as C
    seed, B = 41, 4
    cfg = _ct_cfg()
    conv = filler.fill_state(H.mcq_specs(H.CT_CONV_CFG), seed + 1)
    ctl = filler.fill_state(H.ct_layer_specs(A), seed + 3)
    sd = {**conv, **{"ct_layer." + k: v for k, v in ctl.items() if k != "pos_encoding.pe"}}
    hp = dict(alpha=cfg["c_alpha"], beta=cfg["c_beta"], delta=cfg["c_delta"], epsilon=cfg["c_epsilon"], noise=cfg["noise"])
    mcfg = dict(num_embeddings=cfg["num_embeddings"], codebooks=cfg["codebooks"], beta=cfg["beta"], skip_transition=False)
    x, y, _ = filler.synthetic_pairs(seed, B, A)
    double = H.GNNDouble(64, A + 1, seed + 5)
    kw = {}
    if mode != "base":
        kw = dict(input_y=y, action=torch.nn.functional.one_hot(torch.tensor(actions), A).float())
    _, grads, _ = C.ctmcq_step(sd, mcfg, cfg["gamma"], x, H.CTNoise(seed, "cpu"), lambda n, a: double(n, a), mode, hp=hp, **kw)
    checked = 0
    for k, g in grads.items():
        if not k.startswith("ct_layer.") or k.startswith("ct_layer.graph_transitioner."):
            continue
        want = expected_active(k[len("ct_layer."):], mode, actions or [])
        assert bool((g != 0).any()) == want, (mode, k, want, float(g.abs().max()))
        checked += 1
    assert checked == 2 + 2 + 4 * (A + 1)
