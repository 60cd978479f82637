"""GPU: FlatAdam's absent_grad modes through CT-MCQ-VAE and the training harness (action_dim 12, ``update_parameters:
ct_layer``, 4 pairs per batch): per step the blocks that step are the ones the mode and the batch's actions call for, the
trajectory is torch.optim.Adam's with ``.grad = None`` for the others, a replayed hipGraph steps like the eager harness, and the
default ("zero") does move a scorer whose action is absent -- which is what tells the modes apart.

The expected activity comes from tests/test_adam_blocks_host.expected_active (mode and action list alone; the CPU oracle is
checked against the same rule there), never from the optimizer's own flags.  Bounds: those of tests/test_grad_clip_gpu.py,
restated in tests/test_adam_blocks_gpu.py."""
import os

import pytest
import torch
import yaml

from ctvae_amd import filler
from tests import helpers as H
from tests.test_adam_blocks_gpu import _assert_close_moment, _assert_close_ulp, _f32
from tests.test_adam_blocks_host import SEQUENCE, expected_active

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B, LR, WD = 12, 4, 5e-4, 1e-4
PARAMS = {"LR": LR, "weight_decay": WD, "kld_weight": 0.00025, "update_parameters": "ct_layer"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _model(dev, seed=5):
    from ctvae_amd.models import vae_models
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "ct_mcq_vae.yaml")))["model_params"]
    cfg["action_dim"] = A
    torch.manual_seed(seed)
    m = vae_models["CTMCQVAE"](**cfg)
    m.load_state_dict(filler.fill_state(H.mcq_specs(H.CT_CONV_CFG), seed + 1), strict=False)
    return m.to(dev).train()


def _batches(dev, rounds=1):
    out = []
    for i, (mode, actions) in enumerate(SEQUENCE * rounds):
        x, y, _ = filler.synthetic_pairs(300 + i, B, A)
        opts = {"mode": [mode] * B}
        if mode != "base":
            opts.update(input_y=y.to(dev), action=torch.nn.functional.one_hot(torch.tensor(actions), A).float().to(dev))
        out.append((x.to(dev), torch.zeros(B, device=dev), opts))
    return out


class _FixedNoise:
    """One cached device tensor per (tag, shape): the same noise in every step, eager or replayed, and no host-to-device copy
    inside a capture."""

    def __init__(self, dev):
        self.dev, self.cache = dev, {}

    def draw(self, tag, shape, p=0.0):
        key = (tag, tuple(shape), p)
        if key not in self.cache:
            self.cache[key] = filler.ct_noise(77, tag, len(self.cache) % 5, shape, p).to(self.dev)
        return self.cache[key]


@pytest.fixture()
def fixed_noise(dev):
    from ctvae_amd.models import causal
    prev = causal.set_noise_source(_FixedNoise(dev))
    yield
    causal.set_noise_source(prev)


def _layout(m, opt):
    """name (under ct_layer) -> (lo, hi) inside the optimizer's slice; and the names in block order."""
    start = opt.slice.start
    spans = {k[len("ct_layer."):]: ((p.data_ptr() - m.flat_params.data_ptr()) // 4 - start, p.numel())
             for k, p in m.named_parameters() if k.startswith("ct_layer.")}
    spans = {k: (lo, lo + n) for k, (lo, n) in spans.items()}
    by_lo = {lo: k for k, (lo, _) in spans.items()}
    return spans, by_lo


def _eager_steps(dev, mode):
    """The six batches one by one through VAEXperiment's own step pieces.  Returns the model, the optimizer, the slice of
    the gradient buffer after each backward, the device flags of each step and the slice of the parameters after each step."""
    from ctvae_amd import kernels as K
    from ctvae_amd.experiment import VAEXperiment
    m = _model(dev)
    params = dict(PARAMS, hipgraph=False)
    if mode is not None:
        params["adam_absent_grad"] = mode
    exp = VAEXperiment(m, params)
    opt = exp.optimizer
    p0 = m.flat_params[opt.slice].clone()
    grads, flags, after = [], [], []
    for i, batch in enumerate(_batches(dev)):
        m.zero_grad(lazy=True)
        K.backward(exp.training_step(batch, i))
        grads.append(m.flat_grads[opt.slice].clone())
        exp.optimizer_step()
        torch.cuda.synchronize()
        flags.append(opt.table.active.cpu().tolist() if opt.table is not None else None)
        after.append(m.flat_params[opt.slice].clone())
    return m, opt, p0, grads, flags, after


def test_skip_follows_torch_adam_with_absent_gradients(dev, fixed_noise):
    m, opt, p0, grads, flags, after = _eager_steps(dev, "skip")
    spans, by_lo = _layout(m, opt)
    names = [by_lo[b[0]] for b in opt.blocks]
    assert sorted(names) == sorted(spans)                              # one block per parameter of ct_layer
    ref = {k: torch.nn.Parameter(p0[lo:hi].cpu().double()) for k, (lo, hi) in spans.items()}
    topt = torch.optim.Adam(list(ref.values()), lr=_f32(LR), betas=(_f32(0.9), _f32(0.999)), eps=_f32(1e-8), weight_decay=_f32(WD))
    before = p0
    for s, (mode, actions) in enumerate(SEQUENCE):
        want = {k: expected_active(k, mode, actions or []) for k in spans}
        assert flags[s] == [int(want[k]) for k in names], \
            (s, mode, [k for k, f in zip(names, flags[s]) if int(want[k]) != f])
        g = grads[s].cpu()
        for k, (lo, hi) in spans.items():
            if want[k]:
                ref[k].grad = g[lo:hi].double()
            else:
                assert not bool(g[lo:hi].any()), f"step {s} ({mode}): {k} should have no gradient"
                ref[k].grad = None
                assert torch.equal(before[lo:hi], after[s][lo:hi]), f"step {s} ({mode}): {k} moved without a gradient"
        topt.step()
        before = after[s]
    torch.cuda.synchronize()
    for k, (lo, hi) in spans.items():
        st = topt.state[ref[k]] if ref[k] in topt.state else None
        if st is None or "step" not in st:                              # never had a gradient: a_dense
            assert k.startswith("a_dense.") and not bool(opt.exp_avg[lo:hi].any()) and torch.equal(p0[lo:hi], after[-1][lo:hi])
            continue
        _assert_close_moment(opt.exp_avg[lo:hi].cpu().double(), st["exp_avg"], k + " exp_avg")
        _assert_close_moment(opt.exp_avg_sq[lo:hi].cpu().double(), st["exp_avg_sq"], k + " exp_avg_sq")
        _assert_close_ulp(after[-1][lo:hi].cpu().double(), ref[k].detach(), LR, k + " param")
    steps = dict(zip(names, opt.block_steps().cpu().tolist()))
    for k in spans:
        assert steps[k] == sum(expected_active(k, mode, actions or []) for mode, actions in SEQUENCE), k
    assert steps["graph_discovers.1.0.weight"] == 3 and steps["graph_discovers.8.2.bias"] == 2 and steps["mask.0.weight"] == 4


def test_default_moves_a_scorer_whose_action_is_absent(dev, fixed_noise):
    """Step 4 (actions {3, 7}): scorer 1 (action 0) had a gradient in step 2 and has none now.  Under "zero" its momentum moves
    it; under "skip" it stands still (asserted for every such block above) -- the two modes differ exactly here."""
    m, opt, p0, grads, flags, after = _eager_steps(dev, None)
    assert opt.absent_grad == "zero" and opt.table is None
    spans, _ = _layout(m, opt)
    lo, hi = spans["graph_discovers.1.0.weight"]
    assert not bool(grads[3][lo:hi].any())
    assert not torch.equal(after[2][lo:hi], after[3][lo:hi])
    lo, hi = spans["mask.0.weight"]                                     # and the mask network in the second base batch
    assert not bool(grads[4][lo:hi].any()) and not torch.equal(after[3][lo:hi], after[4][lo:hi])


@pytest.mark.parametrize("mode", ["skip", "skip_until_first"])
def test_replayed_graph_steps_like_the_eager_harness(dev, fixed_noise, mode):
    """VAEXperiment.fit over the sequence three times: the action signature is captured at its fourth batch and replayed five
    times with other action sets than the capture step's, base is replayed twice.  Parameters, moments and per-block counters
    equal the all-eager run bit for bit."""
    from ctvae_amd.experiment import VAEXperiment
    batches = _batches(dev, rounds=3)
    finals = {}
    for graphed in (False, True):
        m = _model(dev)
        exp = VAEXperiment(m, dict(PARAMS, hipgraph=graphed, adam_absent_grad=mode))
        exp.fit(lambda: iter(batches), None, max_epochs=1)
        torch.cuda.synchronize()
        if graphed:
            replays = sorted(g.seen - g.WARM for g in exp._graphed.values() if g.graph is not None)
            assert replays == [3, 6], replays                           # base and action captured; causal (3 batches) stays eager
        opt = exp.optimizer
        finals[graphed] = [m.flat_params.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.table.state.clone()]
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq", "block_state"), finals[False], finals[True]):
        assert torch.isfinite(a).all() and torch.equal(a, b), (name, float((a - b).abs().max()))
    spans_m, spans_opt = m, exp.optimizer
    spans, by_lo = _layout(spans_m, spans_opt)
    steps = dict(zip([by_lo[b[0]] for b in spans_opt.blocks], spans_opt.block_steps().cpu().tolist()))
    seen = {k: False for k in spans}
    want = {k: 0 for k in spans}
    for smode, actions in SEQUENCE * 3:
        for k in spans:
            on = expected_active(k, smode, actions or [])
            seen[k] = seen[k] or on
            want[k] += int(on or (mode == "skip_until_first" and seen[k]))
    assert steps == {k: float(v) for k, v in want.items()}
