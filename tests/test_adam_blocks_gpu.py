"""GPU: the block-aware fused Adam step (FlatAdam absent_grad "skip" / "skip_until_first", ctvae_adam_step_blocks) alone, on a
synthetic flat buffer with a hand-made block table.

The yardstick is ``torch.optim.Adam`` on the CPU in double over ONE TENSOR PER BLOCK, fed the same gradients: for "skip" a block
without a gradient has ``.grad = None``; for "skip_until_first" it has None until its first gradient and a zero tensor afterwards
(``zero_grad(set_to_none=False)``).  The acceptance bounds are those tests/test_grad_clip_gpu.py applies to the fused step
against torch, restated here: parameters within 1e-3 * lr plus 2 fp32 ulp, moments to rtol 1e-5 / atol 1e-6 of the largest
entry, the pre-clip norm to 1e-5 relative.  What must not move is compared bit for bit."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

LR = 1e-3
# block sizes 1, 3, 4, 5, 17, 1023; a gap that holds a whole 16-byte quad ([1056, 1060)); two adjacent blocks whose shared
# boundary 1130 is no multiple of 4 and which are never active together; one block of 67601 >= 2*256*4*33 floats (66 workgroups:
# three first-level ticket groups); three floats behind the last block, and N % 4 == 1 (a partial last quad)
RANGES = [(0, 1), (1, 4), (4, 8), (8, 13), (13, 30), (30, 1053), (1060, 1130), (1130, 1201), (1201, 68802)]
N = 68805
STEPS = 6
#          step:  1  2  3  4  5  6
ACTIVE = [[1, 1, 1, 1, 1, 1],      # always
          [0, 0, 0, 0, 0, 0],      # never
          [0, 0, 1, 1, 0, 1],      # first at step 3
          [1, 0, 1, 1, 0, 1],      # active, absent, active again
          [1, 1, 1, 1, 1, 1],
          [1, 0, 1, 0, 1, 0],
          [1, 0, 1, 0, 1, 0],      # opposite to its right neighbour in every step
          [0, 1, 0, 1, 0, 1],
          [1, 1, 0, 1, 1, 1]]      # the large block misses step 3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _assert_close_ulp(got, want, lr, what):
    """Parameters: within 1e-3 * lr plus 2 ulp of |p|, elementwise (tests/test_grad_clip_gpu.py)."""
    a = want.abs().float()
    ulp = (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).to(want.dtype)      # fp32 ulp
    err = (got - want).abs()
    bad = err > 1e-3 * lr + 2 * ulp
    assert not bool(bad.any()), (what, float(err.max()), int(bad.sum()))


def _assert_close_moment(got, want, what):
    """Moments (tests/test_grad_clip_gpu.py)."""
    scale = float(want.abs().max())
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6 * scale + 1e-30, msg=lambda m: f"{what}: {m}")


def _f32(x):
    """x as the fp32 device state holds it, back in a Python float."""
    return float(torch.tensor(float(x), dtype=torch.float32))


class FlatModel:
    """The four things FlatAdam asks of a model: the flat buffers, gather_torch_grads, zero_grad and adam_blocks -- here a
    hand-made table at `start` floats into the buffers (start = 1: nothing is 16-byte aligned, the scalar paths), whose
    blocks report the activity the test sets in ``present``."""

    def __init__(self, dev, start=0, seed=5):
        g = torch.Generator().manual_seed(seed)
        self.start = start
        self.flat_params = (torch.randn(start + N, generator=g) * 0.3).to(dev)
        self.flat_grads = torch.zeros(start + N, device=dev)
        self.present = [True] * len(RANGES)

    def gather_torch_grads(self):
        pass

    def zero_grad(self):
        self.flat_grads.zero_()

    def adam_blocks(self):
        return [(self.start + lo, self.start + hi, "flag", (lambda i=i: self.present[i]), None) for i, (lo, hi) in enumerate(RANGES)]


def _optimizer(model, mode, wd=0.0, **clip):
    from ctvae_amd.optim import FlatAdam
    return FlatAdam(model, lr=LR, weight_decay=wd, params_slice=slice(model.start, model.start + N), absent_grad=mode, **clip)


def _grads(step, active=None, fill=0.0):
    """The step's gradient over the N floats: random in the active blocks, `fill` in the others; zero in the gaps."""
    gen = torch.Generator().manual_seed(1000 + step)
    g = torch.zeros(N)
    for b, (lo, hi) in enumerate(RANGES):
        r = torch.randn(hi - lo, generator=gen) * (0.5 + 0.25 * b)
        g[lo:hi] = r if (active is None or active[b][step]) else fill
    return g


def _in_blocks():
    mask = torch.zeros(N, dtype=torch.bool)
    for lo, hi in RANGES:
        mask[lo:hi] = True
    return mask


@pytest.mark.parametrize("start", [0, 1])
@pytest.mark.parametrize("case", ["plain", "weight_decay", "value", "norm"])
@pytest.mark.parametrize("mode", ["skip", "skip_until_first"])
def test_blocks_follow_torch_adam_per_block(dev, mode, case, start):
    wd = 0.0 if case == "plain" else 1e-2
    clip = {}
    if case == "value":
        clip = dict(clip_val=_f32(0.4), clip_algorithm="value")
    elif case == "norm":
        clip = dict(clip_val=_f32(20.0), clip_algorithm="norm")       # well below every step's norm (asserted)
    model = FlatModel(dev, start)
    opt = _optimizer(model, mode, wd, **clip)
    sl = slice(start, start + N)
    p0 = model.flat_params[sl].cpu()
    ref = [torch.nn.Parameter(p0[lo:hi].double().clone()) for lo, hi in RANGES]
    topt = torch.optim.Adam(ref, lr=_f32(LR), betas=(_f32(0.9), _f32(0.999)), eps=_f32(1e-8), weight_decay=_f32(wd))
    seen = [False] * len(RANGES)
    # what a block without a gradient holds in the gradient buffer: zeros -- or, where nothing but the update itself could read
    # it ("skip" without the norm pass), NaN, so that a read of an inactive block's gradient shows
    poison = float("nan") if (mode == "skip" and case != "norm") else 0.0
    gaps = ~_in_blocks()
    for s in range(STEPS):
        g = _grads(s, ACTIVE, poison)
        model.flat_grads[sl].copy_(g)
        stepping = []
        for b, (lo, hi) in enumerate(RANGES):
            on = bool(ACTIVE[b][s])
            model.present[b] = on
            seen[b] = seen[b] or on
            if on:
                ref[b].grad = g[lo:hi].double().clone()
            elif mode == "skip_until_first" and seen[b]:
                ref[b].grad = torch.zeros_like(ref[b])
            else:
                ref[b].grad = None
            stepping.append(ref[b].grad is not None)
        if case == "norm":
            ref_norm = float(torch.nn.utils.clip_grad_norm_(ref, clip["clip_val"]))
            assert ref_norm > clip["clip_val"]
        elif case == "value":
            assert any(bool((q.grad.abs() > clip["clip_val"]).any()) for q in ref if q.grad is not None)
            torch.nn.utils.clip_grad_value_(ref, clip["clip_val"])
        topt.step()
        before = [t.clone() for t in (model.flat_params[sl], opt.exp_avg, opt.exp_avg_sq)]
        opt.step()
        torch.cuda.synchronize()
        after = [model.flat_params[sl], opt.exp_avg, opt.exp_avg_sq]
        assert opt.table.active.cpu().tolist() == [int(a) for a in stepping], f"step {s}: device flags"
        if case == "norm":
            assert abs(float(opt.grad_norm) - ref_norm) <= 1e-5 * ref_norm, (float(opt.grad_norm), ref_norm)
        for name, was, now in zip(("param", "exp_avg", "exp_avg_sq"), before, after):
            assert torch.equal(was.cpu()[gaps], now.cpu()[gaps]), f"step {s}: {name} changed in a gap"
        for b, (lo, hi) in enumerate(RANGES):
            what = f"step {s} block {b} [{lo}, {hi})"
            if not stepping[b]:
                for name, was, now in zip(("param", "exp_avg", "exp_avg_sq"), before, after):
                    assert torch.equal(was[lo:hi], now[lo:hi]), f"{what}: {name} of a block without a gradient moved"
                continue
            st = topt.state[ref[b]]
            _assert_close_moment(after[1][lo:hi].cpu().double(), st["exp_avg"], what + " exp_avg")
            _assert_close_moment(after[2][lo:hi].cpu().double(), st["exp_avg_sq"], what + " exp_avg_sq")
            _assert_close_ulp(after[0][lo:hi].cpu().double(), ref[b].detach(), LR, what + " param")
        want_steps = [float(topt.state[q]["step"]) if q in topt.state and "step" in topt.state[q] else 0.0 for q in ref]
        assert opt.block_steps().cpu().tolist() == want_steps, f"step {s}: per-block step counts"
    assert float(opt.state[0]) == STEPS                    # launches
    assert opt.block_steps().cpu().tolist()[1] == 0.0      # the block that never had a gradient never stepped


@pytest.mark.parametrize("start", [0, 1])
@pytest.mark.parametrize("clip", [{}, dict(clip_val=0.4, clip_algorithm="value"), dict(clip_val=20.0, clip_algorithm="norm")],
                         ids=["plain", "value", "norm"])
@pytest.mark.parametrize("mode", ["skip", "skip_until_first"])
def test_every_block_active_is_bit_identical_to_zero_mode(dev, mode, clip, start):
    """With a gradient for every block in every step the block-aware step IS the default step: same parameters and moments
    bit for bit (weight decay on), on the 16-byte and on the scalar path.  Gaps hold zero gradients, zero moments and -- here --
    zero parameters, so the default's update of them is the identity as well."""
    outs = []
    for m in ("zero", mode):
        model = FlatModel(dev, start)
        sl = slice(start, start + N)
        model.flat_params[sl][~_in_blocks().to(dev)] = 0.0
        opt = _optimizer(model, m, 1e-2, **clip)
        for s in range(3):
            model.flat_grads[sl].copy_(_grads(s))
            opt.step()
        torch.cuda.synchronize()
        outs.append([t.clone() for t in (model.flat_params[sl], opt.exp_avg, opt.exp_avg_sq)] +
                    ([opt.grad_norm.clone()] if opt.grad_norm is not None else []))
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq", "grad_norm"), *outs):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))


@pytest.mark.parametrize("mode", ["skip", "skip_until_first"])
def test_state_dict_round_trip_in_mid_pattern(dev, mode):
    """Three steps, state_dict, three more -- against a fresh optimizer that loads the state and runs the last three: bit for
    bit, so the per-block counters, beta powers and seen flags all travel."""
    def run(model, opt, steps):
        for s in steps:
            model.flat_grads.copy_(_grads(s, ACTIVE))
            model.present = [bool(ACTIVE[b][s]) for b in range(len(RANGES))]
            opt.step()
        torch.cuda.synchronize()

    model = FlatModel(dev)
    opt = _optimizer(model, mode, 1e-2)
    run(model, opt, range(3))
    sd = copy.deepcopy({k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in opt.state_dict().items()})
    assert sd["absent_grad"] == mode and tuple(sd["block_state"].shape) == (len(RANGES), 4)
    params = model.flat_params.clone()
    run(model, opt, range(3, STEPS))
    model2 = FlatModel(dev, seed=77)
    model2.flat_params.copy_(params)
    opt2 = _optimizer(model2, mode, 1e-2)
    opt2.load_state_dict(sd)
    run(model2, opt2, range(3, STEPS))
    assert torch.equal(model.flat_params, model2.flat_params)
    assert torch.equal(opt.exp_avg, opt2.exp_avg) and torch.equal(opt.exp_avg_sq, opt2.exp_avg_sq)
    assert torch.equal(opt.table.state, opt2.table.state) and torch.equal(opt.state[:8], opt2.state[:8])


def test_cross_mode_load_is_refused(dev):
    opts = {m: _optimizer(FlatModel(dev), m) for m in ("zero", "skip", "skip_until_first")}
    for a in opts:
        for b in opts:
            if a != b:
                with pytest.raises(RuntimeError, match="adam_absent_grad"):
                    opts[b].load_state_dict(opts[a].state_dict())
    assert "block_state" not in opts["zero"].state_dict() and "absent_grad" not in opts["zero"].state_dict()
    opts["zero"].load_state_dict({k: v.clone() for k, v in opts["zero"].state_dict().items()})      # the default's layout, as before
