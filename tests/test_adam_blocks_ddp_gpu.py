"""GPU (one device): FlatAdam's skip modes under a data-parallel gradient exchange -- the block-activity flags are MAX-reduced
across ranks before "skip_until_first" adds the blocks that have stepped (``FlatAdam.step(reduce_flags=...)``).

* Two ranks emulated one after the other on one GPU (as tests/test_ddp_equiv_gpu.py does), each with its own gradients and
  its own activity pattern per step, on a synthetic flat buffer with a bank of three members.  ``reduce_flags`` takes the
  elementwise max with the other rank's local flags, the gradient buffers hold the sum, ``grad_scale`` is 1/2.  The yardstick
  is ``torch.optim.Adam`` on the CPU in double over one tensor per block, whose ``.grad`` is None iff the block is inactive on
  BOTH ranks and the mean otherwise (torch DDP with ``find_unused_parameters=True``); for "skip_until_first" a zero tensor after
  the first gradient, as tests/test_adam_blocks_gpu.py restates the rule.  Bounds: that file's own.
* The 1-rank RCCL rehearsal of tests/test_ddp_nccl_gpu.py in both skip modes: CT-MCQ-VAE, one mode per batch, through eager
  steps, capture and replay, bit-equal to the ``ddp=None`` harness; and a checkpoint written by the rehearsal run continues in
  a ``ddp=None`` run bit-equal to the uninterrupted run."""
import os
import socket

import pytest
import torch

from tests.test_adam_blocks_ct_gpu import PARAMS, _batches, _FixedNoise, _model

pytestmark = pytest.mark.gpu

LR = 1e-3
# a 5-float block; 1025 floats (more than one 256-thread pass of 16-byte quads, and no multiple of 4); a bank of three 17-float
# members behind a 2-float gap; a 71-float block behind a gap that holds a whole quad; two floats behind the last block
RANGES = [(0, 5), (5, 1030), (1032, 1049), (1049, 1066), (1066, 1083), (1090, 1161)]
BANK = {2: 0, 3: 1, 4: 2}                  # block -> member of the bank
N = 1163
STEPS = 6
# ACTIVE[rank][block][step]
#            step:  1  2  3  4  5  6
ACTIVE = [[[1, 1, 1, 1, 1, 1],      # rank 0 only, every step
           [0, 1, 0, 0, 1, 0],      # the large block: rank 1 only, both, neither, rank 1 only, rank 0 only, neither
           [1, 0, 1, 0, 1, 0],      # member 0: both, neither, rank 0 only, rank 1 only, both, neither
           [0, 0, 0, 0, 0, 0],      # member 1: never, on no rank
           [0, 0, 0, 1, 0, 0],      # member 2: first appears at step 3 (on rank 1), then rank 0 only, neither, rank 1 only
           [0, 0, 0, 0, 0, 0]],     # rank 1 only, with steps on neither
          [[0, 0, 0, 0, 0, 0],
           [1, 1, 0, 1, 0, 0],
           [1, 0, 0, 1, 1, 0],
           [0, 0, 0, 0, 0, 0],
           [0, 0, 1, 0, 0, 1],
           [1, 0, 1, 1, 0, 1]]]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


# ---- helpers of tests/test_adam_blocks_gpu.py -------------------------------------------------------------
def _assert_close_ulp(got, want, lr, what):
    """Parameters: within 1e-3 * lr plus 2 ulp of |p|, elementwise."""
    a = want.abs().float()
    ulp = (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).to(want.dtype)      # fp32 ulp
    err = (got - want).abs()
    bad = err > 1e-3 * lr + 2 * ulp
    assert not bool(bad.any()), (what, float(err.max()), int(bad.sum()))


def _assert_close_moment(got, want, what):
    scale = float(want.abs().max())
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6 * scale + 1e-30, msg=lambda m: f"{what}: {m}")


def _f32(x):
    """x as the fp32 device state holds it, back in a Python float."""
    return float(torch.tensor(float(x), dtype=torch.float32))


class _Bank:
    """Stands for a bank module: FlatAdam hands it its words of the hit vector (``member_hits``)."""
    member_hits = None


class FlatModel:
    """What FlatAdam asks of a model, on a hand-made table: blocks 0, 1 and 5 report the activity the test sets in ``present``;
    blocks 2-4 are the members of one bank -- the host knows only whether the bank got a gradient (``bank_used``), the members'
    own activity lies in the hit words."""

    def __init__(self, dev, seed=5):
        g = torch.Generator().manual_seed(seed)
        self.flat_params = (torch.randn(N, generator=g) * 0.3).to(dev)
        self.flat_grads = torch.zeros(N, device=dev)
        self.present = [True] * len(RANGES)
        self.bank, self.bank_param, self.bank_used = _Bank(), object(), True

    def gather_torch_grads(self):
        pass

    def zero_grad(self):
        self.flat_grads.zero_()

    def torch_grad_present(self, p):
        assert p is self.bank_param
        return self.bank_used

    def adam_blocks(self):
        out = []
        for i, (lo, hi) in enumerate(RANGES):
            if i in BANK:
                out.append((lo, hi, "bank", (self.bank, self.bank_param), BANK[i]))
            else:
                out.append((lo, hi, "flag", (lambda i=i: self.present[i]), None))
        return out

    def set_activity(self, active):
        """One rank's step: ``active`` [nb] 0 / 1.  The bank was used iff one of its members was."""
        self.present = [bool(a) for a in active]
        self.bank_used = any(active[b] for b in BANK)
        hits = [0, 0, 0]
        for b, k in BANK.items():
            hits[k] = int(active[b])
        self.bank.member_hits.copy_(torch.tensor(hits, dtype=torch.int32))


def _grads(step, rank, active):
    """Rank `rank`'s gradient of the step: random in its active blocks, the zeros of zero_grad everywhere else."""
    gen = torch.Generator().manual_seed(1000 + 10 * step + rank)
    g = torch.zeros(N)
    for b, (lo, hi) in enumerate(RANGES):
        r = torch.randn(hi - lo, generator=gen) * (0.5 + 0.25 * b)
        if active[b]:
            g[lo:hi] = r
    return g


def test_patterns_hold_what_the_cases_need():
    """A block active on rank 0 only, on rank 1 only, on both, on neither -- in one and the same step too -- and one whose
    first gradient on any rank comes at step 3."""
    kinds = {(ACTIVE[0][b][s], ACTIVE[1][b][s]) for b in range(len(RANGES)) for s in range(STEPS)}
    assert kinds == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {(ACTIVE[0][b][0], ACTIVE[1][b][0]) for b in range(len(RANGES))} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    union4 = [max(ACTIVE[0][4][s], ACTIVE[1][4][s]) for s in range(STEPS)]
    assert union4[:3] == [0, 0, 1] and 0 in union4[3:]
    assert not any(ACTIVE[r][3][s] for r in (0, 1) for s in range(STEPS))


@pytest.mark.parametrize("wd", [0.0, 1e-2], ids=["plain", "weight_decay"])
@pytest.mark.parametrize("mode", ["skip", "skip_until_first"])
def test_two_emulated_ranks_follow_torch_adam_with_unused_parameters(dev, mode, wd):
    from ctvae_amd import kernels as K
    from ctvae_amd.optim import FlatAdam
    nb = len(RANGES)
    models = [FlatModel(dev) for _ in range(2)]                    # same start: DDP broadcasts rank 0's parameters
    opts = [FlatAdam(m, lr=LR, weight_decay=wd, absent_grad=mode) for m in models]
    assert opts[0].table.hit_index.tolist() == [-1, -1, 0, 1, 2, -1] and opts[0].table.nhits == 3
    p0 = models[0].flat_params.cpu()
    ref = [torch.nn.Parameter(p0[lo:hi].double().clone()) for lo, hi in RANGES]
    topt = torch.optim.Adam(ref, lr=_f32(LR), betas=(_f32(0.9), _f32(0.999)), eps=_f32(1e-8), weight_decay=_f32(wd))
    seen = [False] * nb
    gaps = torch.ones(N, dtype=torch.bool)
    for lo, hi in RANGES:
        gaps[lo:hi] = False
    for s in range(STEPS):
        act = [[ACTIVE[r][b][s] for b in range(nb)] for r in (0, 1)]
        g = [_grads(s, r, act[r]) for r in (0, 1)]
        summed = g[0] + g[1]                                       # what the SUM all-reduce leaves on both ranks
        # every rank's local flags first (on a real node they are formed at the same time): saved for the other's reduction
        local = []
        for r in (0, 1):
            models[r].set_activity(act[r])
            K.adam_block_flags_local(opts[r].table, torch.tensor(opts[r]._host_pattern(), dtype=torch.int32, device=dev))
            local.append(opts[r].table.active.clone())
            assert local[r].cpu().tolist() == act[r], f"step {s} rank {r}: local flags"
        stepping = []
        for b, (lo, hi) in enumerate(RANGES):
            on = bool(act[0][b] or act[1][b])
            seen[b] = seen[b] or on
            if on:
                ref[b].grad = (0.5 * summed[lo:hi].double()).clone()
            elif mode == "skip_until_first" and seen[b]:
                ref[b].grad = torch.zeros_like(ref[b])
            else:
                ref[b].grad = None
            stepping.append(ref[b].grad is not None)
        topt.step()
        for r in (0, 1):
            m, opt = models[r], opts[r]
            m.set_activity(act[r])                                 # (the hit words were consumed above)
            m.flat_grads.copy_(summed)
            before = [t.clone() for t in (m.flat_params, opt.exp_avg, opt.exp_avg_sq)]
            other = local[1 - r]
            opt.step(grad_scale=0.5, reduce_flags=lambda flags: flags.copy_(torch.maximum(flags, other)))
            torch.cuda.synchronize()
            after = [m.flat_params, opt.exp_avg, opt.exp_avg_sq]
            what = f"step {s} rank {r}"
            assert opt.table.active.cpu().tolist() == [int(a) for a in stepping], what + ": final flags"
            assert opt.host_pattern == tuple(int(bool(a)) if b not in BANK else int(any(act[r][k] for k in BANK))
                                             for b, a in enumerate(act[r])), what + ": host_pattern"
            for name, was, now in zip(("param", "exp_avg", "exp_avg_sq"), before, after):
                assert torch.equal(was.cpu()[gaps], now.cpu()[gaps]), f"{what}: {name} changed in a gap"
            for b, (lo, hi) in enumerate(RANGES):
                wb = f"{what} block {b}"
                if not stepping[b]:
                    for name, was, now in zip(("param", "exp_avg", "exp_avg_sq"), before, after):
                        assert torch.equal(was[lo:hi], now[lo:hi]), f"{wb}: {name} of a block inactive on both ranks moved"
                    continue
                st = topt.state[ref[b]]
                _assert_close_moment(after[1][lo:hi].cpu().double(), st["exp_avg"], wb + " exp_avg")
                _assert_close_moment(after[2][lo:hi].cpu().double(), st["exp_avg_sq"], wb + " exp_avg_sq")
                _assert_close_ulp(after[0][lo:hi].cpu().double(), ref[b].detach(), LR, wb + " param")
            want_steps = [float(topt.state[q]["step"]) if q in topt.state and "step" in topt.state[q] else 0.0 for q in ref]
            assert opt.block_steps().cpu().tolist() == want_steps, what + ": per-block step counts"
        assert torch.equal(opts[0].table.state, opts[1].table.state), f"step {s}: the ranks' block states differ"
        assert torch.equal(models[0].flat_params, models[1].flat_params), f"step {s}: the ranks' parameters differ"
    assert opts[0].block_steps().cpu().tolist()[3] == 0.0          # the member no rank ever used never stepped
    assert torch.equal(opts[0].exp_avg, opts[1].exp_avg) and torch.equal(opts[0].exp_avg_sq, opts[1].exp_avg_sq)


# ---- the 1-rank RCCL rehearsal ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_rank_rccl(dev):
    import torch.distributed as dist
    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    yield dist
    torch.cuda.synchronize()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def fixed_noise(dev):
    from ctvae_amd.models import causal
    prev = causal.set_noise_source(_FixedNoise(dev))
    yield
    causal.set_noise_source(prev)


CUT = 9            # batches before the checkpoint: base has run 3 eager steps, action 3 eager + its capture, causal 2 eager
_runs = {}


def _final(m, exp):
    opt = exp.optimizer
    return [m.flat_params.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.table.state.clone()]


def _harness_runs(dev, mode, tmp_path_factory):
    """Per skip mode, once: the ``ddp=None`` harness over the 18 batches (the yardstick), and the rehearsal run over the same
    batches with a checkpoint written after the first CUT."""
    if mode in _runs:
        return _runs[mode]
    from ctvae_amd.ddp import GradBucketAllReduce
    from ctvae_amd.experiment import VAEXperiment
    batches = _batches(dev, rounds=3)
    params = dict(PARAMS, hipgraph=True, adam_absent_grad=mode)
    m = _model(dev)
    exp = VAEXperiment(m, params)
    exp.fit(lambda: iter(batches), None, max_epochs=1)
    torch.cuda.synchronize()
    single = _final(m, exp)
    m = _model(dev)
    ddp = GradBucketAllReduce(m, force=True)
    exp = VAEXperiment(m, params, ddp=ddp)
    assert ddp.active and ddp.world == 1 and ddp.range == exp.optimizer.slice
    exp.fit(lambda: iter(batches[:CUT]), None, max_epochs=1)
    ckpt = str(tmp_path_factory.mktemp("ddp_" + mode) / "last.ckpt")
    torch.save({"state_dict": {"model." + k: v.detach().cpu().clone() for k, v in m.state_dict().items()},
                "trainer": exp.state_dict()}, ckpt)
    exp.fit(lambda: iter(batches[CUT:]), None, max_epochs=1)
    torch.cuda.synchronize()
    replays = sorted(g.seen - g.WARM for g in exp._graphed.values() if g.graph is not None)
    assert replays == [3, 6], replays                  # base and action captured and replayed; causal (3 batches) stays eager
    assert exp.global_step == len(batches)
    _runs[mode] = dict(single=single, rehearsal=_final(m, exp), ckpt=ckpt, batches=batches, params=params)
    return _runs[mode]


@pytest.mark.parametrize("mode", ["skip", "skip_until_first"])
def test_ct_modes_under_rccl_equal_single_process_in_skip_modes(dev, one_rank_rccl, fixed_noise, tmp_path_factory, mode):
    """With one rank the flags' MAX all-reduce and the gradients' SUM all-reduce are the identity: parameters, moments and the
    per-block state equal the ``ddp=None`` harness (flags and Adam inside the graph) bit for bit."""
    runs = _harness_runs(dev, mode, tmp_path_factory)
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq", "block_state"), runs["single"], runs["rehearsal"]):
        assert torch.isfinite(a).all() and torch.equal(a, b), (name, float((a - b).abs().max()))
    steps = runs["single"][3][:, 0]
    assert float(steps.max()) == 18.0 and float(steps.min()) == 0.0 and len(set(steps.tolist())) > 2      # the blocks do differ


@pytest.mark.parametrize("mode", ["skip", "skip_until_first"])
def test_checkpoint_of_the_rehearsal_run_continues_in_a_single_process(dev, one_rank_rccl, fixed_noise, tmp_path_factory, mode):
    """Nothing rank-specific is stored: the checkpoint written under the exchange loads into a ``ddp=None`` run, which
    finishes the batches bit-equal to the uninterrupted ``ddp=None`` run."""
    from ctvae_amd.experiment import VAEXperiment
    runs = _harness_runs(dev, mode, tmp_path_factory)
    ckpt = torch.load(runs["ckpt"], map_location="cpu", weights_only=True)
    assert ckpt["trainer"]["optimizer"]["absent_grad"] == mode and ckpt["trainer"]["global_step"] == CUT
    m = _model(dev, seed=11)                                        # other start values: everything comes from the checkpoint
    m.load_state_dict({k[6:]: v for k, v in ckpt["state_dict"].items()})
    exp = VAEXperiment(m, runs["params"])
    exp.load_state_dict(ckpt["trainer"])
    exp.fit(lambda: iter(runs["batches"][CUT:]), None, max_epochs=1)
    torch.cuda.synchronize()
    assert exp.global_step == len(runs["batches"])
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq", "block_state"), runs["single"], _final(m, exp)):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
