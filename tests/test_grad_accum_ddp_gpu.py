"""GPU: ``accumulate_grad_batches`` with a gradient exchange, rehearsed on one GPU the way tests/test_adam_blocks_ddp_gpu.py
rehearses the skip modes: a 1-rank RCCL group with the collectives forced.  With one rank the flags' MAX and the gradients' SUM
are the identity, so the run must equal the ``ddp=None`` run of the same windows bit for bit -- and the collectives must go out
once per window, on the micro-batch that ends it, and on no other.  (Two ranks, on the CPU: tests/test_grad_accum_gloo.py.)"""
import pytest
import torch

from tests.test_adam_blocks_ct_gpu import PARAMS, _batches, _model
from tests.test_adam_blocks_ddp_gpu import fixed_noise, one_rank_rccl  # noqa: F401

pytestmark = pytest.mark.gpu
K_ACC = 3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")            # (with its index: the process group is bound to it)


def _run(dev, mode, batches, with_ddp):
    from ctvae_amd.ddp import GradBucketAllReduce
    from ctvae_amd.experiment import VAEXperiment
    params = dict(PARAMS, hipgraph=True)
    if mode != "zero":
        params["adam_absent_grad"] = mode
    m = _model(dev)
    ddp = GradBucketAllReduce(m, force=True) if with_ddp else None
    exp = VAEXperiment(m, params, ddp=ddp, accumulate_grad_batches=K_ACC)
    calls = {"grads": [], "flags": []}
    if ddp is not None:
        assert ddp.active and ddp.world == 1 and ddp.range == exp.optimizer.slice and ddp.accumulate == K_ACC
        reduce_grads, reduce_flags = ddp.all_reduce, ddp.all_reduce_flags

        def counted_grads(*a, **kw):
            calls["grads"].append(seen[0])
            return reduce_grads(*a, **kw)

        def counted_flags(flags):
            calls["flags"].append(seen[0])
            return reduce_flags(flags)

        ddp.all_reduce, ddp.all_reduce_flags = counted_grads, counted_flags
    seen = [-1]

    def loader():
        # fit() looks one batch ahead: batch i is being stepped while batch i + 1 has been drawn
        for i, b in enumerate(batches):
            seen[0] = i
            yield b

    exp.fit(loader, None, max_epochs=1)
    torch.cuda.synchronize()
    opt = exp.optimizer
    assert exp.global_step == len(batches) // K_ACC and opt.stashed == 0
    final = [m.flat_params.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.state[:8].clone()]
    if opt.table is not None:
        final.append(opt.table.state.clone())
    return final, calls, exp


@pytest.mark.parametrize("mode", ["zero", "skip", "skip_until_first"])
def test_windows_under_rccl_equal_single_process(dev, one_rank_rccl, fixed_noise, mode):
    """CT-MCQ-VAE (``update_parameters: ct_layer``), k = 3 over the 18 batches of the skip-mode tests: six windows."""
    batches = _batches(dev, rounds=3)
    single, _, _ = _run(dev, mode, batches, False)
    rehearsal, calls, exp = _run(dev, mode, batches, True)
    for a, b in zip(single, rehearsal):
        assert torch.isfinite(a).all() and torch.equal(a, b), float((a.double() - b.double()).abs().max())
    assert float(single[3][0]) == 6.0
    assert any(g.graph is not None for g in exp._graphed.values()), "no hipGraph was captured"
    # a window's last micro-batch i (i % 3 == 2) steps after batch i + 1 was drawn, the epoch's last one after the loader ended
    ends = [min(i + 1, len(batches) - 1) for i in range(len(batches)) if i % K_ACC == K_ACC - 1]
    assert calls["grads"] == ends, calls
    assert calls["flags"] == ([] if mode == "zero" else ends), calls
