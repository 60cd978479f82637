"""GPU: EMA codebooks (``exp_params.codebook_ema_decay``) with a gradient exchange, rehearsed on one GPU as
tests/test_grad_accum_ddp_gpu.py rehearses gradient accumulation: a 1-rank RCCL group with the collectives forced.  With one rank
the SUM of the window accumulators is the identity -- the counts and the fp32 sums travel through float64 exactly -- so the run
must equal the ``ddp=None`` run bit for bit, and the collective must go out once per optimizer step.  (Two ranks, on the CPU:
tests/test_vq_ema_gloo.py.)"""
import pytest
import torch

from tests.test_adam_blocks_ddp_gpu import one_rank_rccl  # noqa: F401
from tests.test_codebook_gpu import EXP, _assert_same, _batches, _mcq, _snapshot

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")            # (with its index: the process group is bound to it)


def _run(dev, batches, with_ddp, accumulate):
    from ctvae_amd.ddp import GradBucketAllReduce
    from ctvae_amd.experiment import VAEXperiment
    m = _mcq(dev)
    ddp = GradBucketAllReduce(m, force=True) if with_ddp else None
    exp = VAEXperiment(m, dict(EXP, codebook_ema_decay=0.99), ddp=ddp, accumulate_grad_batches=accumulate)
    calls = []
    if ddp is not None:
        assert ddp.active and ddp.world == 1
        inner = ddp.all_reduce_codebook_ema

        def counted(words, sums):
            calls.append(exp.global_step)
            return inner(words, sums)
        ddp.all_reduce_codebook_ema = counted
    exp.fit(lambda: iter(batches), None, max_epochs=1)
    torch.cuda.synchronize()
    e = exp.codebook_ema
    return {**_snapshot(exp), "N": e.N.clone(), "M": e.M.clone(), "acc_s": e.acc_s.clone(), "acc_n": e.acc_n.float()}, calls, exp


@pytest.mark.parametrize("accumulate", [1, 2])
def test_one_rank_rccl_equals_single_process(dev, one_rank_rccl, accumulate):
    batches = _batches(dev, 6)
    single, _, _ = _run(dev, batches, False, accumulate)
    rehearsal, calls, exp = _run(dev, batches, True, accumulate)
    _assert_same(single, rehearsal, "ddp=None and a 1-rank RCCL group")
    steps = 6 // accumulate
    assert exp.global_step == steps and calls == list(range(steps)) and exp.codebook_ema.updates == steps
    assert float(single["N"].min()) != 1.0 and not single["acc_s"].any()
