"""CPU, world_size 2, gloo: the exchange's side of FlatAdam's skip modes under data-parallel training --
``GradBucketAllReduce.all_reduce_flags`` leaves the elementwise MAX of the ranks' block-activity flags on every rank, does
nothing for an inactive exchange, and ``VAEXperiment`` accepts the skip modes together with an exchange that has it (and still
refuses one that has not).  (RCCL replaces gloo on the GPUs; the call is the same.  The step itself is a HIP kernel:
tests/test_adam_blocks_ddp_gpu.py.)"""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

CFG = dict(in_channels=3, embedding_dim=16, hidden_dims=[8, 16], num_embeddings=8, img_size=64, codebooks=1, beta=0.25)
PARAMS = {"LR": 1e-3, "weight_decay": 0.0, "kld_weight": 1.0}
#        block:  0  1  2  3  4  5  6
FLAGS = [[1, 0, 0, 1, 0, 1, 0],      # rank 0
         [0, 1, 0, 1, 0, 0, 0]]      # rank 1
MAXED = [1, 1, 0, 1, 0, 1, 0]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _NoFlags:
    """An exchange object from before the flags' reduction existed."""

    def restrict(self, sl):
        self.range = sl


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from ctvae_amd.ddp import GradBucketAllReduce
        from ctvae_amd.experiment import VAEXperiment
        from ctvae_amd.models import vae_models
        torch.manual_seed(7 + rank)
        m = vae_models["MCQVAE"](**CFG)
        ddp = GradBucketAllReduce(m, bucket_bytes=1 << 16)
        assert ddp.active and ddp.world == 2
        flags = torch.tensor(FLAGS[rank], dtype=torch.int32)
        assert ddp.all_reduce_flags(flags) is None
        assert flags.dtype == torch.int32 and flags.tolist() == MAXED, flags.tolist()
        ddp.all_reduce_flags(flags)                               # idempotent on what is already the maximum
        assert flags.tolist() == MAXED
        for mode in ("skip", "skip_until_first"):
            exp = VAEXperiment(m, dict(PARAMS, adam_absent_grad=mode), ddp=ddp)
            assert exp.optimizer.absent_grad == mode and exp.optimizer.table.nb == len(m._grad_blocks)
            try:
                VAEXperiment(m, dict(PARAMS, adam_absent_grad=mode), ddp=_NoFlags())
            except ValueError as e:
                assert "DDP" in str(e), str(e)
            else:
                raise AssertionError("an exchange without all_reduce_flags was accepted in mode " + mode)
        VAEXperiment(m, dict(PARAMS, adam_absent_grad="zero"), ddp=_NoFlags())
        q.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc() + repr(e)))
    finally:
        dist.destroy_process_group()


def test_two_rank_flags_max_and_skip_modes_construct():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in range(2))
    for p in procs:
        p.join(60)
    assert res == {0: "ok", 1: "ok"}, res


def test_inactive_exchange_leaves_the_flags_alone():
    """No process group: one rank, nothing forced -- the exchange is inactive and must not call a collective."""
    from ctvae_amd.ddp import GradBucketAllReduce
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    assert not dist.is_initialized()
    torch.manual_seed(7)
    m = vae_models["MCQVAE"](**CFG)
    ddp = GradBucketAllReduce(m)
    assert not ddp.active
    flags = torch.tensor(FLAGS[0], dtype=torch.int32)
    ddp.all_reduce_flags(flags)
    assert flags.tolist() == FLAGS[0]
    VAEXperiment(m, dict(PARAMS, adam_absent_grad="skip"), ddp=ddp)
    with pytest.raises(ValueError, match="DDP"):
        VAEXperiment(m, dict(PARAMS, adam_absent_grad="skip"), ddp=_NoFlags())
