"""CPU, world_size 2, gloo: ``accumulate_grad_batches`` under data-parallel training, in the manner of tests/test_ddp_gloo.py
-- VAEXperiment.window_step on rank-specific flat gradients with CPU test doubles of the kernels around it.  With k = 2 over 4
micro-batches: the gradients travel exactly twice and, in a skip mode, so do the block flags -- on the micro-batches that end
a window and on no other; both ranks end with the same parameters, those of one process that sums a window's four gradients
and steps with grad_scale = 1 / (2 * 2).  (The kernels themselves: tests/test_grad_accum_ops_gpu.py.)"""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_ddp_gloo import _adam_cpu, _free_port

CFG = dict(in_channels=3, embedding_dim=16, hidden_dims=[8, 16], num_embeddings=8, img_size=64, codebooks=1, beta=0.25)
K_ACC, N_BATCHES = 2, 4


def _install_doubles(K, log):
    """TEST DOUBLES of the HIP launches FlatAdam issues (the product has no CPU path): the accumulate and flag-window kernels
    by their definition, the block-flag halves without bank members, and the block-aware step as the plain rule on the whole
    slice -- it records the flags it was handed, which is what this file checks of it."""
    K.adam_step = _adam_cpu

    def grad_accumulate(acc, grads, mode):
        log.append(("accumulate", mode))
        if mode == "store":
            acc.copy_(grads)
        elif mode == "add":
            acc.add_(grads)
        else:
            grads.copy_(acc + grads)

    def adam_block_flags_local(table, present):
        table.active.copy_(present)

    def adam_flags_window(window, table, mode):
        log.append(("flags", mode))
        if mode == "store":
            window.copy_(table.active)
        elif mode == "add":
            window.copy_(torch.maximum(window, table.active))
        else:
            table.active.copy_(torch.maximum(window, table.active))

    def adam_block_flags_finish(table, mode):
        table.active.copy_((table.active != 0).int())

    def adam_step_blocks(p, g, m, v, state, table, present, mode, grad_scale=1.0, algorithm=None, clip_val=None, workspace=None,
                         norm_out=None, flags_final=False):
        assert flags_final, "a window's step runs on the merged, reduced flags"
        log.append(("stepped_flags", table.active.tolist()))
        _adam_cpu(p, g, m, v, state, grad_scale)

    K.grad_accumulate, K.adam_flags_window = grad_accumulate, adam_flags_window
    K.adam_block_flags_local, K.adam_block_flags_finish, K.adam_step_blocks = adam_block_flags_local, adam_block_flags_finish, adam_step_blocks


def _grads(n, window, rank, mb):
    return torch.randn(n, generator=torch.Generator().manual_seed(1000 * window + 10 * rank + mb))


def _written(nb, window, rank, mb):
    """Which kernel-managed blocks 'got a gradient' in a micro-batch: block 0 never, block 1 on rank 1's first micro-batch of
    window 0 only, block 2 on rank 0's second micro-batch of every window, the others always."""
    w = [True] * nb
    w[0] = False
    w[1] = (window, rank, mb) == (0, 1, 0)
    w[2] = (rank, mb) == (0, 1)
    return w


def _worker(rank, world, port, q, absent):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from ctvae_amd import kernels as K
        from ctvae_amd.ddp import GradBucketAllReduce
        from ctvae_amd.experiment import VAEXperiment
        from ctvae_amd.models import vae_models
        from ctvae_amd.optim import accumulation_schedule
        log = []
        _install_doubles(K, log)
        torch.manual_seed(7 + rank)
        m = vae_models["MCQVAE"](**dict(CFG, hidden_dims=list(CFG["hidden_dims"])))
        ddp = GradBucketAllReduce(m, bucket_bytes=1 << 16)
        params = {"LR": 1e-3, "weight_decay": 0.0, "kld_weight": 1.0}
        if absent != "zero":
            params["adam_absent_grad"] = absent
        exp = VAEXperiment(m, params, ddp=ddp, accumulate_grad_batches=K_ACC)
        n, nb = m.flat_grads.numel(), len(m._grad_blocks)
        assert nb >= 4 and len(ddp.buckets()) > 1
        calls = {"grads": [], "flags": []}
        position = [None]
        reduce_grads, reduce_flags = ddp.all_reduce, ddp.all_reduce_flags

        def counted_grads(*a, **kw):
            calls["grads"].append(position[0])
            return reduce_grads(*a, **kw)

        def counted_flags(flags):
            calls["flags"].append(position[0])
            return reduce_flags(flags)

        ddp.all_reduce, ddp.all_reduce_flags = counted_grads, counted_flags
        single = m.flat_params.clone()
        ea, es, st = torch.zeros(n), torch.zeros(n), exp.optimizer.state.clone()
        ends = accumulation_schedule(N_BATCHES, K_ACC)
        for i in range(N_BATCHES):
            window, mb = divmod(i, K_ACC)
            position[0] = i
            m.zero_grad()
            m._flat_grads.copy_(_grads(n, window, rank, mb))
            for blk, w in zip(m._grad_blocks, _written(nb, window, rank, mb)):
                blk.written = w
            exp.window_step(ends[i])
            exp.global_step += int(ends[i])
            if ends[i]:       # one process: the window's four gradients (per rank first, as the exchange sums them), 1 / (k * world)
                per_rank = [_grads(n, window, r, 0) + _grads(n, window, r, 1) for r in range(world)]
                _adam_cpu(single, per_rank[0] + per_rank[1], ea, es, st, grad_scale=1.0 / (K_ACC * world))
        assert exp.global_step == 2 and float(exp.optimizer.state[0]) == 2.0
        # collectives: one gradient exchange per window, on its last micro-batch; flags likewise in a skip mode, none otherwise
        assert calls["grads"] == [1, 3], calls
        assert calls["flags"] == ([] if absent == "zero" else [1, 3]), calls
        assert [e for e in log if e[0] == "accumulate"] == [("accumulate", "store"), ("accumulate", "finish")] * 2
        if absent != "zero":
            assert [e for e in log if e[0] == "flags"] == [("flags", "store"), ("flags", "finish")] * 2
            stepped = [e[1] for e in log if e[0] == "stepped_flags"]
            want = []
            for window in range(2):
                f = [any(_written(nb, window, r, mb)[b] for r in range(world) for mb in range(K_ACC)) for b in range(nb)]
                want.append([int(x) for x in f])
            assert want[0][:3] == [0, 1, 1] and want[1][:3] == [0, 0, 1]
            assert stepped == want, (stepped, want)
        torch.testing.assert_close(m.flat_params, single, rtol=1e-6, atol=1e-7)
        gathered = [torch.empty_like(m.flat_params) for _ in range(world)]
        dist.all_gather(gathered, m.flat_params)
        assert torch.equal(gathered[0], gathered[1]), "ranks diverged"
        q.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc() + repr(e)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("absent", ["zero", "skip", "skip_until_first"])
def test_two_rank_windows_exchange_once_per_window(absent):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, absent)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in range(2))
    for p in procs:
        p.join(60)
    assert res == {0: "ok", 1: "ok"}, res
