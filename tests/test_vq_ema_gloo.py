"""CPU, world_size 2, gloo: the EMA codebook update (``exp_params.codebook_ema_decay``) under data-parallel training, in the manner
of tests/test_codebook_gloo.py -- VAEXperiment.codebook_update on rank-specific statistics with CPU test doubles of the two
launches around the collective.  Both ranks end with the summed accumulators in front of the update and with identical N, M and
codebooks behind it; one collective per optimizer step and none per micro-batch.  (The kernels themselves:
tests/test_vq_ema_ops_gpu.py.)"""
import os

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_ddp_gloo import _free_port

CFG = dict(in_channels=3, embedding_dim=16, hidden_dims=[8, 16], num_embeddings=8, img_size=64, codebooks=4, beta=0.25)
C, KC, DC, D, HW, B = 4, 8, 4, 16, 6, 3


def _install_doubles(K, seen):
    """TEST DOUBLES of the HIP launches CodebookEMA issues (the product has no CPU path), by their definitions
    (tests/vq_ema_checks.py); the update's double records the accumulators it was handed."""
    from tests import vq_ema_checks as EC

    def vq_ema_stats(latents, inds, acc_n, acc_s, invalid):
        counts, sums, _, bad = EC.stats64(latents.reshape(-1, latents.size(-1)), inds.reshape(inds.size(0), inds.size(1), -1),
                                          acc_n.size(1))
        acc_n += counts
        acc_s += sums.float()
        invalid += bad

    def vq_ema_update(codebooks, N, M, acc_n, acc_s, decay, eps):
        seen.append((acc_n.clone(), acc_s.clone()))
        ref = EC.update64(N, M, acc_n, acc_s, decay, eps)
        N.copy_(ref["N"].float())
        M.copy_(ref["M"].float())
        codebooks.copy_(ref["E"].float())
        acc_n.zero_()
        acc_s.zero_()

    K.vq_ema_stats, K.vq_ema_update = vq_ema_stats, vq_ema_update


def _inds(rank, step):
    g = torch.Generator().manual_seed(50 + 10 * step + rank)
    inds = torch.randint(0, KC, (B, C, HW), generator=g)
    inds[:, 0] = 1 + rank                       # codebook 0: code 1 on rank 0 only, code 2 on rank 1 only
    return inds


def _latents(rank, step):
    # multiples of 1/8 below 2^10: every partial sum is exact in fp32, so the order of the ranks' shares does not matter
    g = torch.Generator().manual_seed(900 + 10 * step + rank)
    return torch.randint(-64, 65, (B, 2, 3, D), generator=g).float() / 8


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from ctvae_amd import kernels as K
        from ctvae_amd.ddp import GradBucketAllReduce
        from ctvae_amd.experiment import VAEXperiment
        from ctvae_amd.models import vae_models
        from tests import vq_ema_checks as EC
        seen = []
        _install_doubles(K, seen)
        torch.manual_seed(7 + rank)
        m = vae_models["MCQVAE"](**dict(CFG, hidden_dims=list(CFG["hidden_dims"])))
        ddp = GradBucketAllReduce(m, bucket_bytes=1 << 16)          # (broadcasts rank 0's parameters)
        exp = VAEXperiment(m, {"LR": 1e-3, "weight_decay": 0.0, "kld_weight": 1.0, "manual_seed": 21, "codebook_ema_decay": 0.9},
                           ddp=ddp)
        ema = exp.codebook_ema
        E0 = ema.codebooks().clone()
        assert torch.equal(ema.M, E0)
        calls = []
        inner = ddp.all_reduce_codebook_ema

        def counted(words, sums):
            calls.append(exp.global_step)
            return inner(words, sums)
        ddp.all_reduce_codebook_ema = counted
        # one window of two micro-batches, then the update; then a second step of one micro-batch
        ema.invalid.fill_(rank + 1)
        for step in range(2):
            ema.observe(_inds(rank, step), _latents(rank, step))
        assert not calls, "a micro-batch issued a collective"
        local = [EC.stats64(_latents(rank, s).reshape(-1, D), _inds(rank, s), KC) for s in range(2)]
        assert torch.equal(ema.acc_n, local[0][0] + local[1][0])
        exp.codebook_update()
        exp.global_step += 1
        total = [EC.stats64(_latents(r, s).reshape(-1, D), _inds(r, s), KC) for r in range(world) for s in range(2)]
        counts, sums = sum(t[0] for t in total), sum(t[1] for t in total)
        assert calls == [0] and len(seen) == 1
        assert torch.equal(seen[0][0], counts) and torch.equal(seen[0][1].double(), sums), "the update saw the summed window"
        assert int(counts[0, 1]) == int(counts[0, 2]) == 2 * B * HW and int(local[0][0][0, 2 - rank]) == 0
        ref = EC.update64(torch.ones(C, KC), E0, counts, sums, ema.decay, ema.eps)
        assert torch.equal(ema.N, ref["N"].float()) and torch.equal(ema.codebooks(), ref["E"].float())
        assert not ema.acc_n.any() and not ema.acc_s.any() and int(ema.invalid) == rank + 1   # (a rank's own count: not reduced)
        ema.observe(_inds(rank, 2), _latents(rank, 2))
        exp.codebook_update()
        exp.global_step += 1
        assert calls == [0, 1] and len(seen) == 2
        for t in (m.flat_params, ema.N, ema.M):
            gathered = [torch.empty_like(t) for _ in range(world)]
            dist.all_gather(gathered, t.contiguous())
            assert torch.equal(gathered[0], gathered[1]), "ranks diverged"
        q.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc() + repr(e)))
    finally:
        dist.destroy_process_group()


def test_two_rank_update_uses_the_summed_window_and_ranks_agree():
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
