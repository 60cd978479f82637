"""CPU, world_size 2, gloo: a dead-code restart (``exp_params.codebook_restart_every``) under data-parallel training, in the manner
of tests/test_grad_accum_gloo.py -- VAEXperiment.codebook_restart on rank-specific counts and pools with CPU test doubles of the
kernels around it.  The dead list comes from the summed counts (a code used on one rank only is alive), both ranks end with the
same codebook, namely rank 0's rows, and the same zeroed moments; one count all-reduce and one broadcast per restart and none on
any other step.  (The kernels themselves: tests/test_codebook_ops_gpu.py.)"""
import os

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_ddp_gloo import _free_port

CFG = dict(in_channels=3, embedding_dim=16, hidden_dims=[8, 16], num_embeddings=8, img_size=64, codebooks=4, beta=0.25)
C, KC, DC, D, HW, B, R = 4, 8, 4, 16, 6, 3, 10


def _install_doubles(K):
    """TEST DOUBLES of the HIP launches CodebookUsage issues (the product has no CPU path), by their definitions."""

    def vq_usage(inds, counts, invalid):
        flat = inds.reshape(inds.size(0), counts.size(0), -1)
        for c in range(counts.size(0)):
            counts[c] += torch.bincount(flat[:, c].reshape(-1), minlength=counts.size(1))

    def vq_pool_fill(latents, pool):
        rows = min(latents.numel() // pool.size(1), pool.size(0))
        pool[:rows] = latents.reshape(-1, pool.size(1))[:rows]
        return rows

    def vq_usage_pool_fill(inds, counts, invalid, latents, pool):
        vq_usage(inds, counts, invalid)
        return vq_pool_fill(latents, pool)

    def vq_restart_gather(entries, pool, valid_rows, n_codebooks, dc):
        assert all(r < valid_rows for _, _, r in entries)
        return torch.stack([pool[r, c:c + dc] for c, _, r in entries])

    def vq_restart(entries, pool, valid_rows, codebooks, exp_avg, exp_avg_sq, rows=None):
        assert rows is not None and pool is None, "a data-parallel restart scatters the broadcast rows"
        for i, (c, k, _) in enumerate(entries):
            codebooks[c, k] = rows[i]
            exp_avg[c, k] = 0
            exp_avg_sq[c, k] = 0

    K.vq_usage, K.vq_pool_fill, K.vq_usage_pool_fill = vq_usage, vq_pool_fill, vq_usage_pool_fill
    K.vq_restart_gather, K.vq_restart = vq_restart_gather, vq_restart


def _inds(rank, step):
    """[B, C, HW] indices: codes 4..7 on both ranks; code 1 on rank 0 only, code 2 on rank 1 only, codes 0 and 3 on neither --
    in codebook 0; codebook 1 uses every code on both ranks; codebooks 2 and 3 use code 5 alone."""
    g = torch.Generator().manual_seed(50 + 10 * step + rank)
    inds = torch.empty((B, C, HW), dtype=torch.int64)
    inds[:, 0] = torch.randint(4, 8, (B, HW), generator=g)
    inds[0, 0, 0] = 1 + rank
    inds[:, 1] = torch.arange(B * HW).reshape(B, HW) % KC
    inds[:, 2:] = 5
    return inds


def _latents(rank, step):
    return torch.randn((B, 2, 3, D), generator=torch.Generator().manual_seed(900 + 10 * step + rank))


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from ctvae_amd import kernels as K
        from ctvae_amd.ddp import GradBucketAllReduce
        from ctvae_amd.experiment import VAEXperiment
        from ctvae_amd.models import vae_models
        from ctvae_amd.optim import codebook_restart_rows
        _install_doubles(K)
        torch.manual_seed(7 + rank)
        m = vae_models["MCQVAE"](**dict(CFG, hidden_dims=list(CFG["hidden_dims"])))
        ddp = GradBucketAllReduce(m, bucket_bytes=1 << 16)
        exp = VAEXperiment(m, {"LR": 1e-3, "weight_decay": 0.0, "kld_weight": 1.0, "manual_seed": 21, "codebook_restart_every": 2,
                               "codebook_restart_pool": R}, ddp=ddp)
        cb = exp.codebook
        calls = {"counts": [], "rows": []}
        reduce_counts, broadcast_rows = ddp.all_reduce_counts, ddp.broadcast_rows

        def counted_reduce(t):
            calls["counts"].append(exp.global_step)
            return reduce_counts(t)

        def counted_broadcast(t, src=0):
            calls["rows"].append(exp.global_step)
            return broadcast_rows(t, src)

        ddp.all_reduce_counts, ddp.broadcast_rows = counted_reduce, counted_broadcast
        exp.optimizer.exp_avg.fill_(1.0)
        exp.optimizer.exp_avg_sq.fill_(2.0)
        before = m.flat_params.clone()
        local = torch.zeros(C, KC, dtype=torch.int64)
        for step in range(3):                       # restarts fall behind the step that makes global_step a multiple of 2: step 1
            cb.observe(_inds(rank, step), _latents(rank, step))
            if step < 2:
                local += torch.stack([torch.bincount(_inds(rank, step)[:, c].reshape(-1), minlength=KC) for c in range(C)])
            if step == 1:
                assert torch.equal(cb.read()[0], local) and cb.valid_rows == min(B * 6, R)
                assert not torch.equal(cb.pool, torch.zeros_like(cb.pool))
            exp.codebook_restart()
            exp.global_step += 1
        assert calls == {"counts": [1], "rows": [1]}, calls
        # the dead list of the summed counts: in codebook 0 codes 0 and 3 -- not 1 (rank 0's) or 2 (rank 1's)
        total = sum(torch.stack([torch.bincount(_inds(r, s)[:, c].reshape(-1), minlength=KC) for c in range(C)])
                    for r in range(world) for s in range(2))
        dead = [(c, k) for c in range(C) for k in range(KC) if int(total[c, k]) == 0]
        assert dead == [(0, 0), (0, 3)] + [(c, k) for c in (2, 3) for k in range(KC) if k != 5]
        assert int(local[0, 2 - rank]) == 0, "the code the other rank used is dead by this rank's own counts"
        assert exp.codebook_ordinal == 1 and exp.codebook_restarted == len(dead) == exp.last_codebook_restart["codebook_restarts"]
        rows = codebook_restart_rows(21, 0, len(dead), R)
        assert len(dead) > R and len(set(rows)) == R                       # more dead codes than pool rows: the draw wrapped around
        pool0 = _latents(0, 1).reshape(-1, D)[:R]                           # rank 0's pool at the restart: step 1's latents
        codebooks, exp_avg, exp_avg_sq = cb.codebook_views(exp.optimizer)
        lo = cb.codebook_offset(exp.optimizer)
        want = before[lo:lo + C * KC * DC].view(C, KC, DC).clone()
        for (c, k), r in zip(dead, rows):
            want[c, k] = pool0[r, c:c + DC]
        assert torch.equal(codebooks, want)
        alive = torch.ones(C, KC, dtype=torch.bool)
        for c, k in dead:
            alive[c, k] = False
        assert bool((exp_avg[alive] == 1.0).all()) and bool((exp_avg_sq[alive] == 2.0).all())
        assert not exp_avg[~alive].any() and not exp_avg_sq[~alive].any()
        untouched = torch.ones_like(before, dtype=torch.bool)
        untouched[lo:lo + C * KC * DC] = False
        assert torch.equal(m.flat_params[untouched], before[untouched])
        # the window after the restart holds step 2 alone
        assert torch.equal(cb.read()[0], torch.stack([torch.bincount(_inds(rank, 2)[:, c].reshape(-1), minlength=KC) for c in range(C)]))
        gathered = [torch.empty_like(m.flat_params) for _ in range(world)]
        dist.all_gather(gathered, m.flat_params)
        assert torch.equal(gathered[0], gathered[1]), "ranks diverged"
        q.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc() + repr(e)))
    finally:
        dist.destroy_process_group()


def test_two_rank_restart_uses_summed_counts_and_rank_zero_rows():
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
