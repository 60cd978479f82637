"""CPU: gradient clipping settings (Lightning 1.6.5's gradient_clip_val / gradient_clip_algorithm) and their way through
VAEXperiment / FlatAdam, and a 2-rank gloo run showing that the norm is taken on the all-reduced, averaged gradient and that
both ranks step identically.  The kernel itself is replaced by a CPU test double here (the product has no CPU Adam)."""
import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_MCQ = dict(in_channels=3, embedding_dim=16, hidden_dims=[8, 16], num_embeddings=8, img_size=64, codebooks=1, beta=0.25)


def test_clip_settings_follow_lightning():
    from ctvae_amd.optim import clip_settings
    assert clip_settings(None) == (None, "norm")
    assert clip_settings(None, None) == (None, "norm")
    assert clip_settings(0) == (None, "norm")
    assert clip_settings(0.0, "value") == (None, "value")
    assert clip_settings(-1.0) == (None, "norm")              # Lightning skips clipping for a value <= 0
    assert clip_settings(0.8) == (0.8, "norm")
    assert clip_settings(2, "Value") == (2.0, "value")
    for bad in ("l2", "", "inf", 2):
        with pytest.raises(ValueError, match="gradient_clip_algorithm"):
            clip_settings(0.8, bad)
    with pytest.raises(ValueError, match="gradient_clip_algorithm"):
        clip_settings(None, "l1")                            # checked even when clipping is off, as the Trainer does
    for bad in ("0.8", True, [0.8], float("nan")):
        with pytest.raises(TypeError):
            clip_settings(bad)


def test_header_algorithm_codes_match_python():
    from ctvae_amd import kernels as K
    hdr = open(os.path.join(ROOT, "include", "ctvae_hip.h")).read()
    codes = {k.lower(): int(v) for k, v in re.findall(r"#define CTVAE_CLIP_([A-Z]+) (\d+)", hdr)}
    assert codes == K.CLIP_ALGORITHMS


def _small_mcq():
    from ctvae_amd.models import vae_models
    torch.manual_seed(0)
    return vae_models["MCQVAE"](**SMALL_MCQ)


def test_experiment_validates_and_routes_the_clip(monkeypatch):
    """An unknown algorithm fails when the experiment is built; clipping off calls K.adam_step with today's arguments, on
    calls K.adam_step_clipped with the optimizer's slice, the DDP scale and the settings."""
    from ctvae_amd import kernels as K
    from ctvae_amd.experiment import VAEXperiment
    params = {"LR": 1e-3, "kld_weight": 1.0}
    m = _small_mcq()
    with pytest.raises(ValueError):
        VAEXperiment(m, params, gradient_clip_val=0.5, gradient_clip_algorithm="max")
    calls = []
    monkeypatch.setattr(K, "adam_step", lambda *a: calls.append(("plain", a)))
    monkeypatch.setattr(K, "adam_step_clipped", lambda *a: calls.append(("clipped", a)))
    for clip in (None, 0):
        exp = VAEXperiment(m, params, gradient_clip_val=clip)
        exp.optimizer_step()
        kind, a = calls.pop()
        assert kind == "plain" and len(a) == 6 and a[5] == 1.0 and exp.optimizer.grad_norm is None
    exp = VAEXperiment(m, {**params, "update_parameters": "decoder"}, gradient_clip_val=0.5, gradient_clip_algorithm="Norm")
    exp.optimizer.step(grad_scale=0.25)
    kind, a = calls.pop()
    sl = m.flat_range("decoder")
    assert kind == "clipped" and a[5:8] == (0.25, "norm", 0.5)
    assert a[0].data_ptr() == m.flat_params[sl].data_ptr() and a[1].numel() == sl.stop - sl.start
    assert a[9] is exp.optimizer.grad_norm and a[9].dim() == 0
    exp = VAEXperiment(m, params, gradient_clip_val=3, gradient_clip_algorithm="value")
    exp.optimizer_step()
    kind, a = calls.pop()
    assert kind == "clipped" and a[5:8] == (1.0, "value", 3.0) and a[9] is None and exp.optimizer.grad_norm is None


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _adam_clipped_cpu(flat_params, flat_grads, exp_avg, exp_avg_sq, state, grad_scale, algorithm, clip_val, workspace=None,
                      norm_out=None):
    """TEST DOUBLE of ctvae_adam_step_clipped (csrc/pointwise.hip): clip g * grad_scale as torch does, then torch.optim.Adam's
    rule on the flat buffers, state = [step, lr, b1, b2, eps, wd, b1^t, b2^t]."""
    g = flat_grads * grad_scale
    if algorithm == "norm":
        total = g.norm()
        if norm_out is not None:
            norm_out.fill_(total)
        g = g * torch.clamp(clip_val / (total + 1e-6), max=1.0)
    else:
        g = g.clamp(-clip_val, clip_val)
    st = state
    st[0] += 1
    st[6] *= st[2]
    st[7] *= st[3]
    g = g + st[5] * flat_params
    exp_avg.mul_(st[2]).add_(g, alpha=float(1 - st[2]))
    exp_avg_sq.mul_(st[3]).addcmul_(g, g, value=float(1 - st[3]))
    denom = (exp_avg_sq / (1 - st[7])).sqrt_().add_(st[4])
    flat_params.addcdiv_(exp_avg / (1 - st[6]), denom, value=-float(st[1]))


def _clip_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from ctvae_amd import kernels as K
        from ctvae_amd.ddp import GradBucketAllReduce
        from ctvae_amd.experiment import VAEXperiment
        from ctvae_amd.models import vae_models
        K.adam_step_clipped = _adam_clipped_cpu               # the product has no CPU Adam; see _adam_clipped_cpu
        for algorithm, clip in (("norm", 0.5), ("value", 0.3)):
            torch.manual_seed(7 + rank)                       # different init per rank: the broadcast makes them equal
            m = vae_models["MCQVAE"](**SMALL_MCQ)
            ddp = GradBucketAllReduce(m, bucket_bytes=1 << 16)
            exp = VAEXperiment(m, {"LR": 1e-3, "weight_decay": 1e-4, "kld_weight": 1.0}, ddp=ddp, gradient_clip_val=clip,
                               gradient_clip_algorithm=algorithm)
            n = m.flat_grads.numel()
            ref = torch.nn.Parameter(m.flat_params.clone())
            ropt = torch.optim.Adam([ref], lr=1e-3, weight_decay=1e-4)
            for step in range(3):
                grads = [torch.randn(n, generator=torch.Generator().manual_seed(1000 * step + r)) * (r + 1) for r in range(world)]
                m.flat_grads.copy_(grads[rank])
                exp.optimizer_step()                          # all-reduce (SUM), then the clipped step with grad_scale = 1/W
                ref.grad = sum(grads) / world                 # what torch DDP hands the clip: the averaged gradient
                if algorithm == "norm":
                    ref_norm = torch.nn.utils.clip_grad_norm_([ref], clip)
                    assert ref_norm > clip
                    torch.testing.assert_close(exp.optimizer.grad_norm, ref_norm, rtol=1e-5, atol=0)
                    local = float(grads[rank].norm())
                    assert abs(local - float(ref_norm)) > 1e-3 * local, "norm of the local gradient, not of the average"
                else:
                    assert bool((ref.grad.abs() > clip).any())
                    torch.nn.utils.clip_grad_value_([ref], clip)
                ropt.step()
            torch.testing.assert_close(m.flat_params, ref.detach(), rtol=1e-5, atol=1e-7)
            gathered = [torch.empty_like(m.flat_params) for _ in range(world)]
            dist.all_gather(gathered, m.flat_params)
            assert torch.equal(gathered[0], gathered[1]), "ranks diverged"
        q.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc() + repr(e)))
    finally:
        dist.destroy_process_group()


def test_two_rank_clip_uses_the_averaged_gradient():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_clip_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in range(2))
    for p in procs:
        p.join(60)
    assert res == {0: "ok", 1: "ok"}, res
