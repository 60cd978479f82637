"""GPU: csrc/loglik.hip op by op against the float64 restatement of tests/loglik_checks.py, at the smallest shapes at which the
kernels can still go wrong, and the closed-form linear-Gaussian case through ``loglik.ImportanceLogLik``.

Bounds.  rows: both sides are float64 over the same fp32 values and differ by summation order only -- the kernel's tree over
12288 terms is about 60 roundings deep (7e-15), the restatement uses ``math.fsum`` -- so 1e-12 of the summed magnitudes leaves
two digits of margin.  latent: ``expf``'s 2 ulp plus two roundings, about 2.4e-7, with a margin of four; ``a`` is restated from the
kernel's own z.  merge: bit for bit between cuts; 1e-12 relative against the restatement (the device's ``exp`` and the host's
differ by an ulp or two of terms in [0, 1])."""
import math

import numpy as np
import pytest
import torch

from tests import loglik_checks as C
from tests.test_loglik_host import CLOSED

pytestmark = pytest.mark.gpu
SHAPES = [(1, 5, 5), (3, 8, 8), (3, 64, 64)]         # P = 25: the scalar path; 192; 12288: the workload's own row
BS = [(1, 1), (2, 3), (3, 4)]                        # (2, 3): where a wrong r / S shows


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _dense(t, fmt):
    return t.contiguous(memory_format=torch.channels_last) if fmt == "nhwc" else t.contiguous()


def _flat(t, fmt):
    """The rows as the kernel walks them: the tensor's memory order."""
    t = t.detach().cpu()
    return (t.permute(0, 2, 3, 1) if fmt == "nhwc" else t).contiguous().reshape(t.size(0), -1).numpy()


def _pictures(seed, B, S, shape):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((B,) + shape, generator=g)
    xhat = x.repeat_interleave(S, dim=0) + 0.1 * torch.randn((B * S,) + shape, generator=g)
    return xhat, x


# ---- rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["nchw", "nhwc"])
@pytest.mark.parametrize("B, S", BS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("sigma", [0.05, 1.0])
def test_rows_against_the_restatement(dev, shape, B, S, fmt, sigma):
    from ctvae_amd import kernels as K
    P, L = shape[0] * shape[1] * shape[2], 3
    xhat, x = _pictures(100 + P + 7 * B + S, B, S, shape)
    g = torch.Generator().manual_seed(5)
    mu, lv, eps = torch.randn(B, L, generator=g), 0.3 * torch.randn(B, L, generator=g), torch.randn(B, S, L, generator=g)
    z, a = K.loglik_latent(mu.to(dev), lv.to(dev), eps.to(dev))
    lw = K.loglik_rows(_dense(xhat.to(dev), fmt), _dense(x.to(dev), fmt), S, a, K.loglik_consts(sigma, P, dev))
    assert lw.dtype == torch.float64 and tuple(lw.shape) == (B * S,)
    ref, scale = C.log_weights(_flat(xhat, fmt), _flat(x, fmt), S, z.cpu().numpy(), eps.reshape(B * S, L).numpy(), lv.numpy(), sigma)
    err = np.abs(lw.cpu().numpy() - ref)
    print(shape, B, S, fmt, sigma, "max err / scale", float((err / scale).max()))
    assert np.all(err <= 1e-12 * scale)                          # every row


def test_rows_without_latent_terms_and_unaligned(dev):
    """a = None is 0; a 16-byte misaligned base takes the scalar path for a P that is a multiple of 4."""
    from ctvae_amd import kernels as K
    shape, B, S = (3, 8, 8), 2, 3
    xhat, x = _pictures(31, B, S, shape)
    consts = torch.tensor([1.0, 0.0], dtype=torch.float64, device=dev)
    ref = -C.sse_rows(_flat(xhat, "nchw"), _flat(x, "nchw"), S)
    lw = K.loglik_rows(xhat.to(dev), x.to(dev), S, None, consts).cpu().numpy()
    assert np.all(np.abs(lw - ref) <= 1e-12 * np.abs(ref))
    buf = torch.zeros(xhat.numel() + 1, device=dev)
    buf[1:] = xhat.reshape(-1).to(dev)
    shifted = buf[1:].view(xhat.shape)
    assert shifted.data_ptr() % 16 == 4
    lw2 = K.loglik_rows(shifted, x.to(dev), S, None, consts).cpu().numpy()
    assert np.all(np.abs(lw2 - ref) <= 1e-12 * np.abs(ref))


def test_rows_refuse_by_name(dev):
    from ctvae_amd import kernels as K
    xhat, x = _pictures(7, 2, 2, (3, 8, 8))
    xhat, x = xhat.to(dev), x.to(dev)
    consts = K.loglik_consts(1.0, 192, dev)
    with pytest.raises(ValueError, match="loglik_rows: xhat is channels-last and x is NCHW-contiguous: both must be dense in the same"):
        K.loglik_rows(_dense(xhat, "nhwc"), x, 2, None, consts)
    with pytest.raises(ValueError, match="loglik_rows: xhat is NCHW-contiguous and x is channels-last"):
        K.loglik_rows(xhat, _dense(x, "nhwc"), 2, None, consts)
    with pytest.raises(ValueError, match="loglik_rows: xhat is not dense"):
        K.loglik_rows(xhat[:, :, :, ::2], x[:, :, :, ::2].contiguous(), 2, None, consts)
    with pytest.raises(ValueError, match=r"loglik_rows: xhat \(4, 3, 8, 8\) must be \[B \* S, C, H, W\]"):
        K.loglik_rows(xhat, x, 3, None, consts)
    with pytest.raises(ValueError, match="loglik_rows: xhat must be a torch.float32"):
        K.loglik_rows(xhat.double(), x, 2, None, consts)
    with pytest.raises(ValueError, match="loglik_rows: S must be an integer"):
        K.loglik_rows(xhat, x, True, None, consts)
    with pytest.raises(ValueError, match="loglik_rows: a must be"):
        K.loglik_rows(xhat, x, 2, torch.zeros(3, dtype=torch.float64, device=dev), consts)
    with pytest.raises(ValueError, match="loglik_rows: consts must be a torch.float64"):
        K.loglik_rows(xhat, x, 2, None, consts.float())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.loglik_rows(xhat.cpu(), x.cpu(), 2, None, consts)
    for bad in (0, -1.0, float("inf"), True, "mse"):
        with pytest.raises(ValueError, match="loglik_consts: sigma"):
            K.loglik_consts(bad, 192, dev)
    got = K.loglik_consts(0.05, 12288, dev).cpu().tolist()
    assert got == list(C.consts(0.05, 12288))


# ---- latent ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [3, 10, 128])
@pytest.mark.parametrize("B, S", BS)
def test_latent_against_float64(dev, L, B, S):
    from ctvae_amd import kernels as K
    g = torch.Generator().manual_seed(40 + L + B)
    mu, lv, eps = 2 * torch.randn(B, L, generator=g), torch.randn(B, L, generator=g), torch.randn(B, S, L, generator=g)
    z, a = K.loglik_latent(mu.to(dev), lv.to(dev), eps.to(dev))
    assert z.dtype == torch.float32 and tuple(z.shape) == (B * S, L) and a.dtype == torch.float64 and tuple(a.shape) == (B * S,)
    ref, mag = C.reparameterize(mu.numpy(), lv.numpy(), eps.numpy(), S)
    zk = z.cpu().numpy()
    assert np.all(np.abs(zk - ref) <= 1e-6 * mag)
    ra, terms = C.latent_a(zk, eps.reshape(B * S, L).numpy(), lv.numpy(), S)              # from the kernel's own z
    assert np.all(np.abs(a.cpu().numpy() - ra) <= 1e-12 * terms)


def test_latent_refuses_by_name(dev):
    from ctvae_amd import kernels as K
    mu, lv, eps = torch.zeros(2, 4, device=dev), torch.zeros(2, 4, device=dev), torch.zeros(2, 3, 4, device=dev)
    with pytest.raises(ValueError, match=r"loglik_latent: eps must be \[B, S, L\]"):
        K.loglik_latent(mu, lv, eps.reshape(6, 4))
    with pytest.raises(ValueError, match="loglik_latent: mu .* must be"):
        K.loglik_latent(mu[:1], lv, eps)
    with pytest.raises(ValueError, match="loglik_latent: log_var must be a torch.float32"):
        K.loglik_latent(mu, lv.double(), eps)
    with pytest.raises(ValueError, match="loglik_latent: mu must be contiguous"):
        K.loglik_latent(torch.zeros(2, 8, device=dev)[:, :4], lv, eps)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.loglik_latent(mu.cpu(), lv.cpu(), eps.cpu())


# ---- merge / finish --------------------------------------------------------------------------------------------------------
def _device_merge(dev, lw, cut, capacity=None, row0=0, state=None):
    from ctvae_amd import kernels as K
    B = lw.shape[0]
    st, fl = state if state is not None else K.loglik_state(capacity or B, dev)
    at = 0
    for S in cut:
        K.loglik_merge(torch.from_numpy(np.ascontiguousarray(lw[:, at:at + S]).reshape(-1)).to(dev), S, st, fl, row0)
        at += S
    return st, fl


def _weights(kind, seed=9, B=5, K=24):
    lw = -1e5 + 1e3 * np.random.default_rng(seed).standard_normal((B, K))
    if kind == "increasing":
        lw = np.sort(lw, axis=1)
    elif kind == "decreasing":
        lw = np.sort(lw, axis=1)[:, ::-1].copy()
    assert kind == "far" or np.all(np.diff(lw, axis=1) != 0)
    return lw


@pytest.mark.parametrize("kind", ["far", "increasing", "decreasing"])
def test_merge_is_chunk_invariant_and_follows_the_restatement(dev, kind):
    from ctvae_amd import loglik
    lw = _weights(kind)
    assert np.all(np.exp(lw) == 0)                               # a naive exp underflows: log gives -inf
    runs = [_device_merge(dev, lw, cut) for cut in C.CUTS]
    for st, fl in runs[1:]:
        assert torch.equal(st, runs[0][0]) and torch.equal(fl, runs[0][1])           # bit for bit
    st, fl = runs[0][0].cpu().numpy(), runs[0][1].cpu().numpy()
    assert not fl.any() and np.all(st[:, 4] == lw.shape[1])
    got = loglik.finish(st, fl)
    want = C.estimate(lw)
    for k, w in zip(("loglik", "elbo", "ess"), want):
        assert np.all(np.abs(got[k] - w) <= 1e-12 * np.abs(w)), k
    lse = np.logaddexp.reduce(lw, axis=1) - math.log(lw.shape[1])
    assert np.all(np.abs(got["loglik"] - lse) <= 1e-12 * np.abs(lse))
    assert np.all(got["loglik"] >= got["elbo"]) and np.all(got["ess"] >= 1) and np.all(got["ess"] <= lw.shape[1])


def test_merge_flags_nonfinite_weights_and_their_image_only(dev):
    lw = _weights("far")
    bad = lw.copy()
    bad[1, 5], bad[3, 0], bad[3, 23] = np.nan, np.inf, -np.inf
    clean = _device_merge(dev, lw, [1, 7, 16])
    st, fl = _device_merge(dev, bad, [1, 7, 16])
    assert fl.cpu().tolist() == [0, 1, 0, 1, 0] and clean[1].cpu().tolist() == [0] * 5
    keep = torch.tensor([0, 2, 4], device=dev)
    assert torch.equal(st[keep], clean[0][keep])
    assert st[1, 4].item() == 23 and st[3, 4].item() == 22       # what was not finite was not merged


def test_merge_writes_its_rows_only(dev):
    from ctvae_amd import kernels as K
    lw = _weights("far", B=3)
    st, fl = K.loglik_state(8, dev)
    st[:] = -7.5                                                  # sentinels around the written range
    fl[:] = 9
    st[2:5], fl[2:5] = K.loglik_state(3, dev)
    _device_merge(dev, lw, [24], row0=2, state=(st, fl))
    alone = _device_merge(dev, lw, [24])
    assert torch.equal(st[2:5], alone[0]) and torch.equal(fl[2:5], alone[1])
    outside = torch.tensor([0, 1, 5, 6, 7], device=dev)
    assert bool((st[outside] == -7.5).all()) and bool((fl[outside] == 9).all())
    with pytest.raises(ValueError, match=r"loglik_merge: rows \[6, 9\) leave the capacity 8"):
        K.loglik_merge(torch.zeros(3, dtype=torch.float64, device=dev), 1, st, fl, 6)
    with pytest.raises(ValueError, match="loglik_merge: lw must be"):
        K.loglik_merge(torch.zeros(5, dtype=torch.float64, device=dev), 2, st, fl, 0)
    with pytest.raises(ValueError, match="loglik_merge: lw must be a torch.float64"):
        K.loglik_merge(torch.zeros(4, device=dev), 2, st, fl, 0)


def test_rows_and_merge_at_row0_with_sentinels(dev):
    """The chain rows -> merge at row0 > 0, as ``ImportanceLogLik`` runs it for its second batch."""
    from ctvae_amd import kernels as K, loglik
    shape, B, S = (3, 8, 8), 2, 3
    xhat, x = _pictures(77, B, S, shape)
    lw = K.loglik_rows(xhat.to(dev), x.to(dev), S, None, K.loglik_consts(0.05, 192, dev))
    st, fl = K.loglik_state(6, dev)
    st[:3], st[5] = 123.0, 123.0
    K.loglik_merge(lw, S, st, fl, 3)
    assert bool((st[:3] == 123.0).all()) and bool((st[5] == 123.0).all())
    got = loglik.finish(st[3:5].cpu().numpy(), fl[3:5].cpu().numpy())
    ref, _ = C.log_weights(_flat(xhat, "nchw"), _flat(x, "nchw"), S, None, None, None, 0.05)
    want = C.estimate(ref.reshape(B, S))
    assert np.all(np.abs(got["loglik"] - want[0]) <= 1e-12 * np.abs(want[0]))


# ---- the closed form through the library -----------------------------------------------------------------------------------
def test_closed_form_through_the_library(dev, monkeypatch):
    """A torch-linear decoder in fp32 with the exact posterior: every log-weight is log p(x) up to fp32 rounding in z and xhat."""
    from ctvae_amd import loglik
    case = C.linear_gaussian(**CLOSED)
    P, L, B, K_, chunk = CLOSED["P"], CLOSED["L"], 3, 32, 8
    W = torch.from_numpy(case["W"]).float().to(dev)
    b = torch.from_numpy(case["b"]).float().to(dev)
    seen = []

    def decode(z):
        seen.append(z.clone())
        return torch.nn.functional.linear(z, W, b).reshape(-1, 3, 4, 4)

    acc = loglik.ImportanceLogLik(L, P, case["sigma"], K_, chunk, dev, capacity=2)
    x = torch.from_numpy(case["x"]).float().to(dev).reshape(B, 3, 4, 4)
    mu, lv = torch.from_numpy(case["mu"]).float().to(dev), torch.from_numpy(case["log_var"]).float().to(dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    before = torch.cuda.get_rng_state(dev)
    acc.add_batch(x, mu, lv, decode, gen)
    assert torch.equal(torch.cuda.get_rng_state(dev), before)    # no other stream moved
    assert len(seen) == K_ // chunk and all(tuple(z.shape) == (B * chunk, L) for z in seen)
    res = acc.result()
    rel = np.abs(res["loglik"] - case["logpx"]) / np.abs(case["logpx"])
    print("closed form: rel err", rel, "ess", res["ess"])
    assert not res["nonfinite"].any() and np.all(rel <= 1e-4) and np.all(res["ess"] >= K_ * (1 - 1e-3))
    assert np.all(res["state"][:, 4] == K_)
    # a second batch grows the state by doubling (capacity 2 -> 4 -> 8) and leaves the first one's rows as they were
    acc.add_batch(x, mu, lv, decode, gen)
    acc.add_batch(x[:1], mu[:1], lv[:1], decode, gen)
    more = acc.result()
    assert acc.rows == 7 and acc.flags.numel() == 8 and np.array_equal(more["loglik"][:3], res["loglik"])
    assert np.all(np.abs(more["loglik"][3:] - case["logpx"][[0, 1, 2, 0]]) <= 1e-4 * np.abs(case["logpx"][[0, 1, 2, 0]]))
    # a batch whose chunk exceeds DECODE_ROWS goes through the decoder in groups of images: 2 + 1 here, in four chunks
    del seen[:]
    monkeypatch.setattr(loglik, "DECODE_ROWS", 16)
    grouped = loglik.ImportanceLogLik(L, P, case["sigma"], K_, chunk, dev)
    grouped.add_batch(x, mu, lv, decode, torch.Generator(device=dev).manual_seed(3))
    assert [z.size(0) for z in seen] == [16, 8] * 4
    assert np.all(np.abs(grouped.result()["loglik"] - case["logpx"]) <= 1e-4 * np.abs(case["logpx"]))
    assert np.all(grouped.result()["state"][:, 4] == K_)
    acc.reset()
    acc.add_batch(x[:2], mu[:2], lv[:2], decode, torch.Generator(device=dev).manual_seed(3))
    again = acc.result()
    assert len(again["loglik"]) == 2 and np.all(again["state"][:, 4] == K_)     # the rows a reset left behind were emptied first
    assert np.all(np.abs(again["loglik"] - case["logpx"][:2]) <= 1e-4 * np.abs(case["logpx"][:2]))
