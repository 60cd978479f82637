"""GPU: EMA codebooks (``exp_params.codebook_ema_decay``) through the training harness, the runner and a checkpoint:
optim.CodebookEMA on csrc/vqema.hip, its observer on the quantisers, its place behind the optimizer step.

The model specs are those of tests/test_codebook_gpu.py: MCQVAE of configs/mcq_vae.yaml at B = 4 (P = 256 latent rows, C = 4,
K = 64, Dc = 32) unless stated; one VQVAE and one CTMCQVAE case.  The model has neither BatchNorm nor noise, so a quantisation of
the test's own in front of a step says what the step's own index search will find.  The reference project has no EMA codebook:
the expected values are the float64 restatement of tests/vq_ema_checks.py."""
import io
import json
import os

import pytest
import torch
import yaml

from ctvae_amd import filler
from tests import helpers as H
from tests import vq_ema_checks as EC
from tests.test_codebook_gpu import (B, C, DC, EXP, KC, P, POISON, _assert_same, _batches, _ct_batch, _lines, _mcq, _snapshot,
                                     fixed_noise)  # noqa: F401
from tests.test_ct_gpu import build_ct

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECAY, EPS = EC.fp32(0.99), EC.fp32(1e-5)
KEY = {"codebook_ema_decay": 0.99}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _search(model, x):
    """(latent rows [P, D] on the host, indices [B, C, HW] on the host) of one batch with the model's weights as they are, by the
    quantiser's own ``compute_inds`` -- with no observer attached."""
    from ctvae_amd import kernels as K
    assert model.vq_layer.usage_observer is None and model.vq_layer.ema_observer is None
    with torch.no_grad():
        lat = model.encode(x)[0]
        inds = model.vq_layer.compute_inds(lat)
        rows = K.to_nhwc(lat).reshape(-1, lat.size(1)).cpu()
    return rows, inds.reshape(inds.size(0), -1, inds.size(-2) * inds.size(-1)).cpu()


def _ema_state(exp):
    torch.cuda.synchronize()
    e = exp.codebook_ema
    return {"N": e.N.clone(), "M": e.M.clone(), "acc_s": e.acc_s.clone(), "acc_n": e.acc_n.clone().float()}


def _codebook_range(exp):
    """[lo, hi): the codebooks inside the model's flat parameter (and gradient) buffer."""
    lo = (exp.codebook_ema.codebooks().data_ptr() - exp.model.flat_params.data_ptr()) // 4
    return lo, lo + C * KC * DC


def _window_bound(E0_N, E0_M, counts, sums, asums):
    """Tolerance of E after one update from the window (counts, sums): the update's own bound on the float64 statistics plus what
    the fp32 statistics may be off by, carried through E = (g M + (1-g) s) / Nt."""
    ref = EC.update64(E0_N, E0_M, counts, sums, DECAY, EPS)
    b = EC.update_bounds(E0_N, E0_M, counts, sums, DECAY, EPS)["E"]
    return ref, b + (1.0 - DECAY) * EC.stats_bound(counts, asums) / ref["Nt"][..., None]


# ---- (a) one step ----------------------------------------------------------------------------------------------
def test_one_step_updates_the_codebook_from_its_own_latents(dev):
    from ctvae_amd.experiment import VAEXperiment
    batch, = _batches(dev, 1)
    exp = VAEXperiment(_mcq(dev), dict(EXP, hipgraph=False, **KEY))
    ema = exp.codebook_ema
    assert exp.model.vq_layer.ema is ema and (ema.C, ema.K, ema.Dc) == (C, KC, DC)
    E0 = ema.codebooks().detach().cpu().clone()
    rows, inds = _search(exp.model, batch[0])
    counts, sums, asums, invalid = EC.stats64(rows, inds, KC)
    assert invalid == 0 and int(counts.sum()) == P * C
    exp.fit(lambda: iter([batch]), None, max_epochs=1)
    torch.cuda.synchronize()
    assert exp.global_step == 1 and ema.updates == 1 and ema.observed == 1 and exp.model.vq_layer.ema_observer is None
    ref, bound = _window_bound(torch.ones(C, KC), E0, counts, sums, asums)
    err = (ema.codebooks().detach().cpu().double() - ref["E"]).abs()
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    assert float((ema.codebooks().detach().cpu() - E0).abs().max()) > 0
    errN = (ema.N.cpu().double() - ref["N"]).abs()
    assert bool((errN <= EC.update_bounds(torch.ones(C, KC), E0, counts, sums, DECAY, EPS)["N"]).all())
    assert not ema.acc_n.any() and not ema.acc_s.any()
    lo, hi = _codebook_range(exp)
    assert not exp.model.flat_grads[lo:hi].any(), "the codebooks' block of the gradient buffer is an absent block: zeros"
    assert exp.model.flat_grads[:lo].any()


def test_loss_is_the_commitment_term_and_the_latent_gradient_is_unchanged(dev):
    """VQ_Loss = beta / (1 + beta) times the value without the key, within 4 ulp; the quantised latents and the gradient to the
    latents are bit for bit the non-EMA path's."""
    from ctvae_amd import kernels as K
    m = _mcq(dev)
    batch, = _batches(dev, 1)
    beta = float(m.vq_layer.beta)
    with torch.no_grad():
        lat = K.to_nhwc(m.encode(batch[0])[0]).contiguous().clone()
        inds = m.vq_layer.compute_inds(K.to_nchw_view(lat))
    w = torch.randn(lat.shape, generator=torch.Generator().manual_seed(3)).to(dev)
    out = {}
    for name, fn in (("plain", K.VQLookup), ("ema", K.VQLookupEMA)):
        m.zero_grad()
        leaf = lat.clone().requires_grad_(True)
        q, vq = fn.apply(leaf, inds, beta, KC, C, *m.vq_layer._codebooks())
        K.backward((q * w).sum() + 3.0 * vq)
        torch.cuda.synchronize()
        cb_grad = torch.cat([p.grad.reshape(-1) for p in m.vq_layer._codebooks()]) if name == "plain" else None
        out[name] = (q.detach().clone(), float(vq.detach()), leaf.grad.clone(), cb_grad)
    assert out["plain"][3].any()                                          # the non-EMA path did form a codebook gradient
    assert torch.equal(out["plain"][0].view(torch.int32), out["ema"][0].view(torch.int32))
    assert torch.equal(out["plain"][2].view(torch.int32), out["ema"][2].view(torch.int32)) and out["ema"][2].any()
    want = out["plain"][1] * (beta / (1.0 + beta))
    ulp = float(torch.tensor(out["ema"][1], dtype=torch.float32).abs().frexp()[1] - 24)
    print(f"VQ_Loss ema {out['ema'][1]!r} against {want!r}: {abs(out['ema'][1] - want) / 2.0 ** ulp:.2f} ulp")
    assert abs(out["ema"][1] - want) <= 4 * 2.0 ** ulp
    # the model's own records carry that value in training and validation
    plain = float(m(batch[0])[2].detach())
    m.vq_layer.ema = object()
    try:
        keyed = float(m(batch[0])[2].detach())
        with torch.no_grad():
            keyed_eval = float(m.eval()(batch[0])[2])
    finally:
        m.vq_layer.ema = None
        m.train()
    assert keyed == keyed_eval and abs(keyed - plain * beta / (1.0 + beta)) <= 4 * 2.0 ** ulp


# ---- (b) captured and eager --------------------------------------------------------------------------------------
def test_captured_and_eager_runs_agree(dev):
    from ctvae_amd.experiment import VAEXperiment, _GraphedTrainStep
    n = _GraphedTrainStep.WARM + 3
    batches = _batches(dev, n)
    out = {}
    for hipgraph in (True, False):
        exp = VAEXperiment(_mcq(dev), dict(EXP, hipgraph=hipgraph, **KEY))
        exp.fit(lambda: iter(batches), None, max_epochs=1)
        if hipgraph:
            gs = list(exp._graphed.values())
            assert len(gs) == 1 and gs[0].graph is not None and gs[0].seen == n
        else:
            assert not exp._graphed
        assert exp.codebook_ema.updates == n
        out[hipgraph] = ({**_snapshot(exp), **_ema_state(exp)})
    _assert_same(out[True], out[False], "captured and eager")
    assert float(out[True]["N"].min()) != 1.0 and not out[True]["acc_s"].any()


# ---- (c) accumulate_grad_batches ---------------------------------------------------------------------------------
@pytest.mark.parametrize("hipgraph", [True, False])
def test_one_update_per_window_from_the_windows_summed_statistics(dev, hipgraph):
    from ctvae_amd.experiment import VAEXperiment
    exp = VAEXperiment(_mcq(dev), dict(EXP, hipgraph=hipgraph, **KEY), accumulate_grad_batches=2)
    ema = exp.codebook_ema
    windows, observed = [], []
    inner_update, inner_observe = ema.update, ema.observe

    def spy_update(*a, **kw):
        torch.cuda.synchronize()
        windows.append((ema.acc_n.cpu().clone(), ema.acc_s.cpu().clone(), ema.N.cpu().clone(), ema.M.cpu().clone(), exp.global_step))
        return inner_update(*a, **kw)

    def spy_observe(*a, **kw):
        observed.append(exp.global_step)
        return inner_observe(*a, **kw)
    ema.update, ema.observe = spy_update, spy_observe
    batches = _batches(dev, 4)
    twin = _mcq(dev)                                                       # the weights both micro-batches of window 0 see
    stats = [EC.stats64(*_search(twin, b[0]), KC) for b in batches[:2]]
    exp.fit(lambda: iter(batches), None, max_epochs=1)
    torch.cuda.synchronize()
    assert exp.global_step == 2 and len(windows) == 2 and [w[4] for w in windows] == [0, 1]
    assert observed == [0, 0, 1, 1]                                         # per micro-batch (all four steps run Python: WARM = 3)
    for acc_n, _, _, _, _ in windows:
        assert [int(v) for v in acc_n.sum(dim=1)] == [2 * P] * C            # both micro-batches, every codebook
    acc_n, acc_s = windows[0][0], windows[0][1]
    assert torch.equal(acc_n, stats[0][0] + stats[1][0])
    err = (acc_s.double() - (stats[0][1] + stats[1][1])).abs()
    assert bool((err <= EC.stats_bound(acc_n, stats[0][2] + stats[1][2])).all())
    # the second update starts from the first one's N and M and the second window's sums
    ref = EC.update64(windows[1][2], windows[1][3], windows[1][0], windows[1][1], DECAY, EPS)
    bound = EC.update_bounds(windows[1][2], windows[1][3], windows[1][0], windows[1][1], DECAY, EPS)
    for name, got in (("N", ema.N), ("M", ema.M), ("E", ema.codebooks())):
        assert bool(((got.detach().cpu().double() - ref[name]).abs() <= bound[name]).all()), name
    assert not ema.acc_n.any() and not ema.acc_s.any()


# ---- (d) validation and sample_images ----------------------------------------------------------------------------
def test_validation_and_sampling_move_nothing(dev, tmp_path):
    from ctvae_amd.experiment import VAEXperiment
    exp = VAEXperiment(_mcq(dev), dict(EXP, **KEY), val_sampling=True, sample_dir=str(tmp_path))
    train, val = _batches(dev, 1), _batches(dev, 2, seed=4900)
    exp.fit(lambda: iter(train), None, max_epochs=1)
    before = {**_snapshot(exp), **_ema_state(exp)}
    hist = exp.fit(lambda: iter([]), lambda: iter(val), max_epochs=2, start_epoch=1, test_batches=lambda: iter(val))
    assert os.path.exists(tmp_path / "Reconstructions") and exp.codebook_ema.observed == 1 and exp.codebook_ema.updates == 1
    _assert_same(before, {**_snapshot(exp), **_ema_state(exp)}, "validation and sample_images")
    # the validation record carries the commitment-only loss: beta / (1 + beta) of a run without the key on the same weights
    plain = VAEXperiment(_mcq(dev), dict(EXP))
    from ctvae_amd import kernels as K
    plain.model.flat_params.copy_(exp.model.flat_params)
    K.bump_param_epoch()                                                   # (cached Winograd filters were made from the old values)
    h2 = plain.fit(lambda: iter([]), lambda: iter(val), max_epochs=1)
    beta = float(exp.model.vq_layer.beta)
    assert abs(hist[0]["val_VQ_Loss"] - h2[0]["val_VQ_Loss"] * beta / (1 + beta)) <= 1e-6 * h2[0]["val_VQ_Loss"]


# ---- (e) the runner: save, resume, refusals ------------------------------------------------------------------------
def _runner_cfg(tmp_path, sub, exp=None, **trainer):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "mcq_vae.yaml")))
    cfg["logging_params"]["save_dir"] = str(tmp_path / sub)
    cfg["data_params"]["train_batch_size"] = 8
    cfg["data_params"]["val_batch_size"] = 8
    cfg["exp_params"].update(exp or {})
    cfg["trainer_params"].update(trainer)
    p = tmp_path / f"{sub}.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_runner_resumes_bit_exactly_and_refuses_by_name(dev, tmp_path):
    from ctvae_amd import run
    last = lambda sub: tmp_path / sub / "MCQVAE" / "checkpoints" / "last.ckpt"
    steps = ["--steps-per-epoch", "3"]
    run.main(["-c", _runner_cfg(tmp_path, "straight", KEY)] + steps + ["--max-epochs", "2"])
    run.main(["-c", _runner_cfg(tmp_path, "first", KEY)] + steps + ["--max-epochs", "1"])
    run.main(["-c", _runner_cfg(tmp_path, "resumed", KEY, resume_from_checkpoint=str(last("first")))] + steps + ["--max-epochs", "2"])
    f = torch.load(last("first"), weights_only=True)
    assert set(f["trainer"]["codebook_ema"]) == {"decay", "eps", "N", "M", "acc_n", "acc_s", "invalid"}
    assert (f["trainer"]["codebook_ema"]["decay"], f["trainer"]["codebook_ema"]["eps"]) == (DECAY, EPS)
    assert not any("ema" in k for k in f["state_dict"])                    # state_dict is unchanged: the buffers are hidden
    a, b = torch.load(last("straight"), weights_only=True), torch.load(last("resumed"), weights_only=True)
    for k, v in a["state_dict"].items():
        assert torch.equal(v, b["state_dict"][k]), k
    for k in ("N", "M", "acc_n", "acc_s"):
        assert torch.equal(a["trainer"]["codebook_ema"][k], b["trainer"]["codebook_ema"][k]), k
    assert float(a["trainer"]["codebook_ema"]["N"].min()) != float(f["trainer"]["codebook_ema"]["N"].min())
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(a["trainer"]["optimizer"][k], b["trainer"]["optimizer"][k]), k
    recs = [json.loads(l) for l in open(tmp_path / "straight" / "MCQVAE" / "metrics_rank0.jsonl")]
    sizes = [r for r in recs if "codebook_ema_min_cluster" in r]
    assert sizes and all(0 < r["codebook_ema_min_cluster"] <= r["codebook_ema_max_cluster"] for r in sizes)
    assert all(f"codebook_ema_max_cluster_{i}" in sizes[0] for i in range(C))
    # a run without the key ignores the entry and writes none
    run.main(["-c", _runner_cfg(tmp_path, "nokey", resume_from_checkpoint=str(last("first")))] + steps + ["--max-epochs", "2"])
    assert "codebook_ema" not in torch.load(last("nokey"), weights_only=True)["trainer"]
    # under the key: another decay, another eps, or a checkpoint without the entry, are refused by name
    with pytest.raises(SystemExit, match=r"exp_params\.codebook_ema_decay.*first"):
        run.main(["-c", _runner_cfg(tmp_path, "bad", {"codebook_ema_decay": 0.9}, resume_from_checkpoint=str(last("first")))]
                 + steps + ["--max-epochs", "2"])
    with pytest.raises(SystemExit, match=r"exp_params\.codebook_ema_eps.*first"):
        run.main(["-c", _runner_cfg(tmp_path, "bad", dict(KEY, codebook_ema_eps=1e-3), resume_from_checkpoint=str(last("first")))]
                 + steps + ["--max-epochs", "2"])
    with pytest.raises(SystemExit, match=r"exp_params\.codebook_ema_decay.*nokey"):
        run.main(["-c", _runner_cfg(tmp_path, "bad", KEY, resume_from_checkpoint=str(last("nokey")))] + steps + ["--max-epochs", "3"])
    assert not last("bad").exists()
    # load_weights_only starts from N = 1, M = the loaded codebooks
    run.main(["-c", _runner_cfg(tmp_path, "wo", KEY, resume_from_checkpoint=str(last("first")), load_weights_only=True),
              "--steps-per-epoch", "1", "--max-epochs", "1"])
    d = torch.load(last("wo"), weights_only=True)["trainer"]["codebook_ema"]
    total = d["N"].double().sum(dim=1)                                     # one update from N = 1: g K + (1 - g) * 8 * 64 positions
    want = DECAY * KC + (1 - DECAY) * 8 * 64
    assert bool(((total - want).abs() <= 1e-5 * want).all()), (total, want)


# ---- (f) with dead-code restarts -----------------------------------------------------------------------------------
def test_restarted_codes_carry_one_observation_at_their_row(dev):
    from ctvae_amd.experiment import VAEXperiment
    exp = VAEXperiment(_mcq(dev, POISON), dict(EXP, codebook_restart_every=2, **KEY))
    dead = []
    inner = exp.codebook.restart

    def spy(*a, **kw):
        res = inner(*a, **kw)
        dead.extend(res[1])
        return res
    exp.codebook.restart = spy
    exp.fit(lambda: iter(_batches(dev, 2)), None, max_epochs=1)
    torch.cuda.synchronize()
    ema = exp.codebook_ema
    assert POISON in dead and 0 < len(dead) < C * KC and exp.codebook_restarted == len(dead) and ema.updates == 2
    N, M, E = ema.N.cpu(), ema.M.cpu(), ema.codebooks().detach().cpu()
    alive = torch.ones(C, KC, dtype=torch.bool)
    for c, k in dead:
        alive[c, k] = False
        assert float(N[c, k]) == 1.0 and torch.equal(M[c, k].view(torch.int32), E[c, k].view(torch.int32)), (c, k)
    assert float(E[POISON].abs().max()) < 1e3 and bool((N[alive] != 1.0).any())
    # the restart ran behind the update: a dead code's row is a pool row, not M / Nt of the poisoned value
    pool = exp.codebook.pool.cpu()
    c, k = POISON
    assert any(torch.equal(E[c, k], pool[r, c:c + DC]) for r in range(exp.codebook.valid_rows))


# ---- (g) the other two models --------------------------------------------------------------------------------------
def _one_step_invariants(exp, batches):
    """One optimizer step: sum_k N_k = g K + (1 - g) * (positions observed) per codebook, the codebook moved and is finite, its
    gradient block is zero."""
    ema = exp.codebook_ema
    seen = []
    inner = ema.update

    def spy(*a, **kw):
        seen.append(ema.acc_n.cpu().clone())
        return inner(*a, **kw)
    ema.update = spy
    E0 = ema.codebooks().detach().clone()
    exp.fit(lambda: iter(batches), None, max_epochs=1)
    torch.cuda.synchronize()
    assert ema.updates == 1 == len(seen) and int(ema.invalid) == 0
    want = DECAY * ema.K + (1 - DECAY) * seen[0].sum(dim=1).double()
    got = ema.N.cpu().double().sum(dim=1)
    assert bool(((got - want).abs() <= 1e-5 * want).all()), (got, want)
    E = ema.codebooks().detach()
    assert bool(torch.isfinite(E).all()) and not torch.equal(E, E0)
    lo = (E.data_ptr() - exp.model.flat_params.data_ptr()) // 4
    assert not exp.model.flat_grads[lo:lo + E.numel()].any()
    return seen[0]


def test_vqvae_takes_one_step(dev):
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    m = vae_models["VQVAE"](**{**H.VQVAE_CFG, "hidden_dims": list(H.VQVAE_CFG["hidden_dims"])})
    m.load_state_dict(filler.fill_state(H.vqvae_specs(), 77))
    exp = VAEXperiment(m.to(dev).train(), dict(EXP, **KEY))
    assert (exp.codebook_ema.C, exp.codebook_ema.K, exp.codebook_ema.Dc) == (1, 512, 64)
    acc_n = _one_step_invariants(exp, _batches(dev, 1))
    assert int(acc_n.sum()) == B * 256


def test_ct_mcq_vae_takes_one_step_and_update_parameters_is_refused(dev, fixed_noise):
    from ctvae_amd.experiment import VAEXperiment
    params = {"LR": 5e-4, "weight_decay": 0.0, "kld_weight": 0.00025, "hipgraph": False}
    with pytest.raises(ValueError, match="codebook_ema_decay.*update_parameters='ct_layer'"):
        VAEXperiment(build_ct(dev, 5), dict(params, update_parameters="ct_layer", **KEY))
    exp = VAEXperiment(build_ct(dev, 5), dict(params, **KEY))
    acc_n = _one_step_invariants(exp, [_ct_batch(dev, 301, "action", [0, 3, 0, 3])])
    assert int(acc_n.sum()) > 0 and int(acc_n.sum()) % (B * 64) == 0       # whole images' worth of positions per index search


# ---- (h) without the key ---------------------------------------------------------------------------------------------
def test_without_the_key_nothing_of_the_feature_runs(dev):
    from ctvae_amd import native
    from ctvae_amd.experiment import VAEXperiment
    batches = _batches(dev, 3)
    finals = {}
    for name, params in (("absent", dict(EXP, hipgraph=False)), ("none", dict(EXP, hipgraph=False, codebook_ema_decay=None))):
        assert ("codebook_ema_decay" in params) == (name == "none")
        log = io.StringIO()
        exp = VAEXperiment(_mcq(dev), params, log_file=log, log_every=1)
        assert exp.codebook_ema is None and exp.model.vq_layer.ema is None
        native.prof_report()
        native.prof_enable(True)
        try:
            exp.fit(lambda: iter(batches), None, max_epochs=1)
            torch.cuda.synchronize()
        finally:
            native.prof_enable(False)
        names = set(native.prof_report())
        assert names and not any("vq_ema" in n or "commit" in n for n in names), names
        assert any("vq_bwd_codebook" in n for n in names)                  # the codebook gradient is still formed
        assert not _lines(log, "codebook_ema_min_cluster") and "codebook_ema" not in exp.state_dict()
        finals[name] = _snapshot(exp)
    _assert_same(finals["absent"], finals["none"], "key absent and key None")
    # and under the key the launches are there, the codebook-gradient launches are not
    exp = VAEXperiment(_mcq(dev), dict(EXP, hipgraph=False, **KEY), log_file=io.StringIO(), log_every=1)
    native.prof_report()
    native.prof_enable(True)
    try:
        exp.fit(lambda: iter(batches), None, max_epochs=1)
        torch.cuda.synchronize()
    finally:
        native.prof_enable(False)
    rep = native.prof_report()
    assert rep["vq_ema_update_kernel"]["count"] == 3 and rep["vq_ema_stats_pos_kernel"]["count"] == 3
    assert rep["vq_lookup+loss_finish_commit"]["count"] == 3
    assert not any("vq_bwd_codebook" in n or n == "vq_cb_reduce_kernel" for n in rep), set(rep)
    assert len(_lines(exp.log_file, "codebook_ema_min_cluster")) == 3
