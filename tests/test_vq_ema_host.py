"""Host side of the EMA codebooks (``exp_params.codebook_ema_decay`` / ``codebook_ema_eps``; optim.CodebookEMA on csrc/vqema.hip):
the settings validator, the refusals of the experiment, the runner and a resume, properties of the float64 restatement the GPU
tests compare against (tests/vq_ema_checks.py), the state round trip on CPU tensors and the C ABI's prototypes.  No GPU: nothing
here launches a kernel."""
import os
import re

import pytest
import torch
import yaml

from tests import vq_ema_checks as EC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(in_channels=3, embedding_dim=16, hidden_dims=[8, 16], num_embeddings=8, img_size=64, codebooks=4, beta=0.25)
PARAMS = {"LR": 1e-3, "weight_decay": 0.0, "kld_weight": 1.0, "manual_seed": 11}


def _mcq(**over):
    from ctvae_amd.models import vae_models
    torch.manual_seed(7)
    cfg = dict(CFG, **over)
    return vae_models["MCQVAE"](**dict(cfg, hidden_dims=list(cfg["hidden_dims"])))


# ---- settings ----------------------------------------------------------------------------------------------
def test_settings_accept_and_round_to_fp32_once():
    from ctvae_amd.optim import codebook_ema_settings
    assert codebook_ema_settings(None) == (None, None)
    d, e = codebook_ema_settings(0.99)
    assert d == EC.fp32(0.99) != 0.99 and e == EC.fp32(1e-5) != 1e-5
    assert codebook_ema_settings(0.5, 0.25) == (0.5, 0.25)
    assert codebook_ema_settings(d, e) == (d, e)                      # rounding again changes nothing


@pytest.mark.parametrize("bad", [True, False, 1, 0, "0.99", 0.0, 1.0, -0.5, 1.5, [0.9], float("nan"), 1.0 - 1e-12, 1e-60])
def test_settings_refuse_the_decay_by_name(bad):
    from ctvae_amd.optim import codebook_ema_settings
    with pytest.raises(ValueError, match="codebook_ema_decay"):
        codebook_ema_settings(bad)


@pytest.mark.parametrize("bad", [True, 1, "1e-5", 0.0, -1e-5, float("inf"), float("nan"), 1e-60, [1e-5]])
def test_settings_refuse_eps_by_name(bad):
    from ctvae_amd.optim import codebook_ema_settings
    with pytest.raises(ValueError, match="codebook_ema_eps"):
        codebook_ema_settings(0.99, bad)


def test_settings_refuse_eps_alone():
    from ctvae_amd.optim import codebook_ema_settings
    with pytest.raises(ValueError, match="codebook_ema_eps.*without codebook_ema_decay"):
        codebook_ema_settings(None, 1e-5)


# ---- the float64 reference ---------------------------------------------------------------------------------
def _state(C=3, K=37, Dc=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    N = torch.rand(C, K, generator=g) * 4 + 0.01
    M = torch.randn(C, K, Dc, generator=g)
    acc_n = torch.randint(0, 50, (C, K), generator=g)
    acc_s = torch.randn(C, K, Dc, generator=g) * acc_n[..., None]
    return N, M, acc_n, acc_s


def test_reference_empty_window_leaves_the_codebook():
    """N = 1, M = E, nothing observed: Nt_k = N_k in exact arithmetic, so E stays -- here to float64's rounding."""
    g = torch.Generator().manual_seed(1)
    E = torch.randn(2, 64, 32, generator=g)
    N = torch.ones(2, 64)
    zero_n, zero_s = torch.zeros(2, 64, dtype=torch.int64), torch.zeros(2, 64, 32)
    d, e = EC.fp32(0.99), EC.fp32(1e-5)
    N1, M1 = N, E
    for _ in range(3):                                                # and again from the decayed state
        ref = EC.update64(N1, M1, zero_n, zero_s, d, e)
        assert float((ref["E"] - E.double()).abs().max()) <= 1e-14 * float(E.abs().max())
        assert float((ref["Nt"] - ref["N"]).abs().max()) <= 1e-15
        N1, M1 = ref["N"], ref["M"]


def test_reference_unused_code_decays_towards_the_origin():
    N, M, acc_n, acc_s = _state()
    acc_n[:, 5], acc_s[:, 5] = 0, 0.0
    d, e = 0.75, EC.fp32(1e-5)
    ref = EC.update64(N, M, acc_n, acc_s, d, e)
    assert torch.equal(ref["M"][:, 5], d * M[:, 5].double()) and torch.equal(ref["N"][:, 5], d * N[:, 5].double())
    # the used codes pull the total up, so the unused code's smoothed size grows relative to its M: |E| shrinks step by step
    prev = (M[:, 5].double() / N[:, 5].double()[:, None]).norm(dim=1)
    Nc, Mc = N, M
    for _ in range(4):
        ref = EC.update64(Nc, Mc, acc_n, acc_s, d, 1.0)               # a large eps makes the shrinkage visible
        now = ref["E"][:, 5].norm(dim=1)
        assert bool((now < prev).all())
        prev, Nc, Mc = now, ref["N"], ref["M"]


def test_reference_smoothed_sizes_sum_to_the_total():
    for seed, eps in ((0, 1e-5), (1, 0.5), (2, 100.0)):
        N, M, acc_n, acc_s = _state(seed=seed)
        ref = EC.update64(N, M, acc_n, acc_s, EC.fp32(0.9), eps)
        assert float((ref["Nt"].sum(dim=1) - ref["n"]).abs().max()) <= 1e-13 * float(ref["n"].max())
        assert float((ref["N"].sum(dim=1) - ref["n"]).abs().max()) == 0.0


def test_reference_statistics_use_the_slice_quirk_and_skip_bad_indices():
    x = torch.arange(2 * 6, dtype=torch.float32).view(2, 6)           # P = 2, D = 6, C = 2, Dc = 3
    inds = torch.tensor([[[1], [0]], [[1], [7]]])                     # [B = 2, C = 2, HW = 1]; 7 is outside K = 3
    counts, sums, asums, invalid = EC.stats64(x, inds, 3)
    assert counts.tolist() == [[0, 2, 0], [1, 0, 0]] and invalid == 1
    assert sums[0, 1].tolist() == [0 + 6, 1 + 7, 2 + 8]               # codebook 0: columns 0 .. 2 of both rows
    assert sums[1, 0].tolist() == [1, 2, 3]                           # codebook 1: columns 1 .. 3 (not 3 .. 5) of row 0
    assert float(sums.sum()) == 6 + 8 + 10 + 6 and torch.equal(sums, asums)


# ---- CodebookEMA on CPU tensors ----------------------------------------------------------------------------
def test_state_dict_round_trip_and_refusals():
    from ctvae_amd.optim import CodebookEMA
    a = CodebookEMA(_mcq().vq_layer, 0.99)
    assert (a.C, a.K, a.Dc, a.D) == (4, 8, 4, 16) and a.decay == EC.fp32(0.99) and a.eps == EC.fp32(1e-5)
    assert torch.equal(a.N, torch.ones(4, 8)) and torch.equal(a.M, a.codebooks()) and a.M.data_ptr() != a.codebooks().data_ptr()
    assert not a.acc_n.any() and not a.acc_s.any() and a.acc_n.dtype == torch.int64 and a.acc_s.dtype == torch.float32
    g = torch.Generator().manual_seed(3)
    a.N.copy_(torch.rand(4, 8, generator=g))
    a.M.copy_(torch.randn(4, 8, 4, generator=g))
    a.acc_n.copy_(torch.randint(0, 9, (4, 8), generator=g))
    a.acc_s.copy_(torch.randn(4, 8, 4, generator=g))
    a.invalid.fill_(3)
    sd = a.state_dict()
    assert set(sd) == {"decay", "eps", "N", "M", "acc_n", "acc_s", "invalid"}
    b = CodebookEMA(_mcq().vq_layer, 0.99)
    b.load_state_dict(sd)
    for k in ("N", "M", "acc_n", "acc_s"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert int(b.invalid) == 3
    sd["N"][0, 0] = -1.0                                              # the state is a copy, not a view
    assert float(a.N[0, 0]) != -1.0
    with pytest.raises(RuntimeError, match="codebook_ema_decay"):
        CodebookEMA(_mcq().vq_layer, 0.9).load_state_dict(a.state_dict())
    with pytest.raises(RuntimeError, match="codebook_ema_eps"):
        CodebookEMA(_mcq().vq_layer, 0.99, 1e-3).load_state_dict(a.state_dict())
    with pytest.raises(RuntimeError, match="does not fit"):
        CodebookEMA(_mcq(num_embeddings=16).vq_layer, 0.99).load_state_dict(a.state_dict())
    with pytest.raises(ValueError, match="codebook_ema_decay"):
        CodebookEMA(_mcq().vq_layer, None)
    # restarted codes: one observation at the new row
    rows = torch.full((2, 4), 7.0)
    b.reset_codes([(1, 2), (3, 0)], rows)
    assert float(b.N[1, 2]) == 1.0 == float(b.N[3, 0]) and torch.equal(b.M[1, 2], rows[0]) and torch.equal(b.M[3, 0], rows[1])
    b.reset_codes([(0, 1, 99)])                                       # without rows: the code's own codebook row
    assert float(b.N[0, 1]) == 1.0 and torch.equal(b.M[0, 1], b.codebooks()[0, 1])
    with pytest.raises(ValueError, match="out of range"):
        b.reset_codes([(4, 0)])
    b.restart_from_codebooks()
    assert torch.equal(b.N, torch.ones(4, 8)) and torch.equal(b.M, b.codebooks()) and not b.words.any() and not b.acc_s.any()


def test_wrappers_check_before_any_launch():
    """Wrong dtype, shape or layout raise a ValueError that names the problem; on CPU tensors a correct call ends at the
    no-CPU-fallback error, so nothing here reaches a launch."""
    from ctvae_amd import kernels as K
    C, Kc, Dc, B, HW = 2, 8, 4, 3, 5
    lat = torch.zeros(B, HW, C * Dc)
    inds = torch.zeros(B, C, HW, dtype=torch.int64)
    acc_n, acc_s, inv = torch.zeros(C, Kc, dtype=torch.int64), torch.zeros(C, Kc, Dc), torch.zeros(1, dtype=torch.int64)
    assert K.vq_ema_supported(64, 4, 32) and K.vq_ema_supported(512, 1, 64) and K.vq_ema_supported(16, 1, 256)
    assert not K.vq_ema_supported(64, 9, 32) and not K.vq_ema_supported(64, 1, 257) and not K.vq_ema_supported(0, 1, 4)
    for bad, match in (((lat.double(), inds, acc_n, acc_s, inv), "latents must be a torch.float32"),
                       ((lat, inds.int(), acc_n, acc_s, inv), "inds must be a torch.int64"),
                       ((lat, inds, acc_n.int(), acc_s, inv), "acc_n must be a torch.int64"),
                       ((lat, inds, acc_n, acc_s.double(), inv), "acc_s must be a torch.float32"),
                       ((lat, inds, acc_n, acc_s, inv.int()), "invalid must be a torch.int64"),
                       ((lat.transpose(0, 1), inds, acc_n, acc_s, inv), "latents must be contiguous"),
                       ((lat, inds.transpose(0, 2), acc_n, acc_s, inv), "inds must be contiguous"),
                       ((lat, inds, acc_n, acc_s[:, :, :2], inv), "acc_s must be contiguous"),
                       ((lat[:2], inds, acc_n, acc_s, inv), "do not fit together"),
                       ((lat, inds[:, :1].contiguous(), acc_n, acc_s, inv), "do not fit together"),
                       ((lat, inds, acc_n[:1], acc_s, inv), "do not fit together"),
                       ((lat, inds, acc_n, acc_s, torch.zeros(2, dtype=torch.int64)), "do not fit together"),
                       ((torch.zeros(B, HW, 9 * Dc), torch.zeros(B, 9, HW, dtype=torch.int64), torch.zeros(9, Kc, dtype=torch.int64),
                         torch.zeros(9, Kc, Dc), inv), "not covered")):
        with pytest.raises(ValueError, match=match):
            K.vq_ema_stats(*bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.vq_ema_stats(lat, inds, acc_n, acc_s, inv)
    cb, N, M = torch.zeros(C, Kc, Dc), torch.ones(C, Kc), torch.zeros(C, Kc, Dc)
    for bad, match in (((cb.double(), N, M, acc_n, acc_s, 0.9, 1e-5), "codebooks must be a torch.float32"),
                       ((cb, N[:, :4], M, acc_n, acc_s, 0.9, 1e-5), "N must be contiguous"),
                       ((cb, N[:1], M, acc_n, acc_s, 0.9, 1e-5), r"N \(1, 8\) \[C, K\]"),
                       ((cb, N, M[:, :, :2].contiguous(), acc_n, acc_s, 0.9, 1e-5), "must be"),
                       ((cb, N, M, acc_n, acc_s, 1.0, 1e-5), "decay"),
                       ((cb, N, M, acc_n, acc_s, 0.9, 0.0), "eps")):
        with pytest.raises(ValueError, match=match):
            K.vq_ema_update(*bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.vq_ema_update(cb, N, M, acc_n, acc_s, 0.9, 1e-5)


# ---- the experiment ----------------------------------------------------------------------------------------
def test_experiment_builds_nothing_without_the_key():
    from ctvae_amd.experiment import VAEXperiment
    m = _mcq()
    exp = VAEXperiment(m, dict(PARAMS))
    assert exp.codebook_ema is None and "codebook_ema" not in exp.state_dict()
    assert m.vq_layer.ema is None and m.vq_layer.ema_observer is None
    exp.codebook_update()                           # nothing to do, nothing launched
    with exp._counting_training_codes():
        assert m.vq_layer.ema_observer is None


def test_experiment_objects_on_the_host():
    from ctvae_amd.experiment import VAEXperiment
    m = _mcq()
    exp = VAEXperiment(m, dict(PARAMS, codebook_ema_decay=0.99, codebook_ema_eps=1e-4))
    ema = exp.codebook_ema
    assert m.vq_layer.ema is ema and m.vq_layer.ema_observer is None            # the observer: inside fit() only
    assert (ema.decay, ema.eps) == (EC.fp32(0.99), EC.fp32(1e-4))
    with exp._counting_training_codes():
        assert m.vq_layer.ema_observer == ema.observe and m.vq_layer.usage_observer is None
    assert m.vq_layer.ema_observer is None
    with pytest.raises(ZeroDivisionError):
        with exp._counting_training_codes():
            1 / 0
    assert m.vq_layer.ema_observer is None
    sd = exp.state_dict()
    assert set(sd["codebook_ema"]) == {"decay", "eps", "N", "M", "acc_n", "acc_s", "invalid"}
    assert not any("ema" in k or k.endswith((".N", ".M")) for k in m.state_dict())      # hidden buffers: state_dict is unchanged
    assert sorted(m.state_dict()) == sorted(_mcq().state_dict())
    # full resume: the same settings load, others and a checkpoint without the entry are refused by name, no key ignores it
    ema.N.mul_(0.5)
    sd = exp.state_dict()
    b = VAEXperiment(_mcq(), dict(PARAMS, codebook_ema_decay=0.99, codebook_ema_eps=1e-4))
    b.load_state_dict(sd)
    assert torch.equal(b.codebook_ema.N, ema.N)
    with pytest.raises(RuntimeError, match="codebook_ema_decay"):
        VAEXperiment(_mcq(), dict(PARAMS, codebook_ema_decay=0.9, codebook_ema_eps=1e-4)).load_state_dict(sd)
    with pytest.raises(RuntimeError, match="codebook_ema_eps"):
        VAEXperiment(_mcq(), dict(PARAMS, codebook_ema_decay=0.99)).load_state_dict(sd)
    with pytest.raises(RuntimeError, match=r"trainer\['codebook_ema'\].*codebook_ema_decay"):
        b.load_state_dict(VAEXperiment(_mcq(), dict(PARAMS)).state_dict())
    VAEXperiment(_mcq(), dict(PARAMS)).load_state_dict(sd)
    # both quantiser classes
    from ctvae_amd.models import vae_models
    from ctvae_amd.optim import CodebookEMA
    v = vae_models["VQVAE"](in_channels=3, embedding_dim=16, num_embeddings=32, hidden_dims=[8, 16], img_size=64)
    u = CodebookEMA(v.vq_layer, 0.9)
    assert (u.C, u.K, u.Dc, u.D) == (1, 32, 16, 16) and v.vq_layer.ema is None


def test_experiment_refuses_by_name():
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    vanilla = vae_models["VanillaVAE"](in_channels=3, latent_dim=16)
    with pytest.raises(ValueError, match="codebook_ema_decay.*vq_layer.*VanillaVAE"):
        VAEXperiment(vanilla, dict(PARAMS, codebook_ema_decay=0.99))
    for bad in (True, 1, "0.99", 1.0, 0.0):
        with pytest.raises(ValueError, match="codebook_ema_decay"):
            VAEXperiment(_mcq(), dict(PARAMS, codebook_ema_decay=bad))
    with pytest.raises(ValueError, match="codebook_ema_eps.*without codebook_ema_decay"):
        VAEXperiment(_mcq(), dict(PARAMS, codebook_ema_eps=1e-5))
    with pytest.raises(ValueError, match="codebook_ema_eps"):
        VAEXperiment(_mcq(), dict(PARAMS, codebook_ema_decay=0.99, codebook_ema_eps=0))
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "ct_mcq_vae.yaml")))
    torch.manual_seed(3)
    ct = vae_models["CTMCQVAE"](**cfg["model_params"])
    ep = dict(cfg["exp_params"])
    assert ep["update_parameters"] == "ct_layer"
    with pytest.raises(ValueError, match="codebook_ema_decay.*update_parameters='ct_layer'"):
        VAEXperiment(ct, dict(ep, codebook_ema_decay=0.99))
    assert ct.vq_layer.ema is None                                   # a refused key leaves the model as it was
    del ep["update_parameters"]
    assert VAEXperiment(ct, dict(ep, codebook_ema_decay=0.99)).codebook_ema is ct.vq_layer.ema is not None


# ---- the runner --------------------------------------------------------------------------------------------
def _config(tmp_path, name, exp=None, **trainer):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", name)))
    cfg["trainer_params"].update(trainer)
    cfg["exp_params"].update(exp or {})
    cfg["logging_params"]["save_dir"] = str(tmp_path / "logs")
    p = tmp_path / name
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_runner_refuses_by_name(tmp_path):
    from ctvae_amd import run
    for bad in (True, 1, "0.99", 1.0, 0.0, -0.1):
        with pytest.raises(SystemExit, match=r"exp_params\.codebook_ema_decay"):
            run.main(["-c", _config(tmp_path, "mcq_vae.yaml", exp={"codebook_ema_decay": bad})])
    for bad in (True, 1, "1e-5", 0.0, -1.0):
        with pytest.raises(SystemExit, match=r"exp_params\.codebook_ema_eps"):
            run.main(["-c", _config(tmp_path, "mcq_vae.yaml", exp={"codebook_ema_decay": 0.99, "codebook_ema_eps": bad})])
    with pytest.raises(SystemExit, match=r"exp_params\.codebook_ema_eps.*without codebook_ema_decay"):
        run.main(["-c", _config(tmp_path, "mcq_vae.yaml", exp={"codebook_ema_eps": 1e-5})])
    with pytest.raises(SystemExit, match=r"exp_params\.codebook_ema_decay.*vq_layer.*VanillaVAE"):
        run.main(["-c", _config(tmp_path, "vae.yaml", exp={"codebook_ema_decay": 0.99})])
    with pytest.raises(SystemExit, match=r"exp_params\.codebook_ema_decay.*update_parameters.*ct_layer"):
        run.main(["-c", _config(tmp_path, "ct_mcq_vae.yaml", exp={"codebook_ema_decay": 0.99})])
    assert not (tmp_path / "logs").exists()
    for name in ("mcq_vae.yaml",):
        cfg = yaml.safe_load(open(_config(tmp_path, name, exp={"codebook_ema_decay": 0.99})))
        assert run.exp_codebook_ema(cfg) == (EC.fp32(0.99), EC.fp32(1e-5))
        assert run.exp_codebook_ema(yaml.safe_load(open(_config(tmp_path, name)))) == (None, None)


def test_resume_check_refuses_by_name():
    from ctvae_amd.run import check_codebook_ema_checkpoint
    d, e = EC.fp32(0.99), EC.fp32(1e-5)
    good = {"state_dict": {}, "trainer": {"codebook_ema": {"decay": d, "eps": e}}}
    check_codebook_ema_checkpoint(good, "a.ckpt", d, e)
    for ckpt in ({"state_dict": {}, "trainer": {}}, {"state_dict": {}}):
        with pytest.raises(SystemExit, match=r"exp_params\.codebook_ema_decay.*a\.ckpt.*trainer\['codebook_ema'\]"):
            check_codebook_ema_checkpoint(ckpt, "a.ckpt", d, e)
    with pytest.raises(SystemExit, match=r"exp_params\.codebook_ema_decay.*a\.ckpt"):
        check_codebook_ema_checkpoint(good, "a.ckpt", 0.5, e)
    with pytest.raises(SystemExit, match=r"exp_params\.codebook_ema_eps.*a\.ckpt"):
        check_codebook_ema_checkpoint(good, "a.ckpt", d, 0.5)


def test_existing_configs_do_not_set_the_keys():
    for name in os.listdir(os.path.join(ROOT, "configs")):
        if name.endswith(".yaml"):
            ep = yaml.safe_load(open(os.path.join(ROOT, "configs", name))).get("exp_params", {})
            assert not any(k.startswith("codebook_ema") for k in ep), name


# ---- the C ABI ---------------------------------------------------------------------------------------------
def test_header_and_ctypes_prototypes_agree():
    import ctypes
    from ctvae_amd import native
    hdr = open(os.path.join(ROOT, "include", "ctvae_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = dict((m.group(1), m.group(2)) for m in re.finditer(r"\b(ctvae_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", hdr, re.S))
    ck = {ctypes.c_void_p: "ptr", ctypes.c_int: "int", ctypes.c_float: "float", ctypes.c_size_t: "long", ctypes.c_long: "long"}

    def kind(param):
        param = " ".join(param.split())
        if "*" in param:
            return "ptr"
        return {"int": "int", "float": "float", "size_t": "long", "long": "long"}[param.rsplit(" ", 1)[0].replace("const ", "")]
    for name in ("ctvae_vq_ema_stats", "ctvae_vq_ema_update", "ctvae_vq_lookup_commit"):
        params = [p for p in protos[name].split(",") if p.strip()]
        assert [kind(p) for p in params] == [ck[a] for a in native.SIGNATURES[name]], name
    assert native.SIGNATURES["ctvae_vq_lookup_commit"] == native.SIGNATURES["ctvae_vq_lookup"]      # the same ABI, another loss
    assert "ctvae_vq_ema_supported" in protos and native._RESTYPES["ctvae_vq_ema_supported"] is ctypes.c_int
    for name in ("ctvae_vq_ema_stats", "ctvae_vq_ema_update", "ctvae_vq_lookup_commit", "ctvae_vq_ema_supported"):
        assert name in native.EXPORTS
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("ctvae_vq_ema_stats", "ctvae_vq_ema_update", "ctvae_vq_lookup_commit"):
        assert name in text, name
