"""GPU: kernels that turn network outputs into a latent sample and a scalar objective, op by op through the C ABI (and, once per
family, through the autograd classes of kernels.py), against the float64 references of tests/loss_checks.py.  The references
are pinned to oracle/vae_cpu.py, their input conditions evaluated and their bounds sized in tests/test_loss_reference_host.py.
Covered: loss.hip, the latent part of pointwise.hip, ladder.hip, tcvae.hip, vamp.hip, swd.hip, gamma.hip, dip.hip,
catlatent.hip, mmd.hip, iwloss.hip and ssim.hip.

Every output buffer starts as NaN and the workspace is filled with NaN before every call, so an element a kernel skips, or scratch
it reads without having written it, is seen.  Every call runs twice: the results must be finite and bit-identical (the kernels
promise a fixed order and no atomics).  The launch log is asserted where the dispatch is not a function of the arguments alone
(mse_partial_kernel, loss_finish_kernel, loss_bwd_kernel against mse_bwd_kernel, gauss_latent_*).  Bounds are derived in
loss_checks.py from the reference and the kernels' code alone; none was tuned on these kernels.

entry point -> cases
  ctvae_loss_forward / _logcosh_loss_forward / _l2l1_loss_forward   test_loss_forward (every LOSS_CASES row of the mode)
  ctvae_loss_forward_grad                                           test_loss_forward_grad_and_its_same_bits_promise
  ctvae_loss_backward (both modes), _mse / _logcosh / _kl_backward  test_loss_backward_launches
  ctvae_l2l1_backward, and the three above without a KL term        test_recon_backward_alone
  log-cosh saturation branches                                      test_logcosh_backward_saturated
  kernels.VAELoss, kernels.GaussKL                                  test_vaeloss_autograd_branches, test_gausskl_autograd
  ctvae_reparam_forward / _backward                                 test_reparam
  ctvae_gauss_latent_forward / _backward                            test_gauss_latent_forward, _noise_is_finite..., _backward
  ctvae_act_forward / _backward, ctvae_sigmoid_forward / _backward  test_activation, test_sigmoid
  ctvae_ladder_merge_forward / _backward, kernels.LadderMerge       test_ladder_forward, test_ladder_backward,
                                                                    test_ladder_refusals_and_autograd
  ctvae_tc_forward / _backward (<16> and <32>), kernels.TCDecomp    test_tc_forward, test_tc_backward, test_tc_refusals_and_autograd
  ctvae_vamp_kl_forward / _backward, kernels.VampKL                 test_vamp_forward_and_backward, test_vamp_refusals_and_autograd
  ctvae_swd_forward, kernels.SWD                                    test_swd, test_swd_refusals_and_autograd
  ctvae_gamma_reparam_forward / _backward                           test_gamma_reparam
  ctvae_gamma_kl_forward / _backward                                test_gamma_kl
  ctvae_dip_forward / _backward (strided rows)                      test_dip
  ctvae_gumbel_softmax_* and ctvae_cat_kl_* (<1>, <2>, <4>)         test_categorical_latent
  ctvae_mmd_forward (<1 / 2 / 4 / 8> x imq / rbf, the finish cap)   test_mmd
  ctvae_iw_loss_forward / _backward (NULL gradient outputs)         test_iw_loss
  ctvae_mssim_forward / _backward                                   test_mssim
"""
import pytest
import torch

from tests import loss_checks as V

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctvae_amd import native
    native.load()
    return native


@pytest.fixture(scope="module")
def K(N):
    from ctvae_amd import kernels
    return kernels


def dev():
    return torch.device("cuda")


def full(shape, fill=NAN, dtype=torch.float32):
    return torch.full(shape, fill, dtype=dtype, device=dev())


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def untouched(t, fill=NAN):
    return same(t, torch.full_like(t, fill))


def logged(native, fn):
    native.prof_report()
    native.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        native.prof_enable(False)
    return out, native.prof_report()


LOGGED = ("mse_partial_kernel", "loss_finish_kernel", "loss_bwd_kernel", "mse_bwd_kernel", "gauss_latent_fwd_kernel",
          "gauss_latent_bwd_kernel")


def labels(rep):
    return {k: v["count"] for k, v in rep.items() if k in LOGGED}


def twice(fn):
    """fn() -> dict of host tensors (None allowed), run twice from NaN scratch: finite where checked later, bit-identical here."""
    a, b = fn(), fn()
    for k in a:
        assert (a[k] is None and b[k] is None) or same(a[k], b[k]), f"{k}: two runs differ"
    return a


def within(what, got, want, tol):
    """|got - want| <= tol elementwise; prints the largest ratio."""
    got = got.double().reshape(want.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    err = (got - want).abs()
    tol = torch.as_tensor(tol, dtype=torch.float64)
    tol = tol.expand_as(err) if tol.shape != err.shape else tol
    ratio = float((err / tol.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: max |err| {float(err.max()) if err.numel() else 0.0:.3e}, max err/bound = {ratio:.4f}")
    assert bool((err <= tol).all()), f"{what}: {int((err > tol).sum())} of {err.numel()} elements beyond the bound, worst ratio {ratio:.3f}"
    return ratio


def fails(native, code, name, *args):
    with pytest.raises(RuntimeError, match=rf"{name} failed.*\(code {code}\)"):
        native.call(name, *args)


def nan_ws(native):
    ws = native.workspace(dev())
    ws.fill_(NAN)
    return ws


def p(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------------------------------
# loss.hip
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loss_data():
    """Inputs of a case on the host and on the device, and its float64 references: made once, shared, left unchanged."""
    cache = {}

    def make(case, far=False):
        key = (case.id, far)
        if key not in cache:
            if len(cache) >= 3:                                   # the 17 MB cases: keep a few, not all
                cache.pop(next(iter(cache)))
            inp = V.loss_inputs(case, far)
            d = dict(r=inp["r"].to(dev()), x=inp["x"].to(dev()), mu=None, lv=None, extra=None if inp["extra"] is None else inp["extra"].to(dev()))
            if inp["heads"] is not None:
                d["heads"] = inp["heads"].to(dev())
                d["mu"], d["lv"] = V.head_views(d["heads"], case)
            cache[key] = (inp, d, {g: V.loss_ref(inp, case, g) for g in V.G_LOSS})
        return cache[key]
    return make


def rs(t):
    return 0 if t is None else t.stride(0)


def run_loss_forward(native, case, d, grad=False, ws_floats=None, n=None):
    out4 = full((4,))
    ws = nan_ws(native)
    wsb = (ws.numel() if ws_floats is None else ws_floats) * 4
    n = case.n if n is None else n
    kl = (p(d["mu"]), rs(d["mu"]), p(d["lv"]), rs(d["lv"]), case.B, case.L, case.M_N)
    g = None
    if grad:
        g = (full((case.n,)), full((case.B, case.L)), full((case.B, case.L)))
        native.call("ctvae_loss_forward_grad", p(d["r"]), p(d["x"]), n, *kl, p(d["extra"]), p(out4), p(g[0]), p(g[1]), p(g[2]), case.ract,
                    p(ws), wsb)
    elif case.mode == "mse":
        native.call("ctvae_loss_forward", p(d["r"]), p(d["x"]), n, *kl, p(d["extra"]), p(out4), p(ws), wsb)
    elif case.mode == "logcosh":
        native.call("ctvae_logcosh_loss_forward", p(d["r"]), p(d["x"]), n, V.LOGCOSH_ALPHA, *kl, p(out4), p(ws), wsb)
    else:
        native.call("ctvae_l2l1_loss_forward", p(d["r"]), p(d["x"]), n, p(d["extra"]), p(out4), p(ws), wsb)
    torch.cuda.synchronize()
    res = dict(out4=out4.cpu())
    if grad:
        res.update(g_r=g[0].cpu(), g_mu=g[1].cpu(), g_lv=g[2].cpu())
    return res


@pytest.mark.parametrize("case", V.LOSS_CASES, ids=lambda c: c.id)
def test_loss_forward(N, loss_data, case):
    inp, d, refs = loss_data(case)
    ref = refs[1.0]
    bnd = V.loss_forward_bounds(inp, case, ref)
    out, rep = logged(N, lambda: twice(lambda: run_loss_forward(N, case, d)))
    assert labels(rep) == {"mse_partial_kernel": 2, "loss_finish_kernel": 2}, rep
    for i, name in enumerate(("loss", "recon", "kld", "-kld")):
        within(f"{case.id}/{name}", out["out4"][i], ref["out4"][i], bnd[i])
    assert same(out["out4"][3], -out["out4"][2])
    if case.layout == "none":
        assert float(out["out4"][2]) == 0.0 and float(out["out4"][3]) == 0.0


KL_MSE = [c for c in V.LOSS_CASES if c.mode == "mse" and c.layout != "none"]
KL_ANY = [c for c in V.LOSS_CASES if c.layout != "none"]


def run_loss_backward(native, case, d, g_loss, split):
    """One launch (ctvae_loss_backward) or the pair ctvae_mse / _logcosh_backward + ctvae_kl_backward."""
    g = torch.tensor([g_loss], dtype=torch.float32, device=dev())
    g_r, g_mu, g_lv = full((case.n,)), full((case.B, case.L)), full((case.B, case.L))
    alpha = V.alpha_of(case)
    if not split:
        native.call("ctvae_loss_backward", p(d["r"]), p(d["x"]), p(g), p(g_r), case.n, alpha, p(d["mu"]), rs(d["mu"]), p(d["lv"]), rs(d["lv"]),
                    p(g_mu), p(g_lv), case.B, case.L, case.M_N, case.ract)
    else:
        if case.mode == "logcosh":
            native.call("ctvae_logcosh_backward", p(d["r"]), p(d["x"]), p(g), p(g_r), case.n, alpha, case.ract)
        else:
            native.call("ctvae_mse_backward", p(d["r"]), p(d["x"]), p(g), p(g_r), case.n, case.ract)
        native.call("ctvae_kl_backward", p(d["mu"]), rs(d["mu"]), p(d["lv"]), rs(d["lv"]), p(g), p(g_mu), p(g_lv), case.B, case.L, case.M_N)
    torch.cuda.synchronize()
    return dict(g_r=g_r.cpu(), g_mu=g_mu.cpu(), g_lv=g_lv.cpu())


def check_grads(tag, out, ref, bnd, case):
    for k in bnd:
        within(f"{tag}/{k}", out[k], ref[k], bnd[k])
    r = out["g_r"]
    if case.mode == "l2l1":
        # recons == x: 2 d + sign(d) is exactly 0 and so is the gradient, whatever multiplies it
        zero = ref["g_r"] == 0
        assert int(zero.sum()) >= (1 if case.n >= 4 else 0)
        assert same(r[zero].abs(), torch.zeros_like(r[zero])), f"{tag}: l1 gradient at recons == x is not a zero"


@pytest.mark.parametrize("case", KL_MSE, ids=lambda c: c.id)
def test_loss_forward_grad_and_its_same_bits_promise(N, loss_data, case):
    """ctvae_loss_forward_grad: the value and the three gradients against float64; the gradients bit-identical to
    ctvae_loss_backward with g_loss = 1, as the comment above LossGradOut in loss.hip promises."""
    inp, d, refs = loss_data(case)
    ref = refs[1.0]
    out, rep = logged(N, lambda: twice(lambda: run_loss_forward(N, case, d, grad=True)))
    assert labels(rep) == {"mse_partial_kernel": 2, "loss_finish_kernel": 2}, rep
    fb = V.loss_forward_bounds(inp, case, ref)
    for i, name in enumerate(("loss", "recon", "kld", "-kld")):
        within(f"{case.id}/fwd_grad/{name}", out["out4"][i], ref["out4"][i], fb[i])
    check_grads(f"{case.id}/fwd_grad", out, ref, V.loss_grad_bounds(inp, case, 1.0), case)
    back, rep = logged(N, lambda: run_loss_backward(N, case, d, 1.0, split=False))
    assert labels(rep) == {"loss_bwd_kernel": 1}, rep
    for k in back:
        assert same(out[k], back[k]), f"{case.id}/{k}: the forward pass's gradient is not the backward launch's, bit for bit"


@pytest.mark.parametrize("g_loss", V.G_LOSS)
@pytest.mark.parametrize("case", KL_ANY, ids=lambda c: c.id)
def test_loss_backward_launches(N, loss_data, case, g_loss):
    inp, d, refs = loss_data(case)
    ref, bnd = refs[g_loss], V.loss_grad_bounds(inp, case, g_loss)
    one, rep = logged(N, lambda: twice(lambda: run_loss_backward(N, case, d, g_loss, split=False)))
    assert labels(rep) == {"loss_bwd_kernel": 2}, rep
    two, rep = logged(N, lambda: twice(lambda: run_loss_backward(N, case, d, g_loss, split=True)))
    assert labels(rep) == {"mse_bwd_kernel": 2}, rep                 # kl_bwd_kernel carries no log label
    check_grads(f"{case.id}/g{g_loss}/one launch", one, ref, bnd, case)
    check_grads(f"{case.id}/g{g_loss}/two launches", two, ref, bnd, case)
    for k in one:
        assert same(one[k], two[k]), f"{case.id}/{k}: loss_bwd_kernel and the pair of launches differ"


def run_recon_backward(native, case, d, g_loss):
    g = torch.tensor([g_loss], dtype=torch.float32, device=dev())
    g_r = full((case.n,))
    if case.mode == "logcosh":
        native.call("ctvae_logcosh_backward", p(d["r"]), p(d["x"]), p(g), p(g_r), case.n, V.LOGCOSH_ALPHA, case.ract)
    else:
        native.call("ctvae_l2l1_backward" if case.mode == "l2l1" else "ctvae_mse_backward", p(d["r"]), p(d["x"]), p(g), p(g_r), case.n, case.ract)
    torch.cuda.synchronize()
    return dict(g_r=g_r.cpu())


@pytest.mark.parametrize("g_loss", V.G_LOSS)
@pytest.mark.parametrize("case", [c for c in V.LOSS_CASES if c.layout == "none"], ids=lambda c: c.id)
def test_recon_backward_alone(N, loss_data, case, g_loss):
    inp, d, refs = loss_data(case)
    out, rep = logged(N, lambda: twice(lambda: run_recon_backward(N, case, d, g_loss)))
    assert labels(rep) == {"mse_bwd_kernel": 2}, rep
    check_grads(f"{case.id}/g{g_loss}", out, refs[g_loss], V.loss_grad_bounds(inp, case, g_loss), case)
    if g_loss > 0 and case.mode == "l2l1":
        zero = inp["r"] == inp["x"]
        assert same(out["g_r"][zero], torch.zeros_like(out["g_r"][zero]))           # (+sc) * (2 * 0 + 0) * act' = +0, bit for bit


@pytest.mark.parametrize("case", [c for c in V.LOSS_CASES if c.mode == "logcosh" and c.n in (1027, V.N_BWD_WRAP)], ids=lambda c: c.id)
def test_logcosh_backward_saturated(N, loss_data, case):
    """2 alpha d < -89: expf overflows and the kernel takes its `-alpha` branch; > +89: e underflows to 0 and the quotient is +alpha."""
    inp, d, refs = loss_data(case, far=True)
    out = twice(lambda: run_recon_backward(N, case, d, 1.0))
    check_grads(f"{case.id}/saturated", out, refs[1.0], dict(g_r=V.loss_grad_bounds(inp, case, 1.0)["g_r"]), case)


def autograd_case(mode, layout="halves", extra=False, M_N=0.00025):
    kl = mode != "l2l1"
    return V.LossCase(f"autograd-{mode}-{layout}", mode, 1027, 7 if kl else 0, 33 if kl else 0, layout if kl else "none", M_N if kl else 0.0,
                      extra, V.ACT_NONE, "through kernels.VAELoss")


# branch -> (reconstruction mode, upstream gradient, the labelled backward launches it must log)
VAELOSS_BRANCHES = {
    "root": ("mse", 1.0, {}),                                  # the forward pass's gradients are handed over: no backward kernel
    "scaled": ("mse", -0.37, {"loss_bwd_kernel": 1}),
    "recons-only": ("mse", 1.0, {"mse_bwd_kernel": 1}),
    "kl-only": ("mse", 1.0, {}),                               # kl_bwd_kernel carries no log label
    "logcosh-scaled": ("logcosh", -0.37, {"loss_bwd_kernel": 1}),
    "l2l1-scaled": ("l2l1", -0.37, {"mse_bwd_kernel": 1}),
}


@pytest.mark.parametrize("branch", list(VAELOSS_BRANCHES))
def test_vaeloss_autograd_branches(N, K, branch):
    """kernels.VAELoss once per branch of its forward / backward: the loss as the root of kernels.backward (the gradients of the
    forward pass are handed over, no backward kernel runs); a scaled upstream gradient (one launch); only recons, only mu /
    logvar requiring grad (the single kernels)."""
    mode, g_loss, want = VAELOSS_BRANCHES[branch]
    case = autograd_case(mode, extra=(mode != "logcosh"))
    inp = V.loss_inputs(case)
    ref, bnd = V.loss_ref(inp, case, g_loss), V.loss_grad_bounds(inp, case, g_loss)
    r = inp["r"].to(dev()).requires_grad_(branch != "kl-only")
    x = inp["x"].to(dev())
    heads = mu = lv = None
    if case.layout != "none":
        heads = inp["heads"].to(dev()).requires_grad_(branch != "recons-only")
        mu, lv = V.head_views(heads, case)
    extra = None if inp["extra"] is None else inp["extra"].to(dev())
    alpha = {"mse": 0.0, "logcosh": V.LOGCOSH_ALPHA, "l2l1": -1.0}[mode]
    out = K.VAELoss.apply(r, x, mu, lv, extra, case.M_N, alpha)
    fb = V.loss_forward_bounds(inp, case, ref)
    for i, name in enumerate(("loss", "recon", "kld", "-kld")):
        within(f"VAELoss/{branch}/{name}", out[i].detach().cpu(), ref["out4"][i], fb[i])
    _, rep = logged(N, (lambda: K.backward(out[0])) if branch == "root" else (lambda: (out[0] * g_loss).backward()))
    assert labels(rep) == want, rep
    if branch != "kl-only":
        within(f"VAELoss/{branch}/g_r", r.grad.cpu(), ref["g_r"], bnd["g_r"])
    else:
        assert r.grad is None
    if heads is not None and branch != "recons-only":
        L = case.L
        within(f"VAELoss/{branch}/g_mu", heads.grad.cpu()[:, :L], ref["g_mu"], bnd["g_mu"])
        within(f"VAELoss/{branch}/g_lv", heads.grad.cpu()[:, L:], ref["g_lv"], bnd["g_lv"])
    elif heads is not None:
        assert heads.grad is None


@pytest.mark.parametrize("B,L", [(1, 1), (6, 128), (7, 33)])
def test_gausskl_autograd(N, K, B, L):
    """kernels.GaussKL: the dummy four-element reconstruction, M_N = 1 -- the KL loop strided over a one-block grid."""
    case = V.LossCase(f"gausskl-{B}-{L}", "mse", 4, B, L, "halves", 1.0, False, V.ACT_NONE, "GaussKL")
    inp = V.loss_inputs(case)
    inp["r"], inp["x"] = torch.zeros(4), torch.zeros(4)
    g = -0.37
    ref, bnd = V.loss_ref(inp, case, g), V.loss_grad_bounds(inp, case, g)
    heads = inp["heads"].to(dev()).requires_grad_(True)
    kld = K.GaussKL.apply(*V.head_views(heads, case))
    within(f"GaussKL/{B}x{L}/kld", kld.detach().cpu(), ref["out4"][2], V.loss_forward_bounds(inp, case, ref)[2])
    (kld * g).backward()
    within(f"GaussKL/{B}x{L}/g_mu", heads.grad.cpu()[:, :L], ref["g_mu"], bnd["g_mu"])
    within(f"GaussKL/{B}x{L}/g_lv", heads.grad.cpu()[:, L:], ref["g_lv"], bnd["g_lv"])


def test_loss_argument_errors_launch_nothing(N, loss_data):
    case = V.case_of(V.LOSS_CASES, "mse-n1027")
    _, d, _ = loss_data(case)
    ws = N.workspace(dev())
    big = ws.numel() * 4
    out4, g_r = full((4,)), full((case.n,))
    g = torch.ones(1, device=dev())
    kl = (p(d["mu"]), rs(d["mu"]), p(d["lv"]), rs(d["lv"]), case.B, case.L, case.M_N)
    no_mu, no_lv = (None,) + kl[1:], kl[:2] + (None,) + kl[3:]
    calls = [
        (V.ERR_BAD_ARG, "ctvae_loss_forward", (p(d["r"]), p(d["x"]), 0, *kl, None, p(out4), p(ws), big)),                      # n = 0
        (V.ERR_BAD_ARG, "ctvae_loss_forward", (p(d["r"]), p(d["x"]), case.n, *no_mu, None, p(out4), p(ws), big)),
        (V.ERR_BAD_ARG, "ctvae_loss_forward", (p(d["r"]), p(d["x"]), case.n, *no_lv, None, p(out4), p(ws), big)),
        (V.ERR_BAD_ARG, "ctvae_logcosh_loss_forward", (p(d["r"]), p(d["x"]), case.n, 0.0, *kl, p(out4), p(ws), big)),           # alpha <= 0
        (V.ERR_BAD_ARG, "ctvae_logcosh_loss_forward", (p(d["r"]), p(d["x"]), case.n, -10.0, *kl, p(out4), p(ws), big)),
        (V.ERR_BAD_ARG, "ctvae_logcosh_loss_forward", (p(d["r"]), p(d["x"]), case.n, 10.0, *no_lv, p(out4), p(ws), big)),
        (V.ERR_BAD_ARG, "ctvae_logcosh_backward", (p(d["r"]), p(d["x"]), p(g), p(g_r), case.n, 0.0, 0)),
        (V.ERR_BAD_ARG, "ctvae_l2l1_loss_forward", (p(d["r"]), p(d["x"]), 0, None, p(out4), p(ws), big)),
        (V.ERR_BAD_ARG, "ctvae_mse_backward", (p(d["r"]), p(d["x"]), p(g), p(g_r), 0, 0)),
        (V.ERR_WORKSPACE, "ctvae_loss_forward", (p(d["r"]), p(d["x"]), case.n, *kl, None, p(out4), p(ws), (V.LOSS_WS_FLOATS - 1) * 4)),
        (V.ERR_WORKSPACE, "ctvae_l2l1_loss_forward", (p(d["r"]), p(d["x"]), case.n, None, p(out4), p(ws), (V.LOSS_WS_FLOATS - 1) * 4)),
    ]
    for code, name, args in calls:
        _, rep = logged(N, lambda: fails(N, code, name, *args))
        assert rep == {}, (name, sorted(rep))
        assert untouched(out4) and untouched(g_r), name
    # a workspace of exactly 2 * 1024 floats is served
    out = run_loss_forward(N, case, d, ws_floats=V.LOSS_WS_FLOATS)
    assert torch.isfinite(out["out4"]).all()


# ---------------------------------------------------------------------------------------------------------------------
# pointwise.hip: reparam, gauss_latent, act; gamma.hip: sigmoid
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("B,L", V.REPARAM_SHAPES)
def test_reparam(N, B, L, strided):
    inp = V.reparam_inputs(B, L, strided)
    ref, bnd = V.reparam_ref(inp["mu"], inp["lv"], inp["eps"], inp["g_z"])
    off = 1 if strided else 0
    muf, lvf, eps, g_z = (inp[k].to(dev()) for k in ("mu_full", "lv_full", "eps", "g_z"))
    mu, lv = muf[:, off:off + L], lvf[:, 2 * off:2 * off + L]

    def run():
        z, g_mu, g_lv = full((B, L)), full((B, L)), full((B, L))
        N.call("ctvae_reparam_forward", p(mu), mu.stride(0), p(lv), lv.stride(0), p(eps), p(z), B, L)
        N.call("ctvae_reparam_backward", p(g_z), p(lv), lv.stride(0), p(eps), p(g_mu), p(g_lv), B, L)
        torch.cuda.synchronize()
        return dict(z=z.cpu(), g_mu=g_mu.cpu(), g_lv=g_lv.cpu())
    out = twice(run)
    tag = f"reparam/{B}x{L}/{'strided' if strided else 'dense'}"
    within(f"{tag}/z", out["z"], ref["z"], bnd["z"])
    assert same(out["g_mu"], inp["g_z"])
    within(f"{tag}/g_lv", out["g_lv"], ref["g_lv"], bnd["g_lv"])


def run_latent_forward(native, case, inp, rng=None):
    B, L, S = case.B, case.L, case.S
    heads = full((B, 2 * L)) if S else inp["heads"].to(dev())
    sl = None if not S else inp["slices"].to(dev())
    bias = None if inp["bias"] is None else inp["bias"].to(dev())
    eps_in = None if rng is not None else inp["eps"].to(dev())
    eps_out, z = full((B, L)), full((B, L))
    native.call("ctvae_gauss_latent_forward", p(heads), p(eps_in), p(rng), p(eps_out), p(z), B, L, p(sl), S, p(bias))
    torch.cuda.synchronize()
    return dict(heads=heads.cpu(), eps=eps_out.cpu(), z=z.cpu())


@pytest.mark.parametrize("case", V.LATENT_CASES, ids=lambda c: c.id)
def test_gauss_latent_forward(N, case):
    inp = V.latent_inputs(case)
    out, rep = logged(N, lambda: twice(lambda: run_latent_forward(N, case, inp)))
    assert labels(rep) == {"gauss_latent_fwd_kernel": 2}, rep
    if case.S:
        h, hb = V.latent_heads_ref(inp)
        within(f"{case.id}/heads", out["heads"], h, hb)
    else:
        assert same(out["heads"], inp["heads"])
    assert same(out["eps"], inp["eps"])
    z, zb = V.latent_z_ref(out["heads"], inp["eps"])
    within(f"{case.id}/z", out["z"], z, zb)


@pytest.mark.parametrize("pos", V.RNG_POSITIONS, ids=lambda v: f"pos{v}")
def test_gauss_latent_noise_is_finite_at_the_counter_word_boundary(N, pos):
    """The stream position is split into two 32-bit counter words: every element's noise is finite on both sides of 2^32, the
    draw leaves rng alone, differs between positions, and z is built from the eps that is handed back."""
    case = V.case_of(V.LATENT_CASES, "B64-L128-S9-bias")
    inp = V.latent_inputs(case)
    rng = torch.tensor([0x5DEECE66D, pos], dtype=torch.int64, device=dev())
    out = twice(lambda: run_latent_forward(N, case, inp, rng=rng))
    assert rng.cpu().tolist() == [0x5DEECE66D, pos]
    assert torch.isfinite(out["eps"]).all() and float(out["eps"].abs().max()) < 6.0 and 0.9 < float(out["eps"].std()) < 1.1
    other = run_latent_forward(N, case, inp, rng=torch.tensor([0x5DEECE66D, pos + 1], dtype=torch.int64, device=dev()))
    assert float((other["eps"] == out["eps"]).double().mean()) < 0.01
    z, zb = V.latent_z_ref(out["heads"], out["eps"])
    within(f"noise/pos{pos}/z", out["z"], z, zb)


@pytest.mark.parametrize("with_rng", [False, True], ids=["rng-null", "rng"])
@pytest.mark.parametrize("cid,B,L,S,given", V.LATENT_BWD, ids=[c[0] for c in V.LATENT_BWD])
def test_gauss_latent_backward(N, cid, B, L, S, given, with_rng):
    inp = V.latent_bwd_inputs(cid, B, L, S, given)
    ref, bnd = V.latent_bwd_ref(inp)
    dv = {k: None if v is None else v.to(dev()) for k, v in inp.items()}
    rng = torch.tensor([77, 2 ** 32 - 1, 5, 6], dtype=torch.int64, device=dev()) if with_rng else None
    runs = []

    def run():
        gh = full((B, 2 * L))
        N.call("ctvae_gauss_latent_backward", p(dv["g_mu"]), p(dv["g_lv"]), p(dv["g_z"]), p(dv["heads"]), p(dv["eps"]), p(gh), p(rng), B, L,
               S if given[2] else 0)
        torch.cuda.synchronize()
        runs.append(1)
        return dict(g_heads=gh.cpu())
    out, rep = logged(N, lambda: twice(run))
    assert labels(rep) == {"gauss_latent_bwd_kernel": 2}, rep
    within(f"latent-bwd/{cid}", out["g_heads"], ref, bnd)
    if with_rng:
        assert rng.cpu().tolist() == [77, 2 ** 32 - 1 + len(runs), 5, 6]       # rng[1] advances by exactly 1 per launch, nothing else moves


def test_gauss_latent_argument_errors_launch_nothing(N):
    B, L = 4, 8
    heads, eps, sl = torch.zeros(B, 2 * L, device=dev()), torch.zeros(B, L, device=dev()), torch.zeros(2, B, 2 * L, device=dev())
    rng = torch.tensor([1, 2], dtype=torch.int64, device=dev())
    eo, z, gh = full((B, L)), full((B, L)), full((B, 2 * L))
    calls = [
        ("ctvae_gauss_latent_forward", (p(heads), p(eps), None, p(eo), p(z), B, 6, None, 0, None)),            # L % 4
        ("ctvae_gauss_latent_forward", (p(heads), None, None, p(eo), p(z), B, L, None, 0, None)),              # neither eps nor rng
        ("ctvae_gauss_latent_forward", (p(heads), p(eps), None, p(eo), p(z), B, L, p(sl), 0, None)),           # slices with S < 1
        ("ctvae_gauss_latent_backward", (p(eps), p(eps), p(eps), p(heads), p(eps), p(gh), p(rng), B, 6, 0)),
        ("ctvae_gauss_latent_backward", (p(eps), p(eps), None, p(heads), p(eps), p(gh), p(rng), B, L, 2)),     # slices announced, no g_z
    ]
    for name, args in calls:
        _, rep = logged(N, lambda: fails(N, V.ERR_BAD_ARG, name, *args))
        assert rep == {}, (name, sorted(rep))
        assert untouched(eo) and untouched(z) and untouched(gh) and rng.cpu().tolist() == [1, 2], name


@pytest.mark.parametrize("act", [V.ACT_NONE, V.ACT_LRELU, V.ACT_RELU, V.ACT_TANH], ids=lambda a: V.ACT_NAME[a])
@pytest.mark.parametrize("n", V.ACT_SIZES)
def test_activation(N, n, act):
    v, g = V.act_inputs(n, act)
    vd, gd = v.to(dev()), g.to(dev())

    def run():
        out, gin = full((n,)), full((n,))
        N.call("ctvae_act_forward", p(vd), p(out), n, act)
        N.call("ctvae_act_backward", p(gd), p(out), p(gin), n, act)
        torch.cuda.synchronize()
        return dict(out=out.cpu(), gin=gin.cpu())
    out = twice(run)
    ref, b = V.act_ref(v, g, act)
    tag = f"act/{V.ACT_NAME[act]}/n{n}"
    within(f"{tag}/out", out["out"], ref, b)
    zero = v == 0
    assert bool((out["out"][zero] == 0).all())
    gin, gb = V.act_bwd_ref(out["out"], g, act)                  # from the output the kernel wrote: both sides see the same numbers
    within(f"{tag}/g_in", out["gin"], gin, gb)
    if act in (V.ACT_LRELU, V.ACT_RELU):                         # the decisions at an output of exactly 0
        want = g[zero] * (V.LEAKY if act == V.ACT_LRELU else 0.0)
        within(f"{tag}/g_in at 0", out["gin"][zero], want.double(), V.EPS32 * want.double().abs())


@pytest.mark.parametrize("n", V.SIGMOID_SIZES)
def test_sigmoid(N, n):
    x, g = V.sigmoid_inputs(n)
    xd, gd = x.to(dev()), g.to(dev())

    def run():
        y, gx = full((n,)), full((n,))
        N.call("ctvae_sigmoid_forward", p(xd), p(y), n)
        N.call("ctvae_sigmoid_backward", p(gd), p(y), p(gx), n)
        torch.cuda.synchronize()
        return dict(y=y.cpu(), gx=gx.cpu())
    out = twice(run)
    ref, b = V.sigmoid_ref(x, g)
    within(f"sigmoid/n{n}/y", out["y"], ref, b)
    gx, gb = V.sigmoid_bwd_ref(out["y"], g)
    within(f"sigmoid/n{n}/g_x", out["gx"], gx, gb)
    y = full((8,))
    for bad in (5, 6, 7, 0):
        fails(N, V.ERR_BAD_ARG, "ctvae_sigmoid_forward", p(xd), p(y), bad)
        fails(N, V.ERR_BAD_ARG, "ctvae_sigmoid_backward", p(gd), p(xd), p(y), bad)
    assert untouched(y)


# ---------------------------------------------------------------------------------------------------------------------
# ladder.hip
# ---------------------------------------------------------------------------------------------------------------------
LADDER_IN = ("mu_e", "lv_e", "mu_t", "lv_t", "eps")


@pytest.fixture(scope="module")
def ladder_data():
    cache = {}

    def make(case):
        if case.id not in cache:
            inp = V.ladder_inputs(case)
            cache[case.id] = (inp, {k: v.to(dev()) for k, v in inp.items()})
        return cache[case.id]
    return make


@pytest.mark.parametrize("case", V.LADDER_CASES, ids=lambda c: c.id)
def test_ladder_forward(N, ladder_data, case):
    inp, d = ladder_data(case)
    ref, bnd = V.ladder_ref(inp), V.ladder_bounds(inp)

    def run():
        z, kl = full((case.B, case.D)), full((case.B,))
        N.call("ctvae_ladder_merge_forward", *[p(d[k]) for k in LADDER_IN], case.B, case.D, p(z), p(kl))
        torch.cuda.synchronize()
        return dict(z=z.cpu(), kl=kl.cpu())
    out = twice(run)
    within(f"ladder/{case.id}/z", out["z"], ref["z"], bnd["z"])
    within(f"ladder/{case.id}/kl", out["kl"], ref["kl"], bnd["kl"])


@pytest.mark.parametrize("grads", V.LADDER_GRADS)
@pytest.mark.parametrize("case", V.LADDER_CASES, ids=lambda c: c.id)
def test_ladder_backward(N, ladder_data, case, grads):
    inp, d = ladder_data(case)
    ref, bnd = V.ladder_ref(inp, grads), V.ladder_bounds(inp, grads)
    gz = None if grads == "no-gz" else d["g_z"]
    gkl = None if grads == "no-gkl" else d["g_kl"]

    def run():
        outs = [full((case.B, case.D)) for _ in range(4)]
        N.call("ctvae_ladder_merge_backward", p(gz), p(gkl), *[p(d[k]) for k in LADDER_IN], case.B, case.D, *[p(o) for o in outs])
        torch.cuda.synchronize()
        return dict(zip(("g_mu_e", "g_lv_e", "g_mu_t", "g_lv_t"), (o.cpu() for o in outs)))
    out = twice(run)
    for k in out:
        within(f"ladder/{case.id}/{grads}/{k}", out[k], ref[k], bnd[k])


def test_ladder_refusals_and_autograd(N, K, ladder_data):
    case = V.case_of(V.LADDER_CASES, "B9-D20")
    inp, d = ladder_data(case)
    outs = [full((case.B, case.D)) for _ in range(4)]
    fails(N, V.ERR_BAD_ARG, "ctvae_ladder_merge_backward", None, None, *[p(d[k]) for k in LADDER_IN], case.B, case.D, *[p(o) for o in outs])
    fails(N, V.ERR_BAD_ARG, "ctvae_ladder_merge_forward", *[p(d[k]) for k in LADDER_IN], 0, case.D, p(outs[0]), p(outs[1]))
    assert all(untouched(o) for o in outs)
    # kernels.LadderMerge with z unused: autograd hands g_z = None
    t = [d[k].clone().requires_grad_(True) for k in LADDER_IN[:4]]
    z, kl = K.LadderMerge.apply(*t, d["eps"])
    ref, bnd = V.ladder_ref(inp, "no-gz"), V.ladder_bounds(inp, "no-gz")
    within("LadderMerge/z", z.detach().cpu(), ref["z"], bnd["z"])
    within("LadderMerge/kl", kl.detach().cpu(), ref["kl"], bnd["kl"])
    (kl * d["g_kl"]).sum().backward()
    for k, v in zip(("g_mu_e", "g_lv_e", "g_mu_t", "g_lv_t"), t):
        within(f"LadderMerge/{k}", v.grad.cpu(), ref[k], bnd[k])


# ---------------------------------------------------------------------------------------------------------------------
# tcvae.hip
# ---------------------------------------------------------------------------------------------------------------------
TC_IN = ("z", "mu", "lv", "liw")


@pytest.fixture(scope="module")
def tc_data():
    cache = {}

    def make(case):
        if case.id not in cache:
            inp = V.tc_inputs(case)
            cache[case.id] = (inp, {k: v.to(dev()) for k, v in inp.items()}, V.tc_ref(inp))
        return cache[case.id]
    return make


@pytest.mark.parametrize("case", V.TC_CASES, ids=lambda c: c.id)
def test_tc_forward(N, tc_data, case):
    inp, d, ref = tc_data(case)
    bnd = V.tc_forward_bounds(inp)
    B, D = case.B, case.D

    def run():
        out3, lse_s, lse_d = full((3,)), full((B,)), full((B, D))
        ws = nan_ws(N)
        N.call("ctvae_tc_forward", *[p(d[k]) for k in TC_IN], B, D, p(out3), p(lse_s), p(lse_d), p(ws), ws.numel() * 4)
        torch.cuda.synchronize()
        return dict(out3=out3.cpu(), lse_s=lse_s.cpu(), lse_d=lse_d.cpu())
    out = twice(run)
    for k in ("out3", "lse_s", "lse_d"):
        within(f"tc/{case.id}/{k}", out[k], ref[k], bnd[k])


@pytest.mark.parametrize("g3", V.TC_G3, ids=lambda g: "g" + "-".join(str(v) for v in g))
@pytest.mark.parametrize("case", V.TC_CASES, ids=lambda c: c.id)
def test_tc_backward(N, tc_data, case, g3):
    """lse_s / lse_d are handed over as the float64 reference rounded to float32, so the backward check stands on its own."""
    inp, d, ref0 = tc_data(case)
    ref, bnd = V.tc_ref(inp, g3), V.tc_backward_bounds(inp, g3)
    B, D = case.B, case.D
    ls, ld, g = ref0["lse_s"].float().to(dev()), ref0["lse_d"].float().to(dev()), torch.tensor(g3, dtype=torch.float32, device=dev())

    def run():
        outs = [full((B, D)) for _ in range(3)]
        N.call("ctvae_tc_backward", *[p(d[k]) for k in TC_IN], p(ls), p(ld), p(g), B, D, *[p(o) for o in outs])
        torch.cuda.synchronize()
        return dict(zip(("g_z", "g_mu", "g_lv"), (o.cpu() for o in outs)))
    out = twice(run)
    for k in out:
        within(f"tc/{case.id}/{g3}/{k}", out[k], ref[k], bnd[k])


def test_tc_refusals_and_autograd(N, K, tc_data):
    case = V.case_of(V.TC_CASES, "B8-D17")
    inp, d, _ = tc_data(case)
    B, D = case.B, case.D
    out3, lse_s, lse_d = full((3,)), full((B,)), full((B, D))
    outs = [full((B, D)) for _ in range(3)]
    ws = N.workspace(dev())
    g = torch.ones(3, device=dev())
    for b_, d_, wsb, code in ((1, D, ws.numel() * 4, V.ERR_BAD_ARG), (V.TC_MAX_B + 1, D, ws.numel() * 4, V.ERR_BAD_ARG),
                              (B, V.TC_MAX_D + 1, ws.numel() * 4, V.ERR_BAD_ARG), (B, D, (4 * B - 1) * 4, V.ERR_WORKSPACE)):
        fails(N, code, "ctvae_tc_forward", *[p(d[k]) for k in TC_IN], b_, d_, p(out3), p(lse_s), p(lse_d), p(ws), wsb)
        if code == V.ERR_BAD_ARG:
            fails(N, code, "ctvae_tc_backward", *[p(d[k]) for k in TC_IN], p(lse_s), p(lse_d), p(g), b_, d_, *[p(o) for o in outs])
    assert untouched(out3) and untouched(lse_s) and untouched(lse_d) and all(untouched(o) for o in outs)
    # kernels.TCDecomp with the tc output unused: autograd hands None for it
    g3 = (1.5, 0.0, 0.3)
    ref, fb, bb = V.tc_ref(inp, g3), V.tc_forward_bounds(inp), V.tc_backward_bounds(inp, g3)
    t = [d[k].clone().requires_grad_(True) for k in TC_IN[:3]]
    mi, tc, kld = K.TCDecomp.apply(*t, d["liw"])
    within("TCDecomp/out3", torch.stack([mi, tc, kld]).detach().cpu(), ref["out3"], fb["out3"])
    (mi * g3[0] + kld * g3[2]).backward()
    # the kernel's own lse outputs take the place of the rounded reference: their forward bounds enter the softmax weights
    bb = V.tc_backward_bounds(inp, g3, lse_err=(fb["lse_s"], fb["lse_d"]))
    for k, v in zip(("g_z", "g_mu", "g_lv"), t):
        within(f"TCDecomp/{k}", v.grad.cpu(), ref[k], bb[k])


# ---------------------------------------------------------------------------------------------------------------------
# vamp.hip
# ---------------------------------------------------------------------------------------------------------------------
VAMP_IN = ("z", "mu", "lv", "pmu", "plv")


@pytest.mark.parametrize("case", V.VAMP_CASES, ids=lambda c: c.id)
def test_vamp_forward_and_backward(N, case):
    """Forward: out3 and the softmax weights.  Backward from the reference weights rounded to float32 (so it stands on its own):
    all five gradients."""
    inp = V.vamp_inputs(case)
    g = -0.37
    ref, bnd = V.vamp_ref(inp, g), V.vamp_bounds(inp, g)
    d = {k: v.to(dev()) for k, v in inp.items()}
    B, D, Kc = case.B, case.D, case.K
    wref, gd = ref["w"].float().to(dev()), torch.tensor([g], dtype=torch.float32, device=dev())

    def run():
        out3, w = full((3,)), full((B, Kc))
        outs = [full((B, D)) for _ in range(3)] + [full((Kc, D)) for _ in range(2)]
        ws = nan_ws(N)
        N.call("ctvae_vamp_kl_forward", *[p(d[k]) for k in VAMP_IN], B, D, Kc, p(out3), p(w), p(ws), ws.numel() * 4)
        N.call("ctvae_vamp_kl_backward", *[p(d[k]) for k in VAMP_IN], p(wref), p(gd), B, D, Kc, *[p(o) for o in outs])
        torch.cuda.synchronize()
        return dict(out3=out3.cpu(), w=w.cpu(), **{"g_" + k: o.cpu() for k, o in zip(VAMP_IN, outs)})
    out = twice(run)
    for k in out:
        within(f"vamp/{case.id}/{k}", out[k], ref[k], bnd[k])


def test_vamp_refusals_and_autograd(N, K):
    case = V.case_of(V.VAMP_CASES, "K5-D65-B7")
    inp = V.vamp_inputs(case)
    d = {k: v.to(dev()) for k, v in inp.items()}
    B, D, Kc = case.B, case.D, case.K
    out3, w = full((3,)), full((B, Kc))
    ws = N.workspace(dev())
    fails(N, V.ERR_BAD_ARG, "ctvae_vamp_kl_forward", *[p(d[k]) for k in VAMP_IN], B, D, V.VAMP_MAX_K + 1, p(out3), p(w), p(ws), ws.numel() * 4)
    fails(N, V.ERR_WORKSPACE, "ctvae_vamp_kl_forward", *[p(d[k]) for k in VAMP_IN], B, D, Kc, p(out3), p(w), p(ws), (2 * B - 1) * 4)
    assert untouched(out3) and untouched(w)
    g = -0.37
    ref, bnd = V.vamp_ref(inp, g), V.vamp_bounds(inp, g)
    t = [d[k].clone().requires_grad_(True) for k in VAMP_IN]
    kld = K.VampKL.apply(*t)
    kld = kld[0] if isinstance(kld, (tuple, list)) else kld
    within("VampKL/kld", kld.detach().cpu().reshape(()), ref["out3"][0], bnd["out3"][0])
    (kld * g).backward()
    # the kernel's own weights take the place of the rounded reference: their forward bound rides on every term that carries one
    bnd = V.vamp_bounds(inp, g, own_weights=True)
    for k, v in zip(VAMP_IN, t):
        within(f"VampKL/g_{k}", v.grad.cpu(), ref["g_" + k], bnd["g_" + k])


# ---------------------------------------------------------------------------------------------------------------------
# swd.hip
# ---------------------------------------------------------------------------------------------------------------------
def run_swd(native, d, N, D, S, p_, ws_floats=None):
    out, grad = full((1,)), full((N, D))
    ws = nan_ws(native)
    native.call("ctvae_swd_forward", p(d["z"]), p(d["prior"]), p(d["proj"]), N, D, S, p_, V.SWD_WEIGHT, p(out), p(grad), p(ws),
                (ws.numel() if ws_floats is None else ws_floats) * 4)
    torch.cuda.synchronize()
    return dict(out=out.cpu(), g_z=grad.cpu())


@pytest.mark.parametrize("case", V.SWD_CASES, ids=lambda c: c.id)
def test_swd(N, case):
    """Exact cases (projections exact in float32, no ties): value and gradient element by element.  Normal draws: the value
    against float64 within the bound, the gradient in the L2 sense as tests/test_models_gpu.py compares it -- rank swaps between
    projections that agree to rounding cannot be told from errors."""
    inp = V.swd_inputs(case)
    ref = V.swd_ref(inp, case)
    bnd = V.swd_bounds(inp, case, ref)
    d = {k: v.to(dev()) for k, v in inp.items()}
    out = twice(lambda: run_swd(N, d, case.N, case.D, case.S, case.p))
    within(f"swd/{case.id}/out", out["out"], ref["out"].reshape(1), bnd["out"].reshape(1))
    if case.exact:
        within(f"swd/{case.id}/g_z", out["g_z"], ref["g_z"], bnd["g_z"])
    else:
        assert torch.isfinite(out["g_z"]).all()
        rel = float((out["g_z"].double() - ref["g_z"]).norm() / ref["g_z"].norm())
        print(f"swd/{case.id}/g_z: relative L2 error {rel:.3e}")
        assert rel <= 2e-3


def test_swd_refusals_and_autograd(N, K):
    case = V.case_of(V.SWD_CASES, "exact-N37")
    inp = V.swd_inputs(case)
    d = {k: v.to(dev()) for k, v in inp.items()}
    out, grad = full((1,)), full((case.N, case.D))
    ws = N.workspace(dev())
    big = ws.numel() * 4
    for n_, d_, wsb, code in ((V.SWD_MAX_N + 1, 8, big, V.ERR_BAD_ARG), (case.N, 2, big, V.ERR_BAD_ARG), (case.N, 6, big, V.ERR_BAD_ARG),
                              (case.N, 516, big, V.ERR_BAD_ARG), (case.N, 8, (case.S + case.N * case.S - 1) * 4, V.ERR_WORKSPACE)):
        fails(N, code, "ctvae_swd_forward", p(d["z"]), p(d["prior"]), p(d["proj"]), n_, d_, case.S, 2.0, V.SWD_WEIGHT, p(out), p(grad), p(ws), wsb)
    assert untouched(out) and untouched(grad)
    ref = V.swd_ref(inp, case)
    bnd = V.swd_bounds(inp, case, ref)
    z = d["z"].clone().requires_grad_(True)
    got = K.SWD.apply(z, d["prior"], d["proj"], case.p, V.SWD_WEIGHT)
    within("SWD/out", got.detach().cpu().reshape(1), ref["out"].reshape(1), bnd["out"].reshape(1))
    (got * -0.37).backward()
    g = float(torch.tensor(-0.37, dtype=torch.float32))
    within("SWD/g_z", z.grad.cpu(), ref["g_z"] * g, bnd["g_z"] * abs(g) + V.EPS32 * (ref["g_z"] * g).abs())


# ---------------------------------------------------------------------------------------------------------------------
# gamma.hip: the reparameterisation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape_b", V.GAMMA_SHAPES)
@pytest.mark.parametrize("n", V.GAMMA_SIZES)
def test_gamma_reparam(N, n, shape_b):
    """z, d z / d beta, and the alpha gradient: a cancellation whose bound is made of the magnitudes of its two partials."""
    inp = V.gamma_inputs(n, shape_b)
    ref, bnd = V.gamma_reparam_ref(inp, shape_b), V.gamma_reparam_bounds(inp, shape_b)
    d = {k: v.to(dev()) for k, v in inp.items()}

    def run():
        z, ga, gb = full((n,)), full((n,)), full((n,))
        N.call("ctvae_gamma_reparam_forward", p(d["alpha"]), p(d["beta"]), p(d["zhat"]), shape_b, p(z), n)
        N.call("ctvae_gamma_reparam_backward", p(d["g"]), p(d["alpha"]), p(d["beta"]), p(d["zhat"]), shape_b, p(ga), p(gb), n)
        torch.cuda.synchronize()
        return dict(z=z.cpu(), g_alpha=ga.cpu(), g_beta=gb.cpu())
    out = twice(run)
    for k in out:
        within(f"gamma/n{n}/Bs{shape_b}/{k}", out[k], ref[k], bnd[k])
    if n == 1:
        z = full((1,))
        fails(N, V.ERR_BAD_ARG, "ctvae_gamma_reparam_forward", p(d["alpha"]), p(d["beta"]), p(d["zhat"]), shape_b, p(z), 0)
        fails(N, V.ERR_BAD_ARG, "ctvae_gamma_reparam_forward", p(d["alpha"]), None, p(d["zhat"]), shape_b, p(z), 1)
        assert untouched(z)


@pytest.mark.parametrize("prior", V.GAMMA_PRIORS, ids=lambda p: f"prior{p[0]}-{p[1]}")
@pytest.mark.parametrize("B,D", V.GAMMA_KL_SHAPES)
def test_gamma_kl(N, B, D, prior):
    """ctvae_gamma_kl_forward / _backward against torch.special.digamma / lgamma in float64."""
    inp = V.gamma_kl_inputs(B, D, prior)
    g = -0.37
    ref, bnd = V.gamma_kl_ref(inp, prior, g), V.gamma_kl_bounds(inp, prior, g)
    d = {k: v.to(dev()) for k, v in inp.items()}
    gd = torch.tensor([g], dtype=torch.float32, device=dev())

    def run():
        out, ga, gb = full((1,)), full((B, D)), full((B, D))
        ws = nan_ws(N)
        N.call("ctvae_gamma_kl_forward", p(d["alpha"]), p(d["beta"]), B, D, prior[0], prior[1], p(out), p(ws), ws.numel() * 4)
        N.call("ctvae_gamma_kl_backward", p(gd), p(d["alpha"]), p(d["beta"]), B, D, prior[0], prior[1], p(ga), p(gb))
        torch.cuda.synchronize()
        return dict(out=out.cpu(), g_alpha=ga.cpu(), g_beta=gb.cpu())
    out = twice(run)
    within(f"gamma-kl/{B}x{D}/{prior}/out", out["out"], ref["out"].reshape(1), bnd["out"].reshape(1))
    within(f"gamma-kl/{B}x{D}/{prior}/g_alpha", out["g_alpha"], ref["g_alpha"], bnd["g_alpha"])
    within(f"gamma-kl/{B}x{D}/{prior}/g_beta", out["g_beta"], ref["g_beta"], bnd["g_beta"])
    if (B, D) == (1, 1):
        o = full((1,))
        ws = N.workspace(dev())
        fails(N, V.ERR_BAD_ARG, "ctvae_gamma_kl_forward", p(d["alpha"]), p(d["beta"]), B, D, 0.0, prior[1], p(o), p(ws), ws.numel() * 4)
        fails(N, V.ERR_BAD_ARG, "ctvae_gamma_kl_forward", p(d["alpha"]), p(d["beta"]), 0, D, prior[0], prior[1], p(o), p(ws), ws.numel() * 4)
        fails(N, V.ERR_WORKSPACE, "ctvae_gamma_kl_forward", p(d["alpha"]), p(d["beta"]), B, D, prior[0], prior[1], p(o), p(ws), 0)
        assert untouched(o)


# ---------------------------------------------------------------------------------------------------------------------
# dip.hip
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,D", V.DIP_SHAPES)
def test_dip(N, B, D):
    """ctvae_dip_forward / _backward with strided rows; the state buffer (c, G, e, partials, out) starts as NaN."""
    inp = V.dip_inputs(B, D)
    g = -0.37
    ref, bnd = V.dip_ref(inp, g), V.dip_bounds(inp, g)
    muf, lvf = inp["mu_full"].to(dev()), inp["lv_full"].to(dev())
    mu, lv = muf[:, 1:1 + D], lvf[:, 2:2 + D]
    gd = torch.tensor([g], dtype=torch.float32, device=dev())
    nstate = int(N.load().ctvae_dip_state_floats(B, D))
    assert nstate == B * D + D * D + 3 * D + 2

    def run():
        state, gm, gl = full((nstate + 8,)), full((B, D)), full((B, D))
        N.call("ctvae_dip_forward", p(mu), mu.stride(0), p(lv), lv.stride(0), B, D, *V.DIP_LAMBDAS, p(state))
        N.call("ctvae_dip_backward", p(state), p(gd), p(gm), p(gl), B, D)
        torch.cuda.synchronize()
        assert untouched(state[nstate:])                          # nothing behind the state is written
        return dict(out=state[nstate - 2:nstate - 1].cpu(), g_mu=gm.cpu(), g_lv=gl.cpu())
    out = twice(run)
    within(f"dip/{B}x{D}/out", out["out"], ref["out"].reshape(1), bnd["out"].reshape(1))
    within(f"dip/{B}x{D}/g_mu", out["g_mu"], ref["g_mu"], bnd["g_mu"])
    within(f"dip/{B}x{D}/g_lv", out["g_lv"], ref["g_lv"], bnd["g_lv"])
    off = bnd["g_lv"] == 0
    assert bool((out["g_lv"][off] == 0).all())
    if D == 1024:
        gm = full((B, D))
        fails(N, V.ERR_BAD_ARG, "ctvae_dip_forward", p(mu), mu.stride(0), p(lv), lv.stride(0), B, V.DIP_MAX_D + 1, *V.DIP_LAMBDAS, p(gm))
        fails(N, V.ERR_BAD_ARG, "ctvae_dip_backward", p(gm), p(gd), p(gm), p(gm), B, V.DIP_MAX_D + 1)
        assert untouched(gm)


# ---------------------------------------------------------------------------------------------------------------------
# catlatent.hip
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", V.CAT_CASES, ids=lambda c: c.id)
def test_categorical_latent(N, case):
    """Gumbel-softmax forward / backward and the categorical KL forward / backward at 1, 2 and 4 categories per lane.  The
    Gumbel backward is checked from the sample the forward kernel wrote: both sides see the same numbers."""
    inp = V.cat_inputs(case)
    rows, Q = case.rows, case.Q
    B = V.cat_batch(rows)
    g = -0.37
    d = {k: v.to(dev()) for k, v in inp.items()}
    gd = torch.tensor([g], dtype=torch.float32, device=dev())
    c = V.cat_log_prior(Q)

    def run():
        s, gz, kld, gq = full((rows, Q)), full((rows, Q)), full((1,)), full((rows, Q))
        ws = nan_ws(N)
        N.call("ctvae_gumbel_softmax_forward", p(d["z"]), p(d["u"]), p(s), rows, Q, V.CAT_TEMP, V.CAT_EPS)
        N.call("ctvae_gumbel_softmax_backward", p(d["gs"]), p(s), p(gz), rows, Q, V.CAT_TEMP)
        N.call("ctvae_cat_kl_forward", p(d["z"]), rows, Q, B, V.CAT_EPS, c, p(kld), p(ws), ws.numel() * 4)
        N.call("ctvae_cat_kl_backward", p(d["z"]), p(gd), p(gq), rows, Q, B, V.CAT_EPS, c)
        torch.cuda.synchronize()
        return dict(s=s.cpu(), g_z=gz.cpu(), kld=kld.cpu(), g_q=gq.cpu())
    out = twice(run)
    s, bs = V.gumbel_ref(inp, case)
    within(f"cat/{case.id}/s", out["s"], s, bs)
    gz, bg = V.gumbel_bwd_ref(out["s"], inp["gs"], case)
    within(f"cat/{case.id}/g_z", out["g_z"], gz, bg)
    ref, bnd = V.cat_kl_ref(inp, case, g), V.cat_kl_bounds(inp, case, g)
    within(f"cat/{case.id}/kld", out["kld"], ref["out"].reshape(1), bnd["out"].reshape(1))
    within(f"cat/{case.id}/g_q", out["g_q"], ref["g_q"], bnd["g_q"])
    if Q == V.CAT_MAX_Q:
        o = full((rows, Q))
        ws = N.workspace(dev())
        fails(N, V.ERR_BAD_ARG, "ctvae_gumbel_softmax_forward", p(d["z"]), p(d["u"]), p(o), 7, Q + 1, V.CAT_TEMP, V.CAT_EPS)
        fails(N, V.ERR_BAD_ARG, "ctvae_gumbel_softmax_backward", p(d["gs"]), p(d["z"]), p(o), 7, Q + 1, V.CAT_TEMP)
        fails(N, V.ERR_BAD_ARG, "ctvae_cat_kl_forward", p(d["z"]), 7, Q + 1, 1, V.CAT_EPS, c, p(o), p(ws), ws.numel() * 4)
        fails(N, V.ERR_BAD_ARG, "ctvae_cat_kl_backward", p(d["z"]), p(gd), p(o), 7, Q + 1, 1, V.CAT_EPS, c)
        fails(N, V.ERR_WORKSPACE, "ctvae_cat_kl_forward", p(d["z"]), rows, Q, B, V.CAT_EPS, c, p(o), p(ws), 1023 * 4)
        assert untouched(o)


# ---------------------------------------------------------------------------------------------------------------------
# mmd.hip, iwloss.hip
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", V.MMD_CASES, ids=lambda c: c.id)
def test_mmd(N, case):
    """mmd_rows_kernel<1 / 2 / 4 / 8, imq / rbf> and the finish: the four scalars and d mmd / d z."""
    inp = V.mmd_inputs(case)
    ref, bnd = V.mmd_ref(inp, case), V.mmd_bounds(inp, case)
    d = {k: v.to(dev()) for k, v in inp.items()}
    kind = 0 if case.kind == "imq" else 1

    def run(n_=case.N, d_=case.D, wsb=None, k_=kind):
        out4, grad = full((4,)), full((case.N, case.D))
        ws = nan_ws(N)
        N.call("ctvae_mmd_forward", p(d["z"]), p(d["prior"]), n_, d_, k_, V.mmd_c(case.D), V.MMD_EPS, *V.MMD_W, p(out4), p(grad), p(ws),
               ws.numel() * 4 if wsb is None else wsb)
        torch.cuda.synchronize()
        return dict(out4=out4.cpu(), g_z=grad.cpu())
    out = twice(run)
    within(f"mmd/{case.id}/out4", out["out4"], ref["out4"], bnd["out4"])
    within(f"mmd/{case.id}/g_z", out["g_z"], ref["g_z"], bnd["g_z"])
    if case.D == V.MMD_MAX_D and case.N == 5:
        for kw, code in ((dict(d_=V.MMD_MAX_D + 1), V.ERR_BAD_ARG), (dict(k_=2), V.ERR_BAD_ARG), (dict(n_=0), V.ERR_BAD_ARG),
                         (dict(wsb=(3 * case.N - 1) * 4), V.ERR_WORKSPACE)):
            with pytest.raises(RuntimeError, match=rf"ctvae_mmd_forward failed.*\(code {code}\)"):
                run(**kw)


IW_IN = ("recons", "x", "mu", "lv")


@pytest.mark.parametrize("nulls", ["none", "no-g_recons", "no-g_mu-g_lv"])
@pytest.mark.parametrize("case", V.IW_CASES, ids=lambda c: c.id)
def test_iw_loss(N, case, nulls):
    """ctvae_iw_loss_forward (lp, kld, coef, out4) and ctvae_iw_loss_backward from the coef the forward launch wrote."""
    inp = V.iw_inputs(case)
    B, S, n, L = case.B, case.S, case.n, case.L
    R = B * S
    g = -0.37
    ref, bnd = V.iw_ref(inp, g), V.iw_bounds(inp, g)
    d = {k: v.to(dev()) for k, v in inp.items()}
    gd = torch.tensor([g], dtype=torch.float32, device=dev())

    def run():
        lp, kld, coef, out4 = full((B, S)), full((B, S)), full((B, S)), full((4,))
        gr = None if nulls == "no-g_recons" else full((B, S, n))
        gm, gl = (None, None) if nulls == "no-g_mu-g_lv" else (full((B, S, L)), full((B, S, L)))
        rx, ml = [p(d[k]) for k in IW_IN[:2]], [p(d["mu"]), p(d["lv"])]
        N.call("ctvae_iw_loss_forward", *rx, n, R, S, *ml, L, S, V.IW_M_N, p(lp), p(kld), p(coef), p(out4))
        N.call("ctvae_iw_loss_backward", *rx, n, R, S, *ml, L, V.IW_M_N, p(coef), p(gd), p(gr), p(gm), p(gl))
        torch.cuda.synchronize()
        c = lambda t: None if t is None else t.cpu()              # noqa: E731
        return dict(lp=lp.cpu(), kld=kld.cpu(), coef=coef.cpu(), out4=out4.cpu(), g_recons=c(gr), g_mu=c(gm), g_lv=c(gl))
    out = twice(run)
    for k in out:
        if out[k] is not None:
            within(f"iw/{case.id}/{nulls}/{k}", out[k], ref[k], bnd[k])
    assert same(out["out4"][3], -out["out4"][2])
    if nulls == "none" and case.S == 2:
        o = full((B, S, n))
        rx, ml = [p(d[k]) for k in IW_IN[:2]], [p(d["mu"]), p(d["lv"])]
        args = lambda n_, r_, s_: (*rx, n_, r_, s_, *ml, L, s_, V.IW_M_N, p(o), p(o), p(o), p(o))   # noqa: E731
        fails(N, V.ERR_BAD_ARG, "ctvae_iw_loss_forward", *args(n - 2, R, S))           # n % 4
        fails(N, V.ERR_BAD_ARG, "ctvae_iw_loss_forward", *args(n, R - 1, S))           # R % S
        fails(N, V.ERR_BAD_ARG, "ctvae_iw_loss_backward", *[p(d[k]) for k in IW_IN[:2]], n, R, S, p(d["mu"]), p(d["lv"]), L, V.IW_M_N, p(o),
              p(gd), p(o), p(o), None)                                                 # one of g_mu / g_logvar alone
        assert untouched(o)


# ---------------------------------------------------------------------------------------------------------------------
# ssim.hip
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", V.SSIM_G)
@pytest.mark.parametrize("case", V.SSIM_CASES, ids=lambda c: c.id)
def test_mssim(N, case, g):
    """ctvae_mssim_forward (loss and the ten level coefficients) and ctvae_mssim_backward from the reference's coefficients rounded
    to float32, so the backward check stands on its own.  Pictures are NHWC on the device."""
    import ctypes
    inp = V.ssim_inputs(case)
    ref, bnd = V.ssim_ref(inp, g), V.ssim_bounds(inp, g)
    B, C, S = case.B, case.C, V.SSIM_SIDE
    a, b = (inp[k].permute(0, 2, 3, 1).contiguous().to(dev()) for k in ("a", "b"))
    win = (ctypes.c_float * 11)(*V.ssim_window().tolist())
    wts = (ctypes.c_float * 5)(*V.SSIM_WEIGHTS)
    npart = int(N.load().ctvae_mssim_part_floats(B, C))
    cref, gd = ref["coef"].float().to(dev()), torch.tensor([g], dtype=torch.float32, device=dev())

    def run():
        part, out, ga = full((npart,)), full((11,)), full((B, S, S, C))
        N.call("ctvae_mssim_forward", p(a), p(b), win, wts, p(part), p(out), out.data_ptr() + 4, B, C, S, S)
        N.call("ctvae_mssim_backward", p(a), p(b), win, p(cref), p(gd), p(ga), B, C, S, S)
        torch.cuda.synchronize()
        return dict(loss=out[:1].cpu(), coef=out[1:].cpu(), g_a=ga.cpu().permute(0, 3, 1, 2))
    out = twice(run)
    within(f"ssim/{case.id}/g{g}/loss", out["loss"], ref["loss"].reshape(1), bnd["loss"].reshape(1))
    within(f"ssim/{case.id}/g{g}/coef", out["coef"], ref["coef"], bnd["coef"])
    within(f"ssim/{case.id}/g{g}/g_a", out["g_a"], ref["g_a"], bnd["g_a"])
    if case.id == "B1-C1" and g == 1.0:
        o = full((11,))
        fails(N, V.ERR_BAD_ARG, "ctvae_mssim_forward", p(a), p(b), win, wts, p(o), p(o), o.data_ptr() + 4, B, C, 32, 32)
        fails(N, V.ERR_BAD_ARG, "ctvae_mssim_backward", p(a), p(b), win, p(cref), p(gd), p(o), B, C, 32, 32)
        assert untouched(o)
