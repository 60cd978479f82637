"""Helpers of the free-bits tests: the float64 restatement of csrc/klfloor.hip's contract and the input builder.

Inputs.  Even columns are collapsed (mu and log_var both 0.01 * randn clamped to +-0.05: a mean KL of at most 0.002), odd columns
are active (mu = randn, log_var = -3 + 0.1 * randn clamped to [-3.5, -2.5]: every element's KL is at least
0.5 * (e^-2.5 + 2.5 - 1) = 0.79).  A floor of 0.05 or 0.5 separates the two by a wide margin, so fp32 and float64 cannot disagree
on which columns are floored; ``reference`` asserts that no column mean lies within 10 % of the floor before anything is compared."""
import torch

# the bounds of tests/test_ops_gpu.py::test_reparam_and_loss (the project's 1e-4 parity target)
VALUE_RTOL = 1e-4            # |got - want| < 1e-4 * |want| for the KL scalars
GRAD_ATOL, GRAD_RTOL = 1e-7, 1e-4


def make_inputs(B, L):
    """(mu, log_var) fp32 [B, L] on the CPU, the same for every call with the same shape."""
    g = torch.Generator().manual_seed(1000003 * B + L)
    mu, lv = torch.empty(B, L), torch.empty(B, L)
    mu[:, 0::2] = (0.01 * torch.randn(B, (L + 1) // 2, generator=g)).clamp(-0.05, 0.05)
    lv[:, 0::2] = (0.01 * torch.randn(B, (L + 1) // 2, generator=g)).clamp(-0.05, 0.05)
    mu[:, 1::2] = torch.randn(B, L // 2, generator=g)
    lv[:, 1::2] = (-3.0 + 0.1 * torch.randn(B, L // 2, generator=g)).clamp(-3.5, -2.5)
    return mu.float(), lv.float()


def reference(mu, log_var, weight, scale, free_bits):
    """float64: dict(out=[w * sum f, sum m, sum f, floored], g_mu, g_lv, m, active) for fp32 inputs (any device)."""
    mu, lv = mu.detach().double().cpu(), log_var.detach().double().cpu()
    B = mu.size(0)
    lam = float(free_bits)
    m = (0.5 * (mu * mu + lv.exp() - lv - 1.0)).mean(dim=0)
    if lam > 0.0:
        assert bool(((m - lam).abs() > 0.1 * lam).all()), "a column mean lies within 10 % of the floor: fp32 could floor it either way"
    active = (m > lam) | ~torch.isfinite(m)
    f = torch.where(active, m, torch.full_like(m, lam))
    w = float(scale) * float(weight)
    a = active.double()
    return {"out": [w * float(f.sum()), float(m.sum()), float(f.sum()), int((~active).sum())],
            "g_mu": a * w * mu / B, "g_lv": a * w * 0.5 * (lv.exp() - 1.0) / B, "m": m, "active": active}
