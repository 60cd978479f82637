"""GPU: the channel-owner BatchNorm launches at the channel counts whose workgroups bnowner.hpp deals out in sector runs
(C = 32, 64, 128: two channels per workgroup, grids of 16 / 32 / 64), one shape per thread-count class of the kernels:
R = 12 (64 threads, odd batch, lanes beyond R), R = 512 (256 threads) and R = 4096 (1024 threads, the flagship step's shape).

Each case is one layer's round trip through the C ABI: ctvae_conv_bn_act_forward (split-K conv + bn_fused_fwd_kernel), then
ctvae_bn_backward_fused (bn_fused_bwd_kernel) on the y, mean and invstd that forward call wrote.  Both are compared with the
float64 references of tests/bn_checks.py under its bounds, with the call helpers of tests/test_bn_ops_gpu.py (NaN-filled outputs
and workspace, every call twice and bit-identical, the launch log says which BatchNorm kernel ran).  A placement that skipped or
doubled a channel group would leave NaN in, or PREFILL under, the channels nobody owned.
"""
import pytest

from tests import bn_checks as V
from tests import test_bn_ops_gpu as T
from tests.test_bn_ops_gpu import K, N, conv_inputs  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

# (B, input size) of the stride-2 3x3 conv whose output [B][H/2][H/2][C] the BatchNorm normalises
ROWS = {12: (3, 4), 512: (8, 16), 4096: (16, 32)}
ACTS = {32: V.ACT_LRELU, 64: V.ACT_TANH, 128: V.ACT_RELU}
SLICES = {12: 9, 512: 3, 4096: 5}          # of the backward call: beyond the unroll of eight / below it / odd against four in flight
CASES = [(C, R) for C in (32, 64, 128) for R in (12, 512, 4096)]


@pytest.mark.parametrize("C,R", CASES, ids=lambda v: str(v))
def test_forward_then_backward_against_float64(N, K, conv_inputs, C, R):  # noqa: F811
    B, H = ROWS[R]
    fwd = V.Conv(f"owner-conv-s2-R{R}-C{C}", False, B, H, 32, C, 3, 2, 1, 0, ACTS[C], R == 512, "bn_fused_fwd_kernel")
    assert V.fused_ok(R, C) and B * (H // 2) ** 2 == R
    inputs = conv_inputs(fwd)
    assert K.bn_apply_is_separate(T.conv_spec_of(K, fwd), B, H, H) is False
    out, rep = T.logged(N, lambda: T.twice(lambda: T.run_conv_bn(K, N, fwd, *inputs[:7])))
    assert T.bn_labels(rep) == ["bn_fused_fwd_kernel"] and rep["bn_fused_fwd_kernel"]["count"] == 2, sorted(rep)
    T.check_conv_bn(fwd, out, inputs, V.FUSED_CHAIN)
    assert int(out["nbt"]) == T.NBT0 + 1

    bwd = V.Fused(f"owner-bwd-R{R}-C{C}", B, H // 2, H // 2, C, SLICES[R], 2, ACTS[C], "conv")
    y, mean, invstd = out["y"], out["mean"], out["invstd"]
    gamma, beta = inputs[3], inputs[4]
    slices, ga, abs_sum = V.split_slices(bwd.id, V.make_ga(bwd.id, R, C), bwd.S, V.fused_pix(bwd))
    ref = V.backward_ref(ga, y, gamma, beta, mean, invstd, bwd.act)
    bnd = V.backward_bounds(ga, y, gamma, beta, mean, invstd, ref, V.FUSED_CHAIN, bwd.act, ga_err=V.dot_bound(bwd.S, abs_sum))
    assert float(bnd["exclude"].double().mean()) <= V.EXCLUDE_CAP and float(max(bnd["dgamma"].max(), bnd["dbeta"].max())) < T.PREFILL / 2
    for accumulate in (0, 1):
        got, rep = T.logged(N, lambda: T.twice(lambda: T.run_fused_backward(N, bwd, slices, y, gamma, beta, mean, invstd, accumulate)))
        assert T.bn_labels(rep) == ["bn_fused_bwd_kernel"] and rep["bn_fused_bwd_kernel"]["count"] == 2, rep
        base = T.PREFILL if accumulate else 0.0
        acc_round = V.EPS32 * T.PREFILL if accumulate else 0.0
        tag = f"{bwd.id}/acc{accumulate} {V.fused_instance(R, C)}"
        T.within(f"{tag}/dgamma", got["dgamma"], ref["dgamma"] + base, bnd["dgamma"] + acc_round)
        T.within(f"{tag}/dbeta", got["dbeta"], ref["dbeta"] + base, bnd["dbeta"] + acc_round)
        T.within(f"{tag}/g_y", got["gy"], ref["gy"], bnd["gy"], skip=bnd["exclude"])
