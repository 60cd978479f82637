"""Flat fused Adam (+ ExponentialLR) over a model's packed parameter buffer.

Same update rule as ``torch.optim.Adam(lr, weight_decay)`` with default betas/eps, which is what the
reference's harness builds (experiment.py:158-160); the schedule is ``ExponentialLR(gamma)`` stepped once
per epoch (experiment.py:173-175).  One kernel launch per step for the whole model, hyper-parameters and the
step counter live in a small device tensor so the launch is hipGraph-capturable.

Deviations from ``torch.optim.Adam`` (documented, not pinned by a fixture):
* ONE step counter for the whole buffer, and every element is updated every step.  torch keeps a step per parameter and
  skips parameters whose ``.grad`` is None.  The two differ only for parameters that receive NO gradient in some steps --
  in this repository CT-MCQ-VAE's per-action ``graph_discovers`` whose action is absent from a batch, ``ct_layer.mask`` in
  base-mode steps, the decoder in causal-mode steps: here they see a zero gradient (first moment decays, the parameter keeps
  drifting by its momentum, bias correction follows the global count), in torch they are frozen for that step.  VanillaVAE /
  MCQ-VAE (every parameter gets a gradient every step) are unaffected: tests/test_ct_gpu.py pins their 3-step trajectory.
* beta1^t / beta2^t are accumulated in fp32 on the device (state[6..7]); torch computes them in double on the host.  After
  10^4 steps the relative difference of the bias corrections is < 1e-4 (beta2^t has decayed to 4.5e-5 by then).

Gradient clipping (Lightning's ``gradient_clip_val`` / ``gradient_clip_algorithm``, which the reference's YAMLs hand to the
Trainer): ``clip_val`` None or <= 0 is off, and the step is the plain Adam launch.  Otherwise the step clips the optimizer's
slice of the gradient after the DDP scale and before the weight decay, on the device and without a host sync:
``"norm"`` = ``torch.nn.utils.clip_grad_norm_(max_norm=clip_val)`` (one extra launch, the squared-norm pass; the pre-clip
norm is left in the device tensor ``grad_norm``), ``"value"`` = ``clip_grad_value_(clip_val)`` (folded into the Adam launch).
Non-finite norms behave as in torch: NaN makes every updated element NaN, inf clips everything to zero.
"""
import math

import torch

from . import kernels as K


def clip_settings(clip_val, algorithm=None):
    """Validated ``(clip_val, algorithm)`` with Lightning 1.6.5's rules: the value is a number or None, and None or <= 0 means
    no clipping (returned as None); the algorithm is "norm" (the default) or "value", in any letter case."""
    algo = "norm" if algorithm is None else algorithm
    if not isinstance(algo, str) or algo.lower() not in K.CLIP_ALGORITHMS:
        raise ValueError(f"gradient_clip_algorithm {algorithm!r} is invalid: allowed are 'norm' and 'value'")
    if clip_val is None:
        return None, algo.lower()
    if isinstance(clip_val, bool) or not isinstance(clip_val, (int, float)) or math.isnan(clip_val):
        raise TypeError(f"gradient_clip_val must be a number, got {clip_val!r}")
    return (float(clip_val) if clip_val > 0 else None), algo.lower()


class FlatAdam:
    def __init__(self, model, lr, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8, params_slice=None, clip_val=None,
                 clip_algorithm="norm"):
        self.model = model
        flat = model.flat_params
        self.slice = params_slice if params_slice is not None else slice(0, flat.numel())
        n = flat[self.slice].numel()
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=flat.device)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=flat.device)
        self.state = K.adam_state([0.0, lr, betas[0], betas[1], eps, weight_decay, 1.0, 1.0], flat.device)
        self.lr = lr
        self.clip_val, self.clip_algorithm = clip_settings(clip_val, clip_algorithm)
        self.clip_ws = self.grad_norm = None        # grad_norm: pre-clip norm of the last step (norm mode), on the device
        if self.clip_val is not None and self.clip_algorithm == "norm":
            self.clip_ws = K.grad_clip_workspace(flat.device)
            self.grad_norm = torch.zeros((), dtype=torch.float32, device=flat.device)

    def set_lr(self, lr):
        self.lr = lr
        self.state[1:2].fill_(lr)

    def step(self, grad_scale=1.0):
        self.model.gather_torch_grads()
        if self.clip_val is None:
            K.adam_step(self.model.flat_params[self.slice], self.model.flat_grads[self.slice], self.exp_avg, self.exp_avg_sq,
                        self.state, grad_scale)
        else:
            K.adam_step_clipped(self.model.flat_params[self.slice], self.model.flat_grads[self.slice], self.exp_avg,
                                self.exp_avg_sq, self.state, grad_scale, self.clip_algorithm, self.clip_val, self.clip_ws,
                                self.grad_norm)

    def zero_grad(self, set_to_none=False):
        self.model.zero_grad()

    def state_dict(self):
        return {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "state": self.state}

    def load_state_dict(self, sd):
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.state[:8].copy_(sd["state"][:8])      # (states saved before the ticket word existed have 8 entries)


class ExponentialLR:
    """lr_epoch = lr0 * gamma**epoch (torch.optim.lr_scheduler.ExponentialLR), stepped once per epoch."""

    def __init__(self, optimizer: FlatAdam, gamma: float):
        self.opt, self.gamma, self.base_lr, self.epoch = optimizer, gamma, optimizer.lr, 0

    def step(self):
        self.epoch += 1
        self.opt.set_lr(self.base_lr * self.gamma ** self.epoch)
