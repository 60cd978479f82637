"""KL weight schedules and free bits for the Gaussian models: what a run does about posterior collapse once ``latent_stats`` shows it.

* ``exp_params.kld_schedule`` -- KL annealing.  ``s`` is ``global_step`` (optimizer steps; every micro-batch of an
  ``accumulate_grad_batches`` window uses the same weight):

  - ``{type: linear, warmup_steps: N, start: a}`` (N >= 1 an int, 0 <= a <= 1, default 0; Bowman et al. 2016):
    ``w(s) = kld_weight * (a + (1 - a) * min(1, s / N))``
  - ``{type: cyclical, cycle_steps: M, ratio: r, cycles: n}`` (M >= 2 an int, 0 < r <= 1, default 0.5, n >= 1 an int or absent: for
    ever; Fu et al. 2019): ``tau = (s mod M) / M``, ``w(s) = kld_weight * min(1, tau / r)``, and ``w = kld_weight`` for ``s >= n * M``

  computed in Python float64 and rounded to fp32 once (``weight``).
* ``exp_params.kld_free_bits: lambda`` -- free bits (Kingma et al. 2016, eq. 15), a float >= 0 in nats per latent dimension: the KL
  term becomes ``sum_d max(lambda, mean_b KL_bd)`` and a dimension under the floor gets no KL gradient (``kernels.FreeBitsKL``,
  csrc/klfloor.hip).  0.0 is allowed: the same path with no floor.

Both work alone or together, on the models whose training loss is ``recon + c * M_N * KL(N(mu, sigma) || N(0, 1))`` with a host
constant ``c`` (``SERVED_MODELS``; BetaVAE with ``loss_type: 'H'`` only).  ``KLControl`` holds the validated settings and the one
persistent 1-element device tensor the loss launch reads its weight from: its address is fixed, so a captured step reads the
value of the replay -- a by-value ``M_N`` would be frozen at capture.  Validation (``M_N = 1.0``) never sees any of this.
"""
import ctypes

import torch

SERVED_MODELS = ("VanillaVAE", "TwoStageVAE", "ConditionalVAE", "MSSIMVAE", "LogCoshVAE", "BetaVAE")
_LINEAR = {"type", "warmup_steps", "start"}
_CYCLICAL = {"type", "cycle_steps", "ratio", "cycles"}


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _is_number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def kld_schedule_setting(value):
    """Validated ``exp_params.kld_schedule`` with its defaults filled in (absent: None); anything else is a ValueError that names
    the key."""
    if value is None:
        return None
    if not isinstance(value, dict):
        raise ValueError(f"kld_schedule must be a mapping with a 'type' of 'linear' or 'cyclical', got {value!r}")
    kind = value.get("type")
    if kind not in ("linear", "cyclical") or not isinstance(kind, str):
        raise ValueError(f"kld_schedule.type must be 'linear' or 'cyclical', got {kind!r}")
    allowed = _LINEAR if kind == "linear" else _CYCLICAL
    extra = sorted(set(value) - allowed, key=str)
    if extra:
        raise ValueError(f"kld_schedule of type {kind!r} has no field {extra[0]!r} (its fields: {', '.join(sorted(allowed))})")
    if kind == "linear":
        if "warmup_steps" not in value:
            raise ValueError("kld_schedule of type 'linear' needs warmup_steps (an integer >= 1)")
        n, a = value["warmup_steps"], value.get("start", 0.0)
        if not _is_int(n) or n < 1:
            raise ValueError(f"kld_schedule.warmup_steps must be an integer >= 1, got {n!r}")
        if not _is_number(a) or not 0.0 <= a <= 1.0:
            raise ValueError(f"kld_schedule.start must be a number in [0, 1], got {a!r}")
        return {"type": "linear", "warmup_steps": int(n), "start": float(a)}
    if "cycle_steps" not in value:
        raise ValueError("kld_schedule of type 'cyclical' needs cycle_steps (an integer >= 2)")
    m, r = value["cycle_steps"], value.get("ratio", 0.5)
    if not _is_int(m) or m < 2:
        raise ValueError(f"kld_schedule.cycle_steps must be an integer >= 2, got {m!r}")
    if not _is_number(r) or not 0.0 < r <= 1.0:
        raise ValueError(f"kld_schedule.ratio must be a number in (0, 1], got {r!r}")
    out = {"type": "cyclical", "cycle_steps": int(m), "ratio": float(r)}
    if "cycles" in value:
        n = value["cycles"]
        if not _is_int(n) or n < 1:
            raise ValueError(f"kld_schedule.cycles must be an integer >= 1 (leave it out for cycles without end), got {n!r}")
        out["cycles"] = int(n)
    return out


def kld_free_bits_setting(value):
    """Validated ``exp_params.kld_free_bits``: a float >= 0 (absent: None); anything else is a ValueError that names the key."""
    if value is None:
        return None
    if not _is_number(value) or not 0.0 <= value < float("inf"):
        raise ValueError(f"kld_free_bits must be a number >= 0 (nats per latent dimension), got {value!r}")
    return float(value)


def kl_settings(params):
    """``(schedule, free_bits)`` of an ``exp_params`` mapping, both None without the keys."""
    return kld_schedule_setting(params.get("kld_schedule")), kld_free_bits_setting(params.get("kld_free_bits"))


def serves(model_or_class, loss_type=None) -> bool:
    """Whether the model's training loss is recon + c * M_N * KL with a host constant c.  A class, or a name's class, needs
    ``loss_type`` for BetaVAE (an instance carries its own)."""
    cls = model_or_class if isinstance(model_or_class, type) else type(model_or_class)
    if cls.__name__ not in SERVED_MODELS:
        return False
    if cls.__name__ == "BetaVAE":
        return (loss_type if isinstance(model_or_class, type) else model_or_class.loss_type) == 'H'
    return True


def needs_served_model(key, name) -> str:
    """The refusal of ``kld_schedule`` / ``kld_free_bits`` for a model they do not serve, by name."""
    return (f"{key} needs a model whose loss is recon + c * M_N * KL ({', '.join(SERVED_MODELS)} with loss_type 'H'), got {name}")


def model_kl_scale(model) -> float:
    """The host constant c in front of M_N * KL in the model's loss (beta for LogCoshVAE and BetaVAE type H, else 1)."""
    return float(model.beta) if type(model).__name__ in ("LogCoshVAE", "BetaVAE") else 1.0


def weight(schedule, kld_weight, step) -> float:
    """w(step) under ``schedule`` (a validated mapping, or None: the constant ``kld_weight``): float64 arithmetic, one rounding
    to fp32 at the end -- the value the device scalar holds during optimizer step ``step``."""
    k, s = float(kld_weight), int(step)
    if schedule is None:
        w = k
    elif schedule["type"] == "linear":
        a = schedule["start"]
        w = k * (a + (1.0 - a) * min(1.0, s / schedule["warmup_steps"]))
    else:
        m, n = schedule["cycle_steps"], schedule.get("cycles")
        w = k if (n is not None and s >= n * m) else k * min(1.0, ((s % m) / m) / schedule["ratio"])
    return ctypes.c_float(w).value


class KLControl:
    """The settings of one run and its device scalar.  ``write(step)`` puts w(step) into the scalar with one eager fill, and only
    when the value differs from the last one written: a constant phase launches nothing."""

    def __init__(self, schedule, free_bits, kld_weight, device):
        self.schedule, self.free_bits, self.kld_weight = schedule, free_bits, float(kld_weight)
        self.tensor = torch.empty(1, dtype=torch.float32, device=device)      # persistent: captured steps hold its address
        self.written = None
        self.fills = 0

    @property
    def floor(self) -> float:
        """The lambda the loss launch gets: 0.0 without ``kld_free_bits``."""
        return 0.0 if self.free_bits is None else self.free_bits

    def weight(self, step) -> float:
        return weight(self.schedule, self.kld_weight, step)

    def write(self, step) -> float:
        w = self.weight(step)
        if self.written is None or w != self.written:
            self.tensor.fill_(w)
            self.written = w
            self.fills += 1
        return w

    def state_dict(self):
        return {"schedule": dict(self.schedule) if self.schedule is not None else None, "free_bits": self.free_bits}

    def mismatch(self, entry):
        """None when ``entry`` (a checkpoint's ``trainer['kl']``) was written under this run's settings, else the refusal."""
        if entry is None:
            return ("checkpoint holds no KL control settings (trainer['kl']), this run uses kld_schedule / kld_free_bits: it was "
                    "written by a run without the keys")
        if entry.get("schedule") != self.state_dict()["schedule"]:
            return f"kld_schedule is {self.schedule!r}, but the checkpoint was written under {entry.get('schedule')!r}"
        if entry.get("free_bits") != self.free_bits:
            return f"kld_free_bits is {self.free_bits!r}, but the checkpoint was written under {entry.get('free_bits')!r}"
        return None
