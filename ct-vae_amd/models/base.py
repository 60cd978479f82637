"""``BaseVAE`` — the drop-in boundary (reference: models/base.py:5-28).

Same abstract API (encode / decode / sample / generate / forward / loss_function); concrete models
additionally mix in ``FlatParamMixin`` so parameters live in one packed HBM buffer.
"""
from abc import abstractmethod
from typing import Any, List

from torch import nn

from .packing import FlatParamMixin
from .types_ import Tensor


class BaseVAE(FlatParamMixin, nn.Module):

    def __init__(self) -> None:
        super().__init__()

    def encode(self, input: Tensor) -> List[Tensor]:
        raise NotImplementedError

    def decode(self, input: Tensor) -> Any:
        raise NotImplementedError

    def sample(self, batch_size: int, current_device: int, **kwargs) -> Tensor:
        raise NotImplementedError

    def generate(self, x: Tensor, **kwargs) -> Tensor:
        raise NotImplementedError

    def gaussian_posterior(self, results: List[Tensor]):
        """(mu, log_var) of ``forward``'s results as [B, L] views, for the models with a Gaussian posterior (latentstats.py);
        None for every other model."""
        return None

    def reconstruction_pair(self, results: List[Tensor]):
        """(recons, target) of ``forward``'s results as two [B, C, S, S] tensors (reconstats.py), or None when the batch has no
        picture pair.  The default: ``results[0], results[1]`` when both are 4-D and of one shape."""
        if len(results) < 2:
            return None
        recons, target = results[0], results[1]
        if not (hasattr(recons, "dim") and hasattr(target, "dim")) or recons.dim() != 4 or recons.shape != target.shape:
            return None
        return recons, target

    @abstractmethod
    def forward(self, *inputs: Tensor) -> Tensor:
        pass

    @abstractmethod
    def loss_function(self, *inputs: Any, **kwargs) -> Tensor:
        pass
