"""What every evaluation of a model shares, on the training harness's side and on the checkpoint commands': the context managers
that leave the caller's run as found, the reading of a data batch, and the ``.npz`` writer.  Imports nothing of the package.
"""
import contextlib
import io
import zipfile

import numpy as np
import torch


@contextlib.contextmanager
def eval_mode(model):
    """eval() + no_grad() for the evaluation; the previous training flag of every module comes back afterwards."""
    if model is None:
        with torch.no_grad():
            yield
        return
    was = [(m, m.training) for m in model.modules()]
    model.eval()
    try:
        with torch.no_grad():
            yield
    finally:
        for m, t in was:
            m.training = t


@contextlib.contextmanager
def seeded_torch_rng(seed: int, device):
    """torch's CPU generator and ``device``'s generator seeded with ``seed`` inside; both states come back afterwards."""
    cuda = device is not None and torch.device(device).type == "cuda"
    cpu_state = torch.get_rng_state()
    dev_state = torch.cuda.get_rng_state(device) if cuda else None
    try:
        torch.default_generator.manual_seed(seed)
        if cuda:
            with torch.cuda.device(device):
                torch.cuda.manual_seed(seed)
        yield
    finally:
        torch.set_rng_state(cpu_state)
        if cuda:
            torch.cuda.set_rng_state(dev_state, device)


def unpack_batch(batch, model=None):
    """``(x, labels[, options, ...])`` -> ``(x, labels, options)``; ``options`` is {} unless the third element is a dict.  With a
    ``model`` that ``uses_labels`` (ConditionalVAE), one label per image comes back as one class column [B, 1]."""
    x, labels, *rest = batch
    opts = rest[0] if rest and isinstance(rest[0], dict) else {}
    if getattr(model, 'uses_labels', False) and torch.is_tensor(labels) and labels.dim() == 1:
        labels = labels.reshape(-1, 1)
    return x, labels, opts


def batch_mode(opts, default=None):
    """The mode of a batch's options: the data hand out one mode per batch, as a string or once per row."""
    mode = opts.get("mode", default)
    if isinstance(mode, (list, tuple)):
        mode = mode[0] if len(mode) else None
    return mode


def npz_bytes(arrays: dict) -> bytes:
    """An uncompressed ``.npz`` (``np.load`` reads it) whose bytes depend on the arrays alone: ``np.savez`` stamps every member
    with the current time."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_STORED) as z:
        for k, v in arrays.items():
            member = io.BytesIO()
            np.lib.format.write_array(member, np.ascontiguousarray(v), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), member.getvalue())
    return buf.getvalue()
