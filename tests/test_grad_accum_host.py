"""CPU: the host side of ``accumulate_grad_batches`` -- the window schedule (Lightning 1.6.5's rule), the validation of the
setting on its way through FlatAdam, VAEXperiment and run.py, and what the feature allocates."""
import pytest
import torch

CFG = dict(in_channels=3, embedding_dim=16, hidden_dims=[8, 16], num_embeddings=8, img_size=64, codebooks=1, beta=0.25)
PARAMS = {"LR": 1e-3, "weight_decay": 0.0, "kld_weight": 1.0}
REFUSED = [True, False, 0, -1, -3, 2.0, 0.5, "2", {0: 2}, {}, [2]]


def _rule(n, k):
    """Batch i (from 0) ends a window when (i + 1) % k == 0 or it is the epoch's last batch -- written out, not computed by
    the code under test."""
    out = []
    for i in range(n):
        out.append(((i + 1) % k == 0) or (i == n - 1))
    return out


CASES = {(1, 1): [True], (5, 1): [True] * 5, (1, 4): [True], (4, 2): [False, True, False, True],
         (5, 2): [False, True, False, True, True], (7, 3): [False, False, True, False, False, True, True]}


@pytest.mark.parametrize("n,k", sorted(CASES))
def test_schedule_follows_the_rule(n, k):
    from ctvae_amd.optim import accumulation_schedule, with_window_ends
    assert _rule(n, k) == CASES[(n, k)]                                   # the table above is the rule
    assert accumulation_schedule(n, k) == CASES[(n, k)]
    # the look-ahead form fit() uses, on an iterable without a length: same batches, same order, same ends
    got = list(with_window_ends((("batch", i) for i in range(n)), k))
    assert [b for b, _ in got] == [("batch", i) for i in range(n)]
    assert [e for _, e in got] == CASES[(n, k)]
    assert sum(CASES[(n, k)]) == -(-n // k)                               # optimizer steps per epoch


def test_schedule_of_an_empty_epoch():
    from ctvae_amd.optim import accumulation_schedule, with_window_ends
    assert accumulation_schedule(0, 3) == [] and list(with_window_ends(iter(()), 3)) == []


def test_look_ahead_reads_one_batch_ahead_only():
    from ctvae_amd.optim import with_window_ends
    pulled = []

    def loader():
        for i in range(5):
            pulled.append(i)
            yield i

    seen = []
    for b, _ in with_window_ends(loader(), 2):
        seen.append((b, max(pulled)))
    assert seen == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 4)]


def test_setting_is_validated_and_names_the_key():
    from ctvae_amd.optim import accumulate_setting
    assert accumulate_setting(None) == 1 and accumulate_setting(1) == 1 and accumulate_setting(7) == 7
    for bad in REFUSED:
        with pytest.raises(ValueError, match="accumulate_grad_batches"):
            accumulate_setting(bad)
    with pytest.raises(ValueError, match="schedule"):
        accumulate_setting({4: 2})


def _model():
    from ctvae_amd.models import vae_models
    torch.manual_seed(7)
    return vae_models["MCQVAE"](**dict(CFG, hidden_dims=list(CFG["hidden_dims"])))


def test_experiment_and_optimizer_refuse_bad_values():
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.optim import FlatAdam
    m = _model()
    for bad in REFUSED:
        with pytest.raises(ValueError, match="accumulate_grad_batches"):
            VAEXperiment(m, PARAMS, accumulate_grad_batches=bad)
        with pytest.raises(ValueError, match="accumulate_grad_batches"):
            FlatAdam(m, lr=1e-3, accumulate=bad)
    assert VAEXperiment(m, PARAMS).accumulate == 1
    assert VAEXperiment(m, PARAMS, accumulate_grad_batches=None).accumulate == 1
    exp = VAEXperiment(m, PARAMS, accumulate_grad_batches=4)
    assert exp.accumulate == 4 and exp.optimizer.accumulate == 4


def test_runner_reads_the_key_from_trainer_params():
    """run.py's reading of a YAML's trainer_params (run.main itself needs a GPU: tests/test_grad_accum_gpu.py)."""
    import yaml
    from ctvae_amd import run
    assert run.trainer_accumulate({"gpus": [1], "max_epochs": 3}) == 1
    assert run.trainer_accumulate(yaml.safe_load("accumulate_grad_batches: 4")) == 4
    for bad in REFUSED:
        tp = yaml.safe_load(yaml.safe_dump({"accumulate_grad_batches": bad}))
        with pytest.raises(SystemExit, match="trainer_params.accumulate_grad_batches"):
            run.trainer_accumulate(tp)


def test_no_accumulator_at_k1_and_a_slice_sized_one_above():
    from ctvae_amd.optim import FlatAdam
    m = _model()
    n = m.flat_params.numel()
    for kw in ({}, {"accumulate": 1}, {"accumulate": None}):
        opt = FlatAdam(m, lr=1e-3, **kw)
        assert opt.acc is None and opt.window_flags is None and opt.stashed == 0
        with pytest.raises(RuntimeError, match="accumulate=1"):
            opt.stash()
    opt = FlatAdam(m, lr=1e-3, accumulate=2)
    assert opt.acc.numel() == n and opt.acc.dtype == torch.float32 and opt.window_flags is None
    assert opt.acc.data_ptr() % 16 == m.flat_grads.data_ptr() % 16
    sl = m.flat_range("decoder")
    assert 0 < sl.start and sl.stop - sl.start < n
    for start in (sl.start, sl.start + 1, sl.start + 2, sl.start + 3):          # a slice may begin at any float
        s = slice(start, sl.stop)
        opt = FlatAdam(m, lr=1e-3, params_slice=s, accumulate=3)
        assert opt.acc.numel() == sl.stop - start and not bool(opt.acc.any())
        assert opt.acc.data_ptr() % 16 == m.flat_grads[s].data_ptr() % 16       # same phase: the kernel's 16-byte loop runs
        assert opt.acc.untyped_storage().nbytes() <= 4 * (sl.stop - start + 3)
    skip = FlatAdam(m, lr=1e-3, absent_grad="skip", accumulate=2)
    assert skip.window_flags.dtype == torch.int32 and skip.window_flags.numel() == skip.table.nb
    assert FlatAdam(m, lr=1e-3, absent_grad="skip").window_flags is None


def test_ranged_exchange_is_refused_under_accumulation():
    """SplitBackward's overlap sends ranges of one micro-batch's gradients: not available inside a window."""
    from ctvae_amd.ddp import GradBucketAllReduce
    from ctvae_amd.experiment import VAEXperiment
    m = _model()
    ddp = GradBucketAllReduce(m)
    assert ddp.accumulate == 1 and ddp.all_reduce_range(0, 8) == []
    VAEXperiment(m, PARAMS, ddp=ddp)
    assert ddp.accumulate == 1
    VAEXperiment(m, PARAMS, ddp=ddp, accumulate_grad_batches=2)
    assert ddp.accumulate == 2
    with pytest.raises(RuntimeError, match="accumulate_grad_batches=2"):
        ddp.all_reduce_range(0, 8)
