"""GPU: the two launches that replace ``ctvae_adam_block_flags`` when the flags are reduced across ranks
(``kernels.adam_block_flags_local`` / ``adam_block_flags_finish``), against a numpy truth table.

7 blocks, 5 hit words: blocks 0 and 3 have no hit index, the other five own one hit word each.  Eight rounds rotate every
block through all eight (present, hit, seen) combinations.  The local launch must ignore ``seen`` and clear every hit word; the
finish launch must turn a reduced 0 into 1 only under "skip_until_first" with ``seen != 0``; and local + finish with nothing in
between must leave what the fused launch leaves."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NB, NHITS = 7, 5
HIT_INDEX = [-1, 0, 1, -1, 2, 3, 4]
MODES = ("skip", "skip_until_first")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _round(t):
    """present [NB], hits [NHITS], seen [NB] of round t: block b gets combination (b + t) % 8, bit 0 = present, bit 1 = its hit
    word (ignored by a block without one), bit 2 = seen."""
    combo = [(b + t) % 8 for b in range(NB)]
    present = np.array([c & 1 for c in combo], dtype=np.int32)
    seen = np.array([(c >> 2) & 1 for c in combo], dtype=np.float32)
    hits = np.zeros(NHITS, dtype=np.int32)
    for b, h in enumerate(HIT_INDEX):
        if h >= 0:
            hits[h] = (combo[b] >> 1) & 1
    return present, hits, seen


def _raw(present, hits):
    return np.array([int(present[b] and (h < 0 or hits[h])) for b, h in enumerate(HIT_INDEX)], dtype=np.int32)


def _table(dev):
    from ctvae_amd import kernels as K
    return K.AdamBlockTable([(4 * b, 4 * b + 3) for b in range(NB)], HIT_INDEX, 4 * NB, NHITS, dev)


def _load(table, hits, seen, dev):
    table.hits.copy_(torch.from_numpy(hits))
    table.state[:, 3] = torch.from_numpy(seen).to(dev)
    table.active.fill_(-7)


def test_rounds_cover_every_combination():
    got = set()
    for t in range(8):
        present, hits, seen = _round(t)
        for b, h in enumerate(HIT_INDEX):
            got.add((h >= 0, int(present[b]), int(hits[h]) if h >= 0 else None, int(seen[b])))
    want = {(True, p, h, s) for p in (0, 1) for h in (0, 1) for s in (0, 1)} | {(False, p, None, s) for p in (0, 1) for s in (0, 1)}
    assert got == want


@pytest.mark.parametrize("t", range(8))
def test_local_ignores_seen_and_clears_the_hit_words(dev, t):
    from ctvae_amd import kernels as K
    present, hits, seen = _round(t)
    table = _table(dev)
    _load(table, hits, seen, dev)
    state = table.state.clone()
    K.adam_block_flags_local(table, torch.from_numpy(present).to(dev))
    torch.cuda.synchronize()
    assert table.active.cpu().numpy().tolist() == _raw(present, hits).tolist()
    assert table.hits.cpu().tolist() == [0] * NHITS
    assert torch.equal(table.state, state)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("t", range(8))
def test_finish_adds_seen_blocks_only_until_first(dev, mode, t):
    from ctvae_amd import kernels as K
    reduced, hits, seen = _round(t)                      # any 0 / 1 vector serves as the reduced flags
    table = _table(dev)
    _load(table, hits, seen, dev)
    table.active.copy_(torch.from_numpy(reduced))
    state = table.state.clone()
    K.adam_block_flags_finish(table, mode)
    torch.cuda.synchronize()
    want = reduced | (seen != 0).astype(np.int32) if mode == "skip_until_first" else reduced
    assert table.active.cpu().numpy().tolist() == want.tolist()
    assert table.hits.cpu().tolist() == hits.tolist() and torch.equal(table.state, state)      # finish touches the flags alone


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("t", range(8))
def test_local_then_finish_equals_the_fused_launch(dev, mode, t):
    from ctvae_amd import kernels as K, native
    present, hits, seen = _round(t)
    pres = torch.from_numpy(present).to(dev)
    fused, split = _table(dev), _table(dev)
    for table in (fused, split):
        _load(table, hits, seen, dev)
    native.call("ctvae_adam_block_flags", pres.data_ptr(), fused.hit_index.data_ptr(), fused.hits.data_ptr(), fused.nhits,
                fused.state.data_ptr(), fused.active.data_ptr(), fused.nb, 1 if mode == "skip_until_first" else 0)
    K.adam_block_flags_local(split, pres)
    K.adam_block_flags_finish(split, mode)               # the identity reduction in between
    torch.cuda.synchronize()
    assert torch.equal(split.active, fused.active) and torch.equal(split.hits, fused.hits)
    want = _raw(present, hits) | (seen != 0).astype(np.int32) if mode == "skip_until_first" else _raw(present, hits)
    assert fused.active.cpu().numpy().tolist() == want.tolist()
