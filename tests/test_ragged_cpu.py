"""fastspeech2_amd/ragged.py: packing against the three rules it replaced (written out below as they stood in preprocess.py /
prepare_align.py, in align.build's `extract` and in align.batches_by_bytes), length and device validation, and the staging buffer
(on pageable memory where there is no GPU runtime to pin with; the pinned buffer and its copy event in the one `gpu` test)."""
import numpy as np
import pytest
import torch

from fastspeech2_amd import ragged


# ------------------------------------------------------------------------------------------------ the old packing rules
def old_audio_batches(lens, batch_samples):
    order = sorted(range(len(lens)), key=lambda i: -lens[i])
    out, batch, longest = [], [], 0
    for i in order:
        if batch and (len(batch) + 1) * max(longest, lens[i]) > batch_samples:
            out.append(batch)
            batch, longest = [], 0
        batch.append(i)
        longest = max(longest, lens[i])
    return out + [batch] if batch else out


def old_extract_batches(lens, batch_samples):
    order = sorted(range(len(lens)), key=lambda i: -lens[i])
    out, batch = [], []
    for i in order + [None]:
        if batch and (i is None or (len(batch) + 1) * lens[batch[0]] > batch_samples):
            out.append(batch)
            batch = []
        if i is not None:
            batch.append(i)
    return out


def byte_cost(dim):
    return lambda n, T, J: n * (T * J * 17 + T * dim * 8 + J * (1 + 2 * dim) * 8)


def old_byte_batches(frames, states, dim, budget):
    order = sorted(range(len(frames)), key=lambda i: (-frames[i], -states[i], i))
    cost = byte_cost(dim)
    out, batch, T, J = [], [], 0, 0
    for i in order:
        if batch and cost(len(batch) + 1, max(T, frames[i]), max(J, states[i])) > budget:
            out.append(batch)
            batch, T, J = [], 0, 0
        batch.append(i)
        T, J = max(T, frames[i]), max(J, states[i])
    return out + [batch] if batch else out


def old_rate_batches(rates, lens, budget):
    by_rate = {}
    for i, sr in enumerate(rates):
        by_rate.setdefault(sr, []).append(i)
    out = []
    for sr in sorted(by_rate):
        idx = by_rate[sr]
        out += [(sr, [idx[k] for k in batch]) for batch in old_audio_batches([lens[i] for i in idx], budget(sr))]
    return out


def _length_lists():
    """seeded random lists: ties (few distinct values), zero lengths, a single item, the empty list"""
    rng = np.random.RandomState(11)
    yield []
    for case in range(300):
        n = 1 if case % 25 == 0 else int(rng.randint(1, 40))
        hi = (4, 50, 100000)[case % 3]
        lens = rng.randint(0, hi + 1, size=n)
        if case % 7 == 0:
            lens[rng.randint(0, n, size=max(n // 3, 1))] = 0
        yield [int(v) for v in lens]


def test_greedy_batches_equals_the_audio_and_extract_rules():
    n_multi = 0
    for lens in _length_lists():
        total, longest = sum(lens), max(lens, default=0)
        for budget in (0, 1, longest - 1, longest, 2 * longest, total // 3, total, 4 * total + 1):     # incl. less than one item
            got = list(ragged.greedy_batches([(n,) for n in lens], budget, ragged.padded_samples))
            assert got == old_audio_batches(lens, budget) == old_extract_batches(lens, budget), (lens, budget)
            assert sorted(i for b in got for i in b) == list(range(len(lens))) and all(got)
            n_multi += len(got) > 1
    assert n_multi > 300


def test_greedy_batches_equals_the_byte_budget_rule():
    rng = np.random.RandomState(5)
    for case, frames in enumerate(_length_lists()):
        states = [int(v) for v in rng.randint(0, (3, 300)[case % 2] + 1, size=len(frames))]
        one = max((byte_cost(160)(1, T, J) for T, J in zip(frames, states)), default=0)
        for budget in (1, one - 1, one, 3 * one, 10 * one + 7):
            got = list(ragged.greedy_batches(list(zip(frames, states)), budget, byte_cost(160)))
            assert got == old_byte_batches(frames, states, 160, budget), (frames, states, budget)


def test_keyed_batches_equals_grouping_by_rate():
    rng = np.random.RandomState(3)
    for lens in _length_lists():
        rates = [int(v) for v in rng.choice([16000, 22050, 24000, 44100], size=len(lens))]
        for scale in (1, 40, 100000):
            budget = lambda sr: scale * sr // 22050                                           # noqa: E731
            got = list(ragged.keyed_batches(rates, [(n,) for n in lens], budget, ragged.padded_samples))
            assert got == old_rate_batches(rates, lens, budget), (rates, lens, scale)


# ------------------------------------------------------------------------------------------------ validation
def test_lengths_accepts_lists_arrays_and_tensors():
    for lens in ([3, 0, 7], np.array([3, 0, 7]), np.array([3, 0, 7], np.int32), torch.tensor([3, 0, 7]), (3, 0, 7)):
        h = ragged.lengths(lens, 3, 7, "lens")
        assert h == [3, 0, 7] and all(type(v) is int for v in h)
    h, d = ragged.lengths(np.array([3, 0, 7]), 3, 7, "lens", torch.device("cpu"))
    assert h == [3, 0, 7] and d.dtype == torch.int32 and d.tolist() == h
    assert ragged.lengths([], 0, 5, "lens") == []
    for bad, B in (([3, 0], 3), ([3, 0, 7, 1], 3), ([3, 0, 8], 3), ([3, -1, 7], 3), (torch.tensor([8]), 1)):
        with pytest.raises(ValueError, match="frames"):
            ragged.lengths(bad, B, 7, "frames")


def test_require_device_and_rows_refuse_the_cpu():
    for t in (torch.zeros(2, 3), torch.device("cpu"), np.zeros(3), None):
        with pytest.raises(RuntimeError) as e:
            ragged.require_device(t, "somewhere")
        assert "AMD GPU only" in str(e.value) and "no CPU fallback" in str(e.value) and "somewhere" in str(e.value)
    dev = torch.device("cuda")
    assert ragged.require_device(dev, "x") is dev                                             # a device names no tensor: no GPU needed
    with pytest.raises(RuntimeError, match="no CPU fallback"):                                # the device check comes first
        ragged.rows(torch.zeros(2, 3, dtype=torch.float64), [9], "x")


# ------------------------------------------------------------------------------------------------ staging
def test_staging_zeroes_tails_clips_grows_and_reuses():
    st = ragged.Staging()
    rows = [np.array([0.5, -3.0, 2.0], np.float32), np.zeros(0, np.float32), np.array([4.0], np.float32)]
    v = st.pack(rows)
    assert v.shape == (3, 3) and v.dtype == torch.float32
    assert v.tolist() == [[0.5, -3.0, 2.0], [0.0, 0.0, 0.0], [4.0, 0.0, 0.0]]
    first = st._buf
    first.fill_(9.0)                                                                          # stale contents must not survive
    v = st.pack(rows[::-1], clip=True)
    assert st._buf is first and v.tolist() == [[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.5, -1.0, 1.0]]
    v = st.pack([np.array([7.0], np.float32)])                                                # smaller: same buffer, its first B * N
    assert st._buf is first and v.shape == (1, 1) and v.data_ptr() == first.data_ptr() and v.item() == 7.0
    big = [np.arange(50, dtype=np.float32), np.arange(20, dtype=np.float32)]
    v = st.pack(big)
    assert st._buf is not first and st._buf.numel() >= 100 and v.shape == (2, 50)
    assert np.array_equal(v[0].numpy(), big[0]) and np.array_equal(v[1, :20].numpy(), big[1]) and not v[1, 20:].any()
    assert torch.equal(st.to(torch.device("cpu")), v)


def test_staging_empty_batches_keep_one_column():
    st = ragged.Staging()
    assert st.pack([]).shape == (0, 1)
    v = st.pack([np.zeros(0, np.float32)] * 4)
    assert v.shape == (4, 1) and not v.any()


@pytest.mark.gpu
def test_staging_is_pinned_and_waits_for_its_copy(dev):
    st = ragged.Staging()
    rng = np.random.RandomState(0)
    first = [rng.randn(n).astype(np.float32) for n in (1 << 20, 1000, 0)]
    host = st.pack(first)
    assert host.is_pinned()
    y = st.to(dev)
    assert st._copied is not None
    second = [rng.randn(n).astype(np.float32) for n in (1 << 20, 1 << 19, 7)]
    st.pack(second, clip=True)                                                                # waits for the copy of `first`
    assert st._copied is None
    z = st.to(dev)
    y, z = y.cpu().numpy(), z.cpu().numpy()
    for b, (r, s) in enumerate(zip(first, second)):
        assert np.array_equal(y[b, :len(r)], r) and not y[b, len(r):].any(), b
        assert np.array_equal(z[b, :len(s)], np.clip(s, -1, 1)) and not z[b, len(s):].any(), b
