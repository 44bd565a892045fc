"""rng_bernoulli_bulk (bt_rng_device.hpp), the bulk draw behind the Gibbs chain start, on the host: n Bernoulli draws of a block-form ring generator taken
call by call, by the bulk routine as a team of one, and by the direct-form generator.  The flags, the eight words drawn afterwards and the generator's
registers (position in block, buffer flags, ring head, unread ring words) are equal in every case — bit-equality, no tolerance."""
import numpy as np
import pytest

N_VALUES = (0, 1, 311, 312, 313, 1000)   # zero, one, two and four blocks of 624 words (two words per draw)
# words drawn before: positions 0, 1 and 623 of the first block (which lives in the second buffer: the seeded words are the block before it),
# 0, 5 and 623 of the second block (the first buffer again), and one past MT_AHEAD words of a block (a block twisted ahead when `ahead` is set)
DISCARDS = (0, 1, 623, 624, 624 + 5, 624 + 623, 330)
RATE = float(np.float32(0.1))   # the product's k-mer subsampling rate, as bernoulli_distribution stores it


def run(seed, discard, n, p, cap=32, ahead=0):
    from bayestyper_amd import lib

    flags = np.full((3, max(n, 1)), 0xEE, np.uint8)
    tail = np.zeros((3, 8), np.uint32)
    state = np.zeros((2, 4), np.uint32)
    lib.check(lib.bt_diag_bulk_bernoulli(seed, discard, n, p, cap, ahead, flags.ctypes.data, tail.ctypes.data, state.ctypes.data))
    return flags.reshape(-1)[: 3 * n].reshape(3, n), tail, state


@pytest.mark.parametrize("p", [0.0, 1.0, RATE])
@pytest.mark.parametrize("discard", DISCARDS)
@pytest.mark.parametrize("n", N_VALUES)
def test_bulk_equals_sequential(n, discard, p):
    for ahead in (0, 1):
        flags, tail, state = run(2024, discard, n, p, ahead=ahead)
        assert np.array_equal(flags[0], flags[1]) and np.array_equal(flags[0], flags[2]), (n, discard, p, ahead)
        assert np.array_equal(tail[0], tail[1]) and np.array_equal(tail[0], tail[2]), (n, discard, p, ahead)
        assert np.array_equal(state[0], state[1]), (n, discard, p, ahead, state)
        if n:
            assert flags[0].min() >= (1 if p == 1.0 else 0) and flags[0].max() <= (0 if p == 0.0 else 1)


@pytest.mark.parametrize("cap", [8, 16, 64])
def test_other_ring_sizes(cap):
    for discard in (0, 3, 623, 950):
        for n in (1, 7, 312, 700):
            flags, tail, state = run(7, discard, n, RATE, cap=cap)
            assert np.array_equal(flags[0], flags[1]) and np.array_equal(flags[0], flags[2]), (cap, discard, n)
            assert np.array_equal(tail[0], tail[1]) and np.array_equal(tail[0], tail[2]), (cap, discard, n)
            assert np.array_equal(state[0], state[1]), (cap, discard, n, state)


def test_stream_is_std_mt19937_bernoulli():
    """the flags against numpy's MT19937 words put through generate_canonical<double, 53> (two words per draw)"""
    n, discard = 1000, 623
    flags, tail, _ = run(99, discard, n, RATE)
    bg = np.random.MT19937(0)
    bg.state = {"bit_generator": "MT19937", "state": {"key": _seeded_key(99), "pos": 624}}
    words = bg.random_raw(discard + 2 * n + 8).astype(np.uint64)[discard:]
    u = (words[0:2 * n:2].astype(np.float64) + words[1:2 * n:2].astype(np.float64) * 4294967296.0) / 18446744073709551616.0
    assert np.array_equal(flags[1], (u < RATE).astype(np.uint8))
    assert np.array_equal(tail[1], words[2 * n:].astype(np.uint32))


def _seeded_key(seed):
    key = np.zeros(624, np.uint32)
    x = seed
    key[0] = x
    for i in range(1, 624):
        x = (1812433253 * (x ^ (x >> 30)) + i) & 0xFFFFFFFF
        key[i] = x
    return key


def test_argument_errors():
    from bayestyper_amd import lib

    tail = np.zeros(24, np.uint32)
    state = np.zeros(8, np.uint32)
    assert lib.bt_diag_bulk_bernoulli(1, 0, 4, 0.5, 32, 0, None, tail.ctypes.data, state.ctypes.data) != 0
    assert lib.bt_diag_bulk_bernoulli(1, 0, 0, 0.5, 24, 0, None, tail.ctypes.data, state.ctypes.data) != 0
    assert b"ring_cap" in lib.bt_last_error()
