"""The packed form of the sparse frequency distribution's sets (nset_*, BT_GIBBS_NIBBLE_SETS): one 64-bit word of 4-bit fields has to iterate in the order
of the unordered_set emulation (uset_*, itself tested against libstdc++ in test_diag_cpu.py) for every universe of 1 to 13 elements and every history.

bt_diag_nset_replay runs an operation list on the packed primitives, bt_diag_uset_replay the same list on the lists.  The two positional operations of the
packed replay (3: erase at a position, 4: read a position) are stated for the lists as "the element the lists iterate to at that position", found by
replaying the history so far on the lists."""
import ctypes as C

import numpy as np
import pytest

from _oracle import _ptr

NONE = 0xFFFFFFFF
UNIVERSES = list(range(1, 14))


def lists_order(universe, ops, vals):
    """iteration order of the lists after the operations (0 insert, 1 erase, 2 clear)"""
    from bayestyper_amd import lib

    if not ops:
        return []
    o, v = np.asarray(ops, np.uint8), np.asarray(vals, np.uint32)
    out, n = np.zeros(universe, np.uint32), C.c_uint32()
    lib.check(lib.bt_diag_uset_replay(universe, _ptr(o), _ptr(v), len(o), _ptr(out), C.byref(n)))
    return out[: n.value].tolist()


def packed(universe, ops, vals):
    """-> (iteration order, picked elements per operation) of the packed replay"""
    from bayestyper_amd import lib

    o, v = np.asarray(ops, np.uint8), np.asarray(vals, np.uint32)
    out, n, at = np.zeros(16, np.uint32), C.c_uint32(), np.zeros(len(o), np.uint32)
    lib.check(lib.bt_diag_nset_replay(universe, _ptr(o), _ptr(v), len(o), _ptr(out), C.byref(n), _ptr(at)))
    assert n.value <= universe
    return out[: n.value].tolist(), at.tolist()


def agree(universe, ops, vals):
    """both forms on one history; returns (order, picked elements).  The lists get the positional operations as operations by value."""
    l_ops, l_vals, want_at = [], [], []
    for op, v in zip(ops, vals):
        if op in (3, 4):
            order = lists_order(universe, l_ops, l_vals)
            e = order[v] if v < len(order) else NONE
            want_at.append(e)
            if op == 3 and e != NONE:
                l_ops.append(1), l_vals.append(e)
        else:
            want_at.append(NONE)
            l_ops.append(op), l_vals.append(v)
    order, at = packed(universe, ops, vals)
    assert order == lists_order(universe, l_ops, l_vals), (universe, list(ops), list(vals))
    assert at == want_at, (universe, list(ops), list(vals))
    return order, at


@pytest.mark.parametrize("universe", UNIVERSES)
def test_single_elements_and_full_sets(universe):
    for e in range(universe):
        assert agree(universe, [0], [e])[0] == [e]
        assert agree(universe, [0, 1], [e, e])[0] == []
    up = list(range(universe))
    assert agree(universe, [0] * universe, up)[0] == up[::-1]            # freq_reset: H-1, ..., 0
    assert agree(universe, [0] * universe, up[::-1])[0] == up
    perm = np.random.default_rng(universe).permutation(universe).tolist()
    assert agree(universe, [0] * universe, perm)[0] == perm[::-1]
    assert agree(universe, [0] * universe + [0], up + [0])[0] == up[::-1]   # an element that is present is not inserted again


@pytest.mark.parametrize("universe", UNIVERSES)
def test_erase_first_last_middle(universe):
    fill_ops, fill = [0] * universe, list(range(universe))
    order = fill[::-1]
    for pos in sorted({0, universe - 1, universe // 2}):
        rest = order[:pos] + order[pos + 1:]
        assert agree(universe, fill_ops + [1], fill + [order[pos]])[0] == rest      # by value
        got, at = agree(universe, fill_ops + [4, 3, 4], fill + [pos, pos, pos])      # by position, the position read before and after
        assert got == rest and at[-3] == order[pos] and at[-2] == order[pos]
        assert at[-1] == (rest[pos] if pos < len(rest) else NONE)
        # ... and the erased element comes back to the front
        assert agree(universe, fill_ops + [3, 0], fill + [pos, order[pos]])[0] == [order[pos]] + rest
    # a position past the end is ignored
    assert agree(universe, fill_ops + [3, 4], fill + [universe, universe])[0] == order


@pytest.mark.parametrize("universe", UNIVERSES)
def test_clear_and_reinsertion(universe):
    fill_ops, fill = [0] * universe, list(range(universe))
    again = np.random.default_rng(100 + universe).permutation(universe).tolist()
    assert agree(universe, fill_ops + [2], fill + [0])[0] == []
    assert agree(universe, fill_ops + [2] + fill_ops, fill + [0] + again)[0] == again[::-1]
    assert agree(universe, [2, 2] + fill_ops + [1, 2, 0], [0, 0] + fill + [0, 0, universe - 1])[0] == [universe - 1]


@pytest.mark.parametrize("universe", UNIVERSES)
def test_frequency_draw_sequence(universe):
    """freq_reset, hfd_increment moves, the add-zeros picks at positions 0 and |zero| - 1, the re-insertion — three draws in a row, the zero and the plus set
    each replayed in both forms"""
    rng = np.random.default_rng(500 + universe)
    z_ops, z_vals = [0] * universe, list(range(universe))      # freq_reset
    for _ in range(3):
        p_ops, p_vals = [], []
        zero = agree(universe, z_ops, z_vals)[0]
        for h in rng.permutation(zero)[: int(rng.integers(0, len(zero) + 1))].tolist():   # incrementCount of an unobserved haplotype: zero -> plus
            z_ops.append(1), z_vals.append(h)
            p_ops.append(0), p_vals.append(h)
        for where in ("first", "last", "random"):               # add zeros
            zero = agree(universe, z_ops, z_vals)[0]
            if not zero:
                break
            pos = {"first": 0, "last": len(zero) - 1, "random": int(rng.integers(0, len(zero)))}[where]
            z_ops.append(3), z_vals.append(pos)
            picked = agree(universe, z_ops, z_vals)[1][-1]
            assert picked == zero[pos]
            p_ops.append(0), p_vals.append(picked)
        plus = agree(universe, p_ops, p_vals)[0] if p_ops else []
        assert sorted(plus + agree(universe, z_ops, z_vals)[0]) == list(range(universe))
        before = agree(universe, z_ops, z_vals)[0]
        for e in plus:                                          # "for p in plus: zero.insert(p)", then plus.clear()
            z_ops.append(0), z_vals.append(e)
        assert agree(universe, z_ops, z_vals)[0] == plus[::-1] + before
        assert agree(universe, p_ops + [2], p_vals + [0])[0] == []


def test_random_histories():
    rng = np.random.default_rng(20260)
    for i in range(3000):
        universe = 1 + i % 13
        n = int(rng.integers(1, 40))
        r = rng.integers(0, 40, n)
        ops = np.select([r == 0, r < 16, r < 28, r < 36], [2, 0, 1, 3], 4).tolist()
        agree(universe, ops, rng.integers(0, universe, n).tolist())


def test_the_limit_is_thirteen():
    """the packed routines refuse a universe of 14 (and an empty one); at 14 the lists do NOT iterate in push-front order any more — the 14th insert
    rehashes from 13 to 29 buckets — so the constant cannot be raised without deriving the order again"""
    from bayestyper_amd import lib

    assert lib.bt_diag_nset_max() == 13
    for universe in (0, 14, 15, 16, 17):
        with pytest.raises(lib.BtError, match="packed form"):
            packed(universe, [0], [0])
    with pytest.raises(lib.BtError, match="outside the universe"):
        packed(13, [0], [13])
    with pytest.raises(lib.BtError, match="unknown operation"):
        packed(13, [5], [0])
    assert lists_order(13, [0] * 13, list(range(13))) == list(range(13))[::-1]
    assert lists_order(14, [0] * 14, list(range(14))) != list(range(14))[::-1]
