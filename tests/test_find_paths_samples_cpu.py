"""planFindPathsBatches (KmerCounter.hpp), the pure function that splits the samples of `bayesTyper cluster` into consecutive batches when
BT_FIND_PATHS_SAMPLES = N asks for up to N samples per best-path launch: batch sizes and the loader thread's permission, from byte counts alone."""
import itertools

import numpy as np

GB = 1 << 30


def _plan(filters, scratch_per_extra_sample, free, n):
    from bayestyper_amd.host import cluster_stage

    batch_bytes = [m * scratch_per_extra_sample for m in range(max(min(n, len(filters)), 1))]   # bt_find_paths_batch_bytes: 0 for one sample, non-decreasing
    sizes, prefetch = cluster_stage.plan_find_paths_batches(filters, batch_bytes, free, n)
    assert sum(sizes) == len(filters) and all(s >= 1 for s in sizes) and len(prefetch) == len(sizes)   # 0 .. S-1 in order, without gaps
    assert all(s <= max(n, 1) for s in sizes)
    assert not prefetch or not prefetch[-1]
    return sizes, prefetch


def test_everything_fits():
    sizes, prefetch = _plan([4 * GB] * 10, GB, 200 * GB, 4)
    assert sizes == [4, 4, 2] and prefetch == [True, True, False]
    assert _plan([4 * GB] * 8, GB, 200 * GB, 4)[0] == [4, 4]


def test_a_filter_larger_than_the_budget_gives_batches_of_one():
    sizes, prefetch = _plan([300 * GB] * 3, GB, 200 * GB, 4)
    assert sizes == [1, 1, 1] and prefetch == [False, False, False]
    # one such filter among small ones stands alone, the others batch around it
    sizes, _ = _plan([GB, GB, 300 * GB, GB, GB], 0, 200 * GB, 4)
    assert sizes == [2, 1, 2]


def test_the_budget_closes_a_batch_early():
    # 3 filters of 60 GB + scratch for 3 (2 GB) = 182 <= 190; a fourth filter would need 243
    sizes, prefetch = _plan([60 * GB] * 7, GB, 190 * GB, 8)
    assert sizes == [3, 3, 1] and prefetch == [False, False, False]   # two batches of three do not fit side by side
    # the scratch alone closes it: the filters of three would fit, their scratch copies would not
    sizes, _ = _plan([10 * GB] * 6, 80 * GB, 120 * GB, 8)
    assert sizes == [2, 2, 2]
    # the loader may work ahead exactly when both batches and the scratch fit
    sizes, prefetch = _plan([40 * GB] * 4, GB, 165 * GB, 2)
    assert sizes == [2, 2] and prefetch == [True, False]
    sizes, prefetch = _plan([40 * GB] * 4, GB, 160 * GB, 2)
    assert sizes == [2, 2] and prefetch == [False, False]


def test_n_larger_than_the_number_of_samples():
    assert _plan([GB] * 3, GB, 100 * GB, 8) == ([3], [False])
    assert _plan([GB], GB, 100 * GB, 8) == ([1], [False])
    assert _plan([], GB, 100 * GB, 8) == ([], [])


def test_n_of_zero_or_one_is_the_per_sample_route():
    for n in (0, 1):
        assert _plan([GB] * 3, GB, 100 * GB, n)[0] == [1, 1, 1]


def test_batches_cover_every_sample_in_order():
    rng = np.random.default_rng(5)
    for s, n in itertools.product((1, 2, 5, 9), (2, 3, 16)):
        for _ in range(20):
            filters = [int(x) for x in rng.integers(1, 80, s) * GB]
            _plan(filters, int(rng.integers(0, 4)) * GB, int(rng.integers(1, 200)) * GB, n)   # (the helper asserts the cover)
