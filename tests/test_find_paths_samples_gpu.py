"""bt_find_paths_samples — several samples' best-path searches in one call — against the same number of bt_find_paths_sample calls on a second object and
against the oracle's findSamplePaths + addPathIndices: equal rows cluster by cluster, on the lane route, the wave route and both in one call."""
import numpy as np
import pytest

from _find_paths_samples import K, Case, clusters, seeds

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small_case(gpu_ctx, oracle):
    """40 clusters of 1-7 variants plus one of 40 variants (about 139 vertices), four samples with filters of their own, max_haps 3, fpr 0.05"""
    rng = np.random.default_rng(53)
    gs, truth, flat = clusters(rng, [int(rng.integers(1, 8)) for _ in range(40)] + [40], max_paths=6)
    case = Case(gpu_ctx, oracle, rng, gs, truth, flat, 3, 0.05, 6, num_samples=4)
    yield case
    case.close()


@pytest.mark.parametrize("wave_min", [0, 1, 100])
def test_batched_equals_sequential_equals_oracle(gpu_ctx, monkeypatch, small_case, wave_min):
    case = small_case
    batched, st, (largest, held) = case.run(gpu_ctx, monkeypatch, wave_min, [[0, 1, 2]], num_samples=3)
    sequential, st_seq, (largest_seq, held_seq) = case.run(gpu_ctx, monkeypatch, wave_min, [0, 1, 2], num_samples=3)
    assert st.num_wave_clusters == {0: 0, 1: len(case.gs), 100: 1}[wave_min]
    assert (largest, largest_seq) == (3, 0) and held > 0 and held_seq == 0
    case.assert_equal(batched, sequential)
    case.assert_equal(batched, case.expect((0, 1, 2)))
    assert st.max_candidate_paths == st_seq.max_candidate_paths
    assert sum(b.shape[0] for b in batched) > len(case.gs)


def test_batched_with_a_wide_cluster_on_the_wave_route(gpu_ctx, oracle, monkeypatch):
    """max_haps 32, fpr 1e-6, the cluster of 150 variants (more than 400 vertices) on a wavefront per sample beside the lane launch of the other 40"""
    rng = np.random.default_rng(52)
    gs, truth, flat = clusters(rng, [int(rng.integers(1, 8)) for _ in range(40)] + [150], max_paths=3)
    case = Case(gpu_ctx, oracle, rng, gs, truth, flat, 32, 1e-6, 2)
    try:
        batched, st, _ = case.run(gpu_ctx, monkeypatch, 400, [[0, 1, 2]])
        sequential, st_seq, _ = case.run(gpu_ctx, monkeypatch, 400, [0, 1, 2])
        assert st.num_wave_clusters == 1 and st.max_vertices > 400
        assert st.max_candidate_paths == st_seq.max_candidate_paths >= 1
        case.assert_equal(batched, sequential)
        case.assert_equal(batched, case.expect())
    finally:
        case.close()


def test_fold_order(gpu_ctx, oracle, monkeypatch):
    """the samples' final paths are folded into the rows in array order: the batch with filters and seed rows reversed equals the reversed sequential run,
    and — on a batch chosen with the oracle so that the order matters — not the forward one"""
    case = None
    for data_seed in range(61, 66):   # the first batch whose rows depend on the order of the samples (decided on the CPU)
        rng = np.random.default_rng(data_seed)
        gs, truth, flat = clusters(rng, [int(rng.integers(1, 8)) for _ in range(40)] + [40], max_paths=6)
        case = Case(gpu_ctx, oracle, rng, gs, truth, flat, 3, 0.05, 6)
        if case.differ(case.expect((0, 1, 2)), case.expect((2, 1, 0))):
            break
        case.close()
        case = None
    assert case is not None, "no batch whose rows depend on the sample order"
    try:
        forward, backward = case.expect((0, 1, 2)), case.expect((2, 1, 0))
        assert case.differ(forward, backward)
        for wave_min in (0, 100):
            got_fwd, _, _ = case.run(gpu_ctx, monkeypatch, wave_min, [[0, 1, 2]])
            got_bwd, _, _ = case.run(gpu_ctx, monkeypatch, wave_min, [[2, 1, 0]])
            seq_bwd, _, _ = case.run(gpu_ctx, monkeypatch, wave_min, [2, 1, 0])
            case.assert_equal(got_fwd, forward)
            case.assert_equal(got_bwd, seq_bwd)
            case.assert_equal(got_bwd, backward)
            assert case.differ(got_fwd, got_bwd)
    finally:
        case.close()


@pytest.mark.parametrize("wave_min", [0, 100])
def test_mixing_calls_on_one_object(gpu_ctx, monkeypatch, small_case, wave_min):
    case = small_case
    expect = case.expect((0, 1, 2, 3))
    mixed, _, (largest, _) = case.run(gpu_ctx, monkeypatch, wave_min, [0, [1, 2], 3])
    sequential, _, _ = case.run(gpu_ctx, monkeypatch, wave_min, [0, 1, 2, 3])
    assert largest == 2
    case.assert_equal(mixed, sequential)
    case.assert_equal(mixed, expect)
    # samples([s]) is sample(s): no batch memory
    single, _, (largest, held) = case.run(gpu_ctx, monkeypatch, wave_min, [[0], [1], [2], [3]])
    assert (largest, held) == (1, 0)
    case.assert_equal(single, expect)
    # a second call with a larger n than the first
    grown, _, (largest, _) = case.run(gpu_ctx, monkeypatch, wave_min, [[0], [1, 2, 3]])
    assert largest == 3
    case.assert_equal(grown, expect)


def test_grow_path(gpu_ctx, monkeypatch, small_case):
    """n = 2 then n = 3 on one object (the batch allocation is replaced by a larger one), then n = 2 again (kept): the rows of five sequential calls"""
    from bayestyper_amd import lib

    case = small_case
    monkeypatch.setenv("BT_FIND_PATHS_WAVE_MIN", "100")
    C = len(case.gs)
    gf = lib.FindPaths(gpu_ctx, case.flat, K, case.max_haps, 7)
    seq = lib.FindPaths(gpu_ctx, case.flat, K, case.max_haps, 7)
    try:
        need2, need3 = gf.batch_bytes(2), gf.batch_bytes(3)
        gf.samples([case.blooms[0], case.blooms[1]], case.seed_rows([0, 1]))
        assert gf.batch_info() == (2, need2) and gf.batch_bytes(2) == 0 and gf.batch_bytes(3) == need3 - need2
        gf.samples([case.blooms[2], case.blooms[3], case.blooms[0]], case.seed_rows([2, 3, 0]))
        assert gf.batch_info() == (3, need3) and gf.batch_bytes(3) == 0
        gf.samples([case.blooms[1], case.blooms[2]], case.seed_rows([1, 2]))
        assert gf.batch_info() == (3, need3)
        for s in (0, 1, 2, 3, 0, 1, 2):
            seq.sample(case.blooms[s], seeds(C, s))
        case.assert_equal(gf.best_paths(), seq.best_paths())
    finally:
        gf.close()
        seq.close()


def test_more_than_64_candidate_paths_at_a_vertex(gpu_ctx, oracle, monkeypatch):
    """four multi-allelic clusters of 9-20 variants, in-degree 3-4 with 32 kept paths per predecessor, two samples batched on the wave route"""
    rng = np.random.default_rng(57)
    gs, truth, flat = clusters(rng, [12, 16, 20, 9], max_paths=6, nested=False, kinds=("multi", "multi", "multi", "snv"))
    case = Case(gpu_ctx, oracle, rng, gs, truth, flat, 32, 0.05, 6, num_samples=2)
    try:
        batched, st, _ = case.run(gpu_ctx, monkeypatch, 1, [[0, 1]])
        sequential, st_seq, _ = case.run(gpu_ctx, monkeypatch, 1, [0, 1])
        print("max_candidate_paths", st.max_candidate_paths, st_seq.max_candidate_paths)
        assert st.num_wave_clusters == len(gs)
        assert st.max_candidate_paths == st_seq.max_candidate_paths > 64
        case.assert_equal(batched, sequential)
        case.assert_equal(batched, case.expect())
    finally:
        case.close()


def test_errors_leave_the_object_usable(gpu_ctx, monkeypatch, small_case):
    from bayestyper_amd import lib

    case = small_case
    monkeypatch.setenv("BT_FIND_PATHS_WAVE_MIN", "100")
    C = len(case.gs)
    other_k = lib.Bloom.create(gpu_ctx, 1000, 0.05, K - 4, threaded=False)
    gf = lib.FindPaths(gpu_ctx, case.flat, K, case.max_haps, 3)
    try:
        for blooms, rows in (([], np.zeros((0, C), np.uint32)), ([case.blooms[0], None], case.seed_rows([0, 1])), ([case.blooms[0], other_k], case.seed_rows([0, 1]))):
            with pytest.raises(RuntimeError) as e:
                gf.samples(blooms, rows)
            assert "bt_find_paths_samples" in str(e.value), str(e.value)
        assert gf.batch_info() == (0, 0)
        assert all(b.shape[0] == 0 for b in gf.best_paths())   # nothing was searched
        gf.samples([case.blooms[0], case.blooms[1], case.blooms[2]], case.seed_rows([0, 1, 2]))
        case.assert_equal(gf.best_paths(), case.expect((0, 1, 2)))
    finally:
        gf.close()
        other_k.close()


def test_batch_bytes(gpu_ctx, monkeypatch, small_case):
    from bayestyper_amd import lib

    monkeypatch.setenv("BT_FIND_PATHS_WAVE_MIN", "100")
    gf = lib.FindPaths(gpu_ctx, small_case.flat, K, small_case.max_haps, 3)
    try:
        need = [gf.batch_bytes(n) for n in range(1, 12)]
        assert need[0] == 0 and need[1] > 0
        assert all(a <= b for a, b in zip(need, need[1:]))
        with pytest.raises(RuntimeError):
            gf.batch_bytes(0)
    finally:
        gf.close()
