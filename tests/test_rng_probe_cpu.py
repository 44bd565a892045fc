"""The references of the generator probe agree, with no GPU: the host twin (bt_diag_rng_probe) equals the textbook mt19937 stream walked by the Python
models of tests/_rng_probe.py and libstdc++ (the oracle's orc_rng) on the whole case corpus that tests/test_rng_probe_gpu.py runs on the device — and the
corpus reaches what it is meant to reach (the census), with every accept / reject decision of its normal and gamma draws clear of its boundary."""
import numpy as np
import pytest

import _oracle
import _rng_probe as P
from _oracle import _ptr


@pytest.fixture(scope="module")
def orc(oracle):
    _oracle._gibbs_sigs(oracle.l)
    return oracle


@pytest.fixture(scope="module")
def twin():
    """the host twin's rows and finals of the whole corpus: [case][generator]"""
    from bayestyper_amd import lib

    cases = P.corpus()
    lane_gen, gens, steps, row_cap = P.pack(cases)
    rows, fin = lib.rng_probe(None, lane_gen, gens, steps, row_cap)
    return cases, rows, fin


def test_twin_equals_textbook_stream(twin):
    """(c) = (a): every word, flag, permutation and canonical double, the state words after every step, the final state and the tail"""
    cases, rows, fin = twin
    for c, cs in enumerate(cases):
        for g, G in cs["gens"].items():
            E = P.expected(c, g)
            n = len(E["row"])
            got = rows[c, g, :n]
            bad = np.flatnonzero((got != E["row"]) & E["known"])
            assert bad.size == 0, (cs["name"], g, bad[:5], got[bad[:5]], E["row"][bad[:5]])
            assert (rows[c, g, n:] == 0xFFFFFFFF).all(), (cs["name"], g)
            assert np.array_equal(fin[c, g], E["final"]), (cs["name"], g, fin[c, g], E["final"])
            for st in E["steps"]:
                if st["kind"] == P.BULK:   # a team of one: the ballot is the flag
                    seg = got[st["begin"]:st["end"]].reshape(-1, 3)
                    assert np.array_equal(seg[:, 1], seg[:, 0]) and not seg[:, 2].any()
        idle = [g for g in range(64) if g not in cs["gens"]]
        assert (rows[c, idle] == 0xFFFFFFFF).all() and (fin[c, idle] == 0xFFFFFFFF).all()


def test_first_word_is_the_textbook_one():
    assert int(P.stream(5489)[0]) == 3499211612


def _orc(orc, seed, kind, a, b, n, out_n):
    a = None if a is None else np.ascontiguousarray(a, np.float64)
    b = None if b is None else np.ascontiguousarray(b, np.float64)
    out = np.zeros(max(out_n, 1))
    orc.l.orc_rng(seed, kind, None if a is None else _ptr(a), None if b is None else _ptr(b), n, _ptr(out))
    return out[:out_n]


def test_twin_equals_libstdcxx_integers(twin, orc):
    """(c) = (b): the lanes of the integer case that run one distribution from the start of the stream"""
    cases, rows, _ = twin
    c = next(i for i, cs in enumerate(cases) if cs["name"] == "integers")
    seen = set()
    for g, G in cases[c]["gens"].items():
        ref = P.libstdcxx_integers(lambda *a: _orc(orc, *a), G)
        if ref is None:
            continue
        E = P.expected(c, g)
        got = P.payload(rows[c, g], E)
        assert np.array_equal(got, ref), (g, G["steps"][0])
        seen.add(G["steps"][0][0])
    assert seen == {P.CANONICAL, P.CANONICAL2, P.BERNOULLI, P.UNIFORM_INT, P.SHUFFLE}


def test_twin_equals_libstdcxx_normal_gamma(twin, orc):
    """(c) = (b), bit for bit (both run the host's libm), values and the raw word after every draw; the Python model's stream position is the same"""
    cases, rows, _ = twin
    c = next(i for i, cs in enumerate(cases) if cs["name"] == "normal_gamma")
    for g, G in cases[c]["gens"].items():
        values, raws = P.libstdcxx_normal_gamma(lambda *a: _orc(orc, *a), G)
        E = P.expected(c, g)
        got = P.payload(rows[c, g], E).reshape(-1, 3)
        assert np.array_equal(P.f64(got[:, :2].reshape(-1)), values), g
        assert np.array_equal(got[:, 2], raws), g
        model = P.payload(E["row"], E).reshape(-1, 3)
        assert np.array_equal(model[:, 2], raws), g
        # the extended-precision model's values: an independent, loose check of the reference itself
        assert np.allclose(P.f64(model[:, :2].reshape(-1)), values, rtol=1e-12, atol=0)


def test_decision_margins():
    """no decision of the normal / gamma corpus — r2 > 1, v <= 0, u > 1 - 0.0331 n^4, the second test — lies within relative 1e-9 of its boundary, in extended
    precision from stream (a): a few units in the last place of the device's log, sqrt and pow cannot legitimately flip one"""
    cases = P.corpus()
    c = next(i for i, cs in enumerate(cases) if cs["name"] == "normal_gamma")
    assert len(cases[c]["gens"]) == 64
    tested = {k: 0 for k in ("r2", "v", "first", "second")}
    for g in cases[c]["gens"]:
        for k, m in P.expected(c, g)["margins"].items():
            assert m > P.MARGIN, (g, k, m)
            tested[k] += np.isfinite(m)
    assert tested["r2"] == 64 and tested["v"] >= 50 and tested["first"] >= 50 and tested["second"] >= 50, tested
    shapes = {s[2] for G in cases[c]["gens"].values() for s in G["steps"] if s[0] == P.GAMMA}
    assert set(P.GAMMA_SHAPES) <= shapes and max(shapes) > 9e6
    assert {s[3] for G in cases[c]["gens"].values() for s in G["steps"] if s[0] == P.GAMMA} >= set(P.GAMMA_SCALES)


def test_census():
    """every mechanism the corpus is built for is reached (from the ring model, which the twin's state words confirm step by step)"""
    cen = P.census()
    print(cen)
    assert cen["block_end_single_lane"] >= 1 and cen["block_end_all_64"] >= 1
    assert cen["flip_without_twist"] >= 1 and cen["twist_at_block_end"] >= 1
    assert cen["bulk_two_blocks"] >= 1
    assert cen["wrap_caps"] == {8, 16, 32, 64}
    assert set(cen["helper_counts"]) >= {1, 2, 3, 56, 57, 58, 63, 64, 32}
    t = cen["topup_positions"]
    assert any(p < P.MT_AHEAD for p in t) and P.MT_AHEAD in t and any(P.MT_AHEAD < p < P.MT_N for p in t)
    assert cen["topup_mixed_wants"] >= 1            # one top-up in which some lanes want the next block and some do not
    assert cen["flags_flip"] >= 1 and cen["flags_twist"] >= 1   # the flags group: a block end after a ready block, and one without
    assert cen["bulk_combos"] == 108 * 2 and cen["bulk_copies"] == {4, 16}
    assert cen["shared_copies"] == {2, 4, 8, 16, 32}


def test_screen_reference(twin):
    """the screen grid: at most 1 % of its cases undecidable in double, cases on both sides of the screen's bound, and the host twin decides as the
    extended-precision reference does"""
    cases, rows, _ = twin
    total = skipped = inside = outside = wrong = 0
    for c, cs in enumerate(cases):
        if cs["group"] != "screen":
            continue
        for g, G in cs["gens"].items():
            got = rows[c, g, 0:3 * len(G["screen"]):3]
            for q, d in zip(G["screen"], got):
                total += 1
                skipped += q["undecidable"]
                inside += q["inside"] is True
                outside += q["inside"] is False
                if not q["undecidable"]:
                    assert d in (0, 1)
                    wrong += bool(d) != q["rejects"]
    print("screen cases", total, "undecidable", skipped, "inside the bound", inside, "outside", outside)
    assert total >= 7776 + 12 + 6
    assert skipped <= total // 100
    assert inside >= 100 and outside >= 100
    assert wrong == 0


def test_malformed_programs_are_refused():
    from bayestyper_amd import lib

    ok = P.case("ok", "x", {0: 0}, {0: P.gen(1, [(P.DRAW, 5)])})

    def run(cs, row_cap=None):
        lane_gen, gens, steps, cap = P.pack([cs])
        return lib.rng_probe(None, lane_gen, gens, steps, row_cap or cap)

    run(ok)
    bad = [
        P.case("kind", "x", {0: 0}, {0: P.gen(1, [(13, 5)])}),
        P.case("cap", "x", {0: 0}, {0: P.gen(1, [(P.DRAW, 5)], cap=24)}),
        P.case("cap4", "x", {0: 0}, {0: P.gen(1, [(P.DRAW, 5)], cap=4)}),
        P.case("place", "x", {0: 0}, {0: P.gen(1, [(P.DRAW, 5)], place=3)}),
        P.case("copies", "x", {0: 0, 1: 0, 2: 0}, {0: P.gen(1, [(P.DRAW, 5)], copies=3)}),
        P.case("lanes", "x", {0: 0, 1: 0}, {0: P.gen(1, [(P.DRAW, 5)], copies=2)}),          # the copies of lane 0 are lanes 0 and 32
        P.case("alone", "x", {0: 0, 32: 0}, {0: P.gen(1, [(P.DRAW, 5)], copies=1)}),
        P.case("discard", "x", {0: 0}, {0: P.gen(1, [(P.DRAW, 5)], discard=1873)}),
        P.case("count", "x", {0: 0}, {0: P.gen(1, [(P.DRAW, 2049)])}),
        P.case("steps", "x", {0: 0}, {0: P.gen(1, [(P.DRAW, 1)] * 65)}),
        P.case("shuffle", "x", {0: 0}, {0: P.gen(1, [(P.SHUFFLE, 449)])}),
        P.case("range", "x", {0: 0}, {0: P.gen(1, [(P.UNIFORM_INT, 1, 0.0)])}),
        P.case("p", "x", {0: 0}, {0: P.gen(1, [(P.BULK, 1, float("nan"))])}),
        P.case("alpha", "x", {0: 0}, {0: P.gen(1, [(P.GAMMA, 1, 0.0, 1.0)])}),
        P.case("width", "x", {0: 0}, {0: P.gen(1, [(P.DIRECT, 3, 3.0)])}),
        P.case("direct", "x", {0: 0, 32: 0}, {0: P.gen(1, [(P.DIRECT, 4, 4.0)], copies=2)}),
    ]
    for cs in bad:
        with pytest.raises(lib.BtError, match="bt_diag_rng_probe"):
            run(cs)
    with pytest.raises(lib.BtError, match="more than a row holds"):
        run(ok, row_cap=6)
    lane_gen, gens, steps, cap = P.pack([ok])
    lane_gen[0, 5] = 64
    with pytest.raises(lib.BtError, match="lane map"):
        lib.rng_probe(None, lane_gen, gens, steps, cap)
    gens[0, 0]["step_off"] = 1
    lane_gen[0, 5] = -1
    with pytest.raises(lib.BtError, match="step list"):
        lib.rng_probe(None, lane_gen, gens, steps, cap)
