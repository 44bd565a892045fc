"""The random-number stack on the device itself: bt_rng_probe runs the case corpus of tests/_rng_probe.py, a wavefront per case, in two launches, and every
word, flag, ballot, permutation and state word must equal the textbook stream (a), libstdc++ (b) and the host twin (c) — which tests/test_rng_probe_cpu.py
shows to agree with one another.  What each group of cases is for: DESIGN.md, section 4.1c."""
import numpy as np
import pytest

import _oracle
import _rng_probe as P
from _oracle import _ptr

pytestmark = pytest.mark.gpu

# Largest distance between the device's value and libstdc++'s over the normal / gamma case, in units in the last place, measured on an MI355X, and the
# bound asserted: four times that (other seeds reach other arguments of log, sqrt and pow).  The accept / reject decisions are not covered by this
# tolerance: the raw word after every draw must be libstdc++'s, exactly.
MEASURED_ULPS = {"normal": 2, "gamma_ge1": 6, "gamma_lt1": 6}   # -> bounds 8, 24, 24
BOUND_ULPS = {k: 4 * v for k, v in MEASURED_ULPS.items()}
BIG = ("bulk", "bulk_one")


@pytest.fixture(scope="module")
def orc(oracle):
    _oracle._gibbs_sigs(oracle.l)
    return oracle


@pytest.fixture(scope="module")
def runs(gpu_ctx):
    """the corpus on the device (rows and finals by LANE) and on the host (by GENERATOR): {case index: (rows, finals, twin rows, twin finals)}"""
    from bayestyper_amd import lib

    cases = P.corpus()
    out = {}
    for pick in (lambda g: g not in BIG, lambda g: g in BIG):
        idx = [i for i, cs in enumerate(cases) if pick(cs["group"])]
        lane_gen, gens, steps, row_cap = P.pack([cases[i] for i in idx])
        rows, fin = lib.rng_probe(gpu_ctx, lane_gen, gens, steps, row_cap)
        trows, tfin = lib.rng_probe(None, lane_gen, gens, steps, row_cap)
        for k, i in enumerate(idx):
            out[i] = rows[k], fin[k], trows[k], tfin[k]
    return cases, out


def _check_lane(cs, c, lane, g, run, skip=None):
    """the lane's row, final state and tail against the model of stream (a) and against the host twin"""
    rows, fin, trows, tfin = run
    E = P.expected(c, g)
    n = len(E["row"])
    got = rows[lane, :n]
    known = E["known"].copy()
    if skip is not None:   # (words the caller checks itself)
        known[skip[0]:skip[1]] = False
    bad = np.flatnonzero((got != E["row"]) & known)
    assert bad.size == 0, (cs["name"], "lane", lane, "generator", g, "first differing words", bad[:5], got[bad[:5]], E["row"][bad[:5]])
    assert (rows[lane, n:] == 0xFFFFFFFF).all(), (cs["name"], lane)
    assert np.array_equal(fin[lane], E["final"]), (cs["name"], "lane", lane, "final state / tail", fin[lane], E["final"])
    assert np.array_equal(fin[lane], tfin[g]), (cs["name"], lane)
    return E, got, trows[g, :n]


@pytest.mark.parametrize("group", ["helpers", "states", "flags", "geometry", "shared", "integers"])
def test_words_states_and_tails(runs, group):
    """every lane of every case of the group: all words drawn, the state words after every step ({position | flags, head | unread}: the twist-ahead
    bookkeeping through every close and reopen), the final state and the eight words after the program equal stream (a) and the host twin — every
    copy of a shared state included, and the idle lanes' rows untouched"""
    cases, out = runs
    seen = 0
    for c, cs in enumerate(cases):
        if cs["group"] != group:
            continue
        seen += 1
        for lane in range(64):
            if lane in cs["lanes"]:
                E, got, twin = _check_lane(cs, c, lane, cs["lanes"][lane], out[c])
                assert np.array_equal(got, twin), (cs["name"], lane)
            else:
                assert (out[c][0][lane] == 0xFFFFFFFF).all() and (out[c][1][lane] == 0xFFFFFFFF).all(), (cs["name"], lane)
    assert seen


def test_bulk_bernoulli_in_teams(runs):
    """teams of 4 and of 16 copies in one wavefront, a different n each: the flags, the ballots handed to emit and the tail equal stream (a); the final
    state equals the host twin's; every lane's emit calls are the ones its rank gets, and no other"""
    cases, out = runs
    teams = 0
    for c, cs in enumerate(cases):
        if cs["group"] != "bulk":
            continue
        rows = out[c][0]
        for g, G in cs["gens"].items():
            lanes = [l for l in sorted(cs["lanes"]) if cs["lanes"][l] == g]
            assert lanes == P.team_lanes(lanes[0], G["copies"])
            E = P.expected(c, g)
            st = next(s for s in E["steps"] if s["kind"] == P.BULK)
            n = st["step"][1]
            want = P.bulk_ballots(G, E, st, lanes)
            for q, lane in enumerate(lanes):
                _check_lane(cs, c, lane, g, out[c], skip=(st["begin"], st["end"]))   # (the words around the bulk call, the states and the tail; the bulk step's words follow)
                seg = rows[lane, st["begin"]:st["end"]].reshape(-1, 3)
                bad = np.flatnonzero((seg != want[q]).any(axis=1))
                assert bad.size == 0, (cs["name"], "generator", g, "lane", lane, "rank", q, "n", n, G["bulk"], "first differing draws", bad[:5], seg[bad[:5]], want[q][bad[:5]])
            teams += 1
    assert teams >= 216


def test_bulk_bernoulli_equals_call_by_call(runs):
    """a lane on its own (MtTeamOne) beside the same program with one rng_bernoulli call after another, both on the device: the same flags, the same
    state after every step, the same final state and tail — and stream (a)'s"""
    cases, out = runs
    pairs = 0
    for c, cs in enumerate(cases):
        if cs["group"] != "bulk_one":
            continue
        rows, fin = out[c][0], out[c][1]
        for g in range(0, len(cs["gens"]), 2):
            Eb, gotb, _ = _check_lane(cs, c, g, g, out[c])
            Ec, gotc, _ = _check_lane(cs, c, g + 1, g + 1, out[c])
            sb, sc = Eb["steps"][2], Ec["steps"][2]
            seg = gotb[sb["begin"]:sb["end"]].reshape(-1, 3)
            assert np.array_equal(seg[:, 0], gotc[sc["begin"]:sc["end"]]), (cs["name"], g)
            assert np.array_equal(seg[:, 1], seg[:, 0]) and not seg[:, 2].any()
            assert np.array_equal(gotb[sb["end"]:], gotc[sc["end"]:]), (cs["name"], g, "the states after the bulk call")
            assert np.array_equal(fin[g], fin[g + 1]), (cs["name"], g)
            pairs += 1
    assert pairs == 108


def _orc(orc, seed, kind, a, b, n, out_n):
    a = None if a is None else np.ascontiguousarray(a, np.float64)
    b = None if b is None else np.ascontiguousarray(b, np.float64)
    res = np.zeros(max(out_n, 1))
    orc.l.orc_rng(seed, kind, None if a is None else _ptr(a), None if b is None else _ptr(b), n, _ptr(res))
    return res[:out_n]


def test_integer_distributions_equal_libstdcxx(runs, orc):
    """generate_canonical (one and two at a time), bernoulli, uniform_int over test_diag_cpu.py's ranges and std::shuffle of its lengths, every lane
    another one: exactly libstdc++'s"""
    cases, out = runs
    c = next(i for i, cs in enumerate(cases) if cs["name"] == "integers")
    seen = set()
    for g, G in cases[c]["gens"].items():
        ref = P.libstdcxx_integers(lambda *a: _orc(orc, *a), G)
        if ref is None:
            continue
        E = P.expected(c, g)
        got = P.payload(out[c][0][g], E)
        assert np.array_equal(got, ref), (g, G["steps"][0])
        seen.add((G["steps"][0][0], G["steps"][0][1]))
    assert {k for k, _ in seen} == {P.CANONICAL, P.CANONICAL2, P.BERNOULLI, P.UNIFORM_INT, P.SHUFFLE}
    assert {n for k, n in seen if k == P.SHUFFLE} == set(P.SHUFFLE_LENGTHS)


def test_normal_and_gamma_draws(runs, orc):
    """64 lanes, a seed each.  Stream position, exact: the raw word after every single draw is libstdc++'s, so every accept / reject decision was the
    reference's.  Values: within BOUND_ULPS of libstdc++'s (the device's log, sqrt and pow are not the host's)."""
    cases, out = runs
    c = next(i for i, cs in enumerate(cases) if cs["name"] == "normal_gamma")
    worst = {k: 0 for k in MEASURED_ULPS}
    for g, G in cases[c]["gens"].items():
        E = _check_lane(cases[c], c, g, g, out[c])[0]   # the raw words, the states, the tail
        values, raws = P.libstdcxx_normal_gamma(lambda *a: _orc(orc, *a), G)
        got = P.payload(out[c][0][g], E).reshape(-1, 3)
        assert np.array_equal(got[:, 2], raws), (g, "stream position differs from draw", np.flatnonzero(got[:, 2] != raws)[:1])
        dev = P.f64(got[:, :2].reshape(-1))
        assert np.isfinite(dev).all() and (np.sign(dev) == np.sign(values)).all()
        d = P.ulps(dev, values)
        at = 0
        for s in G["steps"]:
            k = "normal" if s[0] == P.NORMAL else ("gamma_lt1" if s[2] < 1.0 else "gamma_ge1")
            worst[k] = max(worst[k], int(d[at:at + s[1]].max()))
            at += s[1]
    print("largest distance to libstdc++ in ulps:", worst)
    for k, w in worst.items():
        assert w <= BOUND_ULPS[k], (k, w, BOUND_ULPS[k])


def test_screen_against_extended_precision(runs):
    """gamma_second_test_rejects on the grid and the literal cases: the device's decision is the extended-precision one wherever that is decidable in double"""
    cases, out = runs
    total = wrong = 0
    first = None
    for c, cs in enumerate(cases):
        if cs["group"] != "screen":
            continue
        for g, G in cs["gens"].items():
            _check_lane(cs, c, g, g, out[c])
            got = out[c][0][g, 0:3 * len(G["screen"]):3]
            for q, d in zip(G["screen"], got):
                if q["undecidable"]:
                    continue
                total += 1
                assert d in (0, 1)
                if bool(d) != q["rejects"]:
                    wrong += 1
                    first = first or q
    assert total >= 7700
    assert wrong == 0, (wrong, first)
