"""The count model's tables (host/CountDistribution.cpp, as count_model.build_luts and CountDistribution.tables() hand them to the sampler) against
the same distributions evaluated at 50 significant digits with mpmath:

  genomic table [s][m][c]   log NB(c; size * m, p), counts 0..254, multiplicities 1..32 (NB(size, p) of (mean, var), momentsToParameters)
  noise table   [s][c]      log Poisson(c; rate), counts 0..254
  entry 255 of both         log P(X >= 255): the reference folds the tail into the last count by iterating logAddition to convergence

Tolerance: 1e-12 relative where |value| >= 1, 1e-12 absolute elsewhere — with one stated widening for the NB table.  An NB log-pmf is a sum
of terms that cancel (lgamma(c + r) - lgamma(r) - lgamma(c + 1) + r log p + c log(1 - p), r = size * m); each is evaluated in double, so the sum
carries an error of about one ulp of the LARGEST term, not of the result.  Where r is large (var/mean near 1: size = mean^2 / (var - mean) is 99 at
mean 1 and 19 800 at mean 200) that floor exceeds 1e-12 of the value (measured: up to 1.8e-11 relative).  The bound checked for the NB table is
    |got - want| <= max(1e-12 * max(1, |want|), 4 eps * (sum of |terms|))
(measured: at most 1.5 eps * (sum of |terms|)), and the test asserts that the plain 1e-12 holds wherever size <= 30 (var/mean >= 2 on this
grid).  The folded tail at 255 adds the fold's own truncation: it stops once a term moves the sum by less than 100 eps relative (doubleCompare),
and the terms left out decrease geometrically, so up to ~100 eps |v| / (1 - ratio) more is allowed.  The Poisson table meets 1e-12 everywhere,
its tail included.  (At a rate of 300 the tail is log 0.9964 = -0.0036: the fold's "v > 0 -> 0" clamp does not fire on this grid.)"""
import numpy as np
import pytest

mpmath = pytest.importorskip("mpmath")
mp = mpmath.mp

EPS = np.finfo(np.float64).eps
REL = 1e-12


def nb_params(mean, var):
    """NegativeBinomialDistribution::momentsToParameters in double, as the host computes it"""
    if 0.99 < mean / var:
        var = mean / 0.99
    return mean / var, mean * mean / (var - mean)


def mp_nb_logpmf(p, r, nmax=255):
    """log NB(c; r, p) for c = 0..nmax-1 at 50 digits (the recurrence pmf(c) = pmf(c-1) (c - 1 + r)(1 - p) / c is exact to far below 1e-40 here)"""
    with mp.workdps(50):
        p, r = mp.mpf(p), mp.mpf(r)
        lq = mp.log(1 - p)
        out = [r * mp.log(p)]
        for c in range(1, nmax):
            out.append(out[-1] + mp.log((c - 1 + r) / c) + lq)
        return out


def mp_poisson_logpmf(rate, nmax=255):
    with mp.workdps(50):
        lam = mp.mpf(rate)
        out = [-lam]
        for c in range(1, nmax):
            out.append(out[-1] + mp.log(lam / c))
        return out


def mp_log_tail(logpmf_at, head):
    """log P(X >= 255) at 50 digits: 1 - P(X < 255) when that does not cancel, otherwise the series from 255 on (past the mode: decreasing terms)"""
    with mp.workdps(50):
        below = mp.fsum(mp.exp(x) for x in head)
        if below < mp.mpf("0.5"):
            return mp.log(1 - below)
        c, lt = 255, logpmf_at(255)
        total, term = mp.mpf(0), mp.exp(lt)
        while True:
            total += term
            c += 1
            lt = logpmf_at(c, lt)
            term = mp.exp(lt)
            if term < total * mp.mpf(10) ** -45:
                return mp.log(total)


def check(got, want, scale):
    """got / want: arrays; scale: the magnitude of the terms each double evaluation sums (0: no widening).  -> entries that needed the widening"""
    want = np.asarray(want, np.float64)
    tol_plain = REL * np.maximum(1.0, np.abs(want))
    tol = np.maximum(tol_plain, 4 * EPS * scale)
    err = np.abs(got - want)
    bad = err > tol
    assert not bad.any(), f"{bad.sum()} entries off, worst {err[bad].max()} at {np.argwhere(bad)[:3].tolist()} (tol {tol[bad][:3]})"
    return int((err > tol_plain).sum())


NB_GRID = [(m, vm) for m in (1.0, 7.5, 30.0, 200.0) for vm in (1.01, 2.0, 20.0)]


@pytest.mark.parametrize("mean,vm", NB_GRID)
def test_genomic_table_against_mpmath(mean, vm):
    """count_model.build_luts' genomic table, multiplicities 1..32, every count and the folded tail, against the 50-digit NB"""
    from math import lgamma, log

    from bayestyper_amd.host import count_model

    var = mean * vm
    lut_g, _ = count_model.build_luts(1, mean=mean, var=var, noise_rate=0.05)
    g = lut_g.reshape(256, 256)
    # multiplicity 0: count 0 is certain, any other count impossible (CountDistribution.cpp: genomicCountLogPmf)
    assert g[0, 0] == 0 and np.isneginf(g[0, 1:]).all()
    p, size = nb_params(mean, var)
    widened = []
    for m in range(1, 33):
        r = size * m
        want = mp_nb_logpmf(p, mp.mpf(size) * m)
        c = np.arange(255, dtype=np.float64)
        scale = np.abs([lgamma(x + r) for x in c]) + abs(lgamma(r)) + np.abs([lgamma(x + 1) for x in c]) + abs(log(p) * r) + np.abs(log(1 - p) * c)
        widened.append(check(g[m, :255], [float(x) for x in want], scale))

        def at(cc, prev=None, r=mp.mpf(size) * m):
            with mp.workdps(50):
                if prev is None:
                    return mp.loggamma(cc + r) - mp.loggamma(r) - mp.loggamma(cc + 1) + r * mp.log(p) + cc * mp.log(1 - mp.mpf(p))
                return prev + mp.log((cc - 1 + r) / cc) + mp.log(1 - mp.mpf(p))

        tail = float(mp_log_tail(at, want))
        # the fold's truncation (module docstring) + the cancellation floor of the terms at 255
        ratio = min(0.999, (1 - p) * (255 + r) / 256)   # pmf(c + 1) / pmf(c) at c = 255 (it only falls from there on past the mode)
        fold = 100 * EPS * abs(tail) / (1 - ratio) + 4 * EPS * (abs(lgamma(255 + r)) + abs(lgamma(r)) + lgamma(256) + abs(log(p) * r) + abs(log(1 - p)) * 255)
        assert abs(g[m, 255] - tail) <= max(REL * max(1.0, abs(tail)), fold), (m, g[m, 255], tail)
        assert g[m, 255] <= 0
    # the widening is the exception: it is needed only where size is large
    if size <= 30:
        assert sum(widened) == 0, widened


@pytest.mark.parametrize("rate", [1e-6, 1e-3, 0.05, 1.0, 10.0, 100.0, 254.0, 300.0])
def test_noise_table_against_mpmath(rate):
    """the Poisson noise table (counts 0..254 and the folded tail at 255) of build_luts and of CountDistribution.tables() after setNoiseRates"""
    from bayestyper_amd.host import count_model

    _, lut_n = count_model.build_luts(1, noise_rate=rate)
    cd = count_model.CountDistribution(2)
    cd.set_noise_rates([rate, rate])
    _, lut_n2 = cd.tables()
    cd.close()
    assert np.array_equal(lut_n2.reshape(2, 256)[0], lut_n) and np.array_equal(lut_n2.reshape(2, 256)[1], lut_n)
    want = mp_poisson_logpmf(rate)
    assert check(lut_n[:255], [float(x) for x in want], 0.0) == 0

    def at(cc, prev=None):
        with mp.workdps(50):
            if prev is None:
                return cc * mp.log(rate) - rate - mp.loggamma(cc + 1)
            return prev + mp.log(mp.mpf(rate) / cc)

    tail = float(mp_log_tail(at, want))
    got = lut_n[255]
    assert got <= 0
    assert abs(got - tail) <= REL * max(1.0, abs(tail)), (rate, got, tail)


def test_tables_of_a_count_distribution_match_the_builder():
    """CountDistribution.tables() with per-sample moments (setGenomicFromMoments) gives what build_luts gives for the same parameters"""
    from bayestyper_amd.host import count_model

    cd = count_model.CountDistribution(3)
    params = [(15.0, 30.0, 0.05), (200.0, 202.0, 1e-6), (1.0, 20.0, 300.0)]
    for s, (mean, var, _) in enumerate(params):
        cd.set_genomic(s, mean, var)
    cd.set_noise_rates([x[2] for x in params])
    g, n = cd.tables()
    cd.close()
    for s, (mean, var, rate) in enumerate(params):
        g1, n1 = count_model.build_luts(1, mean=mean, var=var, noise_rate=rate)
        assert np.array_equal(g.reshape(3, 65536)[s], g1) and np.array_equal(n.reshape(3, 256)[s], n1)
