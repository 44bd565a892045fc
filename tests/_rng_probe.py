"""The case corpus of the generator probe (bt_rng_probe / bt_diag_rng_probe), and what it must give.

Three statements of the expected values that share no code: (a) the textbook mt19937 stream from numpy, walked by the Python models below (ring bookkeeping,
Lemire's uniform_int, std::shuffle, the polar normal and Marsaglia-Tsang's gamma in extended precision); (b) libstdc++ through the oracle's orc_rng; (c) the
host twin.  tests/test_rng_probe_cpu.py asserts that they agree and that the corpus reaches what it is meant to reach; tests/test_rng_probe_gpu.py compares
the device with them."""
import functools

import numpy as np

(DRAW, TOPUP, REOPEN, CANONICAL, CANONICAL2, UNIFORM_INT, BERNOULLI, SHUFFLE, NORMAL, GAMMA, BULK, DIRECT, SCREEN) = range(13)
HBM, LDS, LDS_FLAT = range(3)
MT_N, MT_AHEAD = 624, 312
F_CUR, F_READY = 1 << 16, 1 << 17
DISCARDS = [0, 1, 3, 311, 312, 313, 620, 623, 624, 625, 935, 1247, 1248]
UINT_RANGES = [a + 1 for a in (0, 1, 2, 6, 9, 99, 1000, 65535, 2 ** 31 - 2, 3 * 2 ** 29)]   # test_diag_cpu.py's
SHUFFLE_LENGTHS = [0, 1, 2, 3, 10, 11, 110, 441]
MARGIN = 1e-9   # no decision of the normal / gamma corpus lies relatively closer to its boundary
LD = np.longdouble


@functools.lru_cache(maxsize=None)
def stream(seed, n=16384):
    """(a): std::mt19937(seed)'s first n words"""
    m = np.random.MT19937()
    m._legacy_seeding(seed)
    return m.random_raw(n).astype(np.uint32)


def canonical(w0, w1):
    r = (float(w0) + float(w1) * 4294967296.0) / 18446744073709551616.0
    return r if r < 1.0 else float(np.nextafter(1.0, 0.0))


class Ring:
    """bookkeeping of a block-form ring generator (no words): where its reads, refills, block ends and twists fall"""

    def __init__(self, cap):
        self.cap, self.pos, self.cur, self.ready, self.head, self.avail, self.ix = cap, MT_N, 0, 0, 0, 0, 0
        self.events, self.ctx = [], None

    def ev(self, what):
        self.events.append((what, self.ctx))

    def block_end(self):
        self.ev("flip" if self.ready else "twist")
        self.cur ^= 1
        self.ready = 0
        self.pos = 0

    def fill_to(self, want):
        while self.avail < want:
            if self.pos == MT_N:
                self.block_end()
            self.pos += 4
            self.avail += 4

    def take(self, n):
        if self.avail < n:
            self.ev("fill")
            self.fill_to(min(self.cap - 3, 16))
        if self.head + n >= self.cap:
            self.ev("wrap")
        self.head = (self.head + n) % self.cap
        self.avail -= n
        self.ix += n
        return self.ix - n

    def draw(self, n, ctx):
        """n reads of one word; the event context of read i is ctx + (i,)"""
        for i in range(n):
            if self.avail and self.head + 1 < self.cap:
                self.head += 1
                self.avail -= 1
                self.ix += 1
            else:
                self.ctx = ctx + (i,)
                self.take(1)

    def topup(self):
        self.ev("topup@%d" % self.pos)
        if self.pos >= MT_AHEAD and not self.ready:
            self.ready = 1
            self.ev("ahead")
        want = self.cap - 3
        if self.avail < want:
            if self.pos == MT_N:
                self.block_end()
            nc = min((want - self.avail + 3) // 4, 4, (MT_N - self.pos) // 4)
            self.pos += 4 * nc
            self.avail += 4 * nc
        self.fill_to(want)

    def state(self):
        return self.pos, self.cur * F_CUR | self.ready * F_READY, self.head, self.avail


class Reader:
    """a ring model with the stream's words behind it"""

    def __init__(self, seed, cap):
        self.words, self.ring = stream(seed), Ring(cap)

    def take(self, n):
        at = self.ring.take(n)
        return [int(w) for w in self.words[at:at + n]]

    def next(self):
        return self.take(1)[0]

    def canonical(self):
        return canonical(*self.take(2))

    def uniform_int(self, rng):
        product = self.next() * rng
        low = product & 0xFFFFFFFF
        if low < rng:
            threshold = (2 ** 32 - rng) % rng
            while low < threshold:
                product = self.next() * rng
                low = product & 0xFFFFFFFF
        return product >> 32

    def shuffle(self, n):
        a = list(range(n))
        if n == 0:
            return a
        assert 0xFFFFFFFF // n >= n
        i = 1
        if n % 2 == 0:
            j = self.uniform_int(2)
            a[i], a[j] = a[j], a[i]
            i += 1
        while i != n:
            b1 = i + 2
            x = self.uniform_int((i + 1) * b1)
            p0, p1 = x // b1, x % b1
            a[i], a[p0] = a[p0], a[i]
            i += 1
            a[i], a[p1] = a[p1], a[i]
            i += 1
        return a


class Dist:
    """normal_distribution / gamma_distribution on a Reader, in extended precision, recording how close every decision came to its boundary"""

    def __init__(self, reader):
        self.r, self.saved, self.margins = reader, None, {"r2": np.inf, "v": np.inf, "first": np.inf, "second": np.inf}

    def near(self, which, a, b):
        scale = max(abs(a), abs(b))
        if scale > 0:
            self.margins[which] = min(self.margins[which], float(abs(a - b) / scale))

    def normal(self):
        if self.saved is not None:
            ret, self.saved = self.saved, None
            return ret
        while True:
            w = self.r.take(4)
            x, y = LD(2.0 * canonical(w[0], w[1]) - 1.0), LD(2.0 * canonical(w[2], w[3]) - 1.0)
            r2 = x * x + y * y
            self.near("r2", r2, LD(1))
            if not (r2 > 1 or r2 == 0):
                break
        mult = np.sqrt(-2 * np.log(r2) / r2)
        self.saved = x * mult
        return y * mult

    def gamma(self, alpha, beta):
        malpha = alpha + 1.0 if alpha < 1.0 else alpha
        a1 = malpha - 1.0 / 3.0
        a2 = 1.0 / np.sqrt(9.0 * a1)
        while True:
            while True:
                n = self.normal()
                v = 1 + LD(a2) * n
                self.near("v", LD(1), -LD(a2) * n)
                if v > 0:
                    break
            v = v * v * v
            u = LD(self.r.canonical())
            t = 1 - LD(0.0331) * n * n * n * n
            self.near("first", u, t)
            if not u > t:
                break
            lhs, rhs = np.log(u), LD(0.5) * n * n + LD(a1) * (1 - v + np.log(v))
            self.near("second", lhs, rhs)
            if not lhs > rhs:
                break
        if alpha == malpha:
            return LD(a1) * v * LD(beta)
        while True:
            u = self.r.canonical()
            if u != 0.0:
                break
        return np.power(LD(u), 1 / LD(alpha)) * LD(a1) * v * LD(beta)


# ---- the corpus -------------------------------------------------------------------------------------------------------------------------------------


def gen(seed, steps, discard=0, cap=32, place=HBM, copies=1):
    return dict(seed=seed, discard=discard, cap=cap, place=place, copies=copies, steps=[tuple(s) + (0.0,) * (6 - len(s)) for s in steps])


def case(name, group, lanes, gens):
    """lanes: {lane: generator index}; gens: {generator index: gen(...)}"""
    return dict(name=name, group=group, lanes=dict(lanes), gens=dict(gens))


def team_lanes(first, copies):
    return [first % (64 // copies) + k * (64 // copies) for k in range(copies)]


HELPER_MASKS = [("k%d" % k, list(range(k))) for k in (1, 2, 3, 56, 57, 58, 63, 64)] + [("every_other", list(range(0, 64, 2))), ("upper_half", list(range(32, 64))), ("lane63", [63])]


def _draw_topup_program(j, cap):
    steps = []
    for r in range(6):
        steps += [(TOPUP, 0), (DRAW, 1 + (5 * j + 7 * r) % (cap - 3))]
    steps += [(DRAW, 300 + 3 * (j % 11)), (TOPUP, 0), (DRAW, 3), (REOPEN, 0), (DRAW, 2 * cap + j % 5)]
    return steps


def _bulk_setups():
    """(discard, draws after the top-up, ring cap) -> the ring's unread count a0 before the bulk call and whether the next block is ready"""
    out = []
    for ready in (0, 1):
        for odd in (0, 1):
            for cap in (8, 16, 32, 64):
                for discard in ((320, 333) if ready else (100, 17)):
                    for r in (3, 4):
                        m = Ring(cap)
                        for _ in range(discard):
                            m.take(1)
                        m.topup()
                        for _ in range(r):
                            m.take(1)
                        if m.avail % 2 == odd and m.ready == ready:
                            out.append(dict(discard=discard, r=r, cap=cap, a0=m.avail, ready=ready))
    return out


def _bulk_programs():
    """every n of the issue's list x a0 odd / even x next block ready or not x p, the ring caps taken in turn"""
    setups = _bulk_setups()
    progs, i = [], 0
    for ready in (0, 1):
        for odd in (0, 1):
            mine = [s for s in setups if s["ready"] == ready and s["a0"] % 2 == odd]
            assert mine
            for p in (0.0, 0.1, 1.0):
                for which in range(9):
                    s = mine[i % len(mine)]
                    i += 1
                    n = [0, 1, s["a0"] // 2, s["a0"] // 2 + 1, 7, 311, 312, 313, 700][which]
                    progs.append(dict(s, n=n, p=p, seed=7000 + i))
    return progs


def _bulk_gen(pr, kind, copies, place=HBM):
    return gen(pr["seed"], [(TOPUP, 0), (DRAW, pr["r"]), (kind, pr["n"], pr["p"]), (DRAW, 5)], discard=pr["discard"], cap=pr["cap"], place=place, copies=copies)


def _float_shapes():
    """the noise chain's gamma arguments, computed in float as noise_update_kernel does: shape = prior + count sum, scale = prior / (observations * prior + 1)"""
    out = []
    for prior_shape, prior_scale, count_sum, obs in ((1.0, 1.0, 9876543, 9999999), (0.5, 2.5, 123457, 600000), (2.0, 0.01, 1234, 99999), (1.0, 1e-7, 10 ** 7, 3 * 10 ** 6)):
        shape = np.float32(prior_shape) + np.float32(count_sum)
        scale = np.float32(prior_scale) / (np.float32(obs) * np.float32(prior_scale) + np.float32(1.0))
        out.append((float(shape), float(scale)))
    return out


GAMMA_SHAPES = [1.0, 2.0, 3.0, 11.0, 21.0, 250.0, 0.5, 0.25]
GAMMA_SCALES = [1.0, 0.01, 2.5, 1e-7]
NG_DRAWS = 60   # per step; four steps a lane


def _ng_steps(j):
    """lane j of the normal / gamma case: lanes 0 .. 7 draw normals, the others gammas of four (shape, scale) pairs"""
    if j < 8:
        return [(NORMAL, NG_DRAWS, 0.0, 0.0, 1.0)] * 4
    pairs = [(a, b) for a in GAMMA_SHAPES for b in GAMMA_SCALES] + _float_shapes() * 2
    return [(GAMMA, NG_DRAWS) + pairs[(4 * j + q * 9) % len(pairs)] + (1.0,) for q in range(4)]


def ng_margins(seed, steps):
    r = Reader(seed, 32)
    d = Dist(r)
    for s in steps:
        for _ in range(s[1]):
            d.normal() if s[0] == NORMAL else d.gamma(s[2], s[3])
            r.next()
    return d.margins


@functools.lru_cache(maxsize=None)
def ng_seed(j):
    """the first seed from 5000 + 100 j on whose decisions all keep the margin (section 4 of the issue: 'if a seed violates this, choose another')"""
    seed = 5000 + 100 * j
    while min(ng_margins(seed, _ng_steps(j)).values()) <= MARGIN:
        seed += 1
    return seed


def screen_cases():
    """(u, n, v, a1) of the screen grid and its literal cases, with the extended-precision decision and margin of each -> list of dicts"""
    import mpmath as mp

    mp.mp.prec = 200
    top, tiny = float(np.nextafter(1.0, 0.0)), float(np.nextafter(0.0, 1.0))
    ns = [0.0, 0.5, -0.5, 2.3, -2.3, 2.4, -2.4, 6.0, -6.0]
    vs = [1e-30, 1e-12, 0.3, 0.999999, 1.0, 1.000001, 3.0, 50.0, 1e6]
    a1s = [2.0 / 3.0, 5.0 / 3.0, 20.67, 249.67, 1e4, 1e7]
    deltas = [1e-2, 1e-3, 1e-4, 3e-5, 1e-5, 1e-6, 1e-8, 1e-10]

    def rhs_of(n, v, a1):
        return mp.mpf(0.5) * mp.mpf(n) ** 2 + mp.mpf(a1) * (1 - mp.mpf(v) + mp.log(mp.mpf(v)))

    quads = []
    for n in ns:
        for v in vs:
            for a1 in a1s:
                e = mp.exp(rhs_of(n, v, a1))
                for dl in deltas:
                    for sign in (1, -1):
                        quads.append((min(max(float(e * (1 + sign * mp.mpf(dl))), tiny), top), n, v, a1))
    for u in (0.0, 2.0 ** -64, 0.5, top):
        for n, v, a1 in ((0.5, 0.3, 2.0 / 3.0), (2.3, 1.000001, 20.67), (0.0, 3.0, 5.0 / 3.0)):
            quads.append((u, n, v, a1))
    for v in (1e-50, 1e-40):   # float(v) is zero; float(v) is denormal
        assert float(np.float32(v)) == 0.0 or 0.0 < float(np.float32(v)) < float(np.finfo(np.float32).tiny)
        for u in (0.5, 1e-3, top):
            quads.append((u, 1.0, v, 2.0 / 3.0))
    out = []
    for u, n, v, a1 in quads:
        rhs = rhs_of(n, v, a1)
        lhs = mp.log(mp.mpf(u)) if u > 0 else mp.mpf("-inf")
        big = max(abs(float(lhs)), abs(float(rhs)))
        ulp = float(np.spacing(big)) if np.isfinite(big) else 0.0
        margin = abs(lhs - rhs)
        # the single-precision screen's own sides and bound (bt_rng_device.hpp: gamma_second_test_rejects), in exact arithmetic: inside or outside `err`
        fu, fv = float(np.float32(u)), float(np.float32(v))
        inside = None
        if fu > 0 and fv > 0:
            lu, lv = mp.log(mp.mpf(fu)), mp.log(mp.mpf(fv))
            diff = lu - (mp.mpf(0.5) * mp.mpf(n) ** 2 + mp.mpf(a1) * (1 - mp.mpf(v) + lv))
            inside = bool(abs(diff) <= mp.mpf(4e-5) * ((1 + abs(lu)) + mp.mpf(a1) * (1 + abs(lv))))
        out.append(dict(u=u, n=n, v=v, a1=a1, rejects=bool(lhs > rhs), undecidable=bool(margin < 64 * ulp), inside=inside))
    return out


@functools.lru_cache(maxsize=None)
def corpus():
    cases = []
    # -- cooperative twist under every helper count: the drawer at the first active lane, 700 words
    for tag, lanes in HELPER_MASKS:
        # (A) the helpers draw nothing: the block ends fall in the top-ups, where every active lane is present
        steps_d, steps_h = [], []
        for r in range(12):
            steps_d += [(TOPUP, 0), (DRAW, 59 if r < 11 else 51)]
            steps_h += [(TOPUP, 0), (DRAW, 0)]
        gens = {i: gen(100 + i, steps_h if i else steps_d, cap=64) for i in range(len(lanes))}
        cases.append(case("helpers_topup_" + tag, "helpers", {l: i for i, l in enumerate(lanes)}, gens))
        # (B) every lane draws 700 words in its own loop; the rings refill in the same iterations (discards are multiples of 16) and the block ends differ
        gens = {i: gen(200 + i, [(DRAW, 700)], discard=16 * ((7 * i) % 39), cap=64) for i in range(len(lanes))}
        cases.append(case("helpers_draw_" + tag, "helpers", {l: i for i, l in enumerate(lanes)}, gens))
    # -- many distinct states
    for place in (HBM, LDS):
        gens = {j: gen(300 + j, [(DRAW, 650 + (37 * j) % 60)], discard=DISCARDS[j % len(DISCARDS)], cap=32, place=place) for j in range(64)}
        cases.append(case("many_states_%d" % place, "states", {j: j for j in range(64)}, gens))
    # -- twist-ahead and flags: top-ups below, at and above MT_AHEAD, close and reopen between every pair of steps
    for cap, place in ((32, HBM), (16, LDS), (64, LDS_FLAT)):
        gens = {}
        for j in range(64):
            body = [(TOPUP, 0), (DRAW, 1 + j % 13), (TOPUP, 0), (DRAW, cap - 3), (TOPUP, 0), (DRAW, 280 + 5 * (j % 9) + (70 if j % 5 == 0 else 0)), (TOPUP, 0), (DRAW, 40 + j), (TOPUP, 0), (DRAW, 10)]
            steps = []
            for s in body:
                steps += [s, (REOPEN, 0)]
            gens[j] = gen(400 + j, steps, discard=260 + j + (j % 4) * 3, cap=cap, place=place)
        cases.append(case("flags_%d_%d" % (cap, place), "flags", {j: j for j in range(64)}, gens))
    # -- ring geometry: draws and top-ups at every cap, in HBM and in LDS (behind both pointer types)
    for cap in (8, 16, 32, 64):
        for place in (HBM, LDS, LDS_FLAT):
            gens = {j: gen(500 + j, _draw_topup_program(j, cap), discard=DISCARDS[(j + cap) % len(DISCARDS)], cap=cap, place=place) for j in range(64)}
            cases.append(case("geometry_%d_%d" % (cap, place), "geometry", {j: j for j in range(64)}, gens))
    # -- shared states: the lockstep copies of a generator
    for copies in (4, 16, 2, 8, 32):
        for place in (HBM, LDS):
            width, lanes, gens = 64 // copies, {}, {}
            for g in range(width):
                cap = (8, 16, 32, 64)[g % 4]
                gens[g] = gen(600 + g, _draw_topup_program(g, cap) + [(DRAW, 700)], discard=DISCARDS[(g + copies) % len(DISCARDS)], cap=cap, place=place, copies=copies)
                for l in team_lanes(g, copies):
                    lanes[l] = g
            cases.append(case("shared_%d_%d" % (copies, place), "shared", lanes, gens))
    # -- bulk Bernoulli: two teams of 16 and eight teams of 4 share a wavefront; the call-by-call form of every program on lanes of their own
    progs = _bulk_programs()
    firsts = [(0, 16), (1, 16)] + [(f, 4) for f in (2, 3, 6, 7, 10, 11, 14, 15)]
    for copies_of in (4, 16):
        todo = list(progs)
        others = list(reversed(progs))
        c = 0
        while todo:
            lanes, gens = {}, {}
            for g, (first, copies) in enumerate(firsts):
                pr = (todo.pop(0) if todo else progs[g]) if copies == copies_of else others[(c * 10 + g) % len(others)]
                gens[g] = _bulk_gen(pr, BULK, copies, place=(HBM, LDS)[c % 2])
                gens[g]["bulk"] = pr
                for l in team_lanes(first, copies):
                    lanes[l] = g
            cases.append(case("bulk_%d_%d" % (copies_of, c), "bulk", lanes, gens))
            c += 1
    for c in range(0, len(progs), 32):   # a lane on its own: MtTeamOne (even generators) beside the call-by-call form (odd ones)
        gens = {}
        for i, pr in enumerate(progs[c:c + 32]):
            gens[2 * i] = _bulk_gen(pr, BULK, 1)
            gens[2 * i]["bulk"] = pr
            gens[2 * i + 1] = _bulk_gen(pr, BERNOULLI, 1)
        cases.append(case("bulk_one_%d" % c, "bulk_one", {j: j for j in gens}, gens))
    # -- integer and uniform distributions, every lane another one
    gens = {}
    for j in range(64):
        kind = j % 8
        if kind == 0:
            steps = [(CANONICAL, 300)]
        elif kind == 1:
            steps = [(CANONICAL2, 150)]
        elif kind == 2:
            steps = [(BERNOULLI, 300, float(np.float32(0.1)))]
        elif kind == 3:
            steps = [(UNIFORM_INT, 12, float(UINT_RANGES[(j // 8 + q) % len(UINT_RANGES)])) for q in range(30)]
        elif kind == 4:
            steps = [(SHUFFLE, SHUFFLE_LENGTHS[j // 8])]
        elif kind == 5:
            steps = [(DIRECT, 128, 1.0), (DIRECT, 256, 2.0), (DIRECT, 256, 4.0), (DIRECT, 3, 1.0), (DIRECT, 640, 4.0), (DIRECT, 2, 2.0), (DRAW, 20)]
        elif kind == 6:   # a mixture: every distribution on one stream, the ring's refills wherever they fall
            steps = [(UNIFORM_INT, 7, 3.0 * 2 ** 29 + 1), (CANONICAL, 5), (SHUFFLE, 110), (TOPUP, 0), (BERNOULLI, 9, 0.5), (CANONICAL2, 3), (SHUFFLE, 11), (DRAW, 9), (UNIFORM_INT, 40, 7.0)]
        else:
            steps = [(SHUFFLE, SHUFFLE_LENGTHS[(j // 8 + 3) % 8]), (SHUFFLE, SHUFFLE_LENGTHS[(j // 8 + 6) % 8]), (UNIFORM_INT, 50, 2.0 ** 31 - 1)]
        gens[j] = gen(800 + j, steps, cap=(8, 16, 32, 64)[(j // 8) % 4], place=(HBM, LDS)[(j // 32) % 2], discard=0 if kind < 5 else DISCARDS[j % len(DISCARDS)])
    cases.append(case("integers", "integers", {j: j for j in range(64)}, gens))
    # -- normal and gamma draws: 64 lanes, a seed each
    gens = {j: gen(ng_seed(j), _ng_steps(j), cap=(16, 32, 64)[j % 3], place=(HBM, LDS)[j % 2]) for j in range(64)}
    cases.append(case("normal_gamma", "normal_gamma", {j: j for j in range(64)}, gens))
    # -- the screen: 64 calls a lane
    sc = screen_cases()
    for c in range(0, len(sc), 4096):
        gens = {}
        for j in range(64):
            mine = sc[c + 64 * j:c + 64 * (j + 1)]
            if mine:
                gens[j] = gen(1, [(SCREEN, 0, q["u"], q["n"], q["v"], q["a1"]) for q in mine], cap=8)
                gens[j]["screen"] = mine
        cases.append(case("screen_%d" % c, "screen", {j: j for j in gens}, gens))
    return cases


def step_words(s):
    kind, n, raw = s[0], s[1], 1 if s[4] != 0.0 else 0
    return {DRAW: n, UNIFORM_INT: n, BERNOULLI: n, SHUFFLE: n, DIRECT: n, CANONICAL: 2 * n, CANONICAL2: 4 * n, NORMAL: (2 + raw) * n, GAMMA: (2 + raw) * n, BULK: 3 * n, SCREEN: 1}.get(kind, 0) + 2


def pack(cases):
    """-> lane_gen [n][64], gens [n][64], steps, row_cap for lib.rng_probe"""
    from bayestyper_amd import lib

    lane_gen = np.full((len(cases), 64), -1, np.int32)
    gens = np.zeros((len(cases), 64), lib.PROBE_GEN)
    steps, row_cap = [], 1
    for c, cs in enumerate(cases):
        for l, g in cs["lanes"].items():
            lane_gen[c, l] = g
        for g, G in cs["gens"].items():
            gens[c, g] = (G["seed"], G["discard"], G["cap"], G["place"], len(steps), len(G["steps"]), G["copies"], 0)
            steps += G["steps"]
            row_cap = max(row_cap, sum(step_words(s) for s in G["steps"]))
    return lane_gen, gens, np.array(steps, lib.PROBE_STEP), row_cap


def f64(words):
    return np.ascontiguousarray(words, np.uint32).view(np.uint64).view(np.float64)


def ulps(x, y):
    """distance of two arrays of finite doubles of equal sign in units in the last place"""
    a, b = np.ascontiguousarray(x, np.float64).view(np.int64), np.ascontiguousarray(y, np.float64).view(np.int64)
    return np.abs(a - b)


def expect(G):
    """model (a) of one generator's program -> dict: row (uint32, what the model knows), known (bool per word), final [12], events, and per step the slices a
    test needs.  NORMAL / GAMMA values are marked unknown (they come from (b)); their raw words and the stream position are the model's."""
    r = Reader(G["seed"], G["cap"])
    ring = r.ring
    ring.draw(G["discard"], ("discard",))
    row, known, steps = [], [], []
    dist = Dist(r)
    direct_at = 0

    def put(v, k=True):
        row.append(int(v) & 0xFFFFFFFF)
        known.append(k)

    def put_d(x, k=True):
        b = int(np.float64(x).view(np.uint64))
        put(b, k)
        put(b >> 32, k)

    for si, s in enumerate(G["steps"]):
        kind, n = s[0], s[1]
        begin = len(row)
        before = ring.state()
        ring.ctx = (si, kind, 0)
        if kind == DRAW:
            at = ring.ix
            ring.draw(n, (si, kind))
            for w in r.words[at:at + n]:
                put(w)
        elif kind == TOPUP:
            ring.topup()
        elif kind == CANONICAL:
            for i in range(n):
                put_d(r.canonical())
        elif kind == CANONICAL2:
            for i in range(n):
                w = r.take(4)
                put_d(canonical(w[0], w[1]))
                put_d(canonical(w[2], w[3]))
        elif kind == UNIFORM_INT:
            for i in range(n):
                put(r.uniform_int(int(s[2])))
        elif kind == BERNOULLI:
            for i in range(n):
                put(1 if r.canonical() < s[2] else 0)
        elif kind == SHUFFLE:
            for v in r.shuffle(n):
                put(v)
        elif kind in (NORMAL, GAMMA):
            for i in range(n):
                put_d(float(dist.normal() if kind == NORMAL else dist.gamma(s[2], s[3])), False)
                if s[4] != 0.0:
                    put(r.next())
        elif kind == BULK:
            ends = sum(1 for e in ring.events if e[0] in ("flip", "twist"))
            for i in range(n):
                put(1 if r.canonical() < s[2] else 0)
                put(0, False)
                put(0, False)
            ring.ev("bulk_blocks=%d" % (sum(1 for e in ring.events if e[0] in ("flip", "twist")) - ends))
        elif kind == DIRECT:
            for w in stream(G["seed"])[direct_at:direct_at + n]:
                put(w)
            direct_at += n
        elif kind == SCREEN:
            put(0, False)
        st = ring.state()
        put(st[0] | st[1])
        put(st[2] | st[3] << 16)
        steps.append(dict(kind=kind, begin=begin, end=len(row) - 2, before=before, step=s))
    final = list(ring.state())
    ring.ctx = ("tail", 0)
    final += [r.next() for _ in range(8)]
    return dict(row=np.array(row, np.uint32), known=np.array(known, bool), final=np.array(final, np.uint32), events=ring.events, steps=steps, margins=dist.margins)


def bulk_ballots(G, E, st, lanes):
    """what rng_bernoulli_bulk hands to emit in a team of `copies` lanes, from the model's flags: draw i is taken by the lane of rank (i - lo) % copies of
    its block's run of draws [lo, hi) — a draw belongs to the block of its SECOND word — and a ballot holds the selected lanes of one step of `copies`
    consecutive draws.  emit runs on every lane of the team in every step: in a run's last step the ranks beyond its last draw get an index past the run
    with `selected` false (the caller ignores it; the probe records it when the index is below n, and the draw's own lane overwrites nothing of it: the rows
    are per lane) -> per rank, the [n][3] words {flag, ballot low, ballot high} its row holds (0xFFFFFFFF where emit never ran on it)"""
    n, copies = st["step"][1], G["copies"]
    flags = E["row"][st["begin"]:st["end"]:3]
    pos, _, _, a0 = st["before"]
    rows = np.full((copies, n, 3), 0xFFFFFFFF, np.uint32)
    lo, k = 0, 0
    while lo < n:
        hi = min(n, (a0 + MT_N * (k + 1) - pos) // 2)   # draws whose second word 2i + 1 lies before the end of block k: 2i + 1 < a0 + 624 (k + 1) - pos
        for base in range(lo, hi, copies):
            b = 0
            for q in range(min(copies, hi - base)):
                if flags[base + q]:
                    b |= 1 << lanes[q]
            for q in range(copies):
                if base + q < n:
                    rows[q, base + q] = (int(flags[base + q]) if base + q < hi else 0, b & 0xFFFFFFFF, b >> 32)
        lo, k = max(lo, hi), k + 1
    return rows


@functools.lru_cache(maxsize=None)
def expected(c, g):
    return expect(corpus()[c]["gens"][g])


def payload(row, E):
    """a row without the state words after every step"""
    return np.concatenate([row[st["begin"]:st["end"]] for st in E["steps"]])


def _words_of(doubles):
    return np.ascontiguousarray(doubles, np.float64).view(np.uint32)


def libstdcxx_integers(orc, G):
    """(b) for a generator that runs ONE distribution from the start of its stream: the row's words without the state words (None for any other program);
    orc(seed, kind, a, b, n, out_n) -> doubles"""
    kinds = {s[0] for s in G["steps"]}
    if G["discard"] or len(kinds) != 1:
        return None
    kind, n = kinds.pop(), sum(s[1] for s in G["steps"])
    if kind == CANONICAL:
        return _words_of(orc(G["seed"], 1, None, None, n, n))
    if kind == CANONICAL2:
        return _words_of(orc(G["seed"], 1, None, None, 2 * n, 2 * n))
    if kind == BERNOULLI and len(G["steps"]) == 1:
        return orc(G["seed"], 4, [G["steps"][0][2]], None, n, n).astype(np.uint32)
    if kind == UNIFORM_INT:
        a = np.concatenate([np.full(s[1], s[2] - 1.0) for s in G["steps"]])
        return orc(G["seed"], 3, a, None, n, n).astype(np.uint32)
    if kind == SHUFFLE and len(G["steps"]) == 1:
        return orc(G["seed"], 5, [float(n)], None, 0, n).astype(np.uint32)
    return None


def libstdcxx_normal_gamma(orc, G):
    """(b) for a lane of the normal / gamma case -> (values, the raw word after each)"""
    kinds = {s[0] for s in G["steps"]}
    assert len(kinds) == 1 and not G["discard"] and all(s[4] != 0.0 for s in G["steps"])
    n = sum(s[1] for s in G["steps"])
    if kinds == {NORMAL}:
        out = orc(G["seed"], 6, None, None, n, 2 * n)
    else:
        a = np.concatenate([np.full(s[1], s[2]) for s in G["steps"]])
        b = np.concatenate([np.full(s[1], s[3]) for s in G["steps"]])
        out = orc(G["seed"], 7, a, b, n, 2 * n)
    return out[0::2].copy(), out[1::2].astype(np.uint32)


@functools.lru_cache(maxsize=None)
def census():
    cen = dict(block_end_single_lane=0, block_end_all_64=0, flip_without_twist=0, twist_at_block_end=0, bulk_two_blocks=0, wrap_caps=set(), helper_counts=set(),
               topup_positions=set(), topup_mixed_wants=0, flags_flip=0, flags_twist=0, bulk_copies=set(), shared_copies=set())
    combos = set()
    for c, cs in enumerate(corpus()):
        holders = {}
        for l, g in cs["lanes"].items():
            holders.setdefault(g, []).append(l)
        present, ends, ahead = {}, [], {}
        for g, G in cs["gens"].items():
            E = expected(c, g)
            for what, ctx in E["events"]:
                if what == "fill" or what.startswith("topup@"):
                    present.setdefault(ctx, set()).update(holders[g])
                if what.startswith("topup@") and cs["group"] == "flags":
                    cen["topup_positions"].add(int(what[6:]))
                if what in ("twist", "flip"):
                    ends.append((what, ctx, g))
                if what == "ahead":
                    ahead.setdefault(ctx, set()).update(holders[g])
                if what == "wrap":
                    cen["wrap_caps"].add(G["cap"])
                if what.startswith("bulk_blocks=") and int(what[12:]) >= 2:
                    cen["bulk_two_blocks"] += 1
            if cs["group"] == "shared":
                cen["shared_copies"].add(G["copies"])
            if cs["group"] == "bulk" and "bulk" in G:
                pr = G["bulk"]
                st = next(s for s in E["steps"] if s["kind"] == BULK)
                assert st["before"][3] == pr["a0"] and bool(st["before"][1] & F_READY) == bool(pr["ready"])
                combos.add((G["copies"], pr["seed"]))
                cen["bulk_copies"].add(G["copies"])
        for what, ctx, g in ends:
            lanes = present.get(ctx)
            if lanes is None or ctx[0] != "discard" and ctx[1] not in (DRAW, TOPUP):
                continue
            cen["block_end_single_lane"] += len(lanes) == 1
            cen["block_end_all_64"] += len(lanes) == 64
            cen["flip_without_twist"] += what == "flip"
            cen["twist_at_block_end"] += what == "twist"
            if what == "twist" and cs["group"] == "helpers":
                cen["helper_counts"].add(len(lanes))
            if cs["group"] == "flags" and ctx[0] != "discard" and ctx[1] == DRAW:
                cen["flags_flip"] += what == "flip"
                cen["flags_twist"] += what == "twist"
        for ctx, lanes in ahead.items():
            if cs["group"] == "helpers":
                cen["helper_counts"].add(len(present[ctx]))
            if cs["group"] == "flags" and lanes != present[ctx]:
                cen["topup_mixed_wants"] += 1
    cen["bulk_combos"] = len(combos)
    return cen


def write_corpus(path):
    """the packed corpus as one file for tools/bulk_subset_host_check.cpp: three 64-bit words {cases, steps, row capacity}, the lane maps, the generator
    tables, the steps"""
    lane_gen, gens, steps, row_cap = pack(corpus())
    with open(path, "wb") as f:
        f.write(np.array([len(lane_gen), len(steps), row_cap], np.uint64).tobytes())
        for a in (lane_gen, gens, steps):
            f.write(a.tobytes())


if __name__ == "__main__":
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    write_corpus(sys.argv[1])
