"""The launch timeline's C ABI and its summary (bt_gibbs_timeline_summary: plain host code, exact integer ticks) without a GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bt_gibbs_timeline_enable", "bt_gibbs_timeline_sizes", "bt_gibbs_timeline_fetch", "bt_gibbs_timeline_summary")


def records(spans, launch=0, launch_class=0):
    from bayestyper_amd import lib

    r = np.zeros(len(spans), lib.TIMELINE_RECORD)
    for i, (a, b) in enumerate(spans):
        r[i]["start_tick"], r[i]["end_tick"] = a, b
    r["launch"], r["launch_class"] = launch, launch_class
    return r


def brute(spans):
    """the summary by a sweep over every tick (numpy), spans = (start, end) with end != 0"""
    a = np.array([s for s, _ in spans], np.int64)
    b = np.array([e for _, e in spans], np.int64)
    t = np.arange(a.min(), b.max())
    live = ((a[:, None] <= t[None, :]) & (t[None, :] < b[:, None])).sum(axis=0)
    order = np.sort(b)
    med = int(order[(len(b) + 1) // 2 - 1])
    peak = int(live.max()) if len(t) else 0
    tail = (t >= med) & (t < b.max())
    return {"records": len(spans), "first_start": int(a.min()), "last_end": int(b.max()), "busy_ticks": int((b - a).sum()), "peak_live": peak, "median_end": med,
            "idle_after_median_ticks": int((peak - live[tail]).sum()), "last_record": int(np.argmax(b == b.max()))}


def test_symbols_exported_and_declared():
    import ctypes

    from bayestyper_amd import lib

    so = ctypes.CDLL(lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "btgpu.h")).read()
    for name in SYMBOLS:
        assert hasattr(so, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert "typedef struct bt_gibbs_timeline_record" in header
    assert lib.TIMELINE_RECORD.itemsize == 48


def test_summary_worked_example():
    from bayestyper_amd import lib

    s = lib.timeline_summary(records([(0, 10), (0, 10), (0, 40)]))
    assert s == {"records": 3, "unfinished": 0, "first_start": 0, "last_end": 40, "busy_ticks": 60, "peak_live": 3, "median_end": 10, "idle_after_median_ticks": 60,
                 "last_record": 2}


def test_summary_empty_and_single():
    from bayestyper_amd import lib

    s = lib.timeline_summary(records([]))
    assert s["records"] == 0 and s["unfinished"] == 0 and s["busy_ticks"] == 0 and s["peak_live"] == 0 and s["idle_after_median_ticks"] == 0 and s["last_record"] is None
    s = lib.timeline_summary(records([(7, 19)]))
    assert s == {"records": 1, "unfinished": 0, "first_start": 7, "last_end": 19, "busy_ticks": 12, "peak_live": 1, "median_end": 19, "idle_after_median_ticks": 0,
                 "last_record": 0}


def test_summary_equal_ends_and_unfinished():
    from bayestyper_amd import lib

    s = lib.timeline_summary(records([(5, 30), (1, 50), (2, 50), (3, 50)]))
    assert s["last_end"] == 50 and s["last_record"] == 1 and s["median_end"] == 50 and s["peak_live"] == 4 and s["idle_after_median_ticks"] == 0
    # a wavefront that never reached its end stamp is counted and left out of everything else
    spans = [(0, 10), (3, 0), (0, 10), (0, 40)]
    s = lib.timeline_summary(records(spans))
    assert s["unfinished"] == 1 and s["records"] == 3 and s["last_record"] == 3
    assert {k: s[k] for k in ("busy_ticks", "peak_live", "median_end", "last_end", "idle_after_median_ticks")} == {"busy_ticks": 60, "peak_live": 3, "median_end": 10,
                                                                                                                 "last_end": 40, "idle_after_median_ticks": 60}


def test_summary_filters():
    from bayestyper_amd import lib

    r = np.concatenate([records([(0, 10), (0, 10), (0, 40)], launch=0, launch_class=1), records([(100, 130), (100, 110)], launch=1, launch_class=0),
                        records([(100, 200)], launch=1, launch_class=1)])
    assert lib.timeline_summary(r, launch=0)["busy_ticks"] == 60
    s = lib.timeline_summary(r, launch=1)
    assert s["records"] == 3 and s["first_start"] == 100 and s["last_end"] == 200 and s["last_record"] == 5 and s["peak_live"] == 3
    s = lib.timeline_summary(r, launch_class=0)
    assert s["records"] == 2 and s["busy_ticks"] == 40 and s["last_record"] == 3
    s = lib.timeline_summary(r, launch=1, launch_class=1)
    assert s["records"] == 1 and s["busy_ticks"] == 100 and s["last_record"] == 5
    assert lib.timeline_summary(r, launch=2)["records"] == 0
    assert lib.timeline_summary(r)["records"] == 6


def test_summary_order_independent():
    from bayestyper_amd import lib

    rng = np.random.default_rng(3)
    spans = [(int(a), int(a + d)) for a, d in zip(rng.integers(1, 500, 50), rng.integers(0, 300, 50))]
    spans[7] = (spans[7][0], 0)
    base = lib.timeline_summary(records(spans))
    perm = rng.permutation(len(spans))
    s = lib.timeline_summary(records([spans[i] for i in perm]))
    ends = [spans[i][1] for i in perm]
    expect_last = ends.index(max(ends))
    assert s["last_record"] == expect_last and perm[s["last_record"]] in [i for i, sp in enumerate(spans) if sp[1] == base["last_end"]]
    s.pop("last_record")
    b = dict(base)
    b.pop("last_record")
    assert s == b


def test_summary_against_brute_force():
    from bayestyper_amd import lib

    rng = np.random.default_rng(11)
    start = rng.integers(1000, 6000, 200)
    length = rng.integers(0, 2500, 200)   # (records of no length too)
    length[rng.integers(0, 200, 10)] = 0
    spans = [(int(a), int(a + d)) for a, d in zip(start, length)]
    spans[50] = spans[3]                  # equal records, equal ends
    spans[120] = (spans[120][0], spans[3][1])
    s = lib.timeline_summary(records(spans))
    assert s.pop("unfinished") == 0
    assert s == brute(spans)
