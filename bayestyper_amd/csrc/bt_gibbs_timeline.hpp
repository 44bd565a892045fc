// libbtgpu: the launch timeline's summary (bt_gibbs_timeline_summary) — plain host code, no HIP, no device: integer ticks in, integer ticks out.
//
// Over the selected records with end_tick != 0 (the others are counted in `unfinished`), with live(t) = number of records with start <= t < end:
//   busy_ticks = sum(end - start), peak_live = max_t live(t), median_end = the end tick of the ceil(n/2)-th record in ascending end order,
//   idle_after_median_ticks = sum over the ticks t of [median_end, last_end) of (peak_live - live(t)), last_record = the lowest index (into the array
//   handed in) among the records with end = last_end.  The measured peak stands in for "slots": no hardware constant enters.
#pragma once
#include "../../include/btgpu.h"

#include <algorithm>
#include <vector>

namespace bt {
inline void timeline_summary(const bt_gibbs_timeline_record *r, uint64_t n, uint32_t launch, uint32_t launch_class, bt_gibbs_timeline_summary_t *out) {
    bt_gibbs_timeline_summary_t s{};
    s.last_record = ~0ull;
    std::vector<uint64_t> starts, ends;
    std::vector<uint64_t> sel;
    for (uint64_t i = 0; i < n; ++i) {
        if (launch != ~0u && r[i].launch != launch) continue;
        if (launch_class != ~0u && r[i].launch_class != launch_class) continue;
        if (r[i].end_tick == 0) {
            s.unfinished += 1;
            continue;
        }
        sel.push_back(i);
    }
    s.records = sel.size();
    if (sel.empty()) {
        *out = s;
        return;
    }
    s.first_start = ~0ull;
    for (uint64_t i : sel) {
        const uint64_t a = r[i].start_tick, b = r[i].end_tick;
        s.first_start = std::min(s.first_start, a);
        if (b > s.last_end || s.last_record == ~0ull) {   // (ascending index: the first record that reaches a later end is the lowest with that end)
            s.last_end = b;
            s.last_record = i;
        }
        if (b > a) {   // (a record of no length is live at no tick)
            s.busy_ticks += b - a;
            starts.push_back(a);
            ends.push_back(b);
        }
        // (a record whose end precedes its start is malformed: it adds nothing)
    }
    {
        std::vector<uint64_t> all_ends;
        all_ends.reserve(sel.size());
        for (uint64_t i : sel) all_ends.push_back(r[i].end_tick);
        const size_t k = (all_ends.size() + 1) / 2 - 1;
        std::nth_element(all_ends.begin(), all_ends.begin() + k, all_ends.end());
        s.median_end = all_ends[k];
    }
    std::sort(starts.begin(), starts.end());
    std::sort(ends.begin(), ends.end());
    {   // live(t) changes at starts and ends only; at one tick the ends come first ([start, end) is half open)
        uint64_t live = 0;
        size_t ia = 0, ib = 0;
        while (ia < starts.size()) {
            if (ends[ib] <= starts[ia]) {
                --live;
                ++ib;
            } else {
                ++live;
                ++ia;
                s.peak_live = std::max(s.peak_live, live);
            }
        }
    }
    // sum over t of [m, e) of (peak - live(t)) = peak * (e - m) - sum over the records of |[start, end) ∩ [m, e)|
    const uint64_t m = s.median_end, e = s.last_end;
    uint64_t covered = 0;
    for (uint64_t i : sel) {
        const uint64_t a = std::max(r[i].start_tick, m), b = std::min(r[i].end_tick, e);
        if (b > a) covered += b - a;
    }
    s.idle_after_median_ticks = s.peak_live * (e - m) - covered;
    *out = s;
}
}  // namespace bt
