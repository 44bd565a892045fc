// Device-side primitives of the k-mer count table (bt_internal.hpp: TableView), shared by the translation units whose kernels insert into it
// (bt_table.hip, bt_reads.hip): the slot protocol (find, find-or-insert) and the saturating byte add of a sample's count.
#pragma once
#include "bt_internal.hpp"

namespace bt {

constexpr uint32_t ST_EMPTY = 0, ST_BUSY = 1, ST_READY = 2;

__device__ inline uint64_t mix64(uint64_t x) {   // murmur3 finaliser
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ULL;
    x ^= x >> 33;
    return x;
}

__device__ inline uint64_t table_home(Kmer a, const TableView &t) { return mix64(a.lo ^ mix64(a.hi + 0x9e3779b97f4a7c15ULL)) & t.mask; }

// State and key of one slot in one burst: the (state, meta) word pair first, then the key words, issued back to back.  A slot's key words
// are written exactly once (EMPTY -> BUSY -> READY, no deletion; a cleared / fresh table holds zeros), each with one 64-bit store, and the
// writer stores READY only after both key stores have been ACKNOWLEDGED (s_waitcnt vmcnt(0) between them, publish_slot below).  The three
// loads of a look are issued in order but — a 48-byte slot's words may straddle a 64 / 128 / 256-byte boundary, i.e. sit in different
// channels — are not necessarily SERVED in order, so a look that reads READY may still carry a stale key word, and a stale word is
// always zero.  Hence: "READY and equal" is taken as a match from the burst only when neither word of the wanted key is zero (a zero
// word that compares equal could be the stale one: the all-A k-mer, or a k-mer ending in 23 A's); every other READY case — different
// key, or equal with a zero word — is decided by a second look at the key behind an acquire fence (now certainly served after the
// state was seen READY).  So a key is never missed, never matched to another key's slot, and never inserted twice.
struct SlotLook {
    uint32_t st, cw;
    uint64_t lo, hi;
};
constexpr uint32_t NO_COUNT_WORD = 0xFFFFFFFFu;
// cword: index of a count word of the slot to fetch in the same burst (the caller's saturating add then starts from it instead of loading it), or NO_COUNT_WORD
__device__ inline SlotLook slot_look(const TableView &t, uint64_t idx, uint32_t cword = NO_COUNT_WORD) {
    uint32_t *s = t.slot(idx);
    SlotLook p;
    const uint64_t sm = __hip_atomic_load(reinterpret_cast<uint64_t *>(s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    p.lo = __hip_atomic_load(reinterpret_cast<uint64_t *>(s + 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    p.hi = __hip_atomic_load(reinterpret_cast<uint64_t *>(s + 4), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    p.cw = cword != NO_COUNT_WORD ? __hip_atomic_load(s + 6 + cword, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    p.st = (uint32_t)sm;
    return p;
}
__device__ inline bool burst_match(const SlotLook &p, Kmer a) {   // p.st == ST_READY: is the burst alone proof that the slot holds a?
    return p.lo == a.lo && p.hi == a.hi && a.lo != 0 && a.hi != 0;
}
__device__ inline bool slot_holds_other_key(const TableView &t, uint64_t idx, const SlotLook &p, Kmer a) {   // p.st == ST_READY, !burst_match(p, a)
    (void)p;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // s_waitcnt vmcnt(0) + buffer_inv sc1: the second look is served after the READY observation
    const uint64_t lo = __hip_atomic_load(t.key_lo(idx), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t hi = __hip_atomic_load(t.key_hi(idx), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return lo != a.lo || hi != a.hi;
}

// The lane that won a slot (state BUSY) writes the key and publishes it.  The key words are agent-scope atomic stores (global_store ... sc1):
// written through to the point the other XCDs read from.  READY must not overtake them, and stores to different channels are not ordered
// by issue order, so the lane WAITS until both key stores have been acknowledged — an explicit `s_waitcnt vmcnt(0)`: on gfx9 stores count
// in vmcnt, and a workgroup-scope release fence (round 4) emits no instruction at all — and only then stores the state the same way.
// A full agent-scope release store (flags & 1, BT_TABLE_RELEASE_PUBLISH) would in addition write back every dirty line of this XCD's
// L2 (buffer_wbl2) once per inserted key, which nothing here needs: the slot's words are the only data the reader relies on.
__device__ inline void publish_slot(const TableView &t, uint64_t idx, Kmer a) {
    __hip_atomic_store(t.key_lo(idx), a.lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(t.key_hi(idx), a.hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t.flags & 1u) {
        __hip_atomic_store(t.state(idx), ST_READY, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0) expcnt(7) lgkmcnt(15): gfx9 encoding, vmcnt = bits [3:0] + [15:14]
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        __hip_atomic_store(t.state(idx), ST_READY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// findKmer: slot or -1.  A BUSY slot is polled again — the loop has a single exit, no lane leaves it from inside.
__device__ inline int64_t table_find(const TableView &t, Kmer a) {
    uint64_t idx = table_home(a, t);
    int64_t result = -1;
    bool done = false;
    uint64_t probes = 0;
    while (!done) {
        const SlotLook p = slot_look(t, idx);
        if (p.st == ST_EMPTY) {
            done = true;
        } else if (p.st == ST_READY) {
            if (burst_match(p, a) || !slot_holds_other_key(t, idx, p, a)) {
                result = (int64_t)idx;
                done = true;
            } else {
                idx = (idx + 1) & t.mask;
                done = ++probes > t.mask;
            }
        }
        // ST_BUSY: another lane is publishing this slot; poll it again (the writer never waits)
    }
    return result;
}

// addKmer: slot of the (possibly new) key, -1 if the table is full.  The lane that wins a slot publishes it INSIDE the loop body
// (key words, then the READY state with release semantics) before the loop's exit condition is evaluated, so lanes of the same
// wavefront that poll that slot always see it published on a later iteration.
// cword / cw_seen: a count word to fetch along (slot_look) and its value as seen — 0 for a key this lane has just inserted; a hint for sat_add_byte_from.
// inserted: whether this lane created the record (table_unpack_kernel tells a new key from one that was there).
__device__ inline int64_t table_find_or_insert(const TableView &t, Kmer a, uint32_t cword = NO_COUNT_WORD, uint32_t *cw_seen = nullptr, bool *inserted = nullptr) {
    uint64_t idx = table_home(a, t);
    int64_t result = -1;
    bool done = false;
    uint64_t probes = 0;
    uint32_t seen = 0;
    bool won = false;
    while (!done) {
        const SlotLook p = slot_look(t, idx, cword);
        if (p.st == ST_EMPTY) {
            if (atomicCAS(t.state(idx), ST_EMPTY, ST_BUSY) == ST_EMPTY) {
                publish_slot(t, idx, a);
                result = (int64_t)idx;
                won = true;
                done = true;
            }
            // lost the race: the slot is BUSY or READY now; look at it again
        } else if (p.st == ST_READY) {
            if (burst_match(p, a) || !slot_holds_other_key(t, idx, p, a)) {
                result = (int64_t)idx;
                seen = p.cw;
                done = true;
            } else {
                idx = (idx + 1) & t.mask;
                if (++probes > t.mask) {
                    atomicExch(t.overflow, 1u);
                    done = true;
                }
            }
        }
        // ST_BUSY: poll again
    }
    // (no key counter is kept: millions of inserts would serialise on that one word; bt_table_status counts the READY slots)
    if (cw_seen) *cw_seen = seen;
    if (inserted) *inserted = won;
    return result;
}

// saturating u8 add on byte `byte_idx` of a word array (ObservedKmerCounts::addSampleCount,
// KmerCounts.cpp:161-171; KmerCounts::updateMultiplicity :178-188)
__device__ inline void sat_add_byte(uint32_t *words, uint64_t byte_idx, uint32_t add) {
    uint32_t *w = &words[byte_idx >> 2];
    const unsigned sh = (unsigned)(byte_idx & 3u) * 8u;
    uint32_t old = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (true) {
        uint32_t cur = (old >> sh) & 0xFFu;
        uint32_t nv = cur + add;
        if (nv > 255u) nv = 255u;
        uint32_t desired = (old & ~(0xFFu << sh)) | (nv << sh);
        if (desired == old) return;
        uint32_t prev = atomicCAS(w, old, desired);
        if (prev == old) return;
        old = prev;
    }
}

// the same, starting from a value of the word the caller has already seen (a stale value only costs one more round of the loop)
__device__ inline void sat_add_byte_from(uint32_t *words, uint64_t byte_idx, uint32_t add, uint32_t old) {
    uint32_t *w = &words[byte_idx >> 2];
    const unsigned sh = (unsigned)(byte_idx & 3u) * 8u;
    while (true) {
        uint32_t cur = (old >> sh) & 0xFFu;
        uint32_t nv = cur + add;
        if (nv > 255u) nv = 255u;
        uint32_t desired = (old & ~(0xFFu << sh)) | (nv << sh);
        if (desired == old) {   // nothing to add to this value: make sure the value is current before leaving
            const uint32_t now = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (now == old) return;
            old = now;
            continue;
        }
        uint32_t prev = atomicCAS(w, old, desired);
        if (prev == old) return;
        old = prev;
    }
}

}  // namespace bt
