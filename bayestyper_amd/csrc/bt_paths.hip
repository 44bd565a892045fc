// libbtgpu — path k-mer enumeration over variant-cluster graphs.
//   bt_paths_count_kmers  <- VariantClusterGraph::countPathKmers (VariantClusterGraph.cpp:800-846) + KmerCounter.cpp:252-289
//   bt_paths_classify     <- VariantClusterGraph::classifyPathKmers (:848-939)
//   bt_paths_candidates   <- VariantClusterGraph::getHaplotypeCandidates + updateVariantPathIndices (:941-1184)
//
// The reference walks every best path nucleotide by nucleotide three times, filling per-cluster unordered_maps.  Here every
// best path of every cluster is laid out once as a TEXT in HBM (segments of vertex sequences; a separator before every
// disconnected vertex and after every path so that no k-mer window spans them), the canonical k-mer of every window is
// enumerated once by the sequence kernel, and the maps become two open-addressing indexes built with atomics:
//   A: (cluster, k-mer)       -> first text position (atomicMin), max-over-paths multiplicity
//   B: (k-mer, path)          -> multiplicity on that path
// "first-seen order" of the reference's row numbering is the order of first text positions, recovered with a prefix sum.
// Integer / byte work, HBM random access; no MFMA.
#include "bt_internal.hpp"

#include <cerrno>
#include <cstring>

#include <algorithm>
#include <exception>
#include <cstring>
#include <map>
#include <numeric>
#include <thread>

using namespace bt;

namespace {

constexpr unsigned BLOCK = 256;
constexpr uint32_t ST_EMPTY = 0, ST_BUSY = 1, ST_READY = 2;
constexpr uint32_t NOPATH = 0xFFFFFFFFu;

struct Seg {          // one included vertex of one path
    uint64_t dst;     // first text position of its nucleotides
    uint64_t src;     // first nucleotide in the vertex sequence array
    uint32_t len;
    uint32_t nt0;     // num_nucleotides of the path before this vertex
    uint32_t gpath;   // global path id
    uint32_t pad;
};

struct IndexA {       // (cluster, k-mer) -> first position, max multiplicity, list id
    uint64_t *lo, *hi;
    uint32_t *cluster, *state, *maxmult, *list_id;
    unsigned long long *first;
    uint64_t mask;
};
struct IndexB {       // (k-mer, global path) -> count
    uint64_t *lo, *hi;
    uint32_t *gpath, *state, *count, *slot_a;
    uint64_t mask;
};

__device__ inline uint64_t mix64(uint64_t x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ULL;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebULL;
    x ^= x >> 31;
    return x;
}

// find-or-insert: returns the slot of (lo, hi, tag); tag = cluster (A) or global path (B)
__device__ inline uint64_t index_insert(uint64_t *klo, uint64_t *khi, uint32_t *ktag, uint32_t *state, uint64_t mask, uint64_t lo, uint64_t hi, uint32_t tag) {
    uint64_t idx = mix64(lo ^ mix64(hi + 0x9e3779b97f4a7c15ULL * (tag + 1u))) & mask;
    while (true) {
        uint32_t st = __hip_atomic_load(&state[idx], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        if (st == ST_EMPTY) {
            const uint32_t prev = atomicCAS(&state[idx], ST_EMPTY, ST_BUSY);
            if (prev == ST_EMPTY) {
                __hip_atomic_store(&klo[idx], lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&khi[idx], hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&ktag[idx], tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&state[idx], ST_READY, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                return idx;
            }
            st = prev;
        }
        if (st == ST_READY) {
            if (__hip_atomic_load(&klo[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == lo &&
                __hip_atomic_load(&khi[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == hi &&
                __hip_atomic_load(&ktag[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == tag)
                return idx;
            idx = (idx + 1) & mask;
        }
        // ST_BUSY: the writer publishes without waiting; poll again
    }
}

// ---- text layout: every position inside a segment gets its nucleotide (ASCII), its global path and its nucleotide index ----
__global__ __launch_bounds__(BLOCK) void text_kernel(const Seg *__restrict__ segs, uint64_t nseg, const uint8_t *__restrict__ seq, uint64_t L,
                                                      char *__restrict__ text, uint32_t *__restrict__ pos_path, uint32_t *__restrict__ pos_nt) {
    for (uint64_t pos = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; pos < L; pos += (uint64_t)gridDim.x * BLOCK) {
        // last segment with dst <= pos
        uint64_t lo = 0, hi = nseg;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (segs[mid].dst <= pos) lo = mid + 1;
            else hi = mid;
        }
        char ch = 'N';
        uint32_t gp = NOPATH, nt = 0;
        if (lo > 0) {
            const Seg s = segs[lo - 1];
            if (pos - s.dst < s.len) {
                const uint32_t o = (uint32_t)(pos - s.dst);
                ch = "ACGT"[seq[s.src + o] & 3u];
                gp = s.gpath;
                nt = s.nt0 + o;
            }
        }
        text[pos] = ch;
        pos_path[pos] = gp;
        pos_nt[pos] = nt;
    }
}

__global__ __launch_bounds__(BLOCK) void bloom_insert_valid_kernel(BloomView bloom, const uint64_t *__restrict__ kmers, const uint8_t *__restrict__ valid, uint64_t L) {
    for (uint64_t pos = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; pos < L; pos += (uint64_t)gridDim.x * BLOCK)
        if (valid[pos]) bloom_insert(nthash64(Kmer{kmers[2 * pos], kmers[2 * pos + 1]}, bloom.k), bloom);
}

// ---- index build ----
__global__ __launch_bounds__(BLOCK) void index_kernel(IndexA A, IndexB B, const uint64_t *__restrict__ kmers, const uint8_t *__restrict__ valid,
                                                       const uint32_t *__restrict__ pos_path, const uint32_t *__restrict__ path_cluster, uint64_t L,
                                                       uint32_t *__restrict__ pos_slot_a) {
    for (uint64_t pos = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; pos < L; pos += (uint64_t)gridDim.x * BLOCK) {
        if (!valid[pos]) continue;
        const uint64_t lo = kmers[2 * pos], hi = kmers[2 * pos + 1];
        const uint32_t gp = pos_path[pos], c = path_cluster[gp];
        const uint64_t a = index_insert(A.lo, A.hi, A.cluster, A.state, A.mask, lo, hi, c);
        atomicMin(&A.first[a], (unsigned long long)pos);
        pos_slot_a[pos] = (uint32_t)a;
        const uint64_t b = index_insert(B.lo, B.hi, B.gpath, B.state, B.mask, lo, hi, gp);
        B.slot_a[b] = (uint32_t)a;   // every inserter of this entry writes the same value
        atomicAdd(&B.count[b], 1u);
    }
}
// max over paths of the saturating per-path multiplicity (VariantClusterGraph.cpp:887-910)
__global__ __launch_bounds__(BLOCK) void maxmult_kernel(IndexA A, IndexB B) {
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i <= B.mask; i += (uint64_t)gridDim.x * BLOCK) {
        if (B.state[i] != ST_READY) continue;
        const uint32_t cnt = B.count[i] > 255u ? 255u : B.count[i];
        atomicMax(&A.maxmult[B.slot_a[i]], cnt);
    }
}
// dense list of the distinct (cluster, k-mer) entries: order is irrelevant (the table update commutes)
__global__ __launch_bounds__(BLOCK) void list_kernel(IndexA A, uint64_t *__restrict__ list_kmers, uint8_t *__restrict__ list_mult, uint32_t *__restrict__ list_cluster,
                                                      unsigned long long *__restrict__ cursor) {
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i <= A.mask; i += (uint64_t)gridDim.x * BLOCK) {
        if (A.state[i] != ST_READY) continue;
        const unsigned long long j = atomicAdd(cursor, 1ULL);
        list_kmers[2 * j] = A.lo[i];
        list_kmers[2 * j + 1] = A.hi[i];
        list_mult[j] = (uint8_t)A.maxmult[i];
        list_cluster[j] = A.cluster[i];
        A.list_id[i] = (uint32_t)j;
    }
}
__global__ __launch_bounds__(BLOCK) void classify_tally_kernel(const uint32_t *__restrict__ list_cluster, const uint8_t *__restrict__ excluded, uint64_t n,
                                                                uint32_t *__restrict__ num_path_kmers, uint32_t *__restrict__ has_excluded) {
    for (uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; j < n; j += (uint64_t)gridDim.x * BLOCK) {
        atomicAdd(&num_path_kmers[list_cluster[j]], 1u);
        if (excluded[j]) atomicOr(&has_excluded[list_cluster[j]], 1u);
    }
}

// ---- countPathMultigroupKmers: D counts distinct (group, k-mer) pairs, E tracks per k-mer the first group seen and "another group too" ----
// ---- countPathMultigroupKmers in the reference's single-thread order (KmerCounter.cpp:105-145) ----
// The reference walks the groups in index order; a group's distinct path k-mers sit in ONE std::unordered_set<std::bitset<2k>> that
// is clear()ed between groups (its bucket count survives) and are visited in that container's iteration order.  A k-mer the path
// filter reports at that moment goes into the multigroup table — because an earlier group (or unit) holds it, or as a false positive
// of what has been inserted SO FAR — and is otherwise inserted.  Reproduced exactly:
//   1. every distinct (group, k-mer) gets its time t = (k-mers of earlier groups) + (rank in its group's iteration order): the
//      container (libstdc++ _Hashtable, unique keys, std::hash<bitset> = _Hash_bytes, prime rehash policy) is replayed per group by
//      one lane from the k-mers' first occurrences in path order;
//   2. a k-mer is reported at its first time t iff every one of its filter bits was set before t.  A k-mer that is reported is not
//      inserted, but all its bits are set already, so "first time bit b is set" = min t over ALL k-mers having b (0 for bits set by
//      earlier units): no fixed point is needed;
//   3. only k-mers whose bits are ALL either set by earlier units or shared with another k-mer of the unit (a second bit array filled
//      while a scratch copy of the filter takes the unit's k-mers) can qualify — a few per 10^4 —, so the per-bit times are kept in
//      a small hash table over just those k-mers' bits.
constexpr uint32_t SQ_NONE = 0xFFFFFFFFu, SQ_BEFORE = 0xFFFFFFFEu;
// std::hash<std::bitset<2k>>: _Hash_bytes (libstdc++-v3/libsupc++/hash_bytes.cc, 64-bit) over the bitset's first (2k + 7) / 8 bytes, seed 0xc70f6907
__host__ __device__ inline uint64_t std_hash_bitset(uint64_t lo, uint64_t hi, unsigned k) {
    const uint64_t mul = (0xc6a4a793ULL << 32) + 0x5bd1e995ULL;
    const unsigned len = (2 * k + 7) / 8, full = len / 8;
    uint64_t hash = 0xc70f6907ULL ^ (len * mul);
    const uint64_t w[3] = {lo, hi, 0};
    for (unsigned i = 0; i < full; ++i) {
        uint64_t data = w[i] * mul;
        data ^= data >> 47;
        data *= mul;
        hash ^= data;
        hash *= mul;
    }
    if (len & 7u) {
        hash ^= w[full] & ((1ULL << (8u * (len & 7u))) - 1ULL);
        hash *= mul;
    }
    hash ^= hash >> 47;
    hash *= mul;
    hash ^= hash >> 47;
    return hash;
}
// libstdc++'s bucket counts when a container grows one element at a time: 1 -> 13 -> _M_next_bkt(2 B) -> ...
__host__ __device__ inline uint64_t std_next_bucket_count(uint64_t b) {
    const uint64_t chain[31] = {13ull, 29ull, 59ull, 127ull, 257ull, 541ull, 1109ull, 2357ull, 5087ull, 10273ull, 20753ull, 42043ull, 85229ull, 172933ull, 351061ull, 712697ull,
                                1447153ull, 2938679ull, 5967347ull, 12117689ull, 24607243ull, 49969847ull, 101473717ull, 206062531ull, 418451333ull, 849749479ull,
                                1725587117ull, 3504151727ull, 8589934583ull, 25769803693ull, 68719476731ull};
    for (int i = 0; i < 31; ++i)
        if (chain[i] > b) return chain[i];
    return chain[30];
}

// first pass: the (k-mer, group) index D with the first text position of every entry, the k-mer index E with "seen in two groups"
__global__ __launch_bounds__(BLOCK) void multigroup_kernel(uint64_t *__restrict__ dlo, uint64_t *__restrict__ dhi, uint32_t *__restrict__ dtag, uint32_t *__restrict__ dstate,
                                                            uint32_t *__restrict__ dfirst, uint32_t *__restrict__ pos_d, uint64_t *__restrict__ elo, uint64_t *__restrict__ ehi,
                                                            uint32_t *__restrict__ etag, uint32_t *__restrict__ estate, uint32_t *__restrict__ egroup,
                                                            uint32_t *__restrict__ emulti, uint64_t mask, const uint64_t *__restrict__ kmers, const uint8_t *__restrict__ valid,
                                                            const uint32_t *__restrict__ pos_path, const uint32_t *__restrict__ path_cluster,
                                                            const uint32_t *__restrict__ cluster_group, uint64_t L) {
    for (uint64_t pos = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; pos < L; pos += (uint64_t)gridDim.x * BLOCK) {
        if (!valid[pos]) continue;
        const uint64_t lo = kmers[2 * pos], hi = kmers[2 * pos + 1];
        const uint32_t g = cluster_group[path_cluster[pos_path[pos]]];
        const uint64_t d = index_insert(dlo, dhi, dtag, dstate, mask, lo, hi, g);
        atomicMin(&dfirst[d], (uint32_t)pos);
        pos_d[pos] = (uint32_t)d;
        const uint64_t e = index_insert(elo, ehi, etag, estate, mask, lo, hi, 0u);
        const uint32_t prev = atomicCAS(&egroup[e], 0xFFFFFFFFu, g);
        if (prev != 0xFFFFFFFFu && prev != g) emulti[e] = 1u;
    }
}
__global__ __launch_bounds__(BLOCK) void mg_flag_kernel(const uint8_t *__restrict__ valid, const uint32_t *__restrict__ pos_d, const uint32_t *__restrict__ dfirst, uint64_t L,
                                                         uint32_t *__restrict__ flag) {
    for (uint64_t pos = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; pos < L; pos += (uint64_t)gridDim.x * BLOCK)
        flag[pos] = (valid[pos] && dfirst[pos_d[pos]] == (uint32_t)pos) ? 1u : 0u;
}
__global__ __launch_bounds__(BLOCK) void mg_seq_kernel(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ rowpos, uint64_t L, uint32_t *__restrict__ seq_pos) {
    for (uint64_t pos = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; pos < L; pos += (uint64_t)gridDim.x * BLOCK)
        if (flag[pos]) seq_pos[rowpos[pos]] = (uint32_t)pos;
}
// One lane per group: replay the inserts of the group's distinct k-mers (first occurrences, path order) into an unordered_set that
// starts with `b_init[g]` buckets (what earlier groups left behind), then number the nodes in iteration order.
// libstdc++ _Hashtable: a node enters at the front of its bucket (behind the bucket's "before" node) or, for an empty bucket, at the
// front of the whole list; a rehash re-threads the list front to back the same way (hashtable.h: _M_insert_bucket_begin, _M_rehash_aux).
// The bucket array itself is not materialised (a small group may inherit millions of buckets from a large earlier one): the buckets in
// use live in a per-group open-addressing map bucket -> "before" node with room for twice the group's k-mers.
// key(node, lo, hi) hands out the node's k-mer; rank_out(node, rank) receives its position in iteration order.  Shared by the kernel and
// by bt_diag_kmer_set_order (the same code run on the host against the real container in the CPU tests).
template <typename KeyFn, typename RankFn>
__host__ __device__ inline void replay_kmer_set(uint32_t n, uint64_t b_init, unsigned k, uint32_t *nx, uint32_t *mk, uint32_t *mv, uint32_t mmask, KeyFn key, RankFn rank_out) {
    uint64_t B = b_init, next_resize = B > 1 ? B : 0;
    uint32_t head = SQ_NONE;
    auto bucket_of = [&](uint32_t node) {
        uint64_t lo, hi;
        key(node, lo, hi);
        return (uint32_t)(std_hash_bitset(lo, hi, k) % B);
    };
    auto map_clear = [&]() {
        for (uint32_t i = 0; i <= mmask; ++i) mk[i] = SQ_NONE;
    };
    auto map_slot = [&](uint32_t b) {   // slot of bucket b (inserted empty when absent)
        uint32_t i = (b * 2654435761u) & mmask;
        while (mk[i] != b) {
            if (mk[i] == SQ_NONE) {
                mk[i] = b;
                mv[i] = SQ_NONE;
                break;
            }
            i = (i + 1) & mmask;
        }
        return i;
    };
    map_clear();
    for (uint32_t e = 0; e < n; ++e) {
        if ((uint64_t)e + 1 > next_resize) {   // _Prime_rehash_policy::_M_need_rehash(B, e, 1), max_load_factor 1
            uint64_t min_bkts = (uint64_t)e + 1;
            if (next_resize == 0 && min_bkts < 11) min_bkts = 11;
            if (min_bkts >= B) {
                B = std_next_bucket_count(B);   // _M_next_bkt(max(min_bkts + 1, 2 B)) for one-at-a-time growth
                next_resize = B;
                map_clear();
                uint32_t p = head, bbegin = SQ_NONE;   // bbegin: map slot of the bucket that currently begins the list
                head = SQ_NONE;
                while (p != SQ_NONE) {
                    const uint32_t nxt = nx[p], sl = map_slot(bucket_of(p));
                    if (mv[sl] == SQ_NONE) {
                        nx[p] = head;
                        head = p;
                        mv[sl] = SQ_BEFORE;
                        if (nx[p] != SQ_NONE) mv[bbegin] = p;
                        bbegin = sl;
                    } else {
                        const uint32_t prev = mv[sl];
                        if (prev == SQ_BEFORE) {
                            nx[p] = head;
                            head = p;
                        } else {
                            nx[p] = nx[prev];
                            nx[prev] = p;
                        }
                    }
                    p = nxt;
                }
            } else
                next_resize = B;
        }
        const uint32_t sl = map_slot(bucket_of(e));
        if (mv[sl] != SQ_NONE) {
            const uint32_t prev = mv[sl];
            if (prev == SQ_BEFORE) {
                nx[e] = head;
                head = e;
            } else {
                nx[e] = nx[prev];
                nx[prev] = e;
            }
        } else {
            nx[e] = head;
            head = e;
            if (nx[e] != SQ_NONE) mv[map_slot(bucket_of(nx[e]))] = e;
            mv[sl] = SQ_BEFORE;
        }
    }
    uint32_t rank = 0;
    for (uint32_t p = head; p != SQ_NONE; p = nx[p]) rank_out(p, rank++);
}
__global__ __launch_bounds__(BLOCK) void mg_order_kernel(const uint64_t *__restrict__ kmers, const uint32_t *__restrict__ seq_pos, const uint32_t *__restrict__ goff,
                                                          const uint64_t *__restrict__ moff, const uint64_t *__restrict__ b_init, uint32_t *__restrict__ next,
                                                          uint32_t *__restrict__ map_key, uint32_t *__restrict__ map_val, uint32_t *__restrict__ time_of_seq, uint32_t G,
                                                          unsigned k, uint32_t wide_min) {
    const uint32_t g = blockIdx.x * BLOCK + threadIdx.x;
    if (g >= G) return;
    const uint32_t i0 = goff[g], n = goff[g + 1] - i0;
    if (n == 0 || (wide_min && n >= wide_min)) return;   // a group of at least wide_min k-mers is mg_order_wide_kernel's (0: none is)
#ifdef BT_MG_INSERTION_ORDER   // (test of the tests: with insertion order instead of the container's order the parity test must fail)
    for (uint32_t p = 0; p < n; ++p) time_of_seq[i0 + p] = i0 + p + 1u;
    return;
#endif
    replay_kmer_set(
        n, b_init[g], k, next + i0, map_key + moff[g], map_val + moff[g], (uint32_t)(moff[g + 1] - moff[g]) - 1u,
        [&](uint32_t node, uint64_t &lo, uint64_t &hi) {
            const uint64_t pos = seq_pos[i0 + node];
            lo = kmers[2 * pos];
            hi = kmers[2 * pos + 1];
        },
        [&](uint32_t node, uint32_t rank) { time_of_seq[i0 + node] = i0 + rank + 1u; });   // times start at 1: 0 = "set by an earlier unit"
}
// ---- the same order without the insert-by-insert replay: stage by stage ----
// The container's rules (replay_kmer_set) are uniform enough for a closed form.  Cut a group's inserts into STAGES: a stage ends where a
// rehash happens, so a stage has one bucket count B.  Let seq be the stage's input — the list the previous stage left, front to back,
// followed by the nodes inserted during the stage in insertion order —, t(x) a node's position in seq, b(x) = hash(x) % B and
// first(b) = min t over the nodes of bucket b.  A node that enters an empty bucket goes to the front of the whole list, so buckets lie
// in the list by DESCENDING first; a node that enters a non-empty bucket goes to the front of that bucket, so a bucket's nodes lie by
// DESCENDING t; a rehash walks the old list front to back under the same two rules, which is why the old list is the head of seq.
// The list at the end of the stage is seq sorted by (first(b(x)) descending, t(x) descending); the last stage's list is the iteration
// order.  Every stage is data-parallel: nothing in it waits for another lane, and no result depends on the order atomics land in.
struct MgStage {
    uint64_t buckets;      // bucket count during the stage
    uint32_t begin, end;   // the stage inserts nodes [begin, end); the list held the nodes [0, begin) when it began
};
constexpr uint32_t MG_MAX_STAGES = 33;   // the prime chain of std_next_bucket_count has 31 entries
constexpr uint32_t MG_ERR_PROBE = 1, MG_ERR_CHAIN = 2, MG_ERR_PLACE = 4, MG_ERR_STAGES = 8;
__host__ __device__ inline MgStage mg_stage_start(uint64_t b_init) { return MgStage{b_init, 0, 0}; }
// The stage after `st` of a group of n nodes, from rehash to rehash: false when st was the last one (st.buckets is then the container's
// final bucket count).  replay_kmer_set's test before insert e is "e + 1 > next_resize", with next_resize = B once B > 1 and 0 for a
// fresh set; it then rehashes iff max(e + 1, 11 for a fresh set) >= B, which that test implies for every B >= 1.  So a fresh set goes
// to 13 buckets before its first insert, any other set rehashes exactly before insert e = B, and a stage ends at min(n, B).
__host__ __device__ inline bool mg_stage_next(uint32_t n, MgStage &st) {
    if (st.end >= n) return false;
    const uint64_t next_resize = st.buckets > 1 ? st.buckets : 0;
    st.begin = st.end;
    if ((uint64_t)st.begin + 1 > next_resize) st.buckets = std_next_bucket_count(st.buckets);
    st.end = st.buckets < n ? (uint32_t)st.buckets : n;
    return true;
}

// who orders one group: a single thread (a lane's worth of work on the host, bt_diag_kmer_set_order_staged) or a workgroup
struct SoloTeam {   // every atomic is the plain operation
    static constexpr uint32_t W = 1;
    __host__ __device__ static uint32_t lane() { return 0; }
    __host__ __device__ static void sync() {}
    __host__ __device__ static uint32_t load(const uint32_t *p) { return *p; }
    __host__ __device__ static uint32_t cas(uint32_t *p, uint32_t expected, uint32_t v) {
        const uint32_t old = *p;
        if (old == expected) *p = v;
        return old;
    }
    __host__ __device__ static void min(uint32_t *p, uint32_t v) {
        if (v < *p) *p = v;
    }
    __host__ __device__ static uint32_t exch(uint32_t *p, uint32_t v) {
        const uint32_t old = *p;
        *p = v;
        return old;
    }
    __host__ __device__ static void inc(uint32_t *p) { ++*p; }
    __host__ __device__ static uint32_t scan_excl(uint32_t v, uint32_t &total) {
        total = v;
        return 0;
    }
};
struct BlockTeam {   // the BLOCK threads of a workgroup
    static constexpr uint32_t W = BLOCK;
    __device__ static uint32_t lane() { return threadIdx.x; }
    __device__ static void sync() { __syncthreads(); }
    __device__ static uint32_t load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }   // a word other lanes CAS meanwhile
    __device__ static uint32_t cas(uint32_t *p, uint32_t expected, uint32_t v) { return atomicCAS(p, expected, v); }
    __device__ static void min(uint32_t *p, uint32_t v) { atomicMin(p, v); }
    __device__ static uint32_t exch(uint32_t *p, uint32_t v) { return atomicExch(p, v); }
    __device__ static void inc(uint32_t *p) { atomicAdd(p, 1u); }
    // exclusive prefix sum of v over the team in lane order, total = the team's sum; every lane calls it
    __device__ static uint32_t scan_excl(uint32_t v, uint32_t &total) {
        __shared__ uint32_t wave_sum[BLOCK / 64];
        const uint32_t l = threadIdx.x & 63u, w = threadIdx.x >> 6;
        uint32_t inc = v;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(inc, d, 64);
            if (l >= d) inc += o;
        }
        __syncthreads();   // (the previous call's reads of wave_sum are over)
        if (l == 63) wave_sum[w] = inc;
        __syncthreads();
        uint32_t base = 0;
        total = 0;
        for (uint32_t i = 0; i < BLOCK / 64; ++i) {
            if (i < w) base += wave_sum[i];
            total += wave_sum[i];
        }
        return base + inc - v;
    }
};

// one group's work area of the staged order: word offsets of its arrays from the area's start, and its size
struct MgLayout {
    uint64_t seq_a, seq_b;   // n each: the list before and after a stage (node numbers, front to back)
    uint64_t slot_of;        // n: map slot of the node at position t
    uint64_t chain;          // n: next position on the bucket's chain
    uint64_t hist;           // n: at first(b) the size of bucket b, then (after the scan) where bucket b starts in the new list
    uint64_t map_key, map_first, map_head, map_count;   // map_cap each: bucket number, its first(b), its chain's head, its size
    uint64_t map_cap;        // a power of two >= 2 n
    uint64_t total;          // a multiple of four words
};
__host__ __device__ inline MgLayout mg_layout(uint32_t n) {
    MgLayout l{};
    l.map_cap = 16;
    while (l.map_cap < 2ull * n) l.map_cap <<= 1;
    uint64_t o = 0;
    l.seq_a = o, o += n;
    l.seq_b = o, o += n;
    l.slot_of = o, o += n;
    l.chain = o, o += n;
    l.hist = o, o += n;
    l.map_key = o, o += l.map_cap;
    l.map_first = o, o += l.map_cap;
    l.map_head = o, o += l.map_cap;
    l.map_count = o, o += l.map_cap;
    l.total = (o + 3) & ~3ull;
    return l;
}

// One stage of a group of n nodes: `cur` holds the list the previous stage left in [0, st.begin); `nxt` receives the list after the
// stage, [0, st.end).  Returns the lane's MG_ERR_* bits (0: none).  Every lane of the team runs every sync(), and every loop is bounded by
// the stage's node count or its map size: a bound that does not hold is reported, never waited for.
template <typename T, typename KeyFn>
__host__ __device__ inline uint32_t mg_stage_order(uint32_t n, const MgStage &st, unsigned k, uint32_t *area, const MgLayout &l, uint32_t *cur, uint32_t *nxt, KeyFn key) {
    uint32_t *slot_of = area + l.slot_of, *chain = area + l.chain, *hist = area + l.hist;
    uint32_t *mkey = area + l.map_key, *mfirst = area + l.map_first, *mhead = area + l.map_head, *mcount = area + l.map_count;
    const uint32_t m = st.end, lane = T::lane();
    uint64_t cap = 16;   // the stage's part of the map: room for twice its nodes (<= l.map_cap, as m <= n)
    while (cap < 2ull * m) cap <<= 1;
    if (m > n || cap > l.map_cap || cap > (1ull << 31)) return MG_ERR_PLACE;   // (the same for every lane)
    const uint32_t mcap = (uint32_t)cap, mmask = mcap - 1u;
    uint32_t err = 0;
    // 0. empty map and histogram; the stage's own nodes behind the inherited list (node e sits at position e: the list holds nodes 0..begin-1)
    for (uint32_t i = lane; i < mcap; i += T::W) {
        mkey[i] = SQ_NONE;
        mfirst[i] = SQ_NONE;
        mhead[i] = SQ_NONE;
        mcount[i] = 0;
    }
    for (uint32_t t = lane; t < m; t += T::W) {
        hist[t] = 0;
        if (t >= st.begin) cur[t] = t;
    }
    T::sync();
    // 1. every node finds (or makes) its bucket's slot, lowers first(b) to its position and pushes itself on the bucket's chain
    for (uint32_t t = lane; t < m; t += T::W) {
        uint64_t lo = 0, hi = 0;
        const uint32_t node = cur[t];
        if (node < n) key(node, lo, hi);
        const uint32_t b = (uint32_t)(std_hash_bitset(lo, hi, k) % st.buckets);
        uint32_t i = (b * 2654435761u) & mmask, sl = SQ_NONE;
        for (uint32_t probes = 0; probes < mcap && node < n; ++probes) {   // (node >= n: a place an earlier stage reported and left unwritten)
            uint32_t have = T::load(&mkey[i]);
            if (have == SQ_NONE) have = T::cas(&mkey[i], SQ_NONE, b);
            if (have == SQ_NONE || have == b) {
                sl = i;
                break;
            }
            i = (i + 1) & mmask;
        }
        slot_of[t] = sl;
        if (sl == SQ_NONE) {
            err |= MG_ERR_PROBE;
            continue;
        }
        T::min(&mfirst[sl], t);
        chain[t] = T::exch(&mhead[sl], t);
        T::inc(&mcount[sl]);
    }
    T::sync();
    // 2. the size of every bucket, at its first position
    for (uint32_t i = lane; i < mcap; i += T::W)
        if (T::load(&mkey[i]) != SQ_NONE) {   // (words the lanes wrote with atomics are read the same way)
            const uint32_t first = T::load(&mfirst[i]);
            if (first < m) hist[first] = T::load(&mcount[i]);
            else err |= MG_ERR_PLACE;
        }
    T::sync();
    // 3. buckets lie by descending first: a bucket starts behind all buckets with a larger first (exclusive scan from the high end, four entries per lane and round)
    uint32_t carry = 0;
    for (uint32_t base = 0; base < m; base += 4 * T::W) {
        uint32_t v[4], sum = 0;
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t idx = base + 4 * lane + j;
            v[j] = idx < m ? hist[m - 1 - idx] : 0;
            sum += v[j];
        }
        uint32_t total;
        uint32_t at = carry + T::scan_excl(sum, total);
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t idx = base + 4 * lane + j;
            if (idx < m) hist[m - 1 - idx] = at;
            at += v[j];
        }
        carry += total;
    }
    T::sync();
    // 4. a node's place: its bucket's start + the nodes of its chain with a larger t (the chain is in the order the pushes landed in: walk all of it)
    for (uint32_t t = lane; t < m; t += T::W) {
        const uint32_t sl = slot_of[t];
        if (sl == SQ_NONE) continue;
        const uint32_t size = T::load(&mcount[sl]), first = T::load(&mfirst[sl]);
        uint32_t larger = 0, p = T::load(&mhead[sl]);
        for (uint32_t steps = 0; steps < size && p != SQ_NONE; ++steps) {
            if (p >= m) break;
            larger += p > t ? 1u : 0u;
            p = chain[p];
        }
        if (p != SQ_NONE) err |= MG_ERR_CHAIN;
        const uint64_t place = first < m ? (uint64_t)hist[first] + larger : m;
        if (place < m) nxt[place] = cur[t];
        else err |= MG_ERR_PLACE;
    }
    T::sync();
    return err;
}
// All stages of one group of n nodes whose container starts with b_init buckets; rank_out(node, rank) as replay_kmer_set's.  `area` is the
// group's work area (mg_layout(n)).  Returns the lane's MG_ERR_* bits.
template <typename T, typename KeyFn, typename RankFn>
__host__ __device__ inline uint32_t mg_staged_order(uint32_t n, uint64_t b_init, unsigned k, uint32_t *area, KeyFn key, RankFn rank_out) {
    const MgLayout l = mg_layout(n);
    uint32_t *cur = area + l.seq_a, *nxt = area + l.seq_b, err = 0;
    MgStage st = mg_stage_start(b_init);
    for (uint32_t s = 0; mg_stage_next(n, st); ++s) {
        if (s >= MG_MAX_STAGES) return err | MG_ERR_STAGES;   // (the same for every lane)
        err |= mg_stage_order<T>(n, st, k, area, l, cur, nxt, key);
        uint32_t *const x = cur;
        cur = nxt;
        nxt = x;
    }
    for (uint32_t r = T::lane(); r < n; r += T::W)
        if (cur[r] < n) rank_out(cur[r], r);
        else err |= MG_ERR_PLACE;
    return err;
}
// One workgroup per wide group (a group of at least wide_min distinct k-mers; wide_group lists them, area_off[i] = word offset of the work
// area of the i-th).  Writes time_of_seq as mg_order_kernel does, which skips these groups.  A violated loop bound sets *err.
__global__ __launch_bounds__(BLOCK) void mg_order_wide_kernel(const uint64_t *__restrict__ kmers, const uint32_t *__restrict__ seq_pos, const uint32_t *__restrict__ goff,
                                                               const uint64_t *__restrict__ b_init, const uint32_t *__restrict__ wide_group,
                                                               const uint64_t *__restrict__ area_off, uint32_t *__restrict__ areas, uint32_t *__restrict__ time_of_seq,
                                                               uint32_t *__restrict__ err, unsigned k) {
    const uint32_t g = wide_group[blockIdx.x];
    const uint32_t i0 = goff[g], n = goff[g + 1] - i0;
    const uint32_t e = mg_staged_order<BlockTeam>(
        n, b_init[g], k, areas + area_off[blockIdx.x],
        [&](uint32_t node, uint64_t &lo, uint64_t &hi) {
            const uint64_t pos = seq_pos[i0 + node];
            lo = kmers[2 * pos];
            hi = kmers[2 * pos + 1];
        },
        [&](uint32_t node, uint32_t rank) { time_of_seq[i0 + node] = i0 + rank + 1u; });
    if (e) atomicOr(err, e);
}
// first time of every distinct k-mer of the unit
__global__ __launch_bounds__(BLOCK) void mg_etime_kernel(const uint64_t *__restrict__ kmers, const uint32_t *__restrict__ seq_pos, const uint32_t *__restrict__ time_of_seq,
                                                          uint64_t n, uint64_t *__restrict__ elo, uint64_t *__restrict__ ehi, uint32_t *__restrict__ etag,
                                                          uint32_t *__restrict__ estate, uint64_t mask, uint32_t *__restrict__ etime) {
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t pos = seq_pos[i];
        const uint64_t e = index_insert(elo, ehi, etag, estate, mask, kmers[2 * pos], kmers[2 * pos + 1], 0u);
        atomicMin(&etime[e], time_of_seq[i]);
    }
}
__device__ inline void bloom_word_bit(uint64_t h, unsigned i, uint64_t base, const BloomView &b, uint64_t &word, uint32_t &m, uint64_t &bit_id) {
    const uint64_t pos = bloom_probe_pos(h, i, b), byte = base + (pos >> 3);
    word = byte >> 2;
    m = 1u << (uint32_t)((byte & 3u) * 8u + (7u - (unsigned)(pos & 7u)));
    bit_id = base * 8u + pos;
}
// scratch filter f1 takes the unit's distinct k-mers; f2 = bits that were set already when a k-mer set them (shared with another k-mer)
__global__ __launch_bounds__(BLOCK) void mg_shared_bits_kernel(BloomView bv, const uint64_t *__restrict__ elo, const uint64_t *__restrict__ ehi, const uint32_t *__restrict__ estate,
                                                                uint64_t mask, uint32_t *__restrict__ f1, uint32_t *__restrict__ f2) {
    for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e <= mask; e += (uint64_t)gridDim.x * BLOCK) {
        if (estate[e] != ST_READY) continue;
        const uint64_t h = nthash64(Kmer{elo[e], ehi[e]}, bv.k), base = bloom_sub_base(h, bv);
        for (unsigned i = 0; i < bv.num_hashes; ++i) {
            uint64_t w, id;
            uint32_t m;
            bloom_word_bit(h, i, base, bv, w, m, id);
            if (atomicOr(&f1[w], m) & m) atomicOr(&f2[w], m);
        }
    }
}
// candidates: not yet multigroup, every bit set by an earlier unit or shared inside the unit.  out == nullptr: count only.
__global__ __launch_bounds__(BLOCK) void mg_candidates_kernel(BloomView bv, const uint64_t *__restrict__ elo, const uint64_t *__restrict__ ehi, const uint32_t *__restrict__ estate,
                                                               const uint32_t *__restrict__ emulti, uint64_t mask, const uint32_t *__restrict__ f2,
                                                               unsigned long long *__restrict__ cursor, uint64_t *__restrict__ out) {
    for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e <= mask; e += (uint64_t)gridDim.x * BLOCK) {
        if (estate[e] != ST_READY || emulti[e]) continue;
        const uint64_t h = nthash64(Kmer{elo[e], ehi[e]}, bv.k), base = bloom_sub_base(h, bv);
        bool all = true;
        for (unsigned i = 0; i < bv.num_hashes && all; ++i) {
            uint64_t w, id;
            uint32_t m;
            bloom_word_bit(h, i, base, bv, w, m, id);
            all = ((bv.words[w] | f2[w]) & m) != 0;
        }
        if (all) {
            const unsigned long long j = atomicAdd(cursor, 1ULL);
            if (out) out[j] = e;
        }
    }
}
__device__ inline uint64_t cb_find_or_insert(unsigned long long *keys, uint64_t mask, uint64_t id, bool insert) {   // returns the slot, or ~0 if absent
    uint64_t i = mix64(id) & mask;
    while (true) {
        unsigned long long cur = __hip_atomic_load(&keys[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == ~0ULL) {
            if (!insert) return ~0ULL;
            cur = atomicCAS(&keys[i], ~0ULL, (unsigned long long)id);
            if (cur == ~0ULL) return i;
        }
        if (cur == id) return i;
        i = (i + 1) & mask;
    }
}
__global__ __launch_bounds__(BLOCK) void mg_cand_bits_kernel(BloomView bv, const uint64_t *__restrict__ elo, const uint64_t *__restrict__ ehi, const uint64_t *__restrict__ cand,
                                                              uint64_t ncand, unsigned long long *__restrict__ cb_keys, uint32_t *__restrict__ cb_time, uint64_t cb_mask) {
    for (uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; j < ncand; j += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t e = cand[j], h = nthash64(Kmer{elo[e], ehi[e]}, bv.k), base = bloom_sub_base(h, bv);
        for (unsigned i = 0; i < bv.num_hashes; ++i) {
            uint64_t w, id;
            uint32_t m;
            bloom_word_bit(h, i, base, bv, w, m, id);
            const uint64_t slot = cb_find_or_insert(cb_keys, cb_mask, id, true);
            if (bv.words[w] & m) atomicMin(&cb_time[slot], 0u);   // set by an earlier unit
        }
    }
}
__global__ __launch_bounds__(BLOCK) void mg_bit_times_kernel(BloomView bv, const uint64_t *__restrict__ elo, const uint64_t *__restrict__ ehi, const uint32_t *__restrict__ estate,
                                                              const uint32_t *__restrict__ etime, uint64_t mask, unsigned long long *__restrict__ cb_keys,
                                                              uint32_t *__restrict__ cb_time, uint64_t cb_mask) {
    for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e <= mask; e += (uint64_t)gridDim.x * BLOCK) {
        if (estate[e] != ST_READY) continue;
        const uint64_t h = nthash64(Kmer{elo[e], ehi[e]}, bv.k), base = bloom_sub_base(h, bv);
        for (unsigned i = 0; i < bv.num_hashes; ++i) {
            uint64_t w, id;
            uint32_t m;
            bloom_word_bit(h, i, base, bv, w, m, id);
            const uint64_t slot = cb_find_or_insert(cb_keys, cb_mask, id, false);
            if (slot != ~0ULL) atomicMin(&cb_time[slot], etime[e]);
        }
    }
}
__global__ __launch_bounds__(BLOCK) void mg_reported_kernel(BloomView bv, const uint64_t *__restrict__ elo, const uint64_t *__restrict__ ehi, const uint32_t *__restrict__ etime,
                                                             const uint64_t *__restrict__ cand, uint64_t ncand, unsigned long long *__restrict__ cb_keys,
                                                             const uint32_t *__restrict__ cb_time, uint64_t cb_mask, uint32_t *__restrict__ emulti) {
    for (uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; j < ncand; j += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t e = cand[j], h = nthash64(Kmer{elo[e], ehi[e]}, bv.k), base = bloom_sub_base(h, bv);
        uint32_t latest = 0;
        for (unsigned i = 0; i < bv.num_hashes; ++i) {
            uint64_t w, id;
            uint32_t m;
            bloom_word_bit(h, i, base, bv, w, m, id);
            const uint32_t t = cb_time[cb_find_or_insert(cb_keys, cb_mask, id, false)];
            latest = t > latest ? t : latest;
        }
        if (latest < etime[e]) emulti[e] = 1u;   // every bit was set before the k-mer's first turn: the filter reports it
    }
}
__global__ __launch_bounds__(BLOCK) void multigroup_list_kernel(const uint64_t *__restrict__ elo, const uint64_t *__restrict__ ehi, const uint32_t *__restrict__ estate,
                                                                 const uint32_t *__restrict__ emulti, const uint32_t *__restrict__ dstate, uint64_t mask,
                                                                 uint64_t *__restrict__ out, unsigned long long *__restrict__ counters /* [0] multigroup, [1] (group,kmer) pairs */) {
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i <= mask; i += (uint64_t)gridDim.x * BLOCK) {
        if (dstate[i] == ST_READY) atomicAdd(&counters[1], 1ULL);
        if (estate[i] == ST_READY && emulti[i]) {
            const unsigned long long j = atomicAdd(&counters[0], 1ULL);
            out[2 * j] = elo[i];
            out[2 * j + 1] = ehi[i];
        }
    }
}

// ---- candidates ----
// per distinct (cluster, k-mer): table record -> excluded?, multicluster?; list_flags[j]: bit0 in table, bit1 excluded, bit2 multicluster
__global__ __launch_bounds__(BLOCK) void record_kernel(TableView t, const int64_t *__restrict__ slots, uint64_t n, uint8_t *__restrict__ list_flags) {
    for (uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; j < n; j += (uint64_t)gridDim.x * BLOCK) {
        uint8_t f = 0;
        if (slots[j] >= 0) {
            const uint32_t flags = *t.meta((uint64_t)slots[j]) & 0xffu;
            f = 1;
            if (flags & (BT_KC_DECOY_OCC | BT_KC_MAX_MULTIPLICITY | BT_KC_MULTIGROUP_OCC)) f |= 2;   // isExcluded (KmerCounts.cpp:93-96)
            if (flags & BT_KC_MULTICLUSTER_OCC) f |= 4;
        }
        list_flags[j] = f;
    }
}
// 1 at the first text position of every non-excluded distinct (cluster, k-mer): its prefix sum is the reference's row numbering
__global__ __launch_bounds__(BLOCK) void first_flag_kernel(IndexA A, const uint8_t *__restrict__ valid, const uint32_t *__restrict__ pos_slot_a,
                                                            const uint8_t *__restrict__ list_flags, uint64_t L, uint32_t *__restrict__ flag) {
    for (uint64_t pos = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; pos < L; pos += (uint64_t)gridDim.x * BLOCK) {
        uint32_t f = 0;
        if (valid[pos]) {
            const uint32_t a = pos_slot_a[pos];
            f = (A.first[a] == pos && !(list_flags[A.list_id[a]] & 2)) ? 1u : 0u;
        }
        flag[pos] = f;
    }
}
// block-wise exclusive scan: 1024 elements per workgroup (4 per lane); block totals to `sums`
__global__ __launch_bounds__(BLOCK) void scan_block_kernel(const uint32_t *__restrict__ in, uint64_t n, uint32_t *__restrict__ out, uint32_t *__restrict__ sums) {
    __shared__ uint32_t part[BLOCK];
    const uint64_t base = (uint64_t)blockIdx.x * (BLOCK * 4) + (uint64_t)threadIdx.x * 4;
    uint32_t v[4], s = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        v[q] = base + q < n ? in[base + q] : 0u;
        s += v[q];
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (unsigned off = 1; off < BLOCK; off <<= 1) {   // Hillis-Steele over the 256 lane totals
        const uint32_t add = threadIdx.x >= off ? part[threadIdx.x - off] : 0u;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - s;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (base + q < n) out[base + q] = run;
        run += v[q];
    }
    if (threadIdx.x == BLOCK - 1) sums[blockIdx.x] = part[BLOCK - 1];
}
__global__ __launch_bounds__(BLOCK) void scan_add_kernel(uint32_t *__restrict__ out, uint64_t n, const uint32_t *__restrict__ block_off) {
    const uint64_t base = (uint64_t)blockIdx.x * (BLOCK * 4) + (uint64_t)threadIdx.x * 4;
    const uint32_t add = block_off[blockIdx.x];
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (base + q < n) out[base + q] += add;
}
// per row: key, table record
__global__ __launch_bounds__(BLOCK) void rows_kernel(IndexA A, TableView t, const uint8_t *__restrict__ valid, const uint32_t *__restrict__ pos_slot_a,
                                                      const uint32_t *__restrict__ flag, const uint32_t *__restrict__ row_of_pos, const int64_t *__restrict__ slots,
                                                      const uint8_t *__restrict__ list_flags, const uint32_t *__restrict__ pos_path,
                                                      const uint32_t *__restrict__ path_cluster, uint64_t L, uint32_t S, uint32_t *__restrict__ a_row,
                                                      uint64_t *__restrict__ row_key, uint8_t *__restrict__ row_flags, uint8_t *__restrict__ row_counts,
                                                      uint8_t *__restrict__ row_ic, uint32_t *__restrict__ row_cluster) {
    for (uint64_t pos = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; pos < L; pos += (uint64_t)gridDim.x * BLOCK) {
        if (!flag[pos]) continue;
        const uint32_t a = pos_slot_a[pos], row = row_of_pos[pos], j = A.list_id[a];
        a_row[a] = row;
        row_key[2 * (uint64_t)row] = A.lo[a];
        row_key[2 * (uint64_t)row + 1] = A.hi[a];
        row_flags[row] = list_flags[j];
        row_cluster[row] = path_cluster[pos_path[pos]];
        const int64_t slot = slots[j];
        for (uint32_t s = 0; s < S; ++s) row_counts[(uint64_t)row * S + s] = slot >= 0 ? t.count_bytes((uint64_t)slot)[s] : (uint8_t)0;
        const uint32_t meta = slot >= 0 ? *t.meta((uint64_t)slot) : 0u;
        row_ic[2 * (uint64_t)row] = (uint8_t)((meta >> 16) & 0xffu);
        row_ic[2 * (uint64_t)row + 1] = (uint8_t)((meta >> 24) & 0xffu);
    }
}
// haplotype_kmer_multiplicities(row, path) = multiplicity of the k-mer on that path (one writer per cell)
__global__ __launch_bounds__(BLOCK) void mult_kernel(IndexA A, IndexB B, const uint8_t *__restrict__ list_flags, const uint32_t *__restrict__ a_row,
                                                      const uint32_t *__restrict__ path_cluster, const uint32_t *__restrict__ path_local,
                                                      const uint32_t *__restrict__ cluster_row0, const uint64_t *__restrict__ cluster_mult0,
                                                      const uint32_t *__restrict__ cluster_h, uint8_t *__restrict__ mult, uint32_t *__restrict__ over127) {
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i <= B.mask; i += (uint64_t)gridDim.x * BLOCK) {
        if (B.state[i] != ST_READY) continue;
        const uint32_t a = B.slot_a[i];
        if (list_flags[A.list_id[a]] & 2) continue;
        const uint32_t gp = B.gpath[i], c = path_cluster[gp];
        const uint32_t local_row = a_row[a] - cluster_row0[c];
        if (B.count[i] > 127u) atomicOr(over127, 1u);   // the reference asserts <= 127 (VariantClusterGraph.cpp:1060)
        mult[cluster_mult0[c] + (uint64_t)local_row * cluster_h[c] + path_local[gp]] = (uint8_t)B.count[i];
    }
}
// updateVariantPathIndices: one (row, variant, path) triple per window and running variant that covers its last nucleotide
struct Interval {
    uint32_t first, second;
    uint16_t variant, pad;
};
__global__ __launch_bounds__(BLOCK) void triples_kernel(IndexA A, const uint8_t *__restrict__ valid, const uint32_t *__restrict__ pos_slot_a,
                                                         const uint8_t *__restrict__ list_flags, const uint32_t *__restrict__ a_row, const uint32_t *__restrict__ pos_path,
                                                         const uint32_t *__restrict__ pos_nt, const uint32_t *__restrict__ path_local,
                                                         const uint32_t *__restrict__ iv_off, const Interval *__restrict__ iv, uint64_t L,
                                                         unsigned long long *__restrict__ cursor, const uint32_t *__restrict__ row_off, uint32_t *__restrict__ row_cnt,
                                                         uint32_t *__restrict__ out /* null: count pass */) {
    // count pass: row_cnt[row] = triples of the row, *cursor = triples of the batch (64 bits: the caller refuses 2^32 or more before any 32-bit count is used).
    // write pass: a triple goes to the next free place of ITS ROW's segment [row_off[row], row_off[row + 1]) as (variant << 16 | path); the order inside a
    // segment is the arrival order, and nothing downstream depends on it (row_entries_*: distinct variants ascending, OR over the paths).
    for (uint64_t pos = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; pos < L; pos += (uint64_t)gridDim.x * BLOCK) {
        if (!valid[pos]) continue;
        const uint32_t a = pos_slot_a[pos];
        if (list_flags[A.list_id[a]] & 2) continue;
        const uint32_t gp = pos_path[pos], nt = pos_nt[pos], row = a_row[a];
        uint32_t n = 0;
        for (uint32_t e = iv_off[gp]; e < iv_off[gp + 1]; ++e) {
            if (iv[e].first <= nt && nt < iv[e].second) {
                if (out) {
                    const uint32_t j = row_off[row] + atomicAdd(&row_cnt[row], 1u);
                    if (j < row_off[row + 1]) out[j] = ((uint32_t)iv[e].variant << 16) | (path_local[gp] & 0xffffu);
                }
                ++n;
            }
        }
        if (!out && n) {
            atomicAdd(&row_cnt[row], n);
            atomicAdd(cursor, (unsigned long long)n);
        }
    }
}

// ---- variant_haplotype_indices of a row from its triples, without a global sort ----
// A row's entries are its DISTINCT variants in ascending order, an entry's bitset the OR over the entry's paths.  Rows are independent, so every row is
// handled by the smallest unit that holds it: a lane (a sorting network over registers), a wavefront (register bitonic over __shfl_xor) or a workgroup.
// The workgroup path does not sort: the variant index is 16 bits wide, so the set of a row's variants is a 65536-bit map in LDS, an entry's rank the number
// of set bits below it; it holds for a row of any length.  Each path runs twice: count (row_nnz[row] = entries) and, after the scan that makes kv_off, write.
constexpr uint32_t ROW_LANE_MAX = 8, ROW_WAVE_MAX = 64, ROW_MAP_WORDS = 2048;
struct RowJob {
    const uint32_t *trip, *row_off;        // triples, [R+1] segments
    uint32_t *row_nnz;                     // count pass: entries per row
    const uint32_t *kv_off;                // write pass: [R+1]
    const uint32_t *row_cluster;           // [R]
    const uint32_t *cluster_h, *cluster_kv0;   // [C] haplotypes, first entry of the cluster
    const uint64_t *cluster_kvb;           // [C] first bitset word of the cluster
    uint16_t *kv_var;
    uint32_t *kv_bits;
    uint32_t write;
    __device__ inline uint32_t *bits_of(uint32_t row, uint32_t &hw) const {
        const uint32_t c = row_cluster[row];
        hw = (cluster_h[c] + 31u) / 32u;
        return kv_bits + cluster_kvb[c] + (uint64_t)(kv_off[row] - cluster_kv0[c]) * hw;
    }
};
// one lane per row of at most ROW_LANE_MAX (<= 8) triples; longer rows are handed to the wavefront / workgroup lists (count pass only)
__global__ __launch_bounds__(BLOCK) void row_entries_lane_kernel(RowJob J, uint64_t R, uint32_t lane_max, uint32_t wave_max, uint32_t *__restrict__ wave_list,
                                                                  uint32_t wave_cap, uint32_t *__restrict__ block_list, uint32_t block_cap,
                                                                  uint32_t *__restrict__ list_n /* [0] wave, [1] block */) {
    for (uint64_t row = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; row < R; row += (uint64_t)gridDim.x * BLOCK) {
        const uint32_t t0 = J.row_off[row], n = J.row_off[row + 1] - t0;
        if (n > lane_max) {
            if (!J.write) {
                if (n <= wave_max) {
                    const uint32_t j = atomicAdd(&list_n[0], 1u);
                    if (j < wave_cap) wave_list[j] = (uint32_t)row;
                } else {
                    const uint32_t j = atomicAdd(&list_n[1], 1u);
                    if (j < block_cap) block_list[j] = (uint32_t)row;
                }
            }
            continue;
        }
        uint32_t v[ROW_LANE_MAX];
#pragma unroll
        for (uint32_t i = 0; i < ROW_LANE_MAX; ++i) v[i] = i < n ? J.trip[t0 + i] : 0xFFFFFFFFu;
#pragma unroll
        for (uint32_t round = 0; round < ROW_LANE_MAX; ++round)   // odd-even transposition network, fully unrolled: v stays in registers
#pragma unroll
            for (uint32_t i = round & 1u; i + 1 < ROW_LANE_MAX; i += 2) {
                const uint32_t lo = min(v[i], v[i + 1]), hi = max(v[i], v[i + 1]);
                v[i] = lo;
                v[i + 1] = hi;
            }
        uint32_t hw = 0, e = 0;
        uint32_t *bits = J.write && n ? J.bits_of((uint32_t)row, hw) : nullptr;
        uint16_t *var = J.kv_var + (J.write ? J.kv_off[row] : 0u);
#pragma unroll
        for (uint32_t i = 0; i < ROW_LANE_MAX; ++i) {
            if (i >= n) continue;
            if (i == 0 || (v[i] >> 16) != (v[i - (i ? 1 : 0)] >> 16)) {
                if (J.write) var[e] = (uint16_t)(v[i] >> 16);
                ++e;
            }
            if (J.write) bits[(uint64_t)(e - 1) * hw + ((v[i] & 0xffffu) >> 5)] |= 1u << (v[i] & 31u);   // this lane owns the row's words (zeroed before)
        }
        if (!J.write) J.row_nnz[row] = e;
    }
}
// one wavefront per listed row of at most 64 triples: bitonic sort of (variant, path) across the lanes, heads of equal-variant runs are the entries
__global__ __launch_bounds__(BLOCK) void row_entries_wave_kernel(RowJob J, const uint32_t *__restrict__ list, uint32_t nlist) {
    const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (BLOCK / 64);
    for (uint32_t item = blockIdx.x * (BLOCK / 64) + threadIdx.x / 64; item < nlist; item += waves) {
        const uint32_t row = list[item], t0 = J.row_off[row], n = min(J.row_off[row + 1] - t0, 64u);
        uint32_t x = lane < n ? J.trip[t0 + lane] : 0xFFFFFFFFu;
#pragma unroll
        for (uint32_t k = 2; k <= 64; k <<= 1)
#pragma unroll
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                const uint32_t y = (uint32_t)__shfl_xor((int)x, (int)j, 64);
                const bool keep_min = ((lane & k) == 0) == ((lane & j) == 0);
                x = keep_min ? min(x, y) : max(x, y);
            }
        const uint32_t prev = (uint32_t)__shfl_up((int)x, 1, 64);
        const bool head = lane < n && (lane == 0 || (prev >> 16) != (x >> 16));
        const unsigned long long heads = __ballot(head);
        if (!J.write) {
            if (lane == 0) J.row_nnz[row] = (uint32_t)__popcll(heads);
            continue;
        }
        const uint32_t e = (uint32_t)__popcll(heads & (lane == 63 ? ~0ULL : ((2ULL << lane) - 1ULL))) - 1u;   // heads at or before this lane, minus one
        uint32_t hw = 0;
        uint32_t *bits = J.bits_of(row, hw);
        if (head) J.kv_var[J.kv_off[row] + e] = (uint16_t)(x >> 16);
        if (lane < n) atomicOr(&bits[(uint64_t)e * hw + ((x & 0xffffu) >> 5)], 1u << (x & 31u));
    }
}
// one workgroup per listed row, any number of triples: the row's variants as a bit map over the 16-bit variant index, ranks by a prefix sum of popcounts
__global__ __launch_bounds__(BLOCK) void row_entries_block_kernel(RowJob J, const uint32_t *__restrict__ list, uint32_t nlist) {
    __shared__ uint32_t map[ROW_MAP_WORDS], before[ROW_MAP_WORDS], part[BLOCK];
    constexpr uint32_t PER = ROW_MAP_WORDS / BLOCK;
    const uint32_t tid = threadIdx.x;
    for (uint32_t item = blockIdx.x; item < nlist; item += gridDim.x) {
        const uint32_t row = list[item], t0 = J.row_off[row], n = J.row_off[row + 1] - t0;
        for (uint32_t i = tid; i < ROW_MAP_WORDS; i += BLOCK) map[i] = 0;
        __syncthreads();
        for (uint32_t i = tid; i < n; i += BLOCK) {
            const uint32_t var = J.trip[t0 + i] >> 16;
            atomicOr(&map[var >> 5], 1u << (var & 31u));
        }
        __syncthreads();
        uint32_t s = 0;
#pragma unroll
        for (uint32_t q = 0; q < PER; ++q) {
            before[tid * PER + q] = s;
            s += (uint32_t)__popc(map[tid * PER + q]);
        }
        part[tid] = s;
        __syncthreads();
        for (uint32_t off = 1; off < BLOCK; off <<= 1) {
            const uint32_t add = tid >= off ? part[tid - off] : 0u;
            __syncthreads();
            part[tid] += add;
            __syncthreads();
        }
        const uint32_t base = part[tid] - s;
#pragma unroll
        for (uint32_t q = 0; q < PER; ++q) before[tid * PER + q] += base;
        __syncthreads();
        if (!J.write) {
            if (tid == 0) J.row_nnz[row] = part[BLOCK - 1];
        } else {
            uint32_t hw = 0;
            uint32_t *bits = J.bits_of(row, hw);
            uint16_t *var_out = J.kv_var + J.kv_off[row];
            for (uint32_t w = tid; w < ROW_MAP_WORDS; w += BLOCK) {
                uint32_t m = map[w], e = before[w];
                while (m) {
                    var_out[e++] = (uint16_t)(w * 32u + (uint32_t)__ffs((int)m) - 1u);
                    m &= m - 1u;
                }
            }
            for (uint32_t i = tid; i < n; i += BLOCK) {
                const uint32_t t = J.trip[t0 + i], var = t >> 16;
                const uint32_t e = before[var >> 5] + (uint32_t)__popc(map[var >> 5] & ((1u << (var & 31u)) - 1u));
                atomicOr(&bits[(uint64_t)e * hw + ((t & 0xffffu) >> 5)], 1u << (t & 31u));
            }
        }
        __syncthreads();   // (the next row clears the map)
    }
}

// ---- row lists: kmer_has_counts, and the stable split of a cluster's rows into unique / multicluster (first-seen = row order) ----
__global__ __launch_bounds__(BLOCK) void row_flags_kernel(const uint8_t *__restrict__ row_flags, uint64_t R, uint32_t *__restrict__ is_multi, uint8_t *__restrict__ has_counts) {
    for (uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; r < R; r += (uint64_t)gridDim.x * BLOCK) {
        is_multi[r] = (row_flags[r] >> 2) & 1u;
        has_counts[r] = row_flags[r] & 1u;
    }
}
// multi_before[r] = multicluster rows before row r in the batch: the row's place in multi_idx, or r - multi_before[r] in unique_idx (ids local to the cluster)
__global__ __launch_bounds__(BLOCK) void row_lists_kernel(const uint8_t *__restrict__ row_flags, const uint32_t *__restrict__ multi_before, const uint32_t *__restrict__ row_cluster,
                                                           const uint32_t *__restrict__ kmer_off, uint64_t R, uint32_t *__restrict__ unique_idx, uint32_t *__restrict__ multi_idx) {
    for (uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; r < R; r += (uint64_t)gridDim.x * BLOCK) {
        const uint32_t local = (uint32_t)r - kmer_off[row_cluster[r]];
        if (row_flags[r] & 4) multi_idx[multi_before[r]] = local;
        else unique_idx[(uint32_t)r - multi_before[r]] = local;
    }
}

// ---- shared records of multicluster k-mers (KmerCounter.cpp:607-616): inside a group, walking its clusters in vertex order and each cluster's multi_idx in
// order, distinct keys are numbered by first occurrence.  The multicluster rows of a group are a contiguous range of multi_idx (its clusters are), in exactly
// that order, so with m = a row's place in multi_idx: first(m) = the smallest m of the same (group, key) (atomicMin over an open-addressing index: the SLOT an
// entry gets depends on arrival, the minimum does not), number(m) = first occurrences before first(m) in the group (a prefix sum). ----
__global__ __launch_bounds__(BLOCK) void shared_index_kernel(const uint32_t *__restrict__ multi_idx, const uint32_t *__restrict__ multi_off, const uint32_t *__restrict__ kmer_off,
                                                              const uint32_t *__restrict__ cluster_group, uint32_t C, const uint64_t *__restrict__ row_key, uint32_t M,
                                                              uint64_t *__restrict__ klo, uint64_t *__restrict__ khi, uint32_t *__restrict__ ktag, uint32_t *__restrict__ kstate,
                                                              uint32_t *__restrict__ kfirst, uint64_t mask, uint32_t *__restrict__ item_slot, uint32_t *__restrict__ item_row) {
    for (uint32_t m = blockIdx.x * BLOCK + threadIdx.x; m < M; m += gridDim.x * BLOCK) {
        uint32_t lo = 0, hi = C;   // last cluster with multi_off[c] <= m (empty clusters repeat an offset: the last one is the owner)
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (multi_off[mid] <= m) lo = mid;
            else hi = mid;
        }
        const uint32_t row = kmer_off[lo] + multi_idx[m];
        const uint64_t slot = index_insert(klo, khi, ktag, kstate, mask, row_key[2 * (uint64_t)row], row_key[2 * (uint64_t)row + 1], cluster_group[lo]);
        atomicMin(&kfirst[slot], m);
        item_slot[m] = (uint32_t)slot;
        item_row[m] = row;
    }
}
__global__ __launch_bounds__(BLOCK) void shared_first_kernel(const uint32_t *__restrict__ item_slot, const uint32_t *__restrict__ kfirst, uint32_t M, uint32_t *__restrict__ is_first) {
    for (uint32_t m = blockIdx.x * BLOCK + threadIdx.x; m < M; m += gridDim.x * BLOCK) is_first[m] = kfirst[item_slot[m]] == m ? 1u : 0u;
}
__global__ __launch_bounds__(BLOCK) void shared_number_kernel(const uint32_t *__restrict__ item_slot, const uint32_t *__restrict__ item_row, const uint32_t *__restrict__ kfirst,
                                                               const uint32_t *__restrict__ ktag, const uint32_t *__restrict__ firsts_before,
                                                               const uint32_t *__restrict__ group_m0, uint32_t M, int32_t *__restrict__ kmer_shared) {
    for (uint32_t m = blockIdx.x * BLOCK + threadIdx.x; m < M; m += gridDim.x * BLOCK) {
        const uint32_t slot = item_slot[m];
        kmer_shared[item_row[m]] = (int32_t)(firsts_before[kfirst[slot]] - firsts_before[group_m0[ktag[slot]]]);
    }
}
__global__ __launch_bounds__(BLOCK) void gather_u32_idx32_kernel(const uint32_t *__restrict__ in, const uint32_t *__restrict__ idx, uint32_t n, uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) out[i] = in[idx[i]];
}

__global__ __launch_bounds__(BLOCK) void gather_u32_kernel(const uint32_t *__restrict__ in, const uint64_t *__restrict__ idx, uint32_t n, uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) out[i] = in[idx[i]];
}

template <typename T>
int dev_alloc(T **p, uint64_t n, std::vector<void *> &owned) {
    *p = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(p), std::max<uint64_t>(n, 1) * sizeof(T));
    if (e != hipSuccess) return fail(std::string("bt_paths: device allocation of ") + std::to_string(n * sizeof(T)) + " bytes: " + hipGetErrorString(e));
    owned.push_back(*p);
    return BT_OK;
}

uint64_t pow2_at_least(uint64_t n) {
    uint64_t c = 16;
    while (c < n) c <<= 1;
    return c;
}

}  // namespace

struct bt_paths {
    bt_ctx *ctx = nullptr;
    uint32_t k = 0, C = 0;
    // host copies of what the host-side half needs
    std::vector<uint32_t> vertex_off, num_paths, vertex_nested, refvar_off, var_off;
    std::vector<uint64_t> seq_off, path_off;
    std::vector<uint16_t> vertex_variant, vertex_allele, refvar, var_num_alleles;
    std::vector<uint8_t> vertex_flags, path_vertices, var_has_dependency;
    std::vector<uint32_t> path_cluster, path_local, cluster_path0;   // global path ids
    uint64_t num_gpaths = 0, L = 0, num_valid = 0;
    std::vector<void *> owned;
    // device
    uint8_t *d_seq = nullptr;
    char *d_text = nullptr;
    uint32_t *d_pos_path = nullptr, *d_pos_nt = nullptr, *d_pos_slot_a = nullptr;
    uint64_t *d_kmers = nullptr;
    uint8_t *d_valid = nullptr;
    uint32_t *d_path_cluster = nullptr, *d_path_local = nullptr, *d_iv_off = nullptr;
    Interval *d_iv = nullptr;
    IndexA A{};
    IndexB B{};
    bool indexed = false;
    uint64_t n_list = 0;
    uint64_t *d_list_kmers = nullptr;
    uint8_t *d_list_mult = nullptr, *d_list_excluded = nullptr, *d_list_flags = nullptr;
    uint32_t *d_list_cluster = nullptr;
    int64_t *d_list_slots = nullptr;
    std::vector<uint64_t> cluster_text0;   // first text position of each cluster (+ L at the end)
    bt_multigroup_stats mg_stats{};        // how the last bt_paths_count_multigroup call ordered its groups (bt_paths_multigroup_info)
    // candidates result (host)
    bool have_candidates = false;
    uint32_t S = 0;
    std::vector<uint32_t> kmer_off, kv_off, unique_off, unique_idx, multi_off, multi_idx, hapnest_off, hapnest_idx, nestdep_off, nestdep_cluster, nestdep_var_off, kv_bits;
    std::vector<uint8_t> mult, has_counts, counts, ic;
    std::vector<uint64_t> key;
    std::vector<uint16_t> kv_var, hap_allele, nestdep_var;
    // candidates result (device): the per-row / per-entry arrays of bt_paths_candidates_device, until a source takes them or the handle goes
    bool cand_on_device = false;
    std::vector<void *> cand_owned;
    uint64_t R = 0, nnz = 0, kv_words = 0, mult_bytes = 0, num_unique = 0, num_multi = 0;
    std::vector<uint32_t> cluster_kv0;   // [C+1] first incidence entry of each cluster
    uint8_t *d_mult = nullptr, *d_has_counts = nullptr, *d_counts = nullptr, *d_ic = nullptr;
    uint64_t *d_key = nullptr;
    uint32_t *d_kv_off = nullptr, *d_kv_bits = nullptr, *d_unique_idx = nullptr, *d_multi_idx = nullptr;
    uint16_t *d_kv_var = nullptr;
    void drop_device_candidates() {
        for (void *q : cand_owned) (void)hipFree(q);
        cand_owned.clear();
        cand_on_device = false;
        d_mult = d_has_counts = d_counts = d_ic = nullptr;
        d_key = nullptr;
        d_kv_off = d_kv_bits = d_unique_idx = d_multi_idx = nullptr;
        d_kv_var = nullptr;
    }
};

namespace {

// host threads of the assembly steps: BT_HOST_THREADS (the executable sets it from -p), else up to 16; never more than one per 256 items
unsigned host_threads(uint64_t items) {
    unsigned t = 0;
    if (const char *e = getenv("BT_HOST_THREADS")) t = (unsigned)std::max(1, atoi(e));
    else t = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(t, items / 256 + 1));
}
// fn(t) for t in [0, T) on T threads (the caller's included); the first exception of any of them is rethrown after all have been joined
template <typename F>
void run_on_threads(unsigned T, F &&fn) {
    if (T <= 1) {
        fn(0u);
        return;
    }
    std::vector<std::exception_ptr> err(T);
    auto guarded = [&](unsigned t) {
        try {
            fn(t);
        } catch (...) {
            err[t] = std::current_exception();
        }
    };
    std::vector<std::thread> pool;
    try {
        for (unsigned t = 1; t < T; ++t) pool.emplace_back(guarded, t);
    } catch (...) {   // (a thread could not be started: the ranges of the missing threads are run here)
        for (unsigned t = (unsigned)pool.size() + 1; t < T; ++t) guarded(t);
    }
    guarded(0u);
    for (auto &th : pool) th.join();
    for (auto &e : err)
        if (e) std::rethrow_exception(e);
}

// Host half of getHaplotypeCandidates for one path: running-variant intervals in path-nucleotide coordinates
// (VariantClusterGraph.cpp:984-1011), haplotype allele indices (:990-996,1095-1102), nested cluster list (:1013-1017,1093)
void walk_path_host(const bt_paths &p, uint32_t c, uint32_t lp, std::vector<Interval> &iv, std::vector<uint16_t> &alleles, std::vector<uint32_t> &nested) {
    const uint32_t v0 = p.vertex_off[c], nv = p.vertex_off[c + 1] - v0, V = p.var_off[c + 1] - p.var_off[c];
    const uint8_t *row = p.path_vertices.data() + p.path_off[c] + (uint64_t)lp * nv;
    alleles.assign(V, 0xFFFF);
    nested.clear();
    std::map<std::pair<uint16_t, uint16_t>, size_t> open;   // (variant, allele) -> index into iv of its current interval
    uint32_t nn = 0;
    for (uint32_t vi = 0; vi < nv; ++vi) {
        if (!row[vi]) continue;
        const uint32_t v = v0 + vi;
        const uint32_t len = (uint32_t)(p.seq_off[v + 1] - p.seq_off[v]);
        if (p.vertex_variant[v] != 0xFFFF) {
            if (!(p.vertex_flags[v] & 1)) alleles[p.vertex_variant[v]] = p.vertex_allele[v];
            const auto key = std::make_pair(p.vertex_variant[v], p.vertex_allele[v]);
            auto it = open.find(key);
            // the reference's emplace keeps an existing entry only while it is still alive, i.e. ends exactly at nn + k - 1
            if (it == open.end() || iv[it->second].second != nn + p.k - 1) {
                iv.push_back(Interval{nn + ((p.vertex_flags[v] >> 1) & 1u), nn + p.k - 1, p.vertex_variant[v], 0});
                open[key] = iv.size() - 1;
                it = open.find(key);
            }
            iv[it->second].second += len;
        }
        for (uint32_t r = p.refvar_off[v]; r < p.refvar_off[v + 1]; ++r) {
            auto it = open.find(std::make_pair(p.refvar[r], (uint16_t)0));
            if (it != open.end() && iv[it->second].second == nn + p.k - 1) iv[it->second].second += len;
        }
        if (p.vertex_nested[v] != 0xFFFFFFFFu) nested.push_back(p.vertex_nested[v]);
        nn += len;
    }
    std::sort(nested.begin(), nested.end());
    for (uint32_t var = 0; var < V; ++var)
        if (alleles[var] == 0xFFFF) alleles[var] = (uint16_t)(p.var_num_alleles[p.var_off[c] + var] - 1);
}

int build_index(bt_paths *p) {
    if (p->indexed) return BT_OK;
    const uint64_t cap = pow2_at_least(2 * std::max<uint64_t>(p->num_valid, 8));
    IndexA &A = p->A;
    IndexB &B = p->B;
#define TRY(x)                         \
    do {                               \
        const int _rc = (x);           \
        if (_rc != BT_OK) return _rc;  \
    } while (0)
    TRY(dev_alloc(&A.lo, cap, p->owned));
    TRY(dev_alloc(&A.hi, cap, p->owned));
    TRY(dev_alloc(&A.cluster, cap, p->owned));
    TRY(dev_alloc(&A.state, cap, p->owned));
    TRY(dev_alloc(&A.maxmult, cap, p->owned));
    TRY(dev_alloc(&A.list_id, cap, p->owned));
    TRY(dev_alloc(&A.first, cap, p->owned));
    A.mask = cap - 1;
    TRY(dev_alloc(&B.lo, cap, p->owned));
    TRY(dev_alloc(&B.hi, cap, p->owned));
    TRY(dev_alloc(&B.gpath, cap, p->owned));
    TRY(dev_alloc(&B.state, cap, p->owned));
    TRY(dev_alloc(&B.count, cap, p->owned));
    TRY(dev_alloc(&B.slot_a, cap, p->owned));
    B.mask = cap - 1;
    TRY(dev_alloc(&p->d_pos_slot_a, p->L, p->owned));
    hipStream_t st = p->ctx->stream;
    BT_HIP(hipMemsetAsync(A.state, 0, cap * 4, st));
    BT_HIP(hipMemsetAsync(A.maxmult, 0, cap * 4, st));
    BT_HIP(hipMemsetAsync(A.first, 0xFF, cap * 8, st));
    BT_HIP(hipMemsetAsync(B.state, 0, cap * 4, st));
    BT_HIP(hipMemsetAsync(B.count, 0, cap * 4, st));
    const unsigned maxb = p->ctx->num_cu * 16;
    hipLaunchKernelGGL(index_kernel, dim3(grid_for(p->L, BLOCK, maxb)), dim3(BLOCK), 0, st, A, B, p->d_kmers, p->d_valid, p->d_pos_path, p->d_path_cluster, p->L,
                       p->d_pos_slot_a);
    BT_CHECK_LAUNCH();
    hipLaunchKernelGGL(maxmult_kernel, dim3(grid_for(cap, BLOCK, maxb)), dim3(BLOCK), 0, st, A, B);
    BT_CHECK_LAUNCH();
    // dense list of the distinct (cluster, k-mer) entries
    unsigned long long *d_cursor = nullptr;
    TRY(dev_alloc(&d_cursor, 1, p->owned));
    BT_HIP(hipMemsetAsync(d_cursor, 0, 8, st));
    TRY(dev_alloc(&p->d_list_kmers, 2 * p->num_valid, p->owned));
    TRY(dev_alloc(&p->d_list_mult, p->num_valid, p->owned));
    TRY(dev_alloc(&p->d_list_cluster, p->num_valid, p->owned));
    TRY(dev_alloc(&p->d_list_excluded, p->num_valid, p->owned));
    TRY(dev_alloc(&p->d_list_flags, p->num_valid, p->owned));
    TRY(dev_alloc(&p->d_list_slots, p->num_valid, p->owned));
    hipLaunchKernelGGL(list_kernel, dim3(grid_for(cap, BLOCK, maxb)), dim3(BLOCK), 0, st, A, p->d_list_kmers, p->d_list_mult, p->d_list_cluster, d_cursor);
    BT_CHECK_LAUNCH();
    unsigned long long n = 0;
    BT_HIP(hipMemcpyAsync(&n, d_cursor, 8, hipMemcpyDeviceToHost, st));
    BT_HIP(hipStreamSynchronize(st));
    p->n_list = n;
    p->indexed = true;
    return BT_OK;
#undef TRY
}

}  // namespace

extern "C" {

int bt_paths_create(bt_ctx *ctx, const bt_paths_batch *b, uint32_t k, bt_paths **out, uint64_t *h_num_kmer_occurrences) {
    if (!ctx || !b || !out) return fail("bt_paths_create: null argument");
    if (k < 1 || k > 64) return fail("bt_paths_create: k must be in 1..64");
    if (b->num_clusters == 0) return fail("bt_paths_create: empty batch");
    BT_HIP(hipSetDevice(ctx->device));
    bt_paths *p = new bt_paths();
    p->ctx = ctx;
    p->k = k;
    p->C = b->num_clusters;
    const uint32_t C = p->C, NV = b->vertex_off[C];
    p->vertex_off.assign(b->vertex_off, b->vertex_off + C + 1);
    p->num_paths.assign(b->num_paths, b->num_paths + C);
    p->seq_off.assign(b->seq_off, b->seq_off + NV + 1);
    p->vertex_variant.assign(b->vertex_variant, b->vertex_variant + NV);
    p->vertex_allele.assign(b->vertex_allele, b->vertex_allele + NV);
    p->vertex_flags.assign(b->vertex_flags, b->vertex_flags + NV);
    p->vertex_nested.assign(b->vertex_nested, b->vertex_nested + NV);
    p->refvar_off.assign(b->refvar_off, b->refvar_off + NV + 1);
    p->refvar.assign(b->refvar, b->refvar + p->refvar_off[NV]);
    p->path_off.assign(b->path_off, b->path_off + C + 1);
    p->path_vertices.assign(b->path_vertices, b->path_vertices + p->path_off[C]);
    p->var_off.assign(b->var_off, b->var_off + C + 1);
    p->var_num_alleles.assign(b->var_num_alleles, b->var_num_alleles + p->var_off[C]);
    p->var_has_dependency.assign(b->var_has_dependency, b->var_has_dependency + p->var_off[C]);
    // ---- segments: text layout of every path ----
    std::vector<Seg> segs;
    std::vector<uint32_t> iv_off(1, 0);
    std::vector<Interval> iv;
    uint64_t at = 0;
    p->cluster_path0.assign(C + 1, 0);
    std::vector<uint16_t> alleles;
    std::vector<uint32_t> nested;
    for (uint32_t c = 0; c < C; ++c) {
        const uint32_t v0 = p->vertex_off[c], nv = p->vertex_off[c + 1] - v0;
        if (p->path_off[c + 1] - p->path_off[c] != (uint64_t)p->num_paths[c] * nv) {
            delete p;
            return fail("bt_paths_create: path_off does not match num_paths x vertices");
        }
        p->cluster_text0.push_back(at);
        p->cluster_path0[c] = (uint32_t)p->path_cluster.size();
        for (uint32_t lp = 0; lp < p->num_paths[c]; ++lp) {
            const uint32_t gp = (uint32_t)p->path_cluster.size();
            p->path_cluster.push_back(c);
            p->path_local.push_back(lp);
            const uint8_t *row = p->path_vertices.data() + p->path_off[c] + (uint64_t)lp * nv;
            uint32_t nn = 0;
            for (uint32_t vi = 0; vi < nv; ++vi) {
                if (!row[vi]) continue;
                const uint32_t v = v0 + vi;
                const uint32_t len = (uint32_t)(p->seq_off[v + 1] - p->seq_off[v]);
                if (p->vertex_flags[v] & 1) ++at;   // kmer_pair.reset(): one separator position
                if (len) segs.push_back(Seg{at, p->seq_off[v], len, nn, gp, 0});
                at += len;
                nn += len;
            }
            ++at;   // separator between paths
            walk_path_host(*p, c, lp, iv, alleles, nested);
            iv_off.push_back((uint32_t)iv.size());
        }
    }
    p->cluster_path0[C] = (uint32_t)p->path_cluster.size();
    p->cluster_text0.push_back(at);
    p->num_gpaths = p->path_cluster.size();
    p->L = at;
    if (p->L >= (1ull << 32)) {
        delete p;
        return fail("bt_paths_create: more than 2^32 path nucleotides in one batch (split the unit)");
    }
    // ---- upload, build the text, enumerate the k-mers ----
    Seg *d_segs = nullptr;
    int rc = BT_OK;
    auto up = [&](auto **dst, const auto &vec) {
        if (rc != BT_OK) return;
        rc = dev_alloc(dst, vec.size(), p->owned);
        if (rc == BT_OK && !vec.empty() && hipMemcpy(*dst, vec.data(), vec.size() * sizeof(vec[0]), hipMemcpyHostToDevice) != hipSuccess) rc = fail("bt_paths_create: upload failed");
    };
    std::vector<uint8_t> seq(b->seq, b->seq + p->seq_off[NV]);
    up(&p->d_seq, seq);
    up(&d_segs, segs);
    up(&p->d_path_cluster, p->path_cluster);
    up(&p->d_path_local, p->path_local);
    up(&p->d_iv_off, iv_off);
    up(&p->d_iv, iv);
    if (rc == BT_OK) rc = dev_alloc(&p->d_text, p->L, p->owned);
    if (rc == BT_OK) rc = dev_alloc(&p->d_pos_path, p->L, p->owned);
    if (rc == BT_OK) rc = dev_alloc(&p->d_pos_nt, p->L, p->owned);
    if (rc == BT_OK) rc = dev_alloc(&p->d_kmers, 2 * p->L, p->owned);
    if (rc == BT_OK) rc = dev_alloc(&p->d_valid, p->L, p->owned);
    if (rc != BT_OK) {
        bt_paths_destroy(p);
        return rc;
    }
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(text_kernel, dim3(grid_for(p->L, BLOCK, ctx->num_cu * 16)), dim3(BLOCK), 0, st, d_segs, (uint64_t)segs.size(), p->d_seq, p->L, p->d_text,
                       p->d_pos_path, p->d_pos_nt);
    if (hipGetLastError() != hipSuccess || bt_kmers_from_sequence(ctx, p->d_text, p->L, k, p->d_kmers, p->d_valid) != BT_OK) {
        bt_paths_destroy(p);
        return fail("bt_paths_create: k-mer enumeration failed");
    }
    // number of windows
    std::vector<uint8_t> hv(p->L);
    if (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(hv.data(), p->d_valid, p->L, hipMemcpyDeviceToHost) != hipSuccess) {
        bt_paths_destroy(p);
        return fail("bt_paths_create: device error");
    }
    p->num_valid = std::accumulate(hv.begin(), hv.end(), (uint64_t)0);
    if (h_num_kmer_occurrences) *h_num_kmer_occurrences = p->num_valid;
    *out = p;
    return BT_OK;
}

// The iteration orders of G consecutive groups of distinct k-mers (steps 2 and 3 of bt_paths_count_multigroup; all of bt_kmer_set_orders).
// Group g holds the k-mers kmers[2 * seq[i]], i in [goff[g], goff[g + 1]) (goff: the host's copy of d_goff); the first group's container
// starts with initial_buckets buckets, every later one with what its predecessor left.  d_time[i] receives goff[g] + rank + 1.  Groups of
// at least wide_min k-mers (0: none) are ordered stage by stage on a workgroup each (mg_order_wide_kernel, launched first), the others by
// one lane each (mg_order_kernel); without a wide group the launches and allocations are the lane route's alone.  Device memory goes on
// `tmp` (the caller frees it, also after an error) and the host arrays the uploads read live in `up`, which the caller keeps until it has
// synchronised the stream; final_buckets (optional) receives every group's bucket count afterwards.
struct MgUploads {
    std::vector<uint64_t> moff, binit, area_off;
    std::vector<uint32_t> wide;   // the wide groups, in launch order
};
static int mg_group_orders(bt_ctx *ctx, const char *who, const uint64_t *d_kmers, const uint32_t *d_seq, const uint32_t *d_goff, const std::vector<uint32_t> &goff, uint32_t G,
                           unsigned k, uint64_t initial_buckets, uint32_t wide_min, uint32_t *d_time, uint64_t *final_buckets, bt_multigroup_stats &stats,
                           MgUploads &up, std::vector<void *> &tmp) {
    hipStream_t st = ctx->stream;
    const uint64_t n_total = goff[G];
    stats = bt_multigroup_stats{};
    stats.num_groups = G;
    stats.wide_min_kmers = wide_min;
    std::vector<uint64_t> &moff = up.moff, &binit = up.binit, &area_off = up.area_off;
    std::vector<uint32_t> &wide = up.wide;
    moff.assign(G + 1, 0);
    binit.assign(G + 1, 1);
    wide.clear();
    {
        uint64_t B = initial_buckets ? initial_buckets : 1;
        for (uint32_t g = 0; g < G; ++g) {
            const uint32_t n = goff[g + 1] - goff[g];
            const bool is_wide = wide_min && n && n >= wide_min;
            if (is_wide && n > (1u << 30)) return fail(std::string(who) + ": a group of more than 2^30 distinct path k-mers cannot take the workgroup route");
            binit[g] = B;
            if (is_wide) {
                MgStage stage = mg_stage_start(B);
                uint32_t stages = 0;
                while (stages <= MG_MAX_STAGES && mg_stage_next(n, stage)) ++stages;
                stats.max_stages = std::max(stats.max_stages, stages);
                wide.push_back(g);
            }
            // the set keeps its bucket count across clear(); a fresh set goes to 13 buckets with its first k-mer (for the next group's order 1 and 13 are
            // the same start: a fresh set's first insert rehashes an empty list to 13)
            while (B < n || (n && B <= 1)) B = std_next_bucket_count(B);
            if (B >= 0xFFFFFFFEull) return fail(std::string(who) + ": a group with more than 3.5e9 distinct path k-mers");
            if (final_buckets) final_buckets[g] = B;
            moff[g + 1] = moff[g] + (n && !is_wide ? pow2_at_least(2 * (uint64_t)n) : 0);   // (a wide group's bucket map is part of its work area)
            stats.max_group_kmers = std::max(stats.max_group_kmers, n);
        }
    }
    stats.num_wide_groups = (uint32_t)wide.size();
    uint64_t *d_moff = nullptr, *d_binit = nullptr;
    uint32_t *d_next = nullptr, *d_mk = nullptr, *d_mv = nullptr;
    int rc = BT_OK;
    auto A = [&](auto **q, uint64_t n) {
        if (rc == BT_OK) rc = dev_alloc(q, n, tmp);
    };
    A(&d_next, n_total); A(&d_moff, G + 1); A(&d_binit, G + 1); A(&d_mk, moff[G]); A(&d_mv, moff[G]);
    if (rc != BT_OK) return rc;
#define MGO(call)                                                                \
    do {                                                                         \
        const hipError_t _e = (call);                                            \
        if (_e != hipSuccess) return fail(std::string(who) + ": " + hipGetErrorString(_e)); \
    } while (0)
    MGO(hipMemcpyAsync(d_moff, moff.data(), (size_t)(G + 1) * 8, hipMemcpyHostToDevice, st));
    MGO(hipMemcpyAsync(d_binit, binit.data(), (size_t)(G + 1) * 8, hipMemcpyHostToDevice, st));
    uint32_t *d_err = nullptr;
    if (!wide.empty()) {
        // the largest groups first: the launch ends with its longest workgroup either way, the short ones fill in behind it
        std::stable_sort(wide.begin(), wide.end(), [&](uint32_t a, uint32_t b) { return goff[a + 1] - goff[a] > goff[b + 1] - goff[b]; });
        area_off.assign(wide.size(), 0);
        uint64_t words = 0;
        for (size_t i = 0; i < wide.size(); ++i) {
            area_off[i] = words;
            words += mg_layout(goff[wide[i] + 1] - goff[wide[i]]).total;
        }
        stats.wide_scratch_bytes = words * 4;
        uint32_t *d_wide = nullptr, *d_areas = nullptr;
        uint64_t *d_area_off = nullptr;
        A(&d_wide, wide.size()); A(&d_area_off, wide.size()); A(&d_areas, words); A(&d_err, 1);
        if (rc != BT_OK) return rc;
        MGO(hipMemcpyAsync(d_wide, wide.data(), wide.size() * 4, hipMemcpyHostToDevice, st));
        MGO(hipMemcpyAsync(d_area_off, area_off.data(), area_off.size() * 8, hipMemcpyHostToDevice, st));
        MGO(hipMemsetAsync(d_err, 0, 4, st));
        hipLaunchKernelGGL(mg_order_wide_kernel, dim3((unsigned)wide.size()), dim3(BLOCK), 0, st, d_kmers, d_seq, d_goff, d_binit, d_wide, d_area_off, d_areas, d_time, d_err, k);
    }
    if (G) hipLaunchKernelGGL(mg_order_kernel, dim3((G + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, d_kmers, d_seq, d_goff, d_moff, d_binit, d_next, d_mk, d_mv, d_time, G, k, wide_min);
    MGO(hipGetLastError());
    if (d_err) {
        uint32_t err = 0;
        MGO(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, st));
        MGO(hipStreamSynchronize(st));
        if (err) return fail(std::string(who) + ": the staged k-mer order of a wide group met a violated loop bound (code " + std::to_string(err) + ")");
    }
#undef MGO
    return BT_OK;
}

int bt_kmer_set_orders(bt_ctx *ctx, const uint64_t *h_kmers, const uint64_t *h_off, uint32_t G, unsigned k, uint64_t initial_buckets, uint32_t wide_min, uint32_t *h_rank,
                       uint64_t *h_final_buckets, bt_multigroup_stats *stats) {
    if (!ctx || !h_off || !h_rank || (!h_kmers && G && h_off[G])) return fail("bt_kmer_set_orders: null argument");
    if (k == 0 || k > 64) return fail("bt_kmer_set_orders: k must be in 1..64");
    std::vector<uint32_t> goff(G + 1);
    for (uint32_t g = 0; g <= G; ++g) {
        if (h_off[g] >= 0xFFFFFFFEull || (g && h_off[g] < h_off[g - 1]) || h_off[0] != 0) return fail("bt_kmer_set_orders: offsets must start at 0, ascend and stay below 2^32 - 2");
        goff[g] = (uint32_t)h_off[g];
    }
    BT_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t n_total = goff[G];
    std::vector<void *> tmp;
    uint64_t *d_kmers = nullptr;
    uint32_t *d_seq = nullptr, *d_goff = nullptr, *d_time = nullptr;
    int rc = dev_alloc(&d_kmers, 2 * n_total, tmp);
    if (rc == BT_OK) rc = dev_alloc(&d_seq, n_total, tmp);
    if (rc == BT_OK) rc = dev_alloc(&d_goff, G + 1, tmp);
    if (rc == BT_OK) rc = dev_alloc(&d_time, n_total, tmp);
    std::vector<uint32_t> seq(n_total), time(n_total);
    std::iota(seq.begin(), seq.end(), 0u);   // group g's k-mers are h_kmers[h_off[g] .. h_off[g + 1]) themselves
    auto hip_ok = [&](hipError_t e) {
        if (rc == BT_OK && e != hipSuccess) rc = fail(std::string("bt_kmer_set_orders: ") + hipGetErrorString(e));
    };
    if (rc == BT_OK && n_total) hip_ok(hipMemcpyAsync(d_kmers, h_kmers, n_total * 16, hipMemcpyHostToDevice, st));
    if (rc == BT_OK && n_total) hip_ok(hipMemcpyAsync(d_seq, seq.data(), n_total * 4, hipMemcpyHostToDevice, st));
    if (rc == BT_OK) hip_ok(hipMemcpyAsync(d_goff, goff.data(), (size_t)(G + 1) * 4, hipMemcpyHostToDevice, st));
    bt_multigroup_stats local{};
    MgUploads up;
    if (rc == BT_OK) rc = mg_group_orders(ctx, "bt_kmer_set_orders", d_kmers, d_seq, d_goff, goff, G, k, initial_buckets, wide_min, d_time, h_final_buckets, local, up, tmp);
    if (rc == BT_OK && n_total) hip_ok(hipMemcpyAsync(time.data(), d_time, n_total * 4, hipMemcpyDeviceToHost, st));
    hip_ok(hipStreamSynchronize(st));
    for (void *q : tmp) (void)hipFree(q);
    if (rc != BT_OK) return rc;
    for (uint32_t g = 0; g < G; ++g)
        for (uint32_t i = goff[g]; i < goff[g + 1]; ++i) h_rank[i] = time[i] - goff[g] - 1u;
    if (stats) *stats = local;
    return BT_OK;
}

int bt_paths_multigroup_info(bt_paths *p, bt_multigroup_stats *stats) {
    if (!p || !stats) return fail("bt_paths_multigroup_info: null argument");
    *stats = p->mg_stats;
    return BT_OK;
}

int bt_diag_kmer_set_order_staged(const uint64_t *h_kmers, uint32_t n, uint64_t initial_buckets, unsigned k, uint32_t *h_rank, uint64_t *h_final_buckets) {
    if (!h_kmers || !h_rank) return fail("bt_diag_kmer_set_order_staged: null argument");
    if (initial_buckets == 0) initial_buckets = 1;
    MgStage last = mg_stage_start(initial_buckets);   // the plan alone gives the bucket count
    for (uint32_t s = 0; s <= MG_MAX_STAGES && mg_stage_next(n, last); ++s) {
    }
    if (last.end < n || n > (1u << 30)) return fail("bt_diag_kmer_set_order_staged: more than 2^30 k-mers");
    if (last.buckets >= 0xFFFFFFFEull) return fail("bt_diag_kmer_set_order_staged: a bucket count of 2^32 - 2 or more (the stage code numbers buckets in 32 bits)");
    std::vector<uint32_t> area(mg_layout(n).total);
    const uint32_t err = mg_staged_order<SoloTeam>(
        n, initial_buckets, k, area.data(),
        [&](uint32_t node, uint64_t &lo, uint64_t &hi) {
            lo = h_kmers[2 * (size_t)node];
            hi = h_kmers[2 * (size_t)node + 1];
        },
        [&](uint32_t node, uint32_t rank) { h_rank[node] = rank; });
    if (err) return fail("bt_diag_kmer_set_order_staged: a violated loop bound (code " + std::to_string(err) + ")");
    if (h_final_buckets) *h_final_buckets = last.buckets;
    return BT_OK;
}

int bt_diag_kmer_set_order(const uint64_t *h_kmers, uint32_t n, uint64_t initial_buckets, unsigned k, uint32_t *h_rank, uint64_t *h_final_buckets) {
    if (!h_kmers || !h_rank) return fail("bt_diag_kmer_set_order: null argument");
    if (initial_buckets == 0) initial_buckets = 1;
    uint64_t cap = 4;
    while (cap < 2ull * n) cap <<= 1;
    std::vector<uint32_t> nx(std::max<uint32_t>(n, 1)), mk(cap), mv(cap);
    replay_kmer_set(
        n, initial_buckets, k, nx.data(), mk.data(), mv.data(), (uint32_t)cap - 1u,
        [&](uint32_t node, uint64_t &lo, uint64_t &hi) {
            lo = h_kmers[2 * (size_t)node];
            hi = h_kmers[2 * (size_t)node + 1];
        },
        [&](uint32_t node, uint32_t rank) { h_rank[node] = rank; });
    if (h_final_buckets) {
        uint64_t B = initial_buckets;
        while (B < n || (n && B <= 1)) B = std_next_bucket_count(B);   // (a fresh set has 13 buckets after its first insert)
        *h_final_buckets = B;
    }
    return BT_OK;
}

uint64_t bt_diag_std_hash_bitset(uint64_t lo, uint64_t hi, unsigned k) { return (k == 0 || k > 64) ? 0 : std_hash_bitset(lo, hi, k); }

int bt_paths_destroy(bt_paths *p) {
    if (!p) return BT_OK;
    (void)hipSetDevice(p->ctx->device);
    (void)hipStreamSynchronize(p->ctx->stream);
    for (void *q : p->owned) (void)hipFree(q);
    p->drop_device_candidates();
    delete p;
    return BT_OK;
}

int bt_paths_count_kmers(bt_paths *p, bt_bloom *path_bloom) {
    if (!p || !path_bloom) return fail("bt_paths_count_kmers: null argument");
    if (path_bloom->k != p->k) return fail("bt_paths_count_kmers: k mismatch");
    BT_HIP(hipSetDevice(p->ctx->device));
    hipLaunchKernelGGL(bloom_insert_valid_kernel, dim3(grid_for(p->L, BLOCK, p->ctx->num_cu * 16)), dim3(BLOCK), 0, p->ctx->stream, path_bloom->view(), p->d_kmers,
                       p->d_valid, p->L);
    BT_CHECK_LAUNCH();
    return BT_OK;
}

int bt_paths_count_multigroup(bt_paths *p, const uint32_t *h_cluster_group, bt_bloom *path_bloom, bt_table *multigroup_table, uint64_t *h_num_path_kmers) {
    if (!p || !h_cluster_group || !path_bloom || !multigroup_table) return fail("bt_paths_count_multigroup: null argument");
    if (path_bloom->k != p->k || multigroup_table->k != p->k) return fail("bt_paths_count_multigroup: k mismatch");
    for (uint32_t c = 1; c < p->C; ++c)
        if (h_cluster_group[c] < h_cluster_group[c - 1]) return fail("bt_paths_count_multigroup: clusters must be listed group by group, groups in index order");
    if (p->L >= 0xFFFFFFFEull) return fail("bt_paths_count_multigroup: more than 2^32 path positions in one unit");
    BT_HIP(hipSetDevice(p->ctx->device));
    hipStream_t st = p->ctx->stream;
    const uint64_t cap = pow2_at_least(2 * std::max<uint64_t>(p->num_valid, 8));
    if (cap > (1ull << 32)) return fail("bt_paths_count_multigroup: more than 2^31 k-mer occurrences in one unit");
    const uint32_t G = p->C ? h_cluster_group[p->C - 1] + 1u : 0u;
    std::vector<void *> tmp;
    auto cleanup = [&]() {
        for (void *q : tmp) (void)hipFree(q);
    };
    uint64_t *dlo, *dhi, *elo, *ehi, *d_out;
    uint32_t *dtag, *dstate, *dfirst, *pos_d, *etag, *estate, *egroup, *emulti, *etime, *d_cg, *d_flag, *d_rowpos, *d_sums;
    unsigned long long *d_counters;
    const uint64_t nblk = (p->L + BLOCK * 4 - 1) / (BLOCK * 4);
    int rc = BT_OK;
    auto A = [&](auto **q, uint64_t n) {
        if (rc == BT_OK) rc = dev_alloc(q, n, tmp);
    };
    A(&dlo, cap); A(&dhi, cap); A(&dtag, cap); A(&dstate, cap); A(&dfirst, cap); A(&pos_d, p->L);
    A(&elo, cap); A(&ehi, cap); A(&etag, cap); A(&estate, cap); A(&egroup, cap); A(&emulti, cap); A(&etime, cap);
    A(&d_out, 2 * p->num_valid); A(&d_cg, p->C); A(&d_counters, 4);
    A(&d_flag, p->L); A(&d_rowpos, p->L + 1); A(&d_sums, nblk);
    if (rc != BT_OK) {
        cleanup();
        return rc;
    }
#define MGH(call)                                                                             \
    do {                                                                                      \
        const hipError_t _e = (call);                                                         \
        if (_e != hipSuccess) {                                                               \
            cleanup();                                                                        \
            return fail(std::string("bt_paths_count_multigroup: ") + hipGetErrorString(_e));  \
        }                                                                                     \
    } while (0)
#define MGR(call)            \
    do {                     \
        const int _r = (call); \
        if (_r != BT_OK) {   \
            cleanup();       \
            return _r;       \
        }                    \
    } while (0)
    MGH(hipMemsetAsync(dstate, 0, cap * 4, st));
    MGH(hipMemsetAsync(estate, 0, cap * 4, st));
    MGH(hipMemsetAsync(dfirst, 0xFF, cap * 4, st));
    MGH(hipMemsetAsync(egroup, 0xFF, cap * 4, st));
    MGH(hipMemsetAsync(etime, 0xFF, cap * 4, st));
    MGH(hipMemsetAsync(emulti, 0, cap * 4, st));
    MGH(hipMemsetAsync(d_counters, 0, 32, st));
    MGH(hipMemcpyAsync(d_cg, h_cluster_group, (size_t)p->C * 4, hipMemcpyHostToDevice, st));
    const unsigned maxb = p->ctx->num_cu * 16;
    const bt::BloomView bv = path_bloom->view();
    // 1. indexes; first occurrences in path order
    hipLaunchKernelGGL(multigroup_kernel, dim3(grid_for(p->L, BLOCK, maxb)), dim3(BLOCK), 0, st, dlo, dhi, dtag, dstate, dfirst, pos_d, elo, ehi, etag, estate, egroup, emulti,
                       cap - 1, p->d_kmers, p->d_valid, p->d_pos_path, p->d_path_cluster, d_cg, p->L);
    hipLaunchKernelGGL(mg_flag_kernel, dim3(grid_for(p->L, BLOCK, maxb)), dim3(BLOCK), 0, st, p->d_valid, pos_d, dfirst, p->L, d_flag);
    uint64_t n_total = 0;
    if (p->L) {
        hipLaunchKernelGGL(scan_block_kernel, dim3((unsigned)nblk), dim3(BLOCK), 0, st, d_flag, p->L, d_rowpos, d_sums);
        std::vector<uint32_t> sums(nblk);
        MGH(hipMemcpyAsync(sums.data(), d_sums, nblk * 4, hipMemcpyDeviceToHost, st));
        MGH(hipStreamSynchronize(st));
        for (uint64_t i = 0; i < nblk; ++i) {
            const uint32_t v = sums[i];
            sums[i] = (uint32_t)n_total;
            n_total += v;
        }
        MGH(hipMemcpyAsync(d_sums, sums.data(), nblk * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned)nblk), dim3(BLOCK), 0, st, d_rowpos, p->L, d_sums);
        MGH(hipStreamSynchronize(st));   // (sums goes out of scope)
    }
    const uint32_t total32 = (uint32_t)n_total;
    MGH(hipMemcpyAsync(d_rowpos + p->L, &total32, 4, hipMemcpyHostToDevice, st));
    // 2. per group: its range of first occurrences, the bucket count it inherits, room for its bucket map
    std::vector<uint64_t> gstart(G + 1, p->L);
    for (uint32_t c = p->C; c-- > 0;) gstart[h_cluster_group[c]] = p->cluster_text0[c];
    for (uint32_t g = G; g-- > 0;)
        if (gstart[g] == p->L && g + 1 <= G) gstart[g] = gstart[g + 1];   // a group index without clusters
    uint64_t *d_gstart = nullptr;
    uint32_t *d_goff = nullptr, *d_seq = nullptr, *d_time = nullptr;
    A(&d_gstart, G + 1); A(&d_goff, G + 1); A(&d_seq, n_total); A(&d_time, n_total);
    MGR(rc);
    MGH(hipMemcpyAsync(d_gstart, gstart.data(), (size_t)(G + 1) * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(gather_u32_kernel, dim3((G + 1 + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, d_rowpos, d_gstart, G + 1, d_goff);
    hipLaunchKernelGGL(mg_seq_kernel, dim3(grid_for(p->L, BLOCK, maxb)), dim3(BLOCK), 0, st, d_flag, d_rowpos, p->L, d_seq);
    std::vector<uint32_t> goff(G + 1);
    MGH(hipMemcpyAsync(goff.data(), d_goff, (size_t)(G + 1) * 4, hipMemcpyDeviceToHost, st));
    MGH(hipStreamSynchronize(st));
    // 3. times: every group's k-mers in its container's iteration order (the set is fresh before the unit's first group).  BT_MG_WIDE_MIN = N sends groups
    //    of at least N distinct k-mers to a workgroup each (mg_order_wide_kernel); unset or 0: one lane per group for all of them
    uint32_t wide_min = 0;
    if (const char *e = getenv("BT_MG_WIDE_MIN")) {   // a decimal number below 2^32, or the call fails: a mistyped threshold must not quietly become another one
        char *end = nullptr;
        errno = 0;
        const unsigned long long v = std::strtoull(e, &end, 10);
        if (*e < '0' || *e > '9' || *end != '\0' || errno != 0 || v > 0xFFFFFFFFull) {
            cleanup();
            return fail(std::string("bt_paths_count_multigroup: BT_MG_WIDE_MIN must be a decimal number of k-mers below 2^32 (0: off), not '") + e + "'");
        }
        wide_min = (uint32_t)v;
    }
    bt_multigroup_stats mg_stats{};   // (the handle's copy is replaced once the whole call has succeeded)
    MgUploads up;
    MGR(mg_group_orders(p->ctx, "bt_paths_count_multigroup", p->d_kmers, d_seq, d_goff, goff, G, p->k, 1, wide_min, d_time, nullptr, mg_stats, up, tmp));
    hipLaunchKernelGGL(mg_etime_kernel, dim3(grid_for(n_total, BLOCK, maxb)), dim3(BLOCK), 0, st, p->d_kmers, d_seq, d_time, n_total, elo, ehi, etag, estate, cap - 1, etime);
    // 4. k-mers the filter reports at their first turn
    uint32_t *f1 = nullptr, *f2 = nullptr;
    const uint64_t fwords = (path_bloom->bytes + 3) / 4;
    A(&f1, fwords); A(&f2, fwords);
    MGR(rc);
    MGH(hipMemsetAsync(f1, 0, fwords * 4, st));
    MGH(hipMemsetAsync(f2, 0, fwords * 4, st));
    hipLaunchKernelGGL(mg_shared_bits_kernel, dim3(grid_for(cap, BLOCK, maxb)), dim3(BLOCK), 0, st, bv, elo, ehi, estate, cap - 1, f1, f2);
    hipLaunchKernelGGL(mg_candidates_kernel, dim3(grid_for(cap, BLOCK, maxb)), dim3(BLOCK), 0, st, bv, elo, ehi, estate, emulti, cap - 1, f2, d_counters + 2,
                       (uint64_t *)nullptr);
    unsigned long long ncand = 0;
    MGH(hipMemcpyAsync(&ncand, d_counters + 2, 8, hipMemcpyDeviceToHost, st));
    MGH(hipStreamSynchronize(st));
    if (ncand) {
        uint64_t *d_cand = nullptr;
        unsigned long long *cb_keys = nullptr;
        uint32_t *cb_time = nullptr;
        const uint64_t cb_cap = pow2_at_least(2 * ncand * path_bloom->num_hashes);
        A(&d_cand, ncand); A(&cb_keys, cb_cap); A(&cb_time, cb_cap);
        MGR(rc);
        MGH(hipMemsetAsync(cb_keys, 0xFF, cb_cap * 8, st));
        MGH(hipMemsetAsync(cb_time, 0xFF, cb_cap * 4, st));
        hipLaunchKernelGGL(mg_candidates_kernel, dim3(grid_for(cap, BLOCK, maxb)), dim3(BLOCK), 0, st, bv, elo, ehi, estate, emulti, cap - 1, f2, d_counters + 3, d_cand);
        hipLaunchKernelGGL(mg_cand_bits_kernel, dim3(grid_for(ncand, BLOCK, maxb)), dim3(BLOCK), 0, st, bv, elo, ehi, d_cand, (uint64_t)ncand, cb_keys, cb_time, cb_cap - 1);
        hipLaunchKernelGGL(mg_bit_times_kernel, dim3(grid_for(cap, BLOCK, maxb)), dim3(BLOCK), 0, st, bv, elo, ehi, estate, etime, cap - 1, cb_keys, cb_time, cb_cap - 1);
        hipLaunchKernelGGL(mg_reported_kernel, dim3(grid_for(ncand, BLOCK, maxb)), dim3(BLOCK), 0, st, bv, elo, ehi, etime, d_cand, (uint64_t)ncand, cb_keys, cb_time,
                           cb_cap - 1, emulti);
    }
    hipLaunchKernelGGL(multigroup_list_kernel, dim3(grid_for(cap, BLOCK, maxb)), dim3(BLOCK), 0, st, elo, ehi, estate, emulti, dstate, cap - 1, d_out, d_counters);
    unsigned long long counters[2] = {0, 0};
    MGH(hipGetLastError());
    MGH(hipMemcpyAsync(counters, d_counters, 16, hipMemcpyDeviceToHost, st));
    MGH(hipStreamSynchronize(st));
    {   // the reference's KmerHash grows on demand; this table is grown before the unit's multigroup k-mers go in (their number is known here)
        uint64_t keys = 0, capacity = 0;
        int overflowed = 0;
        rc = bt_table_status(multigroup_table, &keys, &capacity, &overflowed);
        if (rc == BT_OK && 2 * (keys + counters[0]) > capacity) rc = bt_table_reserve(multigroup_table, keys + counters[0]);
    }
    if (rc == BT_OK) rc = bt_table_insert_batch(multigroup_table, d_out, counters[0], 0);
    if (rc == BT_OK) rc = bt_paths_count_kmers(p, path_bloom);
    if (rc == BT_OK && hipStreamSynchronize(st) != hipSuccess) rc = fail("bt_paths_count_multigroup: device error");
    cleanup();
#undef MGH
#undef MGR
    if (h_num_path_kmers) *h_num_path_kmers = counters[1];
    if (rc == BT_OK) p->mg_stats = mg_stats;
    return rc;
}

int bt_paths_classify(bt_paths *p, bt_table *table, bt_bloom *multigroup_bloom, uint32_t *h_num_path_kmers, uint8_t *h_has_excluded) {
    if (!p || !table || !multigroup_bloom) return fail("bt_paths_classify: null argument");
    if (table->k != p->k) return fail("bt_paths_classify: k mismatch");
    BT_HIP(hipSetDevice(p->ctx->device));
    int rc = build_index(p);
    if (rc != BT_OK) return rc;
    rc = bt_table_classify_batch(table, multigroup_bloom, p->d_list_kmers, p->d_list_mult, p->n_list, p->d_list_excluded);
    if (rc != BT_OK) return rc;
    uint32_t *d_n = nullptr, *d_ex = nullptr;
    BT_HIP(hipMalloc(reinterpret_cast<void **>(&d_n), (size_t)p->C * 4));
    BT_HIP(hipMalloc(reinterpret_cast<void **>(&d_ex), (size_t)p->C * 4));
    hipStream_t st = p->ctx->stream;
    (void)hipMemsetAsync(d_n, 0, (size_t)p->C * 4, st);
    (void)hipMemsetAsync(d_ex, 0, (size_t)p->C * 4, st);
    hipLaunchKernelGGL(classify_tally_kernel, dim3(grid_for(p->n_list, BLOCK, p->ctx->num_cu * 16)), dim3(BLOCK), 0, st, p->d_list_cluster, p->d_list_excluded,
                       p->n_list, d_n, d_ex);
    std::vector<uint32_t> n(p->C), ex(p->C);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipMemcpy(n.data(), d_n, (size_t)p->C * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(ex.data(), d_ex, (size_t)p->C * 4, hipMemcpyDeviceToHost);
    (void)hipFree(d_n);
    (void)hipFree(d_ex);
    if (e != hipSuccess) return fail(std::string("bt_paths_classify: ") + hipGetErrorString(e));
    for (uint32_t c = 0; c < p->C; ++c) {
        if (h_num_path_kmers) h_num_path_kmers[c] = n[c];
        if (h_has_excluded) h_has_excluded[c] = ex[c] ? 1 : 0;
    }
    return BT_OK;
}

}  // extern "C"

namespace {

// exclusive prefix sum of n words on the context's stream: d_out[0 .. n], d_out[n] = *total.  The totals of the 1024-element blocks pass through the host
// (n / 1024 words).  An error when the total does not fit 32 bits: every offset of the batch layout is a uint32_t.
int exclusive_scan(bt_ctx *ctx, const uint32_t *d_in, uint64_t n, uint32_t *d_out, uint64_t *total, const char *what, std::vector<void *> &tmp) {
    hipStream_t st = ctx->stream;
    const uint64_t nblk = (n + BLOCK * 4 - 1) / (BLOCK * 4);
    uint64_t sum = 0;
    if (nblk) {
        uint32_t *d_sums = nullptr;
        const int rc = dev_alloc(&d_sums, nblk, tmp);
        if (rc != BT_OK) return rc;
        hipLaunchKernelGGL(scan_block_kernel, dim3((unsigned)nblk), dim3(BLOCK), 0, st, d_in, n, d_out, d_sums);
        BT_CHECK_LAUNCH();
        std::vector<uint32_t> sums(nblk);
        BT_HIP(hipMemcpyAsync(sums.data(), d_sums, nblk * 4, hipMemcpyDeviceToHost, st));
        BT_HIP(hipStreamSynchronize(st));
        for (uint64_t i = 0; i < nblk; ++i) {
            const uint32_t v = sums[i];
            sums[i] = (uint32_t)sum;
            sum += v;
        }
        if (sum >= (1ull << 32)) return fail(std::string("bt_paths_candidates: more than 2^32 ") + what + " in one batch: a 32-bit offset of the batch layout would overflow (split the unit)");
        BT_HIP(hipMemcpyAsync(d_sums, sums.data(), nblk * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned)nblk), dim3(BLOCK), 0, st, d_out, n, d_sums);
        BT_CHECK_LAUNCH();
    }
    const uint32_t last = (uint32_t)sum;
    BT_HIP(hipMemcpyAsync(d_out + n, &last, 4, hipMemcpyHostToDevice, st));
    BT_HIP(hipStreamSynchronize(st));
    *total = sum;
    return BT_OK;
}

uint32_t env_threshold(const char *name, uint32_t dflt) {
    const char *e = getenv(name);
    if (!e) return dflt;
    const long v = atol(e);
    return (uint32_t)std::min<long>(std::max<long>(v, 0), dflt);   // (tests lower the thresholds so that small units reach every path; never above the kernels' limits)
}

// getHaplotypeCandidates for every cluster: the per-row / per-entry arrays are built and LEFT on the device (p->d_*), the O(C) arrays and what the host graph
// walk gives (haplotype alleles, nested clusters) in p's host vectors
int candidates_build(bt_paths *p, bt_table *table, bt_paths_candidates_sizes *sizes) {
    if (!p || !table || !sizes) return fail("bt_paths_candidates: null argument");
    if (table->k != p->k) return fail("bt_paths_candidates: k mismatch");
    BT_HIP(hipSetDevice(p->ctx->device));
    p->have_candidates = false;
    p->drop_device_candidates();
    int rc = build_index(p);
    if (rc != BT_OK) return rc;
    hipStream_t st = p->ctx->stream;
    const unsigned maxb = p->ctx->num_cu * 16;
    const uint32_t C = p->C, S = table->num_samples;
    p->S = S;
    // ---- the host half (haplotype alleles, nested clusters, nested dependency map: O(paths x vertices), reads no k-mer data) on host threads of its own
    // while the device kernels are in flight; every thread takes a range of clusters and the pieces are concatenated in cluster order afterwards
    struct Piece {
        std::vector<uint32_t> hapnest_off, hapnest_idx, nestdep_off, nestdep_cluster, nestdep_var_off;
        std::vector<uint16_t> hap_allele, nestdep_var;
    };
    const unsigned T = host_threads(C);
    std::vector<Piece> piece(T);
    auto work = [&](unsigned t) {
        Piece &q = piece[t];
        const uint32_t c0 = (uint32_t)((uint64_t)C * t / T), c1 = (uint32_t)((uint64_t)C * (t + 1) / T);
        std::vector<Interval> iv_dummy;
        std::vector<uint16_t> alleles;
        std::vector<uint32_t> nested;
        for (uint32_t c = c0; c < c1; ++c) {
            for (uint32_t lp = 0; lp < p->num_paths[c]; ++lp) {
                iv_dummy.clear();
                walk_path_host(*p, c, lp, iv_dummy, alleles, nested);
                q.hap_allele.insert(q.hap_allele.end(), alleles.begin(), alleles.end());
                q.hapnest_idx.insert(q.hapnest_idx.end(), nested.begin(), nested.end());
                q.hapnest_off.push_back((uint32_t)q.hapnest_idx.size());
            }
            std::map<uint32_t, std::vector<uint16_t>> dep;   // VariantClusterGraph.cpp:1112-1132
            for (uint32_t v = p->vertex_off[c]; v < p->vertex_off[c + 1]; ++v) {
                if (p->vertex_nested[v] == 0xFFFFFFFFu) continue;
                auto &lst = dep[p->vertex_nested[v]];
                if (p->vertex_variant[v] != 0xFFFF) lst.push_back(p->vertex_variant[v]);
                for (uint32_t r = p->refvar_off[v]; r < p->refvar_off[v + 1]; ++r) lst.push_back(p->refvar[r]);
                std::sort(lst.begin(), lst.end(), std::greater<uint16_t>());
            }
            for (auto &e : dep) {
                q.nestdep_cluster.push_back(e.first);
                q.nestdep_var.insert(q.nestdep_var.end(), e.second.begin(), e.second.end());
                q.nestdep_var_off.push_back((uint32_t)q.nestdep_var.size());
            }
            q.nestdep_off.push_back((uint32_t)q.nestdep_cluster.size());
        }
    };
    std::exception_ptr walk_error;
    std::thread walker;
    struct Joiner {
        std::thread &t;
        ~Joiner() {
            if (t.joinable()) t.join();
        }
    } joiner{walker};
    auto walk_all = [&]() {
        try {
            if (C) run_on_threads(T, work);
        } catch (...) {
            walk_error = std::current_exception();
        }
    };
    try {
        walker = std::thread(walk_all);
    } catch (...) {   // (no thread could be started: the walk runs here, before the device work)
        walk_all();
    }

    std::vector<void *> tmp, keep;
    auto cleanup = [&]() {
        (void)hipStreamSynchronize(st);
        for (void *q : tmp) (void)hipFree(q);
        for (void *q : keep) (void)hipFree(q);
        tmp.clear();
        keep.clear();
        p->drop_device_candidates();   // (nothing owned yet: forgets the pointers)
    };
#define TRYC(x)                  \
    do {                         \
        const int _rc = (x);     \
        if (_rc != BT_OK) {      \
            cleanup();           \
            return _rc;          \
        }                        \
    } while (0)
#define HIPC(call)                                                                      \
    do {                                                                                \
        hipError_t _e = (call);                                                         \
        if (_e != hipSuccess) {                                                         \
            cleanup();                                                                  \
            return bt::fail(std::string(#call) + ": " + hipGetErrorString(_e));         \
        }                                                                               \
    } while (0)
    // 1. table records of the distinct (cluster, k-mer) entries
    TRYC(bt_table_find_batch(table, p->d_list_kmers, p->n_list, p->d_list_slots));
    hipLaunchKernelGGL(record_kernel, dim3(grid_for(p->n_list, BLOCK, maxb)), dim3(BLOCK), 0, st, table->v, p->d_list_slots, p->n_list, p->d_list_flags);
    // 2. row numbering = prefix sum over first-occurrence flags in text order
    uint32_t *d_flag = nullptr, *d_rowpos = nullptr, *d_a_row = nullptr;
    TRYC(dev_alloc(&d_flag, p->L, tmp));
    TRYC(dev_alloc(&d_rowpos, p->L + 1, tmp));
    TRYC(dev_alloc(&d_a_row, p->A.mask + 1, tmp));
    hipLaunchKernelGGL(first_flag_kernel, dim3(grid_for(p->L, BLOCK, maxb)), dim3(BLOCK), 0, st, p->A, p->d_valid, p->d_pos_slot_a, p->d_list_flags, p->L, d_flag);
    uint64_t total_rows = 0;
    TRYC(exclusive_scan(p->ctx, d_flag, p->L, d_rowpos, &total_rows, "k-mer rows", tmp));
    // kmer_off[c] = rows before the cluster's first text position (d_rowpos has L + 1 entries: the last one is the total)
    p->kmer_off.assign(C + 1, 0);
    uint32_t *d_c32 = nullptr;   // [C+1] gather results
    {
        uint64_t *d_idx = nullptr;
        TRYC(dev_alloc(&d_idx, C, tmp));
        TRYC(dev_alloc(&d_c32, C + 1, tmp));
        HIPC(hipMemcpyAsync(d_idx, p->cluster_text0.data(), (size_t)C * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(gather_u32_kernel, dim3((C + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, d_rowpos, d_idx, C, d_c32);
        HIPC(hipMemcpyAsync(p->kmer_off.data(), d_c32, (size_t)C * 4, hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
    }
    p->kmer_off[C] = (uint32_t)total_rows;
    const uint64_t R = total_rows;
    // 3. per row: key + table record + its cluster
    uint8_t *d_row_flags = nullptr;
    uint32_t *d_row_cluster = nullptr;
    TRYC(dev_alloc(&p->d_key, 2 * R, keep));
    TRYC(dev_alloc(&p->d_counts, R * S, keep));
    TRYC(dev_alloc(&p->d_ic, 2 * R, keep));
    TRYC(dev_alloc(&p->d_has_counts, R, keep));
    TRYC(dev_alloc(&d_row_flags, R, tmp));
    TRYC(dev_alloc(&d_row_cluster, R, tmp));
    hipLaunchKernelGGL(rows_kernel, dim3(grid_for(p->L, BLOCK, maxb)), dim3(BLOCK), 0, st, p->A, table->v, p->d_valid, p->d_pos_slot_a, d_flag, d_rowpos, p->d_list_slots,
                       p->d_list_flags, p->d_pos_path, p->d_path_cluster, p->L, S, d_a_row, p->d_key, d_row_flags, p->d_counts, p->d_ic, d_row_cluster);
    // 4. multiplicity matrix
    std::vector<uint64_t> mult0(C + 1, 0);
    for (uint32_t c = 0; c < C; ++c) mult0[c + 1] = mult0[c] + (uint64_t)(p->kmer_off[c + 1] - p->kmer_off[c]) * p->num_paths[c];
    uint32_t *d_row0 = nullptr, *d_h = nullptr, *d_over = nullptr;
    uint64_t *d_mult0 = nullptr;
    TRYC(dev_alloc(&p->d_mult, mult0[C], keep));
    TRYC(dev_alloc(&d_row0, C + 1, tmp));
    TRYC(dev_alloc(&d_h, C, tmp));
    TRYC(dev_alloc(&d_mult0, C + 1, tmp));
    TRYC(dev_alloc(&d_over, 1, tmp));
    HIPC(hipMemsetAsync(p->d_mult, 0, std::max<uint64_t>(mult0[C], 1), st));
    HIPC(hipMemsetAsync(d_over, 0, 4, st));
    HIPC(hipMemcpyAsync(d_row0, p->kmer_off.data(), (size_t)(C + 1) * 4, hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(d_h, p->num_paths.data(), (size_t)C * 4, hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(d_mult0, mult0.data(), (size_t)(C + 1) * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(mult_kernel, dim3(grid_for(p->B.mask + 1, BLOCK, maxb)), dim3(BLOCK), 0, st, p->A, p->B, p->d_list_flags, d_a_row, p->d_path_cluster,
                       p->d_path_local, d_row0, d_mult0, d_h, p->d_mult, d_over);
    // 5. (row, variant, path) triples, each scattered into its row's segment: count per row, scan, write
    unsigned long long *d_cursor = nullptr;
    uint32_t *d_row_cnt = nullptr, *d_row_off = nullptr, *d_trip = nullptr;
    TRYC(dev_alloc(&d_cursor, 1, tmp));
    TRYC(dev_alloc(&d_row_cnt, R, tmp));
    TRYC(dev_alloc(&d_row_off, R + 1, tmp));
    HIPC(hipMemsetAsync(d_cursor, 0, 8, st));
    HIPC(hipMemsetAsync(d_row_cnt, 0, std::max<uint64_t>(R, 1) * 4, st));
    hipLaunchKernelGGL(triples_kernel, dim3(grid_for(p->L, BLOCK, maxb)), dim3(BLOCK), 0, st, p->A, p->d_valid, p->d_pos_slot_a, p->d_list_flags, d_a_row, p->d_pos_path,
                       p->d_pos_nt, p->d_path_local, p->d_iv_off, p->d_iv, p->L, d_cursor, (const uint32_t *)nullptr, d_row_cnt, (uint32_t *)nullptr);
    unsigned long long ntrip = 0;
    HIPC(hipMemcpyAsync(&ntrip, d_cursor, 8, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    if (ntrip >= (1ull << 32)) {
        cleanup();
        return fail("bt_paths_candidates: more than 2^32 (k-mer, variant, haplotype) incidences in one batch: a 32-bit offset of the batch layout would overflow (split the unit)");
    }
    uint64_t ntrip2 = 0;
    TRYC(exclusive_scan(p->ctx, d_row_cnt, R, d_row_off, &ntrip2, "incidences", tmp));
    TRYC(dev_alloc(&d_trip, ntrip, tmp));
    HIPC(hipMemsetAsync(d_row_cnt, 0, std::max<uint64_t>(R, 1) * 4, st));
    hipLaunchKernelGGL(triples_kernel, dim3(grid_for(p->L, BLOCK, maxb)), dim3(BLOCK), 0, st, p->A, p->d_valid, p->d_pos_slot_a, p->d_list_flags, d_a_row, p->d_pos_path,
                       p->d_pos_nt, p->d_path_local, p->d_iv_off, p->d_iv, p->L, d_cursor, d_row_off, d_row_cnt, d_trip);
    HIPC(hipGetLastError());
    // 6. entries per row (distinct variants), rows longer than a lane's share listed for the wavefront / workgroup kernels
    const uint32_t lane_max = env_threshold("BT_PATHS_ROW_LANE_MAX", ROW_LANE_MAX), wave_max = std::max(lane_max, env_threshold("BT_PATHS_ROW_WAVE_MAX", ROW_WAVE_MAX));
    const uint32_t wave_cap = (uint32_t)(ntrip / (lane_max + 1ull)) + 1u, block_cap = (uint32_t)(ntrip / (wave_max + 1ull)) + 1u;   // a listed row has more triples than the threshold
    uint32_t *d_row_nnz = nullptr, *d_wave_list = nullptr, *d_block_list = nullptr, *d_list_n = nullptr;
    TRYC(dev_alloc(&d_row_nnz, R, tmp));
    TRYC(dev_alloc(&d_wave_list, wave_cap, tmp));
    TRYC(dev_alloc(&d_block_list, block_cap, tmp));
    TRYC(dev_alloc(&d_list_n, 2, tmp));
    TRYC(dev_alloc(&p->d_kv_off, R + 1, keep));
    HIPC(hipMemsetAsync(d_list_n, 0, 8, st));
    RowJob J{};
    J.trip = d_trip;
    J.row_off = d_row_off;
    J.row_nnz = d_row_nnz;
    J.row_cluster = d_row_cluster;
    J.cluster_h = d_h;
    J.write = 0;
    hipLaunchKernelGGL(row_entries_lane_kernel, dim3(grid_for(R, BLOCK, maxb)), dim3(BLOCK), 0, st, J, R, lane_max, wave_max, d_wave_list, wave_cap, d_block_list, block_cap, d_list_n);
    uint32_t list_n[2] = {0, 0};
    HIPC(hipMemcpyAsync(list_n, d_list_n, 8, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    if (list_n[0] > wave_cap || list_n[1] > block_cap) {
        cleanup();
        return fail("bt_paths_candidates: internal error: more long rows than their triples allow");
    }
    auto long_rows = [&]() {
        if (list_n[0]) hipLaunchKernelGGL(row_entries_wave_kernel, dim3(grid_for(list_n[0], BLOCK / 64, maxb)), dim3(BLOCK), 0, st, J, d_wave_list, list_n[0]);
        if (list_n[1]) hipLaunchKernelGGL(row_entries_block_kernel, dim3(grid_for(list_n[1], 1, maxb)), dim3(BLOCK), 0, st, J, d_block_list, list_n[1]);
    };
    long_rows();
    HIPC(hipGetLastError());
    uint64_t nnz = 0;
    TRYC(exclusive_scan(p->ctx, d_row_nnz, R, p->d_kv_off, &nnz, "incidence entries", tmp));
    // 7. where each cluster's entries and bitset words start (O(C), host), then the write pass
    uint32_t *d_ckv0 = nullptr;
    uint64_t *d_ckvb = nullptr;
    TRYC(dev_alloc(&d_ckv0, C + 1, tmp));
    TRYC(dev_alloc(&d_ckvb, C + 1, tmp));
    p->cluster_kv0.assign(C + 1, 0);
    hipLaunchKernelGGL(gather_u32_idx32_kernel, dim3((C + 1 + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, p->d_kv_off, d_row0, C + 1, d_ckv0);
    HIPC(hipMemcpyAsync(p->cluster_kv0.data(), d_ckv0, (size_t)(C + 1) * 4, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    std::vector<uint64_t> kvb(C + 1, 0);
    for (uint32_t c = 0; c < C; ++c) kvb[c + 1] = kvb[c] + (uint64_t)(p->cluster_kv0[c + 1] - p->cluster_kv0[c]) * ((p->num_paths[c] + 31) / 32);
    HIPC(hipMemcpyAsync(d_ckvb, kvb.data(), (size_t)(C + 1) * 8, hipMemcpyHostToDevice, st));
    TRYC(dev_alloc(&p->d_kv_var, nnz, keep));
    TRYC(dev_alloc(&p->d_kv_bits, kvb[C], keep));
    HIPC(hipMemsetAsync(p->d_kv_bits, 0, std::max<uint64_t>(kvb[C], 1) * 4, st));
    J.kv_off = p->d_kv_off;
    J.cluster_kv0 = d_ckv0;
    J.cluster_kvb = d_ckvb;
    J.kv_var = p->d_kv_var;
    J.kv_bits = p->d_kv_bits;
    J.write = 1;
    hipLaunchKernelGGL(row_entries_lane_kernel, dim3(grid_for(R, BLOCK, maxb)), dim3(BLOCK), 0, st, J, R, lane_max, wave_max, d_wave_list, wave_cap, d_block_list, block_cap, d_list_n);
    long_rows();
    HIPC(hipGetLastError());
    // 8. kmer_has_counts and the unique / multicluster row lists (stable: a row's place is the number of rows of its kind before it)
    uint32_t *d_is_multi = d_row_nnz, *d_mbefore = nullptr;
    TRYC(dev_alloc(&d_mbefore, R + 1, tmp));
    hipLaunchKernelGGL(row_flags_kernel, dim3(grid_for(R, BLOCK, maxb)), dim3(BLOCK), 0, st, d_row_flags, R, d_is_multi, p->d_has_counts);
    uint64_t num_multi = 0;
    TRYC(exclusive_scan(p->ctx, d_is_multi, R, d_mbefore, &num_multi, "multicluster rows", tmp));
    p->multi_off.assign(C + 1, 0);
    p->unique_off.assign(C + 1, 0);
    hipLaunchKernelGGL(gather_u32_idx32_kernel, dim3((C + 1 + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, d_mbefore, d_row0, C + 1, d_c32);
    HIPC(hipMemcpyAsync(p->multi_off.data(), d_c32, (size_t)(C + 1) * 4, hipMemcpyDeviceToHost, st));
    TRYC(dev_alloc(&p->d_unique_idx, R - num_multi, keep));
    TRYC(dev_alloc(&p->d_multi_idx, num_multi, keep));
    hipLaunchKernelGGL(row_lists_kernel, dim3(grid_for(R, BLOCK, maxb)), dim3(BLOCK), 0, st, d_row_flags, d_mbefore, d_row_cluster, d_row0, R, p->d_unique_idx, p->d_multi_idx);
    HIPC(hipGetLastError());
    uint32_t over = 0;
    HIPC(hipMemcpyAsync(&over, d_over, 4, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    for (uint32_t c = 0; c <= C; ++c) p->unique_off[c] = p->kmer_off[c] - p->multi_off[c];
    if (getenv("BT_PATHS_DEBUG")) {   // which kernel took how many rows, and the triples-per-row distribution (bin b: rows with 2^(b-1) < triples <= 2^b; bin 0: none or one)
        std::vector<uint32_t> off(R + 1, 0);
        HIPC(hipMemcpy(off.data(), d_row_off, (R + 1) * 4, hipMemcpyDeviceToHost));
        uint64_t hist[33] = {0};
        uint32_t longest = 0;
        for (uint64_t r = 0; r < R; ++r) {
            const uint32_t n = off[r + 1] - off[r];
            longest = std::max(longest, n);
            unsigned b = 0;
            while ((1ull << b) < n) ++b;
            ++hist[b];
        }
        std::string h;
        for (unsigned b = 0; b < 33; ++b)
            if (hist[b]) h += " 2^" + std::to_string(b) + ":" + std::to_string(hist[b]);
        fprintf(stderr, "bt_paths_candidates: rows=%llu triples=%llu entries=%llu lane_rows=%llu wave_rows=%u block_rows=%u lane_max=%u wave_max=%u longest_row=%u triples_per_row%s\n",
                (unsigned long long)R, ntrip, (unsigned long long)nnz, (unsigned long long)(R - list_n[0] - list_n[1]), list_n[0], list_n[1], lane_max, wave_max, longest, h.c_str());
    }
    for (void *q : tmp) (void)hipFree(q);
    tmp.clear();
    if (over) {
        cleanup();
        return fail("bt_paths_candidates: a path k-mer occurs more than 127 times on one haplotype (the reference asserts <= 127)");
    }
    // ---- the host half: join, concatenate the pieces in cluster order (`off` lists hold cumulative ends relative to the piece: rebased on what precedes it)
    if (walker.joinable()) walker.join();
    if (walk_error) {
        cleanup();
        try {
            std::rethrow_exception(walk_error);
        } catch (const std::exception &e) {   // (a worker ran out of memory on its pieces: an error of the call, not of the process)
            return fail(std::string("bt_paths_candidates: ") + e.what());
        } catch (...) {
            return fail("bt_paths_candidates: host walk failed");
        }
    }
#undef TRYC
#undef HIPC
    auto cat = [&](auto &dst, auto Piece::*m) {
        size_t n = 0;
        for (auto &q : piece) n += (q.*m).size();
        dst.clear();
        dst.reserve(n);
        for (auto &q : piece) dst.insert(dst.end(), (q.*m).begin(), (q.*m).end());
    };
    auto cat_off = [&](std::vector<uint32_t> &dst, std::vector<uint32_t> Piece::*off, auto Piece::*idx) {
        size_t n = 1;
        for (auto &q : piece) n += (q.*off).size();
        dst.clear();
        dst.reserve(n);
        dst.push_back(0);
        uint32_t base = 0;
        for (auto &q : piece) {
            for (uint32_t v : q.*off) dst.push_back(base + v);
            base += (uint32_t)(q.*idx).size();
        }
    };
    try {
        cat_off(p->hapnest_off, &Piece::hapnest_off, &Piece::hapnest_idx);
        cat_off(p->nestdep_off, &Piece::nestdep_off, &Piece::nestdep_cluster);
        cat_off(p->nestdep_var_off, &Piece::nestdep_var_off, &Piece::nestdep_var);
        cat(p->hap_allele, &Piece::hap_allele);
        cat(p->hapnest_idx, &Piece::hapnest_idx);
        cat(p->nestdep_cluster, &Piece::nestdep_cluster);
        cat(p->nestdep_var, &Piece::nestdep_var);
    } catch (const std::exception &e) {
        cleanup();
        return fail(std::string("bt_paths_candidates: ") + e.what());
    }
    piece.clear();
    for (auto *v : {&p->kv_off, &p->unique_idx, &p->multi_idx, &p->kv_bits}) std::vector<uint32_t>().swap(*v);   // (host copies of an earlier bt_paths_candidates)
    for (auto *v : {&p->mult, &p->has_counts, &p->counts, &p->ic}) std::vector<uint8_t>().swap(*v);
    std::vector<uint64_t>().swap(p->key);
    std::vector<uint16_t>().swap(p->kv_var);
    p->cand_owned = std::move(keep);
    p->cand_on_device = true;
    p->have_candidates = true;
    p->R = R;
    p->nnz = nnz;
    p->kv_words = kvb[C];
    p->mult_bytes = mult0[C];
    p->num_multi = num_multi;
    p->num_unique = R - num_multi;
    sizes->rows = R;
    sizes->mult_bytes = p->mult_bytes;
    sizes->nnz = nnz;
    sizes->kv_words = p->kv_words;
    sizes->num_unique = p->num_unique;
    sizes->num_multi = num_multi;
    sizes->hap_allele = p->hap_allele.size();
    sizes->num_haplotypes = p->num_gpaths;
    sizes->hapnest = p->hapnest_idx.size();
    sizes->nestdep = p->nestdep_cluster.size();
    sizes->nestdep_var = p->nestdep_var.size();
    return BT_OK;
}

}  // namespace

namespace bt {

int paths_device_candidates(bt_paths *p, const char *who, PathsCandidates *out) {
    if (!p->have_candidates || !p->cand_on_device)
        return fail(std::string(who) + ": the paths handle holds no candidates on the device (bt_paths_candidates_device has not run, or a source took them)");
    out->ctx = p->ctx;
    out->C = p->C;
    out->S = p->S;
    out->R = p->R;
    out->nnz = p->nnz;
    out->kv_words = p->kv_words;
    out->mult_bytes = p->mult_bytes;
    out->num_unique = p->num_unique;
    out->num_multi = p->num_multi;
    out->num_paths = p->num_paths.data();
    out->kmer_off = p->kmer_off.data();
    out->unique_off = p->unique_off.data();
    out->multi_off = p->multi_off.data();
    out->cluster_kv0 = p->cluster_kv0.data();
    out->hap_kmer_mult = p->d_mult;
    out->kmer_has_counts = p->d_has_counts;
    out->kmer_counts = p->d_counts;
    out->kmer_ic_mult = p->d_ic;
    out->kv_off = p->d_kv_off;
    out->kv_var = p->d_kv_var;
    out->kv_bits = p->d_kv_bits;
    out->unique_idx = p->d_unique_idx;
    out->multi_idx = p->d_multi_idx;
    return BT_OK;
}

int paths_number_shared(bt_paths *p, const uint32_t *group_cluster_off, uint32_t G, int32_t **d_kmer_shared, uint32_t *h_group_num_shared) {
    BT_HIP(hipSetDevice(p->ctx->device));
    hipStream_t st = p->ctx->stream;
    const unsigned maxb = p->ctx->num_cu * 16;
    const uint32_t C = p->C;
    const uint64_t R = p->R, M = p->num_multi;
    std::vector<void *> tmp;
    int32_t *d_shared = nullptr;
    auto cleanup = [&](bool all) {
        (void)hipStreamSynchronize(st);
        for (void *q : tmp) (void)hipFree(q);
        if (all && d_shared) (void)hipFree(d_shared);
    };
#define TRYC(x)                  \
    do {                         \
        const int _rc = (x);     \
        if (_rc != BT_OK) {      \
            cleanup(true);       \
            return _rc;          \
        }                        \
    } while (0)
#define HIPC(call)                                                                      \
    do {                                                                                \
        hipError_t _e = (call);                                                         \
        if (_e != hipSuccess) {                                                         \
            cleanup(true);                                                              \
            return bt::fail(std::string(#call) + ": " + hipGetErrorString(_e));         \
        }                                                                               \
    } while (0)
    {
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&d_shared), std::max<uint64_t>(R * 4, 16));
        if (e != hipSuccess) return fail(std::string("bt_gibbs_source_create_from_paths: device allocation: ") + hipGetErrorString(e));
    }
    HIPC(hipMemsetAsync(d_shared, 0xFF, std::max<uint64_t>(R * 4, 16), st));   // -1: not a multicluster row
    for (uint32_t g = 0; g < G; ++g) h_group_num_shared[g] = 0;
    if (M) {
        std::vector<uint32_t> cluster_group(C), group_m0(G);
        for (uint32_t g = 0; g < G; ++g) {
            group_m0[g] = p->multi_off[group_cluster_off[g]];
            for (uint32_t c = group_cluster_off[g]; c < group_cluster_off[g + 1]; ++c) cluster_group[c] = g;
        }
        const uint64_t cap = pow2_at_least(2 * M);
        uint64_t *klo = nullptr, *khi = nullptr;
        uint32_t *ktag = nullptr, *kstate = nullptr, *kfirst = nullptr, *item_slot = nullptr, *item_row = nullptr, *is_first = nullptr, *before = nullptr;
        uint32_t *d_multi_off = nullptr, *d_kmer_off = nullptr, *d_cluster_group = nullptr, *d_group_m0 = nullptr, *d_group_end = nullptr, *d_group_n = nullptr;
        TRYC(dev_alloc(&klo, cap, tmp));
        TRYC(dev_alloc(&khi, cap, tmp));
        TRYC(dev_alloc(&ktag, cap, tmp));
        TRYC(dev_alloc(&kstate, cap, tmp));
        TRYC(dev_alloc(&kfirst, cap, tmp));
        TRYC(dev_alloc(&item_slot, M, tmp));
        TRYC(dev_alloc(&item_row, M, tmp));
        TRYC(dev_alloc(&is_first, M, tmp));
        TRYC(dev_alloc(&before, M + 1, tmp));
        TRYC(dev_alloc(&d_multi_off, C + 1, tmp));
        TRYC(dev_alloc(&d_kmer_off, C + 1, tmp));
        TRYC(dev_alloc(&d_cluster_group, C, tmp));
        TRYC(dev_alloc(&d_group_m0, G + 1, tmp));
        TRYC(dev_alloc(&d_group_n, G + 1, tmp));
        (void)d_group_end;
        HIPC(hipMemsetAsync(kstate, 0, cap * 4, st));
        HIPC(hipMemsetAsync(kfirst, 0xFF, cap * 4, st));
        HIPC(hipMemcpy(d_multi_off, p->multi_off.data(), (size_t)(C + 1) * 4, hipMemcpyHostToDevice));
        HIPC(hipMemcpy(d_kmer_off, p->kmer_off.data(), (size_t)(C + 1) * 4, hipMemcpyHostToDevice));
        HIPC(hipMemcpy(d_cluster_group, cluster_group.data(), (size_t)C * 4, hipMemcpyHostToDevice));
        group_m0.push_back((uint32_t)M);
        HIPC(hipMemcpy(d_group_m0, group_m0.data(), (size_t)(G + 1) * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(shared_index_kernel, dim3(grid_for(M, BLOCK, maxb)), dim3(BLOCK), 0, st, p->d_multi_idx, d_multi_off, d_kmer_off, d_cluster_group, C, p->d_key, (uint32_t)M, klo,
                           khi, ktag, kstate, kfirst, cap - 1, item_slot, item_row);
        hipLaunchKernelGGL(shared_first_kernel, dim3(grid_for(M, BLOCK, maxb)), dim3(BLOCK), 0, st, item_slot, kfirst, (uint32_t)M, is_first);
        HIPC(hipGetLastError());
        uint64_t firsts = 0;
        TRYC(exclusive_scan(p->ctx, is_first, M, before, &firsts, "shared k-mer records", tmp));
        hipLaunchKernelGGL(shared_number_kernel, dim3(grid_for(M, BLOCK, maxb)), dim3(BLOCK), 0, st, item_slot, item_row, kfirst, ktag, before, d_group_m0, (uint32_t)M, d_shared);
        hipLaunchKernelGGL(gather_u32_idx32_kernel, dim3((G + 1 + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, before, d_group_m0, G + 1, d_group_n);
        HIPC(hipGetLastError());
        std::vector<uint32_t> at(G + 1);
        HIPC(hipMemcpyAsync(at.data(), d_group_n, (size_t)(G + 1) * 4, hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
        // (groups are in cluster order, so group g's rows end where group g + 1's begin; the last one ends at M)
        for (uint32_t g = 0; g < G; ++g) h_group_num_shared[g] = at[g + 1] - at[g];
    }
    cleanup(false);
#undef TRYC
#undef HIPC
    *d_kmer_shared = d_shared;
    return BT_OK;
}

void paths_release_candidates(bt_paths *p, std::vector<void *> &allocs) {
    for (void *q : p->cand_owned) {
        if (q == p->d_key) (void)hipFree(q);   // (the keys only serve the numbering of the shared records)
        else allocs.push_back(q);
    }
    p->cand_owned.clear();
    p->drop_device_candidates();
    p->have_candidates = false;
}

}  // namespace bt

extern "C" {

int bt_paths_candidates_device(bt_paths *p, bt_table *table, bt_paths_candidates_sizes *sizes) { return candidates_build(p, table, sizes); }

// "device build + copies to the host": the per-row arrays come back into host vectors (what bt_paths_candidates_fetch hands out) and leave the device
int bt_paths_candidates(bt_paths *p, bt_table *table, bt_paths_candidates_sizes *sizes) {
    const int rc = candidates_build(p, table, sizes);
    if (rc != BT_OK) return rc;
    hipError_t e = hipSuccess;
    auto down = [&](auto &v, const auto *d, uint64_t n) {
        if (e != hipSuccess) return;
        v.resize(n);
        if (n) e = hipMemcpy(v.data(), d, n * sizeof(v[0]), hipMemcpyDeviceToHost);
    };
    try {
        down(p->mult, p->d_mult, p->mult_bytes);
        down(p->key, p->d_key, 2 * p->R);
        down(p->has_counts, p->d_has_counts, p->R);
        down(p->counts, p->d_counts, p->R * p->S);
        down(p->ic, p->d_ic, 2 * p->R);
        down(p->kv_off, p->d_kv_off, p->R + 1);
        down(p->kv_var, p->d_kv_var, p->nnz);
        down(p->kv_bits, p->d_kv_bits, p->kv_words);
        down(p->unique_idx, p->d_unique_idx, p->num_unique);
        down(p->multi_idx, p->d_multi_idx, p->num_multi);
    } catch (const std::exception &ex) {
        p->drop_device_candidates();
        p->have_candidates = false;
        return fail(std::string("bt_paths_candidates: ") + ex.what());
    }
    p->drop_device_candidates();
    if (e != hipSuccess) {
        p->have_candidates = false;
        return fail(std::string("bt_paths_candidates: copying the bundle to the host: ") + hipGetErrorString(e));
    }
    return BT_OK;
}

int bt_paths_candidates_fetch_small(bt_paths *p, bt_paths_candidates_out *o) {
    if (!p || !o) return fail("bt_paths_candidates_fetch_small: null argument");
    if (!p->have_candidates) return fail("bt_paths_candidates_fetch_small: no candidates (bt_paths_candidates / bt_paths_candidates_device has not run, or a source took them)");
    if (o->hap_kmer_mult || o->kmer_key || o->kmer_has_counts || o->kmer_counts || o->kmer_ic_mult || o->kv_off || o->kv_var || o->kv_bits || o->unique_idx || o->multi_idx)
        return fail("bt_paths_candidates_fetch_small: the per-row pointers must be NULL");
    auto cp = [](const auto &v, auto *dst) {
        if (dst && !v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(v[0]));
    };
    cp(p->kmer_off, o->kmer_off);
    cp(p->unique_off, o->unique_off);
    cp(p->multi_off, o->multi_off);
    cp(p->hap_allele, o->hap_allele);
    cp(p->hapnest_off, o->hapnest_off);
    cp(p->hapnest_idx, o->hapnest_idx);
    cp(p->nestdep_off, o->nestdep_off);
    cp(p->nestdep_cluster, o->nestdep_cluster);
    cp(p->nestdep_var_off, o->nestdep_var_off);
    cp(p->nestdep_var, o->nestdep_var);
    return BT_OK;
}

int bt_paths_candidates_fetch(bt_paths *p, bt_paths_candidates_out *o) {
    if (!p || !o) return fail("bt_paths_candidates_fetch: null argument");
    if (!p->have_candidates) return fail("bt_paths_candidates_fetch: bt_paths_candidates has not run");
    if (p->cand_on_device) return fail("bt_paths_candidates_fetch: the per-row arrays are on the device (bt_paths_candidates_device): use bt_paths_candidates_fetch_small");
    auto cp = [](const auto &v, auto *dst) {   // (the large arrays on several threads: one core's memcpy into fresh pages is the slow part)
        if (!dst || v.empty()) return;
        const size_t bytes = v.size() * sizeof(v[0]);
        const unsigned T = host_threads(bytes >> 14);   // at least 4 MB per thread
        const uint8_t *src = reinterpret_cast<const uint8_t *>(v.data());
        uint8_t *out = reinterpret_cast<uint8_t *>(dst);
        try {
            run_on_threads(T, [&](unsigned t) {
                const size_t a = bytes * t / T / 64 * 64, b = t + 1 == T ? bytes : bytes * (t + 1) / T / 64 * 64;
                if (b > a) std::memcpy(out + a, src + a, b - a);
            });
        } catch (...) {   // (no thread could be started: one copy)
            std::memcpy(out, src, bytes);
        }
    };
    cp(p->kmer_off, o->kmer_off);
    cp(p->mult, o->hap_kmer_mult);
    cp(p->key, o->kmer_key);
    cp(p->has_counts, o->kmer_has_counts);
    cp(p->counts, o->kmer_counts);
    cp(p->ic, o->kmer_ic_mult);
    cp(p->kv_off, o->kv_off);
    cp(p->kv_var, o->kv_var);
    cp(p->kv_bits, o->kv_bits);
    cp(p->unique_off, o->unique_off);
    cp(p->unique_idx, o->unique_idx);
    cp(p->multi_off, o->multi_off);
    cp(p->multi_idx, o->multi_idx);
    cp(p->hap_allele, o->hap_allele);
    cp(p->hapnest_off, o->hapnest_off);
    cp(p->hapnest_idx, o->hapnest_idx);
    cp(p->nestdep_off, o->nestdep_off);
    cp(p->nestdep_cluster, o->nestdep_cluster);
    cp(p->nestdep_var_off, o->nestdep_var_off);
    cp(p->nestdep_var, o->nestdep_var);
    return BT_OK;
}

}  // extern "C"
