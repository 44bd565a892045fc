// libbtgpu — the per-sample best-path search: VariantClusterGraph::findSamplePaths / mergePaths / isPathsRedundant / filterPaths /
// addPathIndices (src/bayesTyper/VariantClusterGraph.cpp:389-798) with VariantClusterGraphPath (VariantClusterGraphPath.cpp:38-225).
//
// The search is a sequential dynamic programme over the vertices of ONE cluster (candidate paths of a vertex = merged paths of
// its predecessors, shuffled with the cluster's mt19937, extended by the vertex with one sample-Bloom lookup per completed k-mer,
// then cut to max_sample_haplotypes by a two-pass greedy); clusters are independent.  As for the Gibbs sampler the unit of
// parallelism is therefore the cluster, and the random accesses into the (GB-sized) sample Bloom filter of thousands of concurrently
// running searches overlap in HBM.  Every cluster works in a private scratch region (scratch_layout: path slots with a free list,
// per-vertex path lists, the cluster's generator), contiguous, not lane-interleaved (DESIGN.md §7 lists that as the next step).
// Integer work except the k-mer score ratio (fp64 division, IEEE).
//
// There is ONE search, written once as templates over the TEAM that executes a cluster:
//   LaneTeam — one lane.  find_paths_kernel: a launch carries all clusters of a unit, 64 per workgroup.
//   WaveTeam — the 64 lanes of a wavefront.  find_paths_wave_kernel: one 64-thread workgroup per cluster of at least
//              BT_FIND_PATHS_WAVE_MIN vertices (the search is quadratic in the vertex count).
// What is independent is spread over the team's lanes — the candidate paths of a vertex in add_vertex, the existing paths a
// merged-in path is tested against (lowest match wins: ballot, first set bit), the scores of a greedy round, the words of a copy,
// the bytes of a row —, what is order-dependent (free list, appends to cur, the greedy scan with its tolerance compare) is
// executed by every lane on the same values or, where it reads what it writes (shuffle, swaps, generator), by lane 0.  Phases that
// hand data from one lane to another are separated by sync(); no loop waits for another lane.  With a team of one, `for (i = lane();
// i < n; i += W)` is the plain loop, a ballot is the flag itself, lane() == 0 always holds and sync() is nothing: the sequential
// search.  The teams differ in one place, filter_paths: a wavefront computes the scores of a greedy round over its lanes into
// arrays of its scratch region and moves them with their paths, a single lane computes a candidate's scores when the scan reaches
// it and has no such arrays.
//
// The samples depend on each other from addPathIndices on only.  One sample per call (bt_find_paths_sample) runs a cluster's whole routine,
// find_paths_cluster, in one kernel.  n samples per call (bt_find_paths_samples) use its two halves: search_cluster (findSamplePaths, mergePaths,
// filterPaths: graph, filter and seed in, final paths left in the scratch region) for every (sample, cluster) at once, sample j in scratch copy j
// (find_paths_search_kernel / _search_wave_kernel), then fold_cluster (addPathIndices into the accumulated rows) by one team per cluster over copy 0 .. n-1
// in that order (find_paths_fold_kernel / _fold_wave_kernel).  Search and fold are ordered by the stream.
#include "bt_internal.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "bt_rng_device.hpp"

using namespace bt;

namespace {

constexpr uint32_t MIN_OBSERVED_KMERS = 2;      // VariantClusterGraphPath.cpp:36
constexpr uint32_t MIN_NUM_SAMPLE_PATHS = 1;    // VariantClusterGraph.cpp:60
constexpr uint32_t WAVE_MIN_DEFAULT = 0;        // BT_FIND_PATHS_WAVE_MIN when unset (profiles/find_paths_wide.txt); 0: every cluster on the lane kernel
constexpr uint32_t HDR_WORDS = 8;               // slot header: len, score_first, score_second, window count, window lo (2), window hi (2)

struct FindCluster {
    uint32_t v0, nv;
    uint32_t cap_slots, cur_cap;
    uint32_t slot_words;      // HDR_WORDS + nv
    uint32_t best_cap;        // rows the best-path bitmap can hold
    uint64_t scratch;         // word offset of the cluster's scratch region
    uint64_t best;            // byte offset of the cluster's best rows
};

struct FindGraph {
    const uint64_t *seq_off;
    const uint8_t *seq;
    const uint8_t *vflags;
    const uint32_t *in_off, *in_src;   // in_off indexed by global vertex
    const uint32_t *last_use;          // per global vertex: local index of its last successor (or its own index)
};

// who executes one cluster's search
struct LaneTeam {
    static constexpr uint32_t W = 1;
    __device__ static uint32_t lane() { return 0; }
    __device__ static void sync() {}
    __device__ static uint32_t uni(uint32_t x) { return x; }
    __device__ static unsigned long long ballot(bool b) { return b ? 1ull : 0ull; }
};
struct WaveTeam {
    static constexpr uint32_t W = 64;
    __device__ static uint32_t lane() { return threadIdx.x; }
    __device__ static void sync() { __syncthreads(); }
    __device__ static uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }   // a value every lane holds alike
    __device__ static unsigned long long ballot(bool b) { return __ballot(b); }
};

// one cluster's scratch region: word offsets of its arrays from the region's start, and its size
struct ScratchLayout {
    uint64_t slots;       // cap_slots * slot_words
    uint64_t free_stack;  // cap_slots
    uint64_t vlist;       // nv * max_haps
    uint64_t vcount;      // nv
    uint64_t cur;         // cur_cap
    uint64_t tmp;         // nv   (vertex list of a best row)
    uint64_t covered;     // nv   (0/1)
    uint64_t mt;          // MT_WORDS
    uint64_t kscore;      // wavefront only: cur_cap doubles (scores of the candidate paths of a greedy round, by position in cur)
    uint64_t vscore;      // wavefront only: cur_cap
    uint64_t plen;        // wavefront only: cur_cap
    uint64_t total;       // a multiple of four words
};
__host__ __device__ inline ScratchLayout scratch_layout(const FindCluster &fc, uint32_t max_haps, bool wave) {
    ScratchLayout l{};
    uint64_t o = 0;
    l.slots = o;
    o += (uint64_t)fc.cap_slots * fc.slot_words;
    l.free_stack = o;
    o += fc.cap_slots;
    l.vlist = o;
    o += (uint64_t)fc.nv * max_haps;
    l.vcount = o;
    o += fc.nv;
    l.cur = o;
    o += fc.cur_cap;
    l.tmp = o;
    o += fc.nv;
    l.covered = o;
    o += fc.nv;
    l.mt = o;
    o += MT_WORDS;
    if (wave) {
        // a region starts at a multiple of four words, so an even offset is 8-byte aligned; the pad word is reserved whether it is used or not
        l.kscore = o + (o & 1u);
        l.vscore = l.kscore + 2ull * fc.cur_cap;
        l.plen = l.vscore + fc.cur_cap;
        o += 1 + 4ull * fc.cur_cap;
    }
    l.total = (o + 3) & ~3ull;
    return l;
}

// view of one cluster's scratch region
struct Work {
    uint32_t *slots, *free_stack, *vlist, *vcount, *cur, *tmp, *covered, *mt;   // (ScratchLayout)
    double *kscore;       // wavefront only, with vscore and plen: never set for a team of one, and read only under `if constexpr (T::W > 1)`
    uint32_t *vscore, *plen;
    uint32_t free_top;
    uint32_t slot_words, nv, v0, k, max_haps;
    FindGraph g;
    BloomView bloom;
    uint32_t *overflow;   // global flag
};

__device__ inline uint32_t vlen(const Work &w, uint32_t vi) { return (uint32_t)(w.g.seq_off[w.v0 + vi + 1] - w.g.seq_off[w.v0 + vi]); }
__device__ inline uint32_t vnt(const Work &w, uint32_t vi, uint32_t i) { return w.g.seq[w.g.seq_off[w.v0 + vi] + i] & 3u; }
__device__ inline bool vdisc(const Work &w, uint32_t vi) { return w.g.vflags[w.v0 + vi] & 1u; }
__device__ inline bool vredundant(const Work &w, uint32_t vi) { return w.g.vflags[w.v0 + vi] & 2u; }
__device__ inline uint32_t *slot(const Work &w, uint32_t s) { return w.slots + (size_t)s * w.slot_words; }
__device__ inline uint32_t ent_index(uint32_t e) { return e & 0xFFFFFFu; }
__device__ inline uint32_t ent_obs(uint32_t e) { return e >> 24; }

template <class T>
__device__ inline uint32_t slot_alloc(Work &w) {   // every lane: the same pop
    if (w.free_top == 0) {
        if (T::lane() == 0) atomicExch(w.overflow, 1u);
        return 0;
    }
    return T::uni(w.free_stack[--w.free_top]);
}
__device__ inline void slot_free(Work &w, uint32_t s) { w.free_stack[w.free_top++] = s; }
// words over lanes; the caller separates it from readers of dst and writers of src
template <class T>
__device__ inline void slot_copy(const Work &w, uint32_t dst, uint32_t src) {
    const uint32_t *a = slot(w, src);
    uint32_t *b = slot(w, dst);
    const uint32_t n = HDR_WORDS + T::uni(a[0]);
    for (uint32_t i = T::lane(); i < n; i += T::W) b[i] = a[i];
}

// VariantClusterGraphPath::updateScore (VariantClusterGraphPath.cpp:87-129)
__device__ inline void update_score(const Work &w, uint32_t *p, bool observed, uint32_t cur_sequence_length) {
    uint32_t *ent = p + HDR_WORDS;
    if (observed) {
        p[1]++;
        int32_t r = (int32_t)p[0] - 1;
        if (cur_sequence_length > 1 || !vredundant(w, ent_index(ent[r]))) {
            if (ent_obs(ent[r]) < MIN_OBSERVED_KMERS) ent[r] += 1u << 24;
        }
        for (--r; r >= 0; --r) {
            if (w.k <= cur_sequence_length || ent_obs(ent[r]) == MIN_OBSERVED_KMERS) break;
            if (ent_obs(ent[r]) < MIN_OBSERVED_KMERS) ent[r] += 1u << 24;
            cur_sequence_length += vlen(w, ent_index(ent[r]));
        }
    }
    p[2]++;
}
// VariantClusterGraphPath::addVertex (:46-85): the window is the forward k-mer of KmerPair (Kmer.tpp:44-81); count = valid nucleotides since reset
__device__ inline void add_vertex(const Work &w, uint32_t *p, uint32_t vi) {
    uint32_t *ent = p + HDR_WORDS;
    ent[p[0]] = vi;
    p[0]++;
    if (vdisc(w, vi)) {
        if (vlen(w, vi) == 0) ent[p[0] - 1] = vi | (MIN_OBSERVED_KMERS << 24);
        p[3] = 0;
    }
    Kmer fw{(uint64_t)p[4] | ((uint64_t)p[5] << 32), (uint64_t)p[6] | ((uint64_t)p[7] << 32)};
    uint32_t cnt = p[3];
    const uint32_t n = vlen(w, vi), top = 2u * (w.k - 1u);
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t c = vnt(w, vi, i);
        // shift one nucleotide out at the bottom, write the new one at position k-1
        fw.lo = (fw.lo >> 2) | (fw.hi << 62);
        fw.hi >>= 2;
        if (top >= 64u) fw.hi |= c << (top - 64u);
        else fw.lo |= c << top;
        fw = kmer_mask(fw, w.k);
        if (cnt < w.k) ++cnt;
        if (cnt == w.k) {
            const Kmer low = kmer_canonical(fw, w.k);
            update_score(w, p, bloom_contains(nthash64(low, w.k), w.bloom), i + 1u);
        }
    }
    p[3] = cnt;
    p[4] = (uint32_t)fw.lo;
    p[5] = (uint32_t)(fw.lo >> 32);
    p[6] = (uint32_t)fw.hi;
    p[7] = (uint32_t)(fw.hi >> 32);
}
__device__ inline double kmer_score(const uint32_t *p) { return p[2] > 0 ? p[1] / static_cast<double>(p[2]) : 1.0; }   // :136-148
__device__ inline uint32_t vertex_score(const Work &w, const uint32_t *p, bool is_complete) {                         // :150-188
    const uint32_t *ent = p + HDR_WORDS;
    uint32_t score = 0;
    for (uint32_t i = 0; i < p[0]; ++i)
        if (ent_obs(ent[i]) == MIN_OBSERVED_KMERS && !w.covered[ent_index(ent[i])]) ++score;
    if (!is_complete) {
        uint32_t cur = 0;
        for (int32_t r = (int32_t)p[0] - 1; r >= 0; --r) {
            if ((w.k - 1u) <= cur || ent_obs(ent[r]) == MIN_OBSERVED_KMERS) break;
            if (!w.covered[ent_index(ent[r])]) ++score;
            cur += vlen(w, ent_index(ent[r]));
        }
    }
    return score;
}
template <class T>
__device__ inline void clear_covered(const Work &w) {
    for (uint32_t i = T::lane(); i < w.nv; i += T::W) w.covered[i] = 0;
}
// :190-225; the entries over lanes (every write is a 1), the short tail walk by every lane alike
template <class T>
__device__ inline void update_covered(const Work &w, const uint32_t *p, bool is_complete) {
    const uint32_t *ent = p + HDR_WORDS;
    const uint32_t len = T::uni(p[0]);
    for (uint32_t i = T::lane(); i < len; i += T::W)
        if (ent_obs(ent[i]) == MIN_OBSERVED_KMERS) w.covered[ent_index(ent[i])] = 1;
    if (!is_complete) {
        uint32_t cur = 0;
        for (int32_t r = (int32_t)len - 1; r >= 0; --r) {
            if ((w.k - 1u) <= cur || ent_obs(ent[r]) == MIN_OBSERVED_KMERS) break;
            w.covered[ent_index(ent[r])] = 1;
            cur += vlen(w, ent_index(ent[r]));
        }
    }
}
// isPathsRedundant (VariantClusterGraph.cpp:525-626): both vertex lists spell the same nucleotides and separators, read backwards
__device__ inline bool paths_redundant(const Work &w, const uint32_t *e1, uint32_t n1, const uint32_t *e2, uint32_t n2) {
    int32_t i1 = (int32_t)n1 - 1, i2 = (int32_t)n2 - 1;
    uint32_t r1 = vlen(w, ent_index(e1[i1])), r2 = vlen(w, ent_index(e2[i2]));
    bool d1 = false, d2 = false;
    while (true) {
        while (r1 == 0) {
            if (vdisc(w, ent_index(e1[i1]))) d1 = true;
            --i1;
            if (i1 >= 0) r1 = vlen(w, ent_index(e1[i1]));
            else break;
        }
        while (r2 == 0) {
            if (vdisc(w, ent_index(e2[i2]))) d2 = true;
            --i2;
            if (i2 >= 0) r2 = vlen(w, ent_index(e2[i2]));
            else break;
        }
        if (d1 != d2) return false;
        d1 = false;
        d2 = false;
        if (i1 < 0 || i2 < 0) break;
        const uint32_t a = ent_index(e1[i1]), b = ent_index(e2[i2]);
        if (a == b && r1 == r2) {   // the same position of the same vertex: the rest of this vertex is shared
            r1 = 0;
            r2 = 0;
        }
        while (r1 != 0 && r2 != 0) {
            if (vnt(w, a, r1 - 1) != vnt(w, b, r2 - 1)) return false;
            --r1;
            --r2;
        }
    }
    return !(i1 >= 0 || i2 >= 0);
}
// index of the lowest m in [0, n) for which the path of slot_of(m) (0xFFFFFFFF: none) and the fixed path e2 / n2 are redundant, or n; FIXED_FIRST: the
// fixed path is the first argument of paths_redundant (addPathIndices), else the second (mergePaths)
template <class T, bool FIXED_FIRST, class SlotOf>
__device__ inline uint32_t first_redundant(const Work &w, uint32_t n, SlotOf slot_of, const uint32_t *e2, uint32_t n2) {
    for (uint32_t base = 0; base < n; base += T::W) {
        const uint32_t m = base + T::lane();
        bool hit = false;
        if (m < n) {
            const uint32_t s = slot_of(m);
            if (s != 0xFFFFFFFFu) {
                const uint32_t *mp = slot(w, s);
                hit = FIXED_FIRST ? paths_redundant(w, e2, n2, mp + HDR_WORDS, mp[0]) : paths_redundant(w, mp + HDR_WORDS, mp[0], e2, n2);
            }
        }
        const unsigned long long mask = T::ballot(hit);
        if (mask) return base + (uint32_t)__builtin_ctzll(mask);
    }
    return n;
}
// mergePaths (:474-523), copy semantics (the reference's move on the last edge is an optimisation)
template <class T>
__device__ inline void merge_paths(Work &w, uint32_t &ncur, const uint32_t *in, uint32_t nin, uint32_t cur_cap) {
    const uint32_t main_size = ncur;
    for (uint32_t j = 0; j < nin; ++j) {
        const uint32_t sj = T::uni(in[j]);
        const uint32_t *ip = slot(w, sj);
        const uint32_t ilen = T::uni(ip[0]);
        const uint32_t m = first_redundant<T, false>(w, main_size, [&](uint32_t i) { return w.cur[i]; }, ip + HDR_WORDS, ilen);
        T::sync();   // (the tests have read what the copy below overwrites)
        if (m < main_size) {
            const uint32_t sm = T::uni(w.cur[m]);
            if (T::uni(slot(w, sm)[0]) < ilen) slot_copy<T>(w, sm, sj);
        } else {
            if (ncur >= cur_cap) {
                if (T::lane() == 0) atomicExch(w.overflow, 1u);
                return;
            }
            const uint32_t s = slot_alloc<T>(w);
            slot_copy<T>(w, s, sj);
            w.cur[ncur++] = s;
        }
        T::sync();
    }
}
__device__ inline bool double_compare(double a, double b) {   // Utils::doubleCompare (Utils.hpp:81-87)
    const double mn = a < b ? a : b;
    return a == b || fabs(a - b) < fabs(mn) * 2.220446049250313080847263336181640625e-16 * 100;
}
// k-mer score, vertex score and length of the candidate path at position `it` of cur: a wavefront reads what the fill of its greedy round wrote, a
// lane computes them here
struct Scores {
    double kmer;
    uint32_t vertex, len;
};
template <class T>
__device__ inline Scores scores_at(const Work &w, uint32_t it, bool is_complete) {
    if constexpr (T::W > 1) {
        return Scores{w.kscore[it], w.vscore[it], w.plen[it]};
    } else {
        const uint32_t *p = slot(w, w.cur[it]);
        return Scores{kmer_score(p), vertex_score(w, p, is_complete), p[0]};
    }
}
// filterPaths (:628-724)
template <class T>
__device__ inline void filter_paths(Work &w, uint32_t &ncur, uint32_t max_paths, bool is_complete) {
    if (!(ncur > max_paths || (is_complete && ncur > MIN_NUM_SAMPLE_PATHS))) return;
    bool is_first_pass = true;
    [[maybe_unused]] bool fresh = true;
    clear_covered<T>(w);
    T::sync();
    uint32_t sorted_end = 0;
    while (sorted_end != ncur) {
        if constexpr (T::W > 1) {
            // the scores of this round over the lanes: in the first pass `covered` changed, in the second they are the same numbers round after round
            // (and move with their paths)
            if (fresh) {
                for (uint32_t it = sorted_end + T::lane(); it < ncur; it += T::W) {
                    const uint32_t *p = slot(w, w.cur[it]);
                    w.kscore[it] = kmer_score(p);
                    w.vscore[it] = vertex_score(w, p, is_complete);
                    w.plen[it] = p[0];
                }
                T::sync();
            }
            fresh = is_first_pass;
        }
        // the scan of filterPaths, by every lane alike (the tolerance compare is not associative: no tree reduction)
        const Scores front = scores_at<T>(w, sorted_end, is_complete);
        uint32_t best = sorted_end;
        double best_kmer = front.kmer;
        uint32_t best_vertex = front.vertex;
        for (uint32_t it = sorted_end + 1; it < ncur; ++it) {
            const Scores c = scores_at<T>(w, it, is_complete);
            if (is_first_pass) {
                if (c.vertex > 0) {
                    if ((double_compare(c.kmer, best_kmer) && c.vertex > best_vertex) || c.kmer > best_kmer || best_vertex == 0) {
                        best = it;
                        best_kmer = c.kmer;
                        best_vertex = c.vertex;
                    }
                }
            } else if (!is_complete || c.vertex == c.len) {
                if (c.kmer > best_kmer) {
                    best = it;
                    best_kmer = c.kmer;
                    best_vertex = c.vertex;
                }
            }
        }
        best = T::uni(best);
        best_vertex = T::uni(best_vertex);
        const uint32_t s_best = T::uni(w.cur[best]), s_front = T::uni(w.cur[sorted_end]);
        const uint32_t best_len = T::uni(scores_at<T>(w, best, is_complete).len);
        if (is_first_pass) update_covered<T>(w, slot(w, s_best), is_complete);
        else if (is_complete && sorted_end >= MIN_NUM_SAMPLE_PATHS && best_vertex < best_len) break;
        T::sync();   // (every lane has read cur and the scores)
        if (sorted_end != best && T::lane() == 0) {
            w.cur[sorted_end] = s_best;
            w.cur[best] = s_front;
            if constexpr (T::W > 1) {
                w.kscore[sorted_end] = best_kmer, w.vscore[sorted_end] = best_vertex, w.plen[sorted_end] = best_len;
                w.kscore[best] = front.kmer, w.vscore[best] = front.vertex, w.plen[best] = front.len;
            }
        }
        if (is_first_pass && best_vertex == 0) {
            is_first_pass = false;
            clear_covered<T>(w);
        } else {
            ++sorted_end;
            if (sorted_end == max_paths) break;
        }
        T::sync();
    }
    T::sync();
    for (uint32_t i = sorted_end; i < ncur; ++i) slot_free(w, T::uni(w.cur[i]));
    ncur = sorted_end;
}
// a best row := the vertices of path p (bytes over lanes)
template <class T>
__device__ inline void write_row(uint8_t *row, uint32_t nv, const uint32_t *p) {
    for (uint32_t vi = T::lane(); vi < nv; vi += T::W) row[vi] = 0;
    T::sync();
    const uint32_t len = T::uni(p[0]);
    for (uint32_t i = T::lane(); i < len; i += T::W) row[ent_index(p[HDR_WORDS + i])] = 1;
}

// the search of one cluster by team T; best_count: the cluster's own counter; max_candidates: null, or where lane 0 records the most candidate paths a vertex had
template <class T>
__device__ __forceinline__ void find_paths_cluster(const FindCluster &fc, uint32_t seed, const FindGraph &g, const BloomView &bloom, uint32_t k, uint32_t max_haps,
                                                   uint32_t *scratch, uint8_t *best_rows, uint32_t *best_count, uint32_t *overflow, uint32_t *max_candidates) {
    const ScratchLayout l = scratch_layout(fc, max_haps, T::W > 1);
    uint32_t *base = scratch + fc.scratch;
    Work w;
    w.slots = base + l.slots;
    w.free_stack = base + l.free_stack;
    w.vlist = base + l.vlist;
    w.vcount = base + l.vcount;
    w.cur = base + l.cur;
    w.tmp = base + l.tmp;
    w.covered = base + l.covered;
    w.mt = base + l.mt;
    if constexpr (T::W > 1) {
        w.kscore = reinterpret_cast<double *>(base + l.kscore);
        w.vscore = base + l.vscore;
        w.plen = base + l.plen;
    }
    w.slot_words = fc.slot_words;
    w.nv = fc.nv;
    w.v0 = fc.v0;
    w.k = k;
    w.max_haps = max_haps;
    w.g = g;
    w.bloom = bloom;
    w.overflow = overflow;
    w.free_top = fc.cap_slots;
    for (uint32_t i = T::lane(); i < fc.cap_slots; i += T::W) w.free_stack[i] = fc.cap_slots - 1u - i;
    for (uint32_t i = T::lane(); i < fc.nv; i += T::W) w.vcount[i] = 0;
    if (T::lane() == 0) mt_seed(w.mt, seed);
    T::sync();
    Mt rng = mt_open(w.mt);   // (lane 0 draws)
    // ---- findSamplePaths (:389-472) ----
    uint32_t ncur = 0, max_cand = 0;
    for (uint32_t vi = 0; vi < fc.nv; ++vi) {
        ncur = 0;
        const uint32_t e0 = g.in_off[fc.v0 + vi], e1 = g.in_off[fc.v0 + vi + 1];
        if (e0 == e1) {
            const uint32_t s = slot_alloc<T>(w);
            for (uint32_t i = T::lane(); i < HDR_WORDS; i += T::W) slot(w, s)[i] = 0;
            w.cur[ncur++] = s;
        } else {
            for (uint32_t e = e0; e < e1; ++e) {
                const uint32_t src = g.in_src[e];
                merge_paths<T>(w, ncur, w.vlist + (size_t)src * max_haps, T::uni(w.vcount[src]), fc.cur_cap);
            }
        }
        T::sync();
        if (T::lane() == 0) rng_shuffle_u32(rng, w.cur, ncur);
        T::sync();
        for (uint32_t i = T::lane(); i < ncur; i += T::W) add_vertex(w, slot(w, w.cur[i]), vi);
        T::sync();
        max_cand = max_cand > ncur ? max_cand : ncur;
        filter_paths<T>(w, ncur, max_haps, false);
        T::sync();
        for (uint32_t i = T::lane(); i < ncur; i += T::W) w.vlist[(size_t)vi * max_haps + i] = w.cur[i];
        w.vcount[vi] = ncur;
        for (uint32_t e = e0; e < e1; ++e) {   // predecessors whose last successor this vertex is are no longer needed
            const uint32_t src = g.in_src[e];
            const uint32_t n = T::uni(w.vcount[src]);
            if (g.last_use[fc.v0 + src] == vi && n) {
                for (uint32_t i = 0; i < n; ++i) slot_free(w, T::uni(w.vlist[(size_t)src * max_haps + i]));
                w.vcount[src] = 0;
            }
        }
        T::sync();
    }
    if (T::lane() == 0) mt_close(rng);
    max_cand = max_cand > ncur ? max_cand : ncur;
    filter_paths<T>(w, ncur, max_haps, true);
    T::sync();
    // ---- addPathIndices (:726-798): the rows in order, a row's test against the final paths over lanes (the first unmarked match wins) ----
    uint8_t *rows = best_rows + fc.best;
    uint32_t nrows = *best_count;
    // redundant flags of the final paths live in the high bit of cur[]
    for (uint32_t r = 0; r < nrows; ++r) {
        uint8_t *row = rows + (size_t)r * fc.nv;
        uint32_t nb = 0;
        for (uint32_t b0 = 0; b0 < fc.nv; b0 += T::W) {   // tmp := the row's vertices, in order
            const uint32_t vi = b0 + T::lane();
            const bool set = vi < fc.nv && row[vi];
            const unsigned long long mask = T::ballot(set);
            if (set) w.tmp[nb + (uint32_t)__popcll(mask & ((1ull << T::lane()) - 1ull))] = vi;
            nb += (uint32_t)__popcll(mask);
        }
        T::sync();
        const uint32_t pi = first_redundant<T, true>(w, ncur, [&](uint32_t i) { const uint32_t s = w.cur[i]; return (s & 0x80000000u) ? 0xFFFFFFFFu : s; }, w.tmp, nb);
        T::sync();
        if (pi < ncur) {
            const uint32_t s = T::uni(w.cur[pi]);
            const uint32_t *p = slot(w, s);
            if (nb < T::uni(p[0])) write_row<T>(row, fc.nv, p);
            if (T::lane() == 0) w.cur[pi] = s | 0x80000000u;
        }
        T::sync();
    }
    for (uint32_t pi = 0; pi < ncur; ++pi) {
        const uint32_t s = T::uni(w.cur[pi]);
        if (s & 0x80000000u) continue;
        if (nrows >= fc.best_cap) {
            if (T::lane() == 0) atomicExch(overflow, 2u);
            break;
        }
        write_row<T>(rows + (size_t)nrows * fc.nv, fc.nv, slot(w, s));
        ++nrows;
    }
    if (T::lane() == 0) {
        *best_count = nrows;
        if (max_candidates) atomicMax(max_candidates, max_cand);
    }
}

// ---- the two halves of find_paths_cluster as functions of their own, for the launches of several samples (bt_find_paths_samples).  They are COPIES: the
// routine above is the text the per-sample kernels were measured with, and compiling those from the halves moved their register allocation and cost the
// wave kernel 0.7 % (profiles/find_paths_samples.txt (c)).  A change to the search rules goes into both. ----

// view of a cluster's scratch region at `base`
template <class T>
__device__ __forceinline__ Work open_work(const FindCluster &fc, const FindGraph &g, const BloomView &bloom, uint32_t k, uint32_t max_haps, uint32_t *base, uint32_t *overflow) {
    const ScratchLayout l = scratch_layout(fc, max_haps, T::W > 1);
    Work w;
    w.slots = base + l.slots;
    w.free_stack = base + l.free_stack;
    w.vlist = base + l.vlist;
    w.vcount = base + l.vcount;
    w.cur = base + l.cur;
    w.tmp = base + l.tmp;
    w.covered = base + l.covered;
    w.mt = base + l.mt;
    if constexpr (T::W > 1) {
        w.kscore = reinterpret_cast<double *>(base + l.kscore);
        w.vscore = base + l.vscore;
        w.plen = base + l.plen;
    }
    w.slot_words = fc.slot_words;
    w.nv = fc.nv;
    w.v0 = fc.v0;
    w.k = k;
    w.max_haps = max_haps;
    w.g = g;
    w.bloom = bloom;
    w.overflow = overflow;
    w.free_top = 0;
    return w;
}

// SEARCH: findSamplePaths, mergePaths and filterPaths of one cluster by team T in the scratch region w.  It reads the graph, the sample's filter and the seed
// only, and leaves the final paths where they are: cur[0 .. ncur) and their slots.  Returns ncur; max_cand: the most candidate paths a vertex had
template <class T>
__device__ __forceinline__ uint32_t search_cluster(Work &w, const FindCluster &fc, uint32_t seed, uint32_t &max_cand) {
    const FindGraph &g = w.g;
    const uint32_t max_haps = w.max_haps;
    w.free_top = fc.cap_slots;
    for (uint32_t i = T::lane(); i < fc.cap_slots; i += T::W) w.free_stack[i] = fc.cap_slots - 1u - i;
    for (uint32_t i = T::lane(); i < fc.nv; i += T::W) w.vcount[i] = 0;
    if (T::lane() == 0) mt_seed(w.mt, seed);
    T::sync();
    Mt rng = mt_open(w.mt);   // (lane 0 draws)
    // ---- findSamplePaths (:389-472) ----
    uint32_t ncur = 0;
    max_cand = 0;
    for (uint32_t vi = 0; vi < fc.nv; ++vi) {
        ncur = 0;
        const uint32_t e0 = g.in_off[fc.v0 + vi], e1 = g.in_off[fc.v0 + vi + 1];
        if (e0 == e1) {
            const uint32_t s = slot_alloc<T>(w);
            for (uint32_t i = T::lane(); i < HDR_WORDS; i += T::W) slot(w, s)[i] = 0;
            w.cur[ncur++] = s;
        } else {
            for (uint32_t e = e0; e < e1; ++e) {
                const uint32_t src = g.in_src[e];
                merge_paths<T>(w, ncur, w.vlist + (size_t)src * max_haps, T::uni(w.vcount[src]), fc.cur_cap);
            }
        }
        T::sync();
        if (T::lane() == 0) rng_shuffle_u32(rng, w.cur, ncur);
        T::sync();
        for (uint32_t i = T::lane(); i < ncur; i += T::W) add_vertex(w, slot(w, w.cur[i]), vi);
        T::sync();
        max_cand = max_cand > ncur ? max_cand : ncur;
        filter_paths<T>(w, ncur, max_haps, false);
        T::sync();
        for (uint32_t i = T::lane(); i < ncur; i += T::W) w.vlist[(size_t)vi * max_haps + i] = w.cur[i];
        w.vcount[vi] = ncur;
        for (uint32_t e = e0; e < e1; ++e) {   // predecessors whose last successor this vertex is are no longer needed
            const uint32_t src = g.in_src[e];
            const uint32_t n = T::uni(w.vcount[src]);
            if (g.last_use[fc.v0 + src] == vi && n) {
                for (uint32_t i = 0; i < n; ++i) slot_free(w, T::uni(w.vlist[(size_t)src * max_haps + i]));
                w.vcount[src] = 0;
            }
        }
        T::sync();
    }
    if (T::lane() == 0) mt_close(rng);
    max_cand = max_cand > ncur ? max_cand : ncur;
    filter_paths<T>(w, ncur, max_haps, true);
    T::sync();
    return ncur;
}

// FOLD: addPathIndices (:726-798) of the final paths a search left in the scratch region w (cur[0 .. ncur), ncur <= cur_cap) into the cluster's accumulated
// rows; best_count: the cluster's own counter.  The rows in order, a row's test against the final paths over lanes (the first unmarked match wins).  This is
// the one part of a sample's search that depends on the samples before it
template <class T>
__device__ __forceinline__ void fold_cluster(Work &w, const FindCluster &fc, uint32_t ncur, uint8_t *best_rows, uint32_t *best_count) {
    uint32_t *overflow = w.overflow;
    uint8_t *rows = best_rows + fc.best;
    uint32_t nrows = *best_count;
    // redundant flags of the final paths live in the high bit of cur[]
    for (uint32_t r = 0; r < nrows; ++r) {
        uint8_t *row = rows + (size_t)r * fc.nv;
        uint32_t nb = 0;
        for (uint32_t b0 = 0; b0 < fc.nv; b0 += T::W) {   // tmp := the row's vertices, in order
            const uint32_t vi = b0 + T::lane();
            const bool set = vi < fc.nv && row[vi];
            const unsigned long long mask = T::ballot(set);
            if (set) w.tmp[nb + (uint32_t)__popcll(mask & ((1ull << T::lane()) - 1ull))] = vi;
            nb += (uint32_t)__popcll(mask);
        }
        T::sync();
        const uint32_t pi = first_redundant<T, true>(w, ncur, [&](uint32_t i) { const uint32_t s = w.cur[i]; return (s & 0x80000000u) ? 0xFFFFFFFFu : s; }, w.tmp, nb);
        T::sync();
        if (pi < ncur) {
            const uint32_t s = T::uni(w.cur[pi]);
            const uint32_t *p = slot(w, s);
            if (nb < T::uni(p[0])) write_row<T>(row, fc.nv, p);
            if (T::lane() == 0) w.cur[pi] = s | 0x80000000u;
        }
        T::sync();
    }
    for (uint32_t pi = 0; pi < ncur; ++pi) {
        const uint32_t s = T::uni(w.cur[pi]);
        if (s & 0x80000000u) continue;
        if (nrows >= fc.best_cap) {
            if (T::lane() == 0) atomicExch(overflow, 2u);
            break;
        }
        write_row<T>(rows + (size_t)nrows * fc.nv, fc.nv, slot(w, s));
        ++nrows;
    }
    if (T::lane() == 0) *best_count = nrows;
}

__global__ __launch_bounds__(64) void find_paths_kernel(const FindCluster *__restrict__ clusters, uint32_t C, FindGraph g, BloomView bloom, const uint32_t *__restrict__ seeds,
                                                        uint32_t k, uint32_t max_haps, uint32_t *__restrict__ scratch, uint8_t *__restrict__ best_rows,
                                                        uint32_t *__restrict__ best_count, uint32_t *__restrict__ overflow) {
    const uint32_t c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    const FindCluster fc = clusters[c];
    find_paths_cluster<LaneTeam>(fc, seeds[c], g, bloom, k, max_haps, scratch, best_rows, best_count + c, overflow, nullptr);
}

__global__ __launch_bounds__(64) void find_paths_wave_kernel(const FindCluster *__restrict__ clusters, FindGraph g, BloomView bloom, const uint32_t *__restrict__ seeds, uint32_t k,
                                                             uint32_t max_haps, uint32_t *__restrict__ scratch, uint8_t *__restrict__ best_rows, uint32_t *__restrict__ best_count,
                                                             uint32_t *__restrict__ overflow, uint32_t *__restrict__ max_candidates) {
    const uint32_t c = blockIdx.x;
    const FindCluster fc = clusters[c];
    find_paths_cluster<WaveTeam>(fc, seeds[c], g, bloom, k, max_haps, scratch, best_rows, best_count + c, overflow, max_candidates);
}

// ---- a batch of n samples (bt_find_paths_samples): every sample's search at once, then one fold per cluster over the samples in order ----
// Sample j searches in its own copy of the scratch allocation: copy 0 is `scratch`, copy j > 0 lies at extra + (j - 1) * copy_words.
__device__ __forceinline__ uint32_t *scratch_copy(uint32_t *scratch, uint32_t *extra, uint64_t copy_words, uint32_t j) {
    return j == 0 ? scratch : extra + (uint64_t)(j - 1) * copy_words;
}

// one lane per (sample blockIdx.y, cluster); C: clusters of this launch, stride: clusters of the batch (seeds and ncur are [n * stride])
__global__ __launch_bounds__(64) void find_paths_search_kernel(const FindCluster *__restrict__ clusters, uint32_t C, uint32_t stride, FindGraph g, const BloomView *__restrict__ blooms,
                                                               const uint32_t *__restrict__ seeds, uint32_t k, uint32_t max_haps, uint32_t *__restrict__ scratch,
                                                               uint32_t *__restrict__ extra, uint64_t copy_words, uint32_t *__restrict__ ncur_out, uint32_t *__restrict__ overflow) {
    const uint32_t c = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y;
    if (c >= C) return;
    const FindCluster fc = clusters[c];
    Work w = open_work<LaneTeam>(fc, g, blooms[j], k, max_haps, scratch_copy(scratch, extra, copy_words, j) + fc.scratch, overflow);
    uint32_t max_cand = 0;
    ncur_out[(size_t)j * stride + c] = search_cluster<LaneTeam>(w, fc, seeds[(size_t)j * stride + c], max_cand);
}

// one wavefront per (cluster blockIdx.x / n, sample blockIdx.x % n): the clusters are sorted by descending vertex count, so the longest searches of all samples start first
__global__ __launch_bounds__(64) void find_paths_search_wave_kernel(const FindCluster *__restrict__ clusters, uint32_t n, uint32_t stride, FindGraph g, const BloomView *__restrict__ blooms,
                                                                    const uint32_t *__restrict__ seeds, uint32_t k, uint32_t max_haps, uint32_t *__restrict__ scratch,
                                                                    uint32_t *__restrict__ extra, uint64_t copy_words, uint32_t *__restrict__ ncur_out, uint32_t *__restrict__ overflow,
                                                                    uint32_t *__restrict__ max_candidates) {
    const uint32_t c = blockIdx.x / n, j = blockIdx.x % n;
    const FindCluster fc = clusters[c];
    Work w = open_work<WaveTeam>(fc, g, blooms[j], k, max_haps, scratch_copy(scratch, extra, copy_words, j) + fc.scratch, overflow);
    uint32_t max_cand = 0;
    const uint32_t ncur = search_cluster<WaveTeam>(w, fc, seeds[(size_t)j * stride + c], max_cand);
    if (threadIdx.x == 0) {
        ncur_out[(size_t)j * stride + c] = ncur;
        atomicMax(max_candidates, max_cand);
    }
}

// the fold of cluster c by team T: the final paths of copy 0, 1, .. n-1 in that order into the cluster's rows (the order of the samples is the order of the rows)
template <class T>
__device__ __forceinline__ void fold_samples(const FindCluster &fc, uint32_t n, uint32_t stride, const FindGraph &g, uint32_t k, uint32_t max_haps, uint32_t *scratch, uint32_t *extra,
                                             uint64_t copy_words, const uint32_t *ncur_in, uint8_t *best_rows, uint32_t *best_count, uint32_t *overflow) {
    for (uint32_t j = 0; j < n; ++j) {
        Work w = open_work<T>(fc, g, BloomView{}, k, max_haps, scratch_copy(scratch, extra, copy_words, j) + fc.scratch, overflow);
        const uint32_t ncur = T::uni(ncur_in[(size_t)j * stride]);
        fold_cluster<T>(w, fc, ncur < fc.cur_cap ? ncur : fc.cur_cap, best_rows, best_count);
        T::sync();   // (the next sample reads the rows and the count this one wrote)
    }
}

__global__ __launch_bounds__(64) void find_paths_fold_kernel(const FindCluster *__restrict__ clusters, uint32_t C, uint32_t n, uint32_t stride, FindGraph g, uint32_t k, uint32_t max_haps,
                                                             uint32_t *__restrict__ scratch, uint32_t *__restrict__ extra, uint64_t copy_words, const uint32_t *__restrict__ ncur_in,
                                                             uint8_t *__restrict__ best_rows, uint32_t *__restrict__ best_count, uint32_t *__restrict__ overflow) {
    const uint32_t c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    const FindCluster fc = clusters[c];
    fold_samples<LaneTeam>(fc, n, stride, g, k, max_haps, scratch, extra, copy_words, ncur_in + c, best_rows, best_count + c, overflow);
}

__global__ __launch_bounds__(64) void find_paths_fold_wave_kernel(const FindCluster *__restrict__ clusters, uint32_t n, uint32_t stride, FindGraph g, uint32_t k, uint32_t max_haps,
                                                                  uint32_t *__restrict__ scratch, uint32_t *__restrict__ extra, uint64_t copy_words, const uint32_t *__restrict__ ncur_in,
                                                                  uint8_t *__restrict__ best_rows, uint32_t *__restrict__ best_count, uint32_t *__restrict__ overflow) {
    const uint32_t c = blockIdx.x;
    const FindCluster fc = clusters[c];
    fold_samples<WaveTeam>(fc, n, stride, g, k, max_haps, scratch, extra, copy_words, ncur_in + c, best_rows, best_count + c, overflow);
}

}  // namespace

struct bt_find_paths {
    bt_ctx *ctx = nullptr;
    uint32_t k = 0, C = 0, max_haps = 0;
    std::vector<FindCluster> clusters;
    std::vector<uint32_t> nv;
    FindGraph g{};
    FindCluster *d_clusters = nullptr;
    uint32_t *d_scratch = nullptr, *d_best_count = nullptr, *d_overflow = nullptr, *d_seeds = nullptr;
    uint8_t *d_best = nullptr;
    uint64_t best_bytes = 0;
    std::vector<void *> owned;
    // Clusters of at least wave_min vertices (BT_FIND_PATHS_WAVE_MIN) run on a wavefront each.  The device arrays (clusters, seeds, best counts) are in LAUNCH
    // order: the other clusters first, in batch order — find_paths_kernel runs over that prefix unchanged —, then the wide ones by descending vertex count.
    // No wide cluster: launch order is batch order and `order` stays empty.
    uint32_t wave_min = 0, num_wave = 0, max_nv = 0;
    std::vector<uint32_t> order;         // launch position -> cluster of the batch
    std::vector<uint32_t> staged;        // seeds / counts in launch order
    uint32_t *d_max_candidates = nullptr;   // (second word of the overflow allocation)
    hipEvent_t ev_seeds = nullptr, ev_wave = nullptr;
    // bt_find_paths_samples: what a batch of batch_cap samples needs beyond the above, one allocation (batch_layout), made on the first call with n >= 2 and
    // replaced only by a call with a larger n
    uint64_t scratch_words = 0;          // one copy of the scratch allocation
    uint32_t batch_cap = 0, batch_max_n = 0;   // samples the allocation holds; largest n a call has had
    uint8_t *d_batch = nullptr;
    std::vector<uint32_t> staged_batch;  // seeds [n * C] in launch order
    std::vector<BloomView> views;
};

// the batch allocation for n >= 2 samples: byte offsets of its parts (each a multiple of 256) and its size
struct BatchLayout {
    uint64_t extra, ncur, seeds, blooms, total;
};
static BatchLayout batch_layout(const bt_find_paths *f, uint32_t n) {
    auto up256 = [](uint64_t x) { return (x + 255) & ~255ull; };
    BatchLayout l{};
    if (n < 2) return l;
    l.extra = 0;
    l.ncur = up256((uint64_t)(n - 1) * f->scratch_words * 4);
    l.seeds = l.ncur + up256((uint64_t)n * f->C * 4);
    l.blooms = l.seeds + up256((uint64_t)n * f->C * 4);
    l.total = l.blooms + up256((uint64_t)n * sizeof(BloomView));
    return l;
}

// the stream of the wide clusters' launches: the class stream when the context has one that PROVED concurrent with its own and there are lane clusters beside
// them, else the context's stream
static int wave_stream(bt_find_paths *f, uint32_t lanes, hipStream_t *out) {
    *out = f->ctx->stream;
    if (!lanes) return BT_OK;
    int prio_lo = 0, prio_hi = 0;
    BT_HIP(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
    hipStream_t cs[1] = {nullptr};
    BT_HIP(ctx_class_streams(f->ctx, 1, getenv("BT_GIBBS_NO_PRIO") ? prio_lo : prio_hi, cs));   // (the priority the samplers ask for: one probe per context)
    if (f->ctx->class_streams_concurrent >= 1) *out = cs[0];
    return BT_OK;
}

// best_count by cluster of the batch (the device keeps it in launch order)
static hipError_t fetch_counts(bt_find_paths *f, uint32_t *out) {
    if (f->order.empty()) return hipMemcpy(out, f->d_best_count, (size_t)f->C * 4, hipMemcpyDeviceToHost);
    const hipError_t e = hipMemcpy(f->staged.data(), f->d_best_count, (size_t)f->C * 4, hipMemcpyDeviceToHost);
    for (uint32_t i = 0; i < f->C; ++i) out[f->order[i]] = f->staged[i];
    return e;
}

extern "C" {

int bt_find_paths_create(bt_ctx *ctx, const bt_paths_batch *b, uint32_t k, uint32_t max_sample_haplotypes, uint32_t num_samples, bt_find_paths **out) {
    if (!ctx || !b || !out) return fail("bt_find_paths_create: null argument");
    if (!b->in_off || !b->in_src) return fail("bt_find_paths_create: the batch carries no edges (in_off / in_src)");
    if (k < 1 || k > 64) return fail("bt_find_paths_create: k must be in 1..64");
    if (max_sample_haplotypes < 1 || num_samples < 1) return fail("bt_find_paths_create: max_sample_haplotypes and num_samples must be positive");
    BT_HIP(hipSetDevice(ctx->device));
    bt_find_paths *f = new bt_find_paths();
    f->ctx = ctx;
    f->k = k;
    f->C = b->num_clusters;
    f->max_haps = max_sample_haplotypes;
    const uint32_t C = f->C, NV = b->vertex_off[C];
    std::vector<uint32_t> last_use(NV);
    uint64_t scratch_words = 0, best_bytes = 0;
    if (const char *e = getenv("BT_FIND_PATHS_WAVE_MIN")) f->wave_min = (uint32_t)std::strtoul(e, nullptr, 10);
    else f->wave_min = WAVE_MIN_DEFAULT;
    for (uint32_t c = 0; c < C; ++c) {
        const uint32_t v0 = b->vertex_off[c], nv = b->vertex_off[c + 1] - v0;
        if (nv == 0 || nv >= (1u << 24)) {
            delete f;
            return fail("bt_find_paths_create: a cluster needs between 1 and 2^24 - 1 vertices");
        }
        uint32_t max_indeg = 1;
        for (uint32_t vi = 0; vi < nv; ++vi) last_use[v0 + vi] = vi;
        for (uint32_t vi = 0; vi < nv; ++vi) {
            const uint32_t e0 = b->in_off[v0 + vi], e1 = b->in_off[v0 + vi + 1];
            max_indeg = std::max(max_indeg, e1 - e0);
            for (uint32_t e = e0; e < e1; ++e) {
                if (b->in_src[e] >= vi) {
                    delete f;
                    return fail("bt_find_paths_create: edges must point from lower to higher vertex indices");
                }
                last_use[v0 + b->in_src[e]] = std::max(last_use[v0 + b->in_src[e]], vi);
            }
        }
        // vertices whose path lists are alive at the same time: the list of u lives from the step of u to the step of its last successor
        uint32_t live_max = 1;
        {
            std::vector<int32_t> delta(nv + 1, 0);
            for (uint32_t vi = 0; vi < nv; ++vi) {
                delta[vi] += 1;
                delta[last_use[v0 + vi] + 1] -= 1;
            }
            int32_t live = 0;
            for (uint32_t vi = 0; vi < nv; ++vi) {
                live += delta[vi];
                live_max = std::max<uint32_t>(live_max, (uint32_t)live);
            }
        }
        FindCluster fc{};
        fc.v0 = v0;
        fc.nv = nv;
        fc.cur_cap = max_indeg * max_sample_haplotypes + 1;
        fc.cap_slots = (live_max + max_indeg + 1) * max_sample_haplotypes + 1;
        fc.slot_words = HDR_WORDS + nv;
        fc.best_cap = max_sample_haplotypes * num_samples;
        fc.scratch = scratch_words;
        fc.best = best_bytes;
        const bool wave = f->wave_min && nv >= f->wave_min;
        scratch_words += scratch_layout(fc, max_sample_haplotypes, wave).total;
        f->max_nv = std::max(f->max_nv, nv);
        if (wave) f->num_wave++;
        best_bytes += (uint64_t)fc.best_cap * nv;
        f->clusters.push_back(fc);
        f->nv.push_back(nv);
    }
    f->best_bytes = best_bytes;
    f->scratch_words = scratch_words;
    std::vector<FindCluster> launch_order;
    if (f->num_wave) {
        std::vector<uint32_t> wide;
        for (uint32_t c = 0; c < C; ++c) (f->nv[c] >= f->wave_min ? wide : f->order).push_back(c);
        std::stable_sort(wide.begin(), wide.end(), [&](uint32_t a, uint32_t b) { return f->nv[a] > f->nv[b]; });   // the longest starts first
        f->order.insert(f->order.end(), wide.begin(), wide.end());
        for (uint32_t c : f->order) launch_order.push_back(f->clusters[c]);
        f->staged.resize(C);
    }
    int rc = BT_OK;
    auto up = [&](auto **dst, const auto *src, uint64_t n) {
        if (rc != BT_OK) return;
        using T = std::remove_cv_t<std::remove_pointer_t<std::remove_pointer_t<decltype(dst)>>>;
        T *p = nullptr;
        if (hipMalloc(reinterpret_cast<void **>(&p), std::max<uint64_t>(n, 1) * sizeof(T)) != hipSuccess) {
            rc = fail("bt_find_paths_create: device allocation failed");
            return;
        }
        f->owned.push_back(p);
        if (src && n && hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) rc = fail("bt_find_paths_create: upload failed");
        *dst = p;
    };
    uint64_t *d_seq_off = nullptr;
    uint8_t *d_seq = nullptr, *d_vflags = nullptr;
    uint32_t *d_in_off = nullptr, *d_in_src = nullptr, *d_last = nullptr;
    up(&d_seq_off, b->seq_off, (uint64_t)NV + 1);
    up(&d_seq, b->seq, b->seq_off[NV]);
    up(&d_vflags, b->vertex_flags, NV);
    up(&d_in_off, b->in_off, (uint64_t)NV + 1);
    up(&d_in_src, b->in_src, b->in_off[NV]);
    up(&d_last, last_use.data(), NV);
    up(&f->d_clusters, f->num_wave ? launch_order.data() : f->clusters.data(), C);
    up(&f->d_scratch, (const uint32_t *)nullptr, scratch_words);
    up(&f->d_best, (const uint8_t *)nullptr, best_bytes);
    up(&f->d_best_count, (const uint32_t *)nullptr, C);
    up(&f->d_overflow, (const uint32_t *)nullptr, f->num_wave ? 2 : 1);
    up(&f->d_seeds, (const uint32_t *)nullptr, C);
    if (rc == BT_OK && (hipMemset(f->d_best_count, 0, (size_t)C * 4) != hipSuccess || hipMemset(f->d_overflow, 0, f->num_wave ? 8 : 4) != hipSuccess)) rc = fail("bt_find_paths_create: memset failed");
    if (rc == BT_OK && f->num_wave) {
        f->d_max_candidates = f->d_overflow + 1;
        if (hipEventCreateWithFlags(&f->ev_seeds, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&f->ev_wave, hipEventDisableTiming) != hipSuccess)
            rc = fail("bt_find_paths_create: event creation failed");
    }
    if (rc != BT_OK) {
        bt_find_paths_destroy(f);
        return rc;
    }
    f->g = FindGraph{d_seq_off, d_seq, d_vflags, d_in_off, d_in_src, d_last};
    *out = f;
    return BT_OK;
}

int bt_find_paths_destroy(bt_find_paths *f) {
    if (!f) return BT_OK;
    (void)hipSetDevice(f->ctx->device);
    (void)hipStreamSynchronize(f->ctx->stream);
    for (void *q : f->owned) (void)hipFree(q);
    if (f->d_batch) (void)hipFree(f->d_batch);
    if (f->ev_seeds) (void)hipEventDestroy(f->ev_seeds);
    if (f->ev_wave) (void)hipEventDestroy(f->ev_wave);
    delete f;
    return BT_OK;
}

int bt_find_paths_sample(bt_find_paths *f, bt_bloom *sample_bloom, const uint32_t *h_seeds) {
    if (!f || !sample_bloom || !h_seeds) return fail("bt_find_paths_sample: null argument");
    if (sample_bloom->k != f->k) return fail("bt_find_paths_sample: k mismatch");
    BT_HIP(hipSetDevice(f->ctx->device));
    hipStream_t st = f->ctx->stream;
    if (f->num_wave == 0) {
        BT_HIP(hipMemcpyAsync(f->d_seeds, h_seeds, (size_t)f->C * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(find_paths_kernel, dim3((f->C + 63) / 64), dim3(64), 0, st, f->d_clusters, f->C, f->g, sample_bloom->view(), f->d_seeds, f->k, f->max_haps,
                           f->d_scratch, f->d_best, f->d_best_count, f->d_overflow);
        BT_CHECK_LAUNCH();
    } else {
        // the wide clusters on a wavefront each, beside the lane kernel when the context has a stream that PROVED concurrent with its own, else before it
        const uint32_t lanes = f->C - f->num_wave;
        hipStream_t wave_st = st;
        if (wave_stream(f, lanes, &wave_st) != BT_OK) return BT_ERR;
        for (uint32_t i = 0; i < f->C; ++i) f->staged[i] = h_seeds[f->order[i]];
        BT_HIP(hipMemcpyAsync(f->d_seeds, f->staged.data(), (size_t)f->C * 4, hipMemcpyHostToDevice, st));
        if (wave_st != st) {
            BT_HIP(hipEventRecord(f->ev_seeds, st));
            BT_HIP(hipStreamWaitEvent(wave_st, f->ev_seeds, 0));
        }
        hipLaunchKernelGGL(find_paths_wave_kernel, dim3(f->num_wave), dim3(64), 0, wave_st, f->d_clusters + lanes, f->g, sample_bloom->view(), f->d_seeds + lanes, f->k,
                           f->max_haps, f->d_scratch, f->d_best, f->d_best_count + lanes, f->d_overflow, f->d_max_candidates);
        BT_CHECK_LAUNCH();
        if (lanes) {
            hipLaunchKernelGGL(find_paths_kernel, dim3((lanes + 63) / 64), dim3(64), 0, st, f->d_clusters, lanes, f->g, sample_bloom->view(), f->d_seeds, f->k, f->max_haps,
                               f->d_scratch, f->d_best, f->d_best_count, f->d_overflow);
            BT_CHECK_LAUNCH();
        }
        if (wave_st != st) {   // both launches are joined before the flag is read
            BT_HIP(hipEventRecord(f->ev_wave, wave_st));
            BT_HIP(hipStreamWaitEvent(st, f->ev_wave, 0));
        }
    }
    uint32_t ov = 0;
    BT_HIP(hipMemcpyAsync(&ov, f->d_overflow, 4, hipMemcpyDeviceToHost, st));
    BT_HIP(hipStreamSynchronize(st));
    if (ov == 1) return fail("bt_find_paths_sample: path scratch exhausted (internal sizing error)");
    if (ov == 2) return fail("bt_find_paths_sample: more best paths than max_sample_haplotypes x num_samples");
    return BT_OK;
}

int bt_find_paths_batch_bytes(bt_find_paths *f, uint32_t n, uint64_t *bytes) {
    if (!f || !bytes) return fail("bt_find_paths_batch_bytes: null argument");
    if (n == 0) return fail("bt_find_paths_batch_bytes: n must be positive");
    *bytes = n <= f->batch_cap ? 0 : batch_layout(f, n).total - batch_layout(f, f->batch_cap).total;
    return BT_OK;
}

int bt_find_paths_batch_info(bt_find_paths *f, uint32_t *largest_n, uint64_t *held_bytes) {
    if (!f) return fail("bt_find_paths_batch_info: null argument");
    if (largest_n) *largest_n = f->batch_max_n;
    if (held_bytes) *held_bytes = batch_layout(f, f->batch_cap).total;
    return BT_OK;
}

int bt_find_paths_samples(bt_find_paths *f, bt_bloom *const *sample_blooms, uint32_t n, const uint32_t *h_seeds) {
    if (!f || !sample_blooms || !h_seeds) return fail("bt_find_paths_samples: null argument");
    if (n == 0) return fail("bt_find_paths_samples: n must be positive");
    if (n > 65535) return fail("bt_find_paths_samples: at most 65535 samples per call");
    for (uint32_t j = 0; j < n; ++j) {
        if (!sample_blooms[j]) return fail("bt_find_paths_samples: null filter in the array");
        if (sample_blooms[j]->k != f->k) return fail("bt_find_paths_samples: k mismatch");
        if (sample_blooms[j]->ctx && sample_blooms[j]->ctx->device != f->ctx->device) return fail("bt_find_paths_samples: a filter lives on another device");
    }
    f->batch_max_n = std::max(f->batch_max_n, n);
    if (n == 1) return bt_find_paths_sample(f, sample_blooms[0], h_seeds);
    BT_HIP(hipSetDevice(f->ctx->device));
    hipStream_t st = f->ctx->stream;
    const uint32_t C = f->C;
    if (n > f->batch_cap) {   // (nothing of an earlier call is in flight: every call ends with a synchronize)
        if (f->d_batch) BT_HIP(hipFree(f->d_batch));
        f->d_batch = nullptr;
        f->batch_cap = 0;
        void *p = nullptr;
        if (hipMalloc(&p, batch_layout(f, n).total) != hipSuccess) {
            (void)hipGetLastError();
            return fail("bt_find_paths_samples: device allocation of " + std::to_string(batch_layout(f, n).total) + " bytes for " + std::to_string(n) + " samples failed");
        }
        f->d_batch = static_cast<uint8_t *>(p);
        f->batch_cap = n;
    }
    const BatchLayout l = batch_layout(f, f->batch_cap);
    uint32_t *d_extra = reinterpret_cast<uint32_t *>(f->d_batch + l.extra), *d_ncur = reinterpret_cast<uint32_t *>(f->d_batch + l.ncur);
    uint32_t *d_seeds = reinterpret_cast<uint32_t *>(f->d_batch + l.seeds);
    BloomView *d_blooms = reinterpret_cast<BloomView *>(f->d_batch + l.blooms);
    f->views.resize(n);
    for (uint32_t j = 0; j < n; ++j) f->views[j] = sample_blooms[j]->view();
    const uint32_t *seeds = h_seeds;
    if (f->num_wave) {
        f->staged_batch.resize((size_t)n * C);
        for (uint32_t j = 0; j < n; ++j)
            for (uint32_t i = 0; i < C; ++i) f->staged_batch[(size_t)j * C + i] = h_seeds[(size_t)j * C + f->order[i]];
        seeds = f->staged_batch.data();
    }
    BT_HIP(hipMemcpyAsync(d_seeds, seeds, (size_t)n * C * 4, hipMemcpyHostToDevice, st));
    BT_HIP(hipMemcpyAsync(d_blooms, f->views.data(), (size_t)n * sizeof(BloomView), hipMemcpyHostToDevice, st));
    // the routes of bt_find_paths_sample: the wide clusters' search and fold in stream order on their stream, the others' on the context's, joined at the end
    const uint32_t lanes = C - f->num_wave;
    hipStream_t wave_st = st;
    if (f->num_wave) {
        if (wave_stream(f, lanes, &wave_st) != BT_OK) return BT_ERR;
        if (wave_st != st) {
            BT_HIP(hipEventRecord(f->ev_seeds, st));
            BT_HIP(hipStreamWaitEvent(wave_st, f->ev_seeds, 0));
        }
        hipLaunchKernelGGL(find_paths_search_wave_kernel, dim3(f->num_wave * n), dim3(64), 0, wave_st, f->d_clusters + lanes, n, C, f->g, d_blooms, d_seeds + lanes, f->k, f->max_haps,
                           f->d_scratch, d_extra, f->scratch_words, d_ncur + lanes, f->d_overflow, f->d_max_candidates);
        BT_CHECK_LAUNCH();
        hipLaunchKernelGGL(find_paths_fold_wave_kernel, dim3(f->num_wave), dim3(64), 0, wave_st, f->d_clusters + lanes, n, C, f->g, f->k, f->max_haps, f->d_scratch, d_extra,
                           f->scratch_words, d_ncur + lanes, f->d_best, f->d_best_count + lanes, f->d_overflow);
        BT_CHECK_LAUNCH();
    }
    if (lanes) {
        hipLaunchKernelGGL(find_paths_search_kernel, dim3((lanes + 63) / 64, n), dim3(64), 0, st, f->d_clusters, lanes, C, f->g, d_blooms, d_seeds, f->k, f->max_haps, f->d_scratch,
                           d_extra, f->scratch_words, d_ncur, f->d_overflow);
        BT_CHECK_LAUNCH();
        hipLaunchKernelGGL(find_paths_fold_kernel, dim3((lanes + 63) / 64), dim3(64), 0, st, f->d_clusters, lanes, n, C, f->g, f->k, f->max_haps, f->d_scratch, d_extra,
                           f->scratch_words, d_ncur, f->d_best, f->d_best_count, f->d_overflow);
        BT_CHECK_LAUNCH();
    }
    if (wave_st != st) {
        BT_HIP(hipEventRecord(f->ev_wave, wave_st));
        BT_HIP(hipStreamWaitEvent(st, f->ev_wave, 0));
    }
    uint32_t ov = 0;
    BT_HIP(hipMemcpyAsync(&ov, f->d_overflow, 4, hipMemcpyDeviceToHost, st));
    BT_HIP(hipStreamSynchronize(st));
    if (ov == 1) return fail("bt_find_paths_samples: path scratch exhausted (internal sizing error)");
    if (ov == 2) return fail("bt_find_paths_samples: more best paths than max_sample_haplotypes x num_samples");
    return BT_OK;
}

int bt_find_paths_info(bt_find_paths *f, bt_find_paths_stats *out) {
    if (!f || !out) return fail("bt_find_paths_info: null argument");
    BT_HIP(hipSetDevice(f->ctx->device));
    out->num_clusters = f->C;
    out->num_wave_clusters = f->num_wave;
    out->wave_min_vertices = f->wave_min;
    out->max_vertices = f->max_nv;
    out->max_candidate_paths = 0;
    if (f->num_wave) {
        BT_HIP(hipStreamSynchronize(f->ctx->stream));
        BT_HIP(hipMemcpy(&out->max_candidate_paths, f->d_max_candidates, 4, hipMemcpyDeviceToHost));
    }
    return BT_OK;
}

int bt_find_paths_sizes(bt_find_paths *f, uint32_t *h_num_paths, uint64_t *h_total_bytes) {
    if (!f || !h_num_paths) return fail("bt_find_paths_sizes: null argument");
    BT_HIP(hipSetDevice(f->ctx->device));
    BT_HIP(hipStreamSynchronize(f->ctx->stream));
    BT_HIP(fetch_counts(f, h_num_paths));
    uint64_t total = 0;
    for (uint32_t c = 0; c < f->C; ++c) total += (uint64_t)h_num_paths[c] * f->nv[c];
    if (h_total_bytes) *h_total_bytes = total;
    return BT_OK;
}

int bt_find_paths_fetch(bt_find_paths *f, uint8_t *h_path_vertices) {
    if (!f || !h_path_vertices) return fail("bt_find_paths_fetch: null argument");
    BT_HIP(hipSetDevice(f->ctx->device));
    BT_HIP(hipStreamSynchronize(f->ctx->stream));
    std::vector<uint32_t> n(f->C);
    BT_HIP(fetch_counts(f, n.data()));
    std::vector<uint8_t> all(f->best_bytes);
    if (f->best_bytes) BT_HIP(hipMemcpy(all.data(), f->d_best, f->best_bytes, hipMemcpyDeviceToHost));
    uint8_t *o = h_path_vertices;
    for (uint32_t c = 0; c < f->C; ++c) {
        const uint64_t bytes = (uint64_t)n[c] * f->nv[c];
        if (bytes) std::memcpy(o, all.data() + f->clusters[c].best, bytes);
        o += bytes;
    }
    return BT_OK;
}

}  // extern "C"
