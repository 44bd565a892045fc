/*
 * btgpu.h — C ABI of libbtgpu.so: the MI355X (gfx950) implementation of BayesTyper's
 * k-mer matching + per-cluster Gibbs genotyping hot path.
 *
 * The reference (BayesTyper v1.5, C++11) has no FFI; the seams below are cut at the
 * narrowest points of its own class structure.  Every entry point cites
 * the reference interface it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - plain C, opaque handles, no exceptions cross the boundary;
 *   - every call returns int: 0 = ok, non-zero = error, text via bt_last_error();
 *   - pointers named d_* are DEVICE pointers (hipMalloc / bt_malloc / a torch tensor's
 *     data_ptr); everything else is host memory owned by the caller;
 *   - batch calls are asynchronous on the context's stream; bt_sync() waits;
 *   - handles are not thread-safe, distinct handles are; one bt_ctx per GPU;
 *   - k-mers are passed 2-bit packed in two uint64 words {lo, hi}: nucleotide i sits in
 *     bits (2i, 2i+1) of the 128-bit value, A=0 C=1 G=2 T=3 — the bit layout of the
 *     reference's std::bitset<2k> (include/bayesTyper/Nucleotide.hpp:40-70).
 *     k <= 64.  Unless stated otherwise k-mers must already be canonical
 *     (include/bayesTyper/Kmer.tpp:225-255).
 */
#ifndef BTGPU_H
#define BTGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BT_OK 0
#define BT_ERR 1

/* ------------------------------------------------------------------------------------------
 * Context, memory, timing
 * ---------------------------------------------------------------------------------------- */
typedef struct bt_ctx bt_ctx;

/* last error message of the calling thread ("" if none) */
const char *bt_last_error(void);
/* library/ABI version, e.g. 100 = 1.0.0 */
int bt_version(void);
/* number of visible HIP devices (0 and BT_OK when there is none) */
int bt_device_count(int *count);

/* one context = one GPU + one stream (replaces the reference's `-p` thread pool for this path:
 * src/bayesTyper/main.cpp:128,214,467) */
int bt_ctx_create(int device_id, bt_ctx **out);
/* a second context on the same GPU with a stream of its own: work a helper thread enqueues (the next noise chain's sampler construction,
 * InferenceEngine.cpp:191-211 constructs a chain's genotypers while nothing else runs; here it overlaps the previous chain) does not queue behind
 * the first context's stream.  Handles created on either context live in the same device memory. */
int bt_ctx_clone(bt_ctx *ctx, bt_ctx **out);
int bt_ctx_destroy(bt_ctx *ctx);
/* run all subsequent work of this context on an externally owned hipStream_t (e.g. torch's
 * current stream); NULL restores the context's own stream */
int bt_ctx_set_stream(bt_ctx *ctx, void *hip_stream);
/* run all subsequent work on the device's default (null) stream — what torch.cuda.current_stream() is unless the
 * caller switched streams; the default stream's handle is 0, which bt_ctx_set_stream reads as "own stream" */
int bt_ctx_use_default_stream(bt_ctx *ctx);
int bt_sync(bt_ctx *ctx);
/* device properties: compute units, total/free HBM bytes, gcn arch name (buffer >= 64 bytes) */
int bt_ctx_info(bt_ctx *ctx, int *num_cu, uint64_t *hbm_total, uint64_t *hbm_free, char *arch, size_t arch_len);

int bt_malloc(bt_ctx *ctx, size_t bytes, void **d_out);
int bt_free(bt_ctx *ctx, void *d_ptr);
int bt_memset(bt_ctx *ctx, void *d_ptr, int value, size_t bytes);
int bt_memcpy_h2d(bt_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int bt_memcpy_d2h(bt_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
int bt_memcpy_d2d(bt_ctx *ctx, void *d_dst, const void *d_src, size_t bytes);

/* HIP-event timing on the context's stream (bench.py's roofline leg) */
typedef struct bt_timer bt_timer;
int bt_timer_create(bt_ctx *ctx, bt_timer **out);
int bt_timer_destroy(bt_timer *t);
int bt_timer_start(bt_timer *t);
int bt_timer_stop(bt_timer *t);
/* waits for the stop event; milliseconds between start and stop */
int bt_timer_elapsed_ms(bt_timer *t, float *ms);

/* ------------------------------------------------------------------------------------------
 * k-mer packing / canonical form
 *   mirrors KmerPair<k>::move + getLexicographicalLowestKmer
 *   (include/bayesTyper/Kmer.tpp:44-81,116-153,182-255) and Nucleotide::ntToBit
 *   (include/bayesTyper/Nucleotide.hpp:40-70)
 * ---------------------------------------------------------------------------------------- */
/* For every position i of the ASCII sequence d_seq[0..len): if the k characters ending at i are
 * all in ACGTacgt, write the canonical k-mer of seq[i-k+1..i] to d_kmers[2*i..2*i+1] and 1 to
 * d_valid[i]; else d_valid[i] = 0 (the k-mer window "resets" on any other character, exactly
 * as KmerPair::move does). */
int bt_kmers_from_sequence(bt_ctx *ctx, const char *d_seq, uint64_t len, uint32_t k,
                           uint64_t *d_kmers, uint8_t *d_valid);

/* ------------------------------------------------------------------------------------------
 * ntHash (external/ntHash/nthash.hpp:262-267 NTP64(kmer,k); :275-282 NTP64(kmer,k,seed))
 * ---------------------------------------------------------------------------------------- */
/* d_hash[i] = NTP64(kmer_i, k); if seeded != 0: NTP64(kmer_i, k, seed) */
int bt_nthash_batch(bt_ctx *ctx, const uint64_t *d_kmers, uint64_t n, uint32_t k,
                    int seeded, uint32_t seed, uint64_t *d_hash);

/* ------------------------------------------------------------------------------------------
 * Bloom filters: KmerBloom<k> and ThreadedKmerBloom<k>
 *   include/kmerBloom/KmerBloom.hpp:48-108, src/kmerBloom/KmerBloom.cpp:54-286,
 *   external/ntHash/BloomFilter.hpp:40-66,149-161,260-264
 * ---------------------------------------------------------------------------------------- */
typedef struct bt_bloom bt_bloom;

/* KmerBloom<k>(num_kmers, fpr)               threaded == 0   (KmerBloom.cpp:54-60)
 * ThreadedKmerBloom<k>(num_kmers, fpr)       threaded != 0   (KmerBloom.cpp:204-215): 65 536
 * sub-filters each sized for ceil(num_kmers / 65536.0f) k-mers, routed by
 * NTP64(kmer,k,1029283129) % 65536 (KmerBloom.cpp:277-280). */
int bt_bloom_create(bt_ctx *ctx, uint64_t num_kmers, float fpr, uint32_t k, int threaded, bt_bloom **out);
/* KmerBloom<k>(prefix): reads <prefix>.bloomMeta / <prefix>.bloomData (KmerBloom.cpp:63-89).
 * Fails (like the reference's assert) when the stored k differs. */
int bt_bloom_load(bt_ctx *ctx, const char *prefix, uint32_t k, bt_bloom **out);
/* KmerBloom::save (KmerBloom.cpp:149-164); byte-identical files. Single filters only
 * (the reference's ThreadedKmerBloom::save is commented out, KmerBloom.hpp:100). */
int bt_bloom_save(bt_bloom *b, const char *prefix);
int bt_bloom_destroy(bt_bloom *b);
/* sizing as computed by calcOptNumBloomBits / calcOptNumHashes (KmerBloom.cpp:134-146);
 * for a threaded filter num_kmers/num_bits are per sub-filter */
int bt_bloom_info(bt_bloom *b, uint64_t *num_kmers, uint64_t *num_bits, uint32_t *num_hashes,
                  uint32_t *num_sub_filters, uint64_t *device_bytes);
/* addKmer for a batch (BloomFilter::insertF, BloomFilter.hpp:56-66) */
int bt_bloom_insert_batch(bt_bloom *b, const uint64_t *d_kmers, uint64_t n);
/* lookup for a batch (BloomFilter::containsF, BloomFilter.hpp:149-161): d_hits[i] = 0/1 */
int bt_bloom_contains_batch(bt_bloom *b, const uint64_t *d_kmers, uint64_t n, uint8_t *d_hits);
/* raw bit image of sub-filter `sub` (0 for a single filter) as the reference stores it:
 * (num_bits+7)/8 bytes, bit b at byte b/8, mask 1<<(7-b%8) */
int bt_bloom_read_bits(bt_bloom *b, uint32_t sub, uint8_t *h_out, uint64_t nbytes);
int bt_bloom_clear(bt_bloom *b);

/* ------------------------------------------------------------------------------------------
 * k-mer count table: KmerCountsHash / ObservedKmerCountsHash<N> + KmerCounts
 *   include/bayesTyper/KmerHash.hpp:73-87, include/bayesTyper/KmerCounts.hpp:35-101,
 *   src/bayesTyper/KmerCounts.cpp:40-223.  Per-key contents equal the reference's; the
 *   iteration order is free (open addressing in HBM instead of HybridHash's 16.7 M leaves).
 * ---------------------------------------------------------------------------------------- */
typedef struct bt_table bt_table;

/* flag bits of bt_table meta byte 0 (KmerCounts.hpp:70) */
#define BT_KC_CLUSTER_OCC      0x01
#define BT_KC_MULTICLUSTER_OCC 0x02
#define BT_KC_MULTIGROUP_OCC   0x04
#define BT_KC_DECOY_OCC        0x08
#define BT_KC_MAX_MULTIPLICITY 0x10
#define BT_KC_PARAMETER        0x20

/* ObservedKmerCountsHash<N>(expected_size, threads) (src/bayesTyper/KmerHash.cpp:202-210);
 * num_samples <= 30 (src/bayesTyper/main.cpp:72).  Capacity is fixed: 2 x expected rounded
 * up to a power of two; an insert into a full table is an error reported by bt_table_status. */
int bt_table_create(bt_ctx *ctx, uint64_t expected_size, uint32_t num_samples, uint32_t k, bt_table **out);
int bt_table_destroy(bt_table *t);
/* forget every record (the capacity stays): a fresh table for the next unit (main.cpp:513 constructs one per unit) */
int bt_table_clear(bt_table *t);
/* grow to hold `expected_size` records (2 x, power of two) and move the stored records over: the reference's HybridHash
 * grows on demand (HybridHash.tpp:162); callers that know an upper bound of a stage's inserts reserve before it.
 * No-op when the table is large enough; an error when records were already dropped (overflow flag). */
int bt_table_reserve(bt_table *t, uint64_t expected_size);
/* number of stored keys, capacity, overflow flag */
int bt_table_status(bt_table *t, uint64_t *num_keys, uint64_t *capacity, int *overflowed);
/* addKmer(kmer, sorted) for a batch; optionally mark as parameter k-mer
 * (main.cpp:571-577: addKmer + isParameter(true)) */
int bt_table_insert_batch(bt_table *t, const uint64_t *d_kmers, uint64_t n, int mark_parameter);
/* findKmer for a batch: d_slots[i] = slot index or -1 */
int bt_table_find_batch(bt_table *t, const uint64_t *d_kmers, uint64_t n, int64_t *d_slots);
/* read records of slots found with bt_table_find_batch (slot -1 -> zeros):
 * h_counts[i*num_samples + s], h_meta[i*4 + {flags, max_haploid_mult, female_ic, male_ic}] */
int bt_table_read_slots(bt_table *t, const int64_t *h_slots, uint64_t n, uint8_t *h_counts, uint8_t *h_meta);
/* export every stored record (iteration order unspecified); arrays sized by bt_table_status */
int bt_table_export(bt_table *t, uint64_t *h_kmers, uint8_t *h_counts, uint8_t *h_meta, uint64_t max_records, uint64_t *num_written);
/* Merging the sample counts of tables filled by ranks that each scanned their own byte range of the samples' KMC databases
 * (KmerCounter::parseSampleKmers, KmerCounter.cpp:431-524, sharded over GPUs; a (k-mer, sample) count comes from exactly one KMC record,
 * i.e. from one rank).  A count row = 16 key bytes (lo, hi) + *row_bytes - 16 count bytes (the samples' counts, padded to 4).
 * bt_table_export_count_rows: every record with a non-zero sample count -> d_rows (device, capacity_rows rows; *h_num_rows = number of
 * such records, an error if it exceeds the capacity — call with capacity 0 and d_rows NULL to size the buffer).
 * bt_table_merge_count_rows: addKmer + saturating addSampleCount of every sample for each row (rows of OTHER ranks). */
int bt_table_count_row_bytes(bt_table *t, uint32_t *row_bytes);
int bt_table_export_count_rows(bt_table *t, uint8_t *d_rows, uint64_t capacity_rows, uint64_t *h_num_rows);
int bt_table_merge_count_rows(bt_table *t, const uint8_t *d_rows, uint64_t num_rows);
/* The table as packed records, and a checkpoint file of them.  The reference has no counterpart: a genotype run always rebuilds its table; this is
 * the "optionally persist the matched k-mer table per unit (cheap restart of Gibbs)" of SURVEY.md §5, row "Checkpoint / resume".
 * A packed record = 16 key bytes (lo, hi, little endian) + the 4 meta bytes in bt_table_read_slots' order + the samples' counts padded with
 * zeros to a multiple of four: *record_bytes = 20 + that.  Record order is unspecified (as bt_table_export's).
 * bt_table_pack: every stored record -> d_records (device, capacity_records records); *h_num_records = number of stored records.  Capacity 0 and
 *   d_records NULL only counts; a capacity that is too small is an error and nothing is written.
 * bt_table_unpack: addKmer of every record's key, then its meta bytes and counts are SET (not added).  A record whose key the table already holds
 *   (or that repeats an earlier record's key) is not applied and the call fails; a full table raises the overflow flag (bt_table_status). */
int bt_table_record_bytes(bt_table *t, uint32_t *record_bytes);
int bt_table_pack(bt_table *t, uint8_t *d_records, uint64_t capacity_records, uint64_t *h_num_records);
int bt_table_unpack(bt_table *t, const uint8_t *d_records, uint64_t num_records);
/* bt_table_save: the table's records -> the file `path` (written as <path>.tmp and renamed when complete), with the caller's `manifest` text (NULL = "")
 *   — whatever identifies the inputs the table was computed from.  File: header (magic "BTAMDKTBL1", version, k, num_samples, record bytes, record
 *   count, largest chunk, length-prefixed manifest, CRC32), chunks ("CHNK", record count, records, CRC32), trailer ("TEND", record count, CRC32); all
 *   little endian.  The table is walked in ranges of 2^22 slots (BT_TABLE_CKPT_SLOTS lowers that): packed on the device, copied out through pinned
 *   memory while the previous range is written; the host holds two ranges at most.
 * bt_table_load: a new table sized as bt_table_create(expected_size = record count) holding the file's records.  Header, every chunk's CRC, the
 *   trailer and — unless expected_manifest is NULL — the manifest are verified; any mismatch is an error (a manifest mismatch names the first line
 *   that differs), *out stays NULL and nothing is kept.
 * bt_table_file_info: the same verification of the whole file and its header fields, without a GPU (manifest: NUL-terminated, truncated to manifest_len). */
int bt_table_save(bt_table *t, const char *path, const char *manifest);
int bt_table_load(bt_ctx *ctx, const char *path, const char *expected_manifest /* NULL: any */, bt_table **out);
int bt_table_file_info(const char *path, uint32_t *k, uint32_t *num_samples, uint64_t *num_records, char *manifest, size_t manifest_len);

/* ObservedKmerCountsHash<N>::calculateKmerStats (src/bayesTyper/KmerHash.cpp:256-340): one pass over the table.
 * h_class_counts[7] = {total, unique, multicluster, decoy, max_multiplicity, multigroup, non_cluster} exactly as the reference
 * tallies them (:268-321).  For every PARAMETER k-mer without cluster occurrence and every sample s the observed count c enters
 * the bin (s, m = interclusterMultiplicity(gender[s])): the device accumulates the exact integer moments
 *   h_n[s*256+m] += 1, h_nonzero[s*256+m] += (c != 0), h_sum[s*256+m] += c, h_sumsq[s*256+m] += c*c
 * (order-independent, unlike the reference's running Welford update; KmerStats count / fraction / mean / variance follow from them on the host:
 * KmerStats.cpp:51-63,107-121).  gender[s]: 0 female, 1 male (Utils::Gender). */
int bt_table_kmer_stats(bt_table *t, const uint8_t *h_gender, uint64_t *h_class_counts, uint64_t *h_n, uint64_t *h_nonzero, uint64_t *h_sum,
                        uint64_t *h_sumsq);

/* KmerCounter::countInterclusterKmers for ONE region (src/bayesTyper/KmerCounter.cpp:291-338):
 * slide over d_seq[0..len), canonical k-mers that hit `path_bloom` are added to the table
 * (addKmer sorted) and get addInterclusterMultiplicity(is_decoy, {female_ploidy, male_ploidy})
 * (KmerCounts.cpp:98-118). */
int bt_table_count_intercluster(bt_table *t, bt_bloom *path_bloom, const char *d_seq, uint64_t len,
                                int is_decoy, uint32_t female_ploidy, uint32_t male_ploidy);

/* The same for ALL regions of one sequence in one launch (KmerCounter::countInterclusterKmers walks the region list of a unit,
 * src/bayesTyper/KmerCounter.cpp:349-386: one call per region would be one kernel launch per region).  Region r covers
 * d_seq[h_start[r] .. h_start[r] + h_len[r]); its k-mers get addInterclusterMultiplicity(h_is_decoy[r], {h_female_ploidy[r], h_male_ploidy[r]}).
 * The update is commutative, so the result equals the region-by-region calls in any order.  Synchronises the context's stream. */
int bt_table_count_intercluster_regions(bt_table *t, bt_bloom *path_bloom, const char *d_seq, uint32_t num_regions, const uint64_t *h_start, const uint64_t *h_len,
                                        const uint8_t *h_is_decoy, const uint8_t *h_female_ploidy, const uint8_t *h_male_ploidy);

/* KmerCounter::countInterclusterParameterKmers (src/bayesTyper/KmerCounter.cpp:161-250) for a batch of disjoint intercluster
 * regions of one device-resident sequence: region r = d_seq[h_start[r] .. h_start[r] + h_len[r]).  Every canonical k-mer of a
 * region that is NOT in the path Bloom filter is, in window order, either recorded as decoy (h_is_decoy[r]) or accepted by a
 * bernoulli_distribution(fraction) draw of mt19937(h_seed[r]) (h_seed[r] = prng_seed + intercluster_regions_idx, :176); accepted
 * k-mers are inserted with BT_KC_PARAMETER, decoy ones with BT_KC_DECOY_OCC.  The table plays KmerHash<bool>: the reference's
 * final value of a k-mer is PARAMETER && !DECOY_OCC (independent of the order regions are processed in). */
int bt_table_count_parameter_kmers(bt_table *t, bt_bloom *path_bloom, const char *d_seq, uint32_t num_regions, const uint64_t *h_start,
                                   const uint64_t *h_len, const uint8_t *h_is_decoy, const uint32_t *h_seed, float fraction);

/* the table-update half of VariantClusterGraph::classifyPathKmers for one batch of DISTINCT
 * path k-mers of distinct clusters (src/bayesTyper/VariantClusterGraph.cpp:902-938): for k-mer i
 * with max-over-paths multiplicity d_mult[i]: findKmer; absent and mult > 127 -> addKmer;
 * present -> addClusterMultiplicity(mult, multigroup_bloom.lookup(kmer)) (KmerCounts.cpp:137-159);
 * d_excluded[i] = isExcluded() after the update (0 when absent).  A k-mer may occur several
 * times in the batch (once per cluster that contains it). */
int bt_table_classify_batch(bt_table *t, bt_bloom *multigroup_bloom, const uint64_t *d_kmers,
                            const uint8_t *d_mult, uint64_t n, uint8_t *d_excluded);

/* ------------------------------------------------------------------------------------------
 * KMC count-table scan: KmerCounter::parseSampleKmers + parseSampleKmersCallBack
 *   src/bayesTyper/KmerCounter.cpp:388-524; KMC record layout external/kmc_api/kmc_file.cpp:428-494
 * ---------------------------------------------------------------------------------------- */
typedef struct bt_kmc_scan bt_kmc_scan;

/* Describes one KMC database for the scan: k, lut_prefix_length p ((k-p)%4==0), counter_size
 * (1..4 bytes, little endian; counts must be <= 255 as asserted at KmerCounter.cpp:401),
 * total record count and the prefix LUT (4^p + 1 entries: LUT[j] = index of the first record
 * whose prefix is >= j, LUT[4^p] = total; host memory, copied). */
int bt_kmc_scan_create(bt_ctx *ctx, uint32_t k, uint32_t lut_prefix_len, uint32_t counter_size,
                       uint64_t total_records, const uint64_t *h_prefix_lut, bt_kmc_scan **out);
/* The same with an explicit LUT length for KMC2 ("0x200") databases, whose .kmc_pre holds one prefix table per signature bin,
 * concatenated (num_lut_entries = bins * 4^p + 1, last entry = total; external/kmc_api/kmc_file.cpp:186-238,428-449): the record's
 * prefix is (LUT index) mod 4^p. */
int bt_kmc_scan_create_bins(bt_ctx *ctx, uint32_t k, uint32_t lut_prefix_len, uint32_t counter_size, uint64_t total_records,
                            const uint64_t *h_prefix_lut, uint64_t num_lut_entries, bt_kmc_scan **out);
/* the database header's [min_count, max_count]: records whose counter lies outside are skipped, as CKMCFile::ReadNextKmer does
 * (external/kmc_api/kmc_file.cpp:496-511).  Default: no record is skipped. */
int bt_kmc_scan_set_count_range(bt_kmc_scan *s, uint32_t min_count, uint64_t max_count);
int bt_kmc_scan_destroy(bt_kmc_scan *s);
/* Push records [first_record, first_record + n) of the .kmc_suf payload through
 * decode -> path_bloom.lookup -> (on hit) table.addKmer(unsorted) + addSampleCount(sample, count).
 * d_records points at the first byte of record `first_record` and must be 16-byte aligned;
 * record size = (k-p)/4 + counter_size.  d_hit_count (optional, device uint64) is incremented
 * by the number of Bloom hits. */
int bt_kmc_scan_run(bt_kmc_scan *s, bt_bloom *path_bloom, bt_table *table, uint32_t sample_idx,
                    const uint8_t *d_records, uint64_t first_record, uint64_t n, uint64_t *d_hit_count);
/* The same for records in HOST memory (e.g. the memory-mapped .kmc_suf): the range is streamed through two pinned staging
 * buffers and two device buffers — host copy, H2D transfer (own stream) and scan of consecutive chunks overlap.  Blocking;
 * chunk_records = records per transfer (0: default 2^23); the staging buffers are kept with the handle; *h_hit_count = number of Bloom hits. */
int bt_kmc_scan_run_host(bt_kmc_scan *s, bt_bloom *path_bloom, bt_table *table, uint32_t sample_idx, const uint8_t *h_records,
                         uint64_t first_record, uint64_t n, uint64_t chunk_records, uint64_t *h_hit_count);
/* the same from the database's .kmc_suf file: the records [first_record, first_record + n) at payload_offset (4: behind the "KMCS" marker) + first_record x record size
 * are read by several threads with pread() straight into the pinned staging slots (the reference reads the file through CKMCFile's buffered reader,
 * kmc_file.cpp:428-515, one producer thread: KmerCounter.cpp:469-505) — no memory mapping, no page fault per 4 KB of a first pass */
int bt_kmc_scan_run_file(bt_kmc_scan *s, bt_bloom *path_bloom, bt_table *table, uint32_t sample_idx, const char *suf_path, uint64_t payload_offset,
                         uint64_t first_record, uint64_t n, uint64_t chunk_records, uint64_t *h_hit_count);
/* bayesTyperTools makeBloom (src/bayesTyperTools/MakeBloom.cpp:200-295): the k-mers of records [first_record, first_record + n)
 * are added to a sample's KmerBloom (created with bt_bloom_create(ctx, total_kmers, fpr, k, 0, ..), written with bt_bloom_save:
 * byte-identical .bloomMeta / .bloomData, insertion being an order-independent OR) */
int bt_kmc_scan_make_bloom(bt_kmc_scan *s, bt_bloom *sample_bloom, const uint8_t *d_records, uint64_t first_record, uint64_t n);
/* bayesTyperTools getKmerStats (src/bayesTyperTools/scripts/getKmerStats.cpp:87-127): a histogram over (k-mer count, #A, #C, #G, #T) of
 * the records whose counter lies in the count range (bt_kmc_scan_set_count_range, as CKMCFile::ReadNextKmer skips the others).
 * Bin layout: count * C(k+3,3) + comp(a, c, g) for count 0..255, where comp enumerates the compositions a + c + g <= k (t = k - a - c - g)
 * in (a, c, g) lexicographic order:
 *   comp(a, c, g) = [C(k+3,3) - C(k-a+3,3)] + [C(k-a+2,2) - C(k-a-c+2,2)] + g
 * so increasing bin index is increasing (count, A, C, G, T).  bt_kmer_stats_num_bins(k) = 256 * C(k+3,3) (63 MB of uint64 at k = 55, 98 MB at
 * k = 64); 0 for k outside 1..64.
 * The reference asserts count <= 255 (line 113): a record in range with a larger count is not binned but counted in *d_over255.
 * Adds are exact integer adds, so the histogram does not depend on the order records arrive in. */
uint64_t bt_kmer_stats_num_bins(uint32_t k);
/* Records [first_record, first_record + n) in device memory (d_records at record first_record, 16-byte aligned, as for
 * bt_kmc_scan_make_bloom) are ADDED into the caller-zeroed device histogram d_hist (bt_kmer_stats_num_bins(k) uint64) and the device
 * uint64 *d_over255.  Asynchronous on the context's stream. */
int bt_kmc_scan_kmer_stats(bt_kmc_scan *s, const uint8_t *d_records, uint64_t first_record, uint64_t n, uint64_t *d_hist, uint64_t *d_over255);
/* The same for records [first_record, first_record + n) of the .kmc_suf file at payload_offset (4: behind the "KMCS" marker), streamed through
 * the staging slots of bt_kmc_scan_run_file (chunk_records: records per transfer, 0: default).  Blocking.  h_hist (host,
 * bt_kmer_stats_num_bins(k) uint64) receives the histogram; *h_binned = records binned, *h_over255 = records in range above 255 (either may be
 * NULL).  progress (may be NULL) is called with the number of records streamed so far after each chunk is handed to the device. */
int bt_kmc_scan_kmer_stats_file(bt_kmc_scan *s, const char *suf_path, uint64_t payload_offset, uint64_t first_record, uint64_t n, uint64_t chunk_records,
                                uint64_t *h_hist, uint64_t *h_binned, uint64_t *h_over255, void (*progress)(uint64_t records_done, void *user), void *progress_user);
/* decode only (tests): d_kmers[2*i..] = packed k-mer of record i, d_counts[i] = its count */
int bt_kmc_scan_decode(bt_kmc_scan *s, const uint8_t *d_records, uint64_t first_record, uint64_t n,
                       uint64_t *d_kmers, uint32_t *d_counts);

/* ------------------------------------------------------------------------------------------
 * Reads scan: what the consumers of a sample's KMC database compute, computed from the reads themselves.
 * A READS TEXT is ASCII bases, one read per line, joined by '\n'.  Every byte outside ACGTacgt (N, the newline, anything else: the rule of
 * bt_kmers_from_sequence) ends the k-mer window, so no k-mer spans two reads; lower case counts as upper case.  Every window of k valid bases
 * contributes its canonical k-mer once per occurrence.  All three consumers are commutative: the result depends on the multiset of k-mers only, not
 * on the order or the cut of the texts handed in.  The d_ calls are asynchronous on the context's stream; k is 1 .. 64.
 * ---------------------------------------------------------------------------------------- */
/* KmerCounter::parseSampleKmers + parseSampleKmersCallBack (src/bayesTyper/KmerCounter.cpp:388-524) without the database: every k-mer occurrence of
 * d_text[0 .. len) that hits path_bloom does table.addKmer(unsorted) + addSampleCount(sample_idx, 1), saturating at 255 — what bt_kmc_scan_run does
 * with the record (k-mer, min(occurrences, 255)) of a database counted from the same reads.  k is the table's.  d_hit_count (optional, device
 * uint64) is incremented by the number of OCCURRENCES that hit the filter. */
int bt_reads_count(bt_ctx *ctx, bt_bloom *path_bloom, bt_table *table, uint32_t sample_idx, const char *d_text, uint64_t len, uint64_t *d_hit_count);
/* bayesTyperTools makeBloom (src/bayesTyperTools/MakeBloom.cpp:200-295) without the database: the k-mers of d_text[0 .. len) are added to a sample's
 * KmerBloom (bt_bloom_create(ctx, num_kmers, fpr, k, 0, ..)): the bits bt_kmc_scan_make_bloom sets from a database of the same reads. */
int bt_reads_make_bloom(bt_ctx *ctx, bt_bloom *sample_bloom, const char *d_text, uint64_t len, uint32_t k);
/* A HyperLogLog sketch of the distinct canonical k-mers (the number a KMC database states in its header; makeBloom sizes the filter with it,
 * MakeBloom.cpp:200-295): 65536 one-byte registers in device memory (4-byte aligned, zeroed by the caller before the first text).  Register = top 16
 * bits of the splitmix64 finaliser of the k-mer's ntHash, rank = 1 + leading zeros of the other 48 bits (at most 49); a register takes the maximum. */
int bt_reads_sketch(bt_ctx *ctx, const char *d_text, uint64_t len, uint32_t k, uint8_t *d_registers);
/* The same three for a text in HOST memory, streamed through the pinned staging slots of bt_kmc_scan_run_host (kept with the context).  Blocking;
 * chunk_bytes = bytes per transfer (0: default 64 MiB); consecutive transfers overlap by k - 1 bytes and no window is consumed twice, so chunk_bytes
 * changes no result.  A text must end at a read boundary: nothing is carried from one call to the next.  *h_hit_count (optional) = occurrences that
 * hit the filter; h_registers (65536 bytes) is read, merged into and written back. */
int bt_reads_count_host(bt_ctx *ctx, bt_bloom *path_bloom, bt_table *table, uint32_t sample_idx, const char *h_text, uint64_t len, uint64_t chunk_bytes,
                        uint64_t *h_hit_count);   /* KmerCounter.cpp:388-524 */
int bt_reads_make_bloom_host(bt_ctx *ctx, bt_bloom *sample_bloom, const char *h_text, uint64_t len, uint32_t k, uint64_t chunk_bytes);   /* MakeBloom.cpp:200-295 */
int bt_reads_sketch_host(bt_ctx *ctx, const char *h_text, uint64_t len, uint32_t k, uint64_t chunk_bytes, uint8_t *h_registers);   /* MakeBloom.cpp:200-295 */
/* Host only, no GPU: the number of distinct k-mers from 65536 registers (the N of MakeBloom.cpp:200-295's KmerBloom(N, fpr)) — the standard
 * estimator alpha m^2 / sum 2^-register, replaced by linear counting m ln(m / zero registers) at or below 2.5 m. */
int bt_reads_sketch_estimate(const uint8_t *h_registers, double *out);
/* Host only, no GPU: the kernels' window code run by one thread over h_text[0 .. len) (what KmerCounter.cpp:388-524 would see record by record, here
 * occurrence by occurrence).  Window i in text order: h_kmers[2i], h_kmers[2i + 1] = the canonical k-mer (lo, hi), h_hashes[i] = its ntHash,
 * h_ends[i] = index of its last byte (each array may be NULL).  *n = number of windows; an error when capacity is smaller (n is still set). */
int bt_diag_reads_kmers(const char *h_text, uint64_t len, uint32_t k, uint64_t *h_kmers, uint64_t *h_hashes, uint64_t *h_ends, uint64_t capacity, uint64_t *n);
/* Host only, no GPU: the sketch of bt_reads_sketch built by the same window code on one thread; h_registers (65536 bytes) is merged into. */
int bt_diag_reads_sketch(const char *h_text, uint64_t len, uint32_t k, uint8_t *h_registers);

/* ------------------------------------------------------------------------------------------
 * Packed reads: a reads text as 2-bit codes plus one validity bit per position — what the reads scan makes of every byte before it does anything
 * else — so that a later pass over the same sample needs no inflate and no parse (no counterpart in the reference, which reads a KMC database).
 * A text of n bytes becomes ceil(n / 128) blocks of 48 bytes (twelve little-endian 32-bit words); block b covers positions 128 b .. 128 b + 127:
 *   words 0 - 7   codes: position j of the block in word j / 16, bits 2 (j % 16) and up
 *   words 8 - 11  validity: position j in word 8 + j / 32, bit j % 32
 * ACGTacgt give 0..3 and valid, every other byte code 0 and invalid (the rule of bt_kmers_from_sequence); positions at and beyond n in the last block
 * are written as code 0, invalid.  The inverse gives the canonical text: upper-case bases, every invalid position '\n'.  Packed buffers are 4-byte
 * aligned.  Consumers ignore positions at and beyond `positions` whatever their bits say.
 * ---------------------------------------------------------------------------------------- */
uint64_t bt_reads_packed_bytes(uint64_t positions);   /* 48 * ceil(positions / 128); no counterpart */
/* d_text[0 .. len) -> d_packed[0 .. bt_reads_packed_bytes(len)) and back, on the context's stream (no counterpart; the byte rule is Utils.cpp's
 * nucleotide alphabet as in bt_kmers_from_sequence). */
int bt_reads_pack(bt_ctx *ctx, const char *d_text, uint64_t len, uint8_t *d_packed);
int bt_reads_unpack(bt_ctx *ctx, const uint8_t *d_packed, uint64_t positions, char *d_text);
/* Host only, no GPU: the same map by the same code on one thread (no counterpart). */
int bt_diag_reads_pack(const char *h_text, uint64_t len, uint8_t *h_packed);
int bt_diag_reads_unpack(const uint8_t *h_packed, uint64_t positions, char *h_text);
/* The three consumers of the reads scan over a packed text: (packed, positions) in place of (text, len), every other argument and every result as in
 * bt_reads_count / bt_reads_make_bloom / bt_reads_sketch and their _host variants.  chunk_bytes counts packed bytes; a transfer starts on the block
 * boundary at or before the first new position minus k - 1, so chunk_bytes changes no result. */
int bt_reads_count_packed(bt_ctx *ctx, bt_bloom *path_bloom, bt_table *table, uint32_t sample_idx, const uint8_t *d_packed, uint64_t positions,
                          uint64_t *d_hit_count);   /* KmerCounter.cpp:388-524 */
int bt_reads_make_bloom_packed(bt_ctx *ctx, bt_bloom *sample_bloom, const uint8_t *d_packed, uint64_t positions, uint32_t k);   /* MakeBloom.cpp:200-295 */
int bt_reads_sketch_packed(bt_ctx *ctx, const uint8_t *d_packed, uint64_t positions, uint32_t k, uint8_t *d_registers);   /* MakeBloom.cpp:200-295 */
int bt_reads_count_packed_host(bt_ctx *ctx, bt_bloom *path_bloom, bt_table *table, uint32_t sample_idx, const uint8_t *h_packed, uint64_t positions,
                               uint64_t chunk_bytes, uint64_t *h_hit_count);   /* KmerCounter.cpp:388-524 */
int bt_reads_make_bloom_packed_host(bt_ctx *ctx, bt_bloom *sample_bloom, const uint8_t *h_packed, uint64_t positions, uint32_t k,
                                    uint64_t chunk_bytes);   /* MakeBloom.cpp:200-295 */
int bt_reads_sketch_packed_host(bt_ctx *ctx, const uint8_t *h_packed, uint64_t positions, uint32_t k, uint64_t chunk_bytes,
                                uint8_t *h_registers);   /* MakeBloom.cpp:200-295 */
/* Host only, no GPU: bt_diag_reads_kmers over a packed text (KmerCounter.cpp:388-524 occurrence by occurrence); h_ends[i] is a position. */
int bt_diag_reads_kmers_packed(const uint8_t *h_packed, uint64_t positions, uint32_t k, uint64_t *h_kmers, uint64_t *h_hashes, uint64_t *h_ends,
                               uint64_t capacity, uint64_t *n);

/* The reads pack file (no counterpart; the layout is bayestyper_amd/csrc/bt_reads_pack_file.hpp): a checksummed header with k and a manifest text,
 * one checksummed section per slab (positions, and the bases and reads the source reader counted for it, then the packed payload), a trailer with the
 * section count and the totals.  Host only, no GPU.  The writer writes <path>.tmp.<pid> and renames it in _finish: an interrupted run leaves no file. */
typedef struct bt_reads_pack_writer bt_reads_pack_writer;
typedef struct bt_reads_pack_reader bt_reads_pack_reader;
typedef struct {
    uint32_t version, k, block_positions, manifest_bytes;
    uint64_t sections, positions, bases, reads;   /* the trailer's totals */
    uint64_t max_section_positions;               /* a buffer of bt_reads_packed_bytes(this) bytes takes any section */
} bt_reads_pack_info;
int bt_reads_pack_writer_create(const char *path, uint32_t k, const char *manifest, bt_reads_pack_writer **out);   /* no counterpart */
int bt_reads_pack_writer_add(bt_reads_pack_writer *w, const uint8_t *h_packed, uint64_t positions, uint64_t bases, uint64_t reads);   /* no counterpart */
int bt_reads_pack_writer_finish(bt_reads_pack_writer *w);     /* no counterpart */
void bt_reads_pack_writer_destroy(bt_reads_pack_writer *w);   /* no counterpart; before _finish: the temporary file is removed */
/* _open validates the header, every section head, the trailer and the file's size before anything is handed out; a section's CRC-32 is checked when
 * _next reads its payload (the message names the section and its file offset).  *end = 1, and nothing else set, after the last section. */
int bt_reads_pack_reader_open(const char *path, bt_reads_pack_reader **out, bt_reads_pack_info *info);   /* no counterpart */
int bt_reads_pack_reader_manifest(bt_reads_pack_reader *r, char *buf, uint64_t capacity, uint64_t *len);   /* no counterpart */
int bt_reads_pack_reader_next(bt_reads_pack_reader *r, uint8_t *h_packed, uint64_t capacity, uint64_t *positions, uint64_t *bases, uint64_t *reads,
                              int *end);   /* no counterpart */
void bt_reads_pack_reader_close(bt_reads_pack_reader *r);   /* no counterpart */
int bt_reads_pack_file_info(const char *path, bt_reads_pack_info *info);   /* no counterpart */

/* ------------------------------------------------------------------------------------------
 * Path k-mer enumeration over variant-cluster graphs:
 *   VariantClusterGraph::{countPathKmers, classifyPathKmers, getHaplotypeCandidates, updateVariantPathIndices}
 *   (src/bayesTyper/VariantClusterGraph.cpp:800-1184), driven per unit by KmerCounter::{countPathKmers, classifyPathKmers}
 *   (src/bayesTyper/KmerCounter.cpp:252-289,526-555) and VariantClusterGroup::initGenotyper.
 * Input: the graphs as VariantClusterGraph holds them after findSamplePaths — vertices in topological (vertex-index) order
 * with the fields of VariantClusterGraphVertex (include/bayesTyper/VariantClusterGraphVertex.hpp:43-73) and the best-path
 * bitmaps best_paths_indices (P x |V|).  Output of the last stage: the VariantClusterHaplotypes bundle of every cluster in the
 * flattened form bt_gibbs_batch takes.
 * ---------------------------------------------------------------------------------------- */
typedef struct bt_paths_batch {
    uint32_t num_clusters;             /* C */
    const uint32_t *vertex_off;        /* [C+1] vertices of cluster c, in vertex-index order */
    const uint32_t *num_paths;         /* [C] number of best paths (= haplotype candidates H) */
    /* ---- per vertex (NV = vertex_off[C]) ---- */
    const uint64_t *seq_off;           /* [NV+1] nucleotides of vertex v: seq[seq_off[v] .. seq_off[v+1]) */
    const uint8_t *seq;                /* one 2-bit code per byte (A 0, C 1, G 2, T 3: Nucleotide.hpp:40-70) */
    const uint16_t *vertex_variant;    /* variant_allele_idx.first, 0xFFFF = none */
    const uint16_t *vertex_allele;     /* variant_allele_idx.second */
    const uint8_t *vertex_flags;       /* bit 0 is_disconnected, bit 1 is_first_nucleotides_redundant */
    const uint32_t *vertex_nested;     /* nested_variant_cluster_index, 0xFFFFFFFF = none */
    const uint32_t *refvar_off;        /* [NV+1] -> refvar */
    const uint16_t *refvar;            /* reference_variant_indices */
    /* ---- per cluster ---- */
    const uint64_t *path_off;          /* [C+1] -> path_vertices; cluster c: num_paths[c] rows of (vertex_off[c+1]-vertex_off[c]) bytes */
    const uint8_t *path_vertices;      /* best_paths_indices, row-major (path, vertex), 0/1 */
    const uint32_t *var_off;           /* [C+1] -> per-variant arrays (variant_cluster_info) */
    const uint16_t *var_num_alleles;   /* numberOfAlleles(), incl. the missing allele of variants with has_dependency */
    const uint8_t *var_has_dependency;
    /* ---- graph edges: only needed by bt_find_paths_* (may be NULL otherwise) ---- */
    const uint32_t *in_off;            /* [NV+1] in-edges of vertex v -> in_src, in boost::in_edges order (edge insertion order) */
    const uint32_t *in_src;            /* source vertex, local to the cluster (always < the target's local index) */
} bt_paths_batch;

typedef struct bt_paths bt_paths;

/* uploads the graphs, lays every best path out as one text (k-mer windows never span a disconnected vertex or two paths) and
 * enumerates the canonical k-mer of every window once; *h_num_kmer_occurrences (optional) = number of full windows */
int bt_paths_create(bt_ctx *ctx, const bt_paths_batch *batch, uint32_t k, bt_paths **out, uint64_t *h_num_kmer_occurrences);
int bt_paths_destroy(bt_paths *p);
/* VariantClusterGraph::countPathKmers + KmerCounter::countPathKmersCallback (KmerCounter.cpp:252-289): every path k-mer is
 * added to the path Bloom filter (the reference first collects them in an unordered_set; insertion is idempotent) */
int bt_paths_count_kmers(bt_paths *p, bt_bloom *path_bloom);
/* KmerCounter::countPathMultigroupKmers (src/bayesTyper/KmerCounter.cpp:105-159) — cluster stage.  h_cluster_group[c] = index of
 * the variant-cluster group of cluster c; clusters are listed group by group, groups in index order, a group's clusters in its vertex
 * order (an error otherwise).  Every distinct path k-mer of a group is looked up in the path Bloom filter: present -> it goes into
 * the multigroup table (KmerHash<bool>), absent -> it is added to the filter; *h_num_path_kmers = sum over groups of their distinct
 * path k-mers (inference_unit->num_path_kmers).  The outcome — including the k-mers that enter the table as false positives of what
 * the filter holds at that moment — is the one of the reference run with ONE thread (with more threads the reference's outcome
 * depends on thread timing): groups in index order, a group's k-mers in the iteration order of the std::unordered_set<std::bitset<2k>>
 * (libstdc++) the reference collects them in and reuses from group to group.  Afterwards every path k-mer is in the filter. */
int bt_paths_count_multigroup(bt_paths *p, const uint32_t *h_cluster_group, bt_bloom *path_bloom, bt_table *multigroup_table, uint64_t *h_num_path_kmers);
/* How the iteration orders of KmerCounter.cpp:105-159 (the unordered_set of a group's path k-mers, :111-119) are computed on the device.  A group of at
 * least wide_min_kmers distinct path k-mers is ordered by a workgroup of its own, stage by stage (a stage = the inserts between two rehashes; the list after a
 * stage has a closed form), every other group by one lane that replays the container insert by insert; the orders are the same.  The threshold is
 * BT_MG_WIDE_MIN, read at every bt_paths_count_multigroup call: unset or 0 = one lane per group for every group, N = groups of at least N distinct k-mers
 * take a workgroup (1 = every non-empty group); anything but a decimal number below 2^32 fails the call.  The values describe the last call that SUCCEEDED.
 * max_group_kmers: the largest group; max_stages: the most stages a wide group ran (0 without one);
 * wide_scratch_bytes: device memory of the wide groups' work areas (0 without one). */
typedef struct {
    uint32_t num_groups, num_wide_groups, wide_min_kmers, max_group_kmers, max_stages;
    uint64_t wide_scratch_bytes;
} bt_multigroup_stats;
/* the last bt_paths_count_multigroup call of this handle (all zero before the first); KmerCounter.cpp:105-159 has no counterpart */
int bt_paths_multigroup_info(bt_paths *p, bt_multigroup_stats *stats);
/* The container orders of KmerCounter.cpp:105-159 alone, by the routine bt_paths_count_multigroup runs: G consecutive groups of DISTINCT packed k-mers
 * (2 x u64 each; group g = h_kmers[2 * h_off[g] .. 2 * h_off[g + 1]), in insertion order) go through one std::unordered_set<std::bitset<2k>> that starts
 * with initial_buckets buckets (1 = freshly constructed) and is clear()ed between groups, so that every group inherits its predecessor's bucket count.
 * h_rank[i] = position of k-mer i in its group's iteration order, h_final_buckets[g] (optional) = the bucket count after group g — both as
 * bt_diag_kmer_set_order defines them; groups of at least wide_min k-mers (0 = none) take the workgroup route; stats is optional. */
int bt_kmer_set_orders(bt_ctx *ctx, const uint64_t *h_kmers, const uint64_t *h_off, uint32_t G, unsigned k, uint64_t initial_buckets, uint32_t wide_min, uint32_t *h_rank,
                       uint64_t *h_final_buckets, bt_multigroup_stats *stats);
/* VariantClusterGraph::classifyPathKmers for every cluster (VariantClusterGraph.cpp:848-939): per distinct path k-mer of a
 * cluster the maximum over its paths of the (saturating) per-path multiplicity -> table update as bt_table_classify_batch.
 * h_num_path_kmers[c] = distinct k-mers of cluster c (num_path_kmers), h_has_excluded[c] = has_excluded_kmers. */
int bt_paths_classify(bt_paths *p, bt_table *table, bt_bloom *multigroup_bloom, uint32_t *h_num_path_kmers, uint8_t *h_has_excluded);

/* host arrays receiving getHaplotypeCandidates' result for all clusters; sizes from bt_paths_candidates (R rows, NNZ incidence
 * entries, ...).  Field meaning as in bt_gibbs_batch; row ids in unique_idx / multi_idx are local to the cluster. */
typedef struct bt_paths_candidates_out {
    uint32_t *kmer_off;          /* [C+1] */
    uint8_t *hap_kmer_mult;      /* sum_c K_c * H_c */
    uint64_t *kmer_key;          /* [R*2] packed canonical k-mer of the row (identifies shared records of multicluster k-mers) */
    uint8_t *kmer_has_counts;    /* [R] the k-mer has a record in the table */
    uint8_t *kmer_counts;        /* [R*S] */
    uint8_t *kmer_ic_mult;       /* [R*2] */
    uint32_t *kv_off;            /* [R+1] */
    uint16_t *kv_var;            /* [NNZ] entries of a row sorted by variant index (the reference's order is an unordered_map's) */
    uint32_t *kv_bits;           /* ceil(H/32) words per entry */
    uint32_t *unique_off;        /* [C+1] */
    uint32_t *unique_idx;
    uint32_t *multi_off;         /* [C+1] */
    uint32_t *multi_idx;
    uint16_t *hap_allele;        /* sum_c H_c * V_c */
    uint32_t *hapnest_off;       /* [sum_c H_c + 1] */
    uint32_t *hapnest_idx;
    uint32_t *nestdep_off;       /* [C+1] */
    uint32_t *nestdep_cluster;
    uint32_t *nestdep_var_off;   /* [ND+1] */
    uint16_t *nestdep_var;
} bt_paths_candidates_out;

typedef struct bt_paths_candidates_sizes {
    uint64_t rows, mult_bytes, nnz, kv_words, num_unique, num_multi, hap_allele, num_haplotypes, hapnest, nestdep, nestdep_var;
} bt_paths_candidates_sizes;

/* VariantClusterGraph::getHaplotypeCandidates for every cluster (VariantClusterGraph.cpp:941-1135) against the classified
 * table: computes the bundle on the device + host and reports its sizes; bt_paths_candidates_fetch copies it out. */
int bt_paths_candidates(bt_paths *p, bt_table *table, bt_paths_candidates_sizes *sizes);
int bt_paths_candidates_fetch(bt_paths *p, bt_paths_candidates_out *out);
/* The same bundle with every per-row / per-entry array LEFT IN DEVICE MEMORY, owned by `p`: hap_kmer_mult, kmer_key, kmer_has_counts, kmer_counts,
 * kmer_ic_mult, kv_off, kv_var, kv_bits, unique_idx, multi_idx.  The reference builds the bundle inside the genotyper and hands it over in memory
 * (VariantClusterGenotyper.cpp:59-106 <- VariantClusterGraph.cpp:941-1135); here bt_gibbs_source_create_from_paths takes these arrays over without a pass
 * through the host.  Only the [C+1] offset arrays and what the host graph walk gives (hap_allele, hapnest_*, nestdep_*: VariantClusterGraph.cpp:984-1017,
 * 1093-1132) exist on the host: bt_paths_candidates_fetch_small copies them out (the per-row pointers of `out` must be NULL); it also works after
 * bt_paths_candidates.  bt_paths_candidates = this call + copies to the host.  The incidence lists (updateVariantPathIndices, :1137-1184) are built per
 * row without a global sort: with BT_PATHS_DEBUG set, a line on stderr tells how many rows each of the three row kernels took (BT_PATHS_ROW_LANE_MAX /
 * BT_PATHS_ROW_WAVE_MAX lower their thresholds of 8 / 64 triples for tests). */
int bt_paths_candidates_device(bt_paths *p, bt_table *table, bt_paths_candidates_sizes *sizes);
int bt_paths_candidates_fetch_small(bt_paths *p, bt_paths_candidates_out *out);

/* ------------------------------------------------------------------------------------------
 * Best-path search per sample: VariantClusterGraph::{findSamplePaths, mergePaths, isPathsRedundant, filterPaths, addPathIndices}
 *   (src/bayesTyper/VariantClusterGraph.cpp:389-798) with VariantClusterGraphPath (src/bayesTyper/VariantClusterGraphPath.cpp:38-225),
 *   driven per sample by KmerCounter::findVariantClusterPaths (src/bayesTyper/KmerCounter.cpp:59-103).
 * ---------------------------------------------------------------------------------------- */
typedef struct bt_find_paths bt_find_paths;
/* state for the clusters of `batch` (num_paths / path_* fields ignored, in_off / in_src required): empty best_paths_indices */
int bt_find_paths_create(bt_ctx *ctx, const bt_paths_batch *batch, uint32_t k, uint32_t max_sample_haplotypes, uint32_t num_samples, bt_find_paths **out);
int bt_find_paths_destroy(bt_find_paths *f);
/* one sample: findSamplePaths of every cluster against the sample's KmerBloom with mt19937(h_seeds[c]) — the reference's seed is
 * prng_seed + (group_idx + 1) * (sample_idx + 1) + variant_cluster_idx (KmerCounter.cpp:65, VariantClusterGroup.cpp:142) — followed
 * by addPathIndices into the accumulated best paths */
int bt_find_paths_sample(bt_find_paths *f, bt_bloom *sample_bloom, const uint32_t *h_seeds);
/* n samples in one call, defined as exactly n calls of bt_find_paths_sample in array order (the loop of KmerCounter::findVariantClusterPaths,
 * src/bayesTyper/KmerCounter.cpp:59-103, over VariantClusterGraph.cpp:389-798): same rows, same counts, same error codes.  h_seeds: [n * C], sample-major, the
 * clusters in batch order.  findSamplePaths, mergePaths and filterPaths of every (sample, cluster) run at once, each sample in a scratch copy of its own;
 * addPathIndices then folds the samples' final paths into the rows per cluster, sample 0 first.  Errors: a null argument, a null entry, n == 0, a filter of
 * another k or on another device.  n == 1 is bt_find_paths_sample itself and allocates nothing; for n >= 2 the extra scratch copies and the per-(sample,
 * cluster) words are allocated on first need, kept, and replaced only by a call with a larger n (an allocation that fails is an error, the object stays usable). */
int bt_find_paths_samples(bt_find_paths *f, bt_bloom *const *sample_blooms, uint32_t n, const uint32_t *h_seeds);
/* device bytes a bt_find_paths_samples call with n samples would allocate beyond what the object already holds (0 for n == 1); no GPU call */
int bt_find_paths_batch_bytes(bt_find_paths *f, uint32_t n, uint64_t *bytes);
/* largest n a bt_find_paths_samples call had so far (0: none) and the device bytes held for batches; either pointer may be NULL (KmerCounter.cpp:59-103 has
 * no counterpart: the reference searches one sample at a time) */
int bt_find_paths_batch_info(bt_find_paths *f, uint32_t *largest_n, uint64_t *held_bytes);
/* best_paths_indices so far: h_num_paths[c] rows of |V_c| bytes each, clusters concatenated (bt_paths_batch::path_vertices layout) */
int bt_find_paths_sizes(bt_find_paths *f, uint32_t *h_num_paths, uint64_t *h_total_bytes);
int bt_find_paths_fetch(bt_find_paths *f, uint8_t *h_path_vertices);
/* How the search of VariantClusterGraph.cpp:389-798 is laid out on the device.  A cluster with at least wave_min_vertices vertices runs on a wavefront of
 * its own beside the launch that gives every other cluster a lane; the results are the same rows.  The threshold is BT_FIND_PATHS_WAVE_MIN, read when the
 * object is created: 0 = never (every cluster on a lane), 1 = every cluster on a wavefront, unset = the library's default.  max_candidate_paths: the largest
 * number of candidate paths a wavefront met at a vertex before filterPaths, over all bt_find_paths_sample calls so far (0 when no cluster took that route). */
typedef struct {
    uint32_t num_clusters, num_wave_clusters, wave_min_vertices, max_vertices, max_candidate_paths;
} bt_find_paths_stats;
int bt_find_paths_info(bt_find_paths *f, bt_find_paths_stats *out);

/* ------------------------------------------------------------------------------------------
 * Count model LUTs: CountDistribution (src/bayesTyper/CountDistribution.cpp:215-265)
 * ---------------------------------------------------------------------------------------- */
/* layout of the two caches the sampler reads through calcCountLogProb(sample, bias=0, multiplicity, count):
 *   genomic[(s*256 + multiplicity)*256 + count]   (CountDistribution.cpp:215-234; row multiplicity 0 is never read)
 *   noise[s*256 + count]                          (CountDistribution.cpp:236-253)
 * The host computes them in fp64 exactly as the reference does; the device only gathers. */

/* ------------------------------------------------------------------------------------------
 * Gibbs genotyping of variant-cluster groups:
 *   VariantClusterGroup::{initGenotyper, shuffleBranchOrdering, estimateGenotypes, getNoiseCounts,
 *   clearGenotyperCache, resetGroup, collectGenotypes} (include/bayesTyper/VariantClusterGroup.hpp:125-134)
 *   driven as InferenceEngine does (src/bayesTyper/InferenceEngine.cpp:60-133,278-333).
 *
 * Input = the per-cluster tensor bundle VariantClusterGraph::getHaplotypeCandidates produces
 * (VariantClusterHaplotypes, include/bayesTyper/VariantClusterHaplotypes.hpp:52-109), flattened.
 * All arrays are HOST memory and are copied by bt_gibbs_create.
 * ---------------------------------------------------------------------------------------- */
typedef struct bt_gibbs_params {
    uint32_t num_samples;                  /* S <= 30 */
    uint32_t seed;                         /* --random-seed */
    uint32_t num_chains;                   /* --number-of-gibbs-chains (20) */
    uint32_t burn_in;                      /* --gibbs-burn-in (100) */
    uint32_t num_iterations;               /* --gibbs-samples (250) */
    float kmer_subsampling_rate;           /* --kmer-subsampling-rate (0.1f) */
    uint32_t max_haplotype_variant_kmers;  /* --max-haplotype-variant-kmers (500) */
    uint32_t noise_seeding;                /* 0: genotyper seed = seed+(i+1)          (InferenceEngine.cpp:294)
                                              1: genotyper seed = seed+(i+1)*(c+1)    (InferenceEngine.cpp:70) */
    const uint8_t *gender;                 /* [S] 0 = female, 1 = male (Utils::Gender) */
} bt_gibbs_params;

typedef struct bt_gibbs_batch {
    uint32_t num_groups;     /* G */
    uint32_t num_clusters;   /* C = total number of group vertices */
    /* ---- per group ---- */
    const uint32_t *group_index;         /* [G] index i of the group in the unit's sorted group vector (seeds, Appendix B) */
    const uint32_t *group_cluster_off;   /* [G+1] vertices of group g are clusters [off[g], off[g+1]) in vertex order */
    const uint8_t *group_ploidy;         /* [G*S] chromosome ploidy per sample: 0 Null, 1 Haploid, 2 Diploid */
    const uint32_t *group_source_off;    /* [G+1] -> group_sources */
    const uint32_t *group_sources;       /* source vertices (local vertex ids), VariantClusterGroup.hpp:86 */
    const uint32_t *group_num_shared;    /* [G] number of multicluster k-mer records shared by the group's clusters */
    /* ---- per cluster (vertex) ---- */
    const uint32_t *cluster_idx;         /* [C] variant_cluster_idx (seed offset, nested-cluster identity) */
    const uint32_t *edge_off;            /* [C+1] out_edges CSR -> edges */
    const uint32_t *edges;               /* local vertex ids */
    const uint32_t *num_haplotypes;      /* [C] H */
    const uint32_t *num_variants;        /* [C] V */
    const uint32_t *kmer_off;            /* [C+1] k-mer rows of cluster c: [kmer_off[c], kmer_off[c+1]) */
    const uint8_t *hap_kmer_mult;        /* haplotype_kmer_multiplicities, row-major K x H per cluster, clusters concatenated */
    /* ---- per k-mer row (R = kmer_off[C]) ---- */
    const uint8_t *kmer_has_counts;      /* [R] KmerInfo::counts != nullptr */
    const uint8_t *kmer_counts;          /* [R*S] getSampleCount(s) */
    const uint8_t *kmer_ic_mult;         /* [R*2] getInterclusterMultiplicity(Female), (Male) */
    const int32_t *kmer_shared;          /* [R] -1, or index (< group_num_shared) of the shared record of a multicluster k-mer */
    const uint32_t *kv_off;              /* [R+1] variant_haplotype_indices CSR -> kv_var, kv_bits */
    const uint16_t *kv_var;              /* [NNZ] variant index */
    const uint32_t *kv_bits;             /* haplotype bitsets, ceil(H/32) words per entry, entries in kv order */
    /* ---- index lists ---- */
    const uint32_t *unique_off;          /* [C+1] -> unique_idx */
    const uint32_t *unique_idx;          /* unique_kmer_indices (row ids local to the cluster), first-seen order */
    const uint32_t *multi_off;           /* [C+1] -> multi_idx */
    const uint32_t *multi_idx;           /* multicluster_kmer_indices */
    /* ---- haplotypes / variants ---- */
    const uint16_t *hap_allele;          /* variant_allele_indices, row-major H x V per cluster, clusters concatenated */
    const uint32_t *hapnest_off;         /* [sum(H)+1] nested_variant_cluster_indices CSR per haplotype (sorted) */
    const uint32_t *hapnest_idx;
    const uint16_t *var_num_alleles;     /* [sum(V)] numberOfAlleles() incl. the missing allele */
    const uint8_t *var_has_dependency;   /* [sum(V)] */
    /* ---- nested_variant_cluster_dependency (VariantClusterHaplotypes.hpp:97) ---- */
    const uint32_t *nestdep_off;         /* [C+1] -> nestdep_cluster / nestdep_var_off */
    const uint32_t *nestdep_cluster;     /* child variant_cluster_idx */
    const uint32_t *nestdep_var_off;     /* [ND+1] -> nestdep_var */
    const uint16_t *nestdep_var;         /* variant indices, sorted descending (VariantClusterGraph.cpp:1130) */
} bt_gibbs_batch;

typedef struct bt_gibbs bt_gibbs;

int bt_gibbs_create(bt_ctx *ctx, const bt_gibbs_params *params, const bt_gibbs_batch *batch, bt_gibbs **out);
/* the device memory bt_gibbs_create would need for this batch (nothing is allocated): the host sizes its launches from it and
 * bt_ctx_info's free HBM (InferenceEngine.cpp:335-382 hands groups to its workers in batches; here a batch is what fits the GPU) */
int bt_gibbs_state_bytes(bt_ctx *ctx, const bt_gibbs_params *params, const bt_gibbs_batch *batch, uint64_t *bytes);
int bt_gibbs_destroy(bt_gibbs *g);
/* A batch's flat arrays held ON THE DEVICE, and samplers over any selection of its groups built from them without another pass through the host:
 * the reference keeps a unit's clusters in memory for the whole genotyping stage and constructs genotypers from them chain after chain
 * (InferenceEngine.cpp:60-75 initGenotypersCallback over the unit's groups, :172-211 the noise driver's subset per chain, :335-382 the group batches of
 * the default mode); here the unit goes to the GPU once (bt_gibbs_source_create: validated like bt_gibbs_create, uploaded, the caller's arrays are not
 * referenced afterwards) and every sampler — a noise chain's random subset, a launch-sized range of the unit — is laid out by the host from the
 * per-cluster dimensions alone and filled by the device from the resident arrays (bt_gibbs_create_from_source: group_ids = positions in the source
 * batch, in the order the sampler shall hold them; NULL = all groups; ctx = the context whose stream the sampler works on, NULL = the source's, same device).
 * bt_gibbs_create(batch) = source + sampler over all groups + source released. */
typedef struct bt_gibbs_source bt_gibbs_source;
int bt_gibbs_source_create(bt_ctx *ctx, uint32_t num_samples, const bt_gibbs_batch *batch, bt_gibbs_source **out);
/* The source of a unit whose candidates are on the device already (bt_paths_candidates_device): what VariantClusterGroup::initGenotyper does when it hands
 * getHaplotypeCandidates' bundle to the genotyper (VariantClusterGenotyper.cpp:59-106), with no host copy in between.  `structure` carries the per-group,
 * per-cluster, haplotype, variant and nested-dependency fields of bt_gibbs_batch (host memory; hap_allele / hapnest_* / nestdep_* as
 * bt_paths_candidates_fetch_small gives them); its per-row pointers, index lists, kmer_shared and group_num_shared must be NULL and come
 * from `p`, as kmer_off / unique_off / multi_off do (ignored here).  Cluster c of `structure` is cluster c of `p`.  The source TAKES the device arrays out of `p` (`p`
 * afterwards holds no candidates).  kmer_shared / group_num_shared are computed on the device: inside a group, walking its clusters in vertex order and
 * each cluster's multi_idx in order, distinct k-mers are numbered by first occurrence (KmerCounter.cpp:607-616).  On an error `p` keeps its candidates. */
int bt_gibbs_source_create_from_paths(bt_ctx *ctx, uint32_t num_samples, bt_paths *p, const bt_gibbs_batch *structure, bt_gibbs_source **out);
/* host arrays receiving a source's flat device arrays (NULL: skipped), in bt_gibbs_batch's layout, followed by the [G] / [C+1] arrays the source keeps on the host */
typedef struct bt_gibbs_source_arrays {
    uint8_t *group_ploidy;
    uint32_t *group_sources, *edges;
    uint8_t *hap_kmer_mult, *kmer_has_counts, *kmer_counts, *kmer_ic_mult;
    int32_t *kmer_shared;
    uint32_t *kv_off;
    uint16_t *kv_var;
    uint32_t *kv_bits, *unique_idx, *multi_idx;
    uint16_t *hap_allele;
    uint32_t *hapnest_off, *hapnest_idx;
    uint16_t *var_num_alleles;
    uint8_t *var_has_dependency;
    uint32_t *nestdep_cluster, *nestdep_var_off;
    uint16_t *nestdep_var;
    uint32_t *group_num_shared, *kmer_off, *unique_off, *multi_off;
} bt_gibbs_source_arrays;
/* diagnostic: h_counts[25] = number of elements of each of the 25 arrays above, in that order; out != NULL: the arrays are copied to the host (any source) */
int bt_gibbs_source_fetch(bt_gibbs_source *src, uint64_t *h_counts, const bt_gibbs_source_arrays *out);
int bt_gibbs_source_destroy(bt_gibbs_source *src);
int bt_gibbs_source_device_bytes(bt_gibbs_source *src, uint64_t *bytes);
int bt_gibbs_create_from_source(bt_gibbs_source *src, bt_ctx *ctx, const bt_gibbs_params *params, const uint32_t *group_ids, uint32_t num_groups, bt_gibbs **out);
int bt_gibbs_state_bytes_from_source(bt_gibbs_source *src, const bt_gibbs_params *params, const uint32_t *group_ids, uint32_t num_groups, uint64_t *bytes);
/* upload the count-model LUTs (see above); must be called before the first sweep and after every noise update */
int bt_gibbs_set_lut(bt_gibbs *g, const double *h_genomic /* [S*256*256] */, const double *h_noise /* [S*256] */);
int bt_gibbs_set_noise_lut(bt_gibbs *g, const double *h_noise /* [S*256] */);
/* initGenotyper (constructing the genotypers on first use) + shuffleBranchOrdering for every group,
 * with the seeds of chain `chain_idx` (InferenceEngine.cpp:292-295 / :60-75) */
int bt_gibbs_init_chain(bt_gibbs *g, uint32_t chain_idx);
/* estimateGenotypes(count_distribution, ploidy, collect_samples) `num_sweeps` times for every group */
int bt_gibbs_sweep(bt_gibbs *g, uint32_t num_sweeps, int collect_samples);
/* the whole default-mode schedule for every group: for each chain init_chain, burn_in sweeps without and
 * num_iterations sweeps with collection (InferenceEngine.cpp:292-306), in one launch */
int bt_gibbs_run(bt_gibbs *g);
/* getNoiseCounts of every group accumulated into a [S*256] histogram on the device, then clearGenotyperCache
 * (InferenceEngine.cpp:90-92); d_hist is zeroed first when zero_first != 0 */
int bt_gibbs_noise_counts(bt_gibbs *g, uint64_t *d_hist, int zero_first);
/* One iteration of the noise drivers with ONE host synchronisation (InferenceEngine.cpp:77-98): (the noise table of the previous
 * iteration, h_noise [S*256] or NULL, is uploaded without waiting;) one sweep of every group; the noise-count histogram of all groups
 * (+ clearGenotyperCache) lands in h_hist [S*256].  The caller draws the new rates from h_hist (after its all-reduce over the ranks) and
 * hands the rebuilt table to the next call. */
int bt_gibbs_noise_iteration(bt_gibbs *g, const double *h_noise, int collect_samples, uint64_t *h_hist);
/* A whole chain of a noise driver (InferenceEngine.cpp:135-276 estimateNoise, :384-472 estimateNoiseAndGenotypes; one iteration = :77-98) as ONE
 * resident launch: every tile keeps its workgroup — sampler state in registers / LDS — for the num_iterations iterations (collecting from iteration
 * first_collect on, 0-based), and the per-iteration exchange (noise-count histogram out, rebuilt noise table in) goes through a mailbox in pinned host
 * memory instead of a kernel launch + copies + a stream synchronisation per iteration.  The draws stay where they are exact: the caller takes the
 * histogram of iteration i from step i, reduces it over its ranks, draws the rates (CountDistribution::sampleNoiseParameters, CountDistribution.cpp:173-186:
 * libstdc++ / glibc) and hands the rebuilt table to step i + 1.
 *   begin: *resident = 1 when the chain was started this way; 0 (and BT_OK) when this batch cannot be (its workgroups do not fit the GPU together, or
 *          tiles with large dense tables want the whole-GPU refill between iterations): the caller then iterates with bt_gibbs_noise_iteration.
 *   step:  h_noise = the table for this iteration's sweep ([S*256]; NULL: unchanged; must be NULL for the first iteration, which runs with the table
 *          of bt_gibbs_set_lut / bt_gibbs_set_noise_lut); returns when this iteration's histogram is in h_hist [S*256] (caches cleared, :90-92).
 *   end:   after the last step (or earlier: the launch is told to stop at its next exchange); synchronises.  No other operation on g between begin and end.
 * Every wait on either side has a deadline (BT_NOISE_CHAIN_TIMEOUT_S, default 60 s): a stall is an error, never a hang. */
int bt_gibbs_noise_chain_begin(bt_gibbs *g, uint32_t num_iterations, uint32_t first_collect, int *resident);
int bt_gibbs_noise_chain_step(bt_gibbs *g, const double *h_noise, uint64_t *h_hist);
int bt_gibbs_noise_chain_end(bt_gibbs *g);
/* resetGroup for every group (InferenceEngine.cpp:100-113): genotypers are rebuilt by the next init_chain */
int bt_gibbs_reset_groups(bt_gibbs *g);
/* diagnostics: the frequency distribution every cluster's genotyper was constructed with, h_form[C]: 0 dense, 1 sparse with its zero and plus
 * sets as lists, 2 sparse with the sets as packed words (BT_GIBBS_NIBBLE_SETS, clusters of 3 .. 13 haplotypes), 0xFFFFFFFF not constructed yet */
int bt_gibbs_sparse_forms(bt_gibbs *g, uint32_t *h_form);

/* Results (collectGenotypes input): per cluster the diplotype sampling frequencies
 * (VariantClusterGenotyper.hpp:112) and the allele k-mer statistics (:104).
 * sizes: number of distinct sampled diplotypes over all clusters; number of (cluster, sample, allele) cells */
int bt_gibbs_result_sizes(bt_gibbs *g, uint64_t *num_diplotype_entries, uint64_t *num_allele_cells);
/* h_dip_off[C+1]; entry e: haplotypes (h_dip_h1[e] <= h_dip_h2[e], 0xFFFF = none), h_dip_freq[e*S + s];
 * allele cells in the order cluster, sample, variant, allele: h_stats[cell*12 + stat*4 + {count, fraction, mean, M2}]
 * for stat in {count_stats, fraction_stats, mean_stats} (KmerStats.cpp:107-121); h_cell_off[C+1] */
int bt_gibbs_result_fetch(bt_gibbs *g, uint64_t *h_dip_off, uint16_t *h_dip_h1, uint16_t *h_dip_h2, uint32_t *h_dip_freq,
                          uint64_t *h_cell_off, double *h_stats);
/* The same results as ONE string of 32-bit words in DEVICE memory, for the gather to rank 0 (bt_comm_gather_summaries) without a
 * host round trip — the reference's threads push their genotypes into one queue (InferenceEngine.cpp:335-382, 384-399); with
 * one process per GPU that queue is the gather.  Layout: [C, entries, cells, S], [entries, cells] per cluster, h1 | h2 << 16
 * per entry (order of bt_gibbs_result_fetch), counts [entry][S], one pad word if the count so far is odd, statistics
 * [cell][12] doubles.  *d_words belongs to the sampler (valid until the next call or bt_gibbs_destroy); complete on return. */
int bt_gibbs_result_words(bt_gibbs *g, const uint32_t **d_words, uint64_t *num_words);
/* Genotype summaries computed ON THE DEVICE: what VariantClusterGenotyper::getGenotypes (VariantClusterGenotyper.cpp:208-567) derives from the collected
 * samples — genotype / allele posteriors, allele filters, the call, AC / AF / AN / ACP, the non-covered alleles — for every variant of every cluster of the
 * launch, as ONE string of 32-bit words in DEVICE memory.  The string belongs to the sampler (valid until the next call or bt_gibbs_destroy) and is complete
 * on return, like bt_gibbs_result_words'; the sampler's state is not touched (bt_gibbs_result_fetch before and after returns the same arrays).
 * Floats are the host layer's bit for bit (same floatCompare / floatLess, same float sums divided by the number of collected sweeps, the diplotype entries
 * visited in bt_gibbs_result_fetch's order wherever the order can matter).  GQ is NOT in the string: (uint32_t)(-10 * log10(1 - best)) truncates at values
 * common posteriors sit on, so the reader derives it from `best` with its own log10 (99 if best compares equal to 1, 0 if to 0).
 * Layout (word offsets count from the start of the string; every record starts on an even word and has an even length):
 *   [0] C clusters  [1] NV variants of all clusters  [2] S  [3] 0
 *   cluster_var_off [C+1]: the variants of cluster c (the sampler's cluster order) are cluster_var_off[c] .. cluster_var_off[c+1]
 *   var_off [NV+1]: word offset of the record of variant v; var_off[NV] = *num_words (a reader may reorder clusters without recomputing sizes)
 *   one pad word if the count so far is odd
 *   per variant:  [0] A = numberOfAlleles() incl. the missing allele  [1] total_count (AN)  [2] max_alt_allele_call_probability (f32)  [3] has_dependency
 *                 per allele a < A, 4 words: allele call probability ACP (f32); alt allele count AC and alt allele frequency AF (f32) of allele a
 *                 (Genotypes::VariantStats' alt_allele_counts[a - 1]; 0 for a = 0); 1 if no haplotype candidate covers the allele (ANC), else 0
 *     then per sample: [0] chromosome ploidy of the cluster's group  [1] the genotype estimate: first | second << 16 (0xFFFF = no call; second unused for ploidy 1,
 *                 both for ploidy 0)  [2] best = the largest genotype posterior (f32)  [3] 0
 *                 genotype posteriors f32 [G]: G = A (A + 1) / 2 for ploidy 2 (alleles a <= b at b (b + 1) / 2 + a), A for ploidy 1, 0 for ploidy 0
 *                 allele posteriors f32 [A'], allele filter bits [A'] (1 = NAK, 2 = FAK) with A' = A, or 0 for ploidy 0
 *                 one pad word if the count so far is odd
 *                 k-mer means f64 [A][3]: KmerStats::getMean of the allele's count / fraction / mean statistics (-1 when nothing was added): NAK, FAK, MAC
 * Errors (each with a message): a null argument; a resident noise chain in flight; an overflowed diplotype table; more than 2^32 words; nothing collected
 * yet.  An error leaves nothing allocated that was not allocated before.  With BT_GIBBS_DEBUG set, a line on stderr tells how many cells visited their
 * entries in (h1, h2) order — the cells whose sample collected 83 887 sweeps or more, below which the order cannot matter; BT_GENOTYPES_ORDERED_FROM lowers
 * that threshold for tests. */
typedef struct bt_genotype_filters {
    float min_genotype_posterior;
    float min_number_of_kmers;
    const float *min_fraction_observed_kmers;   /* [S] */
} bt_genotype_filters;                           /* Filters.cpp:33-54 */
int bt_gibbs_genotypes(bt_gibbs *g, const bt_genotype_filters *f, const uint32_t **d_words, uint64_t *num_words);
/* The genotype-derived TEXT of the launch's VCF lines formatted ON THE DEVICE from a record string of bt_gibbs_genotypes: what GenotypeWriter formats on its
 * threads (GenotypeWriter.cpp:84-143 the allele fields, :202-230 writeVariantStats / writeAlleleCover, :261-345 writeSamples / writeAlleleKmerStats), byte for
 * byte as the host layer's stream insertions print it (bayestyper_amd/csrc/bt_genotype_text.hpp holds the formatter, shared by the kernels and the host).
 * Text: for every variant, in the string's variant order and contiguous, three pieces:
 *   stats    "AC=..;AF=..;AN=..;ACP=.."
 *   cover    ";ANC=.." with ascending alleles, or nothing
 *   samples  per sample "\tGT:" + a GQ slot of NO bytes + ":GPP:APP:NAK:FAK:MAC:SAF"; "\t:.:.:.:.:.:." for ploidy 0 (no slot)
 * GQ and QUAL are not in the text, for the reason given above: the reader derives GQ from the cell's `best` and QUAL / FILTER from the variant's
 * max_alt_allele_call_probability and total_count with its own log10, and splices GQ in at the slot.
 * Index (32-bit words):
 *   [0] C  [1] NV  [2] S  [3] number of not-covered variants     cluster_var_off [C+1]
 *   per variant, 9 words:  [0] [1] byte offset of its text (low, high word)  [2] [3] [4] lengths of the stats / cover / samples piece  [5] A  [6] total_count
 *                          [7] max_alt_allele_call_probability (f32)  [8] flags: 1 = not covered
 *   per cell (v * S + s), 2 words:  [0] best (f32)  [1] byte offset of the GQ slot inside the samples piece (0xFFFFFFFF: none)
 * Floats and doubles are printed exactly as printf's %g prints their value (precision 6, round half even) when 1e-27 <= |v| < 1e6 or v = 0.  Any other value
 * (non-finite, subnormal, outside that range) is NOT COVERED: nothing is printed for it, its variant is flagged and counted, and the caller must take that
 * variant's — in practice the launch's — text from the record string instead.  This is a condition, not a tolerance: the formatter never guesses.
 * bt_genotype_text_sizes: the exact sizes for a record string in device memory.  bt_genotype_text: text and index into the caller's device buffers;
 *   *text_bytes and *index_words are set first; a capacity that is too small is an error and nothing is written.  num_not_covered may be NULL.
 *   Errors: a null argument; a string whose tables or records do not have bt_gibbs_genotypes' layout (checked before anything is read through them);
 *   more than 2^32 index words.
 * bt_gibbs_genotype_text: bt_gibbs_genotypes, then the same passes; text and index belong to the sampler (valid until the next call or bt_gibbs_destroy) and
 *   are complete on return; the sampler's state is not touched; the errors are bt_gibbs_genotypes', with messages under this entry's name. */
int bt_genotype_text_sizes(bt_ctx *ctx, const uint32_t *d_words, uint64_t num_words, uint64_t *text_bytes, uint64_t *index_words);
int bt_genotype_text(bt_ctx *ctx, const uint32_t *d_words, uint64_t num_words, uint8_t *d_text, uint64_t text_capacity, uint32_t *d_index, uint64_t index_capacity,
                     uint64_t *text_bytes, uint64_t *index_words, uint32_t *num_not_covered);
int bt_gibbs_genotype_text(bt_gibbs *g, const bt_genotype_filters *f, const uint8_t **d_text, uint64_t *text_bytes, const uint32_t **d_index, uint64_t *index_words,
                           uint32_t *num_not_covered);
/* compact posterior summary on the DEVICE (input of the cross-GPU gather to rank 0): for cluster c, sample s
 * d_out[(c*S+s)*2] = h1 | h2<<16 of the most frequently sampled diplotype, d_out[(c*S+s)*2+1] = its frequency */
int bt_gibbs_posterior_summary(bt_gibbs *g, uint32_t *d_out);
/* diagnostics: the diplotype drawn for (cluster, sample) in each of the first `max_sweeps` sweeps after this call:
 * h_trace[(sweep*C + c)*S + s] = h1 | h2 << 16.  Pass max_sweeps = 0 to switch tracing off. */
int bt_gibbs_trace_enable(bt_gibbs *g, uint32_t max_sweeps);
int bt_gibbs_trace_fetch(bt_gibbs *g, uint32_t *h_trace, uint64_t max_words, uint64_t *num_sweeps_recorded);
/* device bytes held by this batch (state + inputs + the timeline's records while it is on) */
int bt_gibbs_device_bytes(bt_gibbs *g, uint64_t *bytes);

/* ------------------------------------------------------------------------------------------
 * Launch timeline (diagnostics, opt-in): when every wavefront of a sampling launch started and ended, and where it ran.
 * While a timeline is on and has room, a launch of bt_gibbs_run / bt_gibbs_sweep / bt_gibbs_init_chain runs the STAMPED sibling of each
 * sampling kernel (gibbs_*_kernel_tl): the same body between two reads of the wall clock, lane 0 of every wavefront writing one record
 * into a buffer nothing else reads.  With the timeline off (the default) no stamp executes and the launches are what they always were.
 * The noise tally, the fill kernels and the launches of a noise chain (bt_gibbs_noise_chain_begin .. _end) are never stamped.
 * ---------------------------------------------------------------------------------------- */
typedef struct bt_gibbs_timeline_record {     /* 48 bytes */
    uint64_t start_tick, end_tick;   /* wall_clock64(); end_tick 0: the wavefront never reached its end stamp */
    uint32_t hw_id, xcc_id;          /* raw HW_ID / XCC_ID registers, undecoded */
    uint32_t tile, wave;             /* tile of the sampler, wavefront within the tile */
    uint32_t launch;                 /* 0-based, counted over recorded launches since enable */
    uint16_t launch_class;           /* index of the launch class (hungriest first, the two-haplotype class last) */
    uint8_t kernel;                  /* 0 general, 1 hot, 2 simple, 3 single */
    uint8_t op;                      /* 0 bt_gibbs_run, 1 bt_gibbs_init_chain, 2 bt_gibbs_sweep */
    uint32_t groups;                 /* groups the tile holds, lockstep copies not counted */
    uint32_t lds_bytes;              /* the tile's own LDS need */
} bt_gibbs_timeline_record;
typedef struct bt_gibbs_timeline_summary_t {
    uint64_t records, unfinished;    /* selected records with / without an end stamp; everything below is over the former */
    uint64_t first_start, last_end;
    uint64_t busy_ticks;             /* sum of (end - start) */
    uint64_t peak_live;              /* max over t of live(t), live(t) = records with start <= t < end */
    uint64_t median_end;             /* end tick of the ceil(records / 2)-th record in ascending end order */
    uint64_t idle_after_median_ticks;/* sum over the ticks t of [median_end, last_end) of (peak_live - live(t)) */
    uint64_t last_record;            /* lowest index among the records with end = last_end (~0: no record) */
} bt_gibbs_timeline_summary_t;
/* room for max_launches launches (x the wavefronts of one launch over all launch classes), zero-filled; counters reset.  0: off, buffer released.
 * Each launch of a sampling operation takes one slot while slots remain (BT_GIBBS_STEPWISE: every launch of a bt_gibbs_run); later ones
 * run unstamped and are counted in `dropped`. */
int bt_gibbs_timeline_enable(bt_gibbs *g, uint32_t max_launches);
/* records bt_gibbs_timeline_fetch would hand out now, launches recorded, launches dropped, rate of the tick in kHz.  Any pointer may be NULL. */
int bt_gibbs_timeline_sizes(bt_gibbs *g, uint64_t *records, uint32_t *launches, uint32_t *dropped, uint32_t *tick_khz);
/* waits for the sampler's stream, then h_out[0 .. *n): the recorded launches in order, within a launch the classes in order, within a class the
 * wavefronts in slot order (slot = blockIdx.x * wavefronts per workgroup + wavefront of the workgroup; the empty slots of a packed launch are left out).
 * tile is what the wavefront reported, checked against the host's plan for its slot: a difference is an error, never a guess.  A capacity that is too
 * small is an error and nothing is written.  With the timeline off *n = 0. */
int bt_gibbs_timeline_fetch(bt_gibbs *g, bt_gibbs_timeline_record *h_out, uint64_t capacity, uint64_t *n);
/* host only, no GPU, exact (integer ticks): the summary of the records with the given launch and launch class (~0u: all) */
int bt_gibbs_timeline_summary(const bt_gibbs_timeline_record *r, uint64_t n, uint32_t launch, uint32_t launch_class, bt_gibbs_timeline_summary_t *out);

/* ------------------------------------------------------------------------------------------
 * The noise half of CountDistribution on the device (src/bayesTyper/CountDistribution.cpp:163-200 sampleNoiseParameters /
 * calcCountSuffStats, :314-352 the Poisson noise table with its tail fold) and a whole chain of a noise driver
 * (InferenceEngine.cpp:77-98 per iteration) without a host round trip per iteration.
 * bt_noise_rng = the run's generator as libstdc++ holds it: std::mt19937 (block form: 624 words + the index of the next word) and
 * the gamma distribution's normal distribution (its saved second variate).  The host exchanges it with its CountDistribution
 * before and after a chain, so host-side and device-side draws continue one stream.
 * ---------------------------------------------------------------------------------------- */
typedef struct bt_noise_rng {
    uint32_t mt[624];
    uint32_t mt_pos;             /* 0..624 (624: the next draw regenerates the block) */
    uint32_t saved_available;    /* std::normal_distribution::_M_saved_available */
    double saved;                /* std::normal_distribution::_M_saved */
} bt_noise_rng;
typedef struct bt_noise_model bt_noise_model;
/* h_prior[2*s], h_prior[2*s+1] = shape, scale of sample s's noise-rate prior (--noise-rate-prior, floats as the reference holds them) */
int bt_noise_model_create(bt_ctx *ctx, uint32_t num_samples, const float *h_prior, bt_noise_model **out);
int bt_noise_model_destroy(bt_noise_model *m);
int bt_noise_model_set_rng(bt_noise_model *m, const bt_noise_rng *h_rng);
int bt_noise_model_get_rng(bt_noise_model *m, bt_noise_rng *h_rng);
/* num_iterations iterations of a chain: { one sweep of every group of g (collecting from iteration first_collect on, 0-based);
 * noise counts of all groups + clearGenotyperCache; reduce(user, d_hist, S*256) if given — it must only ENQUEUE work on the context's
 * stream (bt_comm_allreduce_hist does); one gamma draw per sample from the model's generator (shape + sum of counts,
 * scale / (observations * scale + 1)); the rebuilt noise table becomes g's }.  Everything is enqueued at once; the call returns after
 * the last iteration with h_rates[it*S + s] = the rate drawn in iteration it.  g may be NULL (a rank without groups in this chain
 * still reduces and draws, so that all ranks' generators stay in step). */
int bt_gibbs_noise_chain(bt_gibbs *g, bt_noise_model *m, uint32_t num_iterations, uint32_t first_collect,
                         int (*reduce)(void *user, uint64_t *d_hist, uint64_t n), void *user, double *h_rates);

/* ------------------------------------------------------------------------------------------
 * Diagnostics: host-side entry points of the libstdc++-compatible primitives the sampler relies on
 * (SURVEY Appendix B.2).  They run the same __host__ __device__ code the kernels use.
 * ---------------------------------------------------------------------------------------- */
/* replay a sequence of operations on the unordered_set<uint> emulation: op[i] = 0 insert, 1 erase, 2 clear;
 * afterwards writes the iteration order to h_order (capacity universe) and its length to *n */
int bt_diag_uset_replay(uint32_t universe, const uint8_t *ops, const uint32_t *values, uint64_t num_ops, uint32_t *h_order, uint32_t *n);
/* the same replay on the packed form of the container (one 64-bit word of 4-bit fields; BT_GIBBS_NIBBLE_SETS), which holds universes of
 * 1 .. bt_diag_nset_max() elements and fails for any other.  Operations as above, plus 3: erase the element at position values[i] of the
 * iteration order, 4: read the element at position values[i] (both ignored at a position >= size).  h_at (capacity num_ops, may be NULL):
 * the element of an executed operation 3 or 4, 0xFFFFFFFF for every other operation. */
int bt_diag_nset_replay(uint32_t universe, const uint8_t *ops, const uint32_t *values, uint64_t num_ops, uint32_t *h_order, uint32_t *n, uint32_t *h_at);
uint32_t bt_diag_nset_max(void);
/* draws from the device random-number stack seeded like std::mt19937(seed): kind 0 raw u32, 1 generate_canonical<double,53>,
 * 2 gamma(shape=a, scale=b) with one persistent distribution object, 3 uniform_int(0, a), 4 bernoulli(float a),
 * 5 std::shuffle of 0..a-1 (h_out gets the permutation as doubles, n ignored) */
int bt_diag_rng(uint32_t seed, int kind, const double *a, const double *b, uint64_t n, double *h_out);
/* n Bernoulli(p) draws after `discard` words of a block-form ring generator seeded like std::mt19937(seed), taken three ways: call by call (form 0), by the
 * bulk routine the Gibbs chain start uses, as a team of one (1), and by the direct-form generator (2), each followed by eight more words.  ahead != 0: the
 * next block is twisted ahead first where the position allows it.  h_flags [3][n], h_tail [3][8], h_state [2][4] = {position in block, buffer flags, ring head,
 * unread ring words} of forms 0 and 1.  All three must agree. */
int bt_diag_bulk_bernoulli(uint32_t seed, uint64_t discard, uint32_t n, double p, uint32_t ring_cap, int ahead, uint8_t *h_flags, uint32_t *h_tail, uint32_t *h_state);
/* A probe of the generator stack itself (csrc/bt_rng_probe.hip; a test harness, no production path launches it).  A CASE is one wavefront: h_lane_gen
 * [num_cases][64] gives every lane the index of its generator in the case (0 .. 63) or -1 for a lane that leaves the kernel at once; the lanes that share
 * a generator are its `copies` lockstep copies g0 + k * (64 / copies) and run one program.  h_gens [num_cases][64]: seed (as std::mt19937(seed)), words
 * discarded first (at most 1 872), ring cap (8, 16, 32, 64), where the ring lies, and the generator's steps h_steps[step_off .. step_off + num_steps).
 * A step (n <= 2 048 repetitions; a, b, c, d as its kind says) writes its results to the lane's row of row_cap 32-bit words, a double as two words (low, high):
 *   DRAW n words with next() | TOPUP | REOPEN (mt_close, mt_ring_open) | CANONICAL n doubles | CANONICAL2 n pairs | UNIFORM_INT n draws of range a |
 *   BERNOULLI n flags of probability a | SHUFFLE of 0 .. n-1 (n <= 448) | NORMAL n draws | GAMMA n draws of shape a, scale b (both with one persistent
 *   NormalState; c != 0: one raw word after every draw) | BULK n Bernoulli(a) draws through rng_bernoulli_bulk by the generator's team: three words per draw
 *   {flag, ballot low, ballot high}, written by the lane emit() ran on | DIRECT n words of the direct-form generator of the same seed, a = 1, 2 or 4 at a
 *   time | SCREEN one call of the gamma second-test screen on u = a, n = b, v = c, a1 = d
 * and after every step two words {position | buffer flags, ring head | unread words << 16}.  Words no step wrote read 0xFFFFFFFF.  h_final [num_cases][64][12]:
 * {position, flags, head, unread} after the last step and eight more words of the stream.  A malformed program is an error, never a launch.
 * bt_diag_rng_probe runs the same interpreter on the host, every held generator once as a team of one: there rows and finals are indexed by GENERATOR. */
enum { BT_PROBE_DRAW = 0, BT_PROBE_TOPUP, BT_PROBE_REOPEN, BT_PROBE_CANONICAL, BT_PROBE_CANONICAL2, BT_PROBE_UNIFORM_INT, BT_PROBE_BERNOULLI, BT_PROBE_SHUFFLE,
       BT_PROBE_NORMAL, BT_PROBE_GAMMA, BT_PROBE_BULK, BT_PROBE_DIRECT, BT_PROBE_SCREEN, BT_PROBE_KINDS };
enum { BT_PROBE_RING_HBM = 0, BT_PROBE_RING_LDS = 1, BT_PROBE_RING_LDS_FLAT = 2 };   /* _LDS: LDS-typed pointer (mt_ring_open_as); _LDS_FLAT: generic pointer into LDS */
typedef struct bt_rng_probe_gen {
    uint32_t seed, discard, ring_cap, ring_place, step_off, num_steps, copies, reserved;
} bt_rng_probe_gen;
typedef struct bt_rng_probe_step {
    uint32_t kind, n;
    double a, b, c, d;
} bt_rng_probe_step;
int bt_rng_probe(bt_ctx *ctx, uint32_t num_cases, const int32_t *h_lane_gen, const bt_rng_probe_gen *h_gens, const bt_rng_probe_step *h_steps, uint64_t num_steps, uint32_t row_cap,
                 uint32_t *h_rows, uint32_t *h_final);
int bt_diag_rng_probe(uint32_t num_cases, const int32_t *h_lane_gen, const bt_rng_probe_gen *h_gens, const bt_rng_probe_step *h_steps, uint64_t num_steps, uint32_t row_cap,
                      uint32_t *h_rows, uint32_t *h_final);
/* Host-side run of the genotype summaries behind bt_gibbs_genotypes for ONE cluster given in host arrays (what bt_gibbs_result_fetch returns for it, entries
 * in that call's order; stats [(s * A_total + allele_base(v) + a) * 12]; ploidy [S] of the cluster's group): h_words receives the string bt_gibbs_genotypes
 * would produce for a launch of this one cluster, *num_words its length (an error when capacity is smaller; *num_words is set first). */
int bt_diag_genotype_cluster(uint32_t S, uint32_t H, uint32_t V, const uint16_t *hap_allele, const uint16_t *var_num_alleles, const uint8_t *var_has_dependency,
                             uint64_t num_diplotypes, const uint16_t *h1, const uint16_t *h2, const uint32_t *freq, const double *stats, const uint8_t *ploidy,
                             const bt_genotype_filters *f, uint32_t *h_words, uint64_t capacity, uint64_t *num_words);
/* Host-side run of bt_genotype_text (the same __host__ __device__ code, no GPU) over a record string in host memory; the capacity rule is bt_genotype_text's
 * (replaces GenotypeWriter.cpp:84-143,261-345 as that entry does). */
int bt_diag_genotype_text(const uint32_t *h_words, uint64_t num_words, uint8_t *h_text, uint64_t text_capacity, uint32_t *h_index, uint64_t index_capacity, uint64_t *text_bytes,
                          uint64_t *index_words, uint32_t *num_not_covered);
/* The number formatter alone: h_text16 [n * 16] receives the text of value i at 16 * i (zero padded), h_len [n] its length, or -1 with no text when the value
 * is not covered (operator<< of a double, i.e. printf's %g, in GenotypeWriter.cpp:130-143) */
int bt_diag_format_g6(const double *h_values, uint64_t n, char *h_text16, int32_t *h_len);
/* Host-side run of the container replay behind bt_paths_count_multigroup: n DISTINCT k-mers (2 x u64 each) are inserted, in the given
 * order, into an emulated libstdc++ std::unordered_set<std::bitset<2k>> that starts with `initial_buckets` buckets (1 = freshly
 * constructed; a set that was clear()ed keeps its bucket count); h_rank[i] = position of k-mer i in the set's iteration order,
 * *h_final_buckets = its bucket count afterwards: 13 for a fresh set that received at least one k-mer, as the real container reports (earlier versions
 * reported 1 for n = 1; the ranks were never affected).  (CPU tests compare it with the real container.) */
int bt_diag_kmer_set_order(const uint64_t *h_kmers, uint32_t n, uint64_t initial_buckets, unsigned k, uint32_t *h_rank, uint64_t *h_final_buckets);
/* The same result by the staged order the workgroup route of bt_paths_count_multigroup runs (KmerCounter.cpp:105-159), on the host without a GPU: the same
 * __host__ __device__ code with a team of one thread.  The bucket count comes from the stage plan alone.  initial_buckets (and the count the set grows to)
 * must stay below 2^32 - 2, as on the device route: an error otherwise. */
int bt_diag_kmer_set_order_staged(const uint64_t *h_kmers, uint32_t n, uint64_t initial_buckets, unsigned k, uint32_t *h_rank, uint64_t *h_final_buckets);
/* The hash both replays place a k-mer by: the library's restatement of libstdc++'s std::hash<std::bitset<2k>> of the k-mer (lo, hi), k in 1..64 (0 for any
 * other k).  The ranks expose it only modulo a bucket count.  (CPU tests compare it with the standard library's own hash at every k.) */
uint64_t bt_diag_std_hash_bitset(uint64_t lo, uint64_t hi, unsigned k);

/* ------------------------------------------------------------------------------------------
 * Deflate on the device (RFC 1951) and gzip files written through it (opt-in: BT_GZIP_ON_DEVICE=1 in the executables).
 * Replaces the gzip stream of GenotypeWriter.cpp (the reference's bgzip/boost gzip_compressor over the VCF text; here GenotypeWriter::finalise's single
 * gzwrite) and the gz outputs of main.cpp (parameter_kmers.fa.gz, intercluster_regions.txt.gz; here writeGzFile), which run on host threads.
 * The input is cut into pieces of 64 KiB; no piece carries history from the one before it; each becomes a dynamic-Huffman block (or stored blocks when
 * those are not larger) closed on a byte boundary by an empty stored block, so the pieces laid end to end are ONE raw deflate stream and the bytes are a
 * function of the content alone (bayestyper_amd/csrc/bt_deflate.hpp holds the compressor, one text for the kernels and the host).
 * ---------------------------------------------------------------------------------------- */
typedef struct bt_deflate_stats {
    uint64_t pieces, stored_pieces;            /* pieces of the content; those written as stored blocks */
    uint64_t literals, matches, matched_bytes; /* tokens of all pieces (the stored ones included); literals + matched_bytes = bytes_in */
    uint64_t bytes_in, bytes_out;              /* bytes_out: the deflate stream (bt_gzip_save: without the 18 bytes of header and trailer) */
    double seconds_h2d, seconds_kernels, seconds_d2h, seconds_host;   /* bt_gzip_save only: device time of the copies in, the kernels and the copies out
                                                                         (event pairs, summed over the slabs; they overlap), host time of CRC-32 + file writes */
} bt_deflate_stats;
/* the largest stream bt_deflate / bt_diag_deflate can produce for n bytes: 65551 per full piece, len + 10 (len + 5 for an empty content) for the rest */
int bt_deflate_bound(uint64_t n, uint64_t *capacity);
/* d_in [n] -> d_out: a raw deflate stream, ended by a final block when `last` is non-zero (otherwise it ends on a byte boundary and another call's
 * output continues it).  capacity must be at least bt_deflate_bound(n): a smaller one is an error, checked before anything is launched, and nothing is
 * written past it.  *h_out_bytes = the stream's length; stats may be NULL.  Complete on return. */
int bt_deflate(bt_ctx *ctx, const uint8_t *d_in, uint64_t n, int last, uint8_t *d_out, uint64_t capacity, uint64_t *h_out_bytes, bt_deflate_stats *stats);
/* h_data [n] -> the file `path` as ONE gzip member: writeGzFile's 10-byte header, the stream, CRC-32 and n mod 2^32.  The content goes through the device
 * in slabs (32 MiB; BT_GZIP_SLAB_BYTES overrides, rounded up to a multiple of the piece size) staged in pinned memory: copy in, kernels and copy out of
 * slab i run while the host computes slab i's CRC-32 (on `threads` threads, combined as crc32_combine does) and writes slab i - 1.  Written as
 * <path>.tmp and renamed when complete.  The bytes do not depend on the slab size or the thread count.  64-bit sizes throughout. */
int bt_gzip_save(bt_ctx *ctx, const char *path, const uint8_t *h_data, uint64_t n, uint32_t threads, bt_deflate_stats *stats);
/* Host-side run of bt_deflate (the same __host__ __device__ code with a team of one thread, no GPU): the same bytes, the same capacity rule. */
int bt_diag_deflate(const uint8_t *h_in, uint64_t n, int last, uint8_t *h_out, uint64_t capacity, uint64_t *out_bytes, bt_deflate_stats *stats);

/* ------------------------------------------------------------------------------------------
 * BGZF on the device (SAM specification section 4.1: a series of self-contained gzip members of at most 64 KiB, the format tabix and bcftools index),
 * opt-in: BT_VCF_BGZF=1 with `bayesTyper genotype -z`.  Replaces the bgzip pass a user runs over the unit's VCF before tabix / bcftools concat.
 * The content is cut into blocks of 65280 input bytes (htslib's size; the last one shorter, none for an empty content).  A block is 18 bytes of header
 * (1f 8b 08 04, mtime 0, XFL 0, OS ff, XLEN 6, "BC" 02 00, BSIZE = the block's size - 1), the payload — the piece compressor above with the final bit
 * set, a complete raw deflate stream of at most 65290 bytes — then the CRC-32 of the block's input, computed by the wavefront that compressed it, and its
 * length.  bayestyper_amd/csrc/bt_bgzf.hpp holds the block's code, one text for the kernels and the host.  bt_deflate_stats: pieces = blocks,
 * bytes_out = the payloads without the 26 bytes of framing per block and without the EOF block.
 * ---------------------------------------------------------------------------------------- */
/* the largest stream for n bytes, the 28 bytes of the EOF block included (len + 36 per block), and the number of data blocks */
int bt_bgzf_bound(uint64_t n, uint64_t *capacity, uint64_t *blocks);
/* d_in [n] -> d_out: the data blocks, then with `eof` non-zero the canonical 28-byte EOF block (a constant, not the compressor's empty piece).
 * h_block_offsets [blocks + 1] (may be NULL): the byte offset of every block; the last entry is the EOF block's offset, or the stream's end without one.
 * capacity must be at least bt_bgzf_bound(n): a smaller one is an error, checked before anything is launched, and nothing is written past it.
 * *h_out_bytes = the stream's length; stats may be NULL.  Complete on return. */
int bt_bgzf(bt_ctx *ctx, const uint8_t *d_in, uint64_t n, int eof, uint8_t *d_out, uint64_t capacity, uint64_t *h_out_bytes, uint64_t *h_block_offsets, bt_deflate_stats *stats);
/* h_data [n] -> the file `path` as BGZF with its EOF block: bt_gzip_save's slab pipeline with a slab that is a multiple of 65280 (default 515 blocks,
 * about 32 MiB; BT_BGZF_SLAB_BYTES overrides, rounded up), without a host CRC (`threads` is accepted for symmetry and unused), and with
 * h_block_offsets [blocks + 1] (may be NULL; offsets_capacity entries of room, an error when too few) relative to the file.  Written as <path>.tmp and
 * renamed when complete.  The bytes do not depend on the slab size or on `threads`.  64-bit sizes throughout. */
int bt_bgzf_save(bt_ctx *ctx, const char *path, const uint8_t *h_data, uint64_t n, uint32_t threads, uint64_t *h_block_offsets, uint64_t offsets_capacity, bt_deflate_stats *stats);
/* Host-side run of bt_bgzf (the same __host__ __device__ code with a team of one thread, no GPU): the same bytes and offsets, the same capacity rule. */
int bt_diag_bgzf(const uint8_t *h_in, uint64_t n, int eof, uint8_t *h_out, uint64_t capacity, uint64_t *out_bytes, uint64_t *h_block_offsets, bt_deflate_stats *stats);
/* Host-side run of the blocks' CRC-32 routine: zlib's crc32 of h_in [n] (contents longer than a block: per block, joined as crc32_combine does). */
int bt_diag_crc32(const uint8_t *h_in, uint64_t n, uint32_t *crc);

/* ------------------------------------------------------------------------------------------
 * BAM samples on the device: BGZF read (SAM specification section 4.1) and alignment records -> reads text (section 4.2).
 * Replaces the `samtools fastq` a user would run before the reads route (bt_reads_count / bt_reads_make_bloom / bt_reads_sketch) can take the BAM the
 * reference's workflow counts with `kmc -fbam`.  bayestyper_amd/csrc/bt_inflate.hpp holds the decoder (stored, fixed and dynamic blocks, several per
 * BGZF block), bayestyper_amd/csrc/bt_bam.hpp the record's code, each one text for the kernels and the host.  One BGZF block per wavefront; no
 * workgroup waits on another.  Damaged input is an error naming the block or the record, never a fault: every load is bounded by the block's payload,
 * every store by its ISIZE.
 * ---------------------------------------------------------------------------------------- */
typedef struct bt_bgzf_block {
    uint64_t in_offset;    /* the block's first byte in the input buffer */
    uint64_t out_offset;   /* where its data goes in the output: the sum of the ISIZEs before it */
    uint32_t in_size;      /* the whole block: BSIZE + 1 (SAM 4.1) */
    uint32_t isize;        /* its data's length, at most 65536 (SAM 4.1: ISIZE) */
} bt_bgzf_block;
/* Host only, no GPU.  h_in [n] starts at a block boundary -> h_blocks (may be NULL: the blocks are counted; else at most blocks_capacity are taken) for
 * every WHOLE block, *consumed = the bytes they take, *out_bytes = the sum of their ISIZEs.  Every header field is checked (SAM 4.1: ID1 ID2, CM = 8,
 * FLG = 4, the BC subfield of two bytes inside XLEN, BSIZE no smaller than header + trailer, ISIZE <= 65536): a violation is an error naming the block's
 * offset.  A trailing partial block is not consumed and is no error. */
int bt_bgzf_scan_blocks(const uint8_t *h_in, uint64_t n, bt_bgzf_block *h_blocks, uint64_t blocks_capacity, uint64_t *n_blocks, uint64_t *consumed, uint64_t *out_bytes);
/* d_in [in_bytes] and d_blocks [n_blocks] (a table of bt_bgzf_scan_blocks, in device memory) -> d_out: each block's data at its out_offset (SAM 4.1), its
 * CRC-32 checked against the trailer.  out_bytes = the table's total; capacity below it is an error before any launch, and nothing is written at or past
 * out_bytes: an entry that reaches outside d_in or out_bytes fails as a block.  The first failing block (smallest index) is the error, as
 * "BGZF block at offset <file_offset + in_offset>: <condition>"; the other blocks' data is written all the same.  Complete on return. */
int bt_bgzf_inflate(bt_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes, const bt_bgzf_block *d_blocks, uint64_t n_blocks, uint8_t *d_out, uint64_t capacity, uint64_t out_bytes,
                    uint64_t file_offset);
/* Host-side run of bt_bgzf_inflate (SAM 4.1; the same __host__ __device__ code with a team of one thread, no GPU): the same bytes, the same message. */
int bt_diag_bgzf_inflate(const uint8_t *h_in, uint64_t in_bytes, const bt_bgzf_block *h_blocks, uint64_t n_blocks, uint8_t *h_out, uint64_t capacity, uint64_t out_bytes,
                         uint64_t file_offset);

typedef struct bt_bam_stats {
    uint64_t kept, skipped, bases;   /* records written to the text, records left out by skip_flags, bases of the kept records */
} bt_bam_stats;
/* d_bam [len] (inflated BAM, SAM 4.2, from a record boundary on; len < 4 GiB - 1) -> d_text: for every WHOLE record with flag & skip_flags == 0, in record
 * order, its l_seq bases and '\n' (4-bit codes 1 2 4 8 -> A C G T, every other code -> N; l_seq = 0 gives an empty line; nothing is reverse-complemented).
 * *consumed = the offset of the first record that is not whole; *text_bytes = the text's length; capacity >= len always suffices, a smaller one that
 * does not is an error and nothing is written past it.  A record whose block_size is below 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq,
 * or whose l_seq is negative, is an error naming its offset (the one at the smallest offset).  stats may be NULL.  Complete on return. */
int bt_bam_reads_text(bt_ctx *ctx, const uint8_t *d_bam, uint64_t len, uint32_t skip_flags, char *d_text, uint64_t capacity, uint64_t *text_bytes, uint64_t *consumed,
                      bt_bam_stats *stats);
/* Host-side run of bt_bam_reads_text (SAM 4.2; the same record code, no GPU): the same text, numbers and message. */
int bt_diag_bam_reads_text(const uint8_t *h_bam, uint64_t len, uint32_t skip_flags, char *h_text, uint64_t capacity, uint64_t *text_bytes, uint64_t *consumed, bt_bam_stats *stats);

/* The stream object (SAM 4.1 + 4.2): a BAM file's compressed blocks in slabs -> reads text on the device.  max_in_bytes (64 KiB .. 1 GiB): the largest slab.
 * The slabs go through the context's pinned staging slots (taken when they are large enough, handed back by _destroy). */
typedef struct bt_bam_scan bt_bam_scan;
int bt_bam_scan_create(bt_ctx *ctx, uint64_t max_in_bytes, uint32_t skip_flags, bt_bam_scan **out);
/* h_blocks [n_bytes]: WHOLE BGZF blocks in host memory (SAM 4.1; a slab that ends inside a block is an error), in file order from call to call.  They are
 * inflated behind the tail the previous call left (the record that was not whole) and turned into text: *d_text [*text_len] is device memory, valid until
 * the next call on this object, and fit for bt_reads_count / bt_reads_make_bloom / bt_reads_sketch as it stands (whole reads, no halo needed).
 * skip_first_bytes (first call only): decompressed bytes to step over, the BAM header's; a header longer than the first slab runs on into the next.
 * Blocks with ISIZE 0 (the EOF block, empty blocks mid-file) are legal anywhere.  A record of more than 8 x max_in_bytes bytes is refused.  A slab whose
 * data, with the carried tail, would reach 4 GiB is refused with a message that asks for smaller slabs.  stats (may be
 * NULL): this call's.  After an error the object can only be destroyed.  Complete on return. */
int bt_bam_scan_text(bt_bam_scan *scan, const uint8_t *h_blocks, uint64_t n_bytes, uint64_t skip_first_bytes, const char **d_text, uint64_t *text_len, bt_bam_stats *stats);
/* SAM 4.2: the file has to end at a record boundary: an error when part of a record (or of the header) is left over — a truncated file. */
int bt_bam_scan_finish(bt_bam_scan *scan);
void bt_bam_scan_destroy(bt_bam_scan *scan);

/* ------------------------------------------------------------------------------------------
 * BGZF-compressed FASTQ samples on the device: BGZF read (as above) and FASTQ records -> reads text.  The FASTQ files a sequencer's converter or `bgzip`
 * writes are concatenated gzip members with the BC subfield, which bt_bgzf_inflate takes as they are.  bayestyper_amd/csrc/bt_fastq.hpp holds the grammar
 * (that of the host's ReadsFile), one text for the kernels and the host:
 *   lines end at '\n', one trailing '\r' is stripped; a record is '@' header, bases, '+' line, as many quality values as bases; a blank line (empty, or a
 *   lone '\r') is skipped only where a record's first line is expected, anywhere else it is that line of the record; the file's last line needs no newline.
 * A violation is an error with the 1-based line number in the file (blank lines count) and ReadsFile's words:
 *   "line N: a FASTQ record must start with '@' (a missing line?)", "line N: the third line of a FASTQ record must start with '+' (a missing line?)",
 *   "FASTQ record ending at line N: X bases but Y quality values (a missing line?)", "truncated FASTQ record at the end of the file (n of 4 lines)";
 * of several the one at the smallest line.
 * ---------------------------------------------------------------------------------------- */
typedef struct bt_fastq_stats {
    uint64_t reads, bases, lines;   /* records with at least one base, their sequence bytes, lines consumed (skipped blank lines included) */
} bt_fastq_stats;
/* d_fastq [len] (FASTQ text from a record boundary on; len < 4 GiB - 1) -> d_text: for every WHOLE record with at least one base, in record order, its
 * sequence bytes verbatim and '\n' (no case folding, no N mapping: the consumers' nt_code does that); a record without bases writes nothing.
 * final == 0: a record is whole when the newline of its fourth line is there; *consumed = the offset of the first record that is not whole (blank lines
 * in front of it are consumed); that record is judged by the complete lines that are there of it.  final == 1: the data is the file's end: a last line
 * without a newline is a line, a record of 1 to 3 lines is the "truncated" error, *consumed == len on success.  first_line: the file's line number of
 * d_fastq[0].  capacity >= len always suffices, a smaller one that does not is an error; nothing is written at or past capacity, or past *text_bytes.
 * stats may be NULL.  Complete on return. */
int bt_fastq_reads_text(bt_ctx *ctx, const char *d_fastq, uint64_t len, int final, uint64_t first_line, char *d_text, uint64_t capacity, uint64_t *text_bytes, uint64_t *consumed,
                        bt_fastq_stats *stats);
/* Host-side run of bt_fastq_reads_text (the same line code, no GPU): the same text, numbers and message. */
int bt_diag_fastq_reads_text(const char *h_fastq, uint64_t len, int final, uint64_t first_line, char *h_text, uint64_t capacity, uint64_t *text_bytes, uint64_t *consumed,
                             bt_fastq_stats *stats);
/* Bytes per workgroup of the kernels that find the lines (tiles are counted from d_fastq[0]): where a test puts its line ends. */
uint32_t bt_fastq_count_tile(void);

/* The stream object, the twin of bt_bam_scan: a BGZF FASTQ file's compressed blocks in slabs -> reads text on the device.  max_in_bytes (64 KiB .. 1 GiB):
 * the largest slab.  The slabs go through the context's pinned staging slots (taken when they are large enough, handed back by _destroy). */
typedef struct bt_fastq_scan bt_fastq_scan;
int bt_fastq_scan_create(bt_ctx *ctx, uint64_t max_in_bytes, bt_fastq_scan **out);
/* h_blocks [n_bytes]: WHOLE BGZF blocks in host memory (a slab that ends inside a block is an error), in file order from call to call, from the file's
 * first block on.  They are inflated behind the tail the previous call left (the record that was not whole) and turned into text: *d_text [*text_len] is
 * device memory, valid until the next call on this object, and fit for bt_reads_count / bt_reads_make_bloom / bt_reads_sketch as it stands.  Blocks with
 * ISIZE 0 are legal anywhere.  A tail of more than 8 x max_in_bytes (a record longer than a slab may hold) is refused.  A slab whose data, with the
 * carried tail, would reach 4 GiB is refused with a message that asks for smaller slabs.  stats (may be NULL): this call's.  After an error the object
 * can only be destroyed.  Complete on return. */
int bt_fastq_scan_text(bt_fastq_scan *scan, const uint8_t *h_blocks, uint64_t n_bytes, const char **d_text, uint64_t *text_len, bt_fastq_stats *stats);
/* The carried tail judged as the file's end (final == 1) -> its text, which may be empty (*d_text is then NULL). */
int bt_fastq_scan_finish(bt_fastq_scan *scan, const char **d_text, uint64_t *text_len, bt_fastq_stats *stats);
void bt_fastq_scan_destroy(bt_fastq_scan *scan);

/* ------------------------------------------------------------------------------------------
 * Ordinary gzip FASTQ samples on the device: ONE long gzip member (gzip, pigz, `fasterq-dump | gzip`) inflated by many wavefronts at once, then the FASTQ
 * parse above.  Replaces zlib's `inflate` under the host's ReadsFile, one thread per file.  bayestyper_amd/csrc/bt_gunzip.hpp holds the algorithm, one text
 * for the kernels and the host (the two-stage scheme of pugz and rapidgzip): plausible dynamic block headers are searched at every bit offset, the first of
 * every chunk_bytes of input starts a team that decodes to 16-bit symbols (a byte, or a marker for a byte of the 32 KiB before its start, which it does
 * not know); a team's output is used only when the team before it ended exactly where it started, so the bytes are those of a serial inflate whatever the
 * guesses were.  Damaged input is an error naming the block ("deflate block at offset <byte> (bit <0..7>): <condition>"), never a fault or a hang.
 * ---------------------------------------------------------------------------------------- */
typedef struct bt_gunzip_stats {
    uint64_t rounds;           /* decode launches of team 0 (the candidates' teams are decoded once per call) */
    uint64_t candidates;       /* chunks behind the start's in which a plausible header was found */
    uint64_t links_verified;   /* candidates' teams taken: the team before ended exactly at their start */
    uint64_t links_broken;     /* rounds that ended because a team did not end at the next start (a false candidate, a team out of room) */
    uint64_t blocks, out_bytes;
} bt_gunzip_stats;
/* Replaces zlib's inflate (raw deflate, windowBits -15) under ReadsFile.  d_in [in_bytes] (at most 128 MiB): a raw deflate stream, or a part of one;
 * start_bit: a block boundary in it; d_window [window_bytes <= 32768]: the output that precedes start_bit (none at a stream's start: a distance reaching
 * before it is an error); chunk_bytes: 0 = the default, at least 1024.  Whole blocks are decoded from start_bit into d_out: after the final block
 * *stream_end = 1 and *end_bit is the bit behind it; otherwise *end_bit is the last block boundary whose next block is not whole inside the input or would
 * not fit capacity (at most 1 GiB is produced per call).  Zero progress is a result (*out_bytes = 0, *end_bit = start_bit), not an error.  Nothing is
 * written at or past capacity.  *crc32: zlib's crc32 of the bytes produced.  stats may be NULL.  The bytes, *end_bit, *stream_end and *crc32 do not depend on
 * chunk_bytes.  Complete on return. */
int bt_inflate_raw(bt_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes, uint64_t start_bit, const uint8_t *d_window, uint64_t window_bytes, uint32_t chunk_bytes, uint8_t *d_out,
                   uint64_t capacity, uint64_t *out_bytes, uint64_t *end_bit, int *stream_end, uint32_t *crc32, bt_gunzip_stats *stats);
/* Host-side run of bt_inflate_raw (replaces the same zlib inflate; the same __host__ __device__ code with a team of one thread and host pointers, no GPU):
 * the same bytes, *end_bit, message and stats, which are functions of the input and the parameters alone. */
int bt_diag_inflate_raw(const uint8_t *h_in, uint64_t in_bytes, uint64_t start_bit, const uint8_t *h_window, uint64_t window_bytes, uint32_t chunk_bytes, uint8_t *h_out, uint64_t capacity,
                        uint64_t *out_bytes, uint64_t *end_bit, int *stream_end, uint32_t *crc32, bt_gunzip_stats *stats);
/* The find stage's test alone, on the host (no GPU): h_flags[i] = 1 when a plausible non-final dynamic block header starts at bit first_bit + i of
 * h_in [in_bytes], else 0, for i < n_bits; first_bit + n_bits <= 8 * in_bytes.  What gunzip_find_kernel asks of every bit offset, for the tests. */
int bt_diag_gunzip_plausible(const uint8_t *h_in, uint64_t in_bytes, uint64_t first_bit, uint64_t n_bits, uint8_t *h_flags);
/* What chunk_bytes = 0 stands for, and the symbols of room a candidate's team has per compressed byte of its span. */
uint32_t bt_gunzip_default_chunk_bytes(void);
uint32_t bt_gunzip_expansion_budget(void);
/* Wall seconds this process has spent in the stages of bt_inflate_raw and bt_fastq_gz_scan_text -> seconds5 (may be NULL): find, decode, windows, resolve,
 * crc; reset != 0 zeroes them.  The windows and resolve stages are told apart only when BT_GUNZIP_STAGE_TIMES is set (it adds a synchronisation). */
void bt_diag_gunzip_stage_seconds(double *seconds5, int reset);

/* The stream object, the twin of bt_fastq_scan for a gzip file that is not BGZF (replaces zlib's inflate and gzread under ReadsFile).  max_in_bytes
 * (64 KiB .. 64 MiB): the most a call hands in.  The object parses each member's RFC 1952 header on the host (FEXTRA, FNAME, FCOMMENT, FHCRC), carries the
 * compressed bytes not consumed yet, the bit offset, the 32 KiB window and the running CRC-32 and length, checks each member's trailer (CRC-32 and ISIZE)
 * and goes on into a following member. */
typedef struct bt_fastq_gz_scan bt_fastq_gz_scan;
int bt_fastq_gz_scan_create(bt_ctx *ctx, uint64_t max_in_bytes, uint32_t chunk_bytes /* 0 = default */, bt_fastq_gz_scan **out);
/* h_bytes [n_bytes]: any cut of the file, in file order from call to call.  Every whole deflate block the carried bytes hold is inflated behind the FASTQ
 * tail the previous call left and turned into text as bt_fastq_scan_text does: *d_text [*text_len] is device memory, valid until the next call on this
 * object.  A deflate block that is not whole within max_in_bytes of carried input, or that inflates to more than 8 x max_in_bytes, is refused with a
 * message that says so.  A damaged member is an error naming the member's and the block's file offsets.  stats (may be NULL): this call's.  After an error
 * the object can only be destroyed.  Complete on return. */
int bt_fastq_gz_scan_text(bt_fastq_gz_scan *scan, const uint8_t *h_bytes, uint64_t n_bytes, const char **d_text, uint64_t *text_len, bt_fastq_stats *stats);
/* Fails with "truncated gzip file" unless the file ended at a member boundary; then the carried FASTQ tail is judged as bt_fastq_scan_finish does. */
int bt_fastq_gz_scan_finish(bt_fastq_gz_scan *scan, const char **d_text, uint64_t *text_len, bt_fastq_stats *stats);
/* The sums of the inflate calls' stats so far. */
int bt_fastq_gz_scan_stats(const bt_fastq_gz_scan *scan, bt_gunzip_stats *stats);
void bt_fastq_gz_scan_destroy(bt_fastq_gz_scan *scan);

#ifdef __cplusplus
}
#endif
#endif /* BTGPU_H */
