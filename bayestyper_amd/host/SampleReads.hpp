// Every read file of <prefix>.reads to the consumers of the reads scan (include/btgpu.h: bt_reads_*), whatever its format.  A file is told by its content, not by
// its name: a BAM (BamFile::isBam) goes through the stream object of libbtgpu — compressed blocks in, reads text in device memory out (bt_bam_scan_text) — and
// reaches `device_text`; so does a FASTQ compressed as BGZF (isBgzfFastq; bt_fastq_scan_text), unless BT_FASTQ_BGZF_ON_HOST=1 sends it the old way, and, only
// with BT_FASTQ_GZIP_ON_DEVICE=1, a FASTQ that is ordinary gzip (isGzipFastq, isBgzfFastq's counterpart for one long member; bt_fastq_gz_scan_text); every other
// file is read as FASTA / FASTQ on the host (forEachReadsSlab) and reaches `host_slab`, as before BAM was taken.
// Before any of that the sample's reads pack is looked for (ReadsPack.hpp): when <prefix>.reads.pack is there, whole and made from what this run names, no read
// file is opened and its sections reach `host_packed`; with BT_READS_PACK=1 a pass over the files that found no such pack writes one as it goes.
#pragma once
#include <functional>
#include <iostream>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/btgpu.h"
#include "BamFile.hpp"
#include "GzipFile.hpp"
#include "Options.hpp"
#include "ReadsFile.hpp"
#include "ReadsPack.hpp"

namespace bthost {

struct ReadsSinks {
    std::function<void(const std::string &)> host_slab;              // a slab of reads text in host memory
    std::function<void(const char *, uint64_t)> device_text;         // reads text in device memory, valid until the call returns
    std::function<void(const uint8_t *, uint64_t)> host_packed;      // (bytes, positions): a section of the reads pack in host memory; unset: the pack is not looked for
};

// for the BT_STAGE_TIMES rows of the reads route: which of the files went through a stream object of the device
inline std::string deviceRouteNote(size_t bam_files, size_t bgzf_fastq_files, size_t gzip_fastq_files = 0) {
    std::string note;
    if (bam_files) note += " (" + std::to_string(bam_files) + " BAM file(s) on the device)";
    if (bgzf_fastq_files) note += " (" + std::to_string(bgzf_fastq_files) + " BGZF FASTQ file(s) on the device)";
    if (gzip_fastq_files) note += " (" + std::to_string(gzip_fastq_files) + " gzip FASTQ file(s) on the device)";
    return note;
}

// ReadsTotals of a BAM file: bases and reads of the kept records (flag & skip_flags == 0), slabs = calls of bt_bam_scan_text; of a BGZF FASTQ file: bases and
// reads of the records with at least one base, slabs = calls of bt_fastq_scan_text; of a gzip FASTQ file the same, slabs = calls of bt_fastq_gz_scan_text
// *bam_files, *bgzf_fastq_files, *gzip_fastq_files (may be NULL): how many of the list's files were BAM files, BGZF-compressed FASTQ files and ordinary gzip
// FASTQ files read on the device
inline ReadsTotals forEachSampleReads(bt_ctx *ctx, const std::string &prefix, unsigned kmer_size, unsigned threads, size_t slab_bytes, const ReadsSinks &sinks,
                                      size_t *bam_files = nullptr, size_t *bgzf_fastq_files = nullptr, size_t *gzip_fastq_files = nullptr, bool *from_pack = nullptr) {
    if (from_pack) *from_pack = false;
    if (sinks.host_packed) {
        if (std::unique_ptr<ReadsPackReader> pack = ReadsPackReader::openFor(prefix, kmer_size)) {
            if (bam_files) *bam_files = 0;
            if (bgzf_fastq_files) *bgzf_fastq_files = 0;
            if (gzip_fastq_files) *gzip_fastq_files = 0;
            if (from_pack) *from_pack = true;
            std::cout << "[" << getLocalTime() << "] Reading the reads of " << prefix << ".reads from the reads pack " << pack->path() << std::endl;
            const ReadsPackTotals t = pack->forEachSection(sinks.host_packed);
            ReadsTotals totals;
            totals.bases = t.bases;
            totals.reads = t.reads;
            totals.slabs = t.sections;
            totals.files = readReadsList(prefix).size();   // (the list file; no read file is opened)
            return totals;
        }
    }
    std::vector<std::string> bams, fastqs, gzips, texts;
    const bool fastq_on_host = fastqBgzfOnHost(), gzip_on_device = fastqGzipOnDevice();
    for (const std::string &f : readReadsList(prefix))
        (BamFile::isBam(f) ? bams : !fastq_on_host && isBgzfFastq(f) ? fastqs : gzip_on_device && isGzipFastq(f) ? gzips : texts).push_back(f);
    ReadsTotals totals;
    // BT_READS_PACK=1 and no pack that serves: this pass writes one (device texts are packed where they are, host slabs on the threads that read them)
    std::unique_ptr<ReadsPackWriter> writer;
    if (sinks.host_packed && readsPackWanted()) writer.reset(new ReadsPackWriter(ctx, prefix, kmer_size, !bams.empty()));
    auto deliverDevice = [&](const char *d_text, uint64_t len, uint64_t bases, uint64_t reads) {
        if (len) sinks.device_text(d_text, len);
        if (writer && (len || bases || reads)) writer->addDeviceText(d_text, len, bases, reads);
    };
    if (bam_files) *bam_files = bams.size();
    if (bgzf_fastq_files) *bgzf_fastq_files = fastqs.size();
    if (gzip_fastq_files) *gzip_fastq_files = gzips.size();
    const size_t bgzf_slab = std::max<size_t>(slab_bytes / 2, 65536);   // compressed bytes: about a quarter of the text they hold
    auto check = [](int rc, const std::string &file) {
        if (rc != BT_OK) throw std::runtime_error("read file " + file + ": " + bt_last_error());
    };
    auto warnNoEof = [](const BgzfFile &file, const std::string &f) {
        static std::set<std::string> warned;   // once per file and process: makeBloom -r reads a file in two passes
        if (!file.hasEofBlock() && warned.insert(f).second) std::cerr << "WARNING: read file " << f << " has no BGZF end-of-file block: it may be truncated" << std::endl;
    };
    if (!bams.empty()) {
        const uint32_t skip_flags = bamSkipFlags();
        bt_bam_scan *scan = nullptr;
        for (const std::string &f : bams) {
            BamFile file(f, bgzf_slab);
            warnNoEof(file, f);
            check(bt_bam_scan_create(ctx, bgzf_slab, skip_flags, &scan), f);
            try {
                std::vector<uint8_t> slab;
                for (bool first = true; file.next(slab); first = false) {
                    const char *d_text = nullptr;
                    uint64_t len = 0;
                    bt_bam_stats stats;
                    check(bt_bam_scan_text(scan, slab.data(), slab.size(), first ? file.skipFirstBytes() : 0, &d_text, &len, &stats), f);
                    deliverDevice(d_text, len, stats.bases, stats.kept);
                    totals.bases += stats.bases;
                    totals.reads += stats.kept;
                    totals.slabs++;
                }
                check(bt_bam_scan_finish(scan), f);
            } catch (...) {
                bt_bam_scan_destroy(scan);
                throw;
            }
            bt_bam_scan_destroy(scan);
            totals.files++;
        }
    }
    for (const std::string &f : fastqs) {
        BgzfFastqFile file(f, bgzf_slab);
        warnNoEof(file, f);
        bt_fastq_scan *scan = nullptr;
        check(bt_fastq_scan_create(ctx, bgzf_slab, &scan), f);
        try {
            std::vector<uint8_t> slab;
            const char *d_text = nullptr;
            uint64_t len = 0;
            bt_fastq_stats stats;
            auto deliver = [&]() {
                deliverDevice(d_text, len, stats.bases, stats.reads);
                totals.bases += stats.bases;
                totals.reads += stats.reads;
            };
            while (file.next(slab)) {
                check(bt_fastq_scan_text(scan, slab.data(), slab.size(), &d_text, &len, &stats), f);
                deliver();
                totals.slabs++;
            }
            check(bt_fastq_scan_finish(scan, &d_text, &len, &stats), f);   // the file's last record, when its last line has no newline
            deliver();
        } catch (...) {
            bt_fastq_scan_destroy(scan);
            throw;
        }
        bt_fastq_scan_destroy(scan);
        totals.files++;
    }
    if (!gzips.empty()) {
        // compressed bytes per call: a block is a team's work, and some thousands of teams fill the device; the stream object's buffers take about 60 times as much
        const size_t gzip_slab = std::min<size_t>(std::max<size_t>(slab_bytes, 65536), (size_t)32 << 20);
        const uint32_t chunk_bytes = gunzipChunkBytes();
        for (const std::string &f : gzips) {
            GzipFastqFile file(f, gzip_slab);
            bt_fastq_gz_scan *scan = nullptr;
            check(bt_fastq_gz_scan_create(ctx, gzip_slab, chunk_bytes, &scan), f);
            try {
                std::vector<uint8_t> slab;
                const char *d_text = nullptr;
                uint64_t len = 0;
                bt_fastq_stats stats;
                auto deliver = [&]() {
                    deliverDevice(d_text, len, stats.bases, stats.reads);
                    totals.bases += stats.bases;
                    totals.reads += stats.reads;
                };
                while (file.next(slab)) {
                    check(bt_fastq_gz_scan_text(scan, slab.data(), slab.size(), &d_text, &len, &stats), f);
                    deliver();
                    totals.slabs++;
                }
                check(bt_fastq_gz_scan_finish(scan, &d_text, &len, &stats), f);   // the file ends at a member boundary; its last record, when its last line has no newline
                deliver();
            } catch (...) {
                bt_fastq_gz_scan_destroy(scan);
                throw;
            }
            bt_fastq_gz_scan_destroy(scan);
            totals.files++;
        }
    }
    if (!texts.empty()) {
        const ReadsTotals t = !writer ? forEachReadsSlab(texts, kmer_size, threads, slab_bytes, sinks.host_slab)
                                      : forEachReadsSlabCounted(texts, kmer_size, threads, slab_bytes, ReadsPackWriter::packHost,
                                                                [&](const std::string &slab, const std::vector<uint8_t> &packed, uint64_t bases, uint64_t reads) {
                                                                    if (!slab.empty()) sinks.host_slab(slab);
                                                                    writer->addPacked(packed, slab.size(), bases, reads);
                                                                });
        totals.bases += t.bases;
        totals.reads += t.reads;
        totals.slabs += t.slabs;
        totals.files += t.files;
    }
    if (writer) {
        writer->finish();
        std::cout << "[" << getLocalTime() << "] Wrote the reads pack " << readsPackPath(prefix) << std::endl;
    }
    return totals;
}

}  // namespace bthost
