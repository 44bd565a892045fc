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

// what a call of a stream object leaves: reads text in device memory (valid until the object's next call), and the bases and reads it holds
struct DeviceText {
    const char *text = nullptr;
    uint64_t len = 0, bases = 0, reads = 0;
};

// One read file through a stream object of the device, slab by slab.  create(&scan), text(scan, slab, first, out) and finish(scan, out) return the library's
// status and fill `out`, which `deliver` takes; the scan is destroyed on every path.  totals.slabs counts the calls of `text`, totals.files the files.
template <typename Scan, typename File, typename Create, typename Text, typename Finish, typename Deliver>
void scanOnDevice(File &file, const std::string &f, Create create, Text text, Finish finish, void (*destroy)(Scan *), Deliver deliver, ReadsTotals &totals) {
    auto check = [&](int rc) {
        if (rc != BT_OK) throw std::runtime_error("read file " + f + ": " + bt_last_error());
    };
    Scan *created = nullptr;
    check(create(&created));
    std::unique_ptr<Scan, void (*)(Scan *)> scan(created, destroy);
    std::vector<uint8_t> slab;
    for (bool first = true; file.next(slab); first = false) {
        DeviceText out;
        check(text(scan.get(), slab, first, out));
        deliver(out);
        totals.slabs++;
    }
    DeviceText out;
    check(finish(scan.get(), out));
    deliver(out);
    totals.files++;
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
    auto deliver = [&](const DeviceText &t) {
        if (t.len) sinks.device_text(t.text, t.len);
        if (writer && (t.len || t.bases || t.reads)) writer->addDeviceText(t.text, t.len, t.bases, t.reads);
        totals.bases += t.bases;
        totals.reads += t.reads;
    };
    if (bam_files) *bam_files = bams.size();
    if (bgzf_fastq_files) *bgzf_fastq_files = fastqs.size();
    if (gzip_fastq_files) *gzip_fastq_files = gzips.size();
    const size_t bgzf_slab = std::max<size_t>(slab_bytes / 2, 65536);   // compressed bytes: about a quarter of the text they hold
    auto warnNoEof = [](const BgzfFile &file, const std::string &f) {
        static std::set<std::string> warned;   // once per file and process: makeBloom -r reads a file in two passes
        if (!file.hasEofBlock() && warned.insert(f).second) std::cerr << "WARNING: read file " << f << " has no BGZF end-of-file block: it may be truncated" << std::endl;
    };
    // the two FASTQ stream objects take a slab and finish alike (the file's last record comes from finish when its last line has no newline)
    auto fastqText = [](auto scan_text) {
        return [scan_text](auto *scan, const std::vector<uint8_t> &slab, bool, DeviceText &out) {
            bt_fastq_stats stats;
            const int rc = scan_text(scan, slab.data(), slab.size(), &out.text, &out.len, &stats);
            out.bases = stats.bases, out.reads = stats.reads;
            return rc;
        };
    };
    auto fastqFinish = [](auto scan_finish) {
        return [scan_finish](auto *scan, DeviceText &out) {
            bt_fastq_stats stats;
            const int rc = scan_finish(scan, &out.text, &out.len, &stats);
            out.bases = stats.bases, out.reads = stats.reads;
            return rc;
        };
    };
    if (!bams.empty()) {
        const uint32_t skip_flags = bamSkipFlags();
        for (const std::string &f : bams) {
            BamFile file(f, bgzf_slab);
            warnNoEof(file, f);
            scanOnDevice<bt_bam_scan>(
                file, f, [&](bt_bam_scan **scan) { return bt_bam_scan_create(ctx, bgzf_slab, skip_flags, scan); },
                [&](bt_bam_scan *scan, const std::vector<uint8_t> &slab, bool first, DeviceText &out) {
                    bt_bam_stats stats;
                    const int rc = bt_bam_scan_text(scan, slab.data(), slab.size(), first ? file.skipFirstBytes() : 0, &out.text, &out.len, &stats);
                    out.bases = stats.bases, out.reads = stats.kept;
                    return rc;
                },
                [](bt_bam_scan *scan, DeviceText &) { return bt_bam_scan_finish(scan); }, bt_bam_scan_destroy, deliver, totals);
        }
    }
    for (const std::string &f : fastqs) {
        BgzfFastqFile file(f, bgzf_slab);
        warnNoEof(file, f);
        scanOnDevice<bt_fastq_scan>(
            file, f, [&](bt_fastq_scan **scan) { return bt_fastq_scan_create(ctx, bgzf_slab, scan); }, fastqText(bt_fastq_scan_text), fastqFinish(bt_fastq_scan_finish),
            bt_fastq_scan_destroy, deliver, totals);
    }
    if (!gzips.empty()) {
        // compressed bytes per call: a block is a team's work, and some thousands of teams fill the device; the stream object's buffers take about 60 times as much
        const size_t gzip_slab = std::min<size_t>(std::max<size_t>(slab_bytes, 65536), (size_t)32 << 20);
        const uint32_t chunk_bytes = gunzipChunkBytes();
        for (const std::string &f : gzips) {
            GzipFastqFile file(f, gzip_slab);
            scanOnDevice<bt_fastq_gz_scan>(
                file, f, [&](bt_fastq_gz_scan **scan) { return bt_fastq_gz_scan_create(ctx, gzip_slab, chunk_bytes, scan); }, fastqText(bt_fastq_gz_scan_text),
                fastqFinish(bt_fastq_gz_scan_finish), bt_fastq_gz_scan_destroy, deliver, totals);   // (the file has to end at a member boundary: finish says so)
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
