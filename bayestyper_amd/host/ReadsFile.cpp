#include "ReadsFile.hpp"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <exception>
#include <fstream>
#include <iterator>
#include <mutex>
#include <stdexcept>
#include <thread>

#include <sys/stat.h>

namespace bthost {

ReadsFile::ReadsFile(const std::string &path, unsigned kmer_size, size_t slab_bytes) : path_(path), k_(kmer_size), slab_bytes_(std::max<size_t>(slab_bytes, 2 * (size_t)kmer_size + 2)), buf_(1u << 20) {
    if (kmer_size < 1) throw std::runtime_error("ReadsFile: the kmer size must be positive");
    file_ = gzopen(path.c_str(), "rb");
    if (!file_) throw std::runtime_error("Unable to open read file " + path);
    gzbuffer(file_, 1u << 20);
    try {
        if (refill()) {
            if (buf_[0] == '@') fastq_ = true;
            else if (buf_[0] != '>') fail("neither FASTA nor FASTQ (the first byte is neither '>' nor '@')");
        }
    } catch (...) {   // (no destructor runs for a constructor that throws)
        gzclose(file_);
        file_ = nullptr;
        throw;
    }
}

ReadsFile::~ReadsFile() {
    if (file_) gzclose(file_);
}

void ReadsFile::fail(const std::string &what) const { throw std::runtime_error("read file " + path_ + ": " + what); }

// more bytes into the buffer; false at the end of the file
bool ReadsFile::refill() {
    pos_ = len_ = 0;
    if (eof_) return false;
    const int got = gzread(file_, buf_.data(), (unsigned)buf_.size());
    int errnum = Z_OK;
    const char *msg = gzerror(file_, &errnum);
    if (got < 0 || (errnum != Z_OK && errnum != Z_STREAM_END)) fail(std::string("damaged or truncated compressed data (") + (msg && *msg ? msg : "zlib error") + ")");
    if ((size_t)got < buf_.size()) eof_ = true;
    len_ = (size_t)got;
    return len_ > 0;
}

// the unfinished read does not fit into the slab
void ReadsFile::cut() {
    if (read_start_ > 0) {   // whole reads before it: they are the slab, the read moves to the next one
        ready_.assign(cur_, 0, read_start_);
        cur_.erase(0, read_start_);
        read_start_ = 0;
    } else {   // the read alone fills the slab: this piece ends here and the next one starts with its last k - 1 bases
        ready_ = cur_;
        ready_ += '\n';
        cur_.erase(0, cur_.size() - std::min<size_t>(cur_.size(), k_ - 1));
    }
    have_ready_ = true;
}

// bases of the current read; returns how many were taken (fewer than n: a slab is ready and the rest comes after it has been handed out)
size_t ReadsFile::append(const char *p, size_t n) {
    size_t done = 0;
    while (done < n && !have_ready_) {
        const size_t room = slab_bytes_ - 1 - cur_.size();   // (one byte is kept for the read's newline)
        if (room == 0) {
            cut();
            break;
        }
        const size_t take = std::min(room, n - done);
        cur_.append(p + done, take);
        done += take;
    }
    bases_ += done;
    return done;
}

void ReadsFile::endRead() {
    if (cur_.size() > read_start_) {
        cur_ += '\n';
        reads_++;
    }
    read_start_ = cur_.size();
    if (cur_.size() >= slab_bytes_ - 1 && !have_ready_) {   // no further read fits
        ready_.swap(cur_);
        cur_.clear();
        read_start_ = 0;
        have_ready_ = true;
    }
}

void ReadsFile::endLine() {
    if (fastq_) {
        if (kind_ == SEQ) endRead();
        if (kind_ == QUAL && qual_len_ != seq_len_)
            fail("FASTQ record ending at line " + std::to_string(line_no_ + 1) + ": " + std::to_string(seq_len_) + " bases but " + std::to_string(qual_len_) + " quality values (a missing line?)");
    }
    line_no_++;
    line_begin_ = true;
}

bool ReadsFile::next(std::string &out) {
    while (!have_ready_ && !finished_) {
        if (pos_ == len_ && !refill()) {   // the end of the file
            if (!line_begin_) endLine();   // no final newline
            if (fastq_ && line_no_ % 4 != 0) fail("truncated FASTQ record at the end of the file (" + std::to_string(line_no_ % 4) + " of 4 lines)");
            endRead();
            if (!have_ready_ && !cur_.empty()) {
                ready_.swap(cur_);
                cur_.clear();
                have_ready_ = true;
            }
            finished_ = true;
            break;
        }
        const char *p = buf_.data() + pos_, *e = buf_.data() + len_;
        const char *nl = static_cast<const char *>(std::memchr(p, '\n', (size_t)(e - p)));
        const char *seg_end = nl ? nl : e;
        if (line_begin_) {
            const bool blank = p == seg_end || (*p == '\r' && seg_end - p == 1);
            if (!fastq_) {
                kind_ = !blank && *p == '>' ? HEADER : SEQ;
                if (kind_ == HEADER) endRead();
            } else {
                const unsigned which = (unsigned)(line_no_ % 4);
                if (which == 0 && blank && nl) {   // blank lines between records
                    pos_ = (size_t)(nl - buf_.data()) + 1;
                    continue;
                }
                if (which == 0) {
                    if (blank || *p != '@') fail("line " + std::to_string(line_no_ + 1) + ": a FASTQ record must start with '@' (a missing line?)");
                    kind_ = HEADER;
                    seq_len_ = qual_len_ = 0;
                } else if (which == 1) kind_ = SEQ;
                else if (which == 2) {
                    if (blank || *p != '+') fail("line " + std::to_string(line_no_ + 1) + ": the third line of a FASTQ record must start with '+' (a missing line?)");
                    kind_ = PLUS;
                } else kind_ = QUAL;
            }
            line_begin_ = false;
        }
        size_t n = (size_t)(seg_end - p);
        const size_t raw = n;
        if (n && seg_end[-1] == '\r') n--;   // CRLF
        if (kind_ == SEQ) {
            const size_t took = append(p, n);
            if (fastq_) seq_len_ += took;
            if (took < n) {   // a slab is ready in the middle of the line
                pos_ += took;
                continue;
            }
        } else if (kind_ == QUAL) qual_len_ += n;
        pos_ += raw;
        if (nl) {
            pos_++;
            endLine();
        }
    }
    if (!have_ready_) return false;
    out.swap(ready_);
    ready_.clear();
    have_ready_ = false;
    return true;
}

SampleRoute sampleRoute(const std::string &prefix) {
    struct stat sb;
    if (stat((prefix + ".kmc_pre").c_str(), &sb) == 0) return SampleRoute::Kmc;
    return stat((prefix + ".reads").c_str(), &sb) == 0 ? SampleRoute::Reads : SampleRoute::Kmc;
}

std::string readsSeveralRanksMessage(const std::string &sample_name) {
    return "sample " + sample_name + " has a reads list and no KMC database: the reads route runs on one GPU only (run without BT_GPUS / BT_WORLD, or count the sample with KMC)";
}

std::string readsIdentity(const std::string &prefix) {
    std::ifstream in(prefix + ".reads", std::ios::binary);
    if (!in.is_open()) throw std::runtime_error("Unable to open reads list " + prefix + ".reads");
    const std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    char hex[16];
    std::snprintf(hex, sizeof hex, "%08lx", (unsigned long)crc32(crc32(0L, Z_NULL, 0), reinterpret_cast<const Bytef *>(text.data()), (uInt)text.size()));
    const std::vector<std::string> files = readReadsList(prefix);
    std::string id = "reads list_bytes:" + std::to_string(text.size()) + " list_crc32:" + hex + " files:" + std::to_string(files.size());
    for (const std::string &f : files) {
        struct stat sb;
        if (stat(f.c_str(), &sb) != 0) throw std::runtime_error("Unable to open read file " + f);
        const size_t slash = f.find_last_of('/');
        id += " " + (slash == std::string::npos ? f : f.substr(slash + 1)) + ":" + std::to_string((unsigned long long)sb.st_size);
    }
    return id;
}

std::vector<std::string> readReadsList(const std::string &prefix) {
    const std::string list = prefix + ".reads";
    std::ifstream in(list);
    if (!in.is_open()) throw std::runtime_error("Unable to open reads list " + list);
    const size_t slash = list.find_last_of('/');
    const std::string dir = slash == std::string::npos ? "" : list.substr(0, slash + 1);
    std::vector<std::string> files;
    for (std::string line; std::getline(in, line);) {
        while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
        if (line.empty()) continue;
        files.push_back(line[0] == '/' ? line : dir + line);
    }
    if (files.empty()) throw std::runtime_error("reads list " + list + " names no read file");
    return files;
}


ReadsTotals forEachReadsSlab(const std::string &prefix, unsigned kmer_size, unsigned threads, size_t slab_bytes, const std::function<void(const std::string &)> &consume) {
    return forEachReadsSlab(readReadsList(prefix), kmer_size, threads, slab_bytes, consume);
}

ReadsTotals forEachReadsSlab(const std::vector<std::string> &files, unsigned kmer_size, unsigned threads, size_t slab_bytes, const std::function<void(const std::string &)> &consume) {
    ReadsTotals totals;
    totals.files = files.size();
    std::atomic<size_t> next_file{0};
    std::atomic<bool> stop{false};
    std::mutex device;   // one slab at a time goes to the device; the other threads go on reading
    std::exception_ptr error;
    auto work = [&]() {
        try {
            std::string slab;
            for (size_t f = next_file++; f < files.size() && !stop; f = next_file++) {
                ReadsFile file(files[f], kmer_size, slab_bytes);
                uint64_t slabs = 0;
                while (!stop && file.next(slab)) {
                    std::lock_guard<std::mutex> lock(device);
                    if (stop) break;
                    consume(slab);
                    slabs++;
                }
                std::lock_guard<std::mutex> lock(device);
                totals.bases += file.bases();
                totals.reads += file.reads();
                totals.slabs += slabs;
            }
        } catch (...) {
            std::lock_guard<std::mutex> lock(device);
            if (!error) error = std::current_exception();
            stop = true;
        }
    };
    const size_t n = std::max<size_t>(1, std::min<size_t>(threads ? threads : 1, files.size()));
    std::vector<std::thread> pool;
    for (size_t t = 1; t < n; t++) pool.emplace_back(work);
    work();
    for (auto &th : pool) th.join();
    if (error) std::rethrow_exception(error);
    return totals;
}

ReadsTotals forEachReadsSlabCounted(const std::vector<std::string> &files, unsigned kmer_size, unsigned threads, size_t slab_bytes, const SlabPrepare &prepare, const SlabConsume &consume) {
    ReadsTotals totals;
    totals.files = files.size();
    std::atomic<size_t> next_file{0};
    std::atomic<bool> stop{false};
    std::mutex device;
    std::exception_ptr error;
    auto work = [&]() {
        try {
            std::string slab;
            std::vector<uint8_t> prepared;
            for (size_t f = next_file++; f < files.size() && !stop; f = next_file++) {
                ReadsFile file(files[f], kmer_size, slab_bytes);
                uint64_t slabs = 0, bases = 0, reads = 0;   // bases, reads: handed out with the slabs so far
                while (!stop && file.next(slab)) {
                    prepare(slab, prepared);   // without the lock: the other threads' slabs are prepared at the same time
                    std::lock_guard<std::mutex> lock(device);
                    if (stop) break;
                    consume(slab, prepared, file.bases() - bases, file.reads() - reads);
                    bases = file.bases(), reads = file.reads();
                    slabs++;
                }
                std::lock_guard<std::mutex> lock(device);
                if (!stop && (file.bases() != bases || file.reads() != reads)) {   // counted after the last slab was handed out: a slab of no positions carries it
                    slab.clear();
                    prepared.clear();
                    consume(slab, prepared, file.bases() - bases, file.reads() - reads);
                }
                totals.bases += file.bases();
                totals.reads += file.reads();
                totals.slabs += slabs;
            }
        } catch (...) {
            std::lock_guard<std::mutex> lock(device);
            if (!error) error = std::current_exception();
            stop = true;
        }
    };
    const size_t n = std::max<size_t>(1, std::min<size_t>(threads ? threads : 1, files.size()));
    std::vector<std::thread> pool;
    for (size_t t = 1; t < n; t++) pool.emplace_back(work);
    work();
    for (auto &th : pool) th.join();
    if (error) std::rethrow_exception(error);
    return totals;
}

}  // namespace bthost
