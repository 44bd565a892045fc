// A sample's reads as reads-text slabs for the reads scan of libbtgpu (include/btgpu.h: bt_reads_count / bt_reads_make_bloom / bt_reads_sketch): the input of
// the route that needs no KMC database.  A slab is ASCII bases, a newline after every read, whole reads only — what the _host entry points ask for.
#pragma once
#include <zlib.h>

#include <cstdint>
#include <functional>
#include <string>
#include <vector>

namespace bthost {

// One FASTA or FASTQ file (told apart by its first byte, '>' or '@'), plain or gzip (zlib reads either), streamed: multi-line FASTA, CRLF line ends and a missing
// final newline are handled; FASTQ is parsed as four-line records, so a quality line that starts with '@' or '+' is not taken for a header.  The slabs depend on
// the reads alone, not on how the file spells them: a slab is closed by the first read that does not fit, and a read longer than a slab is cut into pieces that
// overlap by kmer_size - 1 bases, so no k-mer is lost and none counted twice.
class ReadsFile {
   public:
    ReadsFile(const std::string &path, unsigned kmer_size, size_t slab_bytes);
    ~ReadsFile();
    ReadsFile(const ReadsFile &) = delete;
    ReadsFile &operator=(const ReadsFile &) = delete;
    // the next slab (at most slab_bytes bytes) -> out; false when the file is exhausted.  Throws std::runtime_error on a damaged file.
    bool next(std::string &out);
    uint64_t bases() const { return bases_; }   // sequence bytes parsed so far (the overlap of a cut read counts once)
    uint64_t reads() const { return reads_; }

   private:
    enum Kind { HEADER, SEQ, PLUS, QUAL };
    bool refill();
    size_t append(const char *p, size_t n);
    void cut();
    void endRead();
    void endLine();
    [[noreturn]] void fail(const std::string &what) const;

    std::string path_;
    unsigned k_;
    size_t slab_bytes_;
    gzFile file_ = nullptr;
    std::vector<char> buf_;
    size_t pos_ = 0, len_ = 0;
    bool eof_ = false, finished_ = false, fastq_ = false, line_begin_ = true, have_ready_ = false;
    Kind kind_ = HEADER;
    uint64_t line_no_ = 0, seq_len_ = 0, qual_len_ = 0, bases_ = 0, reads_ = 0;
    std::string cur_, ready_;   // the slab under construction (its last read may be unfinished); a finished slab
    size_t read_start_ = 0;     // where the unfinished read starts in cur_
};

// Which input a sample's third column <prefix> names: <prefix>.kmc_pre exists -> its KMC database (whatever else is there); otherwise <prefix>.reads exists ->
// its reads; otherwise the KMC route again, whose error names the missing database.
enum class SampleRoute { Kmc, Reads };
SampleRoute sampleRoute(const std::string &prefix);
// what a run on several ranks says about a reads sample (the reads are not sharded yet)
std::string readsSeveralRanksMessage(const std::string &sample_name);
// the identity of a reads sample in a table checkpoint's manifest: size and CRC32 of the list file, name and size of every read file (as the KMC files are
// listed by their header fields and size, not by their content)
std::string readsIdentity(const std::string &prefix);

// <prefix>.reads: one read file per line (blank lines skipped); a relative path is resolved against the list file's directory
std::vector<std::string> readReadsList(const std::string &prefix);


// Every read file of <prefix>.reads as slabs: the files are read (and inflated) by up to `threads` threads, one file per thread; consume(slab) is called by
// one thread at a time, in the order the slabs arrive — the consumers of the reads scan are commutative, so neither that order nor the thread count changes a
// result.  Returns the totals; the first error of any thread is thrown after all have stopped.
struct ReadsTotals {
    uint64_t bases = 0, reads = 0, slabs = 0, files = 0;
};
ReadsTotals forEachReadsSlab(const std::string &prefix, unsigned kmer_size, unsigned threads, size_t slab_bytes, const std::function<void(const std::string &)> &consume);
// the same over the files given (SampleReads.hpp: the FASTA / FASTQ files of a list that also names BAM files)
ReadsTotals forEachReadsSlab(const std::vector<std::string> &files, unsigned kmer_size, unsigned threads, size_t slab_bytes, const std::function<void(const std::string &)> &consume);
// The same for a run that also writes the reads pack (ReadsPack.hpp): prepare(slab, out) is called by the reading thread before it waits for its turn (the
// slabs of several files are packed at the same time on the -p threads), consume(slab, prepared, bases, reads) by one thread at a time, with the bases and reads
// the file counted since its previous slab.  What a file counts after its last slab arrives with a slab of no bytes, so the sums equal the totals.
using SlabPrepare = std::function<void(const std::string &, std::vector<uint8_t> &)>;
using SlabConsume = std::function<void(const std::string &, const std::vector<uint8_t> &, uint64_t, uint64_t)>;
ReadsTotals forEachReadsSlabCounted(const std::vector<std::string> &files, unsigned kmer_size, unsigned threads, size_t slab_bytes, const SlabPrepare &prepare, const SlabConsume &consume);

}  // namespace bthost
