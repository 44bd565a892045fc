// A tabix index (.tbi, "The Tabix index file format" of the SAM/VCF specifications) for a VCF text written as BGZF blocks of 65280 input bytes
// (bt_bgzf_save): what `tabix -p vcf` computes in a second pass over the compressed file, computed here from what the writer already knows — where every
// line starts in the text and where every block starts in the file.  A pure function; the caller compresses the bytes (the .tbi is itself BGZF).
//   header: magic TBI\1, format 2 (VCF), columns 1 / 2 / 0, meta '#', skip 0, the contig names
//   per contig: the bins (reg2bin with min_shift 14, depth 5) with their chunks — consecutive records of one bin form one chunk — and the linear index:
//   per 16 kb window the smallest start offset of an overlapping record, a window without a record taking the previous window's value
//   n_no_coor = 0 at the end; no pseudo-bin 37450 (optional in the format)
// A record covers [POS - 1, POS - 1 + len(REF)): these VCFs carry no END.  A virtual offset is block offset << 16 | offset inside the block; a position at
// a block's end is the next block's start.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace bthost {

struct TabixLine {
    uint32_t contig;      // index into the contig names
    uint64_t pos;         // POS, 1-based
    uint64_t ref_length;  // len(REF)
    uint64_t offset;      // of the line's first byte in the uncompressed text
    uint64_t length;      // bytes of the line, its newline included
};

constexpr uint64_t kTabixBlockBytes = 65280;          // input bytes per BGZF block (bt_bgzf)
constexpr uint64_t kTabixMaxCoordinate = 1ull << 29;  // min_shift 14, depth 5: coordinates below 2^29

uint32_t tabixReg2bin(uint64_t beg, uint64_t end);   // the bin of [beg, end), 0-based half-open

// contigs: the names in file order (one without a line gets an empty entry); block_offsets [blocks + 1]: the file offset of every block, then of the EOF
// block; lines: the data lines in file order (sorted by contig index, then POS).  Returns true with the index in tbi.  Returns false with one line of
// explanation in warning — and no index — when a record's POS or the 1-based coordinate of its last base is 2^29 or above, the lines are not sorted, or an offset lies outside the blocks.
bool buildTabixIndex(const std::vector<std::string> &contigs, const std::vector<uint64_t> &block_offsets, const std::vector<TabixLine> &lines, std::string &tbi, std::string &warning);

}  // namespace bthost
