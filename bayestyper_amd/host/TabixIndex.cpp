#include "TabixIndex.hpp"

#include <algorithm>
#include <map>
#include <utility>

namespace bthost {

uint32_t tabixReg2bin(uint64_t beg, uint64_t end) {   // SAM specification 5.3, min_shift 14, depth 5
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1u << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1u << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1u << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1u << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1u << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

namespace {

void put32(std::string &s, uint32_t v) {
    for (int i = 0; i < 4; ++i) s.push_back((char)(v >> (8 * i)));
}
void put64(std::string &s, uint64_t v) {
    for (int i = 0; i < 8; ++i) s.push_back((char)(v >> (8 * i)));
}

struct ContigIndex {
    std::map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> bins;
    std::vector<uint64_t> linear;   // ~0 = no record yet
    bool any = false;
    uint32_t last_bin = 0;
    uint64_t last_pos = 0;
};

}  // namespace

bool buildTabixIndex(const std::vector<std::string> &contigs, const std::vector<uint64_t> &block_offsets, const std::vector<TabixLine> &lines, std::string &tbi, std::string &warning) {
    tbi.clear();
    warning.clear();
    if (block_offsets.empty()) {
        warning = "no block offsets";
        return false;
    }
    const uint64_t blocks = block_offsets.size() - 1;
    auto virtual_offset = [&](uint64_t u, uint64_t &v) {
        const uint64_t block = u / kTabixBlockBytes;
        if (block > blocks || block_offsets[block] >> 48) return false;
        v = block_offsets[block] << 16 | (u % kTabixBlockBytes);
        return true;
    };
    std::vector<ContigIndex> index(contigs.size());
    uint32_t last_contig = 0;
    for (const TabixLine &l : lines) {
        if (l.contig >= contigs.size() || l.contig < last_contig) {
            warning = "the lines are not grouped by contig in the order of the contig names";
            return false;
        }
        last_contig = l.contig;
        const uint64_t beg = l.pos - 1, end = beg + std::max<uint64_t>(1, l.ref_length);
        if (l.pos == 0 || l.pos >= kTabixMaxCoordinate || end >= kTabixMaxCoordinate) {   // end = the 1-based coordinate of the record's last base
            warning = "a record of " + contigs[l.contig] + " at position " + std::to_string(l.pos) + " lies outside the tabix scheme (coordinates below 2^29)";
            return false;
        }
        ContigIndex &c = index[l.contig];
        if (c.any && l.pos < c.last_pos) {
            warning = "the lines of " + contigs[l.contig] + " are not sorted by position";
            return false;
        }
        uint64_t v_beg = 0, v_end = 0;
        if (!virtual_offset(l.offset, v_beg) || !virtual_offset(l.offset + l.length, v_end) || l.length == 0) {
            warning = "a line lies outside the blocks";
            return false;
        }
        const uint32_t bin = tabixReg2bin(beg, end);
        auto &chunks = c.bins[bin];
        if (c.any && c.last_bin == bin && !chunks.empty())
            chunks.back().second = v_end;   // consecutive records of one bin: one chunk
        else
            chunks.emplace_back(v_beg, v_end);
        const uint64_t w0 = beg >> 14, w1 = (end - 1) >> 14;
        if (c.linear.size() <= w1) c.linear.resize(w1 + 1, ~0ull);
        for (uint64_t w = w0; w <= w1; ++w) c.linear[w] = std::min(c.linear[w], v_beg);
        c.any = true;
        c.last_bin = bin;
        c.last_pos = l.pos;
    }
    tbi.append("TBI\1", 4);
    put32(tbi, (uint32_t)contigs.size());
    put32(tbi, 2);   // format: VCF
    put32(tbi, 1);   // the sequence name's column
    put32(tbi, 2);   // the position's column
    put32(tbi, 0);   // no end column
    put32(tbi, '#');
    put32(tbi, 0);   // lines to skip
    size_t names = 0;
    for (const auto &n : contigs) names += n.size() + 1;
    put32(tbi, (uint32_t)names);
    for (const auto &n : contigs) tbi.append(n.c_str(), n.size() + 1);
    for (ContigIndex &c : index) {
        put32(tbi, (uint32_t)c.bins.size());
        for (const auto &b : c.bins) {
            put32(tbi, b.first);
            put32(tbi, (uint32_t)b.second.size());
            for (const auto &chunk : b.second) {
                put64(tbi, chunk.first);
                put64(tbi, chunk.second);
            }
        }
        put32(tbi, (uint32_t)c.linear.size());
        uint64_t previous = 0;
        for (uint64_t v : c.linear) {
            if (v != ~0ull) previous = v;
            put64(tbi, previous);
        }
    }
    put64(tbi, 0);   // n_no_coor
    return true;
}

}  // namespace bthost
