// FASTQ records -> the reads text of bt_reads_window.hpp (the bases of a read, then '\n'), written once for the host and the device: the kernels of
// bt_fastq.hip and the host run (bt_diag_fastq_reads_text, tools/fastq_host_check.cpp) judge a line through the same functions.  The grammar is the FASTQ
// branch of host/ReadsFile.cpp, neither looser nor stricter:
//   lines end at '\n' and one trailing '\r' is stripped from every line; a record is four lines: '@' header, bases, '+' line, as many quality values as bases.
//   A blank line (no bytes, or a lone '\r') is skipped only where a record's first line is expected; anywhere else it is that line of the record.
//   The last line of a file needs no newline.  Bases are copied verbatim (the consumers' nt_code folds case and maps N); a record without bases writes nothing.
// Which of its record's four lines a line is (its phase) depends on the blank lines before it, so it is no `line index mod 4`.  Every newline carries one of two
// functions on the four phases, "advance" or — for a blank line — "advance unless phase 0"; a function on four states is a byte (two bits per state), and
// composition is associative, so the phases come out of a prefix scan.
#pragma once
#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BTF_HD __host__ __device__
#else
#define BTF_HD
#endif

namespace btfastq {

// a function on the phases 0..3: bits [2s + 1 : 2s] hold f(s)
constexpr uint32_t kIdentity = 0xE4, kAdvance = 0x39, kBlank = 0x38;
BTF_HD inline uint32_t apply(uint32_t f, uint32_t s) { return (f >> (2 * s)) & 3u; }
// first f, then g
BTF_HD inline uint32_t compose(uint32_t f, uint32_t g) { return apply(g, apply(f, 0)) | apply(g, apply(f, 1)) << 2 | apply(g, apply(f, 2)) << 4 | apply(g, apply(f, 3)) << 6; }

// the function of the newline at data[p], told from the two bytes before it (before data[0] lies a line's start)
BTF_HD inline uint32_t newline_fn(uint64_t p, uint8_t before1, uint8_t before2) {
    const bool blank = p == 0 || before1 == '\n' || (before1 == '\r' && (p == 1 || before2 == '\n'));
    return blank ? kBlank : kAdvance;
}

enum : uint32_t { kNoAt = 0, kNoPlus = 1, kLengths = 2, kTruncated = 3, kLineOk = 4 };

// the line data[start..end) without its '\r'
BTF_HD inline uint32_t stripped(const uint8_t *data, uint64_t start, uint64_t end) {
    const uint64_t n = end - start;
    return (uint32_t)(n && data[end - 1] == '\r' ? n - 1 : n);
}

struct Line {
    uint32_t verdict;   // kLineOk or the violation
    uint32_t bases;     // of a sequence line (phase 1), else 0
};
// One line, entered in `phase`.  last_open: the file's last line, which has no newline (it is never a skipped blank line).  seq_start, seq_end: the line two
// before, looked at for a quality line only.
BTF_HD inline Line judge_line(const uint8_t *data, uint64_t start, uint64_t end, uint32_t phase, bool last_open, uint64_t seq_start, uint64_t seq_end) {
    const uint32_t n = stripped(data, start, end);
    Line l{kLineOk, 0};
    if (phase == 0) {
        if (n == 0 && !last_open) return l;   // a blank line between records
        if (n == 0 || data[start] != '@') l.verdict = kNoAt;
    } else if (phase == 1)
        l.bases = n;
    else if (phase == 2) {
        if (n == 0 || data[start] != '+') l.verdict = kNoPlus;
    } else if (stripped(data, seq_start, seq_end) != n)
        l.verdict = kLengths;
    return l;
}

// the words of host/ReadsFile.cpp; line: 1-based in the file
inline std::string error_text(uint32_t verdict, uint64_t line, uint64_t bases, uint64_t quals, uint32_t lines_of_four) {
    if (verdict == kNoAt) return "line " + std::to_string(line) + ": a FASTQ record must start with '@' (a missing line?)";
    if (verdict == kNoPlus) return "line " + std::to_string(line) + ": the third line of a FASTQ record must start with '+' (a missing line?)";
    if (verdict == kLengths)
        return "FASTQ record ending at line " + std::to_string(line) + ": " + std::to_string(bases) + " bases but " + std::to_string(quals) + " quality values (a missing line?)";
    return "truncated FASTQ record at the end of the file (" + std::to_string(lines_of_four) + " of 4 lines)";
}

// The walk on one host thread, line by line: what the kernels of bt_fastq.hip compute.  verdict != kLineOk: the first violation (err_line: 0-based in data;
// for kLengths err_bases and err_quals, for kTruncated lines_of_four); too_small: the text does not fit the capacity (nothing is written past it).
struct HostText {
    uint64_t text_bytes = 0, consumed = 0, reads = 0, bases = 0, lines = 0, err_line = 0, err_bases = 0, err_quals = 0;
    uint32_t verdict = kLineOk, lines_of_four = 0;
    bool too_small = false;
};
inline HostText reads_text_host(const uint8_t *data, uint64_t len, bool final, char *text, uint64_t capacity) {
    HostText t;
    uint64_t start = 0, line = 0, out = 0, seq_start = 0, seq_end = 0, prev_start = 0, prev_end = 0;
    uint32_t phase = 0;
    while (start < len) {
        uint64_t end = start;
        while (end < len && data[end] != '\n') ++end;
        const bool open = end == len;
        if (open && !final) break;
        const Line l = judge_line(data, start, end, phase, open, seq_start, seq_end);
        if (l.verdict != kLineOk) {
            t.verdict = l.verdict;
            t.err_line = line;
            t.err_bases = stripped(data, seq_start, seq_end);
            t.err_quals = stripped(data, start, end);
            return t;
        }
        const uint32_t left = phase;
        phase = apply(open ? kAdvance : newline_fn(end, end >= 1 ? data[end - 1] : 0, end >= 2 ? data[end - 2] : 0), phase);
        if (left == 3) {   // the record is whole: its bases (the line two before) go to the text
            const uint32_t bases = stripped(data, seq_start, seq_end);
            if (bases) {
                if (out + bases + 1ull > capacity) {
                    t.too_small = true;
                    return t;
                }
                for (uint32_t j = 0; j < bases; ++j) text[out + j] = (char)data[seq_start + j];
                text[out + bases] = '\n';
                out += bases + 1ull;
                ++t.reads;
                t.bases += bases;
            }
        }
        seq_start = prev_start, seq_end = prev_end;
        prev_start = start, prev_end = end;
        ++line;
        start = open ? len : end + 1;
        if (phase == 0) t.text_bytes = out, t.consumed = start, t.lines = line;   // a record is whole, or a blank line between records has been stepped over
    }
    if (final && phase != 0) {
        t.verdict = kTruncated;
        t.lines_of_four = phase;
    }
    return t;
}

}  // namespace btfastq
