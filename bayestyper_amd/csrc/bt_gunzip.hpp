// One long deflate stream (RFC 1951: a gzip member as gzip, pigz and most archives write it) inflated by many teams at once, written once for the host
// and the device: bt_gunzip.hip runs find_lane, decode_team<WaveTeam>, window_step and resolve_symbol in kernels; bt_diag_inflate_raw and
// tools/gunzip_host_check.cpp run the same lines with a team of one thread (HostBackend below).  The rounds (inflate_rounds) are host code for both.
// The two-stage scheme of pugz and rapidgzip over the serial decoder of bt_inflate.hpp.
//
// A call works on in[0..n) from a start bit p0 that is a block boundary, with the up to 32768 bytes of output before p0 (the window).
//   find     the input is cut into chunks of chunk_bytes.  For every chunk behind the one that holds p0: the first bit offset in it where a plausible
//            non-final dynamic block header starts (plausible_header: every test inflate_stream applies to such a header).  One lane per bit offset.
//   decode   one team per start: p0 (team 0) and the candidates, ascending.  A team decodes whole blocks until its position reaches the next start, a
//            final block ends, the next block is not whole inside n, or its room is used up; it ends at the last whole block boundary.  Its output is
//            16-bit symbols: below 256 a byte, kMarker | i the byte i of the 32768 before its start, which it does not know.  Matches copy symbols.
//            Team 0 writes at the symbol buffer's start; the team of a candidate at byte b writes at room0 + kExpand * b, up to the next candidate's
//            place: no scan before the decode, no team waits for another.  A candidate's team depends on the input alone, so it is decoded once per
//            call and kept; the later rounds decode team 0 only.
//   verify   (host) link j -> j + 1 holds when team j ended exactly at start j + 1.  The round's result is the teams up to the first link that does not
//            hold.  By induction the end of the last one is a true block boundary: the next round's p0.  A team whose markers reach further back than
//            the bytes that exist before it (reach) ends the chain in front of it; team 0 knows how many exist and checks every distance itself.
//   windows  one workgroup walks the chain: W_j = the last 32768 bytes of W_{j-1} followed by team j-1's resolved output (window_step).
//   resolve  every symbol of the chain becomes a byte at its place in the output; a marker is looked up in its team's window.
// Every round advances past at least one block or ends the call, so there are at most as many rounds as blocks, plus one.  A false candidate, a team
// out of room or a stream's end costs a round, never a wrong byte.
// An error is only ever team 0's, on the first block it decodes: p0 is a true boundary, so the message names that block, whatever chunk_bytes is.
// Damaged input is an error, never a fault or a hang (the rules of bt_inflate.hpp): every load is below n, every store inside the team's room, every
// turn of a loop consumes a bit or produces a symbol.
#pragma once
#include <zlib.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "bt_inflate.hpp"

namespace btgunzip {

using namespace btinflate;

constexpr uint32_t kWindow = 32768;
constexpr uint32_t kExpand = 10;         // symbols of room per compressed byte of a candidate team's span
constexpr uint32_t kMarker = 0x8000u;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kMaxIn = 1u << 27;     // bit offsets and kExpand times a span are 32 bits
constexpr uint32_t kMaxRun = 1u << 30;    // output bytes of one call
constexpr uint32_t kDefaultChunk = 16384, kMinChunk = 1024;
constexpr uint32_t kCrcPiece = 65536;     // crc32_team's most

enum Stop : uint32_t { kStopLimit = 0, kStopFinal, kStopInput, kStopRoom, kStopError };

struct TeamRec {
    uint32_t end_bit, out_syms, blocks, reach;   // at the last whole block boundary; reach: how far before the team's start its markers go
    uint32_t stop, status, pad0, pad1;           // why it went no further
};
struct ChainEntry {
    uint64_t sym_at, out_at;   // the team's place in the symbol buffer; its bytes' place in the output
    uint32_t n, pad;
};
struct Stats {
    uint64_t rounds, candidates, links_verified, links_broken, blocks, out_bytes;
};

// ---- find -----------------------------------------------------------------------------------------------------------------------------------------------
// Does a plausible non-final dynamic block start at bit `at` of in[0..n)?  Everything inflate_stream checks in such a header, in registers: the code-length
// code as packed words, the two sets as Kraft sums (units of 2^-15).  A header that runs past n is none.
BTD_HD inline bool plausible_header(const uint8_t *in, uint32_t n, uint32_t at) {
    if ((at >> 3) >= n) return false;
    Bits b{in, n, at >> 3, 0, 0};
    b.refill();
    b.drop(at & 7u);
    if (b.cnt < 17) return false;
    const uint32_t h = b.peek(17);
    if ((h & 7u) != 4u) return false;   // BFINAL = 0, BTYPE = 2
    const uint32_t nlit = ((h >> 3) & 31u) + 257, ndist = ((h >> 8) & 31u) + 1, nclen = (h >> 13) + 4;
    if (nlit > 286 || ndist > 30) return false;
    b.drop(17);
    uint64_t cl = 0;     // 3 bits per symbol of the code-length code
    uint32_t kraft = 0;  // units of 2^-7
    for (uint32_t i = 0; i < nclen; ++i) {
        b.refill();
        const uint32_t v = b.take(3);
        cl |= (uint64_t)v << (3 * btdeflate::clen_order(i));
        if (v) kraft += 128u >> v;
    }
    if (b.cnt < 0 || kraft != 128u) return false;   // a complete code
    uint64_t counts = 0, syms[2] = {0, 0};   // 5 bits per length; 5 bits per symbol in code order, 12 to a word
    uint32_t k = 0;
    for (uint32_t l = 1; l <= 7; ++l)
        for (uint32_t s = 0; s < kNumClen; ++s)
            if (((cl >> (3 * s)) & 7u) == l) {
                counts += 1ull << (5 * l);
                if (k < 12) syms[0] |= (uint64_t)s << (5 * k);
                else syms[1] |= (uint64_t)s << (5 * (k - 12));
                ++k;
            }
    uint32_t klit = 0, kdist = 0, maxlit = 0, maxdist = 0, prev = 0;
    bool has256 = false;
    for (uint32_t i = 0; i < nlit + ndist;) {
        b.refill();
        uint32_t code = 0, first = 0, index = 0, s = kNoSymbol;
        for (uint32_t l = 1; l <= 7; ++l) {
            code |= (uint32_t)(b.buf >> (l - 1)) & 1u;
            const uint32_t c = (uint32_t)(counts >> (5 * l)) & 31u;
            if (code < first + c) {
                b.drop(l);
                const uint32_t at_sym = index + (code - first);
                s = (uint32_t)((at_sym < 12 ? syms[0] >> (5 * at_sym) : syms[1] >> (5 * (at_sym - 12))) & 31u);
                break;
            }
            index += c;
            first = (first + c) << 1;
            code <<= 1;
        }
        if (s == kNoSymbol) return false;
        uint32_t rep = 1, v = s;
        if (s == 16) {
            if (i == 0) return false;
            v = prev, rep = 3 + b.take(2);
        } else if (s == 17)
            v = 0, rep = 3 + b.take(3);
        else if (s == 18)
            v = 0, rep = 11 + b.take(7);
        if (b.cnt < 0) return false;
        if (rep > nlit + ndist - i) return false;
        if (v) {
            const uint32_t in_lit = i < nlit ? (rep < nlit - i ? rep : nlit - i) : 0, in_dist = rep - in_lit;
            if (in_lit) {
                klit += in_lit * (32768u >> v);
                if (v > maxlit) maxlit = v;
                if (i <= 256 && 256 < i + in_lit) has256 = true;
            }
            if (in_dist) {
                kdist += in_dist * (32768u >> v);
                if (v > maxdist) maxdist = v;
            }
        }
        prev = v;
        i += rep;
    }
    if (!has256) return false;
    if (klit > 32768u || (klit < 32768u && maxlit != 1)) return false;      // build_table's rule, allow_empty = false
    if (kdist > 32768u || (kdist < 32768u && maxdist > 1)) return false;    // and allow_empty = true
    return true;
}

// ---- decode ---------------------------------------------------------------------------------------------------------------------------------------------
BTD_HD inline uint32_t bit_position(const Bits &b) { return 8u * b.pos - (uint32_t)b.cnt; }

// Whole blocks of in[0..n) from start_bit until the position is >= limit_bit -> out[0..room) as symbols.  known: the bytes that exist before the start
// (team 0 knows; a candidate's team passes kWindow and reports its reach).  The same record on every lane; lane 0 stores it.
template <class T>
BTD_HD inline void decode_team(Shared &sh, const uint8_t *in, uint32_t n, uint32_t start_bit, uint32_t limit_bit, uint16_t *out, uint32_t room, uint32_t known, TeamRec *rec) {
    Bits b{in, n, start_bit >> 3 < n ? start_bit >> 3 : n, 0, 0};
    b.refill();
    b.drop(start_bit & 7u);
    uint32_t opos = 0, reach = 0;
    TeamRec r{start_bit, 0, 0, 0, kStopLimit, kOk, 0, 0};
    for (;;) {
        if (b.cnt >= 0 && bit_position(b) >= limit_bit) break;
        b.refill();
        const bool last = b.take(1) != 0;
        const uint32_t type = b.take(2);
        uint32_t stop = kStopLimit, status = kOk;
        if (b.cnt < 0) stop = kStopInput;
        else if (type == 3) stop = kStopError, status = kBadBlockType;
        else if (type == 0) {   // stored: to the byte boundary, LEN, NLEN, LEN bytes
            b.drop((uint32_t)b.cnt & 7u);
            b.refill();
            const uint32_t len = b.take(16), nlen = b.take(16);
            const uint32_t at = b.cnt < 0 ? n : b.pos - ((uint32_t)b.cnt >> 3);
            if (b.cnt < 0) stop = kStopInput;
            else if ((len ^ nlen) != 0xFFFFu) stop = kStopError, status = kBadBlockType;
            else if (len > n - at) stop = kStopInput;
            else if (len > room - opos) stop = kStopRoom;
            else {
                for (uint32_t i = T::lane(); i < len; i += T::W) out[opos + i] = in[at + i];
                T::sync();
                opos += len;
                b.pos = at + len;
                b.buf = 0;
                b.cnt = 0;
            }
        } else {
            status = block_tables<T>(sh, b, type);
            if (status != kOk) stop = status == kInputEnd ? kStopInput : kStopError;
            while (stop == kStopLimit) {   // a turn takes at most 48 bits; a refill leaves at least 56 unless the input ends
                if (b.cnt < 48) b.refill();
                const uint32_t s = decode(b, sh.lit, kLitBits, sh.lsym, sh.lcount);
                if (s == kNoSymbol) {
                    if (no_symbol_status(b) == kInputEnd) stop = kStopInput;
                    else stop = kStopError, status = kBadSymbol;
                    break;
                }
                if (b.cnt < 0) {
                    stop = kStopInput;
                    break;
                }
                if (s < 256) {
                    if (opos >= room) {
                        stop = kStopRoom;
                        break;
                    }
                    if (T::lane() == 0) out[opos] = (uint16_t)s;
                    ++opos;
                    continue;
                }
                if (s == 256) break;
                if (s >= 286) {
                    stop = kStopError, status = kBadSymbol;
                    break;
                }
                const uint32_t lc = s - 257, leb = lc < 8 || lc == 28 ? 0 : (lc >> 2) - 1;
                const uint32_t len = lc == 28 ? 258 : lc < 8 ? 3 + lc : 3 + ((4 + (lc & 3)) << leb) + b.take(leb);
                const uint32_t dc = decode(b, sh.dist, kDistBits, sh.dsym, sh.dcount);
                if (dc == kNoSymbol) {
                    if (no_symbol_status(b) == kInputEnd) stop = kStopInput;
                    else stop = kStopError, status = kBadSymbol;
                    break;
                }
                if (dc >= 30) {
                    stop = kStopError, status = kBadSymbol;
                    break;
                }
                const uint32_t deb = dc < 4 ? 0 : (dc >> 1) - 1;
                const uint32_t dist = dc < 4 ? 1 + dc : 1 + ((2 + (dc & 1)) << deb) + b.take(deb);   // at most kWindow
                if (b.cnt < 0) {
                    stop = kStopInput;
                    break;
                }
                if (dist > opos) {
                    if (dist - opos > known) {
                        stop = kStopError, status = kBadStreamDistance;
                        break;
                    }
                    if (dist - opos > reach) reach = dist - opos;
                }
                if (len > room - opos) {
                    stop = kStopRoom;
                    break;
                }
                // symbol i's source lies in the dist symbols before the match, also when the copy overlaps itself; before out[0] it is a marker
                const int32_t from = (int32_t)opos - (int32_t)dist;
                if (T::W == 1 || len < kWideCopy) {
                    if (T::lane() == 0)
                        for (uint32_t i = 0; i < len; ++i) {
                            const int32_t src = from + (int32_t)i;
                            out[opos + i] = src >= 0 ? out[src] : (uint16_t)(kMarker | (uint32_t)((int32_t)kWindow + src));
                        }
                } else {
                    T::sync();
                    for (uint32_t i = T::lane(); i < len; i += T::W) {
                        const int32_t src = from + (int32_t)(dist >= len ? i : i % dist);
                        out[opos + i] = src >= 0 ? out[src] : (uint16_t)(kMarker | (uint32_t)((int32_t)kWindow + src));
                    }
                    T::sync();
                }
                opos += len;
            }
        }
        if (stop != kStopLimit) {
            r.stop = stop;
            r.status = status;
            break;
        }
        r.end_bit = bit_position(b);
        r.out_syms = opos;
        r.reach = reach;
        ++r.blocks;
        if (last) {
            r.stop = kStopFinal;
            break;
        }
    }
    T::sync();
    if (T::lane() == 0) *rec = r;
}

// ---- windows and resolve ----------------------------------------------------------------------------------------------------------------------------------
BTD_HD inline uint8_t resolve_symbol(uint32_t s, const uint8_t *window) { return s < 256 ? (uint8_t)s : window[s & (kWindow - 1)]; }

// win[0..kWindow) (LDS on the device), the window of a team, and the team's n symbols -> the window behind the team, into next[] and win[]
template <class T>
BTD_HD inline void window_step(uint8_t *win, const uint16_t *syms, uint32_t n, uint8_t *next) {
    const uint32_t keep = n < kWindow ? kWindow - n : 0;   // bytes of the old window that stay
    for (uint32_t i = T::lane(); i < kWindow; i += T::W) next[i] = i < keep ? win[i + n] : resolve_symbol(syms[n - (kWindow - i)], win);
    T::sync();
    for (uint32_t i = T::lane(); i < kWindow; i += T::W) win[i] = next[i];
    T::sync();
}

// ---- the rounds (host code for both backends) ---------------------------------------------------------------------------------------------------------------
struct RawJob {
    uint32_t n, start_bit, chunk;
    uint32_t known;        // bytes of window that exist before start_bit
    uint64_t capacity;
};
struct RawResult {
    uint64_t out_bytes = 0;
    uint32_t end_bit = 0, crc = 0, stop = kStopInput, status = kOk, known = 0;
    int stream_end = 0;
    Stats stats{0, 0, 0, 0, 0, 0};
};

inline uint64_t symbol_count(uint32_t n, uint64_t room0) { return room0 + (uint64_t)kExpand * n; }

// Backend: find(first_chunk, cand), decode_all(starts, recs, p0, limit, room, known, rec) (the candidates' teams and team 0), decode_first(p0, limit, room,
// known, rec) (team 0 alone), resolve(chain) and crc(n, &crc); each returns 0 or an error already set.  The backend holds the input, the symbols, the windows (slot 0: the current one) and the output.
// Returns 0 and the result (r.status != kOk: the block at r.end_bit is damaged), or the backend's error.
template <class B>
inline int inflate_rounds(B &be, const RawJob &job, RawResult &r) {
    const uint32_t n = job.n, chunk = job.chunk;
    const uint32_t n_chunks = (uint32_t)(((uint64_t)n + chunk - 1) / chunk), first_chunk = (job.start_bit >> 3) / chunk + 1;
    const uint64_t capacity = std::min<uint64_t>(job.capacity, kMaxRun);
    std::vector<uint32_t> cand, starts;
    if (first_chunk < n_chunks && be.find(first_chunk, cand)) return 1;
    for (uint32_t c = first_chunk; c < n_chunks; ++c)
        if (cand[c] != kNone) starts.push_back(cand[c]);
    r.stats.candidates = starts.size();
    std::vector<TeamRec> recs(starts.size());
    uint32_t p0 = job.start_bit, known = job.known;
    uint64_t produced = 0;
    size_t next = 0;   // the first candidate in a chunk behind p0's
    std::vector<ChainEntry> chain;
    r.stop = kStopInput;
    for (;;) {
        while (next < starts.size() && (starts[next] >> 3) / chunk <= (p0 >> 3) / chunk) ++next;
        const uint32_t limit = next < starts.size() ? starts[next] : kNone;
        const uint64_t remaining = capacity - produced;
        // team 0 gets the room a candidate's team would; when that is not enough for one block, all that is left
        const uint32_t span = (limit == kNone ? n : limit >> 3) - std::min(p0 >> 3, n);
        uint32_t room = (uint32_t)std::min<uint64_t>(remaining, (uint64_t)kExpand * std::max(span, 1u));
        TeamRec t0;
        ++r.stats.rounds;
        // the first round decodes the candidates' teams with team 0, in one launch on the device
        if (r.stats.rounds == 1 ? be.decode_all(starts, recs, p0, limit, room, known, &t0) : be.decode_first(p0, limit, room, known, &t0)) return 1;
        if (!t0.blocks && t0.stop == kStopRoom && room < remaining) {
            room = (uint32_t)remaining;
            ++r.stats.rounds;
            if (be.decode_first(p0, limit, room, known, &t0)) return 1;
        }
        if (!t0.blocks) {   // nothing more in this call: the block at p0 is not whole, does not fit, or is damaged
            r.stop = t0.stop;
            r.status = t0.stop == kStopError ? t0.status : (uint32_t)kOk;
            break;
        }
        chain.clear();
        chain.push_back(ChainEntry{0, produced, t0.out_syms, 0});
        uint64_t total = t0.out_syms;
        uint32_t blocks = t0.blocks;
        const TeamRec *t = &t0;
        for (size_t j = next; j < starts.size(); ++j) {
            if (t->stop == kStopFinal) break;
            if (t->end_bit != starts[j]) {
                ++r.stats.links_broken;
                break;
            }
            const TeamRec &c = recs[j];
            if (!c.blocks || c.reach > std::min<uint64_t>(kWindow, known + total) || total + c.out_syms > remaining) break;
            ++r.stats.links_verified;
            chain.push_back(ChainEntry{capacity + (uint64_t)kExpand * (starts[j] >> 3), produced + total, c.out_syms, 0});
            total += c.out_syms;
            blocks += c.blocks;
            t = &c;
        }
        if (be.resolve(chain)) return 1;
        produced += total;
        known = (uint32_t)std::min<uint64_t>(kWindow, known + total);
        r.stats.blocks += blocks;
        p0 = t->end_bit;
        if (t->stop == kStopFinal) {
            r.stream_end = 1;
            r.stop = kStopFinal;
            break;
        }
    }
    r.out_bytes = r.stats.out_bytes = produced;
    r.end_bit = p0;
    r.known = known;
    return be.crc(produced, &r.crc);
}

inline std::string block_error(uint64_t byte_offset, uint32_t bit, uint32_t status) {
    return "deflate block at offset " + std::to_string(byte_offset) + " (bit " + std::to_string(bit) + "): " + status_text(status);
}

// ---- the host's backend: a team of one thread ------------------------------------------------------------------------------------------------------------------
struct HostBackend {
    const uint8_t *in;
    uint32_t n, chunk;
    uint8_t *out;
    std::vector<uint16_t> syms;
    std::vector<uint8_t> window, next;   // slot 0 and the one being built
    std::vector<uint8_t> windows;        // a window per team of the chain
    std::unique_ptr<Shared> sh{new Shared};
    std::unique_ptr<btbgzf::CrcShared> cs{new btbgzf::CrcShared};
    uint64_t room0 = 0;

    // h_window [known]: the bytes before the start, right-aligned into slot 0
    HostBackend(const uint8_t *in_, uint32_t n_, uint32_t chunk_, const uint8_t *h_window, uint32_t known, uint8_t *out_, uint64_t capacity)
        : in(in_), n(n_), chunk(chunk_), out(out_), window(kWindow, 0), next(kWindow, 0) {
        room0 = std::min<uint64_t>(capacity, kMaxRun);
        syms.resize(symbol_count(n, room0));
        for (uint32_t i = 0; i < known; ++i) window[kWindow - known + i] = h_window[i];
    }
    int find(uint32_t first_chunk, std::vector<uint32_t> &cand) {
        const uint32_t n_chunks = (uint32_t)(((uint64_t)n + chunk - 1) / chunk);
        cand.assign(n_chunks, kNone);
        for (uint32_t c = first_chunk; c < n_chunks; ++c) {
            const uint64_t end = std::min<uint64_t>(((uint64_t)c + 1) * chunk, n) * 8;
            for (uint64_t at = (uint64_t)c * chunk * 8; at < end; ++at)
                if (plausible_header(in, n, (uint32_t)at)) {
                    cand[c] = (uint32_t)at;
                    break;
                }
        }
        return 0;
    }
    int decode_all(const std::vector<uint32_t> &starts, std::vector<TeamRec> &recs, uint32_t p0, uint32_t limit, uint32_t room, uint32_t known, TeamRec *rec) {
        decode_team<LaneTeam>(*sh, in, n, p0, limit, syms.data(), room, known, rec);
        for (size_t j = 0; j < starts.size(); ++j) {
            const uint32_t byte = starts[j] >> 3, end_byte = j + 1 < starts.size() ? starts[j + 1] >> 3 : n;
            decode_team<LaneTeam>(*sh, in, n, starts[j], j + 1 < starts.size() ? starts[j + 1] : kNone, syms.data() + room0 + (uint64_t)kExpand * byte, kExpand * (end_byte - byte), kWindow,
                                  &recs[j]);
        }
        return 0;
    }
    int decode_first(uint32_t p0, uint32_t limit, uint32_t room, uint32_t known, TeamRec *rec) {
        decode_team<LaneTeam>(*sh, in, n, p0, limit, syms.data(), room, known, rec);
        return 0;
    }
    int resolve(const std::vector<ChainEntry> &chain) {
        windows.resize(chain.size() * (size_t)kWindow);
        for (size_t j = 0; j < chain.size(); ++j) {
            std::copy(window.begin(), window.end(), windows.begin() + j * kWindow);
            window_step<LaneTeam>(window.data(), syms.data() + chain[j].sym_at, chain[j].n, next.data());
        }
        for (size_t j = 0; j < chain.size(); ++j)
            for (uint32_t k = 0; k < chain[j].n; ++k) out[chain[j].out_at + k] = resolve_symbol(syms[chain[j].sym_at + k], windows.data() + j * kWindow);
        return 0;
    }
    int crc(uint64_t bytes, uint32_t *crc_out) {
        uLong c = crc32(0L, Z_NULL, 0);
        for (uint64_t at = 0; at < bytes; at += kCrcPiece) {
            const uint32_t len = (uint32_t)std::min<uint64_t>(kCrcPiece, bytes - at);
            c = crc32_combine(c, btbgzf::crc32_team<LaneTeam>(*cs, out + at, len), (z_off_t)len);
        }
        *crc_out = (uint32_t)c;
        return 0;
    }
};

// ---- the gzip member around the stream (RFC 1952), host only ------------------------------------------------------------------------------------------------------
// p[0..n) from a member's first byte -> the payload's offset; 0: the header is not whole yet; kNone: not a gzip header (*what says why)
inline uint32_t gzip_header(const uint8_t *p, uint64_t n, std::string *what) {
    if (n >= 1 && p[0] != 0x1f) return *what = "not a gzip header (magic)", kNone;
    if (n >= 2 && p[1] != 0x8b) return *what = "not a gzip header (magic)", kNone;
    if (n >= 3 && p[2] != 8) return *what = "gzip compression method is not deflate", kNone;
    if (n >= 4 && (p[3] & 0xE0u)) return *what = "reserved gzip flag bits are set", kNone;
    if (n < 10) return 0;
    const uint32_t flg = p[3];
    uint64_t at = 10;
    if (flg & 4u) {   // FEXTRA
        if (n < at + 2) return 0;
        at += 2 + (p[at] | ((uint32_t)p[at + 1] << 8));
    }
    for (uint32_t f : {8u, 16u})   // FNAME, FCOMMENT: zero-terminated
        if (flg & f) {
            while (at < n && p[at]) ++at;
            ++at;
        }
    if (flg & 2u) at += 2;   // FHCRC
    if (at > n) return 0;
    if (at >= kNone) return *what = "gzip header too long", kNone;
    return (uint32_t)at;
}

}  // namespace btgunzip
