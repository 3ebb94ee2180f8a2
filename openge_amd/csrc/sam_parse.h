// sam_parse.h -- SAM text -> BAM records (the reference's SamReader::ParseAlignment, util/sam_reader.cpp:313-488,
// with the SAM specification where the reference aborts), written so that the kernels of
// sam_parse.hip and a host program share every line of it.
//
//   oge_sam_tile       one wave per tile of OGE_SAM_TILE text bytes: the tile's newlines by ballot and popcount,
//                      and (FILL) the start of the line behind each newline at its rank in the file
//   oge_sam_line       one wave per line: the tabs of every 64-byte chunk by ballot, each field handled when its
//                      closing tab is met.  Without EMIT it gives the exact record length, the error code, the
//                      warning bit and the host mark; with EMIT it also stores every byte of the record once.
//
// Control flow and field values are wave-uniform; what a lane does on its own is written as a function of
// the lane index and run through oge_sp_each / oge_sp_ballot / oge_sp_sum: on the device those are the lane's
// own evaluation, a ballot and a wave sum, on a host they loop over the 64 lanes (tests/native/sam_parse_main.cpp).
// The text is read strictly inside [0, len) of the line: no slack behind the text is needed.
#pragma once
#include <stdint.h>
#include <string.h>

#include "bam_layout.h"

#ifndef OGE_HDM
#ifdef __HIPCC__
#define OGE_HDM __host__ __device__ __forceinline__
#else
#define OGE_HDM inline
#endif
#endif

enum {  // a line's error code
    OGE_SAM_OK = 0, OGE_SAM_E_SHORT, OGE_SAM_E_FIELDS, OGE_SAM_E_QNAME, OGE_SAM_E_FLAG, OGE_SAM_E_RNAME, OGE_SAM_E_POS,
    OGE_SAM_E_MAPQ, OGE_SAM_E_CIGAR, OGE_SAM_E_CIGAR_OPS, OGE_SAM_E_PNEXT, OGE_SAM_E_TLEN, OGE_SAM_E_QUAL, OGE_SAM_E_TAG,
    OGE_SAM_E_TAG_TYPE, OGE_SAM_E_TAG_INT, OGE_SAM_E_LONG, OGE_SAM_E_COUNT
};
enum { OGE_SAM_TILE = 4096, OGE_SAM_MAX_LINE = 1u << 30 };

OGE_HD const char *oge_sam_error_text(uint32_t e) {
    switch (e) {
        case OGE_SAM_E_SHORT: return "the line is shorter than 10 characters";
        case OGE_SAM_E_FIELDS: return "fewer than 11 fields";
        case OGE_SAM_E_QNAME: return "QNAME is longer than 254 characters";
        case OGE_SAM_E_FLAG: return "FLAG is not a number in 0..65535";
        case OGE_SAM_E_RNAME: return "RNAME is missing from the sequence dictionary";
        case OGE_SAM_E_POS: return "POS is not a number whose POS - 1 fits 32 bits";
        case OGE_SAM_E_MAPQ: return "MAPQ is not a number in 0..255";
        case OGE_SAM_E_CIGAR: return "CIGAR is not '*' or a list of <length below 2^28><one of MIDNSHP=X>";
        case OGE_SAM_E_CIGAR_OPS: return "CIGAR has more than 65535 operations";
        case OGE_SAM_E_PNEXT: return "PNEXT is not a number whose PNEXT - 1 fits 32 bits";
        case OGE_SAM_E_TLEN: return "TLEN is not a number that fits 32 bits";
        case OGE_SAM_E_QUAL: return "QUAL has another length than SEQ";
        case OGE_SAM_E_TAG: return "a tag is not shaped XX:T:value";
        case OGE_SAM_E_TAG_TYPE: return "a tag has a type outside AifZHB";
        case OGE_SAM_E_TAG_INT: return "an integer tag is not a number in -2^31..2^32-1";
        case OGE_SAM_E_LONG: return "the line is longer than 2^30 characters";
        default: return "unknown error";
    }
}

// the device form of the contig table: the names back to back, their n_ref + 1 offsets, and an open-addressing
// hash of the names (slot = refID + 1, 0 = empty; hmask + 1 slots, a power of two >= 2 * n_ref)
struct OgeSamParams {
    int32_t n_ref;
    uint32_t hmask;
    const uint8_t *names;
    const uint32_t *name_off;
    const uint32_t *slots;
};

struct OgeSamRec {  // what one walk over a line finds
    uint32_t err, warn, host;
    uint32_t l_name, n_cigar, l_seq, flag, mapq, span;
    int32_t refid, pos, mref, mpos, tlen;
    uint64_t tag_bytes, len;  // len = the record's bytes, block_size included (0 when err)
};

// ------------------------------------------------------------------------------------------- lane primitives
#if defined(__HIP_DEVICE_COMPILE__)
template <class F> OGE_HDM void oge_sp_each(F f) { f((uint32_t)(threadIdx.x & 63u)); }
template <class F> OGE_HDM uint64_t oge_sp_ballot(F f) { return __ballot(f((uint32_t)(threadIdx.x & 63u)) ? 1 : 0); }
template <class F> OGE_HDM uint32_t oge_sp_sum(F f) {
    uint32_t v = f((uint32_t)(threadIdx.x & 63u));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
#else
template <class F> OGE_HDM void oge_sp_each(F f) { for (uint32_t l = 0; l < 64; ++l) f(l); }
template <class F> OGE_HDM uint64_t oge_sp_ballot(F f) {
    uint64_t m = 0;
    for (uint32_t l = 0; l < 64; ++l) m |= (uint64_t)(f(l) ? 1 : 0) << l;
    return m;
}
template <class F> OGE_HDM uint32_t oge_sp_sum(F f) {
    uint32_t v = 0;
    for (uint32_t l = 0; l < 64; ++l) v += f(l);
    return v;
}
#endif

OGE_HD uint32_t oge_sp_popc(uint64_t m) { return (uint32_t)__builtin_popcountll(m); }
OGE_HD uint64_t oge_sp_below(uint32_t lane) { return ((uint64_t)1 << lane) - 1; }

// n <= 8 bytes of w at dst, low byte first
OGE_HD void oge_sp_small(uint8_t *dst, uint32_t n, uint64_t w) {
    oge_sp_each([&](uint32_t lane) {
        if (lane < n) dst[lane] = (uint8_t)(w >> (8 * lane));
    });
}

// n bytes at dst, byte i = f(i): single bytes up to the first 4-byte boundary of dst and behind the last one,
// the aligned middle as one dword per lane
template <class F> OGE_HDM void oge_sp_bulk(uint8_t *dst, uint32_t n, F f) {
    if (!n) return;
    const uint32_t mis = (uint32_t)(0 - (uintptr_t)dst) & 3u;
    const uint32_t head = mis < n ? mis : n;
    const uint32_t mid = (n - head) >> 2, tail = (n - head) & 3u;
    oge_sp_each([&](uint32_t lane) {
        if (lane < head) dst[lane] = (uint8_t)f(lane);
        else if (lane >= 4 && lane < 4 + tail) {
            const uint32_t i = head + 4 * mid + (lane - 4);
            dst[i] = (uint8_t)f(i);
        }
        for (uint32_t j = lane; j < mid; j += 64) {
            const uint32_t i = head + 4 * j;
            *(uint32_t *)(dst + i) = (f(i) & 0xFF) | ((f(i + 1) & 0xFF) << 8) | ((f(i + 2) & 0xFF) << 16) | ((f(i + 3) & 0xFF) << 24);
        }
    });
}

// ------------------------------------------------------------------------------------------------ line index
// The newlines of text[lo, bytes) inside the tile [tile, tile + OGE_SAM_TILE) (tile a multiple of 4, text 4-byte
// aligned): their count, and with FILL line_off[base + r + 1] = the position behind the tile's r-th newline
// (entries past line_off[n] are not stored).  A lane takes one aligned dword of each 256-byte step; a newline's
// rank is the newlines of the lanes below plus those of its own dword's lower bytes.
template <bool FILL>
OGE_HDM uint32_t oge_sam_tile(const uint8_t *text, uint64_t tile, uint64_t lo, uint64_t bytes, uint64_t base, uint64_t *line_off, uint64_t n) {
    uint32_t cnt = 0;
    const uint64_t stop = tile + OGE_SAM_TILE < bytes ? tile + OGE_SAM_TILE : bytes;
    for (uint64_t c = tile; c < stop; c += 256) {
        auto bits = [&](uint32_t lane) -> uint32_t {  // bit k: byte k of the lane's dword is a newline of the body
            const uint64_t p = c + 4ull * lane;
            uint32_t b = 0;
            if (p + 4 <= stop && p >= lo) {
                const uint32_t w = *(const uint32_t *)(text + p) ^ 0x0A0A0A0Au;
                b = ((w & 0xFF) == 0) | (((w & 0xFF00) == 0) << 1) | (((w & 0xFF0000) == 0) << 2) | (((w >> 24) == 0) << 3);
            } else {
                for (uint32_t k = 0; k < 4; ++k)
                    if (p + k < stop && p + k >= lo && text[p + k] == '\n') b |= 1u << k;
            }
            return b;
        };
        const uint64_t m0 = oge_sp_ballot([&](uint32_t l) { return bits(l) & 1; }), m1 = oge_sp_ballot([&](uint32_t l) { return bits(l) & 2; }),
                       m2 = oge_sp_ballot([&](uint32_t l) { return bits(l) & 4; }), m3 = oge_sp_ballot([&](uint32_t l) { return bits(l) & 8; });
        if (FILL && (m0 | m1 | m2 | m3)) {
            oge_sp_each([&](uint32_t lane) {
                const uint64_t lt = oge_sp_below(lane);
                uint64_t r = base + cnt + oge_sp_popc(m0 & lt) + oge_sp_popc(m1 & lt) + oge_sp_popc(m2 & lt) + oge_sp_popc(m3 & lt);
                const uint64_t p = c + 4ull * lane;
                const uint32_t b = (uint32_t)((m0 >> lane) & 1) | ((uint32_t)((m1 >> lane) & 1) << 1) | ((uint32_t)((m2 >> lane) & 1) << 2) |
                                   ((uint32_t)((m3 >> lane) & 1) << 3);
                for (uint32_t k = 0; k < 4; ++k)
                    if (b & (1u << k)) {
                        if (r + 1 <= n) line_off[r + 1] = p + k + 1;
                        ++r;
                    }
            });
        }
        cnt += oge_sp_popc(m0) + oge_sp_popc(m1) + oge_sp_popc(m2) + oge_sp_popc(m3);
    }
    return cnt;
}

// --------------------------------------------------------------------------------------------- field values
OGE_HD uint32_t oge_sam_hash(const uint8_t *s, uint32_t n) {  // FNV-1a
    uint32_t h = 2166136261u;
    for (uint32_t i = 0; i < n; ++i) h = (h ^ s[i]) * 16777619u;
    return h;
}

// the refID of the contig named s[0, n), -2 when the table does not have it
OGE_HD int32_t oge_sam_lookup(const OgeSamParams &p, const uint8_t *s, uint32_t n) {
    if (p.n_ref <= 0) return -2;
    for (uint32_t h = oge_sam_hash(s, n) & p.hmask;; h = (h + 1) & p.hmask) {
        const uint32_t v = p.slots[h];
        if (!v) return -2;
        const uint32_t a = p.name_off[v - 1], z = p.name_off[v];
        if (z - a != n) continue;
        uint32_t i = 0;
        while (i < n && p.names[a + i] == s[i]) ++i;
        if (i == n) return (int32_t)(v - 1);
    }
}

OGE_HD uint32_t oge_sam_table_slots(int32_t n_ref) {
    uint32_t s = 2;
    while (s < 2 * (uint32_t)n_ref) s *= 2;
    return s;
}
// Host: the hash of n_ref names into slots (oge_sam_table_slots(n_ref) entries, zeroed).  Of two contigs with one
// name the first keeps it.
OGE_HD void oge_sam_table_build(int32_t n_ref, const uint8_t *names, const uint32_t *name_off, uint32_t *slots) {
    const OgeSamParams p = {n_ref, oge_sam_table_slots(n_ref) - 1, names, name_off, slots};
    for (int32_t r = 0; r < n_ref; ++r) {
        const uint8_t *nm = names + name_off[r];
        const uint32_t n = name_off[r + 1] - name_off[r];
        if (oge_sam_lookup(p, nm, n) >= 0) continue;
        uint32_t h = oge_sam_hash(nm, n) & p.hmask;
        while (slots[h]) h = (h + 1) & p.hmask;
        slots[h] = (uint32_t)r + 1;
    }
}

// -?[0-9]+ ; magnitudes above 2^40 are returned as 2^40 (outside every field's range)
OGE_HD bool oge_sam_int(const uint8_t *s, uint32_t n, int64_t *out) {
    uint32_t i = 0;
    const bool neg = n && s[0] == '-';
    if (neg) i = 1;
    if (i >= n) return false;
    uint64_t v = 0;
    for (; i < n; ++i) {
        const uint32_t d = (uint32_t)s[i] - '0';
        if (d > 9) return false;
        v = v * 10 + d;
        if (v > (1ull << 40)) v = 1ull << 40;
    }
    *out = neg ? -(int64_t)v : (int64_t)v;
    return true;
}

OGE_HD uint32_t oge_sam_cigar_code(uint32_t c) {  // MIDNSHP=X -> 0..8, anything else 15
    switch (c) {
        case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4;
        case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8; default: return 15;
    }
}

// The character at t[p] of the CIGAR t[s, e): 0 for a digit, else bit 0 set, bit 1 for a character that is no
// operation or has no length below 2^28 in front of it, and the operation's word in the high half.
OGE_HD uint64_t oge_sam_cigar_at(const uint8_t *t, uint32_t s, uint32_t p) {
    const uint32_t c = t[p];
    if (c - '0' <= 9u) return 0;
    const uint32_t code = oge_sam_cigar_code(c);
    uint64_t v = 0, p10 = 1;
    uint32_t nd = 0;
    bool over = false;
    for (uint32_t q = p; q > s; --q) {
        const uint32_t d = (uint32_t)t[q - 1] - '0';
        if (d > 9) break;
        if (nd < 9) v += d * p10, p10 *= 10;
        else if (d) over = true;
        ++nd;
    }
    const bool bad = code > 8 || nd == 0 || over || v >= (1u << 28);
    return 1u | (bad ? 2u : 0u) | ((uint64_t)(((uint32_t)v << 4) | (code & 15)) << 32);
}

OGE_HD uint32_t oge_sam_base_code(uint32_t c) {  // "=ACMGRSVTWYHKDBN", either case; anything else is N
    if (c == '=') return 0;
    const uint32_t u = c & ~0x20u;
    if (u < 'A' || u > 'Z') return 15;
    // one nibble per letter A..Z: A1 B14 C2 D13 G4 H11 K12 M3 N15 R5 S6 T8 V7 W9 Y10, the others 15
    const uint64_t lo = 0xFFF3FCFFB4FFD2E1ull;                  // A..P
    const uint64_t hi = 0xFAF97F865Full;                        // Q..Z
    const uint32_t k = u - 'A';
    return (uint32_t)((k < 16 ? lo >> (4 * k) : hi >> (4 * (k - 16))) & 15);
}

// an integer tag's BAM type, the reference's order (sam_reader.cpp:436-453) with 2^31..2^32-1 as I
OGE_HD uint32_t oge_sam_int_type(int64_t v) {
    if (v >= 0 && v <= 255) return 'C';
    if (v >= -128 && v < 0) return 'c';
    if (v >= 0 && v <= 65535) return 'S';
    if (v >= -32768 && v < 0) return 's';
    return v >= 0 ? 'I' : 'i';
}
OGE_HD uint32_t oge_sam_b_width(uint32_t sub) {
    return sub == 'c' || sub == 'C' ? 1u : sub == 's' || sub == 'S' ? 2u : sub == 'i' || sub == 'I' || sub == 'f' ? 4u : 0u;
}

// ------------------------------------------------------------------------------------------------- one line
// The line t[0, len) (no newline).  EMIT: the record's bytes go to dst; the caller has sized the line before
// and skips lines with an error or a host mark.  Returns what the walk found, r.len = the record's length.
template <bool EMIT>
OGE_HDM OgeSamRec oge_sam_line(const uint8_t *t, uint32_t len, const OgeSamParams &sp, uint8_t *dst) {
    OgeSamRec r;
    memset(&r, 0, sizeof r);
    r.refid = r.mref = -1;
    if (len < 10) {
        r.err = OGE_SAM_E_SHORT;
        return r;
    }
    uint32_t k = 0, s = 0;
    uint32_t o_cig = 0, o_seq = 0, o_qual = 0, o_tag = 0;  // offsets inside the record
    auto field = [&](uint32_t e) -> bool {                // the field k = t[s, e); false: stop
        const uint8_t *f = t + s;
        const uint32_t n = e - s;
        int64_t v = 0;
        switch (k) {
            case 0:
                if (n > 254) return r.err = OGE_SAM_E_QNAME, false;
                r.l_name = n + 1;
                o_cig = 36 + r.l_name;
                if (EMIT) oge_sp_bulk(dst + 36, n + 1, [&](uint32_t i) -> uint32_t { return i < n ? f[i] : 0u; });
                return true;
            case 1:
                if (!oge_sam_int(f, n, &v) || v < 0 || v > 65535) return r.err = OGE_SAM_E_FLAG, false;
                r.flag = (uint32_t)v;
                return true;
            case 2:
                if (n == 1 && f[0] == '*') return true;
                r.refid = oge_sam_lookup(sp, f, n);
                if (r.refid < 0) return r.err = OGE_SAM_E_RNAME, false;
                return true;
            case 3:
                if (!oge_sam_int(f, n, &v) || v - 1 < INT32_MIN || v - 1 > INT32_MAX) return r.err = OGE_SAM_E_POS, false;
                r.pos = (int32_t)(v - 1);
                return true;
            case 4:
                if (!oge_sam_int(f, n, &v) || v < 0 || v > 255) return r.err = OGE_SAM_E_MAPQ, false;
                r.mapq = (uint32_t)v;
                return true;
            case 5: {
                o_seq = o_cig;
                if (n == 1 && f[0] == '*') return true;
                if (n == 0 || (uint32_t)f[n - 1] - '0' <= 9u) return r.err = OGE_SAM_E_CIGAR, false;
                uint32_t nops = 0, span = 0;
                for (uint32_t c = s; c < e; c += 64) {
                    const uint64_t ops = oge_sp_ballot([&](uint32_t l) { return c + l < e && (oge_sam_cigar_at(t, s, c + l) & 1); });
                    const uint64_t bad = oge_sp_ballot([&](uint32_t l) { return c + l < e && (oge_sam_cigar_at(t, s, c + l) & 2); });
                    if (bad) return r.err = OGE_SAM_E_CIGAR, false;
                    span += oge_sp_sum([&](uint32_t l) -> uint32_t {
                        if (c + l >= e) return 0;
                        const uint64_t a = oge_sam_cigar_at(t, s, c + l);
                        const uint32_t w = (uint32_t)(a >> 32), code = w & 15;
                        return (a & 1) && (code == OGE_CIG_M || code == OGE_CIG_D || code == OGE_CIG_N || code == OGE_CIG_EQ || code == OGE_CIG_X) ? w >> 4 : 0;
                    });
                    if (EMIT)
                        oge_sp_each([&](uint32_t l) {
                            if (c + l >= e) return;
                            const uint64_t a = oge_sam_cigar_at(t, s, c + l);
                            if (a & 1) oge_wr_u32(dst + o_cig + 4ull * (nops + oge_sp_popc(ops & oge_sp_below(l))), (uint32_t)(a >> 32));
                        });
                    nops += oge_sp_popc(ops);
                    if (nops > 65535) return r.err = OGE_SAM_E_CIGAR_OPS, false;
                }
                r.n_cigar = nops;
                r.span = span;
                o_seq = o_cig + 4 * nops;
                return true;
            }
            case 6:
                if (n == 1 && f[0] == '=') r.mref = r.refid;
                else if (!(n == 1 && f[0] == '*')) {
                    r.mref = oge_sam_lookup(sp, f, n);
                    if (r.mref < 0) r.mref = -1, r.warn = 1;
                }
                return true;
            case 7:
                if (!oge_sam_int(f, n, &v) || v - 1 < INT32_MIN || v - 1 > INT32_MAX) return r.err = OGE_SAM_E_PNEXT, false;
                r.mpos = (int32_t)(v - 1);
                return true;
            case 8:
                if (!oge_sam_int(f, n, &v) || v < INT32_MIN || v > INT32_MAX) return r.err = OGE_SAM_E_TLEN, false;
                r.tlen = (int32_t)v;
                return true;
            case 9:
                r.l_seq = n == 1 && f[0] == '*' ? 0 : n;
                o_qual = o_seq + (r.l_seq + 1) / 2;
                o_tag = o_qual + r.l_seq;
                if (EMIT) {
                    const uint32_t ls = r.l_seq;
                    oge_sp_bulk(dst + o_seq, (ls + 1) / 2, [&](uint32_t i) -> uint32_t {
                        return (oge_sam_base_code(f[2 * i]) << 4) | (2 * i + 1 < ls ? oge_sam_base_code(f[2 * i + 1]) : 0u);
                    });
                }
                return true;
            case 10: {
                const bool star = n == 1 && f[0] == '*';
                if (!star && n != r.l_seq) return r.err = OGE_SAM_E_QUAL, false;
                if (EMIT) oge_sp_bulk(dst + o_qual, r.l_seq, [&](uint32_t i) -> uint32_t { return star ? 0xFFu : (uint32_t)f[i] - 33u; });
                return true;
            }
            default: break;
        }
        // a tag
        if (n < 5 || f[2] != ':' || f[4] != ':') return r.err = OGE_SAM_E_TAG, false;
        const uint32_t type = f[3], vn = n - 5;
        const uint8_t *val = f + 5;
        const uint64_t name2 = (uint64_t)f[0] | ((uint64_t)f[1] << 8);
        uint8_t *out = EMIT ? dst + o_tag + r.tag_bytes : nullptr;
        if (type == 'A') {
            if (vn != 1) return r.err = OGE_SAM_E_TAG, false;
            if (EMIT) oge_sp_small(out, 4, name2 | ((uint64_t)'A' << 16) | ((uint64_t)val[0] << 24));
            r.tag_bytes += 4;
        } else if (type == 'i') {
            if (!oge_sam_int(val, vn, &v) || v < INT32_MIN || v > (int64_t)UINT32_MAX) return r.err = OGE_SAM_E_TAG_INT, false;
            const uint32_t ty = oge_sam_int_type(v);
            const uint32_t w = ty == 'C' || ty == 'c' ? 1u : ty == 'S' || ty == 's' ? 2u : 4u;
            if (EMIT) oge_sp_small(out, 3 + w, name2 | ((uint64_t)ty << 16) | ((uint64_t)(uint32_t)v << 24));
            r.tag_bytes += 3 + w;
        } else if (type == 'f') {
            r.host = 1;
            r.tag_bytes += 7;
        } else if (type == 'Z' || type == 'H') {
            if (EMIT) {
                oge_sp_small(out, 3, name2 | ((uint64_t)type << 16));
                oge_sp_bulk(out + 3, vn + 1, [&](uint32_t i) -> uint32_t { return i < vn ? val[i] : 0u; });
            }
            r.tag_bytes += 4ull + vn;
        } else if (type == 'B') {
            const uint32_t w = vn ? oge_sam_b_width(val[0]) : 0;
            if (!w || (vn > 1 && val[1] != ',')) return r.err = OGE_SAM_E_TAG, false;
            uint32_t cnt = 0;
            for (uint32_t c = 1; c < vn; c += 64) cnt += oge_sp_popc(oge_sp_ballot([&](uint32_t l) { return c + l < vn && val[c + l] == ','; }));
            r.host = 1;
            r.tag_bytes += 8ull + (uint64_t)cnt * w;
        } else {
            return r.err = OGE_SAM_E_TAG_TYPE, false;
        }
        return true;
    };
    bool go = true;
    for (uint32_t c = 0; c < len && go; c += 64) {
        uint64_t m = oge_sp_ballot([&](uint32_t l) { return c + l < len && t[c + l] == '\t'; });
        while (m && go) {
            const uint32_t e = c + (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            go = field(e);
            ++k;
            s = e + 1;
        }
    }
    if (go) {
        go = field(len);
        ++k;
    }
    if (!go) {  // a line with too few fields is named for that, whatever else is wrong with it
        uint32_t tabs = 0;
        for (uint32_t c = 0; c < len && tabs < 10; c += 64) tabs += oge_sp_popc(oge_sp_ballot([&](uint32_t l) { return c + l < len && t[c + l] == '\t'; }));
        if (tabs < 10) r.err = OGE_SAM_E_FIELDS;
        return r;
    }
    if (k < 11) {
        r.err = OGE_SAM_E_FIELDS;
        return r;
    }
    r.len = (uint64_t)o_tag + r.tag_bytes;
    if (r.len > 0x7FFFFFF0ull) {
        r.err = OGE_SAM_E_LONG;
        r.len = 0;
        return r;
    }
    if (EMIT) {
        const int32_t end = (int32_t)((uint32_t)r.pos + r.span);
        const uint32_t bin = oge_reg2bin(r.pos, end) & 0xFFFF;
        const uint32_t w[9] = {(uint32_t)r.len - 4, (uint32_t)r.refid, (uint32_t)r.pos, (bin << 16) | (r.mapq << 8) | r.l_name,
                               (r.flag << 16) | r.n_cigar, r.l_seq, (uint32_t)r.mref, (uint32_t)r.mpos, (uint32_t)r.tlen};
        oge_sp_each([&](uint32_t lane) {
            uint32_t v = 0;
            for (uint32_t j = 0; j < 9; ++j) v = (lane >> 2) == j ? w[j] : v;
            if (lane < 36) dst[lane] = (uint8_t)(v >> (8 * (lane & 3)));
        });
    }
    return r;
}
