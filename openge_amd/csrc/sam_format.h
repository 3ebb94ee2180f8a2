// sam_format.h -- one BAM record -> its SAM line or its single-stream FASTQ entry (util/sam_writer.cpp:90-217,
// util/fastq_writer.cpp:99-100 of the reference), written so that the kernels of sam.hip and a host program
// share every line of it.
//
//   oge_text_record_size   one thread per record: the exact text length and the record's mark
//   oge_text_record_emit   one wave per record: control flow and field values are wave-uniform, `lane`
//                          (0..63) only picks which bytes of a piece this lane stores.  Run 64 times with
//                          lane = 0..63 it writes the same bytes on a host (tests/native/sam_format_main.cpp).
//
// A piece is either a short string assembled in four wave-uniform 64-bit words (Txt32: numbers, separators,
// tag heads; lane j stores byte j) or a bulk run copied or translated from the record (names, SEQ, QUAL, Z
// tags): bytes up to the first 4-byte boundary of the output and behind the last one singly, the aligned
// middle as one dword per lane, 256 bytes per wave instruction.  Every output byte is stored once.
#pragma once
#include <stdint.h>
#include <string.h>

#include "bam_layout.h"

#ifdef __HIPCC__
#define OGE_HDM __host__ __device__ __forceinline__
#else
#define OGE_HDM inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#include "dev_util.h"
#define OGE_TXT_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define OGE_TXT_UNI(x) ((uint32_t)(x))
#endif

enum { OGE_TXT_DEVICE = 0, OGE_TXT_HOST = 1, OGE_TXT_BAD = 2 };  // a record's mark

// the device form of oge_text_opts: the contig names back to back (8 bytes of slack behind them) and the
// n_ref + 1 offsets of their starts
struct OgeTextParams {
    int32_t mode, trim_begin, trim_end, n_ref;
    const uint8_t *names;
    const uint32_t *name_off;
};

// four bytes from any address; may read up to 7 bytes past p (the arenas and the name table carry slack)
OGE_HD uint32_t oge_txt_ld32(const uint8_t *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return oge_ldu32(p);
#else
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
#endif
}

OGE_HD uint32_t oge_txt_dec_width(uint32_t v) {
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) +
           (v >= 100000000u) + (v >= 1000000000u);
}
// |v| <= 2^32 - 1
OGE_HD uint32_t oge_txt_sdec_width(int64_t v) { return v < 0 ? 1u + oge_txt_dec_width((uint32_t)(-v)) : oge_txt_dec_width((uint32_t)v); }

OGE_HD uint32_t oge_txt_cigar_letter(uint32_t code) {
    // "MIDNSHP=X", '?' for the codes the format does not define
    const uint64_t lo = 0x3D504853'4E44494Dull;  // M I D N S H P =
    return code < 8 ? (uint32_t)(lo >> (8 * code)) & 0xFF : code == 8 ? 'X' : '?';
}

// byte size of a B array's element, 0 for an unknown subtype
OGE_HD uint32_t oge_txt_b_elem(uint32_t sub) {
    return sub == 'c' || sub == 'C' ? 1u : sub == 's' || sub == 'S' ? 2u : sub == 'i' || sub == 'I' || sub == 'f' ? 4u : 0u;
}

struct OgeTextRec {  // the fixed part of a record, bounds checked
    uint32_t l_name, mapq, n_cigar, flag, l_seq, tag_len;
    int32_t refid, pos, mref, mpos, tlen;
    const uint8_t *name, *cigar, *seq, *qual, *tags;
};

// false: the lengths in the core do not fit the record
OGE_HD bool oge_text_parse(const uint8_t *rec, OgeTextRec &r) {
    const uint32_t bs = oge_txt_ld32(rec);
    const uint32_t w3 = oge_txt_ld32(rec + OGE_OFF_LNAME), w4 = oge_txt_ld32(rec + OGE_OFF_NCIGAR);
    r.refid = (int32_t)oge_txt_ld32(rec + OGE_OFF_REFID);
    r.pos = (int32_t)oge_txt_ld32(rec + OGE_OFF_POS);
    r.l_name = w3 & 0xFF;
    r.mapq = (w3 >> 8) & 0xFF;
    r.n_cigar = w4 & 0xFFFF;
    r.flag = w4 >> 16;
    const int32_t ls = (int32_t)oge_txt_ld32(rec + OGE_OFF_LSEQ);
    r.mref = (int32_t)oge_txt_ld32(rec + OGE_OFF_MREFID);
    r.mpos = (int32_t)oge_txt_ld32(rec + OGE_OFF_MPOS);
    r.tlen = (int32_t)oge_txt_ld32(rec + OGE_OFF_TLEN);
    r.l_seq = ls < 0 ? 0u : (uint32_t)ls;
    const uint64_t var = (uint64_t)r.l_name + 4ull * r.n_cigar + ((uint64_t)r.l_seq + 1) / 2 + r.l_seq;
    if (bs < 32 || ls < 0 || r.l_name < 1 || 32 + var > bs) {
        r.tag_len = 0;
        return false;
    }
    r.name = rec + OGE_OFF_NAME;
    r.cigar = r.name + r.l_name;
    r.seq = r.cigar + 4ull * r.n_cigar;
    r.qual = r.seq + (r.l_seq + 1) / 2;
    r.tags = r.qual + r.l_seq;
    r.tag_len = (uint32_t)(bs - 32 - var);
    return true;
}

// FASTQ: the window [*first, *first + *sl) of SEQ and QUAL
OGE_HD void oge_text_trim_window(const OgeTextParams &tp, uint32_t l_seq, uint32_t *first, uint32_t *sl) {
    const uint64_t b = (uint64_t)tp.trim_begin, e = (uint64_t)tp.trim_end;
    const uint64_t m = l_seq > b + e ? l_seq - b - e : 0;
    *first = m ? (uint32_t)b : 0u;
    *sl = (uint32_t)m;
}

OGE_HD uint32_t oge_text_ref_len(const OgeTextParams &tp, int32_t id) { return tp.name_off[id + 1] - tp.name_off[id]; }

// The text length of the record and its mark: OGE_TXT_HOST for a record with an f or B tag (length 0, the host
// formats it), OGE_TXT_BAD for a record whose tags or lengths do not parse (length 0).  One pass over the tags.
OGE_HD uint64_t oge_text_record_size(const uint8_t *rec, const OgeTextParams &tp, uint32_t *mark) {
    OgeTextRec r;
    *mark = OGE_TXT_BAD;
    if (!oge_text_parse(rec, r)) return 0;
    if (tp.mode != 0) {  // FASTQ: @name \n SEQ \n +name \n QUAL \n
        uint32_t first, sl;
        oge_text_trim_window(tp, r.l_seq, &first, &sl);
        *mark = OGE_TXT_DEVICE;
        return 2ull * (r.l_name - 1) + 2ull * sl + 6;
    }
    uint64_t len = (uint64_t)(r.l_name - 1) + 1 + oge_txt_dec_width(r.flag) + 1;
    len += (r.refid >= 0 && r.refid < tp.n_ref ? oge_text_ref_len(tp, r.refid) : 1u) + 1;
    len += oge_txt_sdec_width((int64_t)r.pos + 1) + 1 + oge_txt_dec_width(r.mapq) + 1;
    if (r.n_cigar == 0) len += 1;
    for (uint32_t k = 0; k < r.n_cigar; ++k) len += oge_txt_dec_width(oge_txt_ld32(r.cigar + 4 * k) >> 4) + 1;
    len += 1;
    if ((r.flag & OGE_F_PAIRED) && r.mref >= 0 && r.mref < tp.n_ref) {
        len += (r.mref == r.refid ? 1u : oge_text_ref_len(tp, r.mref)) + 1;
        len += oge_txt_sdec_width((int64_t)r.mpos + 1) + 1 + oge_txt_sdec_width(r.tlen) + 1;
    } else {
        len += 6;
    }
    len += r.l_seq ? 2ull * r.l_seq + 1 : 3;
    bool host = false;
    const uint8_t *t = r.tags;
    const uint32_t tl = r.tag_len;
    uint32_t i = 0;
    while (i < tl) {
        if (tl - i < 3) return 0;
        const uint32_t type = t[i + 2];
        i += 3;
        len += 6;  // \tXX:T:
        const uint32_t left = tl - i;
        if (type == 'A') {
            if (left < 1) return 0;
            len += 1;
            i += 1;
        } else if (type == 'c' || type == 'C') {
            if (left < 1) return 0;
            len += type == 'c' ? oge_txt_sdec_width((int8_t)t[i]) : oge_txt_dec_width(t[i]);
            i += 1;
        } else if (type == 's' || type == 'S') {
            if (left < 2) return 0;
            const uint32_t v = oge_txt_ld32(t + i) & 0xFFFF;
            len += type == 's' ? oge_txt_sdec_width((int16_t)v) : oge_txt_dec_width(v);
            i += 2;
        } else if (type == 'i' || type == 'I') {
            if (left < 4) return 0;
            const uint32_t v = oge_txt_ld32(t + i);
            len += type == 'i' ? oge_txt_sdec_width((int32_t)v) : oge_txt_dec_width(v);
            i += 4;
        } else if (type == 'Z' || type == 'H') {
            while (i < tl && t[i]) {
                ++i;
                ++len;
            }
            if (i >= tl) return 0;  // no NUL inside the record
            ++i;
        } else if (type == 'f') {
            if (left < 4) return 0;
            host = true;
            i += 4;
        } else if (type == 'B') {
            if (left < 5) return 0;
            const uint32_t es = oge_txt_b_elem(t[i]);
            const uint64_t cnt = oge_txt_ld32(t + i + 1);
            if (!es || cnt * es > left - 5) return 0;
            host = true;
            i += 5 + (uint32_t)cnt * es;
        } else {
            return 0;
        }
        if (i < tl && t[i] == 0) break;  // sam_writer.cpp:210: a NUL behind a tag's value ends the list
    }
    len += 1;
    if (len > 0xFFFFFF00ull) return 0;
    *mark = host ? OGE_TXT_HOST : OGE_TXT_DEVICE;
    return host ? 0 : len;
}

// ------------------------------------------------------------------------------------------------ emit
struct OgeTxt32 {  // up to 32 characters in wave-uniform registers
    uint64_t w0, w1, w2, w3;
    uint32_t n;
};
OGE_HD void oge_txt_clear(OgeTxt32 &b) { b.w0 = b.w1 = b.w2 = b.w3 = 0; b.n = 0; }
OGE_HD void oge_txt_set(OgeTxt32 &b, uint32_t at, uint32_t c) {
    const uint64_t v = (uint64_t)(c & 0xFF) << (8 * (at & 7));
    const uint32_t k = at >> 3;
    if (k == 0) b.w0 |= v;
    else if (k == 1) b.w1 |= v;
    else if (k == 2) b.w2 |= v;
    else if (k == 3) b.w3 |= v;
}
OGE_HD void oge_txt_put(OgeTxt32 &b, uint32_t c) { oge_txt_set(b, b.n++, c); }
OGE_HD void oge_txt_dec(OgeTxt32 &b, uint32_t v) {
    const uint32_t w = oge_txt_dec_width(v);
    for (uint32_t k = w; k-- > 0;) {
        oge_txt_set(b, b.n + k, '0' + v % 10u);
        v /= 10u;
    }
    b.n += w;
}
OGE_HD void oge_txt_sdec(OgeTxt32 &b, int64_t v) {
    if (v < 0) {
        oge_txt_put(b, '-');
        v = -v;
    }
    oge_txt_dec(b, (uint32_t)v);
}

struct OgeTxtOut {
    uint8_t *p;      // the record's first output byte
    uint32_t o, end; // bytes placed so far; the record's text length (nothing is stored at or past it)
    uint32_t lane;
};

OGE_HD void oge_txt_flush(OgeTxtOut &out, OgeTxt32 &b) {
    if (b.n && out.o + b.n <= out.end && out.lane < b.n) {
        const uint32_t k = out.lane >> 3;
        const uint64_t w = k == 0 ? b.w0 : k == 1 ? b.w1 : k == 2 ? b.w2 : b.w3;
        out.p[out.o + out.lane] = (uint8_t)(w >> (8 * (out.lane & 7)));
    }
    out.o += b.n;
    oge_txt_clear(b);
}

// len characters, four at a time from gen(i) = characters i .. i + 3 (character i in the low byte)
template <class Gen>
OGE_HD void oge_txt_bulk(OgeTxtOut &out, uint32_t len, Gen gen) {
    if (len && out.o + len <= out.end) {
        uint8_t *p = out.p + out.o;
        const uint32_t mis = (uint32_t)(0 - (uintptr_t)p) & 3u;
        const uint32_t head = mis < len ? mis : len;
        const uint32_t mid = (len - head) >> 2, tail = (len - head) & 3u;
        const uint32_t lane = out.lane;
        if (lane < head) p[lane] = (uint8_t)gen(lane);
        else if (lane >= 4 && lane < 4 + tail) {
            const uint32_t i = head + 4 * mid + (lane - 4);
            p[i] = (uint8_t)gen(i);
        }
        for (uint32_t j = lane; j < mid; j += 64) {
            const uint32_t i = head + 4 * j;
            *(uint32_t *)(p + i) = gen(i);
        }
    }
    out.o += len;
}

struct OgeTxtCopy {  // bytes as they are
    const uint8_t *s;
    OGE_HDM uint32_t operator()(uint32_t i) const { return oge_txt_ld32(s + i); }
};
struct OgeTxtQual {  // each byte + 33, wrapping at 8 bits
    const uint8_t *s;
    OGE_HDM uint32_t operator()(uint32_t i) const {
        const uint32_t x = oge_txt_ld32(s + i);
        return ((x & 0x7F7F7F7Fu) + 0x21212121u) ^ (x & 0x80808080u);
    }
};
struct OgeTxtSeq {  // 4-bit codes from base `first` on -> "=ACMGRSVTWYHKDBN"
    const uint8_t *s;
    uint32_t first;
    OGE_HDM uint32_t operator()(uint32_t i) const {
        const uint32_t b = first + i;
        const uint32_t w = oge_txt_ld32(s + (b >> 1));
        // nibble k of the stream at bits [4k, 4k + 4): swap the halves of every byte
        const uint32_t ws = ((w & 0x0F0F0F0Fu) << 4) | ((w >> 4) & 0x0F0F0F0Fu);
        const uint32_t y = ws >> (4 * (b & 1));
        const uint32_t c4 = (y & 0xFu) | ((y & 0xF0u) << 4) | ((y & 0xF00u) << 8) | ((y & 0xF000u) << 12);  // one code per byte
        uint32_t r = 0;
#if defined(__HIP_DEVICE_COMPILE__)
        const uint32_t sel = c4 & 0x07070707u, hi = ((c4 >> 3) & 0x01010101u) * 0xFFu;
        const uint32_t a = __builtin_amdgcn_perm(0x56535247u /* GRSV */, 0x4D43413Du /* =ACM */, sel);
        const uint32_t z = __builtin_amdgcn_perm(0x4E42444Bu /* KDBN */, 0x48595754u /* TWYH */, sel);
        r = (a & ~hi) | (z & hi);
#else
        const char *lut = "=ACMGRSVTWYHKDBN";
        for (int k = 0; k < 4; ++k) r |= (uint32_t)(uint8_t)lut[(c4 >> (8 * k)) & 15] << (8 * k);
#endif
        return r;
    }
};

// The record's text at p[0, len), len = what oge_text_record_size returned (> 0: a record the device formats).
OGE_HD void oge_text_record_emit(const uint8_t *rec, const OgeTextParams &tp, uint8_t *p, uint32_t len, uint32_t lane) {
    OgeTextRec r;
    if (!oge_text_parse(rec, r)) return;
    OgeTxtOut out = {p, 0, len, lane};
    OgeTxt32 b;
    oge_txt_clear(b);
    const uint32_t l_name = OGE_TXT_UNI(r.l_name), l_seq = OGE_TXT_UNI(r.l_seq);
    if (tp.mode != 0) {
        uint32_t first, sl;
        oge_text_trim_window(tp, l_seq, &first, &sl);
        oge_txt_put(b, '@');
        oge_txt_flush(out, b);
        oge_txt_bulk(out, l_name - 1, OgeTxtCopy{r.name});
        oge_txt_put(b, '\n');
        oge_txt_flush(out, b);
        oge_txt_bulk(out, sl, OgeTxtSeq{r.seq, first});
        oge_txt_put(b, '\n');
        oge_txt_put(b, '+');
        oge_txt_flush(out, b);
        oge_txt_bulk(out, l_name - 1, OgeTxtCopy{r.name});
        oge_txt_put(b, '\n');
        oge_txt_flush(out, b);
        oge_txt_bulk(out, sl, OgeTxtQual{r.qual + first});
        oge_txt_put(b, '\n');
        oge_txt_flush(out, b);
        return;
    }
    const uint32_t flag = OGE_TXT_UNI(r.flag), mapq = OGE_TXT_UNI(r.mapq), n_cigar = OGE_TXT_UNI(r.n_cigar);
    const int32_t refid = (int32_t)OGE_TXT_UNI(r.refid), pos = (int32_t)OGE_TXT_UNI(r.pos), mref = (int32_t)OGE_TXT_UNI(r.mref),
                  mpos = (int32_t)OGE_TXT_UNI(r.mpos), tlen = (int32_t)OGE_TXT_UNI(r.tlen);
    // QNAME \t FLAG \t RNAME
    oge_txt_bulk(out, l_name - 1, OgeTxtCopy{r.name});
    oge_txt_put(b, '\t');
    oge_txt_dec(b, flag);
    oge_txt_put(b, '\t');
    if (refid >= 0 && refid < tp.n_ref) {
        oge_txt_flush(out, b);
        const uint32_t a = OGE_TXT_UNI(tp.name_off[refid]), z = OGE_TXT_UNI(tp.name_off[refid + 1]);
        oge_txt_bulk(out, z - a, OgeTxtCopy{tp.names + a});
    } else {
        oge_txt_put(b, '*');
    }
    // \t POS \t MAPQ \t CIGAR
    oge_txt_put(b, '\t');
    oge_txt_sdec(b, (int64_t)pos + 1);
    oge_txt_put(b, '\t');
    oge_txt_dec(b, mapq);
    oge_txt_put(b, '\t');
    if (n_cigar == 0) oge_txt_put(b, '*');
    for (uint32_t k = 0; k < n_cigar; ++k) {
        oge_txt_flush(out, b);
        const uint32_t op = OGE_TXT_UNI(oge_txt_ld32(r.cigar + 4 * k));
        oge_txt_dec(b, op >> 4);
        oge_txt_put(b, oge_txt_cigar_letter(op & 15));
    }
    oge_txt_flush(out, b);
    // \t mate
    oge_txt_put(b, '\t');
    if ((flag & OGE_F_PAIRED) && mref >= 0 && mref < tp.n_ref) {
        if (mref == refid) {
            oge_txt_put(b, '=');
        } else {
            oge_txt_flush(out, b);
            const uint32_t a = OGE_TXT_UNI(tp.name_off[mref]), z = OGE_TXT_UNI(tp.name_off[mref + 1]);
            oge_txt_bulk(out, z - a, OgeTxtCopy{tp.names + a});
        }
        oge_txt_put(b, '\t');
        oge_txt_sdec(b, (int64_t)mpos + 1);
        oge_txt_put(b, '\t');
        oge_txt_sdec(b, tlen);
        oge_txt_put(b, '\t');
    } else {
        oge_txt_put(b, '*');
        oge_txt_put(b, '\t');
        oge_txt_put(b, '0');
        oge_txt_put(b, '\t');
        oge_txt_put(b, '0');
        oge_txt_put(b, '\t');
    }
    // SEQ \t QUAL
    if (l_seq == 0) {
        oge_txt_put(b, '*');
        oge_txt_put(b, '\t');
        oge_txt_put(b, '*');
        oge_txt_flush(out, b);
    } else {
        oge_txt_flush(out, b);
        oge_txt_bulk(out, l_seq, OgeTxtSeq{r.seq, 0});
        oge_txt_put(b, '\t');
        oge_txt_flush(out, b);
        oge_txt_bulk(out, l_seq, OgeTxtQual{r.qual});
    }
    // tags: the walk oge_text_record_size accepted
    const uint8_t *t = r.tags;
    const uint32_t tl = OGE_TXT_UNI(r.tag_len);
    uint32_t i = 0;
    while (i + 3 <= tl) {
        const uint32_t h = OGE_TXT_UNI(oge_txt_ld32(t + i));
        const uint32_t type = (h >> 16) & 0xFF;
        i += 3;
        oge_txt_put(b, '\t');
        oge_txt_put(b, h);
        oge_txt_put(b, h >> 8);
        oge_txt_put(b, ':');
        oge_txt_put(b, type == 'A' || type == 'Z' || type == 'H' ? type : 'i');
        oge_txt_put(b, ':');
        if (type == 'Z' || type == 'H') {
            oge_txt_flush(out, b);
            uint32_t e = i;
            while (e < tl) {  // four bytes at a time
                const uint32_t x = OGE_TXT_UNI(oge_txt_ld32(t + e));
                if (((x - 0x01010101u) & ~x & 0x80808080u) == 0) {
                    e += 4;
                    continue;
                }
                e += (x & 0xFF) == 0 ? 0 : (x & 0xFF00) == 0 ? 1 : (x & 0xFF0000) == 0 ? 2 : 3;
                break;
            }
            if (e > tl) e = tl;
            oge_txt_bulk(out, e - i, OgeTxtCopy{t + i});
            i = e + 1;
        } else {
            const uint32_t v = OGE_TXT_UNI(oge_txt_ld32(t + i));
            if (type == 'A') {
                oge_txt_put(b, v);
                i += 1;
            } else if (type == 'c') {
                oge_txt_sdec(b, (int8_t)v);
                i += 1;
            } else if (type == 'C') {
                oge_txt_dec(b, v & 0xFF);
                i += 1;
            } else if (type == 's') {
                oge_txt_sdec(b, (int16_t)v);
                i += 2;
            } else if (type == 'S') {
                oge_txt_dec(b, v & 0xFFFF);
                i += 2;
            } else if (type == 'i') {
                oge_txt_sdec(b, (int32_t)v);
                i += 4;
            } else if (type == 'I') {
                oge_txt_dec(b, v);
                i += 4;
            } else {
                return;  // not a record the device formats
            }
            oge_txt_flush(out, b);
        }
        if (i < tl && OGE_TXT_UNI(t[i]) == 0) break;
    }
    oge_txt_put(b, '\n');
    oge_txt_flush(out, b);
}
