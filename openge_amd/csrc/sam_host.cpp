// sam_host.cpp -- one record's SAM line or FASTQ entry on the host, for the records the device marks
// (an f tag needs printf's %g, a B array is outside the reference's switch).  Written
// on its own, with strings and snprintf, not shared with the kernels' sam_format.h: the two must agree byte
// for byte on every record both can format.  And the other direction: one SAM line's BAM
// record with every tag type (f by strtof, B elements by their type), for the lines the device's parser marks;
// written on its own as well, not shared with the kernels' sam_parse.h.
#include "sam_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "bam_layout.h"

namespace {

std::string ref_name(const oge_text_opts *o, int32_t id) {
    return std::string(o->ref_names + o->ref_name_off[id], o->ref_names + o->ref_name_off[id + 1]);
}

void put_g(std::string &out, const uint8_t *p) {
    float f;
    memcpy(&f, p, 4);
    char buf[48];
    snprintf(buf, sizeof buf, "%g", (double)f);
    out += buf;
}

}  // namespace

bool oge_text_line_host(const uint8_t *rec, uint64_t rec_bytes, const oge_text_opts *o, std::string &out, std::string &err) {
    if (rec_bytes < 36 || (uint64_t)oge_rd_u32(rec) + 4 != rec_bytes) {
        err = "the record's block_size does not match its length";
        return false;
    }
    const int32_t refid = oge_rd_i32(rec + OGE_OFF_REFID), pos = oge_rd_i32(rec + OGE_OFF_POS);
    const uint32_t l_name = rec[OGE_OFF_LNAME], mapq = rec[OGE_OFF_MAPQ], n_cigar = oge_rd_u16(rec + OGE_OFF_NCIGAR),
                   flag = oge_rd_u16(rec + OGE_OFF_FLAG);
    const int32_t l_seq = oge_rd_i32(rec + OGE_OFF_LSEQ), mref = oge_rd_i32(rec + OGE_OFF_MREFID), mpos = oge_rd_i32(rec + OGE_OFF_MPOS),
                  tlen = oge_rd_i32(rec + OGE_OFF_TLEN);
    const uint64_t var = (uint64_t)l_name + 4ull * n_cigar + (l_seq < 0 ? 0 : ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq);
    if (l_seq < 0 || l_name < 1 || 36 + var > rec_bytes) {
        err = "the record's lengths do not fit its block_size";
        return false;
    }
    const uint8_t *name = rec + OGE_OFF_NAME, *cig = name + l_name, *seq = cig + 4ull * n_cigar, *qual = seq + ((uint64_t)l_seq + 1) / 2,
                  *tags = qual + l_seq, *end = rec + rec_bytes;
    auto bases = [&](uint64_t a, uint64_t z) {
        for (uint64_t i = a; i < z; ++i) out += "=ACMGRSVTWYHKDBN"[(seq[i >> 1] >> ((i & 1) ? 0 : 4)) & 15];
    };
    auto quals = [&](uint64_t a, uint64_t z) {
        for (uint64_t i = a; i < z; ++i) out += (char)(uint8_t)(qual[i] + 33);
    };
    const std::string qname((const char *)name, l_name - 1);
    if (o->mode == OGE_TEXT_FASTQ) {
        const uint64_t cut = (uint64_t)o->trim_begin + (uint64_t)o->trim_end;
        const uint64_t a = (uint64_t)l_seq > cut ? (uint64_t)o->trim_begin : 0, z = (uint64_t)l_seq > cut ? (uint64_t)l_seq - o->trim_end : 0;
        out += '@';
        out += qname;
        out += '\n';
        bases(a, z);
        out += "\n+";
        out += qname;
        out += '\n';
        quals(a, z);
        out += '\n';
        return true;
    }
    out += qname;
    out += '\t' + std::to_string(flag) + '\t';
    out += refid >= 0 && refid < o->n_ref ? ref_name(o, refid) : std::string("*");
    out += '\t' + std::to_string((int64_t)pos + 1) + '\t' + std::to_string(mapq) + '\t';
    if (!n_cigar) out += '*';
    for (uint32_t k = 0; k < n_cigar; ++k) {
        const uint32_t op = oge_rd_u32(cig + 4 * k);
        out += std::to_string(op >> 4);
        out += (op & 15) <= 8 ? "MIDNSHP=X"[op & 15] : '?';
    }
    out += '\t';
    if ((flag & OGE_F_PAIRED) && mref >= 0 && mref < o->n_ref) {
        out += mref == refid ? std::string("=") : ref_name(o, mref);
        out += '\t' + std::to_string((int64_t)mpos + 1) + '\t' + std::to_string(tlen) + '\t';
    } else {
        out += "*\t0\t0\t";
    }
    if (l_seq == 0) {
        out += "*\t*";
    } else {
        bases(0, l_seq);
        out += '\t';
        quals(0, l_seq);
    }
    const uint8_t *t = tags;
    while (t < end) {
        if (end - t < 3) {
            err = "a tag is cut short";
            return false;
        }
        const char type = (char)t[2];
        out += '\t';
        out += (char)t[0];
        out += (char)t[1];
        out += ':';
        t += 3;
        const uint64_t left = (uint64_t)(end - t);
        const uint64_t need = type == 'A' || type == 'c' || type == 'C' ? 1 : type == 's' || type == 'S' ? 2
                              : type == 'i' || type == 'I' || type == 'f' ? 4 : type == 'B' ? 5 : 0;
        if (left < need) {
            err = "a tag is cut short";
            return false;
        }
        switch (type) {
            case 'A': out += "A:"; out += (char)t[0]; t += 1; break;
            case 'c': out += "i:" + std::to_string((int)(int8_t)t[0]); t += 1; break;
            case 'C': out += "i:" + std::to_string((unsigned)t[0]); t += 1; break;
            case 's': out += "i:" + std::to_string((int)(int16_t)oge_rd_u16(t)); t += 2; break;
            case 'S': out += "i:" + std::to_string((unsigned)oge_rd_u16(t)); t += 2; break;
            case 'i': out += "i:" + std::to_string(oge_rd_i32(t)); t += 4; break;
            case 'I': out += "i:" + std::to_string(oge_rd_u32(t)); t += 4; break;
            case 'f': out += "f:"; put_g(out, t); t += 4; break;
            case 'Z':
            case 'H': {
                const uint8_t *z = (const uint8_t *)memchr(t, 0, left);
                if (!z) {
                    err = "a string tag has no end";
                    return false;
                }
                out += type;
                out += ':';
                out.append((const char *)t, (size_t)(z - t));
                t = z + 1;
                break;
            }
            case 'B': {
                const char sub = (char)t[0];
                const uint64_t cnt = oge_rd_u32(t + 1);
                const uint64_t es = sub == 'c' || sub == 'C' ? 1 : sub == 's' || sub == 'S' ? 2 : sub == 'i' || sub == 'I' || sub == 'f' ? 4 : 0;
                if (!es || cnt * es > left - 5) {
                    err = es ? "an array tag is cut short" : std::string("unknown array element type '") + sub + "'";
                    return false;
                }
                out += "B:";
                out += sub;
                t += 5;
                for (uint64_t k = 0; k < cnt; ++k, t += es) {
                    out += ',';
                    switch (sub) {
                        case 'c': out += std::to_string((int)(int8_t)t[0]); break;
                        case 'C': out += std::to_string((unsigned)t[0]); break;
                        case 's': out += std::to_string((int)(int16_t)oge_rd_u16(t)); break;
                        case 'S': out += std::to_string((unsigned)oge_rd_u16(t)); break;
                        case 'i': out += std::to_string(oge_rd_i32(t)); break;
                        case 'I': out += std::to_string(oge_rd_u32(t)); break;
                        default: put_g(out, t); break;
                    }
                }
                break;
            }
            default:
                err = std::string("unknown tag type '") + type + "'";
                return false;
        }
        if (t < end && *t == 0) break;  // sam_writer.cpp:210
    }
    out += '\n';
    return true;
}

// ------------------------------------------------------------------------------------------ SAM line -> record
namespace {

bool parse_num(const std::string &s, long long lo, long long hi, long long *out) {
    const size_t i = s.size() && s[0] == '-' ? 1 : 0;
    if (i >= s.size()) return false;
    for (size_t k = i; k < s.size(); ++k)
        if (s[k] < '0' || s[k] > '9') return false;
    size_t z = i;
    while (z < s.size() && s[z] == '0') ++z;
    if (s.size() - z > 18) return false;  // past every field's range (and strtoll's)
    const long long v = strtoll(s.c_str(), nullptr, 10);
    if (v < lo || v > hi) return false;
    *out = v;
    return true;
}

int contig_id(const oge_text_opts *o, const std::string &name) {
    for (int32_t r = 0; r < o->n_ref; ++r)
        if (o->ref_name_off[r + 1] - o->ref_name_off[r] == name.size() && !memcmp(o->ref_names + o->ref_name_off[r], name.data(), name.size()))
            return r;
    return -2;
}

void put32(std::vector<uint8_t> &v, uint32_t x) {
    for (int k = 0; k < 4; ++k) v.push_back((uint8_t)(x >> (8 * k)));
}
void put_le(std::vector<uint8_t> &v, uint64_t x, int bytes) {
    for (int k = 0; k < bytes; ++k) v.push_back((uint8_t)(x >> (8 * k)));
}

}  // namespace

bool oge_sam_record_host(const uint8_t *line, uint64_t len, const oge_text_opts *o, std::vector<uint8_t> &out, bool *warn, std::string &err) {
    *warn = false;
    if (len < 10) return err = "the line is shorter than 10 characters", false;
    std::vector<std::string> f;
    {
        size_t a = 0;
        const char *p = (const char *)line;
        for (size_t i = 0; i <= len; ++i)
            if (i == len || p[i] == '\t') f.emplace_back(p + a, i - a), a = i + 1;
    }
    if (f.size() < 11) return err = "fewer than 11 fields", false;
    long long flag, pos, mapq, pnext, tlen;
    if (f[0].size() > 254) return err = "QNAME", false;
    if (!parse_num(f[1], 0, 65535, &flag)) return err = "FLAG", false;
    int refid = -1, mref = -1;
    if (f[2] != "*" && (refid = contig_id(o, f[2])) < 0) return err = "RNAME", false;
    if (!parse_num(f[3], -2147483647LL, 2147483648LL, &pos)) return err = "POS", false;
    if (!parse_num(f[4], 0, 255, &mapq)) return err = "MAPQ", false;
    std::vector<uint32_t> cigar;
    if (f[5] != "*") {
        const std::string &c = f[5];
        size_t i = 0;
        if (c.empty()) return err = "CIGAR", false;
        while (i < c.size()) {
            size_t d = i;
            while (d < c.size() && c[d] >= '0' && c[d] <= '9') ++d;
            long long n;
            const char *ops = "MIDNSHP=X", *w = d < c.size() ? strchr(ops, c[d]) : nullptr;
            if (d == i || !w || !*w || !parse_num(c.substr(i, d - i), 0, (1 << 28) - 1, &n)) return err = "CIGAR", false;
            cigar.push_back((uint32_t)n << 4 | (uint32_t)(w - ops));
            i = d + 1;
        }
        if (cigar.size() > 65535) return err = "CIGAR (more than 65535 operations)", false;
    }
    if (f[6] == "=") mref = refid;
    else if (f[6] != "*" && (mref = contig_id(o, f[6])) < 0) mref = -1, *warn = true;
    if (!parse_num(f[7], -2147483647LL, 2147483648LL, &pnext)) return err = "PNEXT", false;
    if (!parse_num(f[8], -2147483648LL, 2147483647LL, &tlen)) return err = "TLEN", false;
    const std::string seq = f[9] == "*" ? std::string() : f[9];
    if (f[10] != "*" && f[10].size() != seq.size()) return err = "QUAL", false;
    uint32_t span = 0;
    for (uint32_t op : cigar)
        if ((op & 15) == OGE_CIG_M || (op & 15) == OGE_CIG_D || (op & 15) == OGE_CIG_N || (op & 15) == OGE_CIG_EQ || (op & 15) == OGE_CIG_X) span += op >> 4;
    const int32_t p0 = (int32_t)(pos - 1);
    const uint32_t bin = oge_reg2bin(p0, (int32_t)((uint32_t)p0 + span)) & 0xFFFF;
    out.clear();
    put32(out, 0);
    put32(out, (uint32_t)refid);
    put32(out, (uint32_t)p0);
    put32(out, bin << 16 | (uint32_t)mapq << 8 | (uint32_t)(f[0].size() + 1));
    put32(out, (uint32_t)flag << 16 | (uint32_t)cigar.size());
    put32(out, (uint32_t)seq.size());
    put32(out, (uint32_t)mref);
    put32(out, (uint32_t)(int32_t)(pnext - 1));
    put32(out, (uint32_t)(int32_t)tlen);
    out.insert(out.end(), f[0].begin(), f[0].end());
    out.push_back(0);
    for (uint32_t op : cigar) put32(out, op);
    auto code = [](char c) -> uint32_t {
        const char *lut = "=ACMGRSVTWYHKDBN", *w = strchr(lut, c >= 'a' && c <= 'z' ? c - 32 : c);
        return w && *w ? (uint32_t)(w - lut) : 15u;
    };
    for (size_t i = 0; i < seq.size(); i += 2) out.push_back((uint8_t)(code(seq[i]) << 4 | (i + 1 < seq.size() ? code(seq[i + 1]) : 0)));
    for (size_t i = 0; i < seq.size(); ++i) out.push_back(f[10] == "*" ? 0xFF : (uint8_t)(f[10][i] - 33));
    for (size_t k = 11; k < f.size(); ++k) {
        const std::string &t = f[k];
        if (t.size() < 5 || t[2] != ':' || t[4] != ':') return err = "tag " + std::to_string(k - 10) + " is not shaped XX:T:value", false;
        const std::string v = t.substr(5), nm = t.substr(0, 2);
        const char ty = t[3];
        out.push_back((uint8_t)t[0]);
        out.push_back((uint8_t)t[1]);
        long long iv;
        if (ty == 'A') {
            if (v.size() != 1) return err = "tag " + nm, false;
            out.push_back('A');
            out.push_back((uint8_t)v[0]);
        } else if (ty == 'i') {
            if (!parse_num(v, -2147483648LL, 4294967295LL, &iv)) return err = "tag " + nm + " (integer)", false;
            const char bt = iv >= 0 ? (iv <= 255 ? 'C' : iv <= 65535 ? 'S' : 'I') : (iv >= -128 ? 'c' : iv >= -32768 ? 's' : 'i');
            out.push_back((uint8_t)bt);
            put_le(out, (uint64_t)iv, bt == 'C' || bt == 'c' ? 1 : bt == 'S' || bt == 's' ? 2 : 4);
        } else if (ty == 'f') {
            char *end = nullptr;
            const float x = strtof(v.c_str(), &end);
            if (v.empty() || *end) return err = "tag " + nm + " (float)", false;
            uint32_t raw;
            memcpy(&raw, &x, 4);
            out.push_back('f');
            put32(out, raw);
        } else if (ty == 'Z' || ty == 'H') {
            out.push_back((uint8_t)ty);
            out.insert(out.end(), v.begin(), v.end());
            out.push_back(0);
        } else if (ty == 'B') {
            const char sub = v.empty() ? 0 : v[0];
            const int w = sub == 'c' || sub == 'C' ? 1 : sub == 's' || sub == 'S' ? 2 : sub == 'i' || sub == 'I' || sub == 'f' ? 4 : 0;
            if (!w || (v.size() > 1 && v[1] != ',')) return err = "tag " + nm + " (array)", false;
            std::vector<std::string> el;
            for (size_t a = 2, i = 2; v.size() > 1 && i <= v.size(); ++i)
                if (i == v.size() || v[i] == ',') el.emplace_back(v, a, i - a), a = i + 1;
            out.push_back('B');
            out.push_back((uint8_t)sub);
            put32(out, (uint32_t)el.size());
            for (const std::string &e : el) {
                if (sub == 'f') {
                    char *end = nullptr;
                    const float x = strtof(e.c_str(), &end);
                    if (e.empty() || *end) return err = "tag " + nm + " (array element)", false;
                    uint32_t raw;
                    memcpy(&raw, &x, 4);
                    put32(out, raw);
                } else {
                    const long long lo = sub == 'c' ? -128 : sub == 's' ? -32768 : sub == 'i' ? -2147483648LL : 0;
                    const long long hi = sub == 'c' ? 127 : sub == 'C' ? 255 : sub == 's' ? 32767 : sub == 'S' ? 65535 : sub == 'i' ? 2147483647LL : 4294967295LL;
                    if (!parse_num(e, lo, hi, &iv)) return err = "tag " + nm + " (array element)", false;
                    put_le(out, (uint64_t)iv, w);
                }
            }
        } else {
            return err = "tag " + nm + " has a type outside AifZHB", false;
        }
    }
    if (out.size() > 0x7FFFFFF0ull) return err = "the line is too long", false;
    const uint32_t bs = (uint32_t)out.size() - 4;
    for (int k = 0; k < 4; ++k) out[k] = (uint8_t)(bs >> (8 * k));
    return true;
}
