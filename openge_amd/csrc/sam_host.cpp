// sam_host.cpp -- one record's SAM line or FASTQ entry on the host, for the records the device marks
// (an f tag needs printf's %g, a B array is outside the reference's switch).  Written
// on its own, with strings and snprintf, not shared with the kernels' sam_format.h: the two must agree byte
// for byte on every record both can format.
#include "sam_host.h"

#include <cstdio>
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
