// calmd.hip -- `openge calmd`: the NM and MD tags of records resident in HBM recomputed against the reference
// sequence, which is uploaded once per FASTA and contig list (definitions in DESIGN.md section 28 and
// include/openge_hip.h; the model is tests/calmd_model.py).  Every record is rewritten independently of the others:
// the result does not depend on the order in which the waves run.
//
//   ref      the FASTA through the realigner's loader (fasta.h), the sequences of the header's contigs back to back,
//            upper-cased, with an (offset, length) pair per contig; kept in HBM until the FASTA's path, size or
//            mtime or the contig list changes
//   size     k_cm_size    one wave per record: the CIGAR checked lane-parallel, ONE walk over the tags (first NM, first
//                         MD, every tag checked against block_size), then the ops wave-uniformly -- inside an
//                         M, = or X op 64 bases at a time, one lane per base, the read's nibble against the
//                         reference byte, the mismatch lanes by ballot.  nm is a popcount, the MD length the widths
//                         of the gaps between the mask's set bits; an MD tag that is there is compared on the fly
//                         at the positions the new bytes would take.  Stores the new record size and a 16-byte
//                         decision for the emit pass.  Counters: per-wave sums, ONE 64-bit atomic per workgroup
//                         and counter; a fault is an atomicMin of the record index, taken only when it happens
//   scan     the existing 64-bit exclusive scan of the sizes
//   emit     k_cm_emit    one wave per record: the record minus the removed tag spans as aligned dwords of the
//                         destination put together from the two source dwords each straddles, block_size, the NM
//                         tag, and the MD bytes from the same walk -- a mismatch lane stores its number and its
//                         letter at the wave prefix sum of the widths, every byte once at its final offset
#include <hip/hip_runtime.h>
#include <sys/stat.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "bam_layout.h"
#include "dev_util.h"
#include "fasta.h"
#include "oge_ctx.h"
#include "sam_format.h"

namespace {

constexpr int kT = 256;
constexpr int kWaves = kT / 64;
constexpr unsigned long long kNone = ~0ull;
enum { kBadRef, kBadBlock, kBadCigar, kBadOp, kBadTags, kBadQlen, kLimit, kNBad };
enum { kUsed = 1, kAddNM = 2, kAddMD = 4 };  // flags of a record's decision

struct CalAcc {
    unsigned long long cnt[4];      // skipped, no_reference, nm_changed, md_changed
    unsigned long long bad[kNBad];  // the lowest record with each fault (kNone: none)
};

struct CalRef {
    const uint8_t *bytes;
    const int64_t *off, *len;  // per contig: where its sequence starts in bytes (-1: the FASTA lacks it), its length
};

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// the code of a reference byte in "=ACMGRSVTWYHKDBN", 15 for any other byte
__device__ __forceinline__ uint32_t ref_code(uint32_t b) {
    constexpr uint64_t lo = 0xFFF3FCFFB4FFD2E1ull;  // A..P, a nibble each
    constexpr uint64_t hi = 0xFAF97F865Full;        // Q..Z
    if (b == '=') return 0;
    const uint32_t k = b - 'A';
    if (k >= 26) return 15;
    return (uint32_t)((k < 16 ? lo >> (4 * k) : hi >> (4 * (k - 16))) & 15);
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)v, d, 64);
        if (lane >= (uint32_t)d) v += y;
    }
    return v;
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

// Where the bytes of the new MD value go.  The size pass compares them with the value of the MD tag that is
// there (old == nullptr: nothing to compare); the emit pass stores them, each once, below cap = the length the
// size pass found.
template <bool EMIT>
struct MdSink {
    const uint8_t *old;
    uint8_t *out;
    uint32_t lim;  // size pass: the old value's length; emit pass: the new value's
    bool diff;
    __device__ __forceinline__ void put(uint64_t pos, uint32_t c) {
        if (EMIT) {
            if (pos < lim) out[pos] = (uint8_t)c;
        } else if (old) {
            if (pos >= lim || old[pos] != c) diff = true;
        }
    }
    __device__ __forceinline__ void dec(uint64_t pos, uint32_t v, uint32_t w) {
        if (!EMIT && !old) return;
        for (uint32_t k = w; k-- > 0;) {
            put(pos + k, '0' + v % 10u);
            v /= 10u;
        }
    }
    // c bytes of the reference from pos on, lane-strided
    __device__ __forceinline__ void span(uint64_t pos, const uint8_t *src, uint32_t c, uint32_t lane) {
        if (!EMIT) {
            if (!old) return;
            if (pos + c > lim) {  // the rest cannot match: compare what the old value has
                diff = true;
                c = pos < lim ? (uint32_t)(lim - pos) : 0;
            }
        }
        for (uint32_t k = lane; k < c; k += 64) put(pos + k, src[k]);
    }
};

// The walk of the definition over one record, by one wave: cig (nops ops, every code <= 8), the packed bases at
// seq (the ops' query lengths sum to l_seq), the contig's sequence at ref (rlen bytes), x0 = pos.  Returns nm and
// the MD value's length; the bytes go to the sink.
template <bool EMIT>
__device__ __forceinline__ void md_walk(const uint8_t *cig, uint32_t nops, const uint8_t *seq, const uint8_t *ref, uint64_t rlen, uint32_t x0,
                                        uint32_t lane, MdSink<EMIT> &s, uint64_t &nm_out, uint64_t &md_out) {
    uint64_t x = x0, nm = 0, pos = 0;
    uint32_t y = 0, run = 0;
    bool ended = false;
    for (uint32_t j = 0; j < nops && !ended; ++j) {
        const uint32_t op = uni(oge_ldu32(cig + 4 * j)), code = op & 0xF, len = op >> 4;
        if (code == OGE_CIG_M || code == OGE_CIG_EQ || code == OGE_CIG_X) {
            for (uint32_t k = 0; k < len && !ended; k += 64) {
                uint32_t v = len - k < 64 ? len - k : 64;
                const uint64_t left = x < rlen ? rlen - x : 0;
                if (left < v) {  // the read runs off the sequence: the walk ends with the bases that are on it
                    v = (uint32_t)left;
                    ended = true;
                }
                uint32_t rb = 0;
                bool mis = false;
                if (lane < v) {
                    const uint32_t q = y + lane, sb = seq[q >> 1], c1 = (q & 1) ? sb & 15 : sb >> 4;
                    rb = ref[x + lane];
                    const uint32_t c2 = ref_code(rb);
                    mis = !(c1 == 0 || (c1 == c2 && c1 != 15));
                }
                const uint64_t m = __ballot(mis);
                if (m) {  // wave-uniform
                    const uint64_t prev = m & ((1ull << lane) - 1ull);
                    const uint32_t gap = prev ? lane - 1 - (63 - (uint32_t)__clzll((long long)prev)) : run + lane;
                    const uint32_t w = mis ? oge_txt_dec_width(gap) + 1 : 0;
                    const uint32_t incl = wave_incl_scan(w, lane);
                    if (mis) {
                        const uint64_t p = pos + incl - w;
                        s.dec(p, gap, w - 1);
                        s.put(p + w - 1, rb);
                    }
                    pos += uni((uint32_t)__shfl((int)incl, 63, 64));
                    nm += (uint32_t)__popcll(m);
                    run = v - 1 - (63 - (uint32_t)__clzll((long long)m));
                } else {
                    run += v;
                }
                x += v;
                y += v;
            }
        } else if (code == OGE_CIG_D) {
            const uint32_t w = oge_txt_dec_width(run);
            if (lane == 0) {
                s.dec(pos, run, w);
                s.put(pos + w, '^');
            }
            const uint64_t left = x < rlen ? rlen - x : 0;
            const uint32_t c = left < len ? (uint32_t)left : len;
            s.span(pos + w + 1, ref + x, c, lane);
            pos += w + 1 + c;
            run = 0;
            nm += len;
            x += len;
        } else if (code == OGE_CIG_I) {
            y += len;
            nm += len;
        } else if (code == OGE_CIG_S) {
            y += len;
        } else if (code == OGE_CIG_N) {
            x += len;
        }
    }
    const uint32_t w = oge_txt_dec_width(run);
    if (lane == 0) s.dec(pos, run, w);
    nm_out = nm;
    md_out = pos + w;
}

// The fields of a record's core both passes need, wave-uniform
struct CalCore {
    uint32_t bs, lname, nops, flag, lseq;
    int32_t rid, pos;
};

__device__ __forceinline__ CalCore cal_core(const uint8_t *r) {
    CalCore c;
    const uint32_t w3 = uni(oge_ldu32(r + OGE_OFF_LNAME)), w4 = uni(oge_ldu32(r + OGE_OFF_NCIGAR));
    c.bs = uni(oge_ldu32(r + OGE_OFF_BLOCK));
    c.lname = w3 & 0xFF;
    c.nops = w4 & 0xFFFF;
    c.flag = w4 >> 16;
    c.lseq = uni(oge_ldu32(r + OGE_OFF_LSEQ));
    c.rid = (int32_t)uni(oge_ldu32(r + OGE_OFF_REFID));
    c.pos = (int32_t)uni(oge_ldu32(r + OGE_OFF_POS));
    return c;
}

__device__ __forceinline__ bool cal_skipped(const CalCore &c) {
    return (c.flag & OGE_F_UNMAP) || c.rid < 0 || c.pos < 0 || c.nops == 0 || c.lseq == 0;
}

// The first tag named NM and the first named MD of the tags in [p, end) of r: (at, len) = the whole tag's span in
// the record, type its type byte; len 0: none.  false: a tag does not fit the record or has an unknown type.
struct CalTags {
    uint32_t nm_at, nm_len, nm_type, md_at, md_len, md_type;
};

__device__ __forceinline__ bool cal_tags(const uint8_t *r, uint32_t p, uint32_t end, uint32_t lane, CalTags &t) {
    t = {0, 0, 0, 0, 0, 0};
    while (p < end) {  // p is the same in every lane
        if (p + 3 > end) return false;
        const uint32_t w = uni(oge_ldu32(r + p)), t0 = w & 0xFF, t1 = (w >> 8) & 0xFF, type = (w >> 16) & 0xFF, start = p;
        uint64_t q = (uint64_t)p + 3;
        switch (type) {
        case 'A': case 'c': case 'C': q += 1; break;
        case 's': case 'S': q += 2; break;
        case 'i': case 'I': case 'f': q += 4; break;
        case 'Z': case 'H': {  // the NUL by 64 bytes at a time
            bool found = false;
            while (q < end) {
                const uint32_t b = q + lane < end ? r[q + lane] : 1u;
                const uint64_t z = __ballot(b == 0);
                if (z) {
                    q += (uint32_t)__ffsll((long long)z);  // past the NUL
                    found = true;
                    break;
                }
                q += 64;
            }
            if (!found) return false;
            break;
        }
        case 'B': {
            if (q + 5 > end) return false;
            const uint32_t sz = oge_txt_b_elem(r[q]);
            if (!sz) return false;
            q += 5 + (uint64_t)uni(oge_ldu32(r + q + 1)) * sz;
            break;
        }
        default: return false;
        }
        if (q > end) return false;
        p = (uint32_t)q;
        if (t0 == 'N' && t1 == 'M' && !t.nm_len) t.nm_at = start, t.nm_len = p - start, t.nm_type = type;
        if (t0 == 'M' && t1 == 'D' && !t.md_len) t.md_at = start, t.md_len = p - start, t.md_type = type;
    }
    return true;
}

__global__ __launch_bounds__(kT) void k_cm_size(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ off, uint64_t n, int32_t n_ref,
                                                CalRef ref, uint64_t *__restrict__ size, uint4 *__restrict__ dec, CalAcc *__restrict__ acc) {
    __shared__ unsigned long long s_part[kWaves][4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long cnt[4] = {0, 0, 0, 0};  // skipped, no_reference, nm_changed, md_changed of this wave
    if (blockIdx.x == 0 && threadIdx.x == 0) size[n] = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kWaves + wave; i < n; i += (uint64_t)gridDim.x * kWaves) {  // wave-uniform
        const uint8_t *r = recs + off[i];
        const CalCore c = cal_core(r);
        const uint32_t end = 4 + c.bs;
        uint64_t out_size = end;
        uint4 d = make_uint4(0, 0, 0, 0);
        int fault = -1;
        do {
            if (cal_skipped(c)) {
                ++cnt[0];
                break;
            }
            if (c.rid >= n_ref) {
                fault = kBadRef;
                break;
            }
            const int64_t roff = ref.off[c.rid];
            if (roff < 0) {
                ++cnt[1];
                break;
            }
            if (c.bs > OGE_MAX_BLOCK_SIZE) {  // the decision below packs spans and lengths in 16 bits
                fault = kBadBlock;
                break;
            }
            const uint64_t cig_at = (uint64_t)OGE_OFF_NAME + c.lname, seq_at = cig_at + 4ull * c.nops;
            if (seq_at > end) {
                fault = kBadCigar;
                break;
            }
            // the ops, a lane each: the codes and the bases of the read they take
            bool badop = false;
            uint64_t qlen = 0;
            for (uint32_t j = lane; j < c.nops; j += 64) {
                const uint32_t op = oge_ldu32(r + cig_at + 4 * j), code = op & 0xF;
                badop |= code > 8;
                if ((0x193u >> code) & 1u) qlen += op >> 4;  // M I S = X
            }
            if (__ballot(badop)) {
                fault = kBadOp;
                break;
            }
            const uint64_t tag_at = seq_at + (c.lseq + 1ull) / 2 + c.lseq;
            CalTags t;
            if (tag_at > end || !cal_tags(r, (uint32_t)tag_at, end, lane, t)) {
                fault = kBadTags;
                break;
            }
            if (wave_sum_u64(qlen) != c.lseq) {
                fault = kBadQlen;
                break;
            }
            const bool md_z = t.md_len && t.md_type == 'Z';
            MdSink<false> s{md_z ? r + t.md_at + 3 : nullptr, nullptr, md_z ? t.md_len - 4 : 0, false};
            uint64_t nm, mdl;
            md_walk<false>(r + cig_at, c.nops, r + seq_at, ref.bytes + roff, (uint64_t)ref.len[c.rid], (uint32_t)c.pos, lane, s, nm, mdl);
            const bool md_keep = md_z && mdl == s.lim && !__ballot(s.diff);
            bool nm_keep = false;
            if (t.nm_len) {
                const uint8_t *v = r + t.nm_at + 3;
                int64_t have = -1;
                switch (t.nm_type) {
                case 'c': have = (int8_t)v[0]; break;
                case 'C': have = v[0]; break;
                case 's': have = (int16_t)oge_ldu16(v); break;
                case 'S': have = oge_ldu16(v); break;
                case 'i': have = (int32_t)oge_ldu32(v); break;
                case 'I': have = oge_ldu32(v); break;
                default: break;
                }
                nm_keep = have >= 0 && (uint64_t)have == nm;
            }
            const uint32_t nm_bytes = nm < 256 ? 1 : nm < 65536 ? 2 : 4;
            out_size = (uint64_t)end - (nm_keep ? 0 : t.nm_len) - (md_keep ? 0 : t.md_len) + (nm_keep ? 0 : 3 + nm_bytes) +
                       (md_keep ? 0 : 3 + mdl + 1);
            if (nm > 0xFFFFFFFFull || out_size - 4 > OGE_MAX_BLOCK_SIZE) {
                fault = kLimit;
                break;
            }
            cnt[2] += !nm_keep;
            cnt[3] += !md_keep;
            // a span that stays is no span: the emit pass copies across it
            d.x = (uint32_t)nm;
            d.y = (uint32_t)mdl | (uint32_t)(kUsed | (nm_keep ? 0 : kAddNM) | (md_keep ? 0 : kAddMD)) << 16;
            d.z = nm_keep || !t.nm_len ? 0 : t.nm_at | t.nm_len << 16;
            d.w = md_keep || !t.md_len ? 0 : t.md_at | t.md_len << 16;
        } while (false);
        if (fault >= 0) {
            if (lane == 0) atomicMin(&acc->bad[fault], (unsigned long long)i);
            out_size = 0;
        }
        if (lane == 0) {
            size[i] = out_size;
            dec[i] = d;
        }
    }
    if (lane == 0)
        for (int k = 0; k < 4; ++k) s_part[wave][k] = cnt[k];
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long v = 0;
        for (int w = 0; w < kWaves; ++w) v += s_part[w][threadIdx.x];
        if (v) atomicAdd(&acc->cnt[threadIdx.x], v);
    }
}

// len bytes from src to dst by one wave: the destination's aligned dwords from the two source dwords each
// straddles, the up to three bytes in front of and behind them one by one
__device__ __forceinline__ void wave_copy(uint8_t *dst, const uint8_t *src, uint32_t len, uint32_t lane) {
    const uint32_t head = std::min<uint32_t>(len, (4u - (uint32_t)((uintptr_t)dst & 3)) & 3);
    if (lane < head) dst[lane] = src[lane];
    dst += head, src += head, len -= head;
    const uint32_t nd = len >> 2, sh = (uint32_t)((uintptr_t)src & 3) * 8;
    const uint32_t *s4 = (const uint32_t *)((uintptr_t)src & ~(uintptr_t)3);
    uint32_t *d4 = (uint32_t *)dst;
    if (sh) {
        for (uint32_t i = lane; i < nd; i += 64) d4[i] = (s4[i] >> sh) | (s4[i + 1] << (32 - sh));
    } else {
        for (uint32_t i = lane; i < nd; i += 64) d4[i] = s4[i];
    }
    const uint32_t tail = len & 3;
    if (lane < tail) dst[4 * nd + lane] = src[4 * nd + lane];
}

__global__ __launch_bounds__(kT) void k_cm_emit(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ off, uint64_t n, CalRef ref,
                                                const uint64_t *__restrict__ at, const uint4 *__restrict__ dec, uint8_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t i = (uint64_t)blockIdx.x * kWaves + wave; i < n; i += (uint64_t)gridDim.x * kWaves) {  // wave-uniform
        const uint8_t *r = recs + off[i];
        uint8_t *o = out + at[i];
        const uint4 dv = dec[i];
        const uint32_t dy = uni(dv.y), flags = dy >> 16, mdl = dy & 0xFFFF, nm = uni(dv.x);
        const CalCore c = cal_core(r);
        const uint32_t end = 4 + c.bs;
        if (!(flags & kUsed)) {
            wave_copy(o, r, end, lane);
            continue;
        }
        const uint32_t new_bs = (uint32_t)(at[i + 1] - at[i]) - 4;
        if (lane < 4) o[lane] = (uint8_t)(new_bs >> (8 * lane));
        // the record from byte 4 on, across the spans that leave (none: at = end, length 0), in record order
        uint32_t a_at = uni(dv.z) & 0xFFFF, a_len = uni(dv.z) >> 16, b_at = uni(dv.w) & 0xFFFF, b_len = uni(dv.w) >> 16;
        if (!a_len) a_at = end;
        if (!b_len) b_at = end;
        if (b_at < a_at) {
            const uint32_t t_at = a_at, t_len = a_len;
            a_at = b_at, a_len = b_len, b_at = t_at, b_len = t_len;
        }
        uint32_t w = 4;
        wave_copy(o + w, r + 4, a_at - 4, lane);
        w += a_at - 4;
        wave_copy(o + w, r + a_at + a_len, b_at - (a_at + a_len), lane);
        w += b_at - (a_at + a_len);
        wave_copy(o + w, r + b_at + b_len, end - (b_at + b_len), lane);
        w += end - (b_at + b_len);
        if (flags & kAddNM) {
            const uint32_t vb = nm < 256 ? 1 : nm < 65536 ? 2 : 4, type = vb == 1 ? 'C' : vb == 2 ? 'S' : 'I';
            if (lane < 3 + vb) o[w + lane] = (uint8_t)(lane == 0 ? 'N' : lane == 1 ? 'M' : lane == 2 ? type : nm >> (8 * (lane - 3)));
            w += 3 + vb;
        }
        if (flags & kAddMD) {
            if (lane < 3) o[w + lane] = (uint8_t)(lane == 0 ? 'M' : lane == 1 ? 'D' : 'Z');
            const uint64_t cig_at = (uint64_t)OGE_OFF_NAME + c.lname, seq_at = cig_at + 4ull * c.nops;
            MdSink<true> s{nullptr, o + w + 3, mdl, false};
            uint64_t nm2, mdl2;
            md_walk<true>(r + cig_at, c.nops, r + seq_at, ref.bytes + ref.off[c.rid], (uint64_t)ref.len[c.rid], (uint32_t)c.pos, lane, s, nm2, mdl2);
            if (lane == 0) o[w + 3 + mdl] = 0;
        }
    }
}

// ---- the reference in HBM
int64_t mtime_ns(const struct stat &st) { return (int64_t)st.st_mtim.tv_sec * 1000000000ll + st.st_mtim.tv_nsec; }

// Makes the sequences of `names` from the FASTA at `path` the reference on the device: loaded, laid out and
// uploaded only when the file's path, size or mtime or the contig list differ from what the last call left there.
int calmd_reference(oge_ctx *ctx, const char *path, const std::vector<std::string> &names, const std::string &names_key, int threads,
                    CalRef *ref) {
    OgeRefTable &t = ctx->calmd_ref;
    struct stat st;
    if (stat(path, &st)) return oge_fail(ctx, OGE_ERR_IO, (std::string("calmd: cannot open reference FASTA ") + path).c_str());
    const size_t n_ref = names.size();
    if (t.valid && t.path == path && t.size == (uint64_t)st.st_size && t.mtime == mtime_ns(st) && t.names == names_key && t.n_ref == n_ref) {
        // the workspaces are grow-only: nothing else writes these three
        *ref = {t.d_bytes, t.d_off, t.d_len};
        ctx->counters["calmd_ref_uploads"] = t.uploads;
        return OGE_OK;
    }
    t.valid = false;
    oge::RefTable host;
    {
        oge::Pool pool(threads);
        oge::Fasta fa;
        std::string err;
        if (!fa.load(path, err, pool)) return oge_fail(ctx, OGE_ERR_IO, ("calmd: " + err).c_str());
        oge::build_ref_table(fa, names, pool, host);
    }
    uint8_t *d_bytes = (uint8_t *)ctx->ws("calmd_ref_bytes", host.bytes.size());
    int64_t *d_off = (int64_t *)ctx->ws("calmd_ref_off", (n_ref + 1) * 8), *d_len = (int64_t *)ctx->ws("calmd_ref_len", (n_ref + 1) * 8);
    if (!d_bytes || !d_off || !d_len) return OGE_ERR_HIP;
    OGE_HIP_TRY(ctx, hipMemcpyAsync(d_bytes, host.bytes.data(), host.bytes.size(), hipMemcpyHostToDevice, ctx->stream));
    if (n_ref) {
        OGE_HIP_TRY(ctx, hipMemcpyAsync(d_off, host.off.data(), n_ref * 8, hipMemcpyHostToDevice, ctx->stream));
        OGE_HIP_TRY(ctx, hipMemcpyAsync(d_len, host.len.data(), n_ref * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    OGE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // the staging buffers go out of scope
    t.path = path;
    t.size = (uint64_t)st.st_size;
    t.mtime = mtime_ns(st);
    t.names = names_key;
    t.n_ref = n_ref;
    t.d_bytes = d_bytes;
    t.d_off = d_off;
    t.d_len = d_len;
    t.valid = true;
    ctx->counters["calmd_ref_uploads"] = ++t.uploads;
    *ref = {d_bytes, d_off, d_len};
    return OGE_OK;
}

}  // namespace

int oge_calmd_impl(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, int32_t n_ref, const char *ref_names,
                   uint64_t names_bytes, const char *fasta_path, const oge_calmd_opts *opts, oge_calmd_result *out, const uint8_t **d_out,
                   const uint64_t **d_out_off) {
    memset(out, 0, sizeof *out);
    *d_out = nullptr;
    *d_out_off = nullptr;
    if (opts->flags) return oge_fail(ctx, OGE_ERR_ARG, "calmd: unknown option bits");
    if (!fasta_path || !*fasta_path) return oge_fail(ctx, OGE_ERR_ARG, "calmd: no reference FASTA");
    if (n_ref < 0 || (n_ref && !ref_names)) return oge_fail(ctx, OGE_ERR_ARG, "calmd: n_ref < 0 or no contig names");
    if (n && (!d_recs || !d_off)) return oge_fail(ctx, OGE_ERR_ARG, "calmd: null argument");
    std::vector<std::string> names;
    uint64_t p = 0;
    for (int32_t r = 0; r < n_ref; ++r) {
        const void *z = p < names_bytes ? memchr(ref_names + p, 0, names_bytes - p) : nullptr;
        if (!z) return oge_fail(ctx, OGE_ERR_ARG, "calmd: the contig names are not n_ref NUL-terminated strings");
        names.emplace_back(ref_names + p, (const char *)z - (ref_names + p));
        p += names.back().size() + 1;
    }
    OgeStage stage(ctx, "calmd");
    hipStream_t st = ctx->stream;
    OgeStage part(ctx, "calmd_ref");  // nested in calmd: ref, size (with the scan), emit
    CalRef ref;
    int rc = calmd_reference(ctx, fasta_path, names, std::string(ref_names ? ref_names : "", p), opts->threads, &ref);
    if (rc) return rc;
    part.begin("calmd_size");
    CalAcc *acc = (CalAcc *)ctx->ws("calmd_acc", sizeof(CalAcc));
    uint64_t *at = (uint64_t *)ctx->ws("calmd_out_off", (n + 1) * 8);
    uint4 *dec = (uint4 *)ctx->ws("calmd_dec", (n + 1) * sizeof(uint4));
    if (!acc || !at || !dec) return OGE_ERR_HIP;
    CalAcc h;
    memset(&h, 0, sizeof h);
    for (auto &v : h.bad) v = kNone;
    OGE_HIP_TRY(ctx, hipMemcpyAsync(acc, &h, sizeof h, hipMemcpyHostToDevice, st));
    const dim3 grid((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(oge_ceil_div(n, kWaves), (uint64_t)ctx->cu_count() * 8)));
    hipLaunchKernelGGL(k_cm_size, grid, dim3(kT), 0, st, d_recs, d_off, n, n_ref, ref, at, dec, acc);
    OGE_LAUNCH_CHECK(ctx);
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&h, acc, sizeof h, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    static const char *const kBad[kNBad] = {"has a refID of n_ref or more",
                                            "has a block_size above 10000",
                                            "has a CIGAR that does not fit its block_size",
                                            "has a CIGAR op code above 8",
                                            "has bases, qualities or tags that do not fit its block_size",
                                            "has CIGAR ops whose read bases do not sum to l_seq",
                                            "would exceed the largest block_size (10000) with its new tags"};
    int bad = -1;
    for (int k = 0; k < kNBad; ++k)
        if (h.bad[k] != kNone && (bad < 0 || h.bad[k] < h.bad[bad])) bad = k;
    if (bad >= 0)
        return oge_fail(ctx, bad == kLimit ? OGE_ERR_LIMIT : OGE_ERR_ARG, ("calmd: record " + std::to_string(h.bad[bad]) + " " + kBad[bad]).c_str());
    rc = oge_exclusive_scan_u64(ctx, at, at, n + 1);
    if (rc) return rc;
    uint64_t total = 0;
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&total, at + n, 8, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    part.begin("calmd_emit");
    uint8_t *dst = (uint8_t *)ctx->ws("calmd_out", total + 16);
    if (!dst) return OGE_ERR_HIP;
    if (n) {
        hipLaunchKernelGGL(k_cm_emit, grid, dim3(kT), 0, st, d_recs, d_off, n, ref, (const uint64_t *)at, (const uint4 *)dec, dst);
        OGE_LAUNCH_CHECK(ctx);
    }
    OGE_HIP_TRY(ctx, hipMemsetAsync(dst + total, 0, 16, st));  // the arena's slack
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    out->records = n;
    out->skipped = h.cnt[0];
    out->no_reference = h.cnt[1];
    out->nm_changed = h.cnt[2];
    out->md_changed = h.cnt[3];
    out->bytes_out = total;
    *d_out = dst;
    *d_out_off = at;
    return OGE_OK;
}

extern "C" {

void oge_calmd_opts_init(oge_calmd_opts *o) {
    if (!o) return;
    o->threads = 0;
    o->flags = 0;
}

int oge_calmd_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, int32_t n_ref, const char *ref_names,
                  uint64_t names_bytes, const char *fasta_path, const oge_calmd_opts *opts, oge_calmd_result *result, const uint8_t **d_out,
                  const uint64_t **d_out_off) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!opts || !result || !d_out || !d_out_off) return oge_fail(ctx, OGE_ERR_ARG, "oge_calmd_dev: null argument");
    OgeCall call(ctx, /*hold=*/false);
    return oge_calmd_impl(ctx, d_recs, d_off, n, n_ref, ref_names, names_bytes, fasta_path, opts, result, d_out, d_out_off);
}

int oge_calmd(oge_ctx *ctx, const uint8_t *recs, uint64_t rec_bytes, const uint64_t *rec_off, uint64_t n, int32_t n_ref, const char *ref_names,
              uint64_t names_bytes, const char *fasta_path, const oge_calmd_opts *opts, oge_calmd_result *result, uint8_t *recs_out,
              uint64_t out_cap, uint64_t *off_out) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!opts || !result || (n && (!recs || !rec_off))) return oge_fail(ctx, OGE_ERR_ARG, "oge_calmd: null argument");
    (void)hipSetDevice(ctx->device);
    uint8_t *dr = (uint8_t *)ctx->ws("host_recs", rec_bytes + 16);
    uint64_t *dof = (uint64_t *)ctx->ws("host_off", (n + 1) * 8);
    if (!dr || !dof) return OGE_ERR_HIP;
    if (rec_bytes) OGE_HIP_TRY(ctx, hipMemcpyAsync(dr, recs, rec_bytes, hipMemcpyHostToDevice, ctx->stream));
    OGE_HIP_TRY(ctx, hipMemsetAsync(dr + rec_bytes, 0, 16, ctx->stream));
    if (n) OGE_HIP_TRY(ctx, hipMemcpyAsync(dof, rec_off, n * 8, hipMemcpyHostToDevice, ctx->stream));
    const uint8_t *d_out = nullptr;
    const uint64_t *d_out_off = nullptr;
    const int rc = oge_calmd_dev(ctx, dr, dof, n, n_ref, ref_names, names_bytes, fasta_path, opts, result, &d_out, &d_out_off);
    if (rc) return rc;
    if (result->bytes_out > out_cap || (result->bytes_out && !recs_out) || !off_out)
        return oge_fail(ctx, OGE_ERR_LIMIT, "oge_calmd: output buffer too small");
    if (result->bytes_out) OGE_HIP_TRY(ctx, hipMemcpyAsync(recs_out, d_out, result->bytes_out, hipMemcpyDeviceToHost, ctx->stream));
    OGE_HIP_TRY(ctx, hipMemcpyAsync(off_out, d_out_off, (n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return OGE_OK;
}

}  // extern "C"
