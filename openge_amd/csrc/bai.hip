// bai.hip -- the BAM index (.bai, SAM v1 section 5.2) of coordinate-sorted records resident in HBM.
//
// The reference has no working index (util/bam_index.cpp:245-246 returns at once), so the image is
// defined by DESIGN.md section 19: runs of consecutive records with one (refID, bin) are the chunks,
// chunks of a bin merge when the next one starts in the compressed block its predecessor ends in (or an
// earlier one), bins in ascending order, pseudo-bin 37450 last, no promotion to parent bins.
//
//   record pass   k_bai_rec     one thread per record: core + CIGAR -> one word (refID, first and last 16 Ki
//                               window; the bin is a function of the two windows), order / limit checks,
//                               0x4 counts per reference (workgroup-reduced before the atomic)
//   bounds        k_bai_bounds  run heads (refID or bin changes), first / last record of every reference
//   runs          scan of the head flags, k_bai_runs: (refID << 16 | bin, virtual offset) per run
//   linear index  k_bai_tilemax / k_bai_tilescan / k_bai_lin: the running maximum of the last window
//                 covered tells every record which windows it is the first for -- no atomics, so the
//                 result does not depend on scheduling; k_bai_linfill fills the empty windows
//   chunks        stable radix sort of the runs on (refID, bin), merge flags, scans
//   image         k_bai_refsize + scan, k_bai_bins / k_bai_chunks / k_bai_refs / k_bai_linfill store every
//                 field at its final offset (all fields are 4-byte aligned: u64 as two u32 stores)
//
// Scratch: 12 bytes per record (the word and the scanned head flag), 44 bytes per run, 8 per window; all of
// it is released before the call returns.  The image and the per-reference tables stay until the next call.
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <string>

#include "bam_layout.h"
#include "oge_ctx.h"

namespace {

constexpr int kT = 256;
constexpr int kPer = 4;                 // records per thread in the running-maximum kernels
constexpr int kTile = kT * kPer;
constexpr uint64_t kNone = ~0ull;
constexpr uint32_t kNoRef = 0xFFFFFFFFu;

struct BaiHdr {  // first record index of each kind (kNone: none); records with a reference
    unsigned long long unsorted, limit, bad, ncoord;
};

struct BaiIn {
    const uint8_t *recs;
    const uint64_t *off;
    uint64_t n, base;
    const uint64_t *uoff, *cstart;
    uint64_t nblk;
};

// per-reference tables, n_ref + 1 entries each
struct BaiRef {
    uint64_t *first, *last;    // records [first, last) of the reference
    uint64_t *unm;             // its records with FLAG 0x4
    uint64_t *rs, *re;         // its runs [rs, re) in (refID, bin) order
    uint64_t *nintv, *linoff;  // linear windows, their exclusive scan
    uint64_t *off;             // byte size, then offset of its section behind the 8-byte file header
    uint64_t *linbase;         // image offset of its first ioffset
};

__device__ __forceinline__ uint32_t bin_of_windows(uint32_t wf, uint32_t wl) {  // oge_reg2bin on 16 Ki windows
    if (wf == wl) return 4681 + wf;
    if ((wf >> 3) == (wl >> 3)) return 585 + (wf >> 3);
    if ((wf >> 6) == (wl >> 6)) return 73 + (wf >> 6);
    if ((wf >> 9) == (wl >> 9)) return 9 + (wf >> 9);
    if ((wf >> 12) == (wl >> 12)) return 1 + (wf >> 12);
    return 0;
}
__device__ __forceinline__ uint32_t word_ref(uint64_t v) { return (uint32_t)(v >> 32); }
__device__ __forceinline__ uint32_t word_wl(uint64_t v) { return (uint32_t)(v >> 16) & 0xFFFF; }
__device__ __forceinline__ uint32_t word_wf(uint64_t v) { return (uint32_t)v & 0xFFFF; }
__device__ __forceinline__ uint32_t word_bin(uint64_t v) { return bin_of_windows(word_wf(v), word_wl(v)); }

// decompressed-stream position of record i; i == n: the end of the last record
__device__ __forceinline__ uint64_t rec_pos(const BaiIn &in, uint64_t i) {
    if (i < in.n) return in.base + (in.off[i] - in.off[0]);
    const uint64_t o = in.off[in.n - 1];
    return in.base + (o - in.off[0]) + 4 + oge_rd_u32(in.recs + o);
}

// virtual offset of stream position x: the largest b in [0, nblk] with uoff[b] <= x (a position on a block
// edge belongs to the block that starts there); uoff[0] <= x <= uoff[nblk] was checked by the record pass
__device__ __forceinline__ uint64_t voff(const BaiIn &in, uint64_t x) {
    uint64_t lo = 0, hi = in.nblk;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (in.uoff[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return (in.cstart[lo] << 16) | (x - in.uoff[lo]);
}

__device__ __forceinline__ void put32(uint8_t *img, uint64_t o, uint32_t x) { *(uint32_t *)(img + o) = x; }
__device__ __forceinline__ void put64(uint8_t *img, uint64_t o, uint64_t x) {
    put32(img, o, (uint32_t)x);
    put32(img, o + 4, (uint32_t)(x >> 32));
}

__global__ __launch_bounds__(kT) void k_bai_rec(BaiIn in, int32_t n_ref, uint64_t *__restrict__ v, uint64_t *__restrict__ unm,
                                                BaiHdr *__restrict__ hdr) {
    __shared__ int32_t s_ref0;
    const uint64_t i = (uint64_t)blockIdx.x * kT + threadIdx.x;
    const bool valid = i < in.n;
    int32_t refid = -1;
    bool unmapped = false;
    if (valid) {
        const uint8_t *r = in.recs + in.off[i];
        refid = oge_rd_i32(r + OGE_OFF_REFID);
        const int32_t pos = oge_rd_i32(r + OGE_OFF_POS);
        const uint32_t flag = oge_rd_u16(r + OGE_OFF_FLAG), ncig = oge_rd_u16(r + OGE_OFF_NCIGAR);
        uint64_t word = kNone;
        const uint64_t x = in.base + (in.off[i] - in.off[0]);
        const uint64_t bs = oge_rd_u32(r);
        // a refID outside the dictionary, a record outside the block table, a CIGAR that leaves its record
        if (refid < -1 || refid >= n_ref || x < in.uoff[0] || x + 4 + bs > in.uoff[in.nblk] ||
            (uint64_t)OGE_OFF_NAME + r[OGE_OFF_LNAME] + 4ull * ncig > 4 + bs) {
            atomicMin(&hdr->bad, (unsigned long long)i);
            refid = -1;
        } else if (refid >= 0) {
            if (pos < 0) {
                atomicMin(&hdr->bad, (unsigned long long)i);
            } else {
                int64_t len = 0;
                if (!(flag & OGE_F_UNMAP) && ncig) {
                    const uint8_t *c = r + OGE_OFF_NAME + r[OGE_OFF_LNAME];
                    for (uint32_t k = 0; k < ncig; ++k) {
                        const uint32_t op = oge_rd_u32(c + 4 * k), t = op & 0xF;
                        if (t == OGE_CIG_M || t == OGE_CIG_D || t == OGE_CIG_N || t == OGE_CIG_EQ || t == OGE_CIG_X) len += op >> 4;
                    }
                }
                const int64_t rend = (int64_t)pos + (len > 1 ? len : 1);
                if (rend > (1ll << 29)) atomicMin(&hdr->limit, (unsigned long long)i);
                else word = ((uint64_t)(uint32_t)refid << 32) | ((uint64_t)((rend - 1) >> 14) << 16) | (uint64_t)(pos >> 14);
            }
            unmapped = (flag & OGE_F_UNMAP) != 0;
        }
        if (i) {  // the project's order: refID ascending with -1 last, pos ascending within a reference
            const uint8_t *p = in.recs + in.off[i - 1];
            const uint32_t pr = oge_rd_u32(p + OGE_OFF_REFID), cur = oge_rd_u32(r + OGE_OFF_REFID);
            if (pr > cur || (pr == cur && cur != kNoRef && oge_rd_i32(p + OGE_OFF_POS) > pos))
                atomicMin(&hdr->unsorted, (unsigned long long)i);
        }
        v[i] = word;
    }
    // FLAG 0x4 records per reference: one atomic per workgroup for the reference of its first record
    if (threadIdx.x == 0) s_ref0 = refid;
    __syncthreads();
    const int32_t ref0 = s_ref0;
    const bool mine = valid && unmapped && refid >= 0;
    const int c = __syncthreads_count(mine && refid == ref0);
    if (threadIdx.x == 0 && c) atomicAdd((unsigned long long *)&unm[ref0], (unsigned long long)c);
    if (mine && refid != ref0) atomicAdd((unsigned long long *)&unm[refid], 1ull);
}

// head[i] = 1 where record i starts a run; first / last record of every reference; head has n + 1 entries
__global__ __launch_bounds__(kT) void k_bai_bounds(const uint64_t *__restrict__ v, uint64_t n, uint32_t *__restrict__ head, BaiRef R,
                                                   BaiHdr *__restrict__ hdr) {
    const uint64_t i = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        head[i] = 0;
        return;
    }
    const uint64_t w = v[i];
    const uint32_t r = word_ref(w);
    const uint32_t pr = i ? word_ref(v[i - 1]) : kNoRef;
    const bool newref = i == 0 || pr != r;
    if (r == kNoRef) {
        head[i] = 0;
        if (newref) hdr->ncoord = i;
        return;
    }
    if (newref) R.first[r] = i;
    head[i] = newref || word_bin(w) != word_bin(v[i - 1]);
    if (i + 1 == n || word_ref(v[i + 1]) != r) R.last[r] = i + 1;
}

// run k: key (refID << 16 | bin), begin virtual offset; rbeg[nrun] = the end of the last record with a reference
__global__ __launch_bounds__(kT) void k_bai_runs(BaiIn in, const uint64_t *__restrict__ v, const uint32_t *__restrict__ hs, uint64_t nc,
                                                 uint64_t *__restrict__ rkey, uint32_t *__restrict__ rval, uint64_t *__restrict__ rbeg) {
    const uint64_t i = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (i > nc) return;
    if (i == nc) {
        rbeg[hs[nc]] = voff(in, rec_pos(in, nc));
        return;
    }
    if (hs[i + 1] == hs[i]) return;
    const uint32_t k = hs[i];
    const uint64_t w = v[i];
    rkey[k] = ((uint64_t)word_ref(w) << 16) | word_bin(w);
    rval[k] = k;
    rbeg[k] = voff(in, rec_pos(in, i));
}

__device__ __forceinline__ uint64_t max64(uint64_t a, uint64_t b) { return a > b ? a : b; }

// inclusive running maximum over the workgroup's threads (sm: kT entries); returns the exclusive value
__device__ __forceinline__ uint64_t block_excl_max(uint64_t *sm, uint64_t m) {
    const uint32_t t = threadIdx.x;
    sm[t] = m;
    __syncthreads();
    for (uint32_t d = 1; d < kT; d <<= 1) {
        const uint64_t y = t >= d ? sm[t - d] : 0;
        __syncthreads();
        sm[t] = max64(sm[t], y);
        __syncthreads();
    }
    return t ? sm[t - 1] : 0;
}

__global__ __launch_bounds__(kT) void k_bai_tilemax(const uint64_t *__restrict__ v, uint64_t nc, uint64_t *__restrict__ tmax) {
    __shared__ uint64_t sm[kT];
    const uint64_t i0 = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * kPer;
    uint64_t m = 0;
    for (int k = 0; k < kPer; ++k)
        if (i0 + k < nc) m = max64(m, v[i0 + k]);
    (void)block_excl_max(sm, m);
    if (threadIdx.x == kT - 1) tmax[blockIdx.x] = sm[kT - 1];
}

// one workgroup: tmax -> its exclusive running maximum, in place
__global__ __launch_bounds__(kT) void k_bai_tilescan(uint64_t *__restrict__ tmax, uint64_t nt) {
    __shared__ uint64_t sm[kT];
    uint64_t carry = 0;
    for (uint64_t b = 0; b < nt; b += kT) {
        const uint64_t j = b + threadIdx.x;
        const uint64_t ex = block_excl_max(sm, j < nt ? tmax[j] : 0);
        const uint64_t top = sm[kT - 1];
        if (j < nt) tmax[j] = max64(carry, ex);
        carry = max64(carry, top);
        __syncthreads();
    }
}

// MODE 0: nintv[r] = last window covered by the reference + 1.  MODE 1: record i stores its begin offset into
// the windows no earlier record of its reference covers -- (wf, pm] is covered, pm the running maximum before i.
template <int MODE>
__global__ __launch_bounds__(kT) void k_bai_lin(BaiIn in, const uint64_t *__restrict__ v, uint64_t nc, const uint64_t *__restrict__ tcarry,
                                                BaiRef R, uint64_t *__restrict__ lin) {
    __shared__ uint64_t sm[kT];
    const uint64_t i0 = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * kPer;
    uint64_t x[kPer], m = 0;
    for (int k = 0; k < kPer; ++k) {
        x[k] = i0 + k < nc ? v[i0 + k] : 0;
        m = max64(m, x[k]);
    }
    uint64_t ex = max64(tcarry[blockIdx.x], block_excl_max(sm, m));
    for (int k = 0; k < kPer; ++k) {
        const uint64_t i = i0 + k;
        if (i >= nc) break;
        const uint32_t r = word_ref(x[k]);
        const uint64_t incl = max64(ex, x[k]);
        if (MODE == 0) {
            if (i + 1 == R.last[r]) R.nintv[r] = (uint64_t)word_wl(incl) + 1;
        } else {
            const uint32_t wl = word_wl(x[k]);
            uint32_t lo = word_wf(x[k]);
            if (i != R.first[r] && word_ref(ex) == r) lo = max(lo, word_wl(ex) + 1);
            if (lo <= wl) {
                const uint64_t b = voff(in, rec_pos(in, i));
                for (uint32_t w = lo; w <= wl; ++w) lin[R.linoff[r] + w] = b;
            }
        }
        ex = incl;
    }
}

// sorted runs: ch[j] = 1 where a chunk starts, bh[j] = 1 where a bin starts (nrun + 1 entries each); the
// reference's range of runs
__global__ __launch_bounds__(kT) void k_bai_flags(const uint64_t *__restrict__ ks, const uint32_t *__restrict__ vs,
                                                  const uint64_t *__restrict__ rbeg, uint64_t nrun, uint32_t *__restrict__ ch,
                                                  uint32_t *__restrict__ bh, BaiRef R) {
    const uint64_t j = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (j > nrun) return;
    if (j == nrun) {
        ch[j] = bh[j] = 0;
        return;
    }
    const uint64_t key = ks[j];
    const bool same = j && ks[j - 1] == key;
    // run vs[j - 1] ends where run vs[j - 1] + 1 begins in the file
    const bool merged = same && (rbeg[vs[j - 1] + 1] >> 16) >= (rbeg[vs[j]] >> 16);
    ch[j] = !merged;
    bh[j] = !same;
    const uint64_t r = key >> 16;
    if (j == 0 || (ks[j - 1] >> 16) != r) R.rs[r] = j;
    if (j + 1 == nrun || (ks[j + 1] >> 16) != r) R.re[r] = j + 1;
}

// bfirst[g] = first sorted run of bin g (bi: scanned bin flags); bfirst[nbins] = nrun
__global__ __launch_bounds__(kT) void k_bai_binfirst(const uint32_t *__restrict__ bi, uint64_t nrun, uint32_t *__restrict__ bfirst) {
    const uint64_t j = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (j > nrun) return;
    if (j == nrun) bfirst[bi[nrun]] = (uint32_t)nrun;
    else if (bi[j + 1] != bi[j]) bfirst[bi[j]] = (uint32_t)j;
}

// byte size of every reference's section: n_bin, bins (8 + 16 per chunk), pseudo-bin (40), n_intv, ioffsets
__global__ __launch_bounds__(kT) void k_bai_refsize(int32_t n_ref, const uint32_t *__restrict__ ci, const uint32_t *__restrict__ bi, BaiRef R) {
    const int64_t r = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (r > n_ref) return;
    if (r == n_ref) {
        R.off[r] = 0;
        R.nintv[r] = 0;
        return;
    }
    uint64_t nb = 0, nc = 0;
    if (ci) {
        nb = bi[R.re[r]] - bi[R.rs[r]];
        nc = ci[R.re[r]] - ci[R.rs[r]];
    }
    R.off[r] = 8 + 8 * nb + 16 * nc + (R.last[r] > R.first[r] ? 40 : 0) + 8 * R.nintv[r];
}

__global__ __launch_bounds__(kT) void k_bai_bins(const uint64_t *__restrict__ ks, const uint32_t *__restrict__ ci,
                                                 const uint32_t *__restrict__ bi, const uint32_t *__restrict__ bfirst, uint64_t nbins,
                                                 BaiRef R, uint8_t *__restrict__ img) {
    const uint64_t g = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (g >= nbins) return;
    const uint32_t j0 = bfirst[g], j1 = bfirst[g + 1];
    const uint64_t key = ks[j0], r = key >> 16, rs = R.rs[r];
    const uint64_t o = 8 + R.off[r] + 4 + 8 * (g - bi[rs]) + 16 * (uint64_t)(ci[j0] - ci[rs]);
    put32(img, o, (uint32_t)(key & 0xFFFF));
    put32(img, o + 4, ci[j1] - ci[j0]);
}

// the first run of a chunk stores its begin, the last one its end
__global__ __launch_bounds__(kT) void k_bai_chunks(const uint64_t *__restrict__ ks, const uint32_t *__restrict__ vs,
                                                   const uint64_t *__restrict__ rbeg, const uint32_t *__restrict__ ci,
                                                   const uint32_t *__restrict__ bi, uint64_t nrun, BaiRef R, uint8_t *__restrict__ img) {
    const uint64_t j = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (j >= nrun) return;
    const bool first = ci[j + 1] != ci[j];
    const bool last = j + 1 == nrun || ci[j + 2] != ci[j + 1];
    if (!first && !last) return;
    const uint64_t r = ks[j] >> 16, rs = R.rs[r];
    const uint64_t c = ci[j + 1] - 1, g = bi[j + 1] - 1;  // chunk and bin of run j
    const uint64_t o = 8 + R.off[r] + 4 + 8 * (g - bi[rs] + 1) + 16 * (c - ci[rs]);
    if (first) put64(img, o, rbeg[vs[j]]);
    if (last) put64(img, o + 8, rbeg[vs[j] + 1]);
}

// per reference: n_bin, the pseudo-bin, n_intv; thread n_ref: the file header and the trailing n_no_coor
__global__ __launch_bounds__(kT) void k_bai_refs(BaiIn in, int32_t n_ref, const uint32_t *__restrict__ ci, const uint32_t *__restrict__ bi,
                                                 uint64_t n_no_coor, BaiRef R, uint8_t *__restrict__ img) {
    const int64_t r = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (r > n_ref) return;
    if (r == n_ref) {
        put32(img, 0, 0x01494142u);  // "BAI\1"
        put32(img, 4, (uint32_t)n_ref);
        put64(img, 8 + R.off[n_ref], n_no_coor);
        return;
    }
    uint64_t nb = 0, nc = 0;
    if (ci) {
        nb = bi[R.re[r]] - bi[R.rs[r]];
        nc = ci[R.re[r]] - ci[R.rs[r]];
    }
    const uint64_t cnt = R.last[r] - R.first[r];
    uint64_t o = 8 + R.off[r];
    put32(img, o, (uint32_t)(nb + (cnt ? 1 : 0)));
    o += 4 + 8 * nb + 16 * nc;
    if (cnt) {
        put32(img, o, 37450);
        put32(img, o + 4, 2);
        put64(img, o + 8, voff(in, rec_pos(in, R.first[r])));
        put64(img, o + 16, voff(in, rec_pos(in, R.last[r])));
        put64(img, o + 24, cnt - R.unm[r]);
        put64(img, o + 32, R.unm[r]);
        o += 40;
    }
    put32(img, o, (uint32_t)R.nintv[r]);
    R.linbase[r] = o + 4;
}

// window g of all references: its own value, or that of the next window of the reference that has one (the
// last window of a reference always has one)
__global__ __launch_bounds__(kT) void k_bai_linfill(const uint64_t *__restrict__ lin, uint64_t nwin, int32_t n_ref, BaiRef R,
                                                    uint8_t *__restrict__ img) {
    const uint64_t g = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (g >= nwin) return;
    int64_t lo = 0, hi = n_ref - 1;  // the largest r with linoff[r] <= g
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (R.linoff[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    const uint64_t end = R.linoff[lo] + R.nintv[lo];
    uint64_t x = kNone;
    for (uint64_t h = g; h < end && (x = lin[h]) == kNone; ++h) {}
    put64(img, R.linbase[lo] + 8 * (g - R.linoff[lo]), x);
}

// file offset of every indexed block: the gzip header ends at d0, 18 bytes long in every file this project
// and htslib write (XLEN = 6); otherwise the block starts where its predecessor ended
__global__ __launch_bounds__(kT) void k_bai_cstart(const uint8_t *__restrict__ z, const uint64_t *__restrict__ d0,
                                                   const uint64_t *__restrict__ d1, uint64_t nblk, uint64_t *__restrict__ cstart,
                                                   unsigned long long *__restrict__ bad) {
    const uint64_t b = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (b > nblk) return;
    if (b == nblk) {
        cstart[b] = nblk ? d1[nblk - 1] + 8 : 0;
        return;
    }
    auto starts = [&](uint64_t p) {
        return z[p] == 31 && z[p + 1] == 139 && z[p + 2] == 8 && z[p + 3] == 4 &&
               p + 12 + (z[p + 10] | ((uint64_t)z[p + 11] << 8)) == d0[b];
    };
    uint64_t p = d0[b] - 18;
    if (d0[b] < 18 || !starts(p)) {
        p = b ? d1[b - 1] + 8 : 0;
        if (p + 12 > d0[b] || !starts(p)) {
            atomicMin(bad, (unsigned long long)b);
            p = 0;
        }
    }
    cstart[b] = p;
}

void drop_ws(oge_ctx *ctx, const char *name) {
    auto it = ctx->bufs.find(name);
    if (it == ctx->bufs.end()) return;
    ctx->release(it->second.p);
    ctx->bufs.erase(it);
}

// everything proportional to the records, runs or windows goes back before the call returns
struct Scratch {
    oge_ctx *c;
    ~Scratch() {
        (void)hipStreamSynchronize(c->stream);
        for (const char *nm : {"bai_v", "bai_head", "bai_tmax", "bai_rkey", "bai_rktmp", "bai_rval", "bai_rvtmp", "bai_rbeg", "bai_ch",
                               "bai_bh", "bai_bfirst", "bai_lin", "bai_cstart"})
            drop_ws(c, nm);
        uint64_t held = 0;
        for (auto &kv : c->bufs)
            if (kv.first.compare(0, 4, "bai_") == 0) held += kv.second.cap;
        c->counters["bai_ws_held"] = held;
    }
};

inline dim3 grid_for(uint64_t items) { return dim3(oge_ceil_div(items, kT)); }

}  // namespace

int oge_bai_cstart(oge_ctx *ctx, const uint8_t *d_z, const uint64_t *d0, const uint64_t *d1, uint64_t nblk, uint64_t **cstart_out) {
    uint64_t *cs = (uint64_t *)ctx->ws("bai_cstart", (nblk + 2) * 8);
    unsigned long long *bad = (unsigned long long *)ctx->ws("bai_hdr", sizeof(BaiHdr));
    if (!cs || !bad) return OGE_ERR_HIP;
    OGE_HIP_TRY(ctx, hipMemsetAsync(bad, 0xFF, sizeof(BaiHdr), ctx->stream));
    hipLaunchKernelGGL(k_bai_cstart, grid_for(nblk + 1), dim3(kT), 0, ctx->stream, d_z, d0, d1, nblk, cs, bad);
    OGE_LAUNCH_CHECK(ctx);
    unsigned long long h = 0;
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&h, bad, 8, hipMemcpyDeviceToHost, ctx->stream));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (h != kNone)
        return oge_fail(ctx, OGE_ERR_LIMIT, ("index: the start of BGZF block " + std::to_string(h) + " is not where its header says").c_str());
    *cstart_out = cs;
    return OGE_OK;
}

int oge_bai_build_impl(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, int32_t n_ref, uint64_t stream_base,
                       const uint64_t *d_uoff, const uint64_t *d_cstart, uint64_t nblk, const uint8_t **d_bai, uint64_t *bai_bytes) {
    ctx->bai_ptr = nullptr;
    ctx->bai_bytes = 0;
    // the last call's image and tables go first: what stays behind is sized by this call alone
    (void)hipStreamSynchronize(ctx->stream);
    drop_ws(ctx, "bai_image");
    drop_ws(ctx, "bai_ref");
    if (n_ref < 0) return oge_fail(ctx, OGE_ERR_LIMIT, "index: n_ref < 0");
    if (n >= 0xFFFFFFFFull) return oge_fail(ctx, OGE_ERR_LIMIT, "index: more than 2^32-2 records");
    if (n && (!d_recs || !d_off || !d_uoff || !d_cstart)) return oge_fail(ctx, OGE_ERR_ARG, "index: null argument");
    OgeStage stage(ctx, "bai_build");
    Scratch scratch{ctx};  // destroyed first: the stage's stop event follows the frees' synchronisation
    hipStream_t st = ctx->stream;
    const uint64_t nr1 = (uint64_t)n_ref + 1;
    uint64_t *tab = (uint64_t *)ctx->ws("bai_ref", 9 * nr1 * 8);
    BaiHdr *hdr = (BaiHdr *)ctx->ws("bai_hdr", sizeof(BaiHdr));
    if (!tab || !hdr) return OGE_ERR_HIP;
    OGE_HIP_TRY(ctx, hipMemsetAsync(tab, 0, 9 * nr1 * 8, st));
    BaiRef R = {tab, tab + nr1, tab + 2 * nr1, tab + 3 * nr1, tab + 4 * nr1, tab + 5 * nr1, tab + 6 * nr1, tab + 7 * nr1, tab + 8 * nr1};
    const BaiIn in = {d_recs, d_off, n, stream_base, d_uoff, d_cstart, nblk};
    BaiHdr h = {kNone, kNone, kNone, n};
    uint64_t nrun = 0, nwin = 0;
    uint64_t *v = nullptr, *rbeg = nullptr, *ks = nullptr;
    uint64_t *lin = nullptr;
    uint32_t *hs = nullptr, *vs = nullptr, *ci = nullptr, *bi = nullptr, *bfirst = nullptr;

    if (n) {
        // ---- record pass, run heads, reference bounds
        v = (uint64_t *)ctx->ws("bai_v", n * 8);
        hs = (uint32_t *)ctx->ws("bai_head", (n + 1) * 4);
        if (!v || !hs) return OGE_ERR_HIP;
        OGE_HIP_TRY(ctx, hipMemcpyAsync(hdr, &h, sizeof h, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_bai_rec, grid_for(n), dim3(kT), 0, st, in, n_ref, v, R.unm, hdr);
        OGE_LAUNCH_CHECK(ctx);
        hipLaunchKernelGGL(k_bai_bounds, grid_for(n + 1), dim3(kT), 0, st, (const uint64_t *)v, n, hs, R, hdr);
        OGE_LAUNCH_CHECK(ctx);
        int rc = oge_exclusive_scan_u32(ctx, hs, hs, n + 1);
        if (rc) return rc;
        uint32_t nrun32 = 0;
        OGE_HIP_TRY(ctx, hipMemcpyAsync(&h, hdr, sizeof h, hipMemcpyDeviceToHost, st));
        OGE_HIP_TRY(ctx, hipMemcpyAsync(&nrun32, hs + n, 4, hipMemcpyDeviceToHost, st));
        OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
        nrun = nrun32;
        if (h.bad != kNone)
            return oge_fail(ctx, OGE_ERR_ARG,
                            ("index: record " + std::to_string(h.bad) + " has a refID outside [-1, n_ref), a negative position or lies outside the block table").c_str());
        if (h.unsorted != kNone && h.unsorted <= h.limit)
            return oge_fail(ctx, OGE_ERR_ARG,
                            ("index: record " + std::to_string(h.unsorted) + " is out of order (the input must be coordinate-sorted)").c_str());
        if (h.limit != kNone)
            return oge_fail(ctx, OGE_ERR_LIMIT, ("index: record " + std::to_string(h.limit) + " ends past 2^29 (the BAI limit)").c_str());
    }
    const uint64_t nc = h.ncoord;

    if (nrun) {
        // ---- runs
        uint64_t *rkey = (uint64_t *)ctx->ws("bai_rkey", nrun * 8), *rktmp = (uint64_t *)ctx->ws("bai_rktmp", nrun * 8);
        uint32_t *rval = (uint32_t *)ctx->ws("bai_rval", nrun * 4), *rvtmp = (uint32_t *)ctx->ws("bai_rvtmp", nrun * 4);
        rbeg = (uint64_t *)ctx->ws("bai_rbeg", (nrun + 1) * 8);
        if (!rkey || !rktmp || !rval || !rvtmp || !rbeg) return OGE_ERR_HIP;
        hipLaunchKernelGGL(k_bai_runs, grid_for(nc + 1), dim3(kT), 0, st, in, (const uint64_t *)v, (const uint32_t *)hs, nc, rkey, rval, rbeg);
        OGE_LAUNCH_CHECK(ctx);

        // ---- linear index: window counts, their scan, the first record of every window
        const uint64_t nt = (nc + kTile - 1) / kTile;
        uint64_t *tmax = (uint64_t *)ctx->ws("bai_tmax", nt * 8);
        if (!tmax) return OGE_ERR_HIP;
        hipLaunchKernelGGL(k_bai_tilemax, dim3((uint32_t)nt), dim3(kT), 0, st, (const uint64_t *)v, nc, tmax);
        OGE_LAUNCH_CHECK(ctx);
        hipLaunchKernelGGL(k_bai_tilescan, dim3(1), dim3(kT), 0, st, tmax, nt);
        OGE_LAUNCH_CHECK(ctx);
        hipLaunchKernelGGL(k_bai_lin<0>, dim3((uint32_t)nt), dim3(kT), 0, st, in, (const uint64_t *)v, nc, (const uint64_t *)tmax, R,
                           (uint64_t *)nullptr);
        OGE_LAUNCH_CHECK(ctx);
        int rc = oge_exclusive_scan_u64(ctx, R.nintv, R.linoff, nr1);
        if (rc) return rc;
        OGE_HIP_TRY(ctx, hipMemcpyAsync(&nwin, R.linoff + n_ref, 8, hipMemcpyDeviceToHost, st));
        OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
        lin = (uint64_t *)ctx->ws("bai_lin", nwin * 8);
        if (!lin) return OGE_ERR_HIP;
        OGE_HIP_TRY(ctx, hipMemsetAsync(lin, 0xFF, nwin * 8, st));
        hipLaunchKernelGGL(k_bai_lin<1>, dim3((uint32_t)nt), dim3(kT), 0, st, in, (const uint64_t *)v, nc, (const uint64_t *)tmax, R, lin);
        OGE_LAUNCH_CHECK(ctx);

        // ---- chunks: runs into (refID, bin) order, file order kept within a bin; merge flags; scans
        uint32_t rb = 0;
        while (rb < 32 && ((uint64_t)1 << rb) < (uint64_t)n_ref) ++rb;
        rc = oge_radix_sort_pairs(ctx, rkey, rval, rktmp, rvtmp, nrun, (((uint64_t)1 << (16 + rb)) - 1), &ks, &vs);
        if (rc) return rc;
        ci = (uint32_t *)ctx->ws("bai_ch", (nrun + 2) * 4);
        bi = (uint32_t *)ctx->ws("bai_bh", (nrun + 2) * 4);
        bfirst = (uint32_t *)ctx->ws("bai_bfirst", (nrun + 2) * 4);
        if (!ci || !bi || !bfirst) return OGE_ERR_HIP;
        hipLaunchKernelGGL(k_bai_flags, grid_for(nrun + 1), dim3(kT), 0, st, (const uint64_t *)ks, (const uint32_t *)vs,
                           (const uint64_t *)rbeg, nrun, ci, bi, R);
        OGE_LAUNCH_CHECK(ctx);
        rc = oge_exclusive_scan_u32(ctx, ci, ci, nrun + 1);
        if (!rc) rc = oge_exclusive_scan_u32(ctx, bi, bi, nrun + 1);
        if (rc) return rc;
        hipLaunchKernelGGL(k_bai_binfirst, grid_for(nrun + 1), dim3(kT), 0, st, (const uint32_t *)bi, nrun, bfirst);
        OGE_LAUNCH_CHECK(ctx);
    }

    // ---- section sizes -> offsets, the image
    hipLaunchKernelGGL(k_bai_refsize, grid_for(nr1), dim3(kT), 0, st, n_ref, (const uint32_t *)ci, (const uint32_t *)bi, R);
    OGE_LAUNCH_CHECK(ctx);
    int rc = oge_exclusive_scan_u64(ctx, R.off, R.off, nr1);
    if (rc) return rc;
    uint64_t body = 0;
    uint32_t nbins = 0;
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&body, R.off + n_ref, 8, hipMemcpyDeviceToHost, st));
    if (nrun) OGE_HIP_TRY(ctx, hipMemcpyAsync(&nbins, bi + nrun, 4, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    const uint64_t total = 8 + body + 8;
    uint8_t *img = (uint8_t *)ctx->ws("bai_image", total);
    if (!img) return OGE_ERR_HIP;
    if (nrun) {
        hipLaunchKernelGGL(k_bai_bins, grid_for(nbins), dim3(kT), 0, st, (const uint64_t *)ks, (const uint32_t *)ci, (const uint32_t *)bi,
                           (const uint32_t *)bfirst, (uint64_t)nbins, R, img);
        OGE_LAUNCH_CHECK(ctx);
        hipLaunchKernelGGL(k_bai_chunks, grid_for(nrun), dim3(kT), 0, st, (const uint64_t *)ks, (const uint32_t *)vs, (const uint64_t *)rbeg,
                           (const uint32_t *)ci, (const uint32_t *)bi, nrun, R, img);
        OGE_LAUNCH_CHECK(ctx);
    }
    hipLaunchKernelGGL(k_bai_refs, grid_for(nr1), dim3(kT), 0, st, in, n_ref, (const uint32_t *)ci, (const uint32_t *)bi, n - nc, R, img);
    OGE_LAUNCH_CHECK(ctx);
    if (nwin) {
        hipLaunchKernelGGL(k_bai_linfill, grid_for(nwin), dim3(kT), 0, st, (const uint64_t *)lin, nwin, n_ref, R, img);
        OGE_LAUNCH_CHECK(ctx);
    }
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    ctx->bai_ptr = img;
    ctx->bai_bytes = total;
    ctx->counters["bai_bytes"] = total;
    ctx->counters["bai_runs"] = nrun;
    if (d_bai) *d_bai = img;
    if (bai_bytes) *bai_bytes = total;
    return OGE_OK;
}

extern "C" {

int oge_bai_build_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, int32_t n_ref, uint64_t stream_base,
                      const uint64_t *d_uoff, const uint64_t *d_cstart, uint64_t nblk, const uint8_t **d_bai, uint64_t *bai_bytes) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!d_bai || !bai_bytes) return oge_fail(ctx, OGE_ERR_ARG, "oge_bai_build_dev: null argument");
    OgeCall call(ctx, /*hold=*/false);
    *d_bai = nullptr;
    *bai_bytes = 0;
    return oge_bai_build_impl(ctx, d_recs, d_off, n, n_ref, stream_base, d_uoff, d_cstart, nblk, d_bai, bai_bytes);
}

int oge_bai_build(oge_ctx *ctx, const uint8_t *recs, uint64_t rec_bytes, const uint64_t *rec_off, uint64_t n, int32_t n_ref,
                  uint64_t stream_base, const uint64_t *uoff, const uint64_t *cstart, uint64_t nblk, uint8_t *out, uint64_t cap,
                  uint64_t *bai_bytes) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!bai_bytes || (n && (!recs || !rec_off || !uoff || !cstart))) return oge_fail(ctx, OGE_ERR_ARG, "oge_bai_build: null argument");
    (void)hipSetDevice(ctx->device);
    uint8_t *dr = (uint8_t *)ctx->ws("host_recs", rec_bytes + 16);
    uint64_t *dof = (uint64_t *)ctx->ws("host_off", (n + 1) * 8);
    uint64_t *dt = (uint64_t *)ctx->ws("host_blocks", 2 * (nblk + 1) * 8);
    if (!dr || !dof || !dt) return OGE_ERR_HIP;
    if (rec_bytes) OGE_HIP_TRY(ctx, hipMemcpyAsync(dr, recs, rec_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (n) OGE_HIP_TRY(ctx, hipMemcpyAsync(dof, rec_off, n * 8, hipMemcpyHostToDevice, ctx->stream));
    if (uoff && cstart) {
        OGE_HIP_TRY(ctx, hipMemcpyAsync(dt, uoff, (nblk + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        OGE_HIP_TRY(ctx, hipMemcpyAsync(dt + nblk + 1, cstart, (nblk + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    const uint8_t *img = nullptr;
    uint64_t got = 0;
    const int rc = oge_bai_build_dev(ctx, dr, dof, n, n_ref, stream_base, dt, dt + nblk + 1, nblk, &img, &got);
    if (rc) return rc;
    *bai_bytes = got;
    if (got > cap || !out) return oge_fail(ctx, OGE_ERR_LIMIT, "oge_bai_build: output buffer too small");
    OGE_HIP_TRY(ctx, hipMemcpyAsync(out, img, got, hipMemcpyDeviceToHost, ctx->stream));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return OGE_OK;
}

int oge_ctx_last_bai(oge_ctx *ctx, const uint8_t **d_bai, uint64_t *bai_bytes) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!d_bai || !bai_bytes) return oge_fail(ctx, OGE_ERR_ARG, "oge_ctx_last_bai: null argument");
    if (!ctx->bai_ptr) return oge_fail(ctx, OGE_ERR_ARG, "no index: the context's last call built none");
    *d_bai = ctx->bai_ptr;
    *bai_bytes = ctx->bai_bytes;
    return OGE_OK;
}

}  // extern "C"
