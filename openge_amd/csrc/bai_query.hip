// bai_query.hip -- reading a BAM index (.bai, SAM v1 section 5.2): the virtual-offset ranges of a BAM file that
// a list of regions needs, as the union of half-open intervals, for any valid image (bins in any order).
//
//   open    host: one walk over the image's section headers checks every length against the image and lists the
//           bins: key (refID << 16 | bin), image offset of the bin's chunks, n_chunk (pseudo-bin 37450 left out);
//           per reference n_intv and the image offset of its ioffset array.  A serial walk on the device would be
//           a chain of dependent HBM loads, one per bin.  The lists and the image go to HBM; a directory that
//           does not ascend is sorted there (radix sort of (key, position), k_bq_permute), then the exclusive
//           scan of n_chunk numbers the chunks in directory order.
//   query   one work item per (region, level 0..5): the candidate bins of a level are one interval of bin
//           numbers, so two binary searches in the directory give one interval of chunk numbers.  k_bq_count,
//           scan, k_bq_emit (one wave per item, lanes striding over its chunks): every range stored once at its
//           final place as (max(beg, floor), max(end, max(beg, floor))), floor = ioffset[qbeg >> 14].
//   merge   radix sort of the ranges by beg on the bits that vary; the running maximum of end + 1 over the
//           non-empty ranges (k_bq_tilemax / k_bq_tilescan, as bai.hip's linear index); a range is a head when its
//           beg lies past every earlier end; scan of the head flags; k_bq_merge stores each head's beg and, from
//           the last range before the next head, the union's end.
//
// Scratch is sized by the regions and their ranges and is released before the call returns; the merged ranges
// stay until the context's next query; a decode's arena and offsets are handed to the caller.
#include <hip/hip_runtime.h>

#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "oge_ctx.h"

struct oge_bai {
    oge_ctx *ctx = nullptr;
    int32_t n_ref = 0;
    uint64_t ndir = 0, nchunk = 0, bytes = 0;
    uint8_t *img = nullptr;       // the image, 8 bytes of slack behind it
    uint64_t *key = nullptr;      // ndir directory keys, ascending
    uint64_t *coff = nullptr;     // ndir image offsets of the bins' chunk arrays
    uint64_t *psum = nullptr;     // ndir + 1: chunks before directory entry e
    uint64_t *linoff = nullptr;   // n_ref image offsets of the ioffset arrays
    uint32_t *nintv = nullptr;    // n_ref
};

namespace {

constexpr int kT = 256;
constexpr int kPer = 4;
constexpr int kTile = kT * kPer;
constexpr uint32_t kPseudoBin = 37450;
constexpr int kLevels = 6;
constexpr int64_t kMaxEnd = 1ll << 29;

struct BqTab {
    const uint8_t *img;
    const uint64_t *key, *coff, *psum, *linoff;
    const uint32_t *nintv;
    uint64_t ndir;
    int32_t n_ref;
};

__device__ __forceinline__ uint64_t img_u64(const uint8_t *img, uint64_t o) {  // fields are 4-byte aligned
    const uint32_t *p = (const uint32_t *)(img + o);
    return (uint64_t)p[0] | ((uint64_t)p[1] << 32);
}

// the number of directory keys < x (UPPER = false) or <= x (UPPER = true)
template <bool UPPER>
__device__ __forceinline__ uint64_t dir_bound(const uint64_t *__restrict__ key, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (UPPER ? key[mid] <= x : key[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// item (region g, level l) -> its interval of chunk numbers [c0, c1) and the linear-index floor; false: nothing
__device__ __forceinline__ bool item_slice(const BqTab &t, const oge_region *__restrict__ reg, int32_t widen, uint64_t item, uint64_t *c0,
                                           uint64_t *c1, uint64_t *floor) {
    const oge_region r = reg[item / kLevels];
    const int l = (int)(item % kLevels);
    if (r.ref_id < 0 || r.ref_id >= t.n_ref) return false;
    int64_t qb = (int64_t)r.left_pos - widen, qe = (int64_t)r.right_pos + 1;
    if (qb < 0) qb = 0;
    if (qe > kMaxEnd) qe = kMaxEnd;
    if (qb >= qe) return false;
    const uint64_t w = (uint64_t)qb >> 14;
    if (w >= t.nintv[r.ref_id]) return false;  // past the last window: no record of the reference reaches it
    const int shift = 29 - 3 * l;
    const uint64_t base = ((1ull << (3 * l)) - 1) / 7;
    const uint64_t hi_ref = (uint64_t)r.ref_id << 16;
    const uint64_t a = dir_bound<false>(t.key, t.ndir, hi_ref | (base + ((uint64_t)qb >> shift)));
    const uint64_t b = dir_bound<true>(t.key, t.ndir, hi_ref | (base + ((uint64_t)(qe - 1) >> shift)));
    if (a >= b) return false;
    *c0 = t.psum[a];
    *c1 = t.psum[b];
    *floor = img_u64(t.img, t.linoff[r.ref_id] + 8 * w);
    return *c0 < *c1;
}

__global__ __launch_bounds__(kT) void k_bq_count(BqTab t, const oge_region *__restrict__ reg, int32_t widen, uint64_t items,
                                                 uint64_t *__restrict__ cnt) {
    const uint64_t i = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (i > items) return;
    uint64_t c0 = 0, c1 = 0, fl = 0;
    cnt[i] = i < items && item_slice(t, reg, widen, i, &c0, &c1, &fl) ? c1 - c0 : 0;  // cnt[items]: the scan's total
}

// one wave per item, its lanes striding over the item's chunks
__global__ __launch_bounds__(64) void k_bq_emit(BqTab t, const oge_region *__restrict__ reg, int32_t widen, uint64_t items,
                                                const uint64_t *__restrict__ pos, uint64_t *__restrict__ rbeg, uint64_t *__restrict__ rend) {
    const uint64_t i = blockIdx.x;
    if (i >= items) return;
    uint64_t c0 = 0, c1 = 0, fl = 0;
    if (!item_slice(t, reg, widen, i, &c0, &c1, &fl)) return;
    const uint64_t out = pos[i];
    for (uint64_t c = c0 + threadIdx.x; c < c1; c += 64) {
        const uint64_t e = dir_bound<true>(t.psum, t.ndir + 1, c) - 1;  // the entry whose chunks hold number c
        const uint64_t o = t.coff[e] + 16 * (c - t.psum[e]);
        uint64_t b = img_u64(t.img, o);
        uint64_t z = img_u64(t.img, o + 8);
        if (b < fl) b = fl;
        if (z < b) z = b;
        rbeg[out + (c - c0)] = b;
        rend[out + (c - c0)] = z;
    }
}

// directory entries into sorted order
__global__ __launch_bounds__(kT) void k_bq_permute(const uint32_t *__restrict__ vs, uint64_t n, const uint64_t *__restrict__ coff,
                                                   const uint64_t *__restrict__ nch, uint64_t *__restrict__ coff_out,
                                                   uint64_t *__restrict__ nch_out) {
    const uint64_t j = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (j > n) return;
    if (j == n) {
        nch_out[j] = 0;
        return;
    }
    coff_out[j] = coff[vs[j]];
    nch_out[j] = nch[vs[j]];
}

__global__ __launch_bounds__(kT) void k_bq_iota(uint32_t *__restrict__ v, uint64_t n) {
    const uint64_t j = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (j < n) v[j] = (uint32_t)j;
}

// m[j] = end + 1 of the range at sorted position j, 0 for an empty one (it joins nothing and starts nothing)
__global__ __launch_bounds__(kT) void k_bq_ends(const uint64_t *__restrict__ kbeg, const uint32_t *__restrict__ vs,
                                                const uint64_t *__restrict__ rend, uint64_t n, uint64_t *__restrict__ m) {
    const uint64_t j = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (j >= n) return;
    const uint64_t z = rend[vs[j]];
    m[j] = z > kbeg[j] ? z + 1 : 0;
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

__global__ __launch_bounds__(kT) void k_bq_tilemax(const uint64_t *__restrict__ m, uint64_t n, uint64_t *__restrict__ tmax) {
    __shared__ uint64_t sm[kT];
    const uint64_t i0 = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * kPer;
    uint64_t x = 0;
    for (int k = 0; k < kPer; ++k)
        if (i0 + k < n) x = max64(x, m[i0 + k]);
    (void)block_excl_max(sm, x);
    if (threadIdx.x == kT - 1) tmax[blockIdx.x] = sm[kT - 1];
}

// one workgroup: tmax -> its exclusive running maximum, in place
__global__ __launch_bounds__(kT) void k_bq_tilescan(uint64_t *__restrict__ tmax, uint64_t nt) {
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

// head[j] = 1 where a non-empty range begins past every earlier end; m[j] becomes the inclusive maximum;
// head has n + 1 entries
__global__ __launch_bounds__(kT) void k_bq_heads(const uint64_t *__restrict__ kbeg, uint64_t *__restrict__ m, uint64_t n,
                                                 const uint64_t *__restrict__ tcarry, uint32_t *__restrict__ head) {
    __shared__ uint64_t sm[kT];
    const uint64_t i0 = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * kPer;
    uint64_t x[kPer], mx = 0;
    for (int k = 0; k < kPer; ++k) {
        x[k] = i0 + k < n ? m[i0 + k] : 0;
        mx = max64(mx, x[k]);
    }
    uint64_t ex = max64(tcarry[blockIdx.x], block_excl_max(sm, mx));
    for (int k = 0; k < kPer; ++k) {
        const uint64_t j = i0 + k;
        if (j > n) break;
        if (j == n) {
            head[j] = 0;
            break;
        }
        head[j] = x[k] && kbeg[j] + 1 > ex;  // ex = the largest earlier end + 1, 0 when there is none
        ex = max64(ex, x[k]);
        m[j] = ex;
    }
}

// out[2k], out[2k + 1] = the k-th interval of the union (hs: the scanned head flags)
__global__ __launch_bounds__(kT) void k_bq_merge(const uint64_t *__restrict__ kbeg, const uint64_t *__restrict__ m,
                                                 const uint32_t *__restrict__ hs, uint64_t n, uint64_t *__restrict__ out) {
    const uint64_t j = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (j >= n) return;
    const uint32_t before = hs[j], upto = hs[j + 1];
    if (upto != before) out[2ull * before] = kbeg[j];
    const bool last = j + 1 == n || hs[j + 2] != upto;  // the next range is a head, or there is none
    if (last && upto) out[2ull * (upto - 1) + 1] = m[j] - 1;
}

// ---- decode of the ranges: virtual offsets -> positions in the inflated spans, then the pack -----------------
struct DrTab {
    const uint64_t *span_file, *span_z;  // n_spans file offsets; n_spans + 1 offsets in the loaded bytes
    const uint64_t *cstart, *uoff;       // nblk + 1 each: offset in the loaded bytes / in the inflated stream
    uint64_t n_spans, nblk;
};

// stream position of virtual offset v; an end may sit on the edge behind its span's last block
__device__ __forceinline__ bool dr_position(const DrTab &t, uint64_t v, bool is_end, uint64_t *pos) {
    const uint64_t coff = v >> 16, u = v & 0xFFFF;
    const uint64_t s1 = dir_bound<true>(t.span_file, t.n_spans, coff);  // spans that start at or before coff
    if (!s1) return false;
    const uint64_t s = s1 - 1, d = coff - t.span_file[s], slen = t.span_z[s + 1] - t.span_z[s];
    if (d > slen || (d == slen && !(is_end && u == 0))) return false;
    const uint64_t zo = t.span_z[s] + d;
    const uint64_t b = dir_bound<false>(t.cstart, t.nblk + 1, zo);
    if (b > t.nblk || t.cstart[b] != zo) return false;  // not the first byte of a block
    if (b == t.nblk) {
        if (u) return false;
        *pos = t.uoff[t.nblk];
        return true;
    }
    if (u > t.uoff[b + 1] - t.uoff[b]) return false;
    *pos = t.uoff[b] + u;
    return true;
}

// src[r] / len[r] of every range (len has n + 1 entries for the scan); bad = the first range that does not resolve
__global__ __launch_bounds__(kT) void k_dr_resolve(DrTab t, const uint64_t *__restrict__ ranges, uint64_t n, uint64_t *__restrict__ src,
                                                   uint64_t *__restrict__ len, unsigned long long *__restrict__ bad) {
    const uint64_t r = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (r > n) return;
    if (r == n) {
        len[r] = 0;
        return;
    }
    uint64_t a = 0, z = 0;
    if (!dr_position(t, ranges[2 * r], false, &a) || !dr_position(t, ranges[2 * r + 1], true, &z) || z < a) {
        atomicMin(bad, (unsigned long long)r);
        a = z = 0;
    }
    src[r] = a;
    len[r] = z - a;
}

constexpr uint64_t kPiece = 16384;

// Range blockIdx.x, its 16 KiB pieces dealt over gridDim.y workgroups.  A piece is copied as aligned dwords of
// the destination, each put together from the two source dwords it straddles when the two sides are not aligned
// alike, with bytes at the piece's edges.  The source is read up to 7 bytes past the piece: the stream has slack.
__global__ __launch_bounds__(kT) void k_ranges_pack(const uint8_t *__restrict__ stream, const uint64_t *__restrict__ src,
                                                    const uint64_t *__restrict__ dst, uint64_t n, uint8_t *__restrict__ arena) {
    const uint64_t r = blockIdx.x;
    if (r >= n) return;
    const uint64_t len = dst[r + 1] - dst[r];
    for (uint64_t p0 = (uint64_t)blockIdx.y * kPiece; p0 < len; p0 += (uint64_t)gridDim.y * kPiece) {
        const uint64_t pl = len - p0 < kPiece ? len - p0 : kPiece;
        const uint8_t *sp = stream + src[r] + p0;
        uint8_t *dp = arena + dst[r] + p0;
        uint64_t head = (4 - ((uintptr_t)dp & 3)) & 3;
        if (head > pl) head = pl;
        const uint64_t nd = (pl - head) / 4;
        if (threadIdx.x < head) dp[threadIdx.x] = sp[threadIdx.x];
        const uint32_t sh = (uint32_t)((uintptr_t)(sp + head) & 3) * 8;
        const uint32_t *s4 = (const uint32_t *)(sp + head - sh / 8);
        uint32_t *d4 = (uint32_t *)(dp + head);
        if (sh == 0) {
            for (uint64_t i = threadIdx.x; i < nd; i += kT) d4[i] = s4[i];
        } else {
            for (uint64_t i = threadIdx.x; i < nd; i += kT) d4[i] = (s4[i] >> sh) | (s4[i + 1] << (32 - sh));
        }
        const uint64_t done = head + 4 * nd;
        if (threadIdx.x < pl - done) dp[done + threadIdx.x] = sp[done + threadIdx.x];
    }
}

void drop_ws(oge_ctx *ctx, const char *name) {
    auto it = ctx->bufs.find(name);
    if (it == ctx->bufs.end()) return;
    ctx->release(it->second.p);
    ctx->bufs.erase(it);
}

struct Scratch {
    oge_ctx *c;
    ~Scratch() {
        (void)hipStreamSynchronize(c->stream);
        for (const char *nm : {"bq_reg", "bq_cnt", "bq_rbeg", "bq_rend", "bq_ktmp", "bq_val", "bq_vtmp", "bq_m", "bq_tmax", "bq_head"})
            drop_ws(c, nm);
    }
};

inline dim3 grid_for(uint64_t items) { return dim3(oge_ceil_div(items, kT)); }

int bai_fail(oge_ctx *ctx, const std::string &why) { return oge_fail(ctx, OGE_ERR_ARG, ("index: " + why).c_str()); }

template <typename T>
int upload(oge_ctx *ctx, T **dst, const std::vector<T> &src, size_t extra = 0) {
    *dst = (T *)ctx->alloc((src.size() + extra + 1) * sizeof(T));
    if (!*dst) return OGE_ERR_HIP;
    if (!src.empty()) OGE_HIP_TRY(ctx, hipMemcpyAsync(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return OGE_OK;
}

uint32_t rd32(const uint8_t *p) {
    uint32_t x;
    memcpy(&x, p, 4);
    return x;
}

}  // namespace

extern "C" {

void oge_bai_close(oge_bai *b) {
    if (!b) return;
    if (b->ctx) {
        (void)hipSetDevice(b->ctx->device);
        (void)hipStreamSynchronize(b->ctx->stream);
        for (void *p : {(void *)b->img, (void *)b->key, (void *)b->coff, (void *)b->psum, (void *)b->linoff, (void *)b->nintv})
            if (p) b->ctx->release(p);
    }
    delete b;
}

int oge_bai_open(oge_ctx *ctx, const uint8_t *bai, uint64_t bytes, int32_t n_ref_expected, oge_bai **out) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!out || (bytes && !bai)) return oge_fail(ctx, OGE_ERR_ARG, "oge_bai_open: null argument");
    *out = nullptr;
    // ---- the walk: nothing is launched or allocated on the device before the image has passed
    if (bytes < 8 || memcmp(bai, "BAI\1", 4) != 0) return bai_fail(ctx, "no BAI magic");
    const int32_t n_ref = (int32_t)rd32(bai + 4);
    if (n_ref < 0) return bai_fail(ctx, "n_ref < 0");
    if (n_ref_expected >= 0 && n_ref != n_ref_expected)
        return bai_fail(ctx, "n_ref " + std::to_string(n_ref) + " differs from the header's " + std::to_string(n_ref_expected));
    std::vector<uint64_t> key, coff, nch, linoff;
    std::vector<uint32_t> nintv;
    uint64_t p = 8;
    bool ascending = true;
    for (int32_t r = 0; r < n_ref; ++r) {
        if (p + 4 > bytes) return bai_fail(ctx, "truncated image");
        const int32_t n_bin = (int32_t)rd32(bai + p);
        p += 4;
        if (n_bin < 0) return bai_fail(ctx, "n_bin < 0");
        for (int32_t k = 0; k < n_bin; ++k) {
            if (p + 8 > bytes) return bai_fail(ctx, "truncated image");
            const uint32_t bin = rd32(bai + p);
            const int32_t nc = (int32_t)rd32(bai + p + 4);
            p += 8;
            if (nc < 0 || (uint64_t)nc > (bytes - p) / 16) return bai_fail(ctx, "truncated image");
            if (bin != kPseudoBin) {
                if (bin > kPseudoBin) return bai_fail(ctx, "bin number " + std::to_string(bin) + " out of range");
                const uint64_t kk = ((uint64_t)r << 16) | bin;
                if (!key.empty() && key.back() > kk) ascending = false;
                key.push_back(kk);
                coff.push_back(p);
                nch.push_back((uint64_t)nc);
            }
            p += 16ull * (uint64_t)nc;
        }
        if (p + 4 > bytes) return bai_fail(ctx, "truncated image");
        const int32_t ni = (int32_t)rd32(bai + p);
        p += 4;
        if (ni < 0 || (uint64_t)ni > (bytes - p) / 8) return bai_fail(ctx, "truncated image");
        nintv.push_back((uint32_t)ni);
        linoff.push_back(p);
        p += 8ull * (uint64_t)ni;
    }
    if (p != bytes && p + 8 != bytes)  // n_no_coor is optional (SAM v1 section 5.2)
        return bai_fail(ctx, p + 8 < bytes ? "bytes behind the last section" : "truncated image");
    if (key.size() >= 0xFFFFFFFFull) return oge_fail(ctx, OGE_ERR_LIMIT, "index: more than 2^32-2 bins");

    OgeCall call(ctx, /*hold=*/false);
    oge_bai *b = new oge_bai;
    b->ctx = ctx;
    b->n_ref = n_ref;
    b->ndir = key.size();
    b->bytes = bytes;
    struct Guard {
        oge_bai *b;
        ~Guard() { if (b) oge_bai_close(b); }
    } guard{b};
    const uint64_t nd = b->ndir;
    hipStream_t st = ctx->stream;
    b->img = (uint8_t *)ctx->alloc(bytes + 8);
    if (!b->img) return OGE_ERR_HIP;
    OGE_HIP_TRY(ctx, hipMemcpyAsync(b->img, bai, bytes, hipMemcpyHostToDevice, st));
    int rc = upload(ctx, &b->key, key);
    if (!rc) rc = upload(ctx, &b->coff, coff);
    if (!rc) rc = upload(ctx, &b->psum, nch, 1);
    if (!rc) rc = upload(ctx, &b->linoff, linoff);
    if (!rc) rc = upload(ctx, &b->nintv, nintv);
    if (rc) return rc;
    OGE_HIP_TRY(ctx, hipMemsetAsync(b->psum + nd, 0, 8, st));
    if (!ascending) {  // bins in any order: the directory into key order, a bin's position in the image kept beside it
        uint64_t *ktmp = (uint64_t *)ctx->alloc((nd + 1) * 8), *c2 = (uint64_t *)ctx->alloc((nd + 1) * 8), *n2 = (uint64_t *)ctx->alloc((nd + 2) * 8);
        uint32_t *val = (uint32_t *)ctx->alloc((nd + 1) * 4), *vtmp = (uint32_t *)ctx->alloc((nd + 1) * 4);
        uint64_t *ks = nullptr;
        uint32_t *vs = nullptr;
        rc = ktmp && c2 && n2 && val && vtmp ? OGE_OK : OGE_ERR_HIP;
        if (!rc) {
            hipLaunchKernelGGL(k_bq_iota, grid_for(nd), dim3(kT), 0, st, val, nd);
            uint32_t rb = 0;
            while (rb < 32 && ((uint64_t)1 << rb) < (uint64_t)n_ref) ++rb;
            rc = oge_radix_sort_pairs(ctx, b->key, val, ktmp, vtmp, nd, (((uint64_t)1 << (16 + rb)) - 1), &ks, &vs);
        }
        if (!rc) {
            hipLaunchKernelGGL(k_bq_permute, grid_for(nd + 1), dim3(kT), 0, st, (const uint32_t *)vs, nd, (const uint64_t *)b->coff,
                               (const uint64_t *)b->psum, c2, n2);
            if (hipGetLastError() != hipSuccess) rc = oge_fail(ctx, OGE_ERR_HIP, "index: kernel launch failed");
        }
        (void)hipStreamSynchronize(st);
        if (!rc) {
            std::swap(b->coff, c2);
            std::swap(b->psum, n2);
            if (ks != b->key) std::swap(b->key, ktmp);
        }
        for (void *q : {(void *)ktmp, (void *)c2, (void *)n2, (void *)val, (void *)vtmp})
            if (q) ctx->release(q);
        if (rc) return rc;
    }
    rc = oge_exclusive_scan_u64(ctx, b->psum, b->psum, nd + 1);
    if (rc) return rc;
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&b->nchunk, b->psum + nd, 8, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    guard.b = nullptr;
    *out = b;
    return OGE_OK;
}

int oge_bai_query_dev(oge_ctx *ctx, const oge_bai *bai, const oge_region *regions, uint64_t n_regions, int32_t widen,
                      const uint64_t **d_ranges, uint64_t *n_ranges) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!bai || !d_ranges || !n_ranges || (n_regions && !regions)) return oge_fail(ctx, OGE_ERR_ARG, "oge_bai_query_dev: null argument");
    if (bai->ctx != ctx) return oge_fail(ctx, OGE_ERR_ARG, "oge_bai_query_dev: the index was opened on another context");
    if (widen < 0) return oge_fail(ctx, OGE_ERR_ARG, "oge_bai_query_dev: widen < 0");
    if (n_regions > (1ull << 23)) return oge_fail(ctx, OGE_ERR_LIMIT, "oge_bai_query_dev: more than 2^23 regions");
    OgeCall call(ctx, /*hold=*/false);
    *d_ranges = nullptr;
    *n_ranges = 0;
    ctx->counters["baiq_ranges"] = 0;
    (void)hipStreamSynchronize(ctx->stream);
    drop_ws(ctx, "bq_out");  // the last query's result
    if (!n_regions || !bai->ndir) return OGE_OK;
    OgeStage stage(ctx, "bai_query");
    Scratch scratch{ctx};  // destroyed first: the stage's stop event follows the frees' synchronisation
    hipStream_t st = ctx->stream;
    const BqTab t = {bai->img, bai->key, bai->coff, bai->psum, bai->linoff, bai->nintv, bai->ndir, bai->n_ref};
    const uint64_t items = n_regions * kLevels;
    oge_region *reg = (oge_region *)ctx->ws("bq_reg", n_regions * sizeof(oge_region));
    uint64_t *cnt = (uint64_t *)ctx->ws("bq_cnt", (items + 1) * 8);
    if (!reg || !cnt) return OGE_ERR_HIP;
    OGE_HIP_TRY(ctx, hipMemcpyAsync(reg, regions, n_regions * sizeof(oge_region), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_bq_count, grid_for(items + 1), dim3(kT), 0, st, t, (const oge_region *)reg, widen, items, cnt);
    OGE_LAUNCH_CHECK(ctx);
    int rc = oge_exclusive_scan_u64(ctx, cnt, cnt, items + 1);
    if (rc) return rc;
    uint64_t T = 0;
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&T, cnt + items, 8, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (!T) return OGE_OK;
    if (T >= 0xFFFFFFFFull) return oge_fail(ctx, OGE_ERR_LIMIT, "oge_bai_query_dev: more than 2^32-2 ranges before the merge");
    uint64_t *rbeg = (uint64_t *)ctx->ws("bq_rbeg", T * 8), *rend = (uint64_t *)ctx->ws("bq_rend", T * 8);
    uint64_t *ktmp = (uint64_t *)ctx->ws("bq_ktmp", T * 8), *m = (uint64_t *)ctx->ws("bq_m", T * 8);
    uint32_t *val = (uint32_t *)ctx->ws("bq_val", T * 4), *vtmp = (uint32_t *)ctx->ws("bq_vtmp", T * 4);
    const uint64_t nt = (T + kTile - 1) / kTile;
    uint64_t *tmax = (uint64_t *)ctx->ws("bq_tmax", nt * 8);
    uint32_t *head = (uint32_t *)ctx->ws("bq_head", (T + 2) * 4);
    if (!rbeg || !rend || !ktmp || !m || !val || !vtmp || !tmax || !head) return OGE_ERR_HIP;
    hipLaunchKernelGGL(k_bq_emit, dim3((uint32_t)items), dim3(64), 0, st, t, (const oge_region *)reg, widen, items, (const uint64_t *)cnt,
                       rbeg, rend);
    OGE_LAUNCH_CHECK(ctx);
    // ---- merge: by beg on the varying bits, running maximum of the ends, heads, compaction
    hipLaunchKernelGGL(k_bq_iota, grid_for(T), dim3(kT), 0, st, val, T);
    OGE_LAUNCH_CHECK(ctx);
    uint64_t bor = 0, band = 0, *ks = rbeg;
    uint32_t *vs = val;
    rc = oge_reduce_or_and_u64(ctx, rbeg, T, ~0ull, &bor, &band);
    if (!rc) rc = oge_radix_sort_pairs(ctx, rbeg, val, ktmp, vtmp, T, bor ^ band, &ks, &vs);
    if (rc) return rc;
    hipLaunchKernelGGL(k_bq_ends, grid_for(T), dim3(kT), 0, st, (const uint64_t *)ks, (const uint32_t *)vs, (const uint64_t *)rend, T, m);
    OGE_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_bq_tilemax, dim3((uint32_t)nt), dim3(kT), 0, st, (const uint64_t *)m, T, tmax);
    OGE_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_bq_tilescan, dim3(1), dim3(kT), 0, st, tmax, nt);
    OGE_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_bq_heads, dim3((uint32_t)nt), dim3(kT), 0, st, (const uint64_t *)ks, m, T, (const uint64_t *)tmax, head);
    OGE_LAUNCH_CHECK(ctx);
    if (T % kTile == 0) OGE_HIP_TRY(ctx, hipMemsetAsync(head + T, 0, 4, st));  // entry T falls into a tile of its own
    OGE_HIP_TRY(ctx, hipMemsetAsync(head + T + 1, 0, 4, st));
    rc = oge_exclusive_scan_u32(ctx, head, head, T + 2);
    if (rc) return rc;
    uint32_t nm = 0;
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&nm, head + T, 4, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (!nm) return OGE_OK;
    uint64_t *outp = (uint64_t *)ctx->ws("bq_out", 2ull * nm * 8);
    if (!outp) return OGE_ERR_HIP;
    hipLaunchKernelGGL(k_bq_merge, grid_for(T), dim3(kT), 0, st, (const uint64_t *)ks, (const uint64_t *)m, (const uint32_t *)head, T, outp);
    OGE_LAUNCH_CHECK(ctx);
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    ctx->counters["baiq_ranges"] = nm;
    *d_ranges = outp;
    *n_ranges = nm;
    return OGE_OK;
}

int oge_bai_query(oge_ctx *ctx, const oge_bai *bai, const oge_region *regions, uint64_t n_regions, int32_t widen, uint64_t *out,
                  uint64_t cap, uint64_t *n_ranges) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!n_ranges) return oge_fail(ctx, OGE_ERR_ARG, "oge_bai_query: null argument");
    const uint64_t *d = nullptr;
    const int rc = oge_bai_query_dev(ctx, bai, regions, n_regions, widen, &d, n_ranges);
    if (rc) return rc;
    if (*n_ranges > cap || (*n_ranges && !out)) return oge_fail(ctx, OGE_ERR_LIMIT, "oge_bai_query: output buffer too small");
    if (*n_ranges) {
        OGE_HIP_TRY(ctx, hipMemcpyAsync(out, d, *n_ranges * 16, hipMemcpyDeviceToHost, ctx->stream));
        OGE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return OGE_OK;
}

int oge_bam_decode_ranges_dev(oge_ctx *ctx, const uint8_t *d_z, uint64_t zbytes, const uint64_t *span_z, const uint64_t *span_file,
                              uint64_t n_spans, const uint64_t *d_ranges, uint64_t n_ranges, int32_t n_ref, uint8_t **d_recs,
                              uint64_t **d_off, uint64_t *n, uint64_t *rec_bytes) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!d_recs || !d_off || !n || !rec_bytes || (n_ranges && (!d_z || !span_z || !span_file || !d_ranges || !n_spans)))
        return oge_fail(ctx, OGE_ERR_ARG, "oge_bam_decode_ranges_dev: null argument");
    if ((uintptr_t)d_z & 3) return oge_fail(ctx, OGE_ERR_ARG, "d_z must be 4-byte aligned");
    OgeCall call(ctx, /*hold=*/true);
    *d_recs = nullptr;
    *d_off = nullptr;
    *n = *rec_bytes = 0;
    ctx->counters["baiq_blocks"] = 0;
    if (!n_ranges) return OGE_OK;
    for (uint64_t s = 0; s < n_spans; ++s)
        if (span_z[s + 1] <= span_z[s] || span_z[s + 1] > zbytes || (s && span_file[s] < span_file[s - 1] + (span_z[s] - span_z[s - 1])))
            return oge_fail(ctx, OGE_ERR_ARG, "oge_bam_decode_ranges_dev: spans must ascend, not overlap and lie in d_z");
    if (span_z[0] != 0 || span_z[n_spans] != zbytes) return oge_fail(ctx, OGE_ERR_ARG, "oge_bam_decode_ranges_dev: the spans must cover d_z");
    struct Drop {
        oge_ctx *c;
        ~Drop() {
            (void)hipStreamSynchronize(c->stream);
            for (const char *nm : {"dr_stream", "dr_span", "dr_src", "dr_len", "dr_bad", "bai_cstart", "bai_hdr"}) drop_ws(c, nm);
        }
    } drop{ctx};
    hipStream_t st = ctx->stream;
    // ---- framing of the spans (whole blocks back to back: a BGZF stream of its own), inflate, block starts
    OgeBgzfIndex ix;
    int rc = oge_bgzf_index_ws(ctx, d_z, zbytes, &ix);
    if (rc == 1) return oge_fail(ctx, OGE_ERR_ARG, "index: the spans are not whole BGZF blocks");
    if (rc) return rc;
    if (!ix.nblk) return oge_fail(ctx, OGE_ERR_ARG, "index: the spans hold no data block");
    uint8_t *stream = (uint8_t *)ctx->ws("dr_stream", ix.total + 64);
    if (!stream) return OGE_ERR_HIP;
    rc = oge_bgzf_inflate_dev(ctx, d_z, zbytes, ix.d0, ix.d1, ix.uoff, ix.crc, ix.nblk, stream);
    if (rc) return rc;
    uint64_t *cstart = nullptr;
    rc = oge_bai_cstart(ctx, d_z, ix.d0, ix.d1, ix.nblk, &cstart);
    if (rc) return rc;
    ctx->counters["baiq_blocks"] = ix.nblk;
    // ---- ranges -> stream positions and lengths, scan, pack
    uint64_t *span = (uint64_t *)ctx->ws("dr_span", (2 * n_spans + 1) * 8);
    uint64_t *src = (uint64_t *)ctx->ws("dr_src", n_ranges * 8), *len = (uint64_t *)ctx->ws("dr_len", (n_ranges + 1) * 8);
    unsigned long long *bad = (unsigned long long *)ctx->ws("dr_bad", 8);
    if (!span || !src || !len || !bad) return OGE_ERR_HIP;
    OGE_HIP_TRY(ctx, hipMemcpyAsync(span, span_file, n_spans * 8, hipMemcpyHostToDevice, st));
    OGE_HIP_TRY(ctx, hipMemcpyAsync(span + n_spans, span_z, (n_spans + 1) * 8, hipMemcpyHostToDevice, st));
    OGE_HIP_TRY(ctx, hipMemsetAsync(bad, 0xFF, 8, st));
    const DrTab t = {span, span + n_spans, cstart, ix.uoff, n_spans, ix.nblk};
    {
        OgeStage stage(ctx, "ranges_pack");
        hipLaunchKernelGGL(k_dr_resolve, grid_for(n_ranges + 1), dim3(kT), 0, st, t, d_ranges, n_ranges, src, len, bad);
        OGE_LAUNCH_CHECK(ctx);
        rc = oge_exclusive_scan_u64(ctx, len, len, n_ranges + 1);
        if (rc) return rc;
        unsigned long long hb = 0;
        uint64_t total = 0;
        OGE_HIP_TRY(ctx, hipMemcpyAsync(&hb, bad, 8, hipMemcpyDeviceToHost, st));
        OGE_HIP_TRY(ctx, hipMemcpyAsync(&total, len + n_ranges, 8, hipMemcpyDeviceToHost, st));
        OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
        if (hb != ~0ull)
            return oge_fail(ctx, OGE_ERR_ARG, ("index: range " + std::to_string(hb) + " does not begin and end in BGZF blocks of the spans").c_str());
        if (!total) return OGE_OK;
        // the arena and its offsets are the caller's from here on; an error return frees them
        struct Owned {
            oge_ctx *c;
            void *p = nullptr;
            ~Owned() {
                if (!p) return;
                (void)hipStreamSynchronize(c->stream);
                c->release(p);
            }
        } own_arena{ctx}, own_off{ctx};
        uint8_t *arena = (uint8_t *)(own_arena.p = ctx->alloc(total + 64));
        if (!arena) return oge_fail(ctx, OGE_ERR_HIP, "oge_bam_decode_ranges_dev: out of device memory");
        OGE_HIP_TRY(ctx, hipMemsetAsync(arena + total, 0, 64, st));
        uint64_t lanes = (total / kPiece / n_ranges + 1) * 8;
        if (lanes > 1024) lanes = 1024;
        hipLaunchKernelGGL(k_ranges_pack, dim3((uint32_t)n_ranges, (uint32_t)lanes), dim3(kT), 0, st, (const uint8_t *)stream,
                           (const uint64_t *)src, (const uint64_t *)len, n_ranges, arena);
        OGE_LAUNCH_CHECK(ctx);
        stage.end();
        // ---- the chunks of an index are whole records: the arena is a record stream, walked once
        uint64_t m = 0;
        rc = oge_bam_record_offsets_dev(ctx, arena, 0, total, n_ref, nullptr, 0, &m);
        if (rc) return rc;
        uint64_t *off = (uint64_t *)(own_off.p = ctx->alloc((m + 1) * 8));
        if (!off) return oge_fail(ctx, OGE_ERR_HIP, "oge_bam_decode_ranges_dev: out of device memory");
        rc = oge_bam_record_offsets_dev(ctx, arena, 0, total, n_ref, off, m + 1, &m);
        if (rc) return rc;
        OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
        *d_recs = arena;
        *d_off = off;
        own_arena.p = own_off.p = nullptr;
        *n = m;
        *rec_bytes = total;
    }
    return OGE_OK;
}

}  // extern "C"
