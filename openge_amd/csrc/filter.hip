// filter.hip -- record compaction on the device: mergesort's Filter module (-r region / -q mapq,
// algorithms/filter.cpp:205-249) and the writer side of -r/-R duplicate removal
// (algorithms/mark_duplicates.cpp:456-458).
//
// A region list (-L, oge_filter_regions_dev) is the same compaction: the regions are sorted by (refID, left)
// with the running maximum of their right ends beside them, and the predicate binary-searches them per record.
//
// All are a keep predicate over the record core (one thread per record, 24 bytes of the 32-byte
// core read), an exclusive scan of the keep flags, a keep -> output-position permutation, and the
// shared permutation gather of sort.hip (records copied once, bins recomputed in flight).  The
// predicate costs ~0.1 B/record of HBM against the gather's 2 x record size, so the whole module is
// bound by the gather.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <initializer_list>

#include "bam_layout.h"
#include "oge_ctx.h"
#include "records.h"

namespace {

__global__ void k_keep_flags(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ off, uint64_t n, uint16_t mask,
                             uint32_t *__restrict__ keep) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keep[i] = (oge_rd_u16(recs + off[i] + OGE_OFF_FLAG) & mask) ? 0u : 1u;
}

// Filter::runInternal (filter.cpp:213-242).  getPosition() + getLength() is int arithmetic in the
// reference (int32 pos + int32 l_seq); getMapQuality() is the unsigned MAPQ byte.
__global__ void k_keep_filter(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ off, uint64_t n,
                              oge_filter_opts o, uint32_t *__restrict__ keep) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t *r = recs + off[i];
    const int32_t len = oge_rd_i32(r + OGE_OFF_LSEQ);
    const int32_t mapq = r[OGE_OFF_MAPQ];
    bool k = mapq >= o.mapq_min && len >= o.min_len && len <= o.max_len && len > o.trim_total;
    if (o.has_region) {
        const int32_t ref = oge_rd_i32(r + OGE_OFF_REFID);
        const int32_t pos = oge_rd_i32(r + OGE_OFF_POS);
        k = k && ref >= o.ref_id && ref <= o.ref_id && (int32_t)((uint32_t)pos + (uint32_t)len) >= o.left_pos &&
            pos <= o.right_pos;
    }
    keep[i] = k ? 1u : 0u;
}

// ---- region lists (view / mergesort -L): at least one of n_regions regions holds -------------------
// (refID, x) as one word that orders like the pair: refID as unsigned (-1 last), x with its sign flipped
__device__ __forceinline__ uint64_t region_word(int32_t ref, int32_t x) {
    return ((uint64_t)(uint32_t)ref << 32) | ((uint32_t)x ^ 0x80000000u);
}

// key[j] = (ref_id, left_pos), val[j] = j
__global__ __launch_bounds__(256) void k_region_keys(const oge_region *__restrict__ reg, uint64_t nr, uint64_t *__restrict__ key,
                                                     uint32_t *__restrict__ val) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nr) return;
    key[j] = region_word(reg[j].ref_id, reg[j].left_pos);
    val[j] = (uint32_t)j;
}

// rmax[j] = (ref_id, right_pos) of the region at sorted position j
__global__ __launch_bounds__(256) void k_region_rights(const oge_region *__restrict__ reg, const uint32_t *__restrict__ vs, uint64_t nr,
                                                       uint64_t *__restrict__ rmax) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nr) return;
    const oge_region r = reg[vs ? vs[j] : j];
    rmax[j] = region_word(r.ref_id, r.right_pos);
}

// One workgroup: rmax -> its inclusive running maximum, in place.  The words ascend in ref_id, so the maximum
// at j is (ref_id of j, the largest right_pos of the regions of that ref_id up to j).  A region list is a few
// thousand entries against millions of records: 256 entries per step with a carry is enough.
__global__ __launch_bounds__(256) void k_region_runmax(uint64_t *__restrict__ rmax, uint64_t nr) {
    __shared__ uint64_t sm[256];
    const uint32_t t = threadIdx.x;
    uint64_t carry = 0;
    for (uint64_t b = 0; b < nr; b += 256) {
        const uint64_t j = b + t;
        sm[t] = j < nr ? rmax[j] : 0;
        __syncthreads();
        for (uint32_t d = 1; d < 256; d <<= 1) {
            const uint64_t y = t >= d ? sm[t - d] : 0;
            __syncthreads();
            if (y > sm[t]) sm[t] = y;
            __syncthreads();
        }
        const uint64_t top = sm[255];
        if (j < nr) rmax[j] = sm[t] > carry ? sm[t] : carry;
        if (top > carry) carry = top;
        __syncthreads();
    }
}

// k_keep_filter with the region part replaced: the regions of the record's refID with left_pos <= pos + len
// are a prefix of that refID's sorted regions, and one of them has right_pos >= pos exactly when their largest
// right_pos has.  pos + len wraps as in k_keep_filter.
__global__ void k_keep_regions(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ off, uint64_t n, oge_filter_opts o,
                               const uint64_t *__restrict__ key, const uint64_t *__restrict__ rmax, uint64_t nr,
                               uint32_t *__restrict__ keep) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t *r = recs + off[i];
    const int32_t len = oge_rd_i32(r + OGE_OFF_LSEQ);
    const int32_t mapq = r[OGE_OFF_MAPQ];
    bool k = mapq >= o.mapq_min && len >= o.min_len && len <= o.max_len && len > o.trim_total;
    if (k) {
        const int32_t ref = oge_rd_i32(r + OGE_OFF_REFID);
        const int32_t pos = oge_rd_i32(r + OGE_OFF_POS);
        const uint64_t q = region_word(ref, (int32_t)((uint32_t)pos + (uint32_t)len));
        uint64_t lo = 0, hi = nr;  // the number of regions with key <= q
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (key[mid] <= q) lo = mid + 1;
            else hi = mid;
        }
        k = lo && rmax[lo - 1] >= region_word(ref, pos);  // a smaller ref_id's word is below every word of ref
    }
    keep[i] = k ? 1u : 0u;
}

__global__ void k_keep_perm(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ pos, uint64_t n,
                            uint32_t *__restrict__ perm) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (keep[i]) perm[pos[i]] = (uint32_t)i;
}

}  // namespace

// keep[] (n flags, already written on the stream) -> the first `limit` kept records, in order.
static int compact_kept(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, uint32_t *keep,
                        uint64_t limit, uint8_t *d_out, uint64_t *d_out_off, uint64_t *n_out) {
    uint32_t *pos = (uint32_t *)ctx->ws("keep_pos", (n + 1) * 4);
    uint32_t *perm = (uint32_t *)ctx->ws("keep_perm", (n + 1) * 4);
    if (!pos || !perm) return OGE_ERR_HIP;
    int rc = oge_exclusive_scan_u32(ctx, keep, pos, n);
    if (rc) return rc;
    k_keep_perm<<<oge_ceil_div(n, 256), 256, 0, ctx->stream>>>(keep, pos, n, perm);
    OGE_LAUNCH_CHECK(ctx);
    uint32_t last[2];
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&last[0], pos + n - 1, 4, hipMemcpyDeviceToHost, ctx->stream));
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&last[1], keep + n - 1, 4, hipMemcpyDeviceToHost, ctx->stream));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t m = (uint64_t)last[0] + last[1];
    if (m > limit) m = limit;  // the reference stops pulling records once count_limit were kept
    if (m) {
        rc = oge_gather_with_sizes(ctx, d_recs, d_off, perm, nullptr, m, d_out, d_out_off, nullptr, nullptr);
        if (rc) return rc;
    } else {
        OGE_HIP_TRY(ctx, hipMemsetAsync(d_out_off, 0, 8, ctx->stream));
    }
    *n_out = m;
    return OGE_OK;
}

extern "C" int oge_drop_flagged_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, uint16_t flag_mask,
                                    uint8_t *d_out, uint64_t *d_out_off, uint64_t *n_out) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!n_out) return oge_fail(ctx, OGE_ERR_ARG, "null n_out");
    if (n >= 0xffffffffull) return oge_fail(ctx, OGE_ERR_ARG, "too many records");
    hipSetDevice(ctx->device);
    *n_out = 0;
    if (!n) return OGE_OK;
    uint32_t *keep = (uint32_t *)ctx->ws("keep_flags", (n + 1) * 4);
    if (!keep) return OGE_ERR_HIP;
    k_keep_flags<<<oge_ceil_div(n, 256), 256, 0, ctx->stream>>>(d_recs, d_off, n, flag_mask, keep);
    OGE_LAUNCH_CHECK(ctx);
    return compact_kept(ctx, d_recs, d_off, n, keep, ~0ull, d_out, d_out_off, n_out);
}

extern "C" int oge_filter_records_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n,
                                      const oge_filter_opts *o, uint8_t *d_out, uint64_t *d_out_off, uint64_t *n_out) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!n_out || !o) return oge_fail(ctx, OGE_ERR_ARG, "null argument");
    if (n >= 0xffffffffull) return oge_fail(ctx, OGE_ERR_ARG, "too many records");
    hipSetDevice(ctx->device);
    *n_out = 0;
    if (!n || !o->count_limit) {
        if (d_out_off) OGE_HIP_TRY(ctx, hipMemsetAsync(d_out_off, 0, 8, ctx->stream));
        return OGE_OK;
    }
    uint32_t *keep = (uint32_t *)ctx->ws("keep_flags", (n + 1) * 4);
    if (!keep) return OGE_ERR_HIP;
    OgeStage stage(ctx, "filter");
    k_keep_filter<<<oge_ceil_div(n, 256), 256, 0, ctx->stream>>>(d_recs, d_off, n, *o, keep);
    OGE_LAUNCH_CHECK(ctx);
    stage.end();
    return compact_kept(ctx, d_recs, d_off, n, keep, o->count_limit, d_out, d_out_off, n_out);
}

namespace {

// the region tables go back before the call returns: they are sized by the caller's list, not by the records
struct RegionScratch {
    oge_ctx *c;
    ~RegionScratch() {
        (void)hipStreamSynchronize(c->stream);
        for (const char *nm : {"fr_reg", "fr_key", "fr_ktmp", "fr_val", "fr_vtmp", "fr_max"}) {
            auto it = c->bufs.find(nm);
            if (it == c->bufs.end()) continue;
            c->release(it->second.p);
            c->bufs.erase(it);
        }
    }
};

}  // namespace

extern "C" int oge_filter_regions_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n,
                                      const oge_filter_opts *o, const oge_region *regions, uint64_t n_regions, uint8_t *d_out,
                                      uint64_t *d_out_off, uint64_t *n_out) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!n_out || !o) return oge_fail(ctx, OGE_ERR_ARG, "null argument");
    if (!regions || !n_regions) return oge_fail(ctx, OGE_ERR_ARG, "oge_filter_regions_dev: no region");
    if (n >= 0xffffffffull || n_regions >= 0xffffffffull) return oge_fail(ctx, OGE_ERR_ARG, "too many records or regions");
    hipSetDevice(ctx->device);
    *n_out = 0;
    if (!n || !o->count_limit) {
        if (d_out_off) OGE_HIP_TRY(ctx, hipMemsetAsync(d_out_off, 0, 8, ctx->stream));
        return OGE_OK;
    }
    uint32_t *keep = (uint32_t *)ctx->ws("keep_flags", (n + 1) * 4);
    if (!keep) return OGE_ERR_HIP;
    RegionScratch scratch{ctx};
    const uint64_t nr = n_regions;
    oge_region *reg = (oge_region *)ctx->ws("fr_reg", nr * sizeof(oge_region));
    uint64_t *key = (uint64_t *)ctx->ws("fr_key", nr * 8), *ktmp = (uint64_t *)ctx->ws("fr_ktmp", nr * 8);
    uint32_t *val = (uint32_t *)ctx->ws("fr_val", nr * 4), *vtmp = (uint32_t *)ctx->ws("fr_vtmp", nr * 4);
    uint64_t *rmax = (uint64_t *)ctx->ws("fr_max", nr * 8);
    if (!reg || !key || !ktmp || !val || !vtmp || !rmax) return OGE_ERR_HIP;
    OgeStage stage(ctx, "filter_regions");
    OGE_HIP_TRY(ctx, hipMemcpyAsync(reg, regions, nr * sizeof(oge_region), hipMemcpyHostToDevice, ctx->stream));
    k_region_keys<<<oge_ceil_div(nr, 256), 256, 0, ctx->stream>>>(reg, nr, key, val);
    OGE_LAUNCH_CHECK(ctx);
    uint64_t *ks = key;
    uint32_t *vs = val;
    if (nr > 1) {  // only the bits that differ between two keys are sorted on
        uint64_t bor = 0, band = 0;
        int rc = oge_reduce_or_and_u64(ctx, key, nr, ~0ull, &bor, &band);
        if (!rc) rc = oge_radix_sort_pairs(ctx, key, val, ktmp, vtmp, nr, bor ^ band, &ks, &vs);
        if (rc) return rc;
    }
    k_region_rights<<<oge_ceil_div(nr, 256), 256, 0, ctx->stream>>>(reg, vs, nr, rmax);
    OGE_LAUNCH_CHECK(ctx);
    k_region_runmax<<<1, 256, 0, ctx->stream>>>(rmax, nr);
    OGE_LAUNCH_CHECK(ctx);
    stage.begin("filter");
    k_keep_regions<<<oge_ceil_div(n, 256), 256, 0, ctx->stream>>>(d_recs, d_off, n, *o, ks, rmax, nr, keep);
    OGE_LAUNCH_CHECK(ctx);
    stage.end();
    return compact_kept(ctx, d_recs, d_off, n, keep, o->count_limit, d_out, d_out_off, n_out);
}
