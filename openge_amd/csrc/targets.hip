// targets.hip -- `openge targets`: the realignment target intervals of a record set resident in HBM, from the reads'
// own indels (definitions in DESIGN.md section 25 and include/openge_hip.h; the model is tests/targets_model.py).
// Every count is an integer sum and every interval a maximum: the result depends neither on the order of the
// records nor on the order in which the appends land.
//
//   count    k_tg_count    one pass over the record cores and CIGARs: the read filter, the reads used and their
//                          events summed per workgroup (ONE 64-bit atomic per counter and workgroup), the lowest
//                          record of each kind of fault.  The total sizes the event arena exactly.
//   events   k_tg_events   the same walk again (cores and CIGARs only, nothing else of a record is read): a
//                          workgroup takes kTile consecutive records, the threads' event counts are scanned in the
//                          workgroup and the tile's events are appended with ONE atomic; a thread stores its reads'
//                          events one after the other as key = refID << 32 | start, value = stop
//   sort     the existing radix passes on the key bits that vary.  Events of one (refID, start) need no order
//            among themselves: an interval's stop is a maximum and n_events a count, and two events of one start
//            whose stops lie below it (clipped to the contig's length) carry the same stop.
//   merge    the running maximum of refID << 32 | stop over the sorted events (k_tg_tilemax / k_tg_tilescan /
//            k_tg_heads, as bai_query.hip's union of ranges): an event is a head when its refID differs from the
//            maximum's -- compared on its own, so `+ gap` never carries into the next contig -- or its start lies
//            past the maximum's stop + gap.  The scan of the head flags numbers the intervals; k_tg_intervals
//            stores each head's key and position and each interval's last running stop.
//   drop     k_tg_keep, scan, k_tg_compact: the intervals shorter than max_interval as oge_target records
//            (n_events from the head positions) and, with the text, each line's length from comparisons
//   text     64-bit scan of the lengths, k_tg_emit: every byte of "contig:start-stop\n" stored once at its
//            final offset, the contig names from a table uploaded when it changes
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "bam_layout.h"
#include "dev_util.h"
#include "oge_ctx.h"
#include "sam_format.h"

namespace {

constexpr int kT = 256;
constexpr int kWaves = kT / 64;
constexpr int kPer = 4;
constexpr int kTile = kT * kPer;    // records of one tile of the event pass: one append atomic
constexpr int kMPer = 4;
constexpr int kMTile = kT * kMPer;  // sorted events of one tile of the running maximum
constexpr unsigned long long kNone = ~0ull;
constexpr uint32_t kSkipFlags = OGE_F_UNMAP | OGE_F_SECONDARY | OGE_F_QCFAIL | OGE_F_DUP;
constexpr uint64_t kStartMax = 0x7FFFFFFFull;
constexpr uint64_t kHi = 0xFFFFFFFF00000000ull;

struct TgAcc {
    unsigned long long reads_used, events;
    unsigned long long bad[3];  // the lowest record with a bad refID, CIGAR size, op code (kNone: none)
    unsigned int n_items, pad;
};

struct TgRead {
    const uint8_t *cigar;
    uint32_t first, last;  // the first and the last aligned op
    uint32_t rid, pos, clip;
};

__device__ __forceinline__ bool is_aligned(uint32_t code) { return code == OGE_CIG_M || code == OGE_CIG_EQ || code == OGE_CIG_X; }
__device__ __forceinline__ bool is_indel(uint32_t code) { return code == OGE_CIG_I || code == OGE_CIG_D; }
__device__ __forceinline__ bool takes_ref(uint32_t code) { return (0x18Du >> code) & 1u; }  // M D N = X

// The read filter and the event count of record i.  false: the read is not used (a fault is recorded in acc when
// there is one to record into).  One pass over the ops: indels count once an aligned op follows them.
__device__ __forceinline__ bool tg_open(const uint8_t *r, uint64_t i, int32_t n_ref, const int32_t *__restrict__ ref_len, TgAcc *acc,
                                        TgRead &t, uint32_t &n_events) {
    n_events = 0;
    const uint32_t w3 = oge_ldu32(r + OGE_OFF_LNAME), w4 = oge_ldu32(r + OGE_OFF_NCIGAR);
    const uint32_t lname = w3 & 0xFF, mapq = (w3 >> 8) & 0xFF, nops = w4 & 0xFFFF, flag = w4 >> 16;
    const int32_t rid = (int32_t)oge_ldu32(r + OGE_OFF_REFID), pos = (int32_t)oge_ldu32(r + OGE_OFF_POS);
    if ((flag & kSkipFlags) || mapq == 0 || mapq == 255 || rid < 0 || pos < 0) return false;
    if ((flag & OGE_F_PAIRED) && !(flag & OGE_F_MUNMAP) && (int32_t)oge_ldu32(r + OGE_OFF_MREFID) != rid) return false;  // a bad mate
    if (rid >= n_ref) {
        if (acc) atomicMin(&acc->bad[0], (unsigned long long)i);
        return false;
    }
    if ((uint64_t)OGE_OFF_NAME + lname + 4ull * nops > 4ull + oge_ldu32(r + OGE_OFF_BLOCK)) {
        if (acc) atomicMin(&acc->bad[1], (unsigned long long)i);
        return false;
    }
    const uint8_t *c = r + OGE_OFF_NAME + lname;
    uint32_t first = nops, last = 0, pending = 0, total = 0;
    bool badop = false;
    for (uint32_t j = 0; j < nops; ++j) {
        const uint32_t code = oge_ldu32(c + 4 * j) & 0xF;
        badop |= code > 8;
        if (is_aligned(code)) {
            if (first == nops) first = j;
            last = j;
            total += pending;
            pending = 0;
        } else if (is_indel(code) && first != nops) {
            ++pending;
        }
    }
    if (badop) {
        if (acc) atomicMin(&acc->bad[2], (unsigned long long)i);
        return false;
    }
    const int32_t ln = ref_len[rid];
    t = {c, first, last, (uint32_t)rid, (uint32_t)pos, ln > 0 ? (uint32_t)ln : 0u};
    n_events = total;
    return true;
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

__global__ __launch_bounds__(kT) void k_tg_count(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ off, uint64_t n, int32_t n_ref,
                                                 const int32_t *__restrict__ ref_len, TgAcc *__restrict__ acc) {
    __shared__ unsigned long long s_part[kWaves][2];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t used = 0, events = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kT) {
        TgRead t;
        uint32_t ne;
        if (tg_open(recs + off[i], i, n_ref, ref_len, acc, t, ne)) {
            ++used;
            events += ne;
        }
    }
    used = wave_sum_u64(used), events = wave_sum_u64(events);
    if (lane == 0) s_part[wave][0] = used, s_part[wave][1] = events;
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long v = 0;
        for (int w = 0; w < kWaves; ++w) v += s_part[w][threadIdx.x];
        if (v) atomicAdd(&acc->reads_used + threadIdx.x, v);  // words 0, 1: reads_used, events
    }
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)v, d, 64);
        if (lane >= (uint32_t)d) v += y;
    }
    return v;
}

__global__ __launch_bounds__(kT) void k_tg_events(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ off, uint64_t n, int32_t n_ref,
                                                  const int32_t *__restrict__ ref_len, uint64_t *__restrict__ key, uint32_t *__restrict__ val,
                                                  uint64_t cap, TgAcc *__restrict__ acc) {
    __shared__ uint32_t s_cnt[kWaves];
    __shared__ uint32_t s_base;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t ntiles = (n + kTile - 1) / kTile;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // block-uniform
        TgRead t[kPer];
        uint32_t ne[kPer], mine = 0;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const uint64_t i = tile * kTile + (uint64_t)k * kT + threadIdx.x;
            ne[k] = 0;
            if (i < n && !tg_open(recs + off[i], i, n_ref, ref_len, nullptr, t[k], ne[k])) ne[k] = 0;
            mine += ne[k];
        }
        // ---- slots: the threads' counts scanned in the wave, the wave counts through LDS, one atomic per tile
        const uint32_t incl = wave_incl_scan(mine, lane);
        if (lane == 63) s_cnt[wave] = incl;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t sum = 0;
            for (int w = 0; w < kWaves; ++w) sum += s_cnt[w];
            s_base = sum ? atomicAdd(&acc->n_items, sum) : 0;
        }
        __syncthreads();
        uint64_t slot = (uint64_t)s_base + (incl - mine);
        for (uint32_t w = 0; w < wave; ++w) slot += s_cnt[w];
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            if (!ne[k]) continue;
            uint64_t consumed = 0;
            for (uint32_t j = 0; j <= t[k].last; ++j) {  // from op 0: a D or N in front of `first` is no event but takes bases
                const uint32_t op = oge_ldu32(t[k].cigar + 4 * j), code = op & 0xF, len = op >> 4;
                if (j > t[k].first && j < t[k].last && is_indel(code)) {
                    const uint64_t a = (uint64_t)t[k].pos + consumed;
                    const uint64_t stop = code == OGE_CIG_I ? a + 1 : a + len;
                    if (slot < cap) {
                        key[slot] = ((uint64_t)t[k].rid << 32) | (a < kStartMax ? a : kStartMax);
                        val[slot] = (uint32_t)(stop < t[k].clip ? stop : t[k].clip);
                    }
                    ++slot;
                }
                if (takes_ref(code)) consumed += len;
            }
        }
        __syncthreads();  // the next tile rewrites s_cnt and s_base
    }
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

// refID << 32 | stop of the sorted event j
__device__ __forceinline__ uint64_t ref_stop(const uint64_t *__restrict__ ks, const uint32_t *__restrict__ vs, uint64_t j) {
    return (ks[j] & kHi) | vs[j];
}

__global__ __launch_bounds__(kT) void k_tg_tilemax(const uint64_t *__restrict__ ks, const uint32_t *__restrict__ vs, uint64_t n,
                                                   uint64_t *__restrict__ tmax) {
    __shared__ uint64_t sm[kT];
    const uint64_t i0 = (uint64_t)blockIdx.x * kMTile + (uint64_t)threadIdx.x * kMPer;
    uint64_t x = 0;
    for (int k = 0; k < kMPer; ++k)
        if (i0 + k < n) x = max64(x, ref_stop(ks, vs, i0 + k));
    (void)block_excl_max(sm, x);
    if (threadIdx.x == kT - 1) tmax[blockIdx.x] = sm[kT - 1];
}

// one workgroup: tmax -> its exclusive running maximum, in place
__global__ __launch_bounds__(kT) void k_tg_tilescan(uint64_t *__restrict__ tmax, uint64_t nt) {
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

// head[j] = 1 where event j opens an interval; m[j] = the inclusive running maximum; head has n + 2 entries, the
// last two 0.  Event 0 is a head whatever the (empty) maximum before it says.
__global__ __launch_bounds__(kT) void k_tg_heads(const uint64_t *__restrict__ ks, const uint32_t *__restrict__ vs, uint64_t n, uint64_t gap,
                                                 const uint64_t *__restrict__ tcarry, uint64_t *__restrict__ m, uint32_t *__restrict__ head) {
    __shared__ uint64_t sm[kT];
    const uint64_t i0 = (uint64_t)blockIdx.x * kMTile + (uint64_t)threadIdx.x * kMPer;
    uint64_t x[kMPer], mx = 0;
    for (int k = 0; k < kMPer; ++k) {
        x[k] = i0 + k < n ? ref_stop(ks, vs, i0 + k) : 0;
        mx = max64(mx, x[k]);
    }
    uint64_t ex = max64(tcarry[blockIdx.x], block_excl_max(sm, mx));
    for (int k = 0; k < kMPer; ++k) {
        const uint64_t j = i0 + k;
        if (j >= n + 2) break;
        if (j >= n) {
            head[j] = 0;
            continue;
        }
        const uint64_t key = ks[j];
        // the refID on its own: stop + gap of one contig never reaches into the next
        head[j] = j == 0 || (key >> 32) != (ex >> 32) || (key & 0xFFFFFFFFull) > (ex & 0xFFFFFFFFull) + gap;
        ex = max64(ex, x[k]);
        m[j] = ex;
    }
}

// hs = the exclusive scan of the head flags (n + 2 entries): event j opens interval hs[j] when hs[j + 1] != hs[j]
// and closes its interval when the next event opens one or there is none
__global__ __launch_bounds__(kT) void k_tg_intervals(const uint64_t *__restrict__ ks, const uint64_t *__restrict__ m,
                                                     const uint32_t *__restrict__ hs, uint64_t n, uint64_t *__restrict__ iv_key,
                                                     uint32_t *__restrict__ iv_at, uint32_t *__restrict__ iv_stop) {
    const uint64_t j = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (j >= n) return;
    const uint32_t before = hs[j], upto = hs[j + 1];
    if (upto != before) {
        iv_key[before] = ks[j];
        iv_at[before] = (uint32_t)j;
    }
    if (j + 1 == n || hs[j + 2] != upto) iv_stop[upto - 1] = (uint32_t)(m[j] & 0xFFFFFFFFull);
}

// keep has ni + 1 entries, the last 0
__global__ __launch_bounds__(kT) void k_tg_keep(const uint64_t *__restrict__ iv_key, const uint32_t *__restrict__ iv_stop, uint64_t ni,
                                                int64_t max_interval, uint32_t *__restrict__ keep) {
    const uint64_t d = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (d > ni) return;
    keep[d] = d < ni && (int64_t)iv_stop[d] - (int64_t)(iv_key[d] & 0xFFFFFFFFull) < max_interval;
}

// slot = the exclusive scan of keep; size (nk + 1 entries, the last 0; may be NULL) = the kept intervals' text lengths
__global__ __launch_bounds__(kT) void k_tg_compact(const uint64_t *__restrict__ iv_key, const uint32_t *__restrict__ iv_at,
                                                   const uint32_t *__restrict__ iv_stop, const uint32_t *__restrict__ slot, uint64_t ni,
                                                   uint64_t n_events, const uint32_t *__restrict__ name_off, oge_target *__restrict__ out,
                                                   uint64_t *__restrict__ size) {
    const uint64_t d = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (d > ni) return;
    if (d == ni) {
        if (size) size[slot[ni]] = 0;
        return;
    }
    const uint32_t s = slot[d];
    if (slot[d + 1] == s) return;
    const uint64_t key = iv_key[d];
    const uint32_t rid = (uint32_t)(key >> 32), start = (uint32_t)key, stop = iv_stop[d];
    const uint64_t next = d + 1 < ni ? iv_at[d + 1] : n_events;
    out[s] = {(int32_t)rid, (int32_t)start, (int32_t)stop, (uint32_t)(next - iv_at[d])};
    if (size) size[s] = (uint64_t)(name_off[rid + 1] - name_off[rid]) + 1 + oge_txt_dec_width(start) + 1 + oge_txt_dec_width(stop) + 1;
}

__device__ __forceinline__ uint8_t *put_dec(uint8_t *p, uint32_t v) {
    const uint32_t w = oge_txt_dec_width(v);
    for (uint32_t k = w; k-- > 0;) {
        p[k] = (uint8_t)('0' + v % 10u);
        v /= 10u;
    }
    return p + w;
}

// one thread per line, every byte stored once at its final offset
__global__ __launch_bounds__(kT) void k_tg_emit(const oge_target *__restrict__ tg, uint64_t nk, const uint64_t *__restrict__ at,
                                                const uint8_t *__restrict__ names, const uint32_t *__restrict__ name_off,
                                                uint8_t *__restrict__ text) {
    const uint64_t d = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (d >= nk) return;
    const oge_target t = tg[d];
    uint8_t *p = text + at[d];
    const uint32_t n0 = name_off[t.ref_id], n1 = name_off[t.ref_id + 1];
    for (uint32_t k = n0; k < n1; ++k) *p++ = names[k];
    *p++ = ':';
    p = put_dec(p, (uint32_t)t.start);
    *p++ = '-';
    p = put_dec(p, (uint32_t)t.stop);
    *p = '\n';
}

inline dim3 grid_for(uint64_t items) { return dim3(std::max<uint32_t>(1, oge_ceil_div(items, kT))); }

}  // namespace

int oge_targets_impl(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, int32_t n_ref, const int32_t *ref_len,
                     const char *ref_names, uint64_t names_bytes, const oge_targets_opts *opts, oge_targets_result *out,
                     const oge_target **d_targets, const uint8_t **d_text) {
    memset(out, 0, sizeof *out);
    *d_targets = nullptr;
    if (d_text) *d_text = nullptr;
    const bool want_text = opts->want & OGE_TARGETS_TEXT;
    if (opts->want & ~(uint32_t)OGE_TARGETS_TEXT) return oge_fail(ctx, OGE_ERR_ARG, "targets: unknown request bits");
    if (opts->max_interval < 1) return oge_fail(ctx, OGE_ERR_ARG, "targets: max_interval < 1");
    if (opts->gap < 0) return oge_fail(ctx, OGE_ERR_ARG, "targets: gap < 0");
    if (n_ref < 0 || (n_ref && !ref_len)) return oge_fail(ctx, OGE_ERR_ARG, "targets: n_ref < 0 or no reference lengths");
    if (n && (!d_recs || !d_off)) return oge_fail(ctx, OGE_ERR_ARG, "targets: null argument");
    if (want_text && !d_text) return oge_fail(ctx, OGE_ERR_ARG, "targets: the text requested without an output pointer");
    // the names NUL-terminated one after the other -> back to back with n_ref + 1 offsets (oge_contig_table's form)
    std::string names;
    std::vector<uint32_t> name_off(1, 0);
    if (want_text) {
        if (n_ref && !ref_names) return oge_fail(ctx, OGE_ERR_ARG, "targets: no contig names");
        uint64_t p = 0;
        for (int32_t r = 0; r < n_ref; ++r) {
            const void *z = p < names_bytes ? memchr(ref_names + p, 0, names_bytes - p) : nullptr;
            if (!z) return oge_fail(ctx, OGE_ERR_ARG, "targets: the contig names are not n_ref NUL-terminated strings");
            const uint64_t len = (const char *)z - (ref_names + p);
            names.append(ref_names + p, len);
            name_off.push_back((uint32_t)names.size());
            p += len + 1;
        }
    }
    OgeStage stage(ctx, "targets");
    hipStream_t st = ctx->stream;
    ctx->counters["targets_tile_records"] = kTile;
    ctx->counters["targets_merge_tile"] = kMTile;
    if (want_text) {
        oge_text_opts to;
        memset(&to, 0, sizeof to);
        to.n_ref = n_ref;
        to.ref_names = names.data();
        to.ref_name_off = name_off.data();
        const int rc = oge_contig_table(ctx, &ctx->targets_table, &to, "targets");
        if (rc) return rc;
    }
    TgAcc *acc = (TgAcc *)ctx->ws("tg_acc", sizeof(TgAcc));
    int32_t *dlen = (int32_t *)ctx->ws("tg_ref_len", ((size_t)n_ref + 1) * 4);
    if (!acc || !dlen) return OGE_ERR_HIP;
    TgAcc h;
    memset(&h, 0, sizeof h);
    for (auto &v : h.bad) v = kNone;
    OGE_HIP_TRY(ctx, hipMemcpyAsync(acc, &h, sizeof h, hipMemcpyHostToDevice, st));
    if (n_ref) OGE_HIP_TRY(ctx, hipMemcpyAsync(dlen, ref_len, (size_t)n_ref * 4, hipMemcpyHostToDevice, st));
    // ---- count: the filter, the faults, the exact size of the event arena
    OgeStage part(ctx, "targets_count");  // nested in targets: count, events, sort, merge, text
    if (n) {
        const dim3 g((uint32_t)std::min<uint64_t>(oge_ceil_div(n, kT), (uint64_t)ctx->cu_count() * 8));
        hipLaunchKernelGGL(k_tg_count, g, dim3(kT), 0, st, d_recs, d_off, n, n_ref, (const int32_t *)dlen, acc);
        OGE_LAUNCH_CHECK(ctx);
    }
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&h, acc, sizeof h, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    static const char *const kBad[3] = {"passes the read filter with a refID outside [0, n_ref)", "has a CIGAR that does not fit its block_size",
                                        "has a CIGAR op code above 8"};
    int bad = -1;
    for (int k = 0; k < 3; ++k)
        if (h.bad[k] != kNone && (bad < 0 || h.bad[k] < h.bad[bad])) bad = k;
    if (bad >= 0) return oge_fail(ctx, OGE_ERR_ARG, ("targets: record " + std::to_string(h.bad[bad]) + " " + kBad[bad]).c_str());
    const uint64_t E = h.events;
    out->reads_used = h.reads_used;
    out->events = E;
    ctx->counters["targets_events"] = E;
    if (E >= 0xFFFFFFFFull) return oge_fail(ctx, OGE_ERR_LIMIT, "targets: 2^32-1 or more events");
    if (!E) return OGE_OK;
    // ---- events
    part.begin("targets_events");
    uint64_t *ka = (uint64_t *)ctx->ws("tg_ka", (E + 2) * 8), *kb = (uint64_t *)ctx->ws("tg_kb", (E + 2) * 8);
    uint32_t *va = (uint32_t *)ctx->ws("tg_va", (E + 2) * 4), *vb = (uint32_t *)ctx->ws("tg_vb", (E + 2) * 4);
    const uint64_t nt = (E + 2 + kMTile - 1) / kMTile;  // the tiles of the head flags' E + 2 entries
    uint64_t *tmax = (uint64_t *)ctx->ws("tg_tmax", nt * 8);
    if (!ka || !kb || !va || !vb || !tmax) return OGE_ERR_HIP;
    {
        const uint64_t ntiles = (n + kTile - 1) / kTile;
        const dim3 g((uint32_t)std::min<uint64_t>(ntiles, (uint64_t)ctx->cu_count() * 8));
        hipLaunchKernelGGL(k_tg_events, g, dim3(kT), 0, st, d_recs, d_off, n, n_ref, (const int32_t *)dlen, ka, va, E, acc);
        OGE_LAUNCH_CHECK(ctx);
    }
    uint32_t appended = 0;
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&appended, &acc->n_items, 4, hipMemcpyDeviceToHost, st));
    // ---- sort on the varying key bits; equal keys need no order among themselves (see the head of this file)
    part.begin("targets_sort");
    uint64_t bor = 0, band = 0, *ks = ka;
    uint32_t *vs = va;
    int rc = oge_reduce_or_and_u64(ctx, ka, E, ~0ull, &bor, &band);
    if (rc) return rc;
    if (appended != E) return oge_fail(ctx, OGE_ERR_HIP, "targets: the two passes counted different events (internal error)");
    rc = oge_radix_sort_pairs(ctx, ka, va, kb, vb, E, bor ^ band, &ks, &vs);
    if (rc) return rc;
    uint64_t *m = ks == ka ? kb : ka;      // the sort's other buffers are free
    uint32_t *head = vs == va ? vb : va;   // E + 2 entries
    // ---- merge
    part.begin("targets_merge");
    hipLaunchKernelGGL(k_tg_tilemax, dim3((uint32_t)nt), dim3(kT), 0, st, (const uint64_t *)ks, (const uint32_t *)vs, E, tmax);
    OGE_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_tg_tilescan, dim3(1), dim3(kT), 0, st, tmax, nt);
    OGE_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_tg_heads, dim3((uint32_t)nt), dim3(kT), 0, st, (const uint64_t *)ks, (const uint32_t *)vs, E,
                       (uint64_t)opts->gap, (const uint64_t *)tmax, m, head);
    OGE_LAUNCH_CHECK(ctx);
    rc = oge_exclusive_scan_u32(ctx, head, head, E + 2);
    if (rc) return rc;
    uint32_t ni = 0;
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&ni, head + E, 4, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    out->intervals = ni;
    if (!ni || ni > E) return oge_fail(ctx, OGE_ERR_HIP, "targets: the interval count is out of range (internal error)");
    uint64_t *iv_key = (uint64_t *)ctx->ws("tg_iv_key", (uint64_t)ni * 8);
    uint32_t *iv_at = (uint32_t *)ctx->ws("tg_iv_at", (uint64_t)ni * 4), *iv_stop = (uint32_t *)ctx->ws("tg_iv_stop", (uint64_t)ni * 4);
    uint32_t *keep = (uint32_t *)ctx->ws("tg_keep", ((uint64_t)ni + 1) * 4);
    if (!iv_key || !iv_at || !iv_stop || !keep) return OGE_ERR_HIP;
    hipLaunchKernelGGL(k_tg_intervals, grid_for(E), dim3(kT), 0, st, (const uint64_t *)ks, (const uint64_t *)m, (const uint32_t *)head, E, iv_key,
                       iv_at, iv_stop);
    OGE_LAUNCH_CHECK(ctx);
    // ---- drop and compact
    hipLaunchKernelGGL(k_tg_keep, grid_for((uint64_t)ni + 1), dim3(kT), 0, st, (const uint64_t *)iv_key, (const uint32_t *)iv_stop, (uint64_t)ni,
                       (int64_t)opts->max_interval, keep);
    OGE_LAUNCH_CHECK(ctx);
    rc = oge_exclusive_scan_u32(ctx, keep, keep, (uint64_t)ni + 1);
    if (rc) return rc;
    uint32_t nk = 0;
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&nk, keep + ni, 4, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (nk > ni) return oge_fail(ctx, OGE_ERR_HIP, "targets: more kept intervals than intervals (internal error)");
    out->targets = nk;
    out->dropped_long = ni - nk;
    if (!nk) return OGE_OK;
    oge_target *tg = (oge_target *)ctx->ws("tg_out", (uint64_t)nk * sizeof(oge_target));
    uint64_t *at = want_text ? (uint64_t *)ctx->ws("tg_at", ((uint64_t)nk + 1) * 8) : nullptr;
    if (!tg || (want_text && !at)) return OGE_ERR_HIP;
    hipLaunchKernelGGL(k_tg_compact, grid_for((uint64_t)ni + 1), dim3(kT), 0, st, (const uint64_t *)iv_key, (const uint32_t *)iv_at,
                       (const uint32_t *)iv_stop, (const uint32_t *)keep, (uint64_t)ni, E, ctx->targets_table.d_name_off, tg, at);
    OGE_LAUNCH_CHECK(ctx);
    if (want_text) {
        // ---- text: the lines' offsets, then every byte once
        part.begin("targets_text");
        rc = oge_exclusive_scan_u64(ctx, at, at, (uint64_t)nk + 1);
        if (rc) return rc;
        uint64_t total = 0;
        OGE_HIP_TRY(ctx, hipMemcpyAsync(&total, at + nk, 8, hipMemcpyDeviceToHost, st));
        OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
        uint8_t *text = (uint8_t *)ctx->ws("tg_text", total);
        if (!text) return OGE_ERR_HIP;
        hipLaunchKernelGGL(k_tg_emit, grid_for(nk), dim3(kT), 0, st, (const oge_target *)tg, (uint64_t)nk, (const uint64_t *)at,
                           ctx->targets_table.d_names, ctx->targets_table.d_name_off, text);
        OGE_LAUNCH_CHECK(ctx);
        out->text_bytes = total;
        *d_text = text;
    }
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    *d_targets = tg;
    return OGE_OK;
}

extern "C" {

void oge_targets_opts_init(oge_targets_opts *o) {
    if (!o) return;
    o->max_interval = 500;
    o->gap = 0;
    o->want = OGE_TARGETS_TEXT;
}

int oge_targets_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, int32_t n_ref, const int32_t *ref_len,
                    const char *ref_names, uint64_t names_bytes, const oge_targets_opts *opts, oge_targets_result *result,
                    const oge_target **d_targets, const uint8_t **d_text) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!opts || !result || !d_targets) return oge_fail(ctx, OGE_ERR_ARG, "oge_targets_dev: null argument");
    OgeCall call(ctx, /*hold=*/false);
    return oge_targets_impl(ctx, d_recs, d_off, n, n_ref, ref_len, ref_names, names_bytes, opts, result, d_targets, d_text);
}

int oge_targets(oge_ctx *ctx, const uint8_t *recs, uint64_t rec_bytes, const uint64_t *rec_off, uint64_t n, int32_t n_ref,
                const int32_t *ref_len, const char *ref_names, uint64_t names_bytes, const oge_targets_opts *opts,
                oge_targets_result *result, oge_target *targets_out, uint64_t targets_cap, uint8_t *text_out, uint64_t text_cap) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!opts || !result || (n && (!recs || !rec_off))) return oge_fail(ctx, OGE_ERR_ARG, "oge_targets: null argument");
    (void)hipSetDevice(ctx->device);
    uint8_t *dr = (uint8_t *)ctx->ws("host_recs", rec_bytes + 16);
    uint64_t *dof = (uint64_t *)ctx->ws("host_off", (n + 1) * 8);
    if (!dr || !dof) return OGE_ERR_HIP;
    if (rec_bytes) OGE_HIP_TRY(ctx, hipMemcpyAsync(dr, recs, rec_bytes, hipMemcpyHostToDevice, ctx->stream));
    OGE_HIP_TRY(ctx, hipMemsetAsync(dr + rec_bytes, 0, 16, ctx->stream));
    if (n) OGE_HIP_TRY(ctx, hipMemcpyAsync(dof, rec_off, n * 8, hipMemcpyHostToDevice, ctx->stream));
    const oge_target *dt = nullptr;
    const uint8_t *dx = nullptr;
    const int rc = oge_targets_dev(ctx, dr, dof, n, n_ref, ref_len, ref_names, names_bytes, opts, result, &dt, &dx);
    if (rc) return rc;
    if (result->targets > targets_cap || (result->targets && !targets_out) || result->text_bytes > text_cap ||
        (result->text_bytes && !text_out))
        return oge_fail(ctx, OGE_ERR_LIMIT, "oge_targets: output buffer too small");
    if (result->targets) OGE_HIP_TRY(ctx, hipMemcpyAsync(targets_out, dt, result->targets * sizeof(oge_target), hipMemcpyDeviceToHost, ctx->stream));
    if (result->text_bytes) OGE_HIP_TRY(ctx, hipMemcpyAsync(text_out, dx, result->text_bytes, hipMemcpyDeviceToHost, ctx->stream));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return OGE_OK;
}

}  // extern "C"
