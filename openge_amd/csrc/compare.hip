// compare.hip -- `openge compare`: the multiset difference of the read placements (refID, pos, CIGAR ops) of two
// record sets resident in HBM (the reference's commands/command_compare.cpp; definitions in DESIGN.md section 23
// and include/openge_hip.h).  Every count is an integer sum: the result depends neither on the order of the
// records nor on the hash.
//
//   keys     k_cmp_keys    one pass over the record cores and CIGARs of one set; a workgroup takes kKeyTile
//                          consecutive records, every record inside the region becomes an item
//                            primary    refID : pos (both with the sign bit flipped: unsigned order = signed order)
//                            secondary  n_ops:16 | side:1 | hash:47 of the ops re-coded as len << 4 | rank(type char)
//                            record     its index in its set
//                          appended at a slot from ballot ranks, the wave counts summed in LDS and ONE atomic per
//                          tile; a CIGAR of more than kWideOps ops is hashed by the whole wave (the hash is a sum
//                          of per-op mixes, so the lanes' partial sums add up)
//   pack     k_cmp_pack    both keys into ONE 64-bit sort key, refID | pos | n_ops | hash, every field as wide as its
//                          varying bits (an OR / AND reduction of the keys) and the hash as wide as fills the last
//                          8-bit radix digit (at least kMinHash bits, what is left of 64 at most)
//   sort     the union by that key: one run of the existing radix passes (oge_radix_sort_pairs)
//   flags    k_cmp_flags   per sorted item: does it start a run of equal keys, which side is it from and, inside a
//                          run, do its ops differ from its predecessor's IN THE ARENAS; the existing scan turns the
//                          three flags into run numbers and per-run sums
//   runs     k_cmp_runs    one thread per run: a run whose items all carry the same ops adds min(a, b), a - min and
//                          b - min to the counters (per-wave sums, one 64-bit atomic per workgroup and counter)
//                          and, with a surplus, appends one diff entry; a run that holds two different CIGARs (a
//                          hash collision) goes to the hard list
//            k_cmp_hard    one workgroup per hard run: every item looks for the first item of the run with its
//                          ops; the first of each group counts the group's two sides and does what k_cmp_runs
//                          does for a run.  Exact whatever the hash: with debug_hash_bits = 0 every run that
//                          holds two CIGARs of one length at one position takes this path.
//   diff     k_cmp_size / k_cmp_emit  (OGE_COMPARE_DIFF) entry sizes, scan, then every entry written once at its
//                          final offset: refID, pos, surplus, side, n_ops, ops[]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "bam_layout.h"
#include "dev_util.h"
#include "oge_ctx.h"

namespace {

constexpr int kT = 256;
constexpr int kWaves = kT / 64;
constexpr int kKeyPer = 4;
constexpr int kKeyTile = kT * kKeyPer;  // records of one key tile: one append atomic
constexpr uint32_t kWideOps = 16;       // CIGARs longer than this are hashed by the whole wave
constexpr int kHashBits = 47;
constexpr uint32_t kMinHash = 20;        // hash bits of the sort key before it is rounded up to whole radix digits
constexpr uint64_t kSideBit = 1ull << kHashBits;
constexpr uint64_t kHashMask = kSideBit - 1;
constexpr unsigned long long kNone = ~0ull;
constexpr uint32_t kEntryHead = 24;  // bytes of a diff image entry in front of its ops

struct CmpAcc {
    unsigned long long common, adds, dels;   // the three counters
    unsigned long long bad[2][3];  // per set: the lowest record index with a bad refID, CIGAR size, op code (kNone: none)
    unsigned int n_items, n_diff, n_hard, pad;
};

struct CmpSet {
    const uint8_t *recs;
    const uint64_t *off;
};

// one diff entry before it is sized: a representative record (set `arena`, index rec) and the surplus of `side`
struct CmpDiff {
    uint32_t rec, meta;  // meta bit 0: side of the surplus (0 = file 0: a deletion, 1 = an addition); bit 1: arena
    uint32_t surplus, pad;
};

// rank of the type character among "=DHIMNPSX" by BAM op code ("MIDNSHP=X")
__device__ __forceinline__ uint32_t op_rank(uint32_t code) {
    return (0x806275134ull >> (4 * code)) & 0xF;  // M4 I3 D1 N5 S7 H2 P6 =0 X8
}

__device__ __forceinline__ uint64_t op_mix(uint32_t op, uint32_t i) {
    uint64_t x = (uint64_t)(((op >> 4) << 4) | op_rank(op & 0xF)) + 0x9E3779B97F4A7C15ull * ((uint64_t)i + 1);
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__device__ __forceinline__ uint64_t hash_finish(uint64_t sum) {
    sum ^= sum >> 33;
    sum *= 0xFF51AFD7ED558CCDull;
    return sum ^ (sum >> 29);
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ const uint8_t *cigar_of(const uint8_t *r) { return r + OGE_OFF_NAME + (oge_ldu32(r + OGE_OFF_LNAME) & 0xFF); }

__global__ __launch_bounds__(kT) void k_cmp_keys(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ off, uint64_t n,
                                                 oge_compare_region rg, int32_t n_ref, uint32_t side,
                                                 uint64_t *__restrict__ pri, uint64_t *__restrict__ sec, uint32_t *__restrict__ rec,
                                                 uint64_t cap, CmpAcc *__restrict__ acc) {
    __shared__ uint32_t s_cnt[kWaves];
    __shared__ uint32_t s_base;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t ntiles = (n + kKeyTile - 1) / kKeyTile;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // block-uniform
        uint64_t kp[kKeyPer], ks[kKeyPer], bal[kKeyPer];
        bool in[kKeyPer];
        uint32_t wcount = 0;
#pragma unroll
        for (int k = 0; k < kKeyPer; ++k) {
            const uint64_t i = tile * kKeyTile + (uint64_t)k * kT + threadIdx.x;
            in[k] = false;
            kp[k] = ks[k] = 0;
            const uint8_t *c = nullptr;
            uint32_t nops = 0;
            bool badop = false;
            if (i < n) {
                const uint8_t *r = recs + off[i];
                const int32_t rid = (int32_t)oge_ldu32(r + OGE_OFF_REFID), pos = (int32_t)oge_ldu32(r + OGE_OFF_POS);
                if (rid >= rg.left_ref && rid <= rg.right_ref && pos >= rg.left_pos && pos <= rg.right_pos) {
                    nops = oge_ldu32(r + OGE_OFF_NCIGAR) & 0xFFFF;
                    const uint32_t lname = oge_ldu32(r + OGE_OFF_LNAME) & 0xFF, bs = oge_ldu32(r + OGE_OFF_BLOCK);
                    if (rid < 0 || rid >= n_ref) atomicMin(&acc->bad[side][0], (unsigned long long)i);
                    else if ((uint64_t)OGE_OFF_NAME + lname + 4ull * nops > 4ull + bs) atomicMin(&acc->bad[side][1], (unsigned long long)i);
                    else {
                        in[k] = true;
                        c = r + OGE_OFF_NAME + lname;
                        kp[k] = ((uint64_t)((uint32_t)rid ^ 0x80000000u) << 32) | ((uint32_t)pos ^ 0x80000000u);
                    }
                }
            }
            // ---- the hash: short CIGARs per lane, wide ones by the whole wave
            uint64_t sum = 0;
            if (in[k] && nops <= kWideOps)
                for (uint32_t j = 0; j < nops; ++j) {
                    const uint32_t op = oge_ldu32(c + 4 * j);
                    badop |= (op & 0xF) > 8;
                    sum += op_mix(op, j);
                }
            uint64_t wide = __ballot(in[k] && nops > kWideOps);
            while (wide) {  // wave-uniform
                const int src = __ffsll((long long)wide) - 1;
                wide &= wide - 1;
                const uint8_t *xc = (const uint8_t *)shfl_u64((uint64_t)(uintptr_t)c, src);
                const uint32_t xn = (uint32_t)__shfl((int)nops, src, 64);
                uint64_t part = 0;
                bool xbad = false;
                for (uint32_t j = lane; j < xn; j += 64) {
                    const uint32_t op = oge_ldu32(xc + 4 * j);
                    xbad |= (op & 0xF) > 8;
                    part += op_mix(op, j);
                }
                part = wave_sum_u64(part);
                const bool anybad = __ballot(xbad) != 0;
                if ((int)lane == src) {
                    sum = part;
                    badop = anybad;
                }
            }
            if (badop) {
                atomicMin(&acc->bad[side][2], (unsigned long long)i);
                in[k] = false;
            }
            ks[k] = ((uint64_t)nops << 48) | (side ? kSideBit : 0) | (hash_finish(sum) & kHashMask);
            bal[k] = __ballot(in[k]);
            wcount += (uint32_t)__popcll(bal[k]);
        }
        // ---- slots: the wave counts through LDS, one atomic per tile
        if (lane == 0) s_cnt[wave] = wcount;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t t = 0;
            for (int w = 0; w < kWaves; ++w) t += s_cnt[w];
            s_base = t ? atomicAdd(&acc->n_items, t) : 0;
        }
        __syncthreads();
        uint32_t slot = s_base;
        for (uint32_t w = 0; w < wave; ++w) slot += s_cnt[w];
#pragma unroll
        for (int k = 0; k < kKeyPer; ++k) {
            const uint32_t mine = slot + (uint32_t)__popcll(bal[k] & ((1ull << lane) - 1ull));
            if (in[k] && mine < cap) {
                pri[mine] = kp[k];
                sec[mine] = ks[k];
                rec[mine] = (uint32_t)(tile * kKeyTile + (uint64_t)k * kT + threadIdx.x);
            }
            slot += (uint32_t)__popcll(bal[k]);
        }
        __syncthreads();  // the next tile rewrites s_cnt and s_base
    }
}

// the record of an item (index into the union: the items of set 0 come first) in its set's arena
__device__ __forceinline__ const uint8_t *item_rec(uint32_t item, uint32_t m_a, const uint32_t *rec, CmpSet a, CmpSet b) {
    const CmpSet s = item >= m_a ? b : a;
    return s.recs + s.off[rec[item]];
}

// the same number of ops and the same ops: with refID and pos, which the sort key holds whole, the same element
__device__ __forceinline__ bool same_ops(const uint8_t *x, const uint8_t *y) {
    const uint32_t nops = oge_ldu32(x + OGE_OFF_NCIGAR) & 0xFFFF;
    if (nops != (oge_ldu32(y + OGE_OFF_NCIGAR) & 0xFFFF)) return false;
    const uint8_t *cx = cigar_of(x), *cy = cigar_of(y);
    for (uint32_t j = 0; j < nops; ++j)
        if (oge_ldu32(cx + 4 * j) != oge_ldu32(cy + 4 * j)) return false;
    return true;
}

// field widths of the packed sort key (bits): refID, pos, n_ops, hash
struct CmpPack {
    uint32_t wr, wp, wn, wh;
};

__host__ __device__ __forceinline__ uint64_t low_bits(uint32_t w) { return w >= 64 ? ~0ull : (1ull << w) - 1; }
__host__ __device__ __forceinline__ uint64_t shl(uint64_t v, uint32_t by) { return by >= 64 ? 0 : v << by; }
__host__ __device__ __forceinline__ uint64_t pack_key(uint64_t pri, uint64_t sec, CmpPack f) {
    return shl((pri >> 32) & low_bits(f.wr), f.wp + f.wn + f.wh) | shl(pri & low_bits(f.wp), f.wn + f.wh) |
           shl((sec >> 48) & low_bits(f.wn), f.wh) | (sec & low_bits(f.wh));
}

__global__ __launch_bounds__(kT) void k_cmp_pack(const uint64_t *__restrict__ pri, const uint64_t *__restrict__ sec, uint64_t m, CmpPack f,
                                                 uint64_t *__restrict__ key, uint32_t *__restrict__ item) {
    const uint64_t j = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (j >= m) return;
    key[j] = pack_key(pri[j], sec[j], f);
    item[j] = (uint32_t)j;
}

// head[j] = item j starts a run; packed[j] = side | (ops differ from the predecessor's) << 32; entry m of both is 0
__global__ __launch_bounds__(kT) void k_cmp_flags(const uint64_t *__restrict__ ks, const uint32_t *__restrict__ perm,
                                                  const uint32_t *__restrict__ rec, uint64_t m, uint32_t m_a, CmpSet a, CmpSet b,
                                                  uint32_t *__restrict__ head, uint64_t *__restrict__ packed) {
    const uint64_t j = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (j > m) return;
    if (j == m) {
        head[j] = 0;
        packed[j] = 0;
        return;
    }
    const bool first = j == 0 || ks[j] != ks[j - 1];
    const uint32_t item = perm[j];
    uint64_t mis = 0;
    if (!first) mis = !same_ops(item_rec(item, m_a, rec, a, b), item_rec(perm[j - 1], m_a, rec, a, b));
    head[j] = first;
    packed[j] = (item >= m_a ? 1u : 0u) | (mis << 32);
}

// slot = the exclusive scan of head: item j starts run slot[j] when slot[j + 1] != slot[j]
__global__ __launch_bounds__(kT) void k_cmp_starts(const uint32_t *__restrict__ slot, uint64_t m, uint32_t *__restrict__ start) {
    const uint64_t j = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (j < m && slot[j + 1] != slot[j]) start[slot[j]] = (uint32_t)j;
}

// what a run (or a group of a hard run) of a items of set 0 and b of the other adds to the counters
__device__ __forceinline__ void count_run(uint64_t a, uint64_t b, unsigned long long &common, unsigned long long &adds,
                                          unsigned long long &dels) {
    const uint64_t mn = a < b ? a : b;
    common += mn;
    dels += a - mn;
    adds += b - mn;
}

__global__ __launch_bounds__(kT) void k_cmp_runs(const uint32_t *__restrict__ start, uint64_t nruns, uint64_t m, uint32_t m_a,
                                                 const uint64_t *__restrict__ cum, const uint32_t *__restrict__ perm,
                                                 const uint32_t *__restrict__ rec, CmpAcc *__restrict__ acc, CmpDiff *__restrict__ diff,
                                                 uint64_t diff_cap, uint32_t *__restrict__ hard) {
    __shared__ unsigned long long s_part[kWaves][3];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t r = (uint64_t)blockIdx.x * kT + threadIdx.x;
    unsigned long long common = 0, adds = 0, dels = 0;
    bool is_hard = false, has_diff = false;
    uint32_t s = 0, e = 0;
    uint64_t a = 0, b = 0;
    if (r < nruns) {
        s = start[r];
        e = r + 1 < nruns ? start[r + 1] : (uint32_t)m;
        const uint64_t d = cum[e] - cum[s];
        b = d & 0xFFFFFFFFull;
        a = (uint64_t)(e - s) - b;
        is_hard = (d >> 32) != 0;
        if (!is_hard) {
            count_run(a, b, common, adds, dels);
            has_diff = a != b;
        }
    }
    const uint32_t hslot = oge_wave_append(is_hard, &acc->n_hard);
    if (is_hard) {
        hard[2 * (uint64_t)hslot] = s;
        hard[2 * (uint64_t)hslot + 1] = e;
    }
    if (diff) {
        const uint32_t dslot = oge_wave_append(has_diff, &acc->n_diff);
        if (has_diff && dslot < diff_cap) {
            const uint32_t item = perm[s];
            diff[dslot] = {rec[item], (b > a ? 1u : 0u) | (item >= m_a ? 2u : 0u), (uint32_t)(b > a ? b - a : a - b), 0};
        }
    }
    common = wave_sum_u64(common), adds = wave_sum_u64(adds), dels = wave_sum_u64(dels);
    if (lane == 0) s_part[wave][0] = common, s_part[wave][1] = adds, s_part[wave][2] = dels;
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long v = 0;
        for (int w = 0; w < kWaves; ++w) v += s_part[w][threadIdx.x];
        if (v) atomicAdd(&acc->common + threadIdx.x, v);  // words 0..2: common, adds, dels
    }
}

// One workgroup per hard run [s, e) of the sorted union: the groups of equal ops, found by comparing the ops
// themselves (quadratic in the run's length; runs are hard only after a hash collision).
__global__ __launch_bounds__(kT) void k_cmp_hard(const uint32_t *__restrict__ hard, uint32_t m_a, const uint32_t *__restrict__ perm,
                                                 const uint32_t *__restrict__ rec, CmpSet a, CmpSet b, CmpAcc *__restrict__ acc, CmpDiff *__restrict__ diff, uint64_t diff_cap) {
    __shared__ unsigned long long s_sum[3];
    if (threadIdx.x < 3) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t s = hard[2 * (uint64_t)blockIdx.x], e = hard[2 * (uint64_t)blockIdx.x + 1];
    for (uint32_t i = s + threadIdx.x; i < e; i += kT) {
        const uint32_t item = perm[i];
        const uint8_t *r = item_rec(item, m_a, rec, a, b);
        bool leader = true;
        for (uint32_t j = s; j < i && leader; ++j) leader = !same_ops(r, item_rec(perm[j], m_a, rec, a, b));
        if (!leader) continue;
        uint64_t na = 0, nb = 0;
        for (uint32_t j = i; j < e; ++j) {
            const uint32_t other = perm[j];
            if (j != i && !same_ops(r, item_rec(other, m_a, rec, a, b))) continue;
            if (other >= m_a) ++nb;
            else ++na;
        }
        unsigned long long common = 0, adds = 0, dels = 0;
        count_run(na, nb, common, adds, dels);
        if (common) atomicAdd(&s_sum[0], common);
        if (adds) atomicAdd(&s_sum[1], adds);
        if (dels) atomicAdd(&s_sum[2], dels);
        if (diff && na != nb) {
            const uint32_t dslot = atomicAdd(&acc->n_diff, 1u);  // one per group of a collision: rare
            if (dslot < diff_cap)
                diff[dslot] = {rec[item], (nb > na ? 1u : 0u) | (item >= m_a ? 2u : 0u), (uint32_t)(nb > na ? nb - na : na - nb), 0};
        }
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_sum[threadIdx.x]) atomicAdd(&acc->common + threadIdx.x, s_sum[threadIdx.x]);
}

__global__ __launch_bounds__(kT) void k_cmp_size(const CmpDiff *__restrict__ diff, uint64_t nd, CmpSet a, CmpSet b,
                                                 uint64_t *__restrict__ size) {
    const uint64_t d = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (d > nd) return;
    uint64_t sz = 0;
    if (d < nd) {
        const CmpSet &s = (diff[d].meta & 2) ? b : a;
        sz = kEntryHead + 4ull * (oge_ldu32(s.recs + s.off[diff[d].rec] + OGE_OFF_NCIGAR) & 0xFFFF);
    }
    size[d] = sz;
}

// image words are 4-byte aligned: every entry is a multiple of 4 bytes
__global__ __launch_bounds__(kT) void k_cmp_emit(const CmpDiff *__restrict__ diff, uint64_t nd, CmpSet a, CmpSet b,
                                                 const uint64_t *__restrict__ at, uint8_t *__restrict__ image) {
    const uint64_t d = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (d >= nd) return;
    const CmpDiff e = diff[d];
    const CmpSet &s = (e.meta & 2) ? b : a;
    const uint8_t *r = s.recs + s.off[e.rec];
    const uint32_t nops = oge_ldu32(r + OGE_OFF_NCIGAR) & 0xFFFF;
    const uint8_t *c = cigar_of(r);
    uint32_t *w = (uint32_t *)(image + at[d]);
    w[0] = oge_ldu32(r + OGE_OFF_REFID);
    w[1] = oge_ldu32(r + OGE_OFF_POS);
    w[2] = e.surplus;
    w[3] = 0;
    w[4] = e.meta & 1;
    w[5] = nops;
    for (uint32_t j = 0; j < nops; ++j) w[6 + j] = oge_ldu32(c + 4 * j);
}

inline dim3 grid_for(uint64_t items) { return dim3(std::max<uint32_t>(1, oge_ceil_div(items, kT))); }

int compare_impl(oge_ctx *ctx, const uint8_t *d_recs_a, const uint64_t *d_off_a, uint64_t n_a, const uint8_t *d_recs_b,
                 const uint64_t *d_off_b, uint64_t n_b, int32_t n_ref, const oge_compare_region *rg, uint32_t want, int hash_bits,
                 oge_compare_result *out, const uint8_t **d_diff, uint64_t *diff_bytes) {
    const bool want_diff = want & OGE_COMPARE_DIFF;
    const uint64_t cap = n_a + n_b;
    if (cap >= 0xFFFFFFFFull) return oge_fail(ctx, OGE_ERR_LIMIT, "compare: 2^32-1 or more records in the two sets");
    OgeStage stage(ctx, "compare");
    hipStream_t st = ctx->stream;
    ctx->counters["compare_tile_records"] = kKeyTile;
    ctx->counters["compare_wide_ops"] = kWideOps;
    CmpAcc *acc = (CmpAcc *)ctx->ws("cmp_acc", sizeof(CmpAcc));
    uint64_t *pri = (uint64_t *)ctx->ws("cmp_pri", (cap + 2) * 8), *sec = (uint64_t *)ctx->ws("cmp_sec", (cap + 2) * 8);
    uint64_t *ka = (uint64_t *)ctx->ws("cmp_ka", (cap + 2) * 8), *kb = (uint64_t *)ctx->ws("cmp_kb", (cap + 2) * 8);
    uint32_t *rec = (uint32_t *)ctx->ws("cmp_rec", (cap + 2) * 4), *va = (uint32_t *)ctx->ws("cmp_va", (cap + 2) * 4),
             *vb = (uint32_t *)ctx->ws("cmp_vb", (cap + 2) * 4);
    if (!acc || !pri || !sec || !ka || !kb || !rec || !va || !vb) return OGE_ERR_HIP;
    CmpAcc h;
    memset(&h, 0, sizeof h);
    for (auto &sd : h.bad)
        for (auto &v : sd) v = kNone;
    OGE_HIP_TRY(ctx, hipMemcpyAsync(acc, &h, sizeof h, hipMemcpyHostToDevice, st));
    const CmpSet A = {d_recs_a, d_off_a}, B = {d_recs_b, d_off_b};
    uint32_t m_a = 0;
    OgeStage part(ctx, "compare_keys");  // nested in compare: the key passes, the sort, the runs
    // ---- keys: set 0's items first (its kernel ends before the other one appends), so item < m_a <=> set 0
    for (int side = 0; side < 2; ++side) {
        const uint64_t n = side ? n_b : n_a;
        if (n) {
            const uint64_t ntiles = (n + kKeyTile - 1) / kKeyTile;
            const dim3 g((uint32_t)std::min<uint64_t>(ntiles, (uint64_t)ctx->cu_count() * 8));
            hipLaunchKernelGGL(k_cmp_keys, g, dim3(kT), 0, st, side ? d_recs_b : d_recs_a, side ? d_off_b : d_off_a, n, *rg, n_ref,
                               (uint32_t)side, pri, sec, rec, cap, acc);
            OGE_LAUNCH_CHECK(ctx);
        }
        if (!side) OGE_HIP_TRY(ctx, hipMemcpyAsync(&m_a, &acc->n_items, 4, hipMemcpyDeviceToHost, st));
    }
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&h, acc, sizeof h, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    static const char *const kBad[3] = {"lies in the region with a refID outside [0, n_ref)", "has a CIGAR that does not fit its block_size",
                                        "has a CIGAR op code above 8"};
    for (int side = 0; side < 2; ++side)
        for (int k = 0; k < 3; ++k)
            if (h.bad[side][k] != kNone)
                return oge_fail(ctx, OGE_ERR_ARG, ("compare: record " + std::to_string(h.bad[side][k]) + " of the " +
                                                   (side ? "second" : "first") + " set " + kBad[k]).c_str());
    const uint64_t m = h.n_items;
    out->n_ref = m_a;
    out->n_other = m - m_a;
    ctx->counters["compare_items"] = m;
    if (!m) return OGE_OK;
    // ---- one sort key: the fields as wide as their varying bits, the hash filling the last radix digit
    part.begin("compare_sort");
    uint64_t o = 0, an = 0;
    int rc = oge_reduce_or_and_u64(ctx, sec, m, ~kSideBit, &o, &an);
    if (rc) return rc;
    const uint64_t vary_sec = o ^ an;
    rc = oge_reduce_or_and_u64(ctx, pri, m, ~0ull, &o, &an);
    if (rc) return rc;
    const uint64_t vary_pri = o ^ an;
    auto width = [](uint64_t v) { return v ? 64u - (uint32_t)__builtin_clzll(v) : 0u; };
    CmpPack f = {width(vary_pri >> 32), width(vary_pri & 0xFFFFFFFFull), width(vary_sec >> 48), 0};
    if (f.wr + f.wp + f.wn > 64) f.wn = 0;  // the op count then only through the hash and the ops themselves
    const uint32_t base = f.wr + f.wp + f.wn;
    f.wh = std::min<uint32_t>(std::min<uint32_t>(kHashBits, 64 - base), (base + kMinHash + 7) / 8 * 8 - base);
    if (hash_bits >= 0 && (uint32_t)hash_bits < f.wh) f.wh = (uint32_t)hash_bits;
    ctx->counters["compare_hash_bits"] = f.wh;
    ctx->counters["compare_key_bits"] = base + f.wh;
    hipLaunchKernelGGL(k_cmp_pack, grid_for(m), dim3(kT), 0, st, (const uint64_t *)pri, (const uint64_t *)sec, m, f, ka, va);
    OGE_LAUNCH_CHECK(ctx);
    uint64_t *ks = ka;
    uint32_t *perm = va;
    rc = oge_radix_sort_pairs(ctx, ka, va, kb, vb, m, pack_key(vary_pri, vary_sec | low_bits(f.wh), f), &ks, &perm);
    if (rc) return rc;
    uint32_t *vfree = perm == va ? vb : va;
    uint64_t *kfree = ks == ka ? kb : ka;
    // ---- runs: the unsorted keys are dead, their buffers take the flags
    part.begin("compare_runs");
    uint32_t *head = (uint32_t *)sec;
    uint64_t *cum = pri;
    hipLaunchKernelGGL(k_cmp_flags, grid_for(m + 1), dim3(kT), 0, st, (const uint64_t *)ks, (const uint32_t *)perm,
                       (const uint32_t *)rec, m, m_a, A, B, head, cum);
    OGE_LAUNCH_CHECK(ctx);
    rc = oge_exclusive_scan_u32(ctx, head, head, m + 1);
    if (!rc) rc = oge_exclusive_scan_u64(ctx, cum, cum, m + 1);
    if (rc) return rc;
    uint32_t nruns = 0;
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&nruns, head + m, 4, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    ctx->counters["compare_runs"] = nruns;
    uint32_t *start = vfree;
    hipLaunchKernelGGL(k_cmp_starts, grid_for(m), dim3(kT), 0, st, (const uint32_t *)head, m, start);
    OGE_LAUNCH_CHECK(ctx);
    // a diff entry per run or per group of a hard run: at most one per item
    CmpDiff *diff = nullptr;
    if (want_diff) {
        diff = (CmpDiff *)ctx->ws("cmp_diff", m * sizeof(CmpDiff));
        if (!diff) return OGE_ERR_HIP;
    }
    uint32_t *hard = (uint32_t *)kfree;  // the sort's other key buffer: 2 words per run fit
    hipLaunchKernelGGL(k_cmp_runs, grid_for(nruns), dim3(kT), 0, st, (const uint32_t *)start, (uint64_t)nruns, m, m_a,
                       (const uint64_t *)cum, (const uint32_t *)perm, (const uint32_t *)rec, acc, diff, m, hard);
    OGE_LAUNCH_CHECK(ctx);
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&h, acc, sizeof h, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (h.n_hard) {
        hipLaunchKernelGGL(k_cmp_hard, dim3(h.n_hard), dim3(kT), 0, st, (const uint32_t *)hard, m_a, (const uint32_t *)perm,
                           (const uint32_t *)rec, A, B, acc, diff, m);
        OGE_LAUNCH_CHECK(ctx);
        OGE_HIP_TRY(ctx, hipMemcpyAsync(&h, acc, sizeof h, hipMemcpyDeviceToHost, st));
        OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    out->common = h.common;
    out->additions = h.adds;
    out->deletions = h.dels;
    out->hard_runs = h.n_hard;
    if (h.common + h.dels != out->n_ref || h.common + h.adds != out->n_other)
        return oge_fail(ctx, OGE_ERR_HIP, "compare: the counters do not add up to the item counts (internal error)");
    if (want_diff && h.n_diff) {
        const uint64_t nd = h.n_diff;
        if (nd > m) return oge_fail(ctx, OGE_ERR_HIP, "compare: more diff entries than items (internal error)");
        uint64_t *at = (uint64_t *)ctx->ws("cmp_diff_at", (nd + 1) * 8);
        if (!at) return OGE_ERR_HIP;
        hipLaunchKernelGGL(k_cmp_size, grid_for(nd + 1), dim3(kT), 0, st, (const CmpDiff *)diff, nd, A, B, at);
        OGE_LAUNCH_CHECK(ctx);
        rc = oge_exclusive_scan_u64(ctx, at, at, nd + 1);
        if (rc) return rc;
        uint64_t total = 0;
        OGE_HIP_TRY(ctx, hipMemcpyAsync(&total, at + nd, 8, hipMemcpyDeviceToHost, st));
        OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
        uint8_t *image = (uint8_t *)ctx->ws("cmp_image", total);
        if (!image) return OGE_ERR_HIP;
        hipLaunchKernelGGL(k_cmp_emit, grid_for(nd), dim3(kT), 0, st, (const CmpDiff *)diff, nd, A, B, (const uint64_t *)at, image);
        OGE_LAUNCH_CHECK(ctx);
        OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
        out->diff_entries = nd;
        *d_diff = image;
        *diff_bytes = total;
    }
    return OGE_OK;
}

}  // namespace

extern "C" {

int oge_compare_dev(oge_ctx *ctx, const uint8_t *d_recs_a, const uint64_t *d_off_a, uint64_t n_a, const uint8_t *d_recs_b,
                    const uint64_t *d_off_b, uint64_t n_b, int32_t n_ref, const oge_compare_region *region, uint32_t want,
                    int debug_hash_bits, oge_compare_result *result, const uint8_t **d_diff, uint64_t *diff_bytes) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!result || !region || (n_a && (!d_recs_a || !d_off_a)) || (n_b && (!d_recs_b || !d_off_b)))
        return oge_fail(ctx, OGE_ERR_ARG, "oge_compare_dev: null argument");
    if (want & ~(uint32_t)OGE_COMPARE_DIFF) return oge_fail(ctx, OGE_ERR_ARG, "compare: unknown request bits");
    if ((want & OGE_COMPARE_DIFF) && (!d_diff || !diff_bytes))
        return oge_fail(ctx, OGE_ERR_ARG, "compare: the diff requested without output pointers");
    if (n_ref < 0) return oge_fail(ctx, OGE_ERR_ARG, "compare: n_ref < 0");
    memset(result, 0, sizeof *result);
    if (d_diff) *d_diff = nullptr;
    if (diff_bytes) *diff_bytes = 0;
    OgeCall call(ctx, /*hold=*/false);
    return compare_impl(ctx, d_recs_a, d_off_a, n_a, d_recs_b, d_off_b, n_b, n_ref, region, want, debug_hash_bits, result, d_diff,
                        diff_bytes);
}

int oge_compare(oge_ctx *ctx, const uint8_t *recs_a, uint64_t rec_bytes_a, const uint64_t *rec_off_a, uint64_t n_a,
                const uint8_t *recs_b, uint64_t rec_bytes_b, const uint64_t *rec_off_b, uint64_t n_b, int32_t n_ref,
                const oge_compare_region *region, uint32_t want, int debug_hash_bits, oge_compare_result *result, uint8_t *diff_out,
                uint64_t cap, uint64_t *diff_bytes) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!result || !region || (n_a && (!recs_a || !rec_off_a)) || (n_b && (!recs_b || !rec_off_b)) ||
        ((want & OGE_COMPARE_DIFF) && !diff_bytes))
        return oge_fail(ctx, OGE_ERR_ARG, "oge_compare: null argument");
    (void)hipSetDevice(ctx->device);
    uint8_t *dra = (uint8_t *)ctx->ws("host_recs", rec_bytes_a + 16), *drb = (uint8_t *)ctx->ws("host_recs_b", rec_bytes_b + 16);
    uint64_t *doa = (uint64_t *)ctx->ws("host_off", (n_a + 1) * 8), *dob = (uint64_t *)ctx->ws("host_off_b", (n_b + 1) * 8);
    if (!dra || !drb || !doa || !dob) return OGE_ERR_HIP;
    if (rec_bytes_a) OGE_HIP_TRY(ctx, hipMemcpyAsync(dra, recs_a, rec_bytes_a, hipMemcpyHostToDevice, ctx->stream));
    if (rec_bytes_b) OGE_HIP_TRY(ctx, hipMemcpyAsync(drb, recs_b, rec_bytes_b, hipMemcpyHostToDevice, ctx->stream));
    OGE_HIP_TRY(ctx, hipMemsetAsync(dra + rec_bytes_a, 0, 16, ctx->stream));
    OGE_HIP_TRY(ctx, hipMemsetAsync(drb + rec_bytes_b, 0, 16, ctx->stream));
    if (n_a) OGE_HIP_TRY(ctx, hipMemcpyAsync(doa, rec_off_a, n_a * 8, hipMemcpyHostToDevice, ctx->stream));
    if (n_b) OGE_HIP_TRY(ctx, hipMemcpyAsync(dob, rec_off_b, n_b * 8, hipMemcpyHostToDevice, ctx->stream));
    const uint8_t *dd = nullptr;
    uint64_t nb = 0;
    const int rc = oge_compare_dev(ctx, dra, doa, n_a, drb, dob, n_b, n_ref, region, want, debug_hash_bits, result, &dd, &nb);
    if (rc) return rc;
    if (want & OGE_COMPARE_DIFF) {
        *diff_bytes = nb;
        if (nb > cap || (nb && !diff_out)) return oge_fail(ctx, OGE_ERR_LIMIT, "oge_compare: diff buffer too small");
        if (nb) {
            OGE_HIP_TRY(ctx, hipMemcpyAsync(diff_out, dd, nb, hipMemcpyDeviceToHost, ctx->stream));
            OGE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
    }
    return OGE_OK;
}

}  // extern "C"
