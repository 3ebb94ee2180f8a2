// dupsets.hip -- the pair duplicate SETS of a record set resident in HBM: per library the optical duplicates, over
// all libraries three set-size histograms (definitions in DESIGN.md section 27 and include/openge_hip.h; the model
// is tests/dupsets_model.py).  The ReadEnds and the pairs come from the dedup's own stages, called as
// oge_markdup_run calls them without sort keys (oge_markdup_prepare, oge_input_pass, oge_md_cand_frag,
// oge_md_join_build): no kernel of markdup.hip, records.hip or the sort is touched.
//
//   k_ds_valid / k_ds_pack   drop the pairs whose key is unconfirmed (bit 63 of lo), keep (lo, pair index)
//   two oge_radix_sort_pairs stable, on the varying bits of lo, then of hi & (2^48 - 1): equal keys are neighbours
//   k_ds_heads + scan        head flags -> set ids; k_ds_starts: where every set starts
//   k_ds_sets                one thread per set: all_sets, per-library pairs and sets (a set of one pair is done
//                            here: non_optical_sets[1]); the sizes of sets of two or more -> scan -> compacted members
//   k_ds_locate              one thread per sorted pair; a member of a set of two or more reads its read 1's FLAG,
//                            name and tags and stores {rg, tile, x, y}, the 0x40 / has-location / part bits and the
//                            library at its compacted position; the head of a set above the wave cap lists the set
//   k_ds_wave                one lane per compacted member; a wave takes the whole sets that start in its window of
//                            64 members: first those that also end in it, then the one that straddles its end
//   k_ds_block               one workgroup per listed set up to kBlockCap members, locations and labels in LDS
//   host                     a set above kBlockCap: union-find over the downloaded locations
// Sums are kept in block-private LDS tables and flushed with one 64-bit atomic per non-zero entry and workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "bam_layout.h"
#include "dev_util.h"
#include "markdup_stages.h"
#include "oge_ctx.h"
#include "records.h"
#include "rg_lookup.h"

namespace {

constexpr int kT = 256;
constexpr uint32_t kBins = OGE_DUP_SETS_BINS;
constexpr uint32_t kWaveCap = 64;
// a workgroup of k_ds_block keeps 16 + 4 + 4 bytes per member in LDS: 24 KiB at this cap, so six such workgroups
// fit the 160 KiB of a CU (the issue asks for at least two)
constexpr uint32_t kBlockCap = 1024;
constexpr int32_t kMaxLibs = 2048;  // the per-library LDS tables: at most 2 * 2048 u32 = 16 KiB (k_ds_sets)
constexpr uint64_t kKeyMask = (1ull << 48) - 1;
// fl[c]: bit 0 FLAG 0x40 of read 1, bit 1 has a location, bit 2 the part of a divided set, bits 8.. the library
constexpr uint32_t kFlFirst = 1, kFlHas = 2, kFlPart = 4;
enum { kHistAll = 0, kHistOptical = 1, kHistNonOptical = 2 };
enum { kCntWave = 0, kCntBlock = 1, kCntBig = 2 };

static_assert(sizeof(OgeDupSetsLib) == 32, "oge_dup_sets_lib is four u64");

__device__ __forceinline__ uint32_t bin_of(uint32_t v) { return v < kBins - 1 ? v : kBins - 1; }

// g[k] += s[k] for the non-zero entries of a block-private table; the whole workgroup calls it after a barrier
__device__ __forceinline__ void flush_table(const uint32_t *s, unsigned long long *g, uint32_t nk) {
    for (uint32_t k = threadIdx.x; k < nk; k += kT) {
        const uint32_t v = s[k];
        if (v) atomicAdd(&g[k], (unsigned long long)v);
    }
}

__global__ __launch_bounds__(kT) void k_ds_valid(const uint64_t *__restrict__ lo, uint32_t np, uint32_t *__restrict__ vf) {
    const uint32_t p = blockIdx.x * kT + threadIdx.x;
    if (p <= np) vf[p] = p < np && !(lo[p] >> 63);
}

__global__ __launch_bounds__(kT) void k_ds_pack(const uint64_t *__restrict__ lo, const uint32_t *__restrict__ vpos, uint32_t np,
                                                uint64_t *__restrict__ key, uint32_t *__restrict__ val) {
    const uint32_t p = blockIdx.x * kT + threadIdx.x;
    if (p >= np) return;
    const uint32_t q = vpos[p];
    if (vpos[p + 1] == q) return;
    key[q] = lo[p];
    val[q] = p;
}

__global__ __launch_bounds__(kT) void k_ds_hikeys(const uint64_t *__restrict__ hi, const uint32_t *__restrict__ val, uint32_t m,
                                                  uint64_t *__restrict__ key) {
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    if (i < m) key[i] = hi[val[i]] & kKeyMask;
}

// hf[i] = 1 where sorted pair i opens a set; hf[m] = 0
__global__ __launch_bounds__(kT) void k_ds_heads(const uint64_t *__restrict__ khi, const uint32_t *__restrict__ val,
                                                 const uint64_t *__restrict__ lo, uint32_t m, uint32_t *__restrict__ hf) {
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    if (i > m) return;
    hf[i] = i < m && (i == 0 || khi[i] != khi[i - 1] || lo[val[i]] != lo[val[i - 1]]);
}

// E = the exclusive scan of the head flags: sorted pair i is in set E[i + 1] - 1 and opens it when E[i + 1] != E[i]
__global__ __launch_bounds__(kT) void k_ds_starts(const uint32_t *__restrict__ E, uint32_t m, uint32_t *__restrict__ start) {
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    if (i > m) return;
    if (i == m) start[E[m]] = m;
    else if (E[i + 1] != E[i]) start[E[i]] = i;
}

// s_lib (dynamic): pairs[n_lib], sets[n_lib]
__global__ __launch_bounds__(kT) void k_ds_sets(const uint32_t *__restrict__ start, uint32_t n_sets, const uint32_t *__restrict__ val,
                                                const uint2 *__restrict__ idx, const RecMeta *__restrict__ meta, uint32_t n_lib,
                                                uint32_t *__restrict__ msz, unsigned long long *__restrict__ g_lib,
                                                unsigned long long *__restrict__ g_hist) {
    extern __shared__ uint32_t s_lib[];
    __shared__ uint32_t s_all[kBins];
    __shared__ uint32_t s_one;
    for (uint32_t k = threadIdx.x; k < kBins; k += kT) s_all[k] = 0;
    for (uint32_t k = threadIdx.x; k < 2 * n_lib; k += kT) s_lib[k] = 0;
    if (threadIdx.x == 0) s_one = 0;
    __syncthreads();
    for (uint64_t s = (uint64_t)blockIdx.x * kT + threadIdx.x; s <= n_sets; s += (uint64_t)gridDim.x * kT) {
        if (s == n_sets) { msz[s] = 0; break; }
        const uint32_t a = start[s], sz = start[s + 1] - a;
        uint32_t lib = (uint32_t)((meta[idx[val[a]].x].m >> 16) & 0xFFFF);
        if (lib >= n_lib) lib = n_lib - 1;  // (refused on the host: the table's ids are all below n_lib)
        atomicAdd(&s_all[bin_of(sz)], 1u);
        atomicAdd(&s_lib[lib], sz);
        atomicAdd(&s_lib[n_lib + lib], 1u);
        if (sz == 1) atomicAdd(&s_one, 1u);
        msz[s] = sz >= 2 ? sz : 0;
    }
    __syncthreads();
    flush_table(s_all, g_hist + kHistAll * kBins, kBins);
    for (uint32_t k = threadIdx.x; k < 2 * n_lib; k += kT) {  // pairs, sets are fields 0, 1 of oge_dup_sets_lib
        const uint32_t v = s_lib[k];
        if (v) atomicAdd(&g_lib[(k % n_lib) * 4 + k / n_lib], (unsigned long long)v);
    }
    if (threadIdx.x == 0 && s_one) atomicAdd(&g_hist[kHistNonOptical * kBins + 1], (unsigned long long)s_one);
}

// A number: an optional '-', then decimal digits up to the first other byte; no digit gives 0; held in int32.
__device__ __forceinline__ int32_t ds_number(const uint8_t *p, const uint8_t *e) {
    bool neg = false;
    if (p < e && *p == '-') { neg = true; ++p; }
    uint32_t v = 0;
    while (p < e && *p >= '0' && *p <= '9') v = v * 10u + (uint32_t)(*p++ - '0');
    return neg ? (int32_t)(0u - v) : (int32_t)v;
}

// tile, x, y of a name of exactly 5 or exactly 7 ':'-separated fields: the last three
__device__ __forceinline__ bool ds_location(const uint8_t *nm, uint32_t len, int32_t *tile, int32_t *x, int32_t *y) {
    uint32_t colons = 0, c0 = 0, c1 = 0, c2 = 0;  // the positions behind the last three ':'
    for (uint32_t k = 0; k < len; ++k)
        if (nm[k] == ':') { ++colons; c0 = c1; c1 = c2; c2 = k + 1; }
    if (colons != 4 && colons != 6) return false;
    *tile = ds_number(nm + c0, nm + len);
    *x = ds_number(nm + c1, nm + len);
    *y = ds_number(nm + c2, nm + len);
    return true;
}

// s_lib (dynamic): located[n_lib]
__global__ __launch_bounds__(kT) void k_ds_locate(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ off, const RecMeta *__restrict__ meta,
                                                  const uint2 *__restrict__ idx, const uint32_t *__restrict__ val, const uint32_t *__restrict__ E,
                                                  const uint32_t *__restrict__ start, const uint32_t *__restrict__ mo, uint32_t m, OgeRgTable rg,
                                                  uint32_t n_lib, int4 *__restrict__ loc, uint32_t *__restrict__ fl, uint32_t *__restrict__ cst,
                                                  uint32_t *__restrict__ csz, uint32_t *__restrict__ big, unsigned int *__restrict__ cnt,
                                                  unsigned long long *__restrict__ g_lib) {
    extern __shared__ uint32_t s_lib[];
    for (uint32_t k = threadIdx.x; k < n_lib; k += kT) s_lib[k] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * kT + threadIdx.x; i < m; i += (uint64_t)gridDim.x * kT) {
        const uint32_t s = E[i + 1] - 1, a = start[s], sz = start[s + 1] - a;
        if (sz < 2) continue;
        const uint32_t c0 = mo[s], c = c0 + ((uint32_t)i - a);
        const uint2 ii = idx[val[i]];
        const uint64_t m1 = meta[ii.x].m, m2 = meta[ii.y].m;
        uint32_t lib = (uint32_t)((m1 >> 16) & 0xFFFF);
        if (lib >= n_lib) lib = n_lib - 1;
        const bool divided = ((m1 ^ m2) & OGE_M_REV) != 0;  // FR or RF
        const uint8_t *r = recs + off[ii.x];
        const uint32_t bs = oge_ldu32(r + OGE_OFF_BLOCK);
        const bool sane = bs >= 32 && bs <= OGE_MAX_BLOCK_SIZE;
        const uint32_t flag = oge_ldu32(r + OGE_OFF_NCIGAR) >> 16;
        uint32_t f = (flag & OGE_F_READ1) ? kFlFirst : 0;
        if (divided && (flag & OGE_F_READ1)) f |= kFlPart;
        int4 L = make_int4(-1, 0, 0, 0);
        if (sane) {
            uint32_t len = oge_ldu32(r + OGE_OFF_LNAME) & 0xFF;
            len = min(len, bs - 32);  // the name's bytes inside the record
            const uint8_t *nm = r + OGE_OFF_NAME;
            uint32_t e = 0;
            while (e < len && nm[e]) ++e;
            if (ds_location(nm, e, &L.y, &L.z, &L.w)) {
                f |= kFlHas;
                L.x = oge_rg_index(r, bs, rg);
                atomicAdd(&s_lib[lib], 1u);
            }
        }
        loc[c] = L;
        fl[c] = f | (lib << 8);
        cst[c] = c0;
        csz[c] = sz;
        if (c == c0 && sz > kWaveCap) big[atomicAdd(&cnt[kCntBig], 1u)] = c0;  // one per set above the wave cap
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < n_lib; k += kT) {
        const uint32_t v = s_lib[k];
        if (v) atomicAdd(&g_lib[k * 4 + 2], (unsigned long long)v);
    }
}

__device__ __forceinline__ bool ds_close(const int4 &a, uint32_t fa, const int4 &b, uint32_t fb, int64_t D) {
    if (!(fa & fb & kFlHas) || ((fa ^ fb) & kFlPart) || a.x != b.x || a.y != b.y) return false;
    const int64_t dx = (int64_t)a.z - b.z, dy = (int64_t)a.w - b.w;
    return dx <= D && -dx <= D && dy <= D && -dy <= D;
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
    return ((uint64_t)(uint32_t)__shfl((int)(v >> 32), src, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)v, src, 64);
}

// The sets a round of the wave holds: lane `act` has compacted member c of the set that starts at st (size sz).
// Every member of such a set is in the wave.  Called by the whole wave.  s_lib: optical[n_lib].
__device__ __forceinline__ void ds_wave_round(bool act, uint32_t c, uint32_t st, uint32_t sz, const int4 *__restrict__ loc,
                                              const uint32_t *__restrict__ fl, int64_t D, uint32_t lane, uint32_t *s_lib, uint32_t *s_non,
                                              uint32_t *s_os, uint32_t *s_cnt) {
    const uint64_t am = __ballot(act);
    if (!am) return;  // wave-uniform
    int4 L = make_int4(0, 0, 0, 0);
    uint32_t f = 0;
    if (act) { L = loc[c]; f = fl[c]; }
    const uint32_t key = act ? st : 0xFFFFFFFFu;
    uint64_t adj = 0, smask = 0;
    for (uint64_t mm = am; mm; mm &= mm - 1) {  // wave-uniform: every active lane's location goes round
        const int j = __ffsll((long long)mm) - 1;
        int4 Lj;
        Lj.x = __shfl(L.x, j, 64);
        Lj.y = __shfl(L.y, j, 64);
        Lj.z = __shfl(L.z, j, 64);
        Lj.w = __shfl(L.w, j, 64);
        const uint32_t fj = (uint32_t)__shfl((int)f, j, 64), kj = (uint32_t)__shfl((int)key, j, 64);
        const bool same = act && kj == key;
        if (same) smask |= 1ull << j;
        if (same && ds_close(L, f, Lj, fj, D)) adj |= 1ull << j;
    }
    const bool has = act && (f & kFlHas);
    uint64_t reach = adj | (1ull << lane);
    if (__any(has && (adj & ~(1ull << lane)))) {  // some pair is close to another: close the masks under union
        bool changed;
        do {  // wave-uniform fixpoint
            const uint64_t before = reach;
            for (uint64_t mm = am; mm; mm &= mm - 1) {
                const int j = __ffsll((long long)mm) - 1;
                const uint64_t rj = shfl64(reach, j);
                if ((reach >> j) & 1) reach |= rj;
            }
            changed = reach != before;
        } while (__any(changed));
    }
    const bool root = has && (uint32_t)(__ffsll((long long)reach) - 1) == lane;
    const uint64_t bl = __ballot(has), br = __ballot(root);
    if (act && c == st) {  // the head lane of every set
        const uint32_t located = (uint32_t)__popcll(bl & smask), comps = (uint32_t)__popcll(br & smask), o = located - comps;
        atomicAdd(&s_non[bin_of(sz - o)], 1u);
        if (o) {
            atomicAdd(&s_os[bin_of(o + 1)], 1u);
            atomicAdd(&s_lib[f >> 8], o);
        }
        atomicAdd(s_cnt, 1u);
    }
}

__global__ __launch_bounds__(kT) void k_ds_wave(const int4 *__restrict__ loc, const uint32_t *__restrict__ fl, const uint32_t *__restrict__ cst,
                                                const uint32_t *__restrict__ csz, uint32_t M2, int64_t D, uint32_t n_lib,
                                                unsigned long long *__restrict__ g_lib, unsigned long long *__restrict__ g_hist,
                                                unsigned int *__restrict__ cnt) {
    extern __shared__ uint32_t s_lib[];
    __shared__ uint32_t s_non[kBins], s_os[kBins];
    __shared__ uint32_t s_cnt;
    for (uint32_t k = threadIdx.x; k < kBins; k += kT) s_non[k] = 0, s_os[k] = 0;
    for (uint32_t k = threadIdx.x; k < n_lib; k += kT) s_lib[k] = 0;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, nwin = (M2 + 63) / 64;
    for (uint64_t w = (uint64_t)blockIdx.x * (kT / 64) + (threadIdx.x >> 6); w < nwin; w += (uint64_t)gridDim.x * (kT / 64)) {  // wave-uniform
        const uint32_t base = (uint32_t)w * 64, c = base + lane;
        uint32_t st = 0, sz = 0;
        if (c < M2) { st = cst[c]; sz = csz[c]; }
        const bool mine = c < M2 && st >= base && sz <= kWaveCap;  // the set starts in this wave's window
        const bool inside = mine && st + sz <= base + 64;
        ds_wave_round(inside, c, st, sz, loc, fl, D, lane, s_lib, s_non, s_os, &s_cnt);
        // the one set that starts in the window and ends behind it: taken whole, from its first member
        const uint64_t sm = __ballot(mine && !inside);
        if (sm) {
            const int j = __ffsll((long long)sm) - 1;
            const uint32_t st2 = (uint32_t)__shfl((int)st, j, 64), sz2 = (uint32_t)__shfl((int)sz, j, 64);
            ds_wave_round(lane < sz2, st2 + lane, st2, sz2, loc, fl, D, lane, s_lib, s_non, s_os, &s_cnt);
        }
    }
    __syncthreads();
    flush_table(s_non, g_hist + kHistNonOptical * kBins, kBins);
    flush_table(s_os, g_hist + kHistOptical * kBins, kBins);
    for (uint32_t k = threadIdx.x; k < n_lib; k += kT) {
        const uint32_t v = s_lib[k];
        if (v) atomicAdd(&g_lib[k * 4 + 3], (unsigned long long)v);
    }
    if (threadIdx.x == 0 && s_cnt) atomicAdd(&cnt[kCntWave], s_cnt);
}

// one workgroup per listed set of at most kBlockCap members (larger ones are the host's)
__global__ __launch_bounds__(kT) void k_ds_block(const int4 *__restrict__ loc, const uint32_t *__restrict__ fl, const uint32_t *__restrict__ csz,
                                                 const uint32_t *__restrict__ big, int64_t D, unsigned long long *__restrict__ g_lib,
                                                 unsigned long long *__restrict__ g_hist, unsigned int *__restrict__ cnt) {
    __shared__ int4 s_loc[kBlockCap];
    __shared__ uint32_t s_fl[kBlockCap], s_lab[kBlockCap];
    __shared__ uint32_t s_changed, s_located, s_comps;
    const uint32_t st = big[blockIdx.x], sz = csz[st];
    if (sz > kBlockCap) return;  // block-uniform
    for (uint32_t i = threadIdx.x; i < sz; i += kT) {
        s_loc[i] = loc[st + i];
        s_fl[i] = fl[st + i];
        s_lab[i] = i;
    }
    if (threadIdx.x == 0) s_located = 0, s_comps = 0;
    for (;;) {  // block-uniform
        __syncthreads();
        if (threadIdx.x == 0) s_changed = 0;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < sz; i += kT) {  // a sweep: every label down to the smallest among the close ones
            const uint32_t fi = s_fl[i];
            if (!(fi & kFlHas)) continue;
            const int4 Li = s_loc[i];
            const uint32_t li = s_lab[i];
            uint32_t best = li;
            for (uint32_t j = 0; j < sz; ++j)
                if (ds_close(Li, fi, s_loc[j], s_fl[j], D)) best = min(best, s_lab[j]);
            if (best < li) {
                atomicMin(&s_lab[i], best);
                s_changed = 1;
            }
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < sz; i += kT) {  // pointer jumping: labels are members of the same component
            uint32_t l = s_lab[i], ll = s_lab[l];
            while (ll < l) { l = ll; ll = s_lab[l]; }
            atomicMin(&s_lab[i], l);
        }
        __syncthreads();
        if (!s_changed) break;
    }
    uint32_t located = 0, comps = 0;
    for (uint32_t i = threadIdx.x; i < sz; i += kT)
        if (s_fl[i] & kFlHas) { ++located; comps += s_lab[i] == i; }
    located = oge_wave_sum(located);
    comps = oge_wave_sum(comps);
    if ((threadIdx.x & 63) == 0) { atomicAdd(&s_located, located); atomicAdd(&s_comps, comps); }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t o = s_located - s_comps;
        atomicAdd(&g_hist[kHistNonOptical * kBins + bin_of(sz - o)], 1ull);
        if (o) {
            atomicAdd(&g_hist[kHistOptical * kBins + bin_of(o + 1)], 1ull);
            atomicAdd(&g_lib[(s_fl[0] >> 8) * 4 + 3], (unsigned long long)o);
        }
        atomicAdd(&cnt[kCntBlock], 1u);
    }
}

// The optical duplicates of one set on the host: union-find over the members, the candidates of each found in a
// window of a list sorted by (part, read group, tile, x).
uint32_t host_set_optical(const int4 *loc, const uint32_t *fl, uint32_t sz, int64_t D) {
    std::vector<uint32_t> ord;
    for (uint32_t i = 0; i < sz; ++i)
        if (fl[i] & kFlHas) ord.push_back(i);
    auto group = [&](uint32_t i) { return std::make_tuple(fl[i] & kFlPart, loc[i].x, loc[i].y); };
    std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) {
        return group(a) != group(b) ? group(a) < group(b) : loc[a].z < loc[b].z;
    });
    std::vector<uint32_t> par(sz);
    std::iota(par.begin(), par.end(), 0u);
    auto find = [&](uint32_t v) {
        while (par[v] != v) v = par[v] = par[par[v]];
        return v;
    };
    uint32_t comps = (uint32_t)ord.size();
    for (size_t a = 0; a < ord.size(); ++a) {
        const uint32_t i = ord[a];
        for (size_t b = a + 1; b < ord.size(); ++b) {
            const uint32_t j = ord[b];
            if (group(i) != group(j) || (int64_t)loc[j].z - loc[i].z > D) break;
            const int64_t dy = (int64_t)loc[j].w - loc[i].w;
            if (dy > D || -dy > D) continue;
            const uint32_t ri = find(i), rj = find(j);
            if (ri != rj) { par[ri] = rj; --comps; }
        }
    }
    return (uint32_t)ord.size() - comps;
}

}  // namespace

int oge_dup_sets_impl(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, const oge_markdup_opts *opts_in, int64_t distance,
                      int32_t n_lib, OgeDupSetsLib *out_per_lib, uint64_t *hist) {
    if (n_lib < 1) return oge_fail(ctx, OGE_ERR_ARG, "dup_sets: n_lib < 1");
    if (n_lib > kMaxLibs) return oge_fail(ctx, OGE_ERR_LIMIT, "dup_sets: more than 2048 libraries");
    if (distance < 0 || distance > 0x7fffffffll) return oge_fail(ctx, OGE_ERR_ARG, "dup_sets: distance outside [0, 2^31 - 1]");
    if (n >= (1ull << 31)) return oge_fail(ctx, OGE_ERR_LIMIT, "dup_sets: 2^31 records or more");
    if (n && (!d_recs || !d_off)) return oge_fail(ctx, OGE_ERR_ARG, "dup_sets: null argument");
    if (int rc = oge_rg_table_check(ctx, opts_in, "dup_sets", n_lib)) return rc;
    if (opts_in->split_chains > 1 || opts_in->compat_nonverbose_index)
        return oge_fail(ctx, OGE_ERR_ARG, "dup_sets: split chains and the non-verbose index are not supported");
    oge_markdup_opts o = *opts_in;  // the plain stages: no test knobs
    o.debug_sort_groups = 0;
    o.debug_hash_bits = 0;
    o.remove_duplicates = 0;
    const oge_markdup_opts *opts = &o;
    memset(out_per_lib, 0, (size_t)n_lib * sizeof *out_per_lib);
    memset(hist, 0, 3 * kBins * sizeof(uint64_t));
    ctx->counters["dupsets_wave_cap"] = kWaveCap;
    ctx->counters["dupsets_block_cap"] = kBlockCap;
    ctx->counters["dupsets_wave_sets"] = 0;
    ctx->counters["dupsets_block_sets"] = 0;
    ctx->counters["dupsets_host_sets"] = 0;
    if (!n) return OGE_OK;
    hipStream_t st = ctx->stream;
    const uint32_t nl = (uint32_t)n_lib;
    const size_t out_words = (size_t)nl * 4 + 3 * kBins;
    unsigned long long *g_out = (unsigned long long *)ctx->ws("ds_out", out_words * 8);
    unsigned int *cnt = (unsigned int *)ctx->ws("ds_cnt", 16);
    if (!g_out || !cnt) return OGE_ERR_HIP;
    unsigned long long *g_lib = g_out, *g_hist = g_out + (size_t)nl * 4;

    OgeStage whole(ctx, "dup_sets");
    OGE_HIP_TRY(ctx, hipMemsetAsync(g_out, 0, out_words * 8, st));
    OGE_HIP_TRY(ctx, hipMemsetAsync(cnt, 0, 16, st));
    // ---- ReadEnds and pairs: the dedup's stages, as oge_markdup_run calls them without sort keys
    OgeStage stage(ctx, "ds_readends");
    RecMeta *meta;
    OgeRgTable rg;
    int rc = oge_markdup_prepare(ctx, opts, n, "md_meta", &meta, &rg);
    if (rc) return rc;
    OgePassArgs a = {};
    a.recs = d_recs;
    a.off = d_off;
    a.n = n;
    a.meta = meta;
    a.rg = rg;
    a.n_ref = opts->n_ref;
    if ((rc = oge_input_pass(ctx, a))) return rc;
    stage.begin("ds_join");
    OgeMdFrags F;
    OgeMdPairs P;
    if ((rc = oge_md_cand_frag(ctx, opts, meta, n, false, &F))) return rc;
    if ((rc = oge_md_join_build(ctx, opts, d_recs, meta, n, F, &P))) return rc;
    stage.end();
    const uint32_t np = P.np;
    if (!np) return OGE_OK;

    // ---- grouping: exact, by the whole key
    stage.begin("ds_group");
    uint32_t *vf = (uint32_t *)ctx->scratch("ds_vf", ((uint64_t)np + 1) * 4);
    uint64_t *kA = (uint64_t *)ctx->scratch("ds_ka", ((uint64_t)np + 1) * 8), *kB = (uint64_t *)ctx->scratch("ds_kb", ((uint64_t)np + 1) * 8);
    uint32_t *vA = (uint32_t *)ctx->scratch("ds_va", ((uint64_t)np + 1) * 4), *vB = (uint32_t *)ctx->scratch("ds_vb", ((uint64_t)np + 1) * 4);
    if (!vf || !kA || !kB || !vA || !vB) return OGE_ERR_HIP;
    hipLaunchKernelGGL(k_ds_valid, dim3(oge_ceil_div((uint64_t)np + 1, kT)), dim3(kT), 0, st, (const uint64_t *)P.lo, np, vf);
    OGE_LAUNCH_CHECK(ctx);
    if ((rc = oge_exclusive_scan_u32(ctx, vf, vf, (uint64_t)np + 1))) return rc;
    uint32_t m = 0;
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&m, vf + np, 4, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (!m) return OGE_OK;
    hipLaunchKernelGGL(k_ds_pack, dim3(oge_ceil_div(np, kT)), dim3(kT), 0, st, (const uint64_t *)P.lo, (const uint32_t *)vf, np, kA, vA);
    OGE_LAUNCH_CHECK(ctx);
    uint64_t vo = 0, va = 0;
    if ((rc = oge_reduce_or_and_u64(ctx, kA, m, ~0ull, &vo, &va))) return rc;
    uint64_t *k1;
    uint32_t *v1;
    if ((rc = oge_radix_sort_pairs(ctx, kA, vA, kB, vB, m, vo ^ va, &k1, &v1))) return rc;
    uint64_t *k1o = k1 == kA ? kB : kA;  // the pair of buffers the first sort left free
    uint32_t *v1o = v1 == vA ? vB : vA;
    hipLaunchKernelGGL(k_ds_hikeys, dim3(oge_ceil_div(m, kT)), dim3(kT), 0, st, (const uint64_t *)P.hi, (const uint32_t *)v1, m, k1o);
    OGE_LAUNCH_CHECK(ctx);
    if ((rc = oge_reduce_or_and_u64(ctx, k1o, m, ~0ull, &vo, &va))) return rc;
    uint64_t *k2;
    uint32_t *v2;
    if ((rc = oge_radix_sort_pairs(ctx, k1o, v1, k1, v1o, m, vo ^ va, &k2, &v2))) return rc;
    uint32_t *E = vf;  // (the valid flags are done with; m + 1 <= np + 1)
    hipLaunchKernelGGL(k_ds_heads, dim3(oge_ceil_div((uint64_t)m + 1, kT)), dim3(kT), 0, st, (const uint64_t *)k2, (const uint32_t *)v2,
                       (const uint64_t *)P.lo, m, E);
    OGE_LAUNCH_CHECK(ctx);
    if ((rc = oge_exclusive_scan_u32(ctx, E, E, (uint64_t)m + 1))) return rc;
    uint32_t n_sets = 0;
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&n_sets, E + m, 4, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    uint32_t *start = (uint32_t *)ctx->scratch("ds_start", ((uint64_t)n_sets + 1) * 4);
    uint32_t *mo = (uint32_t *)ctx->scratch("ds_mo", ((uint64_t)n_sets + 1) * 4);
    if (!start || !mo) return OGE_ERR_HIP;
    hipLaunchKernelGGL(k_ds_starts, dim3(oge_ceil_div((uint64_t)m + 1, kT)), dim3(kT), 0, st, (const uint32_t *)E, m, start);
    OGE_LAUNCH_CHECK(ctx);
    const uint32_t cap_blocks = (uint32_t)ctx->cu_count() * 8;
    hipLaunchKernelGGL(k_ds_sets, dim3(std::min(oge_ceil_div((uint64_t)n_sets + 1, kT), cap_blocks)), dim3(kT), 2 * nl * 4, st,
                       (const uint32_t *)start, n_sets, (const uint32_t *)v2, (const uint2 *)P.idx, (const RecMeta *)meta, nl, mo, g_lib, g_hist);
    OGE_LAUNCH_CHECK(ctx);
    if ((rc = oge_exclusive_scan_u32(ctx, mo, mo, (uint64_t)n_sets + 1))) return rc;
    uint32_t M2 = 0;
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&M2, mo + n_sets, 4, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    stage.end();

    std::vector<uint32_t> h_big;
    int4 *loc = nullptr;
    uint32_t *fl = nullptr, *csz = nullptr;
    unsigned int h_cnt[4] = {0, 0, 0, 0};
    if (M2) {
        // ---- locate: the members of sets of two or more, compacted
        stage.begin("ds_locate");
        loc = (int4 *)ctx->scratch("ds_loc", (uint64_t)M2 * sizeof(int4));
        fl = (uint32_t *)ctx->scratch("ds_fl", (uint64_t)M2 * 4);
        uint32_t *cst = (uint32_t *)ctx->scratch("ds_cst", (uint64_t)M2 * 4);
        csz = (uint32_t *)ctx->scratch("ds_csz", (uint64_t)M2 * 4);
        uint32_t *big = (uint32_t *)ctx->scratch("ds_big", ((uint64_t)M2 / (kWaveCap + 1) + 1) * 4);
        if (!loc || !fl || !cst || !csz || !big) return OGE_ERR_HIP;
        hipLaunchKernelGGL(k_ds_locate, dim3(std::min(oge_ceil_div(m, kT), cap_blocks)), dim3(kT), nl * 4, st, d_recs, d_off, (const RecMeta *)meta,
                           (const uint2 *)P.idx, (const uint32_t *)v2, (const uint32_t *)E, (const uint32_t *)start, (const uint32_t *)mo, m, rg, nl,
                           loc, fl, cst, csz, big, cnt, g_lib);
        OGE_LAUNCH_CHECK(ctx);
        // ---- components
        stage.begin("ds_components");
        hipLaunchKernelGGL(k_ds_wave, dim3(std::min(oge_ceil_div(oge_ceil_div(M2, 64), kT / 64), cap_blocks)), dim3(kT), nl * 4, st,
                           (const int4 *)loc, (const uint32_t *)fl, (const uint32_t *)cst, (const uint32_t *)csz, M2, distance, nl, g_lib, g_hist, cnt);
        OGE_LAUNCH_CHECK(ctx);
        OGE_HIP_TRY(ctx, hipMemcpyAsync(h_cnt, cnt, 16, hipMemcpyDeviceToHost, st));
        OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
        const uint32_t nbig = h_cnt[kCntBig];
        if (nbig) {
            hipLaunchKernelGGL(k_ds_block, dim3(nbig), dim3(kT), 0, st, (const int4 *)loc, (const uint32_t *)fl, (const uint32_t *)csz,
                               (const uint32_t *)big, distance, g_lib, g_hist, cnt);
            OGE_LAUNCH_CHECK(ctx);
            h_big.resize(nbig);
            OGE_HIP_TRY(ctx, hipMemcpyAsync(h_big.data(), big, (size_t)nbig * 4, hipMemcpyDeviceToHost, st));
            OGE_HIP_TRY(ctx, hipMemcpyAsync(h_cnt, cnt, 16, hipMemcpyDeviceToHost, st));
            OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
        }
        stage.end();
    }
    whole.end();
    std::vector<unsigned long long> h_out(out_words);
    OGE_HIP_TRY(ctx, hipMemcpyAsync(h_out.data(), g_out, out_words * 8, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    memcpy(out_per_lib, h_out.data(), (size_t)nl * 32);
    memcpy(hist, h_out.data() + (size_t)nl * 4, 3 * kBins * 8);
    // ---- the host tier: sets above the block cap
    uint64_t host_sets = 0;
    for (uint32_t st0 : h_big) {
        uint32_t sz = 0;
        OGE_HIP_TRY(ctx, hipMemcpy(&sz, csz + st0, 4, hipMemcpyDeviceToHost));
        if (sz <= kBlockCap) continue;
        std::vector<int4> hl(sz);
        std::vector<uint32_t> hf(sz);
        OGE_HIP_TRY(ctx, hipMemcpy(hl.data(), loc + st0, (size_t)sz * sizeof(int4), hipMemcpyDeviceToHost));
        OGE_HIP_TRY(ctx, hipMemcpy(hf.data(), fl + st0, (size_t)sz * 4, hipMemcpyDeviceToHost));
        const uint32_t ov = host_set_optical(hl.data(), hf.data(), sz, distance);
        ++hist[kHistNonOptical * kBins + std::min(sz - ov, kBins - 1)];
        if (ov) {
            ++hist[kHistOptical * kBins + std::min(ov + 1, kBins - 1)];
            out_per_lib[hf[0] >> 8].optical += ov;
        }
        ++host_sets;
    }
    ctx->counters["dupsets_wave_sets"] = h_cnt[kCntWave];
    ctx->counters["dupsets_block_sets"] = h_cnt[kCntBlock];
    ctx->counters["dupsets_host_sets"] = host_sets;
    return OGE_OK;
}

extern "C" {

int oge_dup_sets_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, const oge_markdup_opts *opts, int64_t distance,
                     int32_t n_lib, OgeDupSetsLib *out_per_lib, uint64_t *hist) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!opts || !out_per_lib || !hist) return oge_fail(ctx, OGE_ERR_ARG, "oge_dup_sets_dev: null argument");
    OgeCall call(ctx, /*hold=*/false);
    return oge_dup_sets_impl(ctx, d_recs, d_off, n, opts, distance, n_lib, out_per_lib, hist);
}

int oge_dup_sets(oge_ctx *ctx, const uint8_t *recs, uint64_t rec_bytes, const uint64_t *rec_off, uint64_t n, const oge_markdup_opts *opts,
                 int64_t distance, int32_t n_lib, OgeDupSetsLib *out_per_lib, uint64_t *hist) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!opts || !out_per_lib || !hist || (n && (!recs || !rec_off))) return oge_fail(ctx, OGE_ERR_ARG, "oge_dup_sets: null argument");
    (void)hipSetDevice(ctx->device);
    uint8_t *dr = (uint8_t *)ctx->ws("host_recs", rec_bytes + 16);
    uint64_t *dof = (uint64_t *)ctx->ws("host_off", (n + 1) * 8);
    if (!dr || !dof) return OGE_ERR_HIP;
    if (rec_bytes) OGE_HIP_TRY(ctx, hipMemcpyAsync(dr, recs, rec_bytes, hipMemcpyHostToDevice, ctx->stream));
    OGE_HIP_TRY(ctx, hipMemsetAsync(dr + rec_bytes, 0, 16, ctx->stream));
    if (n) OGE_HIP_TRY(ctx, hipMemcpyAsync(dof, rec_off, n * 8, hipMemcpyHostToDevice, ctx->stream));
    return oge_dup_sets_dev(ctx, dr, dof, n, opts, distance, n_lib, out_per_lib, hist);
}

}  // extern "C"
