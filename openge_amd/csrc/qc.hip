// qc.hip -- `openge stats`, `count` and `coverage` as reductions over the record cores resident in HBM
// (the reference's algorithms/statistics.cpp and algorithms/measure_coverage.cpp; definitions in
// DESIGN.md section 20 and include/openge_hip.h).  All sums are integer: results do not depend on order.
//
//   stats      k_qc_stats      every wave walks kWaveRecs consecutive records, 64 at a time: the flag counters by
//                              ballot + popcount into wave-uniform registers, the insert count and sum per lane,
//                              l_seq into a block-private LDS table (lengths below kLenTab) or a count of the
//                              larger ones; per block one 64-bit atomic per counter and per non-empty length
//              sorted          the same walk carries the last two considered (refID, pos) keys in registers and
//                              resolves every triple that lies inside the wave's range; the wave stores its first
//                              two and last two keys, and k_qc_stitch (one workgroup) folds them in file order and
//                              checks the two first keys of every range -- no per-record scratch
//   lengths    k_qc_len_small  compacts the table; lengths >= kLenTab (k_qc_biglen) are appended to a list of their
//                              own, radix-sorted and run-length encoded behind it: any l_seq is right, whatever the
//                              table size
//   inserts    k_qc_sel_hist / k_qc_sel_pick  most-significant-digit radix select of the two middle order
//                              statistics of |tlen|: three histogram passes (11, 11 and 10 bits), no value array
//   coverage   k_qc_cov        a workgroup takes kCovTile consecutive records; when the bins they touch span at
//                              most kCovWin entries of the bin array it accumulates in LDS and flushes every
//                              non-zero bin with one global atomic, else it adds to global memory directly; a read
//                              over more than 64 bins is spread over the lanes of its wave
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "bam_layout.h"
#include "dev_util.h"
#include "oge_ctx.h"

namespace {

constexpr int kT = 256;
constexpr int kWaves = kT / 64;
constexpr int kIter = 16;                      // 64-record steps per wave
constexpr int kWaveRecs = 64 * kIter;          // consecutive records of one wave
constexpr int kBlockRecs = kWaves * kWaveRecs;
constexpr uint32_t kLenTab = 4096;             // l_seq below this goes through the LDS table
constexpr int kStitchT = 1024;
constexpr int kSelBins = 2048;                 // 11-bit digits (the last pass uses 10)
constexpr int kCovPer = 4;
constexpr int kCovTile = kT * kCovPer;         // records of one coverage tile
constexpr uint32_t kCovWin = 4096;             // bins of the LDS window
constexpr int kNumCounters = 12;
constexpr unsigned long long kNone = ~0ull;

// device accumulators of one stats call
struct QcAcc {
    unsigned long long c[kNumCounters];  // the order of oge_bam_stats
    unsigned long long n_insert, insert_sum, n_big, unsorted;
};

// the considered (refID != -1 and pos != -1) records of one wave's range: how many (saturating at 2), the
// first two and the last two keys (r[2] / p[2] the one before the last, r[3] / p[3] the last)
struct QcEdge {
    int32_t cnt;
    int32_t r[4], p[4];
};

struct QcSel {  // radix select of the lower and upper middle: rank inside the current bucket, bits chosen so far
    unsigned long long rank[2];
    uint32_t prefix[2];
};

struct CovOut {
    unsigned long long skipped, badref, overflow;
};

struct Core {
    int32_t refid, pos, lseq, tlen;
    uint32_t flag;
};

__device__ __forceinline__ Core load_core(const uint8_t *r) {
    Core c;
    c.refid = (int32_t)oge_ldu32(r + OGE_OFF_REFID);
    c.pos = (int32_t)oge_ldu32(r + OGE_OFF_POS);
    c.flag = oge_ldu32(r + OGE_OFF_NCIGAR) >> 16;
    c.lseq = (int32_t)oge_ldu32(r + OGE_OFF_LSEQ);
    c.tlen = (int32_t)oge_ldu32(r + OGE_OFF_TLEN);
    return c;
}

// Statistics::runInternal's order test in local form: the record (rid, pos) after the considered records
// (r2, .) and (r1, p1).  The first considered record of a refID run does not leave its position behind
// (the reference resets last_position to -1 there).
__device__ __forceinline__ bool out_of_order(int32_t r2, int32_t r1, int32_t p1, int32_t rid, int32_t pos) {
    if (rid < r1) return true;
    if (rid > r1) return false;
    return pos < (r1 == r2 ? p1 : -1);
}

// h[key] += 1 for every lane with `act`, called by the whole wave: the two most common keys of the wave are
// added once with their lane counts (reads of one length, insert sizes of one bucket), the rest one by one
__device__ __forceinline__ void lds_hist_add(uint32_t *h, uint32_t key, bool act) {
    const uint32_t lane = threadIdx.x & 63;
    for (int r = 0; r < 2; ++r) {
        const uint64_t m = __ballot(act);
        if (!m) return;
        const int ld = __ffsll((long long)m) - 1;
        const uint32_t k = (uint32_t)__shfl((int)key, ld, 64);
        const uint64_t same = __ballot(act && key == k);
        if ((int)lane == ld) atomicAdd(&h[k], (uint32_t)__popcll(same));
        if (key == k) act = false;
    }
    if (act) atomicAdd(&h[key], 1u);
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

__device__ __forceinline__ bool insert_value(const Core &c, uint32_t *v) {
    if (!(c.flag & OGE_F_PAIRED) || !(c.flag & OGE_F_READ1) || c.tlen == 0) return false;
    *v = c.tlen < 0 ? (uint32_t)(-(int64_t)c.tlen) : (uint32_t)c.tlen;  // |INT32_MIN| = 2^31
    return true;
}

template <bool LEN>
__global__ __launch_bounds__(kT) void k_qc_stats(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ off, uint64_t n,
                                                 QcAcc *__restrict__ acc, QcEdge *__restrict__ edge,
                                                 unsigned long long *__restrict__ lenhist) {
    __shared__ unsigned long long s_part[kWaves][kNumCounters + 3];
    __shared__ uint32_t s_hist[LEN ? kLenTab : 1];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t gw = (uint64_t)blockIdx.x * kWaves + wave;
    if (LEN) {
        for (uint32_t b = threadIdx.x; b < kLenTab; b += kT) s_hist[b] = 0;
        __syncthreads();
    }
    unsigned long long c[kNumCounters];
#pragma unroll
    for (int k = 0; k < kNumCounters; ++k) c[k] = 0;
    unsigned long long isum = 0;
    uint32_t icnt = 0, nbig = 0;
    // the last two considered keys before the current step and the first two of the range
    int32_t r1 = -1, p1 = -1, r2 = -1, p2 = -1, f0r = -1, f0p = -1, f1r = -1, f1p = -1;
    uint32_t seen = 0;
    bool bad = false;
    const uint64_t base = gw * kWaveRecs;
    for (int it = 0; it < kIter; ++it) {
        const uint64_t i0 = base + (uint64_t)it * 64;
        if (i0 >= n) break;  // wave-uniform
        const uint64_t i = i0 + lane;
        const bool valid = i < n;
        Core q = {-1, -1, 0, 0, 0};
        if (valid) q = load_core(recs + off[i]);
        const uint32_t f = q.flag;
        const bool mapped = valid && !(f & OGE_F_UNMAP), paired = valid && (f & OGE_F_PAIRED);
        c[0] += __popcll(__ballot(valid));
        c[1] += __popcll(__ballot(mapped));
        c[2] += __popcll(__ballot(valid && !(f & OGE_F_REVERSE)));
        c[3] += __popcll(__ballot(valid && (f & OGE_F_REVERSE)));
        c[4] += __popcll(__ballot(valid && (f & OGE_F_QCFAIL)));
        c[5] += __popcll(__ballot(valid && (f & OGE_F_DUP)));
        c[6] += __popcll(__ballot(paired));
        c[7] += __popcll(__ballot(paired && (f & OGE_F_PROPER)));
        c[8] += __popcll(__ballot(paired && (f & OGE_F_READ1)));
        c[9] += __popcll(__ballot(paired && (f & OGE_F_READ2)));
        c[10] += __popcll(__ballot(paired && mapped && !(f & OGE_F_MUNMAP)));
        c[11] += __popcll(__ballot(paired && mapped && (f & OGE_F_MUNMAP)));
        uint32_t iv = 0;
        if (valid && insert_value(q, &iv)) {
            isum += iv;
            ++icnt;
        }
        if (LEN) {
            const uint32_t key = (uint32_t)q.lseq;
            lds_hist_add(s_hist, key, valid && key < kLenTab);
            if (valid && key >= kLenTab) ++nbig;
        }
        // ---- order: predecessors inside the step by ballot, before it from the carried keys
        const bool cons = valid && q.refid != -1 && q.pos != -1;
        const uint64_t m = __ballot(cons);
        if (m) {
            const uint64_t below = m & ((1ull << lane) - 1ull);
            const int l1 = below ? 63 - __clzll((long long)below) : -1;
            const uint64_t below2 = l1 >= 0 ? below & ~(1ull << l1) : 0;
            const int l2 = below2 ? 63 - __clzll((long long)below2) : -1;
            const int32_t sr1 = __shfl(q.refid, l1 < 0 ? 0 : l1, 64), sp1 = __shfl(q.pos, l1 < 0 ? 0 : l1, 64);
            const int32_t sr2 = __shfl(q.refid, l2 < 0 ? 0 : l2, 64);
            const int32_t a_r1 = l1 >= 0 ? sr1 : r1, a_p1 = l1 >= 0 ? sp1 : p1;
            const int32_t a_r2 = l2 >= 0 ? sr2 : (l1 >= 0 ? r1 : r2);
            const uint32_t ord = seen + (uint32_t)__popcll(below);
            if (cons && ord >= 2 && out_of_order(a_r2, a_r1, a_p1, q.refid, q.pos)) bad = true;
            const int first = __ffsll((long long)m) - 1;
            const uint64_t m2 = m & (m - 1);
            if (seen == 0) {
                f0r = __shfl(q.refid, first, 64);
                f0p = __shfl(q.pos, first, 64);
                if (m2) {
                    const int second = __ffsll((long long)m2) - 1;
                    f1r = __shfl(q.refid, second, 64);
                    f1p = __shfl(q.pos, second, 64);
                }
            } else if (seen == 1) {
                f1r = __shfl(q.refid, first, 64);
                f1p = __shfl(q.pos, first, 64);
            }
            const int t1 = 63 - __clzll((long long)m);
            const uint64_t mm = m & ~(1ull << t1);
            if (mm) {
                const int t2 = 63 - __clzll((long long)mm);
                r2 = __shfl(q.refid, t2, 64);
                p2 = __shfl(q.pos, t2, 64);
            } else {
                r2 = r1;
                p2 = p1;
            }
            r1 = __shfl(q.refid, t1, 64);
            p1 = __shfl(q.pos, t1, 64);
            seen += (uint32_t)__popcll(m);
        }
    }
    if (lane == 0) {
        QcEdge e;
        e.cnt = seen > 2 ? 2 : (int32_t)seen;
        e.r[0] = f0r, e.p[0] = f0p, e.r[1] = f1r, e.p[1] = f1p;
        e.r[2] = r2, e.p[2] = p2, e.r[3] = r1, e.p[3] = p1;
        edge[gw] = e;
    }
    if (__ballot(bad) && lane == 0) atomicOr(&acc->unsorted, 1ull);
    // ---- per block one atomic per counter
    const unsigned long long ws = wave_sum_u64(isum);
    const uint32_t wc = oge_wave_sum(icnt), wb = oge_wave_sum(nbig);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kNumCounters; ++k) s_part[wave][k] = c[k];
        s_part[wave][kNumCounters] = wc;
        s_part[wave][kNumCounters + 1] = ws;
        s_part[wave][kNumCounters + 2] = wb;
    }
    __syncthreads();
    if (threadIdx.x < kNumCounters + 3) {
        unsigned long long v = 0;
        for (int w = 0; w < kWaves; ++w) v += s_part[w][threadIdx.x];
        if (v) atomicAdd((unsigned long long *)acc + threadIdx.x, v);  // words 12..14: n_insert, insert_sum, n_big
    }
    if (LEN)
        for (uint32_t b = threadIdx.x; b < kLenTab; b += kT) {
            const uint32_t v = s_hist[b];
            if (v) atomicAdd(&lenhist[b], (unsigned long long)v);
        }
}

// The first two keys of every wave range against the keys before the range, in file order.  Thread t folds
// ranges [t*S, (t+1)*S) into one summary, thread 0 turns the summaries into the state in front of every
// segment, then every thread walks its segment again with that state.
__global__ __launch_bounds__(kStitchT) void k_qc_stitch(const QcEdge *__restrict__ edge, uint64_t nw, QcAcc *__restrict__ acc) {
    __shared__ int32_t s_cnt[kStitchT], s_r1[kStitchT], s_p1[kStitchT], s_r2[kStitchT], s_p2[kStitchT];
    const uint64_t S = (nw + kStitchT - 1) / kStitchT;
    const uint64_t a = std::min<uint64_t>(nw, threadIdx.x * S), b = std::min<uint64_t>(nw, a + S);
    int32_t cnt = 0, r1 = -1, p1 = -1, r2 = -1, p2 = -1;
    for (uint64_t w = a; w < b; ++w) {
        const QcEdge e = edge[w];
        if (e.cnt >= 2) {
            r2 = e.r[2], p2 = e.p[2], r1 = e.r[3], p1 = e.p[3];
            cnt = 2;
        } else if (e.cnt == 1) {
            r2 = r1, p2 = p1, r1 = e.r[3], p1 = e.p[3];
            cnt = cnt < 2 ? cnt + 1 : 2;
        }
    }
    s_cnt[threadIdx.x] = cnt, s_r1[threadIdx.x] = r1, s_p1[threadIdx.x] = p1, s_r2[threadIdx.x] = r2, s_p2[threadIdx.x] = p2;
    __syncthreads();
    if (threadIdx.x == 0) {  // exclusive fold; before the file: the reference's last_rid = last_position = -1
        int32_t R1 = -1, P1 = -1, R2 = -1, P2 = -1;
        for (int t = 0; t < kStitchT; ++t) {
            const int32_t c = s_cnt[t], x1 = s_r1[t], y1 = s_p1[t], x2 = s_r2[t], y2 = s_p2[t];
            s_r1[t] = R1, s_p1[t] = P1, s_r2[t] = R2, s_p2[t] = P2;
            if (c >= 2) R2 = x2, P2 = y2, R1 = x1, P1 = y1;
            else if (c == 1) R2 = R1, P2 = P1, R1 = x1, P1 = y1;
        }
    }
    __syncthreads();
    r1 = s_r1[threadIdx.x], p1 = s_p1[threadIdx.x], r2 = s_r2[threadIdx.x], p2 = s_p2[threadIdx.x];
    bool bad = false;
    for (uint64_t w = a; w < b; ++w) {
        const QcEdge e = edge[w];
        if (e.cnt < 1) continue;
        bad |= out_of_order(r2, r1, p1, e.r[0], e.p[0]);
        if (e.cnt >= 2) {
            bad |= out_of_order(r1, e.r[0], e.p[0], e.r[1], e.p[1]);
            r2 = e.r[2], p2 = e.p[2], r1 = e.r[3], p1 = e.p[3];
        } else {
            r2 = r1, p2 = p1, r1 = e.r[0], p1 = e.p[0];
        }
    }
    (void)p2;
    if (bad) atomicOr(&acc->unsorted, 1ull);
}

// ascending (length, count) pairs of the table's non-empty entries; *n_small = how many
__global__ __launch_bounds__(kT) void k_qc_len_small(const unsigned long long *__restrict__ lenhist, uint32_t *__restrict__ len,
                                                     unsigned long long *__restrict__ cnt, uint32_t *__restrict__ n_small) {
    __shared__ uint32_t s_n[kT];
    constexpr uint32_t per = kLenTab / kT;
    uint32_t c = 0;
    for (uint32_t k = 0; k < per; ++k) c += lenhist[threadIdx.x * per + k] != 0;
    s_n[threadIdx.x] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int t = 0; t < kT; ++t) {
            const uint32_t v = s_n[t];
            s_n[t] = run;
            run += v;
        }
        *n_small = run;
    }
    __syncthreads();
    uint32_t o = s_n[threadIdx.x];
    for (uint32_t k = 0; k < per; ++k) {
        const unsigned long long v = lenhist[threadIdx.x * per + k];
        if (v) {
            len[o] = threadIdx.x * per + k;
            cnt[o] = v;
            ++o;
        }
    }
}

// every l_seq >= kLenTab into keys (any order; cap entries: the count of the stats pass)
__global__ __launch_bounds__(kT) void k_qc_biglen(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ off, uint64_t n,
                                                  uint64_t *__restrict__ keys, uint64_t cap, unsigned int *__restrict__ fill) {
    const uint64_t stride = (uint64_t)gridDim.x * kT;
    for (uint64_t i0 = (uint64_t)blockIdx.x * kT; i0 < n; i0 += stride) {  // block-uniform bound
        const uint64_t i = i0 + threadIdx.x;
        uint32_t key = 0;
        if (i < n) key = oge_ldu32(recs + off[i] + OGE_OFF_LSEQ);
        const bool big = i < n && key >= kLenTab;
        const uint32_t slot = oge_wave_append(big, fill);
        if (big && slot < cap) keys[slot] = key;
    }
}

// sorted keys -> run heads (head has nbig + 1 entries, the last one 0)
__global__ __launch_bounds__(kT) void k_qc_run_heads(const uint64_t *__restrict__ ks, uint64_t nbig, uint32_t *__restrict__ head) {
    const uint64_t i = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (i > nbig) return;
    head[i] = i < nbig && (i == 0 || ks[i] != ks[i - 1]);
}
// slot = the exclusive scan of head: record i starts run slot[i] when slot[i + 1] != slot[i]
__global__ __launch_bounds__(kT) void k_qc_run_starts(const uint64_t *__restrict__ ks, uint64_t nbig, const uint32_t *__restrict__ slot,
                                                      const uint32_t *__restrict__ n_small, uint32_t *__restrict__ len,
                                                      uint32_t *__restrict__ start) {
    const uint64_t i = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (i >= nbig || slot[i + 1] == slot[i]) return;
    len[*n_small + slot[i]] = (uint32_t)ks[i];
    start[slot[i]] = (uint32_t)i;
}
__global__ __launch_bounds__(kT) void k_qc_run_counts(const uint32_t *__restrict__ start, uint64_t nruns, uint64_t nbig,
                                                      const uint32_t *__restrict__ n_small, unsigned long long *__restrict__ cnt) {
    const uint64_t s = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (s >= nruns) return;
    cnt[*n_small + s] = (s + 1 < nruns ? start[s + 1] : nbig) - start[s];
}

// One pass of the radix select: histogram of the pass's digit over the insert sizes whose higher bits equal
// the bits already chosen, once for the lower and once for the upper middle.
template <int PASS>
__global__ __launch_bounds__(kT) void k_qc_sel_hist(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ off, uint64_t n,
                                                    const QcSel *__restrict__ sel, unsigned long long *__restrict__ hist) {
    __shared__ uint32_t s_h[2][kSelBins];
    for (uint32_t b = threadIdx.x; b < 2 * kSelBins; b += kT) (&s_h[0][0])[b] = 0;
    __syncthreads();
    const uint32_t pa = sel->prefix[0], pb = sel->prefix[1];
    const uint64_t stride = (uint64_t)gridDim.x * kT;
    for (uint64_t i0 = (uint64_t)blockIdx.x * kT; i0 < n; i0 += stride) {  // block-uniform bound
        const uint64_t i = i0 + threadIdx.x;
        uint32_t v = 0;
        bool q = false;
        if (i < n) q = insert_value(load_core(recs + off[i]), &v);
        const uint32_t hi = PASS == 0 ? 0 : PASS == 1 ? v >> 21 : v >> 10;
        const uint32_t dig = PASS == 0 ? v >> 21 : PASS == 1 ? (v >> 10) & 0x7FF : v & 0x3FF;
        lds_hist_add(s_h[0], dig, q && hi == pa);
        lds_hist_add(s_h[1], dig, q && hi == pb);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < 2 * kSelBins; b += kT) {
        const uint32_t v = (&s_h[0][0])[b];
        if (v) atomicAdd(&hist[b], (unsigned long long)v);
    }
}

// the bucket that holds each rank; after the last pass the chosen bits are the values
template <int PASS>
__global__ __launch_bounds__(kT) void k_qc_sel_pick(const unsigned long long *__restrict__ hist, QcSel *__restrict__ sel,
                                                    unsigned long long *__restrict__ mid) {
    if (threadIdx.x >= 2) return;
    const unsigned long long *h = hist + threadIdx.x * kSelBins;
    unsigned long long rank = sel->rank[threadIdx.x], run = 0;
    uint32_t b = 0;
    for (; b + 1 < (uint32_t)kSelBins; ++b) {
        const unsigned long long v = h[b];
        if (rank < run + v) break;
        run += v;
    }
    constexpr int bits = PASS == 2 ? 10 : 11;
    const uint32_t prefix = (sel->prefix[threadIdx.x] << bits) | b;
    sel->rank[threadIdx.x] = rank - run;
    sel->prefix[threadIdx.x] = prefix;
    if (PASS == 2) mid[threadIdx.x] = prefix;
}

__device__ __forceinline__ void cov_add_global(uint32_t *bins, uint64_t g, uint32_t v, CovOut *out) {
    const uint32_t old = atomicAdd(&bins[g], v);
    if ((uint64_t)old + v >= 0xFFFFFFFFull) out->overflow = 1;
}

// positions [lo, hi] of one read into the bins of its contig (first bin of the contig: gb); called by the
// whole wave
template <bool LDS>
__device__ __forceinline__ void cov_add_read(bool ok, uint32_t lo, uint32_t hi, uint64_t gb, uint32_t bs, uint32_t *s_win, uint64_t wmin,
                                             uint32_t *bins, CovOut *out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t b0 = ok ? lo / bs : 0, b1 = ok ? hi / bs : 0;
    const bool wide = ok && b1 - b0 >= 64;
    auto add = [&](uint32_t xlo, uint32_t xhi, uint64_t xgb, uint32_t b) {
        const uint64_t s = std::max<uint64_t>(xlo, (uint64_t)b * bs), e = std::min<uint64_t>(xhi, ((uint64_t)b + 1) * bs - 1);
        const uint32_t v = (uint32_t)(e - s + 1);
        if (LDS) atomicAdd(&s_win[xgb + b - wmin], v);
        else cov_add_global(bins, xgb + b, v, out);
    };
    if (ok && !wide)
        for (uint32_t b = b0;; ++b) {
            add(lo, hi, gb, b);
            if (b == b1) break;
        }
    uint64_t m = __ballot(wide);
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const uint32_t xlo = (uint32_t)__shfl((int)lo, src, 64), xhi = (uint32_t)__shfl((int)hi, src, 64);
        const uint32_t glo = (uint32_t)__shfl((int)(uint32_t)gb, src, 64), ghi = (uint32_t)__shfl((int)(uint32_t)(gb >> 32), src, 64);
        const uint64_t xgb = ((uint64_t)ghi << 32) | glo;
        const uint32_t xb0 = xlo / bs, xb1 = xhi / bs;
        for (uint64_t b = (uint64_t)xb0 + lane; b <= xb1; b += 64) add(xlo, xhi, xgb, (uint32_t)b);
    }
}

__global__ __launch_bounds__(kT) void k_qc_cov(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ off, uint64_t n, int32_t n_ref,
                                               const uint64_t *__restrict__ base, uint32_t bs, uint32_t *__restrict__ bins,
                                               CovOut *__restrict__ out) {
    __shared__ uint32_t s_win[kCovWin];
    __shared__ unsigned long long s_min, s_max;
    __shared__ uint32_t s_maxov;
    const uint64_t ntiles = (n + kCovTile - 1) / kCovTile;
    uint32_t skipped = 0;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // block-uniform
        if (threadIdx.x == 0) {
            s_min = kNone;
            s_max = 0;
            s_maxov = 0;
        }
        __syncthreads();
        uint32_t lo[kCovPer], hi[kCovPer];
        uint64_t gb[kCovPer];
        bool ok[kCovPer];
        unsigned long long tmin = kNone, tmax = 0;
        uint32_t tov = 0;
#pragma unroll
        for (int k = 0; k < kCovPer; ++k) {
            const uint64_t i = tile * kCovTile + (uint64_t)k * kT + threadIdx.x;
            ok[k] = false;
            lo[k] = hi[k] = 0;
            gb[k] = 0;
            if (i >= n) continue;
            const uint8_t *r = recs + off[i];
            const int32_t rid = (int32_t)oge_ldu32(r + OGE_OFF_REFID), pos = (int32_t)oge_ldu32(r + OGE_OFF_POS);
            if (rid == -1 || pos == -1) {
                ++skipped;
                continue;
            }
            if (rid < 0 || rid >= n_ref) {
                atomicMin(&out->badref, (unsigned long long)i);
                continue;
            }
            const int32_t lseq = (int32_t)oge_ldu32(r + OGE_OFF_LSEQ);
            const uint64_t b = base[rid], nb = base[rid + 1] - b;
            // positions pos .. pos + l_seq; those below 0 or past the contig's last bin are dropped
            const int64_t L = pos < 0 ? 0 : pos, H = std::min<int64_t>((int64_t)pos + lseq, (int64_t)(nb * bs) - 1);
            if (L > H) continue;
            ok[k] = true;
            lo[k] = (uint32_t)L, hi[k] = (uint32_t)H, gb[k] = b;
            tmin = std::min<unsigned long long>(tmin, b + lo[k] / bs);
            tmax = std::max<unsigned long long>(tmax, b + hi[k] / bs);
            tov = std::max<uint32_t>(tov, (uint32_t)std::min<int64_t>(bs, H - L + 1));
        }
        if (tmin != kNone) {
            atomicMin(&s_min, tmin);
            atomicMax(&s_max, tmax);
            atomicMax(&s_maxov, tov);
        }
        __syncthreads();
        const uint64_t wmin = s_min, wmax = s_max;
        // the window's sums stay below 2^32: kCovTile reads of at most s_maxov positions per bin
        const bool any = wmin != kNone, lds = any && wmax - wmin < kCovWin && (uint64_t)s_maxov * kCovTile < (1ull << 32);
        if (any) {
            const uint32_t span = lds ? (uint32_t)(wmax - wmin + 1) : 0;
            for (uint32_t j = threadIdx.x; j < span; j += kT) s_win[j] = 0;
            __syncthreads();
#pragma unroll
            for (int k = 0; k < kCovPer; ++k) {
                if (lds) cov_add_read<true>(ok[k], lo[k], hi[k], gb[k], bs, s_win, wmin, bins, out);
                else cov_add_read<false>(ok[k], lo[k], hi[k], gb[k], bs, s_win, wmin, bins, out);
            }
            __syncthreads();
            for (uint32_t j = threadIdx.x; j < span; j += kT) {
                const uint32_t v = s_win[j];
                if (v) cov_add_global(bins, wmin + j, v, out);
            }
        }
        __syncthreads();  // the next tile resets the window and its bounds
    }
    const uint32_t ws = oge_wave_sum(skipped);
    if ((threadIdx.x & 63) == 0 && ws) atomicAdd(&out->skipped, (unsigned long long)ws);
}

void drop_ws(oge_ctx *ctx, const char *name) {
    auto it = ctx->bufs.find(name);
    if (it == ctx->bufs.end()) return;
    ctx->release(it->second.p);
    ctx->bufs.erase(it);
}

inline dim3 grid_for(uint64_t items) { return dim3(std::max<uint32_t>(1, oge_ceil_div(items, kT))); }

}  // namespace

int oge_qc_stats_impl(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, uint32_t want, oge_bam_stats *out,
                      const uint32_t **d_len, const uint64_t **d_len_count) {
    memset(out, 0, sizeof *out);
    out->sorted = 1;
    if (d_len) *d_len = nullptr;
    if (d_len_count) *d_len_count = nullptr;
    if (want & ~(uint32_t)(OGE_STATS_INSERTS | OGE_STATS_LENGTHS)) return oge_fail(ctx, OGE_ERR_ARG, "stats: unknown request bits");
    const bool lengths = want & OGE_STATS_LENGTHS, inserts = want & OGE_STATS_INSERTS;
    if (lengths && (!d_len || !d_len_count)) return oge_fail(ctx, OGE_ERR_ARG, "stats: lengths requested without output pointers");
    if (n && (!d_recs || !d_off)) return oge_fail(ctx, OGE_ERR_ARG, "stats: null argument");
    if (n >= 0xFFFFFFFFull * kBlockRecs) return oge_fail(ctx, OGE_ERR_LIMIT, "stats: too many records");
    OgeStage stage(ctx, "qc_stats");
    hipStream_t st = ctx->stream;
    const uint32_t nblk = oge_ceil_div(n, kBlockRecs);
    const uint64_t nw = (uint64_t)nblk * kWaves;
    ctx->counters["qc_wave_records"] = kWaveRecs;
    ctx->counters["qc_block_records"] = kBlockRecs;
    ctx->counters["qc_length_table"] = kLenTab;
    // accumulators | length table | select histograms (3 passes x 2 ranks) | select state | middles | small count | fill
    constexpr size_t oTab = sizeof(QcAcc), oSel = oTab + kLenTab * 8, oState = oSel + 3 * 2 * kSelBins * 8, oMid = oState + sizeof(QcSel),
                     oSmall = oMid + 16, oFill = oSmall + 8, oEnd = oFill + 8;
    uint8_t *z = (uint8_t *)ctx->ws("qc_acc", oEnd);
    QcEdge *edge = (QcEdge *)ctx->ws("qc_edge", std::max<uint64_t>(nw, 1) * sizeof(QcEdge));
    if (!z || !edge) return OGE_ERR_HIP;
    OGE_HIP_TRY(ctx, hipMemsetAsync(z, 0, oEnd, st));
    QcAcc *acc = (QcAcc *)z;
    unsigned long long *lenhist = (unsigned long long *)(z + oTab), *selhist = (unsigned long long *)(z + oSel),
                       *mid = (unsigned long long *)(z + oMid);
    QcSel *sel = (QcSel *)(z + oState);
    uint32_t *n_small = (uint32_t *)(z + oSmall);
    unsigned int *fill = (unsigned int *)(z + oFill);
    QcAcc h;
    memset(&h, 0, sizeof h);
    if (n) {
        if (lengths) hipLaunchKernelGGL(k_qc_stats<true>, dim3(nblk), dim3(kT), 0, st, d_recs, d_off, n, acc, edge, lenhist);
        else hipLaunchKernelGGL(k_qc_stats<false>, dim3(nblk), dim3(kT), 0, st, d_recs, d_off, n, acc, edge, lenhist);
        OGE_LAUNCH_CHECK(ctx);
        hipLaunchKernelGGL(k_qc_stitch, dim3(1), dim3(kStitchT), 0, st, (const QcEdge *)edge, nw, acc);
        OGE_LAUNCH_CHECK(ctx);
        OGE_HIP_TRY(ctx, hipMemcpyAsync(&h, acc, sizeof h, hipMemcpyDeviceToHost, st));
        OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    uint64_t *dst = &out->reads;
    for (int k = 0; k < kNumCounters; ++k) dst[k] = h.c[k];
    out->sorted = h.unsorted ? 0 : 1;
    out->n_insert = h.n_insert;
    out->insert_sum = h.insert_sum;

    if (inserts && h.n_insert) {
        const QcSel s0 = {{(h.n_insert - 1) / 2, h.n_insert / 2}, {0, 0}};
        OGE_HIP_TRY(ctx, hipMemcpyAsync(sel, &s0, sizeof s0, hipMemcpyHostToDevice, st));
        const dim3 g(std::min<uint32_t>(oge_ceil_div(n, kT), (uint32_t)ctx->cu_count() * 8));
        hipLaunchKernelGGL(k_qc_sel_hist<0>, g, dim3(kT), 0, st, d_recs, d_off, n, (const QcSel *)sel, selhist);
        hipLaunchKernelGGL(k_qc_sel_pick<0>, dim3(1), dim3(kT), 0, st, (const unsigned long long *)selhist, sel, mid);
        hipLaunchKernelGGL(k_qc_sel_hist<1>, g, dim3(kT), 0, st, d_recs, d_off, n, (const QcSel *)sel, selhist + 2 * kSelBins);
        hipLaunchKernelGGL(k_qc_sel_pick<1>, dim3(1), dim3(kT), 0, st, (const unsigned long long *)(selhist + 2 * kSelBins), sel, mid);
        hipLaunchKernelGGL(k_qc_sel_hist<2>, g, dim3(kT), 0, st, d_recs, d_off, n, (const QcSel *)sel, selhist + 4 * kSelBins);
        hipLaunchKernelGGL(k_qc_sel_pick<2>, dim3(1), dim3(kT), 0, st, (const unsigned long long *)(selhist + 4 * kSelBins), sel, mid);
        OGE_LAUNCH_CHECK(ctx);
        unsigned long long m2[2] = {0, 0};
        OGE_HIP_TRY(ctx, hipMemcpyAsync(m2, mid, 16, hipMemcpyDeviceToHost, st));
        OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
        out->insert_mid_lo = m2[0];
        out->insert_mid_hi = m2[1];
    }

    if (lengths) {
        const uint64_t nbig = h.n_big;
        if (nbig >= 0xFFFFFFFFull) return oge_fail(ctx, OGE_ERR_LIMIT, "stats: more than 2^32-2 reads beyond the length table");
        // both arrays hold the table's entries and one per long read; they stay until the next call
        uint32_t *len = (uint32_t *)ctx->ws("qc_len", (kLenTab + nbig) * 4);
        unsigned long long *cnt = (unsigned long long *)ctx->ws("qc_len_count", (kLenTab + nbig) * 8);
        if (!len || !cnt) return OGE_ERR_HIP;
        hipLaunchKernelGGL(k_qc_len_small, dim3(1), dim3(kT), 0, st, (const unsigned long long *)lenhist, len, cnt, n_small);
        OGE_LAUNCH_CHECK(ctx);
        uint32_t nruns = 0;
        if (nbig) {
            uint64_t *keys = (uint64_t *)ctx->ws("qc_big", nbig * 8), *ktmp = (uint64_t *)ctx->ws("qc_big_tmp", nbig * 8), *ks = nullptr;
            uint32_t *slot = (uint32_t *)ctx->ws("qc_big_slot", (nbig + 1) * 4), *start = (uint32_t *)ctx->ws("qc_big_start", nbig * 4);
            if (!keys || !ktmp || !slot || !start) return OGE_ERR_HIP;
            const dim3 g(std::min<uint32_t>(oge_ceil_div(n, kT), (uint32_t)ctx->cu_count() * 8));
            hipLaunchKernelGGL(k_qc_biglen, g, dim3(kT), 0, st, d_recs, d_off, n, keys, nbig, fill);
            OGE_LAUNCH_CHECK(ctx);
            int rc = oge_radix_sort_pairs(ctx, keys, nullptr, ktmp, nullptr, nbig, 0xFFFFFFFFull, &ks, nullptr);
            if (rc) return rc;
            hipLaunchKernelGGL(k_qc_run_heads, grid_for(nbig + 1), dim3(kT), 0, st, (const uint64_t *)ks, nbig, slot);
            OGE_LAUNCH_CHECK(ctx);
            rc = oge_exclusive_scan_u32(ctx, slot, slot, nbig + 1);
            if (rc) return rc;
            OGE_HIP_TRY(ctx, hipMemcpyAsync(&nruns, slot + nbig, 4, hipMemcpyDeviceToHost, st));
            OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
            hipLaunchKernelGGL(k_qc_run_starts, grid_for(nbig), dim3(kT), 0, st, (const uint64_t *)ks, nbig, (const uint32_t *)slot,
                               (const uint32_t *)n_small, len, start);
            OGE_LAUNCH_CHECK(ctx);
            hipLaunchKernelGGL(k_qc_run_counts, grid_for(nruns), dim3(kT), 0, st, (const uint32_t *)start, (uint64_t)nruns, nbig,
                               (const uint32_t *)n_small, cnt);
            OGE_LAUNCH_CHECK(ctx);
        }
        uint32_t ns = 0;
        OGE_HIP_TRY(ctx, hipMemcpyAsync(&ns, n_small, 4, hipMemcpyDeviceToHost, st));
        OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
        for (const char *nm : {"qc_big", "qc_big_tmp", "qc_big_slot", "qc_big_start"}) drop_ws(ctx, nm);
        out->n_lengths = (uint64_t)ns + nruns;
        *d_len = len;
        *d_len_count = (const uint64_t *)cnt;
    }
    return OGE_OK;
}

int oge_qc_coverage_impl(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, int32_t n_ref, const int32_t *ref_len,
                         int32_t binsize, const uint32_t **d_bins, uint64_t *n_skipped, int32_t *overflow) {
    *d_bins = nullptr;
    *n_skipped = 0;
    *overflow = 0;
    if (n && (!d_recs || !d_off)) return oge_fail(ctx, OGE_ERR_ARG, "coverage: null argument");
    std::vector<uint64_t> base((size_t)std::max(n_ref, 0) + 1);
    int rc = oge_coverage_layout(n_ref, ref_len, binsize, base.data());
    if (rc) return oge_fail(ctx, rc, "coverage: binsize < 1, n_ref < 0 or no reference lengths");
    const uint64_t nb = base[n_ref];
    // the last call's bins go first: what is held is sized by this call alone
    (void)hipStreamSynchronize(ctx->stream);
    drop_ws(ctx, "qc_bins");
    size_t free_b = 0, total_b = 0;
    OGE_HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
    const std::string too_many = "coverage: " + std::to_string(nb) + " bins do not fit in free device memory: use a larger --binsize";
    if (nb > (1ull << 60) || nb * 4 > total_b) return oge_fail(ctx, OGE_ERR_LIMIT, too_many.c_str());
    OgeStage stage(ctx, "qc_coverage");
    hipStream_t st = ctx->stream;
    // free memory is what the allocation finds (the context's pool may hold more than hipMemGetInfo reports)
    uint32_t *bins = (uint32_t *)ctx->ws("qc_bins", nb * 4);
    if (!bins) {
        (void)hipGetLastError();
        ctx->bufs.erase("qc_bins");
        return oge_fail(ctx, OGE_ERR_LIMIT, too_many.c_str());
    }
    uint64_t *dbase = (uint64_t *)ctx->ws("qc_base", base.size() * 8);
    CovOut *out = (CovOut *)ctx->ws("qc_cov_out", sizeof(CovOut));
    if (!bins || !dbase || !out) return OGE_ERR_HIP;
    CovOut h = {0, kNone, 0};
    OGE_HIP_TRY(ctx, hipMemsetAsync(bins, 0, std::max<uint64_t>(nb, 1) * 4, st));
    OGE_HIP_TRY(ctx, hipMemcpyAsync(dbase, base.data(), base.size() * 8, hipMemcpyHostToDevice, st));
    OGE_HIP_TRY(ctx, hipMemcpyAsync(out, &h, sizeof h, hipMemcpyHostToDevice, st));
    if (n) {
        const uint64_t ntiles = (n + kCovTile - 1) / kCovTile;
        const dim3 g((uint32_t)std::min<uint64_t>(ntiles, (uint64_t)ctx->cu_count() * 8));
        hipLaunchKernelGGL(k_qc_cov, g, dim3(kT), 0, st, d_recs, d_off, n, n_ref, (const uint64_t *)dbase, (uint32_t)binsize, bins, out);
        OGE_LAUNCH_CHECK(ctx);
    }
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&h, out, sizeof h, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    ctx->counters["qc_cov_tile_records"] = kCovTile;
    ctx->counters["qc_cov_window"] = kCovWin;
    if (h.badref != kNone)
        return oge_fail(ctx, OGE_ERR_ARG, ("coverage: record " + std::to_string(h.badref) + " has a refID outside [-1, n_ref)").c_str());
    *d_bins = bins;
    *n_skipped = h.skipped;
    *overflow = h.overflow ? 1 : 0;
    return OGE_OK;
}

extern "C" {

int oge_coverage_layout(int32_t n_ref, const int32_t *ref_len, int32_t binsize, uint64_t *base) {
    if (binsize < 1 || n_ref < 0 || !base || (n_ref && !ref_len)) return OGE_ERR_ARG;
    base[0] = 0;
    for (int32_t r = 0; r < n_ref; ++r) {
        const uint64_t ln = ref_len[r] > 0 ? (uint64_t)ref_len[r] : 0;
        base[r + 1] = base[r] + (ln + (uint64_t)binsize - 1) / (uint64_t)binsize;
    }
    return OGE_OK;
}

int oge_stats_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, uint32_t want, oge_bam_stats *stats,
                  const uint32_t **d_len, const uint64_t **d_len_count) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!stats) return oge_fail(ctx, OGE_ERR_ARG, "oge_stats_dev: null argument");
    OgeCall call(ctx, /*hold=*/false);
    return oge_qc_stats_impl(ctx, d_recs, d_off, n, want, stats, d_len, d_len_count);
}

int oge_stats(oge_ctx *ctx, const uint8_t *recs, uint64_t rec_bytes, const uint64_t *rec_off, uint64_t n, uint32_t want,
              oge_bam_stats *stats, uint32_t *len_out, uint64_t *len_count_out, uint64_t cap) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!stats || (n && (!recs || !rec_off))) return oge_fail(ctx, OGE_ERR_ARG, "oge_stats: null argument");
    (void)hipSetDevice(ctx->device);
    uint8_t *dr = (uint8_t *)ctx->ws("host_recs", rec_bytes + 16);
    uint64_t *dof = (uint64_t *)ctx->ws("host_off", (n + 1) * 8);
    if (!dr || !dof) return OGE_ERR_HIP;
    if (rec_bytes) OGE_HIP_TRY(ctx, hipMemcpyAsync(dr, recs, rec_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (n) OGE_HIP_TRY(ctx, hipMemcpyAsync(dof, rec_off, n * 8, hipMemcpyHostToDevice, ctx->stream));
    const uint32_t *dl = nullptr;
    const uint64_t *dc = nullptr;
    const int rc = oge_stats_dev(ctx, dr, dof, n, want, stats, &dl, &dc);
    if (rc) return rc;
    if (want & OGE_STATS_LENGTHS) {
        if (stats->n_lengths > cap || (stats->n_lengths && (!len_out || !len_count_out)))
            return oge_fail(ctx, OGE_ERR_LIMIT, "oge_stats: length arrays too small");
        if (stats->n_lengths) {
            OGE_HIP_TRY(ctx, hipMemcpyAsync(len_out, dl, stats->n_lengths * 4, hipMemcpyDeviceToHost, ctx->stream));
            OGE_HIP_TRY(ctx, hipMemcpyAsync(len_count_out, dc, stats->n_lengths * 8, hipMemcpyDeviceToHost, ctx->stream));
            OGE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
    }
    return OGE_OK;
}

int oge_coverage_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, int32_t n_ref, const int32_t *ref_len,
                     int32_t binsize, const uint32_t **d_bins, uint64_t *n_skipped, int32_t *overflow) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!d_bins || !n_skipped || !overflow) return oge_fail(ctx, OGE_ERR_ARG, "oge_coverage_dev: null argument");
    OgeCall call(ctx, /*hold=*/false);
    return oge_qc_coverage_impl(ctx, d_recs, d_off, n, n_ref, ref_len, binsize, d_bins, n_skipped, overflow);
}

int oge_coverage(oge_ctx *ctx, const uint8_t *recs, uint64_t rec_bytes, const uint64_t *rec_off, uint64_t n, int32_t n_ref,
                 const int32_t *ref_len, int32_t binsize, uint32_t *bins_out, uint64_t cap, uint64_t *n_skipped, int32_t *overflow) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!n_skipped || !overflow || (n && (!recs || !rec_off))) return oge_fail(ctx, OGE_ERR_ARG, "oge_coverage: null argument");
    (void)hipSetDevice(ctx->device);
    std::vector<uint64_t> base((size_t)std::max(n_ref, 0) + 1);
    if (oge_coverage_layout(n_ref, ref_len, binsize, base.data()))
        return oge_fail(ctx, OGE_ERR_ARG, "coverage: binsize < 1, n_ref < 0 or no reference lengths");
    if (base[n_ref] > cap || (base[n_ref] && !bins_out)) return oge_fail(ctx, OGE_ERR_LIMIT, "oge_coverage: output buffer too small");
    uint8_t *dr = (uint8_t *)ctx->ws("host_recs", rec_bytes + 16);
    uint64_t *dof = (uint64_t *)ctx->ws("host_off", (n + 1) * 8);
    if (!dr || !dof) return OGE_ERR_HIP;
    if (rec_bytes) OGE_HIP_TRY(ctx, hipMemcpyAsync(dr, recs, rec_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (n) OGE_HIP_TRY(ctx, hipMemcpyAsync(dof, rec_off, n * 8, hipMemcpyHostToDevice, ctx->stream));
    const uint32_t *db = nullptr;
    const int rc = oge_coverage_dev(ctx, dr, dof, n, n_ref, ref_len, binsize, &db, n_skipped, overflow);
    if (rc) return rc;
    if (base[n_ref]) OGE_HIP_TRY(ctx, hipMemcpyAsync(bins_out, db, base[n_ref] * 4, hipMemcpyDeviceToHost, ctx->stream));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return OGE_OK;
}

int oge_ctx_last_refs(oge_ctx *ctx, int32_t *n_ref, const char **names, uint64_t *names_bytes, const int32_t **ref_len) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!n_ref || !names || !names_bytes || !ref_len) return oge_fail(ctx, OGE_ERR_ARG, "oge_ctx_last_refs: null argument");
    if (!ctx->refs_valid) return oge_fail(ctx, OGE_ERR_ARG, "no reference list: the context's last call parsed none");
    *n_ref = (int32_t)ctx->ref_lens.size();
    *names = ctx->ref_names.data();
    *names_bytes = ctx->ref_names.size();
    *ref_len = ctx->ref_lens.data();
    return OGE_OK;
}

}  // extern "C"
