// dupmetrics.hip -- the duplication metrics of a MARKED record set resident in HBM: six read counts per library
// (definitions in DESIGN.md section 26 and include/openge_hip.h; the model is tests/dupmetrics_model.py).  Every
// counter is an integer sum over records, so the counts of any partition of a record set add up: one pass serves
// the in-place dedup, the fused sort, every range of the chunked sort and every rank's slice.
//
//   k_dm_count   one thread per record, a workgroup per tile of kTile records.  A thread reads the FLAG and the
//                refID from the core, walks its tags for RG (rg_lookup.h) and forms the key lib * 6 + counter of
//                its class and, for a flagged pair or unpaired read, a second key for the duplicate counter.
//                The keys are summed in the wave: a loop over the distinct keys present (ballot, the leader's key
//                by shuffle, ballot of the equal ones, popcount), one add per distinct key by the leader lane --
//                into a block-private LDS table of n_lib * 6 u32 that is flushed with one 64-bit atomic per
//                non-zero entry when the workgroup is done, or, with more than kLdsLibs libraries, straight into
//                the global table.  No per-record global atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "bam_layout.h"
#include "dev_util.h"
#include "oge_ctx.h"
#include "records.h"
#include "rg_lookup.h"

namespace {

constexpr int kT = 256;
constexpr int kPer = 4;
constexpr int kTile = kT * kPer;  // records of one tile
constexpr int kNC = 6;            // counters per library: the fields of oge_dup_metrics in order
// libraries the LDS table holds: 64 * 6 * 4 = 1536 bytes.  The kernel's registers allow seven waves per SIMD, that
// is seven workgroups of 256 per CU, which take 10.5 KiB of its 160 KiB: the table never limits the occupancy.
// Real files have 1 to 4 libraries.
constexpr int kLdsLibs = 64;
enum { kUnpaired = 0, kPair = 1, kSecondary = 2, kUnmapped = 3, kUnpairedDup = 4, kPairDup = 5 };

static_assert(sizeof(OgeDupMetrics) == kNC * 8, "oge_dup_metrics is six u64");

// tab[key] += the lanes of the wave with `act` and this key, for every distinct key: one add per key by its
// first lane.  Called by the whole wave.
template <bool LDS>
__device__ __forceinline__ void dm_wave_add(uint32_t *s_tab, unsigned long long *g_tab, uint32_t key, bool act, uint32_t lane) {
    uint64_t m = __ballot(act);
    while (m) {  // wave-uniform
        const int ld = __ffsll((long long)m) - 1;
        const uint32_t k = (uint32_t)__shfl((int)key, ld, 64);
        const uint64_t same = __ballot(act && key == k);
        if ((int)lane == ld) {
            if (LDS) atomicAdd(&s_tab[k], (uint32_t)__popcll(same));
            else atomicAdd(&g_tab[k], (unsigned long long)__popcll(same));
        }
        m &= ~same;
    }
}

template <bool LDS>
__global__ __launch_bounds__(kT) void k_dm_count(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ off, uint64_t n, OgeRgTable rg,
                                                 uint32_t n_keys, unsigned long long *__restrict__ out) {
    __shared__ uint32_t s_tab[LDS ? kLdsLibs * kNC : 1];
    const uint32_t lane = threadIdx.x & 63;
    if (LDS) {
        for (uint32_t k = threadIdx.x; k < n_keys; k += kT) s_tab[k] = 0;
        __syncthreads();
    }
    const uint64_t ntiles = (n + kTile - 1) / kTile;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // block-uniform
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const uint64_t i = tile * kTile + (uint64_t)j * kT + threadIdx.x;
            const bool valid = i < n;
            uint32_t key = 0;
            bool dup = false;
            if (valid) {
                const uint8_t *r = recs + off[i];
                const uint32_t bs = oge_ldu32(r + OGE_OFF_BLOCK);
                const bool sane = bs >= 32 && bs <= OGE_MAX_BLOCK_SIZE;  // any other record has no tags to walk
                const uint32_t flag = oge_ldu32(r + OGE_OFF_NCIGAR) >> 16;
                const int32_t rid = (int32_t)oge_ldu32(r + OGE_OFF_REFID);
                const uint32_t cls = ((flag & OGE_F_UNMAP) || rid == -1)               ? kUnmapped
                                     : (flag & OGE_F_SECONDARY)                         ? kSecondary
                                     : ((flag & OGE_F_PAIRED) && !(flag & OGE_F_MUNMAP)) ? kPair
                                                                                         : kUnpaired;
                const uint32_t lib = (uint32_t)(sane ? oge_rg_library(r, bs, rg) : rg.unknown_lib);
                key = lib * kNC + cls;
                dup = (flag & OGE_F_DUP) && cls <= kPair;  // key + 4: the class's duplicate counter
            }
            dm_wave_add<LDS>(s_tab, out, key, valid, lane);
            dm_wave_add<LDS>(s_tab, out, key + 4, dup, lane);
        }
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < n_keys; k += kT) {
            const uint32_t v = s_tab[k];
            if (v) atomicAdd(&out[k], (unsigned long long)v);
        }
    }
}

}  // namespace

int oge_dup_metrics_impl(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, const oge_markdup_opts *opts, int32_t n_lib,
                         OgeDupMetrics *out) {
    if (n_lib < 1 || n_lib > 32768) return oge_fail(ctx, OGE_ERR_ARG, "dup_metrics: n_lib out of [1, 32768]");
    if (n && (!d_recs || !d_off)) return oge_fail(ctx, OGE_ERR_ARG, "dup_metrics: null argument");
    int rc = oge_rg_table_check(ctx, opts, "dup_metrics", n_lib);
    if (rc) return rc;
    memset(out, 0, (size_t)n_lib * sizeof *out);
    ctx->counters["dupmetrics_tile_records"] = kTile;
    ctx->counters["dupmetrics_lds_libs"] = kLdsLibs;
    // the table in workspaces of its own: a dedup in flight keeps its table
    OgeRgTable rg;
    if ((rc = oge_rg_table_upload(ctx, opts, "dm", &rg))) return rc;
    rg.split_k = 0;
    const uint32_t n_keys = (uint32_t)n_lib * kNC;
    unsigned long long *tab = (unsigned long long *)ctx->ws("dm_table", (size_t)n_keys * 8);
    if (!tab) return OGE_ERR_HIP;
    hipStream_t st = ctx->stream;
    OgeStage stage(ctx, "dup_metrics");
    OGE_HIP_TRY(ctx, hipMemsetAsync(tab, 0, (size_t)n_keys * 8, st));
    if (n) {
        const uint64_t ntiles = (n + kTile - 1) / kTile;
        const dim3 g((uint32_t)std::min<uint64_t>(ntiles, (uint64_t)ctx->cu_count() * 8));
        // a workgroup's u32 LDS sums: at most its tiles' records per key
        if ((ntiles / g.x + 1) * kTile >= (1ull << 32)) return oge_fail(ctx, OGE_ERR_LIMIT, "dup_metrics: too many records");
        if (n_lib <= kLdsLibs) hipLaunchKernelGGL(k_dm_count<true>, g, dim3(kT), 0, st, d_recs, d_off, n, rg, n_keys, tab);
        else hipLaunchKernelGGL(k_dm_count<false>, g, dim3(kT), 0, st, d_recs, d_off, n, rg, n_keys, tab);
        OGE_LAUNCH_CHECK(ctx);
    }
    stage.end();
    OGE_HIP_TRY(ctx, hipMemcpyAsync(out, tab, (size_t)n_keys * 8, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    return OGE_OK;
}

extern "C" {

int oge_dup_metrics_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, const oge_markdup_opts *opts, int32_t n_lib,
                        OgeDupMetrics *out) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!opts || !out) return oge_fail(ctx, OGE_ERR_ARG, "oge_dup_metrics_dev: null argument");
    OgeCall call(ctx, /*hold=*/false);
    return oge_dup_metrics_impl(ctx, d_recs, d_off, n, opts, n_lib, out);
}

int oge_dup_metrics(oge_ctx *ctx, const uint8_t *recs, uint64_t rec_bytes, const uint64_t *rec_off, uint64_t n, const oge_markdup_opts *opts,
                    int32_t n_lib, OgeDupMetrics *out) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!opts || !out || (n && (!recs || !rec_off))) return oge_fail(ctx, OGE_ERR_ARG, "oge_dup_metrics: null argument");
    (void)hipSetDevice(ctx->device);
    uint8_t *dr = (uint8_t *)ctx->ws("host_recs", rec_bytes + 16);
    uint64_t *dof = (uint64_t *)ctx->ws("host_off", (n + 1) * 8);
    if (!dr || !dof) return OGE_ERR_HIP;
    if (rec_bytes) OGE_HIP_TRY(ctx, hipMemcpyAsync(dr, recs, rec_bytes, hipMemcpyHostToDevice, ctx->stream));
    OGE_HIP_TRY(ctx, hipMemsetAsync(dr + rec_bytes, 0, 16, ctx->stream));
    if (n) OGE_HIP_TRY(ctx, hipMemcpyAsync(dof, rec_off, n * 8, hipMemcpyHostToDevice, ctx->stream));
    return oge_dup_metrics_dev(ctx, dr, dof, n, opts, n_lib, out);
}

}  // extern "C"
