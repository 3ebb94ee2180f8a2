// oge_ctx.h -- internal device context: stream, grow-only workspace, HIP-event stage timing.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <deque>
#include <map>
#include <string>
#include <vector>

#include "../../include/openge_hip.h"
#include "capi_common.h"

// the struct by a name of its own: the plain name is the host-buffer entry point's
using OgeDupMetrics = struct oge_dup_metrics;
using OgeDupSetsLib = struct oge_dup_sets_lib;

struct OgeStageTimer {
    hipEvent_t start, stop;
};

// The contig name table the last call of one side uploaded: the names back to back in workspace `ws_names`, their
// n_ref + 1 offsets in `ws_name_off` and, where `ws_slots` is set, the name hash of sam_parse.h; `counter` counts
// the uploads.  The next call with the same table uses it as it is.
struct OgeContigTable {
    const char *ws_names, *ws_name_off, *ws_slots, *counter;
    bool valid = false;
    std::string names;
    std::vector<uint32_t> name_off;
    const uint8_t *d_names = nullptr;
    const uint32_t *d_name_off = nullptr, *d_slots = nullptr;
    uint32_t n_slots = 0;
};

// The reference sequences the last oge_calmd call left on the device (calmd.hip): the FASTA they came from by path,
// size and mtime, the contig list they were laid out for (the names NUL-terminated one after the other), the
// sequences back to back in workspace "calmd_ref_bytes" with each contig's offset (-1: the FASTA lacks it) and
// length.  `uploads` counts the uploads of the context's lifetime (counter "calmd_ref_uploads").
struct OgeRefTable {
    bool valid = false;
    std::string path, names;
    uint64_t size = 0, n_ref = 0, uploads = 0;
    int64_t mtime = 0;
    const uint8_t *d_bytes = nullptr;
    const int64_t *d_off = nullptr, *d_len = nullptr;
};

struct oge_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    struct Buf { void *p = nullptr; size_t cap = 0; };
    std::map<std::string, Buf> bufs;
    // stage -> list of (start, stop) event pairs recorded during the last pipeline call
    std::map<std::string, std::vector<OgeStageTimer>> stage_events;
    std::deque<OgeStageTimer> event_pool;  // deque: an open OgeStage's pointer stays valid while stages nest
    size_t event_pool_used = 0;
    bool timing = true;
    int timing_hold = 0;  // > 0: a composite entry point (OgeCall with hold) keeps its sub-calls' stage events
    int deflate_search = OGE_DEFL_FAST;  // the GPU deflate's match search (oge_ctx_set_deflate_search)
    bool pool = false;  // allocate from the device's stream-ordered pool and keep freed memory in it
    hipStream_t side[4] = {nullptr, nullptr, nullptr, nullptr};  // extra streams a stage pipelines over
    hipStream_t side_stream(int i);
    int ncu = 0;  // compute units of `device` (persistent grids), looked up once per context
    int cu_count() {
        if (!ncu) {
            int c = 0;
            (void)hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, device);
            ncu = c > 0 ? c : 256;
        }
        return ncu;
    }
    void *alloc(size_t bytes);
    void release(void *p);
    // the last count-only record walk: its converged chunk starts and offsets stay in the "rec_walk"
    // workspace, so the offsets call that follows (same stream and range) goes straight to the fill: from
    // the count walk's record slots (rel, a trusted internal caller's `keep`), else a second walk that is
    // checked to join and count the same
    struct RecWalk {
        const void *stream = nullptr;
        uint64_t base = 0, limit = 0, end = 0, n = 0, C = 0, x = 0;
        int32_t n_ref = 0;
        const uint16_t *rel = nullptr;
        uint32_t sc = 0;
    } recwalk;
    // the inflate's phase-1 bitmap buffer and how many of its bytes are known clear (inflate_lane.hip)
    const void *infl_clean_ptr = nullptr;
    uint64_t infl_clean_bytes = 0, infl_clean_next = 0;
    const uint8_t *bai_ptr = nullptr;  // the index image of the last call that built one (workspace "bai_image")
    uint64_t bai_bytes = 0;
    // the binary reference list of the BAM file the last oge_bam_stats_dev / _coverage_dev / _count_dev call
    // parsed (oge_ctx_last_refs): names NUL-terminated one after the other
    bool refs_valid = false;
    std::string ref_names;
    std::vector<int32_t> ref_lens;
    // the contig tables the last oge_text_* and the last oge_sam_* call uploaded (oge_contig_table), and what the
    // last oge_sam_parse call returned (host memory, valid until the next one)
    OgeContigTable text_table{"text_names", "text_name_off", nullptr, "text_table_uploads"};
    OgeContigTable sam_table{"sam_names", "sam_name_off", "sam_slots", "sam_table_uploads"};
    OgeContigTable targets_table{"tg_names", "tg_name_off", nullptr, "targets_table_uploads"};  // oge_targets_dev's
    OgeRefTable calmd_ref;              // oge_calmd_dev's reference
    std::vector<OgeDupMetrics> dm_out;  // what the last oge_bam_dup_metrics_dev call returned
    std::string dm_names;
    std::vector<OgeDupSetsLib> ds_out;  // what the last oge_bam_dup_sets_dev call returned
    std::vector<uint64_t> ds_hist;
    std::vector<uint8_t> sam_out_recs, sam_out_warn;
    std::vector<uint64_t> sam_out_off;
    std::map<std::string, uint64_t> counters;  // per call: work counts a stage reports (oge_ctx_counter)
    bool last_scan_generic = false;  // realign scan fell back to the byte-wise kernel
    double scan_t[3] = {0, 0, 0};    // realign scan host timings: validate, upload, device + download

    // Grow-only named scratch buffer; contents are undefined between calls.
    void *ws(const char *name, size_t bytes);
    // Loaned scratch: while a loan is active (lend), scratch() bump-allocates from the caller's buffer
    // (the fused pipeline lends its output arena, which is only written by the final gather), else it
    // is ws().  Only for buffers that are dead before the lender writes its buffer.
    uint8_t *loan_base = nullptr;
    size_t loan_cap = 0, loan_used = 0;
    void *scratch(const char *name, size_t bytes);
    void lend(void *p, size_t bytes) { loan_base = (uint8_t *)p; loan_cap = p ? bytes : 0; loan_used = 0; }
    void end_loan() { loan_base = nullptr; loan_cap = loan_used = 0; }
    bool in_composite() const { return timing_hold > 0; }  // under a composite entry point's OgeCall
    void reset_timing();
};

// One timed stage of a context's stream, open from begin() to end() or the end of the scope, whichever comes
// first: an error return in between still records the stop event.  begin() closes the stage that is open, so a
// function that runs its stages one after another keeps one object; a stage nested in another takes its own.
// With ctx->timing off nothing is recorded.
class OgeStage {
public:
    explicit OgeStage(oge_ctx *c) : ctx(c) {}
    OgeStage(oge_ctx *c, const char *name) : ctx(c) { begin(name); }
    OgeStage(const OgeStage &) = delete;
    OgeStage &operator=(const OgeStage &) = delete;
    ~OgeStage() { end(); }
    void begin(const char *name);
    void end();

private:
    oge_ctx *ctx;
    OgeStageTimer *open = nullptr;
};

// An entry point's prologue, after its argument checks: makes the context's device current and drops the last
// call's stage events and counters (not under a composite caller, which keeps them).  With `hold` the entry
// point is itself composite: the entry points it calls add to its stages until it returns.
class OgeCall {
public:
    OgeCall(oge_ctx *c, bool hold);
    OgeCall(const OgeCall &) = delete;
    OgeCall &operator=(const OgeCall &) = delete;
    ~OgeCall() { ctx->timing_hold -= held; }

private:
    oge_ctx *ctx;
    int held;
};

// Checks the contig fields of `o` (errors are prefixed with `who`) and, with a table, makes it the one on the
// device: uploaded only when it differs from what the table's last call left there.
int oge_contig_table(oge_ctx *ctx, OgeContigTable *tab, const oge_text_opts *o, const char *who);

#define OGE_HIP_TRY(ctx, expr)                                                                     \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            std::string _m = std::string(#expr) + ": " + hipGetErrorString(_e);                   \
            return oge_fail((ctx), OGE_ERR_HIP, _m.c_str());                                       \
        }                                                                                          \
    } while (0)

// Launch-error check after a kernel launch (names the launch site).
#define OGE_STR2(x) #x
#define OGE_STR(x) OGE_STR2(x)
#define OGE_LAUNCH_CHECK(ctx)                                                                      \
    do {                                                                                           \
        hipError_t _e = hipGetLastError();                                                         \
        if (_e != hipSuccess)                                                                      \
            return oge_fail((ctx), OGE_ERR_HIP,                                                    \
                            (std::string("kernel launch at " __FILE__ ":" OGE_STR(__LINE__) ": ") + \
                             hipGetErrorString(_e)).c_str());                                      \
    } while (0)

static inline uint32_t oge_ceil_div(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

// ---- device primitives (prims.hip) ----
// In-place-or-not exclusive scans. `out` may alias `in`.
int oge_exclusive_scan_u32(oge_ctx *ctx, const uint32_t *in, uint32_t *out, uint64_t n);
int oge_exclusive_scan_u64(oge_ctx *ctx, const uint64_t *in, uint64_t *out, uint64_t n);
// out[0..n] = the exclusive scan of the record sizes in sorted keys' payload bits (key >> 50), out[n] = their
// total, in one reduce-then-scan (keys and out 16-byte aligned; returns 1 without work otherwise)
int oge_offsets_from_keys(oge_ctx *ctx, const uint64_t *keys, uint64_t n, uint64_t *out);
// Stable LSD radix sort of (key, value) pairs on key bits selected by `bit_mask` (only bits set
// in the mask are sorted; set bits are grouped into digit passes of <= 8 contiguous bits).
// Buffers: keys/vals hold the input; ktmp/vtmp scratch of the same size.  On return *kout/*vout
// point at whichever pair of buffers holds the result.  vals == NULL sorts keys only.
int oge_radix_sort_pairs(oge_ctx *ctx, uint64_t *keys, uint32_t *vals, uint64_t *ktmp, uint32_t *vtmp,
                         uint64_t n, uint64_t bit_mask, uint64_t **kout, uint32_t **vout);
// OR / AND reduction of a u64 array (for choosing the varying key bits).
int oge_reduce_or_and_u64(oge_ctx *ctx, const uint64_t *in, uint64_t n, uint64_t mask, uint64_t *or_out, uint64_t *and_out);

// ---- BGZF framing index on the device (inflate.hip) ----
struct OgeBgzfIndex {
    uint64_t *d0 = nullptr, *d1 = nullptr, *uoff = nullptr;  // nblk, nblk, nblk + 1 entries (device)
    uint32_t *crc = nullptr;
    uint64_t nblk = 0, total = 0;
};
// 0 = ok, 1 = candidates are not an exact block chain (use the host walk), < 0 = error
int oge_bgzf_index_ws(oge_ctx *ctx, const uint8_t *d_z, uint64_t zbytes, OgeBgzfIndex *ix);
// The blocks that start in [s, own) of d_z (zbytes >= own bytes readable: the last block may end past
// own): s = kIndexFirst takes the range's first candidate (*s_used), else s must be a candidate; the
// chain must be exact from s to its last block, whose end (>= own) goes to *xend.  0 = ok, 1 = not an
// exact chain, 2 = no candidate in the range (or s >= own: no block), < 0 = error.
constexpr uint64_t kIndexFirst = ~0ull;
int oge_bgzf_index_range_ws(oge_ctx *ctx, const uint8_t *d_z, uint64_t zbytes, uint64_t s, uint64_t own, OgeBgzfIndex *ix,
                            uint64_t *s_used, uint64_t *xend);
// The record walk of oge_bam_record_offsets_dev generalised to a window: records that start in
// [start, limit) of d (bytes readable up to bufend, so the last record may end past limit); at_end says
// bufend is the end of the stream (a guess chain may stop there).  *exit = the end of the last record
// (= the first record start at or past limit); d_off (cap >= n + 1) gets the offsets and d_off[n] = *exit.
// keep (a count call of an internal caller that fills next, on the same unchanged stream): the walk also
// stores each chunk's record positions (in rel_buf when it holds rel_cap >= the slots' bytes, else
// workspace "rec_rel"), and the fill call expands them instead of walking the stream again.
int oge_record_walk(oge_ctx *ctx, const uint8_t *d, uint64_t start, uint64_t limit, uint64_t bufend, bool at_end, int32_t n_ref,
                    uint64_t *d_off, uint64_t cap, uint64_t *n_out, uint64_t *exit, bool keep = false, void *rel_buf = nullptr,
                    uint64_t rel_cap = 0);
// The first plausible record start in [0, lim) of d (bufend readable) as k_rec_guess judges it, or ~0.
int oge_record_guess(oge_ctx *ctx, const uint8_t *d, uint64_t lim, uint64_t bufend, bool at_end, int32_t n_ref, uint64_t *out);
// the framing walk of a host buffer with T threads (inflate.hip); false: use oge_bgzf_index
bool oge_bgzf_index_host_mt(const uint8_t *z, uint64_t zbytes, int T, std::vector<uint64_t> &d0, std::vector<uint64_t> &d1,
                            std::vector<uint64_t> &uoff, std::vector<uint32_t> &crc);
// lane-per-block BGZF inflate (inflate_lane.hip); err/zpow as in oge_bgzf_inflate_dev
int oge_inflate_lanes(oge_ctx *ctx, const uint8_t *d_z, uint64_t zbytes, const uint64_t *d0, const uint64_t *d1,
                      const uint64_t *uoff, const uint32_t *crc, uint64_t nblk, uint8_t *out, uint32_t *err,
                      const uint32_t *zpow);

// ---- BAM index (bai.hip) ----
// oge_bai_build_dev without the argument checks and the timing reset (the chain calls it under its own hold)
int oge_bai_build_impl(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, int32_t n_ref, uint64_t stream_base,
                       const uint64_t *d_uoff, const uint64_t *d_cstart, uint64_t nblk, const uint8_t **d_bai, uint64_t *bai_bytes);
// file offsets of the indexed blocks of d_z (nblk + 1 entries, workspace "bai_cstart"): cstart[nblk] = the end
// of the last one; the oge_bai_build_impl call that consumes the table releases it
int oge_bai_cstart(oge_ctx *ctx, const uint8_t *d_z, const uint64_t *d0, const uint64_t *d1, uint64_t nblk, uint64_t **cstart_out);

// ---- stats / coverage (qc.hip) ----
// oge_stats_dev / oge_coverage_dev without the context checks and the timing reset (the whole-file entry
// points call them under their own hold)
int oge_qc_stats_impl(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, uint32_t want, oge_bam_stats *out,
                      const uint32_t **d_len, const uint64_t **d_len_count);
int oge_qc_coverage_impl(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, int32_t n_ref, const int32_t *ref_len,
                         int32_t binsize, const uint32_t **d_bins, uint64_t *n_skipped, int32_t *overflow);

// ---- realignment targets (targets.hip) ----
// oge_targets_dev without the context checks and the timing reset (oge_bam_targets_dev calls it under its hold)
int oge_targets_impl(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, int32_t n_ref, const int32_t *ref_len,
                     const char *ref_names, uint64_t names_bytes, const oge_targets_opts *opts, oge_targets_result *result,
                     const oge_target **d_targets, const uint8_t **d_text);

// ---- NM / MD tags (calmd.hip) ----
// oge_calmd_dev without the context checks and the timing reset (oge_bam_calmd_dev calls it under its hold)
int oge_calmd_impl(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, int32_t n_ref, const char *ref_names,
                   uint64_t names_bytes, const char *fasta_path, const oge_calmd_opts *opts, oge_calmd_result *result, const uint8_t **d_out,
                   const uint64_t **d_out_off);

// ---- duplication metrics (dupmetrics.hip) ----
// oge_dup_metrics_dev without the context checks and the timing reset (oge_bam_dup_metrics_dev calls it under its hold)
int oge_dup_metrics_impl(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, const oge_markdup_opts *opts, int32_t n_lib,
                         OgeDupMetrics *out);

// ---- duplicate sets (dupsets.hip) ----
// oge_dup_sets_dev without the context checks and the timing reset (oge_bam_dup_sets_dev calls it under its hold)
int oge_dup_sets_impl(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, const oge_markdup_opts *opts, int64_t distance,
                      int32_t n_lib, OgeDupSetsLib *out_per_lib, uint64_t *hist);

// ---- multi-GPU internals (dist.hip)
oge_ctx *oge_comm_ctx(oge_comm *comm);
// in place: v[0..count) = the sum over the communicator's ranks (collective, host values)
int oge_comm_sum_u64(oge_comm *comm, uint64_t *v, int count);
// host allgather (every rank `bytes` bytes, out = G * bytes in rank order) and the device all-to-all-v,
// recorded under `tag` in the communicator's exchange statistics
int oge_comm_allgather(oge_comm *comm, const char *tag, const void *in, void *out, size_t bytes);
int oge_comm_alltoallv_dev(oge_comm *comm, const char *tag, const void *send, const uint64_t *sbytes, const uint64_t *soff, void *recv,
                           const uint64_t *rbytes, const uint64_t *roff);
void oge_comm_reset_stats(oge_comm *comm);
// shard.hip: this rank's records of one BGZF BAM file decoded by byte range (see oge_bgzf_decode_shard);
// *X / *xoff are workspace ("pipe_x", "pipe_xoff"), *header the raw BAM header bytes.  Collective.
int oge_decode_shard(oge_comm *comm, const uint8_t *d_z, uint64_t zbytes, uint64_t own, uint8_t **X, uint64_t **xoff, uint64_t *n,
                     std::vector<uint8_t> *header);
