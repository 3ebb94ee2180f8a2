// sam_parse.hip -- SAM text resident in HBM -> BAM records in HBM (SAM input of every command; the reference's
// util/sam_reader.cpp; DESIGN.md section 22, include/openge_hip.h).  The inverse of sam.hip.
//
//   lines  k_sam_count   one wave per tile of 4096 text bytes: newlines by ballot and popcount
//          scan          oge_exclusive_scan_u64 over the tile counts
//          k_sam_fill    the same walk, each newline stores the start of the next line at its rank; no atomics
//   size   k_sam_size    one wave per line, kWaveLines consecutive lines per wave: tabs by ballot, every field
//                        handled when its closing tab is met; the exact record length, error code, warning bit
//                        and host mark (a line with an f or B tag); the lowest failing line by one atomicMin per
//                        wave that has one
//   scan                 oge_exclusive_scan_u64 over the n + 1 lengths, in place: the record offsets
//   emit   k_sam_emit    the same walk with the stores: every byte of a record once, at its final offset.  A host
//                        marked line gets no f or B tag bytes: its record is not complete until the caller has
//                        copied the host's record (oge_sam_host_record) over it; nothing is stored outside it
// The per-line code is sam_parse.h, shared with a host program that runs it lane by lane.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "bam_layout.h"
#include "bamio.h"
#include "oge_ctx.h"
#include "sam_host.h"
#include "sam_parse.h"

namespace {

constexpr int kT = 256;
constexpr int kWaves = kT / 64;
constexpr int kWaveLines = 4;  // consecutive lines of one wave
constexpr int kBlockLines = kWaves * kWaveLines;
constexpr unsigned long long kNone = ~0ull;

struct SamAcc {
    unsigned long long n_host, first_bad;
};

__device__ __forceinline__ uint64_t uni64(uint64_t v) {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}

__global__ __launch_bounds__(kT) void k_sam_count(const uint8_t *__restrict__ text, uint64_t tile0, uint64_t n_tiles, uint64_t lo, uint64_t bytes,
                                                  uint64_t *__restrict__ cnt) {
    const uint64_t w = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (w > n_tiles) return;
    const uint32_t c = w < n_tiles ? oge_sam_tile<false>(text, (tile0 + w) * OGE_SAM_TILE, lo, bytes, 0, nullptr, 0) : 0;
    if ((threadIdx.x & 63) == 0) cnt[w] = c;
}

__global__ __launch_bounds__(kT) void k_sam_fill(const uint8_t *__restrict__ text, uint64_t tile0, uint64_t n_tiles, uint64_t lo, uint64_t bytes,
                                                 const uint64_t *__restrict__ base, uint64_t *__restrict__ line_off, uint64_t n) {
    const uint64_t w = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (w >= n_tiles) return;
    oge_sam_tile<true>(text, (tile0 + w) * OGE_SAM_TILE, lo, bytes, uni64(base[w]), line_off, n);
}

__global__ __launch_bounds__(kT) void k_sam_size(const uint8_t *__restrict__ text, const uint64_t *__restrict__ line_off, uint64_t n, OgeSamParams sp,
                                                 uint64_t *__restrict__ len_out, uint8_t *__restrict__ mark, uint8_t *__restrict__ warn,
                                                 uint8_t *__restrict__ err, SamAcc *__restrict__ acc) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t i0 = ((uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6)) * kWaveLines;
    if (i0 == 0 && lane == 0) len_out[n] = 0;
    unsigned long long bad = kNone, hosts = 0;
    for (int k = 0; k < kWaveLines; ++k) {
        const uint64_t i = i0 + k;
        if (i >= n) break;
        const uint64_t a = uni64(line_off[i]), z = uni64(line_off[i + 1]) - 1;
        OgeSamRec r;
        if (z - a > OGE_SAM_MAX_LINE) {
            memset(&r, 0, sizeof r);
            r.err = OGE_SAM_E_LONG;
        } else {
            r = oge_sam_line<false>(text + a, (uint32_t)(z - a), sp, nullptr);
        }
        if (lane == 0) {
            len_out[i] = r.err ? 0 : r.len;
            mark[i] = r.err ? 0 : (uint8_t)r.host;
            warn[i] = r.err ? 0 : (uint8_t)r.warn;
            err[i] = (uint8_t)r.err;
        }
        if (r.err && bad == kNone) bad = i;
        hosts += !r.err && r.host;
    }
    if (lane == 0) {
        if (bad != kNone) atomicMin(&acc->first_bad, bad);
        if (hosts) atomicAdd(&acc->n_host, hosts);
    }
}

__global__ __launch_bounds__(kT) void k_sam_emit(const uint8_t *__restrict__ text, const uint64_t *__restrict__ line_off,
                                                 const uint64_t *__restrict__ rec_off, uint64_t first, uint64_t count, OgeSamParams sp,
                                                 uint8_t *__restrict__ out) {
    const uint64_t i0 = first + ((uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6)) * kWaveLines, end = first + count;
    const uint64_t base = rec_off[first];
    for (int k = 0; k < kWaveLines; ++k) {
        const uint64_t i = i0 + k;
        if (i >= end) break;
        const uint64_t ra = uni64(rec_off[i]), rz = uni64(rec_off[i + 1]);
        if (rz <= ra) continue;
        const uint64_t a = uni64(line_off[i]), z = uni64(line_off[i + 1]) - 1;
        oge_sam_line<true>(text + a, (uint32_t)(z - a), sp, out + (ra - base));
    }
}

// the kernels' parameters, with the contig table and its hash on the device
int device_table(oge_ctx *ctx, const oge_text_opts *o, const char *who, OgeSamParams *sp) {
    const OgeContigTable &t = ctx->sam_table;
    const int rc = oge_contig_table(ctx, &ctx->sam_table, o, who);
    if (rc) return rc;
    sp->n_ref = o->n_ref;
    sp->hmask = t.n_slots - 1;
    sp->names = t.d_names;
    sp->name_off = t.d_name_off;
    sp->slots = t.d_slots;
    return OGE_OK;
}

int lines_impl(oge_ctx *ctx, const uint8_t *d_text, uint64_t bytes, uint64_t body_off, uint64_t *d_line_off, uint64_t cap, uint64_t *n_out) {
    *n_out = 0;
    if (body_off > bytes) return oge_fail(ctx, OGE_ERR_ARG, "oge_sam_lines_dev: body_off is past the text");
    if (bytes > body_off && !d_text) return oge_fail(ctx, OGE_ERR_ARG, "oge_sam_lines_dev: null argument");
    if ((uintptr_t)d_text & 3) return oge_fail(ctx, OGE_ERR_ARG, "oge_sam_lines_dev: the text is not 4-byte aligned");
    OgeStage stage(ctx, "sam_lines");
    hipStream_t st = ctx->stream;
    const uint64_t tile0 = body_off / OGE_SAM_TILE;
    const uint64_t n_tiles = bytes > body_off ? (bytes + OGE_SAM_TILE - 1) / OGE_SAM_TILE - tile0 : 0;
    uint64_t *cnt = (uint64_t *)ctx->ws("sam_tile_cnt", (n_tiles + 1) * 8);
    if (!cnt) return OGE_ERR_HIP;
    hipLaunchKernelGGL(k_sam_count, dim3(oge_ceil_div(n_tiles + 1, kWaves)), dim3(kT), 0, st, d_text, tile0, n_tiles, body_off, bytes, cnt);
    OGE_LAUNCH_CHECK(ctx);
    int rc = oge_exclusive_scan_u64(ctx, cnt, cnt, n_tiles + 1);
    if (rc) return rc;
    uint64_t newlines = 0;
    uint8_t last = '\n';
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&newlines, cnt + n_tiles, 8, hipMemcpyDeviceToHost, st));
    if (bytes > body_off) OGE_HIP_TRY(ctx, hipMemcpyAsync(&last, d_text + bytes - 1, 1, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    const bool open_end = bytes > body_off && last != '\n';  // a last line without its newline is a line
    const uint64_t n = newlines + (open_end ? 1 : 0);
    *n_out = n;
    if (n >= 0xFFFFFFFFull) return oge_fail(ctx, OGE_ERR_LIMIT, "oge_sam_lines_dev: more than 2^32-2 lines");
    if (!d_line_off) return OGE_OK;
    if (cap < n + 1) return oge_fail(ctx, OGE_ERR_LIMIT, "oge_sam_lines_dev: d_line_off holds fewer than n + 1 entries");
    if (n_tiles) {
        hipLaunchKernelGGL(k_sam_fill, dim3(oge_ceil_div(n_tiles, kWaves)), dim3(kT), 0, st, d_text, tile0, n_tiles, body_off, bytes, cnt, d_line_off, n);
        OGE_LAUNCH_CHECK(ctx);
    }
    const uint64_t ends[2] = {body_off, bytes + 1};
    OGE_HIP_TRY(ctx, hipMemcpyAsync(d_line_off, &ends[0], 8, hipMemcpyHostToDevice, st));
    if (open_end) OGE_HIP_TRY(ctx, hipMemcpyAsync(d_line_off + n, &ends[1], 8, hipMemcpyHostToDevice, st));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    return OGE_OK;
}

int size_impl(oge_ctx *ctx, const uint8_t *d_text, const uint64_t *d_line_off, uint64_t n, const oge_text_opts *opts, uint64_t *d_rec_off,
              uint8_t *d_host_mark, uint8_t *d_warn, uint64_t *total, uint64_t *n_host) {
    *total = 0;
    *n_host = 0;
    int rc = oge_contig_table(ctx, nullptr, opts, "oge_sam_size_dev");
    if (rc) return rc;
    ctx->counters["sam_wave_lines"] = kWaveLines;
    ctx->counters["sam_block_lines"] = kBlockLines;
    if (!d_rec_off || (n && (!d_text || !d_line_off || !d_host_mark || !d_warn))) return oge_fail(ctx, OGE_ERR_ARG, "oge_sam_size_dev: null argument");
    if (n >= 0xFFFFFFFFull) return oge_fail(ctx, OGE_ERR_LIMIT, "oge_sam_size_dev: more than 2^32-2 lines");
    OgeSamParams sp;
    rc = device_table(ctx, opts, "oge_sam_size_dev", &sp);
    if (rc) return rc;
    OgeStage stage(ctx, "sam_size");
    hipStream_t st = ctx->stream;
    SamAcc *acc = (SamAcc *)ctx->ws("sam_acc", sizeof(SamAcc));
    uint8_t *d_err = (uint8_t *)ctx->ws("sam_err", n + 1);
    // the kernel's results go to workspace and reach the caller's arrays only when every line parsed: an error
    // leaves d_rec_off, d_host_mark and d_warn as they were
    uint64_t *w_len = (uint64_t *)ctx->ws("sam_len", (n + 1) * 8);
    uint8_t *w_mark = (uint8_t *)ctx->ws("sam_size_marks", 2 * n + 2), *w_warn = w_mark + n + 1;
    if (!acc || !d_err || !w_len || !w_mark) return OGE_ERR_HIP;
    SamAcc h = {0, kNone};
    OGE_HIP_TRY(ctx, hipMemcpyAsync(acc, &h, sizeof h, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_sam_size, dim3(std::max<uint32_t>(1, oge_ceil_div(n, kBlockLines))), dim3(kT), 0, st, d_text, d_line_off, n, sp, w_len,
                       w_mark, w_warn, d_err, acc);
    OGE_LAUNCH_CHECK(ctx);
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&h, acc, sizeof h, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (h.first_bad != kNone) {
        // the line's number in the file: the header's lines in front of the body count
        uint8_t code = 0;
        uint64_t lo[2] = {0, 0}, body = 0;
        OGE_HIP_TRY(ctx, hipMemcpyAsync(&code, d_err + h.first_bad, 1, hipMemcpyDeviceToHost, st));
        OGE_HIP_TRY(ctx, hipMemcpyAsync(lo, d_line_off + h.first_bad, 16, hipMemcpyDeviceToHost, st));
        OGE_HIP_TRY(ctx, hipMemcpyAsync(&body, d_line_off, 8, hipMemcpyDeviceToHost, st));
        OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
        std::string head(body, '\0');
        if (body) OGE_HIP_TRY(ctx, hipMemcpy(&head[0], d_text, body, hipMemcpyDeviceToHost));
        const uint64_t line_no = 1 + (uint64_t)std::count(head.begin(), head.end(), '\n') + h.first_bad;
        std::string msg = "sam: line " + std::to_string(line_no) + ": " + oge_sam_error_text(code);
        if (code == OGE_SAM_E_RNAME) {  // the reference's message (sam_reader.cpp:360)
            std::string line(std::min<uint64_t>(lo[1] - 1 - lo[0], 1 << 16), '\0');
            if (!line.empty()) OGE_HIP_TRY(ctx, hipMemcpy(&line[0], d_text + lo[0], line.size(), hipMemcpyDeviceToHost));
            size_t a = line.find('\t');
            a = a == std::string::npos ? a : line.find('\t', a + 1);
            if (a != std::string::npos) msg = "Rname " + line.substr(a + 1, line.find('\t', a + 1) - a - 1) + " missing from sequence dictionary (" + msg + ")";
        }
        ctx->counters["sam_bad_line"] = line_no;
        ctx->counters["sam_bad_code"] = code;
        return oge_fail(ctx, OGE_ERR_ARG, msg.c_str());
    }
    rc = oge_exclusive_scan_u64(ctx, w_len, d_rec_off, n + 1);
    if (rc) return rc;
    if (n) {
        OGE_HIP_TRY(ctx, hipMemcpyAsync(d_host_mark, w_mark, n, hipMemcpyDeviceToDevice, st));
        OGE_HIP_TRY(ctx, hipMemcpyAsync(d_warn, w_warn, n, hipMemcpyDeviceToDevice, st));
    }
    uint64_t tot = 0;
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&tot, d_rec_off + n, 8, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    *total = tot;
    *n_host = h.n_host;
    ctx->counters["sam_host_lines"] = h.n_host;
    return OGE_OK;
}

int emit_impl(oge_ctx *ctx, const uint8_t *d_text, const uint64_t *d_line_off, const uint64_t *d_rec_off, uint64_t first, uint64_t count,
              const oge_text_opts *opts, uint8_t *d_recs, uint64_t cap) {
    int rc = oge_contig_table(ctx, nullptr, opts, "oge_sam_emit_dev");
    if (rc) return rc;
    ctx->counters["sam_wave_lines"] = kWaveLines;
    ctx->counters["sam_block_lines"] = kBlockLines;
    if (!d_rec_off || (count && (!d_text || !d_line_off))) return oge_fail(ctx, OGE_ERR_ARG, "oge_sam_emit_dev: null argument");
    if (first + count < first || first + count >= 0xFFFFFFFFull) return oge_fail(ctx, OGE_ERR_LIMIT, "oge_sam_emit_dev: line range");
    if (!count) return OGE_OK;
    hipStream_t st = ctx->stream;
    uint64_t ends[2] = {0, 0};
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&ends[0], d_rec_off + first, 8, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&ends[1], d_rec_off + first + count, 8, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (ends[1] < ends[0]) return oge_fail(ctx, OGE_ERR_ARG, "oge_sam_emit_dev: record offsets decrease");
    if (ends[1] - ends[0] > cap) return oge_fail(ctx, OGE_ERR_LIMIT, "oge_sam_emit_dev: the record buffer is smaller than the range's records");
    if (ends[1] == ends[0]) return OGE_OK;
    if (!d_recs) return oge_fail(ctx, OGE_ERR_ARG, "oge_sam_emit_dev: null argument");
    OgeSamParams sp;
    rc = device_table(ctx, opts, "oge_sam_emit_dev", &sp);
    if (rc) return rc;
    OgeStage stage(ctx, "sam_emit");
    hipLaunchKernelGGL(k_sam_emit, dim3(oge_ceil_div(count, kBlockLines)), dim3(kT), 0, st, d_text, d_line_off, d_rec_off, first, count, sp, d_recs);
    OGE_LAUNCH_CHECK(ctx);
    return OGE_OK;
}

}  // namespace

extern "C" {

int oge_sam_lines_dev(oge_ctx *ctx, const uint8_t *d_text, uint64_t bytes, uint64_t body_off, uint64_t *d_line_off, uint64_t cap, uint64_t *n) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!n) return oge_fail(ctx, OGE_ERR_ARG, "oge_sam_lines_dev: null argument");
    OgeCall call(ctx, /*hold=*/false);
    return lines_impl(ctx, d_text, bytes, body_off, d_line_off, cap, n);
}

int oge_sam_size_dev(oge_ctx *ctx, const uint8_t *d_text, const uint64_t *d_line_off, uint64_t n, const oge_text_opts *opts, uint64_t *d_rec_off,
                     uint8_t *d_host_mark, uint8_t *d_warn, uint64_t *total, uint64_t *n_host) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!total || !n_host) return oge_fail(ctx, OGE_ERR_ARG, "oge_sam_size_dev: null argument");
    OgeCall call(ctx, /*hold=*/false);
    return size_impl(ctx, d_text, d_line_off, n, opts, d_rec_off, d_host_mark, d_warn, total, n_host);
}

int oge_sam_emit_dev(oge_ctx *ctx, const uint8_t *d_text, const uint64_t *d_line_off, const uint64_t *d_rec_off, uint64_t first, uint64_t count,
                     const oge_text_opts *opts, uint8_t *d_recs, uint64_t cap) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    OgeCall call(ctx, /*hold=*/false);
    return emit_impl(ctx, d_text, d_line_off, d_rec_off, first, count, opts, d_recs, cap);
}

int oge_sam_host_record(const char *line, uint64_t len, const oge_text_opts *opts, uint8_t *buf, uint64_t cap, uint64_t *len_out) {
    if (!line || !len_out) return oge_fail(nullptr, OGE_ERR_ARG, "oge_sam_host_record: null argument");
    const int rc = oge_contig_table(nullptr, nullptr, opts, "oge_sam_host_record");
    if (rc) return rc;
    std::vector<uint8_t> rec;
    std::string err;
    bool warn = false;
    if (!oge_sam_record_host((const uint8_t *)line, len, opts, rec, &warn, err)) return oge_fail(nullptr, OGE_ERR_ARG, ("sam: " + err).c_str());
    *len_out = rec.size();
    if (rec.size() > cap || !buf) return oge_fail(nullptr, OGE_ERR_LIMIT, "oge_sam_host_record: the buffer is too small");
    memcpy(buf, rec.data(), rec.size());
    return OGE_OK;
}

int oge_sam_header(const char *text, uint64_t bytes, uint64_t *header_len, uint64_t *header_lines) {
    if ((bytes && !text) || !header_len) return oge_fail(nullptr, OGE_ERR_ARG, "oge_sam_header: null argument");
    uint64_t p = 0, lines = 0;
    while (p < bytes && text[p] == '@') {
        const void *nl = memchr(text + p, '\n', bytes - p);
        p = nl ? (uint64_t)((const char *)nl - text) + 1 : bytes;
        ++lines;
    }
    *header_len = p;
    if (header_lines) *header_lines = lines;
    return OGE_OK;
}

int oge_sam_parse(oge_ctx *ctx, const char *text, uint64_t bytes, uint64_t *header_len, const uint8_t **recs, uint64_t *rec_bytes,
                  const uint64_t **rec_off, uint64_t *n_out, const uint8_t **warn) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if ((bytes && !text) || !header_len || !recs || !rec_bytes || !rec_off || !n_out) return oge_fail(ctx, OGE_ERR_ARG, "oge_sam_parse: null argument");
    *header_len = *rec_bytes = *n_out = 0;
    *recs = nullptr;
    *rec_off = nullptr;
    if (warn) *warn = nullptr;
    OgeCall call(ctx, /*hold=*/true);
    hipStream_t st = ctx->stream;
    uint64_t body = 0, header_lines = 0;
    oge_sam_header(text, bytes, &body, &header_lines);
    // the contig table: the @SQ names as the header model reads them (BamHeaderModel::parse, the model every
    // reader of the module layer feeds), so refIDs agree with the header the caller parses from the same text
    std::string names;
    std::vector<uint32_t> name_off(1, 0);
    {
        oge::BamHeaderModel hm;
        std::string herr;
        if (!hm.parse(std::string(text, body), herr)) return oge_fail(ctx, OGE_ERR_ARG, ("sam: header: " + herr).c_str());
        for (auto &sq : hm.sq) {
            names += sq.name;
            name_off.push_back((uint32_t)names.size());
        }
    }
    oge_text_opts opts = {0, 0, 0, (int32_t)name_off.size() - 1, names.data(), name_off.data()};
    uint8_t *d_text = (uint8_t *)ctx->ws("sam_text", bytes + 16);
    if (!d_text) return OGE_ERR_HIP;
    if (bytes) OGE_HIP_TRY(ctx, hipMemcpyAsync(d_text, text, bytes, hipMemcpyHostToDevice, st));
    uint64_t n = 0;
    int rc = lines_impl(ctx, d_text, bytes, body, nullptr, 0, &n);
    if (rc) return rc;
    uint64_t *d_lo = (uint64_t *)ctx->ws("sam_line_off", (n + 1) * 8);
    uint64_t *d_ro = (uint64_t *)ctx->ws("sam_rec_off", (n + 1) * 8);
    uint8_t *d_mark = (uint8_t *)ctx->ws("sam_mark", n + 1);
    uint8_t *d_warn = (uint8_t *)ctx->ws("sam_warn", n + 1);
    if (!d_lo || !d_ro || !d_mark || !d_warn) return OGE_ERR_HIP;
    rc = lines_impl(ctx, d_text, bytes, body, d_lo, n + 1, &n);
    if (rc) return rc;
    uint64_t total = 0, n_host = 0;
    rc = size_impl(ctx, d_text, d_lo, n, &opts, d_ro, d_mark, d_warn, &total, &n_host);
    if (rc) return rc;
    uint8_t *d_recs = (uint8_t *)ctx->ws("sam_recs", total + 16);
    if (!d_recs) return OGE_ERR_HIP;
    rc = emit_impl(ctx, d_text, d_lo, d_ro, 0, n, &opts, d_recs, total);
    if (rc) return rc;
    // results in locals first: a host line that fails leaves the last call's results and the caller's pointers alone
    std::vector<uint8_t> out(total + 16, 0), w(n), mark(n);
    std::vector<uint64_t> ro(n + 1, 0), lo;
    if (total) OGE_HIP_TRY(ctx, hipMemcpyAsync(out.data(), d_recs, total, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipMemcpyAsync(ro.data(), d_ro, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    if (n) OGE_HIP_TRY(ctx, hipMemcpyAsync(w.data(), d_warn, n, hipMemcpyDeviceToHost, st));
    if (n_host) {
        lo.resize(n + 1);
        OGE_HIP_TRY(ctx, hipMemcpyAsync(mark.data(), d_mark, n, hipMemcpyDeviceToHost, st));
        OGE_HIP_TRY(ctx, hipMemcpyAsync(lo.data(), d_lo, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    }
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    for (uint64_t i = 0; n_host && i < n; ++i) {
        if (!mark[i]) continue;
        std::vector<uint8_t> rec;
        std::string err;
        bool wn = false;
        const bool ok = oge_sam_record_host((const uint8_t *)text + lo[i], lo[i + 1] - 1 - lo[i], &opts, rec, &wn, err);
        if (ok && rec.size() != ro[i + 1] - ro[i]) err = "the host's record has another length than the size pass gave it";
        if (!err.empty()) return oge_fail(ctx, OGE_ERR_ARG, ("sam: line " + std::to_string(header_lines + i + 1) + ": " + err).c_str());
        memcpy(out.data() + ro[i], rec.data(), rec.size());
    }
    ctx->sam_out_recs.swap(out);
    ctx->sam_out_off.swap(ro);
    ctx->sam_out_warn.swap(w);
    ctx->counters["sam_host_lines"] = n_host;
    *header_len = body;
    *recs = ctx->sam_out_recs.data();
    *rec_bytes = total;
    *rec_off = ctx->sam_out_off.data();
    *n_out = n;
    if (warn) *warn = ctx->sam_out_warn.data();
    return OGE_OK;
}

}  // extern "C"
