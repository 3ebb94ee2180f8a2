// sam.hip -- SAM and FASTQ text of the records resident in HBM (`openge view`, -F sam|fastq; the reference's
// util/sam_writer.cpp:90-217 and util/fastq_writer.cpp:99-100; DESIGN.md section 21, include/openge_hip.h).
//
//   size   k_text_size   one thread per record: the core, the CIGAR lengths and one walk over the tags give the
//                        exact text length (decimal widths by comparisons) and the record's mark; records with
//                        an f or B tag get length 0 and are counted (one atomic per wave), the first record that
//                        does not parse is kept by an atomic minimum
//   scan                 oge_exclusive_scan_u64 over the n + 1 lengths, in place
//   emit   k_text_emit   one wave per record, kWaveRecs consecutive records per wave: numbers, separators and tag
//                        heads are assembled in wave-uniform registers and stored by the first lanes; names, SEQ,
//                        QUAL and string tags are spread over the 64 lanes, one aligned dword per lane (256 bytes
//                        per store instruction) with the unaligned ends as single bytes.  No LDS, no atomics,
//                        every byte stored once at text_off[i] - text_off[first]; nothing is stored at or past a
//                        record's own length, so a record cannot write into its neighbour or past the buffer.
// The per-record code is sam_format.h, shared with a host program that runs it lane by lane.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "bam_layout.h"
#include "dev_util.h"
#include "oge_ctx.h"
#include "sam_format.h"
#include "sam_host.h"

namespace {

constexpr int kT = 256;
constexpr int kWaves = kT / 64;
constexpr int kWaveRecs = 4;  // consecutive records of one wave
constexpr int kBlockRecs = kWaves * kWaveRecs;
constexpr unsigned long long kNone = ~0ull;

struct TextAcc {
    unsigned long long n_host, first_bad;
};

__global__ __launch_bounds__(kT) void k_text_size(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ off, uint64_t n,
                                                  OgeTextParams tp, uint64_t *__restrict__ len_out, uint8_t *__restrict__ mark,
                                                  TextAcc *__restrict__ acc) {
    const uint64_t i = (uint64_t)blockIdx.x * kT + threadIdx.x;
    const bool valid = i < n;
    uint32_t m = OGE_TXT_DEVICE;
    uint64_t len = 0;
    if (valid) {
        len = oge_text_record_size(recs + off[i], tp, &m);
        len_out[i] = len;
        mark[i] = m == OGE_TXT_HOST ? 1 : 0;
        if (m == OGE_TXT_BAD) atomicMin(&acc->first_bad, (unsigned long long)i);
    } else if (i == n) {
        len_out[n] = 0;
    }
    const uint64_t hosts = __ballot(valid && m == OGE_TXT_HOST);
    if (hosts && (threadIdx.x & 63) == 0) atomicAdd(&acc->n_host, (unsigned long long)__popcll(hosts));
}

__device__ __forceinline__ uint64_t uni64(uint64_t v) {
    return ((uint64_t)OGE_TXT_UNI((uint32_t)(v >> 32)) << 32) | OGE_TXT_UNI((uint32_t)v);
}

__global__ __launch_bounds__(kT) void k_text_emit(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ off,
                                                  const uint64_t *__restrict__ text_off, uint64_t first, uint64_t count, OgeTextParams tp,
                                                  uint8_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63, wave = OGE_TXT_UNI(threadIdx.x >> 6);
    const uint64_t i0 = first + ((uint64_t)blockIdx.x * kWaves + wave) * kWaveRecs, end = first + count;
    const uint64_t base = text_off[first];
    for (int k = 0; k < kWaveRecs; ++k) {
        const uint64_t i = i0 + k;
        if (i >= end) break;
        const uint64_t a = uni64(text_off[i]), z = uni64(text_off[i + 1]);
        if (z <= a) continue;  // a record the host formats
        oge_text_record_emit(recs + uni64(off[i]), tp, out + (a - base), (uint32_t)(z - a), lane);
    }
}

// this side's own option checks, then the contig fields
int check_opts(oge_ctx *ctx, const oge_text_opts *o, const char *who) {
    const std::string w(who);
    if (!o) return oge_fail(ctx, OGE_ERR_ARG, (w + ": null argument").c_str());
    if (o->mode != OGE_TEXT_SAM && o->mode != OGE_TEXT_FASTQ) return oge_fail(ctx, OGE_ERR_ARG, (w + ": unknown text mode").c_str());
    if (o->trim_begin < 0 || o->trim_end < 0) return oge_fail(ctx, OGE_ERR_ARG, (w + ": negative trim length").c_str());
    return oge_contig_table(ctx, nullptr, o, who);
}

// the kernels' parameters, with the contig table on the device
int device_params(oge_ctx *ctx, const oge_text_opts *o, const char *who, OgeTextParams *tp) {
    const int rc = oge_contig_table(ctx, &ctx->text_table, o, who);
    if (rc) return rc;
    tp->mode = o->mode;
    tp->trim_begin = o->trim_begin;
    tp->trim_end = o->trim_end;
    tp->n_ref = o->n_ref;
    tp->names = ctx->text_table.d_names;
    tp->name_off = ctx->text_table.d_name_off;
    return OGE_OK;
}

int text_size_impl(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, const oge_text_opts *opts, uint64_t *d_text_off,
                   uint8_t *d_host_mark, uint64_t *total, uint64_t *n_host) {
    *total = 0;
    *n_host = 0;
    int rc = check_opts(ctx, opts, "oge_text_size_dev");
    if (rc) return rc;
    if (!d_text_off || (n && (!d_recs || !d_off || !d_host_mark))) return oge_fail(ctx, OGE_ERR_ARG, "oge_text_size_dev: null argument");
    if (n >= 0xFFFFFFFFull) return oge_fail(ctx, OGE_ERR_LIMIT, "oge_text_size_dev: more than 2^32-2 records");
    OgeTextParams tp;
    rc = device_params(ctx, opts, "oge_text_size_dev", &tp);
    if (rc) return rc;
    OgeStage stage(ctx, "text_size");
    hipStream_t st = ctx->stream;
    TextAcc *acc = (TextAcc *)ctx->ws("text_acc", sizeof(TextAcc));
    if (!acc) return OGE_ERR_HIP;
    TextAcc h = {0, kNone};
    OGE_HIP_TRY(ctx, hipMemcpyAsync(acc, &h, sizeof h, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_text_size, dim3(oge_ceil_div(n + 1, kT)), dim3(kT), 0, st, d_recs, d_off, n, tp, d_text_off, d_host_mark, acc);
    OGE_LAUNCH_CHECK(ctx);
    rc = oge_exclusive_scan_u64(ctx, d_text_off, d_text_off, n + 1);
    if (rc) return rc;
    uint64_t tot = 0;
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&h, acc, sizeof h, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&tot, d_text_off + n, 8, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (h.first_bad != kNone)
        return oge_fail(ctx, OGE_ERR_ARG,
                        ("text: record " + std::to_string(h.first_bad) +
                         " has a tag of an unknown type, a tag cut short or lengths that do not fit its block_size")
                            .c_str());
    *total = tot;
    *n_host = h.n_host;
    ctx->counters["sam_host_lines"] = h.n_host;
    return OGE_OK;
}

int text_emit_impl(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, const uint64_t *d_text_off, uint64_t first, uint64_t count,
                   const oge_text_opts *opts, uint8_t *d_out, uint64_t cap) {
    int rc = check_opts(ctx, opts, "oge_text_emit_dev");
    if (rc) return rc;
    ctx->counters["text_wave_records"] = kWaveRecs;
    ctx->counters["text_block_records"] = kBlockRecs;
    if (!d_text_off || (count && (!d_recs || !d_off))) return oge_fail(ctx, OGE_ERR_ARG, "oge_text_emit_dev: null argument");
    if (first + count < first || first + count >= 0xFFFFFFFFull) return oge_fail(ctx, OGE_ERR_LIMIT, "oge_text_emit_dev: record range");
    if (!count) return OGE_OK;
    hipStream_t st = ctx->stream;
    uint64_t ends[2] = {0, 0};
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&ends[0], d_text_off + first, 8, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipMemcpyAsync(&ends[1], d_text_off + first + count, 8, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (ends[1] < ends[0]) return oge_fail(ctx, OGE_ERR_ARG, "oge_text_emit_dev: text offsets decrease");
    if (ends[1] - ends[0] > cap) return oge_fail(ctx, OGE_ERR_LIMIT, "oge_text_emit_dev: the output buffer is smaller than the range's text");
    if (ends[1] == ends[0]) return OGE_OK;
    if (!d_out) return oge_fail(ctx, OGE_ERR_ARG, "oge_text_emit_dev: null argument");
    OgeTextParams tp;
    rc = device_params(ctx, opts, "oge_text_emit_dev", &tp);
    if (rc) return rc;
    OgeStage stage(ctx, "text_emit");
    hipLaunchKernelGGL(k_text_emit, dim3(oge_ceil_div(count, kBlockRecs)), dim3(kT), 0, st, d_recs, d_off, d_text_off, first, count, tp, d_out);
    OGE_LAUNCH_CHECK(ctx);
    return OGE_OK;
}

}  // namespace

extern "C" {

int oge_text_size_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, const oge_text_opts *opts,
                      uint64_t *d_text_off, uint8_t *d_host_mark, uint64_t *total, uint64_t *n_host) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!total || !n_host) return oge_fail(ctx, OGE_ERR_ARG, "oge_text_size_dev: null argument");
    OgeCall call(ctx, /*hold=*/false);
    return text_size_impl(ctx, d_recs, d_off, n, opts, d_text_off, d_host_mark, total, n_host);
}

int oge_text_emit_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, const uint64_t *d_text_off, uint64_t first,
                      uint64_t count, const oge_text_opts *opts, uint8_t *d_out, uint64_t cap) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    OgeCall call(ctx, /*hold=*/false);
    return text_emit_impl(ctx, d_recs, d_off, d_text_off, first, count, opts, d_out, cap);
}

int oge_text_host_line(const uint8_t *rec, uint64_t rec_bytes, const oge_text_opts *opts, char *buf, uint64_t cap, uint64_t *len) {
    if (!rec || !len) return oge_fail(nullptr, OGE_ERR_ARG, "oge_text_host_line: null argument");
    const int rc = check_opts(nullptr, opts, "oge_text_host_line");
    if (rc) return rc;
    std::string line, err;
    if (!oge_text_line_host(rec, rec_bytes, opts, line, err)) return oge_fail(nullptr, OGE_ERR_ARG, ("text: " + err).c_str());
    *len = line.size();
    if (line.size() > cap || (!buf && !line.empty())) return oge_fail(nullptr, OGE_ERR_LIMIT, "oge_text_host_line: the buffer is too small");
    if (!line.empty()) memcpy(buf, line.data(), line.size());
    return OGE_OK;
}

int oge_text_format(oge_ctx *ctx, const uint8_t *recs, uint64_t rec_bytes, const uint64_t *rec_off, uint64_t n, const oge_text_opts *opts,
                    uint8_t *out, uint64_t cap, uint64_t *bytes) {
    if (!ctx) return oge_fail(nullptr, OGE_ERR_ARG, "null ctx");
    if (!bytes || (n && (!recs || !rec_off))) return oge_fail(ctx, OGE_ERR_ARG, "oge_text_format: null argument");
    *bytes = 0;
    OgeCall call(ctx, /*hold=*/true);
    hipStream_t st = ctx->stream;
    uint8_t *dr = (uint8_t *)ctx->ws("host_recs", rec_bytes + 16);
    uint64_t *dof = (uint64_t *)ctx->ws("host_off", (n + 1) * 8);
    uint64_t *dto = (uint64_t *)ctx->ws("text_off", (n + 1) * 8);
    uint8_t *dm = (uint8_t *)ctx->ws("text_mark", n + 1);
    if (!dr || !dof || !dto || !dm) return OGE_ERR_HIP;
    OGE_HIP_TRY(ctx, hipMemsetAsync(dr + rec_bytes, 0, 16, st));
    if (rec_bytes) OGE_HIP_TRY(ctx, hipMemcpyAsync(dr, recs, rec_bytes, hipMemcpyHostToDevice, st));
    if (n) OGE_HIP_TRY(ctx, hipMemcpyAsync(dof, rec_off, n * 8, hipMemcpyHostToDevice, st));
    uint64_t total = 0, n_host = 0;
    int rc = text_size_impl(ctx, dr, dof, n, opts, dto, dm, &total, &n_host);
    if (rc) return rc;
    // the host's lines first: an error in one of them leaves `out` untouched
    std::vector<uint64_t> to(n + 1);
    std::vector<uint8_t> mark(n);
    std::vector<uint64_t> where;
    std::vector<std::string> lines;
    uint64_t host_bytes = 0;
    if (n_host) {
        OGE_HIP_TRY(ctx, hipMemcpyAsync(to.data(), dto, (n + 1) * 8, hipMemcpyDeviceToHost, st));
        OGE_HIP_TRY(ctx, hipMemcpyAsync(mark.data(), dm, n, hipMemcpyDeviceToHost, st));
        OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
        for (uint64_t i = 0; i < n; ++i) {
            if (!mark[i]) continue;
            const uint8_t *r = recs + rec_off[i];
            std::string line, err;
            if (rec_off[i] + 4 > rec_bytes || rec_off[i] + 4 + (uint64_t)oge_rd_u32(r) > rec_bytes ||
                !oge_text_line_host(r, 4 + (uint64_t)oge_rd_u32(r), opts, line, err))
                return oge_fail(ctx, OGE_ERR_ARG, ("text: record " + std::to_string(i) + ": " + (err.empty() ? "past the buffer" : err)).c_str());
            host_bytes += line.size();
            where.push_back(to[i]);
            lines.push_back(std::move(line));
        }
    }
    *bytes = total + host_bytes;
    ctx->counters["sam_host_lines"] = n_host;
    if (*bytes > cap || (*bytes && !out)) return oge_fail(ctx, OGE_ERR_LIMIT, "oge_text_format: the output buffer is smaller than the text");
    if (!*bytes) return OGE_OK;
    uint8_t *dtext = (uint8_t *)ctx->ws("text_out", total + 16);
    if (!dtext) return OGE_ERR_HIP;
    rc = text_emit_impl(ctx, dr, dof, dto, 0, n, opts, dtext, total);
    if (rc) return rc;
    if (lines.empty()) {
        if (total) OGE_HIP_TRY(ctx, hipMemcpyAsync(out, dtext, total, hipMemcpyDeviceToHost, st));
        OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
        return OGE_OK;
    }
    std::vector<uint8_t> dev(total);
    if (total) OGE_HIP_TRY(ctx, hipMemcpyAsync(dev.data(), dtext, total, hipMemcpyDeviceToHost, st));
    OGE_HIP_TRY(ctx, hipStreamSynchronize(st));
    uint64_t src = 0, dst = 0;
    for (size_t k = 0; k < lines.size(); ++k) {
        if (where[k] > src) memcpy(out + dst, dev.data() + src, where[k] - src);
        dst += where[k] - src;
        src = where[k];
        if (!lines[k].empty()) memcpy(out + dst, lines[k].data(), lines[k].size());
        dst += lines[k].size();
    }
    if (total > src) memcpy(out + dst, dev.data() + src, total - src);
    return OGE_OK;
}

}  // extern "C"
