// modules.cpp -- AlgorithmModule chain over the C ABI (see modules.h).
#include "modules.h"

#include <algorithm>
#include <cctype>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cerrno>
#include <cstring>
#include <memory>
#include <functional>
#include <atomic>
#include <thread>
#include <unistd.h>
#include <sys/stat.h>
#include <fcntl.h>

#include "bam_layout.h"
#include "lib_table.h"

// realign.hip (C++): the realignment result's records and offsets moved out without a copy
void oge_realign_result_take(oge_realign_result *r, oge::bytevec &recs, std::vector<uint64_t> &offs);

namespace oge {

bool AlgorithmModule::verbose_ = false;

using TimePoint = std::chrono::steady_clock::time_point;
static TimePoint clk() { return std::chrono::steady_clock::now(); }
static double sec(TimePoint a, TimePoint z) { return std::chrono::duration<double>(z - a).count(); }

// counts of reads: the counts of two parts of a record set add up
static void add_metrics(OgeDupMetrics &a, const OgeDupMetrics &b) {
    a.unpaired_examined += b.unpaired_examined;
    a.pair_reads_examined += b.pair_reads_examined;
    a.secondary += b.secondary;
    a.unmapped += b.unmapped;
    a.unpaired_dups += b.unpaired_dups;
    a.pair_read_dups += b.pair_read_dups;
}

int ChainContext::fail(const std::string &where) {
    fprintf(stderr, "openge: %s: %s\n", where.c_str(), oge_last_error(ctx));
    return -1;
}

// OGE_WRITE_DEVICE=1: host batches are deflated on the GPU (FileWriter, LocalRealignment's result)
static bool write_device_forced() {
    const char *e = getenv("OGE_WRITE_DEVICE");
    return e && !strcmp(e, "1");
}

int ChainContext::to_device(ReadBatch &b) {
    if (b.dev_valid) return 0;
    const uint64_t bytes = b.offs[b.n];
    DevBuf r(ctx), o(ctx);
    if (r.alloc(bytes + 64) || o.alloc((b.n + 1) * 8)) return fail("device allocation");
    if (oge_memcpy(ctx, r.as<void>(), b.recs.data(), bytes, 1) || oge_memcpy(ctx, o.as<void>(), b.offs.data(), (b.n + 1) * 8, 1))
        return fail("host->device copy");
    b.d_recs = (uint8_t *)r.release();
    b.d_offs = (uint64_t *)o.release();
    b.d_bytes = bytes;
    b.dev_valid = true;
    return 0;
}

int ChainContext::to_host(ReadBatch &b) {
    if (b.host_valid) return 0;
    b.recs.clear();
    b.recs.reserve(b.d_bytes + 16);
    want_huge_pages(b.recs.data(), b.d_bytes + 16);
    b.recs.resize(b.d_bytes + 16);  // uninitialised: the copy below writes every byte but the slack
    memset(b.recs.data() + b.d_bytes, 0, 16);
    b.offs.resize(b.n + 1);
    if (oge_memcpy(ctx, b.recs.data(), b.d_recs, b.d_bytes, 2) || oge_memcpy(ctx, b.offs.data(), b.d_offs, (b.n + 1) * 8, 2))
        return fail("device->host copy");
    b.host_valid = true;
    return 0;
}

void ChainContext::free_device(ReadBatch &b) {
    if (b.d_recs) oge_dev_free(ctx, b.d_recs);
    if (b.d_offs) oge_dev_free(ctx, b.d_offs);
    b.d_recs = nullptr;
    b.d_offs = nullptr;
    b.dev_valid = false;
}

int ChainContext::init_ranks() {
    if (gpus <= 1 || !comms.empty()) return 0;
    const int ndev = oge_device_count();
    if (ndev < 1) return fail("--gpus");
    rank_ctx.assign(gpus, nullptr);
    rank_ctx[0] = ctx;
    for (int g = 1; g < gpus; ++g) {
        if (oge_ctx_create((device + g) % ndev, &rank_ctx[g])) {
            rank_ctx.resize(g);
            return fail("--gpus: context");
        }
        const char *pool = getenv("OGE_POOL");
        if (!(pool && std::string(pool) == "0")) oge_ctx_set_pool(rank_ctx[g], 1);
    }
    // the multi-process route of bench.py / a torchrun launch, one host thread per rank: one id, every
    // rank joins concurrently (RCCL between distinct GPUs, the host-staged transport when they share one)
    std::vector<uint8_t> id(oge_comm_unique_id_bytes());
    if (oge_comm_unique_id(id.data(), id.size())) return fail("--gpus: communicator id");
    comms.assign(gpus, nullptr);
    std::vector<int> rcs(gpus, 0);
    std::vector<std::string> why(gpus);
    {
        std::vector<std::thread> ts;
        for (int g = 0; g < gpus; ++g)
            ts.emplace_back([&, g]() {
                // every rank is a thread of this process: the shared-segment meeting is node-local by
                // construction, so ranks sharing a device take the host transport
                rcs[g] = oge_comm_init_rank_mode(rank_ctx[g], gpus, g, id.data(), gpus > ndev ? "host" : "node", &comms[g]);
                if (rcs[g]) why[g] = oge_last_error(rank_ctx[g]);
            });
        for (auto &t : ts) t.join();
    }
    for (int g = 0; g < gpus; ++g)
        if (rcs[g]) {
            fprintf(stderr, "openge: --gpus: rank %d communicator: %s\n", g, why[g].c_str());
            for (oge_comm *c : comms)
                if (c) oge_comm_destroy(c);
            comms.clear();
            return -1;
        }
    if (verbose)
        fprintf(stderr, "[openge] %d ranks on %d device(s), transport %s\n", gpus, std::min(gpus, ndev), oge_comm_transport(comms[0]));
    return 0;
}

void ChainContext::close_ranks() {
    for (oge_comm *c : comms) oge_comm_destroy(c);
    comms.clear();
    for (size_t g = 1; g < rank_ctx.size(); ++g) oge_ctx_destroy(rank_ctx[g]);
    rank_ctx.clear();
}

// Cut the batch into G contiguous input ranges and run oge_sort_markdup_dist on every rank (one host
// thread each).  A rank whose own preparation failed still joins the collectives with an empty shard
// so the others finish, and the failure is reported.
int run_ranks(ChainContext &cc, ReadBatch &b, bool sort, const oge_markdup_opts *opts, uint64_t *n_dup, std::vector<OgeDupMetrics> *metrics,
              double *metrics_ms) {
    const bool sharded = !b.shards.empty();  // the reader left every rank its own input shard
    if (cc.init_ranks() || (!sharded && cc.to_device(b))) return -1;
    const int G = cc.gpus;
    const uint64_t n = b.n;
    const int32_t n_ref = (int32_t)b.ref_names.size();
    std::vector<uint64_t> cut(G + 1), boff(G + 1);
    for (int g = 0; g <= G && !sharded; ++g) {
        cut[g] = n * (uint64_t)g / (uint64_t)G;
        if (oge_memcpy(cc.ctx, &boff[g], b.d_offs + cut[g], 8, 2)) return cc.fail("device->host copy");
    }
    std::vector<ReadBatch::Slice> sl(G);
    std::vector<int> rcs(G, 0);
    std::vector<uint64_t> nds(G, 0);
    std::vector<std::string> why(G);
    // --metrics: every rank counts the slice it was left with, on its own device
    const bool count = metrics && opts;
    std::vector<std::vector<OgeDupMetrics>> part(G, std::vector<OgeDupMetrics>(count ? metrics->size() : 0));
    std::vector<double> part_ms(G, 0);
    auto count_slice = [&](int g) {
        if (!count || rcs[g]) return;
        oge_ctx *c = cc.rank_ctx[g];
        rcs[g] = oge_dup_metrics_dev(c, sl[g].d_recs, sl[g].d_offs, sl[g].n, opts, (int32_t)part[g].size(), part[g].data());
        if (rcs[g]) why[g] = oge_last_error(c);
        else oge_ctx_timing(c, "dup_metrics", &part_ms[g]);
    };
    std::vector<std::thread> ts;
    for (int g = 0; g < G; ++g)
        ts.emplace_back([&, g]() {
            oge_ctx *c = cc.rank_ctx[g];
            uint8_t *dout = nullptr;
            uint64_t *doff = nullptr, no = 0, nd = 0;
            if (sharded) {  // the rank's own shard, in its HBM already
                const ReadBatch::Slice &s = b.shards[g];
                rcs[g] = oge_sort_markdup_dist(cc.comms[g], s.d_recs, s.d_offs, s.n, n_ref, sort ? 1 : 0, opts, &dout, &doff, &no, &nd);
                if (rcs[g]) why[g] = oge_last_error(c);
                sl[g] = {c, dout, doff, no};
                nds[g] = nd;
                count_slice(g);
                return;
            }
            const uint64_t lo = cut[g], m = cut[g + 1] - lo, bytes = boff[g + 1] - boff[g];
            DevBuf r(c), o(c);
            int rc = r.alloc(bytes + 64);
            if (!rc) rc = o.alloc((m + 1) * 8);
            if (!rc && bytes) rc = oge_memcpy(c, r.as<void>(), b.d_recs + boff[g], bytes, 4);
            if (!rc) rc = oge_memcpy(c, o.as<void>(), b.d_offs + lo, (m + 1) * 8, 4);
            if (rc) why[g] = oge_last_error(c);
            // the offsets stay absolute: the records pointer is shifted back by the range's first one
            const int rd = rc ? oge_sort_markdup_dist(cc.comms[g], nullptr, nullptr, 0, n_ref, sort ? 1 : 0, opts, &dout, &doff, &no, &nd)
                              : oge_sort_markdup_dist(cc.comms[g], r.as<uint8_t>() - boff[g], o.as<uint64_t>(), m, n_ref,
                                                      sort ? 1 : 0, opts, &dout, &doff, &no, &nd);
            if (!rc && rd) why[g] = oge_last_error(c);
            rcs[g] = rc ? rc : rd;
            sl[g] = {c, dout, doff, no};
            nds[g] = nd;
            count_slice(g);
        });
    for (auto &t : ts) t.join();
    for (int g = 0; g < G; ++g)
        if (rcs[g]) {
            fprintf(stderr, "openge: rank %d: %s\n", g, why[g].c_str());
            return -1;
        }
    if (count) {
        for (int g = 0; g < G; ++g)
            for (size_t k = 0; k < metrics->size(); ++k) add_metrics((*metrics)[k], part[g][k]);
        if (metrics_ms) *metrics_ms += *std::max_element(part_ms.begin(), part_ms.end());
    }
    cc.free_device(b);
    b.shards.clear();
    b.slices = sl;
    b.n = 0;
    for (auto &x : sl) b.n += x.n;
    b.host_valid = false;
    *n_dup = nds[0];
    return 0;
}

int AlgorithmModule::runChain(ChainContext &cc) {
    AlgorithmModule *head = this;
    while (head->source_) head = head->source_;
    ReadBatch b;
    bool marked = false;  // ReadSorter fused MarkDuplicates into its device pipeline
    for (AlgorithmModule *m = head; m; m = m->sink_) {
        if (marked && dynamic_cast<MarkDuplicates *>(m)) {
            b.drop_duplicates = static_cast<MarkDuplicates *>(m)->removeDuplicates;
            marked = false;
            continue;
        }
        if (verbose_) fprintf(stderr, "[openge] running %s on %llu records\n", m->name(), (unsigned long long)b.n);
        const auto t0 = clk();
        int rc = m->runInternal(cc, b);
        if (verbose_)
            fprintf(stderr, "[openge] %s: %.3f s\n", m->name(),
                    sec(t0, clk()));
        if (rc) {
            cc.free_device(b);
            return rc;
        }
        if (dynamic_cast<ReadSorter *>(m) && static_cast<ReadSorter *>(m)->sortBy() == BamHeaderModel::COORDINATE &&
            dynamic_cast<MarkDuplicates *>(m->sink_))
            marked = true;
    }
    cc.free_device(b);
    // --metrics: every part of the marked output has been counted by now (the chunked sort's ranges only when
    // the writer asked for them)
    for (AlgorithmModule *m = head; m; m = m->sink_)
        if (auto *md = dynamic_cast<MarkDuplicates *>(m))
            if (!md->metricsFilename.empty() && md->writeMetrics()) return -1;
    return 0;
}

// ------------------------------------------------------------------------------------ SAM input
// MultiReader::open looks at the first byte of every input (util/read_stream_reader.h:45-85): '@' is SAM.
static bool file_is_sam(const std::string &path) {
    const OwnedFd fd(open(path.c_str(), O_RDONLY));
    struct stat st;
    char c = 0;
    return fd.fd >= 0 && !fstat(fd.fd, &st) && S_ISREG(st.st_mode) && pread(fd.fd, &c, 1, 0) == 1 && c == '@';
}

// The header text of a SAM file through the model bam_parse_header feeds: the same header and contig names as
// the BAM file of the same reads gives.
static bool sam_header_model(const std::string &text, BamFile &f, std::string &err) {
    f.header_text = text;
    if (!f.header.parse(text, err)) return false;
    f.ref_names.clear();
    f.ref_lens.clear();
    for (auto &s : f.header.sq) {
        f.ref_names.push_back(s.name);
        f.ref_lens.push_back((int32_t)s.length);
    }
    return true;
}

struct SamOpts {  // oge_text_opts over the contig names of a header
    std::string names;
    std::vector<uint32_t> off;
    oge_text_opts o;
    explicit SamOpts(const std::vector<std::string> &ref_names) : off(1, 0) {
        for (auto &n : ref_names) {
            names += n;
            off.push_back((uint32_t)names.size());
        }
        o = {OGE_TEXT_SAM, 0, 0, (int32_t)ref_names.size(), names.data(), off.data()};
    }
};

// the reference's stderr line for an RNEXT its dictionary does not have (sam_reader.cpp:373)
static void warn_rnext(const char *line, uint64_t len) {
    const char *p = line, *end = line + len;
    for (int k = 0; k < 6 && p; ++k) {
        p = (const char *)memchr(p, '\t', (size_t)(end - p));
        if (p) ++p;
    }
    if (!p) return;
    const char *e = (const char *)memchr(p, '\t', (size_t)(end - p));
    fprintf(stderr, "RNext %.*s missing from sequence dictionary\n", (int)((e ? e : end) - p), p);
}

// a failed oge_sam_* call: the reference's own line for an unknown RNAME (sam_reader.cpp:360), then ours
static int sam_fail(ChainContext &cc, const std::string &name) {
    const std::string m = oge_last_error(cc.ctx);
    const size_t cut = m.find(" (sam: line ");
    if (m.compare(0, 6, "Rname ") == 0 && cut != std::string::npos) {
        fprintf(stderr, "%s\n", m.substr(0, cut).c_str());
        fprintf(stderr, "openge: error reading %s: %s\n", name.c_str(), m.substr(cut + 2, m.size() - cut - 3).c_str());
    } else {
        fprintf(stderr, "openge: error reading %s: %s\n", name.c_str(), m.c_str());
    }
    return -1;
}

// A SAM text in host memory -> a BamFile (records from rec_base 0), parsed on the GPU (oge_sam_parse).
static int sam_host_file(ChainContext &cc, const std::string &name, const bytevec &text, BamFile &f) {
    uint64_t hl = 0, rb = 0, n = 0;
    const uint8_t *recs = nullptr, *warn = nullptr;
    const uint64_t *offs = nullptr;
    if (oge_sam_parse(cc.ctx, (const char *)text.data(), text.size(), &hl, &recs, &rb, &offs, &n, &warn)) return sam_fail(cc, name);
    std::string err;
    if (!sam_header_model(std::string((const char *)text.data(), hl), f, err)) {
        fprintf(stderr, "openge: error reading %s: %s\n", name.c_str(), err.c_str());
        return -1;
    }
    f.rec_base = 0;
    f.data.assign(recs, recs + rb);
    f.offsets.assign(offs, offs + n);
    uint64_t p = hl;
    for (uint64_t i = 0; i < n; ++i) {  // the lines in file order, only to name the unknown mates
        const void *nl = memchr(text.data() + p, '\n', text.size() - p);
        const uint64_t e = nl ? (uint64_t)((const uint8_t *)nl - text.data()) : text.size();
        if (warn[i]) warn_rnext((const char *)text.data() + p, e - p);
        p = e + 1;
    }
    return 0;
}

// SAM text resident in HBM (4-byte aligned) -> the batch's records in HBM: the header from a prefix, then the
// line index, the size pass and the emit pass (oge_sam_*_dev); the few lines with an f or B tag are fetched,
// built on the host and copied to their places.  need_sort_room: the HBM check the BAM reader makes in front
// of a ReadSorter, here over the text plus the records; a text that does not fit is refused, not spilled.
static int sam_device_records(ChainContext &cc, const std::string &name, const uint8_t *d_text, uint64_t bytes, bool need_sort_room, ReadBatch &b,
                              std::vector<int32_t> *ref_lens = nullptr) {
    std::string head;
    uint64_t hl = 0;
    for (uint64_t pre = std::min<uint64_t>(bytes, 1 << 20);; pre = std::min<uint64_t>(bytes, pre * 8)) {
        head.resize(pre);
        if (pre && oge_memcpy(cc.ctx, &head[0], d_text, pre, 2)) return cc.fail("device->host copy");
        oge_sam_header(head.data(), pre, &hl, nullptr);
        if (hl < pre || pre == bytes) break;
    }
    BamFile f;
    std::string err;
    if (!sam_header_model(head.substr(0, hl), f, err)) {
        fprintf(stderr, "openge: error reading %s: %s\n", name.c_str(), err.c_str());
        return -1;
    }
    const SamOpts so(f.ref_names);
    uint64_t n = 0, total = 0, n_host = 0;
    DevBuf dlo(cc.ctx), dro(cc.ctx), dmark(cc.ctx), dwarn(cc.ctx), drecs(cc.ctx);
    if (oge_sam_lines_dev(cc.ctx, d_text, bytes, hl, nullptr, 0, &n)) return sam_fail(cc, name);
    if (dlo.alloc((n + 1) * 8) || dro.alloc((n + 1) * 8) || dmark.alloc(n + 1) || dwarn.alloc(n + 1)) return cc.fail("device allocation");
    if (oge_sam_lines_dev(cc.ctx, d_text, bytes, hl, dlo.as<uint64_t>(), n + 1, &n) ||
        oge_sam_size_dev(cc.ctx, d_text, dlo.as<uint64_t>(), n, &so.o, dro.as<uint64_t>(), dmark.as<uint8_t>(), dwarn.as<uint8_t>(), &total, &n_host))
        return sam_fail(cc, name);
    uint64_t fr = 0, tot = 0;
    if ((need_sort_room && !oge_mem_info(cc.ctx, &fr, &tot) && total / 10 * 25 > fr) || drecs.alloc(total + 64)) {
        fprintf(stderr, "openge: error reading %s: the SAM text (%llu bytes) and its records (%llu bytes) do not fit in device memory; "
                "SAM input larger than HBM is not provided\n", name.c_str(), (unsigned long long)bytes, (unsigned long long)total);
        return -1;
    }
    if (oge_sam_emit_dev(cc.ctx, d_text, dlo.as<uint64_t>(), dro.as<uint64_t>(), 0, n, &so.o, drecs.as<uint8_t>(), total)) return sam_fail(cc, name);
    std::vector<uint8_t> mark(n), warn(n);
    if (n && (oge_memcpy(cc.ctx, mark.data(), dmark.as<void>(), n, 2) || oge_memcpy(cc.ctx, warn.data(), dwarn.as<void>(), n, 2)))
        return cc.fail("device->host copy");
    // the marked and the warned lines: both offset tables come down once; their text comes down line by line while
    // they are few, else as the whole text in one copy; the host's records go up one copy per run of neighbours
    uint64_t n_special = 0;
    for (uint64_t i = 0; i < n; ++i) n_special += mark[i] || warn[i];
    if (n_special) {
        std::vector<uint64_t> lo(n + 1), ro(n + 1);
        if (oge_memcpy(cc.ctx, lo.data(), dlo.as<void>(), (n + 1) * 8, 2) || oge_memcpy(cc.ctx, ro.data(), dro.as<void>(), (n + 1) * 8, 2))
            return cc.fail("device->host copy");
        const bool whole = n_special > 4096;
        bytevec text;
        if (whole) {
            text.resize(bytes);
            if (oge_memcpy(cc.ctx, text.data(), d_text, bytes, 2)) return cc.fail("device->host copy");
        }
        std::string one;
        std::vector<uint8_t> run, rec;  // the records of consecutive marked lines, back to back
        uint64_t run_at = 0;
        auto flush = [&]() -> int {
            const int rc = run.empty() ? 0 : oge_memcpy(cc.ctx, drecs.as<uint8_t>() + run_at, run.data(), run.size(), 1);
            run.clear();
            return rc;
        };
        for (uint64_t i = 0; i < n; ++i) {
            if (!mark[i] && !warn[i]) continue;
            const uint64_t len = lo[i + 1] - 1 - lo[i];
            const char *line = whole ? (const char *)text.data() + lo[i] : nullptr;
            if (!whole) {
                one.resize(len);
                if (len && oge_memcpy(cc.ctx, &one[0], d_text + lo[i], len, 2)) return cc.fail("device->host copy");
                line = one.data();
            }
            if (warn[i]) warn_rnext(line, len);
            if (!mark[i]) continue;
            uint64_t got = 0;
            rec.resize(ro[i + 1] - ro[i]);
            if (oge_sam_host_record(line, len, &so.o, rec.data(), rec.size(), &got) || got != rec.size()) {
                uint64_t hdr_lines = 0;
                oge_sam_header(head.data(), hl, &hl, &hdr_lines);
                fprintf(stderr, "openge: error reading %s: line %llu: %s\n", name.c_str(), (unsigned long long)(hdr_lines + i + 1),
                        oge_last_error(nullptr));
                return -1;
            }
            if (!run.empty() && run_at + run.size() != ro[i] && flush()) return cc.fail("host->device copy");
            if (run.empty()) run_at = ro[i];
            run.insert(run.end(), rec.begin(), rec.end());
            if (run.size() > (64u << 20) && flush()) return cc.fail("host->device copy");
        }
        if (flush()) return cc.fail("host->device copy");
    }
    if (ref_lens) *ref_lens = f.ref_lens;
    b.header = f.header;
    b.ref_names = f.ref_names;
    b.n = n;
    b.d_recs = (uint8_t *)drecs.release();
    b.d_offs = (uint64_t *)dro.release();
    b.d_bytes = total;
    b.dev_valid = true;
    b.host_valid = false;
    if (AlgorithmModule::isVerbose()) {
        double te = 0;
        oge_ctx_timing(cc.ctx, "sam_emit", &te);
        fprintf(stderr, "[openge] SAM input: %llu lines, %llu text bytes -> %llu record bytes, %llu lines built on the host, emit %.3f ms\n",
                (unsigned long long)n, (unsigned long long)bytes, (unsigned long long)total, (unsigned long long)n_host, te);
    }
    return 0;
}

// One SAM file into HBM (the streamed loader, else a host read and one copy up) and its records.
static int read_sam_device(ChainContext &cc, const std::string &path, bool need_sort_room, ReadBatch &b, std::vector<int32_t> *ref_lens = nullptr) {
    LoadedFile z(cc.ctx);
    if (file_to_device(cc, path, LOAD_STREAM, z) != 0) {
        bytevec text;
        std::string err;
        if (!read_file_bytes(path, text, cc.threads > 0 ? cc.threads : 8, err)) {
            fprintf(stderr, "openge: error reading %s: %s\n", path.c_str(), err.c_str());
            return -1;
        }
        if (z.buf.alloc(text.size() + 16) || oge_memcpy(cc.ctx, z.buf.as<void>(), text.data(), text.size(), 1)) {
            fprintf(stderr, "openge: error reading %s: the SAM text (%llu bytes) does not fit in device memory; SAM input larger than HBM is not "
                    "provided\n", path.c_str(), (unsigned long long)text.size());
            return -1;
        }
        z.zbytes = text.size();
    }
    return sam_device_records(cc, path, z.buf.as<uint8_t>(), z.zbytes, need_sort_room, b, ref_lens);
}

// ----------------------------------------------------------------------------------- FileReader
int FileReader::read_device(ChainContext &cc, ReadBatch &b, const std::string &path) {
    const auto t0 = clk();
    const int threads = cc.threads > 0 ? cc.threads : 8;
    bytevec comp;
    std::string err;
    LoadedFile z(cc.ctx);
    DevBuf di(cc.ctx), dc(cc.ctx), dout(cc.ctx), doff(cc.ctx);
    uint64_t nb = 0, total = 0;
    bool streamed = false;
    if (!getenv("OGE_CHUNK_BYTES") && !(getenv("OGE_READER") && std::string(getenv("OGE_READER")) == "hostcopy") &&
        file_to_device(cc, path, LOAD_STREAM, z) == 0) {
        // framing index on the device (count, then fill); anything it rejects goes to the host path
        streamed = oge_bgzf_index_dev(cc.ctx, z.buf.as<uint8_t>(), z.zbytes, nullptr, nullptr, nullptr, nullptr, 0, &nb) == 0 &&
                   di.alloc((3 * nb + 1) * 8) == 0 && dc.alloc(nb * 4 + 4) == 0;
        if (streamed) {
            uint64_t *dd = di.as<uint64_t>();
            streamed = oge_bgzf_index_dev(cc.ctx, z.buf.as<uint8_t>(), z.zbytes, dd, dd + nb, dd + 2 * nb, dc.as<uint32_t>(), nb, &nb) == 0 &&
                       oge_memcpy(cc.ctx, &total, dd + 3 * nb, 8, 2) == 0;
        }
        if (streamed && sink_sorts()) {
            uint64_t fr = 0, tot = 0;
            if (oge_mem_info(cc.ctx, &fr, &tot) || total / 10 * 25 > fr) streamed = false;
        }
        if (!streamed) {
            z.buf.reset(), di.reset(), dc.reset();
            nb = total = 0;
        }
    }
    auto t1 = clk();
    if (!streamed) {
        prefetch_drop();  // OGE_CHUNK_BYTES / OGE_READER=hostcopy: nobody takes it
        if (!read_file_bytes(path, comp, threads, err)) {
            fprintf(stderr, "openge: error reading %s: %s\n", path.c_str(), err.c_str());
            return -1;
        }
        oge_bgzf_index(comp.data(), comp.size(), nullptr, nullptr, nullptr, nullptr, 0, &nb);
        std::vector<uint64_t> idx(3 * nb + 1);
        std::vector<uint32_t> crc(nb);
        if (oge_bgzf_index(comp.data(), comp.size(), idx.data(), idx.data() + nb, idx.data() + 2 * nb, crc.data(), nb, &nb))
            return 1;  // not BGZF / truncated: the host reader reports it
        total = idx[3 * nb];
        if (sink_sorts()) {  // larger than HBM (or the chunked test knob): the sorter works from host memory
            uint64_t fr = 0, tot = 0;
            if (getenv("OGE_CHUNK_BYTES") || (!oge_mem_info(cc.ctx, &fr, &tot) && total / 10 * 25 > fr)) return 1;
        }
        t1 = clk();
        z.zbytes = comp.size();
        if (z.buf.alloc(comp.size() + 16) || di.alloc(idx.size() * 8) || dc.alloc(crc.size() * 4 + 4)) return cc.fail("device allocation");
        if (oge_memcpy(cc.ctx, z.buf.as<void>(), comp.data(), comp.size(), 1) || oge_memcpy(cc.ctx, di.as<void>(), idx.data(), idx.size() * 8, 1) ||
            oge_memcpy(cc.ctx, dc.as<void>(), crc.data(), crc.size() * 4, 1))
            return cc.fail("host->device copy");
    }
    if (dout.alloc(total + 64)) return cc.fail("device allocation");
    const auto t2 = clk();
    const uint64_t *dd = di.as<uint64_t>();
    if (nb && oge_bgzf_inflate_dev(cc.ctx, z.buf.as<uint8_t>(), z.zbytes, dd, dd + nb, dd + 2 * nb, dc.as<uint32_t>(), nb, dout.as<uint8_t>()))
        return 1;
    double t_kern = -1;
    if (verbose_) oge_ctx_timing(cc.ctx, "bgzf_inflate", &t_kern);  // synchronises: the kernels' own time
    const auto t2b = clk();
    z.buf.reset();
    // the host path's copy of the compressed file (29 GB at 150M reads) takes ~1.5 s to unmap: on a
    // thread of its own, beside the device stages that follow
    if (!comp.empty()) std::thread([](bytevec v) { v = bytevec(); }, std::move(comp)).detach();
    comp = bytevec();
    const auto t3 = clk();
    // header from a prefix of the stream
    BamFile f;
    size_t rec_base = 0;
    for (uint64_t pre = std::min<uint64_t>(total, 1 << 20);; pre = std::min<uint64_t>(total, pre * 8)) {
        std::vector<uint8_t> h(pre);
        if (pre && oge_memcpy(cc.ctx, h.data(), dout.as<void>(), pre, 2)) return cc.fail("device->host copy");
        f = BamFile();
        if (bam_parse_header(h.data(), pre, f, err, &rec_base)) break;
        if (pre == total) return 1;
    }
    uint64_t n = 0;
    if (oge_bam_record_offsets_dev(cc.ctx, dout.as<uint8_t>(), rec_base, total, (int32_t)f.ref_names.size(), nullptr, 0, &n) ||
        doff.alloc((n + 1) * 8) ||
        oge_bam_record_offsets_dev(cc.ctx, dout.as<uint8_t>(), rec_base, total, (int32_t)f.ref_names.size(), doff.as<uint64_t>(), n + 1, &n))
        return 1;
    b.header = f.header;
    b.ref_names = f.ref_names;
    b.n = n;
    b.d_recs = (uint8_t *)dout.release();
    b.d_offs = (uint64_t *)doff.release();
    b.d_bytes = total;
    b.dev_valid = true;
    b.host_valid = false;
    if (verbose_)
        fprintf(stderr,
                "[openge] FileReader (device%s): file %.3f s, upload %.3f s, inflate %.3f s (kernels %.3f s, release of the "
                "compressed copies %.3f s), records %.3f s\n",
                streamed ? (z.prefetched ? ", prefetched + device index" : ", streamed + device index") : "", sec(t0, t1),
                sec(t1, t2), sec(t2, t3), t_kern / 1e3, sec(t2b, t3),
                sec(t3, clk()));
    return 0;
}

// ----------------------------------------------------------------------------------- indexed reads
bool FileReader::index_beside(const std::string &path, std::string &bai, std::string &why) {
    struct stat sf, sb;
    if (stat(path.c_str(), &sf) || !S_ISREG(sf.st_mode)) {
        why = "the input is not a regular file";
        return false;
    }
    std::vector<std::string> cand = {path + ".bai"};
    if (path.size() > 4 && path.compare(path.size() - 4, 4, ".bam") == 0) cand.push_back(path.substr(0, path.size() - 4) + ".bai");
    for (auto &c : cand) {
        if (stat(c.c_str(), &sb) || !S_ISREG(sb.st_mode)) continue;
        if (sb.st_mtim.tv_sec < sf.st_mtim.tv_sec || (sb.st_mtim.tv_sec == sf.st_mtim.tv_sec && sb.st_mtim.tv_nsec < sf.st_mtim.tv_nsec)) {
            why = "the index " + c + " is older than the file";
            return false;
        }
        bai = c;
        return true;
    }
    why = "no index beside the file";
    return false;
}

// BSIZE of the BGZF block whose 18-byte header is h (BC first in the extra field, as every writer here and
// htslib places it); 0: no such header
static uint64_t bgzf_block_size(const uint8_t *h) {
    if (h[0] != 31 || h[1] != 139 || h[2] != 8 || h[3] != 4 || h[12] != 'B' || h[13] != 'C' || h[14] != 2 || h[15] != 0) return 0;
    return (uint64_t)(h[16] | (h[17] << 8)) + 1;
}

// The header of a regular input file without reading the file: a BAM file's from its first whole BGZF blocks (a
// 1 MiB prefix, growing by 8), a SAM file's from its leading '@' lines.  False: leave it to the reader.
static bool peek_header(const std::string &path, BamFile &f) {
    OwnedFd in(open(path.c_str(), O_RDONLY));
    struct stat sf;
    if (in.fd < 0 || fstat(in.fd, &sf) || !S_ISREG(sf.st_mode) || sf.st_size < 1) return false;
    const uint64_t fsize = (uint64_t)sf.st_size;
    std::string err;
    for (uint64_t pre = std::min<uint64_t>(fsize, 1 << 20);; pre = std::min<uint64_t>(fsize, pre * 8)) {
        bytevec head(pre), stream;
        if (!pread_all(in.fd, head.data(), 0, pre, 1 << 20, 1)) return false;
        f = BamFile();
        if (head[0] == '@') {  // SAM: every header line is whole once a line that is not one has been seen
            uint64_t p = 0;
            while (p < pre && head[p] == '@') {
                const void *nl = memchr(head.data() + p, '\n', pre - p);
                if (!nl) break;
                p = (uint64_t)((const uint8_t *)nl - head.data()) + 1;
            }
            if ((p < pre && head[p] != '@') || pre == fsize)
                return sam_header_model(std::string((const char *)head.data(), p < pre && head[p] != '@' ? p : pre), f, err);
        } else {
            uint64_t whole = 0;
            while (whole + 18 <= pre) {
                const uint64_t bs = bgzf_block_size(head.data() + whole);
                if (!bs || whole + bs > pre) break;
                whole += bs;
            }
            size_t rec_base = 0;
            if (whole && bgzf_inflate_all(head.data(), whole, stream, 1, err) && bam_parse_header(stream.data(), stream.size(), f, err, &rec_base))
                return true;
            if (pre == fsize) return false;
        }
    }
}

int FileReader::read_indexed(ChainContext &cc, ReadBatch &b, const std::string &path) {
    const auto t0 = clk();
    auto *flt = dynamic_cast<Filter *>(sink_);
    std::string bai_path, why, err;
    auto full_scan = [&](const std::string &reason) {
        if (verbose_) fprintf(stderr, "[openge] FileReader: full scan, %s\n", reason.c_str());
        return 1;
    };
    if (!flt || !index_beside(path, bai_path, why)) return full_scan(why);
    const int threads = cc.threads > 0 ? cc.threads : 8;
    bytevec bai;
    if (!read_file_bytes(bai_path, bai, threads, err)) return full_scan("the index cannot be read: " + err);
    OwnedFd in(open(path.c_str(), O_RDONLY));
    struct stat sf;
    if (in.fd < 0 || fstat(in.fd, &sf)) return full_scan("the file cannot be opened");
    const uint64_t fsize = (uint64_t)sf.st_size;
    // ---- the header, from the file's first blocks
    BamFile f;
    if (!peek_header(path, f)) return full_scan("the header cannot be read from the first blocks");
    const int32_t n_ref = (int32_t)f.ref_names.size();
    std::vector<oge_region> regions;
    if (flt->parseRegions(f.header, regions)) return -1;
    // ---- index -> ranges -> spans of the file
    oge_bai *ix = nullptr;
    if (oge_bai_open(cc.ctx, bai.data(), bai.size(), n_ref, &ix)) return full_scan(oge_last_error(cc.ctx));
    struct CloseBai {
        oge_bai *p;
        ~CloseBai() { oge_bai_close(p); }
    } close_bai{ix};
    const uint64_t *d_ranges = nullptr;
    uint64_t n_ranges = 0;
    if (oge_bai_query_dev(cc.ctx, ix, regions.data(), regions.size(), kIndexWiden, &d_ranges, &n_ranges)) return full_scan(oge_last_error(cc.ctx));
    std::vector<uint64_t> ranges(2 * n_ranges), span_file, span_z = {0};
    if (n_ranges && oge_memcpy(cc.ctx, ranges.data(), d_ranges, n_ranges * 16, 2)) return full_scan(oge_last_error(cc.ctx));
    uint64_t span_end = 0;
    for (uint64_t r = 0; r < n_ranges; ++r) {
        const uint64_t beg = ranges[2 * r], end = ranges[2 * r + 1];
        const uint64_t sb = beg >> 16;
        uint64_t se = end >> 16;
        if (beg >= end || se > fsize) return full_scan("a range of the index is empty or points past the file");
        if (end & 0xFFFF) {  // the block that holds end - 1: its size from its header
            uint8_t h[18];
            if (se + 18 > fsize || !pread_all(in.fd, h, se, 18, 18, 1) || !bgzf_block_size(h) || se + bgzf_block_size(h) > fsize)
                return full_scan("a range of the index does not end in a BGZF block");
            se += bgzf_block_size(h);
        }
        if (sb >= se) return full_scan("a range of the index is empty or points past the file");
        if (!span_file.empty() && sb <= span_end + 65536) {  // touching or less than one maximal block apart
            if (sb < span_file.back()) return full_scan("the ranges of the index do not ascend");
            span_end = std::max(span_end, se);
        } else {
            if (!span_file.empty()) span_z.push_back(span_z.back() + (span_end - span_file.back()));
            span_file.push_back(sb);
            span_end = se;
        }
    }
    if (!span_file.empty()) span_z.push_back(span_z.back() + (span_end - span_file.back()));
    const uint64_t zbytes = span_z.back();
    // a list that names most of the file: the full scan streams it with less work than spans and a pack
    if (zbytes > fsize / 2) return full_scan("the index names more than half of the file");
    const auto t1 = clk();
    DevBuf dz(cc.ctx), dout(cc.ctx), doff(cc.ctx);
    uint64_t n = 0, bytes = 0, blocks = 0;
    if (n_ranges) {
        // the compressed spans, their inflated form and the packed records are in HBM together
        uint64_t fr = 0, tot = 0;
        if (oge_mem_info(cc.ctx, &fr, &tot) || zbytes / 10 * 60 > fr) return full_scan("the spans of the index do not fit beside their records");
        if (dz.alloc(zbytes + 16)) return full_scan(oge_last_error(cc.ctx));
        // long spans stream through page-locked buffers; runs of short ones go up together from one host buffer
        constexpr uint64_t kLong = 8ull << 20;
        bytevec stage;
        for (size_t s = 0; s < span_file.size();) {
            const uint64_t len = span_z[s + 1] - span_z[s];
            if (len >= kLong) {
                if (range_to_device(cc.ctx, in.fd, span_file[s], len, dz.as<uint8_t>() + span_z[s], std::min<uint64_t>(len, 64ull << 20), 4 << 20))
                    return full_scan("the file cannot be read");
                ++s;
                continue;
            }
            size_t e = s;
            while (e < span_file.size() && span_z[e + 1] - span_z[e] < kLong && span_z[e + 1] - span_z[s] <= (256ull << 20)) ++e;
            stage.resize(span_z[e] - span_z[s]);
            for (size_t k = s; k < e; ++k)
                if (!pread_all(in.fd, stage.data() + (span_z[k] - span_z[s]), span_file[k], span_z[k + 1] - span_z[k], 4 << 20, threads))
                    return full_scan("the file cannot be read");
            if (oge_memcpy(cc.ctx, dz.as<uint8_t>() + span_z[s], stage.data(), stage.size(), 1)) return full_scan(oge_last_error(cc.ctx));
            s = e;
        }
        uint8_t *d_recs = nullptr;
        uint64_t *d_off = nullptr;
        if (oge_bam_decode_ranges_dev(cc.ctx, dz.as<uint8_t>(), zbytes, span_z.data(), span_file.data(), span_file.size(), d_ranges, n_ranges,
                                      n_ref, &d_recs, &d_off, &n, &bytes))
            return full_scan(oge_last_error(cc.ctx));
        dout.adopt(d_recs, bytes + 64);
        doff.adopt(d_off, (n + 1) * 8);
        oge_ctx_counter(cc.ctx, "baiq_blocks", &blocks);
    }
    if (!n) {  // no record: an empty batch of its own
        const uint64_t zero = 0;
        if (dout.alloc(64) || doff.alloc(8) || oge_memcpy(cc.ctx, doff.as<void>(), &zero, 8, 1)) return full_scan(oge_last_error(cc.ctx));
        bytes = 0;
    }
    b.header = f.header;
    b.ref_names = f.ref_names;
    b.n = n;
    b.d_recs = (uint8_t *)dout.release();
    b.d_offs = (uint64_t *)doff.release();
    b.d_bytes = bytes;
    b.dev_valid = true;
    b.host_valid = false;
    if (verbose_)
        fprintf(stderr, "[openge] FileReader (indexed): %zu regions, %llu ranges, %llu blocks, %llu of %llu bytes read (index and spans %.3f s, "
                        "load and decode %.3f s)\n", regions.size(), (unsigned long long)n_ranges, (unsigned long long)blocks,
                (unsigned long long)zbytes, (unsigned long long)fsize, sec(t0, t1), sec(t1, clk()));
    return 0;
}

// True when the next module takes per-rank input shards (run_ranks: the coordinate ReadSorter, or a
// standalone MarkDuplicates).
bool FileReader::sink_takes_shards() const {
    if (auto *rs = dynamic_cast<const ReadSorter *>(sink_)) return rs->sortBy() == BamHeaderModel::COORDINATE;
    return dynamic_cast<const MarkDuplicates *>(sink_) != nullptr;
}

// --gpus G with one input file (config 4): rank g reads the file's bytes [a_g, min(size, b_g + 64 KiB))
// into its own HBM and decodes the BGZF blocks that start in [a_g, b_g) (oge_bgzf_decode_shard: block and
// record boundaries joined with the neighbouring ranks), so the G ranks share the codec instead of rank 0
// inflating the whole file.  Returns 1 when the file cannot be opened or decoded this way (the
// whole-file readers take over and report it).
int FileReader::read_sharded(ChainContext &cc, ReadBatch &b, const std::string &path) {
    const auto t0 = clk();
    const OwnedFd file(open(path.c_str(), O_RDONLY));
    const int fd = file.fd;
    struct stat stt;
    if (fd < 0 || fstat(fd, &stt) || !S_ISREG(stt.st_mode)) return 1;
    if (cc.init_ranks()) return -1;
    const int G = cc.gpus;
    const uint64_t Z = (uint64_t)stt.st_size;
    std::vector<ReadBatch::Slice> sh(G);
    std::vector<int> rcs(G, 0);
    std::vector<std::string> why(G);
    std::vector<uint8_t> hdr(1 << 22);
    uint64_t hlen = 0;
    std::vector<double> t_read(G, 0), t_dec(G, 0);
    std::vector<std::thread> ts;
    for (int g = 0; g < G; ++g)
        ts.emplace_back([&, g]() {
            oge_ctx *c = cc.rank_ctx[g];
            const uint64_t a = Z * (uint64_t)g / (uint64_t)G, bnd = Z * (uint64_t)(g + 1) / (uint64_t)G;
            const uint64_t end = std::min<uint64_t>(Z, bnd + 65536), len = end - a;
            DevBuf dz(c);
            const auto r0 = clk();
            int rc = dz.alloc(len + 64);
            // 128 MiB chunks read as 16 MiB slices
            if (!rc && range_to_device(c, fd, a, len, dz.as<uint8_t>(), std::min<uint64_t>(len, 128ull << 20), 16ull << 20)) rc = OGE_ERR_IO;
            if (rc) why[g] = rc == OGE_ERR_IO ? std::string("read failed") : std::string(oge_last_error(c));
            const auto r1 = clk();
            const uint8_t *recs = nullptr;
            const uint64_t *offs = nullptr;
            uint64_t n = 0, hl = 0;
            // a rank whose read failed still takes part, with no buffer: its argument error fails every rank
            const int rd = oge_bgzf_decode_shard(cc.comms[g], rc ? nullptr : dz.as<uint8_t>(), len, bnd - a, &recs, &offs, &n,
                                                 g == 0 ? hdr.data() : nullptr, g == 0 ? hdr.size() : 0, g == 0 ? &hl : nullptr);
            if (!rc && rd) why[g] = oge_last_error(c);
            rcs[g] = rc ? rc : rd;
            if (g == 0) hlen = hl;
            sh[g] = {c, const_cast<uint8_t *>(recs), const_cast<uint64_t *>(offs), n};
            t_read[g] = sec(r0, r1);
            t_dec[g] = sec(r1, clk());
        });
    for (auto &t : ts) t.join();
    // a file the sharded decode rejects goes to the whole-file readers, which report format errors with
    // the reference's messages (the ranks failed together, so their communicators are still in step)
    for (int g = 0; g < G; ++g)
        if (rcs[g]) {
            if (verbose_) fprintf(stderr, "[openge] FileReader: sharded decode failed on rank %d (%s); reading the whole file\n", g, why[g].c_str());
            return 1;
        }
    BamFile f;
    std::string err;
    size_t rec_base = 0;
    if (!bam_parse_header(hdr.data(), hlen, f, err, &rec_base)) return 1;
    b.header = f.header;
    b.ref_names = f.ref_names;
    b.shards = sh;
    b.n = 0;
    for (auto &s : sh) b.n += s.n;
    b.dev_valid = b.host_valid = false;
    if (verbose_) {
        std::string per;
        for (int g = 0; g < G; ++g) {
            uint64_t nb = 0;
            oge_ctx_counter(cc.rank_ctx[g], "shard_blocks", &nb);
            char tmp[160];
            snprintf(tmp, sizeof tmp, " [rank %d: read %.3f s, decode %.3f s, %llu blocks, %llu records]", g, t_read[g], t_dec[g],
                     (unsigned long long)nb, (unsigned long long)sh[g].n);
            per += tmp;
        }
        fprintf(stderr, "[openge] FileReader (sharded over %d ranks): %.3f s%s\n", G, sec(t0, clk()), per.c_str());
    }
    return 0;
}

int FileReader::runInternal(ChainContext &cc, ReadBatch &b) {
    if (files_.empty()) files_.push_back("stdin");
    // regions are parsed against the first input's dictionary: from a look at its header, so that a region or a
    // line of the list that does not parse ends the chain before any input is read (a pipe cannot be looked at:
    // there the Filter reports it, after the read and before anything is written)
    if (auto *flt = dynamic_cast<Filter *>(sink_); flt && flt->hasRegions() && files_[0] != "stdin" && files_[0] != "-") {
        BamFile hf;
        std::vector<oge_region> parsed;
        if (peek_header(files_[0], hf) && flt->parseRegions(hf.header, parsed)) return -1;
    }
    std::vector<uint64_t> file_end;  // record count after each file
    const char *rd = getenv("OGE_READER");
    // one SAM file (first byte '@'): its text into HBM and parsed there; with --gpus on rank 0, then run_ranks'
    // unsharded distribution
    const bool one_sam = files_.size() == 1 && files_[0] != "stdin" && files_[0] != "-" && file_is_sam(files_[0]);
    if (one_sam && !(rd && std::string(rd) == "host")) return read_sam_device(cc, files_[0], sink_sorts(), b);
    // the byte-range sharded reader by default only over the host-staged transport, where every multi-rank
    // test ran; over RCCL (an 8-GPU node) it is opt-in (OGE_READER=sharded) until a G > 1 RCCL run of it has
    // been recorded: its rank joins and tail fetch are collectives that a fall-back cannot undo
    const bool want_shards = cc.gpus > 1 && files_.size() == 1 && files_[0] != "stdin" && files_[0] != "-" && sink_takes_shards() &&
                             !one_sam && !(rd && (std::string(rd) == "host" || std::string(rd) == "whole"));
    if (want_shards && cc.init_ranks()) return -1;  // the ranks (and so the transport) are needed here anyway
    const bool rccl = !cc.comms.empty() && cc.comms[0] && std::string(oge_comm_transport(cc.comms[0])) == "rccl";
    if (want_shards && (!rccl || (rd && std::string(rd) == "sharded"))) {
        const int r = read_sharded(cc, b, files_[0]);
        if (r <= 0) return r;  // 1: the host reader reports why the file cannot be read
    }
    if (files_.size() == 1 && files_[0] != "stdin" && files_[0] != "-" && !one_sam && !(rd && std::string(rd) == "host")) {
        auto *flt = dynamic_cast<Filter *>(sink_);
        if (flt && flt->hasRegions() && cc.gpus == 1 && !no_index_) {
            const int ri = read_indexed(cc, b, files_[0]);
            if (ri <= 0) return ri;  // 1: the full scan below
        }
        const int r = read_device(cc, b, files_[0]);
        if (r <= 0) return r;  // 1: fall through to the host reader (it reports format errors)
    }
    prefetch_drop();  // the host reader reads the file itself
    for (size_t i = 0; i < files_.size(); ++i) {
        const std::string path = files_[i] == "stdin" ? "/dev/stdin" : files_[i];
        BamFile f;
        std::string err;
        const int threads = cc.threads > 0 ? cc.threads : 8;
        const bool is_stdin = path == "/dev/stdin" || path == "-";
        if (is_stdin || file_is_sam(path)) {  // a pipe cannot be looked at first: read it, then decide by its first byte
            bytevec raw, stream;
            bool ok = read_file_bytes(is_stdin ? "stdin" : path, raw, threads, err);
            if (ok && !raw.empty() && raw[0] == '@') {
                if (sam_host_file(cc, files_[i], raw, f)) return -1;
            } else {
                ok = ok && bgzf_inflate_all(raw.data(), raw.size(), stream, threads, err) && bam_parse(std::move(stream), f, err, threads);
            }
            if (!ok) {
                fprintf(stderr, "openge: error reading %s: %s\n", files_[i].c_str(), err.c_str());
                return -1;
            }
        } else if (!bam_read_file(path, f, threads, err)) {
            fprintf(stderr, "openge: error reading %s: %s\n", files_[i].c_str(), err.c_str());
            return -1;
        }
        if (i == 0) {  // take the decompressed stream as it is: records start at rec_base
            b.header = f.header;
            b.ref_names = f.ref_names;
            const uint64_t base = f.rec_base;
            b.offs.resize(f.offsets.size());
            for (size_t k = 0; k < f.offsets.size(); ++k) b.offs[k] = base + f.offsets[k];
            b.recs = std::move(f.data);
        } else {
            if (f.header.sq.size() != b.header.sq.size() || f.ref_names != b.ref_names)  // read_stream_reader.h:116-124
                fprintf(stderr, "Warning; sequence headers vary between files. Data may be corrupt.\n");
            const uint64_t base = b.recs.size();
            b.recs.insert(b.recs.end(), f.recs(), f.recs() + f.rec_bytes());
            for (uint64_t o : f.offsets) b.offs.push_back(base + o);
        }
        file_end.push_back(b.offs.size());
    }
    b.n = b.offs.size();
    b.offs.push_back(b.recs.size());
    b.recs.resize(b.recs.size() + 16, 0);
    b.host_valid = true;
    if (files_.size() > 1 && !sink_sorts()) return merge_inputs(b, file_end, cc.threads);
    return 0;
}

// True when the records go straight (or through a Filter) into a ReadSorter: the sort then makes
// the MultiReader's interleaving irrelevant (records it would order differently are full ByPosition
// ties, ordered by heap address in the reference).
bool FileReader::sink_sorts() const {
    const AlgorithmModule *m = sink_;
    if (m && dynamic_cast<const Filter *>(m)) m = m->sink();
    return m && dynamic_cast<const ReadSorter *>(m);
}

// Sort::ByPosition (util/bamtools/Sort.h:116-133) down to the flag, as a three-way compare; refID
// -1 sorts last and is equivalent to every other refID -1 record.
static int bypos_cmp(const uint8_t *a, const uint8_t *b) {
    const int32_t ra = oge_rd_i32(a + 4), rb = oge_rd_i32(b + 4);
    if (ra == -1 || rb == -1) return (ra == -1) - (rb == -1);
    if (ra != rb) return ra < rb ? -1 : 1;
    const int32_t pa = oge_rd_i32(a + 8), pb = oge_rd_i32(b + 8);
    if (pa != pb) return pa < pb ? -1 : 1;
    const uint16_t fa = oge_rd_u16(a + 18), fb = oge_rd_u16(b + 18);
    const bool va = fa & 0x10, vb = fb & 0x10;
    if (va != vb) return va ? 1 : -1;
    const int la = a[12] - 1, lb = b[12] - 1;
    const int c = memcmp(a + 36, b + 36, (size_t)std::min(la, lb));
    if (c) return c < 0 ? -1 : 1;
    if (la != lb) return la < lb ? -1 : 1;
    if (fa != fb) return fa < fb ? -1 : 1;
    return 0;
}

// MultiReader::read (util/read_stream_reader.h:132-153): the inputs are interleaved by a
// std::multiset of one head per file ordered by ByPosition, so equivalent heads leave in insertion
// order.  A binary heap keyed on (ByPosition, insertion number) reproduces it exactly, for sorted
// and unsorted inputs alike (the reference's final address tie-break is replaced by insertion
// order, Q10).  The arena is then rewritten in that order.
int FileReader::merge_inputs(ReadBatch &b, const std::vector<uint64_t> &file_end, int threads) {
    struct Head {
        uint64_t rec, end, seq;
    };
    const uint8_t *base = b.recs.data();
    auto later = [&](const Head &x, const Head &y) {  // heap "less": x leaves after y
        const int c = bypos_cmp(base + b.offs[x.rec], base + b.offs[y.rec]);
        return c ? c > 0 : x.seq > y.seq;
    };
    std::vector<Head> heap;
    uint64_t seq = 0, begin = 0;
    for (uint64_t e : file_end) {  // MultiReader::open: one read from each file, in file order
        if (e > begin) heap.push_back({begin, e, seq++});
        begin = e;
    }
    std::make_heap(heap.begin(), heap.end(), later);
    std::vector<uint64_t> order;
    order.reserve(b.n);
    while (!heap.empty()) {
        std::pop_heap(heap.begin(), heap.end(), later);
        Head h = heap.back();
        heap.pop_back();
        order.push_back(h.rec);
        if (++h.rec < h.end) {
            h.seq = seq++;
            heap.push_back(h);
            std::push_heap(heap.begin(), heap.end(), later);
        }
    }
    bytevec out;
    out.resize(b.recs.size());
    std::vector<uint64_t> offs(b.n + 1);
    for (uint64_t k = 0; k < b.n; ++k) offs[k + 1] = offs[k] + (b.offs[order[k] + 1] - b.offs[order[k]]);
    const uint64_t shift = b.offs[0];  // keep the reader's leading bytes (header) where they were
    const int T = std::max(1, threads);
    std::vector<std::thread> ts;
    for (int t = 0; t < T; ++t)
        ts.emplace_back([&, t]() {
            for (uint64_t k = (uint64_t)t; k < b.n; k += (uint64_t)T)
                memcpy(out.data() + shift + offs[k], base + b.offs[order[k]], offs[k + 1] - offs[k]);
        });
    for (auto &t : ts) t.join();
    memcpy(out.data(), base, shift);
    memset(out.data() + shift + offs[b.n], 0, out.size() - shift - offs[b.n]);
    for (auto &o : offs) o += shift;
    b.recs = std::move(out);
    b.offs = std::move(offs);
    return 0;
}

// ----------------------------------------------------------------------------------- dedup opts
// The dedup options of a batch: its header's RG -> library table (lib_table.h), which they point into
static oge_markdup_opts markdup_opts(const LibTable &lt, const ReadBatch &b, bool compat, int split) {
    return lt.opts((int32_t)b.ref_names.size(), compat ? 1 : 0, split);
}

// MarkDuplicates::metricsFilename: the module's counters sized and named for this header's libraries (once per
// chain), and the counts of one more part of the marked output added to them
static void metrics_begin(MarkDuplicates *md, const LibTable &lt) {
    md->metricsLibraries = lt.names;
    md->metricsUnknown = lt.unknown_lib;
    md->metrics.assign((size_t)lt.n_lib, OgeDupMetrics{});
    md->metricsMs = 0;
    if (md->opticalDistance >= 0) {
        md->sets.assign((size_t)lt.n_lib, OgeDupSetsLib{});
        md->setsHist.assign(3 * OGE_DUP_SETS_BINS, 0);
        md->setsMs = 0;
        md->setsTiers[0] = md->setsTiers[1] = md->setsTiers[2] = 0;
    }
}
static int metrics_count(MarkDuplicates *md, oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_offs, uint64_t n, const oge_markdup_opts &o) {
    std::vector<OgeDupMetrics> part(md->metrics.size());
    if (oge_dup_metrics_dev(ctx, d_recs, d_offs, n, &o, (int32_t)part.size(), part.data())) return -1;
    for (size_t k = 0; k < part.size(); ++k) add_metrics(md->metrics[k], part[k]);
    double ms = 0;
    if (!oge_ctx_timing(ctx, "dup_metrics", &ms) && ms > 0) md->metricsMs += ms;
    if (md->opticalDistance < 0) return 0;
    // --optical-distance: the duplicate sets of the same records, which are all resident here
    if (oge_dup_sets_dev(ctx, d_recs, d_offs, n, &o, md->opticalDistance, (int32_t)md->sets.size(), md->sets.data(), md->setsHist.data())) return -1;
    if (!oge_ctx_timing(ctx, "dup_sets", &ms) && ms > 0) md->setsMs = ms;
    const char *tiers[3] = {"dupsets_wave_sets", "dupsets_block_sets", "dupsets_host_sets"};
    for (int k = 0; k < 3; ++k) oge_ctx_counter(ctx, tiers[k], &md->setsTiers[k]);
    return 0;
}

// One row for every library an @RG names, one more row for the unknown library when none does and a record
// resolved to it (names by library id, "" = not named); oge_dup_metrics_text sorts them.
// sets / hist (--optical-distance; sets by library id as m): the text of oge_dup_sets_text
static int metrics_text(const std::vector<std::string> &names, int unknown, const std::vector<OgeDupMetrics> &m, const std::string &command_line,
                        std::string &text, const std::vector<OgeDupSetsLib> *sets = nullptr, const uint64_t *hist = nullptr) {
    std::vector<const char *> row_names;
    std::vector<OgeDupMetrics> rows;
    std::vector<OgeDupSetsLib> srows;
    for (size_t k = 0; k < names.size() && k < m.size(); ++k)
        if (!names[k].empty()) {
            row_names.push_back(names[k].c_str()), rows.push_back(m[k]);
            if (sets) srows.push_back((*sets)[k]);
        }
    if (unknown >= 0 && (size_t)unknown < m.size() && names[unknown].empty()) {
        const OgeDupMetrics &u = m[unknown];
        if (u.unpaired_examined | u.pair_reads_examined | u.secondary | u.unmapped | u.unpaired_dups | u.pair_read_dups) {
            row_names.push_back("Unknown Library"), rows.push_back(u);
            if (sets) srows.push_back((*sets)[unknown]);
        }
    }
    std::string cl = command_line;
    while (!cl.empty() && cl.back() == ' ') cl.pop_back();
    uint64_t need = 0;
    if (sets) {
        if (oge_dup_sets_text(row_names.data(), rows.data(), srows.data(), (int32_t)rows.size(), hist, cl.c_str(), nullptr, 0, &need)) return -1;
        text.resize(need + 1);
        if (oge_dup_sets_text(row_names.data(), rows.data(), srows.data(), (int32_t)rows.size(), hist, cl.c_str(), &text[0], need + 1, &need)) return -1;
        text.resize(need);
        return 0;
    }
    if (oge_dup_metrics_text(row_names.data(), rows.data(), (int32_t)rows.size(), cl.c_str(), nullptr, 0, &need)) return -1;
    text.resize(need + 1);
    if (oge_dup_metrics_text(row_names.data(), rows.data(), (int32_t)rows.size(), cl.c_str(), &text[0], need + 1, &need)) return -1;
    text.resize(need);
    return 0;
}

// data[0, bytes) as the whole of a new file; on an error its message, no file left behind and -1
static int write_whole_file(const std::string &path, const void *data, size_t bytes) {
    FILE *f = fopen(path.c_str(), "wb");
    const bool ok = f && fwrite(data, 1, bytes, f) == bytes;
    if ((f && fclose(f) != 0) || !ok) {
        fprintf(stderr, "openge: error writing %s: %s\n", path.c_str(), strerror(errno));
        remove(path.c_str());
        return -1;
    }
    return 0;
}
// the same bytes to the standard output, flushed, when `out` is "stdout" or "-"; else to the file of that name
static int write_stdout_or_file(const std::string &out, const void *data, size_t bytes) {
    if (out != "stdout" && out != "-") return write_whole_file(out, data, bytes);
    if (fwrite(data, 1, bytes, stdout) == bytes && fflush(stdout) == 0 && !ferror(stdout)) return 0;
    fprintf(stderr, "openge: error writing to stdout\n");
    return -1;
}

int MarkDuplicates::writeMetrics() const {
    std::string text;
    const bool optical = opticalDistance >= 0;
    if (metrics_text(metricsLibraries, metricsUnknown, metrics, metricsCommandLine, text, optical ? &sets : nullptr, optical ? setsHist.data() : nullptr)) {
        fprintf(stderr, "openge: MarkDuplicates: metrics: %s\n", oge_last_error(nullptr));
        return -1;
    }
    if (write_whole_file(metricsFilename, text.data(), text.size())) return -1;
    if (verbose_) fprintf(stderr, "[openge] MarkDuplicates: metrics of %zu libraries to %s, stage dup_metrics %.3f ms\n",
                          (size_t)std::count_if(metricsLibraries.begin(), metricsLibraries.end(), [](const std::string &s) { return !s.empty(); }),
                          metricsFilename.c_str(), metricsMs);
    if (verbose_ && optical)
        fprintf(stderr, "[openge] MarkDuplicates: duplicate sets at optical distance %lld, stage dup_sets %.3f ms, sets of two or more pairs: "
                        "%llu in a wave, %llu in a workgroup, %llu on the host\n",
                (long long)opticalDistance, setsMs, (unsigned long long)setsTiers[0], (unsigned long long)setsTiers[1], (unsigned long long)setsTiers[2]);
    return 0;
}

// ----------------------------------------------------------------------------------- Filter
bool Filter::setReadLengths(const std::string &s) {
    int a = 0, z = 0;
    char junk;
    bool ok;
    if (!s.empty() && s[0] == '+') {
        ok = sscanf(s.c_str(), "%c%d", &junk, &a) == 2;
        z = INT32_MAX;
    } else if (!s.empty() && s[0] == '-') {
        ok = sscanf(s.c_str(), "%c%d", &junk, &z) == 2;
        a = INT32_MIN;
    } else if (s.find('-') != std::string::npos) {
        ok = sscanf(s.c_str(), "%d%c%d", &a, &junk, &z) == 3;
    } else {
        ok = sscanf(s.c_str(), "%d", &a) == 1;
        z = a;
    }
    if (!ok) {  // filter.cpp:179-182
        fprintf(stderr, "Error parsing read length requirements. Aborting.\n"
                        "Valid ranges look like: 64, or 64-72, or -64, or +64.\n");
        exit(-1);
    }
    opts_.min_len = a;
    opts_.max_len = z;
    return true;
}

bool Filter::setRegionsFile(const std::string &path) {
    FILE *f = fopen(path.c_str(), "r");
    if (!f) {
        fprintf(stderr, "openge: cannot read the regions file %s\n", path.c_str());
        return false;
    }
    regions_file_ = path;
    std::string line;
    uint64_t no = 0;
    for (int c = 0; c != EOF;) {
        c = fgetc(f);
        if (c != '\n' && c != EOF) {
            line.push_back((char)c);
            continue;
        }
        if (c == EOF && line.empty()) break;
        ++no;
        while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
        if (!line.empty() && line[0] != '#') more_regions_.push_back({line, no});
        line.clear();
    }
    fclose(f);
    return true;
}

int Filter::parseRegions(const BamHeaderModel &h, std::vector<oge_region> &out) const {
    std::string names;
    std::vector<int64_t> lens;
    for (auto &sq : h.sq) {
        names += sq.name;
        names.push_back('\0');
        lens.push_back(sq.length);
    }
    auto one = [&](const std::string &text, uint64_t line) {
        oge_filter_opts o = opts_;
        if (oge_parse_region(text.c_str(), names.data(), (int32_t)lens.size(), lens.data(), &o)) {
            // filter.cpp:243-247: the parse error, then the generic message, then exit(-1)
            const std::string why = oge_last_error(nullptr);
            if (line) fprintf(stderr, "openge: %s line %llu: %s\n", regions_file_.c_str(), (unsigned long long)line, why.c_str());
            else if (why.rfind("ERROR: could not parse", 0) != 0) fprintf(stderr, "%s\n", why.c_str());
            fprintf(stderr, "ERROR: could not parse region'%s'\n"
                            "Check that region description is in valid format (see documentation) and that the "
                            "coordinates are valid\n", text.c_str());
            return false;
        }
        out.push_back({o.ref_id, o.left_pos, o.right_pos});
        return true;
    };
    if (has_region_ && !one(region_, 0)) return -1;
    for (auto &rl : more_regions_)
        if (!one(rl.text, rl.line)) return -1;
    return 0;
}

int Filter::runInternal(ChainContext &cc, ReadBatch &b) {
    oge_filter_opts o = opts_;
    std::vector<oge_region> regions;
    if (hasRegions()) {
        if (verbose_ && has_region_) fprintf(stderr, "Filtering to region %s\n", region_.c_str());
        if (parseRegions(b.header, regions)) return -1;
        if (verbose_ && !more_regions_.empty()) fprintf(stderr, "Filtering to %zu regions\n", regions.size());
        if (regions.size() == 1) {  // one region in all: the single-region predicate
            o.has_region = 1;
            o.ref_id = regions[0].ref_id;
            o.left_pos = regions[0].left_pos;
            o.right_pos = regions[0].right_pos;
            regions.clear();
        }
    }
    if (cc.to_device(b)) return -1;
    DevBuf out(cc.ctx), out_off(cc.ctx);
    if (out.alloc(b.d_bytes + 64) || out_off.alloc((b.n + 1) * 8)) return cc.fail("device allocation");
    uint64_t m = 0, bytes = 0;
    int rc = regions.empty() ? oge_filter_records_dev(cc.ctx, b.d_recs, b.d_offs, b.n, &o, out.as<uint8_t>(), out_off.as<uint64_t>(), &m)
                             : oge_filter_regions_dev(cc.ctx, b.d_recs, b.d_offs, b.n, &o, regions.data(), regions.size(),
                                                      out.as<uint8_t>(), out_off.as<uint64_t>(), &m);
    if (!rc) rc = oge_memcpy(cc.ctx, &bytes, out_off.as<uint64_t>() + m, 8, 2);
    if (!rc) rc = oge_ctx_sync(cc.ctx);
    if (rc) return cc.fail("Filter");
    cc.free_device(b);
    b.d_recs = (uint8_t *)out.release();
    b.d_offs = (uint64_t *)out_off.release();
    b.d_bytes = bytes;
    b.n = m;
    b.dev_valid = true;
    b.host_valid = false;
    kept = m;
    if (verbose_) fprintf(stderr, "%llu alignments processed.\n", (unsigned long long)m);
    return 0;
}

// ----------------------------------------------------------------------------------- ReadSorter
// One GPU, and the chain's records (+ the sort's second arena and workspace) do not fit free HBM,
// or OGE_CHUNK_BYTES forces the chunked path (tests).
static bool use_chunked(ChainContext &cc, const ReadBatch &b) {
    if (cc.gpus > 1) return false;
    if (getenv("OGE_CHUNK_BYTES")) return true;
    if (b.dev_valid) return false;  // the reader already holds them in HBM
    uint64_t fr = 0, tot = 0;
    if (oge_mem_info(cc.ctx, &fr, &tot)) return false;
    return b.bytes() / 10 * 25 + b.n * 100 > fr;
}

int ReadSorter::runInternal(ChainContext &cc, ReadBatch &b) {
    if (order_ != BamHeaderModel::COORDINATE && order_ != BamHeaderModel::QUERYNAME) {
        fprintf(stderr, "openge: unsupported sort order\n");
        return -1;
    }
    MarkDuplicates *md = order_ == BamHeaderModel::COORDINATE ? dynamic_cast<MarkDuplicates *>(sink_) : nullptr;
    if (cc.gpus > 1 && order_ == BamHeaderModel::COORDINATE) {  // --gpus G: range-split sort (+ dedup) over G ranks
        const LibTable lt(b.header);
        oge_markdup_opts o = {};
        if (md) o = markdup_opts(lt, b, md->compatNonverbose, md->splitChains);
        const bool count = md && !md->metricsFilename.empty();
        if (count) metrics_begin(md, lt);
        uint64_t nd = 0;
        const auto t0 = clk();
        if (run_ranks(cc, b, true, md ? &o : nullptr, &nd, count ? &md->metrics : nullptr, count ? &md->metricsMs : nullptr)) return -1;
        if (md) md->duplicates = nd;
        b.header.sort_order = order_;
        if (verbose_)
            fprintf(stderr, "[openge] ReadSorter: %d ranks, %.3f s\n", cc.gpus,
                    sec(t0, clk()));
        return 0;
    }
    if (order_ == BamHeaderModel::COORDINATE && use_chunked(cc, b) && md && md->opticalDistance >= 0) {
        // the duplicate sets need every record resident in HBM at once; refused here, before the writer opens the output
        fprintf(stderr, "openge mergesort: --optical-distance needs the records resident in HBM, and this input takes the chunked path "
                        "(larger than HBM, or OGE_CHUNK_BYTES)\n");
        return -1;
    }
    if (order_ == BamHeaderModel::COORDINATE && use_chunked(cc, b)) {
        // larger than HBM: sorted runs spilled into the host arena, key ranges sorted on the device,
        // produced range by range when the writer asks (oge_sort_markdup_chunked)
        if (cc.to_host(b)) return -1;
        cc.free_device(b);
        auto arena = std::make_shared<ReadBatch>();
        arena->recs = std::move(b.recs);
        arena->offs = std::move(b.offs);
        const auto lt = std::make_shared<LibTable>(b.header);  // lives as long as the closure whose options point into it
        oge_markdup_opts mo = {};
        if (md) mo = markdup_opts(*lt, b, md->compatNonverbose, md->splitChains);
        const char *ce = getenv("OGE_CHUNK_BYTES");
        const uint64_t chunk = ce ? strtoull(ce, nullptr, 10) : 0, n = b.n;
        const int32_t n_ref = (int32_t)b.ref_names.size();
        b.produce = [arena, lt, mo, md, chunk, n, n_ref](ChainContext &c, const ReadBatch::RangeSink &sink) -> int {
            // --metrics: every marked range is counted in front of the sink (which may drop its duplicates)
            const bool count = md && !md->metricsFilename.empty();
            if (count) metrics_begin(md, *lt);
            const ReadBatch::RangeSink counted = [&](const uint8_t *r, const uint64_t *o, uint64_t m) -> int {
                if (metrics_count(md, c.ctx, r, o, m, mo)) return c.fail("MarkDuplicates: metrics");
                return sink(r, o, m);
            };
            struct Tramp {
                const ReadBatch::RangeSink *s;
                static int call(void *u, const uint8_t *r, const uint64_t *o, uint64_t m) { return (*((Tramp *)u)->s)(r, o, m); }
            } tr{count ? &counted : &sink};
            uint64_t nd = 0, runs = 0, ranges = 0;
            const int rc = oge_sort_markdup_chunked(c.ctx, arena->recs.data(), arena->offs.data(), n, n_ref, md ? &mo : nullptr,
                                                    chunk, &Tramp::call, &tr, &nd, &runs, &ranges);
            if (rc) return c.fail("ReadSorter (chunked)");
            if (md) md->duplicates = nd;
            if (verbose_)
                fprintf(stderr, "[openge] ReadSorter: %llu records in %llu sorted runs, output in %llu key ranges\n",
                        (unsigned long long)n, (unsigned long long)runs, (unsigned long long)ranges);
            return 0;
        };
        b.host_valid = false;
        b.header.sort_order = order_;
        return 0;
    }
    const auto t0 = clk();
    if (cc.to_device(b)) return -1;
    const auto t1 = clk();
    DevBuf perm_buf(cc.ctx), out_buf(cc.ctx), off_buf(cc.ctx);
    if (perm_buf.alloc(b.n * 4 + 4) || out_buf.alloc(b.d_bytes + 64) || off_buf.alloc((b.n + 1) * 8)) return cc.fail("device allocation");
    uint32_t *perm = perm_buf.as<uint32_t>();
    uint8_t *out = out_buf.as<uint8_t>();
    uint64_t *out_off = off_buf.as<uint64_t>();
    if (verbose_) oge_ctx_sync(cc.ctx);
    const auto t1a = clk();
    int rc;
    const LibTable lt(b.header);
    oge_markdup_opts m = {};
    if (order_ == BamHeaderModel::QUERYNAME) {  // -b; a MarkDuplicates sink then runs on its own
        rc = oge_sort_name_dev(cc.ctx, b.d_recs, b.d_offs, b.n, perm);
        if (!rc) rc = oge_gather_records_dev(cc.ctx, b.d_recs, b.d_offs, perm, b.n, out, out_off);
    } else if (md) {  // mergesort -M: one fused device pipeline (sort, dedup, gather with 0x400 applied)
        m = markdup_opts(lt, b, md->compatNonverbose, md->splitChains);
        uint64_t nd = 0;
        rc = oge_sort_markdup_dev(cc.ctx, b.d_recs, b.d_offs, b.n, &m, perm, out, out_off, &nd);
        md->duplicates = nd;
    } else {
        rc = oge_sort_coord_dev(cc.ctx, b.d_recs, b.d_offs, b.n, (int32_t)b.ref_names.size(), perm);
        if (!rc) rc = oge_gather_records_dev(cc.ctx, b.d_recs, b.d_offs, perm, b.n, out, out_off);
    }
    if (!rc) rc = oge_ctx_sync(cc.ctx);
    if (verbose_) {
        fprintf(stderr, "[openge] ReadSorter: host->device %.3f s, output allocation %.3f s, device pipeline %.3f s\n", sec(t0, t1),
                sec(t1, t1a), sec(t1a, clk()));
        std::string st;  // HIP-event stage times of the device pipeline (ms)
        for (const char *s : {"input_pass", "sort_radix", "sort_ties", "meta_gather", "md_matejoin", "md_pairs", "md_frags",
                              "md_apply", "gather_offsets", "gather_records", "name_sort"}) {
            double ms = -1;
            if (!oge_ctx_timing(cc.ctx, s, &ms) && ms >= 0) st += std::string(" ") + s + "=" + std::to_string(ms).substr(0, 6);
        }
        fprintf(stderr, "[openge] ReadSorter stages (ms):%s\n", st.c_str());
    }
    if (rc) return cc.fail("ReadSorter");
    if (md && order_ == BamHeaderModel::COORDINATE && !md->metricsFilename.empty()) {  // --metrics: the marked output, before any removal
        metrics_begin(md, lt);
        if (metrics_count(md, cc.ctx, out, out_off, b.n, m)) return cc.fail("MarkDuplicates: metrics");
    }
    cc.free_device(b);
    b.d_recs = (uint8_t *)out_buf.release();
    b.d_offs = (uint64_t *)off_buf.release();
    b.dev_valid = true;
    b.host_valid = false;
    b.header.sort_order = order_;  // read_sorter.cpp:257-258
    return 0;
}

// ----------------------------------------------------------------------------------- MarkDuplicates
int MarkDuplicates::runInternal(ChainContext &cc, ReadBatch &b) {
    if (cc.gpus > 1) {  // --gpus G: every rank marks its input range in place order
        if (compatNonverbose) {
            fprintf(stderr, "openge: --compat-nonverbose-dedup is one-GPU only\n");
            return -1;
        }
        const LibTable lt(b.header);
        const oge_markdup_opts m = markdup_opts(lt, b, false, splitChains);
        const bool count = !metricsFilename.empty();
        if (count) metrics_begin(this, lt);
        uint64_t nd = 0;
        if (run_ranks(cc, b, false, &m, &nd, count ? &metrics : nullptr, count ? &metricsMs : nullptr)) return -1;
        duplicates = nd;
        b.drop_duplicates = removeDuplicates;
        return 0;
    }
    if (cc.to_device(b)) return -1;
    DevBuf dup(cc.ctx);
    if (dup.alloc(b.n + 1)) return cc.fail("device allocation");
    const LibTable lt(b.header);
    const oge_markdup_opts m = markdup_opts(lt, b, compatNonverbose, splitChains);
    uint64_t nd = 0;
    if (oge_markdup_dev(cc.ctx, b.d_recs, b.d_offs, b.n, &m, dup.as<uint8_t>(), 1, &nd) || oge_ctx_sync(cc.ctx)) return cc.fail("MarkDuplicates");
    duplicates = nd;
    if (!metricsFilename.empty()) {  // the records carry their final FLAG now; -r drops them in the writer
        metrics_begin(this, lt);
        if (metrics_count(this, cc.ctx, b.d_recs, b.d_offs, b.n, m)) return cc.fail("MarkDuplicates: metrics");
    }
    b.host_valid = false;
    b.drop_duplicates = removeDuplicates;
    return 0;
}

// ----------------------------------------------------------------------------------- LocalRealignment

// --gpus G: one realignment over the whole input whose per-interval device work (consensus
// generation, the offset scan) is spread over the G ranks' devices by interval ranges balanced by reads
// (oge_localrealign_multi) -- cuts fall inside contigs too, so a single-contig input shards; the binning,
// the decisions and the mate-fixing writer run once, on all host threads, so the output is the one-GPU
// output.  (Until r05 each rank realigned a range of whole contigs on its own, and a mate-fixer backlog at a
// shard boundary aborted the run.)
static int realign_ranks(ChainContext &cc, ReadBatch &b, const std::string &ht, const std::string &ref, const std::string &iv,
                         bool verbose) {
    if (cc.init_ranks()) return -1;
    const int G = cc.gpus;
    oge_realign_opts o;
    oge_realign_opts_init(&o);
    o.threads = cc.threads;
    oge_realign_result *r = nullptr;
    if (oge_localrealign_multi(cc.rank_ctx.data(), G, ht.data(), ht.size(), b.recs.data(), b.offs.data(), b.n, ref.c_str(), iv.c_str(),
                               &o, &r))
        return cc.fail("LocalRealignment");
    if (verbose) fprintf(stderr, "[openge] LocalRealignment over %d devices: %s\n", G, oge_realign_result_stats(r));
    const uint64_t m = oge_realign_result_count(r);
    oge_realign_result_take(r, b.recs, b.offs);  // the records and offsets, moved (offsets from 0, 16 bytes of slack)
    oge_realign_result_free(r);
    if (b.offs.size() != m + 1) b.offs.assign(m + 1, 0);
    b.n = m;
    return 0;
}

static void report_targets(const oge_targets_result &r, int max_interval, int gap);

// --auto-targets: the intervals of `openge targets` at its defaults, from the batch where it lies (the device
// form when it is valid, else through the host form), written to <tmpdir>/oge_targets_<pid>.intervals.
// *n_targets = 0: nothing to realign, no file.
int LocalRealignment::auto_targets(ChainContext &cc, ReadBatch &b, std::string &path, uint64_t *n_targets) {
    const size_t n_ref = b.ref_names.size();
    if (b.header.sq.size() != n_ref) {
        fprintf(stderr, "openge localrealign: --auto-targets needs a header whose @SQ lines match the reference list\n");
        return -1;
    }
    std::vector<int32_t> lens;
    std::string names;
    for (size_t r = 0; r < n_ref; ++r) {
        lens.push_back((int32_t)std::min<long long>(std::max<long long>(b.header.sq[r].length, 0), INT32_MAX));
        names.append(b.ref_names[r].c_str(), b.ref_names[r].size() + 1);
    }
    oge_targets_opts o;
    oge_targets_opts_init(&o);
    oge_targets_result res;
    std::vector<uint8_t> text;
    int rc;
    if (b.dev_valid) {
        const oge_target *d_targets = nullptr;
        const uint8_t *d_text = nullptr;
        rc = oge_targets_dev(cc.ctx, b.d_recs, b.d_offs, b.n, (int32_t)n_ref, lens.data(), names.data(), names.size(), &o, &res, &d_targets,
                             &d_text);
        if (!rc && res.text_bytes) {
            text.resize(res.text_bytes);
            rc = oge_memcpy(cc.ctx, text.data(), d_text, res.text_bytes, 2);
        }
    } else {
        if (cc.to_host(b)) return -1;
        std::vector<oge_target> tg;
        const uint64_t bytes = b.n ? b.offs[b.n] : 0;
        auto call = [&]() {
            return oge_targets(cc.ctx, b.recs.data(), bytes, b.offs.data(), b.n, (int32_t)n_ref, lens.data(), names.data(), names.size(), &o, &res,
                               tg.data(), tg.size(), text.data(), text.size());
        };
        rc = call();  // sizes the outputs
        if (rc == OGE_ERR_LIMIT && res.targets) {
            tg.resize(res.targets);
            text.resize(res.text_bytes);
            rc = call();
        }
    }
    if (rc) return cc.fail("LocalRealignment: targets");
    if (verbose) report_targets(res, o.max_interval, o.gap);
    *n_targets = res.targets;
    if (!res.targets) return 0;
    path = tmpdir_ + (tmpdir_.empty() || tmpdir_.back() == '/' ? "" : "/") + "oge_targets_" + std::to_string((long long)getpid()) + ".intervals";
    return write_whole_file(path, text.data(), text.size());
}

int LocalRealignment::runInternal(ChainContext &cc, ReadBatch &b) {
    const auto t0 = clk();
    // the computed intervals file lives until the realigner has read it
    struct TempFile {
        std::string path;
        ~TempFile() {
            if (!path.empty()) remove(path.c_str());
        }
    } temp;
    if (auto_targets_) {
        uint64_t n_targets = 0;
        if (auto_targets(cc, b, temp.path, &n_targets)) return -1;
        if (!n_targets) {  // the realigner's parser refuses an empty file: the records pass through as they are
            if (verbose) fprintf(stderr, "[openge] LocalRealignment: no targets, the records pass through unchanged\n");
            return 0;
        }
        intervals_ = temp.path;
    }
    if (cc.to_host(b)) return -1;
    cc.free_device(b);
    const std::string ht = b.header.to_string();
    if (cc.gpus > 1) return realign_ranks(cc, b, ht, reference_, intervals_, verbose);
    oge_realign_opts o;
    oge_realign_opts_init(&o);
    o.threads = cc.threads;
    oge_realign_result *r = nullptr;
    const auto t1 = clk();
    if (oge_localrealign(cc.ctx, ht.data(), ht.size(), b.recs.data(), b.offs.data(), b.n, reference_.c_str(),
                         intervals_.c_str(), &o, &r))
        return cc.fail("LocalRealignment");
    const auto t2 = clk();
    uint64_t bytes = 0;
    const uint8_t *rp = oge_realign_result_records(r, &bytes);
    const uint64_t *op = oge_realign_result_offsets(r);
    const uint64_t n = oge_realign_result_count(r);
    // OGE_WRITE_DEVICE=1: the result goes straight up to the device when it fits and the writer deflates it
    // there (a host module downloads it again).  Otherwise (default) the host batch takes it in a threaded
    // copy into huge pages -- one thread copying into fresh 4 KiB pages took 0.52 s for the 1.1 GB C5 result
    // -- and the writer compresses it with the host codec (zlib-class level 6, as the reference writes).
    uint64_t fr = 0, tot = 0;
    const uint64_t base = n ? op[0] : 0, len = n ? op[n] - base : 0;
    DevBuf dr(cc.ctx), dof(cc.ctx);
    bool up = n && write_device_forced() && !bgzf_host_codec_forced() && !oge_mem_info(cc.ctx, &fr, &tot) &&
              2 * len + (n + 1) * 16 + (256ull << 20) < fr;
    if (up) {
        std::vector<uint64_t> ro(op, op + n + 1);
        for (auto &x : ro) x -= base;
        up = !dr.alloc(len + 64) && !dof.alloc((n + 1) * 8) && !oge_memcpy(cc.ctx, dr.as<void>(), rp + base, len, 1) &&
             !oge_memcpy(cc.ctx, dof.as<void>(), ro.data(), (n + 1) * 8, 1);
        if (up) {
            b.recs.clear();
            b.recs.shrink_to_fit();
            b.offs.clear();
            b.offs.shrink_to_fit();
            b.d_recs = (uint8_t *)dr.release();
            b.d_offs = (uint64_t *)dof.release();
            b.d_bytes = len;
            b.dev_valid = true;
            b.host_valid = false;
        }
    }
    if (verbose) fprintf(stderr, "[openge] LocalRealignment: %s\n", oge_realign_result_stats(r));
    if (!up) {
        // the host batch takes the result's own buffers (r06: no copy; r05 copied the 1.1 GB C5 result into
        // fresh huge pages on 16 threads, 0.06 s, and unmapped the library's copy, another 0.06 s)
        oge_realign_result_take(r, b.recs, b.offs);  // (the input's host copy is unmapped here: a background unmap
                                                     // measured slower, its mm lock stalling the writer's threads)
        if (b.offs.size() != n + 1) b.offs.assign(n + 1, 0);
    }
    (void)rp;
    b.n = n;
    const auto t3 = clk();
    oge_realign_result_free(r);
    if (verbose)
        fprintf(stderr, "[openge] LocalRealignment: records to host %.3f s, realign %.3f s, result %s %.3f s, release %.3f s\n",
                sec(t0, t1), sec(t1, t2), up ? "to the device" : "host copy", sec(t2, t3), sec(t3, clk()));
    return 0;
}

// ----------------------------------------------------------------------------------- CalMD
static const char *kCalmdNoFit = "openge calmd: the input does not fit in HBM (the records, their rewritten copy and the reference "
                                 "must be resident together); input larger than HBM is not provided\n";

bool CalMD::fitsDevice(ChainContext &cc, const std::vector<std::string> &inputs, const std::string &reference) {
    uint64_t need = 0, fr = 0, tot = 0;
    struct stat st;
    for (auto &in : inputs)
        if (in != "stdin" && in != "-" && !stat(in.c_str(), &st) && S_ISREG(st.st_mode)) need += 2 * (uint64_t)st.st_size;
    if (!stat(reference.c_str(), &st) && S_ISREG(st.st_mode)) need += (uint64_t)st.st_size;
    if (oge_mem_info(cc.ctx, &fr, &tot) || need <= fr) return true;
    fputs(kCalmdNoFit, stderr);
    return false;
}

int CalMD::runInternal(ChainContext &cc, ReadBatch &b) {
    if (cc.gpus > 1 || !b.slices.empty() || !b.shards.empty() || b.produce) {
        fprintf(stderr, "openge calmd: one GPU with the records resident in HBM is required\n");
        return -1;
    }
    const auto t0 = clk();
    uint64_t fr = 0, tot = 0;
    if (!b.dev_valid && !oge_mem_info(cc.ctx, &fr, &tot) && b.bytes() + b.n * 8 > fr) {
        fputs(kCalmdNoFit, stderr);
        return -1;
    }
    if (cc.to_device(b)) return -1;
    std::string names;
    for (auto &s : b.ref_names) names.append(s.c_str(), s.size() + 1);
    oge_calmd_opts o;
    oge_calmd_opts_init(&o);
    o.threads = cc.threads;
    const uint8_t *d_out = nullptr;
    const uint64_t *d_off = nullptr;
    if (oge_calmd_dev(cc.ctx, b.d_recs, b.d_offs, b.n, (int32_t)b.ref_names.size(), names.data(), names.size(), reference_.c_str(), &o, &result,
                      &d_out, &d_off))
        return cc.fail("CalMD");
    double ms = 0;
    oge_ctx_timing(cc.ctx, "calmd", &ms);
    // the call's output belongs to the context: the batch takes a copy of its own in place of its records
    cc.free_device(b);
    DevBuf r(cc.ctx), of(cc.ctx);
    if (r.alloc(result.bytes_out + 64) || of.alloc((b.n + 1) * 8)) {
        fputs(kCalmdNoFit, stderr);
        return -1;
    }
    if ((result.bytes_out && oge_memcpy(cc.ctx, r.as<void>(), d_out, result.bytes_out + 16, 3)) ||
        oge_memcpy(cc.ctx, of.as<void>(), d_off, (b.n + 1) * 8, 3))
        return cc.fail("CalMD");
    b.d_recs = (uint8_t *)r.release();
    b.d_offs = (uint64_t *)of.release();
    b.d_bytes = result.bytes_out;
    b.dev_valid = true;
    b.host_valid = false;
    if (verbose_)
        fprintf(stderr, "[openge] CalMD: %llu records, %llu skipped, %llu without reference, NM changed in %llu, MD changed in %llu, %llu bytes "
                        "out; device %.3f s, total %.3f s\n",
                (unsigned long long)result.records, (unsigned long long)result.skipped, (unsigned long long)result.no_reference,
                (unsigned long long)result.nm_changed, (unsigned long long)result.md_changed, (unsigned long long)result.bytes_out, ms / 1e3,
                sec(t0, clk()));
    return 0;
}

// ----------------------------------------------------------------------------------- FileWriter
FileFormat detect_file_format(std::string name) {
    std::transform(name.begin(), name.end(), name.begin(), ::tolower);
    auto ends = [&](const char *suffix) {
        const size_t k = strlen(suffix);
        return name.size() >= k && name.compare(name.size() - k, k, suffix) == 0;
    };
    if (ends("rawbam") || ends("bamraw")) return FORMAT_RAWBAM;
    if (ends("bam")) return FORMAT_BAM;
    if (ends("sam")) return FORMAT_SAM;
    if (ends("cram")) return FORMAT_CRAM;
    if (ends("fastq")) return FORMAT_FASTQ;
    return FORMAT_UNKNOWN;
}

int FileWriter::setFormat(const std::string &f) {
    const FileFormat fmt = detect_file_format(f);
    if (fmt == FORMAT_UNKNOWN) {  // file_writer.cpp:49-52
        fprintf(stderr, "Unknown file format specified: %s. Aborting.\n", f.c_str());
        return -1;
    }
    if (fmt == FORMAT_RAWBAM || fmt == FORMAT_CRAM) {
        fprintf(stderr, "openge: output format %s is not provided (bam, sam or fastq)\n", f.c_str());
        return -1;
    }
    format_ = fmt;
    return 0;
}

FileFormat FileWriter::getFileFormat() const {
    if (format_ != FORMAT_UNKNOWN) return format_;
    if (!detect_from_name_) return FORMAT_BAM;
    const FileFormat fmt = detect_file_format(filename_);
    return fmt == FORMAT_UNKNOWN ? default_format_ : fmt;
}

// offs[0] and offs[n] of records that sit back to back: the byte range of their stream (0, 0 when n = 0)
static int stream_ends(oge_ctx *ctx, const uint64_t *offs, uint64_t n, uint64_t ends[2]) {
    ends[0] = ends[1] = 0;
    return n && (oge_memcpy(ctx, &ends[0], offs, 8, 2) || oge_memcpy(ctx, &ends[1], offs + n, 8, 2));
}

// -r / -R: the records without OGE_F_DUP compacted into kept / kept_off (`bytes` of records at most), and
// recs / offs / n repointed at them.  Returns what failed, for ChainContext::fail, or nullptr.
template <class R, class O>
static const char *drop_dups(oge_ctx *ctx, R **recs, O **offs, uint64_t *n, uint64_t bytes, DevBuf &kept, DevBuf &kept_off) {
    uint64_t m = 0;
    if (kept.need(bytes + 64) || kept_off.need((*n + 1) * 8)) return "device allocation";
    if (oge_drop_flagged_dev(ctx, *recs, *offs, *n, OGE_F_DUP, kept.as<uint8_t>(), kept_off.as<uint64_t>(), &m)) return "FileWriter: drop duplicates";
    *recs = kept.as<uint8_t>();
    *offs = kept_off.as<uint64_t>();
    *n = m;
    return nullptr;
}

// Device-resident records -> SAM or FASTQ text.  Everything that can fail on the records (an unknown tag
// type, a host line that does not format) fails before the output is opened.
int FileWriter::write_text(ChainContext &cc, ReadBatch &b, FileFormat fmt) {
    const bool to_stdout = filename_ == "stdout" || filename_ == "-";
    const char *why = !b.slices.empty() ? "--gpus"
                      : b.produce       ? "output larger than device memory (chunked sort)"
                      : index_          ? "--index"
                      : fmt == FORMAT_FASTQ && !to_stdout ? "FASTQ files (only -o stdout: the _1.fastq / _2.fastq / .fastq split is not provided)"
                                        : nullptr;
    if (why) {
        fprintf(stderr, "openge: %s output is not provided with %s\n", fmt == FORMAT_SAM ? "SAM" : "FASTQ", why);
        return -1;
    }
    const auto t0 = clk();
    if (b.n && cc.to_device(b)) return -1;  // a batch that is only host-valid goes up first
    uint8_t *recs = b.d_recs;
    uint64_t *offs = b.d_offs;
    uint64_t n = b.n;
    DevBuf kept(cc.ctx), kept_off(cc.ctx), d_toff(cc.ctx), d_mark(cc.ctx), d_out(cc.ctx);
    PinBuf hz[2] = {PinBuf(cc.ctx), PinBuf(cc.ctx)};
    if (b.drop_duplicates && n)
        if (const char *what = drop_dups(cc.ctx, &recs, &offs, &n, b.d_bytes, kept, kept_off)) return cc.fail(what);
    std::string names;
    std::vector<uint32_t> name_off{0};
    for (auto &sq : b.header.sq) {
        names += sq.name;
        name_off.push_back((uint32_t)names.size());
    }
    oge_text_opts o;
    o.mode = fmt == FORMAT_SAM ? OGE_TEXT_SAM : OGE_TEXT_FASTQ;
    o.trim_begin = fmt == FORMAT_FASTQ ? trim_begin_ : 0;
    o.trim_end = fmt == FORMAT_FASTQ ? trim_end_ : 0;
    o.n_ref = (int32_t)b.header.sq.size();
    o.ref_names = names.data();
    o.ref_name_off = name_off.data();
    uint64_t total = 0, n_host = 0;
    if (d_toff.alloc((n + 1) * 8) || d_mark.alloc(n + 1)) return cc.fail("device allocation");
    if (oge_text_size_dev(cc.ctx, recs, offs, n, &o, d_toff.as<uint64_t>(), d_mark.as<uint8_t>(), &total, &n_host)) return cc.fail("FileWriter");
    std::vector<uint64_t> toff(n + 1);
    if (oge_memcpy(cc.ctx, toff.data(), d_toff.as<void>(), (n + 1) * 8, 2)) return cc.fail("device->host copy");
    // the lines the device leaves out, formatted here from the records' bytes
    std::vector<uint64_t> host_rec;
    std::vector<std::string> host_line;
    if (n_host) {
        std::vector<uint8_t> mark(n);
        if (oge_memcpy(cc.ctx, mark.data(), d_mark.as<void>(), n, 2)) return cc.fail("device->host copy");
        std::vector<uint8_t> rb;
        std::vector<char> line;
        for (uint64_t i = 0; i < n; ++i) {
            if (!mark[i]) continue;
            uint64_t at = 0, len = 0;
            uint32_t bs = 0;
            if (oge_memcpy(cc.ctx, &at, offs + i, 8, 2) || oge_memcpy(cc.ctx, &bs, recs + at, 4, 2)) return cc.fail("device->host copy");
            rb.resize((size_t)bs + 4);
            if (oge_memcpy(cc.ctx, rb.data(), recs + at, rb.size(), 2)) return cc.fail("device->host copy");
            line.resize(16 * rb.size() + 1024);
            if (oge_text_host_line(rb.data(), rb.size(), &o, line.data(), line.size(), &len)) {
                fprintf(stderr, "openge: FileWriter: record %llu: %s\n", (unsigned long long)i, oge_last_error(nullptr));
                return -1;
            }
            host_rec.push_back(i);
            host_line.emplace_back(line.data(), (size_t)len);
        }
    }
    // chunks of records whose text fits the chunk size (one record at least)
    const char *ce = getenv("OGE_TEXT_CHUNK");
    const uint64_t chunk = ce ? std::max<uint64_t>(1, strtoull(ce, nullptr, 10)) : (64ull << 20);
    std::vector<uint64_t> cut{0};
    uint64_t cap = 0;
    while (cut.back() < n) {
        const uint64_t s = cut.back();
        uint64_t e = (uint64_t)(std::upper_bound(toff.begin() + s + 1, toff.end(), toff[s] + chunk) - toff.begin()) - 1;
        if (e == s) e = s + 1;
        cap = std::max(cap, toff[e] - toff[s]);
        cut.push_back(e);
    }
    const size_t nchunks = cut.size() - 1;
    if (cap && (d_out.alloc(cap + 16) || hz[0].alloc(cap) || (nchunks > 1 && hz[1].alloc(cap)))) return cc.fail("FileWriter: buffers");
    OutFile file(to_stdout ? stdout : fopen(filename_.c_str(), "wb"));
    FILE *f = file.f;
    if (!f) {
        fprintf(stderr, "Error opening %s file to write.\n", fmt == FORMAT_SAM ? "SAM" : "FASTQ");
        return -1;
    }
    std::atomic<bool> failed(false);
    auto put = [&failed, f](const void *p, size_t k) {
        if (k && fwrite(p, 1, k, f) != k) failed = true;
    };
    if (fmt == FORMAT_SAM) {  // sam_writer.cpp:75-76: the regenerated header, with the @PG line unless --nopg
        BamHeaderModel h = b.header;
        if (!program_line_.empty()) add_program_record(h, program_line_);
        const std::string text = h.to_string();
        put(text.data(), text.size());
    }
    double t_dev = 0, t_d2h = 0, t_wait = 0;
    size_t hk = 0;  // the next host line
    int k = 0;
    JoinThread wr;  // the last owner declared: joined before the file is closed and the buffers are freed
    for (size_t c = 0; c < nchunks && !failed; ++c, k ^= 1) {
        const uint64_t s = cut[c], e = cut[c + 1], bytes = toff[e] - toff[s];
        auto t = clk();
        if (oge_text_emit_dev(cc.ctx, recs, offs, d_toff.as<uint64_t>(), s, e - s, &o, d_out.as<uint8_t>(), cap) || oge_ctx_sync(cc.ctx))
            return cc.fail("FileWriter: text on the device");
        t_dev += sec(t, clk());
        t = clk();
        wr.join();  // the buffer written two chunks ago is free again
        t_wait += sec(t, clk());
        t = clk();
        if (bytes && oge_memcpy(cc.ctx, hz[k].as<void>(), d_out.as<void>(), bytes, 2)) return cc.fail("device->host copy");
        t_d2h += sec(t, clk());
        const size_t h0 = hk;
        while (hk < host_rec.size() && host_rec[hk] < e) ++hk;
        const size_t h1 = hk;
        const uint8_t *hp = hz[k].as<uint8_t>();
        wr = std::thread([&, hp, s, bytes, h0, h1]() {
            uint64_t done = 0;
            for (size_t j = h0; j < h1; ++j) {
                const uint64_t at = toff[host_rec[j]] - toff[s];
                put(hp + done, at - done);
                done = at;
                put(host_line[j].data(), host_line[j].size());
            }
            put(hp + done, bytes - done);
        });
    }
    auto t = clk();
    wr.join();
    t_wait += sec(t, clk());
    for (DevBuf *p : {&kept, &kept_off, &d_toff, &d_mark, &d_out}) p->reset();  // freed here only so that the total below times it
    hz[0].reset(), hz[1].reset();
    if (file.close() != 0) failed = true;
    if (failed) {
        fprintf(stderr, "openge: error writing %s: %s\n", filename_.c_str(), strerror(errno));
        return -1;
    }
    if (verbose_)
        fprintf(stderr, "[openge] FileWriter: %s text %llu bytes in %zu chunks, %llu lines formatted on the host; size + emit %.3f s (gpu), "
                "device->host %.3f s, waiting on the output %.3f s, total %.3f s\n", fmt == FORMAT_SAM ? "SAM" : "FASTQ",
                (unsigned long long)total, nchunks, (unsigned long long)n_host, t_dev, t_d2h, t_wait, sec(t0, clk()));
    return 0;
}

// the bin every record must carry (bam_serializer.h:112-116), recomputed in place by the workers
static void fix_bins(ReadBatch &b, int threads) {
    const uint64_t n = b.n, chunk = 1 << 16;
    const uint64_t nc = (n + chunk - 1) / chunk;
    std::atomic<uint64_t> next(0);
    std::vector<std::thread> ts;
    for (int t = 0; t < std::max(1, threads); ++t)
        ts.emplace_back([&]() {
            for (uint64_t c; (c = next.fetch_add(1)) < nc;)
                for (uint64_t k = c * chunk, e = std::min(n, k + chunk); k < e; ++k) {
                    uint8_t *r = b.recs.data() + b.offs[k];
                    oge_wr_u16(r + OGE_OFF_BIN, oge_rec_bin(r));
                }
        });
    for (auto &t : ts) t.join();
}

// Device-resident records: drop duplicates (-r/-R), recompute bins and BGZF-compress on the GPU;
// only the compressed stream crosses PCIe.  The records of a batch are back to back in its arena
// (the reader's stream, a gather's output), so the stream is the byte range [off[0], off[n]).
// Device-resident records -> BGZF file.  Bins are recomputed on the device, then the stream is
// deflated in segments of kSeg bytes (a multiple of the 65,280-byte block payload, so the blocks are
// exactly those of one whole-stream deflate); each segment's compressed bytes come down into one of
// two page-locked buffers and are written by a background thread while the next segment is
// deflated and copied.  Timings: device deflate, device->host, and time spent waiting for the disk.
int FileWriter::write_device(ChainContext &cc, ReadBatch &b, BgzfWriter &w, double *t_dev, double *t_d2h, double *t_wait) {
    *t_dev = *t_d2h = *t_wait = 0;
    if (const char *f = getenv("OGE_TEST_FAIL"); f && !strcmp(f, "write_device")) {  // test hook: a failed device write
        fprintf(stderr, "openge: FileWriter: injected failure (OGE_TEST_FAIL=write_device)\n");
        return -1;
    }
    uint8_t *recs = b.d_recs;
    uint64_t *offs = b.d_offs;
    uint64_t n = b.n;
    DevBuf kept(cc.ctx), kept_off(cc.ctx), dz(cc.ctx);
    PinBuf hz[2] = {PinBuf(cc.ctx), PinBuf(cc.ctx)};
    JoinThread wr;  // the last owner declared: joined before the buffers it writes from are freed
    auto t = clk();
    if (b.drop_duplicates && n)
        if (const char *what = drop_dups(cc.ctx, &recs, &offs, &n, b.d_bytes, kept, kept_off)) return cc.fail(what);
    uint64_t ends[2];
    if ((n && oge_fix_bins_dev(cc.ctx, recs, offs, n)) || stream_ends(cc.ctx, offs, n, ends)) return cc.fail("FileWriter: bins");
    *t_dev += sec(t, clk());
    const uint64_t len = ends[1] - ends[0];
    // segments of 1024-32768 payloads (67 MB - 2.14 GB of records), about an eighth of the stream: the
    // page-locked download buffers are sized by the segment and pinning / unpinning them costs ~0.25 s per
    // GB (a 1.1 GB realign output: 0.5 s in 2.1 GB segments, 0.04 s in 67 MB ones), while a large file keeps
    // full-size deflate calls.  OGE_WRITE_SEG_BLOCKS fixes the payloads per segment (tests).
    const char *se = getenv("OGE_WRITE_SEG_BLOCKS");
    const uint64_t want = se ? std::max(1ul, strtoul(se, nullptr, 10)) : std::min<uint64_t>(32768, std::max<uint64_t>(1024, len / 8 / 65280 + 1));
    const uint64_t kSeg = 65280ull * want;
    const uint64_t seg = std::min(len, kSeg);
    const uint64_t cap = oge_bgzf_bound(seg);
    t = clk();
    if (len && (dz.alloc(cap) || hz[0].alloc(cap) || (len > seg && hz[1].alloc(cap)))) return cc.fail("FileWriter: buffers");
    if (getenv("OGE_WRITE_TRACE")) fprintf(stderr, "[openge] FileWriter: buffers %.3f s\n", sec(t, clk()));
    w.write_compressed(nullptr, 0);  // flush the header as blocks of its own
    // --index: the block table of the file, from the BSIZE fields of the bytes that go to it (the header's
    // blocks hold no record: the table starts behind them)
    std::vector<uint64_t> ix_uoff, ix_cstart;
    uint64_t ix_u = index_hdr_u_, ix_z = index_hdr_z_;
    int k = 0;
    for (uint64_t s0 = 0; s0 < len; s0 += seg, k ^= 1) {
        const uint64_t sl = std::min(seg, len - s0);
        uint64_t zb = 0;
        t = clk();
        if (oge_bgzf_deflate_dev(cc.ctx, recs + ends[0] + s0, sl, std::max(0, std::min(9, level_)), dz.as<uint8_t>(), cap, &zb) ||
            oge_ctx_sync(cc.ctx))
            return cc.fail("FileWriter: BGZF on the device");
        *t_dev += sec(t, clk());
        t = clk();
        wr.join();  // the buffer written two segments ago is free again
        *t_wait += sec(t, clk());
        t = clk();
        if (zb && oge_memcpy(cc.ctx, hz[k].as<void>(), dz.as<void>(), zb, 2)) return cc.fail("device->host copy");
        *t_d2h += sec(t, clk());
        const uint8_t *hp = hz[k].as<uint8_t>();
        if (index_) {
            uint64_t nb = 0;
            const int rc = oge_bgzf_index(hp, zb, nullptr, nullptr, nullptr, nullptr, 0, &nb);
            std::vector<uint64_t> d0(nb + 1), uo(nb + 1);
            if ((rc != OGE_OK && rc != OGE_ERR_ARG) || oge_bgzf_index(hp, zb, d0.data(), nullptr, uo.data(), nullptr, nb, &nb))
                return cc.fail("FileWriter: index of the written blocks");
            for (uint64_t i = 0; i < nb; ++i) {  // the device writer's blocks have 18-byte headers
                ix_cstart.push_back(ix_z + d0[i] - 18);
                ix_uoff.push_back(ix_u + uo[i]);
            }
            ix_u += uo[nb];
            ix_z += zb;
        }
        wr = std::thread([&w, hp, zb]() { w.write_compressed(hp, zb); });
    }
    t = clk();
    wr.join();
    *t_wait += sec(t, clk());
    if (index_) {  // from the kept records
        ix_uoff.push_back(ix_u);
        ix_cstart.push_back(ix_z);
        const uint64_t nblk = ix_uoff.size() - 1;
        DevBuf tab(cc.ctx);
        const uint8_t *d_bai = nullptr;
        uint64_t bb = 0;
        int rc = tab.alloc(2 * (nblk + 1) * 8);
        uint64_t *dt = tab.as<uint64_t>();
        if (!rc) rc = oge_memcpy(cc.ctx, dt, ix_uoff.data(), (nblk + 1) * 8, 1);
        if (!rc) rc = oge_memcpy(cc.ctx, dt + nblk + 1, ix_cstart.data(), (nblk + 1) * 8, 1);
        if (!rc) rc = oge_bai_build_dev(cc.ctx, recs, offs, n, (int32_t)b.header.sq.size(), index_hdr_u_, dt, dt + nblk + 1, nblk, &d_bai, &bb);
        if (!rc) {
            bai_.resize(bb);
            rc = oge_memcpy(cc.ctx, bai_.data(), d_bai, bb, 2);
        }
        if (rc) return cc.fail("FileWriter: index");
    }
    t = clk();
    kept.reset(), kept_off.reset(), dz.reset(), hz[0].reset(), hz[1].reset();  // freed here only so that the trace times it
    if (getenv("OGE_WRITE_TRACE")) fprintf(stderr, "[openge] FileWriter: release %.3f s\n", sec(t, clk()));
    return 0;
}

// --gpus G: every rank drops its duplicates (-r / -R) and BGZF-compresses its own slice on its own
// GPU, concurrently; the compressed slices go to the file in rank order (a slice's last block may be
// short, the decompressed stream is the one-GPU stream).
int FileWriter::write_slices(ChainContext &cc, ReadBatch &b, BgzfWriter &w) {
    const int G = (int)b.slices.size();
    struct Out {
        PinBuf host;
        uint64_t zb = 0;
        int rc = 0;
        std::string why;
    };
    std::vector<Out> outs;
    for (auto &s : b.slices) outs.push_back(Out{PinBuf(s.ctx)});
    const int level = std::max(0, std::min(9, level_));
    const bool drop = b.drop_duplicates;
    std::vector<std::thread> ts;
    for (int g = 0; g < G; ++g)
        ts.emplace_back([&, g]() {
            const ReadBatch::Slice &s = b.slices[g];
            Out &o = outs[g];
            oge_ctx *c = s.ctx;
            uint8_t *recs = s.d_recs;
            uint64_t *offs = s.d_offs, n = s.n;
            DevBuf kept(c), kept_off(c), dz(c);
            uint64_t ends[2] = {0, 0};
            int rc = 0;
            if (drop && n)  // kept is sized by the slice's own stream end
                rc = stream_ends(c, offs, n, ends) || drop_dups(c, &recs, &offs, &n, ends[1], kept, kept_off) != nullptr;
            if (!rc) rc = stream_ends(c, offs, n, ends);
            const uint64_t len = ends[1] - ends[0], cap = oge_bgzf_bound(len);
            if (!rc && len) rc = dz.alloc(cap);
            if (!rc && len) rc = oge_bgzf_deflate_dev(c, recs + ends[0], len, level, dz.as<uint8_t>(), cap, &o.zb);
            if (!rc && o.zb) rc = o.host.alloc(o.zb);
            if (!rc && o.zb) rc = oge_memcpy(c, o.host.as<void>(), dz.as<void>(), o.zb, 2);
            if (rc) o.why = oge_last_error(c);
            o.rc = rc;
        });
    w.write_compressed(nullptr, 0);  // the header's blocks first
    int ret = 0;
    for (int g = 0; g < G; ++g) {
        ts[g].join();
        if (outs[g].rc) {
            fprintf(stderr, "openge: FileWriter: rank %d: %s\n", g, outs[g].why.c_str());
            ret = -1;
        } else if (!ret && outs[g].zb) {
            w.write_compressed(outs[g].host.as<uint8_t>(), outs[g].zb);
        }
        outs[g].host.reset();
    }
    return ret;
}

// Inputs larger than HBM: every output range the sorter produces is (with -r / -R) compacted, BGZF
// compressed on the device and written before the next range is made.
int FileWriter::write_ranges(ChainContext &cc, ReadBatch &b, BgzfWriter &w) {
    w.write_compressed(nullptr, 0);  // the header's blocks first
    const int level = std::max(0, std::min(9, level_));
    const bool drop = b.drop_duplicates;
    DevBuf kept(cc.ctx), kept_off(cc.ctx), dz(cc.ctx);  // grown to the largest range, kept between ranges
    PinBuf hz(cc.ctx);
    auto sink = [&](const uint8_t *recs, const uint64_t *offs, uint64_t n) -> int {
        uint64_t ends[2];
        if (stream_ends(cc.ctx, offs, n, ends)) return -1;
        if (drop && n && (drop_dups(cc.ctx, &recs, &offs, &n, ends[1], kept, kept_off) || stream_ends(cc.ctx, offs, n, ends))) return -1;
        const uint64_t len = ends[1] - ends[0];
        if (!len) return 0;
        const uint64_t cap = oge_bgzf_bound(len);
        uint64_t zb = 0;
        if (dz.need(cap) || oge_bgzf_deflate_dev(cc.ctx, recs + ends[0], len, level, dz.as<uint8_t>(), cap, &zb) || hz.need(zb) ||
            oge_memcpy(cc.ctx, hz.as<void>(), dz.as<void>(), zb, 2))
            return -1;
        w.write_compressed(hz.as<uint8_t>(), zb);
        return 0;
    };
    if (b.produce(cc, sink)) return -1;
    return 0;
}

int FileWriter::runInternal(ChainContext &cc, ReadBatch &b) {
    const FileFormat fmt = getFileFormat();
    if (fmt == FORMAT_SAM || fmt == FORMAT_FASTQ) return write_text(cc, b, fmt);
    if (fmt != FORMAT_BAM) {  // file_writer.cpp:192-195
        fprintf(stderr, "Unsupported output file format selected. Aborting.\n");
        return -1;
    }
    const auto t0 = clk();
    const bool sliced = !b.slices.empty(), produced = (bool)b.produce;
    bool on_device = sliced || produced || (b.dev_valid && !b.host_valid && !bgzf_host_codec_forced());
    double t_dev = 0, t_d2h = 0, t_wait = 0;
    // OGE_WRITE_DEVICE=1: host records (the realigner's output) whose bytes sit back to back go up to the
    // device and out through the GPU deflate -- on the C5 set 1.1 GB of records take 0.78 s with 16
    // libdeflate threads (profiles/r05ap_realign_cli.txt), the upload and the device path a fraction of that,
    // for an 11 % larger file (the GPU deflate's greedy search).  Off by default: the host codec writes
    // zlib-class level 6 like the reference.  A device that cannot hold them leaves the host writer in charge.
    if (!on_device && b.host_valid && !b.dev_valid && b.n && write_device_forced() && !bgzf_host_codec_forced()) {
        bool contiguous = b.offs.size() == b.n + 1 && b.offs[b.n] + 16 <= b.recs.size();
        for (uint64_t k = 0; contiguous && k < b.n; ++k)
            contiguous = b.offs[k + 1] == b.offs[k] + 4 + oge_rd_u32(b.recs.data() + b.offs[k]);
        uint64_t fr = 0, tot = 0;
        const uint64_t bytes = contiguous ? b.offs[b.n] : 0;
        if (contiguous && !oge_mem_info(cc.ctx, &fr, &tot) && bytes + oge_bgzf_bound(std::min<uint64_t>(bytes, 65280ull * 32768)) +
                                                                      (b.n + 1) * 8 + (256ull << 20) < fr) {
            if (cc.to_device(b)) return -1;
            on_device = true;
            b.host_valid = false;  // write_device reads the device copy
        }
    }
    if (index_) {  // refused before anything is written
        const char *why = filename_ == "stdout" || filename_ == "-" ? "output to stdout"
                          : sliced                                   ? "--gpus"
                          : produced                                 ? "output larger than device memory (chunked sort)"
                          : !on_device                               ? "the host writer"
                          : b.header.sort_order == BamHeaderModel::QUERYNAME ? "output sorted by name"
                                                                     : nullptr;
        if (why) {
            fprintf(stderr, "openge: --index is not provided with %s\n", why);
            return -1;
        }
    }
    if (!on_device && cc.to_host(b)) return -1;
    const auto t1 = clk();
    if (!on_device) fix_bins(b, cc.threads);
    const auto t2 = clk();
    BamHeaderModel h = b.header;
    if (!program_line_.empty()) add_program_record(h, program_line_);  // file_writer.cpp:76-89
    OutFile file(filename_ == "stdout" || filename_ == "-" ? stdout : fopen(filename_.c_str(), "wb"));
    FILE *f = file.f;
    if (!f) {
        fprintf(stderr, "Error opening BAM file to write.\n");
        return -1;
    }
    bool write_ok = true;
    {
        BgzfWriter w(f, level_, cc.threads > 0 ? cc.threads : 8);
        std::vector<uint8_t> hb = bam_encode_header(h);
        w.write(hb.data(), hb.size());
        if (index_) {  // the header's blocks are flushed now (write_device would do it next): their size in the file
            w.write_compressed(nullptr, 0);
            fflush(f);
            index_hdr_z_ = (uint64_t)ftello(f);
            index_hdr_u_ = hb.size();
        }
        if (on_device) {
            if (produced ? write_ranges(cc, b, w) : sliced ? write_slices(cc, b, w) : write_device(cc, b, w, &t_dev, &t_d2h, &t_wait)) {
                w.abandon();  // no EOF block and no write into the FILE closed at the return
                return -1;
            }
            w.close();
        }
        // maximal runs of records that sit back to back in memory go out as spans (no copy)
        uint64_t k = 0;
        while (!on_device && k < b.n) {
            const uint8_t *r = b.recs.data() + b.offs[k];
            if (b.drop_duplicates && (oge_rd_u16(r + OGE_OFF_FLAG) & OGE_F_DUP)) {
                ++k;
                continue;
            }
            const uint64_t s = b.offs[k];
            uint64_t e = s + 4 + oge_rd_u32(r);
            ++k;
            while (k < b.n && b.offs[k] == e) {
                const uint8_t *q = b.recs.data() + e;
                if (b.drop_duplicates && (oge_rd_u16(q + OGE_OFF_FLAG) & OGE_F_DUP)) break;
                e += 4 + oge_rd_u32(q);
                ++k;
            }
            w.write_span(b.recs.data() + s, e - s);
        }
        w.close();
        write_ok = w.ok();
    }
    if (file.close() != 0) write_ok = false;
    if (!write_ok) {  // a full disk or a closed pipe must not look like success
        fprintf(stderr, "openge: error writing %s: %s\n", filename_.c_str(), strerror(errno));
        return -1;
    }
    // only beside a BAM that was written whole
    if (index_ && write_whole_file(filename_ + ".bai", bai_.data(), bai_.size())) return -1;
    if (verbose_ && on_device)
        fprintf(stderr, "[openge] FileWriter: device bins + BGZF %.3f s (gpu, segmented), device->host %.3f s, waiting on the disk %.3f s, "
                "total %.3f s\n", t_dev, t_d2h, t_wait, sec(t2, clk()));
    else if (verbose_)
        fprintf(stderr, "[openge] FileWriter: device->host %.3f s, bins %.3f s, BGZF %.3f s (%s)\n", sec(t0, t1), sec(t1, t2),
                sec(t2, clk()), bgzf_codec_name());
    else fflush(stdout);
    return 0;
}

// index / stats / count / coverage: the whole file in HBM (64 bytes of slack); `what` names a failed upload,
// timed: the -v line of the qc commands
static int load_whole(ChainContext &cc, const std::string &path, const char *what, bool timed, LoadedFile &z) {
    const int rc = file_to_device(cc, path, LOAD_WHOLE, z);
    if (rc == -2) return cc.fail(what);
    if (!rc && timed && cc.verbose) fprintf(stderr, "[openge] read %.3f s, upload %.3f s\n", z.t_read, z.t_upload);
    return rc;
}

int index_bam_file(ChainContext &cc, const std::string &path, const std::string &out) {
    if (file_is_sam(path)) {
        fprintf(stderr, "openge index: %s is SAM text; only a coordinate-sorted BAM file can be indexed (openge sort %s -o sorted.bam --index)\n",
                path.c_str(), path.c_str());
        return -1;
    }
    LoadedFile z(cc.ctx);
    if (load_whole(cc, path, "index", false, z)) return -1;
    const uint8_t *d_bai = nullptr;
    uint64_t bb = 0;
    std::vector<uint8_t> img;
    int rc = oge_bam_index_dev(cc.ctx, z.buf.as<uint8_t>(), z.zbytes, &d_bai, &bb);
    if (!rc) {
        img.resize(bb);
        rc = oge_memcpy(cc.ctx, img.data(), d_bai, bb, 2);
    }
    z.buf.reset();
    if (rc) return cc.fail("index");
    return write_whole_file(out, img.data(), img.size());
}

// ---- stats / count / coverage ------------------------------------------------------------------------
namespace {

void report_stages(ChainContext &cc, const char *reduce, double t_format) {
    if (!cc.verbose) return;
    double ix = 0, inf = 0, walk = 0, red = 0;
    oge_ctx_timing(cc.ctx, "bgzf_index", &ix);
    oge_ctx_timing(cc.ctx, "bgzf_inflate", &inf);
    oge_ctx_timing(cc.ctx, "rec_walk", &walk);
    oge_ctx_timing(cc.ctx, reduce, &red);
    fprintf(stderr, "[openge] device: framing %.1f ms, inflate %.1f ms, record walk %.1f ms, %s %.1f ms; format %.3f s\n", ix, inf, walk,
            reduce, red, t_format);
}

// The one loader of stats / count / coverage: the input in HBM for either format, and the three reductions over
// it.  A BAM file stays as its compressed bytes and takes the whole-file calls it always took (oge_bam_*_dev:
// inflate, record walk and reduction under one hold, with their stage times for -v); a SAM file becomes records
// in HBM (read_sam_device) and takes oge_stats_dev / oge_coverage_dev, with the contigs of its header text in the
// place of the BAM file's binary reference list.  Everything is freed on every return.
struct QcInput {
    ChainContext &cc;
    LoadedFile z;
    ReadBatch b;
    bool sam = false;
    std::vector<int32_t> sam_lens;
    std::string sam_names;
    explicit QcInput(ChainContext &c) : cc(c), z(c.ctx) {}
    ~QcInput() { cc.free_device(b); }
    int load(const std::string &path) {
        sam = file_is_sam(path);
        return sam ? read_sam_device(cc, path, false, b, &sam_lens) : load_whole(cc, path, "upload", true, z);
    }
    int stats(uint32_t want, oge_bam_stats *s, const uint32_t **d_len, const uint64_t **d_cnt) {
        return sam ? oge_stats_dev(cc.ctx, b.d_recs, b.d_offs, b.n, want, s, d_len, d_cnt)
                   : oge_bam_stats_dev(cc.ctx, z.buf.as<uint8_t>(), z.zbytes, want, s, d_len, d_cnt);
    }
    int count(uint64_t *n) {  // a SAM file's lines have all been checked by now: the count is of records
        if (sam) return *n = b.n, 0;
        return oge_bam_count_dev(cc.ctx, z.buf.as<uint8_t>(), z.zbytes, n);
    }
    int targets(const oge_targets_opts *o, oge_targets_result *res, const oge_target **d_targets, const uint8_t **d_text) {
        if (!sam) return oge_bam_targets_dev(cc.ctx, z.buf.as<uint8_t>(), z.zbytes, o, res, d_targets, d_text);
        for (auto &nm : b.ref_names) sam_names.append(nm.c_str(), nm.size() + 1);
        return oge_targets_dev(cc.ctx, b.d_recs, b.d_offs, b.n, (int32_t)sam_lens.size(), sam_lens.data(), sam_names.data(), sam_names.size(), o,
                               res, d_targets, d_text);
    }
    // the counters by library id, the ids' names ("" = no @RG names it) and unknown_lib, as LibTable gives them
    int dup_metrics(std::vector<OgeDupMetrics> &m, std::vector<std::string> &names, int *unknown) {
        if (sam) {
            const LibTable lt(b.header);
            const oge_markdup_opts mo = markdup_opts(lt, b, false, 0);
            names = lt.names;
            *unknown = lt.unknown_lib;
            m.assign((size_t)lt.n_lib, OgeDupMetrics{});
            return oge_dup_metrics_dev(cc.ctx, b.d_recs, b.d_offs, b.n, &mo, lt.n_lib, m.data());
        }
        const OgeDupMetrics *out = nullptr;
        const char *nm = nullptr;
        int32_t n_lib = 0, unk = 0;
        uint64_t names_bytes = 0;
        const int rc = oge_bam_dup_metrics_dev(cc.ctx, z.buf.as<uint8_t>(), z.zbytes, &out, &n_lib, &nm, &names_bytes, &unk);
        if (rc) return rc;
        m.assign(out, out + n_lib);
        names.clear();
        for (int32_t k = 0; k < n_lib; ++k) {
            names.emplace_back(nm);
            nm += names.back().size() + 1;
        }
        *unknown = unk;
        return 0;
    }
    // --optical-distance: the duplicate sets by library id, the ids of dup_metrics (one header, one LibTable)
    int dup_sets(int64_t distance, std::vector<OgeDupSetsLib> &s, std::vector<uint64_t> &hist) {
        if (sam) {
            const LibTable lt(b.header);
            const oge_markdup_opts mo = markdup_opts(lt, b, false, 0);
            s.assign((size_t)lt.n_lib, OgeDupSetsLib{});
            hist.assign(3 * OGE_DUP_SETS_BINS, 0);
            return oge_dup_sets_dev(cc.ctx, b.d_recs, b.d_offs, b.n, &mo, distance, lt.n_lib, s.data(), hist.data());
        }
        const OgeDupSetsLib *out = nullptr;
        const uint64_t *h = nullptr;
        int32_t got = 0;
        const int rc = oge_bam_dup_sets_dev(cc.ctx, z.buf.as<uint8_t>(), z.zbytes, distance, &out, &h, &got);
        if (rc) return rc;
        s.assign(out, out + got);
        hist.assign(h, h + 3 * OGE_DUP_SETS_BINS);
        return 0;
    }
    int coverage(int32_t binsize, const uint32_t **d_bins, uint64_t *nb, uint64_t *skipped, int32_t *overflow, int32_t *n_ref, const char **names,
                 const int32_t **lens) {
        if (!sam) {
            uint64_t names_bytes = 0;
            int rc = oge_bam_coverage_dev(cc.ctx, z.buf.as<uint8_t>(), z.zbytes, binsize, d_bins, nb, skipped, overflow);
            z.buf.reset();
            if (!rc) rc = oge_ctx_last_refs(cc.ctx, n_ref, names, &names_bytes, lens);
            return rc;
        }
        for (auto &nm : b.ref_names) sam_names.append(nm.c_str(), nm.size() + 1);
        *n_ref = (int32_t)sam_lens.size();
        *names = sam_names.data();
        *lens = sam_lens.data();
        std::vector<uint64_t> base((size_t)*n_ref + 1);
        int rc = oge_coverage_dev(cc.ctx, b.d_recs, b.d_offs, b.n, *n_ref, *lens, binsize, d_bins, skipped, overflow);
        if (!rc) rc = oge_coverage_layout(*n_ref, *lens, binsize, base.data());
        *nb = base[*n_ref];
        return rc;
    }
};

float pct(uint64_t a, uint64_t b) { return ((float)a / (float)b) * 100; }  // statistics.cpp:158: float32

// decimal digits of v and one byte behind them into a buffer that is flushed when nearly full
struct TsvWriter {
    FILE *f;
    std::vector<char> buf;
    size_t used = 0;
    bool ok = true;
    explicit TsvWriter(FILE *file) : f(file), buf(1 << 20) {}
    void flush() {
        if (used && ok) ok = fwrite(buf.data(), 1, used, f) == used;
        used = 0;
    }
    void room(size_t need) {
        if (used + need > buf.size()) flush();
    }
    void text(const char *s, size_t n) {
        if (n > buf.size()) {
            flush();
            if (ok) ok = fwrite(s, 1, n, f) == n;
            return;
        }
        room(n);
        memcpy(buf.data() + used, s, n);
        used += n;
    }
    void number(uint64_t v, char end) {
        room(24);
        char tmp[24];
        int k = 0;
        do tmp[k++] = (char)('0' + v % 10);
        while (v /= 10);
        while (k) buf[used++] = tmp[--k];
        buf[used++] = end;
    }
};

}  // namespace

int stats_bam_file(ChainContext &cc, const std::string &path, bool inserts, bool lengths) {
    QcInput in(cc);
    if (in.load(path)) return -1;
    oge_bam_stats s;
    const uint32_t *d_len = nullptr;
    const uint64_t *d_cnt = nullptr;
    std::vector<uint32_t> len;
    std::vector<uint64_t> cnt;
    const uint32_t want = (inserts ? OGE_STATS_INSERTS : 0) | (lengths ? OGE_STATS_LENGTHS : 0);
    int rc = in.stats(want, &s, &d_len, &d_cnt);
    if (!rc && lengths && s.n_lengths) {
        len.resize(s.n_lengths);
        cnt.resize(s.n_lengths);
        rc = oge_memcpy(cc.ctx, len.data(), d_len, s.n_lengths * 4, 2);
        if (!rc) rc = oge_memcpy(cc.ctx, cnt.data(), d_cnt, s.n_lengths * 8, 2);
    }
    in.z.buf.reset();
    if (rc) return cc.fail("stats");
    const auto t0 = clk();
    auto line = [](const char *label, uint64_t v, uint64_t of) {
        printf("%s%10llu (%5.1f%%)\n", label, (unsigned long long)v, (double)pct(v, of));
    };
    printf("Total reads:       %10llu\n", (unsigned long long)s.reads);
    line("Mapped reads:      ", s.mapped, s.reads);
    line("Forward strand:    ", s.forward, s.reads);
    line("Reverse strand:    ", s.reverse, s.reads);
    line("Failed QC:         ", s.failed_qc, s.reads);
    line("Duplicates:        ", s.duplicates, s.reads);
    line("Paired-end reads:  ", s.paired, s.reads);
    if (s.paired) {
        line("'Proper-pairs':    ", s.proper_pair, s.paired);
        line("Both pairs mapped: ", s.both_mapped, s.paired);
        printf("Read 1:            %10llu\n", (unsigned long long)s.read1);
        printf("Read 2:            %10llu\n", (unsigned long long)s.read2);
        line("Singletons:        ", s.singletons, s.paired);
    }
    printf("Sorted:            %10s\n", s.sorted ? "Yes" : "No");
    if (lengths) {
        fflush(stdout);
        fprintf(stderr, "Read lengths:\n");
        for (size_t k = 0; k < len.size(); ++k) {
            const float p = (float)(100. * (double)cnt[k] / (double)s.reads);  // statistics.cpp:180
            printf(" %5d" "bp:          %10llu (%5.1f%%)\n", (int)len[k], (unsigned long long)cnt[k], (double)p);
        }
    }
    if (inserts) {
        printf("Insert size (absolute value):\n");
        if (s.n_insert) {
            printf("    Mean:          %10.1f\n", (double)s.insert_sum / (double)s.n_insert);
            const double median = s.n_insert % 2 ? (double)s.insert_mid_hi : ((double)s.insert_mid_hi + (double)s.insert_mid_lo) / 2.0;
            printf("    Median:        %10.1f\n", median);
        }
    }
    const bool ok = fflush(stdout) == 0 && !ferror(stdout);
    report_stages(cc, "qc_stats", sec(t0, clk()));
    if (!ok) {
        fprintf(stderr, "openge: error writing to stdout\n");
        return -1;
    }
    return 0;
}

int count_bam_file(ChainContext &cc, const std::string &path) {
    QcInput in(cc);
    uint64_t n = 0;
    if (in.load(path)) return -1;
    if (in.count(&n)) return cc.fail("count");
    printf("%llu\n", (unsigned long long)n);
    if (fflush(stdout) != 0 || ferror(stdout)) {
        fprintf(stderr, "openge: error writing to stdout\n");
        return -1;
    }
    return 0;
}

static void report_targets(const oge_targets_result &r, int max_interval, int gap) {
    fprintf(stderr, "[openge] targets: %llu reads used, %llu events, %llu intervals, %llu dropped (--maxinterval %d), %llu targets (--gap %d), %llu bytes of text\n",
            (unsigned long long)r.reads_used, (unsigned long long)r.events, (unsigned long long)r.intervals, (unsigned long long)r.dropped_long,
            max_interval, (unsigned long long)r.targets, gap, (unsigned long long)r.text_bytes);
}

int targets_bam_file(ChainContext &cc, const std::string &path, const std::string &out, int max_interval, int gap) {
    QcInput in(cc);
    if (in.load(path)) return -1;
    oge_targets_opts o;
    oge_targets_opts_init(&o);
    o.max_interval = max_interval;
    o.gap = gap;
    oge_targets_result res;
    const oge_target *d_targets = nullptr;
    const uint8_t *d_text = nullptr;
    std::vector<uint8_t> text;
    int rc = in.targets(&o, &res, &d_targets, &d_text);
    if (!rc && res.text_bytes) {
        text.resize(res.text_bytes);
        rc = oge_memcpy(cc.ctx, text.data(), d_text, res.text_bytes, 2);
    }
    in.z.buf.reset();
    if (rc) return cc.fail("targets");
    const auto t0 = clk();
    if (write_stdout_or_file(out, text.data(), text.size())) return -1;
    if (cc.verbose) report_targets(res, max_interval, gap);
    report_stages(cc, "targets", sec(t0, clk()));
    return 0;
}

int dupmetrics_bam_file(ChainContext &cc, const std::string &path, const std::string &out, const std::string &command_line,
                        int64_t optical_distance) {
    QcInput in(cc);
    if (in.load(path)) return -1;
    std::vector<OgeDupMetrics> m;
    std::vector<std::string> names;
    int unknown = 0;
    int rc = in.dup_metrics(m, names, &unknown);
    std::vector<OgeDupSetsLib> sets;
    std::vector<uint64_t> hist;
    const bool optical = optical_distance >= 0;
    double metrics_ms = 0;
    if (!rc && optical) {  // the same file once more: the duplicate sets of its records
        oge_ctx_timing(cc.ctx, "dup_metrics", &metrics_ms);
        rc = in.dup_sets(optical_distance, sets, hist);
    }
    in.z.buf.reset();
    if (rc) return cc.fail("dupmetrics");
    const auto t0 = clk();
    std::string text;
    if (metrics_text(names, unknown, m, command_line, text, optical ? &sets : nullptr, optical ? hist.data() : nullptr)) {
        fprintf(stderr, "openge: dupmetrics: %s\n", oge_last_error(nullptr));
        return -1;
    }
    if (write_stdout_or_file(out, text.data(), text.size())) return -1;
    report_stages(cc, optical ? "dup_sets" : "dup_metrics", sec(t0, clk()));
    if (cc.verbose && optical) {
        uint64_t tiers[3] = {0, 0, 0};
        const char *nm[3] = {"dupsets_wave_sets", "dupsets_block_sets", "dupsets_host_sets"};
        for (int k = 0; k < 3; ++k) oge_ctx_counter(cc.ctx, nm[k], &tiers[k]);
        fprintf(stderr, "[openge] dupmetrics: dup_metrics %.1f ms; duplicate sets at optical distance %lld, sets of two or more pairs: "
                        "%llu in a wave, %llu in a workgroup, %llu on the host\n",
                metrics_ms, (long long)optical_distance, (unsigned long long)tiers[0], (unsigned long long)tiers[1], (unsigned long long)tiers[2]);
    }
    return 0;
}

int coverage_bam_file(ChainContext &cc, const std::string &path, const std::string &out, int binsize, bool omit_uncovered) {
    QcInput in(cc);
    uint64_t nb = 0, skipped = 0;
    if (in.load(path)) return -1;
    const uint32_t *d_bins = nullptr;
    int32_t overflow = 0, n_ref = 0;
    const char *names = nullptr;
    const int32_t *lens = nullptr;
    std::vector<uint32_t> bins;
    int rc = in.coverage(binsize, &d_bins, &nb, &skipped, &overflow, &n_ref, &names, &lens);
    if (!rc && nb) {
        bins.resize(nb);
        rc = oge_memcpy(cc.ctx, bins.data(), d_bins, nb * 4, 2);
    }
    if (rc) return cc.fail("coverage");
    const auto t0 = clk();
    std::vector<uint64_t> base((size_t)n_ref + 1);
    oge_coverage_layout(n_ref, lens, binsize, base.data());
    // the reference keeps its contigs in a std::map: bytewise name order, not header order
    std::vector<std::pair<std::string, int32_t>> order;
    const char *p = names;
    for (int32_t r = 0; r < n_ref; ++r) {
        order.emplace_back(p, r);
        p += order.back().first.size() + 1;
    }
    std::sort(order.begin(), order.end());
    if (skipped) fprintf(stderr, "Skipped %llu unmapped reads.\n", (unsigned long long)skipped);
    fprintf(stderr, "Average coverage:\n");
    for (auto &c : order) {
        uint64_t total = 0;
        for (uint64_t i = base[c.second]; i < base[c.second + 1]; ++i) total += bins[i];
        fprintf(stderr, "   %20s: %8gx\n", c.first.c_str(), (double)total / lens[c.second]);
    }
    if (out != "stdout") {
        FILE *f = fopen(out.c_str(), "wb");
        bool ok = f != nullptr;
        if (ok) {
            TsvWriter w(f);
            static const char head[] = "chromosome\tposition\tcoverage\n";
            w.text(head, sizeof head - 1);
            for (auto &c : order) {
                const uint32_t *b = bins.data() + base[c.second];
                const uint64_t m = base[c.second + 1] - base[c.second];
                const std::string row = c.first + "\t";
                for (uint64_t i = 0; i < m; ++i) {
                    if (omit_uncovered && !b[i]) continue;
                    w.text(row.data(), row.size());
                    w.number((uint64_t)binsize * i + 1, '\t');
                    w.number(b[i], '\n');
                }
            }
            w.flush();
            ok = w.ok;
        }
        if ((f && fclose(f) != 0) || !ok) {
            fprintf(stderr, "openge: error writing %s: %s\n", out.c_str(), strerror(errno));
            remove(out.c_str());
            return -1;
        }
    }
    if (overflow) fprintf(stderr, "Error: at least one overflow occurred when measuring coverage- try reducing binsizes.\n");
    report_stages(cc, "qc_coverage", sec(t0, clk()));
    return 0;
}


// ---- compare -------------------------------------------------------------------------------------------
namespace {

// one element of the diff image of oge_compare_dev (include/openge_hip.h)
struct DiffEntry {
    int32_t refid, pos;
    uint64_t surplus;
    uint32_t side;
    std::vector<uint32_t> ops;  // len << 4 | code
};

const char kCigarChars[] = "MIDNSHP=X";

// CompareElement::operator< (command_compare.cpp:50-65): the op's length, then its type CHARACTER
bool diff_less(const DiffEntry &a, const DiffEntry &b) {
    if (a.refid != b.refid) return a.refid < b.refid;
    if (a.pos != b.pos) return a.pos < b.pos;
    if (a.ops.size() != b.ops.size()) return a.ops.size() < b.ops.size();
    for (size_t i = 0; i < a.ops.size(); ++i) {
        if ((a.ops[i] >> 4) != (b.ops[i] >> 4)) return (a.ops[i] >> 4) < (b.ops[i] >> 4);
        const char ta = kCigarChars[a.ops[i] & 0xF], tb = kCigarChars[b.ops[i] & 0xF];
        if (ta != tb) return ta < tb;
    }
    return false;
}

bool decode_diff(const std::vector<uint8_t> &img, uint64_t entries, std::vector<DiffEntry> &out) {
    size_t p = 0;
    out.clear();
    out.reserve(entries);
    for (uint64_t k = 0; k < entries; ++k) {
        if (p + 24 > img.size()) return false;
        DiffEntry e;
        e.refid = oge_rd_i32(img.data() + p);
        e.pos = oge_rd_i32(img.data() + p + 4);
        e.surplus = (uint64_t)oge_rd_u32(img.data() + p + 8) | ((uint64_t)oge_rd_u32(img.data() + p + 12) << 32);
        e.side = oge_rd_u32(img.data() + p + 16);
        const uint32_t nops = oge_rd_u32(img.data() + p + 20);
        if (p + 24 + 4ull * nops > img.size()) return false;
        e.ops.resize(nops);
        for (uint32_t j = 0; j < nops; ++j) e.ops[j] = oge_rd_u32(img.data() + p + 24 + 4 * j);
        p += 24 + 4ull * nops;
        out.push_back(std::move(e));
    }
    return p == img.size();
}

// "Add: " / "Del: " + CompareElement::toString (command_compare.cpp:67-71), once per surplus element
void print_changes(const char *label, uint32_t side, const std::vector<DiffEntry> &d, const std::vector<std::string> &names) {
    std::string line;
    for (const DiffEntry &e : d) {
        if (e.side != side) continue;
        line = label;
        line += names[(size_t)e.refid];
        line += ':';
        line += std::to_string(e.pos);
        line += ' ';
        for (uint32_t op : e.ops) {
            line += std::to_string(op >> 4);
            line += kCigarChars[op & 0xF];
        }
        line += '\n';
        for (uint64_t k = 0; k < e.surplus; ++k) fwrite(line.data(), 1, line.size(), stdout);
    }
}

struct LoadedReads {
    ChainContext &cc;
    ReadBatch b;
    explicit LoadedReads(ChainContext &c) : cc(c) {}
    ~LoadedReads() { cc.free_device(b); }
};

}  // namespace

int compare_files(ChainContext &cc, const std::vector<std::string> &inputs, const std::vector<std::string> &region_strings_in, bool print) {
    // what is held at once: file 0 and one other file, as records in HBM, and the compare's 44 bytes per record
    // of keys.  A BAM file is taken as 8 times its size (records and keys), SAM text as 3 times.
    uint64_t fr = 0, tot = 0, first = 0, largest = 0;
    if (oge_mem_info(cc.ctx, &fr, &tot)) return cc.fail("compare");
    for (size_t i = 0; i < inputs.size(); ++i) {
        struct stat sb;
        if (stat(inputs[i].c_str(), &sb) != 0) continue;  // the reader reports it
        const uint64_t est = (uint64_t)sb.st_size * (file_is_sam(inputs[i]) ? 3 : 8);
        if (i == 0) first = est;
        else largest = std::max(largest, est);
    }
    if (first + largest > tot) {
        fprintf(stderr, "openge compare: the inputs do not fit in device memory together (about %llu MB needed, %llu MB on the device)\n",
                (unsigned long long)((first + largest) >> 20), (unsigned long long)(tot >> 20));
        return -1;
    }
    if (inputs.size() < 2) return 0;  // command_compare.cpp:126-196: nothing is compared, nothing printed

    const auto t_start = clk();
    double t_read = 0, t_compare_ms = 0, t_format = 0;
    LoadedReads ref(cc);
    {
        FileReader reader;
        reader.addFile(inputs[0]);
        if (reader.load(cc, ref.b)) return -1;
    }
    t_read += sec(t_start, clk());
    // regions against file 0's dictionary (command_compare.cpp:100-117)
    std::string names;
    std::vector<int64_t> lens;
    std::vector<std::string> contig;
    for (auto &sq : ref.b.header.sq) {
        names += sq.name;
        names.push_back('\0');
        lens.push_back(sq.length);
        contig.push_back(sq.name);
    }
    std::vector<std::string> region_strings = region_strings_in;
    std::vector<oge_compare_region> regions;
    size_t longest = 0;
    if (!region_strings.empty()) {
        for (const std::string &rs : region_strings) {
            oge_filter_opts o;
            oge_filter_opts_init(&o);
            if (oge_parse_region(rs.c_str(), names.data(), (int32_t)lens.size(), lens.data(), &o)) {
                // Filter::ParseRegionString's own message (none when the string itself does not parse), then the command's
                const std::string why = oge_last_error(nullptr);
                if (why.rfind("ERROR: could not parse", 0) != 0) fprintf(stderr, "%s\n", why.c_str());
                fprintf(stderr, "Couldn't understand region string %s. Exiting.\n", rs.c_str());
                return -1;
            }
            regions.push_back({o.ref_id, o.left_pos, o.ref_id, o.right_pos});
            longest = std::max(longest, rs.size());
        }
    } else {
        region_strings.push_back("");
        regions.push_back({0, 0, INT_MAX, INT_MAX});
    }
    const bool print_file_names = inputs.size() > 2;
    for (size_t f = 1; f < inputs.size(); ++f) {
        const auto t0 = clk();
        LoadedReads other(cc);
        {
            FileReader reader;
            reader.addFile(inputs[f]);
            if (reader.load(cc, other.b)) return -1;
        }
        t_read += sec(t0, clk());
        // The reference's check (command_compare.cpp:140-144) takes both dictionaries from file 0's reader, so its
        // warning never appears; here it is real, and shown with -v only: without -v stderr stays the reference's
        if (cc.verbose && (other.b.header.sq.size() != ref.b.header.sq.size() || other.b.ref_names != ref.b.ref_names))
            fprintf(stderr, "Sequence dictionaries between %s and %s differ. This may produce inconsistent results.\n", inputs[0].c_str(),
                    inputs[f].c_str());
        if (print_file_names) {
            fflush(stdout);
            fprintf(stderr, "%s:\n", inputs[f].c_str());
        }
        for (size_t r = 0; r < regions.size(); ++r) {
            oge_compare_result res;
            const uint8_t *d_diff = nullptr;
            uint64_t diff_bytes = 0;
            std::vector<uint8_t> img;
            int rc = oge_compare_dev(cc.ctx, ref.b.d_recs, ref.b.d_offs, ref.b.n, other.b.d_recs, other.b.d_offs, other.b.n,
                                     (int32_t)contig.size(), &regions[r], print ? OGE_COMPARE_DIFF : 0, -1, &res, &d_diff, &diff_bytes);
            if (!rc && diff_bytes) {
                img.resize(diff_bytes);
                rc = oge_memcpy(cc.ctx, img.data(), d_diff, diff_bytes, 2);
            }
            if (rc) return cc.fail("compare");
            double ms = 0;
            oge_ctx_timing(cc.ctx, "compare", &ms);
            t_compare_ms += ms;
            const auto tf = clk();
            if (print) {
                std::vector<DiffEntry> d;
                if (!decode_diff(img, res.diff_entries, d)) {
                    fprintf(stderr, "openge compare: malformed diff image\n");
                    return -1;
                }
                std::sort(d.begin(), d.end(), diff_less);
                print_changes("Add: ", 1, d, contig);
                print_changes("Del: ", 0, d, contig);
            }
            if (res.additions || res.deletions)
                printf("%s%*s\t%8llu added\t%8llu removed\n", print_file_names ? "   " : "", (int)longest, region_strings[r].c_str(),
                       (unsigned long long)res.additions, (unsigned long long)res.deletions);
            t_format += sec(tf, clk());
        }
    }
    const bool ok = fflush(stdout) == 0 && !ferror(stdout);
    if (cc.verbose)
        fprintf(stderr, "[openge] compare: read + inflate %.3f s, compare %.1f ms on the device, format %.3f s, total %.3f s\n", t_read,
                t_compare_ms, t_format, sec(t_start, clk()));
    if (!ok) {
        fprintf(stderr, "openge: error writing to stdout\n");
        return -1;
    }
    return 0;
}

}  // namespace oge
