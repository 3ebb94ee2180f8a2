// host_capi.cpp -- host-only entry points of libopenge_hip.so: synthetic data, BAM files.
#include "../../include/openge_hip.h"
#include "bamio.h"
#include "capi_common.h"
#include "lib_table.h"
#include "synth.h"

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

using namespace oge;

template <class F>
static void host_parallel(uint64_t n, int threads, F f) {
    if (threads <= 0) threads = (int)std::max(1u, std::thread::hardware_concurrency());
    uint64_t chunk = std::max<uint64_t>(4096, (n + threads * 8 - 1) / (threads * 8));
    std::atomic<uint64_t> next(0);
    std::vector<std::thread> ts;
    for (int t = 0; t < threads; ++t)
        ts.emplace_back([&]() {
            for (;;) {
                uint64_t b = next.fetch_add(chunk);
                if (b >= n) break;
                uint64_t e = std::min(n, b + chunk);
                for (uint64_t i = b; i < e; ++i) f(i);
            }
        });
    for (auto &t : ts) t.join();
}

extern "C" {

uint64_t oge_synth_params_size(void) { return sizeof(oge_synth_params); }

int oge_synth_finalize(void *params) {
    oge_synth_params *P = (oge_synth_params *)params;
    if (!P || P->n_ref == 0 || P->n_ref > OGE_SYNTH_MAX_REF || P->read_len == 0 || P->read_len > 250 ||
        P->n_rg == 0 || P->n_rg > 9 || P->ins_max < P->ins_min || P->qual_max < P->qual_min || P->qual_max > 255)
        return oge_fail(nullptr, OGE_ERR_ARG, "oge_synth_finalize: parameters out of range");
    P->ref_cum[0] = 0;
    for (uint32_t i = 0; i < P->n_ref; ++i) {
        if (P->ref_len[i] <= (uint64_t)P->ins_max + 1 || P->ref_len[i] > 0x7FFFFFFFull)
            return oge_fail(nullptr, OGE_ERR_ARG, "oge_synth_finalize: contig shorter than the insert size");
        P->ref_cum[i + 1] = P->ref_cum[i] + P->ref_len[i];
    }
    return OGE_OK;
}

int oge_synth_offsets_host(const void *params, uint64_t *offs, int threads) {
    const oge_synth_params *P = (const oge_synth_params *)params;
    uint64_t n = 2 * P->n_pairs;
    std::vector<uint32_t> sz(n);
    host_parallel(n, threads, [&](uint64_t s) { sz[s] = oge_synth_slot_bytes(P, s); });
    uint64_t acc = 0;
    for (uint64_t s = 0; s < n; ++s) { offs[s] = acc; acc += sz[s]; }
    offs[n] = acc;
    return OGE_OK;
}

int oge_synth_records_host(const void *params, const uint64_t *offs, uint8_t *out, int threads) {
    const oge_synth_params *P = (const oge_synth_params *)params;
    uint64_t n = 2 * P->n_pairs;
    host_parallel(n, threads, [&](uint64_t s) { oge_synth_write_slot(P, s, out + offs[s]); });
    return OGE_OK;
}

int oge_synth_header_text(const void *params, char *buf, uint64_t cap, uint64_t *len_out) {
    const oge_synth_params *P = (const oge_synth_params *)params;
    std::string t = "@HD\tVN:1.4\tSO:unsorted\n";
    for (uint32_t i = 0; i < P->n_ref; ++i)
        t += "@SQ\tSN:chr" + std::to_string(i + 1) + "\tLN:" + std::to_string(P->ref_len[i]) + "\n";
    for (uint32_t g = 1; g <= P->n_rg; ++g)
        t += "@RG\tID:rg" + std::to_string(g) + "\tLB:lib" + std::to_string(g) + "\tSM:sample1\n";
    if (len_out) *len_out = t.size();
    if (buf && cap) {
        size_t k = std::min<size_t>(cap - 1, t.size());
        memcpy(buf, t.data(), k);
        buf[k] = 0;
    }
    return OGE_OK;
}

struct oge_bam { BamFile f; };

int oge_bam_read(const char *path, int threads, oge_bam **out) {
    if (!path || !out) return oge_fail(nullptr, OGE_ERR_ARG, "oge_bam_read: null argument");
    oge_bam *b = new oge_bam();
    std::string err;
    if (!bam_read_file(path, b->f, threads <= 0 ? 8 : threads, err)) {
        delete b;
        return oge_fail(nullptr, OGE_ERR_IO, ("oge_bam_read: " + err).c_str());
    }
    *out = b;
    return OGE_OK;
}
void oge_bam_free(oge_bam *b) { delete b; }
uint64_t oge_bam_count(const oge_bam *b) { return b->f.offsets.size(); }
const uint8_t *oge_bam_records(const oge_bam *b, uint64_t *bytes_out) {
    if (bytes_out) *bytes_out = b->f.rec_bytes();
    return b->f.recs();
}
const uint64_t *oge_bam_offsets(const oge_bam *b) { return b->f.offsets.data(); }
int32_t oge_bam_n_ref(const oge_bam *b) { return (int32_t)b->f.ref_names.size(); }

int oge_bam_header_text(const oge_bam *b, char *buf, uint64_t cap, uint64_t *len_out) {
    std::string t = b->f.header.to_string();
    if (len_out) *len_out = t.size();
    if (buf && cap) {
        size_t k = std::min<size_t>(cap - 1, t.size());
        memcpy(buf, t.data(), k);
        buf[k] = 0;
    }
    return OGE_OK;
}

int oge_bam_markdup_opts(const oge_bam *b, oge_markdup_opts *opts, char **rg_ids_buf, int16_t **rg_lib_buf) {
    // the header's table (lib_table.h) in malloc'd copies that the caller frees
    const LibTable lt(b->f.header);
    char *idbuf = (char *)malloc(lt.ids.size() + 1);
    int16_t *libs = (int16_t *)malloc(sizeof(int16_t) * lt.rg_lib.size());
    memcpy(idbuf, lt.ids.c_str(), lt.ids.size() + 1);
    memcpy(libs, lt.rg_lib.data(), sizeof(int16_t) * lt.rg_lib.size());
    *opts = lt.opts((int32_t)b->f.ref_names.size());
    opts->rg_ids = idbuf;
    opts->rg_lib = libs;
    *rg_ids_buf = idbuf;
    *rg_lib_buf = libs;
    return OGE_OK;
}

int oge_bam_write(const char *path, const char *header_text, uint64_t header_len, int sort_order,
                  const uint8_t *recs, const uint64_t *offs, uint64_t n, const uint32_t *order,
                  const uint16_t *flags, int level, int threads) {
    BamHeaderModel h;
    std::string err;
    if (!h.parse(std::string(header_text, header_len), err))
        return oge_fail(nullptr, OGE_ERR_ARG, ("oge_bam_write: " + err).c_str());
    if (sort_order >= 0) h.sort_order = (BamHeaderModel::SortOrder)sort_order;
    FILE *f = (strcmp(path, "-") == 0 || strcmp(path, "stdout") == 0) ? stdout : fopen(path, "wb");
    if (!f) return oge_fail(nullptr, OGE_ERR_IO, "oge_bam_write: cannot open output");
    {
        BgzfWriter w(f, level, threads <= 0 ? 8 : threads);
        std::vector<uint8_t> hb = bam_encode_header(h);
        w.write(hb.data(), hb.size());
        std::vector<uint8_t> tmp;
        for (uint64_t k = 0; k < n; ++k) {
            uint64_t i = order ? order[k] : k;
            const uint8_t *r = recs + offs[i];
            uint32_t bs;
            memcpy(&bs, r, 4);
            // BamSerializer::write recomputes bin on every record (util/bam_serializer.h:112-116)
            tmp.assign(r, r + 4 + bs);
            oge_wr_u16(tmp.data() + OGE_OFF_BIN, oge_rec_bin(tmp.data()));
            if (flags) oge_wr_u16(tmp.data() + OGE_OFF_FLAG, flags[i]);
            w.write(tmp.data(), tmp.size());
        }
        w.close();
    }
    if (f != stdout) fclose(f);
    return OGE_OK;
}

} // extern "C"

// ----------------------------------------------------------------------------- duplication metrics (host side)
// Picard's DuplicationMetrics.estimateLibrarySize; the order of the operations is part of the definition
// (include/openge_hip.h, tests/dupmetrics_model.py): the tests ask for the same doubles.
extern "C" int oge_estimate_library_size(uint64_t pairs, uint64_t unique_pairs, uint64_t *size) {
    if (!(pairs > 0 && pairs > unique_pairs)) return 1;
    const double n = (double)pairs, c = (double)unique_pairs;
    auto f = [&](double x) { return c / x - 1 + exp(-n / x); };
    double m = 1, M = 100;
    while (f(M * c) > 0) M *= 10;
    for (int i = 0; i < 40; ++i) {
        const double r = (m + M) / 2;
        const double u = f(r * c);
        if (u == 0) break;
        if (u > 0) m = r;
        else M = r;
    }
    if (size) *size = (uint64_t)(c * (m + M) / 2);
    return 0;
}

extern "C" int oge_dup_metrics_text(const char *const *names, const struct oge_dup_metrics *m, int32_t n_rows, const char *command_line, char *buf,
                                    uint64_t cap, uint64_t *len_out) {
    if (n_rows < 0 || (n_rows && (!names || !m)) || !command_line) return oge_fail(nullptr, OGE_ERR_ARG, "oge_dup_metrics_text: null argument");
    std::vector<int32_t> order(n_rows);
    for (int32_t i = 0; i < n_rows; ++i) {
        if (!names[i]) return oge_fail(nullptr, OGE_ERR_ARG, "oge_dup_metrics_text: null name");
        order[i] = i;
    }
    // byte order (strcmp compares unsigned chars), whatever the locale says; equal names keep the caller's order
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return strcmp(names[a], names[b]) < 0; });
    std::string t = "## htsjdk.samtools.metrics.StringHeader\n# ";
    t += command_line;
    t += "\n\n## METRICS CLASS\tpicard.sam.DuplicationMetrics\n"
         "LIBRARY\tUNPAIRED_READS_EXAMINED\tREAD_PAIRS_EXAMINED\tSECONDARY_OR_SUPPLEMENTARY_RDS\tUNMAPPED_READS\tUNPAIRED_READ_DUPLICATES\t"
         "READ_PAIR_DUPLICATES\tREAD_PAIR_OPTICAL_DUPLICATES\tPERCENT_DUPLICATION\tESTIMATED_LIBRARY_SIZE\n";
    char num[64];
    uint64_t pairs = 0, dup_pairs = 0, size = 0;
    bool has_size = false;
    for (int32_t i : order) {
        const struct oge_dup_metrics &x = m[i];
        pairs = x.pair_reads_examined / 2;
        dup_pairs = x.pair_read_dups / 2;
        const uint64_t den = x.unpaired_examined + x.pair_reads_examined;
        const double pct = den ? (double)(x.unpaired_dups + x.pair_read_dups) / (double)den : 0.0;
        has_size = oge_estimate_library_size(pairs, pairs - dup_pairs, &size) == 0;  // more duplicates than pairs: none
        t += names[i];
        for (uint64_t v : {x.unpaired_examined, pairs, x.secondary, x.unmapped, x.unpaired_dups, dup_pairs, (uint64_t)0}) t += "\t" + std::to_string(v);
        snprintf(num, sizeof num, "\t%.6f\t", pct);
        t += num;
        if (has_size) t += std::to_string(size);
        t += "\n";
    }
    t += "\n";
    // the return on investment of sequencing x times as deep; an estimate of 0 (no unique pair: the bisection ran on
    // NaNs) has none
    if (n_rows == 1 && has_size && size) {
        const double L = (double)size, n = (double)pairs, c = (double)(pairs - dup_pairs);
        t += "## HISTOGRAM\tjava.lang.Double\nBIN\tVALUE\n";
        for (int k = 1; k <= 100; ++k) {
            const double x = (double)k;
            snprintf(num, sizeof num, "%d.0\t%.6f\n", k, L * (1 - exp(-(x * n) / L)) / c);
            t += num;
        }
        t += "\n";
    }
    if (len_out) *len_out = t.size();
    if (buf && cap) {
        const size_t k = std::min<size_t>(cap - 1, t.size());
        memcpy(buf, t.data(), k);
        buf[k] = 0;
    }
    return OGE_OK;
}

// The same file with the optical column filled and the set-size histogram (--optical-distance; DESIGN.md section 27,
// tests/dupsets_model.py).  oge_dup_metrics_text stays as it is: without the option every byte is the one it wrote.
extern "C" int oge_dup_sets_text(const char *const *names, const struct oge_dup_metrics *m, const struct oge_dup_sets_lib *s, int32_t n_rows,
                                 const uint64_t *hist, const char *command_line, char *buf, uint64_t cap, uint64_t *len_out) {
    if (n_rows < 0 || (n_rows && (!names || !m || !s)) || !hist || !command_line) return oge_fail(nullptr, OGE_ERR_ARG, "oge_dup_sets_text: null argument");
    std::vector<int32_t> order(n_rows);
    for (int32_t i = 0; i < n_rows; ++i) {
        if (!names[i]) return oge_fail(nullptr, OGE_ERR_ARG, "oge_dup_sets_text: null name");
        order[i] = i;
    }
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return strcmp(names[a], names[b]) < 0; });
    std::string t = "## htsjdk.samtools.metrics.StringHeader\n# ";
    t += command_line;
    t += "\n\n## METRICS CLASS\tpicard.sam.DuplicationMetrics\n"
         "LIBRARY\tUNPAIRED_READS_EXAMINED\tREAD_PAIRS_EXAMINED\tSECONDARY_OR_SUPPLEMENTARY_RDS\tUNMAPPED_READS\tUNPAIRED_READ_DUPLICATES\t"
         "READ_PAIR_DUPLICATES\tREAD_PAIR_OPTICAL_DUPLICATES\tPERCENT_DUPLICATION\tESTIMATED_LIBRARY_SIZE\n";
    char num[64];
    uint64_t pairs = 0, dup_pairs = 0, optical = 0, size = 0;
    bool has_size = false;
    for (int32_t i : order) {
        const struct oge_dup_metrics &x = m[i];
        pairs = x.pair_reads_examined / 2;
        dup_pairs = x.pair_read_dups / 2;
        optical = s[i].optical;
        const uint64_t den = x.unpaired_examined + x.pair_reads_examined;
        const double pct = den ? (double)(x.unpaired_dups + x.pair_read_dups) / (double)den : 0.0;
        // more optical duplicates or more duplicates than pairs: no estimate
        has_size = optical <= pairs && dup_pairs <= pairs && oge_estimate_library_size(pairs - optical, pairs - dup_pairs, &size) == 0;
        t += names[i];
        for (uint64_t v : {x.unpaired_examined, pairs, x.secondary, x.unmapped, x.unpaired_dups, dup_pairs, optical}) t += "\t" + std::to_string(v);
        snprintf(num, sizeof num, "\t%.6f\t", pct);
        t += num;
        if (has_size) t += std::to_string(size);
        t += "\n";
    }
    t += "\n";
    const bool roi = n_rows == 1 && has_size && size;
    int last = 0;
    for (int k = 1; k < OGE_DUP_SETS_BINS; ++k)
        if (hist[k] || hist[OGE_DUP_SETS_BINS + k] || hist[2 * OGE_DUP_SETS_BINS + k]) last = k;
    if (roi && last < 100) last = 100;
    t += "## HISTOGRAM\tjava.lang.Double\nBIN";
    if (roi) t += "\tCoverageMult";
    t += "\tall_sets\toptical_sets\tnon_optical_sets\n";
    const double L = (double)size, n = (double)(pairs - optical), c = (double)(pairs - dup_pairs);
    for (int k = 1; k <= last; ++k) {
        snprintf(num, sizeof num, "%d.0", k);
        t += num;
        if (roi) {
            const double x = (double)k;
            snprintf(num, sizeof num, "\t%.6f", L * (1 - exp(-(x * n) / L)) / c);
            t += num;
        }
        for (int col = 0; col < 3; ++col) t += "\t" + std::to_string(hist[col * OGE_DUP_SETS_BINS + k]);
        t += "\n";
    }
    t += "\n";
    if (len_out) *len_out = t.size();
    if (buf && cap) {
        const size_t k = std::min<size_t>(cap - 1, t.size());
        memcpy(buf, t.data(), k);
        buf[k] = 0;
    }
    return OGE_OK;
}

// ----------------------------------------------------------------------------- Filter (mergesort -r/-q)
extern "C" void oge_filter_opts_init(oge_filter_opts *o) {  // Filter::Filter (filter.cpp:185-194)
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->max_len = INT32_MAX;
    o->count_limit = INT32_MAX;
}

// Filter::ParseRegionString (filter.cpp:31-137): the same parse (atoi on the pieces, so "chr:5-9"
// reads as the single position 5), the last dictionary entry of that name, the same range checks.
extern "C" int oge_parse_region(const char *region, const char *ref_names, int32_t n_ref, const int64_t *ref_len,
                                oge_filter_opts *o) {
    if (!region || !o || (n_ref > 0 && (!ref_names || !ref_len))) return oge_fail(nullptr, OGE_ERR_ARG, "null argument");
    const std::string rs = region;
    const std::string bad = "ERROR: could not parse region'" + rs + "'";
    if (rs.empty()) return oge_fail(nullptr, OGE_ERR_ARG, bad.c_str());
    std::string chrom;
    int start, stop;
    const size_t c1 = rs.find(':');
    if (c1 == std::string::npos) {
        chrom = rs;
        start = 0;
        stop = -1;
    } else {
        chrom = rs.substr(0, c1);
        const size_t dots = rs.find("..", c1 + 1);
        if (dots == std::string::npos) {
            start = atoi(rs.substr(c1 + 1).c_str());
            stop = start;
        } else {
            start = atoi(rs.substr(c1 + 1, dots - c1 - 1).c_str());
            if (rs.find(':', dots + 1) != std::string::npos) return oge_fail(nullptr, OGE_ERR_ARG, bad.c_str());
            stop = atoi(rs.substr(dots + 2).c_str());
        }
    }
    int ref = -1;
    const char *p = ref_names;
    for (int i = 0; i < n_ref; ++i) {
        if (chrom == p) ref = i;
        p += strlen(p) + 1;
    }
    if (ref == -1) return oge_fail(nullptr, OGE_ERR_ARG, ("Can't find chromosome'" + chrom + "'").c_str());
    const int len = (int)ref_len[ref];
    if (start >= len)
        return oge_fail(nullptr, OGE_ERR_ARG,
                        ("Start position (" + std::to_string(start) + ") after end of the reference sequence (" +
                         std::to_string(len) + ")").c_str());
    if (stop > len)  // the reference's message says "Start" here too (filter.cpp:125)
        return oge_fail(nullptr, OGE_ERR_ARG,
                        ("Start position (" + std::to_string(stop) + ") after end of the reference sequence (" +
                         std::to_string(len) + ")").c_str());
    if (stop == -1) stop = len;
    o->has_region = 1;
    o->ref_id = ref;
    o->left_pos = start;
    o->right_pos = stop;
    return OGE_OK;
}
