// sam_parse_main.cpp -- TEST INFRASTRUCTURE (tests/test_sam_parse_host.py): the per-tile and per-line code of the SAM
// input kernels (openge_amd/csrc/sam_parse.h) run on the host, lane by lane, and the host's record builder
// (openge_amd/csrc/sam_host.cpp), both against the bytes of tests/samin_model.py.  Built with
// -fsanitize=address,undefined: the text buffer is exactly the text, the line table exactly n + 1 entries and the
// record buffer the computed size plus 16 bytes of canary that must stay untouched, so a byte stored or read too far is
// reported.
//
// Case file (little endian): u32 n_ref, names_bytes; u32 name_off[n_ref + 1]; names; u64 text_bytes; text;
// i64 expect_bad (0-based line of the body, -1: none); u32 expect_code; u64 n; u64 line_off[n + 1]; u8 mark[n];
// u8 warn[n]; u64 rec_len[n]; the records back to back.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../openge_amd/csrc/sam_host.h"
#include "../../openge_amd/csrc/sam_parse.h"

namespace {

struct Reader {
    std::vector<uint8_t> d;
    size_t p = 0;
    template <class T> T get() {
        T v;
        if (p + sizeof v > d.size()) die("case file cut short");
        memcpy(&v, d.data() + p, sizeof v);
        p += sizeof v;
        return v;
    }
    const uint8_t *take(size_t n) {
        if (p + n > d.size()) die("case file cut short");
        p += n;
        return d.data() + p - n;
    }
    [[noreturn]] static void die(const char *m) {
        fprintf(stderr, "sam_parse_main: %s\n", m);
        exit(2);
    }
};

int fail(const std::string &m) {
    fprintf(stderr, "MISMATCH: %s\n", m.c_str());
    return 1;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) Reader::die("usage: sam_parse_main case.bin");
    Reader rd;
    FILE *f = fopen(argv[1], "rb");
    if (!f) Reader::die("cannot open the case file");
    fseek(f, 0, SEEK_END);
    rd.d.resize((size_t)ftell(f));
    fseek(f, 0, SEEK_SET);
    if (fread(rd.d.data(), 1, rd.d.size(), f) != rd.d.size()) Reader::die("read error");
    fclose(f);

    oge_text_opts o = {0, 0, 0, 0, nullptr, nullptr};
    o.n_ref = (int32_t)rd.get<uint32_t>();
    const uint32_t names_bytes = rd.get<uint32_t>();
    std::vector<uint32_t> name_off(o.n_ref + 1);
    for (auto &v : name_off) v = rd.get<uint32_t>();
    std::vector<uint8_t> names(names_bytes + 8, 0);  // the device table's slack
    if (names_bytes) memcpy(names.data(), rd.take(names_bytes), names_bytes);
    o.ref_names = (const char *)names.data();
    o.ref_name_off = name_off.data();
    const uint64_t bytes = rd.get<uint64_t>();
    uint8_t *text = (uint8_t *)malloc(bytes ? bytes : 1);  // exactly the text
    if (bytes) memcpy(text, rd.take(bytes), bytes);
    const int64_t expect_bad = rd.get<int64_t>();
    const uint32_t expect_code = rd.get<uint32_t>();
    const uint64_t n_want = rd.get<uint64_t>();
    std::vector<uint64_t> want_off(n_want + 1);
    for (auto &v : want_off) v = rd.get<uint64_t>();
    std::vector<uint8_t> want_mark(n_want), want_warn(n_want);
    if (n_want) memcpy(want_mark.data(), rd.take(n_want), n_want);
    if (n_want) memcpy(want_warn.data(), rd.take(n_want), n_want);
    std::vector<uint64_t> want_len(n_want);
    uint64_t rec_bytes = 0;
    for (auto &v : want_len) rec_bytes += v = rd.get<uint64_t>();
    const uint8_t *want_recs = rd.take(rec_bytes);

    std::vector<uint32_t> slots(oge_sam_table_slots(o.n_ref), 0);
    oge_sam_table_build(o.n_ref, names.data(), name_off.data(), slots.data());
    const OgeSamParams sp = {o.n_ref, (uint32_t)slots.size() - 1, names.data(), name_off.data(), slots.data()};

    // ---- line index: count per tile, scan, fill
    uint64_t body = 0;
    while (body < bytes && text[body] == '@') {
        const void *nl = memchr(text + body, '\n', bytes - body);
        body = nl ? (uint64_t)((const uint8_t *)nl - text) + 1 : bytes;
    }
    const uint64_t tile0 = body / OGE_SAM_TILE, n_tiles = bytes > body ? (bytes + OGE_SAM_TILE - 1) / OGE_SAM_TILE - tile0 : 0;
    std::vector<uint64_t> base(n_tiles + 1, 0);
    for (uint64_t w = 0; w < n_tiles; ++w)
        base[w + 1] = base[w] + oge_sam_tile<false>(text, (tile0 + w) * OGE_SAM_TILE, body, bytes, 0, nullptr, 0);
    const bool open_end = bytes > body && text[bytes - 1] != '\n';
    const uint64_t n = base[n_tiles] + (open_end ? 1 : 0);
    if (n != n_want) return fail("line count " + std::to_string(n) + ", the model's " + std::to_string(n_want));
    uint64_t *line_off = (uint64_t *)malloc((n + 1) * 8);  // exactly n + 1 entries
    memset(line_off, 0xAA, (n + 1) * 8);
    for (uint64_t j = 0; j < n_tiles; ++j) {
        const uint64_t w = n_tiles - 1 - j;  // backwards: the order must not matter
        oge_sam_tile<true>(text, (tile0 + w) * OGE_SAM_TILE, body, bytes, base[w], line_off, n);
    }
    line_off[0] = body;
    if (open_end) line_off[n] = bytes + 1;
    for (uint64_t i = 0; i <= n; ++i)
        if (line_off[i] != want_off[i]) return fail("line offset " + std::to_string(i) + ": " + std::to_string(line_off[i]) + ", the model's " + std::to_string(want_off[i]));

    // ---- size pass
    std::vector<uint64_t> rec_off(n + 1, 0);
    std::vector<OgeSamRec> rs(n);
    int64_t first_bad = -1;
    for (uint64_t i = 0; i < n; ++i) {
        rs[i] = oge_sam_line<false>(text + line_off[i], (uint32_t)(line_off[i + 1] - 1 - line_off[i]), sp, nullptr);
        rec_off[i + 1] = rec_off[i] + (rs[i].err ? 0 : rs[i].len);
        if (rs[i].err && first_bad < 0) first_bad = (int64_t)i;
    }
    if (first_bad != expect_bad) return fail("first bad line " + std::to_string(first_bad) + ", expected " + std::to_string(expect_bad));
    if (expect_bad >= 0) {
        if (rs[expect_bad].err != expect_code)
            return fail("line " + std::to_string(expect_bad) + ": error code " + std::to_string(rs[expect_bad].err) + " (" +
                        oge_sam_error_text(rs[expect_bad].err) + "), expected " + std::to_string(expect_code));
        std::vector<uint8_t> rec;
        std::string err;
        bool warn = false;
        if (oge_sam_record_host(text + line_off[expect_bad], line_off[expect_bad + 1] - 1 - line_off[expect_bad], &o, rec, &warn, err))
            return fail("the host builder accepts the bad line");
        printf("ok: line %lld refused (%s; host: %s)\n", (long long)expect_bad, oge_sam_error_text(expect_code), err.c_str());
        free(line_off);
        free(text);
        return 0;
    }
    for (uint64_t i = 0; i < n; ++i) {
        if (rs[i].len != want_len[i]) return fail("line " + std::to_string(i) + ": record length " + std::to_string(rs[i].len) + ", the model's " + std::to_string(want_len[i]));
        if ((rs[i].host != 0) != (want_mark[i] != 0)) return fail("line " + std::to_string(i) + ": host mark");
        if ((rs[i].warn != 0) != (want_warn[i] != 0)) return fail("line " + std::to_string(i) + ": warning bit");
    }
    // ---- emit pass at every alignment of the arena, then the host's records over the marked ones
    const uint64_t total = rec_off[n];
    uint64_t hosts = 0;
    for (int shift = 0; shift < 4; ++shift) {
        const uint64_t room = ((total + shift + 15) / 16 + 1) * 16;
        uint8_t *raw = (uint8_t *)aligned_alloc(16, room);
        memset(raw, 0xAA, room);
        uint8_t *out = raw + shift;
        for (uint64_t j = 0; j < n; ++j) {
            const uint64_t i = shift & 1 ? n - 1 - j : j;  // backwards too: a record that ran into its successor would spoil it
            oge_sam_line<true>(text + line_off[i], (uint32_t)(line_off[i + 1] - 1 - line_off[i]), sp, out + rec_off[i]);
        }
        for (uint64_t i = 0; i < n; ++i) {
            if (!rs[i].host) continue;
            std::vector<uint8_t> rec;
            std::string err;
            bool warn = false;
            if (!oge_sam_record_host(text + line_off[i], line_off[i + 1] - 1 - line_off[i], &o, rec, &warn, err)) return fail("line " + std::to_string(i) + ": host builder: " + err);
            if (rec.size() != rs[i].len) return fail("line " + std::to_string(i) + ": the host's record has another length than the size pass gave");
            memcpy(out + rec_off[i], rec.data(), rec.size());
            hosts += shift == 0;
        }
        if (total && memcmp(out, want_recs, total)) {
            uint64_t k = 0;
            while (out[k] == want_recs[k]) ++k;
            uint64_t i = 0;
            while (rec_off[i + 1] <= k) ++i;
            return fail("emit (alignment " + std::to_string(shift) + "): byte " + std::to_string(k) + " of the arena, line " + std::to_string(i) +
                        " at its record's byte " + std::to_string(k - rec_off[i]));
        }
        for (uint64_t k = total + shift; k < room; ++k)
            if (raw[k] != 0xAA) return fail("emit wrote past the arena");
        for (int k = 0; k < shift; ++k)
            if (raw[k] != 0xAA) return fail("emit wrote in front of the arena");
        free(raw);
    }
    // ---- the host builder on every line
    for (uint64_t i = 0; i < n; ++i) {
        std::vector<uint8_t> rec;
        std::string err;
        bool warn = false;
        if (!oge_sam_record_host(text + line_off[i], line_off[i + 1] - 1 - line_off[i], &o, rec, &warn, err)) return fail("line " + std::to_string(i) + ": host builder: " + err);
        if (rec.size() != want_len[i] || memcmp(rec.data(), want_recs + rec_off[i], rec.size())) return fail("line " + std::to_string(i) + ": host record");
        if (warn != (want_warn[i] != 0)) return fail("line " + std::to_string(i) + ": host warning");
    }
    printf("ok: %llu lines, %llu record bytes, %llu host lines\n", (unsigned long long)n, (unsigned long long)total, (unsigned long long)hosts);
    free(line_off);
    free(text);
    return 0;
}
