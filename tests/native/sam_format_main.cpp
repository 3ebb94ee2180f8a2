// sam_format_main.cpp -- TEST INFRASTRUCTURE (tests/test_sam_host.py): the per-record code of the SAM / FASTQ
// kernels (openge_amd/csrc/sam_format.h) run on the host, lane by lane, and the host formatter
// (openge_amd/csrc/sam_host.cpp), both against the bytes of tests/sam_model.py.  Built with
// -fsanitize=address,undefined: the output buffer is the size the size pass computed, rounded up to 16 bytes plus 16 of
// canary that must stay untouched, and the records carry exactly the arenas' 16 bytes of slack, so a byte stored
// or read too far is reported.
//
// Case file (little endian): u32 mode, trim_begin, trim_end, n_ref, names_bytes; u32 name_off[n_ref + 1]; names;
// u64 n, rec_bytes; u64 off[n]; records; i64 expect_bad (-1: none); u8 mark[n]; u64 line_len[n]; the whole text
// (sum of line_len bytes: every record's line, the host's included).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../openge_amd/csrc/sam_format.h"
#include "../../openge_amd/csrc/sam_host.h"

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
        fprintf(stderr, "sam_format_main: %s\n", m);
        exit(2);
    }
};

int fail(const std::string &m) {
    fprintf(stderr, "MISMATCH: %s\n", m.c_str());
    return 1;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) Reader::die("usage: sam_format_main case.bin");
    Reader rd;
    FILE *f = fopen(argv[1], "rb");
    if (!f) Reader::die("cannot open the case file");
    fseek(f, 0, SEEK_END);
    rd.d.resize((size_t)ftell(f));
    fseek(f, 0, SEEK_SET);
    if (fread(rd.d.data(), 1, rd.d.size(), f) != rd.d.size()) Reader::die("read error");
    fclose(f);

    oge_text_opts o;
    o.mode = (int32_t)rd.get<uint32_t>();
    o.trim_begin = (int32_t)rd.get<uint32_t>();
    o.trim_end = (int32_t)rd.get<uint32_t>();
    o.n_ref = (int32_t)rd.get<uint32_t>();
    const uint32_t names_bytes = rd.get<uint32_t>();
    std::vector<uint32_t> name_off(o.n_ref + 1);
    for (auto &v : name_off) v = rd.get<uint32_t>();
    std::vector<uint8_t> names(names_bytes + 8, 0);  // the device table's slack
    if (names_bytes) memcpy(names.data(), rd.take(names_bytes), names_bytes);
    o.ref_names = (const char *)names.data();
    o.ref_name_off = name_off.data();
    const uint64_t n = rd.get<uint64_t>(), rec_bytes = rd.get<uint64_t>();
    std::vector<uint64_t> off(n);
    for (auto &v : off) v = rd.get<uint64_t>();
    std::vector<uint8_t> recs(rec_bytes + 16, 0);
    if (rec_bytes) memcpy(recs.data(), rd.take(rec_bytes), rec_bytes);
    const int64_t expect_bad = rd.get<int64_t>();
    std::vector<uint8_t> want_mark(n);
    if (n) memcpy(want_mark.data(), rd.take(n), n);
    std::vector<uint64_t> want_len(n);
    uint64_t text_bytes = 0;
    for (auto &v : want_len) text_bytes += v = rd.get<uint64_t>();
    const uint8_t *want_text = rd.take(text_bytes);

    const OgeTextParams tp = {o.mode, o.trim_begin, o.trim_end, o.n_ref, names.data(), name_off.data()};
    // ---- size pass
    std::vector<uint64_t> text_off(n + 1, 0);
    std::vector<uint32_t> mark(n);
    int64_t first_bad = -1;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t len = oge_text_record_size(recs.data() + off[i], tp, &mark[i]);
        text_off[i + 1] = text_off[i] + len;
        if (mark[i] == OGE_TXT_BAD && first_bad < 0) first_bad = (int64_t)i;
        if (mark[i] != OGE_TXT_DEVICE && len) return fail("record " + std::to_string(i) + ": a marked record has a length");
    }
    if (first_bad != expect_bad) return fail("first bad record " + std::to_string(first_bad) + ", expected " + std::to_string(expect_bad));
    if (expect_bad >= 0) {
        std::string line, err;
        const uint8_t *r = recs.data() + off[expect_bad];
        if (oge_text_line_host(r, 4 + (uint64_t)oge_rd_u32(r), &o, line, err)) return fail("the host formatter accepts the bad record");
        printf("ok: record %lld refused (%s)\n", (long long)expect_bad, err.c_str());
        return 0;
    }
    for (uint64_t i = 0; i < n; ++i) {
        if ((mark[i] == OGE_TXT_HOST) != (want_mark[i] != 0)) return fail("record " + std::to_string(i) + ": mark");
        if (text_off[i + 1] - text_off[i] != (want_mark[i] ? 0 : want_len[i]))
            return fail("record " + std::to_string(i) + ": length " + std::to_string(text_off[i + 1] - text_off[i]) + ", the model's " +
                        std::to_string(want_len[i]));
    }
    // ---- emit pass, lane by lane, at every alignment of the output buffer
    const uint64_t total = text_off[n];
    std::vector<uint8_t> want_dev;
    {
        uint64_t p = 0;
        for (uint64_t i = 0; i < n; p += want_len[i], ++i)
            if (!want_mark[i]) want_dev.insert(want_dev.end(), want_text + p, want_text + p + want_len[i]);
    }
    for (int shift = 0; shift < 4; ++shift) {
        uint8_t *raw = (uint8_t *)aligned_alloc(16, ((total + shift + 15) / 16 + 1) * 16);
        memset(raw, 0xAA, ((total + shift + 15) / 16 + 1) * 16);
        uint8_t *out = raw + shift;
        for (uint64_t j = 0; j < n; ++j) {
            const uint64_t i = shift & 1 ? n - 1 - j : j;  // backwards too: a record that ran into its successor would spoil it
            const uint64_t len = text_off[i + 1] - text_off[i];
            if (!len) continue;
            for (uint32_t lane = 0; lane < 64; ++lane) oge_text_record_emit(recs.data() + off[i], tp, out + text_off[i], (uint32_t)len, lane);
        }
        if (total && memcmp(out, want_dev.data(), total)) {
            uint64_t k = 0;
            while (out[k] == want_dev[k]) ++k;
            uint64_t i = 0;
            while (text_off[i + 1] <= k) ++i;
            return fail("emit (alignment " + std::to_string(shift) + "): byte " + std::to_string(k) + " of the text, record " + std::to_string(i) +
                        " at its byte " + std::to_string(k - text_off[i]));
        }
        for (uint64_t k = total + shift; k < ((total + shift + 15) / 16 + 1) * 16; ++k)
            if (raw[k] != 0xAA) return fail("emit wrote past the text");
        for (int k = 0; k < shift; ++k)
            if (raw[k] != 0xAA) return fail("emit wrote in front of the text");
        free(raw);
    }
    // ---- the host formatter on every record, and the splice
    uint64_t hosts = 0;
    for (uint64_t i = 0, p = 0; i < n; p += want_len[i], ++i) {
        std::string line, err;
        const uint8_t *r = recs.data() + off[i];
        if (!oge_text_line_host(r, 4 + (uint64_t)oge_rd_u32(r), &o, line, err)) return fail("record " + std::to_string(i) + ": host formatter: " + err);
        if (line.size() != want_len[i] || memcmp(line.data(), want_text + p, line.size())) return fail("record " + std::to_string(i) + ": host line");
        hosts += mark[i] == OGE_TXT_HOST;
    }
    printf("ok: %llu records, %llu bytes on the device path, %llu host lines\n", (unsigned long long)n, (unsigned long long)total,
           (unsigned long long)hosts);
    return 0;
}
