// fasta_selftest.cpp -- CPU harness for the FASTA loader and the reference table `openge calmd` uploads
// (openge_amd/csrc/fasta.h, host_pool.h).  Writes its own files into the directory it is given, loads each and
// lays out the table for a contig list, and checks names, sequences, offsets, lengths and the slack bytes: lines of
// 60 and 61 bases and a sequence that ends on a full line, CRLF, a last line without a newline, an empty contig, a
// name with a trailing description (blank and tab), a repeated name, a contig of the header that the FASTA lacks and
// one listed twice, lower case and bytes that are no letters, a second load into the same object, a file that does
// not exist and one without a sequence.  Built with -fsanitize=address,undefined and run by tests/test_fasta_native.py.
//
//   fasta_selftest DIR [threads]
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "fasta.h"

using namespace oge;

static int g_failed = 0;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                      \
        }                                                                    \
    } while (0)

static std::string write_file(const std::string &dir, const char *name, const std::string &content) {
    const std::string path = dir + "/" + name;
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(content.data(), 1, content.size(), f) != content.size()) {
        fprintf(stderr, "cannot write %s\n", path.c_str());
        exit(2);
    }
    fclose(f);
    return path;
}

static std::string bases(size_t n, unsigned seed) {
    std::string s(n, 'A');
    for (size_t i = 0; i < n; ++i) {
        seed = seed * 1664525u + 1013904223u;
        s[i] = "ACGT"[seed >> 30];
    }
    return s;
}

static std::string lined(const std::string &s, size_t width, const char *eol, bool last_eol = true) {
    std::string out;
    for (size_t i = 0; i < s.size(); i += width) {
        out += s.substr(i, width);
        if (i + width < s.size() || last_eol) out += eol;
    }
    return out;
}

static std::string table_seq(const RefTable &t, size_t r) {
    return t.off[r] < 0 ? std::string() : std::string((const char *)t.bytes.data() + t.off[r], (size_t)t.len[r]);
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: fasta_selftest DIR [threads]\n");
        return 2;
    }
    const std::string dir = argv[1];
    Pool pool(argc > 2 ? atoi(argv[2]) : 4);
    std::string err;

    // ---- line geometry: 60 and 61 bases per line, a sequence of whole lines, one base, 8 MiB preads over a chunk edge
    const std::string a = bases(125, 1), b = bases(122, 2), c = bases(120, 3), d = bases(1, 4), big = bases((9u << 20) + 7, 5);
    const std::string geo = ">a\n" + lined(a, 60, "\n") + ">b\n" + lined(b, 61, "\n") + ">c\n" + lined(c, 60, "\n") + ">d\n" + lined(d, 60, "\n") +
                            ">big\n" + lined(big, 60, "\n");
    Fasta fa;
    CHECK(fa.load(write_file(dir, "geo.fa", geo), err, pool));
    CHECK(fa.seq.size() == 5);
    CHECK(fa.get("a") && *fa.get("a") == a);
    CHECK(fa.get("b") && *fa.get("b") == b);
    CHECK(fa.get("c") && *fa.get("c") == c);
    CHECK(fa.get("d") && *fa.get("d") == d);
    CHECK(fa.get("big") && *fa.get("big") == big);
    CHECK(!fa.get("e"));
    {
        // the table: header order, a contig the FASTA lacks, one listed twice; contigs the list lacks stay out
        RefTable t;
        const std::vector<std::string> names = {"c", "nope", "a", "c", "d"};
        build_ref_table(fa, names, pool, t);
        CHECK(t.off.size() == 5 && t.len.size() == 5);
        CHECK(t.off[0] == 0 && t.len[0] == 120);
        CHECK(t.off[1] == -1 && t.len[1] == 0);
        CHECK(t.off[2] == 120 && t.len[2] == 125);
        CHECK(t.off[3] == 245 && t.len[3] == 120);
        CHECK(t.off[4] == 365 && t.len[4] == 1);
        CHECK(t.bytes.size() == 366 + 8);
        CHECK(table_seq(t, 0) == c && table_seq(t, 2) == a && table_seq(t, 3) == c && table_seq(t, 4) == d);
        for (size_t k = 366; k < t.bytes.size(); ++k) CHECK(t.bytes[k] == 0);
        RefTable none;
        build_ref_table(fa, {}, pool, none);
        CHECK(none.off.empty() && none.bytes.size() == 8);
        RefTable missing;
        build_ref_table(fa, {"x", "y"}, pool, missing);
        CHECK(missing.off[0] == -1 && missing.off[1] == -1 && missing.bytes.size() == 8);
    }

    // ---- CRLF, names with descriptions, an empty contig, a repeated name, a last line without its newline,
    //      lower case and other bytes; loaded into the object that held the first file
    const std::string odd = ">one first contig\r\n" + lined(a, 60, "\r\n") + ">empty\n>two\tdescribed by a tab\n" + lined(b, 61, "\n") +
                            ">one again\nacgtNnRy*-\n>last\n" + lined(c, 60, "\n", false);
    CHECK(odd.back() != '\n');
    CHECK(fa.load(write_file(dir, "odd.fa", odd), err, pool));
    CHECK(fa.seq.size() == 4);  // the first file's contigs are gone
    CHECK(!fa.get("a") && !fa.get("big"));
    CHECK(fa.get("one") && *fa.get("one") == "acgtNnRy*-");  // the last of a repeated name; case kept by the loader
    CHECK(fa.get("empty") && fa.get("empty")->empty());
    CHECK(fa.get("two") && *fa.get("two") == b);
    CHECK(fa.get("last") && *fa.get("last") == c);
    {
        RefTable t;
        build_ref_table(fa, {"one", "empty", "two", "last", "gone"}, pool, t);
        CHECK(table_seq(t, 0) == "ACGTNNRY*-");  // a..z upper-cased, everything else as it is
        CHECK(t.off[1] == 10 && t.len[1] == 0);  // an empty contig is there, with no bytes
        CHECK(t.off[2] == 10 && table_seq(t, 2) == b);
        CHECK(table_seq(t, 3) == c && t.off[4] == -1);
        CHECK(t.bytes.size() == 10 + b.size() + c.size() + 8);
    }
    // CRLF on the last line without LF, and a header as the file's last line
    CHECK(fa.load(write_file(dir, "tail.fa", ">x\r\nAC\r\nGT\r\n>y"), err, pool));
    CHECK(fa.get("x") && *fa.get("x") == "ACGT" && fa.get("y") && fa.get("y")->empty());

    // ---- errors
    Fasta bad;
    CHECK(!bad.load(dir + "/does_not_exist.fa", err, pool) && err.find("cannot open") != std::string::npos);
    CHECK(!bad.load(write_file(dir, "none.fa", "no header here\n"), err, pool) && err.find("no sequences") != std::string::npos);
    CHECK(!bad.load(write_file(dir, "zero.fa", ""), err, pool));

    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("fasta_selftest ok\n");
    return 0;
}
