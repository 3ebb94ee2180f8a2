// fasta.h -- the reference FASTA on the host: the loader the realigner reads its windows from (realign.cpp) and the
// table `openge calmd` uploads (calmd.hip): the sequences of a contig list back to back, upper-cased.
#pragma once
#include <sys/types.h>
#include <unistd.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iterator>
#include <string>
#include <unordered_map>
#include <vector>

#include "host_pool.h"

namespace oge {

// =====================================================================================  FASTA
// FastaReader (util/fasta_reader.cpp): sequences by name; readSequence(name, start, length) returns
// the raw bytes (case preserved).
struct Fasta {
    std::unordered_map<std::string, std::string> seq;
    BigVec<char> data;  // the file (kept, like the sequences' storage, for the next load: see Scratch; no zero
                        // fill on a resize, the workers' preads touch its pages first)
    size_t find_nl(size_t from) const {
        if (from >= data.size()) return std::string::npos;
        const void *q = memchr(data.data() + from, '\n', data.size() - from);
        return q ? (size_t)((const char *)q - data.data()) : std::string::npos;
    }
    // Whole file in one read; contigs (">" lines) located serially, their bodies de-lined in
    // parallel.  Line handling as FastaReader: name up to the first blank, CR before LF dropped.
    bool load(const std::string &path, std::string &err, Pool &pool) {
        FILE *f = fopen(path.c_str(), "rb");
        if (!f) {
            err = "cannot open reference FASTA " + path;
            return false;
        }
        data.clear();
        if (fseeko(f, 0, SEEK_END) == 0) {  // regular file: 8 MiB preads on the workers
            const off_t sz = ftello(f);
            if (sz > 0) {
                data.resize((size_t)sz);
                const int fd = fileno(f);
                const size_t chunk = 8ull << 20;
                std::atomic<bool> shortr(false);
                pool.run_chunks((size_t)sz, chunk, [&](size_t o, size_t e) {
                    while (o < e) {
                        const ssize_t r = pread(fd, &data[o], e - o, (off_t)o);
                        if (r <= 0) {
                            shortr = true;
                            return;
                        }
                        o += (size_t)r;
                    }
                });
                if (shortr) {
                    fclose(f);
                    err = "short read on reference FASTA " + path;
                    return false;
                }
                fseeko(f, sz, SEEK_SET);
            }
        }
        char buf[1 << 16];
        size_t k;
        while ((k = fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + k);  // non-seekable input
        fclose(f);
        std::vector<size_t> hs;
        const char *b = data.data(), *e = b + data.size();
        for (const char *q = b; q < e && (q = (const char *)memchr(q, '>', (size_t)(e - q))); ++q)
            if (q == b || q[-1] == '\n') hs.push_back((size_t)(q - b));
        // names first (serially: the map's entries are made here, the last of a repeated name wins),
        // then the bodies into the entries' strings (their storage reused across loads)
        std::vector<std::string> names(hs.size());
        std::vector<size_t> les(hs.size());
        for (size_t c = 0; c < hs.size(); ++c) {
            const size_t h = hs[c], stop = c + 1 < hs.size() ? hs[c + 1] : data.size();
            size_t le = find_nl(h);
            if (le == std::string::npos || le > stop) le = stop;
            size_t ne = h + 1;
            while (ne < le && data[ne] != ' ' && data[ne] != '\t' && data[ne] != '\r') ++ne;
            names[c].assign(data.data() + h + 1, ne - h - 1);
            les[c] = le;
        }
        std::unordered_map<std::string, size_t> last;
        for (size_t c = 0; c < hs.size(); ++c) last[names[c]] = c;
        for (auto it = seq.begin(); it != seq.end();)  // contigs of an earlier file that this one lacks
            it = last.count(it->first) ? std::next(it) : seq.erase(it);
        std::vector<std::string *> bodies(hs.size(), nullptr);
        for (auto &kv : last) bodies[kv.second] = &seq[kv.first];
        pool.run(hs.size(), [&](size_t c) {
            if (!bodies[c]) return;  // a repeated name: a later entry holds it
            const size_t stop = c + 1 < hs.size() ? hs[c + 1] : data.size(), le = les[c];
            std::string &out = *bodies[c];
            out.clear();
            out.reserve(stop > le ? stop - le : 0);
            size_t p = le + 1;
            while (p < stop) {
                size_t q = find_nl(p);
                if (q == std::string::npos || q > stop) q = stop;
                size_t qe = q;
                if (qe > p && data[qe - 1] == '\r') --qe;
                out.append(data.data() + p, qe - p);
                p = q + 1;
            }
        });
        if (seq.empty()) {
            err = "no sequences in reference FASTA " + path;
            return false;
        }
        return true;
    }
    const std::string *get(const std::string &name) const {
        auto it = seq.find(name);
        return it == seq.end() ? nullptr : &it->second;
    }
};

// The sequences of the contigs `names` (a BAM header's, in refID order) as one arena: contig r lies at
// bytes[off[r], off[r] + len[r]) with a..z upper-cased and every other byte as the file has it; off[r] = -1 and
// len[r] = 0 where the FASTA has no sequence of that name.  Contigs of the FASTA that the list lacks are left out;
// a name listed twice gets its sequence twice.  8 bytes of zero slack follow the last sequence.
struct RefTable {
    std::vector<int64_t> off, len;
    BigVec<uint8_t> bytes;
};

static inline void build_ref_table(const Fasta &fa, const std::vector<std::string> &names, Pool &pool, RefTable &t) {
    const size_t n = names.size();
    t.off.assign(n, -1);
    t.len.assign(n, 0);
    std::vector<const std::string *> seq(n, nullptr);
    uint64_t total = 0;
    for (size_t r = 0; r < n; ++r) {
        seq[r] = fa.get(names[r]);
        if (!seq[r]) continue;
        t.off[r] = (int64_t)total;
        t.len[r] = (int64_t)seq[r]->size();
        total += seq[r]->size();
    }
    t.bytes.clear();
    t.bytes.resize(total + 8);
    memset(t.bytes.data() + total, 0, 8);
    pool.run(n, [&](size_t r) {
        if (!seq[r]) return;
        const char *s = seq[r]->data();
        uint8_t *d = t.bytes.data() + t.off[r];
        for (size_t k = 0, m = seq[r]->size(); k < m; ++k) {
            const uint8_t c = (uint8_t)s[k];
            d[k] = c >= 'a' && c <= 'z' ? (uint8_t)(c - 32) : c;
        }
    });
}

}  // namespace oge
