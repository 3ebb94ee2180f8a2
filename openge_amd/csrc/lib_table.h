// lib_table.h -- the read-group -> library table of a BAM header, built in one place (bamio.cpp) for the
// library's chains, the C ABI and the CLI.
//
// MarkDuplicates::getLibraryName (algorithms/mark_duplicates.cpp:301-318): the library of a record is the LB of
// its @RG, "Unknown Library" when the LB is absent or empty.  Library ids run from 1 in the order the names
// first appear in the header; which id a name gets changes no duplicate decision, but the metrics
// are summed and named by it.  unknown_lib is the id of "Unknown Library" when an @RG has that name, else the
// next free id.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/openge_hip.h"
#include "bamio.h"

namespace oge {

struct LibTable {
    std::string ids;                 // the @RG ids in header order, back to back, each NUL-terminated
    std::vector<int16_t> rg_lib;     // library id of read group g; n_rg entries and one spare 0
    int32_t n_rg = 0;
    int16_t unknown_lib = 1;
    int32_t n_lib = 2;               // 1 + the largest id in use (rg_lib, unknown_lib): id 0 is never given out
    std::vector<std::string> names;  // by library id, n_lib entries: "" where no @RG names the id

    explicit LibTable(const BamHeaderModel &h);
    // opts() points into the table: it stays where it was built
    LibTable(const LibTable &) = delete;
    LibTable &operator=(const LibTable &) = delete;

    // The dedup options of this table; every other field is zero.  Valid while the table lives.
    oge_markdup_opts opts(int32_t n_ref, int compat_nonverbose_index = 0, int split_chains = 0) const;
};

}  // namespace oge
