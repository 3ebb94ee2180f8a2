// rg_lookup.h -- the library of a record on the device: the RG tag found as the input pass of records.hip finds it
// (FindTag semantics, util/bamtools/BamAlignment.cpp:270-294,699-780) and looked up in the uploaded read-group
// table.  Used by dupmetrics.hip and dupsets.hip.  The input pass keeps its own copy: there the walk reads through the LDS tile or
// global memory by a reader type and feeds the pair hash from the words it loads, and replacing it with this
// function changes the registers k_input_pass uses, on the benchmark's headline path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bam_layout.h"
#include "dev_util.h"
#include "records.h"

// The library id of the record at r (block_size in [32, OGE_MAX_BLOCK_SIZE]; the arena carries 16 bytes of slack).
//   walk    from the end of QUAL: the first tag named RG, of whatever type byte, gives the bytes up to the next NUL or
//           the record's end.  The walk ends without one at a type byte of 0, an unknown type, a B array whose header
//           does not fit, whose subtype is unknown or whose count is negative (the input pass would step backwards
//           there), and when the next tag would start at or past the record's end or with a NUL.
//   lookup  a non-empty value equal to the id of group g gives rg.lib[g] (the first such g); no tag, an empty value
//           or an unlisted one gives rg.unknown_lib.
//
// oge_rg_index gives the index g itself, or -1 without a listed value (dupsets.hip: two pairs are optical
// duplicates of one another only within one read group); oge_rg_library is rg.lib of it.
__device__ __forceinline__ int32_t oge_rg_index(const uint8_t *__restrict__ r, uint32_t bs, const OgeRgTable &rg) {
    const uint32_t w3 = oge_ldu32(r + OGE_OFF_LNAME), w4 = oge_ldu32(r + OGE_OFF_NCIGAR);
    const uint64_t lname = w3 & 0xFF, nc = w4 & 0xFFFF, lseq = oge_ldu32(r + OGE_OFF_LSEQ);
    const uint64_t tend = 4ull + bs;
    uint64_t p = OGE_OFF_NAME + lname + 4 * nc + (lseq + 1) / 2 + lseq;
    uint64_t rgv = 0;
    uint32_t rgl = 0;
    while (p + 3 <= tend) {
        const uint32_t w = oge_ldu32(r + p);
        const uint32_t t0 = w & 0xff, t1 = (w >> 8) & 0xff, type = (w >> 16) & 0xff;
        p += 3;
        if (t0 == 'R' && t1 == 'G') {
            uint64_t s = p;
            while (s < tend && r[s]) ++s;
            rgv = p;
            rgl = (uint32_t)(s - p);
            break;
        }
        if (type == 0) break;
        bool ok = true;
        switch (type) {
        case 'A': case 'c': case 'C': p += 1; break;
        case 's': case 'S': p += 2; break;
        case 'f': case 'i': case 'I': p += 4; break;
        case 'Z': case 'H':
            while (p < tend && r[p]) ++p;
            ++p;
            break;
        case 'B': {
            if (p + 5 > tend) { ok = false; break; }
            const uint32_t at = r[p];
            const int32_t cnt = (int32_t)oge_ldu32(r + p + 1);
            p += 5;
            const uint32_t sz = (at == 'c' || at == 'C') ? 1 : (at == 's' || at == 'S') ? 2 : (at == 'f' || at == 'i' || at == 'I') ? 4 : 0;
            if (!sz || cnt < 0) { ok = false; break; }
            p += (uint64_t)cnt * sz;
            break;
        }
        default: ok = false;
        }
        if (!ok || p >= tend || r[p] == 0) break;
    }
    if (!rgl) return -1;
    // a value of <= 15 bytes as four zero-padded words, compared with the table's idw
    uint32_t rv[4] = {0u, 0u, 0u, 0u};
    if (rgl <= 15) {
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            if (4 * q >= rgl) continue;
            uint32_t v = 0;
            if (rgv + 4 * q + 4 <= tend) {
                v = oge_ldu32(r + rgv + 4 * q);
            } else {
                for (uint32_t k = 0; 4 * q + k < rgl; ++k) v |= (uint32_t)r[rgv + 4 * q + k] << (8 * k);
            }
            const uint32_t rem = rgl - 4 * q;
            rv[q] = rem < 4 ? v & ((1u << (8 * rem)) - 1u) : v;
        }
    }
    for (int32_t g = 0; g < rg.n_rg; ++g) {
        const uint32_t o = rg.off[g], Lg = rg.off[g + 1] - o - 1;
        if (Lg != rgl) continue;
        bool eq = true;
        if (Lg <= 15) {
            const uint4 w = rg.idw[g];
            eq = w.x == rv[0] && w.y == rv[1] && w.z == rv[2] && w.w == rv[3];
        } else {
            for (uint32_t y = 0; y < Lg && eq; ++y) eq = rg.ids[o + y] == r[rgv + y];
        }
        if (eq) return g;
    }
    return -1;
}

__device__ __forceinline__ int32_t oge_rg_library(const uint8_t *__restrict__ r, uint32_t bs, const OgeRgTable &rg) {
    const int32_t g = oge_rg_index(r, bs, rg);
    return g < 0 ? rg.unknown_lib : rg.lib[g];
}
