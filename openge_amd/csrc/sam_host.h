// sam_host.h -- the host formatter of one record's text (sam_host.cpp): the lines the device leaves out.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/openge_hip.h"

// Appends the record's SAM line (or FASTQ entry) to `out`.  Every tag type of the SAM specification is
// rendered: f as printf("%g"), B as XX:B:t,v,v.  false with `err` set: the record or a tag does not parse.
bool oge_text_line_host(const uint8_t *rec, uint64_t rec_bytes, const oge_text_opts *o, std::string &out, std::string &err);
