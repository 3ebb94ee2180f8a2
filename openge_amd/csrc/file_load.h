// file_load.h -- a file's bytes into HBM, for every reader of the module layer.  Host C++ over the C ABI
// (device and page-locked buffers, oge_memcpy, oge_mem_info) and bamio's parallel reads; a translation unit of
// its own, so a host check can link it without the modules.
#pragma once
#include <cstdint>
#include <string>

#include "dev_buf.h"

namespace oge {

struct ChainContext;

// Start reading the chain's input file into host memory on helper threads (the CLI calls this before it
// brings up HIP); file_to_device takes the bytes when it streams that file.  prefetch_drop joins the helper
// and frees the bytes (on a side thread, so the caller does not wait for a read it will not use): the readers
// that do not take them call it.
void prefetch_input(const std::string &path);
void prefetch_drop();

// Bytes [off, off + len) of the open file into device memory d_dst: chunk c + 1 is read (parallel preads of
// `slice` bytes) into one of two page-locked buffers of `chunk` bytes while chunk c is copied up from the
// other.  0 = ok, -1 = an allocation, a read or a copy failed.
int range_to_device(oge_ctx *ctx, int fd, uint64_t off, uint64_t len, uint8_t *d_dst, uint64_t chunk, uint64_t slice);

enum LoadPolicy {
    LOAD_STREAM,  // the chain reader: the prefetched bytes when they are this file's, else range_to_device
    LOAD_WHOLE,   // index / stats / count / coverage: read_file_bytes, then one copy up
};
struct LoadedFile {
    DevBuf buf;           // the file's bytes (LOAD_STREAM: + 16 bytes of slack, LOAD_WHOLE: + 64)
    uint64_t zbytes = 0;
    bool prefetched = false;
    double t_read = 0, t_upload = 0;  // LOAD_WHOLE (seconds)
    explicit LoadedFile(oge_ctx *c) : buf(c) {}
};
// 0 = ok.  LOAD_STREAM: 2 when it does not apply (a small file, an input close to the HBM size, a failed read
// or allocation): the caller takes the host path.  LOAD_WHOLE: -1 when the file cannot be read (reported),
// -2 when the allocation or the copy failed (oge_last_error says why).
int file_to_device(ChainContext &cc, const std::string &path, LoadPolicy policy, LoadedFile &out);

}  // namespace oge
