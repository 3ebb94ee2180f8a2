// file_load.cpp -- a file's bytes into HBM (see file_load.h).
#include "file_load.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <fcntl.h>
#include <sys/stat.h>

#include "modules.h"

namespace oge {

// ----------------------------------------------------------------------------------- the prefetch
// The input read into host memory on helper threads while the process is still bringing up HIP (r06: the CLI
// starts this before oge_ctx_create, ~0.2 s, and the reader then only copies it up).  One file of 64 MiB to
// 8 GiB; OGE_PREFETCH=0 turns it off.
namespace {
struct Prefetch {
    std::string path;
    uint64_t size = 0;
    bytevec data;
    bool ok = false;
    JoinThread th;  // last: joined before the fields its thread fills go
};
std::unique_ptr<Prefetch> g_prefetch;
}  // namespace

void prefetch_input(const std::string &path) {
    const char *e = getenv("OGE_PREFETCH");
    if ((e && *e == '0') || g_prefetch) return;
    struct stat st;
    const char *mn = getenv("OGE_PREFETCH_MIN");  // smallest file prefetched (bytes; tests lower it)
    const long long pmin = mn && *mn ? atoll(mn) : (64ll << 20);
    if (stat(path.c_str(), &st) || !S_ISREG(st.st_mode) || st.st_size < pmin || st.st_size < 1 || st.st_size > (8ll << 30)) return;
    g_prefetch.reset(new Prefetch());
    Prefetch *P = g_prefetch.get();
    P->path = path;
    P->size = (uint64_t)st.st_size;
    P->th = std::thread([P]() {
        const OwnedFd fd(open(P->path.c_str(), O_RDONLY));
        if (fd.fd < 0) return;
        const uint64_t Z = P->size;
        try {
            P->data.reserve(Z + 16);
            want_huge_pages(P->data.data(), Z + 16);
            P->data.resize(Z + 16);  // uninitialised: the reads below fill it
        } catch (const std::bad_alloc &) {
            return;
        }
        memset(P->data.data() + Z, 0, 16);
        P->ok = pread_all(fd.fd, P->data.data(), 0, Z, (Z + 7) / 8, 8);  // 8 threads, equal parts
    });
}

void prefetch_drop() {  // joined and unmapped beside the caller, which goes on to read the file itself
    if (g_prefetch) std::thread([](std::unique_ptr<Prefetch> p) { p.reset(); }, std::move(g_prefetch)).detach();
}

// ----------------------------------------------------------------------------------- the loaders
int range_to_device(oge_ctx *ctx, int fd, uint64_t off, uint64_t len, uint8_t *d_dst, uint64_t chunk, uint64_t slice) {
    if (!len) return 0;
    PinBuf hb[2] = {PinBuf(ctx), PinBuf(ctx)};
    if (hb[0].alloc(chunk) || hb[1].alloc(chunk)) return -1;
    const uint64_t nch = (len + chunk - 1) / chunk;
    const int threads = (int)((chunk + slice - 1) / slice);  // a chunk's slices are all read at once
    std::atomic<bool> bad(false);
    auto read_chunk = [&](uint64_t c) {  // chunk c into hb[c & 1]
        const uint64_t o = c * chunk;
        if (!pread_all(fd, hb[c & 1].as<uint8_t>(), off + o, std::min(len, o + chunk) - o, slice, threads)) bad = true;
    };
    read_chunk(0);
    for (uint64_t c = 0; c < nch && !bad; ++c) {
        JoinThread next;  // joined at the end of every round
        if (c + 1 < nch) next = std::thread(read_chunk, c + 1);
        const uint64_t o = c * chunk;
        if (oge_memcpy(ctx, d_dst + o, hb[c & 1].as<uint8_t>(), std::min(len, o + chunk) - o, 1)) bad = true;
    }
    return bad ? -1 : 0;
}

// The file streamed into HBM through two page-locked buffers, or copied up from the prefetch: no host copy of
// the whole file to allocate, fault in and unmap (a 29 GB file's unmap alone took 1.5 s).
static int stream_file(ChainContext &cc, const std::string &path, LoadedFile &out) {
    std::unique_ptr<Prefetch> pre = std::move(g_prefetch);  // taken below; any other return joins and frees it
    const OwnedFd fd(open(path.c_str(), O_RDONLY));
    if (fd.fd < 0) return 2;
    struct stat stt;
    const char *mn = getenv("OGE_STREAM_MIN");  // smallest file streamed (bytes; tests lower it)
    const long long smin = mn && *mn ? atoll(mn) : (64ll << 20);
    if (fstat(fd.fd, &stt) || !S_ISREG(stt.st_mode) || stt.st_size < smin || stt.st_size < 1) return 2;
    const uint64_t Z = (uint64_t)stt.st_size;
    uint64_t fr = 0, tot = 0;
    if (oge_mem_info(cc.ctx, &fr, &tot) || Z / 10 * 40 > fr) return 2;  // leave the host path to size what follows
    if (pre && pre->path == path) {
        pre->th.join();
        if (pre->ok && pre->size == Z) {  // read while HIP came up: one copy from the helper's buffer
            out.prefetched = true;
            const bool ok = !out.buf.alloc(Z + 16) && !oge_memcpy(cc.ctx, out.buf.as<uint8_t>(), pre->data.data(), Z, 1);
            std::thread([](bytevec v) { v = bytevec(); }, std::move(pre->data)).detach();  // unmapped beside what follows
            if (!ok) return 2;
            out.zbytes = Z;
            return 0;
        }
    }
    pre.reset();
    const uint64_t CH = getenv("OGE_STREAM_MIN") ? (64ull << 10) : (256ull << 20);  // tests: many small chunks
    if (out.buf.alloc(Z + 16) || range_to_device(cc.ctx, fd.fd, 0, Z, out.buf.as<uint8_t>(), CH, 32ull << 20)) return 2;
    out.zbytes = Z;
    return 0;
}

static int whole_file(ChainContext &cc, const std::string &path, LoadedFile &out) {
    auto clk = [] { return std::chrono::steady_clock::now(); };
    bytevec z;
    std::string err;
    const auto t0 = clk();
    if (!read_file_bytes(path, z, cc.threads > 0 ? cc.threads : 8, err)) {
        fprintf(stderr, "openge: %s: %s\n", path.c_str(), err.c_str());
        return -1;
    }
    const auto t1 = clk();
    if (out.buf.alloc(z.size() + 64) || oge_memcpy(cc.ctx, out.buf.as<uint8_t>(), z.data(), z.size(), 1)) return -2;
    out.zbytes = z.size();
    out.t_read = std::chrono::duration<double>(t1 - t0).count();
    out.t_upload = std::chrono::duration<double>(clk() - t1).count();
    return 0;
}

int file_to_device(ChainContext &cc, const std::string &path, LoadPolicy policy, LoadedFile &out) {
    const int rc = policy == LOAD_STREAM ? stream_file(cc, path, out) : whole_file(cc, path, out);
    if (rc) out.buf.reset();
    prefetch_drop();  // (LOAD_WHOLE reads beside a prefetch the CLI started and never takes it)
    return rc;
}

}  // namespace oge
