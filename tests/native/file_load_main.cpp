// file_load_main.cpp -- TEST INFRASTRUCTURE ONLY: the module layer's loader (csrc/file_load.cpp over bamio's
// pread_all) in one executable for AddressSanitizer / ThreadSanitizer builds, with the six C ABI functions it
// needs defined here over malloc / free / memcpy.  A counter fails the k-th allocation or copy on request.
//   file_load_main FILE        FILE: a few tens of KiB of any bytes
// Checked: the bytes that arrive, a guard region behind them, short files, and that every failing allocation
// or copy fails the call (the sanitizer's leak check then sees what the failure paths free).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <fcntl.h>
#include <unistd.h>

#include "../../openge_amd/csrc/modules.h"

static long g_ops = 0, g_fail_at = 0;  // allocations and copies so far; the one that fails (0 = none)
static long g_live = 0;                // buffers allocated and not yet freed
static int op() { return ++g_ops == g_fail_at ? OGE_ERR_HIP : OGE_OK; }
static int alloc(uint64_t bytes, void **out) {
    *out = nullptr;
    if (op()) return OGE_ERR_HIP;
    *out = malloc(bytes ? bytes : 1);  // exact size: the sanitizer sees a write past it
    ++g_live;
    return OGE_OK;
}
static int release(void *p) {
    free(p);
    --g_live;
    return OGE_OK;
}
extern "C" {
int oge_dev_alloc(oge_ctx *, uint64_t bytes, void **out) { return alloc(bytes, out); }
int oge_host_alloc(oge_ctx *, uint64_t bytes, void **out) { return alloc(bytes, out); }
int oge_dev_free(oge_ctx *, void *p) { return release(p); }
int oge_host_free(oge_ctx *, void *p) { return release(p); }
int oge_memcpy(oge_ctx *, void *dst, const void *src, uint64_t bytes, int) {
    if (op()) return OGE_ERR_HIP;
    memcpy(dst, src, bytes);
    return OGE_OK;
}
int oge_mem_info(oge_ctx *, uint64_t *free_bytes, uint64_t *total_bytes) {
    *free_bytes = *total_bytes = 1ull << 40;
    return OGE_OK;
}
}

static int g_bad = 0;
#define CHECK(cond, ...)                                         \
    do {                                                         \
        if (!(cond)) {                                           \
            fprintf(stderr, "FAILED %s: ", #cond);               \
            fprintf(stderr, __VA_ARGS__), fputc('\n', stderr);   \
            ++g_bad;                                             \
        }                                                        \
    } while (0)

static const uint64_t kChunk = 4096, kSlice = 1024, kGuard = 64;

// one call into a buffer of len + kGuard bytes (the guard must stay) or, exact, of len bytes (the sanitizer's)
template <class F>
static int into(uint64_t len, bool exact, const uint8_t *want, const char *what, uint64_t off, F call) {
    std::vector<uint8_t> dst(len + (exact ? 0 : kGuard), 0xA5);
    const int rc = call(dst.data());
    if (rc || !want) return rc;
    CHECK(!len || !memcmp(dst.data(), want, len), "%s off %llu len %llu: bytes differ", what, (unsigned long long)off, (unsigned long long)len);
    for (uint64_t i = len; i < dst.size(); ++i) CHECK(dst[i] == 0xA5, "%s off %llu len %llu: guard byte %llu written", what,
                                                      (unsigned long long)off, (unsigned long long)len, (unsigned long long)(i - len));
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) return fprintf(stderr, "usage: file_load_main FILE\n"), 2;
    const std::string path = argv[1];
    std::vector<uint8_t> ref;
    {
        FILE *f = fopen(path.c_str(), "rb");
        if (!f) return perror(argv[1]), 2;
        uint8_t buf[4096];
        for (size_t r; (r = fread(buf, 1, sizeof buf, f)) > 0;) ref.insert(ref.end(), buf, buf + r);
        fclose(f);
    }
    const uint64_t F = ref.size();
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) return perror(argv[1]), 2;
    long checks = 0;

    // the whole file through file_to_device first (its prefetched path unmaps on a detached thread, which has
    // long ended when the process does): prefetched, streamed in 64 KiB chunks, whole
    setenv("OGE_PREFETCH_MIN", "1", 1);
    setenv("OGE_STREAM_MIN", "1", 1);
    oge::ChainContext cc;
    cc.threads = 4;
    for (int mode = 0; mode < 3; ++mode) {
        const oge::LoadPolicy pol = mode < 2 ? oge::LOAD_STREAM : oge::LOAD_WHOLE;
        long ops = 0;
        for (long k = 0; k == 0 || k <= ops; ++k) {  // k = 0: nothing fails; then every allocation and copy in turn
            if (mode == 0) oge::prefetch_input(path);
            g_ops = 0, g_fail_at = k;
            {
                oge::LoadedFile z(cc.ctx);
                const int rc = oge::file_to_device(cc, path, pol, z);
                if (k == 0) {
                    ops = g_ops;
                    CHECK(rc == 0 && z.zbytes == F && z.prefetched == (mode == 0), "file_to_device mode %d: rc %d", mode, rc);
                    CHECK(rc || !memcmp(z.buf.as<uint8_t>(), ref.data(), F), "file_to_device mode %d: bytes differ", mode);
                } else {
                    CHECK(rc == (pol == oge::LOAD_STREAM ? 2 : -2) && !z.buf, "file_to_device mode %d, failing op %ld of %ld: rc %d", mode, k, ops, rc);
                }
            }
            CHECK(g_live == 0, "file_to_device mode %d, failing op %ld: %ld buffers left", mode, k, g_live);
            ++checks;
        }
        CHECK(ops >= 2, "file_to_device mode %d: %ld operations", mode, ops);
    }
    g_fail_at = 0;
    oge::prefetch_input(path);  // never taken: dropped
    oge::prefetch_drop();

    const uint64_t lens[] = {0, 1, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 8193, 3 * 4096 + 1025}, offs[] = {0, 1, 4097};
    for (uint64_t off : offs)
        for (uint64_t len : lens) {
            if (off + len > F) return fprintf(stderr, "%s is too short\n", argv[1]), 2;
            const uint8_t *want = ref.data() + off;
            for (bool exact : {false, true}) {
                g_fail_at = 0;
                CHECK(into(len, exact, want, "pread_all", off, [&](uint8_t *d) { return oge::pread_all(fd, d, off, len, kSlice, 4) ? 0 : -1; }) == 0,
                      "pread_all off %llu len %llu", (unsigned long long)off, (unsigned long long)len);
                g_ops = 0;
                CHECK(into(len, exact, want, "range_to_device", off,
                           [&](uint8_t *d) { return oge::range_to_device(nullptr, fd, off, len, d, kChunk, kSlice); }) == 0,
                      "range_to_device off %llu len %llu", (unsigned long long)off, (unsigned long long)len);
                checks += 2;
            }
            // two page-locked buffers and one copy per chunk: each of them failing fails the call
            const long ops = g_ops;
            CHECK(ops == (len ? 2 + (long)((len + kChunk - 1) / kChunk) : 0), "range_to_device len %llu: %ld operations", (unsigned long long)len, ops);
            for (long k = 1; k <= ops; ++k, ++checks) {
                g_ops = 0, g_fail_at = k;
                CHECK(into(len, true, nullptr, "", off, [&](uint8_t *d) { return oge::range_to_device(nullptr, fd, off, len, d, kChunk, kSlice); }) == -1,
                      "range_to_device off %llu len %llu with failing op %ld of %ld succeeded", (unsigned long long)off, (unsigned long long)len, k, ops);
                CHECK(g_live == 0, "range_to_device failing op %ld: %ld buffers left", k, g_live);
            }
        }
    g_fail_at = 0;

    // a file that ends before off + len: failure, in the first chunk, in a later one, and from past the end
    for (uint64_t off : {F - 100, F - kChunk - 100, F + 10}) {
        const uint64_t len = 2 * kChunk + 50;
        CHECK(into(len, false, nullptr, "", off, [&](uint8_t *d) { return oge::pread_all(fd, d, off, len, kSlice, 4) ? 0 : -1; }) == -1,
              "pread_all past the end of the file succeeded (off %llu)", (unsigned long long)off);
        CHECK(into(len, false, nullptr, "", off, [&](uint8_t *d) { return oge::range_to_device(nullptr, fd, off, len, d, kChunk, kSlice); }) == -1,
              "range_to_device past the end of the file succeeded (off %llu)", (unsigned long long)off);
        CHECK(g_live == 0, "short file: %ld buffers left", g_live);
        checks += 2;
    }
    close(fd);
    if (g_bad) return fprintf(stderr, "%d checks failed\n", g_bad), 1;
    printf("ok %ld\n", checks);
    return 0;
}
