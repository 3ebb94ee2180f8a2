// dev_buf.h -- owners for the module layer's temporaries: a device or page-locked host buffer of the C ABI
// (include/openge_hip.h), the output FILE and the writer thread.  Host C++ only.  Each frees (closes, joins)
// in its destructor, so a return can leave nothing behind.
#pragma once
#include <cstdint>
#include <cstdio>
#include <thread>
#include <utility>
#include <unistd.h>

#include "../../include/openge_hip.h"

namespace oge {

template <bool Pinned>
class Buf {
public:
    explicit Buf(oge_ctx *c) : c_(c) {}
    Buf(Buf &&o) noexcept : c_(o.c_), p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
    Buf &operator=(Buf &&o) noexcept {
        if (this != &o) {
            reset();
            c_ = o.c_, p_ = o.p_, cap_ = o.cap_;
            o.p_ = nullptr, o.cap_ = 0;
        }
        return *this;
    }
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() { reset(); }
    void reset() {
        if (p_) Pinned ? oge_host_free(c_, p_) : oge_dev_free(c_, p_);
        p_ = nullptr, cap_ = 0;
    }
    int alloc(uint64_t bytes) {  // frees what it held
        reset();
        const int rc = Pinned ? oge_host_alloc(c_, bytes, &p_) : oge_dev_alloc(c_, bytes, &p_);
        if (rc) p_ = nullptr;
        else cap_ = bytes;
        return rc;
    }
    void adopt(void *p, uint64_t bytes) {  // takes a buffer the C ABI handed to its caller; frees what it held
        reset();
        p_ = p, cap_ = bytes;
    }
    int need(uint64_t bytes) { return bytes <= cap_ ? 0 : alloc(bytes); }  // grows only
    template <class T>
    T *as() const { return (T *)p_; }
    void *release() {  // the caller owns it now (a ReadBatch's d_recs / d_offs)
        cap_ = 0;
        return std::exchange(p_, nullptr);
    }
    explicit operator bool() const { return p_ != nullptr; }

private:
    oge_ctx *c_;
    void *p_ = nullptr;
    uint64_t cap_ = 0;
};
using DevBuf = Buf<false>;  // oge_dev_alloc
using PinBuf = Buf<true>;   // oge_host_alloc

// A background thread that is joined before it is replaced or destroyed.  Declare it after the buffers its
// thread reads, so it is joined before they are freed.
struct JoinThread {
    std::thread t;
    void join() {
        if (t.joinable()) t.join();
    }
    void operator=(std::thread &&n) {
        join();
        t = std::move(n);
    }
    ~JoinThread() { join(); }
};

// A file descriptor closed on every return.
struct OwnedFd {
    const int fd;
    explicit OwnedFd(int d) : fd(d) {}
    OwnedFd(const OwnedFd &) = delete;
    ~OwnedFd() {
        if (fd >= 0) ::close(fd);
    }
};

// An output FILE closed on every return; stdout is never closed.
struct OutFile {
    FILE *f = nullptr;
    explicit OutFile(FILE *file) : f(file) {}
    OutFile(const OutFile &) = delete;
    OutFile &operator=(const OutFile &) = delete;
    int close() {  // fclose, or fflush for stdout: != 0 when bytes were lost
        FILE *g = std::exchange(f, nullptr);
        return !g ? 0 : g != stdout ? fclose(g) : fflush(g);
    }
    ~OutFile() { close(); }
};

}  // namespace oge
