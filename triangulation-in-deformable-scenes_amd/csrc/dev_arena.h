// dev_arena.h — the per-call device buffers of the map-side entries (triangulation, matching, pixel
// errors, depth sampling, measurements): every piece is declared once, with its pointer and element
// count, and commit() makes the one allocation that holds them all, 256-byte aligned, freed with the
// object.  An input is declared with in(): its upload has the piece's own size.  Also the two helpers
// every entry ends with: hip_fail and ms_since.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstddef>
#include <string>
#include <vector>

#include "../../include/deftri.h"

namespace deftri {

// "<what>: <the runtime's text>" into err; the entry's return value
inline int hip_fail(std::string &err, const char *what, hipError_t e) {
    err = std::string(what) + ": " + hipGetErrorString(e);
    return DEFTRI_E_HIP;
}

inline double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

class DevArena {
 public:
    DevArena() = default;
    DevArena(const DevArena &) = delete;
    DevArena &operator=(const DevArena &) = delete;
    ~DevArena() { if (base_) hipFree(base_); }
    // declare a piece of `count` T; *p is set by commit()
    template <typename T> void add(T **p, size_t count) {
        pieces_.push_back({p, total_, [](void *slot, char *at) { *(T **)slot = (T *)at; }});
        total_ += (sizeof(T) * count + 255) & ~(size_t)255;
    }
    // a piece that commit(st) fills from `count` T at `host`
    template <typename T> void in(T **p, const void *host, size_t count) {
        uploads_.push_back({total_, host, sizeof(T) * count});
        add(p, count);
    }
    // one hipMalloc for every declared piece (a zero-size call still allocates); false: it failed
    bool commit() {
        if (hipMalloc(&base_, total_ ? total_ : 256) != hipSuccess) return false;
        for (const Piece &q : pieces_) q.set(q.slot, base_ + q.off);
        return true;
    }
    // the same, then the inputs' uploads on `st` in declaration order (an empty one is no call)
    bool commit(hipStream_t st) {
        if (!commit()) return false;
        for (const Upload &u : uploads_)
            if (u.bytes) hipMemcpyAsync(base_ + u.off, u.host, u.bytes, hipMemcpyHostToDevice, st);
        return true;
    }

 private:
    struct Piece {
        void *slot;
        size_t off;
        void (*set)(void *, char *);
    };
    struct Upload {
        size_t off;
        const void *host;
        size_t bytes;
    };
    std::vector<Piece> pieces_;
    std::vector<Upload> uploads_;
    size_t total_ = 0;
    char *base_ = nullptr;
};

// blocking copy of a host vector into its piece (the measurement calls' uploads)
template <typename T> void upload(T *dst, const std::vector<T> &v) {
    if (!v.empty()) hipMemcpy(dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice);
}

}  // namespace deftri
