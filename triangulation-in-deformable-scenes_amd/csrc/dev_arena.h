// dev_arena.h — the per-call device buffers of the map-side entries (triangulation, matching, pixel
// errors, depth sampling, measurements): every piece is declared once, with its pointer and element
// count, and commit() makes the one allocation that holds them all, 256-byte aligned, freed with the
// object.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <vector>

namespace deftri {

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
    // one hipMalloc for every declared piece (a zero-size call still allocates); false: it failed
    bool commit() {
        if (hipMalloc(&base_, total_ ? total_ : 256) != hipSuccess) return false;
        for (const Piece &q : pieces_) q.set(q.slot, base_ + q.off);
        return true;
    }

 private:
    struct Piece {
        void *slot;
        size_t off;
        void (*set)(void *, char *);
    };
    std::vector<Piece> pieces_;
    size_t total_ = 0;
    char *base_ = nullptr;
};

// blocking copy of a host vector into its piece (the measurement calls' uploads)
template <typename T> void upload(T *dst, const std::vector<T> &v) {
    if (!v.empty()) hipMemcpy(dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice);
}

}  // namespace deftri
