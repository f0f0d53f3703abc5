// dev_arena.h — one device allocation carved into 256-byte aligned pieces, freed with the object (the
// per-call buffers of the triangulation and matching entries).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace deftri {

struct DevArena {
    char *base = nullptr;
    size_t used = 0, cap = 0;
    ~DevArena() { if (base) hipFree(base); }
    static size_t pad(size_t b) { return (b + 255) & ~(size_t)255; }
    bool reserve(size_t bytes) { cap = bytes; return hipMalloc(&base, bytes ? bytes : 256) == hipSuccess; }
    template <typename T> T *take(size_t count) {
        T *p = (T *)(base + used);
        used += pad(sizeof(T) * count);
        return p;
    }
};

}  // namespace deftri
