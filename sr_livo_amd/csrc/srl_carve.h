// srl_carve.h -- internal: how the camera stage's owners lay out a block of memory, and the strided copy of a caller's image.  Nothing of
// HIP in here: tests/carve_main.cpp compiles it as plain C++.
#pragma once
#include <cstddef>
#include <cstring>

// A bump layout over one block.  An owner writes its layout once, as a function that takes its pointers from a carve; run over a null
// base the function only measures (every pointer null, `at` the size), run over the block it assigns.  Every piece starts 256-byte
// aligned in a block that is: the kernels reinterpret these pointers as uint4, uint2, short2 and float2.
struct SrlCarve {
    char *base = nullptr;
    size_t at = 0;
    template <class T> T *take(size_t count) {
        T *p = base ? reinterpret_cast<T *>(base + at) : nullptr;
        at += (count * sizeof(T) + 255) / 256 * 256;
        return p;
    }
};

// rows x row_bytes out of a source whose rows lie stride bytes apart, packed.  Exactly row_bytes of every source row are read, also of
// the last: a caller's buffer may end there.
inline void srl_pack_rows(void *dst, const void *src, size_t rows, size_t row_bytes, size_t stride) {
    if (stride == row_bytes) { std::memcpy(dst, src, rows * row_bytes); return; }
    for (size_t r = 0; r < rows; r++) std::memcpy((char *)dst + r * row_bytes, (const char *)src + r * stride, row_bytes);
}
