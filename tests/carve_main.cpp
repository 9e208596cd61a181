// carve_main.cpp -- a stand-alone program over sr_livo_amd/csrc/srl_carve.h compiled as plain C++ (the header includes nothing of HIP):
// tests/test_carve.py builds it with the host compiler, once plain and once with -fsanitize=address,undefined, and runs it.  It checks
// itself: every failed check prints a line and the exit status is 1; the last line counts the cases.
//   carve      a layout of three pieces per (element size, count) pair, run over a null base and over a block of the measured size:
//              the totals agree, every piece is 256-aligned, consecutive pieces do not overlap, the last ends at or before the total
//   pack_rows  the source is a heap block of exactly (rows - 1) stride + row_bytes bytes and the destination one of rows x row_bytes,
//              so a read of a full stride on the last row, or a write past the packed image, is an AddressSanitizer error
// No device call and nothing of Python in the process.
#include "../sr_livo_amd/csrc/srl_carve.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

struct E12 { char b[12]; };
static const size_t BYTES[] = {0, 1, 255, 256, 257};

// three pieces of na, nb and nc elements of T; the pieces' addresses relative to the base (valid when base is not null)
template <class T>
static size_t layout(char *base, size_t na, size_t nb, size_t nc, T *out[3]) {
    SrlCarve c{base};
    out[0] = c.take<T>(na);
    out[1] = c.take<T>(nb);
    out[2] = c.take<T>(nc);
    return c.at;
}

template <class T>
static int carve_cases() {
    int cases = 0;
    for (size_t ba : BYTES)
        for (size_t bb : BYTES)
            for (size_t bc : BYTES) {
                // "bytes' worth": the fewest elements that cover that many bytes
                const size_t n[3] = {(ba + sizeof(T) - 1) / sizeof(T), (bb + sizeof(T) - 1) / sizeof(T), (bc + sizeof(T) - 1) / sizeof(T)};
                T *p[3];
                const size_t measured = layout<T>(nullptr, n[0], n[1], n[2], p);
                CHECK(p[0] == nullptr && p[1] == nullptr && p[2] == nullptr, "a null base gives null pieces (size %zu)", sizeof(T));
                char *block = (char *)std::aligned_alloc(256, measured ? measured : 256);
                const size_t assigned = layout<T>(block, n[0], n[1], n[2], p);
                CHECK(assigned == measured, "size %zu counts %zu %zu %zu: %zu != %zu", sizeof(T), n[0], n[1], n[2], assigned, measured);
                size_t end = 0;
                for (int k = 0; k < 3; k++) {
                    const size_t at = (size_t)((char *)p[k] - block);
                    CHECK(((uintptr_t)p[k] & 255) == 0, "piece %d of size %zu counts %zu %zu %zu at %zu", k, sizeof(T), n[0], n[1], n[2], at);
                    CHECK(at >= end, "piece %d at %zu begins before %zu", k, at, end);
                    end = at + n[k] * sizeof(T);
                    for (size_t i = 0; i < n[k] * sizeof(T); i++) ((char *)p[k])[i] = (char)(k + 1);      // inside the block, or ASan says so
                }
                CHECK(end <= measured, "the last piece ends at %zu, the total is %zu", end, measured);
                for (int k = 0; k < 3; k++)
                    for (size_t i = 0; i < n[k] * sizeof(T); i++)
                        if (((char *)p[k])[i] != (char)(k + 1)) { CHECK(false, "piece %d was written over", k); break; }
                std::free(block);
                cases++;
            }
    return cases;
}

static int pack_cases() {
    int cases = 0;
    const size_t ROWS[] = {1, 2, 5}, ROW_BYTES[] = {1, 3, 7}, EXTRA[] = {0, 1, 13};
    for (size_t rows : ROWS)
        for (size_t row_bytes : ROW_BYTES)
            for (size_t extra : EXTRA) {
                const size_t stride = row_bytes + extra, src_bytes = (rows - 1) * stride + row_bytes;
                unsigned char *src = (unsigned char *)std::malloc(src_bytes), *dst = (unsigned char *)std::malloc(rows * row_bytes);
                for (size_t i = 0; i < src_bytes; i++) src[i] = (unsigned char)(i * 37 + 11);
                srl_pack_rows(dst, src, rows, row_bytes, stride);
                for (size_t r = 0; r < rows; r++)
                    for (size_t b = 0; b < row_bytes; b++)
                        CHECK(dst[r * row_bytes + b] == src[r * stride + b], "rows %zu row_bytes %zu stride %zu at (%zu, %zu)", rows, row_bytes, stride, r, b);
                std::free(src);
                std::free(dst);
                cases++;
            }
    return cases;
}

int main() {
    const int carve = carve_cases<char>() + carve_cases<float>() + carve_cases<double>() + carve_cases<E12>();
    const int pack = pack_cases();
    std::printf("carve: %d layouts, %d packed images, %d failures\n", carve, pack, failures);
    return failures ? 1 : 0;
}
