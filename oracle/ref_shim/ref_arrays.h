// ref_arrays.h -- the array container the programs of oracle/_ref read their cases from and write their results to, as
// ref_tracker.cpp documents it (that file keeps its own copy, so that its program does not change with this header):
// little endian, char magic[8] = "PAGKARR1"; int32 count; then count arrays, each
//   char name[24] (zero padded); int32 dtype (0 uint8, 1 int32, 2 float32, 3 float64); int32 ndim (<= 3); int32 dims[3];
//   the elements, row-major.
// TEST INFRASTRUCTURE.  tests/reference_cases.py holds the Python side (write_arrays, read_arrays).
#ifndef PAGK_REF_ARRAYS_H
#define PAGK_REF_ARRAYS_H

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace ref_arrays {

struct Array {
    int32_t dtype = 0, ndim = 0, dims[3] = {1, 1, 1};
    std::vector<uint8_t> bytes;
    size_t count() const { return (size_t)dims[0] * (size_t)dims[1] * (size_t)dims[2]; }
    template <typename T> const T *as() const { return reinterpret_cast<const T *>(bytes.data()); }
};
const size_t ELEM[4] = {1, 4, 4, 8};
typedef std::map<std::string, Array> Arrays;

inline bool read_arrays(const char *path, Arrays &out)
{
    FILE *f = fopen(path, "rb");
    char magic[8];
    int32_t count = 0;
    bool ok = f && fread(magic, 1, 8, f) == 8 && memcmp(magic, "PAGKARR1", 8) == 0 && fread(&count, 4, 1, f) == 1;
    for (int32_t k = 0; ok && k < count; k++) {
        char name[25] = {0};
        Array a;
        ok = fread(name, 1, 24, f) == 24 && fread(&a.dtype, 4, 1, f) == 1 && fread(&a.ndim, 4, 1, f) == 1 && fread(a.dims, 4, 3, f) == 3 &&
             a.dtype >= 0 && a.dtype <= 3 && a.ndim >= 0 && a.ndim <= 3 && a.dims[0] >= 0 && a.dims[1] >= 0 && a.dims[2] >= 0;
        if (!ok) break;
        a.bytes.resize(a.count() * ELEM[a.dtype]);
        ok = a.bytes.empty() || fread(a.bytes.data(), 1, a.bytes.size(), f) == a.bytes.size();
        out[name] = a;
    }
    if (f) fclose(f);
    return ok;
}

struct Writer {
    FILE *f;
    int32_t count = 0;
    explicit Writer(const char *path) : f(fopen(path, "wb"))
    {
        if (f) fwrite("PAGKARR1", 1, 8, f), fwrite(&count, 4, 1, f);
    }
    void put(const char *name, int32_t dtype, int32_t ndim, int32_t d0, int32_t d1, int32_t d2, const void *data)
    {
        char nm[24] = {0};
        strncpy(nm, name, 23);
        const int32_t dims[3] = {d0, d1, d2};
        fwrite(nm, 1, 24, f), fwrite(&dtype, 4, 1, f), fwrite(&ndim, 4, 1, f), fwrite(dims, 4, 3, f);
        const size_t n = (size_t)d0 * (size_t)d1 * (size_t)d2 * ELEM[dtype];
        if (n) fwrite(data, 1, n, f);
        count++;
    }
    void i32(const char *name, const std::vector<int32_t> &v, int32_t cols = 0)
    {
        if (cols) put(name, 1, 2, (int32_t)(v.size() / cols), cols, 1, v.data());
        else put(name, 1, 1, (int32_t)v.size(), 1, 1, v.data());
    }
    void f32(const char *name, const std::vector<float> &v, int32_t cols = 0)
    {
        if (cols) put(name, 2, 2, (int32_t)(v.size() / cols), cols, 1, v.data());
        else put(name, 2, 1, (int32_t)v.size(), 1, 1, v.data());
    }
    int close()
    {
        if (fseek(f, 8, SEEK_SET) != 0 || fwrite(&count, 4, 1, f) != 1) return 5;
        return fclose(f) == 0 ? 0 : 5;
    }
};

}   // namespace ref_arrays

#endif
