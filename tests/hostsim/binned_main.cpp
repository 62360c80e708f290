/*
 * binned_main.cpp -- TEST ONLY.  The rule of the binned regional term (medpy_amd/csrc/mgc_binned.h) as a stand-alone program, so
 * that the very lines the kernels compile can be compared with NumPy on the CPU, and built with -fsanitize=address,undefined.
 *
 *   binned_main bins <dtype> <nbins> <lo> <width> <values.bin> <bins.bin>
 *       reads raw values of <dtype> (u8 i8 u16 i16 u32 i32 u64 i64 f32 f64), converts each to double as the library does and
 *       writes its bin as int64
 *   binned_main check <nbins> <lo> <width> <source.bin | -> <sink.bin | ->
 *       runs the argument and table check on two raw f64 tables of nbins entries ("-": NULL) and prints
 *       "OK" or "INVALID <which> <bad> <message>"
 *
 * lo and width are read with strtod (hexadecimal floats are exact).  Exit status 0 unless the arguments or files are unusable.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../medpy_amd/csrc/mgc_binned.h"

static bool read_file(const char* path, std::vector<char>* out)
{
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    out->resize((size_t)(n > 0 ? n : 0));
    const bool ok = n <= 0 || fread(out->data(), 1, (size_t)n, f) == (size_t)n;
    fclose(f);
    return ok;
}

template <class T>
static void bins_of(const std::vector<char>& raw, double lo, double width, int64_t nbins, std::vector<int64_t>* out)
{
    const size_t n = raw.size() / sizeof(T);
    out->resize(n);
    for (size_t i = 0; i < n; ++i) {
        T v;
        memcpy(&v, raw.data() + i * sizeof(T), sizeof(T));
        (*out)[i] = mgc_binned_bin((double)v, lo, width, nbins);
    }
}

int main(int argc, char** argv)
{
    if (argc == 8 && !strcmp(argv[1], "bins")) {
        const std::string dt = argv[2];
        const int64_t nbins = strtoll(argv[3], nullptr, 10);
        const double lo = strtod(argv[4], nullptr), width = strtod(argv[5], nullptr);
        char msg[256] = "";
        if (mgc_binned_check_binning(nbins, lo, width, msg, sizeof(msg)) != MGC_BINNED_OK) { fprintf(stderr, "%s\n", msg); return 2; }
        std::vector<char> raw;
        if (!read_file(argv[6], &raw)) { fprintf(stderr, "cannot read %s\n", argv[6]); return 2; }
        std::vector<int64_t> bins;
        if (dt == "u8") bins_of<uint8_t>(raw, lo, width, nbins, &bins);
        else if (dt == "i8") bins_of<int8_t>(raw, lo, width, nbins, &bins);
        else if (dt == "u16") bins_of<uint16_t>(raw, lo, width, nbins, &bins);
        else if (dt == "i16") bins_of<int16_t>(raw, lo, width, nbins, &bins);
        else if (dt == "u32") bins_of<uint32_t>(raw, lo, width, nbins, &bins);
        else if (dt == "i32") bins_of<int32_t>(raw, lo, width, nbins, &bins);
        else if (dt == "u64") bins_of<uint64_t>(raw, lo, width, nbins, &bins);
        else if (dt == "i64") bins_of<int64_t>(raw, lo, width, nbins, &bins);
        else if (dt == "f32") bins_of<float>(raw, lo, width, nbins, &bins);
        else if (dt == "f64") bins_of<double>(raw, lo, width, nbins, &bins);
        else { fprintf(stderr, "unknown dtype %s\n", dt.c_str()); return 2; }
        FILE* f = fopen(argv[7], "wb");
        if (!f || (bins.size() && fwrite(bins.data(), sizeof(int64_t), bins.size(), f) != bins.size())) { fprintf(stderr, "cannot write %s\n", argv[7]); return 2; }
        fclose(f);
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "check")) {
        const int64_t nbins = strtoll(argv[2], nullptr, 10);
        const double lo = strtod(argv[3], nullptr), width = strtod(argv[4], nullptr);
        std::vector<char> raw[2];
        const double* table[2] = {nullptr, nullptr};
        for (int k = 0; k < 2; ++k) {
            if (!strcmp(argv[5 + k], "-")) continue;
            if (!read_file(argv[5 + k], &raw[k])) { fprintf(stderr, "cannot read %s\n", argv[5 + k]); return 2; }
            if (nbins > 0 && raw[k].size() != (size_t)nbins * sizeof(double)) { fprintf(stderr, "%s does not hold %lld doubles\n", argv[5 + k], (long long)nbins); return 2; }
            table[k] = (const double*)raw[k].data();
        }
        char msg[256] = "";
        int which = -1;
        int64_t bad = -2;
        const int rc = mgc_binned_check(nbins, lo, width, table[0], table[1], &which, &bad, msg, sizeof(msg));
        if (rc == MGC_BINNED_OK) printf("OK\n");
        else printf("INVALID %d %lld %s\n", which, (long long)bad, msg);
        return 0;
    }
    fprintf(stderr, "usage: binned_main bins <dtype> <nbins> <lo> <width> <values.bin> <bins.bin> | check <nbins> <lo> <width> <source.bin|-> <sink.bin|->\n");
    return 2;
}
