/*
 * label_hist_main.cpp -- TEST ONLY.  The run merging of mgc_label_histograms (medpy_amd/csrc/mgc_label_hist.h) as a stand-alone
 * program, so that the very lines k_label_hist compiles can be checked on the CPU, and built with -fsanitize=address,undefined.
 *
 *   label_hist_main <nbins> <labels.bin> <bins.bin> <out.bin>
 *       reads n label bytes and n int64 bins (0 <= bin < nbins), walks the volume as the kernel does -- groups of MGC_LH_GROUP
 *       consecutive voxels, the last one cut short by the end of the volume -- and counts every group through mgc_label_hist_runs
 *       into two histograms.  Writes int64: the 2 * nbins merged counts (fg first), the 2 * nbins counts of a plain per-voxel
 *       loop, the number of adds the merged path made, and the number of groups in which the runs' lengths did not sum to the
 *       group's size or a run was not maximal (must be 0).
 *
 * Exit status 0 unless the arguments or files are unusable.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../medpy_amd/csrc/mgc_label_hist.h"

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

int main(int argc, char** argv)
{
    if (argc != 5) {
        fprintf(stderr, "usage: label_hist_main <nbins> <labels.bin> <bins.bin> <out.bin>\n");
        return 2;
    }
    const int64_t nbins = strtoll(argv[1], nullptr, 10);
    std::vector<char> labels, raw;
    if (nbins < 1 || nbins > 65536 || !read_file(argv[2], &labels) || !read_file(argv[3], &raw) || raw.size() != labels.size() * sizeof(int64_t)) {
        fprintf(stderr, "unusable arguments or files\n");
        return 2;
    }
    const int64_t n = (int64_t)labels.size();
    std::vector<int64_t> bins((size_t)n);
    if (n) memcpy(bins.data(), raw.data(), raw.size());
    for (int64_t b : bins)
        if (b < 0 || b >= nbins) { fprintf(stderr, "bin %lld outside [0, %lld)\n", (long long)b, (long long)nbins); return 2; }
    std::vector<int64_t> out((size_t)(4 * nbins) + 2, 0);
    int64_t* const merged = out.data();
    int64_t* const plain = out.data() + 2 * nbins;
    int64_t adds = 0, bad_groups = 0;
    for (int64_t base = 0; base < n; base += MGC_LH_GROUP) {
        const int count = (int)(n - base < MGC_LH_GROUP ? n - base : MGC_LH_GROUP);
        uint32_t key[MGC_LH_GROUP];
        for (int i = 0; i < MGC_LH_GROUP; ++i) key[i] = i < count ? mgc_label_hist_key(labels[(size_t)(base + i)] != 0, bins[(size_t)(base + i)], nbins) : 0u;
        int64_t total = 0;
        bool first = true, maximal = true;
        uint32_t last = 0u;
        mgc_label_hist_runs(key, count, [&](uint32_t k, uint32_t run) {
            merged[k] += run;
            total += run;
            ++adds;
            if (!first && k == last) maximal = false; /* two runs of one key in a row: they should have been one */
            first = false;
            last = k;
        });
        if (total != count || !maximal) ++bad_groups;
    }
    for (int64_t i = 0; i < n; ++i) plain[mgc_label_hist_key(labels[(size_t)i] != 0, bins[(size_t)i], nbins)] += 1;
    out[(size_t)(4 * nbins)] = adds;
    out[(size_t)(4 * nbins) + 1] = bad_groups;
    FILE* f = fopen(argv[4], "wb");
    if (!f || fwrite(out.data(), sizeof(int64_t), out.size(), f) != out.size()) { fprintf(stderr, "cannot write %s\n", argv[4]); return 2; }
    fclose(f);
    return 0;
}
