/*
 * geo_main.cpp -- TEST ONLY.  The steps of mgc_geodesic_distance (medpy_amd/csrc/mgc_geo.h) as a stand-alone program with one worker,
 * so that the very lines the kernels compile can be checked on the CPU, and built with -fsanitize=address,undefined.  The schedule is
 * the library's: mgc_geo_init_voxel over the voxels, then rounds of tile visits over two work lists swapped, until a round wakes
 * nobody.  The tiles of a round are visited in a seeded random order; the shared arrays of a visit and the plane arrive filled with
 * garbage.
 *
 *   geo_main <dz> <dy> <dx> <full> <gamma> <step> <sz> <sy> <sx> <order seed> <image.bin | -> <seeds.bin> <out.bin>
 *       image.bin: nvox doubles ("-": no image, gamma must be 0); seeds.bin: nvox bytes; out.bin: nvox doubles, then as doubles the
 *       seeds, rounds, tile visits, sweeps summed, visits that ended at the cap, voxels with a finite distance
 *
 * Built with -DGEO_NO_DIAGONAL_WAKE edge and corner neighbours are not woken, with -DGEO_NO_SELF_WAKE a visit that ends at the sweep cap does not
 * wake its own tile: the doctored stand-ins the cases must reject.  Exit status 0 unless the arguments or files are unusable; 3 when
 * the rounds did not end within their bound.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "../../medpy_amd/csrc/mgc_geo.h"

#if defined(GEO_NO_DIAGONAL_WAKE)
#define GEO_DOCTOR_DIAGONAL MGC_GEO_NO_DIAGONAL_WAKE
#else
#define GEO_DOCTOR_DIAGONAL 0
#endif
#if defined(GEO_NO_SELF_WAKE)
#define GEO_DOCTOR_SELF MGC_GEO_NO_SELF_WAKE
#else
#define GEO_DOCTOR_SELF 0
#endif
#define GEO_DOCTOR (GEO_DOCTOR_DIAGONAL | GEO_DOCTOR_SELF)

template <class T>
static bool read_file(const char* path, std::vector<T>* out, size_t want)
{
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    out->resize(want + 1);
    const size_t n = fread(out->data(), sizeof(T), want + 1, f);
    fclose(f);
    out->resize(want);
    return n == want;
}

static bool write_file(const char* path, const std::vector<double>& out)
{
    FILE* f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
    fclose(f);
    return ok;
}

static double garbage()
{
    double g;
    memset(&g, 0xa5, sizeof(g)); /* a negative number: below every distance, should anybody read it */
    return g;
}

/* what the kernels get from the device: no barrier for one worker, a list with a flag per tile */
struct HostDev {
    const double* img;
    std::vector<int>* list;
    std::vector<uint8_t>* flag;
    int64_t sweeps, capped;
    void sync() const {}
    int vote(int b) const { return b; }
    double load(const double* p) const { return *p; }
    void store(double* p, double v) const { *p = v; }
    double image(int64_t id) const { return img[id]; }
    void wake(int t)
    {
        if ((*flag)[(size_t)t]) return;
        (*flag)[(size_t)t] = 1;
        list->push_back(t);
    }
    void visited(int s, bool c)
    {
        sweeps += s;
        capped += c ? 1 : 0;
    }
};

int main(int argc, char** argv)
{
    if (argc != 14) {
        fprintf(stderr, "usage: geo_main <dz> <dy> <dx> <full> <gamma> <step> <sz> <sy> <sx> <order seed> <image.bin | -> <seeds.bin> <out.bin>\n");
        return 2;
    }
    MgcLattice L;
    memset(&L, 0, sizeof(L));
    L.dz = strtoll(argv[1], nullptr, 10);
    L.dy = strtoll(argv[2], nullptr, 10);
    L.dx = strtoll(argv[3], nullptr, 10);
    if (L.dz < 1 || L.dy < 1 || L.dx < 1 || L.dz * L.dy * L.dx > (1ll << 24)) return 2;
    L.nvox = L.dz * L.dy * L.dx;
    L.gz = (int)((L.dz + 7) / 8);
    L.gy = (int)((L.dy + 7) / 8);
    L.gx = (int)((L.dx + 7) / 8);
    L.ntiles = L.gz * L.gy * L.gx;
    const int full = atoi(argv[4]);
    const double gamma = strtod(argv[5], nullptr), step = strtod(argv[6], nullptr);
    const double sp[3] = {strtod(argv[7], nullptr), strtod(argv[8], nullptr), strtod(argv[9], nullptr)};
    const unsigned long long order = strtoull(argv[10], nullptr, 10);
    const bool has_image = strcmp(argv[11], "-") != 0;
    if ((full != 0 && full != 1) || (!has_image && gamma != 0.0)) return 2;
    std::vector<double> image;
    std::vector<uint8_t> seeds;
    if (has_image && !read_file(argv[11], &image, (size_t)L.nvox)) return 2;
    if (!read_file(argv[12], &seeds, (size_t)L.nvox)) return 2;
    MgcGeoSteps S;
    mgc_geo_steps(sp, step, &S);

    std::vector<double> plane((size_t)L.nvox, garbage());
    std::vector<int> list[2];
    std::vector<uint8_t> flag[2] = {std::vector<uint8_t>((size_t)L.ntiles, 0), std::vector<uint8_t>((size_t)L.ntiles, 0)};
    HostDev dev = {has_image ? image.data() : nullptr, &list[0], &flag[0], 0, 0};
    int64_t nseeds = 0;
    for (int64_t v = L.nvox - 1; v >= 0; --v) nseeds += mgc_geo_init_voxel<GEO_DOCTOR>(L, seeds.data(), v, full != 0, plane.data(), dev) ? 1 : 0;

    std::mt19937_64 rng(order);
    std::vector<double> sd(MGC_GEO_CELLS), si(MGC_GEO_CELLS);
    uint8_t wake[27];
    int64_t rounds = 0, visits = 0;
    const int64_t max_rounds = L.nvox + 1;
    for (int cur = 0; !list[cur].empty(); cur ^= 1) {
        if (rounds >= max_rounds) return 3;
        std::vector<int>& tiles = list[cur];
        for (size_t i = tiles.size(); i > 1; --i) std::swap(tiles[i - 1], tiles[(size_t)(rng() % i)]);
        dev.list = &list[cur ^ 1];
        dev.flag = &flag[cur ^ 1];
        for (const int tile : tiles) {
            flag[cur][(size_t)tile] = 0;
            for (double& x : sd) x = garbage();
            for (double& x : si) x = garbage();
            memset(wake, 0xa5, sizeof(wake));
            if (full) mgc_geo_tile_step<true, GEO_DOCTOR, 1>(L, S, gamma, has_image, tile, plane.data(), sd.data(), si.data(), wake, 0, dev);
            else mgc_geo_tile_step<false, GEO_DOCTOR, 1>(L, S, gamma, has_image, tile, plane.data(), sd.data(), si.data(), wake, 0, dev);
        }
        visits += (int64_t)tiles.size();
        tiles.clear();
        ++rounds;
    }
    int64_t finite = 0;
    for (const double d : plane) finite += d < MGC_EDT_INF ? 1 : 0;
    std::vector<double> out = plane;
    const int64_t info[6] = {nseeds, rounds, visits, dev.sweeps, dev.capped, finite};
    for (const int64_t k : info) out.push_back((double)k);
    return write_file(argv[13], out) ? 0 : 2;
}
