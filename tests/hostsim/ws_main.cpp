/*
 * ws_main.cpp -- TEST ONLY.  The steps of mgc_watershed_image (medpy_amd/csrc/mgc_ws.h) as a stand-alone program with one worker, so
 * that the very lines the kernels compile can be checked on the CPU, and built with -fsanitize=address,undefined.  The schedule is
 * the library's: mgc_ws_init_voxel over the voxels, then rounds of tile visits over two work lists swapped, until a round wakes
 * nobody; mgc_ws_parent over the voxels; pointer jumping until a round moves nothing; the marker of the root.  The tiles of a round
 * are visited in a seeded random order; the shared arrays of a visit and the plane arrive filled with garbage.
 *
 *   ws_main <dz> <dy> <dx> <dtype> <order seed> <image.bin> <markers.bin> <mask.bin | -> <out.bin>
 *       image.bin: nvox values of dtype (the ids of medpy_hip.h); markers.bin: nvox int32; mask.bin: nvox bytes ("-": no mask);
 *       out.bin: nvox uint64 (T), nvox uint32 (parents), nvox int32 (labels), then 8 int64: the slots of out8
 *   ws_main minima <dz> <dy> <dx> <dtype> <size> <image.bin> <out.bin>
 *       out.bin: nvox bytes, image == minimum filter of window `size`
 *
 * Built with -DWS_NO_RISE_RESET a rise does not reset D, with -DWS_NO_SELF_WAKE a visit that ends at the sweep cap does not wake its
 * own tile: the doctored stand-ins the cases must reject.  Exit status 0 unless the arguments or files are unusable; 3 when the
 * rounds did not end within their bound.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "../../medpy_amd/csrc/mgc_ws.h"

#if defined(WS_NO_RISE_RESET)
#define WS_DOCTOR_RISE MGC_WS_NO_RISE_RESET
#else
#define WS_DOCTOR_RISE 0
#endif
#if defined(WS_NO_SELF_WAKE)
#define WS_DOCTOR_SELF MGC_WS_NO_SELF_WAKE
#else
#define WS_DOCTOR_SELF 0
#endif
#define WS_DOCTOR (WS_DOCTOR_RISE | WS_DOCTOR_SELF)

static bool read_file(const char* path, std::vector<uint8_t>* out, size_t want)
{
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    out->resize(want + 1);
    const size_t n = fread(out->data(), 1, want + 1, f);
    fclose(f);
    out->resize(want);
    return n == want;
}

static size_t size_of(int dtype)
{
    switch (dtype) {
    case MGC_U8: case MGC_I8: return 1;
    case MGC_U16: case MGC_I16: return 2;
    case MGC_U32: case MGC_I32: case MGC_F32: return 4;
    default: return 0;
    }
}

/* what the kernels get from the device: no barrier for one worker, a list with a flag per tile */
struct HostDev {
    std::vector<int>* list;
    std::vector<uint8_t>* flag;
    int64_t sweeps, capped;
    void sync() const {}
    int vote(int b) const { return b; }
    uint64_t load(const uint64_t* p) const { return *p; }
    void store(uint64_t* p, uint64_t v) const { *p = v; }
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

static int minima(int argc, char** argv)
{
    if (argc != 9) return 2;
    const int64_t dims[3] = {strtoll(argv[2], nullptr, 10), strtoll(argv[3], nullptr, 10), strtoll(argv[4], nullptr, 10)};
    const int dtype = atoi(argv[5]), size = atoi(argv[6]);
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1 || dims[0] * dims[1] * dims[2] > (1ll << 24) || !size_of(dtype) || size < 1) return 2;
    const int64_t nvox = dims[0] * dims[1] * dims[2];
    std::vector<uint8_t> image;
    if (!read_file(argv[7], &image, (size_t)nvox * size_of(dtype))) return 2;
    std::vector<uint32_t> keys((size_t)nvox), a, b((size_t)nvox);
    for (int64_t v = 0; v < nvox; ++v) keys[(size_t)v] = mgc_ws_key(image.data(), dtype, v);
    a = keys;
    const int64_t strides[3] = {dims[1] * dims[2], dims[2], 1};
    for (int ax = 0; ax < 3; ++ax) {
        if (dims[ax] == 1 || size == 1) continue; /* (the driver's rule) */
        for (int64_t v = 0; v < nvox; ++v) {
            const int64_t i = (v / strides[ax]) % dims[ax];
            b[(size_t)v] = mgc_ws_window_min(a.data() + (v - i * strides[ax]), strides[ax], dims[ax], i, size);
        }
        a.swap(b);
    }
    std::vector<uint8_t> out((size_t)nvox);
    for (int64_t v = 0; v < nvox; ++v) out[(size_t)v] = keys[(size_t)v] == a[(size_t)v] ? 1 : 0;
    FILE* f = fopen(argv[8], "wb");
    if (!f) return 2;
    const bool ok = fwrite(out.data(), 1, out.size(), f) == out.size();
    fclose(f);
    return ok ? 0 : 2;
}

int main(int argc, char** argv)
{
    if (argc >= 2 && strcmp(argv[1], "minima") == 0) return minima(argc, argv);
    if (argc != 10) {
        fprintf(stderr, "usage: ws_main <dz> <dy> <dx> <dtype> <order seed> <image.bin> <markers.bin> <mask.bin | -> <out.bin>\n");
        return 2;
    }
    const int64_t dims[3] = {strtoll(argv[1], nullptr, 10), strtoll(argv[2], nullptr, 10), strtoll(argv[3], nullptr, 10)};
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1 || dims[0] * dims[1] * dims[2] > (1ll << 24)) return 2;
    MgcLattice L;
    mgc_ws_lattice(dims, &L);
    const int dtype = atoi(argv[4]);
    const unsigned long long order = strtoull(argv[5], nullptr, 10);
    const bool has_mask = strcmp(argv[8], "-") != 0;
    if (!size_of(dtype)) return 2;
    std::vector<uint8_t> image, marker_bytes, mask;
    if (!read_file(argv[6], &image, (size_t)L.nvox * size_of(dtype))) return 2;
    if (!read_file(argv[7], &marker_bytes, (size_t)L.nvox * sizeof(int32_t))) return 2;
    if (has_mask && !read_file(argv[8], &mask, (size_t)L.nvox)) return 2;
    std::vector<int32_t> markers((size_t)L.nvox);
    memcpy(markers.data(), marker_bytes.data(), marker_bytes.size());
    const uint8_t* const pm = has_mask ? mask.data() : nullptr;

    const uint64_t garbage = 0x00a5a5a5a5a5a5a5ull; /* below many real words, should anybody read it */
    std::vector<uint64_t> plane((size_t)L.nvox, garbage);
    std::vector<int> list[2];
    std::vector<uint8_t> flag[2] = {std::vector<uint8_t>((size_t)L.ntiles, 0), std::vector<uint8_t>((size_t)L.ntiles, 0)};
    HostDev dev = {&list[0], &flag[0], 0, 0};
    int64_t nseeds = 0;
    for (int64_t v = L.nvox - 1; v >= 0; --v) nseeds += mgc_ws_init_voxel(L, image.data(), dtype, markers.data(), pm, v, plane.data(), dev) ? 1 : 0;

    std::mt19937_64 rng(order);
    std::vector<uint64_t> st(MGC_WS_CELLS);
    uint8_t wake[8];
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
            for (uint64_t& x : st) x = garbage;
            memset(wake, 0xa5, sizeof(wake));
            mgc_ws_tile_step<WS_DOCTOR, 1>(L, image.data(), dtype, markers.data(), pm, tile, plane.data(), st.data(), wake, 0, dev);
        }
        visits += (int64_t)tiles.size();
        tiles.clear();
        ++rounds;
    }
    std::vector<uint32_t> parent((size_t)L.nvox), root;
    int64_t reached = 0;
    for (int64_t v = 0; v < L.nvox; ++v) {
        parent[(size_t)v] = mgc_ws_parent(L, plane.data(), markers.data(), pm, v);
        reached += parent[(size_t)v] != MGC_WS_NONE ? 1 : 0;
    }
    root = parent;
    int64_t jumps = 0;
    for (bool moved = true; moved; ++jumps) {
        if (jumps > 33) return 3;
        moved = false;
        for (int64_t v = 0; v < L.nvox; ++v) {
            const uint32_t q = root[(size_t)v];
            if (q == MGC_WS_NONE) continue;
            const uint32_t r = root[q];
            if (r != q) { root[(size_t)v] = r; moved = true; }
        }
    }
    std::vector<int32_t> labels((size_t)L.nvox);
    for (int64_t v = 0; v < L.nvox; ++v) labels[(size_t)v] = root[(size_t)v] == MGC_WS_NONE ? 0 : markers[root[(size_t)v]];
    const int64_t info[8] = {nseeds, rounds, visits, dev.sweeps, dev.capped, reached, jumps, 0};
    FILE* f = fopen(argv[9], "wb");
    if (!f) return 2;
    bool ok = fwrite(plane.data(), sizeof(uint64_t), plane.size(), f) == plane.size();
    ok = ok && fwrite(parent.data(), sizeof(uint32_t), parent.size(), f) == parent.size();
    ok = ok && fwrite(labels.data(), sizeof(int32_t), labels.size(), f) == labels.size();
    ok = ok && fwrite(info, sizeof(int64_t), 8, f) == 8;
    fclose(f);
    return ok ? 0 : 2;
}
