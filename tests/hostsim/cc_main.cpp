/*
 * cc_main.cpp -- TEST ONLY.  The steps of mgc_components (medpy_amd/csrc/mgc_cc.h) as a stand-alone program, so that the very lines
 * the kernels compile can be checked on the CPU, and built with -fsanitize=address,undefined.
 *
 *   cc_main run <dz> <dy> <dx> <seed> <plane.bin> <fg.bin | -> <bg.bin | -> <out.bin>
 *       reads dz * dy * dx label bytes (and marker bytes) and labels the plane four times: (side, full) = (0, 0), (0, 1), (1, 0),
 *       (1, 1).  The tile step runs with one worker; tiles, cross-tile voxels, the flattening and the gathering are visited in an
 *       order shuffled by <seed>; the on-chip arrays of a tile arrive filled with garbage, and so do the three planes.  Per run the
 *       output holds int64: K, unions, longest walk, the nvox ids, then first / size / flags of the K components.
 *       Built with -DCC_SKIP_DIAGONAL the merge runs at the face neighbourhood always, so the edge and corner pairs are left out:
 *       the doctored stand-in the cases must reject.
 *   cc_main rule <min_size> <largest> <seeded> <table.bin> <out.bin>
 *       step 1 of the cleaning rule (mgc_cc_rule_keep) on a table of K sizes followed by K flags (int64 each); writes int64: the K
 *       keep bytes, survivors, voxels removed.
 *
 * Exit status 0 unless the arguments or files are unusable.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "../../medpy_amd/csrc/mgc_cc.h"

/* the doctored stand-in: the tile step at the neighbourhood asked for, the merge at the FACE neighbourhood whatever was asked for */
#ifdef CC_SKIP_DIAGONAL
#define CC_MERGE_FULL(FULL) false
#else
#define CC_MERGE_FULL(FULL) (FULL)
#endif

static bool read_file(const char* path, std::vector<uint8_t>* out)
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

static bool write_file(const char* path, const std::vector<int64_t>& out)
{
    FILE* f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = fwrite(out.data(), sizeof(int64_t), out.size(), f) == out.size();
    fclose(f);
    return ok;
}

struct OneWorker {
    int operator()(int v) const { return v != 0; }
    int bits(int v) const { return v; }
};

template <bool FULL>
static void label(const MgcLattice& L, const uint8_t* plane, int side, const uint8_t* fg, const uint8_t* bg, std::mt19937& rng, std::vector<int64_t>* out)
{
    const size_t n = (size_t)L.nvox;
    std::vector<uint32_t> parent(n, 0xa5a5a5a5u), count(n, 0xa5a5a5a5u);
    std::vector<uint8_t> flags(n, 0xa5);
    MgcCcAtomHost at;
    OneWorker one;
    std::vector<int> tiles((size_t)L.ntiles);
    for (int t = 0; t < L.ntiles; ++t) tiles[(size_t)t] = t;
    std::shuffle(tiles.begin(), tiles.end(), rng);
    uint16_t lab[MGC_CC_BLOCK];
    uint32_t acc[2 * MGC_TV];
    for (int tile : tiles) {
        memset(lab, 0x5a, sizeof(lab));
        memset(acc, 0x5a, sizeof(acc));
        mgc_cc_tile_step<FULL>(L, plane, side, 0, fg, bg, tile, parent.data(), count.data(), flags.data(), lab, acc, 0, 1, at, one);
    }
    uint32_t unions = 0u, walk = 0u;
    std::vector<int64_t> pairs((size_t)L.ntiles * MGC_TV);
    for (size_t k = 0; k < pairs.size(); ++k) pairs[k] = (int64_t)k;
    std::shuffle(pairs.begin(), pairs.end(), rng);
    for (int64_t k : pairs) {
        int tz, ty, tx;
        mgc_tile_coords(L, (int)(k / MGC_TV), tz, ty, tx);
        mgc_cc_merge_voxel<CC_MERGE_FULL(FULL)>(L, parent.data(), tz, ty, tx, (int)(k % MGC_TV), at, unions, walk);
    }
    std::vector<uint32_t> order(n);
    for (size_t v = 0; v < n; ++v) order[v] = (uint32_t)v;
    std::shuffle(order.begin(), order.end(), rng);
    for (uint32_t v : order) mgc_cc_flatten_voxel(parent.data(), v, at, walk);
    std::shuffle(order.begin(), order.end(), rng);
    for (uint32_t v : order) mgc_cc_gather_voxel(parent.data(), count.data(), flags.data(), v, at);
    /* the ranking: roots ascending, rank + 1 into the root's count word, then the ids */
    std::vector<int64_t> first, size, fl;
    for (size_t v = 0; v < n; ++v) {
        if (parent[v] != (uint32_t)v) continue;
        first.push_back((int64_t)v);
        size.push_back((int64_t)count[v]);
        fl.push_back((int64_t)flags[v]);
        count[v] = (uint32_t)first.size();
    }
    out->push_back((int64_t)first.size());
    out->push_back((int64_t)unions);
    out->push_back((int64_t)walk);
    for (size_t v = 0; v < n; ++v) out->push_back(parent[v] == MGC_CC_NONE ? 0 : (int64_t)count[parent[v]]);
    out->insert(out->end(), first.begin(), first.end());
    out->insert(out->end(), size.begin(), size.end());
    out->insert(out->end(), fl.begin(), fl.end());
}

static int run(int argc, char** argv)
{
    if (argc != 10) return 2;
    MgcLattice L;
    memset(&L, 0, sizeof(L));
    L.dz = strtoll(argv[2], nullptr, 10);
    L.dy = strtoll(argv[3], nullptr, 10);
    L.dx = strtoll(argv[4], nullptr, 10);
    if (L.dz < 1 || L.dy < 1 || L.dx < 1 || L.dz * L.dy * L.dx > (1ll << 24)) return 2;
    L.nvox = L.dz * L.dy * L.dx;
    L.gz = (int)((L.dz + 7) / 8);
    L.gy = (int)((L.dy + 7) / 8);
    L.gx = (int)((L.dx + 7) / 8);
    L.ntiles = L.gz * L.gy * L.gx;
    L.tz_own_hi = L.gz;
    std::mt19937 rng((unsigned)strtoul(argv[5], nullptr, 10));
    std::vector<uint8_t> plane, fg, bg;
    if (!read_file(argv[6], &plane) || plane.size() != (size_t)L.nvox) return 2;
    const bool has_fg = strcmp(argv[7], "-") != 0, has_bg = strcmp(argv[8], "-") != 0;
    if (has_fg && (!read_file(argv[7], &fg) || fg.size() != plane.size())) return 2;
    if (has_bg && (!read_file(argv[8], &bg) || bg.size() != plane.size())) return 2;
    std::vector<int64_t> out;
    for (int side = 0; side < 2; ++side) {
        label<false>(L, plane.data(), side, has_fg ? fg.data() : nullptr, has_bg ? bg.data() : nullptr, rng, &out);
        label<true>(L, plane.data(), side, has_fg ? fg.data() : nullptr, has_bg ? bg.data() : nullptr, rng, &out);
    }
    return write_file(argv[9], out) ? 0 : 2;
}

static int rule(int argc, char** argv)
{
    if (argc != 7) return 2;
    std::vector<uint8_t> raw;
    if (!read_file(argv[5], &raw) || raw.size() % (2 * sizeof(int64_t)) != 0) return 2;
    const int64_t K = (int64_t)(raw.size() / (2 * sizeof(int64_t)));
    std::vector<int64_t> table((size_t)(2 * K));
    if (K) memcpy(table.data(), raw.data(), raw.size());
    std::vector<uint8_t> flags((size_t)K), keep((size_t)K + 1, 0);
    for (int64_t k = 0; k < K; ++k) flags[(size_t)k] = (uint8_t)table[(size_t)(K + k)];
    int64_t survivors = 0, removed = 0;
    mgc_cc_rule_keep(K, table.data(), flags.data(), strtoll(argv[2], nullptr, 10), strtoll(argv[3], nullptr, 10), atoi(argv[4]), keep.data(), &survivors, &removed);
    std::vector<int64_t> out;
    for (int64_t k = 0; k < K; ++k) out.push_back(keep[(size_t)k]);
    out.push_back(survivors);
    out.push_back(removed);
    return write_file(argv[6], out) ? 0 : 2;
}

int main(int argc, char** argv)
{
    int rc = 2;
    if (argc > 1 && !strcmp(argv[1], "run")) rc = run(argc, argv);
    else if (argc > 1 && !strcmp(argv[1], "rule")) rc = rule(argc, argv);
    if (rc == 2) fprintf(stderr, "usage: cc_main run <dz> <dy> <dx> <seed> <plane.bin> <fg.bin|-> <bg.bin|-> <out.bin>\n       cc_main rule <min_size> <largest> <seeded> <table.bin> <out.bin>\n");
    return rc;
}
