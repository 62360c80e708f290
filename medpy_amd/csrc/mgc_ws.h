/*
 * mgc_ws.h -- the seeded watershed on the lattice and the minimum filter of its markers (mgc_watershed_image,
 * mgc_local_minima_image), stated once.
 *
 * Inputs.  An image I of 1 to 3 axes in C order, int32 markers (0: none, > 0: a label), an optional byte mask (0: outside).  Face
 * neighbourhood (2 / 4 / 6 neighbours).  A neighbour outside the volume or outside the mask does not exist; a marker outside the
 * mask is no marker.  Only image values are compared: nothing is rounded anywhere.
 *
 * 1. The arrival key T(p) = (H, D), compared lexicographically, held as ONE 64-bit word key(H) << 32 | D.  key maps the image value
 *    to uint32 and keeps the order (mgc_ws_key: integers biased, float32 with the sign flipped and -0.0 on the key of +0.0).
 *        seeds        T(s) = (I(s), 0), fixed
 *        ext(t, p)    = (I(p), 0) if I(p) > H(t), else (H(t), D(t) + 1)         (mgc_ws_ext)
 *    T(p) of a voxel that is no seed is the minimum over the seeds and the lattice paths of the seed's key extended step by step;
 *    MGC_WS_INF where no seed connects.  H is the water level at which p floods (the minimax height of a path), D the steps since
 *    the path last rose.  ext is monotone (t <= t' => ext(t, p) <= ext(t', p)) and inflationary (ext(t, p) > t), so T is the LEAST
 *    FIXPOINT of T(p) <- min(T(p), ext(T(q), p)) over the neighbours q, from the seeds' keys and MGC_WS_INF elsewhere, and every
 *    schedule of relaxations that reaches a fixpoint reaches these very words: a relaxation only ever writes the key of a real path
 *    (never below T), and at a fixpoint induction along an optimal path gives a word never above T.  (mgc_geo.h's argument.)
 * 2. The parent of a reached voxel p that is no seed is the neighbour q with T(q) < T(p) that minimises (T(q), flat index of q)
 *    (mgc_ws_parent).  One exists (the last step of an optimal path), and T falls strictly along parents: a forest rooted in the seeds.
 * 3. The label L(p) is the marker of the root of p's chain; 0 outside the mask and where no seed connects.
 *
 *   mgc_ws_key         image value -> uint32
 *   mgc_ws_init_voxel  T of a seed, MGC_WS_INF elsewhere; a seed wakes its tile and the face tiles that read it as a halo cell
 *   mgc_ws_tile_step   one visit of one 8x8x8 tile: the 10x10x10 block of T into a shared array, sweeps in pull form (Jacobi: every
 *                      read of a sweep before a barrier, every write behind it) until a vote says nothing fell or MGC_WS_SWEEP_CAP
 *                      is reached, the cells that fell written back, the face tiles that read one of them woken for the next
 *                      round (a visit that ended at the cap wakes its own tile): mgc_geo_tile_step's schedule with a u64 word
 *   mgc_ws_parent      the parent of one voxel from the finished plane
 *   mgc_ws_reflect     scipy.ndimage's `reflect` border (d c b a | a b c d | d c b a), any distance outside
 *   mgc_ws_window_min  the minimum of the window scipy.ndimage.minimum_filter(size=...) lays over one position of one axis
 *
 * Everything is MGC_HD and free of HIP: the kernels of mgc_ws_ops.inl and the stand-alone host program of the CPU test tier
 * (tests/hostsim/ws_main.cpp) compile these very lines.  What differs is passed in as `Dev` (see mgc_ws_tile_step).
 */
#ifndef MGC_WS_H
#define MGC_WS_H

#include <stdint.h>

#include "../../include/medpy_hip.h"
#include "mgc_common.h"

#define MGC_WS_SWEEP_CAP 64 /* sweeps of one visit: a corridor that winds inside a tile costs rounds, never an unbounded loop */
#define MGC_WS_EDGE 10      /* the block of a visit: the tile and one layer of halo cells around it */
#define MGC_WS_CELLS 1000
#define MGC_WS_INF 0xffffffffffffffffull /* no seed connects (a real word is below it: D < nvox < 2^32 - 1) */
#define MGC_WS_NONE 0xffffffffu          /* the parent of a voxel no seed reaches, or outside the mask */
#define MGC_WS_MAX_VOXELS 0xffffffffll   /* volumes of this many voxels or more are refused */
/* slots of out8 of mgc_watershed_image */
#define MGC_WS_SEEDS 0
#define MGC_WS_ROUNDS 1
#define MGC_WS_VISITS 2
#define MGC_WS_SWEEPS 3
#define MGC_WS_CAPPED 4
#define MGC_WS_REACHED 5
#define MGC_WS_JUMPS 6
/* what the test program's doctored builds get wrong (the library passes 0) */
#define MGC_WS_NO_RISE_RESET 1
#define MGC_WS_NO_SELF_WAKE 2

/* Voxel id of an image of dtype MGC_U8 .. MGC_I32 or MGC_F32 as a uint32 that keeps the order of the values.  Signed integers are
 * biased by 2^31.  float32: -0.0 becomes +0.0 first, then a negative number has all its bits turned and any other its sign bit set
 * (NaNs are refused before this is called). */
MGC_HD uint32_t mgc_ws_key(const void* image, int dtype, int64_t id)
{
    switch (dtype) {
    case MGC_U8: return (uint32_t)((const uint8_t*)image)[id];
    case MGC_I8: return (uint32_t)(int32_t)((const int8_t*)image)[id] ^ 0x80000000u;
    case MGC_U16: return (uint32_t)((const uint16_t*)image)[id];
    case MGC_I16: return (uint32_t)(int32_t)((const int16_t*)image)[id] ^ 0x80000000u;
    case MGC_U32: return ((const uint32_t*)image)[id];
    case MGC_I32: return ((const uint32_t*)image)[id] ^ 0x80000000u;
    default: {
        uint32_t b = ((const uint32_t*)image)[id]; /* MGC_F32, read as its bits */
        if (b == 0x80000000u) b = 0u;
        return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    }
    }
}

/* is the float32 with these bits finite? */
MGC_HD bool mgc_ws_finite_bits(uint32_t b) { return (b & 0x7f800000u) != 0x7f800000u; }

/* ext(t, p) for the key kp of I(p); MGC_WS_INF stays */
template <int DOCTOR>
MGC_HD uint64_t mgc_ws_ext(uint64_t t, uint32_t kp)
{
    if (t == MGC_WS_INF) return MGC_WS_INF;
    if (kp > (uint32_t)(t >> 32)) return ((uint64_t)kp << 32) | ((DOCTOR & MGC_WS_NO_RISE_RESET) ? (uint64_t)((uint32_t)t + 1u) : 0ull);
    return t + 1ull;
}

/* is voxel v a seed?  a marker inside the mask */
MGC_HD bool mgc_ws_is_seed(const int32_t* markers, const uint8_t* mask, int64_t v) { return markers[v] > 0 && (!mask || mask[v] != 0); }

/* the face tile of tile (tz, ty, tx) in direction f (mgc_common.h), or -1 */
MGC_HD int mgc_ws_face_tile(const MgcLattice& L, int tz, int ty, int tx, int f) { return mgc_tile_nbr(L, tz, ty, tx, f); }

/* The cell (lz, ly, lx) of a tile has a new word: wake[f] = 1 for every face f whose tile reads the cell as a halo cell.  Plain
 * stores of 1: any number of workers may store the same byte. */
MGC_HD void mgc_ws_wake_cell(int lz, int ly, int lx, uint8_t* wake)
{
    if (lx == 0) wake[0] = 1;
    if (lx == MGC_T - 1) wake[1] = 1;
    if (ly == 0) wake[2] = 1;
    if (ly == MGC_T - 1) wake[3] = 1;
    if (lz == 0) wake[4] = 1;
    if (lz == MGC_T - 1) wake[5] = 1;
}

/* Voxel v of the plane (C order): the key of a seed, MGC_WS_INF elsewhere.  A seed wakes its own tile and the face tiles that
 * read it as a halo cell: the seed's own cell never falls, so no visit would.  true: v is a seed. */
template <class Dev>
MGC_HD bool mgc_ws_init_voxel(const MgcLattice& L, const void* image, int dtype, const int32_t* markers, const uint8_t* mask, int64_t v, uint64_t* plane, Dev& dev)
{
    const bool seed = mgc_ws_is_seed(markers, mask, v);
    plane[v] = seed ? (uint64_t)mgc_ws_key(image, dtype, v) << 32 : MGC_WS_INF;
    if (!seed) return false;
    const int64_t x = v % L.dx, r = v / L.dx, y = r % L.dy, z = r / L.dy;
    const int tz = (int)(z >> 3), ty = (int)(y >> 3), tx = (int)(x >> 3);
    uint8_t wake[MGC_NDIR] = {0, 0, 0, 0, 0, 0};
    mgc_ws_wake_cell((int)(z & 7), (int)(y & 7), (int)(x & 7), wake);
    dev.wake(mgc_tile_id(L, tz, ty, tx));
    for (int f = 0; f < MGC_NDIR; ++f) {
        if (!wake[f]) continue;
        const int t = mgc_ws_face_tile(L, tz, ty, tx, f);
        if (t >= 0) dev.wake(t);
    }
    return true;
}

/* One visit of `tile` by NT workers of which this is number t0.  st: MGC_WS_CELLS words, wake: 8 bytes, shared by the workers.
 * Dev: sync() the workers' barrier, vote(b) the barrier that returns the OR of every worker's b, load(p) / store(p, w) a word of
 * the plane (other tiles write their own cells of it meanwhile: aligned 8-byte words that only fall, and whoever lowers one wakes
 * its readers for the next round), wake(t) tile t is visited in the next round, visited(sweeps, capped) the counts of the visit
 * (called by worker 0).  A cell outside the volume or outside the mask holds MGC_WS_INF in the block and is never written; a seed
 * keeps its word. */
template <int DOCTOR, int NT, class Dev>
MGC_HD void mgc_ws_tile_step(const MgcLattice& L, const void* image, int dtype, const int32_t* markers, const uint8_t* mask, int tile, uint64_t* plane, uint64_t* st, uint8_t* wake,
                             int t0, Dev& dev)
{
    constexpr int NV = MGC_TV / NT;
    int tz, ty, tx;
    mgc_tile_coords(L, tile, tz, ty, tx);
    const int64_t z0 = (int64_t)tz * MGC_T - 1, y0 = (int64_t)ty * MGC_T - 1, x0 = (int64_t)tx * MGC_T - 1;
    for (int c = t0; c < MGC_WS_CELLS; c += NT) {
        const int64_t z = z0 + c / (MGC_WS_EDGE * MGC_WS_EDGE), y = y0 + (c / MGC_WS_EDGE) % MGC_WS_EDGE, x = x0 + c % MGC_WS_EDGE;
        const bool inside = z >= 0 && z < L.dz && y >= 0 && y < L.dy && x >= 0 && x < L.dx;
        st[c] = inside ? dev.load(plane + ((z * L.dy + y) * L.dx + x)) : MGC_WS_INF;
    }
    for (int k = t0; k < 8; k += NT) wake[k] = 0;
    dev.sync();
    uint64_t first[NV], now[NV], next[NV];
    uint32_t kp[NV];
    bool open[NV]; /* the cell takes part: inside the volume and the mask, and no seed */
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < NV; ++i) {
        const int v = t0 + i * NT, lz = v >> 6, ly = (v >> 3) & 7, lx = v & 7;
        const int c = ((lz + 1) * MGC_WS_EDGE + ly + 1) * MGC_WS_EDGE + lx + 1;
        const int64_t z = z0 + 1 + lz, y = y0 + 1 + ly, x = x0 + 1 + lx;
        const bool owned = z < L.dz && y < L.dy && x < L.dx;
        const int64_t id = (z * L.dy + y) * L.dx + x;
        open[i] = owned && (!mask || mask[id] != 0) && !(markers[id] > 0);
        kp[i] = open[i] ? mgc_ws_key(image, dtype, id) : 0u;
        first[i] = now[i] = next[i] = st[c];
    }
    int sweeps = 0, more = 0;
    while (sweeps < MGC_WS_SWEEP_CAP) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 0; i < NV; ++i) {
            if (!open[i]) continue;
            const int v = t0 + i * NT, lz = v >> 6, ly = (v >> 3) & 7, lx = v & 7;
            const int c = ((lz + 1) * MGC_WS_EDGE + ly + 1) * MGC_WS_EDGE + lx + 1;
            uint64_t best = now[i];
            const int offs[MGC_NDIR] = {-1, 1, -MGC_WS_EDGE, MGC_WS_EDGE, -MGC_WS_EDGE * MGC_WS_EDGE, MGC_WS_EDGE * MGC_WS_EDGE};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int f = 0; f < MGC_NDIR; ++f) {
                const uint64_t cand = mgc_ws_ext<DOCTOR>(st[c + offs[f]], kp[i]);
                if (cand < best) best = cand;
            }
            next[i] = best;
        }
        dev.sync(); /* every read of the sweep lies before, every write behind */
        int fell = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 0; i < NV; ++i) {
            if (!open[i] || !(next[i] < now[i])) continue;
            const int v = t0 + i * NT, lz = v >> 6, ly = (v >> 3) & 7, lx = v & 7;
            st[((lz + 1) * MGC_WS_EDGE + ly + 1) * MGC_WS_EDGE + lx + 1] = now[i] = next[i];
            fell = 1;
        }
        ++sweeps;
        more = dev.vote(fell);
        if (!more) break;
    }
    /* the cells that fell go back, and whoever reads one as a halo cell is woken */
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < NV; ++i) {
        if (!open[i] || !(now[i] < first[i])) continue;
        const int v = t0 + i * NT, lz = v >> 6, ly = (v >> 3) & 7, lx = v & 7;
        dev.store(plane + (((z0 + 1 + lz) * L.dy + (y0 + 1 + ly)) * L.dx + (x0 + 1 + lx)), now[i]);
        mgc_ws_wake_cell(lz, ly, lx, wake);
    }
    if (t0 == 0 && more && !(DOCTOR & MGC_WS_NO_SELF_WAKE)) wake[6] = 1;
    dev.sync();
    for (int k = t0; k < 7; k += NT) {
        if (!wake[k]) continue;
        const int t = k == 6 ? tile : mgc_ws_face_tile(L, tz, ty, tx, k);
        if (t >= 0) dev.wake(t);
    }
    if (t0 == 0) dev.visited(sweeps, more != 0);
    dev.sync(); /* (the next visit of these workers rewrites the arrays) */
}

/* The parent of voxel v from the finished plane: v itself on a seed, MGC_WS_NONE where T is MGC_WS_INF (unreached, or outside the
 * mask), else the neighbour q with T(q) < T(v) that minimises (T(q), q).  Neighbours are visited in rising flat index, so the
 * first of equal words wins. */
MGC_HD uint32_t mgc_ws_parent(const MgcLattice& L, const uint64_t* plane, const int32_t* markers, const uint8_t* mask, int64_t v)
{
    const uint64_t t = plane[v];
    if (t == MGC_WS_INF) return MGC_WS_NONE;
    if (mgc_ws_is_seed(markers, mask, v)) return (uint32_t)v;
    const int64_t x = v % L.dx, r = v / L.dx, y = r % L.dy, z = r / L.dy;
    const int64_t sy = L.dx, sz = L.dx * L.dy;
    uint64_t best = t;
    uint32_t q = MGC_WS_NONE;
    if (z > 0 && plane[v - sz] < best) { best = plane[v - sz]; q = (uint32_t)(v - sz); }
    if (y > 0 && plane[v - sy] < best) { best = plane[v - sy]; q = (uint32_t)(v - sy); }
    if (x > 0 && plane[v - 1] < best) { best = plane[v - 1]; q = (uint32_t)(v - 1); }
    if (x + 1 < L.dx && plane[v + 1] < best) { best = plane[v + 1]; q = (uint32_t)(v + 1); }
    if (y + 1 < L.dy && plane[v + sy] < best) { best = plane[v + sy]; q = (uint32_t)(v + sy); }
    if (z + 1 < L.dz && plane[v + sz] < best) { best = plane[v + sz]; q = (uint32_t)(v + sz); }
    return q;
}

/* position i + o of an axis of n >= 1 entries under scipy.ndimage's `reflect` (d c b a | a b c d | d c b a): period 2n */
MGC_HD int64_t mgc_ws_reflect(int64_t j, int64_t n)
{
    const int64_t p = 2 * n;
    int64_t m = j % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

/* scipy.ndimage.minimum_filter(size=size) along one axis: the window of position i covers i - size / 2 .. i - size / 2 + size - 1
 * (integer division: the centre of an even window lies right of its middle).  line[k * stride], k in [0, n). */
MGC_HD uint32_t mgc_ws_window_min(const uint32_t* line, int64_t stride, int64_t n, int64_t i, int size)
{
    uint32_t m = 0xffffffffu;
    /* a window of two extents or more covers a whole period of the border: the minimum of the line */
    const bool whole = (int64_t)size >= 2 * n;
    const int64_t lo = whole ? 0 : i - size / 2, count = whole ? n : (int64_t)size;
    for (int64_t o = 0; o < count; ++o) {
        const uint32_t w = line[mgc_ws_reflect(lo + o, n) * stride];
        if (w < m) m = w;
    }
    return m;
}

/* the lattice of a volume of dims (z, y, x): only the fields the steps above read */
inline void mgc_ws_lattice(const int64_t dims[3], MgcLattice* L)
{
    *L = MgcLattice();
    L->dz = dims[0]; L->dy = dims[1]; L->dx = dims[2];
    L->nvox = dims[0] * dims[1] * dims[2];
    L->gz = (int)((dims[0] + MGC_T - 1) / MGC_T);
    L->gy = (int)((dims[1] + MGC_T - 1) / MGC_T);
    L->gx = (int)((dims[2] + MGC_T - 1) / MGC_T);
    L->ntiles = L->gz * L->gy * L->gx;
    L->tz_own_hi = L->gz;
}

#endif /* MGC_WS_H */
