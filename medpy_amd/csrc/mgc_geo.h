/*
 * mgc_geo.h -- the geodesic distance transform on the lattice and the regional term on top of it (mgc_geodesic_distance,
 * mgc_add_tweights_geodesic, mgc_update_tweights_geodesic), stated once.
 *
 * The value.  With the offset d in {-1, 0, 1}^3 between two neighbours p and q = p + d,
 *     a_k   = fl(spacing_k * |d_k|)
 *     e_d   = fl(step * sqrt(fl(fl(fl(a_x^2) + fl(a_y^2)) + fl(a_z^2))))          (x the last array axis: mgc_edt_sq's association)
 *     w(p,q) = fl(e_d + fl(gamma * |fl(I_p - I_q)|))                                (I the image as f64; gamma == 0: the image is not read)
 * D(v) is the minimum over the seeds s and the lattice paths s = p_0 .. p_k = v of the sum added from the seed outwards,
 * fl(..fl(fl(0 + w(p_0,p_1)) + w(p_1,p_2)).. + w(p_k-1,p_k)): 0 on seeds, +inf where no seed connects.  a -> fl(a + w) with w >= 0 is
 * monotone and never below a, so D is the LEAST FIXPOINT of D(q) <- min(D(q), fl(D(p) + w(p,q))) from 0 on the seeds and +inf
 * elsewhere, and every schedule of relaxations that reaches a fixpoint reaches these very f64 numbers: a relaxation only ever writes
 * the sum of a real path (never below D), and at a fixpoint induction along an optimal path gives a value never above D.
 *
 *   mgc_geo_step_length  e_d, ON THE HOST (the one square root; the kernels get a table of 27 values)
 *   mgc_geo_arc          w(p, q) from e_d and the two image values
 *   mgc_geo_init_voxel   D = 0 on a seed, +inf elsewhere; a seed wakes its tile and every tile that reads it as a halo cell
 *   mgc_geo_tile_step    one visit of one 8x8x8 tile: the 10x10x10 block of D and of the image into a shared array, the arc
 *                        lengths of every owned cell once, sweeps in pull form until a vote says nothing fell or MGC_GEO_SWEEP_CAP
 *                        is reached, the cells that fell written back, the tiles that read one of them as a halo cell woken for the
 *                        next round (a visit that ended at the cap wakes its own tile)
 *   mgc_geo_term         the regional term of one voxel from D_F and D_B
 *
 * A sweep reads every neighbour BEFORE a barrier and writes its own cell behind it (Jacobi): no word of the shared array is read
 * while it is written, and a cell has one writer.  Everything is MGC_HD and free of HIP: the kernels of mgc_geo_ops.inl and the
 * stand-alone host program of the CPU test tier (tests/hostsim/geo_main.cpp) compile these very lines.  What differs is passed in
 * as `Dev`: the barrier and the vote (nothing for one worker), the loads and stores of the plane, the image as f64, the wake-up of a
 * tile and the two counts of a visit.  NT is the number of workers of a visit (512 on the device: a thread owns one cell and its
 * arc lengths stay in registers; 1 in the host program, whose one worker owns all 512).
 *
 * NO CONTRACTION: mgc_geo_step_length and mgc_geo_arc switch it off for their own statements, the sum is mgc_edt_add (mgc_edt.h).
 */
#ifndef MGC_GEO_H
#define MGC_GEO_H

#include <math.h>
#include <stdint.h>

#include "mgc_common.h"
#include "mgc_edt.h"

#define MGC_GEO_SWEEP_CAP 64  /* sweeps of one visit: a path that winds inside a tile costs rounds, never an unbounded loop */
#define MGC_GEO_EDGE 10       /* the block of a visit: the tile and one layer of halo cells around it */
#define MGC_GEO_CELLS 1000
#define MGC_GEO_SELF 13       /* the centre of the 27 offsets: the tile itself */
/* slots of out8 of mgc_geodesic_distance */
#define MGC_GEO_SEEDS 0
#define MGC_GEO_ROUNDS 1
#define MGC_GEO_VISITS 2
#define MGC_GEO_SWEEPS 3
#define MGC_GEO_CAPPED 4
#define MGC_GEO_FINITE 5
/* what the test program's doctored builds leave out (the library passes 0) */
#define MGC_GEO_NO_DIAGONAL_WAKE 1
#define MGC_GEO_NO_SELF_WAKE 2

/* e[(oz + 1) * 9 + (oy + 1) * 3 + (ox + 1)]: the step length of the offset (oz, oy, ox); e[MGC_GEO_SELF] is not read */
struct MgcGeoSteps {
    double e[27];
};

/* e_d for the spacing sp of (z, y, x); host only: the device takes no square root */
inline double mgc_geo_step_length(const double sp[3], double step, int oz, int oy, int ox)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double az = sp[0] * (double)(oz < 0 ? -oz : oz);
    const double ay = sp[1] * (double)(oy < 0 ? -oy : oy);
    const double ax = sp[2] * (double)(ox < 0 ? -ox : ox);
    const double xx = ax * ax;
    const double yy = ay * ay;
    const double zz = az * az;
    const double xy = xx + yy;
    const double s = xy + zz;
    const double r = sqrt(s);
    const double e = step * r;
    return e;
}

inline void mgc_geo_steps(const double sp[3], double step, MgcGeoSteps* S)
{
    for (int k = 0; k < 27; ++k) S->e[k] = mgc_geo_step_length(sp, step, k / 9 - 1, (k / 3) % 3 - 1, k % 3 - 1);
}

/* fl(e + fl(gamma * |fl(ip - iq)|)) */
MGC_HD double mgc_geo_arc(double e, double gamma, double ip, double iq)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double d = ip - iq;
    const double a = __builtin_fabs(d);
    const double g = gamma * a;
    const double w = e + g;
    return w;
}

/* is the offset k one of the neighbourhood?  face: one axis moves; full: any */
MGC_HD bool mgc_geo_is_neighbour(int k, bool full)
{
    const int nonzero = (k / 9 != 1) + ((k / 3) % 3 != 1) + (k % 3 != 1);
    return nonzero != 0 && (full || nonzero == 1);
}

/* The cell (lz, ly, lx) of a tile has a new value: wake[k] = 1 for every offset k of a tile that reads the cell as a halo cell --
 * along each axis the cell's own layer, and the layer beyond where the cell lies at that end of the tile; at the face
 * neighbourhood only tiles across a face read halo cells.  Plain stores of 1: any number of workers may store the same byte. */
template <int DOCTOR>
MGC_HD void mgc_geo_wake_cell(int lz, int ly, int lx, bool full, uint8_t* wake)
{
    for (int oz = -1; oz <= 1; ++oz) {
        if ((oz < 0 && lz != 0) || (oz > 0 && lz != MGC_T - 1)) continue;
        for (int oy = -1; oy <= 1; ++oy) {
            if ((oy < 0 && ly != 0) || (oy > 0 && ly != MGC_T - 1)) continue;
            for (int ox = -1; ox <= 1; ++ox) {
                if ((ox < 0 && lx != 0) || (ox > 0 && lx != MGC_T - 1)) continue;
                const int nonzero = (oz != 0) + (oy != 0) + (ox != 0);
                if (nonzero == 0 || (!full && nonzero != 1)) continue;
                if ((DOCTOR & MGC_GEO_NO_DIAGONAL_WAKE) && nonzero != 1) continue;
                wake[(oz + 1) * 9 + (oy + 1) * 3 + (ox + 1)] = 1;
            }
        }
    }
}

/* the tile at offset k of tile (tz, ty, tx), or -1 outside the grid */
MGC_HD int mgc_geo_tile_at(const MgcLattice& L, int tz, int ty, int tx, int k)
{
    const int z = tz + k / 9 - 1, y = ty + (k / 3) % 3 - 1, x = tx + k % 3 - 1;
    if (z < 0 || z >= L.gz || y < 0 || y >= L.gy || x < 0 || x >= L.gx) return -1;
    return mgc_tile_id(L, z, y, x);
}

/* Voxel v of the plane (C order): 0 on a seed (any byte but 0 of `seeds`; NULL: no seeds), +inf elsewhere.  A seed wakes its own
 * tile and the tiles that read it as a halo cell: the seed's own cell never falls, so no visit would.  true: v is a seed. */
template <int DOCTOR, class Dev>
MGC_HD bool mgc_geo_init_voxel(const MgcLattice& L, const uint8_t* seeds, int64_t v, bool full, double* plane, Dev& dev)
{
    const bool seed = seeds && seeds[v] != 0;
    plane[v] = seed ? 0.0 : MGC_EDT_INF;
    if (!seed) return false;
    const int64_t x = v % L.dx, r = v / L.dx, y = r % L.dy, z = r / L.dy;
    const int tz = (int)(z >> 3), ty = (int)(y >> 3), tx = (int)(x >> 3);
    uint8_t wake[27];
    for (int k = 0; k < 27; ++k) wake[k] = 0;
    wake[MGC_GEO_SELF] = 1;
    mgc_geo_wake_cell<DOCTOR>((int)(z & 7), (int)(y & 7), (int)(x & 7), full, wake);
    for (int k = 0; k < 27; ++k) {
        if (!wake[k]) continue;
        const int t = mgc_geo_tile_at(L, tz, ty, tx, k);
        if (t >= 0) dev.wake(t);
    }
    return true;
}

/* One visit of `tile` by NT workers of which this is number t0.  sd, si: MGC_GEO_CELLS doubles each, wake: 27 bytes, shared by the
 * workers.  image NULL (gamma == 0): every arc is its step length.  Dev: sync() the workers' barrier, vote(b) the barrier that
 * returns the OR of every worker's b, load(p) / store(p, v) a word of the plane (other tiles write their own cells of it meanwhile:
 * aligned 8-byte words that only fall, and whoever lowers one wakes its readers for the next round), image(id) voxel id of the image
 * as f64, wake(t) tile t is visited in the next round, visited(sweeps, capped) the counts of the visit (called by worker 0). */
template <bool FULL, int DOCTOR, int NT, class Dev>
MGC_HD void mgc_geo_tile_step(const MgcLattice& L, const MgcGeoSteps& S, double gamma, bool has_image, int tile, double* plane, double* sd, double* si, uint8_t* wake, int t0, Dev& dev)
{
    constexpr int NV = MGC_TV / NT, NA = FULL ? 26 : 6;
    int tz, ty, tx;
    mgc_tile_coords(L, tile, tz, ty, tx);
    const int64_t z0 = (int64_t)tz * MGC_T - 1, y0 = (int64_t)ty * MGC_T - 1, x0 = (int64_t)tx * MGC_T - 1;
    /* the block: cells outside the volume (and so the padding of a partial tile) hold +inf and belong to nothing */
    for (int c = t0; c < MGC_GEO_CELLS; c += NT) {
        const int64_t z = z0 + c / (MGC_GEO_EDGE * MGC_GEO_EDGE), y = y0 + (c / MGC_GEO_EDGE) % MGC_GEO_EDGE, x = x0 + c % MGC_GEO_EDGE;
        const bool inside = z >= 0 && z < L.dz && y >= 0 && y < L.dy && x >= 0 && x < L.dx;
        const int64_t id = (z * L.dy + y) * L.dx + x;
        sd[c] = inside ? dev.load(plane + id) : MGC_EDT_INF;
        si[c] = inside && has_image ? dev.image(id) : 0.0;
    }
    for (int k = t0; k < 27; k += NT) wake[k] = 0;
    dev.sync();
    double w[NV][NA], first[NV], now[NV], next[NV];
    bool owned[NV];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < NV; ++i) {
        const int v = t0 + i * NT, lz = v >> 6, ly = (v >> 3) & 7, lx = v & 7;
        const int c = ((lz + 1) * MGC_GEO_EDGE + ly + 1) * MGC_GEO_EDGE + lx + 1;
        owned[i] = z0 + 1 + lz < L.dz && y0 + 1 + ly < L.dy && x0 + 1 + lx < L.dx;
        first[i] = now[i] = next[i] = sd[c];
        const double ic = si[c];
        int j = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int k = 0; k < 27; ++k) {
            if (!mgc_geo_is_neighbour(k, FULL)) continue;
            const int off = ((k / 9 - 1) * MGC_GEO_EDGE + (k / 3) % 3 - 1) * MGC_GEO_EDGE + k % 3 - 1;
            w[i][j++] = mgc_geo_arc(S.e[k], gamma, si[c + off], ic);
        }
    }
    int sweeps = 0, more = 0;
    while (sweeps < MGC_GEO_SWEEP_CAP) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 0; i < NV; ++i) {
            if (!owned[i]) continue;
            const int v = t0 + i * NT, lz = v >> 6, ly = (v >> 3) & 7, lx = v & 7;
            const int c = ((lz + 1) * MGC_GEO_EDGE + ly + 1) * MGC_GEO_EDGE + lx + 1;
            double best = now[i];
            int j = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int k = 0; k < 27; ++k) {
                if (!mgc_geo_is_neighbour(k, FULL)) continue;
                const int off = ((k / 9 - 1) * MGC_GEO_EDGE + (k / 3) % 3 - 1) * MGC_GEO_EDGE + k % 3 - 1;
                const double cand = mgc_edt_add(sd[c + off], w[i][j++]);
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
            if (!owned[i] || !(next[i] < now[i])) continue;
            const int v = t0 + i * NT, lz = v >> 6, ly = (v >> 3) & 7, lx = v & 7;
            sd[((lz + 1) * MGC_GEO_EDGE + ly + 1) * MGC_GEO_EDGE + lx + 1] = now[i] = next[i];
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
        if (!owned[i] || !(now[i] < first[i])) continue;
        const int v = t0 + i * NT, lz = v >> 6, ly = (v >> 3) & 7, lx = v & 7;
        dev.store(plane + ((z0 + 1 + lz) * L.dy + (y0 + 1 + ly)) * L.dx + (x0 + 1 + lx), now[i]);
        mgc_geo_wake_cell<DOCTOR>(lz, ly, lx, FULL, wake);
    }
    if (t0 == 0 && more && !(DOCTOR & MGC_GEO_NO_SELF_WAKE)) wake[MGC_GEO_SELF] = 1;
    dev.sync();
    for (int k = t0; k < 27; k += NT) {
        if (!wake[k]) continue;
        const int t = mgc_geo_tile_at(L, tz, ty, tx, k);
        if (t >= 0) dev.wake(t);
    }
    if (t0 == 0) dev.visited(sweeps, more != 0);
    dev.sync(); /* (the next visit of these workers rewrites the arrays) */
}

/* the regional term of one voxel from its two distances: t = fl(df + db); both infinite: nothing; one infinite: all of lam to the
 * side that is reached; t == 0: half each; else S = fl(lam * fl(db / t)), K = fl(lam * fl(df / t)) */
MGC_HD void mgc_geo_term(double df, double db, double lam, double* s, double* k)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const bool fi = df == MGC_EDT_INF, bi = db == MGC_EDT_INF;
    if (fi || bi) {
        *s = (bi && !fi) ? lam : 0.0;
        *k = (fi && !bi) ? lam : 0.0;
        return;
    }
    const double t = df + db;
    if (t == 0.0) {
        const double half = lam * 0.5;
        *s = *k = half;
        return;
    }
    const double qs = db / t;
    const double qk = df / t;
    const double vs = lam * qs;
    const double vk = lam * qk;
    *s = vs;
    *k = vk;
}

#endif /* MGC_GEO_H */
