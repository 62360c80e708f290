/*
 * mgc_cc.h -- the connected components of a label plane on the lattice (mgc_components, mgc_clean_labels), stated once.
 *
 * Three planes in C order carry a call: parent (uint32 voxel ids, MGC_CC_NONE = "not of this side"), count (uint32) and flags
 * (uint8).  The steps, each a kernel boundary on the device:
 *
 *   mgc_cc_tile_step      one tile: label propagation in on-chip memory.  Afterwards every voxel's parent is the smallest voxel id of its
 *                         in-tile component, the LOCAL ROOT; local roots carry the in-tile component's size and flag byte, every
 *                         other voxel a count of 0 (count != 0 is what marks a local root from here on)
 *   mgc_cc_merge_voxel    every neighbour pair that crosses a tile border is met once, from its lower tile: mgc_cc_union
 *   mgc_cc_flatten_voxel  parent := global root
 *   mgc_cc_gather_voxel   local roots that are not global roots add their count and flags to their global root
 *
 * Everything is MGC_HD over (first index, stride, barrier) and an ATOM policy that says how a word shared between workgroups is
 * read and linked: the kernels of mgc_cc_ops.inl pass agent-scope atomics, the stand-alone host program of the CPU test tier
 * (tests/hostsim/cc_main.cpp) plain loads and stores.  Only mgc_common.h is needed on the host.
 */
#ifndef MGC_CC_H
#define MGC_CC_H

#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "mgc_common.h"

#define MGC_CC_NONE 0xffffffffu   /* parent word of a voxel of the other side */
#define MGC_CC_MAX_VOXELS 0xffffffffll /* volumes of this many voxels or more are refused: parents are 32-bit */
#define MGC_CC_BLOCK 1000         /* the 10 x 10 x 10 cells around (and including) a tile: the halo cells are never of this side */
#define MGC_CC_LNONE 0xffffu      /* in-tile label of a cell that is not of this side */
#define MGC_CC_SEG 4096           /* voxels a wave ranks at a time: 64 rounds of 64 lanes */
/* flag bits of a component */
#define MGC_CC_FLAG_FG 1u
#define MGC_CC_FLAG_BG 2u
#define MGC_CC_FLAG_BORDER 4u
/* slots of out8 of mgc_components */
#define MGC_CC_K 0
#define MGC_CC_N_SIDE 1
#define MGC_CC_LARGEST_SIZE 2
#define MGC_CC_LARGEST_ID 3
#define MGC_CC_TILES_SKIPPED 4
#define MGC_CC_TILES_PROCESSED 5
#define MGC_CC_UNIONS 6
#define MGC_CC_LONGEST_WALK 7

/* the Atom of host code: one thread, nothing to order.  (Device: MgcCcAtomDev, mgc_cc_ops.inl.) */
struct MgcCcAtomHost {
    uint32_t load(const uint32_t* p) const { return *p; }
    void store(uint32_t* p, uint32_t v) const { *p = v; }
    uint32_t fetch_min(uint32_t* p, uint32_t v) const { const uint32_t old = *p; if (v < old) *p = v; return old; }
    void add(uint32_t* p, uint32_t v) const { *p += v; }
    void or_byte(uint8_t* base, uint32_t i, uint8_t f) const { base[i] |= f; }
    void chip_add(uint32_t* p, uint32_t v) const { *p += v; }
    void chip_or(uint32_t* p, uint32_t v) const { *p |= v; }
};

MGC_HD int mgc_cc_cell(int z, int y, int x) { return ((z + 1) * 10 + (y + 1)) * 10 + (x + 1); }
MGC_HD int mgc_cc_cell_local(int c) { return mgc_local(c / 100 - 1, (c / 10) % 10 - 1, c % 10 - 1); }

/* offset of neighbour d: face 0..5 (-x +x -y +y -z +z), full 0..25 ((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1) without the centre) */
template <bool FULL>
MGC_HD void mgc_cc_offset(int d, int& dz, int& dy, int& dx)
{
    if (!FULL) {
        dz = (d >> 1) == 2 ? ((d & 1) ? 1 : -1) : 0;
        dy = (d >> 1) == 1 ? ((d & 1) ? 1 : -1) : 0;
        dx = (d >> 1) == 0 ? ((d & 1) ? 1 : -1) : 0;
    } else {
        const int c = d < 13 ? d : d + 1;
        dz = c / 9 - 1;
        dy = (c / 3) % 3 - 1;
        dx = c % 3 - 1;
    }
}

/* the border bit of voxel (z, y, x): some coordinate is 0 or dim - 1 among the axes of extent > 1 (a volume of one voxel is all border) */
MGC_HD uint32_t mgc_cc_border(const MgcLattice& L, int64_t z, int64_t y, int64_t x)
{
    const bool b = (L.dz > 1 && (z == 0 || z == L.dz - 1)) || (L.dy > 1 && (y == 0 || y == L.dy - 1)) || (L.dx > 1 && (x == 0 || x == L.dx - 1));
    return (b || L.nvox == 1) ? MGC_CC_FLAG_BORDER : 0u;
}

/* The step of ONE tile, run by `nt` workers of which this is number t0; sync(v) is a barrier that tells whether any worker's
 * v is non-zero, sync.bits(v) one that returns the OR of the workers' v (three bits).  lab: MGC_CC_BLOCK cells, acc: 2 * MGC_TV
 * words, both shared by the workers.  plane: one byte per voxel in C order, any byte but 0 is foreground; side 1 takes the foreground, 0 the background.  hint: 0 = read the plane; 1 / 2 = the caller knows that every
 * voxel of the tile lies on the other side / on this side (the label summaries of the current cut) and the plane is not read.
 * fg / bg: the marker planes of the handle or NULL.  Padding voxels of a partial tile are never read and never written.
 *
 * A mixed tile is labelled by label propagation with pointer jumping: a cell's label is the cell index of a voxel of its own
 * in-tile component, never larger than its own; a sweep replaces it by the smallest label among itself, its neighbours and the
 * label of the cell its label names.  Labels only go down, so a worker may read a cell another one is lowering in the same sweep
 * (a stale value costs a sweep, never a wrong set), and the loop ends at the only fixpoint: every cell names the smallest cell
 * of its component.  Cell order is voxel-id order inside a tile, so that cell is the component's first voxel. */
template <bool FULL, class Atom, class Sync>
MGC_HD void mgc_cc_tile_step(const MgcLattice& L, const uint8_t* plane, int side, int hint, const uint8_t* fg, const uint8_t* bg, int tile, uint32_t* parent,
                             uint32_t* count, uint8_t* flags, uint16_t* lab, uint32_t* acc, int t0, int nt, Atom& at, Sync& sync)
{
    int tz, ty, tx;
    mgc_tile_coords(L, tile, tz, ty, tx);
    const int64_t z0 = (int64_t)tz * 8, y0 = (int64_t)ty * 8, x0 = (int64_t)tx * 8;
    uint32_t* const cnt = acc;
    uint32_t* const fl = acc + MGC_TV;
    int seen = 0; /* bit 0: a voxel of this side, bit 1: a voxel of the other side */
    for (int k = t0; k < MGC_CC_BLOCK; k += nt) {
        const int bz = k / 100 - 1, by = (k / 10) % 10 - 1, bx = k % 10 - 1;
        uint16_t l = MGC_CC_LNONE;
        if (bz >= 0 && bz < 8 && by >= 0 && by < 8 && bx >= 0 && bx < 8 && z0 + bz < L.dz && y0 + by < L.dy && x0 + bx < L.dx) {
            const int64_t id = ((z0 + bz) * L.dy + (y0 + by)) * L.dx + (x0 + bx);
            const bool mine = hint ? hint == 2 : ((plane[id] != 0) == (side != 0));
            if (mine) l = (uint16_t)k;
            seen |= mine ? 1 : 2;
        }
        lab[k] = l;
    }
    for (int v = t0; v < MGC_TV; v += nt) cnt[v] = fl[v] = 0u;
    seen = sync.bits(seen);
    if (!(seen & 1)) { /* wholly on the other side */
        for (int v = t0; v < MGC_TV; v += nt) {
            const int64_t z = z0 + (v >> 6), y = y0 + ((v >> 3) & 7), x = x0 + (v & 7);
            if (z >= L.dz || y >= L.dy || x >= L.dx) continue;
            const int64_t id = (z * L.dy + y) * L.dx + x;
            parent[id] = MGC_CC_NONE;
            count[id] = 0u;
        }
        return;
    }
    const bool solid = !(seen & 2); /* wholly on this side: the voxels of a tile inside the volume are a box, one component under either neighbourhood */
    if (!solid) {
        for (;;) {
            int changed = 0;
            for (int v = t0; v < MGC_TV; v += nt) {
                const int c = mgc_cc_cell(v >> 6, (v >> 3) & 7, v & 7);
                const uint16_t l = lab[c];
                if (l == MGC_CC_LNONE) continue;
                uint16_t m = l;
                for (int d = 0; d < (FULL ? 26 : 6); ++d) {
                    int dz, dy, dx;
                    mgc_cc_offset<FULL>(d, dz, dy, dx);
                    const uint16_t n = lab[c + (dz * 10 + dy) * 10 + dx];
                    if (n < m) m = n;
                }
                const uint16_t j = lab[m];
                if (j < m) m = j;
                if (m < l) {
                    lab[c] = m;
                    changed = 1;
                }
            }
            if (!sync(changed)) break;
        }
    }
    /* sizes and flag bytes of the in-tile components: on chip */
    uint32_t mine_flags = 0u;
    for (int v = t0; v < MGC_TV; v += nt) {
        const int64_t z = z0 + (v >> 6), y = y0 + ((v >> 3) & 7), x = x0 + (v & 7);
        if (z >= L.dz || y >= L.dy || x >= L.dx) continue;
        const uint16_t l = lab[mgc_cc_cell(v >> 6, (v >> 3) & 7, v & 7)];
        if (l == MGC_CC_LNONE) continue;
        const int64_t id = (z * L.dy + y) * L.dx + x;
        const uint32_t f = mgc_cc_border(L, z, y, x) | (fg && fg[id] ? MGC_CC_FLAG_FG : 0u) | (bg && bg[id] ? MGC_CC_FLAG_BG : 0u);
        if (solid) {
            mine_flags |= f;
        } else {
            const int r = mgc_cc_cell_local(l);
            at.chip_add(cnt + r, 1u);
            if (f) at.chip_or(fl + r, f);
        }
    }
    if (solid) {
        /* (every worker may hold voxels: the flags come through the barrier, the count is the box's) */
        const uint32_t all_flags = (uint32_t)sync.bits((int)mine_flags);
        const int64_t nz = L.dz - z0 < 8 ? L.dz - z0 : 8, ny = L.dy - y0 < 8 ? L.dy - y0 : 8, nx = L.dx - x0 < 8 ? L.dx - x0 : 8;
        if (t0 == 0) {
            cnt[0] = (uint32_t)(nz * ny * nx);
            fl[0] = all_flags;
        }
    }
    sync(0);
    for (int v = t0; v < MGC_TV; v += nt) {
        const int64_t z = z0 + (v >> 6), y = y0 + ((v >> 3) & 7), x = x0 + (v & 7);
        if (z >= L.dz || y >= L.dy || x >= L.dx) continue;
        const int64_t id = (z * L.dy + y) * L.dx + x;
        const uint16_t l = lab[mgc_cc_cell(v >> 6, (v >> 3) & 7, v & 7)];
        if (l == MGC_CC_LNONE) {
            parent[id] = MGC_CC_NONE;
            count[id] = 0u;
            continue;
        }
        const int r = solid ? 0 : mgc_cc_cell_local(l);
        parent[id] = (uint32_t)(((z0 + (r >> 6)) * L.dy + (y0 + ((r >> 3) & 7))) * L.dx + (x0 + (r & 7)));
        count[id] = r == v ? cnt[v] : 0u;
        if (r == v) flags[id] = (uint8_t)fl[v];
    }
}

/* The root of v.  Parents only ever DECREASE: a parent word is written by the tile step (the smallest id of the in-tile component,
 * at most the voxel's own), by fetch_min (a minimum), and by the flattening (a root of the voxel's set, hence at most every
 * ancestor).  A walk steps to strictly smaller ids until it meets a word that names itself, so it ends; a value read late -- another
 * workgroup lowered the word meanwhile -- is still an ancestor and only makes the walk longer. */
template <class Atom>
MGC_HD uint32_t mgc_cc_find(uint32_t* parent, uint32_t v, Atom& at, uint32_t& walk)
{
    for (uint32_t steps = 0;; ++steps) {
        const uint32_t p = at.load(parent + v);
        if (p == v) {
            if (steps > walk) walk = steps;
            return v;
        }
        v = p;
    }
}

/* Join the sets of a and b, lock-free.  The larger root goes under the smaller by fetch_min on its parent word, and the value the
 * fetch_min returns is the truth: if it is not the root itself, somebody linked that voxel first.  Its word now names min(old, b),
 * so the link to `old` may have been replaced -- the loop goes on to join old and b, which restores it.  Termination: every retry
 * continues from (old, b) with old < a, so the sum of the two ids falls; with the walks (mgc_cc_find) that is all the waiting there
 * is.  No workgroup waits for another. */
template <class Atom>
MGC_HD void mgc_cc_union(uint32_t* parent, uint32_t a, uint32_t b, Atom& at, uint32_t& walk)
{
    for (;;) {
        a = mgc_cc_find(parent, a, at, walk);
        b = mgc_cc_find(parent, b, at, walk);
        if (a == b) return;
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        const uint32_t old = at.fetch_min(parent + a, b);
        if (old == a) return;
        a = old;
    }
}

/* The cross-tile pairs of local voxel v of tile (tz, ty, tx): v = a against b = a + d for the FORWARD offsets d ((dz, dy, dx) > 0
 * in that order: 3 at face, 13 at full), where b lies in another tile -- a later one, so each pair is met once, from its lower tile.
 * Two kinds of pair are left out before the union, both joined by others:
 *   - (full) a diagonal pair with a voxel of this side BETWEEN the two -- c = a + part of d: a ~ c and c ~ b are neighbour pairs with
 *     fewer non-zero offsets, met in a tile step or here; face pairs are never left out, so the argument ends there;
 *   - a pair whose predecessor along an axis that d does not move on (x before y before z; inside the same two tiles) reads the same
 *     two parent words: a' and a share a parent, b' and b do, and the predecessor joins them or leaves that to ITS predecessor; the
 *     first pair of a run has none.  A face of a solid ball costs one union this way. */
template <bool FULL, class Atom>
MGC_HD void mgc_cc_merge_voxel(const MgcLattice& L, uint32_t* parent, int tz, int ty, int tx, int v, Atom& at, uint32_t& unions, uint32_t& walk)
{
    const int lz = v >> 6, ly = (v >> 3) & 7, lx = v & 7;
    if (lz > 0 && lz < 7 && ly > 0 && ly < 7 && lx > 0 && lx < 7) return;
    const int64_t z = (int64_t)tz * 8 + lz, y = (int64_t)ty * 8 + ly, x = (int64_t)tx * 8 + lx;
    if (z >= L.dz || y >= L.dy || x >= L.dx) return;
    const int64_t sz = L.dy * L.dx, sy = L.dx;
    const int64_t a = z * sz + y * sy + x;
    const uint32_t pa = at.load(parent + a);
    if (pa == MGC_CC_NONE) return;
    for (int c = 14; c < 27; ++c) {
        const int dz = c / 9 - 1, dy = (c / 3) % 3 - 1, dx = c % 3 - 1;
        const int nonzero = (dz != 0) + (dy != 0) + (dx != 0);
        if (!FULL && nonzero != 1) continue;
        const int mz = lz + dz, my = ly + dy, mx = lx + dx;
        if (mz >= 0 && mz < 8 && my >= 0 && my < 8 && mx >= 0 && mx < 8) continue; /* the same tile: joined by its step */
        if (z + dz >= L.dz || y + dy < 0 || y + dy >= L.dy || x + dx < 0 || x + dx >= L.dx) continue;
        const int64_t off = dz * sz + dy * sy + dx;
        const uint32_t pb = at.load(parent + a + off);
        if (pb == MGC_CC_NONE) continue;
        if (nonzero > 1) {
            bool between = false;
            for (int m = 1; m < 7 && !between; ++m) { /* bit 2: z, bit 1: y, bit 0: x */
                const int cz = (m & 4) ? dz : 0, cy = (m & 2) ? dy : 0, cx = (m & 1) ? dx : 0;
                if (((m & 4) && !dz) || ((m & 2) && !dy) || ((m & 1) && !dx)) continue; /* moves on an axis d does not */
                if (cz == dz && cy == dy && cx == dx) continue;                          /* b itself */
                between = at.load(parent + a + cz * sz + cy * sy + cx) != MGC_CC_NONE;
            }
            if (between) continue;
        }
        int64_t back = 0; /* the step to the predecessor of the pair, 0: none */
        if (!dx && lx > 0) back = 1;
        else if (!dy && ly > 0 && (dx || lx == 0)) back = sy;
        else if (!dz && lz > 0 && (dx || lx == 0) && (dy || ly == 0)) back = sz;
        if (back) {
            const uint32_t qa = at.load(parent + a - back);
            if (qa == pa && at.load(parent + a + off - back) == pb) continue;
        }
        ++unions;
        mgc_cc_union(parent, pa, pb, at, walk);
    }
}

/* parent[v] := the root of v.  Other workers compress at the same time: what they store is a root of the voxel's set, an ancestor
 * of everything on the way, so a walk through a word that changes under it still ends at the root. */
template <class Atom>
MGC_HD void mgc_cc_flatten_voxel(uint32_t* parent, uint32_t v, Atom& at, uint32_t& walk)
{
    const uint32_t p = at.load(parent + v);
    if (p == MGC_CC_NONE || p == v) return;
    const uint32_t r = mgc_cc_find(parent, p, at, walk);
    if (r != p) at.store(parent + v, r);
}

/* After the flattening: a local root (count != 0) that is not its own global root adds its count and flags to the root's words.
 * Global roots are local roots too (the first voxel of a component is the first of its in-tile part) and only ever targets; the
 * sources are never written: one count plane serves.  One atomic pair per in-tile component. */
template <class Atom>
MGC_HD void mgc_cc_gather_voxel(const uint32_t* parent, uint32_t* count, uint8_t* flags, uint32_t v, Atom& at)
{
    const uint32_t c = count[v];
    if (!c) return;
    const uint32_t r = parent[v];
    if (r == v) return;
    at.add(count + r, c);
    if (flags[v]) at.or_byte(flags, r, flags[v]);
}

/* Step 1 of the cleaning rule on the table of the K foreground components (host code): a component PASSES with at least min_size voxels
 * and, if seeded, a foreground marker; with largest > 0 only the `largest` biggest of the passing survive, ties on size to the smaller
 * id.  keep[k] (K bytes, zeroed by the caller) = 1 for the survivors; *removed = the voxels of the others. */
static inline void mgc_cc_rule_keep(int64_t K, const int64_t* size, const uint8_t* flags, int64_t min_size, int64_t largest, int seeded, uint8_t* keep, int64_t* survivors,
                                    int64_t* removed)
{
    std::vector<std::pair<int64_t, int64_t>> pass; /* (-size, id): ascending = biggest first, ties to the smaller id */
    for (int64_t k = 0; k < K; ++k)
        if (size[k] >= min_size && (!seeded || (flags[k] & MGC_CC_FLAG_FG))) pass.push_back({-size[k], k});
    if (largest > 0 && (uint64_t)largest < pass.size()) {
        std::partial_sort(pass.begin(), pass.begin() + largest, pass.end());
        pass.resize((size_t)largest);
    }
    *survivors = (int64_t)pass.size();
    for (const auto& p : pass) keep[p.second] = 1;
    *removed = 0;
    for (int64_t k = 0; k < K; ++k)
        if (!keep[k]) *removed += size[k];
}

#endif /* MGC_CC_H */
