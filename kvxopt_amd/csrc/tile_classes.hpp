// Numbering of the workgroups of a trailing-update launch over size classes of fronts (TileClasses, device.hpp) and the tile
// guard of the trailing-update kernels.  One copy for the kernels (kernels_big.hip) and the host: make_tile_classes builds the
// class table a launch passes by value, and kvx_dbg_tile_cover walks every workgroup id of a launch through the same decode and
// guard on the CPU (tests/test_tile_classes.py).
#pragma once
#include "device.hpp"
#include <algorithm>
#include <climits>

namespace kvx {

// Numbering of the workgroups of one launch.  A launch updates every big front of a level that is still in the chain; their
// trailing matrices differ by an order of magnitude, and a (tiles of the largest front) x (fronts) grid is mostly workgroups
// that find nothing to do -- the dispatcher starts one per ~2.6 ns, and the bottom levels of the 21-point system launched
// 870 000 of them per step for 30 000 tiles of work (2.3 ms, measured).  The host therefore hands the kernel the fronts sorted
// by size and cut into classes of similar tile counts; a class is a (tiles of ITS largest front) x (its fronts) block of
// consecutive workgroup ids.
// tile t of a front -> (ti, tj).  Triangular classes of 16 or more tile rows: the 8 XCDs (workgroup ids go round-robin over them,
// each has its own L2) take contiguous eighths of the row-major tile order, so that the workgroups resident on one XCD work on
// neighbouring tiles of a few tile rows and share their operand strips.
__host__ __device__ __forceinline__ unsigned cls_tiles_per_front(int T, int TC)
{
    if (TC > 0) return (unsigned)T * (unsigned)TC;
    const unsigned tri = (unsigned)T * (unsigned)(T + 1) / 2;
    return T >= 16 ? ((tri + 7) / 8) * 8 : tri;
}

// row-major index L of the lower tile triangle -> (ti, tj)
__host__ __device__ __forceinline__ void tri_inv(unsigned L, int &ti, int &tj)
{
    unsigned si = (unsigned)((__builtin_sqrtf(8.0f * (float)L + 1.0f) - 1.0f) * 0.5f);
    while ((si + 1) * (si + 2) / 2 <= L) si++;
    while (si * (si + 1) / 2 > L) si--;
    ti = (int)si;
    tj = (int)(L - si * (si + 1) / 2);
}

// workgroup id -> front index in the launch's list and tile (ti, tj).  false: nothing to do.
__host__ __device__ __forceinline__ bool cls_decode(const TileClasses &tc, const unsigned wgid, int &fi, int &ti, int &tj)
{
    int c = 0;
    while (c + 1 < tc.ncls && wgid >= tc.wg[c + 1]) c++;                   // (uniform)
    const unsigned local = wgid - tc.wg[c];
    const int T = tc.T[c], TC = tc.TC[c];
    if (TC > 0) {                                      // a few tile columns of T tile rows (column-limited launches)
        const unsigned tpf = (unsigned)T * (unsigned)TC;
        const unsigned t = local % tpf;
        fi = tc.first[c] + (int)(local / tpf);
        ti = (int)(t % (unsigned)T);
        tj = (int)(t / (unsigned)T);
    } else {
        const unsigned tri = (unsigned)T * (unsigned)(T + 1) / 2;
        if (T >= 16) {
            const unsigned chunk = (tri + 7) / 8, tpf = 8 * chunk;
            const unsigned t = local % tpf;
            fi = tc.first[c] + (int)(local / tpf);
            const unsigned L = (t & 7u) * chunk + (t >> 3);
            if (L >= tri) return false;
            tri_inv(L, ti, tj);
        } else {
            fi = tc.first[c] + (int)(local / tri);
            tri_inv(local % tri, ti, tj);
        }
    }
    // the ids in the padding in front of an XCD-numbered class decode into the class before it, past its last front: bounded by
    // the class, not by the launch (the next class's own workgroups do those tiles)
    return tj <= ti && fi < tc.first[c + 1];
}

// The tile (ti, tj) of a front of order m with k pivot columns in a trailing update with the panel columns [kb, kb + klen):
// the update region is rows and columns >= t0, lower triangle, columns < cend (see k_syrk_lds for UONLY and col_lim).
// false: the tile lies outside the region (or the front has no column in the K range) and its workgroup exits.
struct SyrkTile { int nbk, t0, r0, c0, cend; };
__host__ __device__ __forceinline__ bool syrk_tile_guard(bool uonly, int m, int k, int kb, int klen, int col_lim, int ti, int tj,
                                                         SyrkTile &g)
{
    if (kb >= k) return false;
    g.nbk = klen < k - kb ? klen : k - kb;
    g.t0 = uonly ? (col_lim < k ? col_lim : k) : kb + g.nbk;
    g.r0 = g.t0 + KVX_TILE * ti;
    g.c0 = g.t0 + KVX_TILE * tj;
    if (g.r0 >= m) return false;
    g.cend = (uonly || col_lim == INT_MAX) ? m : (col_lim < k ? col_lim : k);
    return g.c0 < g.cend;
}

// Size classes of a launch.  hm / hk: order and pivot columns of the fronts in list order (host copies; the list is sorted by the
// order of the update region, largest first, so classes are runs of the list).  A class ends where the tile count of the next
// front falls below ~0.7 of the class's largest, or rises above it.
inline TileClasses make_tile_classes(bool uonly, const int32_t *hm, const int32_t *hk, int count, int kb, int klen, int col_lim)
{
    TileClasses tc;
    int c = -1;
    for (int i = 0; i < count; i++) {
        const int m = hm[i], k = hk[i];
        int R = 0, C = 0;
        if (kb < k) {
            const int t0 = uonly ? std::min(col_lim, k) : kb + std::min(klen, k - kb);
            const int cend = (uonly || col_lim == INT_MAX) ? m : std::min(col_lim, k);
            R = std::max(m - t0, 0);
            C = std::max(cend - t0, 0);
        }
        const int T = (R + KVX_TILE - 1) / KVX_TILE, TCf = (C + KVX_TILE - 1) / KVX_TILE;
        if (c == KVX_MAXCLS - 1) {                     // out of classes: the last one takes the rest, whatever its sizes
            tc.T[c] = std::max(tc.T[c], T);
            tc.TC[c] = std::max(tc.TC[c], TCf);
            continue;
        }
        if (c >= 0 && T <= tc.T[c] && T * 10 >= tc.T[c] * 7) {
            tc.TC[c] = std::max(tc.TC[c], TCf);
            continue;
        }
        c++;
        tc.first[c] = i;
        tc.T[c] = T;
        tc.TC[c] = TCf;
    }
    tc.ncls = c + 1;
    tc.wg[0] = 0;
    tc.first[tc.ncls] = count;
    for (int q = 0; q < tc.ncls; q++) {
        const int T = tc.T[q];
        if (tc.TC[q] * 2 >= T) tc.TC[q] = 0;           // rectangular numbering only where it saves at least half of the workgroups
        unsigned w0 = tc.wg[q];
        if (tc.TC[q] == 0 && T >= 16) w0 = (w0 + 7u) & ~7u;                   // XCD numbering: the class starts on XCD 0
        tc.wg[q] = w0;
        tc.wg[q + 1] = w0 + (T > 0 ? cls_tiles_per_front(T, tc.TC[q]) : 0u) * (unsigned)(tc.first[q + 1] - tc.first[q]);
    }
    return tc;
}

}  // namespace kvx
