// Host side of the local (nearest-neighbour) prediction, seam S3l of include/tgp.h: the whitening factor of the metric and the
// uniform bucket grid over the whitened training points, sorted by cell with a counting sort.  Plain C++ with no HIP in it:
// local.hip includes it, and tests/sanitize/local_grid_driver.cpp compiles it alone under AddressSanitizer + UBSan.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>
#include "../../include/tgp.h"

// "Nearest" is measured on u = R x with R^T R = invLam (ARBF / AVK), R upper triangular: u0 = r00 x + r01 y, u1 = r11 y;
// R = I for the isotropic kinds (every isotropic scale gives the same order).  0 = ok, -1 = invLam has no Cholesky factor
// (not positive definite, or NaN), -2 = unknown kind.
struct LocalWhiten {
    double r00, r01, r11;
};
inline int local_whiten_factor(const tgp_kernel *k, LocalWhiten *R) {
    R->r00 = 1.0; R->r01 = 0.0; R->r11 = 1.0;
    if (k->kind == TGP_RBF || k->kind == TGP_VK) return 0;
    if (k->kind != TGP_ARBF && k->kind != TGP_AVK) return -2;
    if (!(k->a > 0.0) || !std::isfinite(k->a)) return -1;
    const double r00 = std::sqrt(k->a), r01 = k->b / r00, s = k->c - r01 * r01;
    if (!(s > 0.0) || !std::isfinite(s)) return -1;
    R->r00 = r00; R->r01 = r01; R->r11 = std::sqrt(s);
    return 0;
}
inline void local_whiten_point(const LocalWhiten &R, double x, double y, double *u0, double *u1) {
    const double t = R.r01 * y;             // two roundings, never one fused one: host and tests agree to the bit
    *u0 = R.r00 * x + t;
    *u1 = R.r11 * y;
}

// The grid: gx x gy cells of hx x hy over [lox, hix] x [loy, hiy], the bounding box of the finite whitened coordinates.
// cell(u) below is THE assignment, for training rows and queries alike, and it is monotone in u; an axis of zero (or
// non-finite) extent has one cell.
struct LocalGrid {
    double lox, loy, hix, hiy, hx, hy, inv_hx, inv_hy;
    int32_t gx, gy;
};
// NaN-safe: a NaN (or -inf) goes to cell 0, +inf to the last cell; never undefined behaviour in the conversion.  The search
// kernel calls this very function for the query's cell.
#ifdef __HIPCC__
__host__ __device__
#endif
inline int32_t local_cell_axis(double u, double lo, double inv_h, int32_t g) {
    const double t = (u - lo) * inv_h;
    if (!(t >= 1.0)) return 0;
    if (t >= (double)g) return g - 1;
    return (int32_t)t;
}

// occ: the mean occupancy aimed at (of the order of k / 4).  At most min(2 n + 1, 2^30) cells.
inline void local_grid_plan(const double *X, int64_t n, const LocalWhiten &R, int occ, LocalGrid *g) {
    const double inf = std::numeric_limits<double>::infinity();
    double lox = inf, loy = inf, hix = -inf, hiy = -inf;
    for (int64_t i = 0; i < n; ++i) {
        double u0, u1;
        local_whiten_point(R, X[2 * i], X[2 * i + 1], &u0, &u1);
        if (std::isfinite(u0)) { if (u0 < lox) lox = u0; if (u0 > hix) hix = u0; }
        if (std::isfinite(u1)) { if (u1 < loy) loy = u1; if (u1 > hiy) hiy = u1; }
    }
    if (!(lox <= hix)) lox = hix = 0.0;       // no finite coordinate at all
    if (!(loy <= hiy)) loy = hiy = 0.0;
    double wx = hix - lox, wy = hiy - loy;
    if (!(wx > 0.0) || !std::isfinite(wx)) wx = 0.0;
    if (!(wy > 0.0) || !std::isfinite(wy)) wy = 0.0;
    if (occ < 1) occ = 1;
    const double want = (double)n / (double)occ;       // cells aimed at
    double fx = 1.0, fy = 1.0;
    if (wx > 0.0 && wy > 0.0) {
        const double h = std::sqrt(wx / want * wy);    // square cells of area (wx wy) / want
        fx = std::ceil(wx / h);
        fy = std::ceil(wy / h);
    } else if (wx > 0.0) {
        fx = std::ceil(want);
    } else if (wy > 0.0) {
        fy = std::ceil(want);
    }
    const double cap = n < ((int64_t)1 << 29) ? 2.0 * (double)n + 1.0 : 1073741824.0;      // cell ids and counts stay int32
    if (!(fx >= 1.0)) fx = 1.0;                        // (also a NaN from an overflowing product)
    if (!(fy >= 1.0)) fy = 1.0;
    if (fx > cap) fx = cap;
    if (fy > cap) fy = cap;
    while (fx * fy > cap) {                            // an extreme aspect ratio: coarsen the finer axis
        if (fx >= fy) fx = std::ceil(fx / 2.0); else fy = std::ceil(fy / 2.0);
    }
    g->gx = (int32_t)fx; g->gy = (int32_t)fy;
    g->lox = lox; g->loy = loy; g->hix = hix; g->hiy = hiy;
    g->hx = wx > 0.0 ? wx / (double)g->gx : 0.0;
    g->hy = wy > 0.0 ? wy / (double)g->gy : 0.0;
    g->inv_hx = g->hx > 0.0 ? 1.0 / g->hx : 0.0;
    g->inv_hy = g->hy > 0.0 ? 1.0 / g->hy : 0.0;
    if (!std::isfinite(g->inv_hx)) { g->inv_hx = 0.0; g->hx = 0.0; g->gx = 1; }
    if (!std::isfinite(g->inv_hy)) { g->inv_hy = 0.0; g->hy = 0.0; g->gy = 1; }
}
inline int64_t local_grid_cells(const LocalGrid &g) { return (int64_t)g.gx * (int64_t)g.gy; }
inline int32_t local_cell(const LocalGrid &g, double u0, double u1) {
    return local_cell_axis(u1, g.loy, g.inv_hy, g.gy) * g.gx + local_cell_axis(u0, g.lox, g.inv_hx, g.gx);
}

// Counting sort of the rows by cell (stable: rows of a cell stay in row order).  U (n, 2): the whitened coordinates in sorted
// order; perm (n): the original row of each sorted row; cell_start (cells + 1): sorted rows [cell_start[c], cell_start[c + 1])
// lie in cell c.  n < 2^31.
inline void local_grid_sort(const double *X, int64_t n, const LocalWhiten &R, const LocalGrid &g, double *U, int32_t *perm,
                            int32_t *cell_start) {
    const int64_t nc = local_grid_cells(g);
    for (int64_t c = 0; c <= nc; ++c) cell_start[c] = 0;
    for (int64_t i = 0; i < n; ++i) {
        double u0, u1;
        local_whiten_point(R, X[2 * i], X[2 * i + 1], &u0, &u1);
        ++cell_start[(int64_t)local_cell(g, u0, u1) + 1];
    }
    for (int64_t c = 0; c < nc; ++c) cell_start[c + 1] += cell_start[c];      // cell_start[c + 1] = end of cell c
    // scatter from the last row down, each cell filled from its end: cell_start[c + 1] walks back to the start of cell c
    for (int64_t i = n - 1; i >= 0; --i) {
        double u0, u1;
        local_whiten_point(R, X[2 * i], X[2 * i + 1], &u0, &u1);
        const int64_t c = local_cell(g, u0, u1);
        const int32_t s = --cell_start[c + 1];
        U[2 * (int64_t)s] = u0;
        U[2 * (int64_t)s + 1] = u1;
        perm[s] = (int32_t)i;
    }
    // now cell_start[c + 1] = start of cell c: shift down by one place and close with n
    for (int64_t c = 0; c < nc; ++c) cell_start[c] = cell_start[c + 1];
    cell_start[nc] = (int32_t)n;
}

// ---- seam S3v: the host checks of the local conditionals (tests/sanitize/local_cond_driver.cpp compiles them alone) ------------
// rank (n) must be a permutation of 0 .. n - 1.  0 = it is; -1 = it is not, *bad = the first entry that is out of range or
// repeats an earlier one.  O(n).
inline int local_rank_check(const int32_t *rank, int64_t n, int64_t *bad) {
    std::vector<char> seen((size_t)n, 0);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t r = rank[i];
        if (r < 0 || r >= n || seen[(size_t)r]) { *bad = i; return -1; }
        seen[(size_t)r] = 1;
    }
    return 0;
}

// the ranks in the sorted-by-cell order of U: the search reads them beside the coordinates, not through perm
inline void local_rank_sorted(const int32_t *rank, const int32_t *perm, int64_t n, int32_t *rank_s) {
    for (int64_t s = 0; s < n; ++s) rank_s[s] = rank[perm[s]];
}

// Given lists nbr (rows [i0, i1) of an (n, kn) table): every entry a row of [0, n) other than the list's own, or a -1 of the
// padding that closes the list.  cnt[i - i0] = the length of list i.  0 = ok; otherwise *bad_row = the first bad list, *bad_at its
// first bad entry, and the return says why: -1 an entry outside [0, n), -2 the row itself, -3 an entry after a -1.
// A row repeated within a list is not looked for: its matrix is singular and the solve reports it.
inline int local_list_check(const int32_t *nbr, int64_t n, int kn, int64_t i0, int64_t i1, int32_t *cnt, int64_t *bad_row, int *bad_at) {
    for (int64_t i = i0; i < i1; ++i) {
        const int32_t *row = nbr + i * kn;
        int len = 0;
        while (len < kn && row[len] != -1) {
            const int64_t v = row[len];
            if (v < 0 || v >= n || v == i) { *bad_row = i; *bad_at = len; return v == i ? -2 : -1; }
            ++len;
        }
        for (int t = len; t < kn; ++t) {
            if (row[t] != -1) { *bad_row = i; *bad_at = t; return -3; }
        }
        cnt[i - i0] = len;
    }
    return 0;
}
