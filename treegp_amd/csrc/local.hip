// Local kriging (seam S3l of include/tgp.h): every query is conditioned on its k nearest training points alone.
//   host     the whitening factor of the metric and the bucket grid over the whitened training points (local_grid.h)
//   search   one query per 64-lane workgroup: cells in growing square rings around the query's cell, the k best (d^2, row)
//            in LDS, every batch of candidates merged by a bitonic sort of (best, batch)
//   solve    one query per workgroup: K_S, k* and y_S gathered into one LDS matrix of k + 2 rows, factorised in place with the two
//            right-hand sides carried along as rows, v.w and v.v reduced in a fixed order
// No N x N anything, no atomics; a query's bits depend on the training set, the kernel, k and its own coordinates only.
// Local conditionals (seam S3v): the same search and solve with every training row as its own query and a predicate on the
// candidate row (not the row itself: local leave-one-out; only rows earlier in an ordering: Vecchia's likelihood), then
//   terms    log s2 and r^2 / s2 of every row, written to device arrays
//   sums     reduced after the last chunk by a fixed tree over the row index: the bits do not depend on the chunk
#include "tgp_internal.h"
#include "kernel_eval.h"
#include "local_grid.h"

#include <chrono>
#include <climits>

namespace {

constexpr int LOCAL_KMAX = 128;
constexpr int64_t LOCAL_CHUNK_DEFAULT = 65536;

// ---- search ------------------------------------------------------------------------------------------------------------------
// (d2, row) pairs are ordered by distance, then by the ORIGINAL row index: the lower row wins a tie
__device__ __forceinline__ bool pair_after(double da, int ia, double db, int ib) { return da > db || (da == db && ia > ib); }

// Which rows of the table a query may take (seam S3v: the query is training row `self`).  The predicate joins the d2 <= kth test
// of the scan; the termination bound holds for every unexamined row, eligible or not, so the search stays exact.
enum { LS_ALL = 0, LS_NOT_SELF = 1, LS_EARLIER = 2 };
// LS_EARLIER: a row of rank r sees a fraction r / n of the table and needs about 25 n / r cells of rings, one dependent step per cell
// on the rings' sides; below r = n / LOCAL_SWEEP the whole table in one run of n / 64 coalesced steps is the shorter way (measured
// at n = 2^20: 1024 is the best of 128 .. 8192).  A row of rank below kn takes every predecessor: rings gain it nothing either.
constexpr int64_t LOCAL_SWEEP = 1024;

// S3v: query q of the chunk is training row q0 + q, and its list has min(kn, eligible rows) entries: n - 1 rows are eligible for
// LS_NOT_SELF, rank[q0 + q] of them for LS_EARLIER.  rank: the ranks in row order, a permutation of 0 .. n - 1; rank_s: the same
// ranks in the sorted-by-cell order of U, so that their read is as coalesced as U's and no gather through perm.
struct LocalCondArgs {
    int64_t q0, n;
    const int32_t *rank, *rank_s;
    int32_t *cnt;
    int32_t sweep_below;     // LS_EARLIER: rows of rank below this examine the whole table in one run
};

// KBB: capacity of the best list and of the batch (k <= KBB); P = 2 KBB entries are sorted at a merge.  MODE = LS_ALL (S3l) takes
// no further argument: its signature and its code are what they were before the modes.  The other modes take one LocalCondArgs;
// their k is worked out here and the k passed in is not looked at.
template <int KBB, int MODE = LS_ALL, class... Cond>
__global__ __launch_bounds__(64) void local_search_kernel(LocalGrid g, const double *__restrict__ U, const int32_t *__restrict__ perm,
                                                          const int32_t *__restrict__ cell_start, const double *__restrict__ Us,
                                                          int k, int kn, int32_t *__restrict__ nbr, Cond... cond) {
    static_assert(sizeof...(Cond) == (MODE == LS_ALL ? 0 : 1), "one LocalCondArgs for the modes of S3v, nothing for S3l");
    constexpr int P = 2 * KBB;
    __shared__ double bd[P];
    __shared__ int32_t bi[P];
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    const double inf = __builtin_huge_val();
    const double uqx = Us[2 * q], uqy = Us[2 * q + 1];
    [[maybe_unused]] int32_t self = 0, myrank = 0;
    [[maybe_unused]] bool sweep = false;
    [[maybe_unused]] const int32_t *rank_s = nullptr;
    if constexpr (MODE != LS_ALL) {
        const LocalCondArgs ca = (cond, ...);
        self = (int32_t)(ca.q0 + q);
        rank_s = ca.rank_s;
        if constexpr (MODE == LS_EARLIER) {
            myrank = ca.rank[self];
            k = myrank < kn ? myrank : kn;
            sweep = myrank < ca.sweep_below;
        } else {
            k = ca.n - 1 < (int64_t)kn ? (int)(ca.n - 1) : kn;
        }
        if (k < 1) {                                       // no eligible row at all (uniform): an empty list
            for (int t = lane; t < kn; t += 64) nbr[q * kn + t] = -1;
            if (lane == 0) ca.cnt[q] = 0;
            return;
        }
    }
    for (int t = lane; t < P; t += 64) { bd[t] = inf; bi[t] = INT_MAX; }
    double kth = inf;            // distance of the current k-th best (uniform)
    int count = 0;               // candidates waiting in the batch half (uniform)

    // (best, batch) -> sorted; the first KBB entries are the best again
    auto flush = [&]() {
        for (int t = KBB + count + lane; t < P; t += 64) { bd[t] = inf; bi[t] = INT_MAX; }
        for (int size = 2; size <= P; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                __syncthreads();
                for (int t = lane; t < P / 2; t += 64) {
                    const int lo = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), hi = lo + stride;
                    const bool asc = (lo & size) == 0;
                    const double da = bd[lo], db = bd[hi];
                    const int ia = bi[lo], ib = bi[hi];
                    if (pair_after(da, ia, db, ib) == asc) { bd[lo] = db; bi[lo] = ib; bd[hi] = da; bi[hi] = ia; }
                }
            }
        }
        __syncthreads();
        kth = bd[k - 1];
        count = 0;
    };
    // the sorted rows of cells [c0, c1] of one grid row are contiguous: 64 of them per step, one per lane
    auto scan = [&](int64_t c0, int64_t c1) {
        const int32_t s = cell_start[c0], e = cell_start[c1 + 1];
        for (int32_t base = s; base < e; base += 64) {
            const int32_t r = base + lane;
            bool pass = false;
            double d2 = inf;
            if (r < e) {
                const double dx = U[2 * (int64_t)r] - uqx, dy = U[2 * (int64_t)r + 1] - uqy;
                d2 = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
                if (d2 != d2) d2 = inf;                    // a NaN coordinate: last in every order
                pass = d2 <= kth;                          // not below the k-th best: skipped (a tie is decided by the sort)
                if constexpr (MODE == LS_EARLIER) pass = pass && rank_s[r] < myrank;
            }
            [[maybe_unused]] int32_t row = 0;
            if constexpr (MODE == LS_NOT_SELF) {
                if (pass) { row = perm[r]; pass = row != self; }
            }
            const unsigned long long mask = __ballot(pass);
            if (pass) {
                const int pos = KBB + count + __popcll(mask & ((1ull << lane) - 1ull));
                bd[pos] = d2;
                if constexpr (MODE == LS_NOT_SELF) bi[pos] = row; else bi[pos] = perm[r];
            }
            count += __popcll(mask);
            if (count > KBB - 64) flush();                 // the next step may add 64 more
        }
    };

    const int qcx = local_cell_axis(uqx, g.lox, g.inv_hx, g.gx), qcy = local_cell_axis(uqy, g.loy, g.inv_hy, g.gy);
    // rounding in cell(), in the faces and in d2 is a few ulps of the coordinates: the bound gives away 32 of them
    const double e32 = 32.0 * 2.220446049250313e-16;
    const double mx = e32 * (fabs(g.lox) + fabs(g.hix) + fabs(uqx)), my = e32 * (fabs(g.loy) + fabs(g.hiy) + fabs(uqy));
    const double dxo = fmax(fmax(g.lox - uqx, uqx - g.hix) - mx, 0.0);      // the query's distance to the bounding box, per axis
    const double dyo = fmax(fmax(g.loy - uqy, uqy - g.hiy) - my, 0.0);
    __syncthreads();
    for (int r = 0;; ++r) {
        if constexpr (MODE == LS_EARLIER) {
            if (sweep) {                                     // (uniform) every row of the table, in table order: exact as it stands
                scan(0, (int64_t)g.gx * g.gy - 1);
                if (count > 0) flush();
                break;
            }
        }
        const int x0 = qcx - r, x1 = qcx + r, y0 = qcy - r, y1 = qcy + r;
        const int cx0 = x0 > 0 ? x0 : 0, cx1 = x1 < g.gx - 1 ? x1 : g.gx - 1;
        const int cy0 = y0 > 0 ? y0 : 0, cy1 = y1 < g.gy - 1 ? y1 : g.gy - 1;
        for (int cy = cy0; cy <= cy1; ++cy) {                // the cells of ring r that lie on the grid
            const int64_t row = (int64_t)cy * g.gx;
            if (cy == y0 || cy == y1) {
                scan(row + cx0, row + cx1);
            } else {
                if (x0 >= 0) scan(row + x0, row + x0);
                if (x1 < g.gx) scan(row + x1, row + x1);
            }
        }
        if (count > 0) flush();
        if (cx0 == 0 && cx1 == g.gx - 1 && cy0 == 0 && cy1 == g.gy - 1) break;      // the block covers the grid
        // Termination.  A row outside the block [cx0, cx1] x [cy0, cy1] lies in a cell beyond one of the block's four faces, and
        // cell() is monotone in the coordinate: the row is at least that face's distance from the query along that axis and, being
        // inside the bounding box, at least the query's distance to the box along the other.  So every row not examined yet has
        // d2 >= b2, and once the k-th best is strictly below b2 no such row can enter the k best, ties included: the search is
        // exact.  A face on the edge of the grid has nothing beyond it (infinite distance).
        const double fxl = cx0 > 0 ? fmax(uqx - (g.lox + (double)cx0 * g.hx) - mx, 0.0) : inf;
        const double fxr = cx1 < g.gx - 1 ? fmax((g.lox + (double)(cx1 + 1) * g.hx) - uqx - mx, 0.0) : inf;
        const double fyl = cy0 > 0 ? fmax(uqy - (g.loy + (double)cy0 * g.hy) - my, 0.0) : inf;
        const double fyr = cy1 < g.gy - 1 ? fmax((g.loy + (double)(cy1 + 1) * g.hy) - uqy - my, 0.0) : inf;
        const double fx = fmin(fxl, fxr), fy = fmin(fyl, fyr);
        const double b2 = fmin(fx * fx + dyo * dyo, fy * fy + dxo * dxo);
        if (kth < b2 * (1.0 - 1e-14)) break;
    }
    if constexpr (MODE == LS_ALL) {
        for (int t = lane; t < kn; t += 64) nbr[q * kn + t] = t < k ? bi[t] : -1;      // nearest first
    } else {
        // A filler (INT_MAX: fewer eligible rows than k) would become -1 and not be counted.  Never taken: k = min(kn, eligible rows)
        // was worked out above and every eligible row is examined or bounded away, so cnt = k.  Kept as a guard.
        int have = 0;
        for (int t = lane; t < kn; t += 64) {
            const int32_t v = (t < k && bi[t] != INT_MAX) ? bi[t] : -1;
            nbr[q * kn + t] = v;
            have += v >= 0;
        }
        for (int off = 32; off > 0; off >>= 1) have += __shfl_xor(have, off);
        if (lane == 0) (cond, ...).cnt[q] = have;
    }
}

// ---- solve -------------------------------------------------------------------------------------------------------------------
// LDS image: A (KB + 2 rows of LD = KB + 1 doubles: the odd stride puts the 32 rows of a half wave on 32 different 8-byte banks in
// the column walks), the neighbours' x, y and yerr^2, and for the von Karman kinds the Chebyshev table.
constexpr int local_rows_pad(int KB) { return (KB + 2 + 63) / 64 * 64; }
constexpr size_t local_solve_lds(int KE, int KB) {
    return ((size_t)(KB + 2) * (KB + 1) + 3 * (size_t)KB + (KE == KE_GAUSS ? 0 : 6 * K56_NDEG)) * sizeof(double);
}

// Thread (i, g): row i of A (rows k and k + 1 are k* and y_S), columns c = g mod G of the trailing update.  Right-looking, one
// barrier per column: step j reads column j and the pivot d_j = A[j][j] (never overwritten) and writes columns > j only,
// A[i][c] -= (A[i][j] / l_j) (A[c][j] / l_j), l_j = sqrt(d_j).  Column j thereby holds l_j L[., j], and rows k, k + 1 end as
// l_c v_c and l_c w_c with v = L^-1 k*, w = L^-1 y_S.
// S3l passes no further argument (its signature and its code are what they were); S3v passes the lengths of the chunk's lists:
// the order of each workgroup's matrix is then cnt[workgroup] (0 .. kn; the bucket KB >= kn is the launch's) and the k passed in is
// not looked at.  Order 0 falls through every loop: ys = 0, var = amp.
template <int KE, int KB, int G, class... Cnt>
__global__ __launch_bounds__(G *local_rows_pad(KB)) void local_solve_kernel(KParams p, const double *__restrict__ X,
                                                                            const double *__restrict__ y, const double *__restrict__ e2,
                                                                            const double *__restrict__ Xs, const int32_t *__restrict__ nbr,
                                                                            int64_t n, int kn, int k, double *__restrict__ ys,
                                                                            double *__restrict__ var, int32_t *__restrict__ info,
                                                                            Cnt... cnt) {
    static_assert(sizeof...(Cnt) <= 1, "at most the list lengths");
    if constexpr (sizeof...(Cnt) == 1) {
        k = (cnt, ...)[blockIdx.x];
        if (k < 0 || k > kn) k = 0;                          // (never: the search and the list check write 0 .. kn)
    }
    extern __shared__ __attribute__((aligned(16))) double local_lds[];
    constexpr int LD = KB + 1, RB = local_rows_pad(KB), T = G * RB;
    double *A = local_lds, *sx = A + (KB + 2) * LD, *sy = sx + KB, *se = sy + KB, *tab = se + KB;
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    if constexpr (KE != KE_GAUSS) vonkarman_stage_table(tab);
    if (tid < k) {
        int64_t idx = nbr[q * kn + tid];
        if (idx < 0 || idx >= n) idx = 0;                    // (never: the search returns rows of the table)
        sx[tid] = X[2 * idx];
        sy[tid] = X[2 * idx + 1];
        se[tid] = e2 ? e2[idx] : 0.0;
        A[(k + 1) * LD + tid] = y[idx];
    }
    __syncthreads();
    const double xq = Xs[2 * q], yq = Xs[2 * q + 1];
    const int ntri = k * (k + 1) / 2;
    for (int t = tid; t < ntri + k; t += T) {
        if (t < ntri) {
            int64_t i, c;
            tri_index(t, i, c);
            A[i * LD + c] = (i == c) ? p.amp + se[i] : kernel_value_tab<KE>(p, sx[i] - sx[c], sy[i] - sy[c], tab);
        } else {
            const int c = t - ntri;
            A[k * LD + c] = kernel_value_tab<KE>(p, xq - sx[c], yq - sy[c], tab);
        }
    }
    const int g = tid / RB, i = tid - g * RB, rows = k + 2;
    int fail = 0;
    for (int j = 0; j < k; ++j) {
        __syncthreads();
        const double d = A[j * LD + j];
        if (!(d > 0.0)) { fail = j + 1; break; }             // the same value in every thread: a uniform exit
        if (i > j && i < rows) {
            const double inv = 1.0 / sqrt(d);
            const double li = A[i * LD + j] * inv;
            const int cmax = i < k ? i : k - 1;
            int c = j + 1;
            c += (g - c) & (G - 1);                          // the first column > j of this thread's class
            double *Ai = A + i * LD;
            const double *Aj = A + j;
            // four columns per round, their eight LDS reads in flight together: a round waits for LDS once, not four times
            for (; c + 3 * G <= cmax; c += 4 * G) {
                const double l0 = Aj[c * LD], l1 = Aj[(c + G) * LD], l2 = Aj[(c + 2 * G) * LD], l3 = Aj[(c + 3 * G) * LD];
                const double a0 = Ai[c], a1 = Ai[c + G], a2 = Ai[c + 2 * G], a3 = Ai[c + 3 * G];
                Ai[c] = fma(-li, l0 * inv, a0);
                Ai[c + G] = fma(-li, l1 * inv, a1);
                Ai[c + 2 * G] = fma(-li, l2 * inv, a2);
                Ai[c + 3 * G] = fma(-li, l3 * inv, a3);
            }
            for (; c <= cmax; c += G) Ai[c] = fma(-li, Aj[c * LD] * inv, Ai[c]);
        }
    }
    __syncthreads();
    if (tid < 64) {                                          // fixed order: lane l sums c = l, l + 64, then a butterfly
        double svw = 0.0, svv = 0.0;
        if (!fail) {
            for (int c = tid; c < k; c += 64) {
                const double inv = 1.0 / sqrt(A[c * LD + c]);
                const double v = A[k * LD + c] * inv, w = A[(k + 1) * LD + c] * inv;
                svw = fma(v, w, svw);
                svv = fma(v, v, svv);
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            svw += __shfl_xor(svw, off);
            svv += __shfl_xor(svv, off);
        }
        if (tid == 0) {
            const double nan = __builtin_nan("");
            ys[q] = fail ? nan : svw;
            if (var) var[q] = fail ? nan : p.amp - svv;
            info[q] = fail;
        }
    }
}

// ---- the terms of the sums and their reduction ------------------------------------------------------------------------------
// Row i = q0 + j of a chunk: s2 = var + yerr^2; T[0][i] = log s2, T[1][i] = (y_i - mu_i)^2 / s2, T[2][i] = 0 -- or 0, 0, 1 for a
// failed row.  T is (3, n): the reduction below reads it once every chunk has written its part.
__global__ __launch_bounds__(256) void local_terms_kernel(const double *__restrict__ mu, const double *__restrict__ var,
                                                          const int32_t *__restrict__ info, const double *__restrict__ y,
                                                          const double *__restrict__ e2, int64_t q0, int64_t cnt, int64_t n,
                                                          double *__restrict__ T) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= cnt) return;
    const int64_t i = q0 + j;
    double t0 = 0.0, t1 = 0.0, t2 = 1.0;
    if (info[j] == 0) {
        const double s2 = e2 ? __dadd_rn(var[j], e2[i]) : var[j];
        const double r = __dsub_rn(y[i], mu[j]);
        t0 = log(s2);
        t1 = __dmul_rn(r, r) / s2;
        t2 = 0.0;
    }
    T[i] = t0;
    T[n + i] = t1;
    T[2 * n + i] = t2;
}

// One level of a fixed tree over the index: block b of array a sums elements [1024 b, 1024 b + 1024) of in[a], thread t taking
// (e[t] + e[t + 256]) + (e[t + 512] + e[t + 768]) and the 256 threads a halving tree in LDS; elements past `count` are zeros.
// The host applies it until one element is left: two levels up to n = 2^20, the same tree whatever the chunks were.
__global__ __launch_bounds__(256) void local_reduce_kernel(const double *__restrict__ in, int64_t count, int64_t in_stride,
                                                           double *__restrict__ out, int64_t out_stride) {
    __shared__ double sh[256];
    const int t = threadIdx.x;
    const double *src = in + (int64_t)blockIdx.y * in_stride;
    const int64_t base = (int64_t)blockIdx.x * 1024 + t;
    const double e0 = base < count ? src[base] : 0.0, e1 = base + 256 < count ? src[base + 256] : 0.0;
    const double e2 = base + 512 < count ? src[base + 512] : 0.0, e3 = base + 768 < count ? src[base + 768] : 0.0;
    sh[t] = __dadd_rn(__dadd_rn(e0, e1), __dadd_rn(e2, e3));
    for (int half = 128; half > 0; half >>= 1) {
        __syncthreads();
        if (t < half) sh[t] = __dadd_rn(sh[t], sh[t + half]);
    }
    if (t == 0) out[(int64_t)blockIdx.y * out_stride + blockIdx.x] = sh[0];
}

// threads per row of the solve, per k bucket (powers of two; the bits do not depend on them: every element sees the same
// operations in the same order whichever thread applies them)
#ifndef TGP_LOCAL_G32
#define TGP_LOCAL_G32 2
#endif
#ifndef TGP_LOCAL_G64
#define TGP_LOCAL_G64 2
#endif
#ifndef TGP_LOCAL_G128
#define TGP_LOCAL_G128 2
#endif

template <int KE, int KB>
hipError_t run_solve(hipStream_t st, int64_t cnt, const KParams &p, const double *X, const double *y, const double *e2, const double *Xs,
                     const int32_t *nbr, int64_t n, int kn, int k, double *ys, double *var, int32_t *info) {
    constexpr int G = KB == 32 ? TGP_LOCAL_G32 : (KB == 64 ? TGP_LOCAL_G64 : TGP_LOCAL_G128);
    static_assert(G >= 1 && (G & (G - 1)) == 0 && G * local_rows_pad(KB) <= 1024, "threads per row: a power of two, at most 1024 threads");
    constexpr size_t lds = local_solve_lds(KE, KB);
    static const hipError_t attr = hipFuncSetAttribute((const void *)local_solve_kernel<KE, KB, G>,
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (attr != hipSuccess) return attr;
    local_solve_kernel<KE, KB, G><<<(unsigned)cnt, G * local_rows_pad(KB), lds, st>>>(p, X, y, e2, Xs, nbr, n, kn, k, ys, var, info);
    return hipGetLastError();
}
template <int KE>
hipError_t run_solve_k(hipStream_t st, int64_t cnt, const KParams &p, const double *X, const double *y, const double *e2,
                       const double *Xs, const int32_t *nbr, int64_t n, int kn, int k, double *ys, double *var, int32_t *info) {
    if (k <= 32) return run_solve<KE, 32>(st, cnt, p, X, y, e2, Xs, nbr, n, kn, k, ys, var, info);
    if (k <= 64) return run_solve<KE, 64>(st, cnt, p, X, y, e2, Xs, nbr, n, kn, k, ys, var, info);
    return run_solve<KE, 128>(st, cnt, p, X, y, e2, Xs, nbr, n, kn, k, ys, var, info);
}

struct Layout {              // one arena, the same offsets on the device and in the pinned host mirror
    size_t U, X, y, e2, perm, cells, tables_end, Xs, Us, ys, var, info, nbr, end;
};
Layout local_layout(int64_t n, int64_t nc, int64_t chunk, int kn) {
    Layout L;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += rup(bytes); return at; };
    L.U = take(16 * (size_t)n);
    L.X = take(16 * (size_t)n);
    L.y = take(8 * (size_t)n);
    L.e2 = take(8 * (size_t)n);
    L.perm = take(4 * (size_t)n);
    L.cells = take(4 * (size_t)(nc + 1));
    L.tables_end = off;
    L.Xs = take(16 * (size_t)chunk);
    L.Us = take(16 * (size_t)chunk);
    L.ys = take(8 * (size_t)chunk);
    L.var = take(8 * (size_t)chunk);
    L.info = take(4 * (size_t)chunk);
    L.nbr = take(4 * (size_t)chunk * (size_t)kn);
    L.end = off;
    return L;
}

template <int KE, int KB>
hipError_t run_cond_solve(hipStream_t st, int64_t cnt, const KParams &p, const double *X, const double *y, const double *e2,
                          const double *Xs, const int32_t *nbr, const int32_t *d_cnt, int64_t n, int kn, double *ys, double *var,
                          int32_t *info) {
    constexpr int G = KB == 32 ? TGP_LOCAL_G32 : (KB == 64 ? TGP_LOCAL_G64 : TGP_LOCAL_G128);
    constexpr size_t lds = local_solve_lds(KE, KB);
    static const hipError_t attr = hipFuncSetAttribute((const void *)local_solve_kernel<KE, KB, G, const int32_t *>,
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (attr != hipSuccess) return attr;
    local_solve_kernel<KE, KB, G, const int32_t *><<<(unsigned)cnt, G * local_rows_pad(KB), lds, st>>>(p, X, y, e2, Xs, nbr, n, kn, 0,
                                                                                                      ys, var, info, d_cnt);
    return hipGetLastError();
}
template <int KE>
hipError_t run_cond_solve_k(hipStream_t st, int64_t cnt, const KParams &p, const double *X, const double *y, const double *e2,
                            const double *Xs, const int32_t *nbr, const int32_t *d_cnt, int64_t n, int kn, double *ys, double *var,
                            int32_t *info) {
    if (kn <= 32) return run_cond_solve<KE, 32>(st, cnt, p, X, y, e2, Xs, nbr, d_cnt, n, kn, ys, var, info);      // the bucket: by kn
    if (kn <= 64) return run_cond_solve<KE, 64>(st, cnt, p, X, y, e2, Xs, nbr, d_cnt, n, kn, ys, var, info);
    return run_cond_solve<KE, 128>(st, cnt, p, X, y, e2, Xs, nbr, d_cnt, n, kn, ys, var, info);
}
template <int MODE>
void run_cond_search(hipStream_t st, int64_t cnt, const LocalGrid &g, const double *U, const int32_t *perm, const int32_t *cells,
                     const double *Us, int kn, int32_t *nbr, const LocalCondArgs &ca) {
    if (kn <= 64) local_search_kernel<64, MODE, LocalCondArgs><<<(unsigned)cnt, 64, 0, st>>>(g, U, perm, cells, Us, 0, kn, nbr, ca);
    else local_search_kernel<128, MODE, LocalCondArgs><<<(unsigned)cnt, 64, 0, st>>>(g, U, perm, cells, Us, 0, kn, nbr, ca);
}

struct CondLayout {          // S3v: the data, the search tables, the chunk buffers (mirrored in pinned host memory up to host_end),
    size_t X, y, e2, data_end, U, perm, cells, rank, rank_s, tables_end, Us, mu, var, info, cnt, nbr, sums, host_end, T, P0, P1, end;
};                           // then the terms and the partial sums of the reduction, which never leave the device
CondLayout cond_layout(int64_t n, int64_t nc, int64_t chunk, int kn) {
    CondLayout L;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += rup(bytes); return at; };
    L.X = take(16 * (size_t)n);
    L.y = take(8 * (size_t)n);
    L.e2 = take(8 * (size_t)n);
    L.data_end = off;
    L.U = take(16 * (size_t)n);
    L.perm = take(4 * (size_t)n);
    L.cells = take(4 * (size_t)(nc + 1));
    L.rank = take(4 * (size_t)n);
    L.rank_s = take(4 * (size_t)n);
    L.tables_end = off;
    L.Us = take(16 * (size_t)chunk);
    L.mu = take(8 * (size_t)chunk);
    L.var = take(8 * (size_t)chunk);
    L.info = take(4 * (size_t)chunk);
    L.cnt = take(4 * (size_t)chunk);
    L.nbr = take(4 * (size_t)chunk * (size_t)kn);
    L.sums = take(3 * sizeof(double));
    L.host_end = off;
    const size_t p0 = ((size_t)n + 1023) / 1024, p1 = (p0 + 1023) / 1024;
    L.T = take(24 * (size_t)n);
    L.P0 = take(24 * p0);
    L.P1 = take(24 * p1);
    L.end = off;
    return L;
}

}  // namespace

extern "C" int tgp_gp_predict_local(tgp_ctx *ctx, const tgp_kernel *k, const double *X, int64_t n, const double *y, const double *yerr,
                                    const double *Xs, int64_t m, int kn, double *ys, double *var, int32_t *nbr, int32_t *info) {
    if (!ctx) return -1;
    TGP_ARG(k && X && y && Xs && ys && info);
    TGP_ARG(n >= 1 && n < ((int64_t)1 << 31) && m >= 1);
    if (kn < 1 || kn > LOCAL_KMAX) {
        ctx->err = "tgp_gp_predict_local: kn = " + std::to_string(kn) + " is outside 1 .. " + std::to_string(LOCAL_KMAX);
        return -1;
    }
    const int ke = kind_to_ke(k->kind);
    if (ke < 0) {
        ctx->err = "tgp_gp_predict_local: unknown kernel kind " + std::to_string(k->kind);
        return -1;
    }
    LocalWhiten R;
    if (local_whiten_factor(k, &R) != 0) {
        ctx->err = "tgp_gp_predict_local: invLam [[a, b], [b, c]] = [[" + std::to_string(k->a) + ", " + std::to_string(k->b) + "], [" +
                   std::to_string(k->b) + ", " + std::to_string(k->c) + "]] has no Cholesky factor: the metric of the neighbour search "
                   "needs a positive definite one";
        return -1;
    }
    for (double &t : ctx->timings) t = 0.0;
    const int kk = (int64_t)kn < n ? kn : (int)n;
    const auto t0 = std::chrono::steady_clock::now();
    LocalGrid g;
    local_grid_plan(X, n, R, kk / 4 > 1 ? kk / 4 : 1, &g);
    const int64_t nc = local_grid_cells(g);
    int64_t chunk = LOCAL_CHUNK_DEFAULT;
    if (const char *e = getenv("TGP_LOCAL_CHUNK")) {          // read per call, as TGP_BATCH_CHUNK is
        if (atoll(e) > 0) chunk = atoll(e);
    }
    if (chunk > m) chunk = m;
    if (chunk > 0x7fffffff) chunk = 0x7fffffff;
    const Layout L = local_layout(n, nc, chunk, kn);
    TGP_HIP(hipSetDevice(ctx->device));
    if (L.end > ctx->scratch_bytes) {                          // O(n + chunk kn), checked before anything runs
        size_t fr = 0, tot = 0;
        TGP_HIP(hipMemGetInfo(&fr, &tot));
        if (L.end > fr + ctx->scratch_bytes) {
            ctx->err = "tgp_gp_predict_local: needs " + std::to_string(L.end) + " bytes of device memory (n = " + std::to_string(n) +
                       ", chunk = " + std::to_string(chunk) + " queries of kn = " + std::to_string(kn) + "), " +
                       std::to_string(fr + ctx->scratch_bytes) + " are free; lower TGP_LOCAL_CHUNK";
            return -2;
        }
    }
    int rc = tgp_ensure_scratch(ctx, L.end);
    if (rc) return rc;
    void *hp = nullptr;
    rc = tgp_ensure_pinned(ctx, L.end, &hp);
    if (rc) return rc;
    char *h = (char *)hp, *d = (char *)ctx->scratch;
    hipStream_t st = ctx->stream;

    local_grid_sort(X, n, R, g, (double *)(h + L.U), (int32_t *)(h + L.perm), (int32_t *)(h + L.cells));
    memcpy(h + L.X, X, 16 * (size_t)n);
    memcpy(h + L.y, y, 8 * (size_t)n);
    if (yerr) {
        double *e2 = (double *)(h + L.e2);
        for (int64_t i = 0; i < n; ++i) e2[i] = yerr[i] * yerr[i];
    }
    TGP_HIP(hipMemcpyAsync(d, h, L.tables_end, hipMemcpyHostToDevice, st));
    TGP_HIP(hipStreamSynchronize(st));
    ctx->timings[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

    const KParams p = make_kparams(k);
    const double *d_U = (const double *)(d + L.U), *d_X = (const double *)(d + L.X), *d_y = (const double *)(d + L.y);
    const double *d_e2 = yerr ? (const double *)(d + L.e2) : nullptr;
    const int32_t *d_perm = (const int32_t *)(d + L.perm), *d_cells = (const int32_t *)(d + L.cells);
    double *d_Xs = (double *)(d + L.Xs), *d_Us = (double *)(d + L.Us), *d_ys = (double *)(d + L.ys);
    double *d_var = var ? (double *)(d + L.var) : nullptr;
    int32_t *d_info = (int32_t *)(d + L.info), *d_nbr = (int32_t *)(d + L.nbr);
    for (int64_t q0 = 0; q0 < m; q0 += chunk) {
        const int64_t cnt = m - q0 < chunk ? m - q0 : chunk;
        memcpy(h + L.Xs, Xs + 2 * q0, 16 * (size_t)cnt);
        double *hu = (double *)(h + L.Us);
        for (int64_t j = 0; j < cnt; ++j) local_whiten_point(R, Xs[2 * (q0 + j)], Xs[2 * (q0 + j) + 1], hu + 2 * j, hu + 2 * j + 1);
        TGP_HIP(hipMemcpyAsync(d_Xs, h + L.Xs, 16 * (size_t)cnt, hipMemcpyHostToDevice, st));
        TGP_HIP(hipMemcpyAsync(d_Us, h + L.Us, 16 * (size_t)cnt, hipMemcpyHostToDevice, st));
        TGP_HIP(hipEventRecord(ctx->ev[0], st));
        if (kk <= 64) local_search_kernel<64><<<(unsigned)cnt, 64, 0, st>>>(g, d_U, d_perm, d_cells, d_Us, kk, kn, d_nbr);
        else local_search_kernel<128><<<(unsigned)cnt, 64, 0, st>>>(g, d_U, d_perm, d_cells, d_Us, kk, kn, d_nbr);
        TGP_HIP(hipGetLastError());
        TGP_HIP(hipEventRecord(ctx->ev[1], st));
        hipError_t he;
        if (ke == KE_GAUSS) he = run_solve_k<KE_GAUSS>(st, cnt, p, d_X, d_y, d_e2, d_Xs, d_nbr, n, kn, kk, d_ys, d_var, d_info);
        else if (ke == KE_VK) he = run_solve_k<KE_VK>(st, cnt, p, d_X, d_y, d_e2, d_Xs, d_nbr, n, kn, kk, d_ys, d_var, d_info);
        else he = run_solve_k<KE_AVK>(st, cnt, p, d_X, d_y, d_e2, d_Xs, d_nbr, n, kn, kk, d_ys, d_var, d_info);
        TGP_HIP(he);
        TGP_HIP(hipEventRecord(ctx->ev[2], st));
        TGP_HIP(hipMemcpyAsync(h + L.ys, d_ys, 8 * (size_t)cnt, hipMemcpyDeviceToHost, st));
        if (var) TGP_HIP(hipMemcpyAsync(h + L.var, d_var, 8 * (size_t)cnt, hipMemcpyDeviceToHost, st));
        TGP_HIP(hipMemcpyAsync(h + L.info, d_info, 4 * (size_t)cnt, hipMemcpyDeviceToHost, st));
        if (nbr) TGP_HIP(hipMemcpyAsync(h + L.nbr, d_nbr, 4 * (size_t)cnt * (size_t)kn, hipMemcpyDeviceToHost, st));
        TGP_HIP(hipStreamSynchronize(st));
        memcpy(ys + q0, h + L.ys, 8 * (size_t)cnt);
        if (var) memcpy(var + q0, h + L.var, 8 * (size_t)cnt);
        memcpy(info + q0, h + L.info, 4 * (size_t)cnt);
        if (nbr) memcpy(nbr + q0 * kn, h + L.nbr, 4 * (size_t)cnt * (size_t)kn);
        float ms = 0.f;
        TGP_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        ctx->timings[2] += ms;
        TGP_HIP(hipEventElapsedTime(&ms, ctx->ev[1], ctx->ev[2]));
        ctx->timings[3] += ms;
    }
    return 0;
}

extern "C" int tgp_gp_local_cond(tgp_ctx *ctx, const tgp_kernel *k, const double *X, int64_t n, const double *y, const double *yerr,
                                 int mode, const int32_t *rank, int kn, const int32_t *nbr_in, double *mu, double *var, int32_t *nbr,
                                 int32_t *cnt, int32_t *info, double *sums) {
    if (!ctx) return -1;
    TGP_ARG(k && X && y && info);
    TGP_ARG(n >= 1 && n < ((int64_t)1 << 31));
    if (kn < 1 || kn > LOCAL_KMAX) {
        ctx->err = "tgp_gp_local_cond: kn = " + std::to_string(kn) + " is outside 1 .. " + std::to_string(LOCAL_KMAX);
        return -1;
    }
    const int ke = kind_to_ke(k->kind);
    if (ke < 0) {
        ctx->err = "tgp_gp_local_cond: unknown kernel kind " + std::to_string(k->kind);
        return -1;
    }
    const bool search = nbr_in == nullptr;
    LocalWhiten R;
    if (search) {
        if (mode != TGP_LOCAL_LOO && mode != TGP_LOCAL_PRIOR) {
            ctx->err = "tgp_gp_local_cond: mode = " + std::to_string(mode) + " is neither TGP_LOCAL_LOO (0) nor TGP_LOCAL_PRIOR (1)";
            return -1;
        }
        if (local_whiten_factor(k, &R) != 0) {
            ctx->err = "tgp_gp_local_cond: invLam [[a, b], [b, c]] = [[" + std::to_string(k->a) + ", " + std::to_string(k->b) + "], [" +
                       std::to_string(k->b) + ", " + std::to_string(k->c) + "]] has no Cholesky factor: the metric of the neighbour "
                       "search needs a positive definite one";
            return -1;
        }
        if (mode == TGP_LOCAL_PRIOR) {
            if (!rank) {
                ctx->err = "tgp_gp_local_cond: TGP_LOCAL_PRIOR needs rank (n), a permutation of 0 .. n - 1";
                return -1;
            }
            int64_t bad = 0;
            if (local_rank_check(rank, n, &bad) != 0) {
                ctx->err = "tgp_gp_local_cond: rank is not a permutation of 0 .. " + std::to_string(n - 1) + ": rank[" + std::to_string(bad) +
                           "] = " + std::to_string(rank[bad]) + " is out of range or repeats an earlier entry";
                return -1;
            }
        }
    }
    for (double &t : ctx->timings) t = 0.0;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<int32_t> given_cnt;
    if (!search) {
        given_cnt.resize((size_t)n);
        int64_t bad_row = 0;
        int bad_at = 0;
        const int why = local_list_check(nbr_in, n, kn, 0, n, given_cnt.data(), &bad_row, &bad_at);
        if (why != 0) {
            const std::string at = "tgp_gp_local_cond: the neighbour list of row " + std::to_string(bad_row) + ": entry " + std::to_string(bad_at);
            if (why == -2) ctx->err = at + " is the row itself";
            else if (why == -3) ctx->err = at + " = " + std::to_string(nbr_in[bad_row * kn + bad_at]) + " follows a -1: the padding closes a list";
            else ctx->err = at + " = " + std::to_string(nbr_in[bad_row * kn + bad_at]) + " is outside 0 .. " + std::to_string(n - 1);
            return -1;
        }
    }
    const int kk = (int64_t)kn < n - 1 ? kn : (n > 1 ? (int)(n - 1) : 1);
    LocalGrid g;
    int64_t nc = 0;
    if (search) {
        local_grid_plan(X, n, R, kk / 4 > 1 ? kk / 4 : 1, &g);
        nc = local_grid_cells(g);
    }
    int64_t chunk = LOCAL_CHUNK_DEFAULT;
    if (const char *e = getenv("TGP_LOCAL_CHUNK")) {          // read per call, as in tgp_gp_predict_local
        if (atoll(e) > 0) chunk = atoll(e);
    }
    if (chunk > n) chunk = n;
    const CondLayout L = cond_layout(n, nc, chunk, kn);
    TGP_HIP(hipSetDevice(ctx->device));
    if (L.end > ctx->scratch_bytes) {                          // O(n + chunk kn), checked before anything runs
        size_t fr = 0, tot = 0;
        TGP_HIP(hipMemGetInfo(&fr, &tot));
        if (L.end > fr + ctx->scratch_bytes) {
            ctx->err = "tgp_gp_local_cond: needs " + std::to_string(L.end) + " bytes of device memory (n = " + std::to_string(n) +
                       ", chunk = " + std::to_string(chunk) + " rows of kn = " + std::to_string(kn) + "), " +
                       std::to_string(fr + ctx->scratch_bytes) + " are free; lower TGP_LOCAL_CHUNK";
            return -2;
        }
    }
    int rc = tgp_ensure_scratch(ctx, L.end);
    if (rc) return rc;
    void *hp = nullptr;
    rc = tgp_ensure_pinned(ctx, L.host_end, &hp);
    if (rc) return rc;
    char *h = (char *)hp, *d = (char *)ctx->scratch;
    hipStream_t st = ctx->stream;

    memcpy(h + L.X, X, 16 * (size_t)n);
    memcpy(h + L.y, y, 8 * (size_t)n);
    if (yerr) {
        double *e2 = (double *)(h + L.e2);
        for (int64_t i = 0; i < n; ++i) e2[i] = yerr[i] * yerr[i];
    }
    const bool prior = search && mode == TGP_LOCAL_PRIOR;
    if (search) {
        local_grid_sort(X, n, R, g, (double *)(h + L.U), (int32_t *)(h + L.perm), (int32_t *)(h + L.cells));
        if (prior) {
            memcpy(h + L.rank, rank, 4 * (size_t)n);
            local_rank_sorted(rank, (const int32_t *)(h + L.perm), n, (int32_t *)(h + L.rank_s));
        }
    }
    TGP_HIP(hipMemcpyAsync(d, h, search ? L.tables_end : L.data_end, hipMemcpyHostToDevice, st));
    TGP_HIP(hipStreamSynchronize(st));
    ctx->timings[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

    const KParams p = make_kparams(k);
    const double *d_U = (const double *)(d + L.U), *d_X = (const double *)(d + L.X), *d_y = (const double *)(d + L.y);
    const double *d_e2 = yerr ? (const double *)(d + L.e2) : nullptr;
    const int32_t *d_perm = (const int32_t *)(d + L.perm), *d_cells = (const int32_t *)(d + L.cells);
    const int32_t *d_rank = (const int32_t *)(d + L.rank), *d_rank_s = (const int32_t *)(d + L.rank_s);
    double *d_Us = (double *)(d + L.Us), *d_mu = (double *)(d + L.mu), *d_var = (double *)(d + L.var);
    int32_t *d_info = (int32_t *)(d + L.info), *d_cnt = (int32_t *)(d + L.cnt), *d_nbr = (int32_t *)(d + L.nbr);
    double *d_T = (double *)(d + L.T);
    for (int64_t q0 = 0; q0 < n; q0 += chunk) {
        const int64_t c = n - q0 < chunk ? n - q0 : chunk;
        if (search) {
            double *hu = (double *)(h + L.Us);
            for (int64_t j = 0; j < c; ++j) local_whiten_point(R, X[2 * (q0 + j)], X[2 * (q0 + j) + 1], hu + 2 * j, hu + 2 * j + 1);
            TGP_HIP(hipMemcpyAsync(d_Us, h + L.Us, 16 * (size_t)c, hipMemcpyHostToDevice, st));
        } else {
            memcpy(h + L.nbr, nbr_in + q0 * kn, 4 * (size_t)c * (size_t)kn);
            memcpy(h + L.cnt, given_cnt.data() + q0, 4 * (size_t)c);
            TGP_HIP(hipMemcpyAsync(d_nbr, h + L.nbr, 4 * (size_t)c * (size_t)kn, hipMemcpyHostToDevice, st));
            TGP_HIP(hipMemcpyAsync(d_cnt, h + L.cnt, 4 * (size_t)c, hipMemcpyHostToDevice, st));
        }
        TGP_HIP(hipEventRecord(ctx->ev[0], st));
        if (search) {
            const int64_t sweep_below = n / LOCAL_SWEEP > kn ? n / LOCAL_SWEEP : kn;
            const LocalCondArgs ca = {q0, n, prior ? d_rank : nullptr, prior ? d_rank_s : nullptr, d_cnt, (int32_t)sweep_below};
            if (prior) run_cond_search<LS_EARLIER>(st, c, g, d_U, d_perm, d_cells, d_Us, kn, d_nbr, ca);
            else run_cond_search<LS_NOT_SELF>(st, c, g, d_U, d_perm, d_cells, d_Us, kn, d_nbr, ca);
            TGP_HIP(hipGetLastError());
        }
        TGP_HIP(hipEventRecord(ctx->ev[1], st));
        const double *d_Xq = d_X + 2 * q0;                   // the queries are the rows themselves
        hipError_t he;
        if (ke == KE_GAUSS) he = run_cond_solve_k<KE_GAUSS>(st, c, p, d_X, d_y, d_e2, d_Xq, d_nbr, d_cnt, n, kn, d_mu, d_var, d_info);
        else if (ke == KE_VK) he = run_cond_solve_k<KE_VK>(st, c, p, d_X, d_y, d_e2, d_Xq, d_nbr, d_cnt, n, kn, d_mu, d_var, d_info);
        else he = run_cond_solve_k<KE_AVK>(st, c, p, d_X, d_y, d_e2, d_Xq, d_nbr, d_cnt, n, kn, d_mu, d_var, d_info);
        TGP_HIP(he);
        local_terms_kernel<<<(unsigned)((c + 255) / 256), 256, 0, st>>>(d_mu, d_var, d_info, d_y, d_e2, q0, c, n, d_T);
        TGP_HIP(hipGetLastError());
        TGP_HIP(hipEventRecord(ctx->ev[2], st));
        if (mu) TGP_HIP(hipMemcpyAsync(h + L.mu, d_mu, 8 * (size_t)c, hipMemcpyDeviceToHost, st));
        if (var) TGP_HIP(hipMemcpyAsync(h + L.var, d_var, 8 * (size_t)c, hipMemcpyDeviceToHost, st));
        TGP_HIP(hipMemcpyAsync(h + L.info, d_info, 4 * (size_t)c, hipMemcpyDeviceToHost, st));
        if (cnt && search) TGP_HIP(hipMemcpyAsync(h + L.cnt, d_cnt, 4 * (size_t)c, hipMemcpyDeviceToHost, st));
        if (nbr && search) TGP_HIP(hipMemcpyAsync(h + L.nbr, d_nbr, 4 * (size_t)c * (size_t)kn, hipMemcpyDeviceToHost, st));
        TGP_HIP(hipStreamSynchronize(st));
        if (mu) memcpy(mu + q0, h + L.mu, 8 * (size_t)c);
        if (var) memcpy(var + q0, h + L.var, 8 * (size_t)c);
        memcpy(info + q0, h + L.info, 4 * (size_t)c);
        if (cnt) memcpy(cnt + q0, h + L.cnt, 4 * (size_t)c);          // (given lists: the lengths the check counted)
        if (nbr) memcpy(nbr + q0 * kn, h + L.nbr, 4 * (size_t)c * (size_t)kn);
        float ms = 0.f;
        TGP_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        ctx->timings[2] += ms;
        TGP_HIP(hipEventElapsedTime(&ms, ctx->ev[1], ctx->ev[2]));
        ctx->timings[3] += ms;
    }
    if (sums) {
        // the fixed tree over the row index, level by level, after the last chunk: T (3, n) -> ... -> (3, 1)
        TGP_HIP(hipEventRecord(ctx->ev[0], st));
        const double *src = d_T;
        int64_t count = n, stride = n;
        double *bufs[2] = {(double *)(d + L.P0), (double *)(d + L.P1)};
        int which = 0;
        do {
            const int64_t blocks = (count + 1023) / 1024;
            double *dst = bufs[which];
            local_reduce_kernel<<<dim3((unsigned)blocks, 3), 256, 0, st>>>(src, count, stride, dst, blocks);
            TGP_HIP(hipGetLastError());
            src = dst;
            count = stride = blocks;
            which ^= 1;
        } while (count > 1);
        TGP_HIP(hipEventRecord(ctx->ev[1], st));
        TGP_HIP(hipMemcpyAsync(h + L.sums, src, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
        TGP_HIP(hipStreamSynchronize(st));
        memcpy(sums, h + L.sums, 3 * sizeof(double));
        float ms = 0.f;
        TGP_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        ctx->timings[3] += ms;
    }
    return 0;
}
