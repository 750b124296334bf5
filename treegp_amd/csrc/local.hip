// Local kriging (seam S3l of include/tgp.h): every query is conditioned on its k nearest training points alone.
//   host     the whitening factor of the metric and the bucket grid over the whitened training points (local_grid.h)
//   search   one query per 64-lane workgroup: cells in growing square rings around the query's cell, the k best (d^2, row)
//            in LDS, every batch of candidates merged by a bitonic sort of (best, batch)
//   solve    one query per workgroup: K_S, k* and y_S gathered into one LDS matrix of k + 2 rows, factorised in place with the two
//            right-hand sides carried along as rows, v.w and v.v reduced in a fixed order
// No N x N anything, no atomics; a query's bits depend on the training set, the kernel, k and its own coordinates only.
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

// KBB: capacity of the best list and of the batch (k <= KBB); P = 2 KBB entries are sorted at a merge
template <int KBB>
__global__ __launch_bounds__(64) void local_search_kernel(LocalGrid g, const double *__restrict__ U, const int32_t *__restrict__ perm,
                                                          const int32_t *__restrict__ cell_start, const double *__restrict__ Us,
                                                          int k, int kn, int32_t *__restrict__ nbr) {
    constexpr int P = 2 * KBB;
    __shared__ double bd[P];
    __shared__ int32_t bi[P];
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    const double inf = __builtin_huge_val();
    const double uqx = Us[2 * q], uqy = Us[2 * q + 1];
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
            }
            const unsigned long long mask = __ballot(pass);
            if (pass) {
                const int pos = KBB + count + __popcll(mask & ((1ull << lane) - 1ull));
                bd[pos] = d2;
                bi[pos] = perm[r];
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
    for (int t = lane; t < kn; t += 64) nbr[q * kn + t] = t < k ? bi[t] : -1;      // nearest first
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
template <int KE, int KB, int G>
__global__ __launch_bounds__(G *local_rows_pad(KB)) void local_solve_kernel(KParams p, const double *__restrict__ X,
                                                                            const double *__restrict__ y, const double *__restrict__ e2,
                                                                            const double *__restrict__ Xs, const int32_t *__restrict__ nbr,
                                                                            int64_t n, int kn, int k, double *__restrict__ ys,
                                                                            double *__restrict__ var, int32_t *__restrict__ info) {
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
