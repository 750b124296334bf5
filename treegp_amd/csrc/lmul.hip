// Y = L Z with the packed lower factor: realisations of N(0, K + D) from standard normals Z (seam S3d, include/tgp.h).
// Stands in for np.random.multivariate_normal(0, K) (tests/treegp_test_helper.py:64-66, 95-97 of the reference).
//
// No dependency chain, unlike the sweeps of trsv.hip: every (row block, panel) tile can be in flight at once.  HBM-bound
// (tgp_panel_elems(Np) * 8 bytes per group of R right-hand sides).  A block row of 256 rows carries rb + 1 tiles of 512 KiB
// (128 MB for the last one at Np = 65 536), so each block row is cut into segments of at most lmul_seg_tiles(Np) tiles and
// every workgroup streams one segment for R right-hand sides.  Each segment writes its partial sums; lmul_reduce_kernel
// adds the segments of a block row in segment order.  No atomics: the result is bit-identical from run to run, and a
// column of Y does not depend on which or how many other columns were computed with it (the arithmetic of one column is
// fixed by Np alone: the segmentation, the per-lane products and the tree of the cross-lane sum).
#include "tgp_internal.h"

namespace {

constexpr int LMUL_R = 8;           // right-hand sides per group: L is read once per group

// y (R per lane) -> the sum over the 64 lanes of every y[v], slot v landing in lanes v * 64/R .. (v+1) * 64/R - 1.
// A reduce-scatter: the step across lane bit 5 exchanges half the slots (each lane keeps the half its bit names), the
// step across bit 4 half of what is left, ...; once each lane holds one slot the remaining bits are a plain butterfly.
// Every slot is therefore summed over the same tree as a full butterfly would sum it alone (lane pairs across bit 5,
// then 4, ..., 0; a + b == b + a exactly), whatever R is: that is what keeps a column independent of its group.
// Unlike the sweeps' row dot (fwd_update256_kernel: one wave_sum per row), R dots share the 6 exchange steps.
template <int R>
__device__ __forceinline__ double reduce_scatter(double (&y)[R], int lane) {
#pragma unroll
    for (int c = R, o = 32; c > 1; c >>= 1, o >>= 1) {
        const bool hi = (lane & o) != 0;
        const int h = c / 2;
#pragma unroll
        for (int j = 0; j < h; ++j) {
            const double send = hi ? y[j] : y[h + j];
            const double keep = hi ? y[h + j] : y[j];
            y[j] = keep + __shfl_xor(send, o, 64);
        }
    }
    double s = y[0];
#pragma unroll
    for (int o = 32 / R; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

// One workgroup = one segment (block row rb, panels p0 .. p1-1) for one group of R right-hand sides.  Wave w takes the
// rows w, w + 4, ..., each row of a tile a whole 2 KiB panel row (64 lanes x 4 doubles).  The group's 256-column slice
// of Z for the current panel is staged in LDS; every lane keeps its four columns of it in registers for the tile.
// Per row and slot: the lane's four products in a fixed order, then reduce_scatter; the row's sum is added to the
// segment's accumulator (LDS, one owner lane per (slot, row)) in panel order.  The diagonal tile reads columns <= row
// only (the stale upper part of a diagonal block is never used, as everywhere in the library).
template <int R>
__global__ __launch_bounds__(256) void lmul_kernel(const double *__restrict__ A, int64_t Np, int seg_tiles,
                                                   const double *__restrict__ Z, int nrhs, int g0,
                                                   double *__restrict__ partial, int64_t nitems) {
    __shared__ double zs[R][TGP_PW];
    __shared__ double acc[R][TGP_PW];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    // the segment of this workgroup: the longest block rows first (they are the last items), so that the tail of the
    // launch is made of short ones
    int64_t item = nitems - 1 - (int64_t)blockIdx.x;
    const int64_t item_id = item;
    int64_t rb = 0;
    for (;; ++rb) {
        const int64_t ns = rb / seg_tiles + 1;
        if (item < ns) break;
        item -= ns;
    }
    const int64_t ns = rb / seg_tiles + 1, s = item;
    const int64_t p0 = s * (rb + 1) / ns, p1 = (s + 1) * (rb + 1) / ns;
    const int v0 = (g0 + blockIdx.y) * R;
#pragma unroll
    for (int v = 0; v < R; ++v) acc[v][tid] = 0.0;

    for (int64_t p = p0; p < p1; ++p) {
        __syncthreads();                                     // previous tile's zs reads are done
#pragma unroll
        for (int v = 0; v < R; ++v) zs[v][tid] = v0 + v < nrhs ? Z[(int64_t)(v0 + v) * Np + p * TGP_PW + tid] : 0.0;
        __syncthreads();
        double z[4][R];
#pragma unroll
        for (int v = 0; v < R; ++v) {
            const double2 a = *reinterpret_cast<const double2 *>(&zs[v][2 * lane]);
            const double2 b = *reinterpret_cast<const double2 *>(&zs[v][TGP_TB + 2 * lane]);
            z[0][v] = a.x; z[1][v] = a.y; z[2][v] = b.x; z[3][v] = b.y;
        }
        const double *T = A + panel_off(p, Np) + (rb - p) * TGP_PW * TGP_PW;     // tile (rb, p), ld 256
        const bool diag = p == rb;
        const int c0 = 2 * lane, c2 = TGP_TB + 2 * lane;
        for (int r0 = w; r0 < TGP_PW; r0 += 16) {
            double2 a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {                        // 4 rows (8 KiB per wave) in flight
                const double *row = T + (int64_t)(r0 + 4 * u) * TGP_PW;
                a[u] = *reinterpret_cast<const double2 *>(row + c0);
                b[u] = *reinterpret_cast<const double2 *>(row + c2);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int r = r0 + 4 * u;
                double l0 = a[u].x, l1 = a[u].y, l2 = b[u].x, l3 = b[u].y;
                if (diag) {
                    l0 = c0 <= r ? l0 : 0.0;
                    l1 = c0 + 1 <= r ? l1 : 0.0;
                    l2 = c2 <= r ? l2 : 0.0;
                    l3 = c2 + 1 <= r ? l3 : 0.0;
                }
                double y[R];
#pragma unroll
                for (int v = 0; v < R; ++v) y[v] = fma(l3, z[3][v], fma(l2, z[2][v], fma(l1, z[1][v], l0 * z[0][v])));
                const double t = reduce_scatter<R>(y, lane);
                if ((lane & (64 / R - 1)) == 0) acc[lane / (64 / R)][r] += t;
            }
        }
    }
    __syncthreads();
    for (int v = 0; v < R && v0 + v < nrhs; ++v)
        partial[(item_id * nrhs + v0 + v) * TGP_PW + tid] = acc[v][tid];
}

// Y[v, 256 rb + r] = sum over the segments of block row rb, in segment order
__global__ __launch_bounds__(256) void lmul_reduce_kernel(const double *__restrict__ partial, int64_t Np, int seg_tiles,
                                                          int nrhs, int v0, double *__restrict__ Y) {
    const int64_t rb = blockIdx.x;
    const int v = v0 + blockIdx.y;
    const int64_t q = rb / seg_tiles, m = rb % seg_tiles;
    const int64_t first = rb + seg_tiles * q * (q - 1) / 2 + q * m;    // sum over r < rb of (r / seg_tiles + 1)
    const int64_t ns = q + 1;
    double s = 0.0;
    for (int64_t k = 0; k < ns; ++k) s += partial[((first + k) * nrhs + v) * TGP_PW + threadIdx.x];
    Y[(int64_t)v * Np + rb * TGP_PW + threadIdx.x] = s;
}

}  // namespace

// tiles per segment: one tile (512 KiB) per workgroup while the triangle is small, up to 8 (4 MiB) at Np = 65 536
// (about 4200 workgroups per group there).  Depends on Np only: a column's arithmetic must not depend on nrhs.
static int lmul_seg_tiles(int64_t Np) {
    const int64_t nP = Np / TGP_PW;
    const int64_t c = nP / 32;
    return (int)(c < 1 ? 1 : (c > 8 ? 8 : c));
}

static int64_t lmul_items(int64_t Np, int seg) {
    const int64_t nP = Np / TGP_PW;
    const int64_t q = nP / seg, m = nP % seg;
    return nP + (int64_t)seg * q * (q - 1) / 2 + q * m;
}

size_t lmul_partial_bytes(int64_t Np, int nrhs) {
    return (size_t)lmul_items(Np, lmul_seg_tiles(Np)) * nrhs * TGP_PW * sizeof(double);
}

// d_Z, d_Y: (nrhs, Np) row-major, Z zero-padded; d_partial: lmul_partial_bytes(Np, nrhs)
int launch_factor_lmul(tgp_ctx *ctx, const double *d_A, int64_t Np, const double *d_Z, int nrhs, double *d_Y,
                       double *d_partial) {
    hipStream_t st = ctx->stream;
    const int seg = lmul_seg_tiles(Np);
    const int64_t nitems = lmul_items(Np, seg);
    const int ngroups = (nrhs + LMUL_R - 1) / LMUL_R;
    constexpr int maxy = 65535;
    for (int g0 = 0; g0 < ngroups; g0 += maxy) {
        const int gy = ngroups - g0 < maxy ? ngroups - g0 : maxy;
        lmul_kernel<LMUL_R><<<dim3((unsigned)nitems, (unsigned)gy), 256, 0, st>>>(d_A, Np, seg, d_Z, nrhs, g0, d_partial,
                                                                                   nitems);
    }
    for (int v0 = 0; v0 < nrhs; v0 += maxy) {
        const int vy = nrhs - v0 < maxy ? nrhs - v0 : maxy;
        lmul_reduce_kernel<<<dim3((unsigned)(Np / TGP_PW), (unsigned)vy), 256, 0, st>>>(d_partial, Np, seg, nrhs, v0, d_Y);
    }
    TGP_HIP(hipGetLastError());
    return 0;
}
