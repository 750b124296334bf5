// The K-build tile shared by kbuild.hip (first-generation single-GPU build, multi-GPU build) and batch.hip (batched build).
#pragma once
#include "tgp_internal.h"
#include "kernel_eval.h"

// Value and store of the slab builds (kbuild.hip: kbuild_slab_kernel; ksum.hip: the same slabs for sums of kernels).
template <int KE>
__device__ __forceinline__ double kb_value(const KParams &p, double dx, double dy, const double *tab) {
    if constexpr (KE == KE_GAUSS) return p.amp * tgp_exp2_neg(quad_form(p, dx, dy));   // p.a, p.b2, p.c pre-scaled by the host
    else return kernel_value_tab<KE>(p, dx, dy, tab);                                   // von Karman: Chebyshev table in LDS
}

__device__ __forceinline__ void kb_store(double *dst, const double2 &v) {
#ifdef TGP_KBUILD_NT
    __builtin_nontemporal_store(v.x, dst);
    __builtin_nontemporal_store(v.y, dst + 1);
#else
    *reinterpret_cast<double2 *>(dst) = v;
#endif
}

// One 128x128 tile per workgroup of 256 threads.  Lane l of wave w owns columns 2l, 2l+1 and
// rows w, w+4, ... of the tile, so each wave-instruction stores one full 1 KiB row segment.
// (ti, tj) are GLOBAL 128-tile coordinates; `tile` is where the tile lives (ld 256).
template <int KE>
__device__ __forceinline__ void kbuild_tile(const KParams &p, const double *__restrict__ X, int64_t n,
                                            const double *__restrict__ yerr, int64_t ti, int64_t tj,
                                            double *__restrict__ tile) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t j0 = tj * TGP_TB + 2 * lane;
    double xj0 = 0, yj0 = 0, xj1 = 0, yj1 = 0;
    if (j0 < n) { xj0 = X[2 * j0]; yj0 = X[2 * j0 + 1]; }
    if (j0 + 1 < n) { xj1 = X[2 * j0 + 2]; yj1 = X[2 * j0 + 3]; }

    const bool diag_tile = (ti == tj);
    const bool pad_tile = (ti * TGP_TB + TGP_TB > n);   // rows (and maybe columns) beyond n

#pragma unroll 4
    for (int r = wave; r < TGP_TB; r += 4) {
        const int64_t i = ti * TGP_TB + r;
        double2 v;
        if (!pad_tile || i < n) {
            const double xi = X[2 * (i < n ? i : 0)], yi = X[2 * (i < n ? i : 0) + 1];   // wave-uniform
            v.x = kernel_value<KE>(p, xi - xj0, yi - yj0);
            v.y = kernel_value<KE>(p, xi - xj1, yi - yj1);
            if (diag_tile) {
                // exact diagonal (kernels.py:121) + noise (gp_interp.py:180)
                if (i == j0) { const double e = yerr ? yerr[i] : 0.0; v.x = p.amp + e * e; }
                if (i == j0 + 1) { const double e = yerr ? yerr[i] : 0.0; v.y = p.amp + e * e; }
            }
            if (pad_tile) {
                if (j0 >= n) v.x = 0.0;
                if (j0 + 1 >= n) v.y = 0.0;
            }
        } else {
            // padded rows: identity, so the padded factor is [[L, 0], [0, I]]
            v.x = (i == j0) ? 1.0 : 0.0;
            v.y = (i == j0 + 1) ? 1.0 : 0.0;
        }
        *reinterpret_cast<double2 *>(tile + (int64_t)r * TGP_PW + 2 * lane) = v;
    }
}
