// CPU-side AddressSanitizer / UBSan run of the host logic of local kriging (treegp_amd/csrc/local_grid.h, no GPU, no HIP): the
// whitening factor, the grid plan and the counting sort, driven with the degenerate inputs of the neighbour search.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I include tests/sanitize/local_grid_driver.cpp -o drv && ./drv
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>
#include "../../treegp_amd/csrc/local_grid.h"

static int fails = 0;
#define CHECK(cond, name)                                                    \
    do {                                                                     \
        if (!(cond)) { printf("FAILED %s: %s\n", name, #cond); ++fails; return; } \
    } while (0)

static void run_case(const char *name, const std::vector<double> &X, const tgp_kernel &k, int occ) {
    const int64_t n = (int64_t)X.size() / 2;
    LocalWhiten R;
    CHECK(local_whiten_factor(&k, &R) == 0, name);
    LocalGrid g;
    local_grid_plan(X.data(), n, R, occ, &g);
    const int64_t nc = local_grid_cells(g);
    CHECK(g.gx >= 1 && g.gy >= 1 && nc >= 1 && nc <= 2 * n + 1, name);
    CHECK(g.hx >= 0.0 && g.hy >= 0.0 && std::isfinite(g.inv_hx) && std::isfinite(g.inv_hy), name);
    // exact-size buffers: an index one past the end is an AddressSanitizer report
    std::vector<double> U(2 * n);
    std::vector<int32_t> perm(n), start(nc + 1);
    local_grid_sort(X.data(), n, R, g, U.data(), perm.data(), start.data());
    CHECK(start[0] == 0 && start[nc] == n, name);
    for (int64_t c = 0; c < nc; ++c) CHECK(start[c] <= start[c + 1], name);
    std::vector<char> seen(n, 0);
    for (int64_t c = 0; c < nc; ++c) {
        for (int32_t s = start[c]; s < start[c + 1]; ++s) {
            const int32_t i = perm[s];
            CHECK(i >= 0 && i < n && !seen[i], name);
            seen[i] = 1;
            double u0, u1;
            local_whiten_point(R, X[2 * i], X[2 * i + 1], &u0, &u1);
            CHECK((U[2 * s] == u0 || (u0 != u0 && U[2 * s] != U[2 * s])) && (U[2 * s + 1] == u1 || (u1 != u1 && U[2 * s + 1] != U[2 * s + 1])), name);
            CHECK(local_cell(g, u0, u1) == c, name);
            if (s > start[c]) CHECK(perm[s - 1] < i, name);              // stable: rows of a cell keep their order
        }
    }
    // queries anywhere, NaN and infinities included, land on the grid
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (double q : {0.0, 0.5, -1e300, 1e300, 100.0 * (g.hix - g.lox) + g.hix, inf, -inf, nan}) {
        const int32_t cx = local_cell_axis(q, g.lox, g.inv_hx, g.gx), cy = local_cell_axis(q, g.loy, g.inv_hy, g.gy);
        CHECK(cx >= 0 && cx < g.gx && cy >= 0 && cy < g.gy, name);
    }
    // cell() is monotone along each axis
    int32_t last = 0;
    for (int t = 0; t <= 1000; ++t) {
        const int32_t cx = local_cell_axis(g.lox + (g.hix - g.lox) * (t / 1000.0), g.lox, g.inv_hx, g.gx);
        CHECK(cx >= last, name);
        last = cx;
    }
    int64_t biggest = 0;
    for (int64_t c = 0; c < nc; ++c) if (start[c + 1] - start[c] > biggest) biggest = start[c + 1] - start[c];
    printf("%-28s n %6lld  grid %5d x %5d  fullest cell %6lld\n", name, (long long)n, g.gx, g.gy, (long long)biggest);
}

int main() {
    std::mt19937_64 rng(5);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    tgp_kernel rbf = {TGP_RBF, 0, 1.0, 44.0, 0.0, 44.0, 1.0};
    tgp_kernel vk = {TGP_VK, 0, 1.0, 1.0, 0.0, 1.0, 0.6};
    // axis ratio 1000, rotated by 30 degrees: invLam = Q diag(1e6, 1) Q^T
    const double cs = std::cos(0.5235987755982988), sn = std::sin(0.5235987755982988);
    tgp_kernel arbf = {TGP_ARBF, 0, 1.0, 1e6 * cs * cs + sn * sn, (1e6 - 1.0) * cs * sn, 1e6 * sn * sn + cs * cs, 1.0};

    for (int64_t n : {1, 2, 3, 63, 64, 65, 2000, 70000}) {
        std::vector<double> X(2 * n);
        for (auto &v : X) v = u(rng);
        for (int occ : {1, 8, 16, 32}) {
            run_case("uniform rbf", X, rbf, occ);
            run_case("uniform arbf 1000:1", X, arbf, occ);
        }
        run_case("uniform vk", X, vk, 16);
    }
    {   // 2900 of 3000 points inside one cell-sized cluster
        std::vector<double> X(6000);
        for (int i = 0; i < 3000; ++i) {
            const double s = i < 2900 ? 1e-3 : 1.0;
            X[2 * i] = (i < 2900 ? 0.4 : 0.0) + s * u(rng);
            X[2 * i + 1] = (i < 2900 ? 0.7 : 0.0) + s * u(rng);
        }
        run_case("cluster", X, rbf, 16);
    }
    {   // collinear (all y equal), 1-D (y == 0), all x equal, all points equal
        std::vector<double> X(4000);
        for (int i = 0; i < 2000; ++i) { X[2 * i] = u(rng); X[2 * i + 1] = 0.25; }
        run_case("collinear", X, rbf, 16);
        run_case("collinear arbf", X, arbf, 16);
        for (int i = 0; i < 2000; ++i) X[2 * i + 1] = 0.0;
        run_case("one-dimensional", X, rbf, 8);
        for (int i = 0; i < 2000; ++i) { X[2 * i + 1] = X[2 * i]; X[2 * i] = -3.0; }
        run_case("all x equal", X, rbf, 8);
        for (int i = 0; i < 2000; ++i) { X[2 * i] = 0.5; X[2 * i + 1] = 0.5; }
        run_case("all points equal", X, rbf, 32);
    }
    {   // duplicated rows, a lattice
        std::vector<double> X(4000);
        for (int i = 0; i < 1000; ++i) { X[2 * i] = u(rng); X[2 * i + 1] = u(rng); X[2 * (i + 1000)] = X[2 * i]; X[2 * (i + 1000) + 1] = X[2 * i + 1]; }
        run_case("duplicated rows", X, rbf, 16);
        for (int i = 0; i < 2000; ++i) { X[2 * i] = i % 50; X[2 * i + 1] = i / 50; }
        run_case("lattice", X, rbf, 16);
        run_case("lattice occ 1", X, rbf, 1);
    }
    {   // extreme aspect ratio, huge offsets, NaN and infinite coordinates
        std::vector<double> X(2000);
        for (int i = 0; i < 1000; ++i) { X[2 * i] = 1e9 * u(rng); X[2 * i + 1] = 1e-9 * u(rng); }
        run_case("aspect 1e18", X, rbf, 4);
        for (int i = 0; i < 1000; ++i) { X[2 * i] = 1e15 + u(rng); X[2 * i + 1] = -1e15 + u(rng); }
        run_case("offset 1e15", X, rbf, 4);
        X[10] = std::numeric_limits<double>::quiet_NaN();
        X[21] = std::numeric_limits<double>::infinity();
        X[40] = -std::numeric_limits<double>::infinity();
        run_case("NaN and inf rows", X, rbf, 4);
        for (auto &v : X) v = std::numeric_limits<double>::quiet_NaN();
        run_case("all NaN", X, rbf, 4);
        for (auto &v : X) v = 1e308 * (u(rng) - 0.5) * 2.0;
        run_case("extent overflows", X, rbf, 4);
    }
    // an invLam without a factor, an unknown kind
    LocalWhiten R;
    tgp_kernel bad = {TGP_ARBF, 0, 1.0, 1.0, 2.0, 1.0, 1.0};
    if (local_whiten_factor(&bad, &R) != -1) { printf("FAILED: indefinite invLam accepted\n"); ++fails; }
    bad.a = -1.0;
    if (local_whiten_factor(&bad, &R) != -1) { printf("FAILED: negative a accepted\n"); ++fails; }
    bad.a = std::numeric_limits<double>::quiet_NaN();
    if (local_whiten_factor(&bad, &R) != -1) { printf("FAILED: NaN invLam accepted\n"); ++fails; }
    bad.kind = 7;
    if (local_whiten_factor(&bad, &R) != -2) { printf("FAILED: unknown kind accepted\n"); ++fails; }
    if (fails) { printf("%d failures\n", fails); return 1; }
    printf("local grid ok under sanitizers\n");
    return 0;
}
