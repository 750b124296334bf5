// CPU-side AddressSanitizer / UBSan run of the host checks of the local conditionals (seam S3v; treegp_amd/csrc/local_grid.h, no
// GPU, no HIP): the rank check, the list check and the ranks-into-cell-order step, in exact-size buffers.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I include tests/sanitize/local_cond_driver.cpp -o drv && ./drv
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <random>
#include <vector>
#include "../../treegp_amd/csrc/local_grid.h"

static int fails = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++fails; }    \
    } while (0)

static void rank_cases(std::mt19937_64 &rng) {
    for (int64_t n : {1, 2, 3, 64, 1000, 70001}) {
        std::vector<int32_t> rank(n);
        std::iota(rank.begin(), rank.end(), 0);
        std::shuffle(rank.begin(), rank.end(), rng);
        int64_t bad = -5;
        CHECK(local_rank_check(rank.data(), n, &bad) == 0 && bad == -5);
        if (n >= 2) {
            std::vector<int32_t> r2 = rank;
            r2[n - 1] = r2[0];                                             // a repeat: the LATER entry is the offender
            CHECK(local_rank_check(r2.data(), n, &bad) == -1 && bad == n - 1);
            r2 = rank;
            r2[n / 2] = (int32_t)n;                                        // one past the range
            CHECK(local_rank_check(r2.data(), n, &bad) == -1 && bad == n / 2);
            r2 = rank;
            r2[0] = -1;
            CHECK(local_rank_check(r2.data(), n, &bad) == -1 && bad == 0);
            r2[0] = INT32_MIN;
            CHECK(local_rank_check(r2.data(), n, &bad) == -1 && bad == 0);
            r2[0] = INT32_MAX;
            CHECK(local_rank_check(r2.data(), n, &bad) == -1 && bad == 0);
        }
        // the ranks in the order of a real grid sort
        std::vector<double> X(2 * n);
        std::uniform_real_distribution<double> u(0.0, 1.0);
        for (auto &v : X) v = u(rng);
        tgp_kernel rbf = {TGP_RBF, 0, 1.0, 44.0, 0.0, 44.0, 1.0};
        LocalWhiten R;
        CHECK(local_whiten_factor(&rbf, &R) == 0);
        LocalGrid g;
        local_grid_plan(X.data(), n, R, 8, &g);
        const int64_t nc = local_grid_cells(g);
        std::vector<double> U(2 * n);
        std::vector<int32_t> perm(n), start(nc + 1), rank_s(n);
        local_grid_sort(X.data(), n, R, g, U.data(), perm.data(), start.data());
        local_rank_sorted(rank.data(), perm.data(), n, rank_s.data());
        for (int64_t s = 0; s < n; ++s) CHECK(rank_s[s] == rank[perm[s]]);
        CHECK(local_rank_check(rank_s.data(), n, &bad) == 0);              // still a permutation
    }
}

static void list_cases(std::mt19937_64 &rng) {
    for (int64_t n : {1, 2, 5, 300}) {
        for (int kn : {1, 2, 33, 128}) {
            std::vector<int32_t> nbr((size_t)n * kn, -1), cnt(n, -7);
            // row i: min(kn, n - 1, i % (kn + 1)) different rows other than i
            for (int64_t i = 0; i < n; ++i) {
                const int len = (int)std::min<int64_t>(std::min<int64_t>(kn, n - 1), i % (kn + 1));
                for (int t = 0; t < len; ++t) nbr[i * kn + t] = (int32_t)((i + 1 + t) % n);
            }
            int64_t row = -5;
            int at = -5;
            CHECK(local_list_check(nbr.data(), n, kn, 0, n, cnt.data(), &row, &at) == 0 && row == -5 && at == -5);
            for (int64_t i = 0; i < n; ++i) CHECK(cnt[i] == (int)std::min<int64_t>(std::min<int64_t>(kn, n - 1), i % (kn + 1)));
            // a window of rows writes its own lengths from index 0
            if (n >= 5) {
                std::vector<int32_t> part(2, -7);
                CHECK(local_list_check(nbr.data(), n, kn, 2, 4, part.data(), &row, &at) == 0);
                CHECK(part[0] == cnt[2] && part[1] == cnt[3]);
            }
            if (n < 5) continue;
            const int64_t i = n - 1;                                       // the last row: the reads end with the buffer
            std::vector<int32_t> bad = nbr;
            bad[i * kn + 0] = (int32_t)i;
            CHECK(local_list_check(bad.data(), n, kn, 0, n, cnt.data(), &row, &at) == -2 && row == i && at == 0);
            bad[i * kn + 0] = (int32_t)n;
            CHECK(local_list_check(bad.data(), n, kn, 0, n, cnt.data(), &row, &at) == -1 && row == i && at == 0);
            bad[i * kn + 0] = -2;
            CHECK(local_list_check(bad.data(), n, kn, 0, n, cnt.data(), &row, &at) == -1 && row == i && at == 0);
            bad[i * kn + 0] = INT32_MIN;
            CHECK(local_list_check(bad.data(), n, kn, 0, n, cnt.data(), &row, &at) == -1 && row == i && at == 0);
            if (kn >= 2) {
                bad = nbr;
                for (int t = 0; t < kn; ++t) bad[i * kn + t] = -1;
                bad[i * kn + kn - 1] = 0;                                 // an entry after the padding began
                CHECK(local_list_check(bad.data(), n, kn, 0, n, cnt.data(), &row, &at) == -3 && row == i && at == kn - 1);
                // a repeated row is not this check's business
                bad = nbr;
                bad[i * kn + 0] = bad[i * kn + 1] = 0;
                CHECK(local_list_check(bad.data(), n, kn, 0, n, cnt.data(), &row, &at) == 0);
            }
            // the FIRST bad list is the one named
            bad = nbr;
            bad[1 * kn] = 1;
            bad[3 * kn] = 3;
            CHECK(local_list_check(bad.data(), n, kn, 0, n, cnt.data(), &row, &at) == -2 && row == 1);
        }
    }
    (void)rng;
}

int main() {
    std::mt19937_64 rng(9);
    rank_cases(rng);
    list_cases(rng);
    if (fails) { printf("%d failures\n", fails); return 1; }
    printf("local conditionals ok under sanitizers\n");
    return 0;
}
