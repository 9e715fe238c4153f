// Stand-alone host program around pybo_amd/csrc/acq_core.h, the header the acquisition kernels include: it runs the shared
// per-candidate arithmetic on designed inputs and prints inputs and results in hexadecimal; tests/test_acq_core_host.py holds
// every line against the same expression in numpy, bit for bit.  What it can check alone it checks here (exit status 1).
// Build: -std=c++17 -ffp-contract=off (the header's own pragma is clang's; with -ffp-contract=off any compiler rounds every product).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../pybo_amd/csrc/acq_core.h"

using namespace gpx;

static int failures = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
            ++failures;                                           \
        }                                                         \
    } while (0)

static void put(const std::vector<double>& v) {
    for (double x : v) printf(" %a", x);
}

// moments nrb ldp n rho bias | rows * ldp Q | rows * ldp P | q p mu s2 qR        rows = max(nrb, 1), qR = add_rowblocks<false> from 0.0
static void moments_case(int nrb, double rho, double bias, const std::vector<double>& qcol, const std::vector<double>& pcol) {
    const int ldp = 3, n = 1, rows = nrb > 0 ? nrb : 1;
    std::vector<double> Q((size_t)rows * ldp, 7.0e300), P((size_t)rows * ldp, -7.0e300);      // (the other columns: never to be read)
    for (int r = 0; r < rows; ++r) {
        Q[(size_t)r * ldp + n] = qcol[r];
        P[(size_t)r * ldp + n] = pcol[r];
    }
    const CandMoments c = cand_moments(Q.data(), P.data(), ldp, nrb, n, rho, bias);
    double qR = 0.0, unused = 0.0;
    add_rowblocks<false>(Q.data(), nullptr, ldp, nrb, n, qR, unused);
    CHECK(unused == 0.0);
    const CandMoments again = moments_of_sums(c.q, c.p, rho, bias);
    CHECK((again.mu == c.mu || c.mu != c.mu) && again.s2 == c.s2 && c.s2 >= S2_FLOOR);
    printf("moments %d %d %d %a %a", nrb, ldp, n, rho, bias);
    put(Q);
    put(P);
    printf(" %a %a %a %a %a\n", c.q, c.p, c.mu, c.s2, qR);
}

// ens n mode beta | n t0 | n t1 | value mu s2        (mode 0: s2 printed as 0)
static void ens_case(int mode, double beta, const std::vector<double>& t0, const std::vector<double>& t1) {
    const int n = (int)t0.size();
    double acc0 = 1.0e300, acc1 = -3.0;              // (junk: `first` must not read it; mode 0 must leave acc1 alone)
    for (int m = 0; m < n; ++m) ens_fold(mode, m == 0, t0[m], t1[m], acc0, acc1);
    if (mode == 0) CHECK(acc1 == -3.0);
    const double value = ens_value(mode, acc0, acc1, (double)n, beta);
    const double mu = ens_mean(acc0, (double)n);
    const double s2 = mode == 0 ? 0.0 : ens_mix_s2(mu, acc1, (double)n);
    if (mode == 0) CHECK(value == mu);
    else CHECK(value == ens_ucb(mu, s2, beta) && s2 >= 0.0);
    printf("ens %d %d %a", n, mode, beta);
    put(t0);
    put(t1);
    printf(" %a %a %a\n", value, mu, s2);
}

int main() {
    printf("floor %a\n", S2_FLOOR);
    // sums whose order of addition matters: ((0 + a) + b) + c over 1e16, 1, -1e16 and friends
    const double big = 1.0e16, nan = __builtin_nan("");
    const std::vector<std::vector<double>> cols = {{big, 1.0, -big}, {1.0, big, -big}, {big, -big, 1.0}, {5.0, big, -big},
                                                   {0.25, 0.5, 0.125}, {nan, 1.0, 2.0}, {3.0, 0.0, 0.0}};
    for (int nrb : {0, 1, 3})
        for (size_t a = 0; a < cols.size(); ++a) moments_case(nrb, 1.3, 0.2, cols[a], cols[(a + 1) % cols.size()]);
    moments_case(3, 1.0e-100, -0.5, {0.0, 0.0, 0.0}, {1.0, 2.0, 3.0});        // rho at the floor itself
    moments_case(0, 2.0, 0.0, {2.0}, {-0.0});                                 // rho - q = 0: the floor

    // the ensemble, n = 1, 2, 3, 10
    const std::vector<double> mus = {3.0000001, -1.75, 1.0e8, 0.1, 0.2, 0.3, -0.7, 1.0e-9, 2.5, -3.25};
    const std::vector<double> s2s = {1.0e-9, 0.3, 1.0e-3, 0.7, 1.1, 1.0e-100, 0.05, 2.0, 0.9, 0.01};
    for (int n : {1, 2, 3, 10})
        for (int start : {0, 2}) {
            if (start + n > 10 && start) continue;
            const std::vector<double> t0(mus.begin() + start, mus.begin() + start + n), t1(s2s.begin() + start, s2s.begin() + start + n);
            ens_case(0, 0.0, t0, t1);
            ens_case(1, 2.0, t0, t1);
        }
    ens_case(0, 0.0, {big, 1.0, -big}, {0.0, 0.0, 0.0});
    ens_case(0, 0.0, {1.0, big, -big}, {0.0, 0.0, 0.0});

    // the order: every pair of a small set, printed as a 0/1 matrix of better(row, column) after nan_last
    const double inf = __builtin_huge_val();
    const std::vector<double> ov = {1.0, inf, -inf, 0.0, -0.0, 1.0, nan, nan, -0.0, 0.0, inf, -inf};
    printf("orderset %d", (int)ov.size() + 1);
    for (size_t i = 0; i < ov.size(); ++i) printf(" %a %lld", ov[i], (long long)i);
    printf(" %a %lld\n", NEG_INF, (long long)IDX_NONE);
    for (size_t a = 0; a <= ov.size(); ++a) {
        printf("orderrow ");
        for (size_t b = 0; b <= ov.size(); ++b) {
            const double av = a < ov.size() ? nan_last(ov[a]) : NEG_INF, bv = b < ov.size() ? nan_last(ov[b]) : NEG_INF;
            const int64_t ai = a < ov.size() ? (int64_t)a : IDX_NONE, bi = b < ov.size() ? (int64_t)b : IDX_NONE;
            printf("%d", better(av, ai, bv, bi) ? 1 : 0);
        }
        printf("\n");
    }
    CHECK(nan_last(nan) == NEG_INF && nan_last(-0.0) == 0.0 && nan_last(inf) == inf);

    // a pick's scalars
    for (const auto& sv : std::vector<std::pair<double, double>>{{S2_FLOOR, 0.0}, {0.37, 1.0e-3}, {S2_FLOOR, 1.0e-6}}) {
        double scal[4] = {-1.0, -1.0, -1.0, -1.0};
        pick_scalars(sv.first, sv.second, scal);
        CHECK(scal[2] == 0.0 && scal[1] < inf && scal[0] > 0.0);
        printf("pick %a %a %a %a %a %a\n", sv.first, sv.second, scal[0], scal[1], scal[2], scal[3]);
    }

    // the batch fold, j = 0 (no cross term) and j = 3
    for (int j : {0, 3}) {
        const int64_t M = 2, n = 1;
        std::vector<double> V = {9.0, 0.1, 9.0, 1.0e16, 9.0, -0.3, 9.0, 0.77};      // rows 0 .. 3 of (4, M); row j holds vraw
        const std::vector<double> cross = {3.0, 1.0e-16, 0.7};
        const double invd = 1.0 / 3.0, vraw = V[(size_t)j * M + n], qprev = 0.4;
        printf("fold %d %a %a %a", j, invd, vraw, qprev);
        put(cross);
        for (int l = 0; l < 3; ++l) printf(" %a", V[(size_t)l * M + n]);
        const double q = batch_fold(j, M, n, V.data(), cross.data(), invd, vraw, qprev);
        CHECK(V[(size_t)j * M] == 9.0);
        printf(" %a %a\n", V[(size_t)j * M + n], q);
    }

    if (failures) return 1;
    printf("acq core ok\n");
    return 0;
}
