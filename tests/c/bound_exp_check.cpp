// Host checker of pybo_amd/csrc/bound_exp.h, the exponential of k_bound_mfma (tests/test_bound_exp_host.py, tests/test_gpu_bound_exp.py).
//   bound_exp_check                 the self-check: table, accuracy against long double expl, special values, monotonicity
//   bound_exp_check IN OUT          doubles of file IN -> bound_exp<false> of each (the kernel's variant) into file OUT
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <vector>

#include "../../pybo_amd/csrc/bound_exp.h"

using gpx::BEXP_NT;
using gpx::kBoundExpTab;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double uniform01() {                        // splitmix64, 53 bits
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    return (double)(z >> 11) * 0x1.0p-53;
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

static int from_file(const char* in, const char* out) {
    FILE* f = std::fopen(in, "rb");
    if (!f) return 2;
    std::vector<double> x;
    double buf[1024];
    size_t n;
    while ((n = std::fread(buf, 8, 1024, f)) > 0) x.insert(x.end(), buf, buf + n);
    std::fclose(f);
    for (double& v : x) v = gpx::bound_exp<false>(v, kBoundExpTab);
    f = std::fopen(out, "wb");
    if (!f) return 2;
    const bool ok = std::fwrite(x.data(), 8, x.size(), f) == x.size();
    return (std::fclose(f) == 0 && ok) ? 0 : 2;
}

int main(int argc, char** argv) {
    if (argc == 3) return from_file(argv[1], argv[2]);
    int bad = 0;
    // the table: 2^(j / NT) correctly rounded
    for (int j = 0; j < BEXP_NT; ++j)
        if (kBoundExpTab[j] != (double)exp2l((long double)j / BEXP_NT)) {
            std::printf("table entry %d is not the rounded 2^(%d/%d)\n", j, j, BEXP_NT);
            ++bad;
        }
    std::vector<double> x;
    for (int i = 0; i < 1500000; ++i) x.push_back(-60.0 * uniform01());
    for (int i = 0; i < 1500000; ++i) x.push_back(-746.0 * uniform01());
    for (int i = 0; i < 10000; ++i) x.push_back(-1e-3 * uniform01());
    int ngrid = 0;
    for (int k = -4 * BEXP_NT; k <= 0; ++k) {      // the grid points k ln2 / NT, where r changes sign: -1, 0, +1 ulp
        const double g = (double)((long double)k * 0.693147180559945309417232121458L / BEXP_NT);
        for (double v : {std::nextafter(g, -1e9), g, std::nextafter(g, 1e9)})
            if (v <= 0.0) {
                x.push_back(v);
                ++ngrid;
            }
    }
    for (double v : {0.0, -0.0, -745.2, -746.0}) x.push_back(v);
    std::sort(x.begin(), x.end());
    // the seams of j, (k - 1/2) ln2 / NT: accuracy holds there like anywhere; the two sides of a seam use two table entries, each rounded
    // on its own, so neighbouring doubles across a seam may come out one ulp in the wrong order.  Counted and printed, not part of the sorted sample.
    std::vector<double> seams;
    for (int k = -4 * BEXP_NT; k <= 0; ++k) {
        const double g = (double)(((long double)k - 0.5L) * 0.693147180559945309417232121458L / BEXP_NT);
        for (double v : {std::nextafter(g, -1e9), g, std::nextafter(g, 1e9)}) seams.push_back(v);
    }
    std::sort(seams.begin(), seams.end());
    double worst = 0.0, worst_x = 0.0;
    long nnormal = 0, nonmono = 0, seam_inv = 0;
    for (int pass = 0; pass < 2; ++pass) {
        const std::vector<double>& xs = pass ? seams : x;
        double prev = 0.0;
        for (size_t i = 0; i < xs.size(); ++i) {
            const double got = gpx::bound_exp<true>(xs[i], kBoundExpTab);
            if (!same_bits(got, gpx::bound_exp<false>(xs[i], kBoundExpTab))) {
                if (bad++ < 10) std::printf("the two clamps differ at %.17g\n", xs[i]);
            }
            if (i > 0 && got < prev) {
                if (pass) {
                    ++seam_inv;
                    if (got < std::nextafter(prev, 0.0)) bad += std::printf("seam inversion above one ulp at %.17g\n", xs[i]) > 0;
                } else if (nonmono++ < 10) {
                    std::printf("not monotone: f(%.17g) = %.17g < f(%.17g) = %.17g\n", xs[i], got, xs[i - 1], prev);
                }
            }
            prev = got;
            const long double want = expl((long double)xs[i]);
            if (want >= 0x1.0p-1022L) {
                int ex;
                frexpl(want, &ex);                                     // want = m 2^ex, m in [1/2, 1): ulp = 2^(ex - 53)
                const double err = (double)(fabsl((long double)got - want) / ldexpl(1.0L, ex - 53));
                ++nnormal;
                if (err > worst) {
                    worst = err;
                    worst_x = xs[i];
                }
            } else if (!(got >= 0.0 && got <= 0x1.0p-1021)) {
                if (bad++ < 10) std::printf("tail value %.17g at %.17g\n", got, xs[i]);
            }
        }
    }
    bad += nonmono > 0;
    const double one = gpx::bound_exp<true>(0.0, kBoundExpTab), onem = gpx::bound_exp<true>(-0.0, kBoundExpTab);
    if (!(one == 1.0 && onem == 1.0)) bad += std::printf("exp(+-0) = %.17g, %.17g\n", one, onem) > 0;
    for (double v : {-HUGE_VAL, -1e9, -746.0, -746.0000001}) {
        const double a = gpx::bound_exp<true>(v, kBoundExpTab), b = gpx::bound_exp<false>(v, kBoundExpTab);
        if (!(same_bits(a, 0.0) && same_bits(b, 0.0))) bad += std::printf("exp(%g) = %.17g, %.17g, not +0\n", v, a, b) > 0;
    }
    const double qn = std::nan("");
    if (!std::isnan(gpx::bound_exp<true>(qn, kBoundExpTab))) bad += std::printf("exp(NaN) is not NaN\n") > 0;
    if (!same_bits(gpx::bound_exp<false>(qn, kBoundExpTab), 0.0)) bad += std::printf("the kernel's variant at NaN is not the floor's 0\n") > 0;
    std::printf("arguments %zu (normal results %ld, grid points %d, seam points %zu)\n", x.size() + seams.size(), nnormal, ngrid, seams.size());
    std::printf("max error %.4f ulp at %.17g\n", worst, worst_x);
    std::printf("monotone violations %ld over the sorted sample, one-ulp inversions across seams %ld of %d\n", nonmono, seam_inv, 4 * BEXP_NT + 1);
    if (worst > 1.05) bad += std::printf("above 1.05 ulp\n") > 0;
    std::printf(bad ? "bound exp FAILED\n" : "bound exp ok\n");
    return bad ? 1 : 0;
}
