// Host checker of pybo_amd/csrc/kg_math.h, the knowledge gradient's line mathematics (tests/test_kg_host.py).
// Runs designed line sets and random ones with n = 1, 2, 3, 64, 128 lines through kg_value / kg_weights -- the statements the kernels
// of kernels_kg.hip run -- and prints one record per set, doubles in hexadecimal (no decimal conversion between the two sides):
//     set <tag> <n> <value> <a_0> <b_0> ... <a_{n-1}> <b_{n-1}>
// The Python side computes the 50-digit truth of every record and asserts the bound the header derives.  Checked here: the value is
// finite, >= 0 and not -0; the probabilities P_j of the lines sum to 1 and the weights w_j to 0 (to 1e-12); a line that is off has
// neither; the value does not move when the set is read through another accessor (strided storage, as the device's LDS tile).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../pybo_amd/csrc/kg_math.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double uniform01() {                        // splitmix64, 53 bits
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    return (double)(z >> 11) * 0x1.0p-53;
}
static double normal() {
    const double u = uniform01() + 0x1.0p-54, v = uniform01();
    return std::sqrt(-2.0 * std::log(u)) * std::cos(6.283185307179586 * v);
}

// the same lines behind a stride, as a tile [line][candidate] holds them
struct Strided {
    const double* al;
    const double* be;
    int stride;
    double a(int i) const { return al[i]; }
    double b(int i) const { return be[i * stride]; }
};

static int bad = 0, nsets = 0;

static void run(const char* tag, const std::vector<double>& a, const std::vector<double>& b) {
    const int n = (int)a.size();
    const gpx::KgArrays ln = {a.data(), b.data()};
    const double v = gpx::kg_value(n, ln);
    if (!(v >= 0.0) || !std::isfinite(v) || std::signbit(v)) bad += std::printf("%s: value %.17g\n", tag, v) > 0;
    std::vector<double> wide((size_t)n * 7, -1.0);
    for (int i = 0; i < n; ++i) wide[(size_t)i * 7] = b[i];
    const Strided st = {a.data(), wide.data(), 7};
    const double v2 = gpx::kg_value(n, st);
    if (std::memcmp(&v, &v2, 8) != 0) bad += std::printf("%s: strided access gives %.17g, not %.17g\n", tag, v2, v) > 0;
    double sp = 0.0, sw = 0.0;
    for (int j = 0; j < n; ++j) {
        double P, w, lo, hi;
        gpx::kg_weights(j, n, ln, P, w);
        const bool on = gpx::kg_interval(j, n, ln, lo, hi);
        if (!on && (P != 0.0 || w != 0.0)) bad += std::printf("%s: line %d is off but P = %g, w = %g\n", tag, j, P, w) > 0;
        if (P < -1e-15 || P > 1.0 + 1e-15) bad += std::printf("%s: P_%d = %.17g\n", tag, j, P) > 0;
        sp += P;
        sw += w;
    }
    if (std::fabs(sp - 1.0) > 1e-12 || std::fabs(sw) > 1e-12) bad += std::printf("%s: sum P = %.17g, sum w = %.3g\n", tag, sp, sw) > 0;
    std::printf("set %s %d %a", tag, n, v);
    for (int j = 0; j < n; ++j) std::printf(" %a %a", a[j], b[j]);
    std::printf("\n");
    ++nsets;
}

int main() {
    const int sizes[5] = {1, 2, 3, 64, 128};
    for (int n : sizes) {
        std::vector<double> a(n), b(n);
        // random sets at three scales of the slopes
        for (int rep = 0; rep < 6; ++rep) {
            const double sb = rep < 2 ? 1.0 : (rep < 4 ? 1e-3 : 30.0);
            for (int j = 0; j < n; ++j) a[j] = normal(), b[j] = sb * normal();
            run("random", a, b);
        }
        // all slopes equal: KG = 0, only the highest intercept (lowest index on a tie) is on
        for (int j = 0; j < n; ++j) a[j] = (double)((j * 7) % 5), b[j] = 0.25;
        run("equal_slopes", a, b);
        // all intercepts equal: every crossing at 0, KG = (b_max - b_min) / sqrt(2 pi)
        for (int j = 0; j < n; ++j) a[j] = -0.75, b[j] = normal();
        run("equal_intercepts", a, b);
        // duplicated lines: every line twice (a support point given twice, a candidate on a support point)
        for (int j = 0; j < n; ++j) a[j] = normal(), b[j] = normal();
        for (int j = 0; j + 1 < n; j += 2) a[j + 1] = a[j], b[j + 1] = b[j];
        run("duplicates", a, b);
        // three nearly concurrent lines through (z0, y0), the rest far below: the middle line's interval is empty to rounding
        for (int rep = 0; rep < 4; ++rep) {
            const double z0 = 0.3 + 0.4 * rep, y0 = 0.5;
            for (int j = 0; j < n; ++j) {
                b[j] = (j < 3) ? -1.0 + 1.1 * j + 0.01 * rep : 0.3 * normal();
                a[j] = (j < 3) ? y0 - b[j] * z0 : -50.0 - uniform01();
            }
            if (n >= 3 && rep >= 2) a[1] = std::nextafter(a[1], rep == 2 ? 10.0 : -10.0);
            run("concurrent", a, b);
        }
        // slopes of 1e-300: crossings overflow or are huge, products underflow
        for (int j = 0; j < n; ++j) a[j] = 1e-300 * normal() * (j % 3), b[j] = 1e-300 * normal();
        run("tiny_slopes", a, b);
        for (int j = 0; j < n; ++j) a[j] = normal(), b[j] = 1e-300 * (double)(j % 7);
        run("tiny_slopes_far", a, b);
        // crossings beyond |c| = 38: h underflows to +0
        for (int j = 0; j < n; ++j) a[j] = -45.0 * (double)j - uniform01(), b[j] = 1.0 + (double)j + 0.1 * uniform01();
        run("far_crossings", a, b);
        // crossings on both sides of the continued fraction's switch at |c| = 8 and of the cut at 39
        for (int j = 0; j < n; ++j) a[j] = -(7.5 + 0.25 * (double)(j % 9)) * (double)j, b[j] = (double)j;
        run("switch_8", a, b);
        for (int j = 0; j < n; ++j) a[j] = -(38.0 + 0.25 * (double)(j % 9)) * (double)j, b[j] = (double)j;
        run("cut_39", a, b);
    }
    std::printf("sets %d\n", nsets);
    std::printf(bad ? "kg math FAILED\n" : "kg math ok\n");
    return bad ? 1 : 0;
}
