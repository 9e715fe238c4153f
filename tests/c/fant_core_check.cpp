// Stand-alone host program around the fantasised picks' arithmetic in pybo_amd/csrc/acq_core.h (fant_mean_step, fant_fold /
// fant_average, fant_incumbent), the header the kernels of kernels_batch.hip include.  It runs the functions on designed inputs,
// checks them here against long-double arithmetic and against the zero-innovation identity (exit status 1), and prints inputs and
// results in hexadecimal; tests/test_fant_core_host.py recomputes every line in numpy, bit for bit.
// Build: -std=c++17 -ffp-contract=off (the header's own pragma is clang's; with -ffp-contract=off any compiler rounds every product).
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../pybo_amd/csrc/acq_core.h"

using namespace gpx;

static int failures = 0;
#define CHECK(c)                                            \
    do {                                                    \
        if (!(c)) {                                         \
            fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
            ++failures;                                     \
        }                                                   \
    } while (0)

static const double EPS = 2.220446049250313e-16;

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

static void put(const std::vector<double>& v) {
    for (double x : v) printf(" %a", x);
}

// mean j mu | j v | j e | m          the walk of one fantasy's mean over the rows of V in pick order
static double mean_case(double mu, const std::vector<double>& v, const std::vector<double>& e) {
    const int j = (int)v.size();
    double m = mu;
    long double exact = mu, mag = fabsl((long double)mu);
    for (int l = 0; l < j; ++l) {
        m = fant_mean_step(m, v[l], e[l]);
        exact += (long double)v[l] * (long double)e[l];
        mag += fabsl((long double)v[l] * (long double)e[l]);
    }
    // j products and j additions, each rounded once: within 2 j eps of the exact sum relative to the terms' magnitudes
    CHECK(fabsl((long double)m - exact) <= 2.0L * j * EPS * mag);
    printf("mean %d %a", j, mu);
    put(v);
    put(e);
    printf(" %a\n", m);
    return m;
}

// avg S | S vals | value
static double avg_case(const std::vector<double>& vals) {
    const int S = (int)vals.size();
    double acc = 1.0e300;                                 // (junk: `first` must not read it)
    long double exact = 0.0L, mag = 0.0L;
    for (int s = 0; s < S; ++s) {
        fant_fold(s == 0, vals[s], acc);
        exact += vals[s];
        mag += fabsl((long double)vals[s]);
    }
    const double value = fant_average(acc, S);
    if (exact == exact) CHECK(fabsl((long double)value - exact / S) <= (long double)(S + 1) * EPS * mag / S);
    if (S == 1) CHECK(same_bits(value, vals[0]));         // dividing by 1.0 changes nothing
    printf("avg %d", S);
    put(vals);
    printf(" %a\n", value);
    return value;
}

// inc j cs es t mu s2 d | j cross | j + 1 eps | result          cross and eps are laid out with the strides cs, es (fillers between)
static double inc_case(double t, double mu, const std::vector<double>& cross, const std::vector<double>& eps, double s2, double d, int cs, int es) {
    const int j = (int)cross.size();
    std::vector<double> C((size_t)(j > 0 ? j : 1) * cs, 7.0e300), E((size_t)(j + 1) * es, -7.0e300);      // (the fillers: never to be read)
    for (int i = 0; i < j; ++i) C[(size_t)i * cs] = cross[i];
    for (int i = 0; i <= j; ++i) E[(size_t)i * es] = eps[i];
    const double r = fant_incumbent(t, mu, j, C.data(), cs, E.data(), es, s2, d);
    long double u = mu, mag = fabsl((long double)mu);
    for (int i = 0; i < j; ++i) {
        u += (long double)cross[i] * eps[i];
        mag += fabsl((long double)cross[i] * eps[i]);
    }
    u += (long double)s2 / d * eps[j];
    mag += fabsl((long double)s2 / d * eps[j]);
    const long double want = u > t ? u : (long double)t;
    if (u == u) CHECK(fabsl((long double)r - want) <= 2.0L * (j + 2) * EPS * mag);
    CHECK(r >= t || t != t);                               // an incumbent never falls
    printf("inc %d %d %d %a %a %a %a", j, cs, es, t, mu, s2, d);
    put(cross);
    put(eps);
    printf(" %a\n", r);
    return r;
}

int main() {
    const double big = 1.0e16, nan = __builtin_nan("");
    // the mean: zero innovations leave mu's bits, whatever the rows hold (the identity with the believer's batch)
    for (double mu : {0.2, -1.75, 3.0000001, 1.0e-300, 0.0}) {
        CHECK(same_bits(mean_case(mu, {}, {}), mu));
        CHECK(same_bits(mean_case(mu, {0.3, -1.0e3, 1.0e-200}, {0.0, 0.0, 0.0}), mu));
        CHECK(same_bits(mean_case(mu, {0.3, -2.5}, {0.0, -0.0}), mu));
    }
    // the order of the walk and the rounding of every product matter
    CHECK(mean_case(0.0, {big, 1.0, -big}, {1.0, 1.0, 1.0}) == 0.0);
    CHECK(mean_case(0.0, {big, -big, 1.0}, {1.0, 1.0, 1.0}) == 1.0);
    const double third = 1.0 / 3.0;
    CHECK(mean_case(-1.0, {3.0}, {third}) == 0.0);        // fl(3 * 1/3) = 1 first: a fused multiply-add would leave -2^-54
    mean_case(0.2, {0.11, -0.37, 0.051, 0.9, -0.013}, {0.47, -1.3, 2.2, -0.08, 0.6});
    std::vector<double> v63, e63;
    for (int l = 0; l < 63; ++l) {
        v63.push_back(0.5 * sin(1.0 + 0.37 * l) / (1.0 + 0.1 * l));
        e63.push_back(2.5 * cos(0.3 + 1.7 * l));
    }
    mean_case(-0.4, v63, e63);

    // the average over the fantasies: S = 1, 5, 16, 64, and sums whose order matters
    CHECK(avg_case({big, 1.0, -big}) == 0.0);
    CHECK(avg_case({1.0, big, -big}) == 0.0);
    CHECK(avg_case({big, -big, 1.0}) == third);
    for (int S : {1, 5, 16, 64}) {
        std::vector<double> vals;
        for (int s = 0; s < S; ++s) vals.push_back(0.05 * (1.0 + sin(0.9 * s)) + 1.0e-9 * s);
        avg_case(vals);
    }
    avg_case({0.0});
    avg_case({nan, 1.0});

    // the incumbents
    const std::vector<double> cross = {0.11, -0.37, 0.051}, eps = {0.47, -1.3, 2.2, 0.9};
    const double s2 = 0.37, sn2 = 1.0e-3;
    double scal[4];
    pick_scalars(s2, sn2, scal);
    const double a = inc_case(0.1, 0.25, cross, eps, s2, scal[0], 1, 1);
    CHECK(same_bits(a, inc_case(0.1, 0.25, cross, eps, s2, scal[0], 5, 3)));          // the strides change nothing
    CHECK(same_bits(inc_case(5.0, 0.25, cross, eps, s2, scal[0], 1, 64), 5.0));       // a higher incumbent stays
    CHECK(same_bits(inc_case(0.1, 0.25, {}, {-2.0}, s2, scal[0], 1, 1), 0.1));        // first pick, the observation came in low
    inc_case(0.1, 0.25, {}, {2.0}, s2, scal[0], 1, 1);
    CHECK(same_bits(inc_case(0.3, 0.25, cross, {0.0, 0.0, 0.0, 0.0}, s2, scal[0], 1, 1), 0.3));      // zero innovations: u = mu
    CHECK(same_bits(inc_case(0.2, 0.25, cross, {0.0, 0.0, 0.0, 0.0}, s2, scal[0], 1, 1), 0.25));
    CHECK(same_bits(inc_case(0.1, nan, cross, eps, s2, scal[0], 1, 1), 0.1));         // a NaN mean leaves the incumbent
    inc_case(-0.3, -0.2, {1.0e-3}, {0.5, -0.25}, S2_FLOOR, 1.0e-50, 1, 1);            // a pick on top of an observation, no noise

    if (failures) return 1;
    printf("fant core ok\n");
    return 0;
}
