// Stand-alone host program around pybo_amd/csrc/ehvi_math.h, the header k_ehvi_fold includes: the strips of a front and one strip's fold
//  on the host.  tests/test_ehvi_host.py holds every result against pybo_amd/pareto.py and numpy, bit for bit.
//   ehvi_check                      the designed grid of ehvi_fold_term: every combination of the special values below, one line
//                                   "term acc e_prev e_next e2 result" each, in hexadecimal
//   ehvi_check strips IN            IN: r1, r2, then np raw points (f1, f2), doubles; prints "n <n>", then "a <hex>" n + 2 times and
//                                   "b <hex>" n + 1 times
//   ehvi_check fold IN OUT          IN: rows of 4 doubles (acc, e_prev, e_next, e2); OUT: one double per row
// What it can check alone it checks here (exit status 1).
// Build: -std=c++17 -ffp-contract=off (the header's own pragma is clang's; with -ffp-contract=off any compiler rounds every product).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../pybo_amd/csrc/ehvi_math.h"

using namespace gpx;

static int failures = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
            ++failures;                                           \
        }                                                         \
    } while (0)

static bool read_all(const char* path, std::vector<double>& v) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    double x;
    while (fread(&x, sizeof x, 1, f) == 1) v.push_back(x);
    fclose(f);
    return true;
}

static int strips_from_file(const char* in) {
    std::vector<double> v;
    if (!read_all(in, v) || v.size() < 2 || v.size() % 2 != 0) return 1;
    const int np = (int)(v.size() / 2) - 1;
    std::vector<double> a((size_t)np + 2), b((size_t)np + 1);
    const int n = ehvi_strips(v.data() + 2, np, v.data(), a.data(), b.data());
    CHECK(n >= 0 && n <= np);
    CHECK(a[0] == v[0] && b[(size_t)n] == v[1] && a[(size_t)n + 1] == __builtin_huge_val());
    for (int i = 0; i < n; ++i) CHECK(a[(size_t)i] < a[(size_t)i + 1] && b[(size_t)i] > b[(size_t)i + 1]);      // f1 ascending, f2 descending, strictly
    printf("n %d\n", n);
    for (int i = 0; i <= n + 1; ++i) printf("a %a\n", a[(size_t)i]);
    for (int i = 0; i <= n; ++i) printf("b %a\n", b[(size_t)i]);
    if (failures) return 1;
    printf("ehvi ok\n");
    return 0;
}

static int fold_from_file(const char* in, const char* out) {
    std::vector<double> v, res;
    if (!read_all(in, v) || v.size() % 4 != 0) return 1;
    for (size_t i = 0; i < v.size(); i += 4) res.push_back(ehvi_fold_term(v[i], v[i + 1], v[i + 2], v[i + 3]));
    FILE* g = fopen(out, "wb");
    if (!g) return 1;
    const size_t n = fwrite(res.data(), sizeof(double), res.size(), g);
    fclose(g);
    if (n != res.size()) return 1;
    printf("rows %zu\nehvi ok\n", res.size());
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "strips")) return strips_from_file(argv[2]);
    if (argc == 4 && !strcmp(argv[1], "fold")) return fold_from_file(argv[2], argv[3]);
    const double inf = __builtin_huge_val(), nan = __builtin_nan("");
    const std::vector<double> accs = {0.0, 1e-300, 0.75, nan};
    const std::vector<double> es = {0.0, -0.0, 5e-324, 1e-300, 0.1, 0.30000000000000004, 1.0, 1e300, inf, nan, -1e-17};
    const std::vector<double> e2s = {0.0, 5e-324, 1e-9, 3.0, 1e300, inf, nan};
    for (double acc : accs)
        for (double ep : es)
            for (double en : es)
                for (double e2 : e2s) {
                    const double r = ehvi_fold_term(acc, ep, en, e2);
                    printf("term %a %a %a %a %a\n", acc, ep, en, e2, r);
                    if (acc != acc || ep != ep || en != en || e2 != e2) CHECK(r != r);          // a NaN anywhere stays a NaN
                    else if (ep < en && e2 < inf) CHECK(r == acc);                             // a negative difference adds +0
                    else if (ep == inf && en == inf) CHECK(r != r);                            // inf - inf
                }
    CHECK(ehvi_fold_term(0.0, 1.0, 1.0, inf) != ehvi_fold_term(0.0, 1.0, 1.0, inf));      // 0 * inf
    if (failures) return 1;
    printf("ehvi ok\n");
    return 0;
}
