// Stand-alone host program around pybo_amd/csrc/acq_core.h, the header k_con_fold includes: the constraint fold of a constrained sweep
//  on the host.  tests/test_con_core_host.py holds every result against numpy's v * min(p, 1), bit for bit.
//   con_fold_check                      the designed grid: every pair of the special values below, one line "fold v p result" each, in hexadecimal
//   con_fold_check IN OUT J             IN: rows of 1 + J doubles (v_0, p_1 .. p_J); OUT: one double per row, v_J = the fold in order
// What it can check alone it checks here (exit status 1).
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

static int from_file(const char* in, const char* out, int J) {
    FILE* f = fopen(in, "rb");
    if (!f || J < 1) return 1;
    std::vector<double> row((size_t)(1 + J)), res;
    while (fread(row.data(), sizeof(double), row.size(), f) == row.size()) {
        double v = row[0];
        for (int j = 1; j <= J; ++j) v = con_fold(v, row[(size_t)j]);
        res.push_back(v);
    }
    fclose(f);
    FILE* g = fopen(out, "wb");
    if (!g) return 1;
    const size_t n = fwrite(res.data(), sizeof(double), res.size(), g);
    fclose(g);
    if (n != res.size()) return 1;
    printf("rows %zu\ncon fold ok\n", res.size());
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4) return from_file(argv[1], argv[2], atoi(argv[3]));
    const double inf = __builtin_huge_val(), nan = __builtin_nan(""), one_up = __builtin_nextafter(1.0, 2.0), one_down = __builtin_nextafter(1.0, 0.0);
    const std::vector<double> vs = {0.0, -0.0, 5e-324, 2.5e-320, 2.2250738585072014e-308, 1e-300, 1e-9, 0.3, 1.0, one_up, 3.0, 1e300, 1.7976931348623157e308, inf, nan};
    const std::vector<double> ps = {0.0, -0.0, 5e-324, 2.2250738585072014e-308, 1e-300, 1e-17, 0.25, 0.5, one_down, 1.0, one_up, 1.5, 1e300, inf, nan};
    for (double v : vs)
        for (double p : ps) {
            const double r = con_fold(v, p);
            printf("fold %a %a %a\n", v, p, r);
            if (v != v || p != p) CHECK(r != r);                        // NaN in either argument gives NaN
            else if (p >= 0.0 && v >= 0.0 && !(v == inf && p == 0.0)) CHECK(r <= v && r >= 0.0);
            if (p > 1.0 && v == v) CHECK(r == v);                         // the clamp: a factor above 1 is 1
        }
    if (failures) return 1;
    printf("con fold ok\n");
    return 0;
}
