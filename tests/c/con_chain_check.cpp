// Stand-alone host program around pybo_amd/csrc/acq_core.h, the header k_con_batch_score includes: the chain of the constrained batch
//  on the host, the statements the device runs per candidate and member.  tests/test_con_batch_cpu.py holds every
// result against numpy's chain (tests/con_ref.py), bit for bit.
//   con_chain_check                     the designed grid: both starts of the chain over every pair of the special values below, one line
//                                       "chain has_obj t0 t1 result" each, in hexadecimal
//   con_chain_check IN OUT N HAS_OBJ    IN: rows of N doubles, the members' terms in order (HAS_OBJ 1: the objective's value first, then the
//                                       constraints' probabilities; 0: probabilities only); OUT: one double per row, the chain's value
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

// the members in order, as the kernel walks them; the first member's `v` is a NaN nobody may read
static double chain_of(const double* t, int n, int has_obj) {
    double v = __builtin_nan("");
    for (int m = 0; m < n; ++m) v = con_chain(m == 0, m < has_obj, v, t[m]);
    return v;
}

static bool same(double a, double b) { return (a != a && b != b) || (a == b && __builtin_signbit(a) == __builtin_signbit(b)); }

static int from_file(const char* in, const char* out, int n, int has_obj) {
    FILE* f = fopen(in, "rb");
    if (!f || n < 1 || has_obj < 0 || has_obj > 1) return 1;
    std::vector<double> row((size_t)n), res;
    while (fread(row.data(), sizeof(double), row.size(), f) == row.size()) res.push_back(chain_of(row.data(), n, has_obj));
    fclose(f);
    FILE* g = fopen(out, "wb");
    if (!g) return 1;
    const size_t w = fwrite(res.data(), sizeof(double), res.size(), g);
    fclose(g);
    if (w != res.size()) return 1;
    printf("rows %zu\ncon chain ok\n", res.size());
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 5) return from_file(argv[1], argv[2], atoi(argv[3]), atoi(argv[4]));
    const double inf = __builtin_huge_val(), nan = __builtin_nan(""), one_up = __builtin_nextafter(1.0, 2.0), one_down = __builtin_nextafter(1.0, 0.0);
    const std::vector<double> vs = {0.0, -0.0, 5e-324, 2.5e-320, 2.2250738585072014e-308, 1e-300, 1e-9, 0.3, one_down, 1.0, one_up, 3.0, 1e300, inf, nan};
    const std::vector<double> ps = {0.0, -0.0, 5e-324, 2.2250738585072014e-308, 1e-300, 1e-17, 0.25, 0.5, one_down, 1.0, one_up, 1.5, 1e300, inf, nan};
    for (int has_obj = 0; has_obj < 2; ++has_obj)
        for (double t0 : vs)
            for (double t1 : ps) {
                const double t[2] = {t0, t1};
                const double r = chain_of(t, 2, has_obj);
                printf("chain %d %a %a %a\n", has_obj, t0, t1, r);
                // the objective starts the chain at its own value, bits and all; a first constraint at con_fold(1, P)
                CHECK(same(chain_of(t, 1, 1), t0));
                CHECK(same(chain_of(t, 1, 0), con_fold(1.0, t0)));
                CHECK(same(r, con_fold(has_obj ? t0 : con_fold(1.0, t0), t1)));
                if (t0 != t0 || t1 != t1) CHECK(r != r);                    // a NaN term anywhere gives NaN
            }
    if (failures) return 1;
    printf("con chain ok\n");
    return 0;
}
