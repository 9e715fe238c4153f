// Stand-alone host program around ehvi_insert of pybo_amd/csrc/ehvi_math.h, the text the batch pick kernel k_ehvi_batch_pick runs on the
// device: repeated insertion into the strips against ehvi_strips from scratch, bit for bit.
//   ehvi_insert_check               the designed streams below (equal points, points equal in one coordinate, on and below the reference
//                                   point's edges, dominating everything, dominated, into an empty front, growth to exactly 1024 points)
//   ehvi_insert_check stream IN     IN: r1, r2, np0 (as a double), np0 raw points (f1, f2), then the stream's points; prints "n <n>" of the
//                                   starting front and after every insertion, then "a <hex>" n + 2 times and "b <hex>" n + 1 times
// In both, after EVERY insertion the arrays must equal ehvi_strips of all raw points so far (exit status 1 otherwise).  The arrays hold
// exactly what the contract asks for -- a: n + 3, b: n + 2 doubles at the largest n the stream can reach -- so that a build with the
// address sanitizer sees any word written beyond them.
// Build: -std=c++17 -ffp-contract=off.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../pybo_amd/csrc/ehvi_math.h"

using namespace gpx;

static int failures = 0;
#define CHECK(c)                                            \
    do {                                                    \
        if (!(c)) {                                         \
            fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
            ++failures;                                     \
        }                                                   \
    } while (0)

// Inserts the stream (ns points) one by one into the strips of the np0 raw points P0 over r, comparing with ehvi_strips of everything so
// far after each; returns the final n and leaves the arrays in a / b.  ns_out (optional): n after every step, the start included.
static int run_stream(const double* r, const double* P0, int np0, const double* S, int ns, std::vector<double>& a, std::vector<double>& b,
                      std::vector<int>* ns_out) {
    std::vector<double> raw(P0, P0 + 2 * (size_t)np0);
    std::vector<double> a0((size_t)np0 + ns + 2), b0((size_t)np0 + ns + 1);
    int n = ehvi_strips(raw.data(), np0, r, a0.data(), b0.data());
    a.assign((size_t)n + ns + 2, -1.0), b.assign((size_t)n + ns + 1, -1.0);      // n + ns points at most: a n + ns + 2, b n + ns + 1
    memcpy(a.data(), a0.data(), ((size_t)n + 2) * 8), memcpy(b.data(), b0.data(), ((size_t)n + 1) * 8);
    if (ns_out) ns_out->push_back(n);
    const int before = failures;
    for (int k = 0; k < ns; ++k) {
        // (the contract's room for this step, n + 3 and n + 2, is there: n <= start + k)
        const int n2 = ehvi_insert(a.data(), b.data(), n, S[2 * k], S[2 * k + 1]);
        raw.push_back(S[2 * k]), raw.push_back(S[2 * k + 1]);
        const int want = ehvi_strips(raw.data(), np0 + k + 1, r, a0.data(), b0.data());
        CHECK(n2 == want);
        CHECK(n2 >= 0 && n2 <= n + 1);
        if (n2 == want) {
            CHECK(memcmp(a.data(), a0.data(), ((size_t)n2 + 2) * 8) == 0);
            CHECK(memcmp(b.data(), b0.data(), ((size_t)n2 + 1) * 8) == 0);
        }
        n = n2;
        if (ns_out) ns_out->push_back(n);
        if (failures != before) {
            fprintf(stderr, "stream step %d: point (%a, %a), n %d, from scratch %d\n", k, S[2 * k], S[2 * k + 1], n2, want);
            break;
        }
    }
    return n;
}

static bool read_all(const char* path, std::vector<double>& v) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    double x;
    while (fread(&x, sizeof x, 1, f) == 1) v.push_back(x);
    fclose(f);
    return true;
}

static int stream_from_file(const char* in) {
    std::vector<double> v;
    if (!read_all(in, v) || v.size() < 3) return 1;
    const int np0 = (int)v[2];
    if (np0 < 0 || v.size() < 3 + 2 * (size_t)np0 || (v.size() - 3) % 2 != 0) return 1;
    const int ns = (int)((v.size() - 3) / 2) - np0;
    std::vector<double> a, b;
    std::vector<int> steps;
    const int n = run_stream(v.data(), v.data() + 3, np0, v.data() + 3 + 2 * (size_t)np0, ns, a, b, &steps);
    for (int s : steps) printf("n %d\n", s);
    for (int i = 0; i <= n + 1; ++i) printf("a %a\n", a[(size_t)i]);
    for (int i = 0; i <= n; ++i) printf("b %a\n", b[(size_t)i]);
    if (failures) return 1;
    printf("ehvi insert ok\n");
    return 0;
}

static int designed(const std::vector<double>& r, const std::vector<double>& P0, const std::vector<double>& S) {
    std::vector<double> a, b;
    return run_stream(r.data(), P0.data(), (int)P0.size() / 2, S.data(), (int)S.size() / 2, a, b, nullptr);
}

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "stream")) return stream_from_file(argv[2]);
    const std::vector<double> r = {0.0, 0.0};
    const std::vector<double> F3 = {1.0, 3.0, 2.0, 2.0, 3.0, 1.0};
    // into an empty front: below, on the edges, then growth from both ends and the middle
    CHECK(designed(r, {}, {-1.0, 5.0, 0.0, 5.0, 5.0, 0.0, 0.0, 0.0, 2.0, 2.0, 1.0, 3.0, 3.0, 1.0, 1.5, 2.5, 2.5, 1.5}) == 5);
    // equal to a front point (each of them), twice
    CHECK(designed(r, F3, {1.0, 3.0, 2.0, 2.0, 3.0, 1.0, 2.0, 2.0}) == 3);
    // equal in f1 only: below (dominated) and above (replaces; the higher one also takes the left neighbour)
    CHECK(designed(r, F3, {2.0, 1.5, 2.0, 0.5}) == 3);
    CHECK(designed(r, F3, {2.0, 2.5}) == 3);
    CHECK(designed(r, F3, {2.0, 3.0}) == 2);
    CHECK(designed(r, F3, {2.0, 3.5}) == 2);
    CHECK(designed(r, F3, {3.0, 1.5, 3.0, 0.5, 1.0, 3.5, 1.0, 2.5}) == 3);
    // equal in f2 only: left (dominated) and right (replaces; the farther one also takes the right neighbour)
    CHECK(designed(r, F3, {1.5, 2.0, 0.5, 2.0}) == 3);
    CHECK(designed(r, F3, {2.5, 2.0}) == 3);
    CHECK(designed(r, F3, {3.0, 2.0}) == 2);
    CHECK(designed(r, F3, {3.5, 2.0}) == 2);
    CHECK(designed(r, F3, {0.5, 3.0, 1.5, 3.0, 3.5, 1.0, 2.5, 1.0}) == 3);
    // on the reference point's edges, below it, far away
    CHECK(designed(r, F3, {0.0, 9.0, 9.0, 0.0, 0.0, 0.0, -1.0, 9.0, 9.0, -1.0, -5.0, -5.0}) == 3);
    CHECK(designed({-4.0, -4.0}, {-3.0, -1.0, -2.0, -2.0, -1.0, -3.0}, {-4.0, -0.5, -3.5, -0.5, -0.5, -3.5, -2.5, -2.5, -1.5, -1.5}) == 5);
    // dominating the whole front, then dominated by it; dominating a run in the middle, at the left end, at the right end
    CHECK(designed(r, F3, {3.0, 3.0, 2.0, 2.0, 1.0, 1.0, 3.0, 3.0}) == 1);
    CHECK(designed(r, F3, {9.0, 9.0, 9.5, 8.0, 8.0, 9.5}) == 3);
    const std::vector<double> F6 = {1.0, 6.0, 2.0, 5.0, 3.0, 4.0, 4.0, 3.0, 5.0, 2.0, 6.0, 1.0};
    CHECK(designed(r, F6, {4.5, 4.5}) == 5);
    CHECK(designed(r, F6, {3.5, 6.5}) == 4);
    CHECK(designed(r, F6, {6.5, 3.5}) == 4);
    CHECK(designed(r, F6, {2.5, 4.5, 2.6, 4.6, 0.5, 6.5, 6.5, 0.5, 7.0, 7.0}) == 1);
    // neighbours one unit in the last place apart
    const double e = 2.220446049250313e-16;
    CHECK(designed(r, F3, {2.0 + 2 * e, 2.0, 2.0, 2.0 + 2 * e, 2.0 - e, 2.0 - e, 2.0 + 2 * e, 2.0 + 2 * e}) == 3);
    // growth to exactly 1024 points: a staircase of 1000, then 24 points between its steps, at capacity EHVI_STRIP_LD as on the device
    {
        std::vector<double> P, S;
        for (int i = 1; i <= 1000; ++i) P.push_back((double)i), P.push_back((double)(1001 - i));
        for (int k = 0; k < 24; ++k) S.push_back(40.0 * k + 0.5), S.push_back(1001.0 - 40.0 * k - 0.5);
        std::vector<double> a(EHVI_STRIP_LD), b(EHVI_STRIP_LD), a0(P.size() / 2 + 26), b0(P.size() / 2 + 25);
        int n = ehvi_strips(P.data(), 1000, r.data(), a.data(), b.data());
        CHECK(n == 1000);
        for (int k = 0; k < 24; ++k) {
            n = ehvi_insert(a.data(), b.data(), n, S[2 * (size_t)k], S[2 * (size_t)k + 1]);
            P.push_back(S[2 * (size_t)k]), P.push_back(S[2 * (size_t)k + 1]);
            CHECK(n == 1001 + k);
            CHECK(ehvi_strips(P.data(), 1001 + k, r.data(), a0.data(), b0.data()) == n);
            CHECK(memcmp(a.data(), a0.data(), ((size_t)n + 2) * 8) == 0 && memcmp(b.data(), b0.data(), ((size_t)n + 1) * 8) == 0);
        }
        CHECK(n == EHVI_MAX_FRONT && a[(size_t)n + 1] == __builtin_huge_val() && b[(size_t)n] == 0.0);
        // at the cap a point that changes nothing, and one that shrinks the front, still fit
        CHECK(ehvi_insert(a.data(), b.data(), n, 1.0, 1.0) == n);
        CHECK(ehvi_insert(a.data(), b.data(), n, 2000.0, 2000.0) == 1);
        CHECK(a[0] == 0.0 && a[1] == 2000.0 && a[2] == __builtin_huge_val() && b[0] == 2000.0 && b[1] == 0.0);
    }
    if (failures) return 1;
    printf("ehvi insert ok\n");
    return 0;
}
