// Host checker of pybo_amd/csrc/bound_f32.h, the error margin of k_bound_mfma32 (tests/test_bound_f32_host.py).
// It runs the kernel's arithmetic in float -- operands rounded once from the fp64 values, the exponent as an fmaf chain from the sum of
// the two norms (or from 0 with the norms as two more terms), exp2f for v_exp_f32 (its error term stays in the margin), two fmaf sums
// per lane in the kernel's order, the lanes combined in double -- and holds for every candidate of every case
//     dot_hi >= sum_i w_i k_i                      in long double, from the same fp64 centred coordinates;
//     dot_hi - sum_i w_i k_i <= 2 E sum_i |w_i| k_i + 3 F   (F once lost, once added, and the upward rounding);
// and that the guard refuses what the derivation does not cover.  Build with -ffp-contract=off; no arguments; exit status 0 = pass.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../pybo_amd/csrc/bound_f32.h"

namespace {

struct Rng {      // (a fixed generator: the cases are the same on every machine)
    uint64_t s;
    double uni() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(s >> 11) * 0x1p-53;
    }
    double gauss() {
        const double a = uni(), b = uni();
        return std::sqrt(-2.0 * std::log(a + 0x1p-60)) * std::cos(6.283185307179586 * b);
    }
};

struct Case {
    const char* name;
    int N, d, M;
    std::vector<double> X, Z, ell, w;      // observations (N x d), candidates (M x d), length scales (d), weights rho alpha2 (N)
    bool expect_refused;                   // the guard must decline
    bool expect_flush;                     // some covariance must come back as 0 where the truth is positive
};

Case problem(const char* name, int N, int d, int M, uint64_t seed) {
    Case c{name, N, d, M, {}, {}, {}, {}, false, false};
    Rng r{seed};
    c.X.resize((size_t)N * d);
    c.Z.resize((size_t)M * d);
    c.ell.resize(d);
    c.w.resize(N);
    for (double& v : c.X) v = r.uni();
    for (double& v : c.Z) v = r.uni();
    for (double& v : c.ell) v = (0.3 + 0.2 * r.uni()) * (d > 8 ? std::sqrt(d / 4.0) : 1.0);
    for (double& v : c.w) v = 1.3 * 20.0 * r.gauss();      // rho alpha2 of a smooth problem: both signs, tens in size
    return c;
}

struct Result {
    double E, worst_low, worst_high;      // min (dot_hi - truth) / (E B + F) and max (dot_hi - truth) / (2 E B + 3 F)
    bool used, flushed;
    int bad;
};

Result run(const Case& c) {
    const int N = c.N, d = c.d, M = c.M;
    const int Np = (N + 127) / 128 * 128;
    const bool nc = d > 0 && (d + 3) / 4 < (d + 5) / 4;
    const int KS = nc ? (d + 3) / 4 : (d + 5) / 4, K4 = 4 * KS;
    // k_bound_centre, k_bound_aug
    std::vector<double> cen(d), xt((size_t)Np * d, 0.0), nx(Np, 0.0);
    for (int k = 0; k < d; ++k) {
        double lo = HUGE_VAL, hi = -HUGE_VAL;
        for (int i = 0; i < N; ++i) {
            const double x = c.X[(size_t)i * d + k] * (1.0 / c.ell[k]);
            lo = std::fmin(lo, x);
            hi = std::fmax(hi, x);
        }
        cen[k] = 0.5 * lo + 0.5 * hi;
    }
    std::vector<float> a32((size_t)Np * K4, 0.0f), w32(Np, 0.0f), nx32(Np, 0.0f);
    double rx2 = 0.0, badw = 0.0, sum_w = 0.0;
    for (int i = 0; i < N; ++i) {
        double n2 = 0.0;
        for (int k = 0; k < d; ++k) {
            const double v = c.X[(size_t)i * d + k] * (1.0 / c.ell[k]) - cen[k];
            xt[(size_t)i * d + k] = v;
            n2 = std::fma(v, v, n2);
            a32[(size_t)i * K4 + k] = (float)(gpx::B32_LOG2E * v);
        }
        nx[i] = n2;
        if (!nc) {
            a32[(size_t)i * K4 + d] = (float)(gpx::B32_LOG2E * (-0.5 * n2));
            a32[(size_t)i * K4 + d + 1] = 1.0f;
        }
        nx32[i] = (float)(gpx::B32_LOG2E * (-0.5 * n2));
        w32[i] = (float)c.w[i];
        badw = std::fmax(badw, gpx::bound32_bad_weight(c.w[i]));
        sum_w += std::fabs(c.w[i]);
        rx2 = std::fmax(rx2, n2);
    }
    // k_bound_rz
    std::vector<double> zt((size_t)M * d), nz(M);
    double rz2 = 0.0;
    for (int n = 0; n < M; ++n) {
        double n2 = 0.0;
        for (int k = 0; k < d; ++k) {
            const double zs = c.Z[(size_t)n * d + k] * (1.0 / c.ell[k]);
            const double v = zs - cen[k];
            zt[(size_t)n * d + k] = v;
            n2 = std::fma(v, v, n2);
        }
        nz[n] = n2;
        rz2 = std::fmax(rz2, n2);
    }
    // k_bound_guard
    const double R = std::sqrt(rx2) + std::sqrt(rz2);
    const double gv = (double)(d + 4) * R * R;
    const double E = gpx::bound32_E(d, (double)(Np / 16), gv);
    const bool used = gv <= (double)Np && E <= gpx::B32_E_MAX && badw == 0.0;
    const double fac = gpx::bound32_factor(E, badw), F = gpx::bound32_flush(sum_w * (1.0 + 0x1p-20), (double)Np);
    Result res{E, HUGE_VAL, 0.0, used, false, 0};
    // k_bound_mfma32, one candidate at a time
    std::vector<float> b32(K4);
    for (int n = 0; n < M; ++n) {
        for (int k = 0; k < K4; ++k) b32[k] = 0.0f;
        for (int k = 0; k < d; ++k) b32[k] = (float)zt[(size_t)n * d + k];
        const float nz32 = (float)(gpx::B32_LOG2E * (-0.5 * nz[n]));
        if (!nc) {
            b32[d] = 1.0f;
            b32[d + 1] = nz32;
        }
        float accA[16], accB[16];      // [wave][row group]
        for (int p = 0; p < 16; ++p) accA[p] = accB[p] = 0.0f;
        long double truth = 0.0L, Bt = 0.0L;
        for (int i = 0; i < Np; ++i) {
            const int t = i / 16, row = i % 16, p = (t % 4) * 4 + (row / 4);      // C/D row = 4 g + r: tile order, then r, is index order
            float e = nc ? nx32[i] + nz32 : 0.0f;
            for (int k = 0; k < K4; ++k) e = std::fmaf(a32[(size_t)i * K4 + k], b32[k], e);
            const float kf = exp2f(e);
            accA[p] = std::fmaf(w32[i], kf, accA[p]);
            accB[p] = std::fmaf(std::fabs(w32[i]), kf, accB[p]);
            if (i < N) {
                long double r2 = 0.0L;
                for (int k = 0; k < d; ++k) {
                    const long double df = (long double)xt[(size_t)i * d + k] - (long double)zt[(size_t)n * d + k];
                    r2 += df * df;
                }
                const long double kt = expl(-0.5L * r2);
                truth += (long double)c.w[i] * kt;
                Bt += fabsl((long double)c.w[i]) * kt;
                if (kf == 0.0f && kt > 0.0L && c.w[i] != 0.0) res.flushed = true;
            }
        }
        double wa[4], wb[4];
        for (int w = 0; w < 4; ++w) {
            wa[w] = ((double)accA[4 * w] + (double)accA[4 * w + 1]) + ((double)accA[4 * w + 2] + (double)accA[4 * w + 3]);
            wb[w] = ((double)accB[4 * w] + (double)accB[4 * w + 1]) + ((double)accB[4 * w + 2] + (double)accB[4 * w + 3]);
        }
        const double sa = ((wa[0] + wa[1]) + wa[2]) + wa[3], sb = ((wb[0] + wb[1]) + wb[2]) + wb[3];
        const double hi = gpx::bound32_hi(sa, sb, fac, F);
        if (!(fac < HUGE_VAL)) {
            if (hi != HUGE_VAL) res.bad += std::printf("%s: candidate %d: no finite margin, yet dot_hi = %g\n", c.name, n, hi) > 0;
            continue;
        }
        const long double over = (long double)hi - truth;
        if (!(over >= 0.0L)) res.bad += std::printf("%s: candidate %d: dot_hi %.17g below the dot %.21Lg\n", c.name, n, hi, truth) > 0;
        const long double cap = 2.0L * (long double)E * Bt + 3.0L * (long double)F;
        if (!(over <= cap)) res.bad += std::printf("%s: candidate %d: dot_hi - dot %.6Lg above 2 E B + 3 F = %.6Lg\n", c.name, n, over, cap) > 0;
        res.worst_low = std::fmin(res.worst_low, (double)(over / ((long double)E * Bt + (long double)F)));
        res.worst_high = std::fmax(res.worst_high, (double)(over / cap));
    }
    return res;
}

}      // namespace

int main() {
    std::vector<Case> cases;
    const int ds[5] = {1, 2, 8, 9, 16};
    static char names[5][32];
    for (int i = 0; i < 5; ++i) {
        std::snprintf(names[i], sizeof names[i], "problem d=%d", ds[i]);
        cases.push_back(problem(names[i], 1000 + 7 * i, ds[i], 100, 1000 + ds[i]));
    }
    {      // a candidate on an observation: the exponent is 0 up to the form's cancellation, and may come out above it
        Case c = problem("on an observation", 300, 3, 64, 77);
        for (int k = 0; k < 3; ++k) c.Z[5 * 3 + k] = c.X[7 * 3 + k];
        cases.push_back(c);
    }
    {      // weights of alternating sign spanning 10^30, all normal in fp32
        Case c = problem("weights over 1e30", 384, 8, 64, 78);
        for (int i = 0; i < c.N; ++i) c.w[i] = ((i & 1) ? -1.0 : 1.0) * std::pow(10.0, -15.0 + 30.0 * i / (c.N - 1));
        cases.push_back(c);
    }
    {      // one weight that is subnormal in fp32: its rounding is not relative, the guard must refuse
        Case c = problem("subnormal weight", 300, 2, 64, 79);
        c.w[3] = 1e-40;
        c.expect_refused = true;
        cases.push_back(c);
    }
    {      // one weight beyond fp32's range
        Case c = problem("overflowing weight", 300, 2, 64, 80);
        c.w[11] = -1e39;
        c.expect_refused = true;
        cases.push_back(c);
    }
    {      // exponents beyond -87 inside the guard: d = 1, length scale 0.05, observations and candidates 20 length scales apart
        Case c = problem("exponents beyond -87", 2048, 1, 64, 81);
        c.ell[0] = 0.05;
        for (int i = 0; i < c.N; ++i) c.X[i] = (i == 0) ? 0.0 : (i == 1 ? 1.0 : c.X[i]);
        for (int n = 0; n < c.M; ++n) c.Z[n] = (n & 1) ? 0.001 * n : 1.0 - 0.001 * n;
        c.expect_flush = true;
        cases.push_back(c);
    }
    {      // far candidates: the margin still holds where the guard declines (option prune_bound = 2 runs the kernel there)
        Case c = problem("far candidates", 300, 2, 64, 82);
        for (int n = 0; n < 8; ++n) c.Z[n * 2] = 6.0 + n;
        c.expect_refused = true;
        cases.push_back(c);
    }
    int bad = 0;
    for (const Case& c : cases) {
        const Result r = run(c);
        std::printf("%-22s N %4d d %2d  E %.3e  %s  (dot_hi - dot) / (E B + F) >= %.4f  / (2 E B + 3 F) <= %.4f%s\n", c.name, c.N, c.d, r.E,
                    r.used ? "fp32   " : "refused", r.worst_low, r.worst_high, r.flushed ? "  flushed entries" : "");
        bad += r.bad;
        if (c.expect_refused == r.used) bad += std::printf("%s: the guard %s\n", c.name, r.used ? "let it run" : "refused") > 0;
        if (c.expect_flush && !r.flushed) bad += std::printf("%s: no covariance was flushed\n", c.name) > 0;
    }
    if (bad) return 1;
    std::printf("bound f32 ok %d cases\n", (int)cases.size());
    return 0;
}
