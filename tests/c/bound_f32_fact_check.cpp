// Host checker of the two changes to k_bound_mfma32's walk that pybo_amd/csrc/bound_f32.h proves (tests/test_bound_f32_fact_host.py):
// sign-homogeneous row tiles (one FMA per entry into P or Nn, A = P + Nn, B = P - Nn) and the factorised exponent (w' = fl32(w r_i),
// k' = 2^(L x~.z~) from a zero accumulator over the d coordinate slots, the sums times c_n).  It runs the kernel's arithmetic in float --
// the rows reordered by bound32_row_dest with the extra zero tile, per-lane partial sums in the kernel's order (wave = tile mod 4, lane
// group = row / 4), exp2f for v_exp_f32, the lanes combined in double -- and holds for every candidate of every case
//     dot_hi >= sum_i w_i k_i                      in long double, from the same fp64 centred coordinates;
//     dot_hi - sum_i w_i k_i <= 2 E sum_i |w_i| k_i + 3 F;
// that no lane's P or Nn sees more than Np / 16 FMAs with a non-zero weight, that the tiles before tpos hold no negative and the others no
// positive weight, and that the guards refuse what the derivation does not cover.  Every case runs both walks where they are allowed:
// the factorised one behind bound32_fact_ok and the weight flags, the unfactorised one behind the guard of bound_f32_check.cpp.
// Build with -ffp-contract=off; no arguments; exit status 0 = pass.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
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
    std::string name;
    int N, d, M;
    std::vector<double> X, Z, ell, w;      // observations (N x d), candidates (M x d), length scales (d), weights rho alpha2 (N)
    bool expect_fact;                      // the factorised walk's guard must pass
    bool expect_f32;                       // the fp32 kernel's own guard must pass
};

Case problem(const std::string& name, int N, int d, int M, uint64_t seed) {
    Case c{name, N, d, M, {}, {}, {}, {}, true, true};
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
    double E, X, worst_high[2];      // X = L R_x R_z; max (dot_hi - truth) / (2 E B + 3 F) of the unfactorised / factorised walk
    bool f32, fact;
    long long tpos;
    int bad;
};

Result run(const Case& c) {
    const int N = c.N, d = c.d, M = c.M;
    const int Np = (N + 127) / 128 * 128, Np32 = Np + gpx::B32_ZROWS, ntile = Np32 / 16;
    const bool nc = d > 0 && (d + 3) / 4 < (d + 5) / 4;
    const int KS = nc ? (d + 3) / 4 : (d + 5) / 4, K4 = 4 * KS;
    const char* name = c.name.c_str();
    // k_bound_centre
    std::vector<double> cen(d), xt((size_t)Np * d, 0.0);
    for (int k = 0; k < d; ++k) {
        double lo = HUGE_VAL, hi = -HUGE_VAL;
        for (int i = 0; i < N; ++i) {
            const double x = c.X[(size_t)i * d + k] * (1.0 / c.ell[k]);
            lo = std::fmin(lo, x);
            hi = std::fmax(hi, x);
        }
        cen[k] = 0.5 * lo + 0.5 * hi;
    }
    // k_bound_aug: the signs' counts, then every row to its place
    long long npos = 0, nzero = 0;
    for (int i = 0; i < Np; ++i) {
        const double wi = i < N ? c.w[i] : 0.0;
        npos += wi > 0.0;
        nzero += !(wi > 0.0 || wi < 0.0);
    }
    const long long tpos = gpx::bound32_tpos(npos);
    std::vector<float> a32((size_t)Np32 * K4, 0.0f), w32(Np32, 0.0f), wf32(Np32, 0.0f), nx32(Np32, 0.0f);
    std::vector<int> src(Np32, -1);      // the observation behind a row of the copies (-1: a padding or extra zero row)
    std::vector<char> written(Np32, 0);
    double rx2 = 0.0, badw = 0.0, badwf = 0.0, sum_w = 0.0;
    long long rank[3] = {0, 0, 0};
    Result res{0.0, 0.0, {0.0, 0.0}, false, false, tpos, 0};
    for (int i = 0; i < Np; ++i) {
        const bool live = i < N;
        const double wt = live ? c.w[i] : 0.0;
        const int sgn = wt > 0.0 ? 1 : (wt < 0.0 ? -1 : 0);
        const long long i32 = gpx::bound32_row_dest(sgn, rank[1 - sgn]++, npos, nzero);
        if (i32 < 0 || i32 >= Np32 || written[i32]) {
            res.bad += std::printf("%s: row %d goes to %lld, outside the copies or taken\n", name, i, i32) > 0;
            continue;
        }
        written[i32] = 1;
        double n2 = 0.0;
        for (int k = 0; k < d && live; ++k) {
            const double v = c.X[(size_t)i * d + k] * (1.0 / c.ell[k]) - cen[k];
            xt[(size_t)i * d + k] = v;
            n2 = std::fma(v, v, n2);
            a32[(size_t)i32 * K4 + k] = (float)(gpx::B32_LOG2E * v);
        }
        if (!nc && live) {
            a32[(size_t)i32 * K4 + d] = (float)(gpx::B32_LOG2E * (-0.5 * n2));
            a32[(size_t)i32 * K4 + d + 1] = 1.0f;
        }
        const double wf = wt * gpx::bound32_norm_factor(n2);
        nx32[i32] = live ? (float)(gpx::B32_LOG2E * (-0.5 * n2)) : 0.0f;
        w32[i32] = (float)wt;
        wf32[i32] = (float)wf;
        src[i32] = live ? i : -1;
        badw = std::fmax(badw, gpx::bound32_bad_weight(wt));
        badwf = std::fmax(badwf, gpx::bound32_bad_weight_fact(wt, wf));
        sum_w += std::fabs(wt);
        rx2 = std::fmax(rx2, n2);
    }
    for (long long e = npos; e < npos + gpx::B32_ZROWS; ++e)
        if (written[e]++) res.bad += std::printf("%s: the extra zero row %lld is taken\n", name, e) > 0;
    for (int i = 0; i < Np32; ++i) {
        if (!written[i]) res.bad += std::printf("%s: row %d of the copies was never written\n", name, i) > 0;
        const bool first = i / 16 < tpos;
        if (first ? w32[i] < 0.0f : w32[i] > 0.0f) res.bad += std::printf("%s: row %d (tile %d, tpos %lld) holds weight %g\n", name, i, i / 16, tpos, w32[i]) > 0;
    }
    // the rounding FMAs of one lane's P and Nn: wave = tile mod 4, four rows of a tile per lane
    for (int wv = 0; wv < 4; ++wv)
        for (int g = 0; g < 4; ++g) {
            int depth[2] = {0, 0};
            for (int t = wv; t < ntile; t += 4)
                for (int r = 0; r < 4; ++r) depth[t < tpos ? 0 : 1] += w32[t * 16 + 4 * g + r] != 0.0f;
            if (depth[0] > Np / 16 || depth[1] > Np / 16)
                res.bad += std::printf("%s: wave %d lane group %d: %d / %d rounding FMAs, more than Np / 16 = %d\n", name, wv, g, depth[0], depth[1], Np / 16) > 0;
        }
    // k_bound_rz
    std::vector<double> zt((size_t)M * d), nz(M);
    double rz2 = 0.0;
    for (int n = 0; n < M; ++n) {
        double n2 = 0.0;
        for (int k = 0; k < d; ++k) {
            const double v = c.Z[(size_t)n * d + k] * (1.0 / c.ell[k]) - cen[k];
            zt[(size_t)n * d + k] = v;
            n2 = std::fma(v, v, n2);
        }
        nz[n] = n2;
        rz2 = std::fmax(rz2, n2);
    }
    // k_bound_guard
    const double R = std::sqrt(rx2) + std::sqrt(rz2);
    const double gv = (double)(d + 4) * R * R;
    const double E = gpx::bound32_E(d, (double)(Np / 16), gv), sw = sum_w * (1.0 + 0x1p-20);
    res.E = E;
    res.X = gpx::B32_LOG2E * std::sqrt(rx2) * std::sqrt(rz2);
    res.f32 = gv <= (double)Np && E <= gpx::B32_E_MAX && badw == 0.0;
    res.fact = E <= gpx::B32_E_MAX && badw == 0.0 && badwf == 0.0 && gpx::bound32_fact_ok(rx2, rz2, sw) == 1.0;
    const double fac = gpx::bound32_factor(E, badw), F = gpx::bound32_flush(sw, (double)Np);
    // k_bound_mfma32, one candidate at a time, in both forms
    std::vector<float> b32(K4);
    for (int n = 0; n < M; ++n) {
        long double truth = 0.0L, Bt = 0.0L;
        for (int i = 0; i < N; ++i) {
            long double r2 = 0.0L;
            for (int k = 0; k < d; ++k) {
                const long double df = (long double)xt[(size_t)i * d + k] - (long double)zt[(size_t)n * d + k];
                r2 += df * df;
            }
            const long double kt = expl(-0.5L * r2);
            truth += (long double)c.w[i] * kt;
            Bt += fabsl((long double)c.w[i]) * kt;
        }
        for (int form = 0; form < 2; ++form) {
            const bool fact = form == 1;
            if (fact ? !res.fact : !(fac < HUGE_VAL)) continue;      // (the unfactorised walk: wherever its margin is finite, as under prune_bound = 2)
            for (int k = 0; k < K4; ++k) b32[k] = 0.0f;
            for (int k = 0; k < d; ++k) b32[k] = (float)zt[(size_t)n * d + k];
            const float nz32 = (float)(gpx::B32_LOG2E * (-0.5 * nz[n]));
            if (!nc && !fact) {
                b32[d] = 1.0f;
                b32[d + 1] = nz32;
            }
            const std::vector<float>& wv32 = fact ? wf32 : w32;
            float accP[16], accN[16];      // [wave][row group]
            for (int p = 0; p < 16; ++p) accP[p] = accN[p] = 0.0f;
            for (int i = 0; i < Np32; ++i) {
                const int t = i / 16, row = i % 16, p = (t % 4) * 4 + (row / 4);
                float e = (nc && !fact) ? nx32[i] + nz32 : 0.0f;
                for (int k = 0; k < K4; ++k) e = std::fmaf(a32[(size_t)i * K4 + k], b32[k], e);
                const float kf = exp2f(e);
                if (fact && !(kf >= 0x1p-126f && kf <= 0x1.fffffep+127f))
                    res.bad += std::printf("%s: candidate %d row %d: k' = %g is not a normal number behind the guard\n", name, n, i, kf) > 0;
                float& acc = t < tpos ? accP[p] : accN[p];
                acc = std::fmaf(wv32[i], kf, acc);
            }
            double wa[4], wb[4];
            for (int w = 0; w < 4; ++w) {
                double va[4], vb[4];
                for (int g = 0; g < 4; ++g) {
                    va[g] = (double)accP[4 * w + g] + (double)accN[4 * w + g];
                    vb[g] = (double)accP[4 * w + g] - (double)accN[4 * w + g];
                }
                wa[w] = (va[0] + va[1]) + (va[2] + va[3]);
                wb[w] = (vb[0] + vb[1]) + (vb[2] + vb[3]);
            }
            double sa = ((wa[0] + wa[1]) + wa[2]) + wa[3], sb = ((wb[0] + wb[1]) + wb[2]) + wb[3];
            if (fact) {
                const double cz = gpx::bound32_norm_factor(nz[n]);
                sa *= cz;
                sb *= cz;
            }
            const double hi = gpx::bound32_hi(sa, sb, fac, F);
            const long double over = (long double)hi - truth;
            if (!(over >= 0.0L)) res.bad += std::printf("%s: form %d candidate %d: dot_hi %.17g below the dot %.21Lg\n", name, form, n, hi, truth) > 0;
            const long double cap = 2.0L * (long double)E * Bt + 3.0L * (long double)F;
            if (!(over <= cap)) res.bad += std::printf("%s: form %d candidate %d: dot_hi - dot %.6Lg above 2 E B + 3 F = %.6Lg\n", name, form, n, over, cap) > 0;
            res.worst_high[form] = std::fmax(res.worst_high[form], (double)(over / cap));
        }
    }
    return res;
}

}      // namespace

int main() {
    std::vector<Case> cases;
    const int ds[5] = {1, 2, 8, 9, 16};
    const int N = 1000, M = 48;      // Np = 1024
    for (int i = 0; i < 5; ++i) {
        const int d = ds[i];
        const std::string sfx = " d=" + std::to_string(d);
        const uint64_t seed = 2000 + 16 * d;
        cases.push_back(problem("random" + sfx, N, d, M, seed));
        {
            Case c = problem("all positive" + sfx, N, d, M, seed + 1);
            for (double& v : c.w) v = std::fabs(v) + 1e-3;
            cases.push_back(c);
        }
        {
            Case c = problem("all negative" + sfx, 1024, d, M, seed + 2);      // N = Np: only the extra tile separates nothing from the negatives
            for (double& v : c.w) v = -std::fabs(v) - 1e-3;
            cases.push_back(c);
        }
        {
            Case c = problem("16 m positives" + sfx, 1024, d, M, seed + 3);    // N = Np and npos = 16 x 23: no zero row but the extra tile's
            for (int j = 0; j < c.N; ++j) c.w[j] = ((j % 64 < 23) ? 1.0 : -1.0) * (std::fabs(c.w[j]) + 1e-3);
            cases.push_back(c);
        }
        {
            Case c = problem("one positive" + sfx, N, d, M, seed + 4);
            for (int j = 0; j < c.N; ++j) c.w[j] = ((j == 517) ? 1.0 : -1.0) * (std::fabs(c.w[j]) + 1e-3);
            cases.push_back(c);
        }
        {
            Case c = problem("alternating" + sfx, N, d, M, seed + 5);
            for (int j = 0; j < c.N; ++j) c.w[j] = ((j & 1) ? -1.0 : 1.0) * (std::fabs(c.w[j]) + 1e-3);
            cases.push_back(c);
        }
        {
            Case c = problem("zero weights" + sfx, N, d, M, seed + 6);
            for (int j = 0; j < c.N; j += 3) c.w[j] = (j % 2) ? 0.0 : -0.0;
            cases.push_back(c);
        }
        {      // w is normal in fp32, w' = w r_i is not: the row farthest from the centre gets the smallest normal weight
            Case c = problem("subnormal w'" + sfx, N, d, M, seed + 7);
            c.w[5] = 0x1p-126;
            c.expect_fact = false;
            cases.push_back(c);
        }
        {      // L R_x R_z just inside 120 / (1 + 2^-10) and just outside: two observations and the candidates on a line through the centre
            for (int out = 0; out < 2; ++out) {
                Case c = problem(std::string(out ? "range outside" : "range inside") + sfx, N, d, M, seed + 8);
                for (double& v : c.w) v *= 1e-3;      // (sum_w small: the exponent's range binds, not the sum's)
                const double target = (out ? 120.5 : 119.5) / gpx::B32_LOG2E;      // R_x R_z
                const double rx = 3.0, rz = target / rx;
                for (int k = 0; k < d; ++k) {
                    for (int i = 0; i < c.N; ++i) c.X[(size_t)i * d + k] = c.ell[k] * (k ? 0.0 : (i == 0 ? -rx : (i == 1 ? rx : 0.5 * rx * (2.0 * i / c.N - 1.0))));
                    for (int n = 0; n < c.M; ++n) c.Z[(size_t)n * d + k] = c.ell[k] * (k ? 0.0 : (n == 0 ? rz : rz * (2.0 * n / c.M - 1.0)));
                }
                c.expect_fact = !out;
                c.expect_f32 = false;      // (gv > Np at these radii: only the forced kernel walks here, and the margin must hold for it)
                cases.push_back(c);
            }
        }
        {
            Case c = problem("on an observation" + sfx, N, d, M, seed + 9);
            for (int k = 0; k < d; ++k) c.Z[(size_t)5 * d + k] = c.X[(size_t)7 * d + k];
            cases.push_back(c);
        }
    }
    int bad = 0;
    for (const Case& c : cases) {
        const Result r = run(c);
        std::printf("%-24s N %4d d %2d  E %.3e  L Rx Rz %7.2f  tpos %2lld  %s %s  (dot_hi - dot) / (2 E B + 3 F) <= %.4f plain, %.4f fact\n", c.name.c_str(),
                    c.N, c.d, r.E, r.X, r.tpos, r.f32 ? "fp32   " : "refused", r.fact ? "fact   " : "unfact ", r.worst_high[0], r.worst_high[1]);
        bad += r.bad;
        if (c.expect_fact != r.fact) bad += std::printf("%s: the factorised walk's guard %s\n", c.name.c_str(), r.fact ? "let it run" : "refused") > 0;
        if (c.expect_f32 != r.f32) bad += std::printf("%s: the fp32 kernel's guard %s\n", c.name.c_str(), r.f32 ? "let it run" : "refused") > 0;
    }
    if (bad) return 1;
    std::printf("bound f32 fact ok %d cases\n", (int)cases.size());
    return 0;
}
