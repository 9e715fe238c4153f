// ehvi_math.h -- expected hypervolume improvement of two independent objectives (Emmerich et al. 2011, Yang et al.
// 2019), maximisation.  The front cuts the region above the reference point r into n + 1 vertical strips [a_i, a_{i+1}) x [b_i, inf):
//     HVI(y) = sum_i [min(y1, a_{i+1}) - a_i]_+ [y2 - b_i]_+        EHVI = sum_i w_i EI_2(b_i),  w_i = max(EI_1(a_i) - EI_1(a_{i+1}), 0)
// with EI_j(t) the expected improvement of objective j over t and EI_1(+inf) := 0.
// (a) Plain C++ as acq_core.h (no HIP type; tests/c/ehvi_check.cpp includes this file): ehvi_strips, the filter and sort that turns raw
//     points into strips, run on the host by api.hip; ehvi_insert, one more point taken into the strips in place (the batch picks' front
//     follows them on the device); ehvi_fold_term, one strip's clamp, product and add, each rounded (GPX_NO_CONTRACT).
// (b) Device only: ehvi_value, the per-candidate loop of k_ehvi_fold and k_ehvi_batch_score.  Every EI is gpx_math.h's acq_value -- the bits of
//     gpx_sweep(GPX_ACQ_EI) -- so the kernel file includes gpx_math.h first and defines GPX_EHVI_DEVICE.
#ifndef GPX_EHVI_MATH_H
#define GPX_EHVI_MATH_H

#include <algorithm>
#include <utility>
#include <vector>

#include "acq_core.h"

namespace gpx {

constexpr int EHVI_MAX_FRONT = 1024;      // strips' points after filtering
constexpr int EHVI_MAX_RAW = 4096;        // raw points a call takes
constexpr int EHVI_STRIP_LD = EHVI_MAX_FRONT + 2;      // a_0 .. a_{n+1} at the cap

// The strips of the raw points P (np, 2) over the reference point r (2): drops every point not strictly above r in both coordinates,
// every point weakly dominated by another and all but one copy of equal points; the n survivors by f1 ascending (f2 is then strictly
// descending) give a[0] = r1, a[i] = f1 of point i, a[n + 1] = +inf and b[i] = f2 of point i + 1 (i < n), b[n] = r2.  Every output is a
// copy of an input double.  a holds np + 2 and b np + 1 doubles; returns n.  (Finite inputs: the caller's check.)
inline int ehvi_strips(const double* P, int np, const double* r, double* a, double* b) {
    std::vector<std::pair<double, double>> pts;
    for (int i = 0; i < np; ++i)
        if (P[2 * i] > r[0] && P[2 * i + 1] > r[1]) pts.push_back({P[2 * i], P[2 * i + 1]});
    // f1 descending, then f2 descending: a point survives exactly when its f2 exceeds every f2 met before it
    std::sort(pts.begin(), pts.end(), [](const std::pair<double, double>& x, const std::pair<double, double>& y) {
        return x.first > y.first || (x.first == y.first && x.second > y.second);
    });
    std::vector<std::pair<double, double>> front;
    for (const auto& p : pts)
        if (front.empty() || p.second > front.back().second) front.push_back(p);
    const int n = (int)front.size();
    a[0] = r[0];
    for (int i = 1; i <= n; ++i) a[i] = front[(size_t)(n - i)].first;
    a[n + 1] = __builtin_huge_val();
    for (int i = 0; i < n; ++i) b[i] = front[(size_t)(n - 1 - i)].second;
    b[n] = r[1];
    return n;
}

// One strip: acc + max(e_prev - e_next, 0) * e2 with e_prev = EI_1(a_i), e_next = EI_1(a_{i+1}), e2 = EI_2(b_i).  The clamp is a select on
// `< 0`, so a NaN difference stays NaN (and -0 stays -0); the product is rounded before it is added.
GPX_ACQ_FN double ehvi_fold_term(double acc, double e_prev, double e_next, double e2) {
    GPX_NO_CONTRACT;
    const double dif = e_prev - e_next;
    const double w = dif < 0.0 ? 0.0 : dif;
    const double t = w * e2;
    return acc + t;
}

// One more point y = (y1, y2) taken into the strips a[0 .. n + 1], b[0 .. n] in place, by ehvi_strips' own filtering rule: starting from
// ehvi_strips(P, r) and inserting y_0 .. y_{j-1} in order leaves the arrays of ehvi_strips(P + {y_0 .. y_{j-1}}, r), bit for bit (every
// output is a copy of an input double).  A y not strictly above r, or weakly dominated by (or equal to) a front point, changes nothing;
// otherwise the front points it weakly dominates -- one run [lo, end) of the order by f1 -- go and it takes their place.  Returns the
// new n <= n + 1: a must hold n + 3 and b n + 2 doubles.  No allocation, no container: the batch pick kernel runs the same text
// (kernels_batch.hip, one thread).  Point i = 1 .. n is (a[i], b[i - 1]): a ascending, b descending, a[n + 1] = +inf ends every search.
GPX_ACQ_FN int ehvi_insert(double* a, double* b, int n, double y1, double y2) {
    if (!(y1 > a[0] && y2 > b[n])) return n;
    int l = 1, h = n + 1;      // end: the first point with f1 > y1
    while (l < h) {
        const int mid = (l + h) / 2;
        if (a[mid] > y1) h = mid; else l = mid + 1;
    }
    const int end = l;
    const int at = (end > 1 && a[end - 1] == y1) ? end - 1 : end;      // the first point with f1 >= y1: of those, the one highest in f2
    if (at <= n && b[at - 1] >= y2) return n;
    l = 1, h = end;            // lo: the first point left of `end` with f2 <= y2
    while (l < h) {
        const int mid = (l + h) / 2;
        if (b[mid - 1] <= y2) h = mid; else l = mid + 1;
    }
    const int lo = l, shift = lo + 1 - end;      // the points from `end` on, a's +inf and b's r2 move by shift <= 1
    if (shift > 0) {
        for (int i = n + 1; i >= end; --i) a[i + 1] = a[i];
        for (int i = n; i >= end - 1; --i) b[i + 1] = b[i];
    } else if (shift < 0) {
        for (int i = end; i <= n + 1; ++i) a[i + shift] = a[i];
        for (int i = end - 1; i <= n; ++i) b[i + shift] = b[i];
    }
    a[lo] = y1;
    b[lo - 1] = y2;
    return n + shift;
}

#if defined(GPX_EHVI_DEVICE)      // (set by kernels_ehvi.hip and kernels_batch.hip after they have included gpx_math.h)
// EHVI of one candidate from its four moments and the strips a[0 .. n + 1], b[0 .. n]: the accumulator starts at +0.0, the strips are
// added in order i = 0 .. n, every EI_1(a_i) is computed once and carried to the next strip.  a[n + 1] is never read (EI_1(+inf) := 0).
__device__ __forceinline__ double ehvi_value(double mu1, double s2_1, double mu2, double s2_2, const double* a, const double* b, int n) {
    double acc = 0.0;
    double e_prev = acq_value(GPX_ACQ_EI, mu1, s2_1, a[0]);
    for (int i = 0; i <= n; ++i) {
        const double e_next = i < n ? acq_value(GPX_ACQ_EI, mu1, s2_1, a[i + 1]) : 0.0;
        const double e2 = acq_value(GPX_ACQ_EI, mu2, s2_2, b[i]);
        acc = ehvi_fold_term(acc, e_prev, e_next, e2);
        e_prev = e_next;
    }
    return acc;
}
#endif

}  // namespace gpx

#endif
