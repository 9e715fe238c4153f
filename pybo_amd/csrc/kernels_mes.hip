// kernels_mes.hip -- the acquisition line of the sweep for max-value entropy search (GPX_ACQ_MES).
// A translation unit of its own only so that mes_math.h is compiled where it is used: k_acq_mes is k_acq's frame (acq_frame,
// acq_core_dev.h) with the MES value as its scoring step, so its moments -- and the sums a sweep cache is seeded with -- are the bits
// every other acquisition returns, by construction.
#include "acq_core_dev.h"
#include "gpx_internal.h"
#include "mes_math.h"

namespace gpx {

// The sum's add and the one division, as the ensemble's (kernels_ens.hip): plain operators, nothing fused into them.
// mes_add is Knuth's TwoSum: t = fl(a + b) and what the rounding dropped, exactly (finite a, b), added to `lost`.  A plain running sum
// of S equal terms is NOT S times the term -- 3 g already rounds -- so the sum carries its rounding errors along and returns them once,
// before the division: S equal samples then give the bits of one, for every power of two S, and S distinct ones lose one rounding, not S.
__device__ __forceinline__ double mes_add(double a, double b, double& lost) {
#pragma clang fp contract(off)
    const double t = a + b;
    const double bv = t - a;
    lost = lost + ((a - (t - bv)) + (b - bv));
    return t;
}
__device__ __forceinline__ double mes_div(double a, double b) {
#pragma clang fp contract(off)
    return a / b;
}

// The scoring step.  The maxima arrive by value (MesArg, a kernel argument): the index s is wave-uniform, the compiler reads y[s] on
// the scalar path.
// value = (g(c_0) + g(c_1) + ... + g(c_{S-1})) / S, c_s = (y*_s - mu) / sqrt(s2): summed in s ascending from g(c_0) with the roundings
// carried (mes_add), ONE division, no contraction -- equal samples sum exactly and a power-of-two S divides exactly
// (tests/test_gpu_mes.py).  An infinite term (c = -inf) makes the carried part NaN: the sum itself is returned then.
struct MesScore {
    const MesArg& ys;
    __device__ __forceinline__ double operator()(double mu, double s2) const {
        const double s = sqrt(s2);
        double acc = mes_g((ys.y[0] - mu) / s), lost = 0.0;
        for (int i = 1; i < ys.S; ++i) acc = mes_add(acc, mes_g((ys.y[i] - mu) / s), lost);
        double unused = 0.0;
        const double tot = mes_add(acc, lost, unused);
        return mes_div((tot == tot) ? tot : acc, (double)ys.S);
    }
};

__global__ __launch_bounds__(256) void k_acq_mes(const double* __restrict__ Qp, const double* __restrict__ Pp,
                                                 int64_t ldp, int nrb, int64_t m0, int64_t cols_valid,
                                                 double rho, double bias, const MesArg ys,
                                                 double* __restrict__ acq_out, double* __restrict__ mu_out,
                                                 double* __restrict__ s2_out, double* __restrict__ qsum,
                                                 double* __restrict__ psum) {
    acq_frame(Qp, Pp, ldp, nrb, m0, cols_valid, rho, bias, MesScore{ys}, acq_out, mu_out, s2_out, qsum, psum);
}

void launch_acq_mes(hipStream_t s, const double* Qp, const double* Pp, int64_t ldp, int nrb, int64_t m0,
                    int64_t cols_valid, double rho, double bias, const MesArg& ys, double* acq_out,
                    double* mu_out, double* s2_out, double* qsum, double* psum) {
    const unsigned g = (unsigned)((cols_valid + 255) / 256);
    hipLaunchKernelGGL(k_acq_mes, dim3(g), dim3(256), 0, s, Qp, Pp, ldp, nrb, m0, cols_valid, rho, bias, ys,
                       acq_out, mu_out, s2_out, qsum, psum);
}

}  // namespace gpx
