// kernels_bound32.hip -- the bound pass's dots in fp32 on the matrix pipe, with a per-candidate error margin.
// A translation unit of its own because it is compiled with -fno-slp-vectorize (build.sh): left to itself the compiler packs the
// adjacent fp32 additions and FMAs of the walk into v_pk_add_f32 / v_pk_fma_f32, which issue slower beside MFMAs, and keeps every
// broadcast operand twice (128 VGPRs and scratch where 70 to 100 do; profiles/bound_f32_ab.md).
#include <hip/hip_runtime.h>

#include "bound_f32.h"
#include "gpx_internal.h"
#include "gpx_math.h"

namespace gpx {

constexpr int BM32_XN = 128;                   // candidates of one workgroup (kernels_sweep.hip: XN)

// The same walk in fp32 ("the fp32 bound pass"; the margin: bound_f32.h).  The operands are the fp32 copies k_bound_aug
// wrote (coordinates and norms times log2(e)), the candidates' fragments are centred and scaled in fp64 as above and rounded once; the
// exponent comes from v_mfma_f32_16x16x4_f32 and v_exp_f32 is the exponential: no table, no limit (an exponent above 0 by its own
// error is inside the margin).  The rows come in sign-homogeneous tiles (bound_f32.h): tiles [0, tpos) hold only w >= 0, the rest only
// w <= 0, so a wave walks two loops with ONE FMA per entry, P += w k and then Nn += w k, and a lane forms A = P + Nn and B = P - Nn =
// sum |w| k in fp64 (profiles/bound_f32_ops_ab.md); the lanes' sums are combined in fp64 in k_bound_mfma's fixed order and
// out[n] = A + E / (1 - E) B + F rounded upward, an upper bound of the fp64 kernel's dot.
// FACT (where sc[FACT32] says so; the guard and its proof: bound_f32.h): the weights are w' = fl32(w 2^(-L |x~|^2 / 2)), the MFMA chain
// runs over the d coordinate slots from a zero accumulator -- no norm read, no addition per entry -- and the two fp64 sums are multiplied
// by the candidate's 2^(-L |z~|^2 / 2) once, after the walk.  One instance per KS: the unfactorised instance of the same launch returns at once.  A candidate whose |z~|^2 is not finite gets its NaN after the walk, as
// there; so does one whose fp32 norms overflow (inf - inf in the exponent), which only the forced kernel (prune_bound = 2) can meet:
// the guards keep R^2 below 2^25.  Either way the candidate is kept as a survivor.  C/D of the fp32 MFMA: col = l & 15, row = 4 (l >> 4) + r
// (the fp64 one: (l >> 4) + 4 r), so lane group g reads the weights and norms of rows 4 g .. 4 g + 3 of the tile as one 16-byte vector.
typedef float f4 __attribute__((ext_vector_type(4)));

// waves per SIMD (= workgroups per CU) the register allocation is held to: what each instance ran at with two FMAs per entry
// (profiles/bound_f32_ab.md); the factorised walk as the leaner of the two instances it stands in for
constexpr int bm32_waves(int KS, bool NC) { return NC ? (KS <= 2 ? 5 : 4) : (KS == 1 ? 8 : (KS == 4 ? 4 : (KS == 5 ? 5 : 7))); }

template <int KS, bool NC, bool FACT>
__global__ __launch_bounds__(256, bm32_waves(KS, NC)) void k_bound_mfma32(const float* __restrict__ A, const float* __restrict__ W4,
                                                          const float* __restrict__ NX4, int ntile, int d, const double* __restrict__ Z,
                                                          int64_t M, const double* __restrict__ invell, const double* __restrict__ cen,
                                                          const double* __restrict__ sc, double* __restrict__ out) {
    static_assert(!(FACT && NC), "the factorised walk reads no norms");
    __shared__ double redA[4][BM32_XN], redB[4][BM32_XN];
    if (sc[BM_SC_USE32] != 1.0 || (sc[BM_SC_FACT32] == 1.0) != FACT) return;
    const int tpos = (int)sc[BM_SC_TPOS32];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 15, g = lane >> 4;
    const int64_t n0 = (int64_t)blockIdx.x * BM32_XN;
    float b[8][KS], nz[NC ? 8 : 1];
    unsigned lost = 0;                        // bit j: column tile j's candidate has no finite |z~|^2
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int64_t n = n0 + j * 16 + col;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) b[j][ks] = 0.0f;
        double n2 = 0.0;
        if (n < M) {
            for (int k = 0; k < d; ++k) {
                const double v = bound_zt(Z[n * d + k], invell[k], cen[k]);
                n2 = fma(v, v, n2);
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) b[j][ks] = (k == 4 * ks + g) ? (float)v : b[j][ks];
            }
            if (!NC && !FACT) {               // (FACT: the two augmented slots stay 0 and the rows' entries there drop out)
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    b[j][ks] = (d == 4 * ks + g) ? 1.0f : b[j][ks];
                    b[j][ks] = (d + 1 == 4 * ks + g) ? (float)(B32_LOG2E * (-0.5 * n2)) : b[j][ks];
                }
            }
        }
        if (NC) nz[j] = (float)(B32_LOG2E * (-0.5 * n2));
        lost |= (n2 < __builtin_huge_val()) ? 0u : (1u << j);
    }
    float accP[8], accN[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) accP[j] = accN[j] = 0.0f;
    // byte offsets in 32 bits from the kernel's (scalar) pointers (A: 16 KS (Np + 16) bytes)
    unsigned ao = ((unsigned)w * KS * 64 + lane) * 4, wo = ((unsigned)w * 16 + g * 4) * 4;
    const auto ld1 = [](const float* p, unsigned o) { return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(p) + o); };
    const auto ld4 = [](const float* p, unsigned o) { return *reinterpret_cast<const f4*>(reinterpret_cast<const char*>(p) + o); };
    float a[KS], an[KS];
    f4 wv, wn, xv = {0.0f, 0.0f, 0.0f, 0.0f}, xn = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) an[ks] = ld1(A, ao + ks * 256);
    wn = ld4(W4, wo);
    if (NC) xn = ld4(NX4, wo);
    // one 16-row tile into the accumulators of its sign
    const auto tile = [&](float (&acc)[8], int t) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) a[ks] = an[ks];
        wv = wn;
        xv = xn;
        if (t + 4 < ntile) {                  // the next tile's operands while this one computes
            ao += 4 * KS * 64 * 4;
            wo += 4 * 16 * 4;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) an[ks] = ld1(A, ao + ks * 256);
            wn = ld4(W4, wo);
            if (NC) xn = ld4(NX4, wo);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            f4 c = {0.0f, 0.0f, 0.0f, 0.0f};
            if (NC) {
#pragma unroll
                for (int r = 0; r < 4; ++r) c[r] = xv[r] + nz[j];
            }
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ks], b[j][ks], c, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[j] = __builtin_fmaf(wv[r], __builtin_amdgcn_exp2f(c[r]), acc[j]);
        }
    };
    int t = w;
#pragma unroll 1
    for (; t < tpos; t += 4) tile(accP, t);   // w >= 0
#pragma unroll 1
    for (; t < ntile; t += 4) tile(accN, t);  // w <= 0
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        double va = (double)accP[j] + (double)accN[j], vb = (double)accP[j] - (double)accN[j];
        va += __shfl_xor(va, 16);
        va += __shfl_xor(va, 32);
        vb += __shfl_xor(vb, 16);
        vb += __shfl_xor(vb, 32);
        if (g == 0) {
            redA[w][j * 16 + col] = ((lost >> j) & 1u) ? __builtin_nan("") : va;
            redB[w][j * 16 + col] = vb;
        }
    }
    __syncthreads();
    if (threadIdx.x < BM32_XN) {
        const int64_t n = n0 + threadIdx.x;
        double sa = ((redA[0][threadIdx.x] + redA[1][threadIdx.x]) + redA[2][threadIdx.x]) + redA[3][threadIdx.x];
        double sb = ((redB[0][threadIdx.x] + redB[1][threadIdx.x]) + redB[2][threadIdx.x]) + redB[3][threadIdx.x];
        if (FACT) {                           // the candidate's norm factor, from |z~|^2 formed as in the prologue (no register held through the walk)
            double n2 = 0.0;
            if (n < M)
                for (int k = 0; k < d; ++k) {
                    const double v = bound_zt(Z[n * d + k], invell[k], cen[k]);
                    n2 = fma(v, v, n2);
                }
            const double cz = bound32_norm_factor(n2);
            sa *= cz;
            sb *= cz;
        }
        if (n < M) out[n] = (sa != sa) ? sa : bound32_hi(sa, sb, sc[BM_SC_FAC32], sc[BM_SC_FLUSH32]);
    }
}

void launch_bound_mfma32(hipStream_t s, const float* A32, const float* W32, const float* WF32, const float* NX32, int KS, bool nc, int ntile,
                         int d, const double* Z, int64_t M, const double* invell, const double* cen, const double* sc, double* out) {
    const dim3 grid((unsigned)((M + BM32_XN - 1) / BM32_XN));
#define GPX_BM32(K, C) hipLaunchKernelGGL((k_bound_mfma32<K, C, false>), grid, dim3(256), 0, s, A32, W32, NX32, ntile, d, Z, M, invell, cen, sc, out)
    switch (2 * KS + (nc ? 1 : 0)) {
        case 2: GPX_BM32(1, false); break;
        case 3: GPX_BM32(1, true); break;
        case 4: GPX_BM32(2, false); break;
        case 5: GPX_BM32(2, true); break;
        case 6: GPX_BM32(3, false); break;
        case 7: GPX_BM32(3, true); break;
        case 8: GPX_BM32(4, false); break;
        case 9: GPX_BM32(4, true); break;
        default: GPX_BM32(5, false); break;
    }
#undef GPX_BM32
#define GPX_BM32F(K) hipLaunchKernelGGL((k_bound_mfma32<K, false, true>), grid, dim3(256), 0, s, A32, WF32, nullptr, ntile, d, Z, M, invell, cen, sc, out)
    switch (KS) {                             // (the same k-steps: d coordinate slots fill (d + 3) / 4 of them either way)
        case 1: GPX_BM32F(1); break;
        case 2: GPX_BM32F(2); break;
        case 3: GPX_BM32F(3); break;
        case 4: GPX_BM32F(4); break;
        default: GPX_BM32F(5); break;
    }
#undef GPX_BM32F
}

}  // namespace gpx
