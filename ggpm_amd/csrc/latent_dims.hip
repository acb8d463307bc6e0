// The latent column by column ("Per-dimension KL"; include/ggpm_hip.h):
//   ggpm_latent_dim_accumulate  : per column the count and the sums over molecules of mean, mean^2, exp(lv) and the KL addend,
//                                 ADDED to a fp64 accumulator that lives across batches
//   ggpm_latent_dim_finish      : the accumulator -> per-column KL, mean and variance of the posterior means, mean posterior
//                                 variance, aggregate variance, and the number of active units
//   ggpm_free_bits_kl           : klbar_j = (1/B) sum_b w_b kl_dim[b, j] and the free-bits term sum_j max(lambda, klbar_j)
//   ggpm_free_bits_kl_backward  : that term's gradient by mean and pre_var, gated per column by klbar_j > lambda
// with lv = -|pre_var| and kl_dim[b, j] = -0.5 * (1 + lv - mean^2 - expf(lv)), the fp32 addend of csrc/mol_loss.hip's
// latent_terms_k and of ggpm_rsample_forward.  As there: one wave owns one output and its lanes stride the molecules; per-lane
// fp64 partials go through a fixed shuffle tree; every value is rounded to fp32 once, where it is stored; no atomics.
#include "common.h"

namespace {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// rsample's fp32 addend of the KL, times -0.5 (exact)
__device__ __forceinline__ double kl_dim_of(float m, float p) {
    const float lv = -fabsf(p);
    return -0.5 * (double)(1.f + lv - m * m - expf(lv));
}

// sum_b w_b kl_dim[b, j] / B of column j by the calling wave (every lane returns it).  The forward and the backward of the
// free-bits term both call THIS function -- one body of code, not two inlined copies the compiler may contract differently --
// so the two compare bit-identical values with lambda.
__device__ __noinline__ double column_klbar(const float* __restrict__ mean, const float* __restrict__ pv,
                                            const float* __restrict__ w, int B, int L, int j, int lane) {
    double acc = 0.0;
    for (int b = lane; b < B; b += 64) {
        const size_t i = (size_t)b * L + j;
        const double kd = kl_dim_of(mean[i], pv[i]);
        acc = fma(w ? (double)w[b] : 1.0, kd, acc);
    }
    return wave_sum_f64(acc) / (double)B;
}

// block = column j; the lanes stride the molecules.  Lane 0 adds the batch's five sums to the accumulator: launches on one
// stream are ordered and no other wave touches column j, so a plain read-add-write is enough.
__global__ void __launch_bounds__(64) latent_dim_accumulate_k(const float* __restrict__ mean, const float* __restrict__ pv, int B,
                                                              int L, double* __restrict__ acc) {
    const int j = blockIdx.x, lane = threadIdx.x;
    double s_m = 0.0, s_m2 = 0.0, s_e = 0.0, s_kl = 0.0;
    for (int b = lane; b < B; b += 64) {
        const size_t i = (size_t)b * L + j;
        const float m = mean[i], p = pv[i];
        s_m += (double)m;
        s_m2 += (double)m * (double)m;                         // exact in fp64
        s_e += (double)expf(-fabsf(p));
        s_kl += kl_dim_of(m, p);
    }
    s_m = wave_sum_f64(s_m);
    s_m2 = wave_sum_f64(s_m2);
    s_e = wave_sum_f64(s_e);
    s_kl = wave_sum_f64(s_kl);
    if (lane == 0) {
        acc[j] += (double)B;
        acc[(size_t)L + j] += s_m;
        acc[(size_t)2 * L + j] += s_m2;
        acc[(size_t)3 * L + j] += s_e;
        acc[(size_t)4 * L + j] += s_kl;
    }
}

// one wave; the lanes stride the columns.  A column is active when the mu_var it STORES exceeds the threshold, so n_active
// is the count a reader of `out` forms; integer addition makes the order of the count immaterial.
__global__ void __launch_bounds__(64) latent_dim_finish_k(const double* __restrict__ acc, int L, float au_threshold,
                                                          float* __restrict__ out, int32_t* __restrict__ n_active) {
    const int lane = threadIdx.x;
    int active = 0;
    for (int j = lane; j < L; j += 64) {
        const double n = acc[j];
        double kl = 0.0, mu = 0.0, var = 0.0, s2 = 0.0;
        if (n > 0.0) {
            kl = acc[(size_t)4 * L + j] / n;
            mu = acc[(size_t)L + j] / n;
            var = fmax(acc[(size_t)2 * L + j] / n - mu * mu, 0.0);
            s2 = acc[(size_t)3 * L + j] / n;
        }
        const float var32 = (float)var;
        out[j] = (float)kl;
        out[(size_t)L + j] = (float)mu;
        out[(size_t)2 * L + j] = var32;
        out[(size_t)3 * L + j] = (float)s2;
        out[(size_t)4 * L + j] = (float)(var + s2);
        active += (n > 0.0 && var32 > au_threshold) ? 1 : 0;       // nothing accumulated: inactive under any threshold
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) active += __shfl_xor(active, off);
    if (lane == 0) n_active[0] = active;
}

#define FREE_BITS_WAVES 16

// one workgroup of 16 waves: wave v owns the columns v, v + 16, ... and leaves their fp64 klbar in LDS; then wave 0 sums
// max(lambda, klbar_j) with its lanes striding j, and rounds once.
__global__ void __launch_bounds__(64 * FREE_BITS_WAVES) free_bits_kl_k(const float* __restrict__ mean, const float* __restrict__ pv,
                                                                       const float* __restrict__ w, int B, int L, float lambda,
                                                                       float* __restrict__ kl_dims, float* __restrict__ term) {
    __shared__ double klbar[GGPM_FREE_BITS_MAX_L];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int j = wave; j < L; j += FREE_BITS_WAVES) {
        const double v = column_klbar(mean, pv, w, B, L, j, lane);
        if (lane == 0) {
            klbar[j] = v;
            kl_dims[j] = (float)v;
        }
    }
    __syncthreads();
    if (wave == 0) {
        double acc = 0.0;
        for (int j = lane; j < L; j += 64) acc += fmax((double)lambda, klbar[j]);
        acc = wave_sum_f64(acc);
        if (lane == 0) term[0] = (float)acc;
    }
}

// block = column j; the lanes stride the molecules.  The gate is klbar_j > lambda on the forward's own fp64 klbar_j.  Rounding
// to nearest is monotone and lambda is a fp32 value, so a rounded kl_dims[j] above (below) lambda already says that klbar_j
// is above (below) it; only a rounded value EQUAL to lambda decides nothing, and without kl_dims the sum is always re-formed.
__global__ void __launch_bounds__(64) free_bits_kl_bwd_k(const float* __restrict__ mean, const float* __restrict__ pv,
                                                         const float* __restrict__ w, const float* __restrict__ kl_dims, int B,
                                                         int L, float lambda, const float* __restrict__ g,
                                                         float* __restrict__ dmean, float* __restrict__ dpv) {
    const int j = blockIdx.x, lane = threadIdx.x;
    bool open;
    if (kl_dims && kl_dims[j] != lambda)
        open = kl_dims[j] > lambda;
    else
        open = column_klbar(mean, pv, w, B, L, j, lane) > (double)lambda;
    const double gs = (g ? (double)g[0] : 1.0) / (double)B;
    for (int b = lane; b < B; b += 64) {
        const size_t i = (size_t)b * L + j;
        const float m = mean[i], p = pv[i];
        const double c = open ? gs * (w ? (double)w[b] : 1.0) : 0.0;
        dmean[i] = (float)(c * (double)m);
        const double dlv = -0.5 * c * (1.0 - (double)expf(-fabsf(p)));
        dpv[i] = (float)((p > 0.f ? -1.0 : (p < 0.f ? 1.0 : 0.0)) * dlv);          // d(-|p|)/dp = -sign(p)  (0 at p = 0)
    }
}

inline bool sizes_ok(int B, int L) { return B > 0 && L > 0 && (size_t)B * (size_t)L < ((size_t)1 << 31); }

}  // namespace

extern "C" int ggpm_latent_dim_accumulate(const float* mean, const float* pre_var, int B, int L, double* acc,
                                          ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!mean || !pre_var || !acc || !sizes_ok(B, L)) return GGPM_ERR_ARG;
    latent_dim_accumulate_k<<<L, 64, 0, (hipStream_t)stream>>>(mean, pre_var, B, L, acc);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_latent_dim_finish(const double* acc, int L, float au_threshold, float* out, int32_t* n_active,
                                      ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!acc || !out || !n_active || L <= 0 || (size_t)L * GGPM_LATENT_STAT_ROWS >= ((size_t)1 << 31) ||
        !(au_threshold == au_threshold))
        return GGPM_ERR_ARG;
    latent_dim_finish_k<<<1, 64, 0, (hipStream_t)stream>>>(acc, L, au_threshold, out, n_active);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_free_bits_kl(const float* mean, const float* pre_var, const float* w, int B, int L, float lambda,
                                 float* kl_dims, float* term, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!mean || !pre_var || !kl_dims || !term || !sizes_ok(B, L) || L > GGPM_FREE_BITS_MAX_L || !(lambda >= 0.f))
        return GGPM_ERR_ARG;
    free_bits_kl_k<<<1, 64 * FREE_BITS_WAVES, 0, (hipStream_t)stream>>>(mean, pre_var, w, B, L, lambda, kl_dims, term);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_free_bits_kl_backward(const float* mean, const float* pre_var, const float* w, const float* kl_dims_gate,
                                          int B, int L, float lambda, const float* g, float* dmean, float* dpre_var,
                                          ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!mean || !pre_var || !dmean || !dpre_var || !sizes_ok(B, L) || L > GGPM_FREE_BITS_MAX_L || !(lambda >= 0.f))
        return GGPM_ERR_ARG;
    free_bits_kl_bwd_k<<<L, 64, 0, (hipStream_t)stream>>>(mean, pre_var, w, kl_dims_gate, B, L, lambda, g, dmean, dpre_var);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}
