// Per-molecule likelihood terms ("Per-molecule ELBO and the importance-weighted bound"; include/ggpm_hip.h):
//   ggpm_mol_loss_parts : the row losses the loss kernels leave in `work`, summed per (molecule, term)
//   ggpm_latent_terms   : z_k = mean + exp(lv / 2) eps_k, the analytic KL, log p(z_k) - log q(z_k | x)
//   ggpm_iwae_finish    : ELBO and the K-sample importance-weighted bound (max-subtracted logsumexp over k)
// and what training on them needs ("Training on the bound"):
//   ggpm_bound_objective       : the weighted K-sample ELBO / IWAE loss and its partial derivatives c_nll, c_logpq, c_kl
//   ggpm_scale_rows_by_mol     : d[m, 0:N] *= g * coef[mol[m]], the chain rule of a per-molecule upstream gradient
//   ggpm_latent_terms_backward : the backward of ggpm_latent_terms, summed over k in a fixed order
// and the path-derivative estimators of the importance-weighted bound ("STL and DReG"):
//   ggpm_iwae_weights               : the normalised importance weights s = softmax_k(logpq - nll) and 1 / sum_k s^2
//   ggpm_latent_terms_backward_path : ggpm_latent_terms_backward with log q's parameters held fixed (STL), optionally with
//                                     every sample's addend weighted by s once more (DReG)
// One wave owns one output element and walks its addends in a fixed order: no atomics, bitwise reproducible.  Sums are
// carried in fp64 and rounded to fp32 once, where they are stored.
#include "common.h"

namespace {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}

struct LossTerms {
    const float* row_loss[GGPM_MOL_LOSS_TERMS];
    const int32_t* mol[GGPM_MOL_LOSS_TERMS];
    int stride[GGPM_MOL_LOSS_TERMS];
    int n_rows[GGPM_MOL_LOSS_TERMS];
};

// block = (molecule b, term t): the rows of a molecule are scattered (predictions are step-major), so the wave strides all
// rows of the term and keeps its own.  A row whose molecule is outside [0, B) belongs to no block.
__global__ void __launch_bounds__(64) mol_loss_parts_k(LossTerms a, float* __restrict__ parts) {
    const int b = blockIdx.x / GGPM_MOL_LOSS_TERMS, t = blockIdx.x % GGPM_MOL_LOSS_TERMS;
    const int lane = threadIdx.x;
    const float* __restrict__ v = a.row_loss[t];
    const int32_t* __restrict__ mol = a.mol[t];
    const int n = a.n_rows[t], st = a.stride[t];
    double acc = 0.0;
    for (int r = lane; r < n; r += 64)
        if (mol[r] == b) acc += (double)v[(size_t)r * st];
    acc = wave_sum_f64(acc);
    if (lane == 0) parts[blockIdx.x] = (float)acc;
}

// block = (sample k, molecule b).  z and the KL addends are formed in fp32 with rsample's own expressions (csrc/losses.hip:
// eps = 0 gives mean itself, and kl sums the values the training KL sums); logpq reads that stored z in fp64.
__global__ void __launch_bounds__(64) latent_terms_k(const float* __restrict__ mean, const float* __restrict__ pv,
                                                     const float* __restrict__ eps, int B, int L, float* __restrict__ z,
                                                     float* __restrict__ kl, float* __restrict__ logpq) {
    const int k = blockIdx.x / B, b = blockIdx.x - k * B;
    const int lane = threadIdx.x;
    const float* m = mean + (size_t)b * L;
    const float* p = pv + (size_t)b * L;
    const float* e = eps + (size_t)blockIdx.x * L;
    float* zo = z + (size_t)blockIdx.x * L;
    double s_kl = 0.0, s_pq = 0.0;
    for (int j = lane; j < L; j += 64) {
        const float mj = m[j], lv = -fabsf(p[j]), ej = e[j];
        const float zj = mj + expf(0.5f * lv) * ej;
        zo[j] = zj;
        s_pq += -0.5 * (double)zj * (double)zj + 0.5 * ((double)ej * (double)ej + (double)lv);
        s_kl += (double)(1.f + lv - mj * mj - expf(lv));      // rsample's fp32 addend: the KL of training adds the same values
    }
    s_pq = wave_sum_f64(s_pq);
    s_kl = wave_sum_f64(s_kl);
    if (lane == 0) {
        logpq[blockIdx.x] = (float)s_pq;
        if (k == 0) kl[b] = (float)(-0.5 * s_kl);
    }
}

// block = molecule b; the lanes stride the samples.
__global__ void __launch_bounds__(64) iwae_finish_k(const float* __restrict__ parts, const float* __restrict__ logpq,
                                                    const float* __restrict__ kl, int K, int B, float* __restrict__ elbo,
                                                    float* __restrict__ iwae) {
    const int b = blockIdx.x, lane = threadIdx.x;
    double s_nll = 0.0, mx = -INFINITY;
    for (int k = lane; k < K; k += 64) {
        const float* q = parts + ((size_t)k * B + b) * GGPM_MOL_LOSS_TERMS;
        const double nll = ((double)q[0] + (double)q[1]) + ((double)q[2] + (double)q[3]);
        s_nll += nll;
        mx = fmax(mx, (double)logpq[(size_t)k * B + b] - nll);
    }
    s_nll = wave_sum_f64(s_nll);
    mx = wave_max_f64(mx);
    double se = 0.0;
    for (int k = lane; k < K; k += 64) {
        const float* q = parts + ((size_t)k * B + b) * GGPM_MOL_LOSS_TERMS;
        const double nll = ((double)q[0] + (double)q[1]) + ((double)q[2] + (double)q[3]);
        se += exp((double)logpq[(size_t)k * B + b] - nll - mx);
    }
    se = wave_sum_f64(se);
    if (lane == 0) {
        elbo[b] = (float)(-s_nll / (double)K - (double)kl[b]);
        iwae[b] = (float)(mx + log(se) - log((double)K));
    }
}

// block = molecule b; the lanes stride the samples.  Writes the molecule's coefficients and its (unrounded) addend of the loss.
__global__ void __launch_bounds__(64) bound_objective_k(const float* __restrict__ parts, const float* __restrict__ logpq,
                                                        const float* __restrict__ kl, const float* __restrict__ w, int K, int B,
                                                        int objective, float beta, double* __restrict__ addend,
                                                        float* __restrict__ c_nll, float* __restrict__ c_logpq,
                                                        float* __restrict__ c_kl) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const double wb = w ? (double)w[b] : 1.0;
    if (objective == GGPM_BOUND_ELBO) {
        double s_nll = 0.0;
        for (int k = lane; k < K; k += 64) {
            const float* q = parts + ((size_t)k * B + b) * GGPM_MOL_LOSS_TERMS;
            s_nll += ((double)q[0] + (double)q[1]) + ((double)q[2] + (double)q[3]);
            c_nll[(size_t)k * B + b] = (float)(wb / ((double)K * (double)B));
            c_logpq[(size_t)k * B + b] = 0.f;
        }
        s_nll = wave_sum_f64(s_nll);
        if (lane == 0) {
            c_kl[b] = (float)((double)beta * wb / (double)B);
            addend[b] = wb * (s_nll / (double)K + (double)beta * (double)kl[b]);
        }
        return;
    }
    double mx = -INFINITY;
    for (int k = lane; k < K; k += 64) {
        const float* q = parts + ((size_t)k * B + b) * GGPM_MOL_LOSS_TERMS;
        const double nll = ((double)q[0] + (double)q[1]) + ((double)q[2] + (double)q[3]);
        mx = fmax(mx, (double)logpq[(size_t)k * B + b] - nll);
    }
    mx = wave_max_f64(mx);
    double se = 0.0;
    for (int k = lane; k < K; k += 64) {
        const float* q = parts + ((size_t)k * B + b) * GGPM_MOL_LOSS_TERMS;
        const double nll = ((double)q[0] + (double)q[1]) + ((double)q[2] + (double)q[3]);
        se += exp((double)logpq[(size_t)k * B + b] - nll - mx);
    }
    se = wave_sum_f64(se);
    for (int k = lane; k < K; k += 64) {
        const float* q = parts + ((size_t)k * B + b) * GGPM_MOL_LOSS_TERMS;
        const double nll = ((double)q[0] + (double)q[1]) + ((double)q[2] + (double)q[3]);
        const double c = wb * (exp((double)logpq[(size_t)k * B + b] - nll - mx) / se) / (double)B;
        c_nll[(size_t)k * B + b] = (float)c;
        c_logpq[(size_t)k * B + b] = (float)-c;
    }
    if (lane == 0) {
        c_kl[b] = 0.f;
        addend[b] = -wb * (mx + log(se) - log((double)K));
    }
}

// one wave: the molecules' addends in a fixed order, rounded once.
__global__ void __launch_bounds__(64) bound_loss_sum_k(const double* __restrict__ addend, int B, float* __restrict__ loss) {
    double acc = 0.0;
    for (int b = threadIdx.x; b < B; b += 64) acc += addend[b];
    acc = wave_sum_f64(acc);
    if (threadIdx.x == 0) loss[0] = (float)(acc / (double)B);
}

// wave = row m (four per block); the lanes stride its N columns.
__global__ void __launch_bounds__(256) scale_rows_by_mol_k(float* __restrict__ d, int ld, int M, int N,
                                                           const int32_t* __restrict__ mol, const float* __restrict__ coef,
                                                           int coef_stride, int B, const float* __restrict__ g) {
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (m >= M) return;
    const int b = mol[m];
    float s = 0.f;                                           // a row of no molecule counts nowhere: its gradient is 0
    if (b >= 0 && b < B) s = (g ? g[0] : 1.f) * coef[(size_t)b * coef_stride];
    float* row = d + (size_t)m * ld;
    for (int n = lane; n < N; n += 64) row[n] = (b >= 0 && b < B) ? row[n] * s : 0.f;
}

// block = (molecule b, column j); the lanes stride the samples.  z is re-formed with ggpm_latent_terms' fp32 expression.
__global__ void __launch_bounds__(64) latent_terms_bwd_k(const float* __restrict__ dz, const float* __restrict__ mean,
                                                         const float* __restrict__ pv, const float* __restrict__ eps,
                                                         const float* __restrict__ c_logpq, const float* __restrict__ c_kl,
                                                         const float* __restrict__ g, int K, int B, int L,
                                                         float* __restrict__ dmean, float* __restrict__ dpv) {
    const int b = blockIdx.x / L, j = blockIdx.x - b * L, lane = threadIdx.x;
    const size_t i = (size_t)b * L + j;
    const float m = mean[i], p = pv[i], lv = -fabsf(p);
    const float sd = expf(0.5f * lv);
    const double gs = g ? (double)g[0] : 1.0;
    double s_m = 0.0, s_lv = 0.0;
    for (int k = lane; k < K; k += 64) {
        const size_t kb = (size_t)k * B + b;
        const float e = eps[kb * L + j];
        const float z = m + sd * e;
        const double G = c_logpq ? gs * (double)c_logpq[kb] : 0.0;
        const double a = (dz ? (double)dz[kb * L + j] : 0.0) - G * (double)z;      // d/dz: the decoder's and logpq's -z
        s_m += a;
        s_lv += a * (0.5 * (double)sd * (double)e) + 0.5 * G;                      // z's exp(lv / 2) eps and logpq's + lv / 2
    }
    s_m = wave_sum_f64(s_m);
    s_lv = wave_sum_f64(s_lv);
    if (lane == 0) {
        const double gk = c_kl ? gs * (double)c_kl[b] : 0.0;
        dmean[i] = (float)(s_m + gk * (double)m);
        const double dlv = s_lv - 0.5 * gk * (1.0 - (double)expf(lv));
        dpv[i] = (float)((p > 0.f ? -1.0 : (p < 0.f ? 1.0 : 0.0)) * dlv);          // d(-|p|)/dp = -sign(p)  (0 at p = 0)
    }
}

// block = molecule b; the lanes stride the samples.  nll, the maximum and the sum are bound_objective_k's own expressions, so
// s is the softmax that kernel's coefficients hold; the effective sample size adds the squares of the unrounded weights.
__global__ void __launch_bounds__(64) iwae_weights_k(const float* __restrict__ parts, const float* __restrict__ logpq, int K,
                                                     int B, float* __restrict__ s, float* __restrict__ ess) {
    const int b = blockIdx.x, lane = threadIdx.x;
    double mx = -INFINITY;
    for (int k = lane; k < K; k += 64) {
        const float* q = parts + ((size_t)k * B + b) * GGPM_MOL_LOSS_TERMS;
        const double nll = ((double)q[0] + (double)q[1]) + ((double)q[2] + (double)q[3]);
        mx = fmax(mx, (double)logpq[(size_t)k * B + b] - nll);
    }
    mx = wave_max_f64(mx);
    double se = 0.0;
    for (int k = lane; k < K; k += 64) {
        const float* q = parts + ((size_t)k * B + b) * GGPM_MOL_LOSS_TERMS;
        const double nll = ((double)q[0] + (double)q[1]) + ((double)q[2] + (double)q[3]);
        se += exp((double)logpq[(size_t)k * B + b] - nll - mx);
    }
    se = wave_sum_f64(se);
    double s2 = 0.0;
    for (int k = lane; k < K; k += 64) {
        const float* q = parts + ((size_t)k * B + b) * GGPM_MOL_LOSS_TERMS;
        const double nll = ((double)q[0] + (double)q[1]) + ((double)q[2] + (double)q[3]);
        const double sk = exp((double)logpq[(size_t)k * B + b] - nll - mx) / se;
        s[(size_t)k * B + b] = (float)sk;
        s2 += sk * sk;
    }
    s2 = wave_sum_f64(s2);
    if (ess && lane == 0) ess[b] = (float)(1.0 / s2);
}

// block = (molecule b, column j); the lanes stride the samples.  z and sd are re-formed with ggpm_latent_terms' fp32
// expressions, as latent_terms_bwd_k does; r = exp(-lv / 2) is formed in fp64 from the fp32 lv (sd underflows long before r
// overflows, and the two are no exact reciprocals: the lv addend is written multiplied out, G eps^2 / 2).  A sample whose
// G eps is 0 -- a molecule of weight 0, a softmax weight that underflowed, eps = 0 -- takes no r product: 0 * inf never appears.
__global__ void __launch_bounds__(64) latent_terms_bwd_path_k(const float* __restrict__ dz, const float* __restrict__ mean,
                                                              const float* __restrict__ pv, const float* __restrict__ eps,
                                                              const float* __restrict__ c_logpq, const float* __restrict__ s,
                                                              const float* __restrict__ g, int K, int B, int L,
                                                              float* __restrict__ dmean, float* __restrict__ dpv) {
    const int b = blockIdx.x / L, j = blockIdx.x - b * L, lane = threadIdx.x;
    const size_t i = (size_t)b * L + j;
    const float m = mean[i], p = pv[i], lv = -fabsf(p);
    const float sd = expf(0.5f * lv);
    const double r = exp(-0.5 * (double)lv);
    const double gs = g ? (double)g[0] : 1.0;
    double s_m = 0.0, s_lv = 0.0;
    for (int k = lane; k < K; k += 64) {
        const size_t kb = (size_t)k * B + b;
        const float e = eps[kb * L + j];
        const float z = m + sd * e;
        const double G = c_logpq ? gs * (double)c_logpq[kb] : 0.0;
        const double t = (dz ? (double)dz[kb * L + j] : 0.0) - G * (double)z;      // d/dz: the decoder's and log p's -z
        const double Ge = G * (double)e;
        double a = t, v = t * (0.5 * (double)sd * (double)e);
        if (Ge != 0.0) {
            a += Ge * r;                                                           // d(-log q)/dz = eps / sd
            v += 0.5 * Ge * (double)e;                                             // ... times dz/dlv = sd eps / 2
        }
        const double q = s ? (double)s[kb] : 1.0;
        s_m += q * a;
        s_lv += q * v;
    }
    s_m = wave_sum_f64(s_m);
    s_lv = wave_sum_f64(s_lv);
    if (lane == 0) {
        dmean[i] = (float)s_m;
        dpv[i] = (float)((p > 0.f ? -1.0 : (p < 0.f ? 1.0 : 0.0)) * s_lv);         // d(-|p|)/dp = -sign(p)  (0 at p = 0)
    }
}

}  // namespace

extern "C" int ggpm_mol_loss_parts(const ggpm_mol_loss_term* terms, int B, float* parts, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!terms || !parts || B <= 0 || (size_t)B * GGPM_MOL_LOSS_TERMS >= ((size_t)1 << 31)) return GGPM_ERR_ARG;
    LossTerms a;
    for (int t = 0; t < GGPM_MOL_LOSS_TERMS; ++t) {
        const ggpm_mol_loss_term& s = terms[t];
        if (s.n_rows < 0 || (s.n_rows > 0 && (!s.row_loss || !s.mol || s.stride < 1))) return GGPM_ERR_ARG;
        a.row_loss[t] = s.row_loss;
        a.mol[t] = s.mol;
        a.stride[t] = s.stride;
        a.n_rows[t] = s.n_rows;
    }
    mol_loss_parts_k<<<B * GGPM_MOL_LOSS_TERMS, 64, 0, (hipStream_t)stream>>>(a, parts);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_latent_terms(const float* mean, const float* pre_var, const float* eps, int K, int B, int L, float* z,
                                 float* kl, float* logpq, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!mean || !pre_var || !eps || !z || !kl || !logpq || K < 1 || K > GGPM_LIKELIHOOD_MAX_K || B <= 0 || L <= 0 ||
        (size_t)K * (size_t)B >= ((size_t)1 << 31))
        return GGPM_ERR_ARG;
    latent_terms_k<<<K * B, 64, 0, (hipStream_t)stream>>>(mean, pre_var, eps, B, L, z, kl, logpq);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_iwae_finish(const float* parts, const float* logpq, const float* kl, int K, int B, float* elbo,
                                float* iwae, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!parts || !logpq || !kl || !elbo || !iwae || K < 1 || K > GGPM_LIKELIHOOD_MAX_K || B <= 0) return GGPM_ERR_ARG;
    iwae_finish_k<<<B, 64, 0, (hipStream_t)stream>>>(parts, logpq, kl, K, B, elbo, iwae);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_bound_objective(const float* parts, const float* logpq, const float* kl, const float* w, int K, int B,
                                    int objective, float beta, double* work, float* loss, float* c_nll, float* c_logpq,
                                    float* c_kl, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!parts || !logpq || !kl || !work || !loss || !c_nll || !c_logpq || !c_kl || K < 1 || K > GGPM_LIKELIHOOD_MAX_K ||
        B <= 0 || (size_t)K * (size_t)B >= ((size_t)1 << 31) || (objective != GGPM_BOUND_ELBO && objective != GGPM_BOUND_IWAE) ||
        !(beta == beta) || (objective == GGPM_BOUND_IWAE && beta != 1.f))
        return GGPM_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    bound_objective_k<<<B, 64, 0, s>>>(parts, logpq, kl, w, K, B, objective, beta, work, c_nll, c_logpq, c_kl);
    bound_loss_sum_k<<<1, 64, 0, s>>>(work, B, loss);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_scale_rows_by_mol(float* d, int ld, int M, int N, const int32_t* mol, const float* coef, int coef_stride,
                                      int B, const float* g, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!d || !mol || !coef || M <= 0 || N <= 0 || ld < N || B <= 0 || coef_stride < 1) return GGPM_ERR_ARG;
    scale_rows_by_mol_k<<<ggpm_ceil_div(M, 4), 256, 0, (hipStream_t)stream>>>(d, ld, M, N, mol, coef, coef_stride, B, g);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_latent_terms_backward(const float* dz, const float* mean, const float* pre_var, const float* eps,
                                          const float* c_logpq, const float* c_kl, const float* g, int K, int B, int L,
                                          float* dmean, float* dpre_var, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!mean || !pre_var || !eps || !dmean || !dpre_var || K < 1 || K > GGPM_LIKELIHOOD_MAX_K || B <= 0 || L <= 0 ||
        (size_t)B * (size_t)L >= ((size_t)1 << 31) || (size_t)K * (size_t)B >= ((size_t)1 << 31))
        return GGPM_ERR_ARG;
    latent_terms_bwd_k<<<B * L, 64, 0, (hipStream_t)stream>>>(dz, mean, pre_var, eps, c_logpq, c_kl, g, K, B, L, dmean, dpre_var);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_iwae_weights(const float* parts, const float* logpq, int K, int B, float* s, float* ess,
                                 ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!parts || !logpq || !s || K < 1 || K > GGPM_LIKELIHOOD_MAX_K || B <= 0 || (size_t)K * (size_t)B >= ((size_t)1 << 31))
        return GGPM_ERR_ARG;
    iwae_weights_k<<<B, 64, 0, (hipStream_t)stream>>>(parts, logpq, K, B, s, ess);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_latent_terms_backward_path(const float* dz, const float* mean, const float* pre_var, const float* eps,
                                               const float* c_logpq, const float* s, const float* g, int K, int B, int L,
                                               float* dmean, float* dpre_var, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!mean || !pre_var || !eps || !dmean || !dpre_var || K < 1 || K > GGPM_LIKELIHOOD_MAX_K || B <= 0 || L <= 0 ||
        (size_t)B * (size_t)L >= ((size_t)1 << 31) || (size_t)K * (size_t)B >= ((size_t)1 << 31))
        return GGPM_ERR_ARG;
    latent_terms_bwd_path_k<<<B * L, 64, 0, (hipStream_t)stream>>>(dz, mean, pre_var, eps, c_logpq, s, g, K, B, L, dmean, dpre_var);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}
