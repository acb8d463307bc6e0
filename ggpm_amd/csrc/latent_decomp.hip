// The KL split across the batch ("Splitting the KL"; include/ggpm_hip.h):
//   ggpm_latent_decomp            : per draw (k, i) the index-code mutual information, the total correlation and the
//                                   dimension-wise KL of minibatch-weighted sampling, the dimension-wise KL column by column,
//                                   and the two fp64 logsumexp stashes the backward reads
//   ggpm_latent_decomp_backward   : the gradient of sum_{k,i} (a mi + b tc + c3 dwkl) by z (row pass), mean and pre_var (column pass)
//   ggpm_latent_decomp_accumulate : the batch's count and sums of mi, tc, dwkl and of every column of dwkl_dim, ADDED to a fp64
//                                   accumulator that lives across batches
// with lv[j, l] = -|pre_var[j, l]| and ell[k, i, j, l] = -0.5 (log 2pi + lv[j, l] + (z[k, i, l] - mean[j, l])^2 exp(-lv[j, l])).
// As in csrc/latent_dims.hip: one wave owns one output and its lanes stride the other index; per-lane fp64 partials go through
// a fixed shuffle tree; every fp32 value is rounded once, where it is stored; no atomics.  Here ALL of ell, its sums, the
// logsumexps and the softmax weights are fp64 (exp / log on double, the fp32 inputs widened exactly): the three components
// are differences of log-densities of size L log(N B), which must not cancel away.
#include "wave_f64.h"

namespace {

#define DECOMP_WAVES 4

// log N(zv; mean, exp(lv)) of one column; d and iv are left for the gradient
__device__ __forceinline__ double ell_of(float zv, float m, float p, double& d, double& iv) {
    const double lv = -fabs((double)p);
    d = (double)zv - (double)m;
    iv = exp(-lv);
    return -0.5 * (LOG_2PI + lv + d * d * iv);
}

// S[j] = sum_l ell[k, i, j, l] by the calling wave (every lane returns it): lanes stride l, then the shuffle tree.  The
// forward and both passes of the backward call THIS function, so exp(S - A) is formed from the very S the forward's A holds.
__device__ __noinline__ double joint_row(const float* __restrict__ zr, const float* __restrict__ mean,
                                         const float* __restrict__ pv, int L, int j, int lane) {
    double acc = 0.0, d, iv;
    const size_t o = (size_t)j * L;
    for (int l = lane; l < L; l += 64) acc += ell_of(zr[l], mean[o + l], pv[o + l], d, iv);
    return wave_sum_f64(acc);
}

// block = draw (k, i), DECOMP_WAVES waves.  First every wave takes the molecules j = wave, wave + W, ... (lanes stride l) and
// folds S[j] into its logsumexp in that order; the waves' pairs are merged in wave order.  Then every wave takes the columns
// l = wave, wave + W, ... (lanes stride j, the pairs merged by the butterfly) and adds D[l] to its partial of sum_l D, and
// the waves' partials are added in wave order.
__global__ void __launch_bounds__(64 * DECOMP_WAVES) latent_decomp_k(const float* __restrict__ z, const float* __restrict__ mean,
                                                                    const float* __restrict__ pv, int B, int L, double log_nb,
                                                                    float* __restrict__ comps, float* __restrict__ dwkl_dim,
                                                                    double* __restrict__ lse_joint, double* __restrict__ lse_dim) {
    __shared__ double sh_m[DECOMP_WAVES], sh_s[DECOMP_WAVES], sh_d[DECOMP_WAVES], sh_diag, sh_logp;
    const int row = blockIdx.x, i = row % B;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* zr = z + (size_t)row * L;

    Lse a;
    a.m = -INFINITY;
    a.s = 0.0;
    for (int j = wave; j < B; j += DECOMP_WAVES) {
        const double S = joint_row(zr, mean, pv, L, j, lane);
        a = lse_push(a, S);
        if (j == i && lane == 0) sh_diag = S;
    }
    if (lane == 0) {
        sh_m[wave] = a.m;
        sh_s[wave] = a.s;
    }
    if (wave == 0) {
        double acc = 0.0;
        for (int l = lane; l < L; l += 64) acc += -0.5 * (LOG_2PI + (double)zr[l] * (double)zr[l]);
        acc = wave_sum_f64(acc);
        if (lane == 0) sh_logp = acc;
    }

    double dsum = 0.0;
    for (int l = wave; l < L; l += DECOMP_WAVES) {
        Lse c;
        c.m = -INFINITY;
        c.s = 0.0;
        const float zv = zr[l];
        for (int j = lane; j < B; j += 64) {
            double d, iv;
            c = lse_push(c, ell_of(zv, mean[(size_t)j * L + l], pv[(size_t)j * L + l], d, iv));
        }
        const double D = lse_value(wave_lse(c));
        dsum += D;
        if (lane == 0) {
            if (lse_dim) lse_dim[(size_t)row * L + l] = D;
            if (dwkl_dim) dwkl_dim[(size_t)row * L + l] = (float)(D - log_nb + 0.5 * (LOG_2PI + (double)zv * (double)zv));
        }
    }
    if (lane == 0) sh_d[wave] = dsum;
    __syncthreads();
    if (threadIdx.x == 0) {
        Lse t;
        t.m = sh_m[0];
        t.s = sh_s[0];
        double sumD = sh_d[0];
        for (int w = 1; w < DECOMP_WAVES; ++w) {
            Lse o;
            o.m = sh_m[w];
            o.s = sh_s[w];
            t = lse_merge(t, o);
            sumD += sh_d[w];
        }
        const double A = lse_value(t);
        if (lse_joint) lse_joint[row] = A;
        comps[(size_t)row * 3] = (float)(sh_diag - A + log_nb);
        comps[(size_t)row * 3 + 1] = (float)(A - sumD + (double)(L - 1) * log_nb);
        comps[(size_t)row * 3 + 2] = (float)(sumD - (double)L * log_nb - sh_logp);
    }
}

// the weight on ell[k, i, j, l]:  a [i == j] + (b - a) p + (c3 - b) r
__device__ __forceinline__ double weight_of(double a, double b, double c3, bool diag, double p, double r) {
    return (diag ? a : 0.0) + (b - a) * p + (c3 - b) * r;
}

// row pass: block = draw (k, i).  The waves leave p[j] = exp(S[j] - A) in LDS (wave w: j = w, w + W, ...), then take the
// columns l = w, w + W, ... with their lanes striding j.
__global__ void __launch_bounds__(64 * DECOMP_WAVES) latent_decomp_bwd_row_k(const float* __restrict__ z, const float* __restrict__ mean,
                                                                            const float* __restrict__ pv,
                                                                            const double* __restrict__ lse_joint,
                                                                            const double* __restrict__ lse_dim,
                                                                            const float* __restrict__ coef, int B, int L,
                                                                            float* __restrict__ dz) {
    __shared__ double p[GGPM_LATENT_DECOMP_MAX_B];
    const int row = blockIdx.x, i = row % B;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* zr = z + (size_t)row * L;
    const double A = lse_joint[row];
    const double a = (double)coef[(size_t)row * 3], b = (double)coef[(size_t)row * 3 + 1], c3 = (double)coef[(size_t)row * 3 + 2];
    for (int j = wave; j < B; j += DECOMP_WAVES) {
        const double S = joint_row(zr, mean, pv, L, j, lane);
        if (lane == 0) p[j] = exp(S - A);
    }
    __syncthreads();
    for (int l = wave; l < L; l += DECOMP_WAVES) {
        const float zv = zr[l];
        const double D = lse_dim[(size_t)row * L + l];
        double acc = 0.0;
        for (int j = lane; j < B; j += 64) {
            double d, iv;
            const double e = ell_of(zv, mean[(size_t)j * L + l], pv[(size_t)j * L + l], d, iv);
            acc += weight_of(a, b, c3, j == i, p[j], exp(e - D)) * (-d * iv);
        }
        acc = wave_sum_f64(acc);
        if (lane == 0) dz[(size_t)row * L + l] = (float)(acc + c3 * (double)zv);
    }
}

// column pass: block = (molecule j, tile of 64 columns); lane = column tile * 64 + lane.  Wave w takes the draws
// n = w, w + W, ... of the K B in that order: S[n, j] over ALL columns (which passes the lane's own column, kept on the way),
// p, then the lane's two addends.  The waves' partials are added in wave order by wave 0.
__global__ void __launch_bounds__(64 * DECOMP_WAVES) latent_decomp_bwd_col_k(const float* __restrict__ z, const float* __restrict__ mean,
                                                                            const float* __restrict__ pv,
                                                                            const double* __restrict__ lse_joint,
                                                                            const double* __restrict__ lse_dim,
                                                                            const float* __restrict__ coef, int K, int B, int L,
                                                                            float* __restrict__ dmean, float* __restrict__ dpv) {
    __shared__ double sh_m[DECOMP_WAVES][64], sh_v[DECOMP_WAVES][64];
    const int j = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int mine = blockIdx.y * 64 + lane;                    // may lie past L in the last tile
    const size_t o = (size_t)j * L;
    const int rows = K * B;
    double acc_m = 0.0, acc_v = 0.0;
    for (int n = wave; n < rows; n += DECOMP_WAVES) {
        const float* zr = z + (size_t)n * L;
        double S = 0.0, e_mine = 0.0, d_mine = 0.0, iv_mine = 0.0;
        for (int l = lane; l < L; l += 64) {
            double d, iv;
            const double e = ell_of(zr[l], mean[o + l], pv[o + l], d, iv);
            S += e;
            if (l == mine) {
                e_mine = e;
                d_mine = d;
                iv_mine = iv;
            }
        }
        S = wave_sum_f64(S);
        if (mine < L) {
            const double a = (double)coef[(size_t)n * 3], b = (double)coef[(size_t)n * 3 + 1], c3 = (double)coef[(size_t)n * 3 + 2];
            const double G = weight_of(a, b, c3, n % B == j, exp(S - lse_joint[n]), exp(e_mine - lse_dim[(size_t)n * L + mine]));
            acc_m += G * (d_mine * iv_mine);
            acc_v += G * (-0.5 + 0.5 * d_mine * d_mine * iv_mine);
        }
    }
    sh_m[wave][lane] = acc_m;
    sh_v[wave][lane] = acc_v;
    __syncthreads();
    if (wave == 0 && mine < L) {
        double m = sh_m[0][lane], v = sh_v[0][lane];
        for (int w = 1; w < DECOMP_WAVES; ++w) {
            m += sh_m[w][lane];
            v += sh_v[w][lane];
        }
        const float pj = pv[o + mine];
        dmean[o + mine] = (float)m;
        dpv[o + mine] = (float)((pj > 0.f ? -1.0 : (pj < 0.f ? 1.0 : 0.0)) * v);      // d(-|p|)/dp = -sign(p)  (0 at p = 0)
    }
}

// block = one cell of the accumulator behind the count: the sums of mi, tc, dwkl (blocks 0 .. 2), then the columns of dwkl_dim.
// The lanes stride the draws.  Lane 0 adds to the accumulator: launches on one stream are ordered and no other wave touches the
// cell, so a plain read-add-write is enough.
__global__ void __launch_bounds__(64) latent_decomp_accumulate_k(const float* __restrict__ comps, const float* __restrict__ dwkl_dim,
                                                                 int rows, int L, double* __restrict__ acc) {
    const int cell = blockIdx.x, lane = threadIdx.x;
    const float* src = cell < 3 ? comps + cell : dwkl_dim + (cell - 3);
    const int ld = cell < 3 ? 3 : L;
    double s = 0.0;
    for (int n = lane; n < rows; n += 64) s += (double)src[(size_t)n * ld];
    s = wave_sum_f64(s);
    if (lane == 0) {
        if (cell == 0) acc[0] += (double)rows;
        acc[1 + cell] += s;
    }
}

inline bool sizes_ok(int K, int B, int L) {
    return K > 0 && K <= GGPM_LIKELIHOOD_MAX_K && B > 0 && B <= GGPM_LATENT_DECOMP_MAX_B && L > 0 && L <= GGPM_FREE_BITS_MAX_L &&
           (size_t)K * (size_t)B * (size_t)L < ((size_t)1 << 31);
}

}  // namespace

extern "C" int ggpm_latent_decomp(const float* z, const float* mean, const float* pre_var, int K, int B, int L, double log_nb,
                                  float* comps, float* dwkl_dim, double* lse_joint, double* lse_dim, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!z || !mean || !pre_var || !comps || !sizes_ok(K, B, L) || !std::isfinite(log_nb)) return GGPM_ERR_ARG;
    latent_decomp_k<<<K * B, 64 * DECOMP_WAVES, 0, (hipStream_t)stream>>>(z, mean, pre_var, B, L, log_nb, comps, dwkl_dim, lse_joint,
                                                                         lse_dim);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_latent_decomp_backward(const float* z, const float* mean, const float* pre_var, const double* lse_joint,
                                           const double* lse_dim, const float* coef, int K, int B, int L, float* dz, float* dmean,
                                           float* dpre_var, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!z || !mean || !pre_var || !lse_joint || !lse_dim || !coef || !dz || !dmean || !dpre_var || !sizes_ok(K, B, L))
        return GGPM_ERR_ARG;
    latent_decomp_bwd_row_k<<<K * B, 64 * DECOMP_WAVES, 0, (hipStream_t)stream>>>(z, mean, pre_var, lse_joint, lse_dim, coef, B, L, dz);
    GGPM_CHECK_LAUNCH();
    latent_decomp_bwd_col_k<<<dim3(B, (L + 63) / 64), 64 * DECOMP_WAVES, 0, (hipStream_t)stream>>>(z, mean, pre_var, lse_joint, lse_dim,
                                                                                                 coef, K, B, L, dmean, dpre_var);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_latent_decomp_accumulate(const float* comps, const float* dwkl_dim, int K, int B, int L, double* acc,
                                             ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!comps || !dwkl_dim || !acc || !sizes_ok(K, B, L)) return GGPM_ERR_ARG;
    latent_decomp_accumulate_k<<<3 + L, 64, 0, (hipStream_t)stream>>>(comps, dwkl_dim, K * B, L, acc);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}
