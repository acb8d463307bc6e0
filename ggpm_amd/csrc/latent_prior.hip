// The learnable mixture-of-Gaussians prior ("A learned prior"; include/ggpm_hip.h):
//   ggpm_mixture_logp          : per row of z the log-density under the mixture, its difference to the standard normal's, the
//                                responsibilities, and the two fp64 stashes the backward reads
//   ggpm_mixture_logp_backward : the gradient by z (row pass) and by the means, log-variances and logits (column pass)
//   ggpm_sample_mixture        : seeded draws: a component per row from one uniform, then m + exp(s / 2) g with the normals
//                                of ggpm_sample_normal
// with comp[r, c] = log pi_c - 0.5 sum_j (log 2pi + s[c, j] + (z[r, j] - m[c, j])^2 exp(-s[c, j])), pi = softmax(a).
// As in csrc/latent_decomp.hip: one wave owns one output and its lanes stride the other index; per-lane fp64 partials go
// through a fixed shuffle tree; every log-density, logsumexp and softmax weight is fp64 (exp / log on double, the fp32 inputs
// widened exactly); every fp32 value is rounded once, where it is stored; no atomics.  A workgroup keeps one fp64 value per
// component in LDS, which is what GGPM_MIXTURE_MAX_C bounds.
#include "sample_stream.h"
#include "wave_f64.h"

namespace {

#define MIX_WAVES 4

// logsumexp_c a[c] by the calling wave (every lane returns it): lanes stride c, then the butterfly.  The forward and the
// column pass call THIS function, so pi_c = exp(a_c - lse) there is the very weight comp[r, c] holds.
__device__ __noinline__ double logits_lse(const float* __restrict__ a, int C, int lane) {
    Lse t;
    t.m = -INFINITY;
    t.s = 0.0;
    for (int c = lane; c < C; c += 64) t = lse_push(t, (double)a[c]);
    return lse_value(wave_lse(t));
}

// block = row r, MIX_WAVES waves.  Wave w takes the components c = w, w + W, ... (lanes stride j) and leaves comp[c] in LDS
// and in the stash; the last wave also forms the standard normal's log-density.  Then wave 0 folds comp[0:C] (lanes stride c,
// the pairs merged by the butterfly), and all waves write the responsibilities.
__global__ void __launch_bounds__(64 * MIX_WAVES) mixture_logp_k(const float* __restrict__ z, const float* __restrict__ a,
                                                                const float* __restrict__ m, const float* __restrict__ s, int C,
                                                                int L, float* __restrict__ logp, float* __restrict__ ratio,
                                                                float* __restrict__ resp, double* __restrict__ comp_stash,
                                                                double* __restrict__ logp_stash) {
    __shared__ double sh_comp[GGPM_MIXTURE_MAX_C];
    __shared__ double sh_logn, sh_logp;
    const int row = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* zr = z + (size_t)row * L;
    const double la = logits_lse(a, C, lane);
    for (int c = wave; c < C; c += MIX_WAVES) {
        const size_t o = (size_t)c * L;
        double acc = 0.0;
        for (int l = lane; l < L; l += 64) {
            const double d = (double)zr[l] - (double)m[o + l], sv = (double)s[o + l];
            acc += LOG_2PI + sv + d * d * exp(-sv);
        }
        acc = wave_sum_f64(acc);
        if (lane == 0) {
            const double v = ((double)a[c] - la) - 0.5 * acc;
            sh_comp[c] = v;
            if (comp_stash) comp_stash[(size_t)row * C + c] = v;
        }
    }
    if (wave == MIX_WAVES - 1) {
        double acc = 0.0;
        for (int l = lane; l < L; l += 64) acc += LOG_2PI + (double)zr[l] * (double)zr[l];
        acc = wave_sum_f64(acc);
        if (lane == 0) sh_logn = -0.5 * acc;
    }
    __syncthreads();
    if (wave == 0) {
        Lse t;
        t.m = -INFINITY;
        t.s = 0.0;
        for (int c = lane; c < C; c += 64) t = lse_push(t, sh_comp[c]);
        const double lp = lse_value(wave_lse(t));
        if (lane == 0) {
            sh_logp = lp;
            logp[row] = (float)lp;
            ratio[row] = (float)(lp - sh_logn);
            if (logp_stash) logp_stash[row] = lp;
        }
    }
    if (resp) {
        __syncthreads();
        const double lp = sh_logp;
        for (int c = threadIdx.x; c < C; c += 64 * MIX_WAVES) resp[(size_t)row * C + c] = (float)exp(sh_comp[c] - lp);
    }
}

// row pass: block = row r.  The threads leave gamma[c] = exp(comp[r, c] - logp[r]) in LDS, then wave w takes the columns
// j = w, w + W, ... with its lanes striding c.
__global__ void __launch_bounds__(64 * MIX_WAVES) mixture_bwd_row_k(const float* __restrict__ z, const float* __restrict__ m,
                                                                   const float* __restrict__ s,
                                                                   const double* __restrict__ comp_stash,
                                                                   const double* __restrict__ logp_stash,
                                                                   const float* __restrict__ g, int on_logp, int C, int L,
                                                                   float* __restrict__ dz) {
    __shared__ double gam[GGPM_MIXTURE_MAX_C];
    const int row = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* zr = z + (size_t)row * L;
    const double lp = logp_stash[row], gr = (double)g[row];
    for (int c = threadIdx.x; c < C; c += 64 * MIX_WAVES) gam[c] = exp(comp_stash[(size_t)row * C + c] - lp);
    __syncthreads();
    for (int l = wave; l < L; l += MIX_WAVES) {
        const double zv = (double)zr[l];
        double acc = 0.0;
        for (int c = lane; c < C; c += 64) {
            const size_t o = (size_t)c * L + l;
            acc += gam[c] * (((double)m[o] - zv) * exp(-(double)s[o]));
        }
        acc = wave_sum_f64(acc);
        if (lane == 0) dz[(size_t)row * L + l] = (float)(gr * (acc + (on_logp ? 0.0 : zv)));
    }
}

// column pass: block = (component c, tile of 64 columns); lane = column tile * 64 + lane.  Wave w takes the rows
// n = w, w + W, ... of the R in that order; the waves' partials are added in wave order by wave 0.  The blocks of the first
// tile also carry the logit's sum, which is the same in every lane.
__global__ void __launch_bounds__(64 * MIX_WAVES) mixture_bwd_col_k(const float* __restrict__ z, const float* __restrict__ a,
                                                                   const float* __restrict__ m, const float* __restrict__ s,
                                                                   const double* __restrict__ comp_stash,
                                                                   const double* __restrict__ logp_stash,
                                                                   const float* __restrict__ g, int R, int C, int L,
                                                                   float* __restrict__ dm, float* __restrict__ ds,
                                                                   float* __restrict__ da) {
    __shared__ double sh_m[MIX_WAVES][64], sh_v[MIX_WAVES][64], sh_a[MIX_WAVES];
    const int c = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int mine = blockIdx.y * 64 + lane;                    // may lie past L in the last tile
    const bool in = mine < L;
    const size_t o = (size_t)c * L + (in ? mine : 0);
    const double mv = (double)m[o], iv = exp(-(double)s[o]);
    const double pi = exp((double)a[c] - logits_lse(a, C, lane));
    double acc_m = 0.0, acc_v = 0.0, acc_a = 0.0;
    for (int n = wave; n < R; n += MIX_WAVES) {
        const double gr = (double)g[n];
        const double gamma = exp(comp_stash[(size_t)n * C + c] - logp_stash[n]);
        const double w = gr * gamma;
        acc_a += gr * (gamma - pi);
        if (in) {
            const double d = (double)z[(size_t)n * L + mine] - mv;
            acc_m += w * (d * iv);
            acc_v += w * (0.5 * (d * d * iv - 1.0));
        }
    }
    sh_m[wave][lane] = acc_m;
    sh_v[wave][lane] = acc_v;
    if (lane == 0) sh_a[wave] = acc_a;
    __syncthreads();
    if (wave == 0) {
        double tm = sh_m[0][lane], tv = sh_v[0][lane], ta = sh_a[0];
        for (int w = 1; w < MIX_WAVES; ++w) {
            tm += sh_m[w][lane];
            tv += sh_v[w][lane];
            ta += sh_a[w];
        }
        if (in) {
            dm[o] = (float)tm;
            ds[o] = (float)tv;
        }
        if (blockIdx.y == 0 && lane == 0) da[c] = (float)ta;
    }
}

// block = row r, one wave.  The lanes leave e[c] = exp(a_c - max a) in LDS; then every lane walks the same prefix sums in index
// order (LDS broadcast reads), so all of them hold the same component, and the lanes stride the columns.
__global__ void __launch_bounds__(64) sample_mixture_k(const float* __restrict__ a, const float* __restrict__ m,
                                                       const float* __restrict__ s, int C, float* __restrict__ out, int cols,
                                                       int ld, const int32_t* __restrict__ ids, unsigned int seed_lo,
                                                       unsigned int seed_hi, int32_t* __restrict__ comp) {
    __shared__ double e[GGPM_MIXTURE_MAX_C];
    const int r = blockIdx.x, lane = threadIdx.x;
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, a[c]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    for (int c = lane; c < C; c += 64) e[c] = exp((double)a[c] - (double)mx);
    __syncthreads();
    double total = 0.0;
    int last = 0;                                                // the last component with a non-zero weight
    for (int c = 0; c < C; ++c) {
        total += e[c];
        if (e[c] > 0.0) last = c;
    }
    const unsigned int id = (unsigned int)ids[r];
    const double t = (double)sample_m(seed_lo, seed_hi, GGPM_SITE_SAMPLE_PRIOR_COMP, id, 0u, 0u) * (double)TWO_M24 * total;
    int pick = last;
    double pre = 0.0;
    for (int c = 0; c < C; ++c) {
        pre += e[c];
        if (pre > t) {
            pick = c;
            break;
        }
    }
    if (comp && lane == 0) comp[r] = pick;
    const size_t o = (size_t)pick * cols;
    for (int j = lane; j < cols; j += 64)
        out[(size_t)r * ld + j] = fmaf(expf(0.5f * s[o + j]),
                                       sample_gauss(seed_lo, seed_hi, GGPM_SITE_SAMPLE_PRIOR, id, (unsigned int)j), m[o + j]);
}

inline bool sizes_ok(int R, int C, int L) {
    return R > 0 && C > 0 && C <= GGPM_MIXTURE_MAX_C && L > 0 && L <= GGPM_FREE_BITS_MAX_L &&
           (size_t)R * (size_t)L < ((size_t)1 << 31) && (size_t)R * (size_t)C < ((size_t)1 << 31);
}

}  // namespace

extern "C" int ggpm_mixture_logp(const float* z, const float* logits, const float* means, const float* log_vars, int R, int C,
                                 int L, float* logp, float* ratio, float* resp, double* comp_stash, double* logp_stash,
                                 ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!z || !logits || !means || !log_vars || !logp || !ratio || !sizes_ok(R, C, L)) return GGPM_ERR_ARG;
    mixture_logp_k<<<R, 64 * MIX_WAVES, 0, (hipStream_t)stream>>>(z, logits, means, log_vars, C, L, logp, ratio, resp, comp_stash,
                                                                  logp_stash);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_mixture_logp_backward(const float* z, const float* logits, const float* means, const float* log_vars,
                                          const double* comp_stash, const double* logp_stash, const float* g, int on_logp, int R,
                                          int C, int L, float* dz, float* dmeans, float* dlog_vars, float* dlogits,
                                          ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    const int n_param = (dmeans ? 1 : 0) + (dlog_vars ? 1 : 0) + (dlogits ? 1 : 0);
    if (!z || !logits || !means || !log_vars || !comp_stash || !logp_stash || !g || (on_logp != 0 && on_logp != 1) ||
        (n_param != 0 && n_param != 3) || (!dz && n_param == 0) || !sizes_ok(R, C, L))
        return GGPM_ERR_ARG;
    if (dz) {
        mixture_bwd_row_k<<<R, 64 * MIX_WAVES, 0, (hipStream_t)stream>>>(z, means, log_vars, comp_stash, logp_stash, g, on_logp, C, L,
                                                                         dz);
        GGPM_CHECK_LAUNCH();
    }
    if (n_param) {
        mixture_bwd_col_k<<<dim3(C, (L + 63) / 64), 64 * MIX_WAVES, 0, (hipStream_t)stream>>>(z, logits, means, log_vars, comp_stash,
                                                                                            logp_stash, g, R, C, L, dmeans,
                                                                                            dlog_vars, dlogits);
        GGPM_CHECK_LAUNCH();
    }
    return GGPM_OK;
}

extern "C" int ggpm_sample_mixture(const float* logits, const float* means, const float* log_vars, int C, float* out, int rows,
                                   int cols, int ld, const int32_t* ids, unsigned int seed_lo, unsigned int seed_hi,
                                   int32_t* comp, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!logits || !means || !log_vars || !out || !ids || ld < cols || !sizes_ok(rows, C, cols)) return GGPM_ERR_ARG;
    sample_mixture_k<<<rows, 64, 0, (hipStream_t)stream>>>(logits, means, log_vars, C, out, cols, ld, ids, seed_lo, seed_hi, comp);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}
