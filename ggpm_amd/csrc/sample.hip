// Seeded draws of the sampled decode and of the prior ("Sampled decoding and the prior"; include/ggpm_hip.h).
// Stateless and counter-based, as ggpm_dropout's masks are: every random word is a function of
// (seed_lo, seed_hi, site, sample id, step, slot) alone -- not of the row's position in the launch, of the other rows or of
// the batch size.  Plain stores, no atomics, no LDS: the three kernels are a few hundred lanes of work each.
#include "sample_stream.h"

namespace {
// draw[i] = m 2^-24 < p[i]: both sides are exact fp32 values, so p = 0 never draws 1 and p = 1 always does
__global__ void __launch_bounds__(256) sample_topo_k(const float* __restrict__ p, const int32_t* __restrict__ bidx,
                                                     const int32_t* __restrict__ ids, int n, unsigned int step,
                                                     unsigned int seed_lo, unsigned int seed_hi,
                                                     float* __restrict__ draw) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const unsigned int m = sample_m(seed_lo, seed_hi, GGPM_SITE_SAMPLE_TOPO, (unsigned int)ids[bidx[i]], step, 0u);
        draw[i] = ((float)m * TWO_M24 < p[i]) ? 1.f : 0.f;
    }
}

// One wave per row.  Lane q < k holds key_q = score_q - log(e_q), e_q = -log((m_q + 1) 2^-24) floored at 2^-24: an
// exponential race in the log domain.  Its rank is the number of keys ahead of it (greater, or equal at a lower index), so
// the ranks of a row are a permutation whatever the keys are.
__global__ void __launch_bounds__(64) sample_order_k(const int32_t* __restrict__ topk, const int32_t* __restrict__ bidx,
                                                     const int32_t* __restrict__ ids, int k, unsigned int step,
                                                     unsigned int seed_lo, unsigned int seed_hi,
                                                     int32_t* __restrict__ order) {
    const int r = blockIdx.x, q = threadIdx.x;
    float key = 0.f;
    if (q < k) {
        const unsigned int m = sample_m(seed_lo, seed_hi, GGPM_SITE_SAMPLE_BEAM, (unsigned int)ids[bidx[r]], step,
                                        (unsigned int)q);
        const float e = fmaxf(-logf((float)(m + 1u) * TWO_M24), TWO_M24);
        key = __int_as_float(topk[(size_t)r * 3 * k + q]) - logf(e);
    }
    int rank = 0;
    for (int j = 0; j < k; ++j) {
        const float kj = __shfl(key, j);
        rank += (kj > key || (kj == key && j < q)) ? 1 : 0;
    }
    if (q < k) order[(size_t)r * k + rank] = q;
}

__global__ void __launch_bounds__(256) sample_normal_k(float* __restrict__ out, int rows, int cols, int ld,
                                                       const int32_t* __restrict__ ids, unsigned int seed_lo,
                                                       unsigned int seed_hi) {
    const int total = rows * cols;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int r = i / cols, c = i - r * cols;
        out[(size_t)r * ld + c] = sample_gauss(seed_lo, seed_hi, GGPM_SITE_SAMPLE_PRIOR, (unsigned int)ids[r], (unsigned int)c);
    }
}

// eps[k, b, c] of the likelihood estimate: site LATENT, the molecule's id, counter k * L + c
__global__ void __launch_bounds__(256) sample_latent_normal_k(float* __restrict__ out, int K, int B, int L,
                                                              const int32_t* __restrict__ ids, unsigned int seed_lo,
                                                              unsigned int seed_hi) {
    const int total = K * B * L;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int c = i % L, kb = i / L;
        const int b = kb % B, k = kb / B;
        out[i] = sample_gauss(seed_lo, seed_hi, GGPM_SITE_SAMPLE_LATENT, (unsigned int)ids[b], (unsigned int)(k * L + c));
    }
}

inline unsigned int stride_grid(int n) {
    const int b = ggpm_ceil_div(n, 256);
    return (unsigned int)(b > 1024 ? 1024 : b);
}
}  // namespace

extern "C" int ggpm_sample_topo(const float* p, const int32_t* bidx, const int32_t* ids, int n, int step,
                                unsigned int seed_lo, unsigned int seed_hi, float* draw, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!p || !bidx || !ids || !draw || n <= 0 || step < 0) return GGPM_ERR_ARG;
    sample_topo_k<<<stride_grid(n), 256, 0, (hipStream_t)stream>>>(p, bidx, ids, n, (unsigned int)step, seed_lo, seed_hi,
                                                                  draw);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_sample_beam_order(const int32_t* topk, const int32_t* bidx, const int32_t* ids, int M, int k, int step,
                                      unsigned int seed_lo, unsigned int seed_hi, int32_t* order, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!topk || !bidx || !ids || !order || M <= 0 || k < 1 || k > GGPM_SAMPLE_MAX_K || step < 0) return GGPM_ERR_ARG;
    sample_order_k<<<M, 64, 0, (hipStream_t)stream>>>(topk, bidx, ids, k, (unsigned int)step, seed_lo, seed_hi, order);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_sample_normal(float* out, int rows, int cols, int ld, const int32_t* ids, unsigned int seed_lo,
                                  unsigned int seed_hi, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!out || !ids || rows <= 0 || cols <= 0 || ld < cols || (size_t)rows * (size_t)cols >= ((size_t)1 << 31))
        return GGPM_ERR_ARG;
    sample_normal_k<<<stride_grid(rows * cols), 256, 0, (hipStream_t)stream>>>(out, rows, cols, ld, ids, seed_lo, seed_hi);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_sample_latent_normal(float* out, int K, int B, int L, const int32_t* ids, unsigned int seed_lo,
                                         unsigned int seed_hi, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!out || !ids || K < 1 || K > GGPM_LIKELIHOOD_MAX_K || B <= 0 || L <= 0 ||
        (size_t)K * (size_t)L >= ((size_t)1 << 26) || (size_t)K * (size_t)B * (size_t)L >= ((size_t)1 << 31))
        return GGPM_ERR_ARG;
    sample_latent_normal_k<<<stride_grid(K * B * L), 256, 0, (hipStream_t)stream>>>(out, K, B, L, ids, seed_lo, seed_hi);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}
