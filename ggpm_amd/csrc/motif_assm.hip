// Attachment head of the tree-only decoder (MotifDecoder: enum_attach + get_assm_score + the padded cross entropy).
//
// Per prediction p (meta row: n candidates of k rows each, nth_child, molecule b, candidate offset, row offset):
//   a_r     = relu(W1 [e_r | onehot(nth)] + b1)            (matchNN; e_r = E_assm row r, [H])
//   v_c     = sum_{j<k} a_{c*k+j}                          (pair candidates: the sum of their two rows)
//   score_c = (Wa v_c + ba) . z_b = v_c . u_p + s0_p,      u_p = Wa^T z_b,  s0_p = ba . z_b
//   the C - n pad rows score s0_p (a zero row through W_assm); cross entropy with label 0 over all C rows;
//   correct_p = (score_0 == max over the C rows)            (get_accuracy_sym)
// Forward: one launch, one workgroup per prediction; the last workgroup to finish sums the per-prediction losses and
// hits in prediction order (an integer arrival counter, no float atomics).
// Backward: one launch, four roles by block index; every output element is owned by exactly one workgroup, which sums
// over rows / predictions in a fixed order: bitwise reproducible.
#include "common.h"

namespace {

constexpr int ASSM_THREADS = 256;
constexpr int ASSM_MAX_H = 1024;      // hidden width bound: 4 columns per thread
constexpr int ASSM_RCH = 4;           // rows per W1 pass in the forward
constexpr int ASSM_HS = 4;            // hidden units per workgroup in the weight-gradient roles
constexpr int META = 6;               // n, k, nth, b, cand_off, row_off

struct AssmFwd {
    const float* rows; int ld_rows;
    const int32_t* meta; int P, C, H, L;
    const float* W1; int ldw; const float* b1; const float* Wa; const float* ba; const float* z; int ldz;
    float* act; float* score; float* stat; float* out; int32_t* counter;
};

struct AssmBwd {
    const float* dloss; const float* rows; int ld_rows;
    const int32_t* meta; int P, C, H, L, B;
    const float* W1; int ldw; const float* Wa; const float* ba; const float* z; int ldz;
    const float* act; const float* score; const float* stat;
    float* drows; float* dW1; float* db1; float* dWa; float* dba; float* dz;
    int nb_w1, nb_wa;
    const float* coef; int coef_stride;         // per-molecule upstream gradient (ggpm_motif_assm_backward_weighted), else null
};

// fixed-order block sum (every thread gets the result)
__device__ float block_sum(float v, float* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = ASSM_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    float r = red[0];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(ASSM_THREADS) motif_assm_fwd_k(AssmFwd a) {
    __shared__ float u[ASSM_MAX_H];
    __shared__ float e[ASSM_RCH][ASSM_MAX_H + 4];
    __shared__ float red[ASSM_THREADS];
    __shared__ float s0s;
    const int p = blockIdx.x, t = threadIdx.x, H = a.H, L = a.L;
    const int32_t* m = a.meta + (size_t)p * META;
    const int n = m[0], k = m[1], nth = m[2], b = m[3], coff = m[4], roff = m[5];
    const float* zb = a.z + (size_t)b * a.ldz;
    for (int h = t; h < H; h += ASSM_THREADS) {
        float acc = 0.f;
        for (int l = 0; l < L; ++l) acc += a.Wa[(size_t)l * H + h] * zb[l];
        u[h] = acc;
    }
    if (t == 0) {
        float s = 0.f;
        for (int l = 0; l < L; ++l) s += a.ba[l] * zb[l];
        s0s = s;
    }
    __syncthreads();
    const float s0 = s0s;
    float v[ASSM_MAX_H / ASSM_THREADS];
    for (int c = 0; c < n; ++c) {
        for (int q = 0; q < ASSM_MAX_H / ASSM_THREADS; ++q) v[q] = 0.f;
        for (int j0 = 0; j0 < k; j0 += ASSM_RCH) {
            const int nr = min(ASSM_RCH, k - j0);
            const int r0 = roff + c * k + j0;
            for (int j = 0; j < nr; ++j)
                for (int i = t; i < H; i += ASSM_THREADS) e[j][i] = a.rows[(size_t)(r0 + j) * a.ld_rows + i];
            __syncthreads();
            for (int q = 0, h = t; h < H; ++q, h += ASSM_THREADS) {
                const float* w = a.W1 + (size_t)h * a.ldw;
                const float base = a.b1[h] + w[H + nth];
                float acc[ASSM_RCH];
                for (int j = 0; j < ASSM_RCH; ++j) acc[j] = base;
                for (int i = 0; i < H; ++i) {
                    const float wi = w[i];
                    for (int j = 0; j < ASSM_RCH; ++j) acc[j] += wi * e[j][i];
                }
                for (int j = 0; j < nr; ++j) {
                    const float y = fmaxf(acc[j], 0.f);
                    a.act[(size_t)(r0 + j) * H + h] = y;
                    v[q] += y;
                }
            }
            __syncthreads();
        }
        float d = 0.f;
        for (int q = 0, h = t; h < H; ++q, h += ASSM_THREADS) d += v[q] * u[h];
        d = block_sum(d, red);
        if (t == 0) {
            const float s = d + s0;
            a.score[coff + c] = s;
        }
    }
    __syncthreads();
    if (t == 0) {
        const int C = a.C;
        float mx = (n < C) ? s0 : -INFINITY;
        for (int c = 0; c < n; ++c) mx = fmaxf(mx, a.score[coff + c]);
        float se = n < C ? (float)(C - n) * expf(s0 - mx) : 0.f;      // (no pad row: no pad term, not 0 * inf)
        for (int c = 0; c < n; ++c) se += expf(a.score[coff + c] - mx);
        const float lse = mx + logf(se);
        const float s_0 = n > 0 ? a.score[coff] : s0;
        float* st = a.stat + (size_t)p * 4;
        st[0] = lse;
        st[1] = s0;
        st[2] = lse - s_0;
        st[3] = (s_0 == mx) ? 1.f : 0.f;
        __threadfence();
        const int done = atomicAdd(a.counter, 1);
        if (done == a.P - 1) {                     // the last workgroup: sums in prediction order
            __threadfence();
            float ls = 0.f, hit = 0.f;
            for (int q = 0; q < a.P; ++q) {
                const volatile float* sq = a.stat + (size_t)q * 4;
                ls += sq[2];
                hit += sq[3];
            }
            a.out[0] = ls;
            a.out[1] = hit / (float)a.P;
            *a.counter = 0;
        }
    }
}

// d(score_c) of candidate c (< n).  d(s0) of a prediction is sum_c softmax_c - 1 = 0: all C rows carry s0 and the cross
// entropy does not change under a shift of every score.  Evaluated in fp32 that sum is one rounding of lse away from 1
// (about ulp(lse) / 2, 1e-6 at lse = 16), with a sign of its own per prediction; summed over 700 predictions into dba that is
// 2e-5.  So dba is written as the zero it is, and dz gets no ba term.
// the upstream gradient of a prediction of molecule b: dloss[0] (1 when absent), times the molecule's coefficient when given
__device__ __forceinline__ float base_g(const AssmBwd& a) { return a.dloss ? a.dloss[0] : 1.f; }
__device__ __forceinline__ float pred_g(const AssmBwd& a, float g, int b) {
    if (!a.coef) return g;
    return (b >= 0 && b < a.B) ? g * a.coef[(size_t)b * a.coef_stride] : 0.f;
}

__device__ __forceinline__ float dscore(const AssmBwd& a, float g, const float* st, int coff, int c) {
    return g * (expf(a.score[coff + c] - st[0]) - (c == 0 ? 1.f : 0.f));
}

__device__ void bwd_w1(const AssmBwd& a, int blk) {
    // dW1[h, :] / db1[h] for the ASSM_HS hidden units of this workgroup, summed over every row of every prediction
    __shared__ float us[ASSM_HS];
    const int t = threadIdx.x, H = a.H, L = a.L, W = H + 20;
    const int h0 = blk * ASSM_HS;
    const float g = base_g(a);
    float acc[ASSM_HS][4];
    float accb[ASSM_HS];
    for (int s = 0; s < ASSM_HS; ++s) {
        accb[s] = 0.f;
        for (int q = 0; q < 4; ++q) acc[s][q] = 0.f;
    }
    for (int p = 0; p < a.P; ++p) {
        const int32_t* m = a.meta + (size_t)p * META;
        const int n = m[0], k = m[1], nth = m[2], b = m[3], coff = m[4], roff = m[5];
        const float* st = a.stat + (size_t)p * 4;
        __syncthreads();
        if (t < ASSM_HS && h0 + t < H) {
            const float* zb = a.z + (size_t)b * a.ldz;
            float u = 0.f;
            for (int l = 0; l < L; ++l) u += a.Wa[(size_t)l * H + h0 + t] * zb[l];
            us[t] = u;
        }
        __syncthreads();
        for (int c = 0; c < n; ++c) {
            const float dsc = dscore(a, pred_g(a, g, b), st, coff, c);
            for (int j = 0; j < k; ++j) {
                const int r = roff + c * k + j;
                float d[ASSM_HS];
                for (int s = 0; s < ASSM_HS; ++s)
                    d[s] = (h0 + s < H && a.act[(size_t)r * H + h0 + s] > 0.f) ? dsc * us[s] : 0.f;
                const float* er = a.rows + (size_t)r * a.ld_rows;
                for (int q = 0, i = t; i < W; ++q, i += ASSM_THREADS) {
                    const float x = i < H ? er[i] : (i - H == nth ? 1.f : 0.f);
                    for (int s = 0; s < ASSM_HS; ++s) acc[s][q] += d[s] * x;
                }
                for (int s = 0; s < ASSM_HS; ++s) accb[s] += d[s];
            }
        }
    }
    for (int s = 0; s < ASSM_HS; ++s) {
        if (h0 + s >= H) break;
        for (int q = 0, i = t; i < W; ++q, i += ASSM_THREADS) a.dW1[(size_t)(h0 + s) * W + i] = acc[s][q];
        if (t == 0) a.db1[h0 + s] = accb[s];
    }
}

__device__ void bwd_rows(const AssmBwd& a, int p) {
    // d(E_assm row) = W1[:, :H]^T dpre_r for every row of prediction p
    __shared__ float us[ASSM_MAX_H];
    __shared__ float dp[ASSM_MAX_H];
    const int t = threadIdx.x, H = a.H, L = a.L;
    const int32_t* m = a.meta + (size_t)p * META;
    const int n = m[0], k = m[1], b = m[3], coff = m[4], roff = m[5];
    const float* st = a.stat + (size_t)p * 4;
    const float g = pred_g(a, base_g(a), b);
    const float* zb = a.z + (size_t)b * a.ldz;
    for (int h = t; h < H; h += ASSM_THREADS) {
        float u = 0.f;
        for (int l = 0; l < L; ++l) u += a.Wa[(size_t)l * H + h] * zb[l];
        us[h] = u;
    }
    for (int c = 0; c < n; ++c) {
        const float dsc = dscore(a, g, st, coff, c);
        for (int j = 0; j < k; ++j) {
            const int r = roff + c * k + j;
            __syncthreads();
            for (int h = t; h < H; h += ASSM_THREADS) dp[h] = a.act[(size_t)r * H + h] > 0.f ? dsc * us[h] : 0.f;
            __syncthreads();
            for (int i = t; i < H; i += ASSM_THREADS) {
                float acc = 0.f;
                for (int h = 0; h < H; ++h) acc += a.W1[(size_t)h * a.ldw + i] * dp[h];
                a.drows[(size_t)r * a.ld_rows + i] = acc;
            }
        }
    }
}

// du_p[h] = sum_c dscore_c v_c[h]
__device__ __forceinline__ float du_of(const AssmBwd& a, float g, const int32_t* m, const float* st, int h) {
    const int n = m[0], k = m[1], coff = m[4], roff = m[5];
    float du = 0.f;
    for (int c = 0; c < n; ++c) {
        float v = 0.f;
        for (int j = 0; j < k; ++j) v += a.act[(size_t)(roff + c * k + j) * a.H + h];
        du += dscore(a, g, st, coff, c) * v;
    }
    return du;
}

__device__ void bwd_wa(const AssmBwd& a, int blk) {
    // dWa[:, h] for ASSM_HS hidden units, summed over the predictions in order (and, in workgroup 0, dba = 0)
    const int t = threadIdx.x, H = a.H, L = a.L;
    const int h0 = blk * ASSM_HS;
    const float g = base_g(a);
    for (int l = t; l < L; l += ASSM_THREADS) {
        float acc[ASSM_HS];
        for (int s = 0; s < ASSM_HS; ++s) acc[s] = 0.f;
        for (int p = 0; p < a.P; ++p) {
            const int32_t* m = a.meta + (size_t)p * META;
            const float* st = a.stat + (size_t)p * 4;
            const float zl = a.z[(size_t)m[3] * a.ldz + l];
            for (int s = 0; s < ASSM_HS; ++s)
                if (h0 + s < H) acc[s] += du_of(a, pred_g(a, g, m[3]), m, st, h0 + s) * zl;
        }
        for (int s = 0; s < ASSM_HS; ++s)
            if (h0 + s < H) a.dWa[(size_t)l * H + h0 + s] = acc[s];
        if (blk == 0) a.dba[l] = 0.f;
    }
}

__device__ void bwd_z(const AssmBwd& a, int b) {
    // dz[b] = sum over the predictions of molecule b (in order) of Wa du_p  (ds0_p = 0: no ba term)
    __shared__ float du[ASSM_MAX_H];
    const int t = threadIdx.x, H = a.H, L = a.L;
    const float g = pred_g(a, base_g(a), b);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < a.P; ++p) {
        const int32_t* m = a.meta + (size_t)p * META;
        if (m[3] != b) continue;
        const float* st = a.stat + (size_t)p * 4;
        __syncthreads();
        for (int h = t; h < H; h += ASSM_THREADS) du[h] = du_of(a, g, m, st, h);
        __syncthreads();
        for (int q = 0, l = t; l < L && q < 4; ++q, l += ASSM_THREADS) {
            float s = 0.f;
            for (int h = 0; h < H; ++h) s += a.Wa[(size_t)l * H + h] * du[h];
            acc[q] += s;
        }
    }
    for (int q = 0, l = t; l < L && q < 4; ++q, l += ASSM_THREADS) a.dz[(size_t)b * a.ldz + l] = acc[q];
}

__global__ void __launch_bounds__(ASSM_THREADS) motif_assm_bwd_k(AssmBwd a) {
    int blk = blockIdx.x;
    if (blk < a.nb_w1) { bwd_w1(a, blk); return; }
    blk -= a.nb_w1;
    if (blk < a.P) { bwd_rows(a, blk); return; }
    blk -= a.P;
    if (blk < a.nb_wa) { bwd_wa(a, blk); return; }
    blk -= a.nb_wa;
    bwd_z(a, blk);
}

bool dims_ok(int P, int C, int H, int L, int ldw) {
    return P > 0 && C > 0 && H > 0 && H <= ASSM_MAX_H && L > 0 && L <= 4 * ASSM_THREADS && ldw >= H + 20 && H + 20 <= 4 * ASSM_THREADS;
}

}  // namespace

extern "C" int ggpm_motif_assm_forward(const float* rows, int ld_rows, const int32_t* meta, int P, int C, int H, int L,
                                       const float* W1, int ldw, const float* b1, const float* Wa, const float* ba,
                                       const float* z, int ldz, float* act, float* score, float* stat, float* out,
                                       int32_t* counter, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!dims_ok(P, C, H, L, ldw) || ld_rows < H || ldz < L || !rows || !meta || !W1 || !b1 || !Wa || !ba || !z || !act ||
        !score || !stat || !out || !counter)
        return GGPM_ERR_ARG;
    AssmFwd a{rows, ld_rows, meta, P, C, H, L, W1, ldw, b1, Wa, ba, z, ldz, act, score, stat, out, counter};
    hipLaunchKernelGGL(motif_assm_fwd_k, dim3(P), dim3(ASSM_THREADS), 0, (hipStream_t)stream, a);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_motif_assm_backward(const float* dloss, const float* rows, int ld_rows, const int32_t* meta, int P, int C,
                                        int H, int L, int B, const float* W1, int ldw, const float* Wa, const float* ba,
                                        const float* z, int ldz, const float* act, const float* score, const float* stat,
                                        float* drows, float* dW1, float* db1, float* dWa, float* dba, float* dz,
                                        ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!dims_ok(P, C, H, L, ldw) || B <= 0 || ld_rows < H || ldz < L || !dloss || !rows || !meta || !W1 || !Wa || !ba ||
        !z || !act || !score || !stat || !drows || !dW1 || !db1 || !dWa || !dba || !dz)
        return GGPM_ERR_ARG;
    const int nb = ggpm_ceil_div(H, ASSM_HS);
    AssmBwd a{dloss, rows, ld_rows, meta, P, C, H, L, B, W1, ldw, Wa, ba, z, ldz, act, score, stat,
              drows, dW1, db1, dWa, dba, dz, nb, nb, nullptr, 0};
    hipLaunchKernelGGL(motif_assm_bwd_k, dim3(2 * nb + P + B), dim3(ASSM_THREADS), 0, (hipStream_t)stream, a);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

// ggpm_motif_assm_backward with a per-molecule upstream gradient: a prediction of molecule b = meta[p][3] is weighted by
// dloss[0] * coef[b * coef_stride] (dloss nullable: 1).  Same device code; coef = null is not accepted here.
extern "C" int ggpm_motif_assm_backward_weighted(const float* dloss, const float* coef, int coef_stride, const float* rows,
                                                 int ld_rows, const int32_t* meta, int P, int C, int H, int L, int B,
                                                 const float* W1, int ldw, const float* Wa, const float* ba, const float* z,
                                                 int ldz, const float* act, const float* score, const float* stat,
                                                 float* drows, float* dW1, float* db1, float* dWa, float* dba, float* dz,
                                                 ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!dims_ok(P, C, H, L, ldw) || B <= 0 || ld_rows < H || ldz < L || !coef || coef_stride < 1 || !rows || !meta || !W1 ||
        !Wa || !ba || !z || !act || !score || !stat || !drows || !dW1 || !db1 || !dWa || !dba || !dz)
        return GGPM_ERR_ARG;
    const int nb = ggpm_ceil_div(H, ASSM_HS);
    AssmBwd a{dloss, rows, ld_rows, meta, P, C, H, L, B, W1, ldw, Wa, ba, z, ldz, act, score, stat,
              drows, dW1, db1, dWa, dba, dz, nb, nb, coef, coef_stride};
    hipLaunchKernelGGL(motif_assm_bwd_k, dim3(2 * nb + P + B), dim3(ASSM_THREADS), 0, (hipStream_t)stream, a);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}
