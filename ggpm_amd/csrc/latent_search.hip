// The guided latent search (include/ggpm_hip.h):
//   ggpm_latent_search_guided : R = K B trajectories of gradient descent with heavy-ball momentum on
//                                 J(v) = prop(v) + anchor_weight anchor(v) + prior_weight prior(v),
//                               one launch for every row and every step, one workgroup per row
//   ggpm_latent_search_select : per molecule the start with the smallest J, and its row of every output
// The heads are walked as prop_search_k walks them (head_walk.h: the homo head on lanes 0..127, the lumo head on lanes
// 128..255, weights in LDS when they fit); the row's latent, momentum, mu and exp(-lv) stay in LDS for the whole trajectory.
//
// Floating point.  Heads, anchor gradient, standard-normal gradient and the update: fp32, contraction off, explicit fma in the
// dot products.  The mixture term follows csrc/latent_prior.hip: comp[c], the logsumexp, gamma_c and the gradient's sum over c
// are fp64 from the fp32 inputs in a fixed order (lanes stride, then the shuffle tree of wave_f64.h), rounded once where the
// gradient joins the fp32 update.  The three reported terms are summed in fp64 from the fp32 latent and rounded once; J is
// formed from the rounded terms in fp32.  No atomics: two runs give the same bits.
#include "head_walk.h"
#include "wave_f64.h"

#pragma clang fp contract(off)

namespace {

constexpr int GUIDED_MAX_R = 1 << 20;

struct GuidedArgs {
    HeadWalk w;
    int B, R, ld, half, steps, C;
    const float* z0;
    const float* mu;
    const float* lv;
    const float* t[2];
    const float* logits;                     // null: the standard normal
    const float* means;
    const float* log_vars;
    float lr, momentum, delta, wt[2], anchor_weight, prior_weight;
    int xoff;                                // LDS (floats, even): [mom L] [mu L] [iv L] [gp L] then fp64 [comp C] [lp]
    float* z_out;
    float* pred;
    float* terms;
    float* J;
    int32_t* steps_taken;
};

// logsumexp_c a[c] by the calling wave, as csrc/latent_prior.hip forms it
__device__ __noinline__ double guided_logits_lse(const float* __restrict__ a, int C, int lane) {
    Lse t;
    t.m = -INFINITY;
    t.s = 0.0;
    for (int c = lane; c < C; c += 64) t = lse_push(t, (double)a[c]);
    return lse_value(wave_lse(t));
}

// column j of the row's latent: the two halves are the inputs of the two heads' first Linear
__device__ __forceinline__ float latent_at(const GuidedArgs& a, const float* lds, int j) {
    return j < a.half ? lds[a.w.aoff[0][0] + j] : lds[a.w.aoff[1][0] + (j - a.half)];
}

// comp[0:C] and lp = logsumexp_c comp[c] of the resident latent (all four waves; ends on a barrier).  Wave w takes the
// components w, w + 4, ... with its lanes striding j; wave 0 folds them.
__device__ __forceinline__ void mixture_comp(const GuidedArgs& a, const float* lds, double* comp, double* lp, double la) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, L = 2 * a.half;
    for (int c = wave; c < a.C; c += SEARCH_THREADS / 64) {
        const size_t o = (size_t)c * L;
        double acc = 0.0;
        for (int j = lane; j < L; j += 64) {
            const double d = (double)latent_at(a, lds, j) - (double)a.means[o + j], sv = (double)a.log_vars[o + j];
            acc += LOG_2PI + sv + d * d * exp(-sv);
        }
        acc = wave_sum_f64(acc);
        if (lane == 0) comp[c] = ((double)a.logits[c] - la) - 0.5 * acc;
    }
    __syncthreads();
    if (wave == 0) {
        Lse t;
        t.m = -INFINITY;
        t.s = 0.0;
        for (int c = lane; c < a.C; c += 64) t = lse_push(t, comp[c]);
        const double v = lse_value(wave_lse(t));
        if (lane == 0) *lp = v;
    }
    __syncthreads();
}

// gp[j] = (float) sum_c gamma_c (v_j - m_cj) exp(-s_cj), the gradient of -log p(v) (all four waves; ends on a barrier).
// comp[] is overwritten by gamma.  Wave w takes the columns w, w + 4, ... with its lanes striding c.
__device__ __forceinline__ void mixture_grad(const GuidedArgs& a, const float* lds, double* comp, double* lp, float* gp,
                                             double la) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, L = 2 * a.half;
    mixture_comp(a, lds, comp, lp, la);
    const double lpv = *lp;
    for (int c = threadIdx.x; c < a.C; c += SEARCH_THREADS) comp[c] = exp(comp[c] - lpv);
    __syncthreads();
    for (int j = wave; j < L; j += SEARCH_THREADS / 64) {
        const double zv = (double)latent_at(a, lds, j);
        double acc = 0.0;
        for (int c = lane; c < a.C; c += 64) {
            const size_t o = (size_t)c * L + j;
            acc += comp[c] * ((zv - (double)a.means[o]) * exp(-(double)a.log_vars[o]));
        }
        acc = wave_sum_f64(acc);
        if (lane == 0) gp[j] = (float)acc;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(SEARCH_THREADS) latent_search_guided_k(GuidedArgs a) {
    extern __shared__ double lds_f64[];                          // 8-byte aligned: the fp64 tail needs it
    float* lds = reinterpret_cast<float*>(lds_f64);
    const int r = blockIdx.x, b = r % a.B;
    const int tid = threadIdx.x, lt = tid & 127, lane = tid & 63;
    const int h = __builtin_amdgcn_readfirstlane(tid >> 7);     // wave-uniform: the halves are two whole waves each
    const int maxn = max(a.w.head[0].n, a.w.head[1].n);
    const int half = a.half, L = 2 * half;
    float* Wp[PROP_MAX_LINEAR];
    float* bp[PROP_MAX_LINEAR];
    head_walk_weights(a.w, lds, h, lt, Wp, bp);
    float* v = lds + a.w.aoff[h][0];
    float* mom = lds + a.xoff + h * half;                        // this head's half of each resident [L] vector (column j at j)
    float* mu = mom + L;
    float* iv = mu + L;
    float* gp = lds + a.xoff + 3 * L;                            // [L], whole row
    double* comp = reinterpret_cast<double*>(lds + a.xoff + 4 * L);
    double* lp = comp + a.C;
    const bool mixture = a.logits != nullptr;
    {
        const float* zr = a.z0 + (size_t)r * a.ld + h * half;
        const float* mr = a.mu + (size_t)b * L + h * half;
        const float* lr_ = a.lv + (size_t)b * L + h * half;
        for (int k = lt; k < half; k += 128) {
            v[k] = zr[k];
            mom[k] = 0.f;
            mu[k] = mr[k];
            iv[k] = expf(-lr_[k]);
        }
    }
    const double la = mixture ? guided_logits_lse(a.logits, a.C, lane) : 0.0;
    __syncthreads();

    const float th = a.t[0][b], tl = a.t[1][b], tx = h == 0 ? th : tl;
    const float wx = h == 0 ? a.wt[0] : a.wt[1];
    const float aw = a.anchor_weight, pw = a.prior_weight;
    int n = 0;
    for (int it = 0; it < a.steps; ++it) {
        head_walk_forward(a.w, lds, Wp, bp, h, lt, maxn);
        const float oh = lds[a.w.ooff], ol = lds[a.w.ooff + 1];
        const float dh = oh - th, dl = ol - tl;
        const float prop = a.wt[0] * (dh * dh) + a.wt[1] * (dl * dl);
        if (a.delta >= 0.f && prop <= a.delta) break;            // the same value in every lane: a uniform exit
        const float o = h == 0 ? oh : ol;
        const int cur = head_walk_backward(a.w, lds, Wp, h, lt, maxn, (2.f * wx) * (o - tx));
        if (mixture && pw != 0.f) mixture_grad(a, lds, comp, lp, gp, la);
        const float* gin = lds + a.w.goff[h][cur];
        const float* gph = gp + h * half;
        for (int k = lt; k < half; k += 128) {
            float g = gin[k];
            if (aw != 0.f) g = g + aw * ((v[k] - mu[k]) * iv[k]);
            if (pw != 0.f) g = g + pw * (mixture ? gph[k] : v[k]);
            const float m = a.momentum * mom[k] + g;
            mom[k] = m;
            v[k] = v[k] - a.lr * m;
        }
        ++n;
        __syncthreads();
    }
    // the heads and the three terms on the final latent
    head_walk_forward(a.w, lds, Wp, bp, h, lt, maxn);
    if (mixture) mixture_comp(a, lds, comp, lp, la);
    float* zo = a.z_out + (size_t)r * a.ld;
    for (int k = lt; k < half; k += 128) zo[h * half + k] = v[k];
    if (tid < 64) {                                              // wave 0: lanes stride the columns, fixed butterfly
        double acc_a = 0.0, acc_n = 0.0;
        const float* ma = lds + a.xoff + L;
        const float* ia = ma + L;
        for (int j = lane; j < L; j += 64) {
            const double vj = (double)latent_at(a, lds, j);
            const double d = vj - (double)ma[j];
            acc_a += d * d * (double)ia[j];
            acc_n += LOG_2PI + vj * vj;
        }
        acc_a = wave_sum_f64(acc_a);
        acc_n = wave_sum_f64(acc_n);
        if (tid == 0) {
            for (int k = L; k < a.ld; ++k) zo[k] = a.z0[(size_t)r * a.ld + k];
            const float oh = lds[a.w.ooff], ol = lds[a.w.ooff + 1];
            const float dh = oh - th, dl = ol - tl;
            const float prop = a.wt[0] * (dh * dh) + a.wt[1] * (dl * dl);
            const float anchor = (float)(0.5 * acc_a);
            const float prior = mixture ? (float)(-*lp) : (float)(0.5 * acc_n);
            a.pred[r] = oh;
            a.pred[(size_t)a.R + r] = ol;
            a.terms[(size_t)r * 3 + 0] = prop;
            a.terms[(size_t)r * 3 + 1] = anchor;
            a.terms[(size_t)r * 3 + 2] = prior;
            a.J[r] = (prop + aw * anchor) + pw * prior;
            a.steps_taken[r] = n;
        }
    }
}

// thread = molecule b: the smallest J over its K rows b, B + b, ..., the lowest k on a tie; a NaN ranks behind every number
__global__ void __launch_bounds__(256) latent_search_select_k(const float* __restrict__ J, const float* __restrict__ z,
                                                              const float* __restrict__ pred, const float* __restrict__ terms,
                                                              int K, int B, int ld, int32_t* __restrict__ best_k,
                                                              float* __restrict__ z_best, float* __restrict__ pred_best,
                                                              float* __restrict__ terms_best) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int best = 0;
    float jb = J[b];
    for (int k = 1; k < K; ++k) {
        const float j = J[(size_t)k * B + b];
        if (j == j && (jb != jb || j < jb)) {
            best = k;
            jb = j;
        }
    }
    const size_t R = (size_t)K * B, r = (size_t)best * B + b;
    best_k[b] = best;
    for (int c = 0; c < ld; ++c) z_best[(size_t)b * ld + c] = z[r * ld + c];
    pred_best[b] = pred[r];
    pred_best[(size_t)B + b] = pred[R + r];
    for (int c = 0; c < 3; ++c) terms_best[(size_t)b * 3 + c] = terms[r * 3 + c];
}

}  // namespace

extern "C" int ggpm_latent_search_guided(int K, int B, const float* z0, int ld, int half, const float* mu, const float* lv,
                                         const ggpm_prop_head* homo, const ggpm_prop_head* lumo, const float* t_homo,
                                         const float* t_lumo, const float* logits, const float* means, const float* log_vars,
                                         int C, float lr, float momentum, int steps, float delta, float w_h, float w_l,
                                         float anchor_weight, float prior_weight, float* z_out, float* pred, float* terms,
                                         float* J, int32_t* steps_taken, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    GuidedArgs a{};
    int e;
    if ((e = head_from(homo, half, a.w.head[0])) != GGPM_OK || (e = head_from(lumo, half, a.w.head[1])) != GGPM_OK) return e;
    const int n_mix = (logits ? 1 : 0) + (means ? 1 : 0) + (log_vars ? 1 : 0);
    if (!z0 || !mu || !lv || !t_homo || !t_lumo || !z_out || !pred || !terms || !J || !steps_taken || K < 1 || B < 1 ||
        ld < 2 * half || steps < 0 || (n_mix != 0 && n_mix != 3) || (n_mix == 3 && (C < 1 || C > GGPM_MIXTURE_MAX_C)))
        return GGPM_ERR_ARG;
    if ((size_t)K * (size_t)B > (size_t)GUIDED_MAX_R) return GGPM_ERR_UNSUPPORTED;
    a.C = n_mix ? C : 0;
    // beside the heads' plan: four resident [L] vectors (one float of slack to start the fp64 tail on 8 bytes), then comp[C], lp
    const size_t extra = 1 + 4 * (size_t)(2 * half) + 2 * ((size_t)a.C + 1);
    int xoff = 0;
    const size_t lds_bytes = head_walk_plan(a.w, extra, &xoff);
    if (lds_bytes > SEARCH_LDS_MAX) return GGPM_ERR_UNSUPPORTED;
    a.xoff = (xoff + 1) & ~1;
    a.B = B; a.R = K * B; a.ld = ld; a.half = half; a.steps = steps;
    a.z0 = z0; a.mu = mu; a.lv = lv; a.t[0] = t_homo; a.t[1] = t_lumo;
    a.logits = logits; a.means = means; a.log_vars = log_vars;
    a.lr = lr; a.momentum = momentum; a.delta = delta; a.wt[0] = w_h; a.wt[1] = w_l;
    a.anchor_weight = anchor_weight; a.prior_weight = prior_weight;
    a.z_out = z_out; a.pred = pred; a.terms = terms; a.J = J; a.steps_taken = steps_taken;
    if (lds_bytes > 64 * 1024) ggpm_set_lds(latent_search_guided_k, lds_bytes);
    latent_search_guided_k<<<a.R, SEARCH_THREADS, lds_bytes, (hipStream_t)stream>>>(a);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_latent_search_select(const float* J, const float* z, const float* pred, const float* terms, int K, int B,
                                         int ld, int32_t* best_k, float* z_best, float* pred_best, float* terms_best,
                                         ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!J || !z || !pred || !terms || !best_k || !z_best || !pred_best || !terms_best || K < 1 || B < 1 || ld < 1 ||
        (size_t)K * (size_t)B > (size_t)GUIDED_MAX_R)
        return GGPM_ERR_ARG;
    latent_search_select_k<<<ggpm_ceil_div(B, 256), 256, 0, (hipStream_t)stream>>>(J, z, pred, terms, K, B, ld, best_k, z_best,
                                                                                   pred_best, terms_best);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}
