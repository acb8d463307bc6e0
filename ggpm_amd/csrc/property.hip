// HOMO / LUMO property heads of HierPropOptVAE and the latent property search -- reference ggpm/property_optimizer.py
// (PropertyOptimizer, PropertyRegressor), ggpm/property_vae.py:130-254 (their use in the fine-tune step) and
// ggpm/property_control.py:65-180 (fixed / soft / patience search).
//
//   heads forward / backward: one workgroup per head.  The heads are a few Linear layers over a few dozen rows; one
//     workgroup walks them layer by layer, so the batch-mean MSE and the batch reduction of every weight gradient
//     stay inside the workgroup and are summed in a fixed order: no atomics, bitwise reproducible.
//   latent search: one workgroup per molecule for the whole trajectory.  Both heads' weights are copied to LDS once
//     (when they fit), the molecule's two latent halves stay resident, and every step -- forward of both heads on one
//     row, backward with respect to the input, the mode's stopping rule, the signed update -- runs on the device.  The
//     loop is bounded by max_steps.
//
// Floating point: contraction is off in this file, so `a * b + c` is two roundings as in the reference's torch ops; the
// dot products use explicit fma.  The patience ratio |loss - prev| / prev is an IEEE division (prev == 0 gives inf or
// NaN, as torch does) and every comparison is an ordinary IEEE comparison (NaN compares false).
#include "head_walk.h"

#pragma clang fp contract(off)

namespace {

constexpr int PROP_MAX_B = 1024;            // heads forward / backward (one workgroup per head walks every row)
constexpr int PROP_MAX_SEARCH_B = 1 << 20;  // latent search (one workgroup per row)
constexpr int HEAD_THREADS = 512;
constexpr int HEAD_RB = 8;                  // rows per chunk of the heads forward (LDS ping-pong of HEAD_RB x 512 floats)

struct GradK {
    float* dW[PROP_MAX_LINEAR];
    float* db[PROP_MAX_LINEAR];
    int acc;
};

__device__ __forceinline__ unsigned int fmix32(unsigned int h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

// ggpm_dropout's keep test (gather.hip), element `idx` of the [rows, cols] mask of `site`
__device__ __forceinline__ bool keep_elem(unsigned int idx, unsigned int thresh, unsigned int seed_lo, unsigned int seed_hi,
                                          unsigned int site) {
    unsigned int h = fmix32(idx * 0x9E3779B1u + seed_lo);
    h = fmix32(h ^ (seed_hi + site * 0x7F4A7C15u));
    return (h >> 8) >= thresh;
}

// ------------------------------------------------------------------ heads forward
struct HeadsFwdArgs {
    HeadK head[2];
    int B, ld, half;
    const float* z;
    const float* t[2];
    float scale;                             // 1 / (1 - p)
    unsigned int thresh, seed_lo, seed_hi;   // thresh 0: no dropout
    float* pred;                             // [2][B]
    float* loss;                             // [2] (may be null)
    float* xs[2][PROP_MAX_LINEAR - 1];       // inputs of Linear 1 .. n-1 (post ReLU + dropout), [B, w[l]]
};

__global__ void __launch_bounds__(HEAD_THREADS) prop_heads_fwd_k(HeadsFwdArgs a) {
    const int h = blockIdx.x;
    const HeadK& H = a.head[h];
    __shared__ float buf[2][HEAD_RB * PROP_MAX_W];
    __shared__ float pl[PROP_MAX_B];
    const int tid = threadIdx.x;
    const int col0 = h * a.half;
    for (int r0 = 0; r0 < a.B; r0 += HEAD_RB) {
        const int rows = min(HEAD_RB, a.B - r0);
        const int w0 = H.w[0];
        for (int i = tid; i < rows * w0; i += HEAD_THREADS) {
            const int rr = i / w0, k = i - rr * w0;
            buf[0][i] = a.z[(size_t)(r0 + rr) * a.ld + col0 + k];
        }
        __syncthreads();
        int cur = 0;
        for (int l = 0; l < H.n; ++l) {
            const int win = H.w[l], wout = H.w[l + 1];
            const float* __restrict__ W = H.W[l];
            const float* __restrict__ bias = H.b[l];
            const float* X = buf[cur];
            float* Y = buf[cur ^ 1];
            const bool last = l == H.n - 1;
            for (int i = tid; i < rows * wout; i += HEAD_THREADS) {
                const int rr = i / wout, j = i - rr * wout;
                const float* wr = W + (size_t)j * win;
                const float* xr = X + rr * win;
                float s = 0.f;
                for (int k = 0; k < win; ++k) s = __builtin_fmaf(wr[k], xr[k], s);
                s = s + bias[j];
                if (last) {
                    a.pred[(size_t)h * a.B + r0 + rr] = s;
                    pl[r0 + rr] = s;
                } else {
                    float v = s > 0.f ? s : 0.f;
                    if (a.thresh != 0u) {
                        const unsigned int idx = (unsigned int)(r0 + rr) * (unsigned int)wout + (unsigned int)j;
                        const unsigned int site = (unsigned int)(GGPM_SITE_PROP_HOMO + h * (GGPM_SITE_PROP_LUMO - GGPM_SITE_PROP_HOMO) + l);
                        v = keep_elem(idx, a.thresh, a.seed_lo, a.seed_hi, site) ? v * a.scale : 0.f;
                    }
                    Y[i] = v;
                    a.xs[h][l][(size_t)(r0 + rr) * wout + j] = v;
                }
            }
            __syncthreads();
            cur ^= 1;
        }
    }
    // batch-mean MSE, fixed order: lane-strided partial sums, then a fixed butterfly
    if (a.loss && tid < 64) {
        const float* t = a.t[h];
        float s = 0.f;
        for (int r = tid; r < a.B; r += 64) {
            const float d = pl[r] - t[r];
            s = s + d * d;
        }
        s = wave_sum_fixed(s);
        if (tid == 0) a.loss[h] = s / (float)a.B;
    }
}

// ------------------------------------------------------------------ heads backward
struct HeadsBwdArgs {
    HeadK head[2];
    GradK g[2];
    int B, ld, half, ld_dz, acc_dz;
    const float* z;
    const float* t[2];
    const float* pred;
    const float* dloss;
    float norm;                               // (float)(2.0 / B): torch's mse_loss_backward factor
    float scale;                              // 1 / (1 - p) under dropout, else 1
    const float* xs[2][PROP_MAX_LINEAR - 1];
    float* D[2][2];                           // [B, max width] ping-pong per head
    float* dz;
};

__global__ void __launch_bounds__(HEAD_THREADS) prop_heads_bwd_k(HeadsBwdArgs a) {
    const int h = blockIdx.x;
    const HeadK& H = a.head[h];
    const GradK& G = a.g[h];
    const int tid = threadIdx.x, B = a.B, col0 = h * a.half;
    const float g0 = a.dloss[h];
    const float* t = a.t[h];
    float* Dc = a.D[h][0];
    for (int r = tid; r < B; r += HEAD_THREADS) Dc[r] = (a.norm * (a.pred[(size_t)h * B + r] - t[r])) * g0;
    __syncthreads();
    int cur = 0;
    for (int l = H.n - 1; l >= 0; --l) {
        const int win = H.w[l], wout = H.w[l + 1];
        const float* __restrict__ X = l > 0 ? a.xs[h][l - 1] : a.z + col0;
        const size_t ldx = l > 0 ? (size_t)win : (size_t)a.ld;
        const float* __restrict__ W = H.W[l];
        Dc = a.D[h][cur];
        if (G.dW[l]) {
            float* dW = G.dW[l];
            for (int i = tid; i < wout * win; i += HEAD_THREADS) {
                const int j = i / win, k = i - j * win;
                float s = 0.f;
                for (int r = 0; r < B; ++r) s = __builtin_fmaf(Dc[(size_t)r * wout + j], X[(size_t)r * ldx + k], s);
                dW[i] = G.acc ? dW[i] + s : s;
            }
        }
        if (G.db[l]) {
            float* db = G.db[l];
            for (int j = tid; j < wout; j += HEAD_THREADS) {
                float s = 0.f;
                for (int r = 0; r < B; ++r) s = s + Dc[(size_t)r * wout + j];
                db[j] = G.acc ? db[j] + s : s;
            }
        }
        if (l > 0 || a.dz) {
            float* Dn = a.D[h][cur ^ 1];
            for (int i = tid; i < B * win; i += HEAD_THREADS) {
                const int r = i / win, k = i - r * win;
                float s = 0.f;
                for (int j = 0; j < wout; ++j) s = __builtin_fmaf(Dc[(size_t)r * wout + j], W[(size_t)j * win + k], s);
                if (l > 0) {
                    // x = dropout(relu(pre)) > 0  <=>  kept and pre > 0 (relu'(0) = 0, as torch)
                    Dn[i] = X[(size_t)r * ldx + k] > 0.f ? s * a.scale : 0.f;
                } else {
                    float* p = a.dz + (size_t)r * a.ld_dz + col0 + k;
                    *p = a.acc_dz ? *p + s : s;
                }
            }
        }
        __syncthreads();
        cur ^= 1;
    }
}

// ------------------------------------------------------------------ latent search
struct SearchArgs {
    HeadWalk w;                              // the heads and their LDS plan (head_walk.h)
    int mode, B, ld, half, steps, max_steps;
    const float* z;
    const float* t[2];
    float lr, delta, patience, threshold, norm;
    float* z_out;
    float* pred;
    int32_t* steps_taken;
    int32_t* status;
};

__global__ void __launch_bounds__(SEARCH_THREADS) prop_search_k(SearchArgs a) {
    extern __shared__ float lds[];
    const int r = blockIdx.x;
    const int tid = threadIdx.x, lt = tid & 127;
    const int h = __builtin_amdgcn_readfirstlane(tid >> 7);     // wave-uniform: the halves are two whole waves each
    const int maxn = max(a.w.head[0].n, a.w.head[1].n);
    float* Wp[PROP_MAX_LINEAR];
    float* bp[PROP_MAX_LINEAR];
    head_walk_weights(a.w, lds, h, lt, Wp, bp);
    float* v = lds + a.w.aoff[h][0];
    const float* zr = a.z + (size_t)r * a.ld + h * a.half;
    for (int k = lt; k < a.half; k += 128) v[k] = zr[k];
    __syncthreads();

    const bool fixed = a.mode == GGPM_PROP_SEARCH_FIXED;
    const float th = a.t[0][r], tl = a.t[1][r], tx = h == 0 ? th : tl;
    const int limit = fixed ? min(a.steps, a.max_steps) : a.max_steps;
    float pat = a.patience, prev = 0.f;
    int n = 0;
    bool stopped = false;                    // soft mode's delta exit
    while (n < limit && (fixed || pat > 0.f)) {
        head_walk_forward(a.w, lds, Wp, bp, h, lt, maxn);
        const float oh = lds[a.w.ooff], ol = lds[a.w.ooff + 1];
        ++n;
        if (!fixed) {
            const float dh = oh - th, dl = ol - tl;
            const float loss = dh * dh + dl * dl;           // h-term + l-term, two roundings each (no contraction)
            if (a.mode == GGPM_PROP_SEARCH_SOFT && loss <= a.delta) { stopped = true; break; }
            if (loss > prev || fabsf(loss - prev) / prev <= a.threshold) pat = pat - 1.f;
            else pat = a.patience;
            prev = loss;
        }
        // d loss / d v of this head: g = norm (o - t), back through Linear(w, 1), then every hidden layer
        const float o = h == 0 ? oh : ol;
        const int cur = head_walk_backward(a.w, lds, Wp, h, lt, maxn, a.norm * (o - tx));
        // the reference's signed update, both heads every body: v - s lr g, s = -1 if o < t else +1
        const float step = (o < tx ? -1.f : 1.f) * a.lr;
        const float* gin = lds + a.w.goff[h][cur];
        for (int k = lt; k < a.half; k += 128) v[k] = v[k] - step * gin[k];
        __syncthreads();
    }
    // final predictions on the final latent (the reference's predict() after the search)
    head_walk_forward(a.w, lds, Wp, bp, h, lt, maxn);
    float* zo = a.z_out + (size_t)r * a.ld;
    for (int k = lt; k < a.half; k += 128) zo[h * a.half + k] = v[k];
    if (tid == 0) {
        for (int k = 2 * a.half; k < a.ld; ++k) zo[k] = a.z[(size_t)r * a.ld + k];
        a.pred[r] = lds[a.w.ooff];
        a.pred[(size_t)a.B + r] = lds[a.w.ooff + 1];
        a.steps_taken[r] = n;
        const bool capped = fixed ? a.steps > a.max_steps : (!stopped && pat > 0.f && n >= a.max_steps);
        a.status[r] = capped ? GGPM_PROP_CAPPED : GGPM_PROP_DONE;
    }
}

size_t head_stash_floats(const HeadK& H, int B) {
    size_t f = 0;
    for (int l = 1; l < H.n; ++l) f += (size_t)B * H.w[l];
    return f;
}

size_t align_floats(size_t f) { return (f + 63) & ~(size_t)63; }     // 256-byte aligned sub-buffers

// workspace: per head, the stashed inputs of Linear 1..n-1, then the backward's [B, max width] ping-pong
size_t heads_workspace(const HeadK* hk, int B, float* base, float* xs[2][PROP_MAX_LINEAR - 1], float* D[2][2]) {
    size_t off = 0;
    for (int h = 0; h < 2; ++h) {
        for (int l = 1; l < hk[h].n; ++l) {
            if (base) xs[h][l - 1] = base + off;
            off += align_floats((size_t)B * hk[h].w[l]);
        }
        const size_t d = align_floats((size_t)B * head_max_width(hk[h]));
        if (base) { D[h][0] = base + off; D[h][1] = base + off + d; }
        off += 2 * d;
    }
    return off * sizeof(float);
}

}  // namespace

extern "C" size_t ggpm_property_heads_workspace_bytes(int B, int half, const ggpm_prop_head* homo,
                                                      const ggpm_prop_head* lumo) {
    HeadK hk[2];
    if (B < 1 || head_from(homo, half, hk[0]) != GGPM_OK || head_from(lumo, half, hk[1]) != GGPM_OK) return 0;
    return heads_workspace(hk, B, nullptr, nullptr, nullptr);
}

extern "C" int ggpm_property_heads_forward(int B, const float* z, int ld, int half, const ggpm_prop_head* homo,
                                           const ggpm_prop_head* lumo, const float* t_homo, const float* t_lumo, float p,
                                           unsigned int seed_lo, unsigned int seed_hi, float* pred, float* loss, void* ws,
                                           size_t ws_bytes, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    HeadsFwdArgs a{};
    int e;
    if ((e = head_from(homo, half, a.head[0])) != GGPM_OK || (e = head_from(lumo, half, a.head[1])) != GGPM_OK) return e;
    if (!z || !pred || B < 1 || ld < 2 * half || !(p >= 0.f && p < 1.f)) return GGPM_ERR_ARG;
    if (loss && (!t_homo || !t_lumo)) return GGPM_ERR_ARG;
    if (B > PROP_MAX_B) return GGPM_ERR_UNSUPPORTED;
    float* D[2][2];
    const size_t need = heads_workspace(a.head, B, nullptr, nullptr, nullptr);
    if (!ws || ws_bytes < need) return GGPM_ERR_WORKSPACE;
    heads_workspace(a.head, B, static_cast<float*>(ws), a.xs, D);
    a.B = B; a.ld = ld; a.half = half; a.z = z; a.t[0] = t_homo; a.t[1] = t_lumo;
    a.thresh = p > 0.f ? (unsigned int)((double)p * 16777216.0) : 0u;
    a.scale = 1.0f / (1.0f - p);
    a.seed_lo = seed_lo; a.seed_hi = seed_hi; a.pred = pred; a.loss = loss;
    prop_heads_fwd_k<<<2, HEAD_THREADS, 0, (hipStream_t)stream>>>(a);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_property_heads_backward(int B, const float* z, int ld, int half, const ggpm_prop_head* homo,
                                            const ggpm_prop_head* lumo, const float* t_homo, const float* t_lumo, float p,
                                            const float* pred, const float* dloss, void* ws, size_t ws_bytes, float* dz,
                                            int ld_dz, int accumulate_dz, const ggpm_prop_head_grads* g_homo,
                                            const ggpm_prop_head_grads* g_lumo, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    HeadsBwdArgs a{};
    int e;
    if ((e = head_from(homo, half, a.head[0])) != GGPM_OK || (e = head_from(lumo, half, a.head[1])) != GGPM_OK) return e;
    if (!z || !pred || !dloss || !t_homo || !t_lumo || B < 1 || ld < 2 * half || !(p >= 0.f && p < 1.f)) return GGPM_ERR_ARG;
    if (dz && ld_dz < 2 * half) return GGPM_ERR_ARG;
    if (B > PROP_MAX_B) return GGPM_ERR_UNSUPPORTED;
    float* base = static_cast<float*>(ws);
    float* xs[2][PROP_MAX_LINEAR - 1] = {};
    const size_t need = heads_workspace(a.head, B, nullptr, nullptr, nullptr);
    if (!ws || ws_bytes < need) return GGPM_ERR_WORKSPACE;
    heads_workspace(a.head, B, base, xs, a.D);
    for (int h = 0; h < 2; ++h)
        for (int l = 0; l < PROP_MAX_LINEAR - 1; ++l) a.xs[h][l] = xs[h][l];
    const ggpm_prop_head_grads* gs[2] = {g_homo, g_lumo};
    for (int h = 0; h < 2; ++h) {
        a.g[h] = GradK{};
        if (!gs[h]) continue;
        for (int l = 0; l < a.head[h].n; ++l) { a.g[h].dW[l] = gs[h]->dW[l]; a.g[h].db[l] = gs[h]->db[l]; }
        a.g[h].acc = gs[h]->accumulate != 0;
    }
    a.B = B; a.ld = ld; a.half = half; a.ld_dz = ld_dz; a.acc_dz = accumulate_dz != 0;
    a.z = z; a.t[0] = t_homo; a.t[1] = t_lumo; a.pred = pred; a.dloss = dloss; a.dz = dz;
    a.norm = (float)(2.0 / (double)B);
    a.scale = p > 0.f ? 1.0f / (1.0f - p) : 1.0f;
    prop_heads_bwd_k<<<2, HEAD_THREADS, 0, (hipStream_t)stream>>>(a);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_property_latent_search(int mode, int B, const float* z, int ld, int half, const ggpm_prop_head* homo,
                                           const ggpm_prop_head* lumo, const float* t_homo, const float* t_lumo, float lr,
                                           int steps, float delta, float patience, float threshold, int max_steps,
                                           float* z_out, float* pred_out, int32_t* steps_taken, int32_t* status,
                                           ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    SearchArgs a{};
    int e;
    if ((e = head_from(homo, half, a.w.head[0])) != GGPM_OK || (e = head_from(lumo, half, a.w.head[1])) != GGPM_OK) return e;
    if (mode != GGPM_PROP_SEARCH_FIXED && mode != GGPM_PROP_SEARCH_SOFT && mode != GGPM_PROP_SEARCH_PATIENCE)
        return GGPM_ERR_ARG;
    if (!z || !t_homo || !t_lumo || !z_out || !pred_out || !steps_taken || !status || B < 1 || ld < 2 * half ||
        max_steps < 1 || (mode == GGPM_PROP_SEARCH_FIXED && steps < 0))
        return GGPM_ERR_ARG;
    if (B > PROP_MAX_SEARCH_B) return GGPM_ERR_UNSUPPORTED;
    const size_t lds_bytes = head_walk_plan(a.w, 0, nullptr);
    if (lds_bytes > SEARCH_LDS_MAX) return GGPM_ERR_UNSUPPORTED;
    a.mode = mode; a.B = B; a.ld = ld; a.half = half; a.steps = steps; a.max_steps = max_steps;
    a.z = z; a.t[0] = t_homo; a.t[1] = t_lumo;
    a.lr = lr; a.delta = delta; a.patience = patience; a.threshold = threshold;
    a.norm = mode == GGPM_PROP_SEARCH_FIXED ? (float)(2.0 / (double)B) : 2.0f;
    a.z_out = z_out; a.pred = pred_out; a.steps_taken = steps_taken; a.status = status;
    if (lds_bytes > 64 * 1024) ggpm_set_lds(prop_search_k, lds_bytes);
    prop_search_k<<<B, SEARCH_THREADS, lds_bytes, (hipStream_t)stream>>>(a);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}
