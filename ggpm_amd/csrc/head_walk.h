// What the two latent searches share (csrc/property.hip: prop_search_k; csrc/latent_search.hip: latent_search_guided_k): a
// property head as the kernels see it, the LDS plan of a workgroup that walks both heads on ONE resident row -- the homo head
// on lanes 0..127, the lumo head on lanes 128..255 --, and the walk itself: weights to LDS, forward, gradient by the input.
//
// Floating point: contraction is off for everything in this header and in the files that include it, so `a * b + c` is two
// roundings; the dot products use explicit fma, k (forward) or j (backward) ascending.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int PROP_MAX_LINEAR = GGPM_PROP_MAX_LINEAR;
constexpr int PROP_MAX_IN = 256;
constexpr int PROP_MAX_W = 512;
constexpr int SEARCH_THREADS = 256;         // two halves of 128 lanes: homo head, lumo head
constexpr size_t SEARCH_LDS_MAX = 160 * 1024;

struct HeadK {
    int n;                                   // number of Linear layers
    int w[PROP_MAX_LINEAR + 1];              // w[0] input, w[n] = 1
    const float* W[PROP_MAX_LINEAR];
    const float* b[PROP_MAX_LINEAR];
};

// LDS (floats): [weights of both heads, if they fit] [inputs of every Linear] [gradient ping-pong] [two outputs] [extra]
struct HeadWalk {
    HeadK head[2];
    int in_lds;
    int woff[2][PROP_MAX_LINEAR], boff[2][PROP_MAX_LINEAR];   // LDS offsets of the weights (in_lds)
    int wld[2][PROP_MAX_LINEAR];                                // row stride of W[l] as read (LDS: odd, conflict-free)
    int aoff[2][PROP_MAX_LINEAR];                               // LDS offsets of the inputs of every Linear
    int goff[2][2];                                             // LDS gradient ping-pong
    int ooff;                                                   // LDS: the two head outputs
};

__device__ __forceinline__ float wave_sum_fixed(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// where head h's lanes read its weights: LDS (filled by this call; the caller's barrier follows) or global
__device__ __forceinline__ void head_walk_weights(const HeadWalk& a, float* lds, int h, int lt, float** Wp, float** bp) {
    const HeadK& H = a.head[h];
    for (int l = 0; l < PROP_MAX_LINEAR; ++l) {
        Wp[l] = bp[l] = nullptr;
        if (l < H.n) {
            Wp[l] = a.in_lds ? lds + a.woff[h][l] : const_cast<float*>(H.W[l]);
            bp[l] = a.in_lds ? lds + a.boff[h][l] : const_cast<float*>(H.b[l]);
        }
    }
    if (a.in_lds) {
        for (int l = 0; l < H.n; ++l) {
            const int win = H.w[l], nw = win * H.w[l + 1], nb = H.w[l + 1], ldw = a.wld[h][l];
            for (int i = lt; i < nw; i += 128) Wp[l][(i / win) * ldw + i % win] = H.W[l][i];
            for (int i = lt; i < nb; i += 128) bp[l][i] = H.b[l][i];
        }
    }
}

// forward of both heads on the resident row: fills act[h][1..n-1] and o[h]
__device__ __forceinline__ void head_walk_forward(const HeadWalk& a, float* lds, float* const* Wp, float* const* bp, int h,
                                                  int lt, int maxn) {
    const HeadK& H = a.head[h];
    for (int l = 0; l < maxn; ++l) {
        if (l < H.n) {
            const int win = H.w[l], wout = H.w[l + 1];
            const float* W = Wp[l];
            const float* bias = bp[l];
            const float* x = lds + a.aoff[h][l];
            if (l < H.n - 1) {
                float* y = lds + a.aoff[h][l + 1];
                for (int j = lt; j < wout; j += 128) {
                    const float* wr = W + (size_t)j * a.wld[h][l];
                    float s = 0.f;
                    for (int k = 0; k < win; ++k) s = __builtin_fmaf(wr[k], x[k], s);
                    s = s + bias[j];
                    y[j] = s > 0.f ? s : 0.f;
                }
            } else if (lt < 64) {           // Linear(w, 1): one full wave, lane-strided partials + fixed butterfly
                float s = 0.f;
                for (int k = lt; k < win; k += 64) s = __builtin_fmaf(W[k], x[k], s);
                s = wave_sum_fixed(s);
                if (lt == 0) lds[a.ooff + h] = s + bias[0];
            }
        }
        __syncthreads();
    }
}

// g = d objective / d o of head h -> its gradient by the head's input: back through Linear(w, 1), then every hidden layer.
// Returns which half of the ping-pong holds it (lds + goff[h][.]); ends on a barrier.
__device__ __forceinline__ int head_walk_backward(const HeadWalk& a, float* lds, float* const* Wp, int h, int lt, int maxn,
                                                  float g) {
    const HeadK& H = a.head[h];
    {
        const int l = H.n - 1, win = H.w[l];
        float* gin = lds + a.goff[h][0];
        for (int k = lt; k < win; k += 128) gin[k] = g * Wp[l][k];
    }
    __syncthreads();
    int cur = 0;
    for (int s = 1; s < maxn; ++s) {
        const int l = H.n - 1 - s;      // Linear l: input w[l], output w[l + 1] (its output went through ReLU)
        if (l >= 0) {
            const int win = H.w[l], wout = H.w[l + 1];
            const float* gout = lds + a.goff[h][cur];
            const float* act = lds + a.aoff[h][l + 1];
            float* gin = lds + a.goff[h][cur ^ 1];
            const float* W = Wp[l];
            for (int k = lt; k < win; k += 128) {
                float acc = 0.f;
                for (int j = 0; j < wout; ++j)
                    acc = __builtin_fmaf(act[j] > 0.f ? gout[j] : 0.f, W[(size_t)j * a.wld[h][l] + k], acc);
                gin[k] = acc;
            }
        }
        __syncthreads();
        if (l >= 0) cur ^= 1;
    }
    return cur;
}

inline int head_from(const ggpm_prop_head* in, int half, HeadK& out) {
    if (!in) return GGPM_ERR_ARG;
    const int n = in->n_linear;
    if (n < 2 || n > PROP_MAX_LINEAR) return GGPM_ERR_UNSUPPORTED;
    if (in->width[0] != half || in->width[n] != 1) return GGPM_ERR_ARG;
    if (half < 1 || half > PROP_MAX_IN) return GGPM_ERR_UNSUPPORTED;
    out = HeadK{};
    out.n = n;
    for (int l = 0; l <= n; ++l) {
        if (in->width[l] < 1) return GGPM_ERR_ARG;
        if (l > 0 && l < n && in->width[l] > PROP_MAX_W) return GGPM_ERR_UNSUPPORTED;
        out.w[l] = in->width[l];
    }
    for (int l = 0; l < n; ++l) {
        if (!in->W[l] || !in->b[l]) return GGPM_ERR_ARG;
        out.W[l] = in->W[l];
        out.b[l] = in->b[l];
    }
    return GGPM_OK;
}

inline int head_max_width(const HeadK& H) {
    int m = 1;
    for (int l = 0; l < H.n; ++l) m = max(m, H.w[l]);
    return m;
}

// Fills the plan of a.head[0..1] with `extra` further floats resident beside it (at *extra_off): the weights go to LDS when
// everything fits in SEARCH_LDS_MAX, otherwise they are read from global.  Returns the dynamic LDS bytes of the launch
// (more than SEARCH_LDS_MAX: the shape is unsupported).
inline size_t head_walk_plan(HeadWalk& a, size_t extra, int* extra_off) {
    size_t off = 0;
    for (int h = 0; h < 2; ++h)
        for (int l = 0; l < a.head[h].n; ++l) {
            // rows of W in LDS at an odd stride: the forward's lanes (one row each) then hit distinct banks
            a.wld[h][l] = a.head[h].w[l] | 1;
            a.woff[h][l] = (int)off; off += (size_t)a.wld[h][l] * a.head[h].w[l + 1];
            a.boff[h][l] = (int)off; off += (size_t)a.head[h].w[l + 1];
        }
    const size_t weight_floats = off;
    size_t rest = 0;
    int aoff[2][PROP_MAX_LINEAR] = {}, goff[2][2] = {};
    for (int h = 0; h < 2; ++h) {
        for (int l = 0; l < a.head[h].n; ++l) { aoff[h][l] = (int)rest; rest += (size_t)a.head[h].w[l]; }
        const int wm = head_max_width(a.head[h]);
        goff[h][0] = (int)rest; rest += wm;
        goff[h][1] = (int)rest; rest += wm;
    }
    const int ooff = (int)rest;
    rest += 2;
    a.in_lds = (weight_floats + rest + extra) * sizeof(float) <= SEARCH_LDS_MAX;
    if (!a.in_lds)
        for (int h = 0; h < 2; ++h)
            for (int l = 0; l < a.head[h].n; ++l) a.wld[h][l] = a.head[h].w[l];
    const size_t base = a.in_lds ? weight_floats : 0;
    for (int h = 0; h < 2; ++h) {
        for (int l = 0; l < PROP_MAX_LINEAR; ++l) a.aoff[h][l] = (int)base + aoff[h][l];
        a.goff[h][0] = (int)base + goff[h][0];
        a.goff[h][1] = (int)base + goff[h][1];
    }
    a.ooff = (int)base + ooff;
    if (extra_off) *extra_off = (int)(base + rest);
    return (base + rest + extra) * sizeof(float);
}

}  // namespace
