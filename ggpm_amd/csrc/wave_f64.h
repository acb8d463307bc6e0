// What the fp64 latent kernels share (csrc/latent_decomp.hip, csrc/latent_prior.hip): the fixed shuffle tree over a wave's fp64
// partials and the logsumexp in flight.  Everything is a function of its arguments alone and symmetric where two lanes
// exchange values, so a reduction's result does not depend on which lane reads it.
#pragma once
#include "common.h"

#include <cmath>

#define LOG_2PI 1.8378770664093454835606594728112

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// a logsumexp in flight: log(sum) = m + log(s); the empty one is (-inf, 0)
struct Lse {
    double m, s;
};

// symmetric in its arguments bit for bit (max and the fp64 addition commute), so both lanes of a butterfly step hold the
// same pair afterwards
__device__ __forceinline__ Lse lse_merge(Lse a, Lse b) {
    Lse r;
    r.m = fmax(a.m, b.m);
    if (r.m == -INFINITY) {
        r.s = 0.0;
        return r;
    }
    r.s = a.s * exp(a.m - r.m) + b.s * exp(b.m - r.m);
    return r;
}

__device__ __forceinline__ Lse lse_push(Lse a, double v) {
    Lse b;
    b.m = v;
    b.s = 1.0;
    return lse_merge(a, b);
}

__device__ __forceinline__ Lse wave_lse(Lse v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        Lse o;
        o.m = __shfl_xor(v.m, off);
        o.s = __shfl_xor(v.s, off);
        v = lse_merge(v, o);
    }
    return v;
}

__device__ __forceinline__ double lse_value(Lse v) { return v.m + log(v.s); }
