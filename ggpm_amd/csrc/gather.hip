// Row gathers and segmented sums over CSR lists (HBM / L2 bound; fp32 rows of H floats).
// One wave owns one destination row and walks its (short) list; lanes stride the feature dimension
// with 16-byte accesses when the strides allow it, so every load/store is a coalesced row segment.
#include "common.h"
#include <cmath>

namespace {

// The segmented sum (every entry point's): one wave per destination row walks the row's list in order.  Two options let the
// backward drivers drop the launches around it (same sums, same order):
//   addend  the value a row starts from (null: zero; `out` itself: plain accumulation; a matrix of its own: what accumulating
//           onto a copy of it gives),
//   dpre    a second, masked output dpre = act'(y) applied to the finished sum, by ggpm_act_grad (what act_backward_k does
//           to `out` in a launch of its own); `out` may then be left out.
// blockIdx.y picks one of up to two problems over the same CSR (the root read-out's two gradients).
struct SegmentSumX {
    const float* src[2];
    const float* addend[2];
    float* out[2];
    const float* y[2];
    float* dpre[2];
    int ld_src, ld_addend, ld_out, ld_mask, act, zero_row0, zero_to;
};
template <bool VEC>
__global__ void __launch_bounds__(256) segment_sum_x_k(SegmentSumX a, const int32_t* __restrict__ rowptr,
                                                       const int32_t* __restrict__ col, int rows, int width) {
    const int lane = threadIdx.x & 63, p = blockIdx.y;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lo = rowptr[r], hi = rowptr[r + 1];
    const float* __restrict__ src = a.src[p];
    const float* add = a.addend[p] ? a.addend[p] + (size_t)r * a.ld_addend : nullptr;
    float* dst = a.out[p] ? a.out[p] + (size_t)r * a.ld_out : nullptr;
    const float* y = a.dpre[p] ? a.y[p] + (size_t)r * a.ld_mask : nullptr;
    float* dp = a.dpre[p] ? a.dpre[p] + (size_t)r * a.ld_mask : nullptr;
    const bool zero_row = a.zero_row0 && r == 0;
    if (dst) for (int c = width + lane; c < a.zero_to; c += 64) dst[c] = 0.f;      // pad columns of the row
    if (VEC) {
        for (int c = lane * 4; c < width; c += 256) {
            float4 acc = add ? ggpm_ld4(add + c) : ggpm_zero4();
            for (int j = lo; j < hi; ++j) acc = acc + ggpm_ld4(src + (size_t)col[j] * a.ld_src + c);
            if (dst) ggpm_st4(dst + c, acc);
            if (dp) {
                const float4 o = ggpm_ld4(y + c);
                float4 g;
                g.x = ggpm_act_grad(acc.x, o.x, a.act); g.y = ggpm_act_grad(acc.y, o.y, a.act);
                g.z = ggpm_act_grad(acc.z, o.z, a.act); g.w = ggpm_act_grad(acc.w, o.w, a.act);
                if (zero_row) g = ggpm_zero4();
                ggpm_st4(dp + c, g);
            }
        }
    } else {
        for (int c = lane; c < width; c += 64) {
            float acc = add ? add[c] : 0.f;
            for (int j = lo; j < hi; ++j) acc += src[(size_t)col[j] * a.ld_src + c];
            if (dst) dst[c] = acc;
            if (dp) dp[c] = zero_row ? 0.f : ggpm_act_grad(acc, y[c], a.act);
        }
    }
}

__global__ void __launch_bounds__(256) gather_rows_k(const float* __restrict__ table, int ld_table,
                                                     const int32_t* __restrict__ idx, int rows, int width,
                                                     float* __restrict__ out, int ld_out, int col_off, int zero_to) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int id = idx[r];
    float* dst = out + (size_t)r * ld_out + col_off;
    for (int c = width + lane; c < zero_to - col_off; c += 64) dst[c] = 0.f;
    if (id < 0) {
        for (int c = lane; c < width; c += 64) dst[c] = 0.f;
    } else {
        const float* s = table + (size_t)id * ld_table;
        for (int c = lane; c < width; c += 64) dst[c] = s[c];
    }
}

// dst[idx[r]] (+)= src[r]: the write side of gather_rows_k for UNIQUE indices (no atomics), one wave per row.
__global__ void __launch_bounds__(256) scatter_rows_k(const float* __restrict__ src, int ld_src,
                                                      const int32_t* __restrict__ idx, int rows, int width,
                                                      float* __restrict__ dst, int ld_dst, int accumulate) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int id = idx[r];
    if (id < 0) return;
    const float* s = src + (size_t)r * ld_src;
    float* d = dst + (size_t)id * ld_dst;
    if (accumulate) for (int c = lane; c < width; c += 64) d[c] += s[c];
    else for (int c = lane; c < width; c += 64) d[c] = s[c];
}

__global__ void onehot_k(const int32_t* __restrict__ idx, int rows, int classes, float* __restrict__ out,
                         int ld_out, int col_off, int zero_to) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (col_off + c >= (zero_to > col_off + classes ? zero_to : col_off + classes)) return;
    out[(size_t)r * ld_out + col_off + c] = (c < classes && idx[r] == c) ? 1.f : 0.f;
}

__global__ void embed_graph_k(const int64_t* __restrict__ fnode, int N1, const int64_t* __restrict__ fmess,
                              int E1, int atom_size, int bond_types, int max_pos, float* __restrict__ hnode,
                              int ld_n, float* __restrict__ hmess, int ld_m) {
    const int r = blockIdx.x;
    const int c = threadIdx.x;
    if (r < N1) {
        if (c < ld_n) hnode[(size_t)r * ld_n + c] = (c < atom_size && fnode[r] == c) ? 1.f : 0.f;
    } else {
        const int e = r - N1;
        if (e < E1 && c < ld_m) {
            const int64_t* f = fmess + (size_t)e * 4;
            const int64_t a = fnode[f[0]];
            float v = 0.f;
            if (c < atom_size) v = (a == c) ? 1.f : 0.f;
            else if (c < atom_size + bond_types) v = (f[2] == c - atom_size) ? 1.f : 0.f;
            else if (c < atom_size + bond_types + max_pos) v = (f[3] == c - atom_size - bond_types) ? 1.f : 0.f;
            hmess[(size_t)e * ld_m + c] = v;
        }
    }
}

}  // namespace

extern "C" int ggpm_segment_sum(const float* src, int ld_src, const int32_t* rowptr, const int32_t* col,
                                int rows, int width, float* out, int ld_out, int accumulate, int zero_to,
                                ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!src || !rowptr || !col || !out || rows <= 0 || width <= 0) return GGPM_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = (width % 4 == 0) && (ld_src % 4 == 0) && (ld_out % 4 == 0) &&
                     (((uintptr_t)src & 15) == 0) && (((uintptr_t)out & 15) == 0);
    SegmentSumX a = {};
    a.src[0] = src; a.out[0] = out; a.addend[0] = accumulate ? out : nullptr;
    a.ld_src = ld_src; a.ld_out = a.ld_addend = ld_out; a.zero_to = zero_to;
    const dim3 grid(ggpm_ceil_div(rows, 4), 1);
    if (vec) segment_sum_x_k<true><<<grid, 256, 0, s>>>(a, rowptr, col, rows, width);
    else segment_sum_x_k<false><<<grid, 256, 0, s>>>(a, rowptr, col, rows, width);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_segment_sum_masked(int count, const float* const* src, int ld_src, const int32_t* rowptr, const int32_t* col,
                                       int rows, int width, const float* const* addend, int ld_addend, float* const* out,
                                       int ld_out, int zero_to, const float* const* y, float* const* dpre, int ld_mask, int act,
                                       int zero_row0, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (count < 1 || count > 2 || !src || !rowptr || !col || rows <= 0 || width <= 0) return GGPM_ERR_ARG;
    SegmentSumX a = {};
    bool vec = (width % 4 == 0) && (ld_src % 4 == 0);
    bool any_add = false, any_out = false, any_mask = false;
    for (int i = 0; i < count; ++i) {
        a.src[i] = src[i];
        a.addend[i] = addend ? addend[i] : nullptr;
        a.out[i] = out ? out[i] : nullptr;
        a.dpre[i] = dpre ? dpre[i] : nullptr;
        a.y[i] = y ? y[i] : nullptr;
        if (!a.src[i] || (!a.out[i] && !a.dpre[i]) || (a.dpre[i] && !a.y[i])) return GGPM_ERR_ARG;
        any_add = any_add || a.addend[i]; any_out = any_out || a.out[i]; any_mask = any_mask || a.dpre[i];
        vec = vec && (((uintptr_t)a.src[i] | (uintptr_t)a.addend[i] | (uintptr_t)a.out[i] | (uintptr_t)a.y[i] |
                       (uintptr_t)a.dpre[i]) & 15) == 0;
    }
    if ((any_add && ld_addend < width) || (any_out && ld_out < width) || (any_mask && ld_mask < width)) return GGPM_ERR_ARG;
    vec = vec && (!any_add || ld_addend % 4 == 0) && (!any_out || ld_out % 4 == 0) && (!any_mask || ld_mask % 4 == 0);
    a.ld_src = ld_src; a.ld_addend = ld_addend; a.ld_out = ld_out; a.ld_mask = ld_mask; a.act = act; a.zero_row0 = zero_row0;
    a.zero_to = zero_to;
    dim3 grid(ggpm_ceil_div(rows, 4), count);
    if (vec) segment_sum_x_k<true><<<grid, 256, 0, (hipStream_t)stream>>>(a, rowptr, col, rows, width);
    else segment_sum_x_k<false><<<grid, 256, 0, (hipStream_t)stream>>>(a, rowptr, col, rows, width);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_gather_rows(const float* table, int ld_table, const int32_t* idx, int rows, int width,
                                float* out, int ld_out, int col_off, int zero_to, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!table || !idx || !out || rows <= 0 || width <= 0) return GGPM_ERR_ARG;
    gather_rows_k<<<ggpm_ceil_div(rows, 4), 256, 0, (hipStream_t)stream>>>(table, ld_table, idx, rows, width, out,
                                                                          ld_out, col_off, zero_to);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_scatter_rows(const float* src, int ld_src, const int32_t* idx, int rows, int width, float* dst,
                                 int ld_dst, int accumulate, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!src || !idx || !dst || rows <= 0 || width <= 0) return GGPM_ERR_ARG;
    scatter_rows_k<<<ggpm_ceil_div(rows, 4), 256, 0, (hipStream_t)stream>>>(src, ld_src, idx, rows, width, dst, ld_dst,
                                                                           accumulate);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_onehot(const int32_t* idx, int rows, int classes, float* out, int ld_out, int col_off, int zero_to,
                           ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!idx || !out || rows <= 0 || classes <= 0) return GGPM_ERR_ARG;
    const int span = (zero_to > col_off + classes ? zero_to - col_off : classes);
    dim3 grid(ggpm_ceil_div(span, 64), rows);
    onehot_k<<<grid, 64, 0, (hipStream_t)stream>>>(idx, rows, classes, out, ld_out, col_off, zero_to);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_embed_graph(const int64_t* fnode, int N1, const int64_t* fmess, int E1, int atom_size,
                                int bond_types, int max_pos, float* hnode, int ld_n, float* hmess, int ld_m,
                                ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!fnode || !fmess || !hnode || !hmess || N1 <= 0 || E1 <= 0) return GGPM_ERR_ARG;
    if (ld_n > 256 || ld_m > 256 || ld_n < atom_size || ld_m < atom_size + bond_types + max_pos)
        return GGPM_ERR_UNSUPPORTED;
    embed_graph_k<<<N1 + E1, 256, 0, (hipStream_t)stream>>>(fnode, N1, fmess, E1, atom_size, bond_types, max_pos,
                                                           hnode, ld_n, hmess, ld_m);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}


// ---------------------------------------------------------------- dropout (counter-based, stateless)
namespace {
__device__ __forceinline__ unsigned int fmix32(unsigned int h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

__global__ void dropout_k(float* __restrict__ x, int rows, int cols, int ld, unsigned int thresh, float scale,
                          unsigned int seed_lo, unsigned int seed_hi, unsigned int site) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (c >= cols) return;
    const unsigned int idx = (unsigned int)r * (unsigned int)cols + (unsigned int)c;
    unsigned int h = fmix32(idx * 0x9E3779B1u + seed_lo);
    h = fmix32(h ^ (seed_hi + site * 0x7F4A7C15u));
    float* p = x + (size_t)r * ld + c;
    *p = ((h >> 8) >= thresh) ? *p * scale : 0.f;
}
}  // namespace

namespace {
// Adam (torch.optim.Adam's arithmetic, vae_train.py:60) over one flat fp32 buffer: 16 B per lane, grid-stride.
__global__ void __launch_bounds__(256) adam_flat_k(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, size_t n, float b1,
                                                   float b2, float eps, float wd, float step_size, float inv_bc2_sqrt) {
    const size_t n4 = n >> 2;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        float4 pp = ggpm_ld4(p + 4 * i), gg = ggpm_ld4(g + 4 * i), mm = ggpm_ld4(m + 4 * i), vv = ggpm_ld4(v + 4 * i);
        float* P = &pp.x; float* G = &gg.x; float* M = &mm.x; float* V = &vv.x;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float gr = wd != 0.f ? G[k] + wd * P[k] : G[k];
            M[k] = M[k] + (1.f - b1) * (gr - M[k]);
            V[k] = b2 * V[k] + (1.f - b2) * gr * gr;
            P[k] -= step_size * M[k] / (sqrtf(V[k]) * inv_bc2_sqrt + eps);
        }
        ggpm_st4(p + 4 * i, pp); ggpm_st4(m + 4 * i, mm); ggpm_st4(v + 4 * i, vv);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {          // tail of up to three elements
        const size_t i = (n4 << 2) + threadIdx.x;
        const float gr = wd != 0.f ? g[i] + wd * p[i] : g[i];
        const float mk = m[i] + (1.f - b1) * (gr - m[i]);
        const float vk = b2 * v[i] + (1.f - b2) * gr * gr;
        m[i] = mk; v[i] = vk;
        p[i] -= step_size * mk / (sqrtf(vk) * inv_bc2_sqrt + eps);
    }
}
}  // namespace

extern "C" int ggpm_adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                              float eps, float weight_decay, int step, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!p || !g || !m || !v || n == 0 || step < 1) return GGPM_ERR_ARG;
    if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) != 0) return GGPM_ERR_ARG;
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    const float step_size = (float)((double)lr / bc1), inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    size_t blocks = ((n >> 2) + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    adam_flat_k<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(p, g, m, v, n, beta1, beta2, eps, weight_decay, step_size,
                                                                 inv_bc2_sqrt);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

// ---------------------------------------------------------------- gradient-norm clipping and parameter groups (FlatAdam)
// clip_grad_norm_ (vae_train.py:82) and the four optimizers of vae_fine_tune_indv_opt.py:61-70 on the flat buffers.  The sum
// of squares crosses workgroups through KERNEL BOUNDARIES only: one launch writes a double per workgroup, the next launch
// (the Adam step, or the one-workgroup finish behind grad_norm() / param_norm()) adds them up in index order -- every
// workgroup for itself, from the same values in the same order, so all of them hold the same bits.  No counters, no atomics.
namespace {
constexpr int NORM_THREADS = 1024;                       // 16 waves: one workgroup per CU keeps 64 KB of loads in flight
constexpr int NORM_MAX_PARTIALS = GGPM_NORM_MAX_PARTIALS;

__host__ __device__ inline unsigned norm_grid(size_t n) {
    size_t blocks = ((n >> 2) + NORM_THREADS - 1) / NORM_THREADS;
    return (unsigned)(blocks < 1 ? 1 : blocks > (size_t)NORM_MAX_PARTIALS ? (size_t)NORM_MAX_PARTIALS : blocks);
}

__device__ __forceinline__ void sq_acc4(double (&acc)[4], float4 x) {
    acc[0] += (double)x.x * (double)x.x; acc[1] += (double)x.y * (double)x.y;
    acc[2] += (double)x.z * (double)x.z; acc[3] += (double)x.w * (double)x.w;
}

// partials[blockIdx.x] = sum of squares of this workgroup's grid-stride share, fp64 throughout.  The order of every addition
// is a function of n alone: four accumulators per thread (one per float4 component), lanes by shuffle, waves in index order.
__global__ void __launch_bounds__(NORM_THREADS) flat_sqnorm_partials_k(const float* __restrict__ x, size_t n,
                                                                       double* __restrict__ partials) {
    __shared__ double wave_sum[NORM_THREADS / 64];
    const size_t n4 = n >> 2, stride = (size_t)gridDim.x * NORM_THREADS;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    size_t i = (size_t)blockIdx.x * NORM_THREADS + threadIdx.x;
    for (; i + 3 * stride < n4; i += 4 * stride) {         // four independent 16-byte loads in flight per lane
        const float4 a = ggpm_ld4(x + 4 * i), b = ggpm_ld4(x + 4 * (i + stride)), c = ggpm_ld4(x + 4 * (i + 2 * stride)),
                     d = ggpm_ld4(x + 4 * (i + 3 * stride));
        sq_acc4(acc, a); sq_acc4(acc, b); sq_acc4(acc, c); sq_acc4(acc, d);
    }
    for (; i < n4; i += stride) sq_acc4(acc, ggpm_ld4(x + 4 * i));
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {         // tail of up to three elements
        const double t = (double)x[(n4 << 2) + threadIdx.x];
        acc[0] += t * t;
    }
    double s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < NORM_THREADS / 64; ++w) t += wave_sum[w];
        partials[blockIdx.x] = t;
    }
}

// The partials, staged in LDS by the caller (a barrier behind the staging), summed in index order; the norm and
// clip_grad_norm_'s coefficient max_norm / (norm + 1e-6) clamped to 1 as torch.clamp does (a NaN stays a NaN).
__device__ __forceinline__ void norm_and_coef(const double* staged, int n_partials, float max_norm, float& norm, float& coef) {
    double s = 0.0;
    for (int i = 0; i < n_partials; ++i) s += staged[i];
    norm = (float)sqrt(s);
    const float c = max_norm / (norm + 1e-6f);
    coef = c > 1.0f ? 1.0f : c;
}

__global__ void __launch_bounds__(NORM_MAX_PARTIALS) flat_norm_finish_k(const double* __restrict__ partials, int n_partials,
                                                                        float max_norm, float* __restrict__ out) {
    __shared__ double staged[NORM_MAX_PARTIALS];
    if ((int)threadIdx.x < n_partials) staged[threadIdx.x] = partials[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
        float norm, coef;
        norm_and_coef(staged, n_partials, max_norm, norm, coef);
        out[0] = norm;
        if (max_norm > 0.f) out[1] = coef;
    }
}

struct AdamGroupsArgs {                                    // by value: row k of `hp` is group k
    float hp[GGPM_ADAM_MAX_GROUPS][8];                     // b1, b2, eps, wd, step_size, inv_bc2_sqrt, 0, 0
};

// adam_flat_k's arithmetic with the hyper-parameters looked up per 64-float tile (tile_group; null: group 0 everywhere)
// and the gradient scaled by the clip coefficient formed from `partials` (null: no clip).  n % 64 == 0.
__global__ void __launch_bounds__(256) adam_groups_k(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                     float* __restrict__ v, size_t n, const uint8_t* __restrict__ tile_group,
                                                     AdamGroupsArgs args, const double* __restrict__ partials,
                                                     int n_partials, float max_norm, float* __restrict__ clip_out,
                                                     int write_clipped) {
    __shared__ double staged[NORM_MAX_PARTIALS];
    __shared__ __attribute__((aligned(16))) float hp[GGPM_ADAM_MAX_GROUPS][8];
    if (threadIdx.x < GGPM_ADAM_MAX_GROUPS * 8) (&hp[0][0])[threadIdx.x] = (&args.hp[0][0])[threadIdx.x];
    if (partials && (int)threadIdx.x < n_partials) staged[threadIdx.x] = partials[threadIdx.x];
    __syncthreads();
    float coef = 1.0f;
    if (partials) {
        float norm;
        norm_and_coef(staged, n_partials, max_norm, norm, coef);
        if (clip_out && blockIdx.x == 0 && threadIdx.x == 0) { clip_out[0] = norm; clip_out[1] = coef; }
    }
    const bool scale = partials != nullptr, store_g = scale && write_clipped != 0;
    const size_t n4 = n >> 2;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const int grp = tile_group ? (tile_group[i >> 4] & (GGPM_ADAM_MAX_GROUPS - 1)) : 0;
        const float4 h0 = *reinterpret_cast<const float4*>(&hp[grp][0]);
        const float b1 = h0.x, b2 = h0.y, eps = h0.z, wd = h0.w, step_size = hp[grp][4], inv_bc2_sqrt = hp[grp][5];
        float4 pp = ggpm_ld4(p + 4 * i), gg = ggpm_ld4(g + 4 * i), mm = ggpm_ld4(m + 4 * i), vv = ggpm_ld4(v + 4 * i);
        float* P = &pp.x; float* G = &gg.x; float* M = &mm.x; float* V = &vv.x;
        if (scale) {
#pragma unroll
            for (int k = 0; k < 4; ++k) G[k] *= coef;
            if (store_g) ggpm_st4(g + 4 * i, gg);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float gr = wd != 0.f ? G[k] + wd * P[k] : G[k];
            M[k] = M[k] + (1.f - b1) * (gr - M[k]);
            V[k] = b2 * V[k] + (1.f - b2) * gr * gr;
            P[k] -= step_size * M[k] / (sqrtf(V[k]) * inv_bc2_sqrt + eps);
        }
        ggpm_st4(p + 4 * i, pp); ggpm_st4(m + 4 * i, mm); ggpm_st4(v + 4 * i, vv);
    }
}

// ---------------------------------------------------------------- guarded step, effective step count, EMA (FlatAdam)
struct AdamExArgs {                                        // by value: row k of `hp` is group k
    float hp[GGPM_ADAM_MAX_GROUPS][8];                     // b1, b2, eps, wd, step_size, inv_bc2_sqrt, lr, 0
};

__device__ __forceinline__ double pow_int(double b, int e) {       // b^e, e >= 1, by squaring: one fixed order for every e
    double r = 1.0;
    for (; e > 0; e >>= 1, b *= b)
        if (e & 1) r *= b;
    return r;
}

// adam_groups_k's arithmetic (the same expressions: until a step has been skipped, the same bits) with three additions, all
// decided by every workgroup for itself from values that crossed a kernel boundary:
//   * the whole launch leaves p, m, v, ema and g alone when skip_nonfinite is set and the norm is not finite;
//   * the step count of the bias corrections is step - *skipped_in; once that differs from `step`, threads 0..n_groups-1
//     re-form step_size and inv_bc2_sqrt from it in fp64;
//   * ema += (1 - d) (p_new - ema) behind the parameter update.
// Block 0, thread 0 writes status and *skipped_out (a location no thread of this launch reads).  n % 64 == 0.
__global__ void __launch_bounds__(256) adam_ex_k(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                 float* __restrict__ v, size_t n, const uint8_t* __restrict__ tile_group,
                                                 int n_groups, AdamExArgs args, int step, const double* __restrict__ partials,
                                                 int n_partials, float max_norm, int write_clipped, float* __restrict__ ema,
                                                 float ema_decay, int ema_warmup, int skip_nonfinite,
                                                 const int* __restrict__ skipped_in, int* __restrict__ skipped_out,
                                                 float* __restrict__ status) {
    __shared__ double staged[NORM_MAX_PARTIALS];
    __shared__ __attribute__((aligned(16))) float hp[GGPM_ADAM_MAX_GROUPS][8];
    if (threadIdx.x < GGPM_ADAM_MAX_GROUPS * 8) (&hp[0][0])[threadIdx.x] = (&args.hp[0][0])[threadIdx.x];
    if (partials && (int)threadIdx.x < n_partials) staged[threadIdx.x] = partials[threadIdx.x];
    const int skipped = skipped_in ? *skipped_in : 0;
    const int t_eff = step - skipped > 1 ? step - skipped : 1;
    __syncthreads();
    float norm = 0.0f, coef = 1.0f;
    if (partials) {
        norm_and_coef(staged, n_partials, max_norm, norm, coef);
        if (!(max_norm > 0.f)) coef = 1.0f;                // guard without a clip
    }
    // Inf or NaN (exponent all ones); tested on the bits, so no floating-point mode can fold it away
    const bool skip = skip_nonfinite != 0 && (__float_as_uint(norm) & 0x7f800000u) == 0x7f800000u;
    if (skipped > 0 && (int)threadIdx.x < n_groups) {
        float* h = hp[threadIdx.x];
        const double bc1 = 1.0 - pow_int((double)h[0], t_eff), bc2 = 1.0 - pow_int((double)h[1], t_eff);
        h[4] = (float)((double)h[6] / bc1); h[5] = (float)(1.0 / sqrt(bc2));
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (skipped_out) *skipped_out = skipped + (skip ? 1 : 0);
        if (status) {
            if (partials) { status[0] = norm; status[1] = coef; }
            status[2] = skip ? 1.0f : 0.0f; status[3] = (float)t_eff;
        }
    }
    if (skip) return;
    const bool scale = partials != nullptr && max_norm > 0.f, store_g = scale && write_clipped != 0;
    float one_minus_d = 1.f - ema_decay;
    if (ema && ema_warmup) {
        const float w = (float)(1 + t_eff) / (float)(10 + t_eff);
        one_minus_d = 1.f - (w < ema_decay ? w : ema_decay);
    }
    const size_t n4 = n >> 2;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const int grp = tile_group ? (tile_group[i >> 4] & (GGPM_ADAM_MAX_GROUPS - 1)) : 0;
        const float4 h0 = *reinterpret_cast<const float4*>(&hp[grp][0]);
        const float b1 = h0.x, b2 = h0.y, eps = h0.z, wd = h0.w, step_size = hp[grp][4], inv_bc2_sqrt = hp[grp][5];
        float4 pp = ggpm_ld4(p + 4 * i), gg = ggpm_ld4(g + 4 * i), mm = ggpm_ld4(m + 4 * i), vv = ggpm_ld4(v + 4 * i);
        float* P = &pp.x; float* G = &gg.x; float* M = &mm.x; float* V = &vv.x;
        if (scale) {
#pragma unroll
            for (int k = 0; k < 4; ++k) G[k] *= coef;
            if (store_g) ggpm_st4(g + 4 * i, gg);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float gr = wd != 0.f ? G[k] + wd * P[k] : G[k];
            M[k] = M[k] + (1.f - b1) * (gr - M[k]);
            V[k] = b2 * V[k] + (1.f - b2) * gr * gr;
            P[k] -= step_size * M[k] / (sqrtf(V[k]) * inv_bc2_sqrt + eps);
        }
        ggpm_st4(p + 4 * i, pp); ggpm_st4(m + 4 * i, mm); ggpm_st4(v + 4 * i, vv);
        if (ema) {
            float4 ee = ggpm_ld4(ema + 4 * i);
            float* E = &ee.x;
#pragma unroll
            for (int k = 0; k < 4; ++k) E[k] = E[k] + one_minus_d * (P[k] - E[k]);
            ggpm_st4(ema + 4 * i, ee);
        }
    }
}

// a <-> b in place, 16 B per lane, grid-stride
__global__ void __launch_bounds__(256) flat_swap_k(float* __restrict__ a, float* __restrict__ b, size_t n) {
    const size_t n4 = n >> 2;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const float4 x = ggpm_ld4(a + 4 * i), y = ggpm_ld4(b + 4 * i);
        ggpm_st4(a + 4 * i, y); ggpm_st4(b + 4 * i, x);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {          // tail of up to three elements
        const size_t i = (n4 << 2) + threadIdx.x;
        const float x = a[i], y = b[i];
        a[i] = y; b[i] = x;
    }
}
}  // namespace

extern "C" size_t ggpm_flat_sqnorm_workspace_bytes(size_t n) { return (size_t)norm_grid(n) * sizeof(double); }

extern "C" int ggpm_flat_sqnorm_partials(const float* x, size_t n, double* partials, size_t partials_bytes,
                                         ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!x || !partials || n == 0 || (((uintptr_t)x & 15) != 0) || (((uintptr_t)partials & 7) != 0)) return GGPM_ERR_ARG;
    const unsigned grid = norm_grid(n);
    if (partials_bytes < (size_t)grid * sizeof(double)) return GGPM_ERR_ARG;
    flat_sqnorm_partials_k<<<grid, NORM_THREADS, 0, (hipStream_t)stream>>>(x, n, partials);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_flat_norm_finish(const double* partials, int n_partials, float max_norm, float* out,
                                     ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!partials || !out || n_partials < 1 || n_partials > NORM_MAX_PARTIALS) return GGPM_ERR_ARG;
    if ((((uintptr_t)partials & 7) != 0) || (((uintptr_t)out & 3) != 0)) return GGPM_ERR_ARG;
    flat_norm_finish_k<<<1, NORM_MAX_PARTIALS, 0, (hipStream_t)stream>>>(partials, n_partials, max_norm, out);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_adam_step_groups(float* p, float* g, float* m, float* v, size_t n, const uint8_t* tile_group,
                                     int n_groups, const ggpm_adam_group* groups, int step, const double* partials,
                                     int n_partials, float max_norm, float* clip_out, int write_clipped,
                                     ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!p || !g || !m || !v || !groups || n == 0 || n % 64 != 0 || step < 1) return GGPM_ERR_ARG;
    if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) != 0) return GGPM_ERR_ARG;
    if (n_groups < 1 || n_groups > GGPM_ADAM_MAX_GROUPS || (!tile_group && n_groups > 1)) return GGPM_ERR_ARG;
    if (partials && (!(max_norm > 0.f) || n_partials < 1 || n_partials > NORM_MAX_PARTIALS || ((uintptr_t)partials & 7) != 0))
        return GGPM_ERR_ARG;
    if (((uintptr_t)clip_out & 3) != 0) return GGPM_ERR_ARG;
    AdamGroupsArgs args = {};
    for (int k = 0; k < n_groups; ++k) {
        const ggpm_adam_group& q = groups[k];
        const double bc1 = 1.0 - pow((double)q.beta1, step), bc2 = 1.0 - pow((double)q.beta2, step);
        float* h = args.hp[k];
        h[0] = q.beta1; h[1] = q.beta2; h[2] = q.eps; h[3] = q.weight_decay;
        h[4] = (float)((double)q.lr / bc1); h[5] = (float)(1.0 / sqrt(bc2));
    }
    size_t blocks = ((n >> 2) + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    adam_groups_k<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(p, g, m, v, n, tile_group, args, partials, n_partials,
                                                                   max_norm, clip_out, write_clipped);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_adam_step_ex(float* p, float* g, float* m, float* v, size_t n, const uint8_t* tile_group, int n_groups,
                                 const ggpm_adam_group* groups, int step, const double* partials, int n_partials,
                                 float max_norm, int write_clipped, float* ema, float ema_decay, int ema_warmup,
                                 int skip_nonfinite, const int* skipped_in, int* skipped_out, float* status,
                                 ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!p || !g || !m || !v || !groups || n == 0 || n % 64 != 0 || step < 1) return GGPM_ERR_ARG;
    if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) != 0) return GGPM_ERR_ARG;
    if (n_groups < 1 || n_groups > GGPM_ADAM_MAX_GROUPS || (!tile_group && n_groups > 1)) return GGPM_ERR_ARG;
    if (!(max_norm >= 0.f)) return GGPM_ERR_ARG;                                        // negative or NaN
    if (partials && (n_partials < 1 || n_partials > NORM_MAX_PARTIALS || ((uintptr_t)partials & 7) != 0)) return GGPM_ERR_ARG;
    if (!partials && (max_norm > 0.f || skip_nonfinite != 0)) return GGPM_ERR_ARG;      // a clip or the guard needs the norm
    if (ema && (!(ema_decay >= 0.f) || !(ema_decay < 1.f) || ema == p || ema == g || ema == m || ema == v)) return GGPM_ERR_ARG;
    if ((skipped_in == nullptr) != (skipped_out == nullptr) || (skipped_in && skipped_in == skipped_out)) return GGPM_ERR_ARG;
    if ((((uintptr_t)skipped_in | (uintptr_t)skipped_out | (uintptr_t)status) & 3) != 0) return GGPM_ERR_ARG;
    AdamExArgs args = {};
    for (int k = 0; k < n_groups; ++k) {
        const ggpm_adam_group& q = groups[k];
        const double bc1 = 1.0 - pow((double)q.beta1, step), bc2 = 1.0 - pow((double)q.beta2, step);
        float* h = args.hp[k];
        h[0] = q.beta1; h[1] = q.beta2; h[2] = q.eps; h[3] = q.weight_decay;
        h[4] = (float)((double)q.lr / bc1); h[5] = (float)(1.0 / sqrt(bc2)); h[6] = q.lr;
    }
    size_t blocks = ((n >> 2) + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    adam_ex_k<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(p, g, m, v, n, tile_group, n_groups, args, step, partials,
                                                               n_partials, max_norm, write_clipped, ema, ema_decay, ema_warmup,
                                                               skip_nonfinite, skipped_in, skipped_out, status);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_flat_swap(float* a, float* b, size_t n, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!a || !b || n == 0 || ((((uintptr_t)a | (uintptr_t)b) & 15) != 0)) return GGPM_ERR_ARG;
    if ((a <= b ? (size_t)(b - a) : (size_t)(a - b)) < n) return GGPM_ERR_ARG;          // the same buffer, or overlapping
    size_t blocks = ((n >> 2) + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    flat_swap_k<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(a, b, n);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_dropout(float* x, int rows, int cols, int ld, float p, unsigned int seed_lo, unsigned int seed_hi,
                            int site, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!x || rows <= 0 || cols <= 0 || ld < cols || p < 0.f || p >= 1.f) return GGPM_ERR_ARG;
    if (p == 0.f) return GGPM_OK;
    const unsigned int thresh = (unsigned int)((double)p * 16777216.0);
    dim3 grid(ggpm_ceil_div(cols, 256), rows);
    dropout_k<<<grid, 256, 0, (hipStream_t)stream>>>(x, rows, cols, ld, thresh, 1.0f / (1.0f - p), seed_lo, seed_hi,
                                                      (unsigned int)site);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}
