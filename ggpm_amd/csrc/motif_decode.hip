// Greedy decode of the tree-only decoder (MotifDecoder.decode, reference ggpm/decoder.py:901-1095): the device side.
//
// The decode-time tree (IncTree: node features, fmess, agraph, bgraph) and the message states h (and c for LSTM) stay
// resident for the whole decode; the host sends each phase's table edits and work lists in one upload.  Entry points:
//   ggpm_motif_decode_tree_step  two launches: (1) apply the uploaded edits to the tables, (2) one workgroup per work item:
//                                either the read-out of a current node (IncMPNEncoder.forward: E_c row, sum of the incoming
//                                hidden states over agraph, W_o with ReLU) or one new message (reset, input
//                                [E_c(source node) | onehot(pos)], `depth` sparse iterations of the GRU / LSTM over bgraph);
//   ggpm_motif_decode_mlp        two launches: Sequential(Linear, ReLU, Dropout(eval), Linear) on [vec | context of the
//                                molecule] (topoNN / clsNN / iclsNN), optionally with the sigmoid of the topology head;
//   ggpm_hier_topk               one launch: nnutils.hier_topk (or, root mode, the root's arg-max motif and its sorted
//                                masked attachments) with the owner mask read from the vocabulary's owner table;
//   ggpm_motif_decode_assm_score one launch: enum_attach + get_assm_score of every listed beam entry, written to
//                                each of its candidates.
// A new message never reads another message of the same launch (the host checks it): one workgroup per message needs no
// grid-wide barrier between the depth iterations.  Every reduction runs in a fixed order (wave butterflies, LDS trees):
// results are bitwise reproducible and do not depend on which other rows share the launch.  No atomics.
#include "common.h"

namespace {

constexpr int MD_THREADS = 256;
constexpr int MD_WAVES = MD_THREADS / GGPM_WAVE;
constexpr int MD_NB = 12;             // IncBase max_nb: agraph / bgraph slots
constexpr int MD_MAX_H = 1024;
constexpr int MD_MAX_K = 16;          // beam bound of hier_topk

__device__ __forceinline__ float wave_sum(float v) {
    for (int off = GGPM_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// sum_i w[i] * v[i] over one wave (lanes stride i); every lane returns the same value
__device__ __forceinline__ float wave_dot(const float* __restrict__ w, const float* v, int n, int lane) {
    float acc = 0.f;
    for (int i = lane; i < n; i += GGPM_WAVE) acc += w[i] * v[i];
    return wave_sum(acc);
}

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// ------------------------------------------------------------------ tree step
struct TreeStep {
    int rnn, H, P, depth;                 // P: onehot width (MAX_POS)
    const float* E_c; const float* Wo; const float* bo;
    const float* w[8];                    // GRU: W_z, b_z, W_r, U_r, b_ur, W_h, b_h; LSTM: W_i, b_i, W_o, b_o, W_f, b_f, W, b
    int32_t* fnode; int32_t* fmess; int32_t* agraph; int32_t* bgraph; int N, E;
    float* h; float* c;
    const int32_t* edits; int n_node_edits, n_tab_edits;
    const int32_t* nodes; int n_read; float* node_out; int ld_node;
    const int32_t* mess; int n_mess; float* mess_out; int ld_mess;
};

// node edits: (node, motif); table edits: (table 0 agraph / 1 bgraph / 2 fmess, row, slot, value).  Written in parallel:
// the host sends at most one edit per node and per slot (its last value).
__global__ void __launch_bounds__(MD_THREADS) md_apply_edits_k(TreeStep a) {
    for (int q = threadIdx.x; q < a.n_node_edits; q += MD_THREADS) {
        const int n = a.edits[2 * q], v = a.edits[2 * q + 1];
        if (n >= 0 && n < a.N) a.fnode[n] = v;
    }
    const int32_t* t = a.edits + 2 * a.n_node_edits;
    for (int q = threadIdx.x; q < a.n_tab_edits; q += MD_THREADS) {
        const int tab = t[4 * q], row = t[4 * q + 1], slot = t[4 * q + 2], v = t[4 * q + 3];
        if (tab == 0 && row >= 0 && row < a.N && slot >= 0 && slot < MD_NB) a.agraph[(size_t)row * MD_NB + slot] = v;
        else if (tab == 1 && row >= 0 && row < a.E && slot >= 0 && slot < MD_NB) a.bgraph[(size_t)row * MD_NB + slot] = v;
        else if (tab == 2 && row >= 0 && row < a.E && slot >= 0 && slot < 2) a.fmess[(size_t)row * 2 + slot] = v;
    }
}

__device__ void md_readout(const TreeStep& a, int r, float* lds) {
    const int H = a.H, t = threadIdx.x, lane = t % GGPM_WAVE, wv = t / GGPM_WAVE;
    float* x = lds;
    float* nei = lds + H;
    const int n = a.nodes[r];
    if (n < 0 || n >= a.N) return;
    const float* emb = a.E_c + (size_t)a.fnode[n] * H;
    const int32_t* ag = a.agraph + (size_t)n * MD_NB;
    for (int i = t; i < H; i += MD_THREADS) {
        x[i] = emb[i];
        float s = 0.f;
        for (int q = 0; q < MD_NB; ++q) {
            const int e = ag[q];
            if (e > 0 && e < a.E) s += a.h[(size_t)e * H + i];
        }
        nei[i] = s;
    }
    __syncthreads();
    for (int o = wv; o < H; o += MD_WAVES) {
        const float* w = a.Wo + (size_t)o * 2 * H;
        const float y = a.bo[o] + wave_dot(w, x, H, lane) + wave_dot(w + H, nei, H, lane);
        if (lane == 0) a.node_out[(size_t)r * a.ld_node + o] = fmaxf(y, 0.f);
    }
}

__device__ void md_message(const TreeStep& a, int r, float* lds) {
    __shared__ int ids[MD_NB];
    __shared__ int cnt_s;
    const int H = a.H, I = H + a.P, t = threadIdx.x, lane = t % GGPM_WAVE, wv = t / GGPM_WAVE;
    const int e = a.mess[2 * r], out_row = a.mess[2 * r + 1];
    if (e <= 0 || e >= a.E) return;
    const int src = a.fmess[(size_t)e * 2], pos = a.fmess[(size_t)e * 2 + 1];
    if (src < 0 || src >= a.N || pos < 0 || pos >= a.P) return;
    const bool lstm = a.rnn == 1;
    float* x = lds;                       // [H]   E_c row of the source node (the onehot part is one weight column)
    float* s = x + H;                     // [H]   sum of the neighbours' h
    float* g = s + H;                     // [H]   GRU: sum of the gated neighbours
    float* z = g + H;                     // [H]   GRU: update gate
    float* hn = z + H;                    // [12 H] neighbours' h
    float* cn = hn + MD_NB * H;           // [12 H] neighbours' c (LSTM)
    const float* emb = a.E_c + (size_t)a.fnode[src] * H;
    for (int i = t; i < H; i += MD_THREADS) {
        x[i] = emb[i];
        a.h[(size_t)e * H + i] = 0.f;     // sparse_forward resets the recomputed rows
        if (lstm) a.c[(size_t)e * H + i] = 0.f;
    }
    for (int it = 0; it < a.depth; ++it) {
        __syncthreads();
        if (t == 0) {
            int cnt = 0;
            for (int q = 0; q < MD_NB; ++q) {
                const int v = a.bgraph[(size_t)e * MD_NB + q];
                if (v > 0 && v < a.E) ids[cnt++] = v;
            }
            cnt_s = cnt;
        }
        __syncthreads();
        const int cnt = cnt_s;
        for (int j = 0; j < cnt; ++j)
            for (int i = t; i < H; i += MD_THREADS) {
                hn[j * H + i] = a.h[(size_t)ids[j] * H + i];
                if (lstm) cn[j * H + i] = a.c[(size_t)ids[j] * H + i];
            }
        __syncthreads();
        for (int i = t; i < H; i += MD_THREADS) {
            float acc = 0.f;
            for (int j = 0; j < cnt; ++j) acc += hn[j * H + i];
            s[i] = acc;
        }
        __syncthreads();
        const bool last = it == a.depth - 1;
        if (!lstm) {
            const float *Wz = a.w[0], *bz = a.w[1], *Wr = a.w[2], *Ur = a.w[3], *bur = a.w[4];
            for (int o = wv; o < H; o += MD_WAVES) {
                const float* wz = Wz + (size_t)o * (I + H);
                const float zz = sigm(bz[o] + wave_dot(wz, x, H, lane) + wz[H + pos] + wave_dot(wz + I, s, H, lane));
                const float* wr = Wr + (size_t)o * I;
                const float r1 = wave_dot(wr, x, H, lane) + wr[H + pos];
                float gs = 0.f;
                for (int j = 0; j < cnt; ++j) {
                    const float rj = sigm(r1 + (wave_dot(Ur + (size_t)o * H, hn + j * H, H, lane) + bur[o]));
                    gs += rj * hn[j * H + o];
                }
                if (lane == 0) { z[o] = zz; g[o] = gs; }
            }
            __syncthreads();
            const float *Wh = a.w[5], *bh = a.w[6];
            for (int o = wv; o < H; o += MD_WAVES) {
                const float* wh = Wh + (size_t)o * (I + H);
                const float pre = tanhf(bh[o] + wave_dot(wh, x, H, lane) + wh[H + pos] + wave_dot(wh + I, g, H, lane));
                const float nh = (1.f - z[o]) * s[o] + z[o] * pre;
                if (lane == 0) {
                    a.h[(size_t)e * H + o] = nh;
                    if (out_row >= 0 && last) a.mess_out[(size_t)out_row * a.ld_mess + o] = nh;
                }
            }
        } else {
            const float *Wi = a.w[0], *bi = a.w[1], *Wo = a.w[2], *bo = a.w[3], *Wf = a.w[4], *bf = a.w[5];
            const float *Wu = a.w[6], *bu = a.w[7];
            for (int o = wv; o < H; o += MD_WAVES) {
                const size_t ro = (size_t)o * (I + H);
                const float gi = sigm(bi[o] + wave_dot(Wi + ro, x, H, lane) + Wi[ro + H + pos] + wave_dot(Wi + ro + I, s, H, lane));
                const float go = sigm(bo[o] + wave_dot(Wo + ro, x, H, lane) + Wo[ro + H + pos] + wave_dot(Wo + ro + I, s, H, lane));
                const float gu = tanhf(bu[o] + wave_dot(Wu + ro, x, H, lane) + Wu[ro + H + pos] + wave_dot(Wu + ro + I, s, H, lane));
                const float fx = bf[o] + wave_dot(Wf + ro, x, H, lane) + Wf[ro + H + pos];
                float fc = 0.f;
                for (int j = 0; j < cnt; ++j) fc += sigm(fx + wave_dot(Wf + ro + I, hn + j * H, H, lane)) * cn[j * H + o];
                const float cc = gi * gu + fc;
                const float nh = go * tanhf(cc);
                if (lane == 0) {
                    a.h[(size_t)e * H + o] = nh;
                    a.c[(size_t)e * H + o] = cc;
                    if (out_row >= 0 && last) a.mess_out[(size_t)out_row * a.ld_mess + o] = nh;
                }
            }
        }
    }
}

__global__ void __launch_bounds__(MD_THREADS) md_tree_k(TreeStep a) {
    extern __shared__ float lds[];
    const int r = blockIdx.x;
    if (r < a.n_read) md_readout(a, r, lds);
    else if (r - a.n_read < a.n_mess) md_message(a, r - a.n_read, lds);
}

// ------------------------------------------------------------------ score heads
struct Mlp {
    const float* v; int ldv; const int32_t* bidx; const float* ctx; int ldc; int M, H, L;
    const float* W1; const float* b1; const float* W2; const float* b2; int n_out; int sigmoid;
    float* hid; int ldh; float* out; int ldo;
};

__global__ void __launch_bounds__(MD_THREADS) md_mlp_hidden_k(Mlp a) {
    extern __shared__ float lds[];
    const int r = blockIdx.x, t = threadIdx.x, lane = t % GGPM_WAVE, wv = t / GGPM_WAVE, H = a.H, L = a.L;
    if (r >= a.M) return;
    float* x = lds;
    float* cx = lds + H;
    const int b = a.bidx[r];
    for (int i = t; i < H; i += MD_THREADS) x[i] = a.v[(size_t)r * a.ldv + i];
    for (int i = t; i < L; i += MD_THREADS) cx[i] = a.ctx[(size_t)b * a.ldc + i];
    __syncthreads();
    for (int o = wv; o < H; o += MD_WAVES) {
        const float* w = a.W1 + (size_t)o * (H + L);
        const float y = a.b1[o] + wave_dot(w, x, H, lane) + wave_dot(w + H, cx, L, lane);
        if (lane == 0) a.hid[(size_t)r * a.ldh + o] = fmaxf(y, 0.f);
    }
}

// one wave per output column, every row
__global__ void __launch_bounds__(MD_THREADS) md_mlp_out_k(Mlp a) {
    const int t = threadIdx.x, lane = t % GGPM_WAVE;
    const int o = blockIdx.x * MD_WAVES + t / GGPM_WAVE;
    if (o >= a.n_out) return;
    const float* w = a.W2 + (size_t)o * a.H;
    for (int r = 0; r < a.M; ++r) {
        const float y = a.b2[o] + wave_dot(w, a.hid + (size_t)r * a.ldh, a.H, lane);
        if (lane == 0) a.out[(size_t)r * a.ldo + o] = a.sigmoid ? sigm(y) : y;
    }
}

// ------------------------------------------------------------------ hier_topk
struct TopK {
    const float* cls; int ldc, n_cls; const float* icls; int ldi, n_icls; const int32_t* owner; int M, k, root;
    int32_t* out;
};

// (value, index) order: larger value first, lower index on an exact tie
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) {
    return bi < 0 || v > bv || (v == bv && i < bi);
}

__device__ float block_max(float v, float* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = MD_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = fmaxf(red[t], red[t + s]);
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

__device__ float block_sum(float v, float* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = MD_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

__device__ void block_argbest(float v, int i, float* redv, int* redi, float* ov, int* oi) {
    const int t = threadIdx.x;
    redv[t] = v;
    redi[t] = i;
    __syncthreads();
    for (int s = MD_THREADS / 2; s > 0; s >>= 1) {
        if (t < s && redi[t + s] >= 0 && better(redv[t + s], redi[t + s], redv[t], redi[t])) {
            redv[t] = redv[t + s];
            redi[t] = redi[t + s];
        }
        __syncthreads();
    }
    *ov = redv[0];
    *oi = redi[0];
    __syncthreads();
}

// x[j] + vocab.get_mask(c)[j]: 0 on the attachments motif c owns, -1000 elsewhere
__device__ __forceinline__ float masked(const TopK& a, const float* row, int j, int c) {
    return row[j] + (a.owner[j] == c ? 0.f : -1000.f);
}

// the best k of f(j), j < n, in order, into (vals, idx) (shared)
template <typename F>
__device__ void block_topk(int n, int k, F f, float* redv, int* redi, float* vals, int* idx) {
    const int t = threadIdx.x;
    for (int q = 0; q < k; ++q) {
        float bv = 0.f;
        int bi = -1;
        for (int j = t; j < n; j += MD_THREADS) {
            bool taken = false;
            for (int p = 0; p < q; ++p) taken |= idx[p] == j;
            const float y = f(j);
            if (!taken && better(y, j, bv, bi)) { bv = y; bi = j; }
        }
        float yv;
        int yi;
        block_argbest(bv, bi, redv, redi, &yv, &yi);
        if (t == 0) { vals[q] = yv; idx[q] = yi; }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(MD_THREADS) md_topk_k(TopK a) {
    __shared__ float redv[MD_THREADS];
    __shared__ int redi[MD_THREADS];
    __shared__ float cls_s[MD_MAX_K], att_s[MD_MAX_K];
    __shared__ int cls_i[MD_MAX_K], att_i[MD_MAX_K];
    __shared__ float sum_s[MD_MAX_K * MD_MAX_K];
    __shared__ int sum_c[MD_MAX_K * MD_MAX_K], sum_a[MD_MAX_K * MD_MAX_K];
    const int r = blockIdx.x, t = threadIdx.x, k = a.k;
    const float* crow = a.cls + (size_t)r * a.ldc;
    const float* irow = a.icls + (size_t)r * a.ldi;
    int32_t* out = a.out + (size_t)r * 3 * k;
    if (a.root) {
        // root: arg-max motif of the raw scores, then its masked attachment scores sorted, first k
        block_topk(a.n_cls, 1, [&](int j) { return crow[j]; }, redv, redi, cls_s, cls_i);
        const int c = cls_i[0];
        block_topk(a.n_icls, k, [&](int j) { return masked(a, irow, j, c); }, redv, redi, att_s, att_i);
        if (t == 0)
            for (int q = 0; q < k; ++q) {
                out[q] = __float_as_int(att_s[q]);
                out[k + q] = c;
                out[2 * k + q] = att_i[q];
            }
        return;
    }
    // log_softmax over motifs and its top k
    float m = -INFINITY;
    for (int j = t; j < a.n_cls; j += MD_THREADS) m = fmaxf(m, crow[j]);
    m = block_max(m, redv);
    float se = 0.f;
    for (int j = t; j < a.n_cls; j += MD_THREADS) se += expf(crow[j] - m);
    const float lse = logf(block_sum(se, redv));
    block_topk(a.n_cls, k, [&](int j) { return (crow[j] - m) - lse; }, redv, redi, cls_s, cls_i);
    // per chosen motif: masked log_softmax over attachments, its top k, the k x k sums (flat index i * k + j)
    for (int q = 0; q < k; ++q) {
        const int c = cls_i[q];
        float mm = -INFINITY;
        for (int j = t; j < a.n_icls; j += MD_THREADS) mm = fmaxf(mm, masked(a, irow, j, c));
        mm = block_max(mm, redv);
        float s2 = 0.f;
        for (int j = t; j < a.n_icls; j += MD_THREADS) s2 += expf(masked(a, irow, j, c) - mm);
        const float lse2 = logf(block_sum(s2, redv));
        block_topk(a.n_icls, k, [&](int j) { return (masked(a, irow, j, c) - mm) - lse2; }, redv, redi, att_s, att_i);
        if (t == 0)
            for (int p = 0; p < k; ++p) {
                sum_s[q * k + p] = cls_s[q] + att_s[p];
                sum_c[q * k + p] = c;
                sum_a[q * k + p] = att_i[p];
            }
        __syncthreads();
    }
    if (t == 0) {
        int used[MD_MAX_K];
        for (int q = 0; q < k; ++q) {
            int bi = -1;
            float bv = 0.f;
            for (int f = 0; f < k * k; ++f) {
                bool taken = false;
                for (int p = 0; p < q; ++p) taken |= used[p] == f;
                if (!taken && better(sum_s[f], f, bv, bi)) { bv = sum_s[f]; bi = f; }
            }
            used[q] = bi;
            out[q] = __float_as_int(bv);
            out[k + q] = sum_c[bi];
            out[2 * k + q] = sum_a[bi];
        }
    }
}

// ------------------------------------------------------------------ attachment scores
struct Assm {
    const float* E; int H, L, P, n_ids; const int32_t* meta; const int32_t* ids;
    const float* W1; int ldw; const float* b1; const float* Wa; const float* ba; const float* z; int ldz; float* score;
};

// one workgroup per prediction (meta row: n candidates, k ids, nth_child, molecule, first candidate, first id):
// v = sum_{j<k} relu(matchNN [E_assm[id_j] | onehot(nth)]), score = (W_assm v + b) . z_b.  enum_attach never reads the
// candidate's atoms (reference decoder.py:617), so every candidate of a prediction has this score: it is computed once
// and written to all n.  A meta row out of range (k not 1 or 2, nth past the onehot, an id past E_assm) scores NaN.
__global__ void __launch_bounds__(MD_THREADS) md_assm_k(Assm a) {
    extern __shared__ float lds[];
    __shared__ float red[MD_THREADS];
    const int p = blockIdx.x, t = threadIdx.x, lane = t % GGPM_WAVE, wv = t / GGPM_WAVE, H = a.H, L = a.L;
    const int32_t* m = a.meta + (size_t)p * 6;
    const int n = m[0], k = m[1], nth = m[2], b = m[3], coff = m[4], roff = m[5];
    bool ok = k >= 1 && k <= 2 && nth >= 0 && nth < a.ldw - H;
    for (int j = 0; ok && j < k; ++j) ok = a.ids[roff + j] >= 0 && a.ids[roff + j] < a.n_ids;
    if (!ok) {
        for (int c = t; c < n; c += MD_THREADS) a.score[coff + c] = __int_as_float(0x7fc00000);
        return;
    }
    float* e = lds;                 // [2 H]
    float* v = lds + 2 * H;         // [H]
    float* proj = v + H;            // [L]
    const float* zb = a.z + (size_t)b * a.ldz;
    for (int j = 0; j < k; ++j) {
        const float* row = a.E + (size_t)a.ids[roff + j] * H;
        for (int i = t; i < H; i += MD_THREADS) e[j * H + i] = row[i];
    }
    __syncthreads();
    for (int o = wv; o < H; o += MD_WAVES) {
        const float* w = a.W1 + (size_t)o * a.ldw;
        float acc = 0.f;
        for (int j = 0; j < k; ++j) acc += fmaxf(a.b1[o] + wave_dot(w, e + j * H, H, lane) + w[H + nth], 0.f);
        if (lane == 0) v[o] = acc;
    }
    __syncthreads();
    for (int l = wv; l < L; l += MD_WAVES) {
        const float y = a.ba[l] + wave_dot(a.Wa + (size_t)l * H, v, H, lane);
        if (lane == 0) proj[l] = y * zb[l];
    }
    __syncthreads();
    float d = 0.f;
    for (int l = t; l < L; l += MD_THREADS) d += proj[l];
    d = block_sum(d, red);
    for (int c = t; c < n; c += MD_THREADS) a.score[coff + c] = d;
}

}  // namespace

extern "C" int ggpm_motif_decode_tree_step(int rnn_type, int H, int max_pos, int depth, const void* const* params,
                                           int32_t* fnode, int32_t* fmess, int32_t* agraph, int32_t* bgraph, int N, int E,
                                           float* h, float* c, const int32_t* edits, int n_node_edits, int n_tab_edits,
                                           const int32_t* nodes, int n_read, float* node_out, int ld_node,
                                           const int32_t* mess, int n_mess, float* mess_out, int ld_mess,
                                           ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    const int n_w = rnn_type == 0 ? 7 : 8;
    if ((rnn_type != 0 && rnn_type != 1) || H <= 0 || H > MD_MAX_H || max_pos <= 0 || depth < 1 || !params || !fnode ||
        !fmess || !agraph || !bgraph || N <= 0 || E <= 0 || !h || (rnn_type == 1 && !c) || n_node_edits < 0 ||
        n_tab_edits < 0 || n_read < 0 || n_mess < 0 || (n_node_edits + n_tab_edits > 0 && !edits) ||
        (n_read > 0 && (!nodes || !node_out || ld_node < H)) || (n_mess > 0 && (!mess || !mess_out || ld_mess < H)) ||
        (n_read > 0 && n_mess > 0))       // a read-out reads the messages of an earlier launch
        return GGPM_ERR_ARG;
    for (int i = 0; i < 3 + n_w; ++i)
        if (!params[i]) return GGPM_ERR_ARG;
    TreeStep a{};
    a.rnn = rnn_type; a.H = H; a.P = max_pos; a.depth = depth;
    a.E_c = (const float*)params[0]; a.Wo = (const float*)params[1]; a.bo = (const float*)params[2];
    for (int i = 0; i < n_w; ++i) a.w[i] = (const float*)params[3 + i];
    a.fnode = fnode; a.fmess = fmess; a.agraph = agraph; a.bgraph = bgraph; a.N = N; a.E = E; a.h = h; a.c = c;
    a.edits = edits; a.n_node_edits = n_node_edits; a.n_tab_edits = n_tab_edits;
    a.nodes = nodes; a.n_read = n_read; a.node_out = node_out; a.ld_node = ld_node;
    a.mess = mess; a.n_mess = n_mess; a.mess_out = mess_out; a.ld_mess = ld_mess;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(md_apply_edits_k, dim3(1), dim3(MD_THREADS), 0, s, a);
    const size_t lds = (size_t)(4 + 2 * MD_NB) * H * sizeof(float);
    ggpm_set_lds_addr((const void*)md_tree_k, lds);
    hipLaunchKernelGGL(md_tree_k, dim3(n_read + n_mess > 0 ? n_read + n_mess : 1), dim3(MD_THREADS), lds, s, a);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_motif_decode_mlp(const float* vecs, int ld_v, const int32_t* bidx, const float* ctx, int ld_ctx, int M,
                                     int H, int L, const float* W1, const float* b1, const float* W2, const float* b2,
                                     int n_out, int sigmoid, float* hid, int ld_hid, float* out, int ld_out,
                                     ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (M <= 0 || H <= 0 || H > MD_MAX_H || L <= 0 || L > MD_MAX_H || n_out <= 0 || ld_v < H || ld_ctx < L ||
        ld_hid < H || ld_out < n_out || !vecs || !bidx || !ctx || !W1 || !b1 || !W2 || !b2 || !hid || !out)
        return GGPM_ERR_ARG;
    Mlp a{vecs, ld_v, bidx, ctx, ld_ctx, M, H, L, W1, b1, W2, b2, n_out, sigmoid, hid, ld_hid, out, ld_out};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(md_mlp_hidden_k, dim3(M), dim3(MD_THREADS), (size_t)(H + L) * sizeof(float), s, a);
    hipLaunchKernelGGL(md_mlp_out_k, dim3((n_out + MD_WAVES - 1) / MD_WAVES), dim3(MD_THREADS), 0, s, a);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_hier_topk(const float* cls, int ld_cls, int n_cls, const float* icls, int ld_icls, int n_icls,
                              const int32_t* owner, int M, int k, int root, int32_t* out, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (M <= 0 || k <= 0 || k > MD_MAX_K || n_icls < k || (!root && n_cls < k) || n_cls <= 0 || ld_cls < n_cls ||
        ld_icls < n_icls || !cls || !icls || !owner || !out)
        return GGPM_ERR_ARG;
    TopK a{cls, ld_cls, n_cls, icls, ld_icls, n_icls, owner, M, k, root, out};
    hipLaunchKernelGGL(md_topk_k, dim3(M), dim3(MD_THREADS), 0, (hipStream_t)stream, a);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_motif_decode_assm_score(const float* E_assm, int n_ids, int H, int L, const int32_t* meta,
                                            const int32_t* ids, int P, const float* W1, int ldw, const float* b1,
                                            const float* Wa, const float* ba, const float* z, int ldz, float* score,
                                            ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (P <= 0 || n_ids <= 0 || H <= 0 || H > MD_MAX_H || L <= 0 || L > MD_MAX_H || ldw < H + 1 || ldz < L || !E_assm ||
        !meta || !ids || !W1 || !b1 || !Wa || !ba || !z || !score)
        return GGPM_ERR_ARG;
    Assm a{E_assm, H, L, P, n_ids, meta, ids, W1, ldw, b1, Wa, ba, z, ldz, score};
    hipLaunchKernelGGL(md_assm_k, dim3(P), dim3(MD_THREADS), (size_t)(3 * H + L) * sizeof(float), (hipStream_t)stream, a);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}
