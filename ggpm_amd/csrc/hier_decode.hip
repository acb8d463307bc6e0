// Greedy decode of the hierarchical decoder (HierMPNDecoder.decode, reference ggpm/decoder.py:303-472): the device side.
//
// Resident for the whole decode (the `state` pointer array, HD_S_*): the decode-time tree's tables (node features with two
// columns, fmess, agraph, bgraph, cgraph; the tree and the inter level share them), the atom tables of the graph batch (fnode,
// fmess, agraph, bgraph), the message states of the three levels (h, and c for LSTM; the atom level's twice), the atom
// read-out rows (hgraph.node) with the step that wrote each, and the node inputs of the current call.  Entry points:
//   ggpm_hier_decode_atom_step   2 + diterG launches: (1) apply the uploaded edits to the tree and atom tables and reset the
//                                listed messages; (2) one launch per Jacobi iteration of the GRU / LSTM over the listed
//                                cluster messages, one workgroup per message; (3) the read-out W_o([fnode | sum over agraph
//                                of h]) of the listed cluster atoms, stamped with the step.
//   ggpm_hier_decode_tree_step   without new messages 1 launch: per current node the inter input W_i([E_i | sum over cgraph
//                                of the atom read-outs]), the inter read-out, the tree input W_c([E_c | inter read-out]) and
//                                the tree read-out.  With new messages 5 launches: edits; inter inputs; inter messages;
//                                inter read-outs and tree inputs; tree messages.
//   ggpm_hier_decode_assm_score  1 launch: enum_attach + get_assm_score, one workgroup per candidate.
// The atom level is a Jacobi iteration: the messages of a cluster read each other, and every row of iteration i + 1 reads
// iteration i's values (rnn.py:52-59).  Iteration i reads state buffer i % 2 and writes the listed rows of the other one; the
// read-out launch copies the final rows back, so both buffers agree between calls.  The rows are spread over workgroups, one
// launch per iteration: a cluster's 2 to 60 messages then stream the gate weights through up to 60 compute units at once (out
// of L2 after the first) instead of one workgroup walking them row after row.  On the tree and inter levels a step adds one
// message per molecule and none reads another (the host checks it), so their iterations run inside one launch.
// Every index that comes from an upload or a table is range-checked before it is used as an address.  Every reduction runs in
// a fixed order (wave butterflies, LDS trees); no atomics: results are bitwise reproducible and a row does not depend on which
// other rows share the launch.
#include "common.h"

namespace {

constexpr int HD_THREADS = 256;
constexpr int HD_WAVES = HD_THREADS / GGPM_WAVE;
constexpr int HD_TNB = 12;            // IncTree max_nb
constexpr int HD_ANB = 10;            // IncGraph max_nb
constexpr int HD_CG = 30;             // IncTree max_sub_nodes
constexpr int HD_MAX_H = 1024;
constexpr int HD_EDIT_BLOCKS = 64;

enum { HD_D_RNN, HD_D_H, HD_D_P, HD_D_N, HD_D_E, HD_D_NA, HD_D_EA, HD_D_AF, HD_D_EF, HD_D_DT, HD_D_DG, HD_D_NCLS, HD_D_NICLS,
       HD_D_B, HD_D_COUNT };
enum { HD_S_TFNODE, HD_S_TFMESS, HD_S_TAGRAPH, HD_S_TBGRAPH, HD_S_TCGRAPH, HD_S_AFNODE, HD_S_AFMESS, HD_S_AAGRAPH,
       HD_S_ABGRAPH, HD_S_GH0, HD_S_GH1, HD_S_GC0, HD_S_GC1, HD_S_ANODE, HD_S_ASTAMP, HD_S_IH, HD_S_IC, HD_S_TH, HD_S_TC,
       HD_S_XI, HD_S_XC, HD_S_COUNT };
// params: three cells of 8 slots (GRU: W_z, b_z, W_r, U_r, b_Ur, W_h, b_h, unused; LSTM: W_i, b_i, W_o, b_o, W_f, b_f, W, b) --
// atom, inter, tree -- then the read-outs and the node inputs
enum { HD_P_CELL_G = 0, HD_P_CELL_I = 8, HD_P_CELL_T = 16, HD_P_WOG = 24, HD_P_BOG, HD_P_WOI, HD_P_BOI, HD_P_WOT, HD_P_BOT,
       HD_P_EI, HD_P_EC, HD_P_WI, HD_P_BI, HD_P_WC, HD_P_BC, HD_P_COUNT };

struct Cell { int rnn, H, I; const float* w[8]; };

struct Dec {
    int rnn, H, P, N, E, NA, EA, AF, EF, dT, dG, n_cls, n_icls, B;
    int32_t *t_fnode, *t_fmess, *t_agraph, *t_bgraph, *t_cgraph;
    float *a_fnode, *a_fmess; int32_t *a_agraph, *a_bgraph;
    float *gh[2], *gc[2], *anode; int32_t* astamp;
    float *ih, *ic, *th, *tc, *xi, *xc;
    Cell cg, ci, ct;
    const float *Wog, *bog, *Woi, *boi, *Wot, *bot, *Ei, *Ec, *Wi, *bi, *Wc, *bc;
    // one call's work
    const int32_t* tedits; int n_tedits;
    const int32_t *fn_rows, *fn_data, *fm_rows, *fm_data, *ag_rows, *ag_data, *bg_rows, *bg_data; int n_fn, n_fm, n_ag, n_bg;
    const int32_t* edges; int n_edges; const int32_t* atoms; int n_atoms;
    const int32_t* nodes; int n_nodes; const int32_t* mess; int n_mess;
    int stamp; float* node_out; int ld_node; float* mess_out; int ld_mess;
};

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

__device__ float block_sum(float v, float* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = HD_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// One row of GRU.GRU / LSTM.LSTM (rnn.py:25-39, 85-94): x [I] and the cnt neighbours' hn (cn) [cnt x H] are in LDS and
// visible; the new row goes to oh (oc) [H] in LDS, visible on return.  s, g, z: [H] scratch.
__device__ void hd_cell(const Cell& k, const float* x, const float* hn, const float* cn, int cnt, float* s, float* g, float* z,
                        float* oh, float* oc) {
    const int H = k.H, I = k.I, t = threadIdx.x, lane = t % GGPM_WAVE, wv = t / GGPM_WAVE;
    for (int i = t; i < H; i += HD_THREADS) {
        float acc = 0.f;
        for (int j = 0; j < cnt; ++j) acc += hn[j * H + i];
        s[i] = acc;
    }
    __syncthreads();
    if (k.rnn == 0) {
        const float *Wz = k.w[0], *bz = k.w[1], *Wr = k.w[2], *Ur = k.w[3], *bur = k.w[4], *Wh = k.w[5], *bh = k.w[6];
        for (int o = wv; o < H; o += HD_WAVES) {
            const float* wz = Wz + (size_t)o * (I + H);
            const float zz = sigm(bz[o] + wave_dot(wz, x, I, lane) + wave_dot(wz + I, s, H, lane));
            const float r1 = wave_dot(Wr + (size_t)o * I, x, I, lane);
            float gs = 0.f;
            for (int j = 0; j < cnt; ++j) {
                const float rj = sigm(r1 + (wave_dot(Ur + (size_t)o * H, hn + j * H, H, lane) + bur[o]));
                gs += rj * hn[j * H + o];
            }
            if (lane == 0) { z[o] = zz; g[o] = gs; }
        }
        __syncthreads();
        for (int o = wv; o < H; o += HD_WAVES) {
            const float* wh = Wh + (size_t)o * (I + H);
            const float pre = tanhf(bh[o] + wave_dot(wh, x, I, lane) + wave_dot(wh + I, g, H, lane));
            if (lane == 0) oh[o] = (1.f - z[o]) * s[o] + z[o] * pre;
        }
    } else {
        const float *Wi = k.w[0], *bi = k.w[1], *Wo = k.w[2], *bo = k.w[3], *Wf = k.w[4], *bf = k.w[5], *Wu = k.w[6], *bu = k.w[7];
        for (int o = wv; o < H; o += HD_WAVES) {
            const size_t ro = (size_t)o * (I + H);
            const float gi = sigm(bi[o] + wave_dot(Wi + ro, x, I, lane) + wave_dot(Wi + ro + I, s, H, lane));
            const float go = sigm(bo[o] + wave_dot(Wo + ro, x, I, lane) + wave_dot(Wo + ro + I, s, H, lane));
            const float gu = tanhf(bu[o] + wave_dot(Wu + ro, x, I, lane) + wave_dot(Wu + ro + I, s, H, lane));
            const float fx = bf[o] + wave_dot(Wf + ro, x, I, lane);
            float fc = 0.f;
            for (int j = 0; j < cnt; ++j) fc += sigm(fx + wave_dot(Wf + ro + I, hn + j * H, H, lane)) * cn[j * H + o];
            const float cc = gi * gu + fc;
            if (lane == 0) { oh[o] = go * tanhf(cc); oc[o] = cc; }
        }
    }
    __syncthreads();
}

// the LDS of a kernel that runs hd_cell: x [xw] | s g z oh oc [5 H] | hn [12 H] | cn [12 H]
struct CellLds { float *x, *s, *g, *z, *oh, *oc, *hn, *cn; };
__device__ __forceinline__ CellLds cell_lds(float* lds, int xw, int H) {
    CellLds m;
    m.x = lds; m.s = lds + xw; m.g = m.s + H; m.z = m.g + H; m.oh = m.z + H; m.oc = m.oh + H; m.hn = m.oc + H;
    m.cn = m.hn + HD_TNB * H;
    return m;
}
__host__ __device__ inline int hd_xw(int H, int P, int EF) { const int a = H + P; return ((a > EF ? a : EF) + 3) / 4 * 4; }

// the live neighbours of a row (ids in (0, limit)) into ids[], in slot order
__device__ int hd_neighbours(const int32_t* row, int nb, int limit, int* ids, int* cnt_s) {
    __syncthreads();
    if (threadIdx.x == 0) {
        int cnt = 0;
        for (int q = 0; q < nb; ++q) {
            const int v = row[q];
            if (v > 0 && v < limit) ids[cnt++] = v;
        }
        *cnt_s = cnt;
    }
    __syncthreads();
    return *cnt_s;
}

// ------------------------------------------------------------------ edits and reset
// Tree edits: quads (table 0 agraph / 1 bgraph / 2 fmess (source, position) / 3 fnode (motif, attachment) / 4 cgraph, row,
// slot, value).  Atom edits: whole rows (row ids, then the rows).  The host sends at most one edit per slot and per row, so
// they are written in parallel.  Then the listed messages' rows of atom state buffer 0 are zeroed (sparse_forward's reset).
__global__ void __launch_bounds__(HD_THREADS) hd_edit_k(Dec a) {
    const int stride = gridDim.x * HD_THREADS, t0 = blockIdx.x * HD_THREADS + threadIdx.x;
    for (int q = t0; q < a.n_tedits; q += stride) {
        const int tab = a.tedits[4 * q], row = a.tedits[4 * q + 1], slot = a.tedits[4 * q + 2], v = a.tedits[4 * q + 3];
        if (row < 0 || slot < 0) continue;
        if (tab == 0 && row < a.N && slot < HD_TNB) a.t_agraph[(size_t)row * HD_TNB + slot] = v;
        else if (tab == 1 && row < a.E && slot < HD_TNB) a.t_bgraph[(size_t)row * HD_TNB + slot] = v;
        else if (tab == 2 && row < a.E && slot < 2) a.t_fmess[(size_t)row * 2 + slot] = v;
        else if (tab == 3 && row < a.N && slot < 2) a.t_fnode[(size_t)row * 2 + slot] = v;
        else if (tab == 4 && row < a.N && slot < HD_CG) a.t_cgraph[(size_t)row * HD_CG + slot] = v;
    }
    for (int q = t0; q < a.n_fn * a.AF; q += stride) {
        const int row = a.fn_rows[q / a.AF];
        if (row >= 0 && row < a.NA) a.a_fnode[(size_t)row * a.AF + q % a.AF] = __int_as_float(a.fn_data[q]);
    }
    for (int q = t0; q < a.n_fm * a.EF; q += stride) {
        const int row = a.fm_rows[q / a.EF];
        if (row >= 0 && row < a.EA) a.a_fmess[(size_t)row * a.EF + q % a.EF] = __int_as_float(a.fm_data[q]);
    }
    for (int q = t0; q < a.n_ag * HD_ANB; q += stride) {
        const int row = a.ag_rows[q / HD_ANB];
        if (row >= 0 && row < a.EA) a.a_agraph[(size_t)row * HD_ANB + q % HD_ANB] = a.ag_data[q];
    }
    for (int q = t0; q < a.n_bg * HD_ANB; q += stride) {
        const int row = a.bg_rows[q / HD_ANB];
        if (row >= 0 && row < a.EA) a.a_bgraph[(size_t)row * HD_ANB + q % HD_ANB] = a.bg_data[q];
    }
    for (int q = t0; q < a.n_edges * a.H; q += stride) {
        const int e = a.edges[q / a.H];
        if (e > 0 && e < a.EA) {
            a.gh[0][(size_t)e * a.H + q % a.H] = 0.f;
            if (a.rnn == 1) a.gc[0][(size_t)e * a.H + q % a.H] = 0.f;
        }
    }
}

// ------------------------------------------------------------------ atom level
// one Jacobi iteration: workgroup r updates message edges[r] from buffer it % 2 into buffer (it + 1) % 2
__global__ void __launch_bounds__(HD_THREADS) hd_atom_iter_k(Dec a, int it) {
    extern __shared__ float lds[];
    __shared__ int ids[HD_TNB];
    __shared__ int cnt_s;
    const int r = blockIdx.x, t = threadIdx.x, H = a.H;
    if (r >= a.n_edges) return;
    const int e = a.edges[r];
    if (e <= 0 || e >= a.EA) return;
    const CellLds m = cell_lds(lds, hd_xw(H, a.P, a.EF), H);
    const float* hs = a.gh[it % 2];
    const float* cs = a.gc[it % 2];
    const bool lstm = a.rnn == 1;
    for (int i = t; i < a.EF; i += HD_THREADS) m.x[i] = a.a_fmess[(size_t)e * a.EF + i];
    const int cnt = hd_neighbours(a.a_bgraph + (size_t)e * HD_ANB, HD_ANB, a.EA, ids, &cnt_s);
    for (int j = 0; j < cnt; ++j)
        for (int i = t; i < H; i += HD_THREADS) {
            m.hn[j * H + i] = hs[(size_t)ids[j] * H + i];
            if (lstm) m.cn[j * H + i] = cs[(size_t)ids[j] * H + i];
        }
    __syncthreads();
    hd_cell(a.cg, m.x, m.hn, m.cn, cnt, m.s, m.g, m.z, m.oh, m.oc);
    float* hd = a.gh[(it + 1) % 2];
    for (int i = t; i < H; i += HD_THREADS) {
        hd[(size_t)e * H + i] = m.oh[i];
        if (lstm) a.gc[(it + 1) % 2][(size_t)e * H + i] = m.oc[i];
    }
}

// workgroups [0, n_atoms): the read-out of atom atoms[r] from the final buffer, stamped; workgroups [n_atoms, n_atoms +
// n_edges): the final row of a listed message copied to the other buffer
__global__ void __launch_bounds__(HD_THREADS) hd_atom_read_k(Dec a) {
    extern __shared__ float lds[];
    const int r = blockIdx.x, t = threadIdx.x, lane = t % GGPM_WAVE, wv = t / GGPM_WAVE, H = a.H;
    const int fin = a.dG % 2;
    if (r >= a.n_atoms) {
        if (r - a.n_atoms >= a.n_edges) return;
        const int e = a.edges[r - a.n_atoms];
        if (e <= 0 || e >= a.EA) return;
        for (int i = t; i < H; i += HD_THREADS) {
            a.gh[1 - fin][(size_t)e * H + i] = a.gh[fin][(size_t)e * H + i];
            if (a.rnn == 1) a.gc[1 - fin][(size_t)e * H + i] = a.gc[fin][(size_t)e * H + i];
        }
        return;
    }
    const int v = a.atoms[r];
    if (v < 0 || v >= a.NA) return;
    float* x = lds;                           // [AF]
    float* nei = lds + (a.AF + 3) / 4 * 4;    // [H]
    const int32_t* ag = a.a_agraph + (size_t)v * HD_ANB;
    const float* hs = a.gh[fin];
    for (int i = t; i < a.AF; i += HD_THREADS) x[i] = a.a_fnode[(size_t)v * a.AF + i];
    for (int i = t; i < H; i += HD_THREADS) {
        float s = 0.f;
        for (int q = 0; q < HD_ANB; ++q) {
            const int e = ag[q];
            if (e > 0 && e < a.EA) s += hs[(size_t)e * H + i];
        }
        nei[i] = s;
    }
    __syncthreads();
    for (int o = wv; o < H; o += HD_WAVES) {
        const float* w = a.Wog + (size_t)o * (a.AF + H);
        const float y = a.bog[o] + wave_dot(w, x, a.AF, lane) + wave_dot(w + a.AF, nei, H, lane);
        if (lane == 0) a.anode[(size_t)v * H + o] = fmaxf(y, 0.f);
    }
    if (t == 0) a.astamp[v] = a.stamp;
}

// ------------------------------------------------------------------ inter and tree levels: nodes
// out[o] = relu(b[o] + W[o] . [u | v]) for o < H, W [H x 2H]; out in LDS, visible on return
__device__ void hd_lin2(const float* W, const float* b, const float* u, const float* v, int H, float* out) {
    const int t = threadIdx.x, lane = t % GGPM_WAVE, wv = t / GGPM_WAVE;
    for (int o = wv; o < H; o += HD_WAVES) {
        const float* w = W + (size_t)o * 2 * H;
        const float y = b[o] + wave_dot(w, u, H, lane) + wave_dot(w + H, v, H, lane);
        if (lane == 0) out[o] = fmaxf(y, 0.f);
    }
    __syncthreads();
}

// sum over the live slots of an agraph row of a level's hidden states -> out [H] (LDS), visible on return
__device__ void hd_incoming(const Dec& a, const float* h, int n, float* out) {
    const int32_t* ag = a.t_agraph + (size_t)n * HD_TNB;
    for (int i = threadIdx.x; i < a.H; i += HD_THREADS) {
        float s = 0.f;
        for (int q = 0; q < HD_TNB; ++q) {
            const int e = ag[q];
            if (e > 0 && e < a.E) s += h[(size_t)e * a.H + i];
        }
        out[i] = s;
    }
    __syncthreads();
}

constexpr int HD_ST_XI = 1, HD_ST_RI = 2, HD_ST_XC = 4, HD_ST_RC = 8;

// workgroup r, node nodes[r]: the stages asked for, in order -- inter input (to xi row r), inter read-out, tree input (to
// xc row r), tree read-out (to node_out row r).  A stage that is not run reads its input from the row an earlier launch
// wrote.  A node whose motif or attachment id is out of range is skipped.
__global__ void __launch_bounds__(HD_THREADS) hd_nodes_k(Dec a, int stages) {
    extern __shared__ float lds[];
    const int r = blockIdx.x, t = threadIdx.x, H = a.H;
    if (r >= a.n_nodes) return;
    const int n = a.nodes[r];
    if (n < 0 || n >= a.N) return;
    const int f0 = a.t_fnode[(size_t)n * 2], f1 = a.t_fnode[(size_t)n * 2 + 1];
    if (f0 < 0 || f0 >= a.n_cls || f1 < 0 || f1 >= a.n_icls) return;
    float* u = lds;             // [H] embedding row
    float* v = u + H;           // [H] pooled rows
    float* xi = v + H;
    float* ri = xi + H;
    float* xc = ri + H;
    float* rc = xc + H;
    if (stages & HD_ST_XI) {
        const int32_t* cg = a.t_cgraph + (size_t)n * HD_CG;
        for (int i = t; i < H; i += HD_THREADS) {
            u[i] = a.Ei[(size_t)f1 * H + i];
            float s = 0.f;
            for (int q = 0; q < HD_CG; ++q) {
                const int at = cg[q];
                if (at >= 0 && at < a.NA && a.astamp[at] == a.stamp) s += a.anode[(size_t)at * H + i];
            }
            v[i] = s;
        }
        __syncthreads();
        hd_lin2(a.Wi, a.bi, u, v, H, xi);
        for (int i = t; i < H; i += HD_THREADS) a.xi[(size_t)r * H + i] = xi[i];
    } else if (stages & HD_ST_RI) {
        for (int i = t; i < H; i += HD_THREADS) xi[i] = a.xi[(size_t)r * H + i];
        __syncthreads();
    }
    if (stages & HD_ST_RI) {
        hd_incoming(a, a.ih, n, v);
        hd_lin2(a.Woi, a.boi, xi, v, H, ri);
    }
    if (stages & HD_ST_XC) {
        for (int i = t; i < H; i += HD_THREADS) u[i] = a.Ec[(size_t)f0 * H + i];
        __syncthreads();
        hd_lin2(a.Wc, a.bc, u, ri, H, xc);
        for (int i = t; i < H; i += HD_THREADS) a.xc[(size_t)r * H + i] = xc[i];
    }
    if (stages & HD_ST_RC) {
        hd_incoming(a, a.th, n, v);
        hd_lin2(a.Wot, a.bot, xc, v, H, rc);
        for (int i = t; i < H; i += HD_THREADS) a.node_out[(size_t)r * a.ld_node + i] = rc[i];
    }
}

// ------------------------------------------------------------------ inter and tree levels: messages
// workgroup r, message mess[2r]: reset, input [node input of its source node (zero when the source is not among the call's
// nodes) | onehot(position)], `depth` sparse iterations over bgraph.  tree != 0: the tree level (state th / tc, inputs xc, the
// hidden row copied to mess_out row mess[2r + 1] when that is a row of it); else the inter level (ih / ic, xi).
__global__ void __launch_bounds__(HD_THREADS) hd_mess_k(Dec a, int tree) {
    extern __shared__ float lds[];
    __shared__ int ids[HD_TNB];
    __shared__ int cnt_s, found_s;
    const int r = blockIdx.x, t = threadIdx.x, H = a.H;
    if (r >= a.n_mess) return;
    const int e = a.mess[2 * r], out_row = a.mess[2 * r + 1];
    if (e <= 0 || e >= a.E) return;
    const int src = a.t_fmess[(size_t)e * 2], pos = a.t_fmess[(size_t)e * 2 + 1];
    if (src < 0 || src >= a.N || pos < 0 || pos >= a.P) return;
    const CellLds m = cell_lds(lds, hd_xw(H, a.P, a.EF), H);
    float* h = tree ? a.th : a.ih;
    float* c = tree ? a.tc : a.ic;
    const float* xin = tree ? a.xc : a.xi;
    const Cell& cell = tree ? a.ct : a.ci;
    const bool lstm = a.rnn == 1;
    if (t == 0) {
        int f = -1;
        for (int i = 0; i < a.n_nodes && f < 0; ++i)
            if (a.nodes[i] == src) f = i;
        found_s = f;
    }
    __syncthreads();
    const int found = found_s;
    for (int i = t; i < H; i += HD_THREADS) {
        m.x[i] = found >= 0 ? xin[(size_t)found * H + i] : 0.f;
        h[(size_t)e * H + i] = 0.f;           // sparse_forward resets the recomputed rows
        if (lstm) c[(size_t)e * H + i] = 0.f;
    }
    for (int i = t; i < a.P; i += HD_THREADS) m.x[H + i] = i == pos ? 1.f : 0.f;
    for (int it = 0; it < a.dT; ++it) {
        const int cnt = hd_neighbours(a.t_bgraph + (size_t)e * HD_TNB, HD_TNB, a.E, ids, &cnt_s);
        for (int j = 0; j < cnt; ++j)
            for (int i = t; i < H; i += HD_THREADS) {
                m.hn[j * H + i] = h[(size_t)ids[j] * H + i];
                if (lstm) m.cn[j * H + i] = c[(size_t)ids[j] * H + i];
            }
        __syncthreads();
        hd_cell(cell, m.x, m.hn, m.cn, cnt, m.s, m.g, m.z, m.oh, m.oc);
        const bool out = tree && it == a.dT - 1 && out_row >= 0 && out_row < a.B;
        for (int i = t; i < H; i += HD_THREADS) {
            h[(size_t)e * H + i] = m.oh[i];
            if (lstm) c[(size_t)e * H + i] = m.oc[i];
            if (out) a.mess_out[(size_t)out_row * a.ld_mess + i] = m.oh[i];
        }
    }
}

// ------------------------------------------------------------------ attachment scores
struct Assm {
    const float* E; int n_ids, H, L, Pmax, NA, B; const float* anode; const int32_t* astamp; int stamp;
    const int32_t* meta; const int32_t* ids; const int32_t* atoms; int P, n_cand, n_id_list, n_atom_list;
    const float* W1; int ldw; const float* b1; const float* Wa; const float* ba; const float* z; int ldz; float* score;
};

// One workgroup per candidate c.  Its prediction is the meta row {n candidates, k (1 or 2), nth_child, molecule, first
// candidate, first id, first atom} with first candidate <= c < first candidate + n; its k atoms are atoms[first atom +
// (c - first candidate) k ..].  v = sum_{j<k} relu(matchNN [hgraph.node[atom_j] | E_assm[id_j] | onehot(nth)]) (an atom the
// step's atom level did not write reads as zero, as the rebuilt hgraph.node gives), score = (W_assm v + b) . z_molecule.
// A candidate without a row, or whose row is out of range anywhere, scores NaN.
__global__ void __launch_bounds__(HD_THREADS) hd_assm_k(Assm a) {
    extern __shared__ float lds[];
    __shared__ float red[HD_THREADS];
    __shared__ int row_s;
    const int c = blockIdx.x, t = threadIdx.x, lane = t % GGPM_WAVE, wv = t / GGPM_WAVE, H = a.H, L = a.L;
    if (t == 0) {
        int f = -1;
        for (int p = 0; p < a.P && f < 0; ++p) {
            const int32_t* m = a.meta + (size_t)p * 7;
            if (m[0] > 0 && m[4] >= 0 && c >= m[4] && c - m[4] < m[0]) f = p;
        }
        row_s = f;
    }
    __syncthreads();
    const int p = row_s;
    bool ok = p >= 0;
    int k = 0, nth = 0, b = 0, roff = 0, abase = 0;
    if (ok) {
        const int32_t* m = a.meta + (size_t)p * 7;
        k = m[1]; nth = m[2]; b = m[3]; roff = m[5];
        ok = k >= 1 && k <= 2 && nth >= 0 && nth < a.Pmax && b >= 0 && b < a.B && roff >= 0 && roff <= a.n_id_list - k &&
             m[6] >= 0 && (long long)m[6] + (long long)(c - m[4] + 1) * k <= (long long)a.n_atom_list;
        abase = m[6] + (c - m[4]) * k;
    }
    for (int j = 0; ok && j < k; ++j)
        ok = a.ids[roff + j] >= 0 && a.ids[roff + j] < a.n_ids && a.atoms[abase + j] >= 0 && a.atoms[abase + j] < a.NA;
    if (!ok) {
        if (t == 0) a.score[c] = __int_as_float(0x7fc00000);
        return;
    }
    float* av = lds;                // [2 H] atom rows
    float* em = av + 2 * H;         // [2 H] embedding rows
    float* v = em + 2 * H;          // [H]
    float* proj = v + H;            // [L]
    const float* zb = a.z + (size_t)b * a.ldz;
    for (int j = 0; j < k; ++j) {
        const int at = a.atoms[abase + j];
        const bool live = a.astamp[at] == a.stamp;
        const float* row = a.E + (size_t)a.ids[roff + j] * H;
        for (int i = t; i < H; i += HD_THREADS) {
            av[j * H + i] = live ? a.anode[(size_t)at * H + i] : 0.f;
            em[j * H + i] = row[i];
        }
    }
    __syncthreads();
    for (int o = wv; o < H; o += HD_WAVES) {
        const float* w = a.W1 + (size_t)o * a.ldw;
        float acc = 0.f;
        for (int j = 0; j < k; ++j)
            acc += fmaxf(a.b1[o] + wave_dot(w, av + j * H, H, lane) + wave_dot(w + H, em + j * H, H, lane) + w[2 * H + nth], 0.f);
        if (lane == 0) v[o] = acc;
    }
    __syncthreads();
    for (int l = wv; l < L; l += HD_WAVES) {
        const float y = a.ba[l] + wave_dot(a.Wa + (size_t)l * H, v, H, lane);
        if (lane == 0) proj[l] = y * zb[l];
    }
    __syncthreads();
    float d = 0.f;
    for (int l = t; l < L; l += HD_THREADS) d += proj[l];
    d = block_sum(d, red);
    if (t == 0) a.score[c] = d;
}

// dims / state / params -> Dec; false when anything is missing or out of the accepted shapes
bool hd_fill(Dec& a, const int* dims, void* const* st, const void* const* pw) {
    if (!dims || !st) return false;
    a.rnn = dims[HD_D_RNN]; a.H = dims[HD_D_H]; a.P = dims[HD_D_P]; a.N = dims[HD_D_N]; a.E = dims[HD_D_E];
    a.NA = dims[HD_D_NA]; a.EA = dims[HD_D_EA]; a.AF = dims[HD_D_AF]; a.EF = dims[HD_D_EF]; a.dT = dims[HD_D_DT];
    a.dG = dims[HD_D_DG]; a.n_cls = dims[HD_D_NCLS]; a.n_icls = dims[HD_D_NICLS]; a.B = dims[HD_D_B];
    if ((a.rnn != 0 && a.rnn != 1) || a.H <= 0 || a.H > HD_MAX_H || a.P <= 0 || a.P > 64 || a.N <= 0 || a.E <= 0 || a.NA <= 0 ||
        a.EA <= 0 || a.AF <= 0 || a.AF > HD_MAX_H || a.EF <= 0 || a.EF > HD_MAX_H || a.dT < 1 || a.dG < 1 || a.n_cls <= 0 ||
        a.n_icls <= 0 || a.B <= 0)
        return false;
    for (int i = 0; i < HD_S_COUNT; ++i) {
        const bool lstm_only = i == HD_S_GC0 || i == HD_S_GC1 || i == HD_S_IC || i == HD_S_TC;
        if (!st[i] && !(lstm_only && a.rnn == 0)) return false;
    }
    a.t_fnode = (int32_t*)st[HD_S_TFNODE]; a.t_fmess = (int32_t*)st[HD_S_TFMESS]; a.t_agraph = (int32_t*)st[HD_S_TAGRAPH];
    a.t_bgraph = (int32_t*)st[HD_S_TBGRAPH]; a.t_cgraph = (int32_t*)st[HD_S_TCGRAPH];
    a.a_fnode = (float*)st[HD_S_AFNODE]; a.a_fmess = (float*)st[HD_S_AFMESS];
    a.a_agraph = (int32_t*)st[HD_S_AAGRAPH]; a.a_bgraph = (int32_t*)st[HD_S_ABGRAPH];
    a.gh[0] = (float*)st[HD_S_GH0]; a.gh[1] = (float*)st[HD_S_GH1]; a.gc[0] = (float*)st[HD_S_GC0]; a.gc[1] = (float*)st[HD_S_GC1];
    a.anode = (float*)st[HD_S_ANODE]; a.astamp = (int32_t*)st[HD_S_ASTAMP];
    a.ih = (float*)st[HD_S_IH]; a.ic = (float*)st[HD_S_IC]; a.th = (float*)st[HD_S_TH]; a.tc = (float*)st[HD_S_TC];
    a.xi = (float*)st[HD_S_XI]; a.xc = (float*)st[HD_S_XC];
    if (!pw) return true;
    const int n_w = a.rnn == 0 ? 7 : 8;
    Cell* cells[3] = {&a.cg, &a.ci, &a.ct};
    for (int l = 0; l < 3; ++l) {
        cells[l]->rnn = a.rnn; cells[l]->H = a.H; cells[l]->I = l == 0 ? a.EF : a.H + a.P;
        for (int i = 0; i < 8; ++i) {
            cells[l]->w[i] = (const float*)pw[8 * l + i];
            if (i < n_w && !pw[8 * l + i]) return false;
        }
    }
    for (int i = HD_P_WOG; i < HD_P_COUNT; ++i)
        if (!pw[i]) return false;
    a.Wog = (const float*)pw[HD_P_WOG]; a.bog = (const float*)pw[HD_P_BOG]; a.Woi = (const float*)pw[HD_P_WOI];
    a.boi = (const float*)pw[HD_P_BOI]; a.Wot = (const float*)pw[HD_P_WOT]; a.bot = (const float*)pw[HD_P_BOT];
    a.Ei = (const float*)pw[HD_P_EI]; a.Ec = (const float*)pw[HD_P_EC]; a.Wi = (const float*)pw[HD_P_WI];
    a.bi = (const float*)pw[HD_P_BI]; a.Wc = (const float*)pw[HD_P_WC]; a.bc = (const float*)pw[HD_P_BC];
    return true;
}

size_t hd_cell_lds_bytes(const Dec& a) { return (size_t)(hd_xw(a.H, a.P, a.EF) + (5 + 2 * HD_TNB) * a.H) * sizeof(float); }

}  // namespace

extern "C" int ggpm_hier_decode_atom_step(const int* dims, void* const* state, const void* const* params, const int32_t* up,
                                          const int* offs, const int* counts, int stamp, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    Dec a{};
    if (!params || !hd_fill(a, dims, state, params) || !up || !offs || !counts) return GGPM_ERR_ARG;
    for (int i = 0; i < 7; ++i)
        if (counts[i] < 0) return GGPM_ERR_ARG;
    for (int i = 0; i < 11; ++i)
        if (offs[i] < 0) return GGPM_ERR_ARG;
    a.tedits = up + offs[0]; a.n_tedits = counts[0];
    a.fn_rows = up + offs[1]; a.fn_data = up + offs[2]; a.n_fn = counts[1];
    a.fm_rows = up + offs[3]; a.fm_data = up + offs[4]; a.n_fm = counts[2];
    a.ag_rows = up + offs[5]; a.ag_data = up + offs[6]; a.n_ag = counts[3];
    a.bg_rows = up + offs[7]; a.bg_data = up + offs[8]; a.n_bg = counts[4];
    a.edges = up + offs[9]; a.n_edges = counts[5];
    a.atoms = up + offs[10]; a.n_atoms = counts[6];
    a.stamp = stamp;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(hd_edit_k, dim3(HD_EDIT_BLOCKS), dim3(HD_THREADS), 0, s, a);
    const size_t lds = hd_cell_lds_bytes(a);
    ggpm_set_lds_addr((const void*)hd_atom_iter_k, lds);
    for (int it = 0; it < a.dG; ++it)
        hipLaunchKernelGGL(hd_atom_iter_k, dim3(a.n_edges > 0 ? a.n_edges : 1), dim3(HD_THREADS), lds, s, a, it);
    const size_t lds_r = (size_t)((a.AF + 3) / 4 * 4 + a.H) * sizeof(float);
    const int work = a.n_atoms + a.n_edges;
    hipLaunchKernelGGL(hd_atom_read_k, dim3(work > 0 ? work : 1), dim3(HD_THREADS), lds_r, s, a);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_hier_decode_tree_step(const int* dims, void* const* state, const void* const* params,
                                          const int32_t* edits, int n_edits, const int32_t* nodes, int n_nodes,
                                          const int32_t* mess, int n_mess, int stamp, float* node_out, int ld_node,
                                          float* mess_out, int ld_mess, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    Dec a{};
    if (!params || !hd_fill(a, dims, state, params) || n_edits < 0 || n_nodes <= 0 || n_nodes > a.B || n_mess < 0 || !nodes ||
        (n_edits > 0 && !edits) || (n_mess == 0 && (n_edits > 0 || !node_out || ld_node < a.H)) ||
        (n_mess > 0 && (!mess || !mess_out || ld_mess < a.H)))
        return GGPM_ERR_ARG;
    a.tedits = edits; a.n_tedits = n_edits; a.nodes = nodes; a.n_nodes = n_nodes; a.mess = mess; a.n_mess = n_mess;
    a.stamp = stamp; a.node_out = node_out; a.ld_node = ld_node; a.mess_out = mess_out; a.ld_mess = ld_mess;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds_n = (size_t)6 * a.H * sizeof(float);
    if (n_mess == 0) {
        hipLaunchKernelGGL(hd_nodes_k, dim3(n_nodes), dim3(HD_THREADS), lds_n, s, a, HD_ST_XI | HD_ST_RI | HD_ST_XC | HD_ST_RC);
        GGPM_CHECK_LAUNCH();
        return GGPM_OK;
    }
    const size_t lds = hd_cell_lds_bytes(a);
    ggpm_set_lds_addr((const void*)hd_mess_k, lds);
    hipLaunchKernelGGL(hd_edit_k, dim3(HD_EDIT_BLOCKS), dim3(HD_THREADS), 0, s, a);
    hipLaunchKernelGGL(hd_nodes_k, dim3(n_nodes), dim3(HD_THREADS), lds_n, s, a, HD_ST_XI);
    hipLaunchKernelGGL(hd_mess_k, dim3(n_mess), dim3(HD_THREADS), lds, s, a, 0);
    hipLaunchKernelGGL(hd_nodes_k, dim3(n_nodes), dim3(HD_THREADS), lds_n, s, a, HD_ST_RI | HD_ST_XC);
    hipLaunchKernelGGL(hd_mess_k, dim3(n_mess), dim3(HD_THREADS), lds, s, a, 1);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_hier_decode_assm_score(const int* dims, void* const* state, const float* E_assm, const int32_t* meta,
                                           const int32_t* ids, const int32_t* atoms, int P, int n_cand, int n_ids,
                                           int n_atoms, const float* W1, int ldw, const float* b1, const float* Wa,
                                           const float* ba, int L, const float* z, int ldz, int stamp, float* score,
                                           ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    Dec d{};
    if (!hd_fill(d, dims, state, nullptr) || P <= 0 || n_cand <= 0 || n_ids <= 0 || n_atoms <= 0 || L <= 0 || L > HD_MAX_H ||
        ldw < 2 * d.H + d.P || ldz < L || !E_assm || !meta || !ids || !atoms || !W1 || !b1 || !Wa || !ba || !z || !score)
        return GGPM_ERR_ARG;
    Assm a{E_assm, d.n_icls, d.H, L, d.P, d.NA, d.B, d.anode, d.astamp, stamp, meta, ids, atoms, P, n_cand, n_ids, n_atoms,
           W1, ldw, b1, Wa, ba, z, ldz, score};
    hipLaunchKernelGGL(hd_assm_k, dim3(n_cand), dim3(HD_THREADS), (size_t)(5 * d.H + L) * sizeof(float), (hipStream_t)stream, a);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}
