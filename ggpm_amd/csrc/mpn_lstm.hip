// Fused LSTM message step for gfx950 (all 32 shipped reference configs use rnn_type = LSTM).
//
// Reference arithmetic: LSTM.forward / LSTM.LSTM (ggpm/rnn.py:96-108, 85-94).  Restated over CSR
// predecessors; the x-halves of W_i/W_o/W/W_f (+ their biases) are hoisted (Xi, Xo, Xu, Xf) and the hidden
// half of the forget gate is applied once per message (qf = Wf_h h) instead of once per padded slot.
//
// Same geometry as mpn_gru.hip (16-row message tiles x column groups, 16 waves, MFMA f32 16x16x4):
//   fwd  A: P1 gather (h_p, c_p, qf_p) -> s, fc tiles | P2 [Wi_h;Wo_h;Wu_h].s + gate math -> h', c'
//           P3 (one column group) qf' = Wf_h h'          B: otherwise the same product from rows re-read from L2
//   bwd  A: P1 successors -> dh partial, dqf, dc tiles | P2 dh += dqf.Wf_h ; gate derivatives, dXf += dFC * F
//           P3 (one column group) dS = di_pre.Wi_h + do_pre.Wo_h + du_pre.Wu_h      B: otherwise, from L2
#include "tile_mma.h"
#include "level_host.h"
#include "level_call.h"
#include <cstdlib>

namespace {

constexpr int ROWS = 16;      // rows of a row tile (the kernels take one or two per workgroup: template parameter RTT)

struct LstmFwdArgs {
    int E1, Hp, tg;
    const float *Xi, *Xo, *Xu, *Xf;
    const float *Hprev, *Cprev, *Qprev;
    float *Hnew, *Cnew, *Qnew;
    float *S, *I, *O, *U, *F;        // stash slot (nullptr when not saving); F = sum_p c_p f(1-f)
    const float *Wi, *Wo, *Wu, *Wf;  // packed
    const int32_t *rowptr, *col;
    const unsigned char* frozen;     // sparse_forward only: rows that keep their (h, c)
    int fuse_b;                      // single column group: kernel A also forms qf' = Wf_h h' (no B launch)
    int h0_zero;                     // first depth of a dense level: h^0 = c^0 = 0 -> no gather, no gate products
    int bf16;                        // gate products on bf16 operands (packed weights are bf16 fragments then)
    int st16;                        // bf16 storage of Hs / Qs / S / I / O / U (gate mode 1, large dense training levels; tile_mma.h)
    float* Hout;                     // ... then the LAST depth also writes h' in fp32 here (the level's result)
    const float *src_h, *src_c;      // kernel B of a sparse forward's qf^0 launch (ggpm_level_opts.gather_*): the start
    const int32_t* src_idx;          // (h, c) of row r is (src_h, src_c)[src_idx[r]] (zero when < 0), written to Hnew / Cnew
};

__device__ __forceinline__ float4 one_minus(float4 r) { return make_float4(1.f - r.x, 1.f - r.y, 1.f - r.z, 1.f - r.w); }

// ---------------------------------------------------------------------------------------------- forward
// Kernel A (16 waves): every wave gathers one message row at a time: s over the full row (GEMM operand), the
// forget sum fc (and its backward coefficient) only over this workgroup's column group; then the first `tg`
// waves run [Wi_h; Wo_h; Wu_h] . s for their output tile and the gate math.
template <bool STASH, int GM, int RTT, bool ST16 = false>
__global__ void GGPM_A_BOUNDS lstm_fwd_a(LstmFwdArgs a) {
    static_assert(!ST16 || GM == 1, "bf16 storage goes with bf16 gate products");      // the cell state c and F stay fp32
    constexpr int ROWS = RTT * 16;      // RTT = 2: two row tiles per workgroup (ggpm_level_opts.prefer_narrow), no fused P3
    constexpr bool BF16 = GM == 1, SPLIT = GM == 2;      // gate mode (LstmFwdArgs.bf16): 0 fp32 MFMA, 1 bf16, 2 split operands
    static_assert(!SPLIT || RTT == 1, "split operands: one row tile per workgroup");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int Hp = a.Hp, LD = Hp + 4, KC = Hp / 16, NT = Hp / 16;
    // split operands (tile_mma.h): fc keeps its fp32 tile (epilogue only) at the head; behind it the bf16 images of s and,
    // for the fused qf' phase, h' (s itself is a GEMM operand only)
    float* Ts = SPLIT ? nullptr : lds;
    float* Tf = SPLIT ? lds : lds + ROWS * LD;      // fc, full-width tile of which only the group's columns are written/read
    const int LDH = ggpm_split_ldh(Hp), PLANE = ROWS * LDH, KC32 = ggpm_kc32_dev(Hp), IMG = ggpm_split_image_halves(ROWS, Hp);
    __bf16* Is = reinterpret_cast<__bf16*>(lds + ROWS * LD);
    __bf16* Ih = Is + IMG;
    if constexpr (SPLIT) ggpm_split_init(Is, a.fuse_b ? 2 : 1, ROWS, Hp);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r0 = blockIdx.x * ROWS;
    const int grp = blockIdx.y;
    const int t = grp * a.tg + wave;
    const int g_lo = 16 * a.tg * grp, g_hi = min(Hp, g_lo + 16 * a.tg);   // column range of this group

    for (int lr = wave; lr < ROWS; lr += GGPM_NWA) {
        const int row = r0 + lr;
        GgpmRowList rl;
        if (a.h0_zero) { rl.lo = 0; rl.n = 0; } else rl = ggpm_row_list(a.rowptr, row, a.E1);
        const size_t rowo = (size_t)(row < a.E1 ? row : 0) * Hp;
        for (int c0 = 0; c0 < Hp; c0 += 512) {
            int c[2], cs[2], cf[2];
            bool on[2], mine[2];
            float4 s[2], fc[2], fco[2], xf[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                c[k] = c0 + 256 * k + lane * 4;
                on[k] = c[k] < Hp;
                cs[k] = on[k] ? c[k] : 0;
                mine[k] = c[k] >= g_lo && c[k] < g_hi;
                cf[k] = mine[k] ? c[k] : g_lo;           // other lanes re-read one in-group column (no branch)
                s[k] = ggpm_zero4(); fc[k] = ggpm_zero4(); fco[k] = ggpm_zero4();
                xf[k] = ggpm_ld4(a.Xf + rowo + cf[k]);
            }
            for (int base = 0; base < rl.n; base += 64) {
                const int chunk = ggpm_list_chunk(a.col, rl, base, lane);
                const int m = min(64, rl.n - base);
                for (int j = 0; j < m; j += 2) {
                    float4 h[2][2], cc[2][2], q[2][2];
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const size_t p = (size_t)ggpm_list_at(chunk, j + u, m) * Hp;
#pragma unroll
                        for (int k = 0; k < 2; ++k) {
                            h[u][k] = ggpm_ldx<ST16>(a.Hprev, p + cs[k]);
                            cc[u][k] = ggpm_ld4(a.Cprev + p + cf[k]);
                            q[u][k] = ggpm_ldx<ST16>(a.Qprev, p + cf[k]);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int k = 0; k < 2; ++k) {          // null slots: h[0] = c[0] = 0
                            const float4 f = ggpm_fsigmoid4<BF16>(xf[k] + q[u][k]);
                            const float4 fcc = f * cc[u][k];
                            s[k] = s[k] + h[u][k];
                            fc[k] = fc[k] + fcc;
                            fco[k] = fco[k] + fcc * one_minus(f);
                        }
                }
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (!on[k]) continue;
                if constexpr (ST16) s[k] = ggpm_rne4(s[k]);
                if constexpr (SPLIT) ggpm_split_store(Is, PLANE, LDH, lr, c[k], s[k]);
                else ggpm_st4(Ts + lr * LD + c[k], s[k]);
                if (mine[k]) {
                    ggpm_st4(Tf + lr * LD + c[k], fc[k]);
                    if (STASH && row < a.E1) {
                        const size_t o = (size_t)row * Hp + c[k];
                        ggpm_stx<ST16>(a.S, o, s[k]);
                        ggpm_st4(a.F + o, fco[k]);
                    }
                }
            }
        }
    }

    // the first weight fragments of P2 travel from L2 while this wave waits for the slower gatherers
    const int t_end = min(NT, (grp + 1) * a.tg);
    const float* const wps2[3] = {a.Wi, a.Wo, a.Wu};
    std::conditional_t<GM == 0, GgpmRing<3>, GgpmNoRing> ring2;
    std::conditional_t<SPLIT, GgpmSplitRing<3>, GgpmNoRing> sring2;
    if constexpr (GM == 0)
        if (!a.h0_zero && t < t_end) ggpm_ring_prefetch<3>(wps2, KC, t, lane, ring2);
    if constexpr (SPLIT)
        if (!a.h0_zero && t < t_end) ggpm_split_ring_prefetch<3>(wps2, KC32, t, lane, sring2);
    ggpm_lds_barrier();      // LDS tiles only: the stash stores above finish under the GEMM

    const int lr = lane & 15;
    float* Th = lds + 2 * ROWS * LD;      // fused P3 only: the complete h' rows of this workgroup
    for (int tt = t; tt < t_end; tt += GGPM_NWA) {
        const int c = 16 * tt + 4 * (lane >> 4);
        float4 xi[RTT], xo[RTT], xu[RTT];
        auto load_inputs = [&](int r) {
            const int row = r0 + 16 * r + lr;
            const size_t o = (size_t)(row < a.E1 ? row : 0) * Hp + c;
            xi[r] = ggpm_ld4(a.Xi + o); xo[r] = ggpm_ld4(a.Xo + o); xu[r] = ggpm_ld4(a.Xu + o);
        };
        if constexpr (RTT == 1 && !SPLIT) load_inputs(0);     // in flight under the GEMM (two row tiles / split operands: the
                                                              // registers go to the GEMM)
        f32x4 acc[3][RTT];
        ggpm_zero_acc<3, RTT>(acc);
        if (!a.h0_zero) {
            const float* const tiles[3] = {Ts, Ts, Ts};
            const int tn = tt + GGPM_NWA < t_end ? tt + GGPM_NWA : -1;
            if constexpr (SPLIT) {
                const __bf16* const imgs[3] = {Is, Is, Is};
                ggpm_wave_gemm_split<3, true>(imgs, PLANE, LDH, wps2, KC32, tt, tn, lane, acc, sring2);
            } else if constexpr (BF16) ggpm_wave_gemm_bf16<3, RTT>(tiles, LD, wps2, Hp, tt, lane, acc);
            else ggpm_wave_gemm_ring<3, RTT>(tiles, LD, wps2, KC, tt, tn, lane, acc, ring2);
        }
#pragma unroll
        for (int r = 0; r < RTT; ++r) {
            if constexpr (RTT != 1 || SPLIT) load_inputs(r);
            const int lrow = 16 * r + lr, row = r0 + lrow;
            const size_t o = (size_t)(row < a.E1 ? row : 0) * Hp + c;
            float4 h = ggpm_zero4(), cn = ggpm_zero4(), gi = ggpm_zero4(), go = ggpm_zero4(), gu = ggpm_zero4();
            auto keep_h = [&](float4 v) {          // the complete h' rows for the fused qf' phase
                if constexpr (SPLIT) ggpm_split_store(Ih, PLANE, LDH, lrow, c, v);
                else ggpm_st4(Th + lrow * LD + c, v);
            };
            if (row >= a.E1) {
                if (a.fuse_b) keep_h(h);
                continue;
            }
            if (a.frozen && a.frozen[row]) {
                h = ggpm_ld4(a.Hprev + o);             // gates stashed as 0 => the backward passes dh, dc through
                cn = ggpm_ld4(a.Cprev + o);
            } else if (row != 0 || a.frozen) {
                const float4 pi = ggpm_f4(acc[0][r]) + xi[r];
                const float4 po = ggpm_f4(acc[1][r]) + xo[r];
                const float4 pu = ggpm_f4(acc[2][r]) + xu[r];
                const float4 fc = ggpm_ld4(Tf + lrow * LD + c);
                gi = ggpm_sigmoid4(pi);
                go = ggpm_sigmoid4(po);
                gu = make_float4(tanhf(pu.x), tanhf(pu.y), tanhf(pu.z), tanhf(pu.w));
                if constexpr (ST16) { gi = ggpm_rne4(gi); go = ggpm_rne4(go); gu = ggpm_rne4(gu); }      // (as stashed)
                cn = gi * gu + fc;
                h = go * make_float4(tanhf(cn.x), tanhf(cn.y), tanhf(cn.z), tanhf(cn.w));
                if constexpr (ST16) h = ggpm_rne4(h);
            }
            ggpm_stx<ST16>(a.Hnew, o, h);
            if constexpr (ST16) if (a.Hout) ggpm_st4(a.Hout + o, h);
            ggpm_st4(a.Cnew + o, cn);
            if (a.fuse_b) keep_h(h);
            if (STASH) {
                ggpm_stx<ST16>(a.I, o, gi);
                ggpm_stx<ST16>(a.O, o, go);
                ggpm_stx<ST16>(a.U, o, gu);
            }
        }
    }
    if (!a.fuse_b) return;

    // ---- P3 (single column group, RTT = 1 only): qf' = Wf_h h' from the rows this workgroup already holds
    if constexpr (RTT == 1) {
        const int row = r0 + lr;
        const float* const wps3[1] = {a.Wf};
        std::conditional_t<GM == 0, GgpmRing<1>, GgpmNoRing> ring3;
        std::conditional_t<SPLIT, GgpmSplitRing<1>, GgpmNoRing> sring3;
        if constexpr (GM == 0)
            if (wave < NT) ggpm_ring_prefetch<1>(wps3, KC, wave, lane, ring3);
        if constexpr (SPLIT)
            if (wave < NT) ggpm_split_ring_prefetch<1>(wps3, KC32, wave, lane, sring3);
        ggpm_lds_barrier();
        for (int tt = wave; tt < NT; tt += GGPM_NWA) {
            f32x4 acc[1][1];
            ggpm_zero_acc<1, 1>(acc);
            const float* const tiles[1] = {Th};
            const int tn = tt + GGPM_NWA < NT ? tt + GGPM_NWA : -1;
            if constexpr (SPLIT) {
                const __bf16* const imgs[1] = {Ih};
                ggpm_wave_gemm_split<1>(imgs, PLANE, LDH, wps3, KC32, tt, tn, lane, acc, sring3);
            } else if constexpr (BF16) ggpm_wave_gemm_bf16<1, 1>(tiles, LD, wps3, Hp, tt, lane, acc);
            else ggpm_wave_gemm_ring<1, 1>(tiles, LD, wps3, KC, tt, tn, lane, acc, ring3);
            const int c = 16 * tt + 4 * (lane >> 4);
            if (row < a.E1) ggpm_stx<ST16>(a.Qnew, (size_t)row * Hp + c, ggpm_f4(acc[0][0]));
        }
    }
}

// Kernel B (same geometry as A): qf' = Wf_h h'.
template <int GM, int RTT, bool ST16 = false>
__global__ void GGPM_A_BOUNDS lstm_fwd_b(LstmFwdArgs a) {
    constexpr int ROWS = RTT * 16;
    constexpr bool BF16 = GM == 1, SPLIT = GM == 2;
    static_assert(!SPLIT || RTT == 1, "split operands: one row tile per workgroup");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int Hp = a.Hp, LD = Hp + 4, KC = Hp / 16, NT = Hp / 16;
    float* Th = lds;
    const int LDH = ggpm_split_ldh(Hp), PLANE = ROWS * LDH, KC32 = ggpm_kc32_dev(Hp);
    __bf16* Ih = reinterpret_cast<__bf16*>(lds);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r0 = blockIdx.x * ROWS;
    const int grp = blockIdx.y;
    const int t_end = min(NT, (grp + 1) * a.tg);
    const float* const wps[1] = {a.Wf};
    std::conditional_t<GM == 0, GgpmRing<1>, GgpmNoRing> ring;
    std::conditional_t<SPLIT, GgpmSplitRing<1>, GgpmNoRing> sring;
    if constexpr (GM == 0)
        if (grp * a.tg + wave < t_end) ggpm_ring_prefetch<1>(wps, KC, grp * a.tg + wave, lane, ring);     // under the row copy
    if constexpr (SPLIT) {
        if (grp * a.tg + wave < t_end) ggpm_split_ring_prefetch<1>(wps, KC32, grp * a.tg + wave, lane, sring);
        ggpm_split_init(Ih, 1, ROWS, Hp);
    }
    if (a.src_idx) {
        if constexpr (SPLIT) ggpm_gather_rows_to_lds_split<ROWS>(a.src_h, a.src_idx, r0, a.E1, Hp, Ih, PLANE, LDH, grp == 0 ? a.Hnew : nullptr);
        else ggpm_gather_rows_to_lds<ROWS>(a.src_h, a.src_idx, r0, a.E1, Hp, LD, Th, grp == 0 ? a.Hnew : nullptr);
        if (grp == 0) {            // the cell state of the same rows: copied through, not a GEMM operand
            const int q = Hp >> 2;
            for (int it = threadIdx.x; it < ROWS * q; it += blockDim.x) {
                const int lr = it / q, c = (it - lr * q) * 4, r = r0 + lr;
                if (r >= a.E1) continue;
                const int id = a.src_idx[r];
                ggpm_st4(a.Cnew + (size_t)r * Hp + c, id >= 0 ? ggpm_ld4(a.src_c + (size_t)id * Hp + c) : ggpm_zero4());
            }
        }
    } else {
        if constexpr (SPLIT) ggpm_load_rows_to_lds_split<ROWS>(a.Hnew, r0, a.E1, Hp, Ih, PLANE, LDH);
        else ggpm_load_rows_to_lds<ROWS, ST16>(a.Hnew, r0, a.E1, Hp, LD, Th);
    }
    __syncthreads();
    for (int tt = grp * a.tg + wave; tt < t_end; tt += GGPM_NWA) {
        f32x4 acc[1][RTT];
        ggpm_zero_acc<1, RTT>(acc);
        {
            const float* const tiles[1] = {Th};
            const int tn = tt + GGPM_NWA < t_end ? tt + GGPM_NWA : -1;
            if constexpr (SPLIT) {
                const __bf16* const imgs[1] = {Ih};
                ggpm_wave_gemm_split<1>(imgs, PLANE, LDH, wps, KC32, tt, tn, lane, acc, sring);
            } else if constexpr (BF16) ggpm_wave_gemm_bf16<1, RTT>(tiles, LD, wps, Hp, tt, lane, acc);
            else ggpm_wave_gemm_ring<1, RTT>(tiles, LD, wps, KC, tt, tn, lane, acc, ring);
        }
        const int c = 16 * tt + 4 * (lane >> 4);
#pragma unroll
        for (int r = 0; r < RTT; ++r) {
            const int row = r0 + 16 * r + (lane & 15);
            if (row < a.E1) ggpm_stx<ST16>(a.Qnew, (size_t)row * Hp + c, ggpm_f4(acc[0][r]));
        }
    }
}

// ---------------------------------------------------------------------------------------------- backward
struct LstmBwdArgs {
    int E1, Hp, tg;
    int first;
    const float* Xf;
    const float *Ccur, *Qcur;        // Cs[t], Qs[t]
    const float *I, *O, *U, *F;      // stash slot t-1
    const float* dHD;
    const float *dSin, *dFCin;
    float *dSout, *dFCout;
    float* DQ;                       // dqf^t stash slot (nullptr when first)
    float *DI, *DO, *DU;             // stash slot t-1
    float *dXi, *dXo, *dXu, *dXf;    // running sums (zeroed by the driver)
    const float *WiT, *WoT, *WuT, *WfT;
    const int32_t *srowptr, *scol;
    // sparse_forward only (see mpn_gru.hip): frozen rows carry dh / dc through the loop; final gather-only launch
    const unsigned char* frozen;
    const float* dCD;                // gradient of c_D (sparse_forward returns the cell state too)
    float *carry_h, *carry_c;        // [E1,Hp] each, started by the first backward depth
    int final_pass;
    float *dHin, *dCin;
    float *scat_h, *scat_c;          // ggpm_level_opts.scatter_*: the final pass ADDS row r's results to
    const int32_t* scat_idx;         // (scat_h, scat_c)[scat_idx[r]] (unique ids; < 0: dropped) instead of writing dHin / dCin
    int fuse_b;                      // single column group: kernel A also forms dS for depth t-1 (no B launch)
    int bf16;                        // gate products on bf16 operands
    int skip_xsum;                   // dXi / dXo / dXu are NOT accumulated here (the caller sums the DI / DO / DU stash slots)
    int st16;                        // bf16 storage of Hs / Qs / I / O / U / dS / DQ / DI / DO / DU (see LstmFwdArgs)
};

// Kernel A (16 waves): successors -> dqf (full rows), dh partial / dc (own columns) -> dh += dqf.Wf_h ->
// gate derivatives; dXf += dFC * F.
template <int GM, int RTT, bool ST16 = false>
__global__ void GGPM_A_BOUNDS lstm_bwd_a(LstmBwdArgs a) {
    constexpr int ROWS = RTT * 16;      // RTT = 2: two row tiles per workgroup (ggpm_level_opts.prefer_narrow), no fused P3
    constexpr bool BF16 = GM == 1, SPLIT = GM == 2;
    static_assert(!SPLIT || RTT == 1, "split operands: one row tile per workgroup");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int Hp = a.Hp, LD = Hp + 4, KC = Hp / 16, NT = Hp / 16;
    // split operands: the fp32 tiles of dh partial and dc (epilogue only) at the head, behind them the bf16 images of dqf
    // and, for the fused dS phase, di_pre / do_pre / du_pre
    float* T1 = lds;                      // dqf  (full rows)
    float* T0 = SPLIT ? lds : lds + ROWS * LD;                    // dh partial (group columns)
    float* T2 = SPLIT ? lds + ROWS * LD : lds + 2 * ROWS * LD;    // dc         (group columns)
    const int LDH = ggpm_split_ldh(Hp), PLANE = ROWS * LDH, KC32 = ggpm_kc32_dev(Hp), IMG = ggpm_split_image_halves(ROWS, Hp);
    __bf16* I1 = reinterpret_cast<__bf16*>(lds + 2 * ROWS * LD);
    __bf16* Ia = I1 + IMG;
    __bf16* Ib = Ia + IMG;
    __bf16* Ic = Ib + IMG;
    if constexpr (SPLIT) ggpm_split_init(I1, a.fuse_b ? 4 : 1, ROWS, Hp);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r0 = blockIdx.x * ROWS;
    const int grp = blockIdx.y;
    const int t = grp * a.tg + wave;
    const int g_lo = 16 * a.tg * grp, g_hi = min(Hp, g_lo + 16 * a.tg);

    if (!a.first) {
        for (int lr = wave; lr < ROWS; lr += GGPM_NWA) {
            const int p = r0 + lr;
            const GgpmRowList rl = ggpm_row_list(a.srowptr, p, a.E1);
            const size_t po = (size_t)(p < a.E1 ? p : 0) * Hp;
            for (int c0 = 0; c0 < Hp; c0 += 512) {
                int c[2], cs[2], cf[2];
                bool on[2], mine[2];
                float4 dh[2], dq[2], dc[2], cp[2], qp[2];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    c[k] = c0 + 256 * k + lane * 4;
                    on[k] = c[k] < Hp;
                    cs[k] = on[k] ? c[k] : 0;
                    mine[k] = c[k] >= g_lo && c[k] < g_hi;
                    cf[k] = mine[k] ? c[k] : g_lo;
                    dh[k] = ggpm_zero4(); dq[k] = ggpm_zero4(); dc[k] = ggpm_zero4();
                    cp[k] = ggpm_ld4(a.Ccur + po + cs[k]);
                    qp[k] = ggpm_ldx<ST16>(a.Qcur, po + cs[k]);
                }
                for (int base = 0; base < rl.n; base += 64) {
                    const int chunk = ggpm_list_chunk(a.scol, rl, base, lane);
                    const int m = min(64, rl.n - base);
                    for (int j = 0; j < m; j += 2) {
                        float4 xf[2][2], dfc[2][2], ds[2][2];
#pragma unroll
                        for (int u = 0; u < 2; ++u) {
                            const size_t e = (size_t)ggpm_list_at(chunk, j + u, m) * Hp;
#pragma unroll
                            for (int k = 0; k < 2; ++k) {
                                xf[u][k] = ggpm_ld4(a.Xf + e + cs[k]);
                                dfc[u][k] = ggpm_ld4(a.dFCin + e + cs[k]);
                                ds[u][k] = ggpm_ldx<ST16>(a.dSin, e + cf[k]);
                            }
                        }
#pragma unroll
                        for (int u = 0; u < 2; ++u)
#pragma unroll
                            for (int k = 0; k < 2; ++k) {
                                const float4 f = ggpm_fsigmoid4<BF16>(xf[u][k] + qp[k]);
                                const float4 dff = dfc[u][k] * f;
                                dh[k] = dh[k] + ds[u][k];
                                dc[k] = dc[k] + dff;
                                dq[k] = dq[k] + dff * cp[k] * one_minus(f);
                            }
                    }
                }
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    if (!on[k]) continue;
                    if constexpr (SPLIT) ggpm_split_store(I1, PLANE, LDH, lr, c[k], dq[k]);
                    else ggpm_st4(T1 + lr * LD + c[k], dq[k]);
                    if (mine[k]) {
                        ggpm_st4(T0 + lr * LD + c[k], dh[k]);
                        ggpm_st4(T2 + lr * LD + c[k], dc[k]);
                        if (p < a.E1) ggpm_stx<ST16>(a.DQ, (size_t)p * Hp + c[k], dq[k]);
                    }
                }
            }
        }
    }

    const int t_end = min(NT, (grp + 1) * a.tg);
    const float* const wps2[1] = {a.WfT};
    std::conditional_t<GM == 0, GgpmRing<1>, GgpmNoRing> ring2;
    std::conditional_t<SPLIT, GgpmSplitRing<1>, GgpmNoRing> sring2;
    if constexpr (GM == 0)
        if (!a.first && t < t_end) ggpm_ring_prefetch<1>(wps2, KC, t, lane, ring2);      // under the wait for the gatherers
    if constexpr (SPLIT)
        if (!a.first && t < t_end) ggpm_split_ring_prefetch<1>(wps2, KC32, t, lane, sring2);
    if (!a.first) ggpm_lds_barrier();      // LDS tiles only: the dqf stash stores finish under the GEMM

    const int lr = lane & 15;
    float* Ta = lds + 3 * ROWS * LD;      // fused P3 only: complete di_pre / do_pre / du_pre rows
    float* Tb = lds + 4 * ROWS * LD;
    float* Tc = lds + 5 * ROWS * LD;
    for (int tt = t; tt < t_end; tt += GGPM_NWA) {
        // split operands: everything the epilogue derives from the lane id (row, column, LDS and global addresses) is formed
        // BEHIND the GEMM from an opaque copy of it -- hoisted in front of the tile loop those ~20 values lived across the
        // GEMM beside its ring and spilled
        int lane_e = lane;
        int c = 16 * tt + 4 * (lane >> 4), lr = lane & 15;
        float4 gi[RTT], go[RTT], gu[RTT], cc[RTT], fco[RTT], oxi[RTT], oxo[RTT], oxu[RTT], oxf[RTT], dhd[RTT], dcd[RTT];
        auto load_inputs = [&](int r) {
            const int row = r0 + 16 * r + lr;
            const unsigned o = ((unsigned)(row < a.E1 ? row : 0) * (unsigned)Hp + (unsigned)c) * 4u;      // BYTES (E1 * Hp < 2^29, checked by the host)
            gi[r] = go[r] = gu[r] = cc[r] = fco[r] = oxi[r] = oxo[r] = oxu[r] = oxf[r] = ggpm_zero4();
            if (!a.final_pass) {
                gi[r] = ggpm_ldxo<ST16>(a.I, o); go[r] = ggpm_ldxo<ST16>(a.O, o); gu[r] = ggpm_ldxo<ST16>(a.U, o); cc[r] = ggpm_ld4o(a.Ccur, o);
                fco[r] = ggpm_ld4o(a.F, o);
                if (!a.first) {        // depth D starts the dX sums
                    if (!a.skip_xsum) { oxi[r] = ggpm_ld4o(a.dXi, o); oxo[r] = ggpm_ld4o(a.dXo, o); oxu[r] = ggpm_ld4o(a.dXu, o); }
                    oxf[r] = ggpm_ld4o(a.dXf, o);
                }
            }
            dhd[r] = a.first ? ggpm_ld4o(a.dHD, o) : ggpm_zero4();
            dcd[r] = (a.first && a.dCD) ? ggpm_ld4o(a.dCD, o) : ggpm_zero4();
        };
        if constexpr (RTT == 1 && !SPLIT) load_inputs(0);     // in flight under the GEMM (two row tiles / split operands: the
                                                              // registers go to the GEMM, each tile's operands are fetched
                                                              // where its epilogue starts)
        f32x4 acc[1][RTT];
        ggpm_zero_acc<1, RTT>(acc);
        if (!a.first) {
            const float* const tiles[1] = {T1};
            const int tn = tt + GGPM_NWA < t_end ? tt + GGPM_NWA : -1;
            if constexpr (SPLIT) {
                // (the ring is NOT carried into the epilogue -- its eleven operand loads need the registers: a wave's second
                // tile fetches its first fragments here)
                if (tt != t) ggpm_split_ring_prefetch<1>(wps2, KC32, tt, lane, sring2);
                const __bf16* const imgs[1] = {I1};
                ggpm_wave_gemm_split<1>(imgs, PLANE, LDH, wps2, KC32, tt, -1, lane, acc, sring2);
            } else if constexpr (BF16) ggpm_wave_gemm_bf16<1, RTT>(tiles, LD, wps2, Hp, tt, lane, acc);
            else ggpm_wave_gemm_ring<1, RTT>(tiles, LD, wps2, KC, tt, tn, lane, acc, ring2);
        }
        if constexpr (SPLIT) {
            asm volatile("" : "+v"(lane_e));
            c = 16 * tt + 4 * (lane_e >> 4);
            lr = lane_e & 15;
        }
#pragma unroll
        for (int r = 0; r < RTT; ++r) {
            if constexpr (RTT != 1 || SPLIT) load_inputs(r);
            const int lrow = 16 * r + lr, row = r0 + lrow;
            const unsigned o = ((unsigned)(row < a.E1 ? row : 0) * (unsigned)Hp + (unsigned)c) * 4u;      // BYTES (E1 * Hp < 2^29, checked by the host)
            auto keep_iou = [&](float4 vi, float4 vo, float4 vu) {      // the complete gate-gradient rows for the fused dS phase
                if constexpr (SPLIT) {
                    ggpm_split_store(Ia, PLANE, LDH, lrow, c, vi);
                    ggpm_split_store(Ib, PLANE, LDH, lrow, c, vo);
                    ggpm_split_store(Ic, PLANE, LDH, lrow, c, vu);
                } else {
                    ggpm_st4(Ta + lrow * LD + c, vi);
                    ggpm_st4(Tb + lrow * LD + c, vo);
                    ggpm_st4(Tc + lrow * LD + c, vu);
                }
            };
            if (row >= a.E1) {
                if (a.fuse_b) keep_iou(ggpm_zero4(), ggpm_zero4(), ggpm_zero4());
                continue;
            }
            const bool frz = a.frozen && a.frozen[row];
            if (a.final_pass) {        // gradient of the incoming (h, c): frozen rows only
                float4 dh0 = ggpm_zero4(), dc0 = ggpm_zero4();
                if (frz) {
                    dh0 = ggpm_f4(acc[0][r]) + ggpm_ld4(T0 + lrow * LD + c) + ggpm_ld4o(a.carry_h, o);
                    dc0 = ggpm_ld4(T2 + lrow * LD + c) + ggpm_ld4o(a.carry_c, o);
                }
                if (a.scat_idx) {
                    const int id = frz ? a.scat_idx[row] : -1;
                    if (id >= 0) {
                        float* dh_to = a.scat_h + (size_t)id * Hp + c;
                        float* dc_to = a.scat_c + (size_t)id * Hp + c;
                        ggpm_st4(dh_to, ggpm_ld4(dh_to) + dh0);
                        ggpm_st4(dc_to, ggpm_ld4(dc_to) + dc0);
                    }
                } else {
                    ggpm_st4o(a.dHin, o, dh0);
                    ggpm_st4o(a.dCin, o, dc0);
                }
                continue;
            }
            float4 dip = ggpm_zero4(), dop = ggpm_zero4(), dup = ggpm_zero4(), dfc = ggpm_zero4();
            if (row != 0 || a.frozen) {
                float4 dh, dc;
                if (a.first) { dh = dhd[r]; dc = dcd[r]; }
                else { dh = ggpm_f4(acc[0][r]) + ggpm_ld4(T0 + lrow * LD + c); dc = ggpm_ld4(T2 + lrow * LD + c); }
                if (frz) {             // (h, c)_t = (h, c)_{t-1}: carry both gradients to the previous depth
                    if (!a.first) {        // (the first backward depth starts the carries: no memset)
                        dh = dh + ggpm_ld4o(a.carry_h, o);
                        dc = dc + ggpm_ld4o(a.carry_c, o);
                    }
                    ggpm_st4o(a.carry_h, o, dh);
                    ggpm_st4o(a.carry_c, o, dc);
                    dh = ggpm_zero4();
                    dc = ggpm_zero4();
                }
                const float dhv[4] = {dh.x, dh.y, dh.z, dh.w}, dcv[4] = {dc.x, dc.y, dc.z, dc.w};
                const float iv[4] = {gi[r].x, gi[r].y, gi[r].z, gi[r].w}, ov[4] = {go[r].x, go[r].y, go[r].z, go[r].w};
                const float uv[4] = {gu[r].x, gu[r].y, gu[r].z, gu[r].w}, cv[4] = {cc[r].x, cc[r].y, cc[r].z, cc[r].w};
                float r_i[4], r_o[4], r_u[4], r_c[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float tc = tanhf(cv[k]);
                    const float dct = dcv[k] + dhv[k] * ov[k] * (1.f - tc * tc);
                    r_c[k] = dct;
                    r_o[k] = dhv[k] * tc * ov[k] * (1.f - ov[k]);
                    r_i[k] = dct * uv[k] * iv[k] * (1.f - iv[k]);
                    r_u[k] = dct * iv[k] * (1.f - uv[k] * uv[k]);
                }
                dip = make_float4(r_i[0], r_i[1], r_i[2], r_i[3]);
                dop = make_float4(r_o[0], r_o[1], r_o[2], r_o[3]);
                dup = make_float4(r_u[0], r_u[1], r_u[2], r_u[3]);
                dfc = make_float4(r_c[0], r_c[1], r_c[2], r_c[3]);
                if constexpr (ST16) { dip = ggpm_rne4(dip); dop = ggpm_rne4(dop); dup = ggpm_rne4(dup); }      // (as stored)
            }
            ggpm_stxo<ST16>(a.DI, o, dip);
            ggpm_stxo<ST16>(a.DO, o, dop);
            ggpm_stxo<ST16>(a.DU, o, dup);
            ggpm_st4o(a.dFCout, o, dfc);
            if (!a.skip_xsum) {
                ggpm_st4o(a.dXi, o, oxi[r] + dip);
                ggpm_st4o(a.dXo, o, oxo[r] + dop);
                ggpm_st4o(a.dXu, o, oxu[r] + dup);
            }
            ggpm_st4o(a.dXf, o, oxf[r] + dfc * fco[r]);      // dXf_e += dFC_e * sum_p c_p f(1-f)
            if (a.fuse_b) keep_iou(dip, dop, dup);
        }
    }
    if (!a.fuse_b) return;

    // ---- P3 (single column group, RTT = 1 only): dS = di_pre.Wi_h + do_pre.Wo_h + du_pre.Wu_h from the rows held here
    if constexpr (RTT == 1) {
        const int row = r0 + lr;
        const float* const wps3[3] = {a.WiT, a.WoT, a.WuT};
        std::conditional_t<GM == 0, GgpmRing<3>, GgpmNoRing> ring3;
        std::conditional_t<SPLIT, GgpmSplitRing<3>, GgpmNoRing> sring3;
        if constexpr (GM == 0)
            if (wave < NT) ggpm_ring_prefetch<3>(wps3, KC, wave, lane, ring3);
        if constexpr (SPLIT)
            if (wave < NT) ggpm_split_ring_prefetch<3>(wps3, KC32, wave, lane, sring3);
        ggpm_lds_barrier();
        for (int tt = wave; tt < NT; tt += GGPM_NWA) {
            f32x4 acc[3][1];
            ggpm_zero_acc<3, 1>(acc);
            {
                const float* const tiles[3] = {Ta, Tb, Tc};
                const int tn = tt + GGPM_NWA < NT ? tt + GGPM_NWA : -1;
                if constexpr (SPLIT) {      // (the three products are summed: one accumulator pair, acc[0]; acc[1], acc[2] stay 0)
                    const __bf16* const imgs[3] = {Ia, Ib, Ic};
                    ggpm_wave_gemm_split<3, false, true>(imgs, PLANE, LDH, wps3, KC32, tt, tn, lane, acc, sring3);
                } else if constexpr (BF16) ggpm_wave_gemm_bf16<3, 1>(tiles, LD, wps3, Hp, tt, lane, acc);
                else ggpm_wave_gemm_ring<3, 1>(tiles, LD, wps3, KC, tt, tn, lane, acc, ring3);
            }
            const int c = 16 * tt + 4 * (lane >> 4);
            if (row < a.E1)
                ggpm_stx<ST16>(a.dSout, (size_t)row * Hp + c, ggpm_f4(acc[0][0]) + ggpm_f4(acc[1][0]) + ggpm_f4(acc[2][0]));
        }
    }
}

// Kernel B (same geometry as A): dS = di_pre.Wi_h + do_pre.Wo_h + du_pre.Wu_h (for depth t-1).
template <int GM, int RTT, bool ST16 = false>
__global__ void GGPM_A_BOUNDS lstm_bwd_b(LstmBwdArgs a) {
    constexpr int ROWS = RTT * 16;
    constexpr bool BF16 = GM == 1, SPLIT = GM == 2;
    static_assert(!SPLIT || RTT == 1, "split operands: one row tile per workgroup");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int Hp = a.Hp, LD = Hp + 4, KC = Hp / 16, NT = Hp / 16;
    float* Ta = lds;
    float* Tb = lds + ROWS * LD;
    float* Tc = lds + 2 * ROWS * LD;
    const int LDH = ggpm_split_ldh(Hp), PLANE = ROWS * LDH, KC32 = ggpm_kc32_dev(Hp), IMG = ggpm_split_image_halves(ROWS, Hp);
    __bf16* Ia = reinterpret_cast<__bf16*>(lds);
    __bf16* Ib = Ia + IMG;
    __bf16* Ic = Ib + IMG;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r0 = blockIdx.x * ROWS;
    const int grp = blockIdx.y;
    const int t_end = min(NT, (grp + 1) * a.tg);
    const float* const wps[3] = {a.WiT, a.WoT, a.WuT};
    std::conditional_t<GM == 0, GgpmRing<3>, GgpmNoRing> ring;
    std::conditional_t<SPLIT, GgpmSplitRing<3>, GgpmNoRing> sring;
    if constexpr (GM == 0)
        if (grp * a.tg + wave < t_end) ggpm_ring_prefetch<3>(wps, KC, grp * a.tg + wave, lane, ring);     // under the row copies
    if constexpr (SPLIT) {
        if (grp * a.tg + wave < t_end) ggpm_split_ring_prefetch<3>(wps, KC32, grp * a.tg + wave, lane, sring);
        ggpm_split_init(Ia, 3, ROWS, Hp);
        ggpm_load_rows_to_lds_split<ROWS>(a.DI, r0, a.E1, Hp, Ia, PLANE, LDH);
        ggpm_load_rows_to_lds_split<ROWS>(a.DO, r0, a.E1, Hp, Ib, PLANE, LDH);
        ggpm_load_rows_to_lds_split<ROWS>(a.DU, r0, a.E1, Hp, Ic, PLANE, LDH);
    } else {
        ggpm_load_rows_to_lds<ROWS, ST16>(a.DI, r0, a.E1, Hp, LD, Ta);
        ggpm_load_rows_to_lds<ROWS, ST16>(a.DO, r0, a.E1, Hp, LD, Tb);
        ggpm_load_rows_to_lds<ROWS, ST16>(a.DU, r0, a.E1, Hp, LD, Tc);
    }
    __syncthreads();
    for (int tt = grp * a.tg + wave; tt < t_end; tt += GGPM_NWA) {
        f32x4 acc[3][RTT];
        ggpm_zero_acc<3, RTT>(acc);
        {
            const float* const tiles[3] = {Ta, Tb, Tc};
            const int tn = tt + GGPM_NWA < t_end ? tt + GGPM_NWA : -1;
            if constexpr (SPLIT) {
                const __bf16* const imgs[3] = {Ia, Ib, Ic};
                ggpm_wave_gemm_split<3, false, true>(imgs, PLANE, LDH, wps, KC32, tt, tn, lane, acc, sring);
            } else if constexpr (BF16) ggpm_wave_gemm_bf16<3, RTT>(tiles, LD, wps, Hp, tt, lane, acc);
            else ggpm_wave_gemm_ring<3, RTT>(tiles, LD, wps, KC, tt, tn, lane, acc, ring);
        }
        const int c = 16 * tt + 4 * (lane >> 4);
#pragma unroll
        for (int r = 0; r < RTT; ++r) {
            const int e = r0 + 16 * r + (lane & 15);
            if (e < a.E1)
                ggpm_stx<ST16>(a.dSout, (size_t)e * Hp + c, ggpm_f4(acc[0][r]) + ggpm_f4(acc[1][r]) + ggpm_f4(acc[2][r]));
        }
    }
}

// What level_host.h needs to know about the LSTM (each line is a difference from the GRU; DESIGN.md 5.1 has the table).
struct LstmCell {
    static constexpr StepNeed fwd = {{3, 1, 2}, {2, 1, 1}, {1, 0, 1}};      // fused: s, fc, h' | A: s, fc | B: the h' rows
    static constexpr StepNeed bwd = {{6, 2, 4}, {3, 2, 1}, {3, 0, 3}};      // kernel B: the three gate-gradient row sets
    static constexpr int bwd_fuse_max_tiles = 0;                            // no limit beyond the LDS
    static constexpr bool rt2_bf16 = false;                                 // bf16 mode has no two-row-tile form
    static constexpr int gate_products = 3;                                 // forward [Wi; Wo; Wu].s; backward B the three dS terms
    static constexpr int timing_base = 2;                                   // ggpm_timing_begin slots 2 / 3 / 6 / 7
    static constexpr int n_mat = 4, n_stash = 3;                            // Wi, Wo, Wu, Wf; DI, DO, DU
    static constexpr int csws_rows = 0;                                     // no bias gradient here
    // ggpm_level_opts.prefer_narrow: two row tiles per workgroup for a dense fp32 level call
    static bool use_rt2(const ggpm_level_opts& o, int, int Hp, bool sparse) {
        return o.prefer_narrow && !sparse && o.gate_dtype != 1 && lds_tiles(3, Hp, 32) <= GGPM_LDS_LIMIT;
    }
    // mode 2: kernel A of the backward (two fp32 tiles + the dqf image) and kernel B of the backward (three gate-gradient images)
    static bool mode2_fits(int Hp) {
        const size_t img = ggpm_split_image_bytes(16, Hp);
        return lds_tiles(2, Hp) + img <= GGPM_LDS_LIMIT && 3 * img <= GGPM_LDS_LIMIT;
    }
    // three LDS tiles of 16 rows must fit a CU; 32-bit byte offsets inside a slot
    static bool shape_ok(int E1, int Hp) { return lds_tiles(3, Hp) <= GGPM_LDS_LIMIT && (size_t)E1 * Hp < ((size_t)1 << 30); }
};

void launch_fwd(LstmFwdArgs a, bool rt2, bool stash, bool with_b, double flops1, hipStream_t s) {
    const StepLds step = fwd_step<LstmCell>(a.Hp, a.tg, rt2, a.bf16, with_b);
    a.fuse_b = step.fuse;
    ggpm_timing_begin(LstmCell::timing_base, s, (step.fuse + (a.h0_zero ? 0 : LstmCell::gate_products)) * flops1);     // the first depth has no gate products
    for_variant<LstmCell>(a.st16, rt2, a.bf16, [&](auto GM, auto RTT, auto ST16) {
        launch_step(stash ? lstm_fwd_a<true, GM, RTT, ST16> : lstm_fwd_a<false, GM, RTT, ST16>, a, rt2, step.a, s);
    });
    ggpm_timing_end(LstmCell::timing_base, s);
    if (with_b && !step.fuse) {
        ggpm_timing_begin(LstmCell::timing_base + 4, s, 1 * flops1);
        for_variant<LstmCell>(a.st16, rt2, a.bf16, [&](auto GM, auto RTT, auto ST16) {
            launch_step(lstm_fwd_b<GM, RTT, ST16>, a, rt2, step.b, s);
        });
        ggpm_timing_end(LstmCell::timing_base + 4, s);
    }
}

void launch_bwd(LstmBwdArgs a, bool rt2, bool with_b, double flops1, hipStream_t s) {
    const StepLds step = bwd_step<LstmCell>(a.Hp, a.tg, rt2, a.bf16, with_b, a.final_pass != 0);
    a.fuse_b = step.fuse;
    ggpm_timing_begin(LstmCell::timing_base + 1, s, (step.fuse ? 1 + LstmCell::gate_products : 1) * flops1);
    for_variant<LstmCell>(a.st16, rt2, a.bf16, [&](auto GM, auto RTT, auto ST16) {
        launch_step(lstm_bwd_a<GM, RTT, ST16>, a, rt2, step.a, s);
    });
    ggpm_timing_end(LstmCell::timing_base + 1, s);
    if (with_b && !step.fuse) {
        ggpm_timing_begin(LstmCell::timing_base + 5, s, LstmCell::gate_products * flops1);
        for_variant<LstmCell>(a.st16, rt2, a.bf16, [&](auto GM, auto RTT, auto ST16) {
            launch_step(lstm_bwd_b<GM, RTT, ST16>, a, rt2, step.b, s);
        });
        ggpm_timing_end(LstmCell::timing_base + 5, s);
    }
}

}  // namespace

extern "C" size_t ggpm_lstm_pack_floats(int H) {
    return 4 * ggpm_packed_matrix_slot(ggpm_padded_hidden(H));
}

// ggpm_level_form_query (capi.hip) for an LSTM level
int ggpm_lstm_level_form(int E1, int H, int sparse, int training, const ggpm_level_opts& o, ggpm_level_form* out) {
    return level_form<LstmCell>(E1, H, sparse, training, o, out);
}

namespace {
__global__ void lstm_sparse_init_state(const float* __restrict__ h_in, const float* __restrict__ c_in,
                                       const unsigned char* __restrict__ frozen, float* __restrict__ H0,
                                       float* __restrict__ C0, int Hp) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (c >= Hp) return;
    const size_t o = (size_t)r * Hp + c;
    H0[o] = frozen[r] ? h_in[o] : 0.f;
    C0[o] = frozen[r] ? c_in[o] : 0.f;
}
}  // namespace

int lstm_forward_impl(const LevelCall& c, int save_for_backward, const ggpm_level_opts& o, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    const int E1 = c.rows, H = c.H, depth = c.depth;
    float *Hs = c.Hs, *Cs = c.Cs, *Qs = c.Qs, *wpack = c.wpack;
    const unsigned char* frozen = c.frozen;
    bool ok = E1 > 0 && H > 0 && depth > 0 && c.pred_rowptr && c.pred_col && Hs && Cs && Qs && wpack;
    for (int k = 0; k < 4; ++k) ok = ok && c.X[k] && c.W[k];
    for (int k = 0; k < 5; ++k) ok = ok && (c.St[k] || !save_for_backward);
    if (!ok) return GGPM_ERR_ARG;
    const int Hp = ggpm_padded_hidden(H);
    if (!LstmCell::shape_ok(E1, Hp)) return GGPM_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const size_t slot = (size_t)E1 * Hp;
    const LevelPlan plan = level_plan<LstmCell>(o, E1, Hp, frozen != nullptr);
    const bool rt2 = plan.rt2;
    const int bf16 = plan.gm;      // gate mode 0 / 1 / 2
    const size_t mstep = ggpm_packed_matrix_floats(Hp, bf16);
    float* pWi = wpack; float* pWo = wpack + mstep; float* pWu = wpack + 2 * mstep; float* pWf = wpack + 3 * mstep;
    {
        GgpmPackArgs pk = {};
        for (int k = 0; k < 4; ++k) { pk.W[k] = c.W[k]; pk.ldw[k] = c.ldw[k]; }
        pk.H = H; pk.Hp = Hp; pk.transpose = 0; pk.dst = wpack; pk.bias = nullptr; pk.bias_out = nullptr; pk.bf16 = bf16;
        if (!o.weights_packed) ggpm_launch_pack(pk, 4, s);
    }
    const int tg = plan.tg;
    const bool gathered = o.gather_h && o.gather_idx && frozen && o.gather_c;
    if (frozen) {      // sparse_forward: start from the caller's (h, c); qf^0 = Wf_h h^0 by one B launch
        dim3 ig(ggpm_ceil_div(Hp, 256), E1);
        // (h_in == Hs and c_in == Cs: the caller put the masked start state into slot 0 itself; ggpm_level_opts.gather_*:
        // the qf^0 launch fetches it through the index and writes slot 0 of both on the way)
        if ((c.h_in != Hs || c.c_in != Cs) && !gathered) lstm_sparse_init_state<<<ig, 256, 0, s>>>(c.h_in, c.c_in, frozen, Hs, Cs, Hp);
        LstmFwdArgs a0 = {};
        a0.E1 = E1; a0.Hp = Hp; a0.tg = tg; a0.Hnew = Hs; a0.Qnew = Qs; a0.Wf = pWf; a0.bf16 = bf16;
        if (gathered) { a0.src_h = o.gather_h; a0.src_c = o.gather_c; a0.src_idx = o.gather_idx; a0.Cnew = Cs; }
        const size_t lb = fwd_step<LstmCell>(Hp, tg, false, bf16, true).b;
        for_variant<LstmCell>(false, false, bf16, [&](auto GM, auto RTT, auto ST16) {
            launch_step(lstm_fwd_b<GM, RTT, ST16>, a0, false, lb, s);
        });
    } else {
        (void)hipMemsetAsync(Hs, 0, slot * sizeof(float), s);
        (void)hipMemsetAsync(Cs, 0, slot * sizeof(float), s);
        (void)hipMemsetAsync(Qs, 0, slot * sizeof(float), s);
    }

    const double flops1 = 2.0 * (double)(E1 - 1) * H * H;   // algorithmic flops of ONE gate product
    // forward-only form (ggpm_level_opts.h_out): the training forward's steps and roundings, without stashes
    const bool infer = !save_for_backward && o.h_out;
    int run_depth = o.run_depth;
    if (run_depth <= 0 || run_depth > depth || frozen || !(save_for_backward || infer)) run_depth = depth;
    // bf16 storage (tile_mma.h): bf16 gate products, dense, training, every stash contraction on the bf16 tall kernel
    const bool st16 = ggpm_level_st16(bf16, frozen != nullptr, save_for_backward || infer, E1, H);
    // fixed-point level (ggpm_level_opts.fixed_slot): only the last step's stash slot is ever read
    const int fs = (o.fixed_slot > 0 && save_for_backward && !frozen && !st16) ? o.fixed_slot : 0;
    if (fs && fs != run_depth) return GGPM_ERR_ARG;
    for (int t = 1; t <= run_depth; ++t) {
        const bool stash = save_for_backward && (!fs || t == fs);
        LstmFwdArgs a = {};
        a.E1 = E1; a.Hp = Hp; a.tg = tg; a.Xi = c.X[0]; a.Xo = c.X[1]; a.Xu = c.X[2]; a.Xf = c.X[3];
        a.Wi = pWi; a.Wo = pWo; a.Wu = pWu; a.Wf = pWf; a.rowptr = c.pred_rowptr; a.col = c.pred_col;
        a.frozen = frozen;
        a.bf16 = bf16;
        a.st16 = st16 ? 1 : 0;
        a.h0_zero = (t == 1 && !frozen) ? 1 : 0;
        if (save_for_backward) {
            a.Hprev = ggpm_slot_ptr(Hs, t - 1, slot, st16); a.Hnew = ggpm_slot_ptr(Hs, t, slot, st16);
            a.Hout = (st16 && t == depth) ? Hs + (size_t)depth * slot : nullptr;      // the level's result stays fp32, at its usual place
            a.Cprev = Cs + (size_t)(t - 1) * slot; a.Cnew = Cs + (size_t)t * slot;
            a.Qprev = ggpm_slot_ptr(Qs, t - 1, slot, st16); a.Qnew = (t < depth) ? ggpm_slot_ptr(Qs, t, slot, st16) : nullptr;
            a.S = ggpm_slot_ptr(c.St[0], t - 1, slot, st16); a.I = ggpm_slot_ptr(c.St[1], t - 1, slot, st16);
            a.O = ggpm_slot_ptr(c.St[2], t - 1, slot, st16); a.U = ggpm_slot_ptr(c.St[3], t - 1, slot, st16);
            a.F = c.St[4] + (size_t)(t - 1) * slot;
            if (!stash) a.S = a.I = a.O = a.U = a.F = nullptr;
        } else if (infer) {
            a.Hprev = ggpm_slot_ptr(Hs, (t - 1) & 1, slot, st16); a.Hnew = ggpm_slot_ptr(Hs, t & 1, slot, st16);
            a.Cprev = Cs + (size_t)((t - 1) & 1) * slot; a.Cnew = Cs + (size_t)(t & 1) * slot;
            a.Qprev = ggpm_slot_ptr(Qs, (t - 1) & 1, slot, st16); a.Qnew = ggpm_slot_ptr(Qs, t & 1, slot, st16);
            if (t == run_depth) {          // the level's result, fp32, where the caller wants it
                if (st16) a.Hout = o.h_out;
                else a.Hnew = o.h_out;
                if (o.c_out) a.Cnew = o.c_out;
            }
            a.S = a.I = a.O = a.U = a.F = nullptr;
        } else {
            a.Hprev = Hs + (size_t)((t - 1) & 1) * slot; a.Hnew = Hs + (size_t)(t & 1) * slot;
            a.Cprev = Cs + (size_t)((t - 1) & 1) * slot; a.Cnew = Cs + (size_t)(t & 1) * slot;
            a.Qprev = Qs + (size_t)((t - 1) & 1) * slot; a.Qnew = Qs + (size_t)(t & 1) * slot;
            a.S = a.I = a.O = a.U = a.F = nullptr;
        }
        launch_fwd(a, rt2, stash, t < depth, flops1, s);
    }
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

// the operands both forward entry points name, by the parameter names they share
#define LSTM_FORWARD_OPERANDS(c) \
    c.lstm = true; c.rows = E1; c.H = H; c.depth = depth; \
    c.X[0] = Xi; c.X[1] = Xo; c.X[2] = Xu; c.X[3] = Xf; \
    c.W[0] = Wi_h; c.ldw[0] = ld_wi; c.W[1] = Wo_h; c.ldw[1] = ld_wo; c.W[2] = Wu_h; c.ldw[2] = ld_wu; c.W[3] = Wf_h; c.ldw[3] = ld_wf; \
    c.pred_rowptr = pred_rowptr; c.pred_col = pred_col; \
    c.Hs = Hs; c.Cs = Cs; c.Qs = Qs; c.St[0] = Ss; c.St[1] = Is; c.St[2] = Os; c.St[3] = Us; c.St[4] = Fs; c.wpack = wpack;
extern "C" int ggpm_lstm_forward(int E1, int H, int depth, const float* Xi, const float* Xo, const float* Xu,
                                 const float* Xf, const float* Wi_h, int ld_wi, const float* Wo_h, int ld_wo,
                                 const float* Wu_h, int ld_wu, const float* Wf_h, int ld_wf,
                                 const int32_t* pred_rowptr, const int32_t* pred_col, float* Hs, float* Cs,
                                 float* Qs, float* Ss, float* Is, float* Os, float* Us, float* Fs,
                                 float* wpack, int save_for_backward, const ggpm_level_opts* opts, ggpm_stream_t stream) {
    LevelCall c = {};
    LSTM_FORWARD_OPERANDS(c);
    return lstm_forward_impl(c, save_for_backward, ggpm_opts_or_default(opts), stream);
}

extern "C" int ggpm_lstm_sparse_forward(int E1, int H, int depth, const float* h_in, const float* c_in,
                                        const unsigned char* frozen, const float* Xi, const float* Xo,
                                        const float* Xu, const float* Xf, const float* Wi_h, int ld_wi,
                                        const float* Wo_h, int ld_wo, const float* Wu_h, int ld_wu,
                                        const float* Wf_h, int ld_wf, const int32_t* pred_rowptr,
                                        const int32_t* pred_col, float* Hs, float* Cs, float* Qs, float* Ss,
                                        float* Is, float* Os, float* Us, float* Fs, float* wpack,
                                        int save_for_backward, const ggpm_level_opts* opts, ggpm_stream_t stream) {
    if (!h_in || !c_in || !frozen) return GGPM_ERR_ARG;
    LevelCall c = {};
    LSTM_FORWARD_OPERANDS(c);
    c.h_in = h_in; c.c_in = c_in; c.frozen = frozen;
    return lstm_forward_impl(c, save_for_backward, ggpm_opts_or_default(opts), stream);
}
#undef LSTM_FORWARD_OPERANDS

extern "C" size_t ggpm_lstm_backward_workspace_bytes(int E1, int H, int depth) {
    return backward_workspace_bytes<LstmCell>(E1, H, depth);      // (level_host.h: carve)
}

int lstm_backward_impl(const LevelCall& c, int weight_grads, const ggpm_level_opts& o, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    const int E1 = c.rows, H = c.H, depth = c.depth;
    const float *Xf = c.X[LSTM_GATES.reread], *Cs = c.Cs, *Qs = c.Qs;
    float* work = c.work;
    const unsigned char* frozen = c.frozen;
    if (o.skip_sparse_wgrads && frozen) weight_grads = 0;      // (ggpm_level_weight_grads follows)
    const bool scattered = o.scatter_h && o.scatter_idx && frozen && o.scatter_c;
    bool ok = E1 > 0 && H > 0 && depth > 0 && Xf && c.pred_rowptr && c.pred_col && c.succ_rowptr && c.succ_col && c.Hs && Cs &&
              Qs && c.d_out && work;
    for (int k = 0; k < 4; ++k) ok = ok && c.W[k] && c.dX[k] && c.dW[k];
    for (int k = 0; k < 5; ++k) ok = ok && c.St[k];
    if (!ok) return GGPM_ERR_ARG;
    if (c.work_bytes < ggpm_lstm_backward_workspace_bytes(E1, H, depth)) return GGPM_ERR_WORKSPACE;
    const int Hp = ggpm_padded_hidden(H);
    if (!LstmCell::shape_ok(E1, Hp)) return GGPM_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const size_t slot = (size_t)E1 * Hp;

    const bool skip_xsum = o.skip_x_sums && !frozen;
    const LevelPlan plan = level_plan<LstmCell>(o, E1, Hp, frozen != nullptr);
    const bool rt2 = plan.rt2;
    const int bf16 = plan.gm;      // gate mode 0 / 1 / 2
    const size_t mstep = ggpm_packed_matrix_floats(Hp, bf16);
    const LevelWork<LstmCell> wk = carve<LstmCell>(work, E1, Hp, depth);
    float* pWiT = wk.packedT; float* pWoT = pWiT + mstep; float* pWuT = pWiT + 2 * mstep; float* pWfT = pWiT + 3 * mstep;
    float* DI = wk.stash[0]; float* DO = wk.stash[1]; float* DU = wk.stash[2]; float* DQ = wk.DQ;
    float* const dSb[2] = {wk.scratch[0], wk.scratch[1]}; float* const dFb[2] = {wk.scratch[2], wk.scratch[3]};
    float* carry_h = wk.scratch[4]; float* carry_c = wk.scratch[5];
    if (o.defer_stash[0]) {       // deferred weight gradients: the stashes go to the caller's stacked buffers
        if (!frozen || !o.defer_stash[1] || !o.defer_stash[2] || !o.defer_stash[3]) return GGPM_ERR_ARG;
        DI = o.defer_stash[0]; DO = o.defer_stash[1]; DU = o.defer_stash[2]; DQ = o.defer_stash[3];
        weight_grads = 0;
    }

    {
        GgpmPackArgs pk = {};
        for (int k = 0; k < 4; ++k) { pk.W[k] = c.W[k]; pk.ldw[k] = c.ldw[k]; }
        pk.H = H; pk.Hp = Hp; pk.transpose = 1; pk.dst = pWiT; pk.bias = nullptr; pk.bias_out = nullptr; pk.bf16 = bf16;
        if (!o.weights_packed) ggpm_launch_pack(pk, 4, s);
    }
    // dXi / dXo / dXu / dXf are started (not accumulated) by the first backward depth

    const int tg = plan.tg;
    const double flops1 = 2.0 * (double)(E1 - 1) * H * H;   // algorithmic flops of ONE gate product
    // tree-side levels: d(h^t), d(c^t) vanish below step `lo` (nilpotent Jacobian, common.h)
    int lo = o.lo;
    if (lo < 1 || lo > depth || frozen) lo = 1;
    const bool st16 = ggpm_level_st16(bf16, frozen != nullptr, true, E1, H);      // (as the forward decided)
    // fixed-point level (ggpm_level_opts.fixed_slot): state slots above fs and stash slots above fs - 1 alias those
    const int fs = (o.fixed_slot > 0 && !frozen && !st16) ? o.fixed_slot : 0;
    if (fs && (fs >= depth || lo < fs)) return GGPM_ERR_ARG;      // (every slot a step >= lo reads must be the settled one)
    auto state_slot = [fs](int t) { return fs && t > fs ? fs : t; };
    auto stash_slot = [fs](int t) { return fs && t > fs ? fs - 1 : t - 1; };
    for (int t = depth; t >= lo; --t) {
        LstmBwdArgs a = {};
        a.E1 = E1; a.Hp = Hp; a.tg = tg; a.first = (t == depth);
        a.st16 = st16 ? 1 : 0;
        a.Xf = Xf;
        a.Ccur = Cs + (size_t)state_slot(t) * slot;
        a.Qcur = (t < depth) ? ggpm_slot_ptr(Qs, state_slot(t), slot, st16) : nullptr;
        a.F = c.St[4] + (size_t)stash_slot(t) * slot;
        a.I = ggpm_slot_ptr(c.St[1], stash_slot(t), slot, st16); a.O = ggpm_slot_ptr(c.St[2], stash_slot(t), slot, st16);
        a.U = ggpm_slot_ptr(c.St[3], stash_slot(t), slot, st16);
        a.dHD = c.d_out;
        a.dSin = dSb[(t + 1) & 1]; a.dFCin = dFb[(t + 1) & 1];
        a.dSout = dSb[t & 1]; a.dFCout = dFb[t & 1];
        a.DQ = (t < depth) ? ggpm_slot_ptr(DQ, t, slot, st16) : nullptr;
        a.frozen = frozen; a.dCD = c.dc_out; a.carry_h = carry_h; a.carry_c = carry_c; a.final_pass = 0;
        a.dHin = nullptr; a.dCin = nullptr;
        a.DI = ggpm_slot_ptr(DI, t - 1, slot, st16); a.DO = ggpm_slot_ptr(DO, t - 1, slot, st16);
        a.DU = ggpm_slot_ptr(DU, t - 1, slot, st16);
        a.dXi = c.dX[0]; a.dXo = c.dX[1]; a.dXu = c.dX[2]; a.dXf = c.dX[3];
        a.WiT = pWiT; a.WoT = pWoT; a.WuT = pWuT; a.WfT = pWfT; a.bf16 = bf16;
        a.srowptr = c.succ_rowptr; a.scol = c.succ_col;
        a.skip_xsum = skip_xsum ? 1 : 0;
        launch_bwd(a, rt2, t > 1 || frozen != nullptr, flops1, s);
    }
    GGPM_CHECK_LAUNCH();
    if (frozen) {      // gradient of the incoming (h, c): one more gather + dqf.Wf_h launch at t = 0
        LstmBwdArgs a = {};
        a.E1 = E1; a.Hp = Hp; a.tg = tg; a.first = 0; a.final_pass = 1;
        a.Xf = Xf; a.Ccur = Cs; a.Qcur = Qs;
        a.dSin = dSb[1]; a.dFCin = dFb[1];          // written by the launches of depth 1
        a.DQ = DQ; a.WfT = pWfT; a.srowptr = c.succ_rowptr; a.scol = c.succ_col; a.bf16 = bf16;
        a.frozen = frozen; a.carry_h = carry_h; a.carry_c = carry_c; a.dHin = c.d_in; a.dCin = c.dc_in;
        if (scattered) { a.scat_h = o.scatter_h; a.scat_c = o.scatter_c; a.scat_idx = o.scatter_idx; }
        launch_bwd(a, rt2, false, flops1, s);
        GGPM_CHECK_LAUNCH();
    }

    if (!weight_grads) return GGPM_OK;
    return lstm_weight_grads_impl(c, lo, o, stream);
}

// where ggpm_lstm_backward left its di_pre / do_pre / du_pre stashes inside `work` (slot t-1 of each = backward step t)
extern "C" int ggpm_lstm_backward_stashes(float* work, int E1, int H, int depth, float** DI, float** DO, float** DU) {
    if (!work || !DI || !DO || !DU || E1 <= 0 || H <= 0 || depth <= 0) return GGPM_ERR_ARG;
    const LevelWork<LstmCell> wk = carve<LstmCell>(work, E1, ggpm_padded_hidden(H), depth);
    *DI = wk.stash[0];
    *DO = wk.stash[1];
    *DU = wk.stash[2];
    return GGPM_OK;
}

// the operands both backward entry points name, by the parameter names they share
#define LSTM_BACKWARD_OPERANDS(c) \
    c.lstm = true; c.rows = E1; c.H = H; c.depth = depth; \
    c.X[LSTM_GATES.reread] = Xf; \
    c.W[0] = Wi_h; c.ldw[0] = ld_wi; c.W[1] = Wo_h; c.ldw[1] = ld_wo; c.W[2] = Wu_h; c.ldw[2] = ld_wu; c.W[3] = Wf_h; c.ldw[3] = ld_wf; \
    c.pred_rowptr = pred_rowptr; c.pred_col = pred_col; c.succ_rowptr = succ_rowptr; c.succ_col = succ_col; \
    c.Hs = level_read(Hs); c.Cs = level_read(Cs); c.Qs = level_read(Qs); \
    c.St[0] = level_read(Ss); c.St[1] = level_read(Is); c.St[2] = level_read(Os); c.St[3] = level_read(Us); c.St[4] = level_read(Fs); \
    c.d_out = dHD; c.dX[0] = dXi; c.dX[1] = dXo; c.dX[2] = dXu; c.dX[3] = dXf; \
    c.dW[0] = dWi_h; c.ld_dw[0] = ld_dwi; c.dW[1] = dWo_h; c.ld_dw[1] = ld_dwo; c.dW[2] = dWu_h; c.ld_dw[2] = ld_dwu; \
    c.dW[3] = dWf_h; c.ld_dw[3] = ld_dwf; \
    c.work = work; c.work_bytes = work_bytes;
extern "C" int ggpm_lstm_backward(int E1, int H, int depth, const float* Xf, const float* Wi_h, int ld_wi,
                                  const float* Wo_h, int ld_wo, const float* Wu_h, int ld_wu, const float* Wf_h,
                                  int ld_wf, const int32_t* pred_rowptr, const int32_t* pred_col,
                                  const int32_t* succ_rowptr, const int32_t* succ_col, const float* Hs,
                                  const float* Cs, const float* Qs, const float* Ss, const float* Is,
                                  const float* Os, const float* Us, const float* Fs, const float* dHD, float* dXi,
                                  float* dXo, float* dXu, float* dXf, float* dWi_h, int ld_dwi, float* dWo_h,
                                  int ld_dwo, float* dWu_h, int ld_dwu, float* dWf_h, int ld_dwf, float* work,
                                  size_t work_bytes, int weight_grads, const ggpm_level_opts* opts, ggpm_stream_t stream) {
    LevelCall c = {};
    LSTM_BACKWARD_OPERANDS(c);
    return lstm_backward_impl(c, weight_grads, ggpm_opts_or_default(opts), stream);
}

// sparse_forward backward: takes dL/dh_D and dL/dc_D, additionally returns dHin / dCin (zero on the recomputed rows)
extern "C" int ggpm_lstm_sparse_backward(int E1, int H, int depth, const unsigned char* frozen, const float* Xf,
                                         const float* Wi_h, int ld_wi, const float* Wo_h, int ld_wo,
                                         const float* Wu_h, int ld_wu, const float* Wf_h, int ld_wf,
                                         const int32_t* pred_rowptr, const int32_t* pred_col,
                                         const int32_t* succ_rowptr, const int32_t* succ_col, const float* Hs,
                                         const float* Cs, const float* Qs, const float* Ss, const float* Is,
                                         const float* Os, const float* Us, const float* Fs, const float* dHD,
                                         const float* dCD, float* dHin, float* dCin, float* dXi, float* dXo,
                                         float* dXu, float* dXf, float* dWi_h, int ld_dwi, float* dWo_h, int ld_dwo,
                                         float* dWu_h, int ld_dwu, float* dWf_h, int ld_dwf, float* work,
                                         size_t work_bytes, const ggpm_level_opts* opts, ggpm_stream_t stream) {
    if (!frozen || !dHin || !dCin) return GGPM_ERR_ARG;
    LevelCall c = {};
    LSTM_BACKWARD_OPERANDS(c);
    c.frozen = frozen; c.dc_out = dCD; c.d_in = dHin; c.dc_in = dCin;
    return lstm_backward_impl(c, 1, ggpm_opts_or_default(opts), stream);
}
#undef LSTM_BACKWARD_OPERANDS

// Weight gradients of the LSTM message function from the stashes ggpm_lstm_backward left in `work` (sparse: dqf^0 included).
int lstm_weight_grads_impl(const LevelCall& c, int lo, const ggpm_level_opts& o, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    const int E1 = c.rows, H = c.H, depth = c.depth;
    const bool with_slot0 = c.frozen != nullptr;
    if (E1 <= 0 || H <= 0 || depth <= 0 || !c.Hs || !c.St[0] || !c.work || !c.dW[0] || !c.dW[1] || !c.dW[2] || !c.dW[3])
        return GGPM_ERR_ARG;
    if (lo < 1 || lo > depth || with_slot0) lo = 1;       // backward steps depth .. lo ran (stash slots lo-1 .. depth-1)
    if (c.work_bytes < ggpm_lstm_backward_workspace_bytes(E1, H, depth)) return GGPM_ERR_WORKSPACE;
    const LevelWork<LstmCell> wk = carve<LstmCell>(c.work, E1, ggpm_padded_hidden(H), depth);
    // dW*_h = D*^T S for the i / o / u gates, dWf_h = DQ^T h (dqf^t pairs with h^t)
    WgradTerm gate[3];
    for (int k = 0; k < 3; ++k) gate[k] = {wk.stash[k], c.St[0], c.dW[k], c.ld_dw[k]};
    return level_weight_grads(E1, H, depth, lo, with_slot0, o, 3, gate, {wk.DQ, c.Hs, c.dW[3], c.ld_dw[3]}, nullptr, nullptr,
                              wk.skws, wk.skbytes(c.work_bytes), stream);
}

// The hidden-half weight gradients of MANY sparse backward calls at once (see ggpm_gru_weight_grads_stacked).
extern "C" int ggpm_lstm_weight_grads_stacked(int rows, int rows_q, int H, const float* DI, const float* DO,
                                              const float* DU, const float* Ss, const float* DQ, const float* Hs,
                                              float* dWi_h, int ld_dwi, float* dWo_h, int ld_dwo, float* dWu_h, int ld_dwu,
                                              float* dWf_h, int ld_dwf, float* work, size_t work_bytes,
                                              ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (rows <= 0 || rows_q <= 0 || H <= 0 || !DI || !DO || !DU || !Ss || !DQ || !Hs || !dWi_h || !dWo_h || !dWu_h ||
        !dWf_h || !work)
        return GGPM_ERR_ARG;
    if (work_bytes < ggpm_weight_grads_stacked_workspace_bytes(H, rows > rows_q ? rows : rows_q)) return GGPM_ERR_WORKSPACE;
    const int Hp = ggpm_padded_hidden(H);
    float* skws = work + (size_t)256 * Hp;
    const size_t skbytes = work_bytes - (size_t)256 * Hp * sizeof(float);
    const WgradTerm gate[3] = {{DI, Ss, dWi_h, ld_dwi}, {DO, Ss, dWo_h, ld_dwo}, {DU, Ss, dWu_h, ld_dwu}};
    return tall_weight_grads(H, Hp, 3, gate, rows, {DQ, Hs, dWf_h, ld_dwf}, rows_q, nullptr, nullptr, false, 0, skws, skbytes, stream);
}

extern "C" int ggpm_lstm_weight_grads(int E1, int H, int depth, const float* Hs, const float* Ss, float* work,
                                      size_t work_bytes, float* dWi_h, int ld_dwi, float* dWo_h, int ld_dwo,
                                      float* dWu_h, int ld_dwu, float* dWf_h, int ld_dwf, const ggpm_level_opts* opts,
                                      ggpm_stream_t stream) {
    LevelCall c = {};
    c.lstm = true; c.rows = E1; c.H = H; c.depth = depth;
    c.Hs = level_read(Hs); c.St[0] = level_read(Ss);
    c.dW[0] = dWi_h; c.ld_dw[0] = ld_dwi; c.dW[1] = dWo_h; c.ld_dw[1] = ld_dwo; c.dW[2] = dWu_h; c.ld_dw[2] = ld_dwu;
    c.dW[3] = dWf_h; c.ld_dw[3] = ld_dwf;
    c.work = work; c.work_bytes = work_bytes;
    return ggpm_level_weight_grads(c, opts, stream);
}
