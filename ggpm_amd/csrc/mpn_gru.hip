// Fused GRU message step for gfx950 -- the hot loop of the hierarchical encoder.
//
// Reference arithmetic: GRU.forward / GRU.GRU (ggpm/rnn.py:41-50, 25-39) + index_select_ND
// (ggpm/nnutils.py:65-70).  Restated over CSR predecessor lists with the x-halves of W_z/W_r/W_h hoisted
// out of the depth loop and U_r applied once per message (q = U_r h + b_u) instead of once per padded slot.
//
// Geometry (tile_mma.h): grid = (16-row message tiles) x (column groups of `tg` output tiles), 16 waves per workgroup.
// Per depth, forward:
//   kernel A  P1  CSR gather of predecessor rows (h_p, q_p) -> s, g tiles in LDS (one wave per row, 16 B per lane,
//                 hardware exp2/rcp sigmoid; the stash stores drain under the GEMM: LDS-only barrier)
//             P2  gate GEMMs on MFMA f32 16x16x4:  Wz_h . s  and  Wh_h . g  (weights streamed packed from L2)
//                 + fused gate math -> h'
//             P3  only when the level has ONE column group (the workgroup then holds the complete h' rows):
//                 q' = U_r h' + b_u from an LDS tile -- no second launch
//   kernel B  otherwise: q' = U_r h' + b_u with the h' rows re-read from L2
// Backward mirrors it (gather over SUCCESSORS through the transposed CSR, so no atomics):
//   kernel A  P1  dq, dh-partial tiles from successors   P2  dh = partial + dq.U_r ; gate derivatives
//             P3  (one column group) dG = dm_pre.Wh_h, dS = ds_dir + dz_pre.Wz_h, dXr += dG * R
//   kernel B  otherwise the same products from rows re-read from L2
// Weight gradients are three tall split-K GEMMs over the [depth*E1, Hp] stashes (gemm.hip), issued by the caller
// on a second stream.  sparse_forward (rows with a `frozen` mask) reuses the same kernels.
#include "tile_mma.h"
#include "level_host.h"
#include "level_call.h"
#include <cstdlib>
#include <cstdio>

__global__ void ggpm_pack_weight_kernel(GgpmPackArgs a) {
    const int Hp = a.Hp, H = a.H, KC = Hp / 16;
    const int lane = threadIdx.x;            // 64
    const int kc = blockIdx.x, t = blockIdx.y, m = blockIdx.z;
    const float* __restrict__ W = a.W[m];
    const int ldw = a.ldw[m];
    const int out = 16 * t + (lane & 15);
    if (a.bf16 == 2) {                       // three bf16 planes (ggpm_wave_gemm_split); grid.x = kc32(Hp) chunks of 32 columns
        const int KC32 = ggpm_kc32_dev(Hp);
        float x[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = 32 * kc + 8 * (lane >> 4) + i;
            x[i] = (out < H && k < H) ? (a.transpose ? W[(size_t)k * ldw + out] : W[(size_t)out * ldw + k]) : 0.f;
        }
        uint2 lo[3], hi[3];
        ggpm_split3(make_float4(x[0], x[1], x[2], x[3]), lo[0], lo[1], lo[2]);
        ggpm_split3(make_float4(x[4], x[5], x[6], x[7]), hi[0], hi[1], hi[2]);
        __bf16* dst = reinterpret_cast<__bf16*>(a.dst) + (size_t)m * 2 * ggpm_packed_matrix_floats(Hp, 2);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
            *reinterpret_cast<uint4*>(dst + ggpm_pack_index_split(t, kc, KC32, pl, lane)) = make_uint4(lo[pl].x, lo[pl].y, hi[pl].x, hi[pl].y);
        if (a.bias && m == 0 && t == 0 && kc * 64 + lane < Hp) {
            const int c = kc * 64 + lane;
            a.bias_out[c] = (c < H) ? a.bias[c] : 0.f;
        }
        return;
    }
    if (a.bf16) {                            // grid.x = kc32(Hp) chunks of 32 columns
        const int KC32 = ggpm_kc32_dev(Hp);
        bf16x8 v;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = 32 * kc + 8 * (lane >> 4) + i;
            float x = 0.f;
            if (out < H && k < H) x = a.transpose ? W[(size_t)k * ldw + out] : W[(size_t)out * ldw + k];
            v[i] = (__bf16)x;
        }
        __bf16* dst = reinterpret_cast<__bf16*>(a.dst) + (size_t)m * Hp * 32 * KC32;
        *reinterpret_cast<bf16x8*>(dst + ggpm_pack_index_bf16(t, kc, KC32, lane)) = v;
        if (a.bias && m == 0 && t == 0 && kc * 64 + lane < Hp) {
            const int c = kc * 64 + lane;
            a.bias_out[c] = (c < H) ? a.bias[c] : 0.f;
        }
        return;                              // (kc32 * 64 >= Hp: the blocks above cover every bias column)
    }
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = 16 * kc + 4 * (lane >> 4) + i;
        float x = 0.f;
        if (out < H && k < H) x = a.transpose ? W[(size_t)k * ldw + out] : W[(size_t)out * ldw + k];
        v[i] = x;
    }
    ggpm_st4(a.dst + (size_t)m * Hp * Hp + ggpm_pack_index(t, kc, KC, lane), make_float4(v[0], v[1], v[2], v[3]));
    // optional bias pad (once, by the first block row of matrix 0)
    if (a.bias && m == 0 && t == 0 && kc * 64 + lane < Hp) {
        const int c = kc * 64 + lane;
        a.bias_out[c] = (c < H) ? a.bias[c] : 0.f;
    }
}

void ggpm_launch_pack(const GgpmPackArgs& a, int nmat, hipStream_t s) {
    dim3 grid(a.bf16 ? ggpm_kc32(a.Hp) : a.Hp / 16, a.Hp / 16, nmat);
    ggpm_pack_weight_kernel<<<grid, 64, 0, s>>>(a);
}

namespace {

#ifndef GGPM_GATHER_U
#define GGPM_GATHER_U 2            // predecessor rows gathered per trip of the forward gather (null slots read row 0;
                                   // 4 per trip measured equal on the atom level, 1.3 us slower on the tree levels)
#endif
constexpr int RT = 1;              // row tiles (of 16 messages) per workgroup (default; the kernels take it as RTT)
constexpr int ROWS = RT * 16;
// RTT = 2 (32 message rows per workgroup): every weight fragment a wave streams from L2 then feeds TWO row tiles, which
// halves the weight stream of a level -- at H = 600 with ~950 row tiles (configs[4]) every workgroup reads all 3 Hp^2 packed
// weights per launch, 4.2 GB in total, and that stream, not the matrix pipe, bounds the launch.  Two tiles of 32 rows
// fill the LDS, so there is no room for the fused q' / dS,dG phase: those levels use the B launches.
constexpr int GGPM_RT2_MIN_ROW_TILES = 512;

struct GruFwdArgs {
    int E1, Hp, tg;                // tg: output tiles per column group of kernel A
    const float *Xz, *Xr, *Xh;
    const float *Hprev, *Qprev;
    float *Hnew, *Qnew;
    float *S, *G, *Z, *M, *R;      // stash slot of this depth (nullptr when not saving)
    const float *Wz, *Wh, *Ur;     // packed
    const float* bu;               // [Hp] zero padded
    const int32_t *rowptr, *col;
    int ablate;                    // timing experiments only (GGPM_ABLATE): 1 no gather, 2 no GEMM
    const unsigned char* frozen;   // sparse_forward only: rows with frozen[row] != 0 keep their state (h' = h)
    int fuse_b;                    // single column group: kernel A also forms q' = U_r h' + b_u (no B launch)
    unsigned long long* dbg;       // optional phase stamps of workgroup (0,0) (GGPM_ADEBUG; dev only)
    int bf16;                      // gate mode: 0 fp32 MFMA, 1 bf16 operands (packed weights are bf16 fragments), 2 fp32 on
                                   // split operands (three bf16 planes per operand, tile_mma.h)
    int st16;                      // bf16 storage of Hs / Qs / S / G / Z / M (gate mode 1, large dense training levels; tile_mma.h)
    int h0_zero;                   // first depth of a dense level: h^0 = 0, so s = g = 0 without a gather and the gate
                                   // products vanish (h^1 = sigmoid(x_z) tanh(x_h)); H^0 / Q^0 are neither built nor read
    float* Hout;                   // bf16 storage only: where the LAST depth also writes h' in fp32 (the level's result)
    const float* src_h;            // kernel B of a sparse forward's q^0 launch (ggpm_level_opts.gather_*): row r of the
    const int32_t* src_idx;        // start state is src_h[src_idx[r]] (zero when < 0); the launch writes it to Hnew itself
    // K-split q' (ggpm_level_opts.q_part; gru_fwd_a_ks / gru_fwd_b_ks): blocks of [groups][E1][Hp] partial q rows
    float* Qpart_out;              // kernel A: where column group `grp` stores U_r[:, its k chunks] h'[its columns] (group 0: + b_u); null: none
    const float* Qpart_in;         // kernel A: the previous step's partials, which the gather adds in group order in place of Qprev rows
    float* Qsum;                   // ... and their sums for this workgroup's rows and columns (the Qs slot of the previous step; null: not kept)
    int groups;                    // column groups (kernel B: q' as the sum of the groups' K slices, bit for bit what the partials add up to)
};

// ---- K-split q': the product of one K slice [k0, k1) of a packed matrix with the matching columns of an LDS tile.
constexpr int GGPM_KS_MAXG = GGPM_KSPLIT_MAX_GROUPS;
// fragments of chunks k0 .. k0 + 3 of tile t (past the slice: its last chunk again, unused)
__device__ __forceinline__ void ggpm_slice_head(const float* wp, int KC, int t, int k0, int k1, int lane, f32x4 (&r)[4]) {
#pragma unroll
    for (int d = 0; d < 4; ++d)
        r[d] = *reinterpret_cast<const f32x4*>(wp + ggpm_pack_index(t, min(k0 + d, k1 - 1), KC, lane));
}
// acc += Wp(tile t)[:, chunks k0 .. k1) x tile[:, those columns]^T, chunk by chunk in ascending order (the order is the result:
// kernel A's partials and kernel B's slices run this same chain).  `head` holds the slice's first four fragments
// (ggpm_slice_head) and is left holding those of slice [k0n, k1n) of tile tn (tn < 0: nothing), loaded a slice ahead.
__device__ __forceinline__ void ggpm_wave_gemm_slice(const float* tile, int LD, const float* wp, int KC, int t, int k0, int k1,
                                                     int tn, int k0n, int k1n, int lane, f32x4& acc, f32x4 (&head)[4]) {
    const int boff = (lane & 15) * LD + 4 * (lane >> 4);
    for (int kb = k0; kb < k1; kb += 4) {
        f32x4 nxt[4];
        const bool more = kb + 4 < k1;
        if (more) ggpm_slice_head(wp, KC, t, kb + 4, k1, lane, nxt);
        else if (tn >= 0) ggpm_slice_head(wp, KC, tn, k0n, k1n, lane, nxt);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            if (kb + d < k1) {
                const f32x4 b = *reinterpret_cast<const f32x4*>(tile + boff + (kb + d) * 16);
#pragma unroll
                for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(head[d][s], b[s], acc, 0, 0, 0);
            }
        }
        if (more || tn >= 0) {
#pragma unroll
            for (int d = 0; d < 4; ++d) head[d] = nxt[d];
        }
    }
}

__global__ void pad_bias(const float* __restrict__ b, int H, int Hp, float* __restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < Hp) out[c] = (c < H) ? b[c] : 0.f;
}

__device__ __forceinline__ float4 one_minus(float4 r) { return make_float4(1.f - r.x, 1.f - r.y, 1.f - r.z, 1.f - r.w); }

// ---------------------------------------------------------------------------------------------- forward
// Kernel A (16 waves): every wave gathers one message row at a time (full Hp width: two 256-column sweeps
// and 4 predecessor rows in flight -> 16 independent 16-byte loads per lane), then the first `tg` waves run
// the gate GEMMs of their output tile and the gate math.
template <bool STASH, int GM, int RTT, bool ST16 = false>
__global__ void GGPM_A_BOUNDS gru_fwd_a(GruFwdArgs a) {
    constexpr int ROWS = RTT * 16;
    constexpr bool BF16 = GM == 1, SPLIT = GM == 2;
    static_assert(!SPLIT || RTT == 1, "split operands: one row tile per workgroup");
    static_assert(!ST16 || GM == 1, "bf16 storage goes with bf16 gate products");      // Hs, Qs, S, G, Z, M in bf16 (tile_mma.h)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int Hp = a.Hp, LD = Hp + 4, KC = Hp / 16, NT = Hp / 16;
    float* Ts = lds;
    float* Tg = lds + ROWS * LD;
    // split operands: Ts stays (the epilogue reads s in fp32); behind it the bf16 images of s, g and (fused q') h'
    const int LDH = ggpm_split_ldh(Hp), PLANE = ROWS * LDH, KC32 = ggpm_kc32_dev(Hp);
    const int IMG = ggpm_split_image_halves(ROWS, Hp);
    __bf16* Is = reinterpret_cast<__bf16*>(lds + ROWS * LD);
    __bf16* Ig = Is + IMG;
    __bf16* Ih = Ig + IMG;
    if constexpr (SPLIT) ggpm_split_init(Is, a.fuse_b ? 3 : 2, ROWS, Hp);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r0 = blockIdx.x * ROWS;
    const int grp = blockIdx.y;
    const int t = grp * a.tg + wave;              // this wave's output tile (if wave < tg)
    const bool dbg_on = a.dbg && blockIdx.x == 1 && blockIdx.y == 0 && threadIdx.x == 0;
    if (dbg_on) a.dbg[0] = wall_clock64();
    const bool dbg15 = a.dbg && blockIdx.x == 1 && blockIdx.y == 0 && threadIdx.x == 15 * 64;
    if (dbg15) a.dbg[5] = wall_clock64();

    // ---- P1: gather
    for (int lr = wave; lr < ROWS; lr += GGPM_NWA) {
        const int row = r0 + lr;
        GgpmRowList rl;
        if (a.h0_zero) { rl.lo = 0; rl.n = 0; } else rl = ggpm_row_list(a.rowptr, row, a.E1);
        if (a.ablate & 1) rl.n = 0;
        const size_t rowo = (size_t)(row < a.E1 ? row : 0) * Hp;
        for (int c0 = 0; c0 < Hp; c0 += 512) {
            int c[2], cs[2];
            bool on[2];
            float4 s[2], g[2], rc[2], xr[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                c[k] = c0 + 256 * k + lane * 4;
                on[k] = c[k] < Hp;
                cs[k] = on[k] ? c[k] : 0;      // lanes past the row end re-read column 0 (no branch), store nothing
                s[k] = ggpm_zero4(); g[k] = ggpm_zero4(); rc[k] = ggpm_zero4();
                xr[k] = ggpm_ld4(a.Xr + rowo + cs[k]);
            }
            for (int base = 0; base < rl.n; base += 64) {
                const int chunk = ggpm_list_chunk(a.col, rl, base, lane);
                const int m = min(64, rl.n - base);
                for (int j = 0; j < m; j += GGPM_GATHER_U) {
                    float4 h[GGPM_GATHER_U][2], q[GGPM_GATHER_U][2];
#pragma unroll
                    for (int u = 0; u < GGPM_GATHER_U; ++u) {
                        const size_t p = (size_t)ggpm_list_at(chunk, j + u, m) * Hp;
#pragma unroll
                        for (int k = 0; k < 2; ++k) {
                            h[u][k] = ggpm_ldx<ST16>(a.Hprev, p + cs[k]);
                            q[u][k] = ggpm_ldx<ST16>(a.Qprev, p + cs[k]);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < GGPM_GATHER_U; ++u)
#pragma unroll
                        for (int k = 0; k < 2; ++k) {          // null slots: h[0] == 0 contributes nothing
                            const float4 r = ggpm_fsigmoid4<BF16>(xr[k] + q[u][k]);
                            const float4 rh = r * h[u][k];
                            s[k] = s[k] + h[u][k];
                            g[k] = g[k] + rh;
                            rc[k] = rc[k] + rh * one_minus(r);
                        }
                }
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (!on[k]) continue;
                if constexpr (ST16) s[k] = ggpm_rne4(s[k]);      // what the stash holds is what the epilogue below uses
                ggpm_st4(Ts + lr * LD + c[k], s[k]);
                if constexpr (SPLIT) {
                    ggpm_split_store(Is, PLANE, LDH, lr, c[k], s[k]);
                    ggpm_split_store(Ig, PLANE, LDH, lr, c[k], g[k]);
                } else {
                    ggpm_st4(Tg + lr * LD + c[k], g[k]);
                }
                if (STASH && row < a.E1 && (c[k] >> 4) / a.tg == grp) {
                    const size_t o = (size_t)row * Hp + c[k];
                    ggpm_stx<ST16>(a.S, o, s[k]);
                    ggpm_stx<ST16>(a.G, o, g[k]);
                    ggpm_st4(a.R + o, rc[k]);     // sum_p h_p r(1-r): lets the backward form dXr without a gather
                }
            }
        }
    }

    if (dbg_on) a.dbg[1] = wall_clock64();
    if (dbg15) a.dbg[6] = wall_clock64();
    // the first weight fragments of P2 travel from L2 while this wave waits for the slower gatherers
    const int t_end = min(NT, (grp + 1) * a.tg);
    const bool p2_gemm = !(a.ablate & 2) && !a.h0_zero;
    const float* const wps2[2] = {a.Wz, a.Wh};
    std::conditional_t<GM == 0, GgpmRing<2>, GgpmNoRing> ring2;
    std::conditional_t<SPLIT, GgpmSplitRing<2>, GgpmNoRing> sring2;
    if constexpr (GM == 0)
        if (p2_gemm && t < t_end) ggpm_ring_prefetch<2>(wps2, KC, t, lane, ring2);
    if constexpr (SPLIT)
        if (p2_gemm && t < t_end) ggpm_split_ring_prefetch<2>(wps2, KC32, t, lane, sring2);
    ggpm_lds_barrier();      // LDS tiles only: the stash stores above finish under the GEMM
    if (dbg_on) a.dbg[2] = wall_clock64();

    // ---- P2: gate GEMMs + gate math for this wave's tiles (wave, wave+16, ... inside the column group)
    const int lr = lane & 15;
    for (int tt = t; tt < t_end; tt += GGPM_NWA) {
        const int c = 16 * tt + 4 * (lane >> 4);
        float4 xz[RTT], xh[RTT];
        auto load_inputs = [&]() {
#pragma unroll
            for (int r = 0; r < RTT; ++r) {
                const int row = r0 + 16 * r + lr;
                const size_t o = (size_t)(row < a.E1 ? row : 0) * Hp + c;
                xz[r] = ggpm_ld4(a.Xz + o);
                xh[r] = ggpm_ld4(a.Xh + o);
            }
        };
        if constexpr (RTT == 1) load_inputs();      // in flight under the GEMM (two row tiles: the registers go to the GEMM)
        f32x4 acc[2][RTT];
        ggpm_zero_acc<2, RTT>(acc);
        if (p2_gemm) {
            const float* const tiles[2] = {Ts, Tg};
            const int tn = tt + GGPM_NWA < t_end ? tt + GGPM_NWA : -1;
            if constexpr (SPLIT) {
                const __bf16* const imgs[2] = {Is, Ig};
                ggpm_wave_gemm_split<2>(imgs, PLANE, LDH, wps2, KC32, tt, tn, lane, acc, sring2);
            } else if constexpr (BF16) ggpm_wave_gemm_bf16<2, RTT>(tiles, LD, wps2, Hp, tt, lane, acc);
            else ggpm_wave_gemm_ring<2, RTT>(tiles, LD, wps2, KC, tt, tn, lane, acc, ring2);
        }
        if constexpr (RTT != 1) load_inputs();
        if (dbg_on) a.dbg[3] = wall_clock64();
#pragma unroll
        for (int r = 0; r < RTT; ++r) {
            const int lrow = 16 * r + lr, row = r0 + lrow;
            const size_t o = (size_t)(row < a.E1 ? row : 0) * Hp + c;
            float4 h = ggpm_zero4(), z = ggpm_zero4(), m = ggpm_zero4();
            auto keep_h = [&](float4 v) {          // the complete h' rows for the fused q' phase
                if constexpr (SPLIT) ggpm_split_store(Ih, PLANE, LDH, lrow, c, v);
                else ggpm_st4(lds + 2 * ROWS * LD + lrow * LD + c, v);
            };
            if (row >= a.E1) {
                if (a.fuse_b) keep_h(h);
                continue;
            }
            if (a.frozen && a.frozen[row]) {
                h = ggpm_ld4(a.Hprev + o);             // z = m = 0 in the stash => the backward passes dh through
            } else if (row != 0 || a.frozen) {
                const float4 s = ggpm_ld4(Ts + lrow * LD + c);
                const float4 pz = ggpm_f4(acc[0][r]) + xz[r], pm = ggpm_f4(acc[1][r]) + xh[r];
                z = ggpm_sigmoid4(pz);
                m = make_float4(tanhf(pm.x), tanhf(pm.y), tanhf(pm.z), tanhf(pm.w));
                if constexpr (ST16) { z = ggpm_rne4(z); m = ggpm_rne4(m); }
                h = make_float4((1.f - z.x) * s.x + z.x * m.x, (1.f - z.y) * s.y + z.y * m.y,
                                (1.f - z.z) * s.z + z.z * m.z, (1.f - z.w) * s.w + z.w * m.w);
                if constexpr (ST16) h = ggpm_rne4(h);
            }
            ggpm_stx<ST16>(a.Hnew, o, h);
            if constexpr (ST16) if (a.Hout) ggpm_st4(a.Hout + o, h);      // the level's result (last depth) also in fp32
            if (a.fuse_b) keep_h(h);
            if (STASH) {
                ggpm_stx<ST16>(a.Z, o, z);
                ggpm_stx<ST16>(a.M, o, m);
            }
        }
    }
    if (dbg_on) a.dbg[4] = wall_clock64();
    if (!a.fuse_b) return;

    // ---- P3 (single column group, RTT = 1 only): the workgroup holds the complete h' rows -> q' = U_r h' + b_u
    if constexpr (RTT == 1) {
        const int row = r0 + lr;
        const float* const wps3[1] = {a.Ur};
        std::conditional_t<GM == 0, GgpmRing<1>, GgpmNoRing> ring3;
        std::conditional_t<SPLIT, GgpmSplitRing<1>, GgpmNoRing> sring3;
        if constexpr (GM == 0)
            if (wave < NT) ggpm_ring_prefetch<1>(wps3, KC, wave, lane, ring3);
        if constexpr (SPLIT)
            if (wave < NT) ggpm_split_ring_prefetch<1>(wps3, KC32, wave, lane, sring3);
        ggpm_lds_barrier();
        const float* Th = lds + 2 * ROWS * LD;
        for (int tt = wave; tt < NT; tt += GGPM_NWA) {
            const int c = 16 * tt + 4 * (lane >> 4);
            const float4 b = ggpm_ld4(a.bu + c);
            f32x4 acc[1][1];
            ggpm_zero_acc<1, 1>(acc);
            const float* const tiles[1] = {Th};
            const int tn = tt + GGPM_NWA < NT ? tt + GGPM_NWA : -1;
            if constexpr (SPLIT) {
                const __bf16* const imgs[1] = {Ih};
                ggpm_wave_gemm_split<1>(imgs, PLANE, LDH, wps3, KC32, tt, tn, lane, acc, sring3);
            } else if constexpr (BF16) ggpm_wave_gemm_bf16<1, 1>(tiles, LD, wps3, Hp, tt, lane, acc);
            else ggpm_wave_gemm_ring<1, 1>(tiles, LD, wps3, KC, tt, tn, lane, acc, ring3);
            if (row < a.E1) ggpm_stx<ST16>(a.Qnew, (size_t)row * Hp + c, ggpm_f4(acc[0][0]) + b);
        }
    }
}

// Kernel A of a level on the K-split form of q' (GruFwdArgs.Qpart_*; dense, fp32 MFMA, one row tile, 2 .. GGPM_KS_MAXG column
// groups, at most two tiles of the group per wave: level_host.h, ksplit_q_form).  P1 and P2 are gru_fwd_a's, with two
// differences: the gather adds the previous step's `groups` partial q rows of a predecessor, in ascending group order, where
// gru_fwd_a reads one q row; and behind P2 the group's h' columns go back to LDS and ALL waves multiply them by the group's
// K slice of U_r over every output tile: Qpart[grp] = U_r[:, slice] h'[slice] (+ b_u in group 0).  The groups' partials add
// up to q' = U_r h' + b_u and nothing crosses workgroups inside the launch.  The step also sums the previous step's partials
// of its own rows and columns into that step's Qs slot, which is what the backward reads.
template <bool STASH>
__global__ void GGPM_A_BOUNDS gru_fwd_a_ks(GruFwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int Hp = a.Hp, LD = Hp + 4, KC = Hp / 16, NT = Hp / 16;
    float* Ts = lds;
    float* Tg = lds + 16 * LD;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // 1-D grid (ks_grid): workgroups go to the 8 XCDs round robin by their id, and the `groups` workgroups of a row tile
    // gather the same rows -- they get ids that are equal modulo 8, so they share one XCD's L2
    const int rtile = ((int)(blockIdx.x >> 3) / a.groups) * 8 + (int)(blockIdx.x & 7);
    if (rtile * 16 >= a.E1) return;
    const int r0 = rtile * 16;
    const int grp = (int)(blockIdx.x >> 3) % a.groups;
    const int t = grp * a.tg + wave;              // this wave's first output tile (if < t_end)
    const int t_end = min(NT, (grp + 1) * a.tg);
    const size_t pslot = (size_t)a.E1 * Hp;       // one group's partial rows
    const bool dbg_on = a.dbg && rtile == 1 && grp == 0 && threadIdx.x == 0;
    if (dbg_on) a.dbg[0] = wall_clock64();

    // ---- P1: gather.  Groups past the last re-read group 0 and are not added; null slots read row 0, whose h is 0 and whose
    // partials are finite.
    for (int lr = wave; lr < 16; lr += GGPM_NWA) {
        const int row = r0 + lr;
        GgpmRowList rl;
        if (a.h0_zero) { rl.lo = 0; rl.n = 0; } else rl = ggpm_row_list(a.rowptr, row, a.E1);
        const size_t rowo = (size_t)(row < a.E1 ? row : 0) * Hp;
        if (Hp <= 320) {
            // H = 250, 300: a lane takes four of the first 256 columns and, as scalars, one of the up to 64 behind them, so
            // the h row and the partial q rows of a predecessor are 5 * (1 + GGPM_KS_MAXG) = 30 registers of loads and TWO
            // predecessors per trip fit the 128 registers of a 16-wave workgroup, as in gru_fwd_a
            const int c = lane * 4, tc = 256 + lane;
            const bool on = c < Hp, ton = tc < Hp;
            const int cs = on ? c : 0, tcs = ton ? tc : 0;
            float4 s = ggpm_zero4(), g = ggpm_zero4(), rc = ggpm_zero4();
            float s1 = 0.f, g1 = 0.f, rc1 = 0.f;
            const float4 xr = ggpm_ld4(a.Xr + rowo + cs);
            const float xr1 = a.Xr[rowo + tcs];
            for (int base = 0; base < rl.n; base += 64) {
                const int chunk = ggpm_list_chunk(a.col, rl, base, lane);
                const int m = min(64, rl.n - base);
                for (int j = 0; j < m; j += 2) {
                    float4 h[2], qp[2][GGPM_KS_MAXG];
                    float h1[2], qp1[2][GGPM_KS_MAXG];
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const size_t p = (size_t)ggpm_list_at(chunk, j + u, m) * Hp;
                        h[u] = ggpm_ld4(a.Hprev + p + cs);
                        h1[u] = a.Hprev[p + tcs];
#pragma unroll
                        for (int gi = 0; gi < GGPM_KS_MAXG; ++gi) {
                            const float* part = a.Qpart_in + (gi < a.groups ? gi : 0) * pslot + p;
                            qp[u][gi] = ggpm_ld4(part + cs);
                            qp1[u][gi] = part[tcs];
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        float4 q = qp[u][0];
                        float q1 = qp1[u][0];
#pragma unroll
                        for (int gi = 1; gi < GGPM_KS_MAXG; ++gi)
                            if (gi < a.groups) { q = q + qp[u][gi]; q1 = q1 + qp1[u][gi]; }      // before xr + q
                        const float4 r = ggpm_fsigmoid4<false>(xr + q);
                        const float4 rh = r * h[u];
                        s = s + h[u];
                        g = g + rh;
                        rc = rc + rh * one_minus(r);
                        const float r1 = ggpm_fsigmoid<false>(xr1 + q1), rh1 = r1 * h1[u];
                        s1 = s1 + h1[u];
                        g1 = g1 + rh1;
                        rc1 = rc1 + rh1 * (1.f - r1);
                    }
                }
            }
            if (on) {
                ggpm_st4(Ts + lr * LD + c, s);
                ggpm_st4(Tg + lr * LD + c, g);
                if (STASH && row < a.E1 && (c >> 4) / a.tg == grp) {
                    const size_t o = (size_t)row * Hp + c;
                    ggpm_st4(a.S + o, s); ggpm_st4(a.G + o, g); ggpm_st4(a.R + o, rc);
                }
            }
            if (ton) {
                Ts[lr * LD + tc] = s1;
                Tg[lr * LD + tc] = g1;
                if (STASH && row < a.E1 && (tc >> 4) / a.tg == grp) {
                    const size_t o = (size_t)row * Hp + tc;
                    a.S[o] = s1; a.G[o] = g1; a.R[o] = rc1;
                }
            }
        } else {
            // wider rows: 512 columns per sweep as in gru_fwd_a, ONE predecessor per trip (2 + 2 * GGPM_KS_MAXG loads of 16 bytes)
            for (int c0 = 0; c0 < Hp; c0 += 512) {
                int c[2], cs[2];
                bool on[2];
                float4 s[2], g[2], rc[2], xr[2];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    c[k] = c0 + 256 * k + lane * 4;
                    on[k] = c[k] < Hp;
                    cs[k] = on[k] ? c[k] : 0;
                    s[k] = ggpm_zero4(); g[k] = ggpm_zero4(); rc[k] = ggpm_zero4();
                    xr[k] = ggpm_ld4(a.Xr + rowo + cs[k]);
                }
                for (int base = 0; base < rl.n; base += 64) {
                    const int chunk = ggpm_list_chunk(a.col, rl, base, lane);
                    const int m = min(64, rl.n - base);
                    for (int j = 0; j < m; ++j) {
                        const size_t p = (size_t)ggpm_list_at(chunk, j, m) * Hp;
                        float4 h[2], qp[2][GGPM_KS_MAXG];
#pragma unroll
                        for (int k = 0; k < 2; ++k) {
                            h[k] = ggpm_ld4(a.Hprev + p + cs[k]);
#pragma unroll
                            for (int gi = 0; gi < GGPM_KS_MAXG; ++gi)
                                qp[k][gi] = ggpm_ld4(a.Qpart_in + (gi < a.groups ? gi : 0) * pslot + p + cs[k]);
                        }
#pragma unroll
                        for (int k = 0; k < 2; ++k) {
                            float4 q = qp[k][0];
#pragma unroll
                            for (int gi = 1; gi < GGPM_KS_MAXG; ++gi)
                                if (gi < a.groups) q = q + qp[k][gi];
                            const float4 r = ggpm_fsigmoid4<false>(xr[k] + q);
                            const float4 rh = r * h[k];
                            s[k] = s[k] + h[k];
                            g[k] = g[k] + rh;
                            rc[k] = rc[k] + rh * one_minus(r);
                        }
                    }
                }
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    if (!on[k]) continue;
                    ggpm_st4(Ts + lr * LD + c[k], s[k]);
                    ggpm_st4(Tg + lr * LD + c[k], g[k]);
                    if (STASH && row < a.E1 && (c[k] >> 4) / a.tg == grp) {
                        const size_t o = (size_t)row * Hp + c[k];
                        ggpm_st4(a.S + o, s[k]); ggpm_st4(a.G + o, g[k]); ggpm_st4(a.R + o, rc[k]);
                    }
                }
            }
        }
    }
    if (dbg_on) a.dbg[1] = wall_clock64();

    const bool p2_gemm = !a.h0_zero;
    const float* const wps2[2] = {a.Wz, a.Wh};
    GgpmRing<2> ring2;
    if (p2_gemm && t < t_end) ggpm_ring_prefetch<2>(wps2, KC, t, lane, ring2);
    ggpm_lds_barrier();      // LDS tiles only: the stash stores above finish under the GEMM
    if (dbg_on) a.dbg[2] = wall_clock64();

    // ---- P2: gate GEMMs + gate math for this wave's (at most two) tiles, as straight-line code.  What the phase behind it
    // reads from memory is asked for BEFORE the epilogue's stores (a wave's loads and stores are acknowledged in order:
    // behind them every load would wait for the stores to land) -- by a wave without a tile right away, by the others behind
    // their last gate GEMM: the U_r fragments of this group's K slice for the wave's first two output tiles, and the previous
    // step's partials of the wave's own rows and columns (first tile).
    const int lr = lane & 15, row = r0 + lr;
    const int k0 = grp * a.tg, k1 = t_end;
    f32x4 head[4], head2[4];
    float4 hkeep[2] = {ggpm_zero4(), ggpm_zero4()};      // the h' fragments of this wave's tiles; rows past E1 stay 0
    // the previous step's partials of this workgroup's rows and columns, summed (the order of the gather) into that step's Qs
    // slot: 16 rows x 4 (k1 - k0) float4, spread over the waves [w0, w0 + nw)
    auto own_sums = [&](int w0, int nw) {
        const int n4 = 4 * (k1 - k0);
        for (int i = (wave - w0) * 64 + lane; i < 16 * n4; i += nw * 64) {
            const int orow = r0 + i / n4;
            if (orow >= a.E1) continue;
            const size_t o = (size_t)orow * Hp + 16 * k0 + 4 * (i % n4);
            float4 qo[GGPM_KS_MAXG];
#pragma unroll
            for (int gi = 0; gi < GGPM_KS_MAXG; ++gi) qo[gi] = ggpm_ld4(a.Qpart_in + (gi < a.groups ? gi : 0) * pslot + o);
            float4 q = qo[0];
#pragma unroll
            for (int gi = 1; gi < GGPM_KS_MAXG; ++gi)
                if (gi < a.groups) q = q + qo[gi];
            ggpm_st4(a.Qsum + o, q);
        }
    };
    const bool qsum_on = a.Qsum && a.Qpart_in;
    const int nown = min(k1 - k0, GGPM_NWA);      // waves that own a tile; the others are idle during P2 and take the sums
    auto prefetch = [&]() {
        if (a.Qpart_out) {
            if (wave < NT) ggpm_slice_head(a.Ur, KC, wave, k0, k1, lane, head);
            if (wave + GGPM_NWA < NT) ggpm_slice_head(a.Ur, KC, wave + GGPM_NWA, k0, k1, lane, head2);
        }
    };
    auto p2_tile = [&](int tt, float4& keep, bool last) {
        const int c = 16 * tt + 4 * (lane >> 4);
        const size_t o = (size_t)(row < a.E1 ? row : 0) * Hp + c;
        const float4 xz = ggpm_ld4(a.Xz + o), xh = ggpm_ld4(a.Xh + o);      // in flight under the GEMM
        f32x4 acc[2][1];
        ggpm_zero_acc<2, 1>(acc);
        if (p2_gemm) {
            const float* const tiles[2] = {Ts, Tg};
            ggpm_wave_gemm_ring<2, 1>(tiles, LD, wps2, KC, tt, last ? -1 : tt + GGPM_NWA, lane, acc, ring2);
        }
        if (last) prefetch();
        if (dbg_on) a.dbg[3] = wall_clock64();
        if (row >= a.E1) return;
        float4 h = ggpm_zero4(), z = ggpm_zero4(), m = ggpm_zero4();
        if (row != 0) {
            const float4 s = ggpm_ld4(Ts + lr * LD + c);
            const float4 pz = ggpm_f4(acc[0][0]) + xz, pm = ggpm_f4(acc[1][0]) + xh;
            z = ggpm_sigmoid4(pz);
            m = make_float4(tanhf(pm.x), tanhf(pm.y), tanhf(pm.z), tanhf(pm.w));
            h = make_float4((1.f - z.x) * s.x + z.x * m.x, (1.f - z.y) * s.y + z.y * m.y,
                            (1.f - z.z) * s.z + z.z * m.z, (1.f - z.w) * s.w + z.w * m.w);
        }
        ggpm_st4(a.Hnew + o, h);
        keep = h;
        if (STASH) {
            ggpm_st4(a.Z + o, z);
            ggpm_st4(a.M + o, m);
        }
    };
    if (t >= t_end) {
        prefetch();
        if (qsum_on) own_sums(nown, GGPM_NWA - nown);
    } else if (t + GGPM_NWA >= t_end) p2_tile(t, hkeep[0], true);
    else { p2_tile(t, hkeep[0], false); p2_tile(t + GGPM_NWA, hkeep[1], true); }
    if (dbg_on) a.dbg[4] = wall_clock64();

    // ---- partial q' of this group
    if (a.Qpart_out) {
        ggpm_lds_barrier();      // every wave is done with g
        if (t < t_end) ggpm_st4(Tg + lr * LD + 16 * t + 4 * (lane >> 4), hkeep[0]);
        if (t + GGPM_NWA < t_end) ggpm_st4(Tg + lr * LD + 16 * (t + GGPM_NWA) + 4 * (lane >> 4), hkeep[1]);
        ggpm_lds_barrier();
        float* const part = a.Qpart_out + (size_t)grp * pslot;
        int pi = 0;
        for (int tt = wave; tt < NT; tt += GGPM_NWA, ++pi) {
            const int c = 16 * tt + 4 * (lane >> 4);
            const float4 b = grp == 0 ? ggpm_ld4(a.bu + c) : ggpm_zero4();
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            if (pi == 1) {
#pragma unroll
                for (int d = 0; d < 4; ++d) head[d] = head2[d];
            }
            // (a third tile and beyond: their fragments come a tile ahead)
            ggpm_wave_gemm_slice(Tg, LD, a.Ur, KC, tt, k0, k1, pi >= 1 && tt + GGPM_NWA < NT ? tt + GGPM_NWA : -1, k0, k1, lane, acc, head);
            if (row < a.E1) ggpm_st4(part + (size_t)row * Hp + c, grp == 0 ? ggpm_f4(acc) + b : ggpm_f4(acc));
        }
    }
    if (qsum_on && nown == GGPM_NWA) own_sums(0, GGPM_NWA);      // (no idle wave: everyone, at the end)
    if (dbg_on) a.dbg[7] = wall_clock64();
}

// Kernel B of such a level (its last executed step, when that is not the level's last): q' as the sum over the column groups'
// K slices in group order, each slice the chain gru_fwd_a_ks's partials run, so what the step leaves in Qs has the bits a
// sum of partials would have (the fixed-point level stops early and must agree bit for bit with the level that does not).
__global__ void GGPM_A_BOUNDS gru_fwd_b_ks(GruFwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int Hp = a.Hp, LD = Hp + 4, KC = Hp / 16, NT = Hp / 16;
    float* Th = lds;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r0 = blockIdx.x * 16;
    const int grp = blockIdx.y;
    const int t_end = min(NT, (grp + 1) * a.tg);
    ggpm_load_rows_to_lds<16, false>(a.Hnew, r0, a.E1, Hp, LD, Th);
    __syncthreads();
    const int row = r0 + (lane & 15);
    for (int tt = grp * a.tg + wave; tt < t_end; tt += GGPM_NWA) {
        const int c = 16 * tt + 4 * (lane >> 4);
        const float4 b = ggpm_ld4(a.bu + c);
        f32x4 head[4];
        ggpm_slice_head(a.Ur, KC, tt, 0, min(NT, a.tg), lane, head);
        float4 q = ggpm_zero4();
        for (int gi = 0; gi < a.groups; ++gi) {
            const int k0 = gi * a.tg, k1 = min(NT, k0 + a.tg);
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            ggpm_wave_gemm_slice(Th, LD, a.Ur, KC, tt, k0, k1, gi + 1 < a.groups ? tt : -1, k1, min(NT, k1 + a.tg), lane, acc, head);
            q = gi == 0 ? ggpm_f4(acc) + b : q + ggpm_f4(acc);
        }
        if (row < a.E1) ggpm_st4(a.Qnew + (size_t)row * Hp + c, q);
    }
}

// Kernel B (same geometry as A): q' = U_r h' + b_u (h' rows come back from L2).
template <int GM, int RTT, bool ST16 = false>
__global__ void GGPM_A_BOUNDS gru_fwd_b(GruFwdArgs a) {
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
    const float* const wps[1] = {a.Ur};
    std::conditional_t<GM == 0, GgpmRing<1>, GgpmNoRing> ring;
    std::conditional_t<SPLIT, GgpmSplitRing<1>, GgpmNoRing> sring;
    if constexpr (GM == 0)
        if (grp * a.tg + wave < t_end) ggpm_ring_prefetch<1>(wps, KC, grp * a.tg + wave, lane, ring);     // under the row copy
    if constexpr (SPLIT) {
        if (grp * a.tg + wave < t_end) ggpm_split_ring_prefetch<1>(wps, KC32, grp * a.tg + wave, lane, sring);
        ggpm_split_init(Ih, 1, ROWS, Hp);
        if (a.src_idx) ggpm_gather_rows_to_lds_split<ROWS>(a.src_h, a.src_idx, r0, a.E1, Hp, Ih, PLANE, LDH, grp == 0 ? a.Hnew : nullptr);
        else ggpm_load_rows_to_lds_split<ROWS>(a.Hnew, r0, a.E1, Hp, Ih, PLANE, LDH);
    } else {
        if (a.src_idx) ggpm_gather_rows_to_lds<ROWS>(a.src_h, a.src_idx, r0, a.E1, Hp, LD, Th, grp == 0 ? a.Hnew : nullptr);
        else ggpm_load_rows_to_lds<ROWS, ST16>(a.Hnew, r0, a.E1, Hp, LD, Th);
    }
    __syncthreads();
    for (int tt = grp * a.tg + wave; tt < t_end; tt += GGPM_NWA) {
        const int c = 16 * tt + 4 * (lane >> 4);
        const float4 b = ggpm_ld4(a.bu + c);
        f32x4 acc[1][RTT];
        ggpm_zero_acc<1, RTT>(acc);
        if (!(a.ablate & 2)) {
            const float* const tiles[1] = {Th};
            const int tn = tt + GGPM_NWA < t_end ? tt + GGPM_NWA : -1;
            if constexpr (SPLIT) {
                const __bf16* const imgs[1] = {Ih};
                ggpm_wave_gemm_split<1>(imgs, PLANE, LDH, wps, KC32, tt, tn, lane, acc, sring);
            } else if constexpr (BF16) ggpm_wave_gemm_bf16<1, RTT>(tiles, LD, wps, Hp, tt, lane, acc);
            else ggpm_wave_gemm_ring<1, RTT>(tiles, LD, wps, KC, tt, tn, lane, acc, ring);
        }
#pragma unroll
        for (int r = 0; r < RTT; ++r) {
            const int row = r0 + 16 * r + (lane & 15);
            if (row < a.E1) ggpm_stx<ST16>(a.Qnew, (size_t)row * Hp + c, ggpm_f4(acc[0][r]) + b);
        }
    }
}

// ---------------------------------------------------------------------------------------------- backward
struct GruBwdArgs {
    int E1, Hp, tg;
    int first;                     // t == depth: dH comes from dHD, no successor gather
    const float* Xr;
    const float *Hcur, *Qcur;      // Hs[t],   Qs[t]      (kernel A gather; unused when first)
    const float *S, *Z, *M, *R;    // stash slot t-1
    const float* dHD;              // [E1,Hp], used when first
    const float *dSin, *dGin;      // from depth t+1
    float *dSout, *dGout;          // for depth t-1
    float* DQ;                     // stash slot for dq^t (nullptr when first)
    float *DMP, *DZP, *DSD;        // dm_pre / dz_pre stash slot t-1, ds_dir scratch
    float *dXz, *dXr, *dXh;        // running sums (zeroed by the driver)
    const float *WzT, *WhT, *UrT;  // packed transposes
    const int32_t *srowptr, *scol; // successors
    // sparse_forward only: frozen rows pass their gradient straight through the depth loop (carry), and a final
    // gather-only launch (t = 0) yields the gradient of the incoming state for them.
    const unsigned char* frozen;
    float* carry;                  // [E1,Hp] running dh of frozen rows (started by the first backward depth)
    int final_pass;                // t == 0: P1 + dq.U_r only, result to dHin
    float* dHin;                   // [E1,Hp]
    float* scat_h;                 // ggpm_level_opts.scatter_*: the final pass ADDS row r's result to
    const int32_t* scat_idx;       // scat_h[scat_idx[r]] (unique ids; < 0: dropped) instead of writing dHin
    int fuse_b;                    // single column group: kernel A also forms dS, dG for depth t-1 (no B launch)
    unsigned long long* dbg;       // optional phase stamps (GGPM_ADEBUG; dev only)
    int bf16;                      // gate products on bf16 operands
    int skip_xsum;                 // dXz / dXh are NOT accumulated here: the caller sums the DZP / DMP stash slots afterwards
    int st16;                      // bf16 storage of Hs / Qs / S / Z / M / dS / dG / DQ / DZP / DMP (see GruFwdArgs)
};

// Kernel A (16 waves): gather over successors (dq full rows, dh partial) -> dh = partial + dq.U_r ->
// gate derivatives for this workgroup's column group.
template <int GM, int RTT, bool ST16 = false>
__global__ void GGPM_A_BOUNDS gru_bwd_a(GruBwdArgs a) {
    constexpr int ROWS = RTT * 16;      // ST16: Hs, Qs, S, Z, M, dS / dG, DQ, DZP, DMP in bf16 (tile_mma.h)
    constexpr bool BF16 = GM == 1, SPLIT = GM == 2;
    static_assert(!SPLIT || RTT == 1, "split operands: one row tile per workgroup");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int Hp = a.Hp, LD = Hp + 4, KC = Hp / 16, NT = Hp / 16;
    float* T0 = lds;                  // dh partial
    float* T1 = lds + ROWS * LD;      // dq
    // split operands: T0 stays fp32 (epilogue only); behind it the bf16 images of dq and (fused dS / dG) dz_pre, dm_pre
    const int LDH = ggpm_split_ldh(Hp), PLANE = ROWS * LDH, KC32 = ggpm_kc32_dev(Hp);
    const int IMG = ggpm_split_image_halves(ROWS, Hp);
    __bf16* I1 = reinterpret_cast<__bf16*>(lds + ROWS * LD);
    __bf16* Iz = I1 + IMG;
    __bf16* Im = Iz + IMG;
    if constexpr (SPLIT) ggpm_split_init(I1, a.fuse_b ? 3 : 1, ROWS, Hp);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r0 = blockIdx.x * ROWS;
    const int grp = blockIdx.y;
    const int t = grp * a.tg + wave;

    const bool dbg_on = a.dbg && blockIdx.x == 1 && blockIdx.y == 0 && threadIdx.x == 0;
    if (dbg_on) a.dbg[0] = wall_clock64();
    // ---- P1: dh_p += dS_e + dG_e*r ; dq_p += dG_e * h_p * r(1-r) over successors e (null slots: row 0,
    // where dS = dG = 0)
    if (!a.first) {
        for (int lr = wave; lr < ROWS; lr += GGPM_NWA) {
            const int p = r0 + lr;
            const GgpmRowList rl = ggpm_row_list(a.srowptr, p, a.E1);
            const size_t po = (size_t)(p < a.E1 ? p : 0) * Hp;
            for (int c0 = 0; c0 < Hp; c0 += 512) {
                int c[2], cs[2];
                bool on[2];
                float4 dh[2], dq[2], hp[2], qp[2];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    c[k] = c0 + 256 * k + lane * 4;
                    on[k] = c[k] < Hp;
                    cs[k] = on[k] ? c[k] : 0;
                    dh[k] = ggpm_zero4(); dq[k] = ggpm_zero4();
                    hp[k] = ggpm_ldx<ST16>(a.Hcur, po + cs[k]);
                    qp[k] = ggpm_ldx<ST16>(a.Qcur, po + cs[k]);
                }
                for (int base = 0; base < rl.n; base += 64) {
                    const int chunk = ggpm_list_chunk(a.scol, rl, base, lane);
                    const int m = min(64, rl.n - base);
                    for (int j = 0; j < m; j += 2) {
                        float4 xr[2][2], dg[2][2], ds[2][2];
#pragma unroll
                        for (int u = 0; u < 2; ++u) {
                            const size_t e = (size_t)ggpm_list_at(chunk, j + u, m) * Hp;
#pragma unroll
                            for (int k = 0; k < 2; ++k) {
                                xr[u][k] = ggpm_ld4(a.Xr + e + cs[k]);
                                dg[u][k] = ggpm_ldx<ST16>(a.dGin, e + cs[k]);
                                ds[u][k] = ggpm_ldx<ST16>(a.dSin, e + cs[k]);
                            }
                        }
#pragma unroll
                        for (int u = 0; u < 2; ++u)
#pragma unroll
                            for (int k = 0; k < 2; ++k) {
                                const float4 r = ggpm_fsigmoid4<BF16>(xr[u][k] + qp[k]);
                                const float4 dgr = dg[u][k] * r;
                                dh[k] = dh[k] + ds[u][k] + dgr;
                                dq[k] = dq[k] + dgr * hp[k] * one_minus(r);
                            }
                    }
                }
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    if (!on[k]) continue;
                    ggpm_st4(T0 + lr * LD + c[k], dh[k]);
                    if constexpr (SPLIT) ggpm_split_store(I1, PLANE, LDH, lr, c[k], dq[k]);
                    else ggpm_st4(T1 + lr * LD + c[k], dq[k]);
                    if (p < a.E1 && (c[k] >> 4) / a.tg == grp) ggpm_stx<ST16>(a.DQ, (size_t)p * Hp + c[k], dq[k]);
                }
            }
        }
    }

    if (dbg_on) a.dbg[1] = wall_clock64();
    const int t_end = min(NT, (grp + 1) * a.tg);
    const float* const wps2[1] = {a.UrT};
    std::conditional_t<GM == 0, GgpmRing<1>, GgpmNoRing> ring2;
    std::conditional_t<SPLIT, GgpmSplitRing<1>, GgpmNoRing> sring2;
    if constexpr (GM == 0)
        if (!a.first && t < t_end) ggpm_ring_prefetch<1>(wps2, KC, t, lane, ring2);      // under the wait for the gatherers
    if constexpr (SPLIT)
        if (!a.first && t < t_end) ggpm_split_ring_prefetch<1>(wps2, KC32, t, lane, sring2);
    if (!a.first) ggpm_lds_barrier();      // LDS tiles only: the dq stash stores finish under the GEMM
    if (dbg_on) a.dbg[2] = wall_clock64();

    // ---- P2: dh = partial + dq . U_r ; gate derivatives, for this wave's tiles
    const int lr = lane & 15;
    float4 dsd_keep[2] = {ggpm_zero4(), ggpm_zero4()};      // fused P3 (RTT = 1): ds_dir of this wave's (at most two) tiles
    int it = 0;
    for (int tt = t; tt < t_end; tt += GGPM_NWA, ++it) {
        const int c = 16 * tt + 4 * (lane >> 4);
        float4 s[RTT], z[RTT], m[RTT], oxz[RTT], oxh[RTT], dhd[RTT];
        auto load_inputs = [&]() {
#pragma unroll
            for (int r = 0; r < RTT; ++r) {
                const int row = r0 + 16 * r + lr;
                const size_t o = (size_t)(row < a.E1 ? row : 0) * Hp + c;
                s[r] = z[r] = m[r] = oxz[r] = oxh[r] = ggpm_zero4();
                if (!a.final_pass) {
                    s[r] = ggpm_ldx<ST16>(a.S, o); z[r] = ggpm_ldx<ST16>(a.Z, o); m[r] = ggpm_ldx<ST16>(a.M, o);
                    if (!a.first && !a.skip_xsum) { oxz[r] = ggpm_ld4(a.dXz + o); oxh[r] = ggpm_ld4(a.dXh + o); }    // depth D starts the sums
                }
                dhd[r] = a.first ? ggpm_ld4(a.dHD + o) : ggpm_zero4();
            }
        };
        if constexpr (RTT == 1) load_inputs();      // in flight under the GEMM (two row tiles: the registers go to the GEMM)
        f32x4 acc[1][RTT];
        ggpm_zero_acc<1, RTT>(acc);
        if (!a.first) {
            const float* const tiles[1] = {T1};
            const int tn = tt + GGPM_NWA < t_end ? tt + GGPM_NWA : -1;
            if constexpr (SPLIT) {
                const __bf16* const imgs[1] = {I1};
                ggpm_wave_gemm_split<1>(imgs, PLANE, LDH, wps2, KC32, tt, tn, lane, acc, sring2);
            } else if constexpr (BF16) ggpm_wave_gemm_bf16<1, RTT>(tiles, LD, wps2, Hp, tt, lane, acc);
            else ggpm_wave_gemm_ring<1, RTT>(tiles, LD, wps2, KC, tt, tn, lane, acc, ring2);
        }
        if constexpr (RTT != 1) load_inputs();
        if (dbg_on) a.dbg[3] = wall_clock64();
#pragma unroll
        for (int r = 0; r < RTT; ++r) {
            const int lrow = 16 * r + lr, row = r0 + lrow;
            const size_t o = (size_t)(row < a.E1 ? row : 0) * Hp + c;
            auto keep_zm = [&](float4 vz, float4 vm) {      // the complete dz_pre / dm_pre rows for the fused dS / dG phase
                if constexpr (SPLIT) {
                    ggpm_split_store(Iz, PLANE, LDH, lrow, c, vz);
                    ggpm_split_store(Im, PLANE, LDH, lrow, c, vm);
                } else {
                    ggpm_st4(lds + 2 * ROWS * LD + lrow * LD + c, vz);
                    ggpm_st4(lds + 3 * ROWS * LD + lrow * LD + c, vm);
                }
            };
            if (row >= a.E1) {
                if (a.fuse_b) keep_zm(ggpm_zero4(), ggpm_zero4());
                continue;
            }
            const bool frz = a.frozen && a.frozen[row];
            if (a.final_pass) {        // gradient of the incoming state: frozen rows only (active rows started from 0)
                float4 dh0 = ggpm_zero4();
                if (frz) dh0 = ggpm_f4(acc[0][r]) + ggpm_ld4(T0 + lrow * LD + c) + ggpm_ld4(a.carry + o);
                if (a.scat_idx) {
                    const int id = frz ? a.scat_idx[row] : -1;
                    if (id >= 0) {
                        float* d = a.scat_h + (size_t)id * Hp + c;
                        ggpm_st4(d, ggpm_ld4(d) + dh0);
                    }
                } else {
                    ggpm_st4(a.dHin + o, dh0);
                }
                continue;
            }
            float4 dsdir = ggpm_zero4(), dzp = ggpm_zero4(), dmp = ggpm_zero4();
            if (row != 0 || a.frozen) {
                float4 dh = a.first ? dhd[r] : (ggpm_f4(acc[0][r]) + ggpm_ld4(T0 + lrow * LD + c));
                if (frz) {             // h_t = h_{t-1} for frozen rows: carry the whole dh to the previous depth
                    if (!a.first) dh = dh + ggpm_ld4(a.carry + o);      // (the first backward depth starts the carry: no memset)
                    ggpm_st4(a.carry + o, dh);
                    dh = ggpm_zero4();   // nothing flows through gates (their stash is 0 anyway)
                }
                const float dhv[4] = {dh.x, dh.y, dh.z, dh.w}, sv[4] = {s[r].x, s[r].y, s[r].z, s[r].w};
                const float zv[4] = {z[r].x, z[r].y, z[r].z, z[r].w}, mv[4] = {m[r].x, m[r].y, m[r].z, m[r].w};
                float o_ds[4], o_dz[4], o_dm[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    o_ds[k] = dhv[k] * (1.f - zv[k]);
                    o_dz[k] = dhv[k] * (mv[k] - sv[k]) * zv[k] * (1.f - zv[k]);
                    o_dm[k] = dhv[k] * zv[k] * (1.f - mv[k] * mv[k]);
                }
                dsdir = make_float4(o_ds[0], o_ds[1], o_ds[2], o_ds[3]);
                dzp = make_float4(o_dz[0], o_dz[1], o_dz[2], o_dz[3]);
                dmp = make_float4(o_dm[0], o_dm[1], o_dm[2], o_dm[3]);
                if constexpr (ST16) { dzp = ggpm_rne4(dzp); dmp = ggpm_rne4(dmp); }      // (the stored values: every user sees them)
            }
            ggpm_stx<ST16>(a.DZP, o, dzp);
            ggpm_stx<ST16>(a.DMP, o, dmp);
            if (!a.skip_xsum) {
                ggpm_st4(a.dXz + o, oxz[r] + dzp);
                ggpm_st4(a.dXh + o, oxh[r] + dmp);
            }
            if (a.fuse_b) {
                keep_zm(dzp, dmp);
                if (it == 0) dsd_keep[0] = dsdir; else dsd_keep[1] = dsdir;
            } else {
                ggpm_st4(a.DSD + o, dsdir);
            }
        }
    }
    if (dbg_on) a.dbg[4] = wall_clock64();
    if (!a.fuse_b) return;

    // ---- P3 (single column group, RTT = 1 only): the workgroup holds the complete dz_pre / dm_pre rows ->
    // dG = dm_pre . Wh_h ; dS = ds_dir + dz_pre . Wz_h ; dXr += dG * R   (the body of kernel B)
    if constexpr (RTT == 1) {
        const int row = r0 + lr;
        const float* const wps3[2] = {a.WhT, a.WzT};
        std::conditional_t<GM == 0, GgpmRing<2>, GgpmNoRing> ring3;
        std::conditional_t<SPLIT, GgpmSplitRing<2>, GgpmNoRing> sring3;
        if constexpr (GM == 0)
            if (wave < NT) ggpm_ring_prefetch<2>(wps3, KC, wave, lane, ring3);
        if constexpr (SPLIT)
            if (wave < NT) ggpm_split_ring_prefetch<2>(wps3, KC32, wave, lane, sring3);
        ggpm_lds_barrier();
        it = 0;
        for (int tt = wave; tt < NT; tt += GGPM_NWA, ++it) {
            const int c = 16 * tt + 4 * (lane >> 4);
            const size_t o = (size_t)(row < a.E1 ? row : 0) * Hp + c;
            const float4 dsd = it == 0 ? dsd_keep[0] : dsd_keep[1];
            const float4 rco = ggpm_ld4(a.R + o), oxr = a.first ? ggpm_zero4() : ggpm_ld4(a.dXr + o);
            f32x4 acc[2][1];
            ggpm_zero_acc<2, 1>(acc);
            {
                const float* const tiles[2] = {lds + 3 * ROWS * LD, lds + 2 * ROWS * LD};
                const int tn = tt + GGPM_NWA < NT ? tt + GGPM_NWA : -1;
                if constexpr (SPLIT) {
                    const __bf16* const imgs[2] = {Im, Iz};
                    ggpm_wave_gemm_split<2>(imgs, PLANE, LDH, wps3, KC32, tt, tn, lane, acc, sring3);
                } else if constexpr (BF16) ggpm_wave_gemm_bf16<2, 1>(tiles, LD, wps3, Hp, tt, lane, acc);
                else ggpm_wave_gemm_ring<2, 1>(tiles, LD, wps3, KC, tt, tn, lane, acc, ring3);
            }
            if (row >= a.E1) continue;
            float4 dg = ggpm_f4(acc[0][0]);
            if constexpr (ST16) dg = ggpm_rne4(dg);
            ggpm_stx<ST16>(a.dGout, o, dg);
            ggpm_stx<ST16>(a.dSout, o, ggpm_f4(acc[1][0]) + dsd);
            ggpm_st4(a.dXr + o, oxr + dg * rco);
        }
    }
}

// Kernel B (same geometry as A): dG = dm_pre . Wh_h ; dS = ds_dir + dz_pre . Wz_h (for depth t-1) ;
// dXr += dG * R with R = sum_p h_p r(1-r) stashed by the forward gather.
template <int GM, int RTT, bool ST16 = false>
__global__ void GGPM_A_BOUNDS gru_bwd_b(GruBwdArgs a) {
    constexpr int ROWS = RTT * 16;
    constexpr bool BF16 = GM == 1, SPLIT = GM == 2;
    static_assert(!SPLIT || RTT == 1, "split operands: one row tile per workgroup");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int Hp = a.Hp, LD = Hp + 4, KC = Hp / 16, NT = Hp / 16;
    float* T1 = lds;                  // dz_pre rows
    float* T2 = lds + ROWS * LD;      // dm_pre rows
    const int LDH = ggpm_split_ldh(Hp), PLANE = ROWS * LDH, KC32 = ggpm_kc32_dev(Hp);
    __bf16* Iz = reinterpret_cast<__bf16*>(lds);
    __bf16* Im = Iz + ggpm_split_image_halves(ROWS, Hp);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r0 = blockIdx.x * ROWS;
    const int grp = blockIdx.y;
    const int t_end = min(NT, (grp + 1) * a.tg);
    const float* const wps[2] = {a.WhT, a.WzT};
    std::conditional_t<GM == 0, GgpmRing<2>, GgpmNoRing> ring;
    std::conditional_t<SPLIT, GgpmSplitRing<2>, GgpmNoRing> sring;
    if constexpr (GM == 0)
        if (grp * a.tg + wave < t_end) ggpm_ring_prefetch<2>(wps, KC, grp * a.tg + wave, lane, ring);     // under the row copies
    if constexpr (SPLIT) {
        if (grp * a.tg + wave < t_end) ggpm_split_ring_prefetch<2>(wps, KC32, grp * a.tg + wave, lane, sring);
        ggpm_split_init(Iz, 2, ROWS, Hp);
        ggpm_load_rows_to_lds_split<ROWS>(a.DZP, r0, a.E1, Hp, Iz, PLANE, LDH);
        ggpm_load_rows_to_lds_split<ROWS>(a.DMP, r0, a.E1, Hp, Im, PLANE, LDH);
    } else {
        ggpm_load_rows_to_lds<ROWS, ST16>(a.DZP, r0, a.E1, Hp, LD, T1);
        ggpm_load_rows_to_lds<ROWS, ST16>(a.DMP, r0, a.E1, Hp, LD, T2);
    }
    __syncthreads();
    for (int tt = grp * a.tg + wave; tt < t_end; tt += GGPM_NWA) {
        const int c = 16 * tt + 4 * (lane >> 4);
        float4 dsd[RTT], rco[RTT], oxr[RTT];
        auto load_inputs = [&]() {
#pragma unroll
            for (int r = 0; r < RTT; ++r) {
                const int e = r0 + 16 * r + (lane & 15);
                const size_t o = (size_t)(e < a.E1 ? e : 0) * Hp + c;
                dsd[r] = ggpm_ld4(a.DSD + o); rco[r] = ggpm_ld4(a.R + o);
                oxr[r] = a.first ? ggpm_zero4() : ggpm_ld4(a.dXr + o);
            }
        };
        if constexpr (RTT == 1) load_inputs();
        f32x4 acc[2][RTT];
        ggpm_zero_acc<2, RTT>(acc);
        {
            const float* const tiles[2] = {T2, T1};
            const int tn = tt + GGPM_NWA < t_end ? tt + GGPM_NWA : -1;
            if constexpr (SPLIT) {
                const __bf16* const imgs[2] = {Im, Iz};
                ggpm_wave_gemm_split<2>(imgs, PLANE, LDH, wps, KC32, tt, tn, lane, acc, sring);
            } else if constexpr (BF16) ggpm_wave_gemm_bf16<2, RTT>(tiles, LD, wps, Hp, tt, lane, acc);
            else ggpm_wave_gemm_ring<2, RTT>(tiles, LD, wps, KC, tt, tn, lane, acc, ring);
        }
        if constexpr (RTT != 1) load_inputs();
#pragma unroll
        for (int r = 0; r < RTT; ++r) {
            const int e = r0 + 16 * r + (lane & 15);
            if (e >= a.E1) continue;
            const size_t o = (size_t)e * Hp + c;
            float4 dg = ggpm_f4(acc[0][r]);
            if constexpr (ST16) dg = ggpm_rne4(dg);
            ggpm_stx<ST16>(a.dGout, o, dg);
            ggpm_stx<ST16>(a.dSout, o, ggpm_f4(acc[1][r]) + dsd[r]);
            ggpm_st4(a.dXr + o, oxr[r] + dg * rco[r]);
        }
    }
}

// What level_host.h needs to know about the GRU (each line is a difference from the LSTM; DESIGN.md 5.1 has the table).
struct GruCell {
    static constexpr StepNeed fwd = {{3, 1, 3}, {2, 1, 2}, {1, 0, 1}};      // fused: s, g, h' | A: s, g | B: the h' rows
    static constexpr StepNeed bwd = {{4, 1, 3}, {2, 1, 1}, {2, 0, 2}};      // kernel B: the dz_pre and dm_pre rows
    static constexpr int bwd_fuse_max_tiles = 2 * GGPM_NWA;                 // the fused dS / dG phase: two output tiles per wave
    static constexpr bool rt2_bf16 = true;                                  // gru_*<1, 2> and gru_*<1, 2, true> exist
    static constexpr int gate_products = 2;                                 // forward Wz.s, Wh.g; backward B dG, dS
    static constexpr int timing_base = 0;                                   // ggpm_timing_begin slots 0 / 1 / 4 / 5
    static constexpr int n_mat = 3, n_stash = 2;                            // Wz, Wh, Ur; DMP, DZP
    static constexpr int csws_rows = 256;                                   // column-sum scratch of db_u
    // two row tiles per workgroup where the level is large enough to be bound by the weight stream (see GGPM_RT2_MIN_ROW_TILES)
    // or the caller asks for it (ggpm_level_opts.prefer_narrow)
    static bool use_rt2(const ggpm_level_opts& o, int E1, int Hp, bool sparse) {
        static const int mode = [] { const char* e = ggpm_dev_env("GGPM_RT2"); return e ? atoi(e) : 1; }();     // 0 off, 2 always
        if (mode == 0 || sparse) return false;
        if (lds_tiles(2, Hp, 32) > GGPM_LDS_LIMIT) return false;
        return mode == 2 || o.prefer_narrow || ggpm_ceil_div(E1, 16) >= GGPM_RT2_MIN_ROW_TILES;
    }
    // mode 2: the fp32 tile + two bf16 images of the forward A launch
    static bool mode2_fits(int Hp) { return lds_tiles(1, Hp) + 2 * ggpm_split_image_bytes(16, Hp) <= GGPM_LDS_LIMIT; }
    // one LDS tile pair of 16 rows must fit a CU
    static bool shape_ok(int, int Hp) { return lds_tiles(2, Hp) <= GGPM_LDS_LIMIT; }
};

// GGPM_ADEBUG (dev variant; the GRU A kernels only): where workgroup (0,0) leaves its phase stamps
inline unsigned long long* adebug_stamps(unsigned long long*& buf) {
    if (!env_adebug()) return nullptr;
    if (!buf) (void)hipMalloc(&buf, 64);
    return buf;
}

// the 1-D grid of gru_fwd_a_ks: ids i, i + 8, .. i + 8 (groups - 1) are the column groups of one row tile
inline dim3 ks_grid(const GruFwdArgs& a) { return dim3(8 * ggpm_ceil_div(ggpm_ceil_div(a.E1, 16), 8) * a.groups); }

// ks: the level runs on the K-split form of q' (ksplit_q_form: gate mode 0, one row tile, column groups, so nothing is fused);
// a step that leaves partials (a.Qpart_out) has no B launch
void launch_fwd(GruFwdArgs a, bool rt2, bool stash, bool with_b, bool ks, double flops1, hipStream_t s) {
    const StepLds step = fwd_step<GruCell>(a.Hp, a.tg, rt2, a.bf16, with_b);
    a.fuse_b = step.fuse;
    if (ks) {
        static unsigned long long* ks_dbg_buf = nullptr;
        static int ks_dbg_count = 0;
        a.dbg = adebug_stamps(ks_dbg_buf);
        ggpm_timing_begin(GruCell::timing_base, s, ((a.Qpart_out ? 1 : 0) + (a.h0_zero ? 0 : GruCell::gate_products)) * flops1);
        {
            auto kernel = stash ? gru_fwd_a_ks<true> : gru_fwd_a_ks<false>;
            set_lds(kernel, step.a);
            kernel<<<ks_grid(a), GGPM_NWA * 64, step.a, s>>>(a);
        }
        ggpm_timing_end(GruCell::timing_base, s);
        if (a.dbg && a.Qpart_in && a.Qpart_out && (++ks_dbg_count % 97) == 0) {
            unsigned long long h[8];
            (void)hipStreamSynchronize(s);
            (void)hipMemcpy(h, a.dbg, sizeof(h), hipMemcpyDeviceToHost);
            fprintf(stderr, "[adebug ksplit E1=%d groups=%d] gather %.2f barrier %.2f gemm %.2f epilogue %.2f partial q' %.2f us\n",
                    a.E1, a.groups, (h[1] - h[0]) * 0.01, (h[2] - h[1]) * 0.01, (h[3] - h[2]) * 0.01, (h[4] - h[3]) * 0.01,
                    (h[7] - h[4]) * 0.01);
        }
        if (with_b && !a.Qpart_out) {
            ggpm_timing_begin(GruCell::timing_base + 4, s, 1 * flops1);
            launch_step(gru_fwd_b_ks, a, false, step.b, s);
            ggpm_timing_end(GruCell::timing_base + 4, s);
        }
        return;
    }
    static unsigned long long* dbg_buf = nullptr;
    static int dbg_count = 0;
    a.dbg = adebug_stamps(dbg_buf);
    ggpm_timing_begin(GruCell::timing_base, s, (step.fuse + (a.h0_zero ? 0 : GruCell::gate_products)) * flops1);     // the first depth has no gate products
    for_variant<GruCell>(a.st16, rt2, a.bf16, [&](auto GM, auto RTT, auto ST16) {
        launch_step(stash ? gru_fwd_a<true, GM, RTT, ST16> : gru_fwd_a<false, GM, RTT, ST16>, a, rt2, step.a, s);
    });
    ggpm_timing_end(GruCell::timing_base, s);
    if (a.dbg && (++dbg_count % 97) == 0) {
        unsigned long long h[7];
        const dim3 grid = step_grid(a, rt2);
        (void)hipStreamSynchronize(s);
        (void)hipMemcpy(h, a.dbg, sizeof(h), hipMemcpyDeviceToHost);
        fprintf(stderr, "[adebug E1=%d grid=%dx%d fuse=%d] gather %.2f barrier %.2f gemm %.2f epilogue %.2f us; wave 15 starts "
                "+%.2f, gathers %.2f\n", a.E1, grid.x, grid.y, a.fuse_b, (h[1] - h[0]) * 0.01, (h[2] - h[1]) * 0.01,
                (h[3] - h[2]) * 0.01, (h[4] - h[3]) * 0.01, ((double)h[5] - (double)h[0]) * 0.01, (h[6] - h[5]) * 0.01);
    }
    if (with_b && !step.fuse) {
        ggpm_timing_begin(GruCell::timing_base + 4, s, 1 * flops1);
        for_variant<GruCell>(a.st16, rt2, a.bf16, [&](auto GM, auto RTT, auto ST16) {
            launch_step(gru_fwd_b<GM, RTT, ST16>, a, rt2, step.b, s);
        });
        ggpm_timing_end(GruCell::timing_base + 4, s);
    }
}

void launch_bwd(GruBwdArgs a, bool rt2, bool with_b, double flops1, hipStream_t s) {
    const StepLds step = bwd_step<GruCell>(a.Hp, a.tg, rt2, a.bf16, with_b, a.final_pass != 0);
    a.fuse_b = step.fuse;
    static unsigned long long* dbg_buf = nullptr;
    static int dbg_count = 0;
    a.dbg = adebug_stamps(dbg_buf);
    ggpm_timing_begin(GruCell::timing_base + 1, s, (step.fuse ? 1 + GruCell::gate_products : 1) * flops1);
    for_variant<GruCell>(a.st16, rt2, a.bf16, [&](auto GM, auto RTT, auto ST16) {
        launch_step(gru_bwd_a<GM, RTT, ST16>, a, rt2, step.a, s);
    });
    ggpm_timing_end(GruCell::timing_base + 1, s);
    if (a.dbg && !a.first && (++dbg_count % 89) == 0) {
        unsigned long long h[5];
        const dim3 grid = step_grid(a, rt2);
        (void)hipStreamSynchronize(s);
        (void)hipMemcpy(h, a.dbg, sizeof(h), hipMemcpyDeviceToHost);
        fprintf(stderr, "[adebug bwd E1=%d grid=%dx%d fuse=%d] gather %.2f barrier %.2f gemm %.2f epilogue %.2f us\n", a.E1,
                grid.x, grid.y, a.fuse_b, (h[1] - h[0]) * 0.01, (h[2] - h[1]) * 0.01, (h[3] - h[2]) * 0.01,
                (h[4] - h[3]) * 0.01);
    }
    if (with_b && !step.fuse) {
        ggpm_timing_begin(GruCell::timing_base + 5, s, GruCell::gate_products * flops1);
        for_variant<GruCell>(a.st16, rt2, a.bf16, [&](auto GM, auto RTT, auto ST16) {
            launch_step(gru_bwd_b<GM, RTT, ST16>, a, rt2, step.b, s);
        });
        ggpm_timing_end(GruCell::timing_base + 5, s);
    }
}

}  // namespace

extern "C" size_t ggpm_gru_pack_floats(int H) {
    const int Hp = ggpm_padded_hidden(H);
    return 3 * ggpm_packed_matrix_slot(Hp) + (size_t)Hp;
}

// ggpm_level_form_query (capi.hip) for a GRU level
int ggpm_gru_level_form(int E1, int H, int sparse, int training, const ggpm_level_opts& o, ggpm_level_form* out) {
    return level_form<GruCell>(E1, H, sparse, training, o, out);
}

// the K-split form of q' (ggpm_level_opts.q_part): the buffer of a level, and whether a forward call would use one
extern "C" size_t ggpm_level_q_part_bytes(int E1, int H) {
    if (E1 <= 0 || H <= 0) return 0;
    const int Hp = ggpm_padded_hidden(H);
    return q_part_floats(E1, Hp, pick_tg(E1, Hp / 16)) * sizeof(float);
}
extern "C" int ggpm_level_ksplit_q(int lstm, int E1, int H, int sparse, const ggpm_level_opts* opts) {
    if (lstm || sparse || E1 <= 0 || H <= 0) return 0;
    const int Hp = ggpm_padded_hidden(H);
    if (!GruCell::shape_ok(E1, Hp)) return 0;
    return ksplit_q_form(level_plan<GruCell>(ggpm_opts_or_default(opts), E1, Hp, false), Hp) ? 1 : 0;
}

namespace {
__global__ void sparse_init_state(const float* __restrict__ h_in, const unsigned char* __restrict__ frozen,
                                  float* __restrict__ H0, int Hp) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (c >= Hp) return;
    H0[(size_t)r * Hp + c] = frozen[r] ? h_in[(size_t)r * Hp + c] : 0.f;    // rows being recomputed start from 0
}
}  // namespace

int gru_forward_impl(const LevelCall& c, int save_for_backward, const ggpm_level_opts& o, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    const int E1 = c.rows, H = c.H, depth = c.depth;
    float *Hs = c.Hs, *Qs = c.Qs, *wpack = c.wpack;
    const unsigned char* frozen = c.frozen;
    bool ok = E1 > 0 && H > 0 && depth > 0 && c.bu && c.pred_rowptr && c.pred_col && Hs && Qs && wpack;
    for (int k = 0; k < 3; ++k) ok = ok && c.X[k] && c.W[k];
    for (int k = 0; k < 5; ++k) ok = ok && (c.St[k] || !save_for_backward);
    if (!ok) return GGPM_ERR_ARG;
    const int Hp = ggpm_padded_hidden(H);
    if (!GruCell::shape_ok(E1, Hp)) return GGPM_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const size_t slot = (size_t)E1 * Hp;
    const LevelPlan plan = level_plan<GruCell>(o, E1, Hp, frozen != nullptr);
    const bool rt2 = plan.rt2;
    const int bf16 = plan.gm;      // gate mode 0 / 1 / 2
    // K-split q' (ggpm_level_opts.q_part): every step but the last executed one leaves partials in place of its B launch
    const bool ks = o.q_part && !frozen && ksplit_q_form(plan, Hp);
    const size_t qblock = q_part_floats(E1, Hp, plan.tg) / 2;
    if (ks && o.q_part_bytes < 2 * qblock * sizeof(float)) return GGPM_ERR_WORKSPACE;
    const size_t mstep = ggpm_packed_matrix_floats(Hp, bf16);
    float* pWz = wpack; float* pWh = wpack + mstep; float* pUr = wpack + 2 * mstep;
    float* pbu = wpack + 3 * ggpm_packed_matrix_slot(Hp);
    {
        GgpmPackArgs pk = {};
        pk.W[0] = c.W[0]; pk.ldw[0] = c.ldw[0]; pk.W[1] = c.W[2]; pk.ldw[1] = c.ldw[2]; pk.W[2] = c.W[1]; pk.ldw[2] = c.ldw[1];
        pk.H = H; pk.Hp = Hp; pk.transpose = 0; pk.dst = wpack; pk.bias = c.bu; pk.bias_out = pbu; pk.bf16 = bf16;
        if (!o.weights_packed) ggpm_launch_pack(pk, 3, s);
    }
    dim3 ig(ggpm_ceil_div(Hp, 256), E1);
    const int tg0 = plan.tg;
    const bool gathered = o.gather_h && o.gather_idx && frozen;
    if (frozen) {      // sparse_forward: start from the caller's state, q^0 = U_r h^0 + b_u by one B launch
        // (h_in == Hs: the caller put the masked start state -- frozen rows' states, zero elsewhere -- into slot 0 itself;
        // ggpm_level_opts.gather_*: the q^0 launch fetches it through the index and writes slot 0 on the way)
        if (c.h_in != Hs && !gathered) sparse_init_state<<<ig, 256, 0, s>>>(c.h_in, frozen, Hs, Hp);
        GruFwdArgs a0 = {};
        a0.E1 = E1; a0.Hp = Hp; a0.tg = tg0; a0.Hnew = Hs; a0.Qnew = Qs; a0.Ur = pUr; a0.bu = pbu; a0.bf16 = bf16;
        if (gathered) { a0.src_h = o.gather_h; a0.src_idx = o.gather_idx; }
        const size_t lds_b = fwd_step<GruCell>(Hp, tg0, false, bf16, true).b;
        for_variant<GruCell>(false, false, bf16, [&](auto GM, auto RTT, auto ST16) {
            launch_step(gru_fwd_b<GM, RTT, ST16>, a0, false, lds_b, s);
        });
    }
    // dense levels start from h^0 = 0: the first depth launch knows that (h0_zero), so H^0 / Q^0 are never materialised

    const int tg = plan.tg;
    const double flops1 = 2.0 * (double)(E1 - 1) * H * H;   // algorithmic flops of ONE gate product
    static const char* const abl = ggpm_dev_env("GGPM_ABLATE");
    // forward-only form (ggpm_level_opts.h_out): the training forward's steps and roundings, without stashes
    const bool infer = !save_for_backward && o.h_out;
    // bf16 storage (tile_mma.h): bf16 gate products, dense, training, every stash contraction on the bf16 tall kernel
    const bool st16 = ggpm_level_st16(bf16, frozen != nullptr, save_for_backward || infer, E1, H);
    int run_depth = o.run_depth;
    if (run_depth <= 0 || run_depth > depth || frozen || !(save_for_backward || infer)) run_depth = depth;
    // fixed-point level (ggpm_level_opts.fixed_slot): only the last step's stash slot is ever read
    const int fs = (o.fixed_slot > 0 && save_for_backward && !frozen && !st16) ? o.fixed_slot : 0;
    if (fs && fs != run_depth) return GGPM_ERR_ARG;
    for (int t = 1; t <= run_depth; ++t) {
        const bool stash = save_for_backward && (!fs || t == fs);
        GruFwdArgs a = {};
        a.E1 = E1; a.Hp = Hp; a.tg = tg; a.Xz = c.X[0]; a.Xr = c.X[1]; a.Xh = c.X[2];
        a.Wz = pWz; a.Wh = pWh; a.Ur = pUr; a.bu = pbu; a.rowptr = c.pred_rowptr; a.col = c.pred_col;
        a.ablate = abl ? atoi(abl) : 0;
        a.frozen = frozen;
        a.bf16 = bf16;
        a.st16 = st16 ? 1 : 0;
        a.h0_zero = (t == 1 && !frozen) ? 1 : 0;
        if (save_for_backward) {
            a.Hprev = ggpm_slot_ptr(Hs, t - 1, slot, st16); a.Hnew = ggpm_slot_ptr(Hs, t, slot, st16);
            a.Hout = (st16 && t == depth) ? Hs + (size_t)depth * slot : nullptr;      // the level's result stays fp32, at its usual place
            a.Qprev = ggpm_slot_ptr(Qs, t - 1, slot, st16);
            a.Qnew = (t < depth) ? ggpm_slot_ptr(Qs, t, slot, st16) : nullptr;   // q^depth is never consumed
            a.S = ggpm_slot_ptr(c.St[0], t - 1, slot, st16); a.G = ggpm_slot_ptr(c.St[1], t - 1, slot, st16);
            a.Z = ggpm_slot_ptr(c.St[2], t - 1, slot, st16); a.M = ggpm_slot_ptr(c.St[3], t - 1, slot, st16);
            a.R = c.St[4] + (size_t)(t - 1) * slot;
            if (!stash) a.S = a.G = a.Z = a.M = a.R = nullptr;
        } else if (infer) {
            a.Hprev = ggpm_slot_ptr(Hs, (t - 1) & 1, slot, st16); a.Hnew = ggpm_slot_ptr(Hs, t & 1, slot, st16);
            a.Qprev = ggpm_slot_ptr(Qs, (t - 1) & 1, slot, st16); a.Qnew = ggpm_slot_ptr(Qs, t & 1, slot, st16);
            if (t == run_depth) {          // the level's result, fp32, where the caller wants it
                if (st16) a.Hout = o.h_out;
                else a.Hnew = o.h_out;
            }
            a.S = a.G = a.Z = a.M = a.R = nullptr;
        } else {
            a.Hprev = Hs + (size_t)((t - 1) & 1) * slot; a.Hnew = Hs + (size_t)(t & 1) * slot;
            a.Qprev = Qs + (size_t)((t - 1) & 1) * slot; a.Qnew = Qs + (size_t)(t & 1) * slot;
            a.S = a.G = a.Z = a.M = a.R = nullptr;
        }
        if (ks) {
            a.groups = ggpm_ceil_div(Hp / 16, tg);
            if (t < run_depth) a.Qpart_out = o.q_part + (size_t)(t & 1) * qblock;
            if (t > 1) {
                a.Qpart_in = o.q_part + (size_t)((t - 1) & 1) * qblock;
                a.Qsum = save_for_backward ? const_cast<float*>(a.Qprev) : nullptr;      // (only the backward reads Qs again)
            }
        }
        launch_fwd(a, rt2, stash, t < depth, ks, flops1, s);
    }
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

// the operands both forward entry points name, by the parameter names they share
#define GRU_FORWARD_OPERANDS(c) \
    c.rows = E1; c.H = H; c.depth = depth; \
    c.X[0] = Xz; c.X[1] = Xr; c.X[2] = Xh; \
    c.W[0] = Wz_h; c.ldw[0] = ld_wz; c.W[1] = Ur; c.ldw[1] = ld_ur; c.W[2] = Wh_h; c.ldw[2] = ld_wh; c.bu = bu; \
    c.pred_rowptr = pred_rowptr; c.pred_col = pred_col; \
    c.Hs = Hs; c.Qs = Qs; c.St[0] = Ss; c.St[1] = Gs; c.St[2] = Zs; c.St[3] = Ms; c.St[4] = Rs; c.wpack = wpack;
extern "C" int ggpm_gru_forward(int E1, int H, int depth, const float* Xz, const float* Xr, const float* Xh,
                                const float* Wz_h, int ld_wz, const float* Ur, int ld_ur, const float* bu,
                                const float* Wh_h, int ld_wh, const int32_t* pred_rowptr,
                                const int32_t* pred_col, float* Hs, float* Qs, float* Ss, float* Gs, float* Zs,
                                float* Ms, float* Rs, float* wpack, int save_for_backward,
                                const ggpm_level_opts* opts, ggpm_stream_t stream) {
    LevelCall c = {};
    GRU_FORWARD_OPERANDS(c);
    return gru_forward_impl(c, save_for_backward, ggpm_opts_or_default(opts), stream);
}

extern "C" int ggpm_gru_sparse_forward(int E1, int H, int depth, const float* h_in, const unsigned char* frozen,
                                       const float* Xz, const float* Xr, const float* Xh, const float* Wz_h,
                                       int ld_wz, const float* Ur, int ld_ur, const float* bu, const float* Wh_h,
                                       int ld_wh, const int32_t* pred_rowptr, const int32_t* pred_col, float* Hs,
                                       float* Qs, float* Ss, float* Gs, float* Zs, float* Ms, float* Rs,
                                       float* wpack, int save_for_backward, const ggpm_level_opts* opts,
                                       ggpm_stream_t stream) {
    if (!h_in || !frozen) return GGPM_ERR_ARG;
    LevelCall c = {};
    GRU_FORWARD_OPERANDS(c);
    c.h_in = h_in; c.frozen = frozen;
    return gru_forward_impl(c, save_for_backward, ggpm_opts_or_default(opts), stream);
}
#undef GRU_FORWARD_OPERANDS

extern "C" size_t ggpm_gru_backward_workspace_bytes(int E1, int H, int depth) {
    return backward_workspace_bytes<GruCell>(E1, H, depth);      // (level_host.h: carve)
}

// a small pool of re-recordable events (the encoder drivers' stream ordering, encoder.hip)
hipEvent_t ggpm_wgrad_event(int i) {
    static thread_local hipEvent_t pool[64] = {};
    i &= 63;
    if (!pool[i] && hipEventCreateWithFlags(&pool[i], hipEventDisableTiming) != hipSuccess) return nullptr;
    return pool[i];
}

int gru_backward_impl(const LevelCall& c, int weight_grads, const ggpm_level_opts& o, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    const int E1 = c.rows, H = c.H, depth = c.depth;
    const float *Xr = c.X[GRU_GATES.reread], *Hs = c.Hs, *Qs = c.Qs;
    float* work = c.work;
    const unsigned char* frozen = c.frozen;
    if (o.skip_sparse_wgrads && frozen) weight_grads = 0;      // (ggpm_level_weight_grads follows, on the caller's choice of stream)
    const bool skip_xsum = o.skip_x_sums && !frozen;
    const bool scattered = o.scatter_h && o.scatter_idx && frozen;
    bool ok = E1 > 0 && H > 0 && depth > 0 && Xr && c.pred_rowptr && c.pred_col && c.succ_rowptr && c.succ_col && Hs && Qs &&
              c.d_out && c.dbu && work;
    for (int k = 0; k < 3; ++k) ok = ok && c.W[k] && c.dX[k] && c.dW[k];
    for (int k = 0; k < 5; ++k) ok = ok && c.St[k];
    if (!ok) return GGPM_ERR_ARG;
    if (c.work_bytes < ggpm_gru_backward_workspace_bytes(E1, H, depth)) return GGPM_ERR_WORKSPACE;
    const int Hp = ggpm_padded_hidden(H);
    if (!GruCell::shape_ok(E1, Hp)) return GGPM_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const size_t slot = (size_t)E1 * Hp;

    const LevelPlan plan = level_plan<GruCell>(o, E1, Hp, frozen != nullptr);
    const bool rt2 = plan.rt2;
    const int bf16 = plan.gm;      // gate mode 0 / 1 / 2
    const size_t mstep = ggpm_packed_matrix_floats(Hp, bf16);
    const LevelWork<GruCell> wk = carve<GruCell>(work, E1, Hp, depth);
    float* pWzT = wk.packedT; float* pWhT = pWzT + mstep; float* pUrT = pWzT + 2 * mstep;
    float* DMP = wk.stash[0]; float* DZP = wk.stash[1]; float* DQ = wk.DQ;
    float* const dSb[2] = {wk.scratch[0], wk.scratch[1]}; float* const dGb[2] = {wk.scratch[2], wk.scratch[3]};
    float* DSD = wk.scratch[4];      // ds_dir scratch
    float* carry = wk.scratch[5];
    if (o.defer_stash[0]) {       // deferred weight gradients: the stashes go to the caller's stacked buffers
        if (!frozen || !o.defer_stash[1] || !o.defer_stash[2]) return GGPM_ERR_ARG;
        DMP = o.defer_stash[0]; DZP = o.defer_stash[1]; DQ = o.defer_stash[2];
        weight_grads = 0;
    }

    {
        GgpmPackArgs pk = {};
        pk.W[0] = c.W[0]; pk.ldw[0] = c.ldw[0]; pk.W[1] = c.W[2]; pk.ldw[1] = c.ldw[2]; pk.W[2] = c.W[1]; pk.ldw[2] = c.ldw[1];
        pk.H = H; pk.Hp = Hp; pk.transpose = 1; pk.dst = pWzT; pk.bias = nullptr; pk.bias_out = nullptr; pk.bf16 = bf16;
        if (!o.weights_packed) ggpm_launch_pack(pk, 3, s);
    }
    // dXz / dXh are started (not accumulated) by the first backward depth; so is dXr when that depth has a dS/dG product
    if (depth == 1 && !frozen) (void)hipMemsetAsync(c.dX[1], 0, slot * sizeof(float), s);

    const int tg = plan.tg;
    const double flops1 = 2.0 * (double)(E1 - 1) * H * H;   // algorithmic flops of ONE gate product
    const bool st16 = ggpm_level_st16(bf16, frozen != nullptr, true, E1, H);      // (as the forward decided)
    // tree-side levels: d(h^t) vanishes below step `lo` (nilpotent Jacobian, common.h); sparse runs go all the way
    int lo = o.lo;
    if (lo < 1 || lo > depth || frozen) lo = 1;
    // fixed-point level (ggpm_level_opts.fixed_slot): state slots above fs and stash slots above fs - 1 alias those
    const int fs = (o.fixed_slot > 0 && !frozen && !st16) ? o.fixed_slot : 0;
    if (fs && (fs >= depth || lo < fs)) return GGPM_ERR_ARG;      // (every slot a step >= lo reads must be the settled one)
    auto state_slot = [fs](int t) { return fs && t > fs ? fs : t; };
    auto stash_slot = [fs](int t) { return fs && t > fs ? fs - 1 : t - 1; };
    for (int t = depth; t >= lo; --t) {
        GruBwdArgs a = {};
        a.E1 = E1; a.Hp = Hp; a.tg = tg; a.first = (t == depth);
        a.Xr = Xr;
        a.st16 = st16 ? 1 : 0;
        a.Hcur = ggpm_slot_ptr(Hs, state_slot(t), slot, st16);
        a.Qcur = (t < depth) ? ggpm_slot_ptr(Qs, state_slot(t), slot, st16) : nullptr;
        a.S = ggpm_slot_ptr(c.St[0], stash_slot(t), slot, st16); a.Z = ggpm_slot_ptr(c.St[2], stash_slot(t), slot, st16);
        a.M = ggpm_slot_ptr(c.St[3], stash_slot(t), slot, st16);
        a.R = c.St[4] + (size_t)stash_slot(t) * slot;
        a.dHD = c.d_out;
        a.dSin = dSb[(t + 1) & 1]; a.dGin = dGb[(t + 1) & 1];      // (bf16 storage: bf16 in the first half of each buffer)
        a.dSout = dSb[t & 1]; a.dGout = dGb[t & 1];
        a.DQ = (t < depth) ? ggpm_slot_ptr(DQ, t, slot, st16) : nullptr;
        a.frozen = frozen; a.carry = carry; a.final_pass = 0; a.dHin = nullptr;
        a.DMP = ggpm_slot_ptr(DMP, t - 1, slot, st16); a.DZP = ggpm_slot_ptr(DZP, t - 1, slot, st16); a.DSD = DSD;
        a.dXz = c.dX[0]; a.dXr = c.dX[1]; a.dXh = c.dX[2];
        a.WzT = pWzT; a.WhT = pWhT; a.UrT = pUrT; a.bf16 = bf16;
        a.srowptr = c.succ_rowptr; a.scol = c.succ_col;
        a.skip_xsum = skip_xsum ? 1 : 0;
        launch_bwd(a, rt2, t > 1 || frozen != nullptr, flops1, s);     // (the dS/dG launch of step lo > 1 still forms dXr)
    }
    GGPM_CHECK_LAUNCH();

    if (frozen) {      // gradient of the incoming state: one more gather + dq.U_r launch at t = 0
        GruBwdArgs a = {};
        a.E1 = E1; a.Hp = Hp; a.tg = tg; a.first = 0; a.final_pass = 1;
        a.Xr = Xr; a.Hcur = Hs; a.Qcur = Qs;
        a.dSin = dSb[1]; a.dGin = dGb[1];          // written by the B launch of depth 1
        a.DQ = DQ; a.UrT = pUrT; a.srowptr = c.succ_rowptr; a.scol = c.succ_col; a.bf16 = bf16;
        a.frozen = frozen; a.carry = carry; a.dHin = c.d_in;
        if (scattered) { a.scat_h = o.scatter_h; a.scat_idx = o.scatter_idx; }
        launch_bwd(a, rt2, false, flops1, s);
        GGPM_CHECK_LAUNCH();
    }
    if (!weight_grads) return GGPM_OK;
    return gru_weight_grads_impl(c, lo, o, stream);
}

// the operands both backward entry points name, by the parameter names they share
#define GRU_BACKWARD_OPERANDS(c) \
    c.rows = E1; c.H = H; c.depth = depth; \
    c.X[GRU_GATES.reread] = Xr; \
    c.W[0] = Wz_h; c.ldw[0] = ld_wz; c.W[1] = Ur; c.ldw[1] = ld_ur; c.W[2] = Wh_h; c.ldw[2] = ld_wh; \
    c.pred_rowptr = pred_rowptr; c.pred_col = pred_col; c.succ_rowptr = succ_rowptr; c.succ_col = succ_col; \
    c.Hs = level_read(Hs); c.Qs = level_read(Qs); \
    c.St[0] = level_read(Ss); c.St[1] = level_read(Gs); c.St[2] = level_read(Zs); c.St[3] = level_read(Ms); c.St[4] = level_read(Rs); \
    c.d_out = dHD; c.dX[0] = dXz; c.dX[1] = dXr; c.dX[2] = dXh; \
    c.dW[0] = dWz_h; c.ld_dw[0] = ld_dwz; c.dW[1] = dUr; c.ld_dw[1] = ld_dur; c.dW[2] = dWh_h; c.ld_dw[2] = ld_dwh; c.dbu = dbu; \
    c.work = work; c.work_bytes = work_bytes;
extern "C" int ggpm_gru_backward(int E1, int H, int depth, const float* Xr, const float* Wz_h, int ld_wz,
                                 const float* Ur, int ld_ur, const float* Wh_h, int ld_wh,
                                 const int32_t* pred_rowptr, const int32_t* pred_col,
                                 const int32_t* succ_rowptr, const int32_t* succ_col, const float* Hs,
                                 const float* Qs, const float* Ss, const float* Gs, const float* Zs,
                                 const float* Ms, const float* Rs, const float* dHD, float* dXz, float* dXr,
                                 float* dXh, float* dWz_h, int ld_dwz, float* dUr, int ld_dur, float* dbu,
                                 float* dWh_h, int ld_dwh, float* work, size_t work_bytes, int weight_grads,
                                 const ggpm_level_opts* opts, ggpm_stream_t stream) {
    LevelCall c = {};
    GRU_BACKWARD_OPERANDS(c);
    return gru_backward_impl(c, weight_grads, ggpm_opts_or_default(opts), stream);
}

// sparse_forward backward: additionally returns dHin (gradient of the incoming state; zero on the recomputed rows)
extern "C" int ggpm_gru_sparse_backward(int E1, int H, int depth, const unsigned char* frozen, const float* Xr,
                                        const float* Wz_h, int ld_wz, const float* Ur, int ld_ur,
                                        const float* Wh_h, int ld_wh, const int32_t* pred_rowptr,
                                        const int32_t* pred_col, const int32_t* succ_rowptr,
                                        const int32_t* succ_col, const float* Hs, const float* Qs, const float* Ss,
                                        const float* Gs, const float* Zs, const float* Ms, const float* Rs,
                                        const float* dHD, float* dHin, float* dXz, float* dXr, float* dXh,
                                        float* dWz_h, int ld_dwz, float* dUr, int ld_dur, float* dbu, float* dWh_h,
                                        int ld_dwh, float* work, size_t work_bytes, const ggpm_level_opts* opts,
                                        ggpm_stream_t stream) {
    if (!frozen || !dHin) return GGPM_ERR_ARG;
    LevelCall c = {};
    GRU_BACKWARD_OPERANDS(c);
    c.frozen = frozen; c.d_in = dHin;
    return gru_backward_impl(c, 1, ggpm_opts_or_default(opts), stream);
}
#undef GRU_BACKWARD_OPERANDS

// Weight gradients of the GRU message function: tall contractions over every (depth, message) row of the
// stashes ggpm_gru_backward left in `work`.  Separate entry point so that the host can run them on a second
// stream while the next level's (latency-bound) depth loop occupies the main one.  A sparse level (c.frozen): dq^0 included.
int gru_weight_grads_impl(const LevelCall& c, int lo, const ggpm_level_opts& o, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    const int E1 = c.rows, H = c.H, depth = c.depth;
    const bool with_slot0 = c.frozen != nullptr;
    if (E1 <= 0 || H <= 0 || depth <= 0 || !c.Hs || !c.St[0] || !c.St[1] || !c.work || !c.dW[0] || !c.dW[1] || !c.dbu || !c.dW[2])
        return GGPM_ERR_ARG;
    if (lo < 1 || lo > depth || with_slot0) lo = 1;       // backward steps depth .. lo ran (stash slots lo-1 .. depth-1)
    if (c.work_bytes < ggpm_gru_backward_workspace_bytes(E1, H, depth)) return GGPM_ERR_WORKSPACE;
    const LevelWork<GruCell> wk = carve<GruCell>(c.work, E1, ggpm_padded_hidden(H), depth);
    // dWh_h = DMP^T G, dWz_h = DZP^T S, dUr = DQ^T h, db_u = colsum(DQ) (skip_bias_u: ggpm_gru_bias_u_grad forms it elsewhere)
    const WgradTerm gate[2] = {{wk.stash[0], c.St[1], c.dW[2], c.ld_dw[2]}, {wk.stash[1], c.St[0], c.dW[0], c.ld_dw[0]}};
    return level_weight_grads(E1, H, depth, lo, with_slot0, o, 2, gate, {wk.DQ, c.Hs, c.dW[1], c.ld_dw[1]},
                              o.skip_bias_u ? nullptr : c.dbu, wk.csws, wk.skws, wk.skbytes(c.work_bytes), stream);
}

// db_u of a dense level by itself (what gru_weight_grads_impl does last unless ggpm_level_opts.skip_bias_u is set): the
// column sum of the dq stash slots lo .. depth-1 (dq^t pairs with h^t; the dense level never produces dq^0).
int ggpm_gru_bias_u_grad(int E1, int H, int depth, int lo, float* work, float* dbu, float* csws, const ggpm_level_opts* opts,
                         ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (E1 <= 0 || H <= 0 || depth <= 0 || !work || !dbu || !csws) return GGPM_ERR_ARG;
    if (lo < 1 || lo > depth) lo = 1;
    const int Hp = ggpm_padded_hidden(H);
    const size_t slot = (size_t)E1 * Hp;
    const float* DQ = carve<GruCell>(work, E1, Hp, depth).DQ;
    if (depth <= lo) {
        (void)hipMemsetAsync(dbu, 0, H * sizeof(float), (hipStream_t)stream);
        return GGPM_OK;
    }
    const bool st16 = ggpm_opts_or_default(opts).gate_dtype == 1 && ggpm_bf16_storage_applies(E1, H);
    return ggpm_colsum_dtype(ggpm_slot_ptr(DQ, lo, slot, st16), Hp, (depth - lo) * E1, H, dbu, csws, st16, stream);
}

namespace {
template <bool B16>
__global__ void __launch_bounds__(256) sum_slots_k(const float* __restrict__ src, int slots, size_t slot4, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= slot4) return;
    float4 acc = ggpm_ldx<B16>(src, 4 * i);
    for (int t = 1; t < slots; ++t) acc = acc + ggpm_ldx<B16>(src, 4 * ((size_t)t * slot4 + i));          // fixed order
    reinterpret_cast<float4*>(out)[i] = acc;
}
}  // namespace

namespace {
struct SumPairArgs {
    const float* src[4];
    float *hi[4], *lo[4];
    int slots[4];
    size_t slot4;
};
// s + e == a + b exactly (Knuth's two-sum: no ordering of |a|, |b| assumed)
__device__ __forceinline__ void two_sum(float a, float b, float& s, float& e) {
    s = a + b;
    const float bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}
__global__ void __launch_bounds__(256) sum_slots_pair_k(SumPairArgs p) {
    const int m = blockIdx.y;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.slot4) return;
    const float4* __restrict__ src = reinterpret_cast<const float4*>(p.src[m]);
    float4 h = src[i], l = ggpm_zero4(), e;
    for (int t = 1; t < p.slots[m]; ++t) {          // fixed order
        const float4 x = src[(size_t)t * p.slot4 + i];
        two_sum(h.x, x.x, h.x, e.x); two_sum(h.y, x.y, h.y, e.y); two_sum(h.z, x.z, h.z, e.z); two_sum(h.w, x.w, h.w, e.w);
        l = l + e;
    }
    reinterpret_cast<float4*>(p.hi[m])[i] = h;
    reinterpret_cast<float4*>(p.lo[m])[i] = l;
}
}  // namespace

int ggpm_sum_slots_pair_grouped(int count, const float* const* src, const int* slots, size_t slot_floats, float* const* hi,
                                float* const* lo, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (count <= 0 || count > 4 || !src || !slots || !hi || !lo || slot_floats == 0 || (slot_floats & 3)) return GGPM_ERR_ARG;
    SumPairArgs p = {};
    for (int m = 0; m < count; ++m) {
        if (!src[m] || !hi[m] || !lo[m] || slots[m] <= 0) return GGPM_ERR_ARG;
        p.src[m] = src[m]; p.hi[m] = hi[m]; p.lo[m] = lo[m]; p.slots[m] = slots[m];
    }
    p.slot4 = slot_floats / 4;
    sum_slots_pair_k<<<dim3((unsigned)((p.slot4 + 255) / 256), count), 256, 0, (hipStream_t)stream>>>(p);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_sum_slots(const float* src, int slots, size_t slot_floats, float* out, ggpm_stream_t stream) {
    return ggpm_sum_slots_any(src, slots, slot_floats, out, false, stream);
}

int ggpm_sum_slots_any(const float* src, int slots, size_t slot_floats, float* out, bool src_bf16, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!src || !out || slots <= 0 || slot_floats == 0 || (slot_floats & 3)) return GGPM_ERR_ARG;
    const size_t slot4 = slot_floats / 4;
    if (src_bf16) sum_slots_k<true><<<(unsigned)((slot4 + 255) / 256), 256, 0, (hipStream_t)stream>>>(src, slots, slot4, out);
    else sum_slots_k<false><<<(unsigned)((slot4 + 255) / 256), 256, 0, (hipStream_t)stream>>>(src, slots, slot4, out);
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

// where ggpm_gru_backward left its dm_pre / dz_pre stashes inside `work` (slot t-1 of each = backward step t)
extern "C" int ggpm_gru_backward_stashes(float* work, int E1, int H, int depth, float** DMP, float** DZP) {
    if (!work || !DMP || !DZP || E1 <= 0 || H <= 0 || depth <= 0) return GGPM_ERR_ARG;
    const LevelWork<GruCell> wk = carve<GruCell>(work, E1, ggpm_padded_hidden(H), depth);
    *DMP = wk.stash[0];
    *DZP = wk.stash[1];
    return GGPM_OK;
}

extern "C" size_t ggpm_weight_grads_stacked_workspace_bytes(int H, int rows) {
    const size_t Hp = (size_t)ggpm_padded_hidden(H);
    return 256 * Hp * sizeof(float) + ggpm_gemm_workspace_bytes(H, H, rows) + 256;
}

// The hidden-half weight gradients of MANY sparse backward calls at once: their stashes stacked row-wise (one block per
// call, the same block order in every buffer), see ggpm_level_opts.defer_stash.
extern "C" int ggpm_gru_weight_grads_stacked(int rows, int rows_q, int H, const float* DMP, const float* Gs,
                                             const float* DZP, const float* Ss, const float* DQ, const float* Hs,
                                             float* dWz_h, int ld_dwz, float* dUr, int ld_dur, float* dbu, float* dWh_h,
                                             int ld_dwh, float* work, size_t work_bytes, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (rows <= 0 || rows_q <= 0 || H <= 0 || !DMP || !Gs || !DZP || !Ss || !DQ || !Hs || !dWz_h || !dUr || !dbu ||
        !dWh_h || !work)
        return GGPM_ERR_ARG;
    if (work_bytes < ggpm_weight_grads_stacked_workspace_bytes(H, rows > rows_q ? rows : rows_q)) return GGPM_ERR_WORKSPACE;
    const int Hp = ggpm_padded_hidden(H);
    float* csws = work;
    float* skws = work + (size_t)256 * Hp;
    const size_t skbytes = work_bytes - (size_t)256 * Hp * sizeof(float);
    const WgradTerm gate[2] = {{DMP, Gs, dWh_h, ld_dwh}, {DZP, Ss, dWz_h, ld_dwz}};
    // (the light column sum first: whatever else shares the GPU at the end of a pass, the stream ends with the contraction)
    return tall_weight_grads(H, Hp, 2, gate, rows, {DQ, Hs, dUr, ld_dur}, rows_q, dbu, csws, false, 0, skws, skbytes, stream);
}

extern "C" int ggpm_gru_weight_grads(int E1, int H, int depth, const float* Hs, const float* Ss, const float* Gs,
                                     float* work, size_t work_bytes, float* dWz_h, int ld_dwz, float* dUr,
                                     int ld_dur, float* dbu, float* dWh_h, int ld_dwh, const ggpm_level_opts* opts,
                                     ggpm_stream_t stream) {
    LevelCall c = {};
    c.rows = E1; c.H = H; c.depth = depth;
    c.Hs = level_read(Hs); c.St[0] = level_read(Ss); c.St[1] = level_read(Gs);
    c.dW[0] = dWz_h; c.ld_dw[0] = ld_dwz; c.dW[1] = dUr; c.ld_dw[1] = ld_dur; c.dW[2] = dWh_h; c.ld_dw[2] = ld_dwh; c.dbu = dbu;
    c.work = work; c.work_bytes = work_bytes;
    return ggpm_level_weight_grads(c, opts, stream);
}
