// Host side of a GRU / LSTM level call, written once for both cells (mpn_gru.hip, mpn_lstm.hip): the form decisions
// (LevelPlan, StepLds: what the impl functions, the launchers and ggpm_level_form_query all decide through), the choice of
// kernel instantiation, the launch geometry, the layout of the backward workspace and the weight-gradient tail.
//
// A cell describes itself by one struct (GruCell, LstmCell, beside the kernels they name) with these members, each of
// which is a real difference between the cells:
//   StepNeed fwd, bwd        LDS of a depth step: the fused A launch, A alone, B -- as (fp32 tiles, and on split operands
//                            fp32 tiles + images); a tile is rows x (Hp + 4) floats, an image ggpm_split_image_bytes
//   int bwd_fuse_max_tiles   the fused backward holds at most this many output tiles (0: no limit)
//   bool rt2_bf16            the two-row-tile kernels also exist on bf16 operands (GM = 1, with and without bf16 storage)
//   int gate_products        gate products of a forward A launch = products of a backward B launch (timing flops)
//   int timing_base          ggpm_timing_begin slots: forward A base, backward A base + 1, forward B base + 4, backward B base + 5
//   int n_mat, n_stash       packed weight matrices; gate-gradient stashes of the backward workspace
//   int csws_rows            rows of Hp floats of column-sum scratch in the backward workspace
//   use_rt2(o, E1, Hp, sparse), mode2_fits(Hp), shape_ok(E1, Hp)      the predicates DESIGN.md 5.1 tabulates
// Host only: nothing here is device code, and nothing here allocates or reads the environment per launch.
#pragma once
#include "tile_mma.h"
#include <cstdlib>
#include <type_traits>

namespace {

constexpr size_t GGPM_LDS_LIMIT = 160 * 1024;      // dynamic LDS of a workgroup

template <typename K>
inline void set_lds(K kernel, size_t bytes) { ggpm_set_lds(kernel, bytes); }      // (common.h)

// Environment switches are read once: getenv walks the whole environment (~0.5 us) and the launch helpers run
// ~120 times per training step.
inline bool env_no_fuse_b() { static const bool v = ggpm_dev_env("GGPM_NO_FUSE_B") != nullptr; return v; }
inline bool env_adebug() { static const bool v = ggpm_dev_env("GGPM_ADEBUG") != nullptr; return v; }

inline int pick_tg(int E1, int NT) {
    static const char* const tg_env = ggpm_dev_env("GGPM_TG");
    if (const char* e = tg_env) { int v = atoi(e); if (v >= 1 && v <= 64) return v; }   // tuning override
    static const char* const tg_small_env = ggpm_dev_env("GGPM_TG_SMALL");
    if (const char* e = tg_small_env) {      // tuning override for the small (motif / attachment) levels only
        int v = atoi(e);
        if (v >= 1 && v <= 64 && (E1 + 15) / 16 <= 64) return v < NT ? v : NT;
    }
    static const char* const tg_large_env = ggpm_dev_env("GGPM_TG_LARGE");
    if (const char* e = tg_large_env) {      // tuning override for the large (atom) levels only
        int v = atoi(e);
        if (v >= 1 && v <= 64 && (E1 + 15) / 16 > 64) return v < NT ? v : NT;
    }
    return ggpm_tiles_per_group(E1, NT);
}

struct LdsNeed { int tiles, split_tiles, split_imgs; };      // fp32 operands: `tiles`; split operands: split_tiles + split_imgs
struct StepNeed { LdsNeed fused, a, b; };
inline size_t lds_tiles(int n, int Hp, int rows = 16) { return (size_t)n * rows * (Hp + 4) * sizeof(float); }
inline size_t lds_bytes(const LdsNeed& n, int rows, int Hp, bool split) {
    return split ? lds_tiles(n.split_tiles, Hp, rows) + n.split_imgs * ggpm_split_image_bytes(rows, Hp) : lds_tiles(n.tiles, Hp, rows);
}

// Gate mode of a level call (the kernels' GM): the caller's dtype 1 (bf16 operands) stays; an fp32 call runs its gate products
// on split operands (mode 2: fp32 accuracy on the bf16 matrix pipe, tile_mma.h) where that form is the faster one -- DENSE
// levels whose row tiles alone fill the chip (one column group: one 16-wave workgroup per 16 messages owns all gate columns,
// four waves per SIMD take turns on the pipe; the atom level: 33.9 -> 31.4 / 39.1 -> 35.8 us per launch, LSTM 46.2 -> 36.7 /
// 49.7 -> 42.0) and whose tiles and images fit the LDS (Cell::mode2_fits) -- and on fp32 MFMA (mode 0) otherwise: with column
// groups (the tree-side levels, the decode steps) ONE wave per SIMD streams three weight planes with nothing to hide their
// latency behind and the launch gets slower (attachment level gru_bwd_a 11.7 -> 16.7 us).  Sparse calls are always mode 0, so a
// sequence of them sharing one packed weight set (ggpm_level_opts.weights_packed) agrees on it.  dtype 3 forces mode 2 wherever it
// fits (tests); GGPM_GATE_SPLIT=0: mode 0 everywhere (A/B runs).
template <class Cell>
inline int gate_mode(const ggpm_level_opts& o, int Hp, bool rt2, bool single_group, bool sparse) {
    const int dtype = o.gate_dtype;
    if (dtype == 1) return 1;
    if (dtype == 2) return 0;
    static const bool on = [] { const char* e = ggpm_dev_env("GGPM_GATE_SPLIT"); return !e || atoi(e) != 0; }();
    if (!on || rt2) return 0;
    if (dtype != 3 && (!single_group || sparse)) return 0;
    return Cell::mode2_fits(Hp) ? 2 : 0;
}

// The form of a level call: its geometry (LevelPlan) and, per depth step, whether kernel A takes the B launch's product with
// it and the dynamic LDS of the two launches (StepLds).
struct LevelPlan { int tg; bool rt2; int gm; };      // tiles per column group, two row tiles per workgroup, gate mode 0 / 1 / 2
template <class Cell>
inline LevelPlan level_plan(const ggpm_level_opts& o, int E1, int Hp, bool sparse) {
    LevelPlan p;
    p.tg = pick_tg(E1, Hp / 16);
    p.rt2 = Cell::use_rt2(o, E1, Hp, sparse);
    p.gm = gate_mode<Cell>(o, Hp, p.rt2, p.tg >= Hp / 16, sparse);
    return p;
}
// K-split q' (ggpm_level_opts.q_part; GRU forward): a column group forms a partial q' over its own K slice of U_r inside kernel A
// and the next step's gather adds the partials, so only the last executed step keeps its B launch.  The geometry it applies
// to: fp32 MFMA, one row tile, 2 .. GGPM_KSPLIT_MAX_GROUPS column groups (the gather holds that many partial rows per
// predecessor in registers), at most two tiles of a group per wave (kernel A keeps their h' fragments in registers across
// the barrier that frees the LDS tile).  Dense calls only (the caller checks).  GGPM_KSPLIT_Q=0: off (A/B runs).
constexpr int GGPM_KSPLIT_MAX_GROUPS = 5;
inline bool ksplit_q_form(const LevelPlan& p, int Hp) {
    static const bool on = [] { const char* e = ggpm_dev_env("GGPM_KSPLIT_Q"); return !e || atoi(e) != 0; }();
    const int groups = ggpm_ceil_div(Hp / 16, p.tg);
    return on && p.gm == 0 && !p.rt2 && groups >= 2 && groups <= GGPM_KSPLIT_MAX_GROUPS && p.tg <= 2 * GGPM_NWA;
}
inline size_t q_part_floats(int E1, int Hp, int tg) { return (size_t)2 * ggpm_ceil_div(Hp / 16, tg) * E1 * Hp; }

struct StepLds { int fuse; size_t a, b; };      // b: what the B launch takes when there is one
// may_fuse: the step has a B product at all; the fused form needs one row tile, one column group and room in the LDS
inline StepLds step_lds(const StepNeed& need, int max_tiles, int Hp, int tg, bool rt2, int gm, bool may_fuse) {
    const int rows = rt2 ? 32 : 16, NT = Hp / 16;
    const bool split = gm == 2;
    const size_t fused = lds_bytes(need.fused, rows, Hp, split);
    StepLds p;
    p.fuse = (!rt2 && may_fuse && ggpm_ceil_div(NT, tg) == 1 && (!max_tiles || NT <= max_tiles) && fused <= GGPM_LDS_LIMIT &&
              !env_no_fuse_b()) ? 1 : 0;
    p.a = p.fuse ? fused : lds_bytes(need.a, rows, Hp, split);
    p.b = lds_bytes(need.b, rows, Hp, split);
    return p;
}
// a forward depth step; with_b: the step forms q' / qf' (every step but the level's last)
template <class Cell>
inline StepLds fwd_step(int Hp, int tg, bool rt2, int gm, bool with_b) {
    return step_lds(Cell::fwd, 0, Hp, tg, rt2, gm, with_b);
}
// a backward depth step; with_b: the step forms dS (dG) for the one below it; final_pass: the sparse backward's t = 0 launch
template <class Cell>
inline StepLds bwd_step(int Hp, int tg, bool rt2, int gm, bool with_b, bool final_pass) {
    return step_lds(Cell::bwd, Cell::bwd_fuse_max_tiles, Hp, tg, rt2, gm, with_b && !final_pass);
}

// ggpm_level_form_query (capi.hip) for one cell: the decisions above, nothing launched
template <class Cell>
inline int level_form(int E1, int H, int sparse, int training, const ggpm_level_opts& o, ggpm_level_form* out) {
    const int Hp = ggpm_padded_hidden(H);
    if (!Cell::shape_ok(E1, Hp)) return GGPM_ERR_UNSUPPORTED;
    const LevelPlan plan = level_plan<Cell>(o, E1, Hp, sparse != 0);
    const StepLds f = fwd_step<Cell>(Hp, plan.tg, plan.rt2, plan.gm, true);
    const StepLds b = bwd_step<Cell>(Hp, plan.tg, plan.rt2, plan.gm, true, false);
    *out = ggpm_level_form{};
    out->Hp = Hp; out->tiles = Hp / 16; out->tg = plan.tg; out->groups = ggpm_ceil_div(Hp / 16, plan.tg);
    out->rt2 = plan.rt2 ? 1 : 0; out->gate_mode = plan.gm;
    out->st16 = ggpm_level_st16(plan.gm, sparse != 0, training || o.h_out, E1, H) ? 1 : 0;
    out->fuse_fwd = f.fuse;
    out->lds_fwd_a = f.a; out->lds_fwd_b = (f.fuse && !sparse) ? 0 : f.b;      // (a sparse forward forms q^0 / qf^0 by a B launch)
    if (training) { out->fuse_bwd = b.fuse; out->lds_bwd_a = b.a; out->lds_bwd_b = b.fuse ? 0 : b.b; }
    return GGPM_OK;
}

// The kernel instantiation of a launch: f(GM, RTT, ST16) as integral constants, over exactly the variants that exist --
// bf16 storage: GM 1 (one row tile; two where Cell::rt2_bf16); two row tiles: GM 0 (and 1 where Cell::rt2_bf16); otherwise
// GM 0 / 1 / 2 on one row tile.
template <class Cell, class F>
inline void for_variant(bool st16, bool rt2, int gm, F&& f) {
    using std::integral_constant;
    constexpr integral_constant<int, 0> i0{}; constexpr integral_constant<int, 1> i1{}; constexpr integral_constant<int, 2> i2{};
    constexpr std::true_type yes{}; constexpr std::false_type no{};
    if (st16) {      // (training levels, and the forward-only form of such a level: ggpm_level_opts.h_out)
        if constexpr (Cell::rt2_bf16) { if (rt2) return f(i1, i2, yes); }
        f(i1, i1, yes);
    } else if (rt2) {
        if constexpr (Cell::rt2_bf16) { if (gm == 1) return f(i1, i2, no); }
        f(i0, i2, no);
    } else if (gm == 2) f(i2, i1, no);
    else if (gm == 1) f(i1, i1, no);
    else f(i0, i1, no);
}

// one A or B launch of a depth step: (row tiles) x (column groups of `tg` output tiles), GGPM_NWA waves
template <class Args>
inline dim3 step_grid(const Args& a, bool rt2) { return dim3(ggpm_ceil_div(a.E1, rt2 ? 32 : 16), ggpm_ceil_div(a.Hp / 16, a.tg)); }
template <class Args>
inline void launch_step(void (*kernel)(Args), const Args& a, bool rt2, size_t lds, hipStream_t s) {
    set_lds(kernel, lds);
    kernel<<<step_grid(a, rt2), GGPM_NWA * 64, lds, s>>>(a);
}

// The backward workspace of a level call, in order: the packed transposes (n_mat slots of the largest gate mode's size; first,
// because their place does not depend on E1 -- a sequence of calls that shares one `work` buffer and one set of weights packs
// them once, ggpm_level_opts.weights_packed), the gate-gradient stashes and DQ (`depth` slots of E1 * Hp floats each; DQ slot
// t = dq^t, slot 0 only used by sparse_forward), six scratch slots (double buffers and carries), the column-sum scratch,
// the split-K workspace.  work == nullptr: sizes only.
template <class Cell>
struct LevelWork {
    float* packedT;
    float* stash[Cell::n_stash];
    float* DQ;
    float* scratch[6];
    float* csws;
    float* skws;
    size_t floats;      // everything before skws
    size_t skbytes(size_t work_bytes) const { return work_bytes - floats * sizeof(float); }
};
template <class Cell>
inline LevelWork<Cell> carve(float* work, int E1, int Hp, int depth) {
    const size_t slot = (size_t)E1 * Hp;
    LevelWork<Cell> w;
    size_t f = 0;
    auto take = [&](size_t n) { float* p = work ? work + f : nullptr; f += n; return p; };
    w.packedT = take(Cell::n_mat * ggpm_packed_matrix_slot(Hp));
    for (int i = 0; i < Cell::n_stash; ++i) w.stash[i] = take((size_t)depth * slot);
    w.DQ = take((size_t)depth * slot);
    for (int i = 0; i < 6; ++i) w.scratch[i] = take(slot);
    w.csws = take((size_t)Cell::csws_rows * Hp);
    w.skws = take(0);
    w.floats = f;
    return w;
}
template <class Cell>
inline size_t backward_workspace_bytes(int E1, int H, int depth) {
    return carve<Cell>(nullptr, E1, ggpm_padded_hidden(H), depth).floats * sizeof(float) +
           ggpm_gemm_workspace_bytes(H, H, depth * E1) + 256;      // split-K slabs (largest contraction)
}

// One weight gradient dW = D^T B: a stash of the backward and the forward array its rows pair with.
struct WgradTerm { const float* D; const float* B; float* dW; int ld; };

// The contractions of a weight-gradient tail over rows that are already in place: n_gate terms of K rows each and the dq term
// of KQ rows, in ONE launch and one reduce (they share the split-K workspace); dbu (or null) = column sums of the dq rows -- the
// light column sum first, the contraction last.  KQ == 0: there is no dq row, its gradients are zero.
inline int tall_weight_grads(int H, int Hp, int n_gate, const WgradTerm* gate, int K, const WgradTerm& q, int KQ, float* dbu,
                             float* csws, bool st16, int tall_mode, float* skws, size_t skbytes, ggpm_stream_t stream) {
    ggpm_gemm_problem gp[GGPM_GEMM_MAX_GROUP];
    int Ks[GGPM_GEMM_MAX_GROUP];
    for (int i = 0; i < n_gate; ++i) {
        gp[i] = {gate[i].D, Hp, gate[i].B, Hp, gate[i].dW, gate[i].ld, H, nullptr, 0, GGPM_ACT_NONE, 0};
        Ks[i] = K;
    }
    gp[n_gate] = {q.D, Hp, q.B, Hp, q.dW, q.ld, H, nullptr, 0, GGPM_ACT_NONE, 0};
    Ks[n_gate] = KQ;
    int rc;
    if (KQ > 0) {
        if (dbu) {
            rc = ggpm_colsum_dtype(q.D, Hp, KQ, H, dbu, csws, st16, stream);
            if (rc) return rc;
        }
        rc = ggpm_gemm_tn_tall_grouped(H, H, n_gate + 1, gp, Ks, skws, skbytes, tall_mode, stream);
        if (rc) return rc;
    } else {
        rc = ggpm_gemm_tn_tall_grouped(H, H, n_gate, gp, Ks, skws, skbytes, tall_mode, stream);
        if (rc) return rc;
        for (int r = 0; r < H; ++r) (void)hipMemsetAsync(q.dW + (size_t)r * q.ld, 0, H * sizeof(float), (hipStream_t)stream);
        if (dbu) (void)hipMemsetAsync(dbu, 0, H * sizeof(float), (hipStream_t)stream);
    }
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

// The weight-gradient tail of a level: tall contractions over every (depth, message) row of the stashes the backward left in
// `work`.  gate[i].D / .B and q.D / q.B are the BASES of the stashes (gate stash slot t - 1 = backward step t; dq^t, in slot t,
// pairs with h^t); backward steps depth .. lo ran; with_slot0: a sparse level, whose dq^0 exists.  dbu: null for none.
inline int level_weight_grads(int E1, int H, int depth, int lo, bool with_slot0, const ggpm_level_opts& o, int n_gate,
                              const WgradTerm* gate, const WgradTerm& q, float* dbu, float* csws, float* skws, size_t skbytes,
                              ggpm_stream_t stream) {
    const int Hp = ggpm_padded_hidden(H);
    const size_t slot = (size_t)E1 * Hp;
    // bf16 storage (as the forward / backward decided): the stashes are bf16 in the first half of their buffers and the bf16
    // tall kernel reads them as they are
    const bool st16 = o.gate_dtype == 1 && !with_slot0 && ggpm_bf16_storage_applies(E1, H);
    const int tall_mode = st16 ? 2 : (o.gate_dtype == 1 ? 1 : 0);
    if (o.fixed_slot > 0 && !with_slot0) {
        // fixed-point level (ggpm_level_opts.fixed_slot): every forward block a step >= lo pairs with is the settled slot, so
        // dW = (sum_t D_t)^T B*, and db_u = colsum(sum_t DQ_t).  The slot sums do not round on their own: hi + lo pairs in
        // slots 0 / 1 of each stash (free: lo - 1 >= 2), K = 2 E1.
        const int fs = o.fixed_slot;
        if (fs >= depth || lo < fs || lo < 3 || o.gate_dtype == 1) return GGPM_ERR_ARG;
        const int nq = depth - lo;                         // dq^t exists for t = lo .. depth - 1
        const int n = nq > 0 ? n_gate + 1 : n_gate;
        const float* src[GGPM_GEMM_MAX_GROUP];
        int slots[GGPM_GEMM_MAX_GROUP];
        float *hi[GGPM_GEMM_MAX_GROUP], *lw[GGPM_GEMM_MAX_GROUP];
        ggpm_pair_problem pp[GGPM_GEMM_MAX_GROUP];
        for (int i = 0; i <= n_gate; ++i) {
            const WgradTerm& t = i < n_gate ? gate[i] : q;
            const int first = i < n_gate ? lo - 1 : lo;
            src[i] = t.D + (size_t)first * slot; slots[i] = depth - first;
            hi[i] = const_cast<float*>(t.D); lw[i] = hi[i] + slot;
            pp[i] = {hi[i], lw[i], t.B + (size_t)(i < n_gate ? fs - 1 : fs) * slot, t.dW, t.ld};
        }
        int rc = ggpm_sum_slots_pair_grouped(n, src, slots, slot, hi, lw, stream);
        if (rc) return rc;
        if (nq > 0) {
            if (dbu) {      // hi and lo are adjacent slots: one column sum over both
                rc = ggpm_colsum(q.D, Hp, 2 * E1, H, dbu, csws, stream);
                if (rc) return rc;
            }
        } else {
            for (int r = 0; r < H; ++r) (void)hipMemsetAsync(q.dW + (size_t)r * q.ld, 0, H * sizeof(float), (hipStream_t)stream);
            if (dbu) (void)hipMemsetAsync(dbu, 0, H * sizeof(float), (hipStream_t)stream);
        }
        rc = ggpm_gemm_tn_pair_grouped_c(H, H, E1, Hp, n, pp, stream);
        if (rc) return rc;
        GGPM_CHECK_LAUNCH();
        return GGPM_OK;
    }
    WgradTerm g[GGPM_GEMM_MAX_GROUP];
    for (int i = 0; i < n_gate; ++i)
        g[i] = {ggpm_slot_ptr(gate[i].D, lo - 1, slot, st16), ggpm_slot_ptr(gate[i].B, lo - 1, slot, st16), gate[i].dW, gate[i].ld};
    // the dense level never produces dq^0 (h^0 = 0), sparse_forward does
    const int first_slot = with_slot0 ? 0 : lo;
    const WgradTerm dq = {ggpm_slot_ptr(q.D, first_slot, slot, st16), ggpm_slot_ptr(q.B, first_slot, slot, st16), q.dW, q.ld};
    return tall_weight_grads(H, Hp, n_gate, g, (depth - lo + 1) * E1, dq, (depth - first_slot) * E1, dbu, csws, st16, tall_mode,
                             skws, skbytes, stream);
}

}  // namespace
