// One level call of the message function, for both cells: what the C++ drivers (encoder.hip, decode.hip, tree_level.hip) and the
// extern "C" entry points of mpn_gru.hip / mpn_lstm.hip hand to the impl functions.  Every operand is named once; the
// per-gate operands are arrays in the gate order Python and ggpm_decode_steps_* use:
//   GRU   X planes z, r, h;  hidden matrices Wz_h, U_r, Wh_h (+ b_u);  gradients dWz_h, dU_r, dWh_h (+ db_u);  St = S, G, Z, M, R
//   LSTM  i, o, u, f throughout;                                                                                St = S, I, O, U, F
// Fields a cell or a direction does not use stay null.  One struct serves both directions: the forward writes Hs / Cs / Qs /
// St, the backward only reads them.  Host only, not part of include/ggpm_hip.h, nothing exported.
#pragma once
#include "common.h"

struct LevelCall {
    bool lstm;
    int rows, H, depth;
    // forward operands
    const float* X[4];                  // hoisted gate inputs (the backward reads plane CellGates::reread only)
    const float* W[4];                  // hidden matrices
    int ldw[4];
    const float* bu;                    // GRU
    const int32_t *pred_rowptr, *pred_col, *succ_rowptr, *succ_col;      // (succ: the backward)
    float *Hs, *Cs, *Qs, *St[5], *wpack;
    // sparse operands: frozen != null selects the sparse form
    const unsigned char* frozen;
    const float *h_in, *c_in;
    // backward operands
    const float *d_out, *dc_out;        // d(h_D); sparse LSTM: d(c_D)
    float *d_in, *dc_in;                // sparse: gradient of the incoming state
    float *dX[4], *dW[4];
    int ld_dw[4];
    float* dbu;                         // GRU
    float* work;
    size_t work_bytes;
};
// for a backward caller that holds the forward's arrays as const (the backward only reads them)
inline float* level_read(const float* p) { return const_cast<float*>(p); }

// What the drivers need to know about a cell's gates (DESIGN.md 5.1 has the table).
struct CellGates {
    int n;                  // gates = X planes = hidden matrices
    int reread;             // the X plane the backward reads again (GRU r, LSTM f)
    bool full[4];           // the gate's weight is [H, I + H] and has a bias (W_r: [H, I], no bias -- U_r and b_u stand alone)
    int n_sum;              // gate-gradient stashes of the backward workspace ...
    struct { int stash, plane; } sum[3];      // ... and the dX plane each sums to under skip_x_sums, in launch order
};
constexpr CellGates GRU_GATES = {3, 1, {true, false, true, false}, 2, {{1, 0}, {0, 2}, {0, 0}}};      // DZP -> dXz, DMP -> dXh
constexpr CellGates LSTM_GATES = {4, 3, {true, true, true, true}, 3, {{0, 0}, {1, 1}, {2, 2}}};       // DI, DO, DU
inline const CellGates& cell_gates(bool lstm) { return lstm ? LSTM_GATES : GRU_GATES; }

// the impl functions (mpn_gru.hip, mpn_lstm.hip); `lo`: backward steps depth .. lo ran
int gru_forward_impl(const LevelCall& c, int save_for_backward, const ggpm_level_opts& o, ggpm_stream_t stream);
int gru_backward_impl(const LevelCall& c, int weight_grads, const ggpm_level_opts& o, ggpm_stream_t stream);
int gru_weight_grads_impl(const LevelCall& c, int lo, const ggpm_level_opts& o, ggpm_stream_t stream);
int lstm_forward_impl(const LevelCall& c, int save_for_backward, const ggpm_level_opts& o, ggpm_stream_t stream);
int lstm_backward_impl(const LevelCall& c, int weight_grads, const ggpm_level_opts& o, ggpm_stream_t stream);
int lstm_weight_grads_impl(const LevelCall& c, int lo, const ggpm_level_opts& o, ggpm_stream_t stream);

inline int ggpm_level_forward(const LevelCall& c, bool save, const ggpm_level_opts* opts, ggpm_stream_t stream) {
    if (c.frozen && (!c.h_in || (c.lstm && !c.c_in))) return GGPM_ERR_ARG;
    const ggpm_level_opts& o = ggpm_opts_or_default(opts);
    return c.lstm ? lstm_forward_impl(c, save, o, stream) : gru_forward_impl(c, save, o, stream);
}
inline int ggpm_level_backward(const LevelCall& c, int weight_grads, const ggpm_level_opts* opts, ggpm_stream_t stream) {
    if (c.frozen && (!c.d_in || (c.lstm && !c.dc_in))) return GGPM_ERR_ARG;
    const ggpm_level_opts& o = ggpm_opts_or_default(opts);
    return c.lstm ? lstm_backward_impl(c, weight_grads, o, stream) : gru_backward_impl(c, weight_grads, o, stream);
}
// the weight gradients a backward without them left out, dense (opts->lo as the backward had it) or sparse
inline int ggpm_level_weight_grads(const LevelCall& c, const ggpm_level_opts* opts, ggpm_stream_t stream) {
    const ggpm_level_opts& o = ggpm_opts_or_default(opts);
    return c.lstm ? lstm_weight_grads_impl(c, o.lo, o, stream) : gru_weight_grads_impl(c, o.lo, o, stream);
}
inline size_t ggpm_level_pack_floats(bool lstm, int H) { return lstm ? ggpm_lstm_pack_floats(H) : ggpm_gru_pack_floats(H); }
inline size_t ggpm_level_backward_workspace_bytes(bool lstm, int rows, int H, int depth) {
    return lstm ? ggpm_lstm_backward_workspace_bytes(rows, H, depth) : ggpm_gru_backward_workspace_bytes(rows, H, depth);
}
