// Step loop of the teacher-forced decoder's atom level as ONE C call per direction.
//
// Reference: HierMPNDecoder.forward calls IncHierMPNEncoder.forward once per decode step (ggpm/decoder.py:201-222); its
// atom-level block (ggpm/encoder.py:235-239 -> IncMPNEncoder.forward, :165-179) recomputes the bond messages of the
// step's motif with `diterG` iterations of sparse_forward (ggpm/rnn.py:52-59, 110-121).  ggpm_amd/atom_decode.py runs
// every step on its compact row set (the step's bonds + the frozen older bonds they read) out of stacked state / stash
// buffers; what is left inside the loop is `gather the frozen rows -> sparse_forward` and, backwards,
// `sparse_backward -> scatter-add to the rows' producers`.  These two drivers issue exactly those calls, in the same
// order, from C++: ~25 launches per step and direction that Python + ctypes otherwise issue one by one (the full VAE step
// is as long on the host as on the GPU).
#include "common.h"
#include "level_call.h"
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>

namespace {

// GGPM_DECODE_FOLD=0 (dev A/B, tests): the start-state gather and the incoming-gradient scatter of every decode step as
// launches of their own instead of inside the step's first / last launch
inline bool decode_fold() { static const bool v = [] { const char* e = ggpm_dev_env("GGPM_DECODE_FOLD"); return !e || atoi(e) != 0; }(); return v; }

struct Offs { size_t f0, r0, q0; };      // first F id of the step, first row of its [depth][n] and [depth + 1][n] blocks
inline Offs offs(const ggpm_decode_steps* d, int t) { return {(size_t)d->foff[t], (size_t)d->roff[t], (size_t)d->qoff[t]}; }

// what every level call of a step loop shares: shape, cell, hidden matrices (gate order: level_call.h)
inline LevelCall step_call(const ggpm_decode_steps* d, const float* const* W, const int* ldw, const float* bu) {
    LevelCall c = {};
    c.lstm = d->lstm != 0; c.H = d->H; c.depth = d->depth; c.bu = bu;
    for (int k = 0; k < cell_gates(c.lstm).n; ++k) { c.W[k] = W[k]; c.ldw[k] = ldw[k]; }
    return c;
}
// ... and what step t adds: its rows, CSRs, frozen mask and the X planes of its block
inline void set_step(LevelCall& c, const ggpm_decode_steps* d, int t, const float* x) {
    c.rows = d->n[t]; c.frozen = d->frozen[t];
    c.pred_rowptr = d->pred_rowptr[t]; c.pred_col = d->pred_col[t]; c.succ_rowptr = d->succ_rowptr[t]; c.succ_col = d->succ_col[t];
    for (int k = 0; k < cell_gates(c.lstm).n; ++k) c.X[k] = x + (size_t)k * c.rows * ggpm_padded_hidden(c.H);
}

inline bool steps_ok(const ggpm_decode_steps* d) {
    return d && d->T > 0 && d->H > 0 && d->depth > 0 && d->n && d->foff && d->roff && d->qoff && d->srcH && d->srcF &&
           d->frozen && d->pred_rowptr && d->pred_col && d->succ_rowptr && d->succ_col;
}

}  // namespace

extern "C" int ggpm_decode_steps_forward(const ggpm_decode_steps* d, const float* const* W, const int* ldw, const float* bu,
                                         const float* X_all, float* Hs_all, float* Cs_all, float* Qs_all, float* St_all,
                                         size_t st_stride, float* wpack, float* tmp, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!steps_ok(d) || !W || !ldw || !X_all || !Hs_all || !Qs_all || !St_all || !wpack || !tmp || (d->lstm && !Cs_all) ||
        (!d->lstm && !bu))
        return GGPM_ERR_ARG;
    LevelCall c = step_call(d, W, ldw, bu);
    const int Hp = ggpm_padded_hidden(d->H), G = cell_gates(c.lstm).n;
    c.wpack = wpack;
    const bool fold = decode_fold();
    for (int t = 0; t < d->T; ++t) {
        const Offs o = offs(d, t);
        set_step(c, d, t, X_all + (size_t)G * o.f0 * Hp);
        c.Hs = Hs_all + o.q0 * Hp;
        c.Cs = c.lstm ? Cs_all + o.q0 * Hp : nullptr;
        c.Qs = Qs_all + o.r0 * Hp;
        for (int k = 0; k < 5; ++k) c.St[k] = St_all + (size_t)k * st_stride + o.r0 * Hp;
        c.h_in = c.Hs; c.c_in = c.Cs;
        // the step's start state goes straight into slot 0 of its block: frozen rows from the blocks of the steps that
        // produced them, zero for the rows the step recomputes (srcH = -1) -- exactly the masked state sparse_forward would
        // build.  The step's first launch (q^0 = U_r h^0 / qf^0 = Wf_h h^0) fetches the rows through srcH and writes slot 0
        // on the way (ggpm_level_opts.gather_*); GGPM_DECODE_FOLD=0: a gather launch of its own, as before.
        ggpm_level_opts opts = {};
        opts.weights_packed = t > 0;      // same weights, same `wpack`: packed by the first step
        int rc = GGPM_OK;
        if (fold) {
            opts.gather_h = Hs_all; opts.gather_c = Cs_all; opts.gather_idx = d->srcH[t];
        } else {
            rc = ggpm_gather_rows(Hs_all, Hp, d->srcH[t], c.rows, Hp, c.Hs, Hp, 0, 0, stream);
            if (!rc && c.lstm) rc = ggpm_gather_rows(Cs_all, Hp, d->srcH[t], c.rows, Hp, c.Cs, Hp, 0, 0, stream);
            if (rc) return rc;
        }
        rc = ggpm_level_forward(c, true, &opts, stream);
        if (rc) return rc;
    }
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

// Forward-only form: the same sparse_forward calls in the same order without stashes.  Every step runs its depth loop in
// the ping-pong scratch Hs / Qs (/ Cs) and writes its rows' final states to F_h / F_c at its F ids (ggpm_level_opts.h_out);
// the frozen rows of later steps are gathered from there through srcF.
extern "C" int ggpm_decode_steps_infer(const ggpm_decode_steps* d, const float* const* W, const int* ldw, const float* bu,
                                       const float* X_all, float* F_h, float* F_c, float* Hs, float* Cs, float* Qs,
                                       float* wpack, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!steps_ok(d) || !W || !ldw || !X_all || !F_h || !Hs || !Qs || !wpack || (d->lstm && (!F_c || !Cs)) ||
        (!d->lstm && !bu))
        return GGPM_ERR_ARG;
    LevelCall c = step_call(d, W, ldw, bu);
    const int Hp = ggpm_padded_hidden(d->H), G = cell_gates(c.lstm).n;
    c.Hs = Hs; c.Cs = Cs; c.Qs = Qs; c.wpack = wpack;
    c.h_in = Hs; c.c_in = Cs;
    const bool fold = decode_fold();
    for (int t = 0; t < d->T; ++t) {
        const Offs o = offs(d, t);
        set_step(c, d, t, X_all + (size_t)G * o.f0 * Hp);
        ggpm_level_opts opts = {};
        opts.weights_packed = t > 0;
        opts.h_out = F_h + o.f0 * Hp;
        opts.c_out = c.lstm ? F_c + o.f0 * Hp : nullptr;
        int rc = GGPM_OK;
        if (fold) {
            opts.gather_h = F_h; opts.gather_c = F_c; opts.gather_idx = d->srcF[t];
        } else {
            rc = ggpm_gather_rows(F_h, Hp, d->srcF[t], c.rows, Hp, Hs, Hp, 0, 0, stream);
            if (!rc && c.lstm) rc = ggpm_gather_rows(F_c, Hp, d->srcF[t], c.rows, Hp, Cs, Hp, 0, 0, stream);
            if (rc) return rc;
        }
        rc = ggpm_level_forward(c, false, &opts, stream);
        if (rc) return rc;
    }
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

extern "C" int ggpm_decode_steps_backward(const ggpm_decode_steps* d, const float* const* W, const int* ldw,
                                          const float* X_all, const float* Hs_all, const float* Cs_all, const float* Qs_all,
                                          const float* St_all, size_t st_stride, float* dF, float* dCF, float* dX_all,
                                          float* DG_all, size_t dg_stride, float* DQ_all, float* const* dW_unused,
                                          float* work, size_t work_bytes, float* tmp, ggpm_stream_t stream) {
    GGPM_CLEAR_STALE_ERROR();
    if (!steps_ok(d) || !W || !ldw || !X_all || !Hs_all || !Qs_all || !St_all || !dF || !dX_all || !DG_all || !DQ_all ||
        !dW_unused || !work || !tmp || (d->lstm && (!Cs_all || !dCF)))
        return GGPM_ERR_ARG;
    LevelCall c = step_call(d, W, ldw, nullptr);
    const int Hp = ggpm_padded_hidden(d->H), G = cell_gates(c.lstm).n;
    int nmax = 0;
    for (int t = 0; t < d->T; ++t) nmax = d->n[t] > nmax ? d->n[t] : nmax;
    c.d_in = tmp;                                  // the frozen rows' gradient of one step
    c.dc_in = tmp + (size_t)nmax * Hp;
    // the weight gradients are deferred (defer_stash): what a level call would write them to is never written
    for (int k = 0; k < G; ++k) { c.dW[k] = dW_unused[k]; c.ld_dw[k] = d->H; }
    c.dbu = dW_unused[3];                          // (GRU)
    c.work = work; c.work_bytes = work_bytes;
    const bool fold = decode_fold();
    for (int t = d->T - 1; t >= 0; --t) {
        const Offs o = offs(d, t);
        set_step(c, d, t, X_all + (size_t)G * o.f0 * Hp);
        for (int k = 0; k < G; ++k) c.dX[k] = dX_all + ((size_t)G * o.f0 + (size_t)k * c.rows) * Hp;
        c.Hs = level_read(Hs_all) + o.q0 * Hp;
        c.Cs = c.lstm ? level_read(Cs_all) + o.q0 * Hp : nullptr;
        c.Qs = level_read(Qs_all) + o.r0 * Hp;
        for (int k = 0; k < 5; ++k) c.St[k] = level_read(St_all) + (size_t)k * st_stride + o.r0 * Hp;
        c.d_out = dF + o.f0 * Hp;
        c.dc_out = c.lstm ? dCF + o.f0 * Hp : nullptr;
        ggpm_level_opts opts = {};
        opts.weights_packed = t < d->T - 1;      // same weights, same `work`: the transposes were packed by the first call
        // the frozen rows' gradient goes to the step that produced their state (rows recomputed here: none): added there by
        // the step's last launch (ggpm_level_opts.scatter_*), or by scatter launches of their own
        if (fold) { opts.scatter_h = dF; opts.scatter_c = dCF; opts.scatter_idx = d->srcF[t]; }
        // the stashes go to the stacked buffers, contracted once after the loop (ggpm_*_weight_grads_stacked)
        const int ns = cell_gates(c.lstm).n_sum;      // the gate-gradient stashes, then dq
        for (int k = 0; k < ns; ++k) opts.defer_stash[k] = DG_all + (size_t)k * dg_stride + o.r0 * Hp;
        opts.defer_stash[ns] = DQ_all + o.q0 * Hp;
        int rc = ggpm_level_backward(c, 1, &opts, stream);
        if (rc) return rc;
        if (!fold && c.lstm) rc = ggpm_scatter_rows(c.dc_in, Hp, d->srcF[t], c.rows, Hp, dCF, Hp, 1, stream);
        if (!fold && !rc) rc = ggpm_scatter_rows(c.d_in, Hp, d->srcF[t], c.rows, Hp, dF, Hp, 1, stream);
        if (rc) return rc;
    }
    GGPM_CHECK_LAUNCH();
    return GGPM_OK;
}

// ---- issuing the step loops from a worker thread ------------------------------------------------------------------------
// A step loop is ~280 launches = 1.5-1.8 ms of host time inside ONE call.  While the calling thread sits in it, nothing else
// of the training step can be issued: in the backward pass the autograd engine reaches the atom level's node and the
// encoder's node at about the same time, and whichever it takes second starts that much later on the GPU although the two
// chains do not depend on each other ("the two chains have to be ISSUED side by side").  The _async
// forms hand the loop to a thread of the library and return at once; ggpm_decode_join waits until that thread has issued
// everything (it does not wait for the GPU).  The caller keeps every buffer and the descriptor alive until then and
// enqueues what follows the loop on the same stream only after the join.  One worker, jobs in order.
namespace {

class DecodeWorker {
public:
    static DecodeWorker& get() { static DecodeWorker w; return w; }
    void post(int dev, std::function<int()> job) {
        { std::lock_guard<std::mutex> lk(mu_); q_.push_back({dev, std::move(job)}); }
        cv_.notify_one();
    }
    int join() {
        std::unique_lock<std::mutex> lk(mu_);
        idle_.wait(lk, [&] { return q_.empty() && !busy_; });
        const int e = err_;
        err_ = GGPM_OK;
        return e;
    }

private:
    DecodeWorker() : th_([this] { run(); }) {}
    ~DecodeWorker() {
        { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
        cv_.notify_one();
        if (th_.joinable()) th_.join();
    }
    void run() {
        int dev = -1;
        for (;;) {
            std::pair<int, std::function<int()>> job;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || !q_.empty(); });
                if (q_.empty()) return;
                job = std::move(q_.front());
                q_.pop_front();
                busy_ = true;
            }
            if (job.first != dev && job.first >= 0) { (void)hipSetDevice(job.first); dev = job.first; }
            int rc = job.second();
            if (!rc && hipGetLastError() != hipSuccess) rc = GGPM_ERR_LAUNCH;
            {
                std::lock_guard<std::mutex> lk(mu_);
                if (rc && !err_) err_ = rc;
                busy_ = false;
                if (q_.empty()) idle_.notify_all();
            }
        }
    }
    std::mutex mu_;
    std::condition_variable cv_, idle_;
    std::deque<std::pair<int, std::function<int()>>> q_;
    bool busy_ = false, stop_ = false;
    int err_ = GGPM_OK;
    std::thread th_;
};

inline int current_device() { int d = -1; (void)hipGetDevice(&d); return d; }

}  // namespace

extern "C" int ggpm_decode_steps_forward_async(const ggpm_decode_steps* d, const float* const* W, const int* ldw, const float* bu,
                                               const float* X_all, float* Hs_all, float* Cs_all, float* Qs_all, float* St_all,
                                               size_t st_stride, float* wpack, float* tmp, ggpm_stream_t stream) {
    if (!d || !W || !ldw) return GGPM_ERR_ARG;
    const float* Wc[4] = {W[0], W[1], W[2], W[3]};
    const int lc[4] = {ldw[0], ldw[1], ldw[2], ldw[3]};
    DecodeWorker::get().post(current_device(), [=]() -> int {
        return ggpm_decode_steps_forward(d, Wc, lc, bu, X_all, Hs_all, Cs_all, Qs_all, St_all, st_stride, wpack, tmp, stream);
    });
    return GGPM_OK;
}

extern "C" int ggpm_decode_steps_backward_async(const ggpm_decode_steps* d, const float* const* W, const int* ldw,
                                                const float* X_all, const float* Hs_all, const float* Cs_all,
                                                const float* Qs_all, const float* St_all, size_t st_stride, float* dF,
                                                float* dCF, float* dX_all, float* DG_all, size_t dg_stride, float* DQ_all,
                                                float* const* dW_unused, float* work, size_t work_bytes, float* tmp,
                                                ggpm_stream_t stream) {
    if (!d || !W || !ldw || !dW_unused) return GGPM_ERR_ARG;
    const float* Wc[4] = {W[0], W[1], W[2], W[3]};
    const int lc[4] = {ldw[0], ldw[1], ldw[2], ldw[3]};
    float* dWc[4] = {dW_unused[0], dW_unused[1], dW_unused[2], dW_unused[3]};
    DecodeWorker::get().post(current_device(), [=]() -> int {
        return ggpm_decode_steps_backward(d, Wc, lc, X_all, Hs_all, Cs_all, Qs_all, St_all, st_stride, dF, dCF, dX_all, DG_all,
                                          dg_stride, DQ_all, dWc, work, work_bytes, tmp, stream);
    });
    return GGPM_OK;
}

extern "C" int ggpm_decode_steps_infer_async(const ggpm_decode_steps* d, const float* const* W, const int* ldw, const float* bu,
                                             const float* X_all, float* F_h, float* F_c, float* Hs, float* Cs, float* Qs,
                                             float* wpack, ggpm_stream_t stream) {
    if (!d || !W || !ldw) return GGPM_ERR_ARG;
    const float* Wc[4] = {W[0], W[1], W[2], W[3]};
    const int lc[4] = {ldw[0], ldw[1], ldw[2], ldw[3]};
    DecodeWorker::get().post(current_device(), [=]() -> int {
        return ggpm_decode_steps_infer(d, Wc, lc, bu, X_all, F_h, F_c, Hs, Cs, Qs, wpack, stream);
    });
    return GGPM_OK;
}

extern "C" int ggpm_decode_join(void) { return DecodeWorker::get().join(); }
