/*
 * ggpm_hip.h -- C ABI of the MI355X (gfx950) hierarchical message-passing library.
 *
 * The reference (quocdat32461997/ggpm) is pure Python/PyTorch and has NO native
 * interface for this path; the seam is Python class substitution.
 * Each entry point below therefore cites the reference *Python* lines whose
 * arithmetic it replaces.  All paths are relative to the reference checkout.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (the host side uses the
 *     PyTorch caching allocator); the library allocates nothing and keeps no state;
 *   - fp32 row-major matrices with an explicit leading dimension (in floats);
 *     index arrays are int32 (CSR) or the int64 padded tensors MolGraph.tensorize
 *     delivers (ggpm/mol_graph.py:199-281, ggpm/nnutils.py:210-214);
 *   - "E1"/"N1" row counts INCLUDE the pad row 0 of the reference layout;
 *   - feature matrices use a padded row stride Hp = ggpm_padded_hidden(H)
 *     (multiple of 16); pad columns are zero on input and kept zero on output;
 *   - work is enqueued on `stream` (a hipStream_t) and never synchronised;
 *   - return value 0 = ok, otherwise a GGPM_ERR_* code (ggpm_error_string()).
 *     Nothing aborts; the Python wrappers raise RuntimeError.
 *   - re-entrant: no globals, safe from autograd's worker threads.
 */
#ifndef GGPM_HIP_H
#define GGPM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ggpm_stream_t; /* hipStream_t */

enum {
    GGPM_OK = 0,
    GGPM_ERR_ARG = 1,         /* bad size / null pointer / misaligned leading dimension */
    GGPM_ERR_LAUNCH = 2,      /* hipGetLastError() != hipSuccess after a launch */
    GGPM_ERR_UNSUPPORTED = 3, /* shape outside what the kernels were built for */
    GGPM_ERR_WORKSPACE = 4    /* workspace too small */
};

enum { GGPM_ACT_NONE = 0, GGPM_ACT_RELU = 1, GGPM_ACT_TANH = 2, GGPM_ACT_SIGMOID = 3 };

int ggpm_version(void);
const char* ggpm_error_string(int code);
/* Padded feature stride used by the message kernels: H rounded up to a multiple of 16. */
int ggpm_padded_hidden(int H);

/* ------------------------------------------------------------------ graph layout
 * A0 (ggpm/mol_graph.py:238-281, create_pad_tensor ggpm/nnutils.py:105-110): agraph/bgraph/cgraph
 * arrive as zero-padded int64 [rows, width]; entry 0 means "no neighbour" (row 0 is the pad row, so
 * index 0 always gathers zeros in the reference).  These build the equivalent CSR over the real
 * entries, which is what makes the padded gather of index_select_ND (ggpm/nnutils.py:65-70) unnecessary.
 */
/* rowptr[rows+1], col[>= rows*width]; entries keep their in-row order. */
int ggpm_padded_to_csr(const int64_t* padded, int rows, int width, int32_t* rowptr, int32_t* col,
                       ggpm_stream_t stream);
/* Two ggpm_padded_to_csr in one launch (one workgroup per list when both are small; the plain calls otherwise). */
int ggpm_padded_to_csr_pair(const int64_t* padded_a, int rows_a, int width_a, int32_t* rowptr_a, int32_t* col_a,
                            const int64_t* padded_b, int rows_b, int width_b, int32_t* rowptr_b, int32_t* col_b,
                            ggpm_stream_t stream);
/* Transpose of a CSR whose column ids lie in [0, ncols): rowptrT[ncols+1], colT[>= nnz capacity]
 * hold, for every column id, the ascending list of rows that reference it (deterministic order);
 * `cursor` is int32 scratch of ncols entries. Used for the atomics-free backward gathers. */
int ggpm_csr_transpose(const int32_t* rowptr, const int32_t* col, int rows, int ncols,
                       int32_t* rowptrT, int32_t* colT, int32_t* cursor, ggpm_stream_t stream);
/* out[r] = (int32) mat[r*width + column]   (e.g. fmess[:,0], fnode[:,1]) */
int ggpm_extract_column(const int64_t* mat, int rows, int width, int column, int32_t* out,
                        ggpm_stream_t stream);

/* ------------------------------------------------------------------ dense algebra (fp32 MFMA)
 * C[m,n] = act( sum_k A'(m,k) B'(k,n) + bias[n] + (accumulate ? C[m,n] : 0) ),
 *   A'(m,k) = trans_a ? A[k*lda+m] : A[m*lda+k],   B'(k,n) = trans_b ? B[n*ldb+k] : B[k*ldb+n].
 * Columns N..n_pad-1 of C are zero-filled (n_pad <= ldc; pass n_pad = N for none); zero_row0 forces
 * row 0 of C to zero (the reference's "first node/message is padding" masks, ggpm/encoder.py:36-38).
 * Replaces nn.Linear on this path (ggpm/rnn.py:13-16,69-72, ggpm/encoder.py:15-19,62-82) and autograd's
 * mm/addmm for its gradients.  `splitk_ws` (may be NULL) enables a deterministic split-K reduction for
 * tall contractions (weight gradients over depth*E rows); it needs ggpm_gemm_workspace_bytes() bytes.
 */
size_t ggpm_gemm_workspace_bytes(int M, int N, int K);
int ggpm_gemm(int trans_a, int trans_b, int M, int N, int K, const float* A, int lda, const float* B,
              int ldb, float* C, int ldc, int n_pad, const float* bias, int accumulate, int act,
              int zero_row0, float* splitk_ws, size_t splitk_ws_bytes, ggpm_stream_t stream);
/* Several products in ONE launch (the motif / attachment levels have a few hundred rows, so one product fills a
 * fraction of the chip and is bound by launch latency):
 *   ggpm_gemm_grouped   -- `count` (<= 4) independent products of the same (M, N, K, transposes), e.g. the gate input
 *                          projections x W_z^T, x W_r^T, x W_h^T of GRU.forward (ggpm/rnn.py:25-39; LSTM: rnn.py:85-94);
 *   ggpm_gemm_ksegments -- C = act(sum_s A_s B_s' + bias (+ C)) over `nseg` (<= 4) K segments in one accumulator chain:
 *                          A_s is [M x K_s] row-major, B_s is [K_s x N] (trans_b = 0) or [N x K_s] (trans_b = 1), each
 *                          with its own leading dimension -- nn.Linear over a torch.cat of inputs without the cat
 *                          (ggpm/encoder.py:31-35,62-82), and its input gradient summed over the gate slabs.
 * Both fall back to a sequence of ggpm_gemm calls when an operand does not allow 16-byte loads.
 */
typedef struct ggpm_gemm_problem {
    const float* A; int lda;
    const float* B; int ldb;
    float* C; int ldc; int n_pad;
    const float* bias;
    int accumulate, act, zero_row0;
} ggpm_gemm_problem;
int ggpm_gemm_grouped(int trans_a, int trans_b, int M, int N, int K, int count, const ggpm_gemm_problem* problems,
                      ggpm_stream_t stream);
/* ggpm_gemm_grouped with the K range cut into chunks (deterministic: partial tiles to `ws`, summed in fixed order by a
 * second launch that applies bias / accumulate / activation): for groups with few output tiles and a long K -- the input
 * halves dW[:, :I] = dX^T x of a level's gate weights (autograd's mm backward of the nn.Linear layers of ggpm/rnn.py:13-16,
 * 69-72 over all E messages), whose 60 tiles would otherwise walk 2 848 rows each.  `ws` needs
 * ggpm_gemm_grouped_splitk_workspace_bytes() bytes; when that is 0 (nothing to split) or `ws` is NULL / too small the call
 * is ggpm_gemm_grouped. */
size_t ggpm_gemm_grouped_splitk_workspace_bytes(int M, int N, int K, int count);
int ggpm_gemm_grouped_splitk(int trans_a, int trans_b, int M, int N, int K, int count, const ggpm_gemm_problem* problems,
                             float* ws, size_t ws_bytes, ggpm_stream_t stream);
/* ggpm_gemm_grouped (count >= 1) with two epilogue options per problem, so that the launches around a product can go:
 *   addend   -- with problems[i].accumulate != 0 the product is added to addend[m, n] (leading dimension ld_addend) instead
 *               of to C[m, n]: the same value in the same place of the same sum as accumulating onto a copy of `addend`;
 *   mask_out -- mask_out[m, n] = ggpm_act_backward(C, mask_y, ..., mask_act, mask_zero_row0) of the value just stored to
 *               C (both with leading dimension ld_mask; NULL: no second output).
 * Runs on the small-tile kernel only: GGPM_ERR_UNSUPPORTED (nothing launched) when an operand does not allow 16-byte
 * loads or the group has too many tiles for it; the caller then issues copy, product and ggpm_act_backward itself. */
typedef struct ggpm_gemm_epilogue {
    const float* addend; int ld_addend;
    const float* mask_y; float* mask_out; int ld_mask, mask_act, mask_zero_row0;
} ggpm_gemm_epilogue;
int ggpm_gemm_grouped_masked(int trans_a, int trans_b, int M, int N, int K, int count, const ggpm_gemm_problem* problems,
                             const ggpm_gemm_epilogue* epilogues, ggpm_stream_t stream);
int ggpm_gemm_ksegments(int trans_b, int M, int N, int nseg, const float* const* A, const int* lda,
                        const float* const* B, const int* ldb, const int* K, float* C, int ldc, int n_pad,
                        const float* bias, int accumulate, int act, int zero_row0, ggpm_stream_t stream);
/* C[M x N] = rne_bf16(A)^T rne_bf16(B), fp32 accumulate (v_mfma_f32_16x16x32_bf16), A [K x lda] and B [K x ldb] row-major
 * fp32: the tall weight-gradient contraction dW = dY^T X over K = depth*E stash rows -- autograd's mm backward of the
 * hidden x hidden gate products of GRU.GRU / LSTM.LSTM (ggpm/rnn.py:27-36, 88-91) -- with bf16 operands, as the level
 * calls use it under gate_dtype = bf16 (BASELINE configs[4]).  `ws`: ggpm_gemm_workspace_bytes(M, N, K) bytes (split-K
 * slabs, summed in fixed order).  Shapes the tall kernel does not take (K < 6144, a 160 x 160 tiling that would be
 * mostly padding, operands not 16-byte aligned) are computed on fp32 operands by ggpm_gemm instead. */
int ggpm_gemm_tn_bf16(int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc, float* ws,
                      size_t ws_bytes, ggpm_stream_t stream);
/* 1 when a contraction of this shape runs on bf16 operands (host-only query; 16-byte aligned operands assumed). */
int ggpm_gemm_tn_bf16_applies(int M, int N, int K);
/* A batch of Linear weight gradients in one call: item i forms dW_i[N x K] = dpre_i[M x N]^T x_i[M x K] (ggpm_gemm(1, 0, N, K, M,
 * ...), split-K over the M rows through `ws` where that pays) and, when `db` is not NULL, db_i[N] = column sums of dpre_i -- autograd's
 * mm / sum backward of a Linear (the score heads of ggpm/decoder.py:35-58, the read-outs of ggpm/encoder.py:15-19,62-72), which the
 * deferred-gradient queue of ggpm_amd/functional.py forms once per parameter and pass.  The items run one after the other on
 * `stream` and share `ws` (>= the largest ggpm_gemm_workspace_bytes(N, K, M); NULL / 0: no split-K) and `csws` (256 * max N
 * floats).  Same launches and results as the separate calls. */
typedef struct ggpm_wgrad_item {
    const float* dpre; int ld_dpre;
    const float* x; int ld_x;
    float* dW; int ld_dw;
    float* db;
    int M, N, K;
} ggpm_wgrad_item;
int ggpm_linear_wgrads_batch(int count, const ggpm_wgrad_item* items, float* ws, size_t ws_bytes, float* csws,
                             ggpm_stream_t stream);
/* out[n] = sum_m A[m*lda+n] (bias gradients), deterministic two-stage; ws >= 256*N floats. */
int ggpm_colsum(const float* A, int lda, int M, int N, float* out, float* ws, ggpm_stream_t stream);
/* The three products the level weight gradients are built from (csrc/mpn_gru.hip, csrc/mpn_lstm.hip), callable by themselves:
 *   ggpm_gemm_tn_tall_grouped -- `count` (<= 4) contractions C_i = A_i^T B_i of one output shape, K[i] rows each, in one launch
 *       of a 160 x 160 tall kernel plus one reduce; mode 0: fp32 operands at fp32 accuracy, 1: fp32 operands rounded to bf16,
 *       2: the operands ARE bf16 in memory (lda / ldb in elements).  A group that does not qualify for the tall kernel runs
 *       as ggpm_gemm(1, 0, ...) per member (modes 0, 1) or returns GGPM_ERR_UNSUPPORTED and launches nothing (mode 2).
 *   ggpm_gemm_tn_pair_grouped_c -- C_i[M x N] = hi_i^T B_i + lo_i^T B_i, every operand [rows, ld], in one launch of the
 *       small-tile kernel (one accumulator chain over both); two products per member when the group has too many tiles.
 *   ggpm_colsum_dtype -- ggpm_colsum of an fp32 (a_bf16 = 0) or bf16 (lda in elements) matrix. */
typedef struct ggpm_pair_problem { const float *hi, *lo, *B; float* C; int ldc; } ggpm_pair_problem;
int ggpm_gemm_tn_tall_grouped(int M, int N, int count, const ggpm_gemm_problem* problems, const int* K, float* ws,
                              size_t ws_bytes, int mode, ggpm_stream_t stream);
int ggpm_gemm_tn_pair_grouped_c(int M, int N, int rows, int ld, int count, const ggpm_pair_problem* problems,
                                ggpm_stream_t stream);
int ggpm_colsum_dtype(const float* A, int lda, int M, int N, float* out, float* ws, int a_bf16, ggpm_stream_t stream);

/* Which kernel a product runs on.  Host only: no HIP call, nothing launched.  The entry points above and this query decide
 * through the same functions (csrc/gemm.hip: plan_gemm, plan_group, plan_group_splitk, plan_group_masked, plan_segments,
 * plan_tall_group, plan_tn_bf16, plan_pairs, one per GGPM_GEMM_ENTRY_* in that order), and an entry point fills its kernel
 * arguments and launches from the plan alone (fill_group, run_plan), so what the query reports is what a call does;
 * DESIGN.md ("The GEMM forms") lists the thresholds.
 * `call` describes what the dispatchers look at; pointers appear as the low four bits of their address only.
 *   entry   -- GGPM_GEMM_ENTRY_*: the entry point; count: members (grouped entries) or segments (ksegments), 1 for gemm
 *   K[i]    -- per member (tall_grouped) or per segment (ksegments); the other entries read K[0] (pair_grouped: rows)
 *   lda, ldb, ldc, n_pad, base_a, base_b -- per member / segment (ksegments: ldc[0], n_pad[0]; pair_grouped: lda[0] = ld,
 *              base_a = hi, base_lo = lo, base_b = B)
 *   has_ws, ws_bytes -- whether a workspace pointer is passed, and its size
 *   mode    -- tall_grouped: 0 / 1 / 2 as above
 * The form: kernel (GGPM_GEMM_KERNEL_*; SEQUENCE: one ggpm_gemm call per member / segment (pair_grouped: two), each with
 * the form ggpm_gemm reports for it), vec_a / vec_b (bit i: 16-byte loads legal for member i's operand), reduce
 * (GGPM_GEMM_REDUCE_*), splits (grid.z chunks per member), k_chunk per member, the grid, static + dynamic LDS bytes of the
 * product kernel, the bytes of workspace the call writes, and `rc`: what the entry point itself would return
 * (GGPM_ERR_ARG / GGPM_ERR_UNSUPPORTED launch nothing: kernel = NONE).  Returns GGPM_ERR_ARG for a NULL argument or an
 * unknown entry, GGPM_OK otherwise. */
enum { GGPM_GEMM_ENTRY_GEMM = 0, GGPM_GEMM_ENTRY_GROUPED, GGPM_GEMM_ENTRY_GROUPED_SPLITK, GGPM_GEMM_ENTRY_GROUPED_MASKED,
       GGPM_GEMM_ENTRY_KSEGMENTS, GGPM_GEMM_ENTRY_TALL_GROUPED, GGPM_GEMM_ENTRY_PAIR_GROUPED, GGPM_GEMM_ENTRY_TN_BF16 };
enum { GGPM_GEMM_KERNEL_NONE = 0, GGPM_GEMM_KERNEL_SCALAR, GGPM_GEMM_KERNEL_SEGS, GGPM_GEMM_KERNEL_GROUP, GGPM_GEMM_KERNEL_V2,
       GGPM_GEMM_KERNEL_GROUP_V2, GGPM_GEMM_KERNEL_SMALL_V3, GGPM_GEMM_KERNEL_TALL, GGPM_GEMM_KERNEL_TALL_BF16,
       GGPM_GEMM_KERNEL_TALL_BF16_IN16, GGPM_GEMM_KERNEL_TALL_SPLIT, GGPM_GEMM_KERNEL_SEQUENCE };
enum { GGPM_GEMM_REDUCE_NONE = 0, GGPM_GEMM_REDUCE_SPLITK, GGPM_GEMM_REDUCE_SPLITK_GROUP, GGPM_GEMM_REDUCE_TALL };
typedef struct ggpm_gemm_call {
    int entry, trans_a, trans_b, M, N, count;
    int K[4], lda[4], ldb[4], ldc[4], n_pad[4];
    int base_a[4], base_b[4], base_lo[4];
    int has_ws, mode;
    size_t ws_bytes;
} ggpm_gemm_call;
typedef struct ggpm_gemm_form {
    int kernel, vec_a, vec_b, reduce, splits;
    int k_chunk[4];
    int grid[3];
    int rc;
    size_t lds_bytes, ws_used;
} ggpm_gemm_form;
int ggpm_gemm_form_query(const ggpm_gemm_call* call, ggpm_gemm_form* out);
/* dpre = dy * act'(y) given the activation OUTPUT y; optional row-0 zeroing. In-place allowed. */
int ggpm_act_backward(const float* dy, const float* y, int rows, int cols, int ld, int act,
                      int zero_row0, float* dpre, ggpm_stream_t stream);

/* ------------------------------------------------------------------ gathers / segmented sums
 * out[r, 0:width] = sum_{j in rowptr[r]..rowptr[r+1]} src[col[j], 0:width]
 * = index_select_ND(h, 0, agraph).sum(1) of ggpm/encoder.py:31-32,99,135-136 (and, through the
 * transposed CSR, every scatter-add autograd would run for their backward).  accumulate!=0 adds to out.
 * zero_to (all three below): columns [end of the written block, zero_to) of every row are set to 0 as well (the pad
 * columns of the Hp-strided matrices), 0 = leave them alone. */
int ggpm_segment_sum(const float* src, int ld_src, const int32_t* rowptr, const int32_t* col, int rows,
                     int width, float* out, int ld_out, int accumulate, int zero_to, ggpm_stream_t stream);
/* `count` (1 or 2) segmented sums over ONE CSR in one launch, each with two options:
 *   addend[i] -- row r starts from addend[i][r, :] (leading dimension ld_addend) instead of from zero: what accumulate != 0
 *                does with a copy of `addend` in `out`, same order of additions (NULL array / entry: start from zero);
 *   dpre[i]   -- a second output dpre[i] = ggpm_act_backward(sum, y[i], ..., act, zero_row0), y / dpre with leading
 *                dimension ld_mask (NULL: none).  out[i] may be NULL when dpre[i] is given: the plain sum is not stored.
 * zero_to as above (applies to out). */
int ggpm_segment_sum_masked(int count, const float* const* src, int ld_src, const int32_t* rowptr, const int32_t* col,
                            int rows, int width, const float* const* addend, int ld_addend, float* const* out, int ld_out,
                            int zero_to, const float* const* y, float* const* dpre, int ld_mask, int act, int zero_row0,
                            ggpm_stream_t stream);
/* out[r, col_off : col_off+width] = table[idx[r], 0:width]; rows with idx<0 give zeros.
 * = nn.Embedding / index_select of ggpm/encoder.py:98,103,111,114 */
int ggpm_gather_rows(const float* table, int ld_table, const int32_t* idx, int rows, int width,
                     float* out, int ld_out, int col_off, int zero_to, ggpm_stream_t stream);
/* dst[idx[r], 0:width] = src[r, 0:width] (accumulate != 0: +=); rows with idx < 0 are skipped.  The indices must be
 * UNIQUE (plain stores).  The write side of index_select for the compact row sets of the teacher-forced atom-level
 * decode (ggpm/encoder.py:165-179 run on the rows a step touches; ggpm_amd/atom_decode.py). */
int ggpm_scatter_rows(const float* src, int ld_src, const int32_t* idx, int rows, int width, float* dst, int ld_dst,
                      int accumulate, ggpm_stream_t stream);
/* out[r, col_off + idx[r]] = 1, the other `classes` columns of that block 0: the one-hot tables
 * E_a/E_b/E_apos/E_pos of ggpm/encoder.py:74-77,121-125,104-105. */
/* nn.Dropout in training mode (ggpm/encoder.py:15-19, 52-72), in place on x[rows, cols] (leading dimension ld):
 * x[r][c] = keep ? x[r][c] / (1 - p) : 0 with keep = (mix(seed, site, r * cols + c) >> 8) >= p * 2^24, mix = two rounds of
 * the murmur3 32-bit finaliser (see gather.hip; restated in numpy by tests/golden_utils.dropout_keep).  Stateless: the
 * backward applies the same call to the incoming gradient.  Cannot be bit-matched to torch's generator; parity tests
 * inject the same mask into the oracle. */
int ggpm_dropout(float* x, int rows, int cols, int ld, float p, unsigned int seed_lo, unsigned int seed_hi, int site,
                 ggpm_stream_t stream);
/* ------------------------------------------------------------------ property heads and latent search (property.hip)
 * HierPropOptVAE's HOMO / LUMO heads (ggpm/property_optimizer.py: PropertyOptimizer = two PropertyRegressor) and the
 * latent property search of ggpm/property_control.py:65-180.  One head is
 *     Linear(width[0], width[1]) -> ReLU -> Dropout -> ... -> Linear(width[n_linear - 1], 1)
 * with nn.Linear's row-major weights W[l] [width[l + 1], width[l]] and biases b[l] [width[l + 1]].  The homo head reads
 * columns [0, half) of the latent z [B, ld], the lumo head columns [half, 2 half).
 * Supported: 2 <= n_linear <= GGPM_PROP_MAX_LINEAR (1 to 4 hidden layers), 1 <= half <= 256, hidden widths <= 512,
 * B <= 1024 for the heads forward / backward; anything else returns GGPM_ERR_UNSUPPORTED.
 * Dropout (training forward, p > 0): the masks of ggpm_dropout() over the [B, width[l + 1]] output of hidden layer l at
 * site GGPM_SITE_PROP_HOMO + l (homo head) or GGPM_SITE_PROP_LUMO + l (lumo head); p == 0 generates none. */
#define GGPM_PROP_MAX_LINEAR 5
#define GGPM_SITE_PROP_HOMO 16     /* dropout sites 16..19: homo head hidden layers 0..3 */
#define GGPM_SITE_PROP_LUMO 20     /* dropout sites 20..23: lumo head hidden layers 0..3 */
typedef struct ggpm_prop_head {
    int n_linear;
    int width[GGPM_PROP_MAX_LINEAR + 1];  /* width[0] = half, width[n_linear] = 1 */
    const float* W[GGPM_PROP_MAX_LINEAR];
    const float* b[GGPM_PROP_MAX_LINEAR];
} ggpm_prop_head;
typedef struct ggpm_prop_head_grads {
    float* dW[GGPM_PROP_MAX_LINEAR];      /* same shapes as W / b; a null pointer skips that gradient */
    float* db[GGPM_PROP_MAX_LINEAR];
    int accumulate;                       /* 0: write, 1: add into what is there */
} ggpm_prop_head_grads;
/* Bytes of the workspace the forward fills and the backward reads (0: bad arguments). */
size_t ggpm_property_heads_workspace_bytes(int B, int half, const ggpm_prop_head* homo, const ggpm_prop_head* lumo);
/* Both heads in one launch: pred[2][B] (homo row, then lumo row) and, when `loss` is given, the two batch-mean MSEs
 * loss[0] = mean (pred[0] - t_homo)^2, loss[1] = mean (pred[1] - t_lumo)^2 (each summed in a fixed order).  p: dropout
 * probability of a training forward (0 in eval mode), seed_lo / seed_hi its mask stream.  `ws` is kept for the backward. */
int ggpm_property_heads_forward(int B, const float* z, int ld, int half, const ggpm_prop_head* homo,
                                const ggpm_prop_head* lumo, const float* t_homo, const float* t_lumo, float p,
                                unsigned int seed_lo, unsigned int seed_hi, float* pred, float* loss, void* ws,
                                size_t ws_bytes, ggpm_stream_t stream);
/* The backward of that forward (same z, heads, targets, p, pred and ws) from dloss[2] (device), in one launch:
 * dz[:, head columns] written (accumulate_dz = 0) or added into (1), every weight and bias gradient per
 * ggpm_prop_head_grads (a null struct skips that head's parameter gradients).  Batch reductions in a fixed order. */
int ggpm_property_heads_backward(int B, const float* z, int ld, int half, const ggpm_prop_head* homo,
                                 const ggpm_prop_head* lumo, const float* t_homo, const float* t_lumo, float p,
                                 const float* pred, const float* dloss, void* ws, size_t ws_bytes, float* dz, int ld_dz,
                                 int accumulate_dz, const ggpm_prop_head_grads* g_homo, const ggpm_prop_head_grads* g_lumo,
                                 ggpm_stream_t stream);
/* The latent search of ggpm/property_control.py:65-180, ONE launch for the whole batch and every step (one workgroup per
 * molecule; heads in eval form, no dropout).  Per molecule, fp32, v_h / v_l the two halves of its row of z:
 *   soft / patience:  pat = patience; prev = 0; n = 0
 *     while pat > 0 and n < max_steps:
 *       o_x = f_x(v_x); loss = (o_h - t_h)^2 + (o_l - t_l)^2; n += 1
 *       soft: if loss <= delta: stop (no update)
 *       if loss > prev or |loss - prev| / prev <= threshold: pat -= 1 else pat = patience     (IEEE: prev = 0 gives inf / NaN)
 *       prev = loss
 *       v_x -= s_x lr 2 (o_x - t_x) df_x/dv_x,  s_x = -1 if o_x < t_x else +1                   (both heads, every body)
 *   fixed:  min(steps, max_steps) bodies, the same update with the batch-mean factor 2 / B, no stopping rule.
 * Outputs: z_out [B, ld] (columns past 2 half copied), pred_out[2][B] = the heads on the final latent, steps_taken[B]
 * (loop bodies executed) and status[B]: GGPM_PROP_DONE, or GGPM_PROP_CAPPED when max_steps ended the loop (fixed: steps >
 * max_steps).  max_steps >= 1 is required: the reference's loop need not end (a loss of exactly 0 resets the patience
 * forever). */
enum { GGPM_PROP_SEARCH_FIXED = 0, GGPM_PROP_SEARCH_SOFT = 1, GGPM_PROP_SEARCH_PATIENCE = 2 };
enum { GGPM_PROP_DONE = 0, GGPM_PROP_CAPPED = 1 };
int ggpm_property_latent_search(int mode, int B, const float* z, int ld, int half, const ggpm_prop_head* homo,
                                const ggpm_prop_head* lumo, const float* t_homo, const float* t_lumo, float lr, int steps,
                                float delta, float patience, float threshold, int max_steps, float* z_out, float* pred_out,
                                int32_t* steps_taken, int32_t* status, ggpm_stream_t stream);
/* One Adam step (torch.optim.Adam's arithmetic; ggpm/../vae_train.py:60,83 `optimizer.step()`) over ONE flat fp32 buffer that
 * all parameters are views of; p, g, m, v 16-byte aligned, n elements; step counts from 1.
 *   m += (1-b1)(g' - m); v = b2 v + (1-b2) g'^2; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps),  g' = g + wd p */
int ggpm_adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
                   float weight_decay, int step, ggpm_stream_t stream);
/* Gradient-norm clipping (torch.nn.utils.clip_grad_norm_, vae_train.py:82) and per-group Adam (the four optimizers of
 * vae_fine_tune_indv_opt.py:61-70) over the same flat buffers.  The sum of squares is combined ACROSS KERNEL BOUNDARIES:
 * the partials launch writes one fp64 sum per workgroup into a caller-owned workspace; the launch behind it (the grouped Adam
 * step, or the one-workgroup finish) adds the partials in index order.  Nothing is allocated, copied to the host or
 * synchronised, and the result is the same bits on every call and in every workgroup.
 *   partials:  x 16-byte aligned, any n >= 1; `partials` holds the workspace query's bytes (a function of n alone, at
 *              most GGPM_NORM_MAX_PARTIALS doubles); n_partials of the calls below = those bytes / 8.
 *   finish:    out[0] = (float)sqrt(sum); with max_norm > 0 also out[1] = min(max_norm / (out[0] + 1e-6f), 1), a NaN kept
 *              (torch's clip coefficient).  max_norm <= 0 leaves out[1] alone. */
#define GGPM_NORM_MAX_PARTIALS 256
size_t ggpm_flat_sqnorm_workspace_bytes(size_t n);
int ggpm_flat_sqnorm_partials(const float* x, size_t n, double* partials, size_t partials_bytes, ggpm_stream_t stream);
int ggpm_flat_norm_finish(const double* partials, int n_partials, float max_norm, float* out, ggpm_stream_t stream);
/* ggpm_adam_step's arithmetic with up to GGPM_ADAM_MAX_GROUPS hyper-parameter sets and an optional clip.  n % 64 == 0:
 * tile_group[n / 64] (device, values < n_groups) names the group of every 64-float tile (FlatGradSync.ALIGN puts every
 * parameter on such a boundary; padding may carry any group: zeros stay zeros); NULL with one group.  One step count
 * serves all groups.  partials != NULL (n_partials, max_norm > 0): the gradient is used as g * coef, coef as in the
 * finish above, formed by every workgroup for itself; clip_out (device float[2], may be NULL) receives {norm, coef};
 * write_clipped != 0 also stores g * coef back to g.  A non-finite gradient propagates as under clip_grad_norm_ with
 * error_if_nonfinite=False. */
#define GGPM_ADAM_MAX_GROUPS 8
typedef struct ggpm_adam_group { float lr, beta1, beta2, eps, weight_decay; } ggpm_adam_group;
int ggpm_adam_step_groups(float* p, float* g, float* m, float* v, size_t n, const uint8_t* tile_group, int n_groups,
                          const ggpm_adam_group* groups, int step, const double* partials, int n_partials, float max_norm,
                          float* clip_out, int write_clipped, ggpm_stream_t stream);
/* ggpm_adam_step_groups with a non-finite guard, a step count that leaves skipped steps out, and an exponential moving
 * average of the parameters, in the same single launch.  Everything up to `write_clipped` is as above, except:
 *   partials   required with max_norm > 0 or skip_nonfinite; with partials and max_norm == 0 the guard runs without a clip
 *              (coefficient exactly 1, no multiply issued).  max_norm < 0 or NaN is refused.
 *   guard      skip_nonfinite != 0 and the fp32 norm (status[0], the value clip_out[0] above would hold) not finite: the
 *              step is SKIPPED: no byte of p, m, v, ema or g changes, with write_clipped too.  This covers an Inf or a NaN
 *              anywhere in g, and also an all-finite g whose 2-norm overflows fp32 (above 3.4e38).
 *   counter    skipped_in / skipped_out: two DIFFERENT device ints (both or neither); *skipped_out = *skipped_in + 1 on a
 *              skipped step, = *skipped_in on an applied one.  The caller alternates the two call by call, so no workgroup
 *              reads what another writes in the same launch.  `step` stays the caller's call count; the bias corrections
 *              use t_eff = step - *skipped_in, as torch.optim.Adam does when optimizer.step() is simply not called.
 *              While *skipped_in is 0 (or NULL) the corrections are the host-formed values of ggpm_adam_step_groups and
 *              p, m, v are its bits; afterwards the device forms lr / (1 - b1^t_eff) and 1 / sqrt(1 - b2^t_eff) in fp64 with
 *              the power by repeated squaring, which may differ from a host-formed value in the last fp32 bit.
 *   ema        NULL, or n floats, 16-byte aligned, no alias of p, g, m, v; on an applied step, behind the update,
 *              ema += (1 - d)(p_new - ema) in fp32, d = ema_decay in [0, 1), or with ema_warmup != 0
 *              d = min(ema_decay, (1 + t_eff) / (10 + t_eff)) (one correctly rounded fp32 division; t_eff < 2^24).
 *   status     NULL or device float[4] = {norm, coef, skipped (0 / 1), t_eff}; the first two only with partials. */
int ggpm_adam_step_ex(float* p, float* g, float* m, float* v, size_t n, const uint8_t* tile_group, int n_groups,
                      const ggpm_adam_group* groups, int step, const double* partials, int n_partials, float max_norm,
                      int write_clipped, float* ema, float ema_decay, int ema_warmup, int skip_nonfinite,
                      const int* skipped_in, int* skipped_out, float* status, ggpm_stream_t stream);
/* a[i] <-> b[i] for i < n in place (16 B per lane, nothing allocated); a, b 16-byte aligned and not overlapping. */
int ggpm_flat_swap(float* a, float* b, size_t n, ggpm_stream_t stream);
int ggpm_onehot(const int32_t* idx, int rows, int classes, float* out, int ld_out, int col_off, int zero_to,
                ggpm_stream_t stream);
/* embed_graph (ggpm/encoder.py:119-126) in one launch: hnode[N1, ld_n] = onehot(fnode), hmess[E1, ld_m] =
 * [onehot(fnode[src]) | onehot(bond) | onehot(pos)] from the int64 A0 tensors. */
int ggpm_embed_graph(const int64_t* fnode, int N1, const int64_t* fmess, int E1, int atom_size,
                     int bond_types, int max_pos, float* hnode, int ld_n, float* hmess, int ld_m,
                     ggpm_stream_t stream);

/* Where a dense backward (e.g. one called with ggpm_level_opts.skip_x_sums) left its per-depth gate gradients inside `work`
 * (slot t-1 of each = backward step t).  ggpm_sum_slots sums slots in fixed order: out[i] = sum_t src[t * slot_floats + i]. */
int ggpm_gru_backward_stashes(float* work, int E1, int H, int depth, float** DMP, float** DZP);
/* ... and for ggpm_lstm_backward: dXi, dXo, dXu = sums of the DI / DO / DU stash slots (dXf still accumulates per depth) */
int ggpm_lstm_backward_stashes(float* work, int E1, int H, int depth, float** DI, float** DO, float** DU);
int ggpm_sum_slots(const float* src, int slots, size_t slot_floats, float* out, ggpm_stream_t stream);
/* 1 when a DENSE TRAINING level (GRU or LSTM) of E1 message rows (pad row included) and hidden size H keeps the arrays of
 * its depth loop in bf16 under gate dtype 1 (BASELINE configs[4]: "bf16 storage"): the state h and the per-message product
 * q, the stashes S / G / Z / M (LSTM: S / I / O / U), the backward's dS / dG and its DQ / DZP / DMP (DQ / DI / DO / DU)
 * stashes -- rounded (RNE) where they are written, in
 * the first half of the fp32 buffers the caller passes (no size or layout changes at this boundary; the level's result, slot
 * `depth` of Hs, stays fp32 at its usual place).  The rule: E1 >= 6144 and the H x H x E1 contraction qualifies for the
 * bf16 tall kernel, which then reads the stashes as they are.  Kept fp32: gate inputs X and their gradients, R / F, the
 * LSTM cell state c and dFC, every weight and weight gradient.  oracle/ref_encoder.py restates the roundings as gate_dtype "bf16s" (ggpm/rnn.py:25-50). */
int ggpm_level_bf16_storage(int E1, int H);
/* ------------------------------------------------------------------ level-call options
 * Options of ONE call of the GRU / LSTM level entry points below (forward, backward, weight_grads, sparse_forward,
 * sparse_backward): each takes `const ggpm_level_opts* opts` before its stream and reads it during that call only.
 * NULL (or a zero-initialised struct) = all defaults.  Fields a call does not use are ignored. */
typedef struct ggpm_level_opts {
    /* Gate-product dtype: 0 = fp32 operands (default, the 1e-4 parity mode: on dense levels large enough for one column
     * group the H x H products run at fp32 accuracy on the bf16 matrix pipe, every operand split exactly into three bf16
     * values and six of the nine partial products kept; on v_mfma_f32_16x16x4_f32 otherwise), 1 = bf16 operands with fp32
     * accumulate for the hidden x hidden products of the depth loops and the tall weight-gradient contractions (BASELINE
     * configs[4]; the reference's cells are ggpm/rnn.py:27-36, 88-91), 2 = fp32 on v_mfma_f32_16x16x4_f32 only, 3 = fp32
     * on split operands wherever their images fit the LDS (0 chooses between 2 and 3 per level: split operands for dense
     * levels of one column group).  A level's forward, backward and weight_grads must agree on it. */
    int gate_dtype;
    /* Nonzero: a dense fp32 call uses two row tiles per workgroup whatever the level's size, i.e. half as many workgroups
     * (the same products in the same order per row; results agree with the default form to rounding, 5e-6 norm-wise after
     * 20 depth steps -- the two instantiations contract the gate expressions differently).  For a level that runs BESIDE a
     * latency-bound chain on another stream -- the encoder next to the decoder's atom level in the full VAE step
     * (ggpm/property_vae.py:47-58 runs them one after the other) -- this leaves the chain's launches free CUs. */
    int prefer_narrow;
    /* Nonzero: the call skips packing its gate weights: `wpack` (forward) resp. the head of `work` (backward) still holds
     * the fragments an earlier call with the SAME weights and the same buffer left there -- the decode steps share one set
     * of weights. */
    int weights_packed;
    /* Sparse backward, non-NULL defer_stash[0]: the call writes its gate-gradient stashes to caller memory and leaves
     * dW*_h / dUr / dbu untouched (see ggpm_*_weight_grads_stacked).  GRU: [0] = DMP, [1] = DZP ([depth][E1][Hp] each,
     * pairing with the forward's Gs / Ss), [2] = DQ ([depth][E1][Hp], slot t pairs with Hs slot t; give the block depth+1
     * slots, the last one zero, so that it lines up with Hs), [3] unused.  LSTM: [0..2] = DI, DO, DU (pair with Ss),
     * [3] = DQ (pairs with Hs, as above). */
    float* defer_stash[4];
    /* Start state / incoming-state gradient of a sparse call through an index (the decode steps keep every step's rows in
     * stacked blocks; a step's frozen rows are the final states of rows of earlier blocks, ggpm/encoder.py:165-179 reads
     * them out of the level-wide `hmess` instead).  Rows are [Hp] floats.
     * gather_*: with gather_h and gather_idx non-NULL (LSTM: gather_c too) a sparse forward takes the start state of row r
     * from gather_h[gather_idx[r]] (gather_c likewise; zero where the index is < 0) and writes it to slot 0 of Hs (Cs)
     * itself, inside its first launch; `h_in` / `c_in` are not read. */
    const float* gather_h;
    const float* gather_c;
    const int32_t* gather_idx;
    /* scatter_*: with scatter_h and scatter_idx non-NULL (LSTM: scatter_c too) a sparse backward ADDS the gradient of the
     * incoming state of row r to scatter_h[scatter_idx[r]] (scatter_c likewise; indices unique, rows with index < 0
     * dropped) inside its last launch; dHin / dCin are not written. */
    float* scatter_h;
    float* scatter_c;
    const int32_t* scatter_idx;
    /* Dense backward, nonzero: do not accumulate the gate-input gradients dXz / dXh (LSTM: dXi, dXo, dXu) per depth (those
     * outputs are then undefined).  The per-depth gate gradients are stashed anyway (for the weight-gradient
     * contractions), so a caller that does not need the sums on the critical path -- the atom level has no input gradient:
     * its inputs are one-hot constants, ggpm/encoder.py:119-126 -- forms them afterwards with ggpm_sum_slots over the slots
     * ggpm_gru_backward_stashes / ggpm_lstm_backward_stashes name, e.g. on a second stream: 13 MB less HBM traffic and four
     * memory operations fewer per element in every depth launch. */
    int skip_x_sums;
    /* Driver-internal shortcuts (the whole-encoder and tree-level drivers set them; exact only under the conditions
     * stated, which the caller vouches for):
     * run_depth -- dense training forward: issue only steps 1 .. run_depth of `depth` (0 / >= depth: all of them).  Message
     *   passing on a tree reaches a fixed point after as many steps as the longest dependency chain; the caller then
     *   replicates the last computed slot of every stash array, or passes fixed_slot (below) and replicates nothing.
     * lo -- dense backward / weight_grads: stop at step `lo` (<= 1: all steps).  The same acyclic structure makes the
     *   Jacobian of a tree level's recurrence nilpotent: with a longest dependency chain of C messages, d(h^{D-k}) is
     *   exactly zero for k >= C, so the backward of such a level only has to run its steps t = D .. lo with
     *   lo = max(1, D - C + 1); every skipped launch would compute exact zeros and every skipped stash slot would add exact
     *   zeros to the weight-gradient contractions.  A backward and its separate weight_grads call pass the same value.
     * skip_bias_u -- GRU weight_grads: leave db_u alone; the caller forms it with its own column sum of the same dq stash
     *   rows on another stream.
     * skip_sparse_wgrads -- sparse backward: leave the hidden-half weight gradients to a later sparse weight-gradient call
     *   with the same arguments (the same launches, on whatever stream that call names). */
    int run_depth;
    int lo;
    int skip_bias_u;
    int skip_sparse_wgrads;
    /* Forward without stashes (save_for_backward = 0), h_out non-NULL: the forward-only form of a level, dense or sparse.
     * The call honours run_depth as the dense training forward does, keeps the depth loop in the two ping-pong slots of Hs / Qs (LSTM:
     * and Cs), writes the last computed step's h [E1][Hp] to h_out (LSTM: c to c_out when that is non-NULL) and applies
     * bf16 storage (ggpm_level_bf16_storage) exactly as the training forward of the same level does, so h_out is
     * bit-identical to slot `depth` of the training forward's Hs.  NULL (default): the result is Hs[depth & 1] as
     * documented at ggpm_gru_forward, all `depth` steps run and the depth loop stays fp32. */
    float* h_out;
    float* c_out;
    /* Driver-internal, dense fp32 training calls of a tree-side level that reached its fixed point (run_depth = C + 1 of
     * `depth` = D steps, D >= 2C, so lo - 1 >= run_depth - 1): fixed_slot = run_depth (0: off) means "state slots above
     * fixed_slot and stash slots above fixed_slot - 1 alias those" -- nothing replicates them.
     *   forward: only step fixed_slot writes its stash slot (the only one the backward reads); the state slots as ever.
     *   backward: reads state slot min(t, fixed_slot) and stash slot min(t - 1, fixed_slot - 1) at step t; the gate
     *     gradient stashes it writes itself keep their real slots.
     *   weight_grads: every stash row block a step >= lo pairs with is the one settled slot X*, so the hidden-half gradients
     *     are (sum_t D_t)^T X* -- the slot sums are kept as unevaluated fp32 pairs hi + lo (slots 0 and 1 of each gate
     *     gradient stash, free below lo - 1 >= 2) and contracted as [hi; lo]^T [X*; X*], K = 2 E1 instead of C E1.
     * A level's forward, backward and weight_grads pass the same value. */
    int fixed_slot;
    /* Dense GRU forward on a column-grouped level (ggpm_level_ksplit_q says which calls): q_part non-NULL, of at least
     * ggpm_level_q_part_bytes(E1, H) bytes, lets every forward step but the last executed one drop its B launch.  A column
     * group multiplies the h' columns it holds by the matching K slice of U_r inside kernel A and stores a partial q' over
     * all output columns (group 0 adds b_u); the next step's gather adds the `groups` partial rows of a predecessor in
     * ascending group order and writes the sums of its own rows to Qs, so Qs holds what it always held.  The buffer is two
     * blocks of [groups][E1][Hp] floats used alternately by depth parity; its contents before and after the call mean
     * nothing.  q' is then a sum of `groups` short chains instead of one long one: results agree with the B-launch form to
     * fp32 summation order and are run-to-run identical.  NULL (default), or a call the form does not apply to: the B
     * launches as ever.  A buffer that is too small: GGPM_ERR_WORKSPACE. */
    float* q_part;
    size_t q_part_bytes;
} ggpm_level_opts;
/* Bytes of ggpm_level_opts.q_part for a level of E1 rows and hidden size H: 2 * groups * E1 * Hp * sizeof(float), with
 * `groups` as ggpm_level_form_query reports it under default options.  Host only. */
size_t ggpm_level_q_part_bytes(int E1, int H);
/* 1 when a forward call of this level (arguments as ggpm_level_form_query) takes the K-split form of q' once it is given
 * ggpm_level_opts.q_part: a dense GRU call on fp32 MFMA (gate mode 0) with one row tile per workgroup, 2 to 5 column groups
 * and at most two output tiles of a group per wave.  0 otherwise (LSTM, sparse, other geometries), and on bad arguments.
 * The answer does not depend on q_part itself, nor does ggpm_level_form_query's.  Host only. */
int ggpm_level_ksplit_q(int lstm, int E1, int H, int sparse, const ggpm_level_opts* opts);

/* The form a level call takes: which of the depth kernels' launch geometries, gate modes and LDS layouts a GRU (lstm = 0) or
 * LSTM level of E1 message rows (pad row included) and hidden size H runs on -- dense (sparse = 0: ggpm_*_forward / _backward)
 * or sparse (ggpm_*_sparse_forward / _sparse_backward), with stashes (training != 0: save_for_backward, and the backward) or
 * without, under `opts` (NULL: defaults; gate_dtype, prefer_narrow and h_out are read).  Host only: no HIP call, nothing
 * launched.  The level entry points and this query decide through the same functions (csrc/mpn_gru.hip, csrc/mpn_lstm.hip:
 * level_plan, fwd_step, bwd_step), so what it reports is what a call does; DESIGN.md ("The lattice of level forms") lists
 * the forms the configured hidden sizes reach.
 *   tiles = Hp / 16 output tiles are cut into `groups` = ceil(tiles / tg) column groups (grid.y) of tg tiles, the last one
 *   ragged when tg does not divide tiles; each of the 16 waves of a workgroup owns ceil(tg / 16) tiles of its group at most.
 *   rt2: two row tiles (32 message rows) per workgroup.  gate_mode: 0 fp32 MFMA, 1 bf16 operands, 2 fp32 on split operands.
 *   st16: bf16 storage (ggpm_level_bf16_storage).  fuse_fwd / fuse_bwd: a depth step that needs q' (LSTM: qf') resp.
 *   dS, dG (dS) forms it inside kernel A instead of by a B launch.  lds_*: dynamic LDS bytes of such a step's A and B
 *   launches, 0 = not launched (a sparse forward always has its q^0 B launch; the level's last forward step and the first
 *   backward step of a dense level need no B product and take the unfused A size, which is never the larger one;
 *   training = 0 leaves the backward fields 0).
 * Returns GGPM_OK, GGPM_ERR_UNSUPPORTED for a shape the level entry points refuse (see the accepted hidden sizes below), or
 * GGPM_ERR_ARG (E1 <= 0, H <= 0, out == NULL). */
typedef struct ggpm_level_form {
    int Hp, tiles;            /* padded hidden size, NT = Hp / 16 */
    int tg, groups;           /* tiles per column group, grid.y */
    int rt2, gate_mode, st16; /* as the launchers decide them */
    int fuse_fwd, fuse_bwd;   /* q' resp. dS/dG inside kernel A */
    size_t lds_fwd_a, lds_fwd_b, lds_bwd_a, lds_bwd_b;   /* dynamic LDS bytes per launch, 0 = not launched */
} ggpm_level_form;
int ggpm_level_form_query(int lstm, int E1, int H, int sparse, int training, const ggpm_level_opts* opts,
                          ggpm_level_form* out);

/* ------------------------------------------------------------------ GRU message function
 * GRU.forward (ggpm/rnn.py:41-50) with GRU.GRU (ggpm/rnn.py:25-39) restated over CSR predecessors with
 * the depth-invariant input halves hoisted:  Xz = x W_z[:, :I]^T + b_z, Xr = x W_r^T, Xh = x W_h[:, :I]^T + b_h
 * are computed once by ggpm_gemm; per depth
 *     s_e = sum_p h_p,  g_e = sum_p sigmoid(Xr_e + q_p) * h_p,   q_p = U_r h_p + b_u,
 *     z = sigmoid(Xz + Wz_h s), m = tanh(Xh + Wh_h g), h' = (1-z) s + z m, row 0 := 0.
 * Two launches per depth over a (row tiles) x (column groups) grid: A = CSR gather -> LDS tiles -> MFMA gate
 * GEMMs -> gate math -> h'; B = MFMA q' GEMM from the h' rows.
 * Stash layout ([t] = depth slot): Hs[depth+1][E1][Hp] (Hs[0]=0, Hs[depth] = result), Qs/Ss/Gs/Zs/Ms/Rs
 * [depth][E1][Hp] (Rs = sum_p h_p r(1-r), which lets the backward form dXr without a gather).  With
 * save_for_backward = 0 only Hs[2][E1][Hp] and Qs[2][E1][Hp] are needed and the result is Hs[depth & 1].
 * wpack: ggpm_gru_pack_floats(H) floats of scratch.
 * Accepted hidden sizes: Hp = ggpm_padded_hidden(H) <= 1264, i.e. H <= 1264 (two fp32 LDS tiles of 16 rows x (Hp + 4) columns
 * must fit the 160 KiB of a workgroup); every GRU level entry point (forward, backward, sparse_*) returns
 * GGPM_ERR_UNSUPPORTED beyond that and launches nothing.  Inside the range the form changes with H (ggpm_level_form_query); a
 * dense fp32 level of one column group runs on split gate operands with q' and dS / dG fused up to Hp = 448, on split
 * operands with B launches up to Hp = 624 (also the last size with two row tiles per workgroup), on fp32 MFMA with q'
 * fused up to Hp = 848, and on fp32 MFMA with B launches in both directions above that, a wave owning up to five tiles.
 */
size_t ggpm_gru_pack_floats(int H);
int ggpm_gru_forward(int E1, int H, int depth, const float* Xz, const float* Xr, const float* Xh,
                     const float* Wz_h, int ld_wz, const float* Ur, int ld_ur, const float* bu,
                     const float* Wh_h, int ld_wh, const int32_t* pred_rowptr, const int32_t* pred_col,
                     float* Hs, float* Qs, float* Ss, float* Gs, float* Zs, float* Ms, float* Rs,
                     float* wpack, int save_for_backward, const ggpm_level_opts* opts, ggpm_stream_t stream);
/* Backward of the above (replaces autograd's replay of ggpm/rnn.py:41-50): given dHD = dL/dh_D it
 * overwrites dXz/dXr/dXh [E1][Hp] and the weight gradients (written as [H,H] blocks with the given
 * leading dimension so they can land inside the full W_z/W_h gradient tensors), dbu[H].
 * succ_* is the CSR transpose of pred_* (ggpm_csr_transpose).  work: ggpm_gru_backward_workspace_bytes(). */
size_t ggpm_gru_backward_workspace_bytes(int E1, int H, int depth);
int ggpm_gru_backward(int E1, int H, int depth, const float* Xr, const float* Wz_h, int ld_wz,
                      const float* Ur, int ld_ur, const float* Wh_h, int ld_wh,
                      const int32_t* pred_rowptr, const int32_t* pred_col, const int32_t* succ_rowptr,
                      const int32_t* succ_col, const float* Hs, const float* Qs, const float* Ss,
                      const float* Gs, const float* Zs, const float* Ms, const float* Rs, const float* dHD, float* dXz,
                      float* dXr, float* dXh, float* dWz_h, int ld_dwz, float* dUr, int ld_dur,
                      float* dbu, float* dWh_h, int ld_dwh, float* work, size_t work_bytes,
                      int weight_grads, const ggpm_level_opts* opts, ggpm_stream_t stream);
/* The weight-gradient tail of ggpm_gru_backward (called with weight_grads = 0) as its own entry point, so the
 * host may enqueue it on a second stream beside the next level's depth loop. Same `work` buffer. */
int ggpm_gru_weight_grads(int E1, int H, int depth, const float* Hs, const float* Ss, const float* Gs, float* work,
                          size_t work_bytes, float* dWz_h, int ld_dwz, float* dUr, int ld_dur, float* dbu,
                          float* dWh_h, int ld_dwh, const ggpm_level_opts* opts, ggpm_stream_t stream);

/* GRU.sparse_forward (ggpm/rnn.py:52-59) -- the incremental form the decoder uses (IncMPNEncoder, ggpm/encoder.py:160-179):
 * rows with frozen[row] != 0 keep their state for the whole loop, the other rows (the `submess` subset) start from 0 and
 * are recomputed `depth` times from the current states of their predecessors.  Same kernels as the dense level:
 * frozen rows have empty predecessor lists, copy their state in the epilogue and pass their gradient through a carry
 * buffer; Hs[0] = masked h_in, Qs[0] = U_r Hs[0] + b_u.  The backward also returns dHin [E1][Hp] (zero on recomputed rows). */
int ggpm_gru_sparse_forward(int E1, int H, int depth, const float* h_in, const unsigned char* frozen, const float* Xz,
                            const float* Xr, const float* Xh, const float* Wz_h, int ld_wz, const float* Ur, int ld_ur,
                            const float* bu, const float* Wh_h, int ld_wh, const int32_t* pred_rowptr,
                            const int32_t* pred_col, float* Hs, float* Qs, float* Ss, float* Gs, float* Zs, float* Ms,
                            float* Rs, float* wpack, int save_for_backward, const ggpm_level_opts* opts, ggpm_stream_t stream);
int ggpm_gru_sparse_backward(int E1, int H, int depth, const unsigned char* frozen, const float* Xr, const float* Wz_h,
                             int ld_wz, const float* Ur, int ld_ur, const float* Wh_h, int ld_wh,
                             const int32_t* pred_rowptr, const int32_t* pred_col, const int32_t* succ_rowptr,
                             const int32_t* succ_col, const float* Hs, const float* Qs, const float* Ss, const float* Gs,
                             const float* Zs, const float* Ms, const float* Rs, const float* dHD, float* dHin,
                             float* dXz, float* dXr, float* dXh, float* dWz_h, int ld_dwz, float* dUr, int ld_dur,
                             float* dbu, float* dWh_h, int ld_dwh, float* work, size_t work_bytes,
                             const ggpm_level_opts* opts, ggpm_stream_t stream);

/* ------------------------------------------------------------------ LSTM message function
 * LSTM.forward (ggpm/rnn.py:96-108) with LSTM.LSTM (ggpm/rnn.py:85-94), same restatement:
 *     Xi/Xo/Xu/Xf = x W_*[:, :I]^T + b_*  (hoisted),   qf_p = Wf_h h_p,
 *     s = sum_p h_p,  fc = sum_p sigmoid(Xf_e + qf_p) * c_p,
 *     i = sigmoid(Xi + Wi_h s), o = sigmoid(Xo + Wo_h s), u = tanh(Xu + Wu_h s),
 *     c' = i u + fc,  h' = o tanh(c'),  rows 0 := 0.
 * Stash: Hs, Cs [depth+1][E1][Hp]; Qs (qf), Ss, Is, Os, Us, Fs [depth][E1][Hp] (Fs = sum_p c_p f(1-f)).
 * Accepted hidden sizes: Hp = ggpm_padded_hidden(H) <= 848, i.e. H <= 848 (three fp32 LDS tiles of 16 rows x (Hp + 4) columns
 * must fit the 160 KiB of a workgroup), and E1 * Hp < 2^30 (32-bit byte offsets inside a slot); every LSTM level entry point
 * returns GGPM_ERR_UNSUPPORTED beyond either and launches nothing.  ggpm_level_form_query reports the form inside the range
 * (a dense fp32 level of one column group: split operands up to Hp = 560, dS fused up to Hp = 304, qf' fused throughout).
 */
size_t ggpm_lstm_pack_floats(int H);
int ggpm_lstm_forward(int E1, int H, int depth, const float* Xi, const float* Xo, const float* Xu,
                      const float* Xf, const float* Wi_h, int ld_wi, const float* Wo_h, int ld_wo,
                      const float* Wu_h, int ld_wu, const float* Wf_h, int ld_wf,
                      const int32_t* pred_rowptr, const int32_t* pred_col, float* Hs, float* Cs,
                      float* Qs, float* Ss, float* Is, float* Os, float* Us, float* Fs, float* wpack,
                      int save_for_backward, const ggpm_level_opts* opts, ggpm_stream_t stream);
size_t ggpm_lstm_backward_workspace_bytes(int E1, int H, int depth);
int ggpm_lstm_backward(int E1, int H, int depth, const float* Xf, const float* Wi_h, int ld_wi,
                       const float* Wo_h, int ld_wo, const float* Wu_h, int ld_wu, const float* Wf_h,
                       int ld_wf, const int32_t* pred_rowptr, const int32_t* pred_col,
                       const int32_t* succ_rowptr, const int32_t* succ_col, const float* Hs,
                       const float* Cs, const float* Qs, const float* Ss, const float* Is,
                       const float* Os, const float* Us, const float* Fs, const float* dHD, float* dXi,
                       float* dXo, float* dXu, float* dXf, float* dWi_h, int ld_dwi, float* dWo_h, int ld_dwo,
                       float* dWu_h, int ld_dwu, float* dWf_h, int ld_dwf, float* work,
                       size_t work_bytes, int weight_grads, const ggpm_level_opts* opts, ggpm_stream_t stream);
int ggpm_lstm_weight_grads(int E1, int H, int depth, const float* Hs, const float* Ss, float* work, size_t work_bytes,
                           float* dWi_h, int ld_dwi, float* dWo_h, int ld_dwo, float* dWu_h, int ld_dwu,
                           float* dWf_h, int ld_dwf, const ggpm_level_opts* opts, ggpm_stream_t stream);

/* LSTM.sparse_forward (ggpm/rnn.py:110-121): as ggpm_gru_sparse_forward, with the cell state carried too.  The backward
 * takes dL/dh_D and dL/dc_D (the decoder keeps both) and returns dHin / dCin. */
int ggpm_lstm_sparse_forward(int E1, int H, int depth, const float* h_in, const float* c_in, const unsigned char* frozen,
                             const float* Xi, const float* Xo, const float* Xu, const float* Xf, const float* Wi_h,
                             int ld_wi, const float* Wo_h, int ld_wo, const float* Wu_h, int ld_wu, const float* Wf_h,
                             int ld_wf, const int32_t* pred_rowptr, const int32_t* pred_col, float* Hs, float* Cs,
                             float* Qs, float* Ss, float* Is, float* Os, float* Us, float* Fs, float* wpack,
                             int save_for_backward, const ggpm_level_opts* opts, ggpm_stream_t stream);
int ggpm_lstm_sparse_backward(int E1, int H, int depth, const unsigned char* frozen, const float* Xf, const float* Wi_h,
                              int ld_wi, const float* Wo_h, int ld_wo, const float* Wu_h, int ld_wu, const float* Wf_h,
                              int ld_wf, const int32_t* pred_rowptr, const int32_t* pred_col,
                              const int32_t* succ_rowptr, const int32_t* succ_col, const float* Hs, const float* Cs,
                              const float* Qs, const float* Ss, const float* Is, const float* Os, const float* Us,
                              const float* Fs, const float* dHD, const float* dCD, float* dHin, float* dCin, float* dXi,
                              float* dXo, float* dXu, float* dXf, float* dWi_h, int ld_dwi, float* dWo_h, int ld_dwo,
                              float* dWu_h, int ld_dwu, float* dWf_h, int ld_dwf, float* work, size_t work_bytes,
                              const ggpm_level_opts* opts, ggpm_stream_t stream);

/* Deferred hidden-half weight gradients for a SEQUENCE of sparse backward calls (the decode steps of one batch,
 * ggpm/decoder.py:201-222 -> ggpm/encoder.py:165-179 once per step; ggpm_amd/atom_decode.py): every step contracts a few
 * hundred rows against the same four H x H matrices, so instead of three or four small contractions per step the
 * gate-gradient stashes of all steps are kept, stacked row-wise (ggpm_level_opts.defer_stash), and contracted ONCE.
 *   ggpm_*_weight_grads_stacked: rows = total stash rows (sum over the calls of depth*E1), rows_q = total rows of the
 *   DQ / Hs stacks (sum of (depth+1)*E1); every buffer holds the calls' blocks in the same order.  Outputs are
 *   overwritten.  work: ggpm_weight_grads_stacked_workspace_bytes(H, max(rows, rows_q)). */
size_t ggpm_weight_grads_stacked_workspace_bytes(int H, int rows);
int ggpm_gru_weight_grads_stacked(int rows, int rows_q, int H, const float* DMP, const float* Gs, const float* DZP,
                                  const float* Ss, const float* DQ, const float* Hs, float* dWz_h, int ld_dwz, float* dUr,
                                  int ld_dur, float* dbu, float* dWh_h, int ld_dwh, float* work, size_t work_bytes,
                                  ggpm_stream_t stream);
int ggpm_lstm_weight_grads_stacked(int rows, int rows_q, int H, const float* DI, const float* DO, const float* DU,
                                   const float* Ss, const float* DQ, const float* Hs, float* dWi_h, int ld_dwi,
                                   float* dWo_h, int ld_dwo, float* dWu_h, int ld_dwu, float* dWf_h, int ld_dwf, float* work,
                                   size_t work_bytes, ggpm_stream_t stream);

/* The atom level's decode loop as ONE call per direction (ggpm/decoder.py:201-222 -> ggpm/encoder.py:235-239,165-179 once per
 * step, on the compact row sets of ggpm_amd/atom_decode.py): per step `gather the frozen rows from the stacked state buffer ->
 * ggpm_*_sparse_forward`, backwards `ggpm_*_sparse_backward (stashes deferred, see above) -> scatter-add of dHin to the rows'
 * producers`.  All arrays of the descriptor are HOST arrays of length T (T + 1 for the offsets); the pointers in them are
 * device pointers.  foff: first F id (one per (step, local row)) of a step; roff / qoff: first row of the step's [depth][n]
 * resp. [depth + 1][n] block in the stacked stash / state buffers.  X_all: the steps' gate inputs [G][n][Hp] per step at row
 * G * foff[t]; St_all: five stash kinds, `st_stride` floats apart; DG_all likewise (two kinds GRU, three LSTM).
 * W / ldw: hidden halves, GRU {Wz_h, U_r, Wh_h} (+ bu), LSTM {Wi_h, Wo_h, Wu_h, Wf_h}.  tmp: 2 * max(n) * Hp floats.
 * dW_unused: four H x H (ld H) scratch outputs the deferred backward leaves untouched (GRU: [3] = H floats). */
typedef struct ggpm_decode_steps {
    int T, H, depth, lstm;
    const int32_t* n;
    const int64_t *foff, *roff, *qoff;
    const int32_t* const* srcH;          /* rows of Hs_all / Cs_all a step's frozen rows are read from (-1: zero) */
    const int32_t* const* srcF;          /* the same as F ids (where the backward adds dHin / dCin) */
    const unsigned char* const* frozen;
    const int32_t* const* pred_rowptr;
    const int32_t* const* pred_col;
    const int32_t* const* succ_rowptr;
    const int32_t* const* succ_col;
} ggpm_decode_steps;
int ggpm_decode_steps_forward(const ggpm_decode_steps* steps, const float* const* W, const int* ldw, const float* bu,
                              const float* X_all, float* Hs_all, float* Cs_all, float* Qs_all, float* St_all, size_t st_stride,
                              float* wpack, float* tmp, ggpm_stream_t stream);
int ggpm_decode_steps_backward(const ggpm_decode_steps* steps, const float* const* W, const int* ldw, const float* X_all,
                               const float* Hs_all, const float* Cs_all, const float* Qs_all, const float* St_all,
                               size_t st_stride, float* dF, float* dCF, float* dX_all, float* DG_all, size_t dg_stride,
                               float* DQ_all, float* const* dW_unused, float* work, size_t work_bytes, float* tmp,
                               ggpm_stream_t stream);
/* The same two loops ISSUED by a worker thread of the library: the call returns at once, ggpm_decode_join() waits until
 * the worker has issued everything posted so far (not for the GPU) and returns its first error.  Until then the caller
 * keeps the descriptor, the arrays it points to and every buffer alive, and enqueues what follows the loop on `stream`
 * only after the join.  Lets the ~1.5 ms of host time a loop takes run beside the calling thread's other launches (the
 * encoder's backward, which autograd reaches at the same moment). */
int ggpm_decode_steps_forward_async(const ggpm_decode_steps* steps, const float* const* W, const int* ldw, const float* bu,
                                    const float* X_all, float* Hs_all, float* Cs_all, float* Qs_all, float* St_all,
                                    size_t st_stride, float* wpack, float* tmp, ggpm_stream_t stream);
int ggpm_decode_steps_backward_async(const ggpm_decode_steps* steps, const float* const* W, const int* ldw, const float* X_all,
                                     const float* Hs_all, const float* Cs_all, const float* Qs_all, const float* St_all,
                                     size_t st_stride, float* dF, float* dCF, float* dX_all, float* DG_all, size_t dg_stride,
                                     float* DQ_all, float* const* dW_unused, float* work, size_t work_bytes, float* tmp,
                                     ggpm_stream_t stream);
int ggpm_decode_join(void);
/* Forward-only form of ggpm_decode_steps_forward (no backward follows), and its worker-thread form (join as above): the
 * same sparse_forward calls in the same order without stashes.  Each step runs its depth loop in the scratch Hs / Qs (LSTM:
 * Cs), 2 * max(n) * Hp floats each, and writes the final states of its n rows to F_h (LSTM: F_c) [sum of n][Hp] at rows
 * foff[t] ..; later steps gather their frozen rows from there through srcF.  F_h holds exactly the rows that slot `depth`
 * of every block of the training forward's Hs_all holds, bit for bit.  No Qs_all / St_all. */
int ggpm_decode_steps_infer(const ggpm_decode_steps* steps, const float* const* W, const int* ldw, const float* bu,
                            const float* X_all, float* F_h, float* F_c, float* Hs, float* Cs, float* Qs, float* wpack,
                            ggpm_stream_t stream);
int ggpm_decode_steps_infer_async(const ggpm_decode_steps* steps, const float* const* W, const int* ldw, const float* bu,
                                  const float* X_all, float* F_h, float* F_c, float* Hs, float* Cs, float* Qs, float* wpack,
                                  ggpm_stream_t stream);

/* ------------------------------------------------------------------ one tree-side level of the teacher-forced decoder
 * IncHierMPNEncoder.embed_sub_tree + IncMPNEncoder.forward (ggpm/encoder.py:208-245, 165-179), which
 * HierMPNDecoder.forward calls once per decode step (ggpm/decoder.py:201-222), for ALL steps at once over the decode-time
 * DAG of the level's messages (ggpm_amd/decoder.py: DecodeSchedule._level_plan), as one call per direction:
 *   finput = E[ids]; hnode = relu([finput | lower] W^T + b); hmess = [hnode[mess_inst] | onehot(mess_pos)];
 *   h = sparse_forward(h0, hmess, all real messages, DAG, `depth` = longest chain); node = relu([hnode | sum_in h] W_o^T + b_o)
 * E1 message rows (row 0 = pad) + n_extra frozen rows that carry `extra` (the motif level's pseudo-messages with the root
 * vectors); n_inst visits.  Index tables int32 on the device: ids[n_inst], mess_inst / mess_pos[E1-1], frozen[E1+n_extra],
 * pred_* / succ_* the DAG's CSR and its transpose over E1+n_extra rows, in_* the incoming-message CSR of every visit
 * (n_inst rows) and inT_* its transpose (E1+n_extra rows), srcT_* the transpose of the message -> visit index (n_inst rows).
 * gate_w / gate_b: GRU {W_z, W_r, W_h} ([H, H+20+H]; W_r [H, H+20], gate_b[1] = null) + Ur, bu; LSTM {W_i, W_o, W, W_f}.
 * Dropout must be inactive (the caller falls back to the per-op entry points otherwise).
 * Embedding-input mode (the tree-only decoder's level, IncEncoder): W, b and lower null, He == H -- hnode = E[ids] with no
 * linear and no ReLU; the backward then writes d_finput = d(hnode) and leaves dpre_w (may be null) and d_lower (must be null).
 * forward: `saved` = ggpm_tree_level_saved_floats floats; on return `views` names the intermediates inside it (node
 * [n_inst, Hp] and slot `depth` of Hs [E1+n_extra, Hp] are the level's two results).  backward: d_node / d_hid nullable;
 * `grads` names caller-owned outputs -- full-shape gate weight gradients (both halves written), gate bias gradients
 * (null where the gate has none), dUr / dbu (GRU), dpre_w / dpre_o [n_inst, Hp] and d_finput [n_inst, pad16(He)] for the
 * caller's contractions of W, W_o and the embedding table, d_lower (nullable) and dHin [E1+n_extra, Hp] whose rows E1.. are
 * d(extra); work: ggpm_tree_level_work_bytes. */
typedef struct ggpm_tree_level {
    int lstm, H, He, E1, n_extra, depth, n_inst;
    const int32_t *ids, *mess_inst, *mess_pos;
    const unsigned char* frozen;
    const int32_t *pred_rowptr, *pred_col, *succ_rowptr, *succ_col;
    const int32_t *in_rowptr, *in_col, *inT_rowptr, *inT_col;
    const int32_t *srcT_rowptr, *srcT_col;
    const float* emb; int ld_emb;
    const float *W, *b; int ld_w;
    const float *Wo, *bo; int ld_wo;
    const float* gate_w[4]; int ld_gate[4]; const float* gate_b[4];
    const float *Ur, *bu; int ld_ur;
    const float* lower; int ld_lower;
    const float* extra; int ld_extra;
} ggpm_tree_level;
typedef struct ggpm_tree_level_views {
    float *finput, *hnode, *hmess, *X, *hp, *cp, *Hs, *Cs, *Qs, *St, *wpack, *nei, *node;
} ggpm_tree_level_views;
typedef struct ggpm_tree_level_grads {
    float* dgate_w[4]; int ld_dgate[4]; float* dgate_b[4];
    float *dUr, *dbu;
    float *dpre_w, *dpre_o, *d_finput;
    float* d_lower; int ld_dlower, n_pad_dlower;
    float* dHin;
} ggpm_tree_level_grads;
size_t ggpm_tree_level_saved_floats(const ggpm_tree_level* level);
size_t ggpm_tree_level_work_bytes(const ggpm_tree_level* level);
int ggpm_tree_level_forward(const ggpm_tree_level* level, float* saved, size_t saved_floats, ggpm_tree_level_views* views,
                            ggpm_stream_t stream);
/* Forward-only form of ggpm_tree_level_forward (no backward follows): the same launches in the same order without the
 * depth loop's stashes -- the loop runs in two ping-pong state slots, so `views->Hs` holds 2 slots (LSTM: Cs too) and the
 * final state h^depth is slot depth & 1; views->St is NULL.  node and that final state are bit-identical to the training
 * forward's.  arena: ggpm_tree_level_infer_floats floats. */
size_t ggpm_tree_level_infer_floats(const ggpm_tree_level* level);
int ggpm_tree_level_infer(const ggpm_tree_level* level, float* arena, size_t arena_floats, ggpm_tree_level_views* views,
                          ggpm_stream_t stream);
/* side_stream (nullable): where the level's PARAMETER gradients (grads->dgate_w / dgate_b / dUr / dbu) are formed, behind an
 * event the main stream records after the depth loop -- the gradients that flow on (d_lower, dHin, dpre_*, d_finput) are
 * then not queued behind ~145 us of contractions.  Same launches, same results.  The caller joins that stream before it
 * reads those four outputs and keeps `work` and the forward's `saved` alive until then. */
int ggpm_tree_level_backward(const ggpm_tree_level* level, const ggpm_tree_level_views* views, const float* d_node,
                             const float* d_hid, const ggpm_tree_level_grads* grads, float* work, size_t work_bytes,
                             ggpm_stream_t stream, ggpm_stream_t side_stream);

/* ------------------------------------------------------------------ decoder score-head losses
 * Softmax cross entropy with reduction = sum and the additive vocabulary mask of ggpm/vocab.py:34-41,56-58 fused in
 * (ggpm/decoder.py:66-69,143-157,268-271): z[m,:] = logits[m,:] + mask[mask_row[m],:] (mask / mask_row both null for
 * no mask), loss[0] = sum_m logsumexp(z[m,:]) - z[m,label[m]]; dlogits (nullable) = softmax(z) - onehot(label);
 * argmax (nullable) = first maximal class per row (get_accuracy, ggpm/nnutils.py:84-87).  work: M floats.
 * ggpm_bce_logits: nn.BCEWithLogitsLoss(size_average=False) of the topology head (decoder.py:66,262-264).
 * ggpm_scale_rows: d[m,:] *= scale[0] (upstream gradient held on the device).  All sums are order-fixed. */
int ggpm_softmax_ce(const float* logits, int ld, int M, int N, const float* mask, int ld_mask, const int32_t* mask_row,
                    const int32_t* label, float* loss, float* dlogits, int ld_d, int32_t* argmax, float* work,
                    ggpm_stream_t stream);
int ggpm_bce_logits(const float* x, const float* y, int M, float* loss, float* dx, float* work, ggpm_stream_t stream);
int ggpm_scale_rows(float* d, int ld, int M, int N, const float* scale, ggpm_stream_t stream);
/* The four accuracies of the teacher-forced decoder pass (ggpm/decoder.py:262-283 with get_accuracy / get_accuracy_bin /
 * get_accuracy_sym, ggpm/nnutils.py:84-97) in one launch: out4 = {motif class, attachment class, topology, attachment}.
 * cls_pred / icls_pred: the arg-max ggpm_softmax_ce returned; topo: the topology scores (element i at topo[i * ld_topo]);
 * assm: the [P x C] attachment scores (row stride ld_assm; P = 0: out4[3] = 1 as the reference's `assm_acc = 1`); labels
 * int64 (labels_int64 = 1) or int32. */
int ggpm_head_accuracies(const int32_t* cls_pred, const void* cls_lab, const int32_t* icls_pred, const void* icls_lab,
                         int n_cls, const float* topo, int ld_topo, const void* topo_lab, int n_topo, const float* assm,
                         int ld_assm, int P, int C, int labels_int64, float* out4, ggpm_stream_t stream);

/* KL head, elementwise part of HierPropertyVAE.rsample (ggpm/property_vae.py:26-33) after the two [B,H]x[H,L] products:
 * lv = -|pv|; kl[0] = -0.5 * sum(1 + lv - mean^2 - exp(lv)) / B; z = mean + exp(lv/2) * eps (eps null: z = mean).
 * mean, pv, eps, z, dz, dmean, dpv: contiguous [B, L]; dz / dkl may be null (no gradient from that output). */
int ggpm_rsample_forward(const float* mean, const float* pv, const float* eps, int B, int L, float* z, float* kl,
                         ggpm_stream_t stream);
int ggpm_rsample_backward(const float* mean, const float* pv, const float* eps, const float* dz, const float* dkl,
                          int B, int L, float* dmean, float* dpv, ggpm_stream_t stream);

/* Attachment head of the tree-only decoder (MotifDecoder, ggpm/decoder.py:475-899: enum_attach, get_assm_score and the
 * cross entropy over max_cls_size rows), one launch per direction.  rows: [R x H] E_assm rows (row stride ld_rows), every
 * candidate's k rows consecutive; meta: [P x 6] int32 per prediction {n candidates, k rows per candidate (1 or 2),
 * nth_child, molecule, first candidate, first row}; W1: matchNN.0.weight [H x (H + 20)] (row stride ldw), b1 its bias;
 * Wa / ba: W_assm [L x H] / [L]; z: [B x L] latent (row stride ldz).  The C - n pad rows of a prediction score ba . z.
 * Forward writes act [R x H] (matchNN output per row), score [candidates], stat [P x 4] (for the backward), out[0] = loss
 * sum, out[1] = accuracy (get_accuracy_sym); counter: one int32, zero on entry, zero again on return.
 * Backward (dloss: device scalar) writes drows [R x ld_rows], dW1 [H x (H + 20)] contiguous, db1, dWa [L x H], dba, dz
 * [B x ldz]: plain stores, fixed-order sums, no atomics.  H <= 1024, L <= 1024. */
int ggpm_motif_assm_forward(const float* rows, int ld_rows, const int32_t* meta, int P, int C, int H, int L,
                            const float* W1, int ldw, const float* b1, const float* Wa, const float* ba, const float* z,
                            int ldz, float* act, float* score, float* stat, float* out, int32_t* counter,
                            ggpm_stream_t stream);
int ggpm_motif_assm_backward(const float* dloss, const float* rows, int ld_rows, const int32_t* meta, int P, int C, int H,
                             int L, int B, const float* W1, int ldw, const float* Wa, const float* ba, const float* z,
                             int ldz, const float* act, const float* score, const float* stat, float* drows, float* dW1,
                             float* db1, float* dWa, float* dba, float* dz, ggpm_stream_t stream);
/* ggpm_motif_assm_backward for a per-molecule upstream gradient (bound_loss): prediction p counts with
 * dloss[0] * coef[meta[p][3] * coef_stride] (dloss nullable: 1; a molecule outside [0, B): 0).  Same device code and the same
 * outputs; coef must not be null, coef_stride >= 1. */
int ggpm_motif_assm_backward_weighted(const float* dloss, const float* coef, int coef_stride, const float* rows, int ld_rows,
                                      const int32_t* meta, int P, int C, int H, int L, int B, const float* W1, int ldw,
                                      const float* Wa, const float* ba, const float* z, int ldz, const float* act,
                                      const float* score, const float* stat, float* drows, float* dW1, float* db1, float* dWa,
                                      float* dba, float* dz, ggpm_stream_t stream);

/* Greedy decode of the tree-only decoder (MotifDecoder.decode, ggpm/decoder.py:901-1095; csrc/motif_decode.hip).
 * ggpm_motif_decode_tree_step (two launches): applies the edits -- n_node_edits pairs {node, motif} to fnode [N], then
 * n_tab_edits quads {table 0 agraph [N x 12] / 1 bgraph [E x 12] / 2 fmess [E x 2] (source node, position), row, slot,
 * value} -- then EITHER the read-outs of the n_read nodes (node_out row r = relu(W_o [E_c[fnode[n]] | sum of h over
 * agraph[n]] + b)) OR the n_mess new messages (pairs {message, output row or -1}: reset, input [E_c[fnode[source]] |
 * onehot(position)], `depth` GRU / LSTM iterations over bgraph; h (and c) rows written, the hidden row copied to mess_out
 * row when given).  No new message may appear in another new message's bgraph row.  params: host array of device pointers
 * {E_c [n_motif x H], W_o.0.weight [H x 2H], W_o.0.bias} then GRU {W_z, b_z, W_r, U_r, b_Ur, W_h, b_h} or LSTM {W_i, b_i,
 * W_o, b_o, W_f, b_f, W, b} (contiguous, input width H + max_pos).  h, c: [E x H].  H <= 1024.
 * ggpm_motif_decode_mlp (two launches): out[r] = W2 relu(W1 [vecs[r] | ctx[bidx[r]]] + b1) + b2 (sigmoid if asked);
 * W1 [H x (H + L)], W2 [n_out x H] contiguous; hid: [M x ld_hid] scratch.
 * ggpm_hier_topk (one launch, one workgroup per row): nnutils.hier_topk of (cls [M x n_cls], icls [M x n_icls]) with the
 * mask 0 / -1000 from owner[n_icls] (the motif each attachment belongs to); root != 0: the arg-max motif of the raw cls
 * row and the top k of its masked icls row.  out [M x 3k] int32: k scores (fp32 bits), k motifs, k attachments.  Ties: the
 * lower index.  k <= 16.
 * ggpm_motif_decode_assm_score (one launch, one workgroup per meta row {n candidates, k (1 or 2), nth_child, molecule,
 * first candidate, first id}): (W_assm sum_{j<k} relu(matchNN [E_assm[id_j] | onehot(nth)]) + b) . z[molecule], written
 * to score[first candidate .. + n) (enum_attach reads no candidate atom: the n candidates score the same).  E_assm:
 * [n_ids x H]; a row with k, nth or an id out of range scores NaN. */
int ggpm_motif_decode_tree_step(int rnn_type, int H, int max_pos, int depth, const void* const* params, int32_t* fnode,
                                int32_t* fmess, int32_t* agraph, int32_t* bgraph, int N, int E, float* h, float* c,
                                const int32_t* edits, int n_node_edits, int n_tab_edits, const int32_t* nodes, int n_read,
                                float* node_out, int ld_node, const int32_t* mess, int n_mess, float* mess_out,
                                int ld_mess, ggpm_stream_t stream);
int ggpm_motif_decode_mlp(const float* vecs, int ld_v, const int32_t* bidx, const float* ctx, int ld_ctx, int M, int H,
                          int L, const float* W1, const float* b1, const float* W2, const float* b2, int n_out,
                          int sigmoid, float* hid, int ld_hid, float* out, int ld_out, ggpm_stream_t stream);
int ggpm_hier_topk(const float* cls, int ld_cls, int n_cls, const float* icls, int ld_icls, int n_icls,
                   const int32_t* owner, int M, int k, int root, int32_t* out, ggpm_stream_t stream);
int ggpm_motif_decode_assm_score(const float* E_assm, int n_ids, int H, int L, const int32_t* meta, const int32_t* ids,
                                 int P, const float* W1, int ldw, const float* b1, const float* Wa, const float* ba,
                                 const float* z, int ldz, float* score, ggpm_stream_t stream);

/* Greedy decode of the hierarchical decoder (HierMPNDecoder.decode, ggpm/decoder.py:303-472; csrc/hier_decode.hip).
 * dims: host int[14] {rnn_type, H, max_pos, N, E, NA, EA, atom_size, edge_fdim, diterT, diterG, n_motif, n_attach, B}.
 * state: host array of 21 device pointers, resident for the decode -- the tree tables fnode [N x 2], fmess [E x 2] (source
 * node, position), agraph [N x 12], bgraph [E x 12], cgraph [N x 30] (int32); the atom tables fnode [NA x atom_size], fmess
 * [EA x edge_fdim] (fp32), agraph [EA x 10], bgraph [EA x 10] (int32); the atom level's states h0, h1, c0, c1 [EA x H] (two
 * buffers: a Jacobi iteration reads one and writes the other; both agree between calls); the atom read-outs [NA x H] and
 * the step that wrote each [NA] (int32); the inter level's h, c and the tree level's h, c [E x H]; the inter and tree node
 * inputs of the current call [B x H].  The c pointers may be null for GRU.
 * params: host array of 36 device pointers (contiguous fp32) -- the atom, inter and tree cells, 8 slots each (GRU {W_z, b_z,
 * W_r, U_r, b_Ur, W_h, b_h, unused}, LSTM {W_i, b_i, W_o, b_o, W_f, b_f, W, b}; input widths edge_fdim, H + max_pos,
 * H + max_pos), then graph_encoder.W_o.0 {weight [H x (atom_size + H)], bias}, inter_encoder.W_o.0, tree_encoder.W_o.0
 * {weight [H x 2H], bias}, E_i [n_attach x H], E_c [n_motif x H], W_i.0 {weight [H x 2H], bias}, W_c.0 {weight, bias}.
 * ggpm_hier_decode_atom_step (2 + diterG launches): `up` holds, at the int32 offsets offs[0..10], the tree edits (counts[0]
 * quads {table 0 agraph / 1 bgraph / 2 fmess / 3 fnode / 4 cgraph, row, slot, value}), then for the atom tables fnode,
 * fmess, agraph, bgraph the ids of counts[1..4] changed rows and those rows (fp32 bits for the first two), then counts[5]
 * cluster messages and counts[6] cluster atoms.  Applies the edits, resets the listed messages, runs diterG Jacobi
 * iterations of the GRU / LSTM over them (input row fmess, neighbours bgraph), writes relu(W_o [fnode | sum of h over
 * agraph]) of the listed atoms to the read-out rows and stamps them with `stamp`.
 * ggpm_hier_decode_tree_step: per node of `nodes` (n_nodes <= B) the inter input relu(W_i [E_i[fnode[.,1]] | sum over
 * cgraph of the read-out rows stamped `stamp`]) and the tree input relu(W_c [E_c[fnode[.,0]] | inter read-out]).  n_mess
 * == 0 (1 launch; n_edits must be 0): both levels' read-outs, the tree's to node_out row r.  n_mess > 0 (5 launches): the
 * tree edits, then per level the new messages (pairs {message, mess_out row or -1}: reset, input [node input of the source
 * node, zero when it is not among `nodes` | onehot(position)], diterT sparse iterations over bgraph), inter before tree;
 * the tree level's hidden rows go to mess_out.  No new message may appear in another new message's bgraph row.
 * ggpm_hier_decode_assm_score (1 launch, one workgroup per candidate): meta rows {n candidates, k (1 or 2), nth_child,
 * molecule, first candidate, first id, first atom}; candidate c of a row reads k atoms from `atoms` and scores
 * (W_assm sum_{j<k} relu(matchNN [read-out[atom_j] | E_assm[id_j] | onehot(nth)]) + b) . z[molecule]; a read-out row not
 * stamped `stamp` reads as zero.  W1 [H x ldw], ldw >= 2H + max_pos.  A candidate whose row is out of range scores NaN. */
int ggpm_hier_decode_atom_step(const int* dims, void* const* state, const void* const* params, const int32_t* up,
                               const int* offs, const int* counts, int stamp, ggpm_stream_t stream);
int ggpm_hier_decode_tree_step(const int* dims, void* const* state, const void* const* params, const int32_t* edits,
                               int n_edits, const int32_t* nodes, int n_nodes, const int32_t* mess, int n_mess, int stamp,
                               float* node_out, int ld_node, float* mess_out, int ld_mess, ggpm_stream_t stream);
int ggpm_hier_decode_assm_score(const int* dims, void* const* state, const float* E_assm, const int32_t* meta,
                                const int32_t* ids, const int32_t* atoms, int P, int n_cand, int n_ids, int n_atoms,
                                const float* W1, int ldw, const float* b1, const float* Wa, const float* ba, int L,
                                const float* z, int ldz, int stamp, float* score, ggpm_stream_t stream);

/* Seeded draws of the sampled decode (decode_sampled; the reference's greedy=False, ggpm/decoder.py:371-374, 409-416) and of
 * the prior (HierPropertyVAE.sample, ggpm/property_vae.py:35-37); csrc/sample.hip.  Stateless and counter-based:
 *     base = mix(mix(id * 0x9E3779B1 + seed_lo) ^ (seed_hi + site * 0x7F4A7C15))
 *     m(site, id, step, slot) = mix(base + (step * 64 + slot) * 0x9E3779B1) >> 8          (24 bits)
 * in 32-bit arithmetic, mix = the murmur3 32-bit finaliser of ggpm_dropout().  `ids` [B] holds the sample id (the stream
 * key) of every molecule, `bidx` the molecule of every row; nothing else about the launch enters a draw.
 * ggpm_sample_topo (one launch): draw[i] = m(TOPO, ids[bidx[i]], step, 0) * 2^-24 < p[i] ? 1.f : 0.f, i < n.
 * ggpm_sample_beam_order (one launch, one wave per row): topk is ggpm_hier_topk's out [M x 3k]; with key_q = score_q -
 * log(e_q), e_q = max(-log((m(BEAM, ids[bidx[r]], step, q) + 1) * 2^-24), 2^-24), order [M x k] lists the entries q by
 * descending key, ties to the lower q: a draw without replacement with probabilities proportional to exp(score_q).
 * 1 <= k <= GGPM_SAMPLE_MAX_K.
 * ggpm_sample_normal (one launch): out[r, c] = sqrt(-2 log((m0 + 1) * 2^-24)) * cos(2 pi m1 * 2^-24) with m0 / m1 =
 * m(PRIOR, ids[r], c, 0 / 1), for c < cols; columns cols..ld of a row are left alone.  rows * cols < 2^31.
 * A null pointer, n / M / rows / cols <= 0, step < 0, ld < cols or k outside its range returns GGPM_ERR_ARG; nothing is
 * launched then. */
#define GGPM_SITE_SAMPLE_TOPO 256   /* sites no dropout mask uses */
#define GGPM_SITE_SAMPLE_BEAM 257
#define GGPM_SITE_SAMPLE_PRIOR 258
#define GGPM_SAMPLE_MAX_K 16
int ggpm_sample_topo(const float* p, const int32_t* bidx, const int32_t* ids, int n, int step, unsigned int seed_lo,
                     unsigned int seed_hi, float* draw, ggpm_stream_t stream);
int ggpm_sample_beam_order(const int32_t* topk, const int32_t* bidx, const int32_t* ids, int M, int k, int step,
                           unsigned int seed_lo, unsigned int seed_hi, int32_t* order, ggpm_stream_t stream);
int ggpm_sample_normal(float* out, int rows, int cols, int ld, const int32_t* ids, unsigned int seed_lo,
                       unsigned int seed_hi, ggpm_stream_t stream);

/* Per-molecule likelihood terms of the teacher-forced decoder (log_likelihood of the four VAEs; csrc/mol_loss.hip and, for
 * the draw, csrc/sample.hip).  One wave owns one output element and adds in a fixed order: no atomics, bitwise reproducible;
 * sums are carried in fp64 and rounded to fp32 once.  1 <= K <= GGPM_LIKELIHOOD_MAX_K samples, B molecules, L latent columns.
 * ggpm_sample_latent_normal (one launch): out[k, b, c] = the Box-Muller normal of ggpm_sample_normal from the words
 * m(LATENT, ids[b], k * L + c, 0 / 1): a molecule's draws depend on its id, k, c and the seed only, and the first K samples of
 * a larger call are the K-sample call's.  K * L < 2^26, K * B * L < 2^31.
 * ggpm_mol_loss_parts (one launch): parts[b, t] = sum over the rows r < n_rows of term t with mol[r] == b of
 * row_loss[r * stride], t < GGPM_MOL_LOSS_TERMS (topology BCE, motif-class CE, attachment-class CE, attachment CE): what
 * ggpm_softmax_ce / ggpm_bce_logits leave in `work` (stride 1) or ggpm_motif_assm_forward in `stat` (stride 4, from
 * stat + 2).  `terms` is a host array of GGPM_MOL_LOSS_TERMS entries; an absent term has n_rows 0 (its pointers may be
 * null) and a molecule without rows in a term gets 0.  A row whose molecule is outside [0, B) is counted nowhere.
 * ggpm_latent_terms (one launch): with lv = -|pre_var|,
 *     z[k, b, j] = mean[b, j] + exp(lv[b, j] / 2) * eps[k, b, j]          (fp32, ggpm_rsample_forward's expression)
 *     kl[b] = -0.5 * sum_j (1 + lv - mean^2 - exp(lv))                     (ggpm/property_vae.py:26-33 before its / B;
 *                                                                           fp32 addends, ggpm_rsample_forward's)
 *     logpq[k, b] = log p(z_k) - log q(z_k | x_b) = -0.5 * sum_j z^2 + 0.5 * sum_j (eps^2 + lv)     (the 2 pi terms cancel)
 * mean, pre_var [B x L], eps and z [K x B x L], all dense.
 * ggpm_iwae_finish (one launch): with nll[k, b] = sum_t parts[k, b, t],
 *     elbo[b] = -mean_k nll[k, b] - kl[b]
 *     iwae[b] = logsumexp_k (logpq[k, b] - nll[k, b]) - log K               (maximum subtracted before the exponentials)
 * A null pointer, a size <= 0, K outside its range, a negative n_rows or a stride < 1 returns GGPM_ERR_ARG; nothing is
 * launched then. */
#define GGPM_SITE_SAMPLE_LATENT 259
#define GGPM_LIKELIHOOD_MAX_K 1024
#define GGPM_MOL_LOSS_TERMS 4
typedef struct ggpm_mol_loss_term {
    const float* row_loss;      /* device, n_rows values `stride` floats apart */
    const int32_t* mol;         /* device, the molecule of every row */
    int stride, n_rows;
} ggpm_mol_loss_term;
int ggpm_sample_latent_normal(float* out, int K, int B, int L, const int32_t* ids, unsigned int seed_lo,
                              unsigned int seed_hi, ggpm_stream_t stream);
int ggpm_mol_loss_parts(const ggpm_mol_loss_term* terms, int B, float* parts, ggpm_stream_t stream);
int ggpm_latent_terms(const float* mean, const float* pre_var, const float* eps, int K, int B, int L, float* z, float* kl,
                      float* logpq, ggpm_stream_t stream);
int ggpm_iwae_finish(const float* parts, const float* logpq, const float* kl, int K, int B, float* elbo, float* iwae,
                     ggpm_stream_t stream);

/* Training on the bound (bound_loss of the four VAEs; csrc/mol_loss.hip): the same conventions as the entries above.
 * ggpm_bound_objective (two launches): with nll, kl, logpq as above and w (nullable: all ones) the molecules' weights,
 *     GGPM_BOUND_ELBO: loss = (1/B) sum_b w_b ((1/K) sum_k nll[k, b] + beta kl[b])
 *                      c_nll[k, b] = w_b / (K B), c_logpq = 0, c_kl[b] = beta w_b / B
 *     GGPM_BOUND_IWAE: loss = -(1/B) sum_b w_b (logsumexp_k (logpq - nll)[k, b] - log K)            (beta must be 1)
 *                      c_nll[k, b] = w_b softmax_k(logpq - nll)[k, b] / B, c_logpq = -c_nll, c_kl = 0
 * c_* are the partial derivatives of loss by nll, logpq and kl; the softmax is formed in fp64 with the maximum subtracted.
 * work: B doubles (the molecules' addends, summed in molecule order by one wave and rounded once).
 * ggpm_scale_rows_by_mol (one launch): d[m, 0:N] *= g[0] * coef[mol[m] * coef_stride] for the M rows of d (row stride
 * ld >= N; g nullable: 1); a row whose molecule is outside [0, B) becomes 0, as ggpm_mol_loss_parts counts it nowhere.
 * ggpm_latent_terms_backward (one launch): with G[k, b] = g[0] c_logpq[k, b], a = dz[k, b, j] - G z[k, b, j], gk = g[0] c_kl[b],
 *     dmean[b, j] = sum_k a + gk mean
 *     dlv[b, j]   = sum_k (a exp(lv / 2) eps[k, b, j] / 2 + G / 2) - gk (1 - exp(lv)) / 2
 *     dpre_var    = -sign(pre_var) dlv                                     (0 at pre_var = 0, as ggpm_rsample_backward)
 * dz is the gradient that reached z (not scaled by g); dz, c_logpq, c_kl and g are nullable (zeros, zeros, zeros, 1).  The
 * sum over k is formed in fp64 in a fixed order.
 * A null required pointer, a size <= 0, K outside its range, ld < N, a stride < 1, an unknown objective or beta != 1 with
 * GGPM_BOUND_IWAE returns GGPM_ERR_ARG; nothing is launched then. */
#define GGPM_BOUND_ELBO 0
#define GGPM_BOUND_IWAE 1
int ggpm_bound_objective(const float* parts, const float* logpq, const float* kl, const float* w, int K, int B, int objective,
                         float beta, double* work, float* loss, float* c_nll, float* c_logpq, float* c_kl,
                         ggpm_stream_t stream);
int ggpm_scale_rows_by_mol(float* d, int ld, int M, int N, const int32_t* mol, const float* coef, int coef_stride, int B,
                           const float* g, ggpm_stream_t stream);
int ggpm_latent_terms_backward(const float* dz, const float* mean, const float* pre_var, const float* eps,
                               const float* c_logpq, const float* c_kl, const float* g, int K, int B, int L, float* dmean,
                               float* dpre_var, ggpm_stream_t stream);

/* Path-derivative estimators of the importance-weighted bound (bound_loss(objective="iwae", estimator="stl" | "dreg") of the
 * four VAEs; csrc/mol_loss.hip): the conventions of the entries above.
 * ggpm_iwae_weights (one launch, one wave per molecule): with nll[k, b] = sum_t parts[k, b, t] as ggpm_bound_objective forms it,
 *     s[k, b] = softmax_k (logpq - nll)[k, b]          (fp64, the maximum subtracted; GGPM_BOUND_IWAE's c_nll is w_b s / B)
 *     ess[b]  = 1 / sum_k s[k, b]^2                     (the unrounded weights; between 1 and K)
 * ess is nullable.
 * ggpm_latent_terms_backward_path (one launch, one wave per (b, j)): the gradient by mean and pre_var with the parameters of
 * log q(z | mean, lv) held fixed, so that d(-log q)/dz = eps / sd and lv has no direct term.  With sd = expf(lv / 2) and
 * z = mean + sd eps (fp32, ggpm_latent_terms' expressions), r = exp(-lv / 2) formed in fp64 from the fp32 lv,
 * G[k, b] = g[0] c_logpq[k, b] and q[k, b] = s[k, b] (s null: 1),
 *     t = dz[k, b, j] - G z                          a = t + G eps r
 *     dmean[b, j] = sum_k q a
 *     dlv[b, j]   = sum_k q (t sd eps / 2 + G eps^2 / 2)
 *     dpre_var    = -sign(pre_var) dlv                (0 at pre_var = 0)
 * s null is the "sticking the landing" estimator, s = ggpm_iwae_weights' the doubly reparameterised one.  A sample with
 * G eps = 0 adds no r term (r may be inf there).  dz is the gradient that reached z (not scaled by g); dz, c_logpq, s and g
 * are nullable (zeros, zeros, ones, 1).  The sums over k are formed in fp64 in a fixed order.  The size limits are
 * ggpm_latent_terms_backward's.
 * A null required pointer, a size <= 0 or K outside its range returns GGPM_ERR_ARG; nothing is launched then. */
int ggpm_iwae_weights(const float* parts, const float* logpq, int K, int B, float* s, float* ess, ggpm_stream_t stream);
int ggpm_latent_terms_backward_path(const float* dz, const float* mean, const float* pre_var, const float* eps,
                                    const float* c_logpq, const float* s, const float* g, int K, int B, int L, float* dmean,
                                    float* dpre_var, ggpm_stream_t stream);

/* The latent column by column (latent_stats and bound_loss(free_bits=) of the four VAEs; csrc/latent_dims.hip): the
 * conventions of the entries above -- one wave per output with its lanes striding the molecules, fp64 partials through a fixed
 * shuffle tree, one rounding where a value is stored, no atomics, bitwise reproducible.  With lv = -|pre_var|,
 *     a[b, j] = 1 + lv - mean^2 - expf(lv)      (fp32: the addend of ggpm_latent_terms' kl and of ggpm_rsample_forward)
 *     kl_dim[b, j] = -0.5 a[b, j]                (sum_j kl_dim[b, j] is kl[b] of ggpm_latent_terms before its rounding)
 * mean, pre_var [B x L] dense, B * L < 2^31.
 * ggpm_latent_dim_accumulate (one launch, one wave per column): acc is double[GGPM_LATENT_STAT_ROWS][L] on the device, zeroed
 * once by the caller; the call ADDS to it: row 0 += B, row 1 += sum_b mean, row 2 += sum_b mean^2 (the squares exact in fp64),
 * row 3 += sum_b expf(lv), row 4 += sum_b kl_dim.  Calls on one stream are ordered, so a data set is accumulated batch by
 * batch without a host synchronisation; calls on different streams into one acc must be ordered by the caller.
 * ggpm_latent_dim_finish (one launch, one wave): out is float[GGPM_LATENT_STAT_OUT][L]; with N = acc row 0, in fp64,
 *     row 0 kl_dims     = row 4 / N                      row 3 sigma2_mean = row 3 / N
 *     row 1 mu_mean     = row 1 / N                      row 4 agg_var     = mu_var + sigma2_mean
 *     row 2 mu_var      = max(row 2 / N - mu_mean^2, 0)  (the population variance of the posterior means)
 * each rounded once.  n_active[0] = the number of columns whose STORED (fp32) mu_var > au_threshold.  A column with N = 0
 * gives zeros and counts as inactive.  acc is only read: accumulation may go on afterwards.
 * ggpm_free_bits_kl (one launch, one workgroup): with w (nullable: all ones) the molecules' weights, in fp64,
 *     klbar_j = (1/B) sum_b w_b kl_dim[b, j]             kl_dims[j] = (float)klbar_j
 *     term[0] = (float) sum_j max((double)lambda, klbar_j)      (one wave, its lanes striding j, then the shuffle tree)
 * 1 <= L <= GGPM_FREE_BITS_MAX_L: the workgroup keeps the L fp64 column sums in LDS (32 KiB at the limit).  With lambda = 0,
 * beta * term is the KL part of GGPM_BOUND_ELBO's loss up to the order of summation.
 * ggpm_free_bits_kl_backward (one launch, one wave per column): with c[b, j] = g[0] w_b / B where klbar_j > lambda, else 0,
 *     dmean = c mean        dlv = -c (1 - expf(lv)) / 2        dpre_var = -sign(pre_var) dlv     (0 at pre_var = 0)
 * WRITTEN to dmean / dpre_var (not added); g nullable: 1.  The comparison is strict and made in fp64 on the very klbar_j of the
 * forward (a column exactly at lambda is free): the backward re-forms the column sum with the forward's own code.
 * kl_dims_gate (nullable): the forward's kl_dims of the same inputs.  Rounding is monotone and lambda is a fp32 value, so a
 * kl_dims[j] above (below) lambda already says klbar_j is above (below) it and the sum of that column is not re-formed; a
 * kl_dims[j] equal to lambda decides nothing and the sum is re-formed.  The result is the same with and without it.
 * A null required pointer, a size <= 0, L above its limit, a negative or NaN lambda or a NaN au_threshold returns
 * GGPM_ERR_ARG; nothing is launched then. */
#define GGPM_LATENT_STAT_ROWS 5
#define GGPM_LATENT_STAT_OUT 5
#define GGPM_FREE_BITS_MAX_L 4096
int ggpm_latent_dim_accumulate(const float* mean, const float* pre_var, int B, int L, double* acc, ggpm_stream_t stream);
int ggpm_latent_dim_finish(const double* acc, int L, float au_threshold, float* out, int32_t* n_active, ggpm_stream_t stream);
int ggpm_free_bits_kl(const float* mean, const float* pre_var, const float* w, int B, int L, float lambda, float* kl_dims,
                      float* term, ggpm_stream_t stream);
int ggpm_free_bits_kl_backward(const float* mean, const float* pre_var, const float* w, const float* kl_dims_gate, int B, int L,
                               float lambda, const float* g, float* dmean, float* dpre_var, ggpm_stream_t stream);

/* The KL split across the batch (latent_decomposition and bound_loss(objective="tcvae") of the four VAEs;
 * csrc/latent_decomp.hip): Chen et al.'s split of E_x KL(q(z|x) || p(z)) into the index-code mutual information, the total
 * correlation and the dimension-wise KL, estimated by minibatch-weighted sampling.  z [K x B x L] the draws, mean, pre_var
 * [B x L] the posteriors, lv = -|pre_var|, log_nb = log(N B) with N the size of the data set.  EVERYTHING below is formed in
 * fp64 from the fp32 inputs (exp / log on double); fixed reduction orders, no atomics, bitwise reproducible; one rounding where
 * a fp32 value is stored.
 *     ell[k,i,j,l] = -0.5 (log 2pi + lv[j,l] + (z[k,i,l] - mean[j,l])^2 exp(-lv[j,l]))
 *     S[k,i,j] = sum_l ell      A[k,i] = logsumexp_j S      D[k,i,l] = logsumexp_j ell      logp[k,i] = sum_l -0.5 (log 2pi + z^2)
 * ggpm_latent_decomp (one launch, one workgroup of 4 waves per draw (k, i)):
 *     comps[k,i,0] = mi   = S[k,i,i] - A + log_nb
 *     comps[k,i,1] = tc   = A - sum_l D + (L - 1) log_nb
 *     comps[k,i,2] = dwkl = sum_l D - L log_nb - logp
 *     dwkl_dim[k,i,l]     = D - log_nb + 0.5 (log 2pi + z^2)                          (nullable)
 *     lse_joint[k,i] = A,  lse_dim[k,i,l] = D   (double; both nullable for a forward-only call)
 * mi + tc + dwkl = S[k,i,i] - logp[k,i] whatever log_nb is.
 * ggpm_latent_decomp_backward (two launches): with (a, b, c3) = coef[k,i,0:3] the gradients that reached mi, tc and dwkl,
 * p = exp(S - A), r = exp(ell - D), G[k,i,j,l] = a [i == j] + (b - a) p + (c3 - b) r, d = z[k,i,l] - mean[j,l], iv = exp(-lv[j,l]):
 *     dz[k,i,l]   = sum_j G (-d iv) + c3 z[k,i,l]             (row pass: one workgroup per draw; p[0:B] in LDS)
 *     dmean[j,l]  = sum_{k,i} G d iv                          (column pass: one workgroup per molecule and 64 columns)
 *     dlv[j,l]    = sum_{k,i} G (-0.5 + 0.5 d^2 iv)           dpre_var = -sign(pre_var) dlv     (0 at pre_var = 0)
 * WRITTEN (not added); partial derivatives with z, mean and pre_var held independent.  lse_joint / lse_dim: the forward's, of
 * the same inputs.
 * ggpm_latent_decomp_accumulate (one launch, one wave per cell): acc is double[GGPM_LATENT_DECOMP_ROWS + L] on the device,
 * zeroed once by the caller; the call ADDS to it: acc[0] += K B, acc[1 + t] += sum_{k,i} comps[k,i,t],
 * acc[GGPM_LATENT_DECOMP_ROWS + l] += sum_{k,i} dwkl_dim[k,i,l].  Ordering as for ggpm_latent_dim_accumulate.
 * 1 <= K <= GGPM_LIKELIHOOD_MAX_K, 1 <= B <= GGPM_LATENT_DECOMP_MAX_B, 1 <= L <= GGPM_FREE_BITS_MAX_L, K * B * L < 2^31,
 * log_nb finite.  A null required pointer or a size outside these limits returns GGPM_ERR_ARG; nothing is launched then. */
#define GGPM_LATENT_DECOMP_ROWS 4
#define GGPM_LATENT_DECOMP_MAX_B 4096
int ggpm_latent_decomp(const float* z, const float* mean, const float* pre_var, int K, int B, int L, double log_nb, float* comps,
                       float* dwkl_dim, double* lse_joint, double* lse_dim, ggpm_stream_t stream);
int ggpm_latent_decomp_backward(const float* z, const float* mean, const float* pre_var, const double* lse_joint,
                                const double* lse_dim, const float* coef, int K, int B, int L, float* dz, float* dmean,
                                float* dpre_var, ggpm_stream_t stream);
int ggpm_latent_decomp_accumulate(const float* comps, const float* dwkl_dim, int K, int B, int L, double* acc,
                                  ggpm_stream_t stream);

/* A learnable mixture-of-Gaussians prior (prior.MixturePrior and the prior= of log_likelihood, bound_loss and sample of the four
 * VAEs; csrc/latent_prior.hip): p(z) = sum_c pi_c N(z; m_c, diag(exp(s_c))), pi = softmax(a), with logits a [C], means m
 * [C x L] and log_vars s [C x L]; z [R x L] (R = K B for the objectives: one call covers all K draws); everything fp32 and
 * dense.  The conventions of ggpm_latent_decomp: EVERYTHING below is formed in fp64 from the fp32 inputs (exp / log on
 * double); fixed reduction orders, no atomics, bitwise reproducible; one rounding where a fp32 value is stored.
 *     comp[r,c] = (a_c - logsumexp a) - 0.5 sum_j (log 2pi + s[c,j] + (z[r,j] - m[c,j])^2 exp(-s[c,j]))
 *     lp[r]     = logsumexp_c comp[r,c]                logn[r] = -0.5 sum_j (log 2pi + z[r,j]^2)
 * ggpm_mixture_logp (one launch, one workgroup of 4 waves per row: wave w takes the components w, w + 4, ... with its lanes
 * striding j; comp[r, 0:C] stays in LDS):
 *     logp[r] = lp      ratio[r] = lp - logn   (the difference formed in fp64)      resp[r,c] = exp(comp - lp)   (nullable)
 *     comp_stash[r,c] = comp,  logp_stash[r] = lp   (double; both nullable for a forward-only call)
 * ggpm_mixture_logp_backward (at most two launches): with g[r] the gradient that reached ratio[r] (on_logp = 0) or logp[r]
 * (on_logp = 1), gamma[r,c] = exp(comp_stash - logp_stash), d = z[r,j] - m[c,j], iv = exp(-s[c,j]):
 *     dz[r,j] = g_r (sum_c gamma (-d iv) + [on_logp = 0] z[r,j])        (row pass: one workgroup per row, gamma[r, 0:C] in LDS,
 *                                                                        wave w takes the columns w, w + 4, ..., lanes stride c)
 *     dmeans[c,j]    = sum_r g_r gamma d iv                             (column pass: one workgroup per component and 64
 *     dlog_vars[c,j] = sum_r g_r gamma 0.5 (d^2 iv - 1)                  columns; wave w takes the rows w, w + 4, ... in that
 *     dlogits[c]     = sum_r g_r (gamma - pi_c)                          order, the waves' partials are added in wave order)
 * WRITTEN (not added).  dz is nullable (no row pass); dmeans, dlog_vars and dlogits are nullable as a group (all three or none:
 * no column pass, for a frozen prior); all four null is refused.  The stashes are the forward's, of the same inputs.
 * ggpm_sample_mixture (one launch, one wave per row): with u = m(PRIOR_COMP, ids[r], 0, 0) 2^-24 (the seeded stream of
 * ggpm_sample_normal) and e_c = exp(a_c - max a), comp[r] (int32, nullable) = the smallest c whose prefix sum e_0 + ... + e_c,
 * taken in index order, exceeds u * sum_c e_c -- the last component with e_c > 0 if rounding leaves none -- and
 *     out[r, j] = fmaf(expf(0.5f s[c,j]), n[r,j], m[c,j]),  j < cols = L            (fp32)
 * with n[r,j] exactly ggpm_sample_normal's value for (seed, ids[r], j); columns cols..ld of a row are left alone.  A draw
 * depends on the seed, the id and the column only.
 * 1 <= C <= GGPM_MIXTURE_MAX_C: the workgroup of each of the three keeps one fp64 value per component in LDS (comp, gamma,
 * e: 32 KiB at the limit, half of what a workgroup may declare statically).  1 <= L <= GGPM_FREE_BITS_MAX_L, R >= 1,
 * R * L < 2^31 and R * C < 2^31 (rows for R and cols for L in ggpm_sample_mixture, ld >= cols).  A null required pointer, a size
 * outside these limits, on_logp other than 0 / 1 or a partly given gradient group returns GGPM_ERR_ARG; nothing is launched
 * then. */
#define GGPM_SITE_SAMPLE_PRIOR_COMP 260
#define GGPM_MIXTURE_MAX_C 4096
int ggpm_mixture_logp(const float* z, const float* logits, const float* means, const float* log_vars, int R, int C, int L,
                      float* logp, float* ratio, float* resp, double* comp_stash, double* logp_stash, ggpm_stream_t stream);
int ggpm_mixture_logp_backward(const float* z, const float* logits, const float* means, const float* log_vars,
                               const double* comp_stash, const double* logp_stash, const float* g, int on_logp, int R, int C,
                               int L, float* dz, float* dmeans, float* dlog_vars, float* dlogits, ggpm_stream_t stream);
int ggpm_sample_mixture(const float* logits, const float* means, const float* log_vars, int C, float* out, int rows, int cols,
                        int ld, const int32_t* ids, unsigned int seed_lo, unsigned int seed_hi, int32_t* comp,
                        ggpm_stream_t stream);

/* The guided latent search (PropertyVAEOptimizer.search; csrc/latent_search.hip): R = K B trajectories, row r
 * of z0 [R x ld] belonging to molecule b = r mod B (the layout of z [K, B, L]), L = 2 half, v = the row's first L columns:
 *     prop(v)   = w_h (f_homo(v[0:half]) - t_homo[b])^2 + w_l (f_lumo(v[half:L]) - t_lumo[b])^2
 *     anchor(v) = 0.5 sum_j (v_j - mu[b,j])^2 exp(-lv[b,j])
 *     prior(v)  = -log p(v): 0.5 sum_j (log 2pi + v_j^2) with the mixture pointers null, else -lp of ggpm_mixture_logp
 *     J(v)      = prop + anchor_weight anchor + prior_weight prior
 * ggpm_latent_search_guided (ONE launch for all rows and every step; one workgroup of 256 threads per row, the heads walked
 * as ggpm_property_latent_search walks them; heads in eval form, no dropout):
 *     m = 0; n = 0
 *     repeat `steps` times:
 *       o_x = f_x(v_x); prop = w_h (o_h - t_h)^2 + w_l (o_l - t_l)^2
 *       if delta >= 0 and prop <= delta: stop (no update)
 *       g = 2 w_x (o_x - t_x) df_x/dv  [+ anchor_weight (v - mu) exp(-lv)]  [+ prior_weight d prior/dv]
 *       m = momentum m + g;  v = v - lr m;  n += 1
 * (a term whose weight is exactly 0 is not evaluated inside the loop), then the heads and the three terms on the final v:
 *     z_out [R x ld] (columns past L copied from z0), pred[2][R] (homo row, then lumo row), terms [R x 3] = prop, anchor,
 *     prior (unweighted), J [R] = (prop + anchor_weight anchor) + prior_weight prior, steps_taken [R] = n.
 * Arithmetic: heads, anchor gradient, standard-normal gradient (v) and the update are fp32 with contraction off (every
 * product and sum above is one rounding, in the order written; exp(-lv) is expf, formed once); the dot products are fma
 * chains as in ggpm_property_latent_search.  The mixture's gradient sum_c gamma_c (v_j - m[c,j]) exp(-s[c,j]) -- comp, the
 * logsumexp and gamma included -- is fp64 from the fp32 inputs in a fixed order and rounded once to fp32 before it is weighed.
 * The reported anchor and prior are summed in fp64 from the fp32 v, mu and expf(-lv) and rounded once; prop and J are fp32.
 * No atomics: the same inputs give the same bits, and a row's results do not depend on B, K or the other rows.
 * LDS: the heads' plan of ggpm_property_latent_search plus 4 L floats (momentum, mu, exp(-lv), the mixture gradient) and
 * C + 1 doubles.  The weights of both heads stay in LDS when all of it fits in 160 KiB, otherwise they are read from global
 * memory; if even that does not fit, GGPM_ERR_UNSUPPORTED.
 * K, B >= 1, K B <= 2^20, ld >= L, steps >= 0; logits [C], means [C x L], log_vars [C x L] all null or all given with
 * 1 <= C <= GGPM_MIXTURE_MAX_C; delta < 0 (or NaN) disables the exit.  A null required pointer, a bad size or a partly given
 * mixture returns GGPM_ERR_ARG; heads outside the envelope above (2 <= n_linear <= GGPM_PROP_MAX_LINEAR, half <= 256, hidden
 * widths <= 512) or K B > 2^20 return GGPM_ERR_UNSUPPORTED; nothing is launched then.
 * ggpm_latent_search_select (one launch, one thread per molecule): best_k[b] (int32) = the k in 0..K-1 with the smallest
 * J[k B + b]; ties go to the lowest k; a NaN ranks behind every number (+-inf included); all K NaN gives 0.  With
 * r = best_k[b] B + b: z_best[b, 0:ld] = z[r, 0:ld], pred_best[2][B] = pred[.][r], terms_best[b, 0:3] = terms[r, 0:3].
 * Every pointer required, K, B, ld >= 1, K B <= 2^20, else GGPM_ERR_ARG. */
int ggpm_latent_search_guided(int K, int B, const float* z0, int ld, int half, const float* mu, const float* lv,
                              const ggpm_prop_head* homo, const ggpm_prop_head* lumo, const float* t_homo, const float* t_lumo,
                              const float* logits, const float* means, const float* log_vars, int C, float lr, float momentum,
                              int steps, float delta, float w_h, float w_l, float anchor_weight, float prior_weight,
                              float* z_out, float* pred, float* terms, float* J, int32_t* steps_taken, ggpm_stream_t stream);
int ggpm_latent_search_select(const float* J, const float* z, const float* pred, const float* terms, int K, int B, int ld,
                              int32_t* best_k, float* z_best, float* pred_best, float* terms_best, ggpm_stream_t stream);

/* ------------------------------------------------------------------ whole-encoder drivers
 * HierMPNEncoder.forward (ggpm/encoder.py:140-157, with embed_graph/inter/tree/root :96-138) and its backward as ONE
 * call each: the same kernels the op-by-op host path issues, sequenced from C++ (GRU or LSTM message function).
 * Inputs are the A0 tensors of MolGraph.tensorize() after make_cuda (int64, row-major) plus the molecules' root node
 * ids; outputs are [rows, Hp] with zero pad columns (Hp = ggpm_padded_hidden(H)).
 * params / grads: 35 (GRU) or 38 (LSTM) device pointers, contiguous fp32, in this order (shapes as in the reference
 * state_dict): E_c.0.weight, E_i.0.weight, W_c.0.weight, W_c.0.bias, W_i.0.weight, W_i.0.bias, W_root.0.weight,
 *   W_root.0.bias, then for tree_encoder, inter_encoder, graph_encoder: W_o.0.weight, W_o.0.bias and the cell's
 *   GRU:  rnn.W_z.weight, rnn.W_z.bias, rnn.W_r.weight, rnn.U_r.weight, rnn.U_r.bias, rnn.W_h.weight, rnn.W_h.bias
 *   LSTM: rnn.W_i.0.weight, rnn.W_i.0.bias, rnn.W_o.0.weight, rnn.W_o.0.bias, rnn.W.0.weight, rnn.W.0.bias,
 *         rnn.W_f.0.weight, rnn.W_f.0.bias.
 * saved: ggpm_encoder_saved_bytes() bytes written by the forward and read by the backward; work: backward scratch of
 * ggpm_encoder_work_bytes().  side_stream (may be 0): transposed CSRs and all weight-gradient contractions run there,
 * event-ordered against `stream`; on return from the backward `stream` is ordered behind it.  d_* may be null.
 * phase: 0 = whole backward; 1 = all but the atom level, 2 = atom level + final join (same arguments, same work
 * arena): between the two a data-parallel caller starts all-reducing the gradients of every slot before graph_encoder.
 * Dropout (ggpm/encoder.py:15-19, 52-72: after E_c, E_i, W_c, W_i and every level's W_o): `dropout` > 0 applies the
 * counter-based masks of ggpm_dropout() with `seed_lo/seed_hi` at sites 0 E_i rows, 1 E_c rows, 2 atom-level W_o,
 * 3 W_i, 4 attachment-level W_o, 5 W_c, 6 motif-level W_o; the backward regenerates the same masks from the seed. */
typedef struct ggpm_enc_dims {
    int H, He, depthT, depthG, atom_size, n_motif, n_attach;
    int N1g, E1g, Kg_a, Kg_b;            /* atom graph: nodes+1, messages+1, agraph / bgraph widths */
    int N1t, E1t, Kt_a, Kt_b, Kt_c;      /* motif tree: nodes+1, messages+1, agraph / bgraph / cgraph widths */
    int B;                               /* molecules */
    int rnn_type;                        /* 0 GRU, 1 LSTM */
    int tree_chain;                      /* longest dependency chain among the motif-tree messages of this batch (message
                                            u->v depends on the messages w->u, w != v), or 0 if unknown.  The tree is
                                            acyclic, so after that many steps every message has reached its fixed point:
                                            the two tree-side levels then run tree_chain + 1 of their depthT steps and
                                            replicate the last stash slot -- bit-identical to running all of them
                                            (ggpm/rnn.py:41-50 iterates a fixed depth regardless). */
    float dropout;                       /* drop probability of the training forward (0: none / eval) */
    unsigned int seed_lo, seed_hi;       /* mask stream of this forward/backward pair */
    int gate_dtype;                      /* as ggpm_level_opts.gate_dtype.  0: fp32 gate products (the 1e-4 parity configurations);
                                            2: fp32 on v_mfma_f32_16x16x4_f32 only;
                                            1: bf16 operands, fp32 accumulate (v_mfma_f32_16x16x32_bf16) for the H x H gate
                                            products of the depth loops -- BASELINE configs[4].  State, stashes, gate math,
                                            input projections and weight-gradient contractions stay fp32. */
    int prefer_narrow;                   /* as ggpm_level_opts.prefer_narrow, for every level call of this driver call */
} ggpm_enc_dims;
size_t ggpm_encoder_saved_bytes(const ggpm_enc_dims* dims);
size_t ggpm_encoder_work_bytes(const ggpm_enc_dims* dims);
int ggpm_encoder_forward(const ggpm_enc_dims* dims, float* const* params, const int64_t* tfnode, const int64_t* tfmess,
                         const int64_t* tagraph, const int64_t* tbgraph, const int64_t* tcgraph, const int64_t* gfnode,
                         const int64_t* gfmess, const int64_t* gagraph, const int64_t* gbgraph, const int32_t* roots,
                         void* saved, size_t saved_bytes, float* hroot, float* hnode, float* hinter, float* hatom,
                         ggpm_stream_t stream, ggpm_stream_t side_stream);
/* Forward-only form of ggpm_encoder_forward, for calls no backward follows (no-grad evaluation, latent encoding): the
 * same launches that compute values, in the same order, with the same dropout masks (dims->dropout as above), so the four
 * outputs are bit-identical to ggpm_encoder_forward's (fp32 and gate dtype 1 alike).  `arena`:
 * ggpm_encoder_infer_bytes() bytes of scratch, free again when the call's work on `stream` has run: the forward CSRs and
 * index columns, the tree-side inputs, per-level neighbour sums and ONE depth-loop scratch shared by the three levels (hoisted
 * inputs, two ping-pong state slots, the level's result: ggpm_level_opts.h_out) -- no per-depth stashes, no transposed CSRs.
 * side_stream (may be 0): the tree-side layout runs there beside the atom level, as in the training forward. */
size_t ggpm_encoder_infer_bytes(const ggpm_enc_dims* dims);
int ggpm_encoder_infer(const ggpm_enc_dims* dims, float* const* params, const int64_t* tfnode, const int64_t* tfmess,
                       const int64_t* tagraph, const int64_t* tbgraph, const int64_t* tcgraph, const int64_t* gfnode,
                       const int64_t* gfmess, const int64_t* gagraph, const int64_t* gbgraph, const int32_t* roots,
                       void* arena, size_t arena_bytes, float* hroot, float* hnode, float* hinter, float* hatom,
                       ggpm_stream_t stream, ggpm_stream_t side_stream);
int ggpm_encoder_backward(const ggpm_enc_dims* dims, float* const* params, float* const* grads, const int32_t* roots,
                          void* saved, size_t saved_bytes, const float* hroot, const float* hnode, const float* hinter,
                          const float* hatom, const float* d_hroot, const float* d_hnode, const float* d_hinter,
                          const float* d_hatom, void* work, size_t work_bytes, int phase, ggpm_stream_t stream,
                          ggpm_stream_t side_stream);

/* ------------------------------------------------------------------ instrumentation
 * When a timing sink is installed, every depth-step kernel launch is bracketed by HIP events on its own
 * stream; ggpm_timing_collect() synchronises those events and returns launches / total milliseconds /
 * algorithmic flops for kernel class `which` (0 gru_fwd_a, 1 gru_bwd_a, 2 lstm_fwd_a, 3 lstm_bwd_a,
 * 4 gru_fwd_b, 5 gru_bwd_b, 6 lstm_fwd_b, 7 lstm_bwd_b) + 8 * level tag (0 launches issued through the per-op
 * entry points, 1 atom level, 2 attachment level, 3 motif level of ggpm_encoder_forward / _backward), so that the
 * atom-level launch (one workgroup per CU, MFMA bound) is reported apart from the small latency-bound levels.
 * Used by bench.py for roofline.achieved; off by default (no events, no overhead). */
int ggpm_timing_enable(int on);
int ggpm_timing_collect(int which, int* launches, double* total_ms, double* flops);

/* ------------------------------------------------------------------ gate-function self-test (tests only)
 * out[i] = f(x[i]) for n <= 2^30 device floats, f being a device gate function exactly as the level kernels compile
 * it: which = 0 the gather sigmoid of the fp32 gate modes, 1 the gather sigmoid of the bf16 gate mode, 2 the libm
 * sigmoid of the gate epilogues.  NaN arguments give NaN; -inf gives 0 (or a flushed denormal), +inf gives 1. */
int ggpm_selftest_gate_math(int which, const float* x, int n, float* out, ggpm_stream_t stream);

/* ------------------------------------------------------------------ decode schedule (host only, no GPU work)
 * The integer bookkeeping of the teacher-forced decoder for one tensorized batch, which the reference interleaves
 * with device work on every step of HierMPNDecoder.forward (ggpm/decoder.py:186-259: the per-step subtree / subgraph
 * lists, update_graph_mask :85-100, init_decoder_state :102-122, apply_tree_mask / apply_graph_mask :72-83, the
 * prediction tuples) and IncHierMPNEncoder.get_sub_tensor (ggpm/encoder.py:195-206), derived once per batch:
 * the tables of ggpm_amd.decoder.DecodeSchedule (from_tensors, _level_plan) and ggpm_amd.atom_decode.AtomPlan
 * (compact row sets, compact_tables) -- the numpy forms there are the checker (tests/test_schedule_native.py).
 * Inputs are host arrays, int64, row-major, in the MolGraph.tensorize layout (ggpm/mol_graph.py:199-281):
 *   tree  fnode [Nt1 x 2], fmess [Et1 x 4], agraph [Nt1 x At], bgraph [Et1 x Kt], cgraph [Nt1 x C], scope [B x 2];
 *   graph fmess [Eg1 x 4], agraph [Ng1 x Ag], bgraph [Eg1 x Kg];
 *   orders [n x 3] = (x, y or -1 for None, label) of all molecules back to back, order_off [B + 1];
 *   per tree node v: the attachment ids of its inter_label, icls[icls_off[v] .. icls_off[v+1]) (k_v = their number), and
 *   its assm_cands as cand_off[v+1] - cand_off[v] candidates of k_v atoms each, flat from cands[cand_atom_off[v]].
 * depth / gates: also build the tables that depend on the decoder's diterG and cell (3 GRU / 4 LSTM); 0 = leave out.
 * The int32 pack also carries the index structures the device would otherwise derive per batch from those tables
 * (ggpm_padded_to_csr / ggpm_csr_transpose semantics: in-row order kept, transposed rows ascending): for the two
 * tree-side levels L in {inter, tree} pred_L / succ_L / in_L / inT_L (_rp, _col) and frozen_L (bytes), the message ->
 * visit transpose srcT, the transposes topoT / clsT / assmT of the heads' molecule indices, and iota (the rowptr of any
 * one-entry-per-row CSR); every _col table ends with one pad entry so that none is empty.
 * Returns an opaque handle (NULL: malformed input); tables are read with ggpm_schedule_get by name (pack 0 = host
 * only; 1 / 2 = inside the int64 / int32 device pack; ggpm_schedule_pack returns a pack's base, `offset` is in bytes from it).  The
 * call keeps no global state and may run on any thread. */
typedef struct ggpm_sched_in {
    int B, Nt1, Et1, At, Kt, C;
    int Ng1, Eg1, Ag, Kg;
    int depth, gates;
    const int64_t *tfnode, *tfmess, *tagraph, *tbgraph, *cgraph, *tree_scope;
    const int64_t *gfmess, *gagraph, *gbgraph;
    const int64_t *orders, *order_off;
    const int64_t *icls_off, *icls;
    const int64_t *cand_off, *cand_atom_off, *cands;
} ggpm_sched_in;
void* ggpm_schedule_build(const ggpm_sched_in* in);
int ggpm_schedule_get(void* handle, const char* name, const void** data, int64_t* count, int* elem_bytes, int* pack,
                      int64_t* offset);
int ggpm_schedule_pack(void* handle, int pack, const void** data, int64_t* bytes);
int ggpm_schedule_names(void* handle, char* out, int64_t capacity);      /* newline-separated table names */
/* (pack, byte offset, count, element bytes) per table in the order of ggpm_schedule_names.  Returns the number of
 * tables, or -GGPM_ERR_* on error.  `capacity` in int64 elements (4 per table). */
int ggpm_schedule_directory(void* handle, int64_t* out, int64_t capacity);
void ggpm_schedule_free(void* handle);

#ifdef __cplusplus
}
#endif
#endif /* GGPM_HIP_H */
