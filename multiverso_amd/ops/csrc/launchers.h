// The launchers of kernels.hip, declared once for both translation units:
// kernels.hip defines them, bindings.cpp calls them. They have C linkage,
// so a definition and a call that disagreed on an argument would still link;
// with this header in both files the compiler refuses the disagreement.

#pragma once

#include <hip/hip_runtime_api.h>
#include <cstdint>

// The list of a pooled Add, the same for every updater: vals [P, cols] holds
// fp32, or bf16 when wire has WIRE_DELTA; rows [n] are the sorted local ids,
// perm [n] the caller's position of each; src [n] (the row of vals, below P)
// and wts [n] (or null) are in caller order. n and P are below 2^31; n == 0
// launches nothing. The row-wise AdaGrad launcher alone also takes a null src
// (the keyed Add: position p names row p of vals, so vals has n rows) and
// then a null perm (the identity: rows is in caller order).
struct MvUnpool {
  const void* vals;
  int wire;
  const int64_t* rows;
  const int64_t* perm;
  const int64_t* src;
  const float* wts;
  int64_t n, cols;
};

extern "C" {
// elementwise updaters: a non-null `out` (the pointer before `wire`)
// selects the fused Add+Get form. The fp32 forms take the delta and `out`
// as void* and, in `wire`, the WIRE_* bits that say which holds bf16. The
// trailing int of the updaters is the sweep direction (1 = descending): a
// performance hint, the result is the same either way.
void mv_launch_copy(void*, const float*, int, int64_t, hipStream_t);
void mv_launch_add(float*, const void*, int, int64_t, hipStream_t, int);
void mv_launch_add_f64(double*, const double*, int64_t, hipStream_t, int);
void mv_launch_add_i32(int32_t*, const int32_t*, int64_t, hipStream_t, int);
void mv_launch_add_i64(int64_t*, const int64_t*, int64_t, hipStream_t, int);
void mv_launch_sgd(float*, const void*, void*, int, float, int64_t,
                   hipStream_t, int);
void mv_launch_sgd_f64(double*, const double*, double*, double, int64_t,
                       hipStream_t, int);
void mv_launch_momentum(float*, float*, const void*, void*, int, float,
                        int64_t, hipStream_t, int);
void mv_launch_momentum_f64(double*, double*, const double*, double, int64_t,
                            hipStream_t, int);
void mv_launch_adagrad(float*, float*, const void*, void*, int, float, float,
                       float, int64_t, hipStream_t, int);
void mv_launch_adagrad_f64(double*, double*, const double*, double, double,
                           double, int64_t, hipStream_t, int);
void mv_launch_dcasgd(float*, float*, const void*, void*, int, float, float,
                      int64_t, hipStream_t, int);
void mv_launch_dcasgda(float*, float*, float*, const void*, void*, int, float,
                       float, float, float, int64_t, hipStream_t, int);
// adam: (..., b1, b2, step = lr/(1-b1^t), rbc2 = 1/sqrt(1-b2^t),
// decay = 1-lr*wd, eps, n), all scalars in double
void mv_launch_adam(float*, float*, float*, const void*, void*, int, double,
                    double, double, double, double, double, int64_t,
                    hipStream_t, int);
void mv_launch_adam_f64(double*, double*, double*, const double*, double,
                        double, double, double, double, double, int64_t,
                        hipStream_t, int);
// keyed kernels: `vals` (the gather's `out`) is void* followed by `wire`
void mv_launch_onebit_encode(const float*, float*, uint8_t*, int64_t,
                             hipStream_t);
void mv_launch_onebit_decode_sum(float*, const uint8_t*, int, int64_t,
                                 hipStream_t);
// top-k wire: (..., n, keep)
void mv_launch_topk_encode(const float*, float*, uint8_t*, int64_t, int,
                           hipStream_t);
void mv_launch_topk_decode_sum(float*, const uint8_t*, int, int64_t, int,
                               hipStream_t);
void mv_launch_row_gather(void*, int, const float*, const int64_t*, int64_t,
                          int64_t, hipStream_t);
// destination-indexed K6: (out, shard, rows, nrows, cols), unique rows
void mv_launch_row_gather_at(float*, const float*, const int64_t*, int64_t,
                             int64_t, hipStream_t);
// pooled rows: (out [B, cols], wire, shard, rows [nnz], offsets [B+1],
// weights [nnz] or null, B, cols); out[b] = sum of shard[rows[i]] (times
// weights[i]) over offsets[b] <= i < offsets[b+1], in list order. B and nnz
// are below 2^31 and nnz is not 0; B == 0 launches nothing.
void mv_launch_row_pool(void*, int, const float*, const int64_t*,
                        const int64_t*, const float*, int64_t, int64_t,
                        hipStream_t);
// stale-row lists over the byte bitmap [workers, R], 1 <= R < 2^31, for nw
// workers from w0 (1 <= nw <= 65535). tiles(R) is the tiles per worker.
// count (bitmap, R, w0, nw, tile_count [nw*tiles], plan): plan [nw*tiles + nw
// + 1] gets the tile bases, then each worker's total, then the grand total.
// emit (bitmap, R, w0, nw, plan, ids [n], n) over the unchanged bitmap.
int64_t mv_stale_tiles(int64_t);
void mv_launch_stale_count(const uint8_t*, int64_t, int, int, int*, int64_t*,
                           hipStream_t);
void mv_launch_stale_emit(uint8_t*, int64_t, int, int, const int64_t*,
                          int64_t*, int64_t, hipStream_t);
void mv_launch_row_scatter_add(float*, const void*, int, const int64_t*, float,
                               int64_t, int64_t, int, hipStream_t);
void mv_launch_row_scatter_adagrad(float*, float*, const void*, int,
                                   const int64_t*, float, float, float,
                                   int64_t, int64_t, int, hipStream_t);
// keyed stateful updaters: (shard, state..., vals, wire, rows, perm-or-null,
// scalars..., nrows, cols)
void mv_launch_row_momentum(float*, float*, const void*, int, const int64_t*,
                            const int64_t*, float, int64_t, int64_t,
                            hipStream_t);
void mv_launch_row_dcasgd(float*, float*, const void*, int, const int64_t*,
                          const int64_t*, float, float, int64_t, int64_t,
                          hipStream_t);
void mv_launch_row_dcasgda(float*, float*, float*, const void*, int,
                           const int64_t*, const int64_t*, float, float,
                           float, float, int64_t, int64_t, hipStream_t);
void mv_launch_row_adam(float*, float*, float*, const void*, int,
                        const int64_t*, const int64_t*, double, double,
                        double, double, double, double, int64_t, int64_t,
                        hipStream_t);
// pooled Add (k_row_unpool): (shard, state..., scalars..., list). Row
// rows[k] of the shard gets the sum of weights[p] * vals[src[p]] over its run
// of equal ids, p = perm[k], in list order, then one updater step.
void mv_launch_unpool_sgd(float*, float, const MvUnpool*, hipStream_t);
void mv_launch_unpool_adagrad(float*, float*, float, float, float,
                              const MvUnpool*, hipStream_t);
void mv_launch_unpool_momentum(float*, float*, float, const MvUnpool*,
                               hipStream_t);
void mv_launch_unpool_dcasgd(float*, float*, float, float, const MvUnpool*,
                             hipStream_t);
void mv_launch_unpool_dcasgda(float*, float*, float*, float, float, float,
                              float, const MvUnpool*, hipStream_t);
void mv_launch_unpool_adam(float*, float*, float*, double, double, double,
                           double, double, double, const MvUnpool*,
                           hipStream_t);
// row-wise AdaGrad (k_rowwise_elem, k_row_unpool_rowwise): gsq holds ONE
// accumulator per row. Whole shard: (data, gsq [rows], delta, out-or-null,
// wire, lr, rho, eps, rows, cols, stream, reverse); keyed and pooled: the
// arguments of mv_launch_unpool_adagrad. Both return 0, having launched
// nothing, when a row is wider than one lane group holds: 1024 columns with
// cols % 4 == 0 and aligned pointers, 256 otherwise.
int mv_launch_rowwise_adagrad(float*, float*, const void*, void*, int, float,
                              float, float, int64_t, int64_t, hipStream_t,
                              int);
int mv_launch_unpool_rowwise_adagrad(float*, float*, float, float, float,
                                     const MvUnpool*, hipStream_t);
// word2vec: (in_emb, out_emb, in_gsq, out_gsq, in_idx, in_off, ...,
// groups, dim, use_adagrad, use_atomic)
void mv_launch_w2v(float*, float*, float*, float*, const int64_t*, const int*,
                   const int64_t*, const float*, const int*, float, int64_t,
                   int64_t, int, int, hipStream_t);
void mv_launch_w2v_ns(float*, float*, float*, float*, const int64_t*,
                      const int*, const int64_t*, const int64_t*, int64_t,
                      int, uint64_t, float, int64_t, int64_t, int, int,
                      hipStream_t);
// sparse logreg forwards: (table, keys, vals, ptr, labels, wts-or-null, err,
// loss, scalars..., B[, K]); scatters: (table, keys, vals, ptr, err,
// scalars..., B[, K]). The FTRL table is the (z | n) state, its first
// scalar 1/alpha.
void mv_launch_lr_sigmoid_fwd(const float*, const int64_t*, const float*,
                              const int*, const float*, const float*,
                              float*, float*, int64_t, hipStream_t);
void mv_launch_lr_sigmoid_scatter(float*, const int64_t*, const float*,
                                  const int*, const float*, float, int,
                                  float, int64_t, hipStream_t);
void mv_launch_lr_softmax_fwd(const float*, const int64_t*, const float*,
                              const int*, const float*, const float*,
                              float*, float*, int64_t, int64_t, hipStream_t);
void mv_launch_lr_softmax_scatter(float*, const int64_t*, const float*,
                                  const int*, const float*, float, int,
                                  float, int64_t, int64_t, hipStream_t);
void mv_launch_lr_ftrl_fwd(const float*, const int64_t*, const float*,
                           const int*, const float*, const float*, float*,
                           float*, float, float, float, float, int64_t,
                           int64_t, hipStream_t);
void mv_launch_lr_ftrl_scatter(float*, const int64_t*, const float*,
                               const int*, const float*, float, float,
                               float, float, int64_t, int64_t, hipStream_t);
// class-per-lane forwards, same arguments as the two forwards above: softmax
// for 65..1024 classes, FTRL for 33..1024 outputs (the scatters above serve
// any K)
void mv_launch_lr_softmax_wide_fwd(const float*, const int64_t*, const float*,
                                   const int*, const float*, const float*,
                                   float*, float*, int64_t, int64_t,
                                   hipStream_t);
void mv_launch_lr_ftrl_wide_fwd(const float*, const int64_t*, const float*,
                                const int*, const float*, const float*,
                                float*, float*, float, float, float, float,
                                int64_t, int64_t, hipStream_t);
// dense post for 65..1024 columns, same arguments as mv_launch_lr_dense_post
void mv_launch_lr_dense_post_wide(float*, const float*, const float*, float*,
                                  float, int64_t, int64_t, hipStream_t);
// dense logreg: post (logits, labels, wts-or-null, loss_acc, inv_b, B, K);
// fwd (X, W, labels, wts-or-null, diff, loss_acc, inv_b, B, d, K, nt),
// which returns 0 when the caller has to take the GEMM + post path
void mv_launch_lr_dense_post(float*, const float*, const float*, float*,
                             float, int64_t, int64_t, hipStream_t);
int mv_launch_lr_dense_fwd(const float*, const float*, const float*,
                           const float*, float*, float*, float, int64_t,
                           int64_t, int64_t, int, hipStream_t);
// nearest rows: plan (R, cols, Q, &waves) returns the queries one pass takes,
// 0 when the launcher cannot run the request (one query's cols*4 bytes exceed
// the LDS budget), and in `waves` the lists per query the partials must hold.
// launch (shard, queries, part_scores [min(Q,16)*waves*k], part_rows (same),
// out_scores [Q,k], out_ids [Q,k], R, cols, Q, k, cosine, row_offset) returns
// 0 on the same refusal, having launched nothing. R == 0 launches nothing
// and leaves the outputs as they are.
int mv_row_topk_plan(int64_t, int64_t, int64_t, int*);
int mv_launch_row_topk(const float*, const float*, float*, int*, float*,
                       int64_t*, int64_t, int64_t, int64_t, int64_t, int,
                       int64_t, hipStream_t);
// nearest rows for query batches (k_row_topk_mm, the MFMA scan), the same two
// signatures: plan returns the queries one pass takes (up to 64), 0 when the
// launcher cannot run the request (R too large for int row indices, or more
// than 2048 columns), and in `lists` the workgroups, each with one list per
// query. launch takes partials of min(Q,64)*lists*k pairs.
int mv_row_topk_mm_plan(int64_t, int64_t, int64_t, int*);
int mv_launch_row_topk_mm(const float*, const float*, float*, int*, float*,
                          int64_t*, int64_t, int64_t, int64_t, int64_t, int,
                          int64_t, hipStream_t);
}
