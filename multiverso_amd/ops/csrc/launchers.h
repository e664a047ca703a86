// The launchers of kernels.hip, declared once for both translation units:
// kernels.hip defines them, bindings.cpp calls them. They have C linkage,
// so a definition and a call that disagreed on an argument would still link;
// with this header in both files the compiler refuses the disagreement.

#pragma once

#include <hip/hip_runtime_api.h>
#include <cstdint>

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
void mv_launch_row_gather(void*, int, const float*, const int64_t*, int64_t,
                          int64_t, hipStream_t);
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
}
