// CDNA4 (gfx950 / MI355X) kernels for multiverso_amd.
//
// These are the rebuild's equivalents of the reference's CPU hot loops
// (SURVEY.md §2.9): K1 dense add (src/updater/updater.cpp:25-28), K2 SGD
// (sgd_updater.h:16-18), K3 momentum (momentum_updater.h:19-24), K4 adagrad
// (adagrad_updater.h:27-40, with the accumulator bug fixed), K5/K6 row
// scatter/gather (matrix_table.cpp:406-412 / :444-450).
//
// Design (per the CDNA4 HIP guide): every kernel here is memory-bound, so
// the shape is {block = 256 threads (4 waves of 64), float4 16B/lane
// vectorized loads/stores, grid-stride}. The grid cap is probe-swept per
// stream count (defines below): UPD_GRID = 768 blocks for add/sgd,
// STATE_GRID = 768 for the stateful updaters, both with or without the
// fused Get buffer, ELEM_GRID = 1024 for the plain copy and the f64/int
// forms; MAX_GRID = 2048 (256 CUs x 8 blocks) only caps the row-keyed,
// word2vec and logreg kernels. Whole-shard passes alternate their sweep
// direction so that the Infinity Cache serves the turning end (SWEEP note
// at launch_elem). The stateful updaters (momentum/adagrad/dcasgd/adam) fuse
// the state read-modify-write into the same pass as the weight update — one
// trip through HBM3E instead of the 3-4 separate passes a torch-op
// composition would make.
//
// No CUDA compatibility paths: this file is HIP-only, compiled by hipcc
// with --offload-arch=gfx950.

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "launchers.h"

#define WAVE 64
#define BLOCK 256
#define MAX_GRID 2048
// elementwise streaming kernels saturate HBM at a smaller grid
// (tools/probe_sgd.hip sweep: 5.85 TB/s at 1024 blocks w/ nontemporal
// access vs 5.16 at 2048 plain). Kernels with >=4 concurrent HBM streams
// (fused add+get, momentum/adagrad/dcasgd state updates) peak lower
// still: 6.05/5.84 TB/s at 768 blocks vs 5.45/5.15 at 1024 (same sweep).
#define ELEM_GRID 1024
#define STATE_GRID 768
// 3-stream update kernels (read data + read delta + write data) peak at
// 768 blocks, not 1024: 6.05-6.07 vs 5.85-5.86 TB/s on two boxes
// (tools/probe_sgd2.hip round-2 sweep). The pure 2-stream copy keeps
// ELEM_GRID (6.15 at 1024).
#define UPD_GRID 768
// The fused Add+Get bodies ran FAT blocks (COPY_BLOCK = 1024 threads x 768)
// while every pass swept forward: 6.14 TB/s vs 5.87 at 256x768 on the
// round-2 box (tools/probe_sgd2.hip). Under the alternating sweep they do
// not (tools/probe_sweep_dir.hip, range over its runs, ms per 2.0 GB
// pass, delta never reused): a CU holds 32 waves, so only 512 of 768
// 16-wave blocks are resident at once, the other 256 start late at the far
// end and break the front the next pass turns on; 1024x768 alternating
// 0.343-0.358 (forward, all non-temporal, as before: 0.361-0.377), and at
// 1024x512, all resident, 0.323-0.331. 256x768 (3 blocks of 4 waves per CU,
// all resident) 0.292-0.298 and 256x512 0.289-0.295; 256x384, x640, x1024
// and x2048 are slower (0.307-0.333). The fused bodies therefore use BLOCK
// threads and their updater's own cap, chosen for residency; 768 over 512
// because the 3-stream body is level between them and the 6-stream body
// was measured with the shard-only policy at 768 (0.498 vs 0.571 forward).
// COPY_BLOCK stays the block of k_lr_dense_fwd.
#define COPY_BLOCK 1024

typedef float v4f __attribute__((ext_vector_type(4)));

// Streaming access helpers, overloaded so each updater body is written
// once: the float4 forms are non-temporal, the scalar forms (fp32 tails,
// double, int) are plain loads and stores.
static __device__ __forceinline__ v4f ntload(const v4f* p) {
  return __builtin_nontemporal_load(p);
}
static __device__ __forceinline__ void ntstore(v4f* p, v4f v) {
  __builtin_nontemporal_store(v, p);
}
template <class T>
static __device__ __forceinline__ T ntload(const T* p) { return *p; }
template <class T>
static __device__ __forceinline__ void ntstore(T* p, T v) { *p = v; }

static __device__ __forceinline__ float rsq(float x) {
  return __frsqrt_rn(x);
}
static __device__ __forceinline__ v4f rsq(v4f x) {
  v4f r;
  r.x = __frsqrt_rn(x.x); r.y = __frsqrt_rn(x.y);
  r.z = __frsqrt_rn(x.z); r.w = __frsqrt_rn(x.w);
  return r;
}

// element i of a T array viewed as an array of V (V = T, or v4f over float)
template <class V, class T>
static __device__ __forceinline__ V ld(const T* p, int64_t i) {
  return ntload((const V*)p + i);
}
template <class V, class T>
static __device__ __forceinline__ void st(T* p, int64_t i, V v) {
  ntstore((V*)p + i, v);
}

// The shard's own load in a whole-shard pass (KEEP) is a plain, cacheable
// one; everything else such a pass touches stays non-temporal. Consecutive
// passes run in opposite directions (k_elem's `rev`), and only a plainly
// loaded line is still served by the Infinity Cache when the next pass
// comes back to it; a non-temporal load never hits, and the state, delta
// and Get-buffer streams kept non-temporal leave the cache to the shard
// (tools/probe_sweep_dir.hip, profiles/sweep_direction.md). The row-keyed
// kernels keep the non-temporal form (KEEP = false).
template <class V, bool KEEP, class T>
static __device__ __forceinline__ V ld_shard(const T* p, int64_t i) {
  if constexpr (KEEP) return *((const V*)p + i);
  else return ld<V>(p, i);
}

// bf16 wire format: the delta / vals a kernel reads and the Get buffer it
// writes may hold bfloat16 while the shard and all state stay fp32. bf16 is
// storage only: the ld/st overloads below widen on load and narrow on
// store, so every formula keeps its one fp32 body. A V of 4 (2) floats
// moves as one 8-byte (4-byte) access; those need that alignment, which the
// launchers check.
struct bf16 { uint16_t bits; };
typedef uint16_t v4h __attribute__((ext_vector_type(4)));
typedef uint16_t v2h __attribute__((ext_vector_type(2)));

// exact: bf16 is the top half of the fp32 with the same value
static __device__ __forceinline__ float widen(uint16_t h) {
  return __builtin_bit_cast(float, (uint32_t)h << 16);
}
// round to nearest even with gfx950's packed convert (v_cvt_pk_bf16_f32).
// Checked on the device over all 2^32 inputs against the integer form
// (u + 0x7FFF + ((u >> 16) & 1)) >> 16, which is torch's .to(torch.bfloat16):
// equal bits for every finite value and +-inf (denormals round like any
// other value, a large finite value carries into inf), and a NaN stays a NaN
// (tools/probe_bf16_cvt.hip, profiles/bf16_wire.md)
static __device__ __forceinline__ uint16_t narrow(float f) {
  return __builtin_bit_cast(uint16_t, (__bf16)f);
}

template <class V>
static __device__ __forceinline__ V ld(const bf16* p, int64_t i) {
  if constexpr (std::is_same<V, v4f>::value) {
    v4h h = __builtin_nontemporal_load((const v4h*)p + i);
    v4f v;
    v.x = widen(h.x); v.y = widen(h.y); v.z = widen(h.z); v.w = widen(h.w);
    return v;
  } else {
    static_assert(std::is_same<V, float>::value, "bf16 widens to fp32");
    return widen(p[i].bits);
  }
}
// V = v4f (non-temporal, the streaming kernels), float4 / float2 (plain, the
// row gather) or float
template <class V>
static __device__ __forceinline__ void st(bf16* p, int64_t i, V v) {
  if constexpr (sizeof(V) == 16) {
    v4h h;
    h.x = narrow(v.x); h.y = narrow(v.y); h.z = narrow(v.z); h.w = narrow(v.w);
    if constexpr (std::is_same<V, v4f>::value)
      __builtin_nontemporal_store(h, (v4h*)p + i);
    else
      *((v4h*)p + i) = h;
  } else if constexpr (sizeof(V) == 8) {
    v2h h;
    h.x = narrow(v.x); h.y = narrow(v.y);
    *((v2h*)p + i) = h;
  } else {
    p[i].bits = narrow(v);
  }
}

// which pointers of a launch hold bf16 (the `wire` argument of the
// launchers below): the delta or vals, the Get buffer
#define WIRE_DELTA 1
#define WIRE_OUT 2
#define ELEM_OF(p) std::remove_cv_t<std::remove_pointer_t<decltype(p)>>

// f(delta, out) with each pointer cast to what `wire` says it holds
template <class F>
static void with_wire(int wire, const void* delta, void* out, F f) {
  switch (wire & (WIRE_DELTA | WIRE_OUT)) {
    case 0: f((const float*)delta, (float*)out); break;
    case WIRE_DELTA: f((const bf16*)delta, (float*)out); break;
    case WIRE_OUT: f((const float*)delta, (bf16*)out); break;
    default: f((const bf16*)delta, (bf16*)out);
  }
}

// fp32 buffers are 16-byte aligned torch allocations; a bf16 one can be a
// view such as x[1:] or a slice of a staged blob, 2 bytes off
static inline bool vec_ok(const float*) { return true; }
static inline bool vec_ok(const bf16* p) { return ((uintptr_t)p & 7) == 0; }

static inline int grid_for_cap(int64_t work_items, int cap,
                               int block = BLOCK) {
  int64_t blocks = (work_items + block - 1) / block;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}
static inline int grid_for(int64_t work_items) {
  return grid_for_cap(work_items, MAX_GRID);
}

// ---------------------------------------------------------------------------
// Elementwise updaters (K1-K4 + DC-ASGD). One op struct per updater holds
// its pointers and scalars; step<V>(i) applies the update to element i of
// the arrays viewed as V and returns the new weight. fp32 runs V = v4f over
// the n/4 body and V = float over the n%4 tail (all pointers are
// 16B-aligned torch allocs); double (every updater the reference
// instantiates, array_table.cpp:153-154) and int32/int64 (add-only,
// updater.cpp:40-43) run the same ops with V = T, plain scalar access.
// D is the delta's element type: T, or bf16 on an fp32 shard (widened by ld).
// Every step issues all its loads before its first store: struct members
// carry no __restrict__, so a load written after a store would wait for it.
// The momentum, DC-ASGD and Adam ops keep their formula in
// step_at<V>(i, g), which takes the gradient as a value (step loads it from
// delta first): the row-keyed k_row_update below hands it a per-row sum
// instead.
// ---------------------------------------------------------------------------

template <class T, class D = T>
struct AddOp {
  using elem = T;
  T* data; const D* delta;
  template <class V> __device__ __forceinline__ V step(int64_t i) const {
    V v = ld_shard<V, true>(data, i) + ld<V>(delta, i);
    st(data, i, v);
    return v;
  }
};

// sign = -1 is sgd; the fused Add+Get passes +1 for the default (add)
// updater.
template <class T, class D = T>
struct SgdOp {
  using elem = T;
  T* data; const D* delta; T sign;
  template <class V> __device__ __forceinline__ V step(int64_t i) const {
    V v = ld_shard<V, true>(data, i) + sign * ld<V>(delta, i);
    st(data, i, v);
    return v;
  }
};

template <class T, class D = T>
struct MomentumOp {
  using elem = T;
  T* data; T* m; const D* delta; T mu;
  template <class V, bool KEEP = false>
  __device__ __forceinline__ V step_at(int64_t i, V g) const {
    V d = ld_shard<V, KEEP>(data, i);
    // explicit fma, so that every instantiation rounds alike: left to
    // contract on its own, the compiler fused mu*m + (1-mu)*delta in the
    // float4 bodies and the fused tail but not in the plain scalar tail
    V mm = __builtin_elementwise_fma((V)mu, ld<V>(m, i), ((T)1 - mu) * g);
    st(m, i, mm);
    d -= mm;
    st(data, i, d);
    return d;
  }
  template <class V> __device__ __forceinline__ V step(int64_t i) const {
    return step_at<V, true>(i, ld<V>(delta, i));
  }
};

template <class T, class D = T>
struct AdagradOp {
  using elem = T;
  T* data; T* gsq; const D* delta; T inv_lr, rho, eps;
  template <class V> __device__ __forceinline__ V step(int64_t i) const {
    V d = ld_shard<V, true>(data, i), G = ld<V>(gsq, i);
    V g = ld<V>(delta, i) * inv_lr;
    G += g * g;
    // double keeps the exact divide; fp32 uses the hardware rsq
    if constexpr (std::is_same<T, double>::value) d -= rho * g / sqrt(G + eps);
    else d -= rho * g * rsq(G + eps);
    st(gsq, i, G);
    st(data, i, d);
    return d;
  }
};

// DC-ASGD updaters ("dcasgd"/"dcasgda", selected at reference
// updater.cpp:51-54 from a submodule ABSENT from the snapshot
// (.gitmodules:1-3, empty dir) — math reconstructed from the DC-ASGD
// paper (Zheng et al., "Asynchronous SGD with Delay Compensation",
// ICML 2017): the server compensates a delayed gradient g with a
// diagonal Hessian approximation g*g against the backup weights the
// worker pulled:
//   w    -= lr * (g + lambda * g*g * (w - bak))
//   bak   = w            (per-worker backup, updated after the step)
// Adaptive variant keeps a mean-square m = rho*m + (1-rho)*g*g and uses
// lambda / sqrt(m + eps) as the compensation coefficient.
template <class D = float>
struct DcasgdOp {
  using elem = float;
  float* data; float* bak; const D* delta; float lr, lambda;
  template <class V, bool KEEP = false>
  __device__ __forceinline__ V step_at(int64_t i, V g) const {
    V w = ld_shard<V, KEEP>(data, i), b = ld<V>(bak, i);
    w -= lr * (g + lambda * g * g * (w - b));
    st(data, i, w);
    st(bak, i, w);
    return w;
  }
  template <class V> __device__ __forceinline__ V step(int64_t i) const {
    return step_at<V, true>(i, ld<V>(delta, i));
  }
};

template <class D = float>
struct DcasgdaOp {
  using elem = float;
  float* data; float* bak; float* msq; const D* delta;
  float lr, lambda, rho, eps;
  template <class V, bool KEEP = false>
  __device__ __forceinline__ V step_at(int64_t i, V g) const {
    V w = ld_shard<V, KEEP>(data, i), b = ld<V>(bak, i);
    V m = rho * ld<V>(msq, i) + (1.0f - rho) * g * g;
    st(msq, i, m);
    V lam = lambda * rsq(m + eps);
    w -= lr * (g + lam * g * g * (w - b));
    st(data, i, w);
    st(bak, i, w);
    return w;
  }
  template <class V> __device__ __forceinline__ V step(int64_t i) const {
    return step_at<V, true>(i, ld<V>(delta, i));
  }
};

// Adam / AdamW ("adam"; not in the reference's set, semantics as
// torch.optim.Adam/AdamW with amsgrad off, SparseAdam for keyed batches):
//   w  = w * decay                         decay = 1 - lr*wd (1 is plain Adam)
//   m  = b1*m + (1-b1)*g
//   v  = b2*v + (1-b2)*g*g
//   w -= alpha * m / (sqrt(v) * rbc2 + eps)
// alpha = lr / (1 - b1^t) and rbc2 = 1 / sqrt(1 - b2^t) are the bias
// corrections for the shard's update count t; the host computes them, and
// decay, in double, so the kernel keeps no step state. One pass at
// 28 B/element (fp32): read w, m, v, g; write w, m, v. The pass is
// memory-bound, so sqrt and the divide are the correctly rounded ones (not
// the rsq helper). Every multiply-add that could contract is an explicit
// fma, as in MomentumOp: the v4f body, the scalar tail and k_row_update
// must round alike.
template <class T, class D = T>
struct AdamOp {
  using elem = T;
  T* data; T* m; T* v; const D* delta;
  T b1, omb1, b2, omb2, alpha, rbc2, decay, eps;
  template <class V, bool KEEP = false>
  __device__ __forceinline__ V step_at(int64_t i, V g) const {
    V w = ld_shard<V, KEEP>(data, i), mm = ld<V>(m, i), vv = ld<V>(v, i);
    mm = __builtin_elementwise_fma((V)b1, mm, omb1 * g);
    vv = __builtin_elementwise_fma((V)b2, vv, omb2 * g * g);
    V den = __builtin_elementwise_fma(__builtin_elementwise_sqrt(vv), (V)rbc2,
                                      (V)eps);
    w = __builtin_elementwise_fma((V)(-alpha), mm / den, w * decay);
    st(m, i, mm);
    st(v, i, vv);
    st(data, i, w);
    return w;
  }
  template <class V> __device__ __forceinline__ V step(int64_t i) const {
    return step_at<V, true>(i, ld<V>(delta, i));
  }
};

// Adam's scalars arrive in double (the host's bias corrections and decay
// factor) and are rounded to the table's type once, here.
template <class T, class D>
static AdamOp<T, D> adam_op(T* data, T* m, T* v, const D* delta, double b1,
                            double b2, double step, double rbc2, double decay,
                            double eps) {
  return AdamOp<T, D>{data, m, v, delta, (T)b1, (T)(1.0 - b1), (T)b2,
                      (T)(1.0 - b2), (T)step, (T)rbc2, (T)decay, (T)eps};
}

// K7 Access / shard copy-out: non-temporal streaming copy; O = bf16 narrows
// the shard into a bf16 Get buffer.
template <class O = float>
struct CopyOp {
  using elem = float;
  O* dst; const float* src;
  template <class V> __device__ __forceinline__ V step(int64_t i) const {
    V v = ld<V>(src, i);
    st(dst, i, v);
    return v;
  }
};

// The one elementwise kernel: grid-stride over V-elements [start, n).
// COPY is the fused Add+Get (single-rank fast path): an Add immediately
// followed by a whole-table Get re-reads the shard the updater just
// wrote. Streaming the updated weights to the Get buffer in the same pass
// saves that re-read — 2.0 GB instead of 2.5 GB per Add+Get step on the
// 1e6x128 headline config (observable semantics identical: shard updated
// AND out filled with the updated values).
// `out` is the Get buffer, an array of O (the shard's type, or bf16) that
// st views as V like the op's own arrays.
//
// `rev` (body launches only: start == 0, block a multiple of WAVE) makes
// the pass descend: wave w of the grid-stride order takes the w-th 64
// V-elements from the top, lanes still ascending inside them, so a wave
// keeps its one contiguous request per access. Element j is computed from
// element j of every array either way; only the order in which the
// elements are visited changes. The launchers alternate it from one
// whole-shard pass to the next (see the SWEEP note at launch_elem), so the
// lines a pass touched last are the ones the next pass touches first,
// while the Infinity Cache still holds them.
template <class Op, class V, bool COPY, class O>
__global__ void k_elem(Op op, O* __restrict__ out, int64_t start, int64_t n,
                       int rev) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  // whole waves mirror: the loop covers n rounded up to WAVE, and an index
  // past n (the ragged wave) is skipped
  int64_t n_pad = (n + (WAVE - 1)) & ~(int64_t)(WAVE - 1);
  for (int64_t i = start + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < n_pad; i += stride) {
    int64_t lane = threadIdx.x & (WAVE - 1);
    int64_t j = rev ? n_pad - WAVE - i + 2 * lane : i;
    if (j < n) {
      V v = op.template step<V>(j);
      if (COPY) st(out, j, v);
    }
  }
}

// SWEEP: `rev` is the direction of the body launch (start == 0) of every
// path below; the n%4 tail (one wave) ignores it. The caller alternates it
// from one pass over the same arrays to the next (Updater._sweep). With
// the shard loaded plainly (ld_shard) the last ~128 MiB of the shard that
// pass k touched are read from the Infinity Cache by pass k+1 and
// overwritten there before their write-back: 0.361 -> 0.292 ms per
// fused sgd pass at 1e6x128 in the probe, against no change at all while
// every access is non-temporal (profiles/sweep_direction.md).
//
// fp32: float4 body over n/4 vectors with the given grid cap and block,
// then one wave over the n%4 scalar tail. Other types, and fp32 with
// vec = false (a bf16 pointer that is not 8-byte aligned): scalar
// grid-stride.
template <bool COPY, class Op, class O>
static void launch_elem(const Op& op, O* out, int64_t n, int cap, int block,
                        hipStream_t s, bool vec = true, int rev = 0) {
  using T = typename Op::elem;
  if constexpr (std::is_same<T, float>::value) {
    if (vec) {
      int64_t n4 = n / 4;
      if (n4) k_elem<Op, v4f, COPY><<<grid_for_cap(n4, cap, block), block, 0,
                                      s>>>(op, out, 0, n4, rev);
      if (n > n4 * 4) k_elem<Op, float, COPY><<<1, 64, 0, s>>>(op, out,
                                                               n4 * 4, n, 0);
      return;
    }
  }
  if (n > 0)
    k_elem<Op, T, COPY><<<grid_for_cap(n, cap, block), block, 0, s>>>(
        op, out, 0, n, rev);
}

// fp32 updater launch: a non-null `out` selects the fused Add+Get form.
// Both forms run BLOCK threads x `cap` blocks (see the note at the
// COPY_BLOCK define); the bf16 forms keep the geometry of their fp32
// siblings.
template <class Op, class O>
static void launch_update(const Op& op, O* out, int64_t n, int cap,
                          hipStream_t s, int rev) {
  bool vec = vec_ok(op.delta) && vec_ok(out);
  if (out) launch_elem<true>(op, out, n, cap, BLOCK, s, vec, rev);
  else launch_elem<false>(op, (float*)nullptr, n, cap, BLOCK, s, vec, rev);
}

extern "C" {

// The fp32 launchers take the delta and the Get buffer as void* plus the
// WIRE_* bits that say which of the two holds bf16.
void mv_launch_copy(void* dst, const float* src, int wire, int64_t n,
                    hipStream_t s) {
  with_wire(wire, nullptr, dst, [&](auto*, auto* o) {
    launch_elem<false>(CopyOp<ELEM_OF(o)>{o, src}, (float*)nullptr, n,
                       ELEM_GRID, BLOCK, s, vec_ok(o));
  });
}

void mv_launch_add(float* data, const void* delta, int wire, int64_t n,
                   hipStream_t s, int rev) {
  with_wire(wire, delta, nullptr, [&](auto* d, auto*) {
    launch_elem<false>(AddOp<float, ELEM_OF(d)>{data, d}, (float*)nullptr, n,
                       UPD_GRID, BLOCK, s, vec_ok(d), rev);
  });
}
void mv_launch_add_f64(double* d, const double* x, int64_t n, hipStream_t s,
                       int rev) {
  launch_elem<false>(AddOp<double>{d, x}, (double*)nullptr, n, ELEM_GRID,
                     BLOCK, s, true, rev);
}
void mv_launch_add_i32(int32_t* d, const int32_t* x, int64_t n, hipStream_t s,
                       int rev) {
  launch_elem<false>(AddOp<int32_t>{d, x}, (int32_t*)nullptr, n, ELEM_GRID,
                     BLOCK, s, true, rev);
}
void mv_launch_add_i64(int64_t* d, const int64_t* x, int64_t n, hipStream_t s,
                       int rev) {
  launch_elem<false>(AddOp<int64_t>{d, x}, (int64_t*)nullptr, n, ELEM_GRID,
                     BLOCK, s, true, rev);
}

void mv_launch_sgd(float* data, const void* delta, void* out, int wire,
                   float sign, int64_t n, hipStream_t s, int rev) {
  with_wire(wire, delta, out, [&](auto* d, auto* o) {
    launch_update(SgdOp<float, ELEM_OF(d)>{data, d, sign}, o, n, UPD_GRID, s,
                  rev);
  });
}
void mv_launch_sgd_f64(double* d, const double* x, double* out, double sign,
                       int64_t n, hipStream_t s, int rev) {
  SgdOp<double> op{d, x, sign};
  if (out) launch_elem<true>(op, out, n, STATE_GRID, BLOCK, s, true, rev);
  else launch_elem<false>(op, out, n, ELEM_GRID, BLOCK, s, true, rev);
}

void mv_launch_momentum(float* data, float* m, const void* delta, void* out,
                        int wire, float mu, int64_t n, hipStream_t s, int rev) {
  with_wire(wire, delta, out, [&](auto* d, auto* o) {
    launch_update(MomentumOp<float, ELEM_OF(d)>{data, m, d, mu}, o, n,
                  STATE_GRID, s, rev);
  });
}
void mv_launch_momentum_f64(double* d, double* m, const double* x, double mu,
                            int64_t n, hipStream_t s, int rev) {
  launch_elem<false>(MomentumOp<double>{d, m, x, mu}, (double*)nullptr, n,
                     STATE_GRID, BLOCK, s, true, rev);
}

void mv_launch_adagrad(float* data, float* gsq, const void* delta, void* out,
                       int wire, float lr, float rho, float eps, int64_t n,
                       hipStream_t s, int rev) {
  with_wire(wire, delta, out, [&](auto* d, auto* o) {
    launch_update(AdagradOp<float, ELEM_OF(d)>{data, gsq, d, 1.0f / lr, rho,
                                               eps},
                  o, n, STATE_GRID, s, rev);
  });
}
void mv_launch_adagrad_f64(double* d, double* g, const double* x, double lr,
                           double rho, double eps, int64_t n, hipStream_t s,
                           int rev) {
  launch_elem<false>(AdagradOp<double>{d, g, x, 1.0 / lr, rho, eps},
                     (double*)nullptr, n, STATE_GRID, BLOCK, s, true, rev);
}

void mv_launch_dcasgd(float* data, float* bak, const void* delta, void* out,
                      int wire, float lr, float lambda, int64_t n,
                      hipStream_t s, int rev) {
  with_wire(wire, delta, out, [&](auto* d, auto* o) {
    launch_update(DcasgdOp<ELEM_OF(d)>{data, bak, d, lr, lambda}, o, n,
                  STATE_GRID, s, rev);
  });
}

void mv_launch_dcasgda(float* data, float* bak, float* msq, const void* delta,
                       void* out, int wire, float lr, float lambda, float rho,
                       float eps, int64_t n, hipStream_t s, int rev) {
  with_wire(wire, delta, out, [&](auto* d, auto* o) {
    launch_update(DcasgdaOp<ELEM_OF(d)>{data, bak, msq, d, lr, lambda, rho,
                                        eps},
                  o, n, STATE_GRID, s, rev);
  });
}

// Geometry is the other stateful updaters' STATE_GRID: no grid sweep has
// been run for a 4-read/3-write stream.
void mv_launch_adam(float* data, float* m, float* v, const void* delta,
                    void* out, int wire, double b1, double b2, double step,
                    double rbc2, double decay, double eps, int64_t n,
                    hipStream_t s, int rev) {
  with_wire(wire, delta, out, [&](auto* d, auto* o) {
    launch_update(adam_op(data, m, v, d, b1, b2, step, rbc2, decay, eps), o,
                  n, STATE_GRID, s, rev);
  });
}
void mv_launch_adam_f64(double* d, double* m, double* v, const double* x,
                        double b1, double b2, double step, double rbc2,
                        double decay, double eps, int64_t n, hipStream_t s,
                        int rev) {
  launch_elem<false>(adam_op(d, m, v, x, b1, b2, step, rbc2, decay, eps),
                     (double*)nullptr, n, STATE_GRID, BLOCK, s, true, rev);
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Row-keyed gather/scatter (K5/K6): shard is [local_rows, cols] row-major,
// rows[] are LOCAL row indices. Thread-per-element over (nrows * cols):
// adjacent lanes hit adjacent columns -> fully coalesced on both sides of
// the gather; the scatter uses device-scope atomicAdd so duplicate rows
// (the same row touched by several workers in one exchange) accumulate
// correctly.
//
// Idx is the loop-index type. A 64-bit divide is ~40 cycles per element
// and these kernels run one divide per 4 B moved, so the launchers pick
// Idx = uint32_t whenever the element count fits (all real pulls and
// pushes do) and int64_t otherwise. Only the (i -> r, c) math narrows —
// the shard offset stays 64-bit (1e9-row tables).
//
// ATOMIC = false are the unique-rows forms: when the caller guarantees no
// duplicate row ids (e.g. a sorted-unique union pushed from ONE rank) the
// atomics are unnecessary — plain read-modify-write is substantially
// faster for scattered few-column rows.
// ---------------------------------------------------------------------------

// V = float, float2 or float4 column groups; total and cols count V's. O is
// out's element type: float, or bf16 (each group narrowed as it is stored).
template <class V, class O, class Idx>
__global__ void k_row_gather(O* __restrict__ out, const V* __restrict__ shard,
                             const int64_t* __restrict__ rows,
                             Idx total, Idx cols) {
  Idx stride = (Idx)gridDim.x * blockDim.x;
  for (Idx i = (Idx)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    Idx r = i / cols, c = i - r * cols;
    V v = shard[rows[r] * (int64_t)cols + c];
    if constexpr (std::is_same<O, bf16>::value) st(out, i, v);
    else ((V*)out)[i] = v;
  }
}

// D is vals' element type in the three keyed update kernels below: float,
// or bf16 (widened per element; sums and atomics stay fp32).
template <class D, class Idx, bool ATOMIC>
__global__ void k_row_scatter_add(float* __restrict__ shard,
                                  const D* __restrict__ vals,
                                  const int64_t* __restrict__ rows,
                                  float sign, Idx total, Idx cols) {
  Idx stride = (Idx)gridDim.x * blockDim.x;
  for (Idx i = (Idx)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    Idx r = i / cols, c = i - r * cols;
    int64_t k = rows[r] * (int64_t)cols + c;
    float x = ld<float>(vals, i);
    if (ATOMIC) atomicAdd(&shard[k], sign * x);
    else shard[k] += sign * x;
  }
}

// Keyed AdaGrad scatter-update (K15 + K4 keyed form): for each incoming
// (row, value) pair apply the adagrad step to the owned shard row. Used by
// the LogisticRegression sparse path (BASELINE config: 1e9 sparse
// features, AdaGrad updater). Duplicate rows race benignly (hogwild):
// G accumulates via atomicAdd; the weight step uses the post-add G.
template <class D, class Idx, bool ATOMIC>
__global__ void k_row_scatter_adagrad(float* __restrict__ shard,
                                      float* __restrict__ gsq,
                                      const D* __restrict__ vals,
                                      const int64_t* __restrict__ rows,
                                      float inv_lr, float rho, float eps,
                                      Idx total, Idx cols) {
  Idx stride = (Idx)gridDim.x * blockDim.x;
  for (Idx i = (Idx)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    Idx r = i / cols, c = i - r * cols;
    int64_t k = rows[r] * (int64_t)cols + c;
    float g = ld<float>(vals, i) * inv_lr;
    if (g != 0.0f) {
      float G;
      if (ATOMIC) G = atomicAdd(&gsq[k], g * g) + g * g;
      else { G = gsq[k] + g * g; gsq[k] = G; }
      float dw = -rho * g * rsq(G + eps);
      if (ATOMIC) atomicAdd(&shard[k], dw);
      else shard[k] += dw;
    }
  }
}

// Keyed stateful update (momentum, dcasgd, dcasgda, adam; the per-row
// updater_->Update(...) of matrix_table.cpp:403-412): value rows that carry
// the same row id are summed in fp32 in list order, then the updater steps
// ONCE per distinct row on that row's weights and state. Rows not listed
// are not touched.
//
// rows[n] holds local row ids with equal ids adjacent (no other order
// needed); perm[j], when perm is non-null, is the row of vals that belongs
// to rows[j], so a caller that sorted the ids need not reorder the payload.
// Work item (j, c) = list position j, column-vector c, as in the kernels
// above. An item whose id equals its predecessor's does nothing; a head
// item walks its run of equal ids, sums vals[perm[k]][c] and hands the sum
// to Op::step_at. Fixed summation order, no atomics, no LDS and no segment
// table, so the result is reproducible and the host never syncs to learn
// the number of distinct rows.
//
// Known limit: one thread group sums all occurrences of a row serially, so
// a row listed thousands of times in one batch stretches the launch to the
// length of that run. Splitting long runs is not done here.
template <class Op, class V, class Idx, class D>
__global__ void k_row_update(Op op, const D* __restrict__ vals,
                             const int64_t* __restrict__ rows,
                             const int64_t* __restrict__ perm, int64_t n,
                             Idx total, Idx cols) {
  Idx stride = (Idx)gridDim.x * blockDim.x;
  for (Idx i = (Idx)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    Idx j = i / cols, c = i - j * cols;
    int64_t r = rows[j];
    if (j > 0 && rows[j - 1] == r) continue;
    int64_t k = j;
    V sum = ld<V>(vals, (perm ? perm[k] : k) * (int64_t)cols + c);
    for (++k; k < n && rows[k] == r; ++k)
      sum += ld<V>(vals, (perm ? perm[k] : k) * (int64_t)cols + c);
    op.template step_at<V>(r * (int64_t)cols + c, sum);
  }
}

static inline bool aligned16(const void* p) {
  return ((uintptr_t)p & 15) == 0;
}
// what V = v4f asks of vals: 16 bytes for fp32, 8 for bf16
static inline bool vals_vec_ok(const float* p) { return aligned16(p); }
static inline bool vals_vec_ok(const bf16* p) { return vec_ok(p); }

// `vec` (decided by the caller from cols % 4 and the alignment of every
// pointer the op and the kernel touch) selects V = v4f. Geometry is
// the other row kernels' BLOCK x grid_for(total); no grid sweep has been
// run for this shape. The 32-bit index form also needs room for the last
// grid stride, so that i += stride cannot wrap.
template <class Op, class D>
static void launch_row_update(const Op& op, bool vec, const D* vals,
                              const int64_t* rows, const int64_t* perm,
                              int64_t n, int64_t cols, hipStream_t s) {
  if (!n || !cols) return;
  vec = vec && cols % 4 == 0 && vals_vec_ok(vals);
  int64_t vcols = vec ? cols / 4 : cols, total = n * vcols;
  int grid = grid_for(total);
  bool narrow = total <= (int64_t)UINT32_MAX - (int64_t)MAX_GRID * BLOCK;
  if (vec && narrow)
    k_row_update<Op, v4f, uint32_t, D><<<grid, BLOCK, 0, s>>>(
        op, vals, rows, perm, n, (uint32_t)total, (uint32_t)vcols);
  else if (vec)
    k_row_update<Op, v4f, int64_t, D><<<grid, BLOCK, 0, s>>>(
        op, vals, rows, perm, n, total, vcols);
  else if (narrow)
    k_row_update<Op, float, uint32_t, D><<<grid, BLOCK, 0, s>>>(
        op, vals, rows, perm, n, (uint32_t)total, (uint32_t)vcols);
  else
    k_row_update<Op, float, int64_t, D><<<grid, BLOCK, 0, s>>>(
        op, vals, rows, perm, n, total, vcols);
}

// Column groups of 4, 2 or 1 by cols; a bf16 out also needs the group's
// store alignment (8 or 4 bytes), an fp32 out is a 16-byte torch allocation.
template <class O>
static void launch_row_gather(O* out, const float* shard, const int64_t* rows,
                              int64_t nrows, int64_t cols, hipStream_t s) {
  if (!nrows || !cols) return;
  int64_t total = nrows * cols;
  constexpr bool narrow_out = std::is_same<O, bf16>::value;
  bool g4 = cols % 4 == 0 && (!narrow_out || ((uintptr_t)out & 7) == 0);
  bool g2 = cols % 2 == 0 && (!narrow_out || ((uintptr_t)out & 3) == 0);
  if (g4 && total / 4 <= UINT32_MAX) {
    k_row_gather<float4, O, uint32_t><<<grid_for(total / 4), BLOCK, 0, s>>>(
        out, (const float4*)shard, rows, (uint32_t)(total / 4),
        (uint32_t)(cols / 4));
  } else if (g4) {
    k_row_gather<float4, O, int64_t><<<grid_for(total / 4), BLOCK, 0, s>>>(
        out, (const float4*)shard, rows, total / 4, cols / 4);
  } else if (g2 && total / 2 <= UINT32_MAX) {
    k_row_gather<float2, O, uint32_t><<<grid_for(total / 2), BLOCK, 0, s>>>(
        out, (const float2*)shard, rows, (uint32_t)(total / 2),
        (uint32_t)(cols / 2));
  } else if (total <= UINT32_MAX) {
    k_row_gather<float, O, uint32_t><<<grid_for(total), BLOCK, 0, s>>>(
        out, shard, rows, (uint32_t)total, (uint32_t)cols);
  } else {
    k_row_gather<float, O, int64_t><<<grid_for(total), BLOCK, 0, s>>>(
        out, shard, rows, total, cols);
  }
}

template <class D>
static void launch_row_scatter_add(float* shard, const D* vals,
                                   const int64_t* rows, float sign,
                                   int64_t nrows, int64_t cols,
                                   int assume_unique, hipStream_t s) {
  if (!nrows || !cols) return;
  int64_t total = nrows * cols;
  int grid = grid_for(total);
  if (total <= UINT32_MAX) {
    uint32_t t = (uint32_t)total, c = (uint32_t)cols;
    if (assume_unique)
      k_row_scatter_add<D, uint32_t, false><<<grid, BLOCK, 0, s>>>(
          shard, vals, rows, sign, t, c);
    else
      k_row_scatter_add<D, uint32_t, true><<<grid, BLOCK, 0, s>>>(
          shard, vals, rows, sign, t, c);
  } else if (assume_unique) {
    k_row_scatter_add<D, int64_t, false><<<grid, BLOCK, 0, s>>>(
        shard, vals, rows, sign, total, cols);
  } else {
    k_row_scatter_add<D, int64_t, true><<<grid, BLOCK, 0, s>>>(
        shard, vals, rows, sign, total, cols);
  }
}

template <class D>
static void launch_row_scatter_adagrad(
    float* shard, float* gsq, const D* vals, const int64_t* rows,
    float lr, float rho, float eps, int64_t nrows, int64_t cols,
    int assume_unique, hipStream_t s) {
  if (!nrows || !cols) return;
  int64_t total = nrows * cols;
  int grid = grid_for(total);
  float inv_lr = 1.0f / lr;
  if (total <= UINT32_MAX) {
    uint32_t t = (uint32_t)total, c = (uint32_t)cols;
    if (assume_unique)
      k_row_scatter_adagrad<D, uint32_t, false><<<grid, BLOCK, 0, s>>>(
          shard, gsq, vals, rows, inv_lr, rho, eps, t, c);
    else
      k_row_scatter_adagrad<D, uint32_t, true><<<grid, BLOCK, 0, s>>>(
          shard, gsq, vals, rows, inv_lr, rho, eps, t, c);
  } else if (assume_unique) {
    k_row_scatter_adagrad<D, int64_t, false><<<grid, BLOCK, 0, s>>>(
        shard, gsq, vals, rows, inv_lr, rho, eps, total, cols);
  } else {
    k_row_scatter_adagrad<D, int64_t, true><<<grid, BLOCK, 0, s>>>(
        shard, gsq, vals, rows, inv_lr, rho, eps, total, cols);
  }
}

extern "C" {

// In the keyed launchers `vals` (and the gather's `out`) is void* plus the
// WIRE_* bit that says whether it holds bf16, as in the elementwise ones.
void mv_launch_row_momentum(float* shard, float* m, const void* vals, int wire,
                            const int64_t* rows, const int64_t* perm,
                            float mu, int64_t nrows, int64_t cols,
                            hipStream_t s) {
  bool vec = aligned16(shard) && aligned16(m);
  with_wire(wire, vals, nullptr, [&](auto* x, auto*) {
    launch_row_update(MomentumOp<float>{shard, m, nullptr, mu}, vec, x, rows,
                      perm, nrows, cols, s);
  });
}

void mv_launch_row_dcasgd(float* shard, float* bak, const void* vals, int wire,
                          const int64_t* rows, const int64_t* perm, float lr,
                          float lambda, int64_t nrows, int64_t cols,
                          hipStream_t s) {
  bool vec = aligned16(shard) && aligned16(bak);
  with_wire(wire, vals, nullptr, [&](auto* x, auto*) {
    launch_row_update(DcasgdOp<float>{shard, bak, nullptr, lr, lambda}, vec,
                      x, rows, perm, nrows, cols, s);
  });
}

void mv_launch_row_dcasgda(float* shard, float* bak, float* msq,
                           const void* vals, int wire, const int64_t* rows,
                           const int64_t* perm, float lr, float lambda,
                           float rho, float eps, int64_t nrows, int64_t cols,
                           hipStream_t s) {
  bool vec = aligned16(shard) && aligned16(bak) && aligned16(msq);
  with_wire(wire, vals, nullptr, [&](auto* x, auto*) {
    launch_row_update(DcasgdaOp<float>{shard, bak, msq, nullptr, lr, lambda,
                                       rho, eps},
                      vec, x, rows, perm, nrows, cols, s);
  });
}

void mv_launch_row_adam(float* shard, float* m, float* v, const void* vals,
                        int wire, const int64_t* rows, const int64_t* perm,
                        double b1, double b2, double step, double rbc2,
                        double decay, double eps, int64_t nrows, int64_t cols,
                        hipStream_t s) {
  bool vec = aligned16(shard) && aligned16(m) && aligned16(v);
  with_wire(wire, vals, nullptr, [&](auto* x, auto*) {
    launch_row_update(adam_op<float, float>(shard, m, v, nullptr, b1, b2,
                                            step, rbc2, decay, eps),
                      vec, x, rows, perm, nrows, cols, s);
  });
}

void mv_launch_row_gather(void* out, int wire, const float* shard,
                          const int64_t* rows, int64_t nrows, int64_t cols,
                          hipStream_t s) {
  with_wire(wire, nullptr, out, [&](auto*, auto* o) {
    launch_row_gather(o, shard, rows, nrows, cols, s);
  });
}

void mv_launch_row_scatter_add(float* shard, const void* vals, int wire,
                               const int64_t* rows, float sign,
                               int64_t nrows, int64_t cols,
                               int assume_unique, hipStream_t s) {
  with_wire(wire, vals, nullptr, [&](auto* x, auto*) {
    launch_row_scatter_add(shard, x, rows, sign, nrows, cols, assume_unique,
                           s);
  });
}

void mv_launch_row_scatter_adagrad(
    float* shard, float* gsq, const void* vals, int wire, const int64_t* rows,
    float lr, float rho, float eps, int64_t nrows, int64_t cols,
    int assume_unique, hipStream_t s) {
  with_wire(wire, vals, nullptr, [&](auto* x, auto*) {
    launch_row_scatter_adagrad(shard, gsq, x, rows, lr, rho, eps, nrows, cols,
                               assume_unique, s);
  });
}

}  // extern "C"

// ---------------------------------------------------------------------------
// 1-bit Add wire with error feedback (onebit_filter.py; Seide et al.,
// Interspeech 2014 — the scheme the reference's empty OneBitsFilter,
// quantization_util.h:160-161, was named for).
//
// A piece of n fp32 elements is coded in blocks of 1024, the last one maybe
// partial. Payload of nb = ceil(n/1024) blocks, 136*nb bytes, 8-byte aligned:
//   [0, 8*nb)       nb x (neg, pos) fp32: the mean of the block's values with
//                   bit 0 / bit 1 (0 for an empty group)
//   [8*nb, 136*nb)  nb x 16 little-endian 64-bit words; element i of the
//                   block is bit i%64 of word i/64, pad bits are 0
// Encode: v = r + d, bit = (v >= 0), r <- v - (bit ? pos : neg).
// One launch codes one piece (the tables launch once per server).
// ---------------------------------------------------------------------------

#define ONEBIT_BLOCK 1024

// One 256-thread workgroup per block. Thread t holds elements t, t+256,
// t+512, t+768 of the block in registers, so wave w's ballot in round j is
// exactly word 4*j + w, and every load and store is a coalesced 4-byte access
// (d and r are pieces of a larger tensor: only 4-byte alignment is assumed).
// All 64 lanes stay active through the ballots: past the end of a partial
// block a lane loads the block's last valid element (clamped index) and
// contributes bit 0, count 0 and sum +0. Counts are popcounts of the ballots,
// exact. The sums have one fixed order: a thread's four values in round
// order, then the xor butterfly across the wave, then waves 0..3 from LDS —
// the same input gives the same payload on every run. d and r are streamed
// once, so their accesses are non-temporal like the updaters' (measured at
// 128M elements: 0.24 ms against 0.26-0.28 ms with plain accesses).
__global__ __launch_bounds__(BLOCK) void k_onebit_encode(
    const float* __restrict__ d, float* __restrict__ r,
    uint8_t* __restrict__ payload, int64_t n, int64_t nb) {
  __shared__ float s_sum[2][BLOCK / WAVE];
  __shared__ int s_cnt[2][BLOCK / WAVE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t blk = blockIdx.x;
  const int64_t base = blk * ONEBIT_BLOCK;
  const int64_t left = n - base;
  const int valid = left < ONEBIT_BLOCK ? (int)left : ONEBIT_BLOCK;  // >= 1
  float v[4];
  unsigned long long word[4];
  float sum[2] = {0.f, 0.f};
  int cnt[2] = {0, 0};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int e = j * BLOCK + tid;
    bool ok = e < valid;
    int64_t at = base + (ok ? e : valid - 1);
    v[j] = __builtin_nontemporal_load(r + at) +
           __builtin_nontemporal_load(d + at);
    bool pos = ok && v[j] >= 0.f;
    bool neg = ok && !(v[j] >= 0.f);
    word[j] = __ballot(pos);
    cnt[1] += __popcll(word[j]);
    cnt[0] += __popcll(__ballot(neg));
    sum[1] += pos ? v[j] : 0.f;
    sum[0] += neg ? v[j] : 0.f;
  }
#pragma unroll
  for (int m = WAVE / 2; m; m >>= 1) {
    sum[0] += __shfl_xor(sum[0], m, WAVE);
    sum[1] += __shfl_xor(sum[1], m, WAVE);
  }
  if (lane == 0) {
    s_sum[0][wave] = sum[0]; s_sum[1][wave] = sum[1];
    s_cnt[0][wave] = cnt[0]; s_cnt[1][wave] = cnt[1];
  }
  __syncthreads();
  float scale[2];
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    float t = ((s_sum[g][0] + s_sum[g][1]) + s_sum[g][2]) + s_sum[g][3];
    int c = s_cnt[g][0] + s_cnt[g][1] + s_cnt[g][2] + s_cnt[g][3];
    scale[g] = c ? __fdiv_rn(t, (float)c) : 0.f;   // correctly rounded
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int e = j * BLOCK + tid;
    // the sign bit was taken from v itself, so recompute it the same way
    if (e < valid)
      __builtin_nontemporal_store(
          v[j] - (v[j] >= 0.f ? scale[1] : scale[0]), r + base + e);
  }
  if (tid == 0) {
    float* scales = (float*)payload + 2 * blk;
    scales[0] = scale[0];
    scales[1] = scale[1];
  }
  if (lane < 4) {
    unsigned long long w = lane == 0 ? word[0] : lane == 1 ? word[1]
                         : lane == 2 ? word[2] : word[3];
    unsigned long long* words =
        (unsigned long long*)(payload + 8 * nb) + blk * 16;
    words[lane * 4 + wave] = w;
  }
}

// out[i] = ((q_0 + q_1) + ...) + q_{P-1}, q_p = bit_p(i) ? pos_p : neg_p, for
// P payloads of the same piece laid `stride` bytes apart, in that order
// (source-rank order on the sync plane; P = 1 on the async plane). The sign
// bits of all blocks are one contiguous bit string, so element i is bit i%8
// of byte i/8 of the bits region. VEC: one item is 4 consecutive elements
// (one nibble, one non-temporal float4 store — 0.085 ms against 0.115 ms
// with a plain store at 128M elements; a group never straddles a block);
// otherwise one element. Items [start, end).
template <bool VEC>
__global__ void k_onebit_decode_sum(float* __restrict__ out,
                                    const uint8_t* __restrict__ payloads,
                                    int64_t stride, int P, int64_t nb,
                                    int64_t start, int64_t end) {
  int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t it = start + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       it < end; it += step) {
    int64_t i = VEC ? it * 4 : it;
    int64_t blk = i / ONEBIT_BLOCK;
    int sh = VEC ? (int)(i & 4) : (int)(i & 7);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < P; ++p) {
      const uint8_t* pl = payloads + p * stride;
      const float* sc = (const float*)pl + 2 * blk;
      float neg = sc[0], pos = sc[1];
      unsigned b = (unsigned)pl[8 * nb + (i >> 3)] >> sh;
#pragma unroll
      for (int k = 0; k < (VEC ? 4 : 1); ++k) {
        float q = (b >> k) & 1u ? pos : neg;
        acc[k] = p ? acc[k] + q : q;
      }
    }
    if (VEC) {
      v4f o = {acc[0], acc[1], acc[2], acc[3]};
      ntstore((v4f*)out + it, o);
    } else {
      out[it] = acc[0];
    }
  }
}

extern "C" {

// n >= 1; payload holds 136 * ceil(n/1024) bytes and is 8-byte aligned
void mv_launch_onebit_encode(const float* d, float* r, uint8_t* payload,
                             int64_t n, hipStream_t s) {
  int64_t nb = (n + ONEBIT_BLOCK - 1) / ONEBIT_BLOCK;
  k_onebit_encode<<<(unsigned)nb, BLOCK, 0, s>>>(d, r, payload, n, nb);
}

// float4 stores where `out` is 16-byte aligned (then one wave over the n%4
// tail), scalar stores otherwise
void mv_launch_onebit_decode_sum(float* out, const uint8_t* payloads, int P,
                                 int64_t n, hipStream_t s) {
  int64_t nb = (n + ONEBIT_BLOCK - 1) / ONEBIT_BLOCK;
  int64_t stride = 136 * nb;
  if (aligned16(out)) {
    int64_t n4 = n / 4;
    if (n4)
      k_onebit_decode_sum<true><<<grid_for(n4), BLOCK, 0, s>>>(
          out, payloads, stride, P, nb, 0, n4);
    if (n > n4 * 4)
      k_onebit_decode_sum<false><<<1, WAVE, 0, s>>>(out, payloads, stride, P,
                                                    nb, n4 * 4, n);
    return;
  }
  k_onebit_decode_sum<false><<<grid_for(n), BLOCK, 0, s>>>(
      out, payloads, stride, P, nb, 0, n);
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Fused word2vec training kernel (K9+K10+K11):
// the reference's FeedForward / BPOutputLayer / context-embedding update
// (Applications/WordEmbedding/src/wordembedding.cpp:57-166) fused into ONE
// kernel over a block of training groups.
//
// A group = one (input set, output set) sample: skip-gram has 1 input and
// 1+neg outputs (labels 1,0,..); CBOW has window inputs; hierarchical
// softmax passes labels = 1-code over the Huffman path nodes. The caller
// maps global word ids to block-local rows of the gathered in_emb/out_emb
// buffers (the PS "requested parameters" of communicator.cpp:117-155).
//
// Geometry: one 64-lane wave per group, grid-stride over groups; each lane
// owns columns lane, lane+64, ... (DPL = ceil(dim/64) registers). The dot
// product reduces across the wave with __shfl_xor. Row updates use
// device-scope atomicAdd: waves share hot vocabulary rows (the reference
// used unsynchronized hogwild OpenMP updates; atomics keep the sum exact).
// ADAGRAD variant implements the app-side per-element accumulator math of
// wordembedding.cpp:101-165 (G += g^2; w += g*lr0/rsqrt(G) when G>1e-10).
// ---------------------------------------------------------------------------

// Phase 1: h = mean of the group's input rows in_idx[ib..ie).
template <int DPL>
static __device__ __forceinline__ void w2v_hidden(
    float (&h)[DPL], const float* __restrict__ in_emb,
    const int64_t* __restrict__ in_idx, int ib, int ie, int dim, int lane) {
  for (int i = ib; i < ie; ++i) {
    const float* row = in_emb + in_idx[i] * dim;
    // clamped UNCONDITIONAL loads: a divergent `if (c < dim)` around
    // the load compiled to a branch + s_waitcnt vmcnt(0) PER DPL
    // GROUP (full-latency serial, the round-2 ladder disease).
    // min() keeps the read in-bounds; inactive lanes accumulate a
    // duplicate element that nothing reads (wv[d]=0 gates every use).
#pragma unroll
    for (int d = 0; d < DPL; ++d) {
      int c = lane + 64 * d;
      h[d] += row[c < dim ? c : dim - 1];
    }
  }
  if (ie - ib > 1) {
    float inv = 1.f / (float)(ie - ib);
#pragma unroll
    for (int d = 0; d < DPL; ++d) h[d] *= inv;
  }
}

// Phase 2: score output row `node` against h, step it towards `label`
// (NS: 1 / 0; HS: the caller passes 1-code) and accumulate the hidden
// error into err.
template <int DPL, bool ADAGRAD, bool ATOMIC>
static __device__ __forceinline__ void w2v_output(
    const float (&h)[DPL], float (&err)[DPL], float* __restrict__ out_emb,
    float* __restrict__ out_gsq, int64_t node, float label, float lr,
    int dim, int lane) {
  float* w = out_emb + node * dim;
  float wv[DPL];
  float f = 0.f;
  // unconditional clamped load + select (see w2v_hidden): wv[d] MUST be
  // 0 for inactive lanes (it feeds the wave-reduced dot), so the select
  // stays — but on the value, not the load
#pragma unroll
  for (int d = 0; d < DPL; ++d) {
    int c = lane + 64 * d;
    float x = w[c < dim ? c : dim - 1];
    wv[d] = (c < dim) ? x : 0.f;
    f += h[d] * wv[d];
  }
#pragma unroll
  for (int s = 32; s; s >>= 1) f += __shfl_xor(f, s, 64);
  f = 1.f / (1.f + expf(-f));
  float e = label - f;
#pragma unroll
  for (int d = 0; d < DPL; ++d) {
    int c = lane + 64 * d;
    if (c < dim) {
      err[d] += e * wv[d];  // hidden_err uses the PRE-update classifier
      if (ADAGRAD) {
        float gg = e * h[d];
        float* gq = out_gsq + node * dim + c;
        float G2;
        if (ATOMIC) G2 = atomicAdd(gq, gg * gg) + gg * gg;
        else { G2 = *gq + gg * gg; *gq = G2; }
        float dw = (G2 > 1e-10f) ? gg * lr * __frsqrt_rn(G2) : 0.f;
        if (ATOMIC) atomicAdd(&w[c], dw);
        else w[c] = wv[d] + dw;
      } else {
        if (ATOMIC) atomicAdd(&w[c], e * lr * h[d]);
        else w[c] = wv[d] + e * lr * h[d];
      }
    }
  }
}

// Phase 3: apply the accumulated hidden error to every input row.
template <int DPL, bool ADAGRAD, bool ATOMIC>
static __device__ __forceinline__ void w2v_writeback(
    const float (&err)[DPL], float* __restrict__ in_emb,
    float* __restrict__ in_gsq, const int64_t* __restrict__ in_idx,
    int ib, int ie, float lr, int dim, int lane) {
  for (int i = ib; i < ie; ++i) {
    float* row = in_emb + in_idx[i] * dim;
    if (!ADAGRAD && !ATOMIC) {
      // hogwild-default path: branch-free rmw — unconditional clamped
      // loads (issue back-to-back under one wait), guarded stores
      float cur[DPL];
#pragma unroll
      for (int d = 0; d < DPL; ++d) {
        int c = lane + 64 * d;
        cur[d] = row[c < dim ? c : dim - 1];
      }
#pragma unroll
      for (int d = 0; d < DPL; ++d) {
        int c = lane + 64 * d;
        if (c < dim) row[c] = cur[d] + lr * err[d];
      }
      continue;
    }
#pragma unroll
    for (int d = 0; d < DPL; ++d) {
      int c = lane + 64 * d;
      if (c < dim) {
        if (ADAGRAD) {
          float* gq = in_gsq + in_idx[i] * dim + c;
          float G2;
          if (ATOMIC) G2 = atomicAdd(gq, err[d] * err[d]) + err[d] * err[d];
          else { G2 = *gq + err[d] * err[d]; *gq = G2; }
          float dw = (G2 > 1e-10f) ? err[d] * lr * __frsqrt_rn(G2) : 0.f;
          if (ATOMIC) atomicAdd(&row[c], dw);
          else row[c] += dw;
        } else {
          if (ATOMIC) atomicAdd(&row[c], lr * err[d]);
          else row[c] += lr * err[d];
        }
      }
    }
  }
}

// General form: ragged out_idx/out_label lists per group.
template <int DPL, bool ADAGRAD, bool ATOMIC>
__global__ void k_w2v(float* __restrict__ in_emb, float* __restrict__ out_emb,
                      float* __restrict__ in_gsq, float* __restrict__ out_gsq,
                      const int64_t* __restrict__ in_idx,
                      const int* __restrict__ in_off,
                      const int64_t* __restrict__ out_idx,
                      const float* __restrict__ out_label,
                      const int* __restrict__ out_off,
                      float lr, int G, int dim) {
  int wid = (int)((blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6);
  int lane = threadIdx.x & 63;
  int nwaves = (int)((gridDim.x * (int64_t)blockDim.x) >> 6);
  for (int g = wid; g < G; g += nwaves) {
    float h[DPL], err[DPL];
#pragma unroll
    for (int d = 0; d < DPL; ++d) { h[d] = 0.f; err[d] = 0.f; }
    int ib = in_off[g], ie = in_off[g + 1];
    w2v_hidden<DPL>(h, in_emb, in_idx, ib, ie, dim, lane);
    int ob = out_off[g], oe = out_off[g + 1];
    for (int o = ob; o < oe; ++o)
      w2v_output<DPL, ADAGRAD, ATOMIC>(h, err, out_emb, out_gsq, out_idx[o],
                                       out_label[o], lr, dim, lane);
    w2v_writeback<DPL, ADAGRAD, ATOMIC>(err, in_emb, in_gsq, in_idx, ib, ie,
                                        lr, dim, lane);
  }
}

// Negative-sampling variant with IN-KERNEL negative generation: for
// NS-only training (no hierarchical softmax) the output list of group g
// is implicit — 1 positive (centers[g], label 1) + `neg` draws from the
// per-block pool with the reference's own LCG scheme
// (wordembedding.cpp:276-279: next_random = next_random*25214903917+11;
// index = (next_random >> 8) % pool_size; skip if == positive). This
// removes the host-side randint/gather/label/ragged-offset build and
// shrinks the per-group index traffic from (1+neg) ids to 1.
template <int DPL, bool ADAGRAD, bool ATOMIC>
__global__ void k_w2v_ns(float* __restrict__ in_emb, float* __restrict__ out_emb,
                         float* __restrict__ in_gsq, float* __restrict__ out_gsq,
                         const int64_t* __restrict__ in_idx,
                         const int* __restrict__ in_off,
                         const int64_t* __restrict__ centers,
                         const int64_t* __restrict__ pool, int64_t pool_n,
                         int neg, uint64_t seed,
                         float lr, int G, int dim) {
  int wid = (int)((blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6);
  int lane = threadIdx.x & 63;
  int nwaves = (int)((gridDim.x * (int64_t)blockDim.x) >> 6);
  for (int g = wid; g < G; g += nwaves) {
    float h[DPL], err[DPL];
#pragma unroll
    for (int d = 0; d < DPL; ++d) { h[d] = 0.f; err[d] = 0.f; }
    // in_off == nullptr: skip-gram (exactly one input per group) — the
    // offset loads vanish (probe V7: 5% over the ragged form)
    int ib = in_off ? in_off[g] : g, ie = in_off ? in_off[g + 1] : g + 1;
    w2v_hidden<DPL>(h, in_emb, in_idx, ib, ie, dim, lane);
    int64_t pos = centers[g];
    // per-group random stream (same recurrence as util.cpp:144)
    uint64_t next_random = seed + (uint64_t)g * 25214903917ull + 11ull;
    for (int o = 0; o <= neg; ++o) {
      int64_t node;
      float label;
      if (o == 0) {
        node = pos; label = 1.f;
      } else {
        next_random = next_random * 25214903917ull + 11ull;
        node = pool[(int64_t)((next_random >> 8) % (uint64_t)pool_n)];
        label = 0.f;
        if (node == pos) continue;  // wordembedding.cpp:279
      }
      w2v_output<DPL, ADAGRAD, ATOMIC>(h, err, out_emb, out_gsq, node, label,
                                       lr, dim, lane);
    }
    w2v_writeback<DPL, ADAGRAD, ATOMIC>(err, in_emb, in_gsq, in_idx, ib, ie,
                                        lr, dim, lane);
  }
}

// DPL register bucket for a row width: exact up to 8, then the next
// instantiated bucket (the kernels guard c < dim, so oversize DPL only
// costs idle iterations). Beyond 2048 columns the per-lane register
// arrays (3*DPL VGPRs) would spill; that returns a DPL with no
// instantiation, which the dispatch refuses LOUDLY instead of silently
// doing nothing.
static int w2v_dpl_bucket(int64_t dim) {
  int dpl = (int)((dim + 63) / 64);
  if (dpl > 8) dpl = (dpl <= 12) ? 12 : (dpl <= 16) ? 16
                   : (dpl <= 24) ? 24 : (dpl <= 32) ? 32 : dpl;
  return dpl;
}

// Launch KERNEL<DPL, ADAGRAD, ATOMIC> over G groups, one wave per group
// (4 waves per 256-thread block).
#define W2V_CASE(KERNEL, D, ...)                                             \
  case D:                                                                    \
    if (use_adagrad) {                                                       \
      if (use_atomic) KERNEL<D, true, true><<<grid, BLOCK, 0, s>>>(__VA_ARGS__); \
      else KERNEL<D, true, false><<<grid, BLOCK, 0, s>>>(__VA_ARGS__);       \
    } else {                                                                 \
      if (use_atomic) KERNEL<D, false, true><<<grid, BLOCK, 0, s>>>(__VA_ARGS__); \
      else KERNEL<D, false, false><<<grid, BLOCK, 0, s>>>(__VA_ARGS__);      \
    }                                                                        \
    break;
#define W2V_DISPATCH(KERNEL, ...)                                            \
  do {                                                                       \
    if (!G) return;                                                          \
    int grid = grid_for(G * 64);                                             \
    switch (w2v_dpl_bucket(dim)) {                                           \
      W2V_CASE(KERNEL, 1, __VA_ARGS__) W2V_CASE(KERNEL, 2, __VA_ARGS__)      \
      W2V_CASE(KERNEL, 3, __VA_ARGS__) W2V_CASE(KERNEL, 4, __VA_ARGS__)      \
      W2V_CASE(KERNEL, 5, __VA_ARGS__) W2V_CASE(KERNEL, 6, __VA_ARGS__)      \
      W2V_CASE(KERNEL, 7, __VA_ARGS__) W2V_CASE(KERNEL, 8, __VA_ARGS__)      \
      W2V_CASE(KERNEL, 12, __VA_ARGS__) W2V_CASE(KERNEL, 16, __VA_ARGS__)    \
      W2V_CASE(KERNEL, 24, __VA_ARGS__) W2V_CASE(KERNEL, 32, __VA_ARGS__)    \
      default:                                                               \
        fprintf(stderr, "%s: dim=%lld exceeds the 2048-column kernel "       \
                "limit\n", __func__, (long long)dim);                        \
        abort();                                                             \
    }                                                                        \
  } while (0)

// Hogwild (plain-store) row updates by default — the reference's own
// unsynchronized OpenMP trainers race identically (wordembedding.cpp
// trainers share rows with no locks); on MI355X plain stores measured
// 11x faster than per-element atomics (tools/probe_w2v.hip: 4.6 ms vs
// 52.8 ms per 2.1M-group launch). use_atomic=1 restores exact
// accumulation for strict tests.
extern "C" void mv_launch_w2v(float* in_emb, float* out_emb,
                              float* in_gsq, float* out_gsq,
                              const int64_t* in_idx, const int* in_off,
                              const int64_t* out_idx, const float* out_label,
                              const int* out_off, float lr, int64_t G,
                              int64_t dim, int use_adagrad, int use_atomic,
                              hipStream_t s) {
  W2V_DISPATCH(k_w2v, in_emb, out_emb, in_gsq, out_gsq, in_idx, in_off,
               out_idx, out_label, out_off, lr, (int)G, (int)dim);
}

extern "C" void mv_launch_w2v_ns(float* in_emb, float* out_emb,
                                 float* in_gsq, float* out_gsq,
                                 const int64_t* in_idx, const int* in_off,
                                 const int64_t* centers,
                                 const int64_t* pool, int64_t pool_n,
                                 int neg, uint64_t seed, float lr, int64_t G,
                                 int64_t dim, int use_adagrad, int use_atomic,
                                 hipStream_t s) {
  W2V_DISPATCH(k_w2v_ns, in_emb, out_emb, in_gsq, out_gsq, in_idx, in_off,
               centers, pool, pool_n, neg, seed, lr, (int)G, (int)dim);
}
#undef W2V_DISPATCH
#undef W2V_CASE

// ---------------------------------------------------------------------------
// Logistic regression: eight kernels, one 64-lane wave per sample in all of
// them, composed from the stages below. Each stage is written once; where
// a term differs between objectives the kernel passes it in as a functor.
// ---------------------------------------------------------------------------

// keeps every log of a loss finite
constexpr float LR_LOG_EPS = 1e-12f;

// Wave-per-sample geometry: this wave's index in the grid, the lane's in
// the wave, and the waves in the grid (the stride of the sample loop).
// The kernel passes its blockDim.x in: read in here it costs every kernel a
// vector load and a partial-block select in its prologue, which the
// compiler folds away only where a kernel body reads it itself.
struct Wave { int id, lane, n; };
static __device__ __forceinline__ Wave this_wave(unsigned block) {
  return {(int)((blockIdx.x * (int64_t)block + threadIdx.x) >> 6),
          (int)(threadIdx.x & 63), (int)((gridDim.x * (int64_t)block) >> 6)};
}

// butterfly reductions: the result lands on every lane
static __device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int sh = 32; sh; sh >>= 1) v += __shfl_xor(v, sh, 64);
  return v;
}
static __device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int sh = 32; sh; sh >>= 1) v = fmaxf(v, __shfl_xor(v, sh, 64));
  return v;
}
template <int K>
static __device__ __forceinline__ void wave_sum(float (&l)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) l[k] = wave_sum(l[k]);
}

// l[lane] for the lanes below KK, `fill` for the rest: lane k owns class k
// from here (the reduced logits are identical on all lanes). The unrolled
// select keeps l[] in registers (no dynamic indexing).
template <int K>
static __device__ __forceinline__ float lane_select(const float (&l)[K],
                                                    int lane, int KK,
                                                    float fill) {
  float mine = fill;
#pragma unroll
  for (int k = 0; k < K; ++k)
    if (k < KK && lane == k) mine = l[k];
  return mine;
}

// One feature of a sample's CSR walk: l[k] += v * term(row, k) for the KK
// classes, `row` being the feature's table row and v its value. The
// `k < KK` guards fold away where the kernel pins KK at compile time (see
// k_lr_softmax_fwd). The lane-strided loop around it stays in the two
// kernels: moved into a function with it (l by reference or returned by
// value) it was scheduled differently, 90 VGPRs for 61 in
// k_lr_softmax_fwd<32> and 97 for 86 in k_lr_ftrl_fwd<32>, an occupancy
// step each (profiles/lr_refactor.md).
template <int K, class Term>
static __device__ __forceinline__ void add_feature(float (&l)[K], float v,
                                                   const float* row, int KK,
                                                   Term term) {
#pragma unroll
  for (int k = 0; k < K; ++k)
    if (k < KK) l[k] += v * term(row, k);
}

// sample i's weight; 1 where the batch carries none
static __device__ __forceinline__ float weight_of(const float* wts, int i) {
  return wts ? wts[i] : 1.f;
}

// Softmax of sample i across the live lanes of a wave, lane k holding class
// k's logit in `mine` (dead lanes hold -1e30f). Writes this lane's
// (p_k - [k == y]) * wt to out[lane] and returns the sample's loss
// -log(p_y + eps) (SoftmaxObjective.loss) on every lane. Label and weight
// are read here, after the reductions: read before them they stay live
// across them (87 VGPRs for 61 in k_lr_softmax_fwd<32>).
static __device__ __forceinline__ float softmax_epilogue(
    float mine, bool live, int lane, int i, const float* labels,
    const float* wts, float* out) {
  float mx = wave_max(mine);
  float e = live ? expf(mine - mx) : 0.f;
  float se = wave_sum(e);
  float p = e / se;
  int y = (int)labels[i];
  float wt = weight_of(wts, i);
  if (live) out[lane] = (p - (lane == y)) * wt;
  float py = __shfl(p, y, 64);
  return -logf(py + LR_LOG_EPS);
}

// Sigmoid of one logit s of sample i against its target y: the label itself
// for a binary output (cls < 0), else [cls == label]. Writes (p - y) * wt to
// *err and returns the binary loss -(y log p + (1-y) log(1-p))
// (Objective.loss). Label and weight are read after p, as in
// softmax_epilogue.
static __device__ __forceinline__ float sigmoid_epilogue(
    float s, int cls, int i, const float* labels, const float* wts,
    float* err) {
  float p = 1.f / (1.f + expf(-s));
  float y = (cls < 0) ? labels[i] : (float)(cls == (int)labels[i]);
  float wt = weight_of(wts, i);
  *err = (p - y) * wt;
  return -(y * logf(p + LR_LOG_EPS) + (1.f - y) * logf(1.f - p + LR_LOG_EPS));
}

// g plus the regulariser's gradient at the weight *w: reg_type 0 none,
// 1 = l1 coef*sign(w), 2 = l2 coef*w. The weight is read only if needed.
static __device__ __forceinline__ float with_reg(float g, const float* w,
                                                 int reg_type, float coef) {
  if (reg_type == 1) {
    float wv = *w;
    g += coef * ((wv > 0.f) - (wv < 0.f));
  } else if (reg_type == 2) {
    g += coef * *w;
  }
  return g;
}

// f(j, k) over the flattened (feature, class) pairs of one sample: lane t
// handles pair t, t+64, ... -> consecutive lanes hit consecutive classes of
// the same table row (coalesced atomics).
template <class F>
static __device__ __forceinline__ void for_pairs(int jb, int je, int K,
                                                 int lane, F f) {
  // u32 pair math: nnz*K < 2^32 always (B*nnz is int32 CSR already);
  // a 64-bit div per pair was ~40 VALU cycles each
  uint32_t pairs = (uint32_t)(je - jb) * (uint32_t)K;
  for (uint32_t t = lane; t < pairs; t += 64) {
    uint32_t q = t / (uint32_t)K;
    f(jb + (int)q, (int)(t - q * (uint32_t)K));
  }
}

// Block mean-loss accumulate, in two halves around a kernel's sample loop:
// *loss_acc += inv_b * (the sum of every wave's lane-0 ll_sum). The barrier
// of the first half also publishes what the kernel wrote to LDS before it.
// Loss goes lane-private -> one LDS atomic per wave -> ONE global
// atomic per block: a naive per-sample atomicAdd on the single
// loss_acc cache line serialized 4096 waves and cost 54 us (measured,
// profiles/round2_dense_fused.md) — 13x the kernel's real work.
// (One function taking the loop as a lambda cost k_lr_dense_post 3 VGPRs
// and 0.3 us at K = 1, profiles/lr_refactor.md.)
static __device__ __forceinline__ float* block_loss_begin() {
  __shared__ float block_loss;
  if (threadIdx.x == 0) block_loss = 0.f;
  __syncthreads();
  return &block_loss;
}
static __device__ __forceinline__ void block_loss_end(float* block_loss,
                                                      float* loss_acc,
                                                      float inv_b, int lane,
                                                      float ll_sum) {
  if (lane == 0 && ll_sum != 0.f) atomicAdd(block_loss, ll_sum);
  __syncthreads();
  if (threadIdx.x == 0 && *block_loss != 0.f)
    atomicAdd(loss_acc, *block_loss * inv_b);
}

// f(kint<K>()) for a runtime K in [LO, HI], so that f can instantiate a
// kernel on the exact class count; false, and no call, for any other K.
template <int N> using kint = std::integral_constant<int, N>;
template <int LO, int HI, class F>
static bool with_exact_k(int64_t K, F f) {
  if constexpr (LO <= HI) {
    if (K == LO) {
      f(kint<LO>());
      return true;
    }
    return with_exact_k<LO + 1, HI>(K, f);
  }
  return false;
}

// ---------------------------------------------------------------------------
// Fused sparse logistic regression minibatch (K13/K14 fused): the
// reference's per-sample scalar loops (LogisticRegression
// objective/objective.cpp:63-188 sigmoid path + updater apply) as TWO
// kernels per minibatch instead of ~20 torch ops.
//
// Forward: one 64-lane wave per sample walks its CSR segment
// [ptr[i], ptr[i+1]), accumulates s = sum(vals_j * w[keys_j]), wave-
// reduces, then err[i] = (sigmoid(s) - y_i) * wt_i and the log loss.
// Scatter: same geometry; lanes apply w[keys_j] -= lr * (vals_j * err_i
// + reg(w)) with device atomics (duplicate keys accumulate, matching
// index_add semantics).
// ---------------------------------------------------------------------------

__global__ void k_lr_sigmoid_fwd(const float* __restrict__ w,
                                 const int64_t* __restrict__ keys,
                                 const float* __restrict__ vals,
                                 const int* __restrict__ ptr,
                                 const float* __restrict__ labels,
                                 const float* __restrict__ wts,
                                 float* __restrict__ err,
                                 float* __restrict__ loss, int B) {
  const Wave wv = this_wave(blockDim.x);
  for (int i = wv.id; i < B; i += wv.n) {
    int jb = ptr[i], je = ptr[i + 1];
    float s = 0.f;
    for (int j = jb + wv.lane; j < je; j += 64) s += vals[j] * w[keys[j]];
    s = wave_sum(s);
    if (wv.lane == 0)
      loss[i] = sigmoid_epilogue(s, -1, i, labels, wts, &err[i]);
  }
}

__global__ void k_lr_sigmoid_scatter(float* __restrict__ w,
                                     const int64_t* __restrict__ keys,
                                     const float* __restrict__ vals,
                                     const int* __restrict__ ptr,
                                     const float* __restrict__ err,
                                     float lr, int reg_type, float reg_coef,
                                     int B) {
  const Wave wv = this_wave(blockDim.x);
  for (int i = wv.id; i < B; i += wv.n) {
    int jb = ptr[i], je = ptr[i + 1];
    float e = err[i];
    for (int j = jb + wv.lane; j < je; j += 64) {
      float* wk = w + keys[j];
      atomicAdd(wk, -lr * with_reg(vals[j] * e, wk, reg_type, reg_coef));
    }
  }
}

extern "C" void mv_launch_lr_sigmoid_fwd(
    const float* w, const int64_t* keys, const float* vals, const int* ptr,
    const float* labels, const float* wts, float* err, float* loss,
    int64_t B, hipStream_t s) {
  if (!B) return;
  k_lr_sigmoid_fwd<<<grid_for(B * 64), BLOCK, 0, s>>>(w, keys, vals, ptr,
                                                      labels, wts, err, loss,
                                                      (int)B);
}

extern "C" void mv_launch_lr_sigmoid_scatter(
    float* w, const int64_t* keys, const float* vals, const int* ptr,
    const float* err, float lr, int reg_type, float reg_coef, int64_t B,
    hipStream_t s) {
  if (!B) return;
  k_lr_sigmoid_scatter<<<grid_for(B * 64), BLOCK, 0, s>>>(
      w, keys, vals, ptr, err, lr, reg_type, reg_coef, (int)B);
}

// ---------------------------------------------------------------------------
// Fused multiclass softmax minibatch (K13 softmax path,
// objective.cpp:193-230): one 64-lane wave per sample. Forward: each lane
// walks the sample's CSR features strided by 64, accumulating all K class
// logits in registers (K <= 64); per-class wave reduction via shfl_xor;
// lane k then owns class k for the softmax (max/sum reduced the same way)
// and writes err[i*K+k] = (p_k - [k==y]) * wt and lane 0 the NLL loss.
//
// MFMA verdict: this op is a gather-dominated GEMV batch —
// arithmetic intensity 2K FLOP per (4B value + K*4B gathered row) = 0.5
// FLOP/B at any K, ~150x below the f32-MFMA ridge (157 TF / 8 TB/s = 20
// FLOP/B); staging gathered rows through LDS to feed v_mfma_f32_16x16x4_f32
// adds LDS round-trips without reducing HBM bytes, so matrix cores cannot
// help. Measured confirmation in profiles/ (MemUnitBusy ~ 100%, VALU low).
// docs/ENGINEERING_NOTES.md carries the full argument.
// ---------------------------------------------------------------------------

// KKC != 0 pins the runtime class count at compile time: the `k < KK`
// guards in the unrolled row loop then constant-fold away.  With a
// runtime KK the compiler emits a PER-CLASS BRANCH LADDER with a full
// `s_waitcnt vmcnt(0)` after every gathered-row load — each feature's
// row read serializes at full memory latency (the same disease measured
// at 5x on k_lr_dense_fwd; see profiles/round2_dense_fused.md).  The
// launcher dispatches exact K for K <= 16, guarded buckets beyond.
template <int K, int KKC = 0>
__global__ void k_lr_softmax_fwd(const float* __restrict__ w,
                                 const int64_t* __restrict__ keys,
                                 const float* __restrict__ vals,
                                 const int* __restrict__ ptr,
                                 const float* __restrict__ labels,
                                 const float* __restrict__ wts,
                                 float* __restrict__ err,
                                 float* __restrict__ loss, int B, int KK) {
  if (KKC != 0) KK = KKC;
  const Wave wv = this_wave(blockDim.x);
  for (int i = wv.id; i < B; i += wv.n) {
    int jb = ptr[i], je = ptr[i + 1];
    float l[K] = {};
    for (int j = jb + wv.lane; j < je; j += 64)
      add_feature(l, vals[j], w + keys[j] * KK, KK,
                  [](const float* row, int k) { return row[k]; });
    wave_sum(l);
    float ll = softmax_epilogue(lane_select(l, wv.lane, KK, -1e30f),
                                wv.lane < KK, wv.lane, i, labels, wts,
                                err + (int64_t)i * KK);
    if (wv.lane == 0) loss[i] = ll;
  }
}

__global__ void k_lr_softmax_scatter(float* __restrict__ w,
                                     const int64_t* __restrict__ keys,
                                     const float* __restrict__ vals,
                                     const int* __restrict__ ptr,
                                     const float* __restrict__ err,
                                     float lr, int reg_type, float reg_coef,
                                     int B, int K) {
  const Wave wv = this_wave(blockDim.x);
  for (int i = wv.id; i < B; i += wv.n) {
    const float* e = err + (int64_t)i * K;
    for_pairs(ptr[i], ptr[i + 1], K, wv.lane, [&](int j, int k) {
      float* wk = w + (keys[j] * K + k);
      atomicAdd(wk, -lr * with_reg(vals[j] * e[k], wk, reg_type, reg_coef));
    });
  }
}

extern "C" void mv_launch_lr_softmax_fwd(
    const float* w, const int64_t* keys, const float* vals, const int* ptr,
    const float* labels, const float* wts, float* err, float* loss,
    int64_t B, int64_t K, hipStream_t s) {
  if (!B) return;
  int grid = grid_for(B * 64);
  auto launch = [&](auto kb, auto kkc) {
    k_lr_softmax_fwd<decltype(kb)::value, decltype(kkc)::value>
        <<<grid, BLOCK, 0, s>>>(w, keys, vals, ptr, labels, wts, err, loss,
                                (int)B, (int)K);
  };
  if (with_exact_k<2, 16>(K, [&](auto k) { launch(k, k); })) return;
  if (K <= 32) launch(kint<32>(), kint<0>());
  else if (K <= 64) launch(kint<64>(), kint<0>());
  else __builtin_trap();  // K > 64: host refuses before launch
}

extern "C" void mv_launch_lr_softmax_scatter(
    float* w, const int64_t* keys, const float* vals, const int* ptr,
    const float* err, float lr, int reg_type, float reg_coef, int64_t B,
    int64_t K, hipStream_t s) {
  if (!B) return;
  k_lr_softmax_scatter<<<grid_for(B * 64), BLOCK, 0, s>>>(
      w, keys, vals, ptr, err, lr, reg_type, reg_coef, (int)B, (int)K);
}

// ---------------------------------------------------------------------------
// Fused FTRL minibatch (objective.cpp:250-345 + updater.cpp:79-101):
// state rows carry (z | n) interleaved as [row*2K + k] = z_k and
// [row*2K + K + k] = n_k, exactly the app's (z|n) column layout.
//
// Forward: wave per sample; each lane walks features strided, per class
// reconstructs w from (z, n) — w = (sign(z)*l1 - z) / ((beta+sqrt(n))/
// alpha + l2) when |z| > l1 else 0 — accumulates the K logits, wave-
// reduces, sigmoid -> err (FTRL is a sigmoid objective in the reference).
// Scatter: per (feature, class) pair, g = val*err; dz = (sqrt(n+g^2) -
// sqrt(n))/alpha * w - g; dn = -g^2; state -= (dz | dn) applied in place
// (the local chunk buffer; the push is pulled-local, server 'sgd'
// subtracts). Duplicate keys inside one minibatch race hogwild-style —
// the reference's async workers raced these identically across workers.
// ---------------------------------------------------------------------------

static __device__ __forceinline__ float ftrl_w(float z, float n,
                                               float alpha_inv, float beta,
                                               float l1, float l2) {
  float nz = fmaxf(n, 0.f);
  float sgn = (z > 0.f) - (z < 0.f);
  float w = (sgn * l1 - z) / ((beta + sqrtf(nz)) * alpha_inv + l2);
  return (fabsf(z) > l1) ? w : 0.f;
}

template <int K, int KKC = 0>
__global__ void k_lr_ftrl_fwd(const float* __restrict__ zn,
                              const int64_t* __restrict__ keys,
                              const float* __restrict__ vals,
                              const int* __restrict__ ptr,
                              const float* __restrict__ labels,
                              const float* __restrict__ wts,
                              float* __restrict__ err,
                              float* __restrict__ loss,
                              float alpha_inv, float beta, float l1,
                              float l2, int B, int KK) {
  if (KKC != 0) KK = KKC;  // see k_lr_softmax_fwd: exact-K folds guards
  const Wave wv = this_wave(blockDim.x);
  for (int i = wv.id; i < B; i += wv.n) {
    int jb = ptr[i], je = ptr[i + 1];
    float l[K] = {};
    for (int j = jb + wv.lane; j < je; j += 64)
      add_feature(l, vals[j], zn + keys[j] * (2 * KK), KK,
                  [&](const float* row, int k) {
                    return ftrl_w(row[k], row[KK + k], alpha_inv, beta, l1,
                                  l2);
                  });
    wave_sum(l);
    float ll = 0.f;
    if (wv.lane < KK) {
      // sigmoid_epilogue (the formula of record) written out: through the
      // call k_lr_ftrl_fwd<2,2> ran 0.4 us (5 %) over the parent's slowest
      // repeat; this form compiles to the code it had before the helpers
      // (profiles/lr_refactor.md). Every lane in here is below KK <= K, so
      // the select needs no guard.
      float mine = lane_select(l, wv.lane, K, 0.f);
      float p = 1.f / (1.f + expf(-mine));
      int y = (int)labels[i];
      float yk = (KK == 1) ? labels[i] : (float)(wv.lane == y);
      float wt = weight_of(wts, i);
      err[(int64_t)i * KK + wv.lane] = (p - yk) * wt;
      ll = -(yk * logf(p + LR_LOG_EPS) +
             (1.f - yk) * logf(1.f - p + LR_LOG_EPS));
    }
    // binary NLL summed over the KK outputs, as Objective.loss does: lanes
    // >= KK hold 0 and KK <= K, so the shifts below K bring every term to
    // lane 0 (none at K == 1)
    for (int sh = 32; sh; sh >>= 1)
      if (sh < K) ll += __shfl_xor(ll, sh, 64);
    if (wv.lane == 0) loss[i] = ll;
  }
}

__global__ void k_lr_ftrl_scatter(float* __restrict__ zn,
                                  const int64_t* __restrict__ keys,
                                  const float* __restrict__ vals,
                                  const int* __restrict__ ptr,
                                  const float* __restrict__ err,
                                  float alpha_inv, float beta, float l1,
                                  float l2, int B, int K) {
  const Wave wv = this_wave(blockDim.x);
  for (int i = wv.id; i < B; i += wv.n) {
    const float* e = err + (int64_t)i * K;
    for_pairs(ptr[i], ptr[i + 1], K, wv.lane, [&](int j, int k) {
      int64_t base = keys[j] * (2 * (int64_t)K);
      float z = zn[base + k];
      float n = zn[base + K + k];
      float w = ftrl_w(z, n, alpha_inv, beta, l1, l2);
      float g = vals[j] * e[k];
      float g2 = g * g;
      float nc = fmaxf(n, 0.f);
      float dz = alpha_inv * (sqrtf(nc + g2) - sqrtf(nc)) * w - g;
      // local state -= (dz | dn): z -= dz, n -= -g2
      zn[base + k] = z - dz;
      zn[base + K + k] = n + g2;
    });
  }
}

extern "C" void mv_launch_lr_ftrl_fwd(
    const float* zn, const int64_t* keys, const float* vals, const int* ptr,
    const float* labels, const float* wts, float* err, float* loss,
    float alpha_inv, float beta, float l1, float l2, int64_t B, int64_t K,
    hipStream_t s) {
  if (!B) return;
  int grid = grid_for(B * 64);
  auto launch = [&](auto kb, auto kkc) {
    k_lr_ftrl_fwd<decltype(kb)::value, decltype(kkc)::value>
        <<<grid, BLOCK, 0, s>>>(zn, keys, vals, ptr, labels, wts, err, loss,
                                alpha_inv, beta, l1, l2, (int)B, (int)K);
  };
  if (with_exact_k<1, 16>(K, [&](auto k) { launch(k, k); })) return;
  if (K <= 32) launch(kint<32>(), kint<0>());
  else __builtin_trap();  // K > 32: host refuses before launch
}

extern "C" void mv_launch_lr_ftrl_scatter(
    float* zn, const int64_t* keys, const float* vals, const int* ptr,
    const float* err, float alpha_inv, float beta, float l1, float l2,
    int64_t B, int64_t K, hipStream_t s) {
  if (!B) return;
  k_lr_ftrl_scatter<<<grid_for(B * 64), BLOCK, 0, s>>>(
      zn, keys, vals, ptr, err, alpha_inv, beta, l1, l2, (int)B, (int)K);
}

// ---------------------------------------------------------------------------
// Dense-mode minibatch post-GEMM fusion (reference sparse=false — its
// mnist.config deployment, objective.cpp:193-230 dense branch).  The two
// GEMMs (scores = X@W, grad = X^T@diff) stay on rocBLAS/MFMA; this kernel
// replaces the ~10 elementwise torch ops BETWEEN them (softmax/sigmoid,
// one_hot, diff, weighting, per-sample loss, loss mean-accumulate) with
// ONE launch that turns the logits buffer into the diff buffer in place
// and atomically accumulates mean loss into a chunk-wide scalar (one
// host sync per chunk).
//
// K >= 2: softmax, one wave per sample, lane k owns class k (K <= 64);
// loss = -log(p_y + eps) (SoftmaxObjective.loss).  K == 1: sigmoid;
// loss = -(y log p + (1-y) log(1-p)) (base Objective.loss at O=1).
// ---------------------------------------------------------------------------

// Sample i of the dense kernels, lane k holding class k's logit in `mine`:
// writes the K diffs to out[0..K) and returns the sample's loss on lane 0,
// 0 on the others.
static __device__ __forceinline__ float dense_sample(
    float mine, int K, int lane, int i, const float* labels,
    const float* wts, float* out) {
  float ll = 0.f;
  if (K == 1) {
    if (lane == 0) ll = sigmoid_epilogue(mine, -1, i, labels, wts, out);
  } else {
    float t = softmax_epilogue(mine, lane < K, lane, i, labels, wts, out);
    if (lane == 0) ll = t;
  }
  return ll;
}

__global__ void k_lr_dense_post(float* __restrict__ logits,
                                const float* __restrict__ labels,
                                const float* __restrict__ wts,
                                float* __restrict__ loss_acc,
                                float inv_b, int B, int K) {
  float* block_loss = block_loss_begin();
  const Wave wv = this_wave(blockDim.x);
  const int lane = wv.lane;
  float ll_sum = 0.f;
  for (int i = wv.id; i < B; i += wv.n) {
    if (K == 1) {
      // sigmoid_epilogue (the formula of record) written out: through the
      // call this path ran 0.3 us (3 %) over the parent's slowest repeat
      // (profiles/lr_refactor.md)
      if (lane == 0) {
        float wt = weight_of(wts, i);
        float s = logits[i];
        float p = 1.f / (1.f + expf(-s));
        float y = labels[i];
        logits[i] = (p - y) * wt;
        ll_sum -= y * logf(p + LR_LOG_EPS) +
                  (1.f - y) * logf(1.f - p + LR_LOG_EPS);
      }
      continue;
    }
    float* row = logits + (int64_t)i * K;
    float t = softmax_epilogue((lane < K) ? row[lane] : -1e30f, lane < K,
                               lane, i, labels, wts, row);
    if (lane == 0) ll_sum += t;
  }
  block_loss_end(block_loss, loss_acc, inv_b, lane, ll_sum);
}

extern "C" void mv_launch_lr_dense_post(float* logits, const float* labels,
                                        const float* wts, float* loss_acc,
                                        float inv_b, int64_t B, int64_t K,
                                        hipStream_t s) {
  if (!B) return;
  k_lr_dense_post<<<grid_for_cap(B * 64, 512), BLOCK, 0, s>>>(
      logits, labels, wts, loss_acc, inv_b, (int)B, (int)K);
}

// ---------------------------------------------------------------------------
// Dense-mode fused FORWARD (scores = X@W -> softmax/sigmoid -> diff +
// loss) in ONE kernel: W staged to LDS once per workgroup (d*K*4 B,
// odd-padded row stride so the per-element class reads are LDS
// bank-conflict-free), one 64-lane wave per sample, lane e-strided over
// the X row (coalesced 256 B/instr stream — X is read EXACTLY ONCE, the
// memory floor for this op).  Replaces the rocBLAS skinny GEMM
// [B,d]x[d,K<=16] whose 16x16 macro-tiles ran at 1.3 TB/s.
//
// K is an EXACT compile-time parameter (one instantiation per class
// count 1..16).  The first version carried a runtime `if (k < K)` guard
// inside the unrolled class loop; the compiler turned that into a
// per-class branch ladder with a full `s_waitcnt vmcnt(0) lgkmcnt(0)`
// after EVERY ds_read_b32 — 102 us measured (5x SLOWER than the rocBLAS
// pair it meant to replace).  Branch-free exact-K bodies batch the K
// LDS reads under one waitcnt.  Falls back to rocBLAS +
// k_lr_dense_post when K > 16 or d*(K|1)*4 exceeds the LDS budget.
// ---------------------------------------------------------------------------

template <int K, bool NT>
__global__ void k_lr_dense_fwd(const float* __restrict__ X,
                               const float* __restrict__ W,
                               const float* __restrict__ labels,
                               const float* __restrict__ wts,
                               float* __restrict__ diff,
                               float* __restrict__ loss_acc,
                               float inv_b, int B, int d) {
  extern __shared__ float wlds[];  // [d][K|1]
  constexpr int S = K | 1;  // odd stride: (S*lane) % 64 banks all distinct
  for (int t = threadIdx.x; t < d * K; t += blockDim.x)
    wlds[(t / K) * S + (t % K)] = W[t];
  float* block_loss = block_loss_begin();  // its barrier publishes wlds
  const Wave wv = this_wave(blockDim.x);
  float ll_sum = 0.f;
  for (int i = wv.id; i < B; i += wv.n) {
    const float* __restrict__ xrow = X + (int64_t)i * d;
    float acc[K] = {};
    for (int e = wv.lane; e < d; e += 64) {
      float x = NT ? __builtin_nontemporal_load(xrow + e) : xrow[e];
      add_feature(acc, x, wlds + e * S, K,
                  [](const float* wr, int k) { return wr[k]; });
    }
    wave_sum(acc);
    ll_sum += dense_sample(lane_select(acc, wv.lane, K, -1e30f), K, wv.lane,
                           i, labels, wts, diff + (int64_t)i * K);
  }
  block_loss_end(block_loss, loss_acc, inv_b, wv.lane, ll_sum);
}

extern "C" int mv_launch_lr_dense_fwd(const float* X, const float* W,
                                      const float* labels, const float* wts,
                                      float* diff, float* loss_acc,
                                      float inv_b, int64_t B, int64_t d,
                                      int64_t K, int nt, hipStream_t s) {
  if (!B) return 1;
  size_t lds = (size_t)d * (K | 1) * sizeof(float);
  if (K > 16 || lds > 144 * 1024) return 0;  // rocBLAS + post fallback
  // The W staging leaves LDS room for only ~1 WG/CU, so the workgroup
  // carries the CU's whole latency-hiding budget itself: 1024 threads
  // = 16 waves, one workgroup per CU, one staging pass per CU.
  int64_t blocks = (B + 15) / 16;  // 16 waves/block, one sample per wave
  if (blocks > 256) blocks = 256;  // 1 LDS-heavy WG per CU
  int grid = (int)blocks;
  return with_exact_k<1, 16>(K, [&](auto k) {
    constexpr int KT = decltype(k)::value;
    auto* kernel = nt ? k_lr_dense_fwd<KT, true> : k_lr_dense_fwd<KT, false>;
    kernel<<<grid, COPY_BLOCK, lds, s>>>(X, W, labels, wts, diff, loss_acc,
                                         inv_b, (int)B, (int)d);
  });
}


// ---------------------------------------------------------------------------
// Nearest rows (MatrixTable.nearest_rows): the k best rows of the shard for
// each of Q queries, in two plain launches with no atomics and no
// cross-workgroup communication.
//
// Ordering rule, used at every level (inside a wave, across waves, across
// shards in tables/matrix_table.py merge_topk): candidate a comes before b
// when a.score > b.score, or the scores are equal and a.id < b.id. A NaN
// score enters selection as -inf. An empty slot is (-inf, TOPK_EMPTY), an
// id above every real row, so it never comes before a real candidate.
//
// k_row_topk<Q, COSINE>: the queries are staged once per workgroup into LDS
// ([col][Q|1], the odd stride of k_lr_dense_fwd), one 64-lane wave takes one
// row at a time, lanes e-strided over it with Q fma accumulators each (and
// rr = sum x*x under cosine), wave_sum leaves all Q scores on every lane.
// The shard is read exactly once. A row's score depends on the row, the
// query and num_col only (fixed lane assignment, fixed butterfly), never on
// the wave that computed it, so the result does not depend on the grid.
// Each wave keeps Q sorted lists, lane j holding the j-th best (score, local
// row) so far, and stores them to the partials buffer at the end.
//
// k_topk_merge: one workgroup per query streams that query's partials
// through the same insertion routine and writes the final k pairs with
// global ids. The partials are laid out [Q][waves][k], not [waves][Q][k]:
// a query's candidates are then one contiguous run that the merge reads 64
// at a time, fully coalesced, whatever k is.
// ---------------------------------------------------------------------------

#define TOPK_EMPTY 0x7fffffff
// partials stay small: 1024 blocks of 4 waves hold 16 waves on each of the
// 256 CUs, and 4096 lists of 64 pairs for 16 queries are 32 MiB
#define ROW_TOPK_GRID 1024
// the default dynamic LDS allowance of a launch; two such workgroups still
// fit a CU's 160 KiB
#define ROW_TOPK_LDS (64 * 1024)
#define MERGE_WAVES (COPY_BLOCK / WAVE)
// 64-column chunks of its next row that a scanning wave loads ahead
#define TOPK_PF 4

static __device__ __forceinline__ bool topk_before(float sa, int ia, float sb,
                                                   int ib) {
  return sa > sb || (sa == sb && ia < ib);
}

// value of lane `src` (wave-uniform) on every lane
static __device__ __forceinline__ float lane_bcast(float v, int src) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src));
}
static __device__ __forceinline__ int lane_bcast(int v, int src) {
  return __builtin_amdgcn_readlane(v, src);
}

// Offers (s, id), the same on all 64 lanes, to the sorted list whose j-th
// entry lane j holds in (ls, li); the list keeps its first k entries in
// order. All 64 lanes come in and stay together: the one branch is taken by
// the whole wave or by none of it, so the ballot and the shuffles inside
// see every lane. Lanes from k up only ever hold entries that fell off the
// end; nobody reads them.
static __device__ __forceinline__ void topk_insert(float& ls, int& li, float s,
                                                   int id, int k, int lane) {
  s = (s != s) ? -INFINITY : s;
  if (!topk_before(s, id, lane_bcast(ls, k - 1), lane_bcast(li, k - 1)))
    return;
  int pos = __popcll(__ballot(topk_before(ls, li, s, id)));
  float us = __shfl_up(ls, 1, 64);
  int ui = __shfl_up(li, 1, 64);
  if (lane > pos) { ls = us; li = ui; }
  if (lane == pos) { ls = s; li = id; }
}

// Offers 64 candidates, lane j holding the j-th, to the list: one ballot
// finds those that come before the list's last entry, and only they go
// through topk_insert, which tests each against the list as it then stands.
static __device__ __forceinline__ void topk_insert_lanes(float& ls, int& li,
                                                         float cs, int ci,
                                                         int k, int lane) {
  unsigned long long m = __ballot(
      topk_before(cs, ci, lane_bcast(ls, k - 1), lane_bcast(li, k - 1)));
  while (m) {
    int j = __ffsll(m) - 1;
    m &= m - 1;
    topk_insert(ls, li, lane_bcast(cs, j), lane_bcast(ci, j), k, lane);
  }
}

template <int Q, bool COSINE>
__global__ __launch_bounds__(BLOCK) void k_row_topk(
    const float* __restrict__ shard, const float* __restrict__ queries,
    float* __restrict__ part_s, int* __restrict__ part_i, int R, int cols,
    int k) {
  extern __shared__ float qlds[];  // [cols][Q|1]
  constexpr int S = Q | 1;  // odd stride: (S*lane) % 64 banks all distinct
  for (int t = threadIdx.x; t < cols * Q; t += BLOCK)
    qlds[(t % cols) * S + t / cols] = queries[t];
  __syncthreads();
  const Wave wv = this_wave(BLOCK);
  float ls[Q];
  int li[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) { ls[q] = -INFINITY; li[q] = TOPK_EMPTY; }
  // A wave's NEXT row is already on its way while the current one is
  // reduced and offered to the lists: the first TOPK_PF chunks of 64 columns
  // (the whole row up to 256 columns) are loaded one row ahead. Without it
  // a wave has one row's loads in flight, waits out their latency, then
  // runs the butterfly and the insertions with nothing outstanding
  // (profiles/nearest_rows.md). Each lane still adds its columns in
  // ascending order, so the scores are the same bits.
  float xn[TOPK_PF];
  auto fetch = [&](int r) {
    const float* __restrict__ row = shard + (int64_t)r * cols;
#pragma unroll
    for (int j = 0; j < TOPK_PF; ++j) {
      int e = wv.lane + WAVE * j;
      xn[j] = e < cols ? row[e] : 0.f;
    }
  };
  if (wv.id < R) fetch(wv.id);
  for (int r = wv.id; r < R; r += wv.n) {
    const float* __restrict__ row = shard + (int64_t)r * cols;
    float x[TOPK_PF];
#pragma unroll
    for (int j = 0; j < TOPK_PF; ++j) x[j] = xn[j];
    if ((int64_t)r + wv.n < R) fetch(r + wv.n);
    float acc[Q] = {};
    float rr = 0.f;
    auto term = [](const float* qr, int q) { return qr[q]; };
#pragma unroll
    for (int j = 0; j < TOPK_PF; ++j) {
      int e = wv.lane + WAVE * j;
      if (e < cols) {
        add_feature(acc, x[j], qlds + e * S, Q, term);
        if (COSINE) rr += x[j] * x[j];
      }
    }
    for (int e = wv.lane + WAVE * TOPK_PF; e < cols; e += WAVE) {
      float xe = row[e];
      add_feature(acc, xe, qlds + e * S, Q, term);
      if (COSINE) rr += xe * xe;
    }
    wave_sum(acc);
    float rinv = 1.f;
    if (COSINE) {
      rr = wave_sum(rr);
      rinv = 1.f / sqrtf(rr);
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      // a zero-norm row scores exactly 0; a NaN norm stays NaN (-> -inf)
      float s = COSINE ? (rr == 0.f ? 0.f : acc[q] * rinv) : acc[q];
      topk_insert(ls[q], li[q], s, r, k, wv.lane);
    }
  }
  if (wv.lane < k) {
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      int64_t at = ((int64_t)q * wv.n + wv.id) * k + wv.lane;
      part_s[at] = ls[q];
      part_i[at] = li[q];
    }
  }
}

__global__ __launch_bounds__(COPY_BLOCK) void k_topk_merge(
    const float* __restrict__ part_s, const int* __restrict__ part_i,
    float* __restrict__ out_s, int64_t* __restrict__ out_i, int n, int k,
    int64_t row_offset) {
  __shared__ float ms[COPY_BLOCK];
  __shared__ int mi[COPY_BLOCK];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float* __restrict__ ps = part_s + (int64_t)blockIdx.x * n;
  const int* __restrict__ pi = part_i + (int64_t)blockIdx.x * n;
  float ls = -INFINITY;
  int li = TOPK_EMPTY;
  for (int base = w * WAVE; base < n; base += COPY_BLOCK) {
    int j = base + lane;
    float cs = j < n ? ps[j] : -INFINITY;
    int ci = j < n ? pi[j] : TOPK_EMPTY;
    topk_insert_lanes(ls, li, cs, ci, k, lane);
  }
  ms[threadIdx.x] = ls;
  mi[threadIdx.x] = li;
  __syncthreads();
  if (w) return;
  for (int o = 1; o < MERGE_WAVES; ++o)
    topk_insert_lanes(ls, li, ms[o * WAVE + lane], mi[o * WAVE + lane], k,
                      lane);
  if (lane < k) {
    int64_t at = (int64_t)blockIdx.x * k + lane;
    out_s[at] = ls;
    out_i[at] = li == TOPK_EMPTY ? INT64_MAX : li + row_offset;
  }
}

// queries one pass can take: the most, up to 16 and Q, whose [cols][q|1]
// image fits the LDS budget; 0 when a single query does not
static int row_topk_chunk(int64_t cols, int64_t Q) {
  int64_t c = Q < 16 ? Q : 16;
  while (c > 0 && (size_t)cols * (c | 1) * sizeof(float) > ROW_TOPK_LDS) --c;
  return (int)c;
}

extern "C" int mv_row_topk_plan(int64_t R, int64_t cols, int64_t Q,
                                int* waves) {
  *waves = grid_for_cap((R + 3) / 4 * BLOCK, ROW_TOPK_GRID) * (BLOCK / WAVE);
  // row indices are ints, and the row loop steps one past R by `waves`
  if (R > INT32_MAX - ROW_TOPK_GRID * (BLOCK / WAVE) || cols < 1) return 0;
  return row_topk_chunk(cols, Q);
}

extern "C" int mv_launch_row_topk(const float* shard, const float* queries,
                                  float* part_s, int* part_i, float* out_s,
                                  int64_t* out_i, int64_t R, int64_t cols,
                                  int64_t Q, int64_t k, int cosine,
                                  int64_t row_offset, hipStream_t s) {
  int waves;
  int chunk = mv_row_topk_plan(R, cols, Q, &waves);
  if (!chunk || k < 1 || k > WAVE) return 0;
  if (!R) return 1;
  // every pass reuses the one partials buffer: the stream orders the merge
  // of a pass before the scan of the next
  for (int64_t q0 = 0; q0 < Q; q0 += chunk) {
    int64_t qc = Q - q0 < chunk ? Q - q0 : chunk;
    size_t lds = (size_t)cols * (qc | 1) * sizeof(float);
    with_exact_k<1, 16>(qc, [&](auto qt) {
      constexpr int QT = decltype(qt)::value;
      auto* kernel = cosine ? k_row_topk<QT, true> : k_row_topk<QT, false>;
      kernel<<<waves / (BLOCK / WAVE), BLOCK, lds, s>>>(
          shard, queries + q0 * cols, part_s, part_i, (int)R, (int)cols,
          (int)k);
    });
    k_topk_merge<<<(int)qc, COPY_BLOCK, 0, s>>>(
        part_s, part_i, out_s + q0 * k, out_i + q0 * k, (int)(waves * k),
        (int)k, row_offset);
  }
  return 1;
}
