// Torch binding layer for the gfx950 HIP kernels (kernels.hip).
//
// This translation unit is compiled by torch.utils.cpp_extension (it needs
// the ATen headers); the kernels themselves are hipcc-compiled pure HIP in
// kernels.hip and linked in as an object, so no hipify/CUDA-compat layer
// ever touches the device code.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <cstdint>
#include <limits>
#include <tuple>

#include "launchers.h"

namespace {

hipStream_t cur_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

void check_f32(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be fp32");
}

void check_dev(const torch::Tensor& t, const char* name,
               torch::ScalarType st) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == st, name, " dtype mismatch");
}

// Validation shared by the elementwise wrappers: every tensor on the GPU,
// contiguous and of dtype st (fp32, with check_f32's wording, when no st
// is given), and all of one numel, which is returned.
using Named = std::pair<const char*, torch::Tensor>;
int64_t check_same(std::initializer_list<Named> ts,
                   c10::optional<torch::ScalarType> st = c10::nullopt) {
  for (const auto& t : ts) {
    if (st) check_dev(t.second, t.first, *st);
    else check_f32(t.second, t.first);
  }
  int64_t n = ts.begin()->second.numel();
  for (const auto& t : ts)
    TORCH_CHECK(t.second.numel() == n, "size mismatch");
  return n;
}

float* f32(const torch::Tensor& t) { return t.data_ptr<float>(); }
double* f64(const torch::Tensor& t) { return t.data_ptr<double>(); }

// bf16 wire format: on an fp32 shard the delta (or vals) and the Get buffer
// may hold bfloat16; the kernels widen and narrow in registers. The bits
// match WIRE_DELTA / WIRE_OUT in kernels.hip.
constexpr int kWireDelta = 1, kWireOut = 2;

// Validates one such tensor (on the GPU, contiguous, n elements, of the
// shard's dtype st or, where st is fp32, bf16) and returns `bit` if it
// holds bf16, else 0. Without st the shard is fp32, worded as check_f32.
int wire_bit(const torch::Tensor& t, const char* name, int64_t n, int bit,
             c10::optional<torch::ScalarType> st = c10::nullopt) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.numel() == n, "size mismatch");
  auto want = st.value_or(torch::kFloat32);
  if (want == torch::kFloat32 && t.scalar_type() == torch::kBFloat16)
    return bit;
  if (st) {
    TORCH_CHECK(t.scalar_type() == want, name, " dtype mismatch");
  } else {
    TORCH_CHECK(t.scalar_type() == want, name, " must be fp32 or bf16");
  }
  return 0;
}

void nt_copy(torch::Tensor dst, torch::Tensor src) {
  int64_t n = check_same({{"src", src}});
  int wire = wire_bit(dst, "dst", n, kWireOut);
  mv_launch_copy(dst.data_ptr(), f32(src), wire, n, cur_stream());
}

void add_inplace(torch::Tensor data, torch::Tensor delta, bool reverse) {
  // dtype-dispatched K1 (reference instantiates int/float/double tables,
  // array_table.cpp:153-154; int updater is add-only, updater.cpp:40-43)
  auto st = data.scalar_type();
  int64_t n = check_same({{"data", data}}, st);
  int wire = wire_bit(delta, "delta", n, kWireDelta, st);
  if (st == torch::kFloat32)
    mv_launch_add(f32(data), delta.data_ptr(), wire, n, cur_stream(), reverse);
  else if (st == torch::kFloat64)
    mv_launch_add_f64(f64(data), f64(delta), n, cur_stream(), reverse);
  else if (st == torch::kInt32)
    mv_launch_add_i32(data.data_ptr<int32_t>(), delta.data_ptr<int32_t>(), n,
                      cur_stream(), reverse);
  else if (st == torch::kInt64)
    mv_launch_add_i64(data.data_ptr<int64_t>(), delta.data_ptr<int64_t>(), n,
                      cur_stream(), reverse);
  else
    TORCH_CHECK(false, "add_inplace: unsupported dtype ", data.dtype());
}

// data += sign * delta; `out`, when given, also receives the updated data
void launch_sgd(const char* fn, const torch::Tensor& data,
                const torch::Tensor& delta, const torch::Tensor* out,
                double sign, bool reverse) {
  auto st = data.scalar_type();
  int64_t n = check_same({{"data", data}}, st);
  int wire = wire_bit(delta, "delta", n, kWireDelta, st);
  if (out) wire |= wire_bit(*out, "out", n, kWireOut, st);
  if (st == torch::kFloat32)
    mv_launch_sgd(f32(data), delta.data_ptr(), out ? out->data_ptr() : nullptr,
                  wire, (float)sign, n, cur_stream(), reverse);
  else if (st == torch::kFloat64)
    mv_launch_sgd_f64(f64(data), f64(delta), out ? f64(*out) : nullptr, sign,
                      n, cur_stream(), reverse);
  else
    TORCH_CHECK(false, fn, ": unsupported dtype ", data.dtype());
}

void sgd_update(torch::Tensor data, torch::Tensor delta, bool reverse) {
  launch_sgd("sgd_update", data, delta, nullptr, -1.0, reverse);
}

void sgd_copy_update(torch::Tensor data, torch::Tensor delta,
                     torch::Tensor out, double sign, bool reverse) {
  launch_sgd("sgd_copy_update", data, delta, &out, sign, reverse);
}

void momentum_update(torch::Tensor data, torch::Tensor m, torch::Tensor delta,
                     double mu, bool reverse) {
  auto st = data.scalar_type();
  int64_t n = check_same({{"data", data}, {"m", m}}, st);
  int wire = wire_bit(delta, "delta", n, kWireDelta, st);
  if (st == torch::kFloat32)
    mv_launch_momentum(f32(data), f32(m), delta.data_ptr(), nullptr, wire,
                       (float)mu, n, cur_stream(), reverse);
  else if (st == torch::kFloat64)
    mv_launch_momentum_f64(f64(data), f64(m), f64(delta), mu, n,
                           cur_stream(), reverse);
  else
    TORCH_CHECK(false, "momentum_update: unsupported dtype ", data.dtype());
}

void momentum_copy_update(torch::Tensor data, torch::Tensor m,
                          torch::Tensor delta, torch::Tensor out, double mu,
                          bool reverse) {
  int64_t n = check_same({{"data", data}, {"m", m}});
  int wire = wire_bit(delta, "delta", n, kWireDelta) |
             wire_bit(out, "out", n, kWireOut);
  mv_launch_momentum(f32(data), f32(m), delta.data_ptr(), out.data_ptr(),
                     wire, (float)mu, n, cur_stream(), reverse);
}

void adagrad_update(torch::Tensor data, torch::Tensor gsq, torch::Tensor delta,
                    double lr, double rho, double eps, bool reverse) {
  auto st = data.scalar_type();
  int64_t n = check_same({{"data", data}, {"gsq", gsq}}, st);
  int wire = wire_bit(delta, "delta", n, kWireDelta, st);
  if (st == torch::kFloat32)
    mv_launch_adagrad(f32(data), f32(gsq), delta.data_ptr(), nullptr, wire,
                      (float)lr, (float)rho, (float)eps, n, cur_stream(),
                      reverse);
  else if (st == torch::kFloat64)
    mv_launch_adagrad_f64(f64(data), f64(gsq), f64(delta), lr, rho, eps, n,
                          cur_stream(), reverse);
  else
    TORCH_CHECK(false, "adagrad_update: unsupported dtype ", data.dtype());
}

void adagrad_copy_update(torch::Tensor data, torch::Tensor gsq,
                         torch::Tensor delta, torch::Tensor out,
                         double lr, double rho, double eps, bool reverse) {
  int64_t n = check_same({{"data", data}, {"gsq", gsq}});
  int wire = wire_bit(delta, "delta", n, kWireDelta) |
             wire_bit(out, "out", n, kWireOut);
  mv_launch_adagrad(f32(data), f32(gsq), delta.data_ptr(), out.data_ptr(),
                    wire, (float)lr, (float)rho, (float)eps, n, cur_stream(),
                    reverse);
}

void dcasgd_update(torch::Tensor data, torch::Tensor bak, torch::Tensor delta,
                   double lr, double lambda, bool reverse) {
  int64_t n = check_same({{"data", data}, {"bak", bak}});
  int wire = wire_bit(delta, "delta", n, kWireDelta);
  mv_launch_dcasgd(f32(data), f32(bak), delta.data_ptr(), nullptr, wire,
                   (float)lr, (float)lambda, n, cur_stream(), reverse);
}

void dcasgd_copy_update(torch::Tensor data, torch::Tensor bak,
                        torch::Tensor delta, torch::Tensor out,
                        double lr, double lambda, bool reverse) {
  int64_t n = check_same({{"data", data}, {"bak", bak}});
  int wire = wire_bit(delta, "delta", n, kWireDelta) |
             wire_bit(out, "out", n, kWireOut);
  mv_launch_dcasgd(f32(data), f32(bak), delta.data_ptr(), out.data_ptr(),
                   wire, (float)lr, (float)lambda, n, cur_stream(), reverse);
}

void dcasgda_update(torch::Tensor data, torch::Tensor bak, torch::Tensor msq,
                    torch::Tensor delta, double lr, double lambda, double rho,
                    double eps, bool reverse) {
  int64_t n = check_same({{"data", data}, {"bak", bak}, {"msq", msq}});
  int wire = wire_bit(delta, "delta", n, kWireDelta);
  mv_launch_dcasgda(f32(data), f32(bak), f32(msq), delta.data_ptr(), nullptr,
                    wire, (float)lr, (float)lambda, (float)rho, (float)eps, n,
                    cur_stream(), reverse);
}

void dcasgda_copy_update(torch::Tensor data, torch::Tensor bak,
                         torch::Tensor msq, torch::Tensor delta,
                         torch::Tensor out, double lr, double lambda,
                         double rho, double eps, bool reverse) {
  int64_t n = check_same({{"data", data}, {"bak", bak}, {"msq", msq}});
  int wire = wire_bit(delta, "delta", n, kWireDelta) |
             wire_bit(out, "out", n, kWireOut);
  mv_launch_dcasgda(f32(data), f32(bak), f32(msq), delta.data_ptr(),
                    out.data_ptr(), wire, (float)lr, (float)lambda,
                    (float)rho, (float)eps, n, cur_stream(), reverse);
}

// step = lr / (1 - b1^t), rbc2 = 1 / sqrt(1 - b2^t), decay = 1 - lr*wd:
// the caller owns the update count t
void adam_update(torch::Tensor data, torch::Tensor m, torch::Tensor v,
                 torch::Tensor delta, double b1, double b2, double step,
                 double rbc2, double decay, double eps, bool reverse) {
  auto st = data.scalar_type();
  int64_t n = check_same({{"data", data}, {"m", m}, {"v", v}}, st);
  int wire = wire_bit(delta, "delta", n, kWireDelta, st);
  if (st == torch::kFloat32)
    mv_launch_adam(f32(data), f32(m), f32(v), delta.data_ptr(), nullptr, wire,
                   b1, b2, step, rbc2, decay, eps, n, cur_stream(), reverse);
  else if (st == torch::kFloat64)
    mv_launch_adam_f64(f64(data), f64(m), f64(v), f64(delta), b1, b2, step,
                       rbc2, decay, eps, n, cur_stream(), reverse);
  else
    TORCH_CHECK(false, "adam_update: unsupported dtype ", data.dtype());
}

void adam_copy_update(torch::Tensor data, torch::Tensor m, torch::Tensor v,
                      torch::Tensor delta, torch::Tensor out, double b1,
                      double b2, double step, double rbc2, double decay,
                      double eps, bool reverse) {
  int64_t n = check_same({{"data", data}, {"m", m}, {"v", v}});
  int wire = wire_bit(delta, "delta", n, kWireDelta) |
             wire_bit(out, "out", n, kWireOut);
  mv_launch_adam(f32(data), f32(m), f32(v), delta.data_ptr(), out.data_ptr(),
                 wire, b1, b2, step, rbc2, decay, eps, n, cur_stream(),
                 reverse);
}

// 1-bit Add wire (onebit_filter.py): 136 bytes per block of 1024 elements
int64_t onebit_bytes(int64_t n) { return 136 * ((n + 1023) / 1024); }

void check_payload(const torch::Tensor& t, const char* name, int64_t bytes) {
  check_dev(t, name, torch::kUInt8);
  TORCH_CHECK(t.numel() == bytes, name, " must hold ", bytes, " bytes");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 8 == 0, name,
              " must be 8-byte aligned");
}

// payload <- code of (residual + delta); residual <- the quantisation error.
// delta and residual may be 4-byte-aligned views (pieces of a table).
void onebit_encode(torch::Tensor delta, torch::Tensor residual,
                   torch::Tensor payload) {
  int64_t n = check_same({{"delta", delta}, {"residual", residual}});
  TORCH_CHECK(n >= 1, "onebit_encode: empty piece");
  TORCH_CHECK((n + 1023) / 1024 <= INT32_MAX, "onebit_encode: piece too large");
  check_payload(payload, "payload", onebit_bytes(n));
  mv_launch_onebit_encode(f32(delta), f32(residual),
                          payload.data_ptr<uint8_t>(), n, cur_stream());
}

// out <- the sum, in payload order, of the values nparts consecutive
// payloads of one n-element piece decode to
void onebit_decode_sum(torch::Tensor out, torch::Tensor payloads,
                       int64_t nparts) {
  check_f32(out, "out");
  int64_t n = out.numel();
  TORCH_CHECK(n >= 1, "onebit_decode_sum: empty piece");
  TORCH_CHECK(nparts >= 1 && nparts <= INT32_MAX,
              "onebit_decode_sum: nparts must be >= 1");
  check_payload(payloads, "payloads", nparts * onebit_bytes(n));
  mv_launch_onebit_decode_sum(f32(out), payloads.data_ptr<uint8_t>(),
                              (int)nparts, n, cur_stream());
}

void row_gather_out(torch::Tensor out, torch::Tensor shard, torch::Tensor rows) {
  check_f32(shard, "shard");
  TORCH_CHECK(shard.dim() == 2, "shard must be 2-D");
  TORCH_CHECK(rows.scalar_type() == torch::kInt64 && rows.is_cuda() &&
              rows.is_contiguous(), "rows must be contiguous int64 on GPU");
  TORCH_CHECK(out.numel() == rows.numel() * shard.size(1), "out size mismatch");
  int wire = wire_bit(out, "out", out.numel(), kWireOut);
  mv_launch_row_gather(out.data_ptr(), wire, shard.data_ptr<float>(),
                       rows.data_ptr<int64_t>(), rows.numel(), shard.size(1),
                       cur_stream());
}

// dtype: the result's, fp32 (the default) or bf16
torch::Tensor row_gather(torch::Tensor shard, torch::Tensor rows,
                         c10::optional<torch::ScalarType> dtype) {
  check_f32(shard, "shard");
  TORCH_CHECK(shard.dim() == 2, "shard must be 2-D");
  auto out = torch::empty({rows.numel(), shard.size(1)},
                          shard.options().dtype(
                              dtype.value_or(torch::kFloat32)));
  row_gather_out(out, shard, rows);
  return out;
}

void row_scatter_add(torch::Tensor shard, torch::Tensor rows,
                     torch::Tensor vals, double sign,
                     bool assume_unique = false) {
  check_f32(shard, "shard");
  TORCH_CHECK(shard.dim() == 2, "shard must be 2-D");
  TORCH_CHECK(rows.scalar_type() == torch::kInt64 && rows.is_cuda() &&
              rows.is_contiguous(), "rows must be contiguous int64 on GPU");
  TORCH_CHECK(vals.numel() == rows.numel() * shard.size(1), "vals size mismatch");
  int wire = wire_bit(vals, "vals", vals.numel(), kWireDelta);
  mv_launch_row_scatter_add(shard.data_ptr<float>(), vals.data_ptr(), wire,
                            rows.data_ptr<int64_t>(), (float)sign,
                            rows.numel(), shard.size(1),
                            assume_unique ? 1 : 0, cur_stream());
}

void row_scatter_adagrad(torch::Tensor shard, torch::Tensor gsq,
                         torch::Tensor rows, torch::Tensor vals,
                         double lr, double rho, double eps,
                         bool assume_unique = false) {
  check_f32(shard, "shard"); check_f32(gsq, "gsq");
  TORCH_CHECK(shard.dim() == 2, "shard must be 2-D");
  TORCH_CHECK(gsq.sizes() == shard.sizes(), "gsq shape mismatch");
  TORCH_CHECK(rows.scalar_type() == torch::kInt64 && rows.is_cuda() &&
              rows.is_contiguous(), "rows must be contiguous int64 on GPU");
  TORCH_CHECK(vals.numel() == rows.numel() * shard.size(1), "vals mismatch");
  int wire = wire_bit(vals, "vals", vals.numel(), kWireDelta);
  mv_launch_row_scatter_adagrad(
      shard.data_ptr<float>(), gsq.data_ptr<float>(), vals.data_ptr(), wire,
      rows.data_ptr<int64_t>(), (float)lr, (float)rho, (float)eps,
      rows.numel(), shard.size(1), assume_unique ? 1 : 0, cur_stream());
}

// Validation shared by the keyed stateful updaters; returns perm's data
// pointer, or null for the identity, and in `wire` whether vals holds bf16.
const int64_t* check_row_update(const torch::Tensor& shard,
                                std::initializer_list<Named> state,
                                const torch::Tensor& rows,
                                const torch::Tensor& vals,
                                const c10::optional<torch::Tensor>& perm,
                                int* wire) {
  check_f32(shard, "shard");
  *wire = wire_bit(vals, "vals", vals.numel(), kWireDelta);
  TORCH_CHECK(shard.dim() == 2, "shard must be 2-D");
  for (const auto& t : state) {
    check_f32(t.second, t.first);
    TORCH_CHECK(t.second.sizes() == shard.sizes(), t.first,
                " shape mismatch");
  }
  TORCH_CHECK(rows.scalar_type() == torch::kInt64 && rows.is_cuda() &&
              rows.is_contiguous(), "rows must be contiguous int64 on GPU");
  TORCH_CHECK(vals.numel() == rows.numel() * shard.size(1), "vals mismatch");
  if (!perm.has_value()) return nullptr;
  TORCH_CHECK(perm->scalar_type() == torch::kInt64 && perm->is_cuda() &&
              perm->is_contiguous(), "perm must be contiguous int64 on GPU");
  TORCH_CHECK(perm->numel() == rows.numel(), "perm size mismatch");
  return perm->data_ptr<int64_t>();
}

void row_momentum_update(torch::Tensor shard, torch::Tensor m,
                         torch::Tensor rows, torch::Tensor vals, double mu,
                         c10::optional<torch::Tensor> perm) {
  int wire;
  const int64_t* pp = check_row_update(shard, {{"m", m}}, rows, vals, perm,
                                       &wire);
  mv_launch_row_momentum(f32(shard), f32(m), vals.data_ptr(), wire,
                         rows.data_ptr<int64_t>(), pp, (float)mu,
                         rows.numel(), shard.size(1), cur_stream());
}

void row_dcasgd_update(torch::Tensor shard, torch::Tensor bak,
                       torch::Tensor rows, torch::Tensor vals, double lr,
                       double lambda, c10::optional<torch::Tensor> perm) {
  int wire;
  const int64_t* pp = check_row_update(shard, {{"bak", bak}}, rows, vals,
                                       perm, &wire);
  mv_launch_row_dcasgd(f32(shard), f32(bak), vals.data_ptr(), wire,
                       rows.data_ptr<int64_t>(), pp, (float)lr,
                       (float)lambda, rows.numel(), shard.size(1),
                       cur_stream());
}

void row_dcasgda_update(torch::Tensor shard, torch::Tensor bak,
                        torch::Tensor msq, torch::Tensor rows,
                        torch::Tensor vals, double lr, double lambda,
                        double rho, double eps,
                        c10::optional<torch::Tensor> perm) {
  int wire;
  const int64_t* pp = check_row_update(shard, {{"bak", bak}, {"msq", msq}},
                                       rows, vals, perm, &wire);
  mv_launch_row_dcasgda(f32(shard), f32(bak), f32(msq), vals.data_ptr(), wire,
                        rows.data_ptr<int64_t>(), pp, (float)lr,
                        (float)lambda, (float)rho, (float)eps, rows.numel(),
                        shard.size(1), cur_stream());
}

void row_adam_update(torch::Tensor shard, torch::Tensor m, torch::Tensor v,
                     torch::Tensor rows, torch::Tensor vals, double b1,
                     double b2, double step, double rbc2, double decay,
                     double eps, c10::optional<torch::Tensor> perm) {
  int wire;
  const int64_t* pp = check_row_update(shard, {{"m", m}, {"v", v}}, rows,
                                       vals, perm, &wire);
  mv_launch_row_adam(f32(shard), f32(m), f32(v), vals.data_ptr(), wire,
                     rows.data_ptr<int64_t>(), pp, b1, b2, step, rbc2, decay,
                     eps, rows.numel(), shard.size(1), cur_stream());
}

void w2v_train(torch::Tensor in_emb, torch::Tensor out_emb,
               torch::Tensor in_gsq, torch::Tensor out_gsq,
               torch::Tensor in_idx, torch::Tensor in_off,
               torch::Tensor out_idx, torch::Tensor out_label,
               torch::Tensor out_off, double lr, bool use_adagrad,
               bool use_atomic) {
  check_f32(in_emb, "in_emb"); check_f32(out_emb, "out_emb");
  check_f32(out_label, "out_label");
  TORCH_CHECK(in_emb.dim() == 2 && out_emb.dim() == 2, "emb must be 2-D");
  TORCH_CHECK(in_emb.size(1) == out_emb.size(1), "dim mismatch");
  TORCH_CHECK(in_emb.size(1) <= 2048, "w2v kernel supports dim <= 2048");
  TORCH_CHECK(in_idx.scalar_type() == torch::kInt64 &&
              out_idx.scalar_type() == torch::kInt64, "idx must be int64");
  TORCH_CHECK(in_off.scalar_type() == torch::kInt32 &&
              out_off.scalar_type() == torch::kInt32, "offsets must be int32");
  // the kernel takes these as raw device pointers
  check_dev(in_idx, "in_idx", torch::kInt64);
  check_dev(out_idx, "out_idx", torch::kInt64);
  check_dev(in_off, "in_off", torch::kInt32);
  check_dev(out_off, "out_off", torch::kInt32);
  TORCH_CHECK(in_off.numel() >= 1, "in_off needs at least one entry");
  TORCH_CHECK(out_idx.numel() == out_label.numel(),
              "out_idx/out_label mismatch");
  int64_t G = in_off.numel() - 1;
  TORCH_CHECK(out_off.numel() - 1 == G, "group count mismatch");
  float *igq = nullptr, *ogq = nullptr;
  if (use_adagrad) {
    check_f32(in_gsq, "in_gsq"); check_f32(out_gsq, "out_gsq");
    TORCH_CHECK(in_gsq.sizes() == in_emb.sizes() &&
                out_gsq.sizes() == out_emb.sizes(), "gsq shape mismatch");
    igq = in_gsq.data_ptr<float>();
    ogq = out_gsq.data_ptr<float>();
  }
  mv_launch_w2v(in_emb.data_ptr<float>(), out_emb.data_ptr<float>(), igq, ogq,
                in_idx.data_ptr<int64_t>(), in_off.data_ptr<int>(),
                out_idx.data_ptr<int64_t>(), out_label.data_ptr<float>(),
                out_off.data_ptr<int>(), (float)lr, G, in_emb.size(1),
                use_adagrad ? 1 : 0, use_atomic ? 1 : 0, cur_stream());
}

void w2v_train_ns(torch::Tensor in_emb, torch::Tensor out_emb,
                  torch::Tensor in_gsq, torch::Tensor out_gsq,
                  torch::Tensor in_idx,
                  c10::optional<torch::Tensor> in_off_opt,
                  torch::Tensor centers, torch::Tensor pool, int64_t neg,
                  int64_t seed, double lr, bool use_adagrad,
                  bool use_atomic) {
  check_f32(in_emb, "in_emb"); check_f32(out_emb, "out_emb");
  TORCH_CHECK(in_emb.dim() == 2 && out_emb.dim() == 2, "emb must be 2-D");
  TORCH_CHECK(in_emb.size(1) == out_emb.size(1), "dim mismatch");
  TORCH_CHECK(in_emb.size(1) <= 2048, "w2v kernel supports dim <= 2048");
  TORCH_CHECK(in_idx.scalar_type() == torch::kInt64 &&
              centers.scalar_type() == torch::kInt64 &&
              pool.scalar_type() == torch::kInt64, "ids must be int64");
  // the kernel takes these as raw device pointers
  check_dev(in_idx, "in_idx", torch::kInt64);
  check_dev(centers, "centers", torch::kInt64);
  check_dev(pool, "pool", torch::kInt64);
  TORCH_CHECK(neg >= 0, "neg must be >= 0");
  const int* in_off_ptr = nullptr;
  if (in_off_opt.has_value()) {
    TORCH_CHECK(in_off_opt->scalar_type() == torch::kInt32,
                "offsets must be int32");
    check_dev(*in_off_opt, "in_off", torch::kInt32);
    TORCH_CHECK(in_off_opt->numel() >= 1, "in_off needs at least one entry");
    TORCH_CHECK(in_off_opt->numel() - 1 == centers.numel(),
                "centers/group count mismatch");
    in_off_ptr = in_off_opt->data_ptr<int>();
  } else {
    // skip-gram: one input per group (in_idx[g] is group g's context)
    TORCH_CHECK(in_idx.numel() == centers.numel(),
                "skip-gram in_idx/centers mismatch");
  }
  TORCH_CHECK(pool.numel() > 0, "empty negative pool");
  int64_t G = centers.numel();
  float *igq = nullptr, *ogq = nullptr;
  if (use_adagrad) {
    check_f32(in_gsq, "in_gsq"); check_f32(out_gsq, "out_gsq");
    TORCH_CHECK(in_gsq.sizes() == in_emb.sizes() &&
                out_gsq.sizes() == out_emb.sizes(), "gsq shape mismatch");
    igq = in_gsq.data_ptr<float>();
    ogq = out_gsq.data_ptr<float>();
  }
  mv_launch_w2v_ns(in_emb.data_ptr<float>(), out_emb.data_ptr<float>(), igq,
                   ogq, in_idx.data_ptr<int64_t>(), in_off_ptr,
                   centers.data_ptr<int64_t>(), pool.data_ptr<int64_t>(),
                   pool.numel(), (int)neg, (uint64_t)seed, (float)lr, G,
                   in_emb.size(1), use_adagrad ? 1 : 0, use_atomic ? 1 : 0,
                   cur_stream());
}

// The sparse logreg kernels read keys and ptr through raw device pointers:
// both on the GPU and contiguous, one value per key, ptr with its leading
// entry. Returns the batch size. Key range and ptr's monotonicity lie in
// device memory and are not checked (that would take a sync).
int64_t check_csr(const torch::Tensor& keys, const torch::Tensor& vals,
                  const torch::Tensor& ptr) {
  TORCH_CHECK(keys.scalar_type() == torch::kInt64 && keys.is_cuda() &&
              keys.is_contiguous(), "keys must be contiguous int64 on GPU");
  TORCH_CHECK(ptr.scalar_type() == torch::kInt32 && ptr.is_cuda() &&
              ptr.is_contiguous(), "ptr must be contiguous int32 on GPU");
  TORCH_CHECK(ptr.numel() >= 1, "ptr needs at least one entry");
  TORCH_CHECK(keys.numel() == vals.numel(), "keys/vals mismatch");
  return ptr.numel() - 1;
}

// The optional per-sample weights of the logreg kernels: fp32, on the GPU,
// contiguous, one per sample. Returns their pointer, or null without any.
const float* opt_weights(const c10::optional<torch::Tensor>& wts, int64_t B) {
  if (!wts.has_value()) return nullptr;
  check_f32(*wts, "wts");
  TORCH_CHECK(wts->numel() == B, "weights size mismatch");
  return f32(*wts);
}

// K lies within the class counts the kernels are instantiated for, and the
// table holds whole rows: K weights (softmax), 2*K state values (FTRL).
void check_softmax_k(const torch::Tensor& w, int64_t K) {
  TORCH_CHECK(K >= 2 && K <= 64,
              "fused softmax supports 2..64 classes (got ", K, ")");
  TORCH_CHECK(w.numel() % K == 0, "w must hold whole rows of K");
}
void check_ftrl_k(const torch::Tensor& zn, int64_t K) {
  TORCH_CHECK(K >= 1 && K <= 32,
              "fused FTRL supports 1..32 outputs (got ", K, ")");
  TORCH_CHECK(zn.numel() % (2 * K) == 0,
              "zn must hold whole rows of 2*K (z | n)");
}

void lr_sigmoid_forward(torch::Tensor w, torch::Tensor keys,
                        torch::Tensor vals, torch::Tensor ptr,
                        torch::Tensor labels,
                        c10::optional<torch::Tensor> wts,
                        torch::Tensor err, torch::Tensor loss) {
  check_f32(w, "w"); check_f32(vals, "vals"); check_f32(labels, "labels");
  check_f32(err, "err"); check_f32(loss, "loss");
  int64_t B = check_csr(keys, vals, ptr);
  TORCH_CHECK(labels.numel() == B && err.numel() == B && loss.numel() == B,
              "batch size mismatch");
  mv_launch_lr_sigmoid_fwd(f32(w), keys.data_ptr<int64_t>(), f32(vals),
                           ptr.data_ptr<int>(), f32(labels),
                           opt_weights(wts, B), f32(err), f32(loss), B,
                           cur_stream());
}

void lr_sigmoid_scatter(torch::Tensor w, torch::Tensor keys,
                        torch::Tensor vals, torch::Tensor ptr,
                        torch::Tensor err, double lr, int64_t reg_type,
                        double reg_coef) {
  check_f32(w, "w"); check_f32(vals, "vals"); check_f32(err, "err");
  int64_t B = check_csr(keys, vals, ptr);
  TORCH_CHECK(err.numel() == B, "err size mismatch");
  mv_launch_lr_sigmoid_scatter(f32(w), keys.data_ptr<int64_t>(), f32(vals),
                               ptr.data_ptr<int>(), f32(err), (float)lr,
                               (int)reg_type, (float)reg_coef, B,
                               cur_stream());
}

void lr_softmax_forward(torch::Tensor w, torch::Tensor keys,
                        torch::Tensor vals, torch::Tensor ptr,
                        torch::Tensor labels,
                        c10::optional<torch::Tensor> wts,
                        torch::Tensor err, torch::Tensor loss, int64_t K) {
  check_f32(w, "w"); check_f32(vals, "vals"); check_f32(labels, "labels");
  check_f32(err, "err"); check_f32(loss, "loss");
  check_softmax_k(w, K);
  int64_t B = check_csr(keys, vals, ptr);
  TORCH_CHECK(labels.numel() == B && loss.numel() == B, "batch mismatch");
  TORCH_CHECK(err.numel() == B * K, "err must be [B, K]");
  mv_launch_lr_softmax_fwd(f32(w), keys.data_ptr<int64_t>(), f32(vals),
                           ptr.data_ptr<int>(), f32(labels),
                           opt_weights(wts, B), f32(err), f32(loss), B, K,
                           cur_stream());
}

void lr_softmax_scatter(torch::Tensor w, torch::Tensor keys,
                        torch::Tensor vals, torch::Tensor ptr,
                        torch::Tensor err, double lr, int64_t reg_type,
                        double reg_coef, int64_t K) {
  check_f32(w, "w"); check_f32(vals, "vals"); check_f32(err, "err");
  check_softmax_k(w, K);
  int64_t B = check_csr(keys, vals, ptr);
  TORCH_CHECK(err.numel() == B * K, "err must be [B, K]");
  mv_launch_lr_softmax_scatter(f32(w), keys.data_ptr<int64_t>(), f32(vals),
                               ptr.data_ptr<int>(), f32(err), (float)lr,
                               (int)reg_type, (float)reg_coef, B, K,
                               cur_stream());
}

void lr_ftrl_forward(torch::Tensor zn, torch::Tensor keys,
                     torch::Tensor vals, torch::Tensor ptr,
                     torch::Tensor labels, c10::optional<torch::Tensor> wts,
                     torch::Tensor err, torch::Tensor loss, double alpha,
                     double beta, double l1, double l2, int64_t K) {
  check_f32(zn, "zn"); check_f32(vals, "vals"); check_f32(labels, "labels");
  check_f32(err, "err"); check_f32(loss, "loss");
  check_ftrl_k(zn, K);
  int64_t B = check_csr(keys, vals, ptr);
  TORCH_CHECK(labels.numel() == B && loss.numel() == B, "batch mismatch");
  TORCH_CHECK(err.numel() == B * K, "err must be [B, K]");
  mv_launch_lr_ftrl_fwd(f32(zn), keys.data_ptr<int64_t>(), f32(vals),
                        ptr.data_ptr<int>(), f32(labels), opt_weights(wts, B),
                        f32(err), f32(loss), (float)(1.0 / alpha),
                        (float)beta, (float)l1, (float)l2, B, K,
                        cur_stream());
}

void lr_dense_post(torch::Tensor logits, torch::Tensor labels,
                   c10::optional<torch::Tensor> wts, torch::Tensor loss_acc,
                   double inv_b) {
  check_f32(logits, "logits"); check_f32(labels, "labels");
  check_f32(loss_acc, "loss_acc");
  int64_t B = labels.numel();
  TORCH_CHECK(B > 0 && logits.numel() % B == 0,
              "logits/labels batch mismatch");
  int64_t K = logits.numel() / B;
  TORCH_CHECK(K >= 1 && K <= 64,
              "fused dense post supports 1..64 classes (got ", K, ")");
  TORCH_CHECK(loss_acc.numel() == 1, "loss_acc must be a scalar");
  mv_launch_lr_dense_post(f32(logits), f32(labels), opt_weights(wts, B),
                          f32(loss_acc), (float)inv_b, B, K, cur_stream());
}

bool lr_dense_fwd(torch::Tensor x, torch::Tensor w, torch::Tensor labels,
                  c10::optional<torch::Tensor> wts, torch::Tensor diff,
                  torch::Tensor loss_acc, double inv_b, bool nt) {
  check_f32(x, "x"); check_f32(w, "w"); check_f32(labels, "labels");
  check_f32(diff, "diff"); check_f32(loss_acc, "loss_acc");
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && x.size(1) == w.size(0),
              "x [B,d] and w [d,K] shape mismatch");
  TORCH_CHECK(x.is_contiguous() && w.is_contiguous(), "x/w must be "
              "contiguous");
  int64_t B = x.size(0), d = x.size(1), K = w.size(1);
  TORCH_CHECK(labels.numel() == B, "labels batch mismatch");
  TORCH_CHECK(diff.numel() == B * K, "diff must be [B, K]");
  TORCH_CHECK(loss_acc.numel() == 1, "loss_acc must be a scalar");
  return mv_launch_lr_dense_fwd(f32(x), f32(w), f32(labels),
                                opt_weights(wts, B), f32(diff), f32(loss_acc),
                                (float)inv_b, B, d, K, nt ? 1 : 0,
                                cur_stream()) != 0;
}

void lr_ftrl_scatter(torch::Tensor zn, torch::Tensor keys,
                     torch::Tensor vals, torch::Tensor ptr,
                     torch::Tensor err, double alpha, double beta, double l1,
                     double l2, int64_t K) {
  check_f32(zn, "zn"); check_f32(vals, "vals"); check_f32(err, "err");
  check_ftrl_k(zn, K);
  int64_t B = check_csr(keys, vals, ptr);
  TORCH_CHECK(err.numel() == B * K, "err must be [B, K]");
  mv_launch_lr_ftrl_scatter(f32(zn), keys.data_ptr<int64_t>(), f32(vals),
                            ptr.data_ptr<int>(), f32(err),
                            (float)(1.0 / alpha), (float)beta, (float)l1,
                            (float)l2, B, K, cur_stream());
}

// (scores [Q,k] fp32, ids [Q,k] int64, global) of the k nearest shard rows
// per query, or None when the launcher refuses (the caller takes its torch
// path). Slots past the shard's rows are (-inf, INT64_MAX).
c10::optional<std::tuple<torch::Tensor, torch::Tensor>> row_topk(
    torch::Tensor shard, torch::Tensor queries, int64_t k, bool cosine,
    int64_t row_offset) {
  check_f32(shard, "shard"); check_f32(queries, "queries");
  TORCH_CHECK(shard.dim() == 2 && queries.dim() == 2 &&
              shard.size(1) == queries.size(1),
              "shard [R,cols] and queries [Q,cols] shape mismatch");
  TORCH_CHECK(shard.device() == queries.device(),
              "shard and queries must share a device");
  TORCH_CHECK(k >= 1 && k <= 64, "k must be in 1..64 (got ", k, ")");
  int64_t R = shard.size(0), cols = shard.size(1), Q = queries.size(0);
  int waves = 0;
  int chunk = Q ? mv_row_topk_plan(R, cols, Q, &waves) : 1;
  if (!chunk) return c10::nullopt;
  auto iopt = shard.options().dtype(torch::kInt64);
  if (!Q || !R)
    return std::make_tuple(
        torch::full({Q, k}, -std::numeric_limits<float>::infinity(),
                    shard.options()),
        torch::full({Q, k}, std::numeric_limits<int64_t>::max(), iopt));
  // the merge writes every one of the Q*k slots
  auto scores = torch::empty({Q, k}, shard.options());
  auto ids = torch::empty({Q, k}, iopt);
  auto part_s = torch::empty({(int64_t)chunk * waves * k}, shard.options());
  auto part_i = torch::empty({(int64_t)chunk * waves * k},
                             shard.options().dtype(torch::kInt32));
  int ok = mv_launch_row_topk(f32(shard), f32(queries), f32(part_s),
                              part_i.data_ptr<int>(), f32(scores),
                              ids.data_ptr<int64_t>(), R, cols, Q, k,
                              cosine ? 1 : 0, row_offset, cur_stream());
  TORCH_CHECK(ok, "row_topk: launcher refused a planned request");
  return std::make_tuple(scores, ids);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  // fp32 shards also take a bf16 delta / vals / out (the bf16 wire format)
  // The whole-shard updaters take a trailing reverse=False: True sweeps
  // the arrays from the top down. It is a performance hint (alternate it
  // from pass to pass and the Infinity Cache serves the turning end); the
  // result is bit for bit the same either way.
  auto rev = py::arg("reverse") = false;
  auto data = py::arg("data"), delta = py::arg("delta"), out = py::arg("out");
  m.def("add_inplace", &add_inplace, "K1: data += delta (fp32, fused)", data,
        delta, rev);
  m.def("nt_copy", &nt_copy,
        "K7: non-temporal streaming copy (a bf16 dst narrows)");
  m.def("sgd_update", &sgd_update, "K2: data -= delta", data, delta, rev);
  m.def("momentum_update", &momentum_update, "K3: fused momentum update",
        data, py::arg("m"), delta, py::arg("mu"), rev);
  m.def("adagrad_update", &adagrad_update, "K4: fused adagrad update", data,
        py::arg("gsq"), delta, py::arg("lr"), py::arg("rho"), py::arg("eps"),
        rev);
  m.def("momentum_copy_update", &momentum_copy_update,
        "fused momentum Add+Get", data, py::arg("m"), delta, out,
        py::arg("mu"), rev);
  m.def("adagrad_copy_update", &adagrad_copy_update,
        "fused adagrad Add+Get", data, py::arg("gsq"), delta, out,
        py::arg("lr"), py::arg("rho"), py::arg("eps"), rev);
  m.def("dcasgd_copy_update", &dcasgd_copy_update,
        "fused dcasgd Add+Get", data, py::arg("bak"), delta, out,
        py::arg("lr"), py::arg("lambda_"), rev);
  m.def("dcasgda_copy_update", &dcasgda_copy_update,
        "fused dcasgda Add+Get", data, py::arg("bak"), py::arg("msq"), delta,
        out, py::arg("lr"), py::arg("lambda_"), py::arg("rho"),
        py::arg("eps"), rev);
  m.def("sgd_copy_update", &sgd_copy_update,
        "fused Add+Get: data (+/-)= delta; out = data (saves the Get's "
        "shard re-read at N=1)", data, delta, out, py::arg("sign"), rev);
  m.def("dcasgd_update", &dcasgd_update,
        "DC-ASGD: delay-compensated update with per-worker backup", data,
        py::arg("bak"), delta, py::arg("lr"), py::arg("lambda_"), rev);
  m.def("dcasgda_update", &dcasgda_update,
        "DC-ASGD-a: adaptive lambda via mean-square of gradients", data,
        py::arg("bak"), py::arg("msq"), delta, py::arg("lr"),
        py::arg("lambda_"), py::arg("rho"), py::arg("eps"), rev);
  m.def("adam_update", &adam_update,
        "fused Adam/AdamW step (fp32, fp64); step = lr/(1-b1^t), "
        "rbc2 = 1/sqrt(1-b2^t), decay = 1-lr*wd",
        py::arg("data"), py::arg("m"), py::arg("v"), py::arg("delta"),
        py::arg("b1"), py::arg("b2"), py::arg("step"), py::arg("rbc2"),
        py::arg("decay"), py::arg("eps"), rev);
  m.def("adam_copy_update", &adam_copy_update, "fused adam Add+Get",
        py::arg("data"), py::arg("m"), py::arg("v"), py::arg("delta"),
        py::arg("out"), py::arg("b1"), py::arg("b2"), py::arg("step"),
        py::arg("rbc2"), py::arg("decay"), py::arg("eps"), rev);
  m.def("onebit_encode", &onebit_encode,
        "1-bit wire: payload = code(residual + delta), residual = the error",
        py::arg("delta"), py::arg("residual"), py::arg("payload"));
  m.def("onebit_decode_sum", &onebit_decode_sum,
        "1-bit wire: out = sum over nparts payloads of their decoded values",
        py::arg("out"), py::arg("payloads"), py::arg("nparts"));
  m.def("row_gather", &row_gather,
        "K6: out[i] = shard[rows[i]]; dtype=torch.bfloat16 narrows",
        py::arg("shard"), py::arg("rows"), py::arg("dtype") = py::none());
  m.def("row_gather_out", &row_gather_out, "K6 (preallocated out)");
  m.def("row_scatter_add", &row_scatter_add,
        "K5: shard[rows[i]] += sign*vals[i] (atomic; assume_unique=True "
        "uses plain stores)", py::arg("shard"), py::arg("rows"),
        py::arg("vals"), py::arg("sign"), py::arg("assume_unique") = false);
  m.def("lr_sigmoid_forward", &lr_sigmoid_forward,
        "K13 fused: per-sample CSR dot + sigmoid + error/loss");
  m.def("lr_sigmoid_scatter", &lr_sigmoid_scatter,
        "K14 fused: w[keys] -= lr*(vals*err + reg), atomic");
  m.def("lr_softmax_forward", &lr_softmax_forward,
        "K13 softmax fused: per-sample CSR K-class logits + softmax + "
        "err/loss (objective.cpp:193-230)");
  m.def("lr_softmax_scatter", &lr_softmax_scatter,
        "K14 softmax fused: w[key*K+k] -= lr*(val*err_k + reg), atomic");
  m.def("lr_dense_fwd", &lr_dense_fwd,
        "Dense-mode fused forward: X@W + softmax/sigmoid diff + loss in "
        "one kernel, W LDS-staged; returns False when d*K exceeds the "
        "LDS budget (caller uses the GEMM + lr_dense_post path)",
        py::arg("x"), py::arg("w"), py::arg("labels"), py::arg("wts"),
        py::arg("diff"), py::arg("loss_acc"), py::arg("inv_b"),
        py::arg("nt") = true);
  m.def("lr_dense_post", &lr_dense_post,
        "Dense-mode fused post-GEMM: logits -> softmax/sigmoid diff in "
        "place + atomic mean-loss accumulate (objective.cpp:193-230 "
        "dense branch)");
  m.def("lr_ftrl_forward", &lr_ftrl_forward,
        "FTRL fused forward: reconstruct w from (z|n), sigmoid, err/loss "
        "(objective.cpp:250-345)");
  m.def("lr_ftrl_scatter", &lr_ftrl_scatter,
        "FTRL fused z/n state update (updater.cpp:79-101 applied to the "
        "local chunk buffer)");
  m.def("row_scatter_adagrad", &row_scatter_adagrad,
        "K15: keyed adagrad update on owned shard rows "
        "(assume_unique=True uses plain stores)",
        py::arg("shard"), py::arg("gsq"), py::arg("rows"), py::arg("vals"),
        py::arg("lr"), py::arg("rho"), py::arg("eps"),
        py::arg("assume_unique") = false);
  m.def("row_momentum_update", &row_momentum_update,
        "keyed momentum: sum value rows per row id (equal ids adjacent in "
        "rows; perm maps list position to vals row), one step per row",
        py::arg("shard"), py::arg("m"), py::arg("rows"), py::arg("vals"),
        py::arg("mu"), py::arg("perm") = py::none());
  m.def("row_dcasgd_update", &row_dcasgd_update,
        "keyed DC-ASGD, same row/perm contract as row_momentum_update",
        py::arg("shard"), py::arg("bak"), py::arg("rows"), py::arg("vals"),
        py::arg("lr"), py::arg("lam"), py::arg("perm") = py::none());
  m.def("row_dcasgda_update", &row_dcasgda_update,
        "keyed DC-ASGD-a, same row/perm contract as row_momentum_update",
        py::arg("shard"), py::arg("bak"), py::arg("msq"), py::arg("rows"),
        py::arg("vals"), py::arg("lr"), py::arg("lam"), py::arg("rho"),
        py::arg("eps"), py::arg("perm") = py::none());
  m.def("row_adam_update", &row_adam_update,
        "keyed Adam, same row/perm contract as row_momentum_update",
        py::arg("shard"), py::arg("m"), py::arg("v"), py::arg("rows"),
        py::arg("vals"), py::arg("b1"), py::arg("b2"), py::arg("step"),
        py::arg("rbc2"), py::arg("decay"), py::arg("eps"),
        py::arg("perm") = py::none());
  m.def("row_topk", &row_topk,
        "nearest rows: (scores [Q,k], global ids [Q,k]) of the k best shard "
        "rows per query, dot or cosine; None when one query exceeds the LDS "
        "budget (caller uses torch ops)",
        py::arg("shard"), py::arg("queries"), py::arg("k"),
        py::arg("cosine"), py::arg("row_offset") = 0);
  m.def("w2v_train", &w2v_train,
        "K9-K11: fused word2vec block training (skip-gram/CBOW, NS/HS, "
        "optional adagrad)");
  m.def("w2v_train_ns", &w2v_train_ns,
        "K9-K11 NS fast path: negatives generated in-kernel from the "
        "per-block pool (reference LCG scheme)");
}
