// Exhaustive check of the bf16 narrowing used by ops/csrc/kernels.hip:
// gfx950's packed convert (what `(__bf16)x` compiles to, v_cvt_pk_bf16_f32)
// against the integer round-to-nearest-even form, which is torch's
// .to(torch.bfloat16), over all 2^32 fp32 bit patterns.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/probe_bf16_cvt.hip \
//         -o tools/probe_bf16_cvt.bin && tools/probe_bf16_cvt.bin
//
// Prints the number of non-NaN inputs on which the two differ (and the
// first such pattern) and the number of NaN inputs whose convert is not a
// NaN; exits 1 unless both are 0. Recorded in profiles/bf16_wire.md.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>

__device__ __forceinline__ uint16_t narrow_int(float f) {
  uint32_t u = __builtin_bit_cast(uint32_t, f);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0x7FC0;
  return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ uint16_t narrow_hw(float f) {
  return __builtin_bit_cast(uint16_t, (__bf16)f);
}

// res: [non-NaN mismatches, NaN inputs not NaN out, first mismatching input]
__global__ void k_compare(unsigned long long* res) {
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < (1ull << 32); i += stride) {
    uint32_t u = (uint32_t)i;
    float f = __builtin_bit_cast(float, u);
    uint16_t a = narrow_int(f), b = narrow_hw(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) {
      if ((b & 0x7FFF) <= 0x7F80) atomicAdd(&res[1], 1ull);
    } else if (a != b) {
      if (atomicAdd(&res[0], 1ull) == 0) res[2] = u;
    }
  }
}

int main() {
  unsigned long long* d;
  unsigned long long h[3] = {0, 0, 0};
  if (hipMalloc(&d, sizeof(h)) != hipSuccess) return 2;
  if (hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice) != hipSuccess)
    return 2;
  k_compare<<<2048, 256>>>(d);
  if (hipDeviceSynchronize() != hipSuccess) return 3;
  if (hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess)
    return 2;
  printf("non-NaN mismatches %llu (first pattern 0x%08llx), "
         "NaN inputs not NaN out %llu\n", h[0], h[2], h[1]);
  return (h[0] || h[1]) ? 1 : 0;
}
