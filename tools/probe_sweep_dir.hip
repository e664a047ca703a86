// Sweep-direction probe: does alternating the direction of the
// elementwise pass from launch to launch let the 256 MiB Infinity Cache
// serve the lines the previous launch touched last?
//
// Headline shape (1e6 x 128 fp32): the 4-stream fused sgd+copy body (read
// shard, read delta, write shard, write Get buffer = 2.0 GB nominal per
// launch). Variants: forward-only, reverse-only, alternating, alternating
// with the delta rotated over three buffers ("rot": the delta never hits,
// the real-use number), block/grid geometry, which accesses are plain and
// which non-temporal, the two index mirrors, and the 3-stream / 6-stream
// bodies. Two one-stream
// kernels (read-only, write-only) separate read hits from dirty-line
// retention.
//
// Every variant is timed REPS times (LAUNCHES launches per timing, event
// timed), round-robin over the variants so that drift hits all alike.
// Prints each repeat, the median and the spread (max - min).
//
//   hipcc -O3 --offload-arch=gfx950 tools/probe_sweep_dir.hip -o tools/probe_sweep_dir.bin
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

typedef float v4f __attribute__((ext_vector_type(4)));
#define NT_L(p) __builtin_nontemporal_load(p)
#define NT_S(p, v) __builtin_nontemporal_store(v, p)

#define CHECK(x)                                                        \
  do {                                                                  \
    hipError_t e_ = (x);                                                \
    if (e_ != hipSuccess) {                                             \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__,                 \
              hipGetErrorString(e_));                                   \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

// MAP 0: mirror in units of one wave's 64 vectors (lanes still ascend
// inside the wave's 1 KiB); MAP 1: plain mirror (lanes descend).
// The loop runs over n rounded up to 64 so that whole waves mirror; a
// vector index past n is skipped.
template <int MAP>
static __device__ __forceinline__ long map_index(long i, long n_pad, int rev) {
  if (!rev) return i;
  if (MAP == 0) return n_pad - 64 - i + 2 * (long)(threadIdx.x & 63);
  return n_pad - 1 - i;
}

// today's kernel shape, no direction argument at all (the control for
// "the runtime flag costs nothing forward")
__global__ void sgd_copy_today(v4f* __restrict__ d, const v4f* __restrict__ g,
                               v4f* __restrict__ o, long n) {
  long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    v4f r = NT_L(&d[i]) - NT_L(&g[i]);
    NT_S(&d[i], r);
    NT_S(&o[i], r);
  }
}

// MASK says which accesses are plain (the rest are non-temporal):
// 1 shard load, 2 shard store, 4 Get-buffer store, 8 delta load
template <int MASK, int MAP>
__global__ void sgd_copy(v4f* __restrict__ d, const v4f* __restrict__ g,
                         v4f* __restrict__ o, long n, int rev) {
  long n_pad = (n + 63) & ~63L;
  long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_pad;
       i += stride) {
    long j = map_index<MAP>(i, n_pad, rev);
    if (j >= n) continue;
    v4f dv = (MASK & 1) ? d[j] : NT_L(&d[j]);
    v4f gv = (MASK & 8) ? g[j] : NT_L(&g[j]);
    v4f r = dv - gv;
    if (MASK & 2) d[j] = r; else NT_S(&d[j], r);
    if (MASK & 4) o[j] = r; else NT_S(&o[j], r);
  }
}

// 3-stream update body: read shard, read delta, write shard.
// MASK: 1 shard load plain, 2 shard store plain; the delta stays
// non-temporal
template <int MASK>
__global__ void sgd3(v4f* __restrict__ d, const v4f* __restrict__ g, long n,
                     int rev) {
  long n_pad = (n + 63) & ~63L;
  long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_pad;
       i += stride) {
    long j = map_index<0>(i, n_pad, rev);
    if (j >= n) continue;
    v4f r = ((MASK & 1) ? d[j] : NT_L(&d[j])) - NT_L(&g[j]);
    if (MASK & 2) d[j] = r; else NT_S(&d[j], r);
  }
}

// momentum-shaped fused body: read shard, state, delta; write shard,
// state, Get buffer (24 B/element). MASK: 1 shard load, 2 shard store,
// 4 state load, 8 state store are plain; delta and Get buffer stay
// non-temporal
template <int MASK>
__global__ void mom6(v4f* __restrict__ d, v4f* __restrict__ m,
                     const v4f* __restrict__ g, v4f* __restrict__ o, long n,
                     int rev) {
  long n_pad = (n + 63) & ~63L;
  long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_pad;
       i += stride) {
    long j = map_index<0>(i, n_pad, rev);
    if (j >= n) continue;
    v4f dv = (MASK & 1) ? d[j] : NT_L(&d[j]);
    v4f mv = (MASK & 4) ? m[j] : NT_L(&m[j]);
    v4f gv = NT_L(&g[j]);
    mv = 0.9f * mv + 0.1f * gv;
    dv -= mv;
    if (MASK & 8) m[j] = mv; else NT_S(&m[j], mv);
    if (MASK & 2) d[j] = dv; else NT_S(&d[j], dv);
    NT_S(&o[j], dv);
  }
}

// one stream, read only (the store never happens: the buffers hold zeros)
template <bool NT>
__global__ void rd1(const v4f* __restrict__ g, v4f* __restrict__ o, long n,
                    int rev) {
  long n_pad = (n + 63) & ~63L;
  long stride = (long)gridDim.x * blockDim.x;
  v4f acc = 0.0f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_pad;
       i += stride) {
    long j = map_index<0>(i, n_pad, rev);
    if (j >= n) continue;
    acc += NT ? NT_L(&g[j]) : g[j];
  }
  if (acc.x + acc.y + acc.z + acc.w == 12345.0f) o[threadIdx.x] = acc;
}

// one stream, write only
template <bool NT>
__global__ void wr1(v4f* __restrict__ o, long n, int rev, float val) {
  long n_pad = (n + 63) & ~63L;
  long stride = (long)gridDim.x * blockDim.x;
  v4f v = val;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_pad;
       i += stride) {
    long j = map_index<0>(i, n_pad, rev);
    if (j >= n) continue;
    if (NT) NT_S(&o[j], v); else o[j] = v;
  }
}

struct Variant {
  std::string name;
  double gbytes;                    // nominal bytes per launch / 1e9
  std::function<void(int)> launch;  // argument: launch index
  std::vector<float> ms;
};

int main(int argc, char** argv) {
  int reps = argc > 1 ? atoi(argv[1]) : 7;
  int launches = argc > 2 ? atoi(argv[2]) : 24;  // even: ends as it began
  long nf = 128L * 1000000;  // 1e6 x 128 fp32
  long n = nf / 4;
  size_t bytes = nf * 4;
  float *d, *m, *o, *g[3];
  CHECK(hipMalloc(&d, bytes)); CHECK(hipMalloc(&m, bytes));
  CHECK(hipMalloc(&o, bytes));
  CHECK(hipMemset(d, 0, bytes)); CHECK(hipMemset(m, 0, bytes));
  CHECK(hipMemset(o, 0, bytes));
  for (auto& p : g) { CHECK(hipMalloc(&p, bytes)); CHECK(hipMemset(p, 0, bytes)); }
  v4f *D = (v4f*)d, *M = (v4f*)m, *O = (v4f*)o;
  const v4f* G[3] = {(const v4f*)g[0], (const v4f*)g[1], (const v4f*)g[2]};
  double gb = (double)bytes / 1e9;

  std::vector<Variant> vs;
  auto add = [&](std::string name, double streams, std::function<void(int)> f) {
    vs.push_back({name, streams * gb, f, {}});
  };
  // mode: 0 forward, 1 reverse, 2 alternating; rot: the delta comes from
  // three buffers in turn, so that it never hits (real use)
  auto dir_of = [](int mode, int k) { return mode == 2 ? (k & 1) : mode; };
  const char* mode_name[3] = {"fwd", "rev", "alt"};
  auto label = [&](const char* body, const char* pol, int blk, int grd,
                   int mode, const char* extra) {
    char buf[96];
    snprintf(buf, sizeof buf, "%-5s %-22s %4dx%-4d %s %-18s", body, pol, blk,
             grd, mode_name[mode], extra);
    return std::string(buf);
  };
#define SGD4(MASK, MAP, POLNAME, BLK, GRD, MODE, ROT)                        \
  add(label("sgd4", POLNAME, BLK, GRD, MODE,                                 \
            MAP ? (ROT ? "plain-mirror rot" : "plain-mirror")                \
                : (ROT ? "rot" : "same-delta")),                             \
      4, [=](int k) {                                                        \
        sgd_copy<MASK, MAP><<<GRD, BLK>>>(D, G[ROT ? k % 3 : 0], O, n,       \
                                          dir_of(MODE, k));                  \
      })
  add(label("sgd4", "nt (today, no flag)", 1024, 768, 0, "same-delta"), 4,
      [=](int) { sgd_copy_today<<<768, 1024>>>(D, G[0], O, n); });
  // baseline, reverse-only, alternating; the two mirrors
  SGD4(0, 0, "nt", 1024, 768, 0, 0);
  SGD4(0, 0, "nt", 1024, 768, 0, 1);
  SGD4(0, 0, "nt", 1024, 768, 1, 0);
  SGD4(0, 1, "nt", 1024, 768, 1, 0);
  SGD4(0, 0, "nt", 1024, 768, 2, 0);
  SGD4(0, 0, "nt", 1024, 768, 2, 1);
  SGD4(0, 1, "nt", 1024, 768, 2, 0);
  SGD4(0, 1, "nt", 1024, 768, 2, 1);
  // geometry, all non-temporal: forward and alternating, delta rotated
#define GEO(MASK, POLNAME, BLK, GRD)                                         \
  SGD4(MASK, 0, POLNAME, BLK, GRD, 0, 1); SGD4(MASK, 0, POLNAME, BLK, GRD, 2, 1)
  GEO(0, "nt", 1024, 256); GEO(0, "nt", 1024, 512);
  GEO(0, "nt", 512, 512); GEO(0, "nt", 512, 768); GEO(0, "nt", 512, 1024);
  GEO(0, "nt", 256, 512); GEO(0, "nt", 256, 768); GEO(0, "nt", 256, 1024);
  GEO(0, "nt", 256, 2048);
  // geometry with the shard plain (load and store), rest non-temporal
  GEO(3, "shard-plain", 1024, 256); GEO(3, "shard-plain", 1024, 384);
  GEO(3, "shard-plain", 1024, 512); GEO(3, "shard-plain", 1024, 768);
  GEO(3, "shard-plain", 512, 512); GEO(3, "shard-plain", 512, 768);
  GEO(3, "shard-plain", 512, 1024);
  GEO(3, "shard-plain", 256, 512); GEO(3, "shard-plain", 256, 768);
  GEO(3, "shard-plain", 256, 1024); GEO(3, "shard-plain", 256, 2048);
  GEO(3, "shard-plain", 256, 384); GEO(3, "shard-plain", 256, 640);
  GEO(1, "shard-load-plain", 256, 384); GEO(1, "shard-load-plain", 256, 512);
  GEO(1, "shard-load-plain", 256, 640); GEO(1, "shard-load-plain", 256, 768);
  SGD4(3, 0, "shard-plain", 256, 768, 2, 0);
  SGD4(3, 0, "shard-plain", 256, 768, 1, 1);
  SGD4(3, 1, "shard-plain", 256, 768, 2, 1);
  SGD4(3, 1, "shard-plain", 1024, 512, 2, 1);
  SGD4(3, 0, "shard-plain", 1024, 512, 2, 0);
  SGD4(3, 0, "shard-plain", 1024, 512, 1, 1);
  // which access carries it, at 1024x512
  GEO(1, "shard-load-plain", 1024, 512);
  GEO(2, "shard-store-plain", 1024, 512);
  GEO(4, "out-plain", 1024, 512);
  GEO(7, "shard+out-plain", 1024, 512);
  GEO(11, "shard+delta-plain", 1024, 512);
  GEO(15, "all-plain", 1024, 512);
  GEO(15, "all-plain", 1024, 768);
  SGD4(7, 0, "shard+out-plain", 1024, 512, 2, 0);
  SGD4(15, 0, "all-plain", 1024, 512, 2, 0);
  // the other bodies
#define SGD3(PLAIN, POLNAME, BLK, GRD, MODE)                                 \
  add(label("sgd3", POLNAME, BLK, GRD, MODE, "rot"), 3, [=](int k) {         \
    sgd3<PLAIN><<<GRD, BLK>>>(D, G[k % 3], n, dir_of(MODE, k));              \
  })
#define MOM6(PLAIN, POLNAME, BLK, GRD, MODE)                                 \
  add(label("mom6", POLNAME, BLK, GRD, MODE, "rot"), 6, [=](int k) {         \
    mom6<PLAIN><<<GRD, BLK>>>(D, M, G[k % 3], O, n, dir_of(MODE, k));        \
  })
#define SGD3B(MASK, POLNAME, BLK, GRD)                                       \
  SGD3(MASK, POLNAME, BLK, GRD, 0); SGD3(MASK, POLNAME, BLK, GRD, 2)
#define MOM6B(MASK, POLNAME, BLK, GRD)                                       \
  MOM6(MASK, POLNAME, BLK, GRD, 0); MOM6(MASK, POLNAME, BLK, GRD, 2)
  SGD3B(0, "nt", 256, 768);
  SGD3B(3, "shard-plain", 256, 512); SGD3B(3, "shard-plain", 256, 768);
  SGD3B(3, "shard-plain", 256, 1024); SGD3B(3, "shard-plain", 1024, 512);
  SGD3B(1, "shard-load-plain", 256, 512); SGD3B(1, "shard-load-plain", 256, 768);
  MOM6B(0, "nt", 1024, 768); MOM6B(0, "nt", 1024, 512); MOM6B(0, "nt", 256, 768);
  MOM6B(15, "shard+state-plain", 1024, 768);
  MOM6B(15, "shard+state-plain", 1024, 512);
  MOM6B(15, "shard+state-plain", 256, 512);
  MOM6B(15, "shard+state-plain", 256, 768);
  MOM6B(5, "shard+state-load-plain", 256, 512);
  MOM6B(5, "shard+state-load-plain", 256, 768);
  MOM6B(3, "shard-plain", 256, 768);
  MOM6B(1, "shard-load-plain", 256, 768);
  // one stream: read hits and dirty-line retention on their own
#define ONE(KERN, NTFLAG, POLNAME, MODE, ...)                                \
  add(label(#KERN, POLNAME, 256, 1024, MODE, ""), 1, [=](int k) {            \
    KERN<NTFLAG><<<1024, 256>>>(__VA_ARGS__);                                \
  })
  ONE(rd1, true, "nt", 0, G[0], O, n, 0);
  ONE(rd1, true, "nt", 2, G[0], O, n, k & 1);
  ONE(rd1, false, "plain", 0, G[0], O, n, 0);
  ONE(rd1, false, "plain", 2, G[0], O, n, k & 1);
  ONE(wr1, true, "nt", 0, O, n, 0, 0.0f);
  ONE(wr1, true, "nt", 2, O, n, k & 1, 0.0f);
  ONE(wr1, false, "plain", 0, O, n, 0, 0.0f);
  ONE(wr1, false, "plain", 2, O, n, k & 1, 0.0f);

  hipEvent_t a, b;
  CHECK(hipEventCreate(&a)); CHECK(hipEventCreate(&b));
  for (int r = 0; r < reps; ++r) {
    for (auto& v : vs) {
      // two untimed launches bring the cache to the variant's steady state
      v.launch(launches - 2); v.launch(launches - 1);
      CHECK(hipDeviceSynchronize());
      CHECK(hipEventRecord(a));
      for (int k = 0; k < launches; ++k) v.launch(k);
      CHECK(hipEventRecord(b));
      CHECK(hipEventSynchronize(b));
      CHECK(hipGetLastError());
      float ms;
      CHECK(hipEventElapsedTime(&ms, a, b));
      v.ms.push_back(ms / launches);
    }
  }
  printf("%d repeats x %d launches, ms per launch; TB/s of the nominal "
         "bytes at the median\n", reps, launches);
  for (auto& v : vs) {
    std::vector<float> s = v.ms;
    std::sort(s.begin(), s.end());
    float med = s[s.size() / 2];
    printf("%s  med %.4f  min %.4f  max %.4f  spread %.4f  %.2f TB/s  |",
           v.name.c_str(), med, s.front(), s.back(), s.back() - s.front(),
           v.gbytes / med);
    for (float x : v.ms) printf(" %.4f", x);
    printf("\n");
  }
  return 0;
}
