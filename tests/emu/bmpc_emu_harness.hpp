// tests/emu/bmpc_emu_harness.hpp -- TEST INFRASTRUCTURE: what lets the HIP kernels' sources run on the CPU, one std::thread
// per lane of a workgroup, so that the kernels' logic (thread map, LDS exchanges, barriers, cross-lane swaps) can be checked
// against the oracle without a GPU.  Nothing of the product loads this; it is not a CPU path of the library (libbmpc.so
// has none) and it is orders of magnitude too slow to be one.  The entries over it are in bmpc_emu.cpp.
//
// How: the kernel files are included as plain C++ after this one.  __shared__ becomes a function-local static (one image
// shared by the lane threads; workgroups run one after another), threadIdx / blockIdx are thread-local, __syncthreads
// is a std::barrier over the workgroup, and the cross-lane operations (pair swap, wave maximum, row broadcast, MFMA,
// lane_read) go through a shared array between two barriers -- which demands what the GPU code must guarantee anyway:
// every lane of the workgroup reaches every barrier and every cross-lane operation.
#ifndef BMPC_EMU_HARNESS_HPP
#define BMPC_EMU_HARNESS_HPP
#include <atomic>
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#define BMPC_EMU 1
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(...)
#define __restrict__

struct emu_idx { int x; };
static thread_local emu_idx threadIdx, blockIdx;
static std::barrier<>* g_bar = nullptr;
static int g_or[2];
// byte the LDS image starts from (all-ones = NaNs; BMPC_EMU_POISON tries other leftovers: a result that changes with
// it reads LDS that nobody wrote)
static int g_poison = 0xFF;
static int g_swap[1024];
static std::atomic<unsigned> g_pair[512];
static std::barrier<>* g_wbar[16] = {};      // one per wave
static unsigned g_red[1024];

static inline void __syncthreads() { g_bar->arrive_and_wait(); }
static inline int __syncthreads_or(int v) {
  // two slots so that back-to-back calls cannot race on the reset
  static thread_local int phase = 0;
  int* slot = &g_or[phase & 1];
  __syncthreads();
  if (v) __atomic_store_n(slot, 1, __ATOMIC_RELAXED);
  __syncthreads();
  const int r = __atomic_load_n(slot, __ATOMIC_RELAXED);
  __syncthreads();
  if (threadIdx.x == 0) *slot = 0;
  ++phase;
  return r;
}
static inline long long clock64() { return 0; }
struct float2 { float x, y; };
struct alignas(16) float4 { float x, y, z, w; };
struct alignas(16) double2 { double x, y; };
static inline int __float_as_int(float f) { int i; std::memcpy(&i, &f, 4); return i; }
static inline float __int_as_float(int i) { float f; std::memcpy(&f, &i, 4); return f; }
static inline unsigned __float_as_uint(float f) { unsigned i; std::memcpy(&i, &f, 4); return i; }
static inline float __uint_as_float(unsigned i) { float f; std::memcpy(&f, &i, 4); return f; }
static inline int __double2loint(double d) { long long i; std::memcpy(&i, &d, 8); return (int)(i & 0xffffffffLL); }
static inline int __double2hiint(double d) { long long i; std::memcpy(&i, &d, 8); return (int)(i >> 32); }
static inline double __hiloint2double(int hi, int lo) {
  const long long i = ((long long)hi << 32) | (unsigned)lo;
  double d; std::memcpy(&d, &i, 8); return d;
}
using std::fma; using std::fmin; using std::fmax; using std::fabs;

namespace bmpc {
static inline double rcp_approx(double x) { return 1.0 / x; }
static inline float rcp_approx(float x) { return 1.0f / x; }
static inline float rsq_approx(float x) { return 1.0f / std::sqrt(x); }
static inline void sync_workgroup() { __syncthreads(); }
static inline int sync_workgroup_or(int v) { return __syncthreads_or(v); }
// The cross-lane operations synchronise only the lanes that take part (the pair, the wave), as on the GPU, where a
// DPP exchange is no barrier: an LDS hand-over that relied on one would be a race there, and is one here (visible
// to ThreadSanitizer: tests/emu/tsan.sh).
static inline void pair_sync() {
  // two-party barrier of lanes (l, l ^ 1): the counter goes 2 k -> 2 k + 2 per rendezvous
  std::atomic<unsigned>& cnt = g_pair[threadIdx.x >> 1];
  const unsigned old = cnt.fetch_add(1, std::memory_order_acq_rel);
  const unsigned target = (old | 1u) + 1u;
  while (cnt.load(std::memory_order_acquire) < target) std::this_thread::yield();
}
static inline int pair_swap_i(int v) {
  g_swap[threadIdx.x] = v;
  pair_sync();
  const int r = g_swap[threadIdx.x ^ 1];
  pair_sync();
  return r;
}
static inline unsigned wave_umax(unsigned v) {          // maximum over the lane's wave (64 consecutive lanes)
  std::barrier<>& wb = *g_wbar[threadIdx.x >> 6];
  g_red[threadIdx.x] = v;
  wb.arrive_and_wait();
  unsigned m = 0;
  const int w0 = threadIdx.x & ~63;
  for (int i = 0; i < 64; ++i) m = g_red[w0 + i] > m ? g_red[w0 + i] : m;
  wb.arrive_and_wait();
  return m;
}
static inline unsigned row0_umax(unsigned v) {          // maximum over lanes 0 .. 15 of the lane's wave, to every lane of it
  std::barrier<>& wb = *g_wbar[threadIdx.x >> 6];
  g_red[threadIdx.x] = v;
  wb.arrive_and_wait();
  unsigned m = 0;
  const int w0 = threadIdx.x & ~63;
  for (int i = 0; i < 16; ++i) m = g_red[w0 + i] > m ? g_red[w0 + i] : m;
  wb.arrive_and_wait();
  return m;
}
// sum over the lane's wave in the order of the GPU's DPP tree (bmpc_kernels.hip wave_sum): inclusive scan inside rows of
// 16 by shifts 1, 2, 4, 8 (zero where the source lane is outside the row), then row 1 += lane 15, rows 2, 3 += lane 31
static float g_redf[1024];
static inline float wave_sum(float v) {
  std::barrier<>& wb = *g_wbar[threadIdx.x >> 6];
  const int w0 = threadIdx.x & ~63, ln = threadIdx.x & 63;
  for (int sh = 1; sh <= 8; sh <<= 1) {
    g_redf[threadIdx.x] = v;
    wb.arrive_and_wait();
    const float o = ((ln & 15) >= sh) ? g_redf[threadIdx.x - sh] : 0.f;
    wb.arrive_and_wait();
    v += o;
  }
  g_redf[threadIdx.x] = v;
  wb.arrive_and_wait();
  const float b15 = ln >= 16 ? g_redf[w0 + ((ln >> 4) - 1) * 16 + 15] : 0.f;     // row_bcast:15, every row enabled
  wb.arrive_and_wait();
  v += b15;
  g_redf[threadIdx.x] = v;
  wb.arrive_and_wait();
  const float b31 = ln >= 32 ? g_redf[w0 + 31] : 0.f;                            // row_bcast:31
  wb.arrive_and_wait();
  v += b31;
  g_redf[threadIdx.x] = v;
  wb.arrive_and_wait();
  const float r = g_redf[w0 + 63];
  wb.arrive_and_wait();
  return r;
}
}  // namespace bmpc
#define BMPC_WAVE_SYNC() g_wbar[threadIdx.x >> 6]->arrive_and_wait()
#define BMPC_DRAIN_LDS() do { } while (0)
#define BMPC_FENCE() do { } while (0)
#define BMPC_OPAQUE(x) do { } while (0)
#define BMPC_UNIFORM(x) (x)
#define BMPC_UNIFORM_INT(x) (x)
#define BMPC_SCHED_BARRIER() do { } while (0)

static float g_bc[1024];
namespace bmpc {
// value of lane N of the own row of 16 lanes (DPP row_newbcast on the GPU); all lanes of the wave call
template <int N>
static inline float row_bcast(float v) {
  std::barrier<>& wb = *g_wbar[threadIdx.x >> 6];
  g_bc[threadIdx.x] = v;
  wb.arrive_and_wait();
  const float r = g_bc[(threadIdx.x & ~15) + N];
  wb.arrive_and_wait();
  return r;
}
}  // namespace bmpc

namespace bmpc {
// v_mfma_f64_16x16x4_f64 on the CPU: every lane of the wave hands over its A and B entry (A[i = l & 15][k = l >> 4],
// B[k = l >> 4][j = l & 15]) and accumulates its 4 entries of D (row = (l >> 4) + 4 reg, col = l & 15)
typedef double emu_f64x4 __attribute__((ext_vector_type(4)));
static double g_mfa[1024], g_mfb[1024];
static inline emu_f64x4 mfma_f64_16x16x4(double a, double b, emu_f64x4 c) {
  std::barrier<>& wb = *g_wbar[threadIdx.x >> 6];
  const int w0 = threadIdx.x & ~63, ln = threadIdx.x & 63;
  g_mfa[threadIdx.x] = a;
  g_mfb[threadIdx.x] = b;
  wb.arrive_and_wait();
  for (int v = 0; v < 4; ++v) {
    const int row = (ln >> 4) + 4 * v, col = ln & 15;
    double acc = c[v];
    for (int k = 0; k < 4; ++k) acc = std::fma(g_mfa[w0 + 16 * k + row], g_mfb[w0 + 16 * k + col], acc);
    c[v] = acc;
  }
  wb.arrive_and_wait();
  return c;
}
}  // namespace bmpc

// value of lane `src` of the own wave (a wave-wide permute on the GPU: the evaluation family's one cross-lane primitive); all
// lanes of the wave call
static double g_lr[1024];
static int g_lri[1024];
namespace bmpc {
static inline double lane_read(double v, int src) {
  std::barrier<>& wb = *g_wbar[threadIdx.x >> 6];
  g_lr[threadIdx.x] = v;
  wb.arrive_and_wait();
  const double r = g_lr[(threadIdx.x & ~63) + src];
  wb.arrive_and_wait();
  return r;
}
static inline int lane_read(int v, int src) {
  std::barrier<>& wb = *g_wbar[threadIdx.x >> 6];
  g_lri[threadIdx.x] = v;
  wb.arrive_and_wait();
  const int r = g_lri[(threadIdx.x & ~63) + src];
  wb.arrive_and_wait();
  return r;
}
}  // namespace bmpc

// `kernel()` in every lane of a grid of `blocks` workgroups of NT lanes (a multiple of 64), block after block: one thread per
// lane, one barrier for the workgroup, one per wave, one rendezvous counter per lane pair
template <typename Kernel>
static void emu_run_grid(int NT, int blocks, Kernel kernel) {
  for (int b = 0; b < blocks; ++b) {
    std::barrier<> bar(NT);
    g_bar = &bar;
    std::vector<std::unique_ptr<std::barrier<>>> wb;
    for (int w = 0; w < NT / 64; ++w) { wb.emplace_back(new std::barrier<>(64)); g_wbar[w] = wb.back().get(); }
    for (int p = 0; p < NT / 2; ++p) g_pair[p].store(0);
    g_or[0] = g_or[1] = 0;
    std::vector<std::thread> th;
    th.reserve(NT);
    for (int t = 0; t < NT; ++t)
      th.emplace_back([&, t]() {
        threadIdx.x = t;
        blockIdx.x = b;
        kernel();
      });
    for (auto& x : th) x.join();
  }
}

#endif
