// bmpc_capi.hip -- C ABI (include/bmpc.h) over the HIP kernels.  Built into libbmpc.so.
// There is deliberately no CPU path here: without a HIP device every entry point that would
// compute returns BMPC_ERR_NO_DEVICE.
#include "bmpc_kernels.hip"
#include "bmpc_stage.hip"
#include "bmpc_lowlevel.hip"
#include "bmpc_plant.hip"
#include "bmpc_evaluate.hip"
#include "bmpc_evaluate_grad.hip"
#include "bmpc_certify.hip"
#include "bmpc_evaluate_samples.hip"
#include "bmpc_plant_rollout.hip"
#include "bmpc_plant_rollout_grad.hip"

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>

#include "bmpc.h"
#include "bmpc_host_params.hpp"
#include "bmpc_host_staging.hpp"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) return fail(BMPC_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// parameters and kernel variants: bmpc_host_params.hpp, shared with the CPU emulation of tests/emu
using namespace bmpc_host;
int make_dev_params(const bmpc_params& p, bmpc::DevParams* d) { return bmpc_host::make_dev_params(p, d, ErrBuf{g_err, sizeof(g_err)}); }

// page-locked host memory (the staging of the host-pointer entry points: copies to and from it run at the full PCIe rate
// and asynchronously, which pageable memory does not allow)
// (the three buffer types below free what they hold when they go -- with the handle, in bmpc_destroy -- and are not copied)
struct NoCopy {
  NoCopy() = default;
  NoCopy(const NoCopy&) = delete;
  NoCopy& operator=(const NoCopy&) = delete;
};

struct PinnedBuf : NoCopy {
  char* p = nullptr;
  size_t n = 0;
  ~PinnedBuf() { if (p) (void)hipHostFree(p); }
  hipError_t ensure(size_t bytes) {
    if (bytes <= n) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr; n = 0;
    // (mapped: the kernels of the host-pointer entry points store their results straight into this memory)
    // (coherent / non-coherent / write-combined make no difference to what a kernel's own stores into it sustain: ~8.6 GB/s, round 5)
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), bytes, hipHostMallocMapped | hipHostMallocPortable);
    if (e == hipSuccess) n = bytes;
    return e;
  }
};

// The same for memory the CALLER holds pointers into (the I/O block of bmpc_host_io): a block that has to grow is not freed but
// retired until the handle goes -- a view of the old layout that a caller still holds must not dangle --, and it grows by half at
// least, so that what is retired stays below twice what is in use.
struct RetiringPinnedBuf : NoCopy {
  char* p = nullptr;
  size_t n = 0;
  static constexpr int MAX_RETIRED = 64;
  char* retired[MAX_RETIRED] = {};
  int n_retired = 0;
  ~RetiringPinnedBuf() {
    if (p) (void)hipHostFree(p);
    for (int i = 0; i < n_retired; ++i) (void)hipHostFree(retired[i]);
  }
  hipError_t ensure(size_t bytes) {
    if (bytes <= n) return hipSuccess;
    size_t cap = n + n / 2;
    if (cap < bytes) cap = bytes;
    char* q = nullptr;
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&q), cap, hipHostMallocMapped | hipHostMallocPortable);
    if (e != hipSuccess) return e;
    if (p) {
      if (n_retired < MAX_RETIRED) retired[n_retired++] = p;
      else (void)hipHostFree(p);              // (64 growths by half: a block 10^11 times the first one -- not reached)
    }
    p = q; n = cap;
    return hipSuccess;
  }
};

template <typename T>
struct DevBuf : NoCopy {
  T* p = nullptr;
  size_t n = 0;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t ensure(size_t count) {
    if (count <= n) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr; n = 0;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T));
    if (e == hipSuccess) n = count;
    return e;
  }
};

// ---- The per-instance arrays of a solve, stated once: everything that packs, stages, lays out or views them walks these tables.

// elements per instance (fixed + per_step * h) and bytes per element of one array
struct Width {
  size_t fixed, per_step, elem;
  constexpr size_t count(size_t H) const { return fixed + per_step * H; }
  constexpr size_t bytes(size_t H) const { return count(H) * elem; }        // per instance
};

// The buffers of one solve launch: device-addressable pointers (on the I/O path some point into mapped page-locked host
// memory), null where bmpc_solve_inputs_device allows it.  controls64 / states64: fp64 outputs that take the place of controls /
// states (bmpc::WarmArgs).
struct SolveIO {
  bmpc_inputs in = {};               // (x_ref, foot_ref: supplied references or null)
  float *controls = nullptr, *states = nullptr, *resid = nullptr;
  int32_t *iters = nullptr, *status = nullptr, *nfactor = nullptr;
  double *controls64 = nullptr, *states64 = nullptr;
};

// A row: where the array's pointer sits in its descriptor (inputs: bmpc_inputs; outputs: SolveIO) and in bmpc_host_views (NO_VIEW:
// the I/O block never holds it), its width (elem 0: f32 or f64, as the caller of the layout chooses, and widened from the
// kernels' f32 by the host-pointer entries), and whether a packed block always has room for it.  The rows are in the order
// of the packed blocks, which the enums name.  A further input is a row here, a bmpc_inputs member and its kernel parameter.
struct Field { size_t member, view; Width w; bool always; };
constexpr size_t NO_VIEW = ~(size_t)0;
enum { I_XFB, I_FOOT, I_PHASE, I_XCMD, I_MU, I_CON, I_XREF, I_FREF, N_IN };
enum { O_U, O_S, O_IT, O_ST, O_NF, O_RS, N_OUT };
#define BMPC_IN(m) offsetof(bmpc_inputs, m), offsetof(bmpc_host_views, m)
constexpr Field IN[N_IN] = {
    {BMPC_IN(x_fb), {12, 0, 4}, true},   {BMPC_IN(foot), {6, 0, 4}, true}, {BMPC_IN(phase), {1, 0, 4}, true},
    {BMPC_IN(x_cmd), {12, 0, 4}, false}, {BMPC_IN(mu), {0, 2, 4}, false},  {BMPC_IN(contact), {0, 2, 1}, true},
    {offsetof(bmpc_inputs, x_ref), NO_VIEW, {0, 12, 4}, false}, {offsetof(bmpc_inputs, foot_ref), NO_VIEW, {0, 6, 4}, false}};
#undef BMPC_IN
#define BMPC_OUT(m, v) offsetof(SolveIO, m), offsetof(bmpc_host_views, v)
constexpr Field OUT[N_OUT] = {{BMPC_OUT(controls, controls), {0, 12, 0}, true}, {BMPC_OUT(states, states), {0, 13, 0}, false},
                              {BMPC_OUT(iters, iters), {1, 0, 4}, true},        {BMPC_OUT(status, status), {1, 0, 4}, true},
                              {BMPC_OUT(nfactor, nfactor), {1, 0, 4}, true},    {BMPC_OUT(resid, residuals), {2, 0, 4}, true}};
#undef BMPC_OUT

// the pointer members of the descriptors, by offset
const void* get_ptr(const void* desc, size_t member) { const void* p; std::memcpy(&p, (const char*)desc + member, sizeof(p)); return p; }
void set_ptr(void* desc, size_t member, const void* p) { std::memcpy((char*)desc + member, &p, sizeof(p)); }

// Offsets of the packed arrays of n instances, every array `align`-byte aligned (a power of two): inputs and outputs in the
// order of the tables; has_in / has_out: bit i set where row i is there (the `always` rows are), controls and states in elements
// of out_elem bytes.  (x_ref and foot_ref come after everything else: without them the layout is the one the handle's I/O block
// has always had.)
struct PackedLayout {
  size_t H = 0, out_elem = 0;
  unsigned has_in = 0, has_out = 0;
  size_t in[N_IN] = {}, in_bytes = 0, out[N_OUT] = {}, out_bytes = 0;
  size_t stride(const Field& f) const { return f.w.count(H) * (f.w.elem ? f.w.elem : out_elem); }   // bytes per instance
  // byte offset of input / output array i, from instance lo on
  size_t in_at(int i, size_t lo) const { return in[i] + lo * stride(IN[i]); }
  size_t out_at(int i, size_t lo) const { return out[i] + lo * stride(OUT[i]); }
};
PackedLayout packed_layout(size_t n, size_t H, unsigned has_in, unsigned has_out, size_t align, size_t out_elem) {
  PackedLayout L;
  L.H = H; L.out_elem = out_elem; L.has_in = has_in; L.has_out = has_out;
  auto lay = [&](const Field* f, int rows, unsigned& has, size_t* off) {
    size_t at = 0;
    for (int i = 0; i < rows; ++i) {
      if (f[i].always) has |= 1u << i;
      off[i] = at;
      at = (at + (has >> i & 1 ? n * L.stride(f[i]) : 0) + align - 1) & ~(align - 1);
    }
    return at;
  };
  L.in_bytes = lay(IN, N_IN, L.has_in, L.in);
  L.out_bytes = lay(OUT, N_OUT, L.has_out, L.out);
  return L;
}
// the rows of IN a descriptor holds an array for
unsigned present(const bmpc_inputs& in) {
  unsigned has = 0;
  for (int i = 0; i < N_IN; ++i) has |= get_ptr(&in, IN[i].member) ? 1u << i : 0;
  return has;
}

}  // namespace

struct bmpc_handle_s {
  int device = 0;
  int max_batch = 0;
  bmpc_params params;
  bmpc::DevParams dev;
  int path = BMPC_PATH_DENSE;      // resolved kernel family (resolve_path)
  bool rescue_on = false;          // dense solves are followed by the stage family's rescue pass (resolve_rescue)
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;
  // staging for the host-pointer entry points.  bmpc_solve_batch*: ONE packed block of inputs and one of outputs on either side
  // of PCIe (pinned on the host), the batch solved in up to HOST_CHUNKS chunks on streams of descending priority so that a
  // chunk's results cross PCIe -- and are unpacked / widened by the calling thread -- while the later chunks still solve
  static constexpr int HOST_CHUNKS = 3;
  PinnedBuf pin_in, pin_out;
  DevBuf<char> dev_in, dev_out;
  hipStream_t cstream[HOST_CHUNKS] = {nullptr, nullptr, nullptr};
  hipEvent_t cev[HOST_CHUNKS] = {nullptr, nullptr, nullptr};
  hipEvent_t cev_own = nullptr;     // what the handle's own stream held when a host-pointer call began: the chunk streams wait for it
  // the chunking of the host-pointer entry points, fixed at creation (BMPC_HOST_CUTS = "a,b" with 0 < a <= b <= 1, or "1": one
  // chunk; anything else is ignored) and the diagnostics switch BMPC_HOST_TIMING
  int host_chunks = HOST_CHUNKS;
  double host_cut[HOST_CHUNKS + 1] = {0.0, 0.55, 0.85, 1.0};
  bool host_timing = false;
  // the handle's I/O block (bmpc_host_io / bmpc_solve_batch_io): page-locked host memory, mapped into the device's address
  // space -- the caller writes its inputs there, the kernels store the fp64 results there
  RetiringPinnedBuf io_in, io_out;
  DevBuf<char> io_dev;
  DevBuf<double> io_states;         // fp64 states of a batch in HBM, on their way to the I/O block by copy engine
  hipEvent_t cev_in = nullptr;      // the I/O block's inputs have arrived
  int io_gen = 0;                   // moves with every bmpc_host_io call (bmpc_host_io_generation)
  struct IoLayout : PackedLayout { int B = 0; } io;
  // The staging of every other host-pointer entry.  A synchronous host entry is its _device twin between a stage and a fetch:
  // all host inputs of the call are laid out in ONE block, host_in, all wanted outputs and the scratch of the call in ONE other,
  // host_out (stage / carve / fetch below); the twin runs on the handle's own stream on pointers into them, the outputs are
  // copied back and the stream is synchronised.  The entries are synchronous, so no two of them use the blocks at once.  No
  // _device entry touches either: that keeps those asynchronous and leaves the handle alone.
  DevBuf<char> host_in, host_out;
  DevBuf<double> samples;           // sample reductions, either entry: scores / weights they need and the caller did not ask for
  DevBuf<int32_t> status;           // the rescue pass's, where the caller asks for none
  long long* prof_dev = nullptr;   // optional cycle-stamp buffer (bmpc_debug_set_profile)
  // receding-horizon warm start (bmpc_set_warm_start): solver state of the last batch, kept on the device
  DevBuf<double> warm;
  bool warm_on = false, warm_valid = false;
  int warm_batch = 0, warm_shift = 0;
  float warm_theta = 0.5f;
  // roll-out scratch (bmpc_rollout_device)
  DevBuf<float> ro_controls, ro_states;
  DevBuf<uint8_t> ro_contact;
  DevBuf<int32_t> ro_phase, ro_iters, ro_status, ro_order;
  // roll-out gradient scratch (bmpc_plant_rollout_grad*): recorded states and footholds, substep states
  DevBuf<float> rg_states, rg_feet;
  DevBuf<double> rg_sub;
  const int32_t* order = nullptr;   // dispatch order of the next solves (bmpc_set_dispatch_order; roll-outs set their own)
  bool longest_first = true;        // roll-outs order each period's solve by the previous period's iteration counts
};

namespace {

// One launch of kernel family `path`: the warm-start set-up (warm_doubles of solver state per instance), then
// `kernel(args...)`, which launches the family's kernel with the parameter list both families share.
template <typename Kernel>
int launch_family(bmpc_handle hd, int B, int path, const SolveIO& io, const bmpc::DebugOut& dbg, const int32_t* order,
                  const int32_t* rescue_status, Kernel kernel) {
  // (the references go to every launch of the solve, the rescue pass included: it solves the same problem again)
  bmpc::WarmArgs warm = {nullptr, 0, 0, 0, 1.f, 0, dbg.assemble_only ? nullptr : order, rescue_status, io.controls64, io.states64,
                         io.in.x_ref, io.in.foot_ref};
  if (hd->warm_on && !dbg.assemble_only && !rescue_status) {   // (a rescue pass starts cold: the stored state is the dense family's)
    const size_t need = (size_t)B * (size_t)warm_doubles(path, hd->dev.h);
    if (need > hd->warm.n) hd->warm_valid = false;          // growing the buffer loses the stored state
    HIP_TRY(hd->warm.ensure(need));
    warm.buf = hd->warm.p;
    warm.load = (hd->warm_valid && hd->warm_batch == B) ? 1 : 0;
    warm.store = 1;
    warm.shift = hd->warm_shift;
    warm.theta = hd->warm_theta;
    warm.adapt_start = hd->params.warm_adapt_start;
  }
  kernel(hd->dev, B, io.in.x_fb, io.in.foot, io.in.contact, io.in.phase, io.in.x_cmd, io.in.mu, io.controls, io.states, io.iters, io.resid,
         io.status, io.nfactor, dbg, warm);
  HIP_TRY(hipGetLastError());
  if (warm.buf) { hd->warm_valid = true; hd->warm_batch = B; }
  return BMPC_OK;
}

// The kernel of the handle's horizon, through the variant lists of bmpc_host_params.hpp.
// (dbg.prof: the diagnostics build of the same body, with in-kernel cycle stamps -- bmpc_debug_set_profile)
int launch_dense(bmpc_handle hd, int B, const SolveIO& io, const bmpc::DebugOut& dbg, hipStream_t st, const int32_t* order) {
  const int rc = dispatch_dense(hd->dev.h, NO_VARIANT, [&](auto Hc) {
    constexpr int H = decltype(Hc)::value, NT = bmpc::Dims<H>::NT;
    return launch_family(hd, B, BMPC_PATH_DENSE, io, dbg, order, nullptr, [&](auto... args) {
      if (dbg.prof) hipLaunchKernelGGL((bmpc::solve_kernel_prof<H>), dim3(B), dim3(NT), 0, st, args...);
      else hipLaunchKernelGGL((bmpc::solve_kernel<H>), dim3(B), dim3(NT), 0, st, args...);
    });
  });
  return rc == NO_VARIANT ? fail(BMPC_ERR_INVALID, "unsupported horizon h=%d", hd->dev.h) : rc;
}

int launch_stage(bmpc_handle hd, int B, const SolveIO& io, const bmpc::DebugOut& dbg, hipStream_t st, const int32_t* order,
                 const int32_t* rescue_status) {
  const int rc = dispatch_stage(hd->dev.h, NO_VARIANT, [&](auto NPc, auto NWc) {
    constexpr int NP = decltype(NPc)::value, NW = decltype(NWc)::value;
    return launch_family(hd, B, BMPC_PATH_STAGE, io, dbg, order, rescue_status, [&](auto... args) {
      if (dbg.prof) hipLaunchKernelGGL((bmpc::stage_kernel_prof<NP, NW>), dim3(B), dim3(64 * NW), 0, st, args...);
      else hipLaunchKernelGGL((bmpc::stage_kernel<NP, NW>), dim3(B), dim3(64 * NW), 0, st, args...);
    });
  });
  return rc == NO_VARIANT ? fail(BMPC_ERR_INVALID, "unsupported horizon h=%d", hd->dev.h) : rc;
}

int launch(bmpc_handle hd, int B, SolveIO io, const bmpc::DebugOut& dbg, hipStream_t st, const int32_t* order) {
  const bool dense_views = dbg.assemble_only && (dbg.Gt || dbg.qt);      // Gt, qt only exist on the dense path
  if (hd->path == BMPC_PATH_STAGE && !(dense_views && dense_horizon(hd->dev.h))) {
    if (dense_views) return fail(BMPC_ERR_INVALID, "Gt / qt views exist for h <= 20 only (h=%d never forms them)", hd->dev.h);
    return launch_stage(hd, B, io, dbg, st, order, nullptr);
  }
  // Dense family.  With the rescue pass on, the instances whose status is not 0 afterwards are solved again by the
  // stage-structured kernel of the same horizon (f32 Riccati recursion instead of the f32 explicit inverse: it does not
  // share the dense sweep's rare breakdowns; profiles/r03_soak.txt): one more launch whose workgroups leave at once
  // where the status is 0, no host round trip.
  const bool rescue = hd->rescue_on && !dbg.assemble_only;
  if (rescue && !io.status) {
    HIP_TRY(hd->status.ensure((size_t)B));
    io.status = hd->status.p;
  }
  const int rc = launch_dense(hd, B, io, dbg, st, order);
  if (rc != BMPC_OK || !rescue) return rc;
  bmpc::DebugOut quiet = dbg;
  quiet.prof = nullptr;                        // the cycle stamps stay those of the first solve
  return launch_stage(hd, B, io, quiet, st, order, io.status);
}

// NULL is HIP's null (legacy default) stream, like every hip* call; BMPC_STREAM_OWN the handle's own stream
hipStream_t pick_stream(bmpc_handle h, void* stream) {
  if (stream == BMPC_STREAM_OWN) return h->stream;
  return static_cast<hipStream_t>(stream);
}

// The handle and batch size every batched entry point checks first: an error code (< 0), BMPC_OK (0) when there is nothing to
// do (B == 0), or 1 when the call goes on.
int check_batch(bmpc_handle h, int B) {
  if (!h) return fail(BMPC_ERR_INVALID, "null handle");
  if (B < 0 || B > h->max_batch) return fail(BMPC_ERR_INVALID, "batch %d outside [0, max_batch=%d]", B, h->max_batch);
  return B > 0 ? 1 : BMPC_OK;
}

// check_batch and the arrays a solve cannot do without (foot: unless foot_ref takes its place)
int check_common(bmpc_handle h, int B, const bmpc_inputs& in, const void* controls) {
  const int rc = check_batch(h, B);
  if (rc > 0 && (!in.x_fb || !(in.foot || in.foot_ref) || !in.contact || !in.phase || !controls))
    return fail(BMPC_ERR_INVALID, "x_fb, foot (or foot_ref), contact, phase and controls must be non-null");
  return rc;
}

// one solve launch with the dispatch order given explicitly (roll-outs use their own, the handle's stays untouched)
// (ev: which of the handle's timing events this launch records -- bit 0: ev0 before it, bit 1: ev1 after it; a batch that goes
//  out in chunks records ev0 before its first kernel and ev1 after its last, so bmpc_last_kernel_ms spans them all)
int solve_device_ordered(bmpc_handle h, int B, const SolveIO& io, void* stream, const int32_t* order, int ev = 3) {
  const void* controls = io.controls64 ? static_cast<const void*>(io.controls64) : static_cast<const void*>(io.controls);
  if (int rc = check_common(h, B, io.in, controls); rc <= 0) return rc;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = pick_stream(h, stream);
  bmpc::DebugOut dbg = {nullptr, nullptr, nullptr, nullptr, h->prof_dev, 0};
  if (ev & 1) HIP_TRY(hipEventRecord(h->ev0, st));
  if (int rc = launch(h, B, io, dbg, st, order); rc != BMPC_OK) return rc;
  if (ev & 2) { HIP_TRY(hipEventRecord(h->ev1, st)); h->timed = true; }
  return BMPC_OK;
}

// ---- the chunked host-pointer entry points (bmpc_solve_batch*, bmpc_solve_batch_io)

// How such a call splits its n instances: contiguous chunks [lo, lo + nb), one per stream priority the device offers (MI355X:
// three; chunks that share a priority are served round robin and finish together), the later ones smaller: the last chunk's
// unpacking is the exposed part, and a chunk's unpacking (~1/3 of its solve time) has to fit before the next chunk arrives.
// Warm start, a dispatch order and the profile buffer index by the instance's position in the whole batch: with any of them
// set, or `whole`, the batch goes out as one chunk.
struct ChunkPlan {
  int n = 1;
  size_t lo[bmpc_handle_s::HOST_CHUNKS] = {}, nb[bmpc_handle_s::HOST_CHUNKS] = {};
  int events(int c) const { return (c == 0 ? 1 : 0) | (c == n - 1 ? 2 : 0); }   // solve_device_ordered's ev of chunk c
};
ChunkPlan plan_chunks(bmpc_handle h, size_t n, bool whole) {
  ChunkPlan p;
  const int k = (whole || h->warm_on || h->order || h->prof_dev) ? 1 : (int)(n / 512);
  p.n = k < 1 ? 1 : (k > h->host_chunks ? h->host_chunks : k);
  for (int c = 0; c < p.n; ++c) {
    p.lo[c] = p.n >= 2 ? (size_t)(n * h->host_cut[c]) : 0;
    p.nb[c] = (c == p.n - 1 ? n : (size_t)(n * h->host_cut[c + 1])) - p.lo[c];
  }
  return p;
}

// The chunk streams come after what the handle's own stream holds (a device-pointer solve on BMPC_STREAM_OWN, the warm-start
// state it writes); an idle stream -- the usual case -- is not made to process a marker the chunk streams would then wait for
// (tens of us).
hipError_t chunks_after_own_stream(bmpc_handle h, int nchunk) {
  if (hipStreamQuery(h->stream) == hipSuccess) return hipSuccess;
  hipError_t e = hipEventRecord(h->cev_own, h->stream);
  for (int c = 0; c < nchunk && e == hipSuccess; ++c) e = hipStreamWaitEvent(h->cstream[c], h->cev_own, 0);
  return e;
}

// An error return of a chunked call first waits for the chunk streams it has queued work on: their copies still read and write
// the handle's page-locked blocks.
int bail(bmpc_handle h, int issued, int code) {
  for (int c = 0; c < issued; ++c) (void)hipStreamSynchronize(h->cstream[c]);
  return code;
}
#define CHUNK_TRY(expr)                                                                                        \
  do {                                                                                                         \
    hipError_t e_ = (expr);                                                                                    \
    if (e_ != hipSuccess) return bail(h, issued, fail(BMPC_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_))); \
  } while (0)

// The arrays of instances lo.. in packed blocks `in` / `out` laid out by L, but for controls and states (f32 or f64: the caller's)
SolveIO packed_io(const PackedLayout& L, const char* in, char* out, size_t lo) {
  SolveIO io;
  for (int i = 0; i < N_IN; ++i)
    if (L.has_in >> i & 1) set_ptr(&io.in, IN[i].member, in + L.in_at(i, lo));
  for (int i = 0; i < N_OUT; ++i)
    if (OUT[i].w.elem) set_ptr(&io, OUT[i].member, out + L.out_at(i, lo));
  return io;
}

// Host pointers in, host pointers out (T = float: bmpc_solve_batch; T = double: bmpc_solve_batch_f64, the dtype the reference
// returns).  What the reference's callers get (REF:487), so PCIe is part of the path:
//   * per chunk the inputs are packed into one pinned block and cross in ONE copy; outputs come back one packed block;
//   * the batch is split into up to HOST_CHUNKS contiguous chunks (plan_chunks), each launched on its own stream (descending
//     priority: the dispatcher serves chunk 0's workgroups first), followed on that stream by the chunk's device-to-host copy:
//     the results of chunk c cross PCIe, and are unpacked (widened to fp64) into the caller's pageable arrays by the calling
//     thread, while chunks c + 1 .. still solve.  Only the last chunk's copy and unpacking are exposed.
//     (A caller that can take its results in the handle's own page-locked block has no unpacking at all: bmpc_solve_batch_io.)
// The kernels' arithmetic does not depend on the position in a batch, so the results are bit-identical to a single launch.
// Ordering: the chunk streams wait for what was queued on the handle's own stream before the call, and the call returns with
// every chunk complete.
template <typename T>
int solve_host(bmpc_handle h, int B, const bmpc_inputs& in, T* controls, T* states, int32_t* iters, float* residuals,
               int32_t* status, int32_t* nfactor) {
  if (int rc = check_common(h, B, in, controls); rc <= 0) return rc;
  void* const dst[N_OUT] = {controls, states, iters, status, nfactor, residuals};      // (the order of OUT)
  HIP_TRY(hipSetDevice(h->device));
  const size_t n = (size_t)B, H = (size_t)h->dev.h;
  const bool timing = h->host_timing;                                 // (diagnostics: where a host-pointer call spends its time)
  auto now = []() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t_begin = timing ? now() : 0.0;
  double t_wait = 0, t_unpack = 0, t_last_wait = 0, t_last_unpack = 0;
  const ChunkPlan plan = plan_chunks(h, n, false);
  // each chunk's packed blocks (16-byte aligned arrays, f32 outputs), one after the other in pin_in / dev_in and pin_out / dev_out
  struct Chunk { PackedLayout L; size_t in, out; } ck[bmpc_handle_s::HOST_CHUNKS];
  size_t in_bytes = 0, out_bytes = 0;
  for (int c = 0; c < plan.n; ++c) {
    ck[c] = {packed_layout(plan.nb[c], H, present(in), states ? 1u << O_S : 0, 16, 4), in_bytes, out_bytes};
    in_bytes += ck[c].L.in_bytes;
    out_bytes += ck[c].L.out_bytes;
  }
  HIP_TRY(h->pin_in.ensure(in_bytes));
  HIP_TRY(h->dev_in.ensure(in_bytes));
  HIP_TRY(h->pin_out.ensure(out_bytes));
  HIP_TRY(h->dev_out.ensure(out_bytes));
  HIP_TRY(chunks_after_own_stream(h, plan.n));
  int issued = 0;                               // chunks whose work is queued (an error below waits for them before returning)
  for (int c = 0; c < plan.n; ++c) {
    const PackedLayout& L = ck[c].L;
    const size_t lo = plan.lo[c], nb = plan.nb[c];
    // inputs of this chunk: packed into the pinned block and sent in ONE copy (chunk 0 is on its way while the later
    // chunks are still being packed)
    char* pin = h->pin_in.p + ck[c].in;
    char* din = h->dev_in.p + ck[c].in;
    for (int i = 0; i < N_IN; ++i)
      if (const void* src = get_ptr(&in, IN[i].member))
        std::memcpy(pin + L.in[i], static_cast<const char*>(src) + lo * IN[i].w.bytes(H), nb * IN[i].w.bytes(H));
    hipStream_t st = h->cstream[c];
    issued = c + 1;
    CHUNK_TRY(hipMemcpyAsync(din, pin, L.in_bytes, hipMemcpyHostToDevice, st));
    char* dout = h->dev_out.p + ck[c].out;
    SolveIO io = packed_io(L, din, dout, 0);
    if (!in.foot) io.in.foot = nullptr;         // (foot_ref given: the kernels never read foot)
    io.controls = reinterpret_cast<float*>(dout + L.out[O_U]);
    if (states) io.states = reinterpret_cast<float*>(dout + L.out[O_S]);
    if (int rc = solve_device_ordered(h, (int)nb, io, st, h->order, plan.events(c)); rc != BMPC_OK) return bail(h, issued, rc);
    // (the copy engine moves a chunk at ~50 GB/s while the later chunks solve; stores of the kernels themselves into mapped host
    //  memory sustain ~8.6 GB/s on MI355X -- measured, round 5 -- which a 4096-instance batch's 4 MB would just fit under, with
    //  nothing to spare)
    CHUNK_TRY(hipMemcpyAsync(h->pin_out.p + ck[c].out, dout, L.out_bytes, hipMemcpyDeviceToHost, st));
    CHUNK_TRY(hipEventRecord(h->cev[c], st));
  }
  const double t_issued = timing ? now() : 0.0;
  // ---- unpack chunk by chunk, as each arrives
  for (int c = 0; c < plan.n; ++c) {
    const PackedLayout& L = ck[c].L;
    const size_t lo = plan.lo[c], nb = plan.nb[c];
    const double tw0 = timing ? now() : 0.0;
    CHUNK_TRY(hipEventSynchronize(h->cev[c]));
    const double tw1 = timing ? now() : 0.0;
    t_wait += tw1 - tw0; t_last_wait = tw1 - tw0;
    if (timing) std::fprintf(stderr, "[bmpc host path]   chunk %d ready %.0f us after the call began (waited %.0f)\n", c, tw1 - t_begin, tw1 - tw0);
    const char* src = h->pin_out.p + ck[c].out;
    for (int i = 0; i < N_OUT; ++i) {
      if (!dst[i]) continue;
      const size_t cnt = OUT[i].w.count(H);
      const char* from = src + L.out[i];
      if (sizeof(T) != sizeof(float) && !OUT[i].w.elem) {     // controls, states: widened
        T* to = static_cast<T*>(dst[i]) + lo * cnt;
        for (size_t q = 0; q < nb * cnt; ++q) to[q] = (T)reinterpret_cast<const float*>(from)[q];
      } else std::memcpy(static_cast<char*>(dst[i]) + lo * cnt * sizeof(float), from, nb * cnt * sizeof(float));
    }
    if (timing) { const double tu = now() - tw1; t_unpack += tu; t_last_unpack = tu; }
  }
  if (timing)
    std::fprintf(stderr, "[bmpc host path] B %d chunks %d: pack + issue %.0f us, waiting %.0f us (last chunk %.0f), unpack %.0f us (last chunk %.0f), total %.0f us\n",
                 B, plan.n, t_issued - t_begin, t_wait, t_last_wait, t_unpack, t_last_unpack, now() - t_begin);
  return BMPC_OK;
}

// ---- the synchronous host entries (the rule: bmpc_handle_s).  A further one is a table of rows and about ten lines.

// One array of such a call: the caller's host array (null: the row is absent, it takes no room and its device pointer is null)
// and its width.  An output row with `keep` set is laid out whatever p says: what the twin forms whether or not the caller wants
// it back, and, with p null, scratch that is not copied back.
struct InSlot { const void* p; Width w; };
struct OutSlot { void* p; Width w; bool keep = false; };
template <size_t N> struct OutSlots { OutSlot s[N]; };

// widths of the low-level and plant entries' arrays that no table above holds
constexpr Width W_JOINTS = {10, 0, 4}, W_FEET = {6, 0, 4}, W_WRENCH = {6, 0, 4}, W_U0 = {12, 0, 4}, W_CONTACT0 = {2, 0, 1},
                W_FLAGS = {1, 0, 1}, W_T = {1, 0, 8}, W_MASS = {1, 0, 8}, W_INERTIA = {9, 0, 8}, W_GRAVITY = {1, 0, 8},
                W_GROUND_MU = {2, 0, 8};
// the f32 controls of `plans` plans per instance; a row of IN as the fp64 view an assembly launch stores
constexpr Width controls_width(size_t plans = 1) { return {0, OUT[O_U].w.per_step * plans, sizeof(float)}; }
constexpr Width f64_view(const Field& f) { return {f.w.fixed, f.w.per_step, sizeof(double)}; }

// the rows of a block on the device, in table order: pointer (null: absent) and bytes of each, and the bytes of the block
template <size_t N>
struct Slices {
  void* d[N];
  size_t bytes[N], total;
  template <typename T> T* at(size_t i) const { return static_cast<T*>(d[i]); }
};

// `rows` of B instances laid out in `block` (stage_layout of bmpc_host_staging.hpp), the block made large enough
inline bool wanted(const InSlot& s) { return s.p; }
inline bool wanted(const OutSlot& s) { return s.p || s.keep; }
template <size_t N, typename Slot>
int lay_out(bmpc_handle h, DevBuf<char>& block, int B, const Slot (&rows)[N], Slices<N>* L) {
  StageRow r[N]; size_t off[N];
  for (size_t i = 0; i < N; ++i) r[i] = {wanted(rows[i]), (size_t)B * rows[i].w.bytes((size_t)h->dev.h)};
  L->total = stage_layout(r, N, off);
  HIP_TRY(block.ensure(L->total));
  for (size_t i = 0; i < N; ++i) { L->bytes[i] = r[i].bytes; L->d[i] = r[i].present ? block.p + off[i] : nullptr; }
  return BMPC_OK;
}

// stage: the host inputs of a call into host_in, one copy per present row queued on the handle's own stream
template <size_t N>
int stage(bmpc_handle h, int B, const InSlot (&in)[N], Slices<N>* L) {
  if (int rc = lay_out(h, h->host_in, B, in, L); rc != BMPC_OK) return rc;
  for (size_t i = 0; i < N; ++i)
    if (in[i].p) HIP_TRY(hipMemcpyAsync(L->d[i], in[i].p, L->bytes[i], hipMemcpyHostToDevice, h->stream));
  return BMPC_OK;
}

// carve: the wanted outputs and the scratch of a call out of host_out
template <size_t N>
int carve(bmpc_handle h, int B, const OutSlot (&out)[N], Slices<N>* L) { return lay_out(h, h->host_out, B, out, L); }

// (both, for the entries that have nothing to do in between)
template <size_t NI, size_t NO>
int stage(bmpc_handle h, int B, const InSlot (&in)[NI], Slices<NI>* d, const OutSlot (&out)[NO], Slices<NO>* o) {
  const int rc = stage(h, B, in, d);
  return rc != BMPC_OK ? rc : carve(h, B, out, o);
}

// fetch: one copy back per wanted output, then the call waits for its stream
template <size_t N>
int fetch(bmpc_handle h, const OutSlot (&out)[N], const Slices<N>& L) {
  for (size_t i = 0; i < N; ++i)
    if (out[i].p) HIP_TRY(hipMemcpyAsync(out[i].p, L.d[i], L.bytes[i], hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return BMPC_OK;
}

// The inputs of a solve, host arrays, and `controls` (null: none) of `plans` plans per instance behind them, staged: *din the
// descriptor of the copies, *dcontrols the controls' (the evaluation family's host entries and bmpc_debug_assemble_inputs).
int stage_inputs(bmpc_handle h, int B, const bmpc_inputs& in, const float* controls, size_t plans, bmpc_inputs* din, const float** dcontrols) {
  InSlot rows[N_IN + 1];
  for (int i = 0; i < N_IN; ++i) rows[i] = {get_ptr(&in, IN[i].member), IN[i].w};
  rows[N_IN] = {controls, controls_width(plans)};
  Slices<N_IN + 1> L;
  if (int rc = stage(h, B, rows, &L); rc != BMPC_OK) return rc;
  for (int i = 0; i < N_IN; ++i) set_ptr(din, IN[i].member, L.d[i]);
  *dcontrols = L.at<const float>(N_IN);
  return BMPC_OK;
}

// ---- the evaluation family: bmpc_evaluate, bmpc_evaluate_grad, bmpc_certify and their _device twins.  One launch each, nothing
// of the handle's per-solve state involved.  The kernels differ (bmpc_evaluate.hip, bmpc_evaluate_grad.hip, bmpc_certify.hip);
// the path around them is stated once here.  A further operation is a kernel, an EvalOp row, a slot table and two entries.

// what an operation takes besides the inputs and the controls: certify's act_tol, the sampling descriptor of evaluate_samples
struct EvalArg { double act_tol = 0.0; const bmpc_samples* smp = nullptr; };

// `launch`: the operation's kernel on device-addressable inputs; `out`: one pointer per slot, in the table's order
using EvalLaunch = int (*)(bmpc_handle h, int B, const bmpc_inputs& in, const float* controls, const EvalArg& arg, void* const* out,
                           hipStream_t st);
struct EvalOp { const char *null_out, *none_out; EvalLaunch launch; };

template <auto Kernel, typename... Tail>
int launch_eval(bmpc_handle h, int B, const bmpc_inputs& in, const float* controls, hipStream_t st, Tail... tail) {
  const long long lanes = (long long)B * bmpc::eval_lanes(h->params.h);
  hipLaunchKernelGGL(Kernel, dim3((unsigned)((lanes + bmpc::EVAL_NT - 1) / bmpc::EVAL_NT)), dim3(bmpc::EVAL_NT), 0, st,
                     bmpc::eval_params(h->params, h->dev.Iinv), B, in.x_fb, in.foot, in.contact, in.phase, in.x_cmd, in.mu, in.x_ref,
                     in.foot_ref, controls, tail...);
  HIP_TRY(hipGetLastError());
  return BMPC_OK;
}

int launch_evaluate(bmpc_handle h, int B, const bmpc_inputs& in, const float* controls, const EvalArg&, void* const* o, hipStream_t st) {
  return launch_eval<bmpc::evaluate_kernel>(h, B, in, controls, st, bmpc::EvalOut{(double*)o[0], (double*)o[1], (double*)o[2], (double*)o[3]});
}
int launch_evaluate_grad(bmpc_handle h, int B, const bmpc_inputs& in, const float* controls, const EvalArg&, void* const* o, hipStream_t st) {
  return launch_eval<bmpc::evaluate_grad_kernel>(h, B, in, controls, st, bmpc::GradOut{(double*)o[0], (double*)o[1], (double*)o[2]});
}
int launch_certify(bmpc_handle h, int B, const bmpc_inputs& in, const float* controls, const EvalArg& arg, void* const* o, hipStream_t st) {
  return launch_eval<bmpc::certify_kernel>(h, B, in, controls, st, arg.act_tol,
                                           bmpc::CertOut{(double*)o[0], (double*)o[1], (double*)o[2], (int32_t*)o[3], (int32_t*)o[4]});
}

// The tail both sampling operations share: `per_sample(score)`, the operation's own launch, then -- where one of the reduced
// outputs r[0 .. 4] (best, n_valid, weights, u_mean, ess: the order of both descriptors) is wanted -- the per-instance reductions
// behind it on the same stream.  The reductions read the scores and the weights from the device: where the caller wants
// neither array they live in the handle's `samples` scratch, grown on demand (a call that has to grow it is not asynchronous:
// the old block is freed).  `always_score`: the per-sample kernel stores its scores whether or not anything is reduced.
template <typename PerSample>
int launch_sampled(bmpc_handle h, int B, int S, double temperature, bool always_score, double* score, const float* controls,
                   void* const* r, hipStream_t st, PerSample per_sample) {
  const size_t n = (size_t)B * (size_t)S;
  const bool reduce = r[0] || r[1] || r[2] || r[3] || r[4];
  double* weights = (double*)r[2];
  const bool own_score = (always_score || reduce) && !score, own_weights = reduce && !weights;
  if (own_score || own_weights) {
    HIP_TRY(h->samples.ensure(n * ((size_t)own_score + (size_t)own_weights)));
    if (own_score) score = h->samples.p;
    if (own_weights) weights = h->samples.p + (own_score ? n : 0);
  }
  if (int rc = per_sample(score); rc != BMPC_OK) return rc;
  HIP_TRY(hipGetLastError());
  if (reduce) {
    hipLaunchKernelGGL(bmpc::sample_reduce_kernel, dim3((unsigned)B), dim3(bmpc::REDUCE_NT), 0, st, (int)h->params.h, S, temperature,
                       (const double*)score, controls, bmpc::ReduceOut{(int32_t*)r[0], (int32_t*)r[1], weights, (double*)r[3], (double*)r[4]});
    HIP_TRY(hipGetLastError());
  }
  return BMPC_OK;
}

// evaluate_samples: the per-sample kernel over B ceil(S / C) groups, C samples each (bmpc::eval_samples_per_group), and the
// reductions.  o: the slots of bmpc_samples_out, in its order.
int launch_evaluate_samples(bmpc_handle h, int B, const bmpc_inputs& in, const float* controls, const EvalArg& arg, void* const* o,
                            hipStream_t st) {
  const bmpc_samples& smp = *arg.smp;
  return launch_sampled(h, B, (int)smp.S, smp.temperature, true, (double*)o[2], controls, o + 3, st, [&](double* score) {
    const int C = bmpc::eval_samples_per_group(B, smp.S);
    const long long groups = (long long)B * (((long long)smp.S + C - 1) / C);
    const long long blocks = (groups * bmpc::eval_lanes(h->params.h) + bmpc::EVAL_NT - 1) / bmpc::EVAL_NT;
    if (blocks > 0x7fffffffLL)
      return fail(BMPC_ERR_INVALID, "B x S = %zu plans are more than one launch holds", (size_t)B * (size_t)smp.S);
    bmpc::SamplesPrice price;
    for (int c = 0; c < 4; ++c) price.w[c] = smp.w_viol[c];
    hipLaunchKernelGGL(bmpc::evaluate_samples_kernel, dim3((unsigned)blocks), dim3(bmpc::EVAL_NT), 0, st,
                       bmpc::eval_params(h->params, h->dev.Iinv), B, (int)smp.S, C, in.x_fb, in.foot, in.contact, in.phase, in.x_cmd,
                       in.mu, in.x_ref, in.foot_ref, controls, price, bmpc::SamplesOut{(double*)o[0], (double*)o[1], score});
    return (int)BMPC_OK;
  });
}

const EvalOp EVALUATE = {"null bmpc_eval_out", "bmpc_eval_out: at least one of cost, objective, states, violation must be non-null",
                         launch_evaluate};
const EvalOp EVALUATE_GRAD = {"null bmpc_grad_out", "bmpc_grad_out: at least one of cost, grad_u, grad_x0 must be non-null",
                              launch_evaluate_grad};
const EvalOp CERTIFY = {"null bmpc_cert_out", "bmpc_cert_out: at least one of lam, resid, summary, n_active, status must be non-null",
                        launch_certify};
const EvalOp EVALUATE_SAMPLES = {"null bmpc_samples_out",
                                 "bmpc_samples_out: at least one of cost, violation, score, best, n_valid, weights, u_mean, ess must be non-null",
                                 launch_evaluate_samples};

// the slot tables, in the member order of the descriptors (include/bmpc.h); a null descriptor gives all-null slots
OutSlots<4> slots_of(const bmpc_eval_out* out) {
  const bmpc_eval_out o = out ? *out : bmpc_eval_out{};
  return {{{o.cost, {1, 0, 8}}, {o.objective, {1, 0, 8}}, {o.states, {0, 13, 8}}, {o.violation, {4, 0, 8}}}};
}
OutSlots<3> slots_of(const bmpc_grad_out* out) {
  const bmpc_grad_out o = out ? *out : bmpc_grad_out{};
  return {{{o.cost, {1, 0, 8}}, {o.grad_u, {0, 12, 8}}, {o.grad_x0, {12, 0, 8}}}};
}
OutSlots<5> slots_of(const bmpc_cert_out* out) {
  const bmpc_cert_out o = out ? *out : bmpc_cert_out{};
  return {{{o.lam, {0, 36, 8}}, {o.resid, {0, 12, 8}}, {o.summary, {4, 0, 8}}, {o.n_active, {1, 0, 4}}, {o.status, {1, 0, 4}}}};
}

// (per-sample arrays: S entries per instance; S = 1 where the sampling descriptor is null or out of range -- the entry refuses it)
OutSlots<8> slots_of(const bmpc_samples_out* out, const bmpc_samples* smp) {
  const bmpc_samples_out o = out ? *out : bmpc_samples_out{};
  const size_t S = smp && smp->S >= 1 && smp->S <= bmpc::SAMPLES_MAX ? (size_t)smp->S : 1;
  return {{{o.cost, {S, 0, 8}}, {o.violation, {4 * S, 0, 8}}, {o.score, {S, 0, 8}}, {o.best, {1, 0, 4}}, {o.n_valid, {1, 0, 4}},
           {o.weights, {S, 0, 8}}, {o.u_mean, {0, 12, 8}}, {o.ess, {1, 0, 8}}}};
}

// What both sampling descriptors (`name`: bmpc_samples, bmpc_rollout_price) hold alike, checked before anything else of the
// call: S, the nw prices w -- `which` names them in the message, and may take the index of the offending one --, the temperature
int check_sampling(const char* name, int S, const double* w, int nw, const char* which, double temperature) {
  if (S < 1 || S > bmpc::SAMPLES_MAX) return fail(BMPC_ERR_INVALID, "%s: S = %d outside [1, %d]", name, S, bmpc::SAMPLES_MAX);
  char what[64];
  for (int c = 0; c < nw; ++c)
    if (!(w[c] >= 0.0 && w[c] <= 1.7976931348623157e308)) {
      std::snprintf(what, sizeof(what), which, c);
      return fail(BMPC_ERR_INVALID, "%s: %s must be finite and >= 0", name, what);
    }
  if (!(temperature > 0.0)) return fail(BMPC_ERR_INVALID, "%s: temperature must be > 0 (+inf allowed)", name);
  return BMPC_OK;
}
int check_samples(const bmpc_samples* smp) {
  if (!smp) return fail(BMPC_ERR_INVALID, "null bmpc_samples");
  return check_sampling("bmpc_samples", (int)smp->S, smp->w_viol, 4, "w_viol[%d]", smp->temperature);
}

// what every entry checks before a device is touched (and before the handle is read): an error code (< 0), BMPC_OK when there is
// nothing to do, 1 to go on.  `out`: the entry's output descriptor
template <size_t N>
int check_eval(const EvalOp& op, bmpc_handle h, int B, const bmpc_inputs* in, const float* controls, const void* out,
               const OutSlots<N>& slots) {
  if (!h) return fail(BMPC_ERR_INVALID, "null handle");
  if (!in) return fail(BMPC_ERR_INVALID, "null bmpc_inputs");
  if (!controls) return fail(BMPC_ERR_INVALID, "null controls");
  if (!out) return fail(BMPC_ERR_INVALID, op.null_out);
  bool any_out = false;
  for (const OutSlot& s : slots.s) any_out = any_out || s.p;
  if (!any_out) return fail(BMPC_ERR_INVALID, op.none_out);
  return check_common(h, B, *in, controls);
}

// the device entry: everything device-addressable, asynchronous on `stream`
template <size_t N>
int eval_device(const EvalOp& op, bmpc_handle h, int B, const bmpc_inputs* in, const float* controls, const EvalArg& arg,
                const void* out, const OutSlots<N>& slots, void* stream) {
  if (int rc = check_eval(op, h, B, in, controls, out, slots); rc <= 0) return rc;
  HIP_TRY(hipSetDevice(h->device));
  void* d[N];
  for (size_t i = 0; i < N; ++i) d[i] = slots.s[i].p;
  return op.launch(h, B, *in, controls, arg, d, pick_stream(h, stream));
}

// the host entry: the operation's launch between stage and fetch (controls of B * S plans where there is a sampling descriptor)
template <size_t N>
int eval_host(const EvalOp& op, bmpc_handle h, int B, const bmpc_inputs* in, const float* controls, const EvalArg& arg,
              const void* out, const OutSlots<N>& slots) {
  if (int rc = check_eval(op, h, B, in, controls, out, slots); rc <= 0) return rc;
  HIP_TRY(hipSetDevice(h->device));
  Slices<N> o;
  if (int rc = carve(h, B, slots.s, &o); rc != BMPC_OK) return rc;
  bmpc_inputs din;
  const float* dcontrols;
  if (int rc = stage_inputs(h, B, *in, controls, arg.smp ? (size_t)arg.smp->S : 1, &din, &dcontrols); rc != BMPC_OK) return rc;
  if (int rc = op.launch(h, B, din, dcontrols, arg, o.d, h->stream); rc != BMPC_OK) return rc;
  return fetch(h, slots.s, o);
}

}  // namespace

extern "C" {

int bmpc_abi_version(void) { return BMPC_ABI_VERSION; }

const char* bmpc_last_error(void) { return g_err; }

int bmpc_supported_horizon(int h) { return resolve_path(h, BMPC_PATH_AUTO) ? 1 : 0; }

int bmpc_supported_horizon_path(int h, int path) { return resolve_path(h, path) ? 1 : 0; }

int bmpc_effective_penalties(const bmpc_params* params, double* out5) {
  if (!params || !out5) return fail(BMPC_ERR_INVALID, "null argument");
  bmpc::DevParams d;
  int rc = make_dev_params(*params, &d);
  if (rc != BMPC_OK) return rc;
  out5[0] = d.rho; out5[1] = d.rho_eq; out5[2] = d.rho_lo; out5[3] = d.rho_hi_f; out5[4] = d.rho_hi_m;
  return BMPC_OK;
}

int bmpc_solver_path(bmpc_handle h) {
  if (!h) return fail(BMPC_ERR_INVALID, "null handle");
  return h->path;
}

int bmpc_rescue_enabled(bmpc_handle h) {
  if (!h) return fail(BMPC_ERR_INVALID, "null handle");
  return h->rescue_on ? 1 : 0;
}

int bmpc_default_params(bmpc_params* p, int h) {
  if (!p) return fail(BMPC_ERR_INVALID, "null params");
  default_params(p, h);
  return BMPC_OK;
}

int bmpc_create(bmpc_handle* out, const bmpc_params* params, int device, int max_batch) {
  if (!out || !params) return fail(BMPC_ERR_INVALID, "null argument");
  *out = nullptr;
  if (max_batch < 1) return fail(BMPC_ERR_INVALID, "max_batch must be >= 1");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(BMPC_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
  if (device < 0 || device >= ndev) return fail(BMPC_ERR_INVALID, "device %d outside [0, %d)", device, ndev);
  bmpc::DevParams dev;
  int rc = make_dev_params(*params, &dev);
  if (rc != BMPC_OK) return rc;
  bmpc_handle h = new (std::nothrow) bmpc_handle_s();
  if (!h) return fail(BMPC_ERR_ALLOC, "out of host memory");
  h->device = device; h->max_batch = max_batch; h->params = *params; h->dev = dev;
  h->path = resolve_path(params->h, params->path);
  h->rescue_on = resolve_rescue(*params);
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreate(&h->ev0);
  if (e == hipSuccess) e = hipEventCreate(&h->ev1);
  {
    // chunk streams of the host-pointer path: the first chunk on the highest priority the device offers, the last ones on the
    // lowest, so that the workgroup dispatcher serves the chunks in order and the first results leave early
    int least = 0, greatest = 0;
    if (e == hipSuccess) e = hipDeviceGetStreamPriorityRange(&least, &greatest);
    h->host_timing = std::getenv("BMPC_HOST_TIMING") != nullptr;
    if (h->host_timing) std::fprintf(stderr, "[bmpc host path] stream priorities: least %d greatest %d\n", least, greatest);
    if (const char* ev = std::getenv("BMPC_HOST_CUTS")) {          // (experiments: "0.5,0.8", "0.6" for two chunks, "1" for one)
      double a = 1.0, b = 1.0;
      const int k = std::sscanf(ev, "%lf,%lf", &a, &b);
      if (k == 1 && a >= 1.0) h->host_chunks = 1;
      else if (k == 1 && a > 0.0) { h->host_chunks = 2; h->host_cut[1] = a; h->host_cut[2] = 1.0; }
      else if (k == 2 && a > 0.0 && a <= b && b <= 1.0) { h->host_cut[1] = a; h->host_cut[2] = b; }
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->cev_own, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->cev_in, hipEventDisableTiming);
    for (int c = 0; c < bmpc_handle_s::HOST_CHUNKS && e == hipSuccess; ++c) {
      int prio = greatest + c;                   // (numerically lower = more urgent)
      if (prio > least) prio = least;
      e = hipStreamCreateWithPriority(&h->cstream[c], hipStreamNonBlocking, prio);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&h->cev[c], hipEventDisableTiming);
    }
  }
  if (e != hipSuccess) {
    bmpc_destroy(h);
    return fail(BMPC_ERR_HIP, "bmpc_create: %s", hipGetErrorString(e));
  }
  *out = h;
  return BMPC_OK;
}

int bmpc_destroy(bmpc_handle h) {
  if (!h) return BMPC_OK;                       // (bmpc_create's failure path comes here with some streams and events still null)
  (void)hipSetDevice(h->device);
  const hipStream_t streams[] = {h->stream, h->cstream[0], h->cstream[1], h->cstream[2]};
  const hipEvent_t events[] = {h->cev[0], h->cev[1], h->cev[2], h->cev_own, h->cev_in, h->ev0, h->ev1};
  static_assert(bmpc_handle_s::HOST_CHUNKS == 3, "one entry per chunk stream and event above");
  // nothing is freed under a running copy or kernel: every stream of the handle is drained first
  for (hipStream_t st : streams)
    if (st) (void)hipStreamSynchronize(st);
  delete h;                                     // every DevBuf / PinnedBuf / RetiringPinnedBuf member frees itself
  for (hipEvent_t ev : events)
    if (ev) (void)hipEventDestroy(ev);
  for (hipStream_t st : streams)
    if (st) (void)hipStreamDestroy(st);
  return BMPC_OK;
}

int bmpc_set_params(bmpc_handle h, const bmpc_params* params) {
  if (!h || !params) return fail(BMPC_ERR_INVALID, "null argument");
  if (params->h != h->params.h) return fail(BMPC_ERR_INVALID, "horizon is fixed at creation (h=%d)", h->params.h);
  bmpc::DevParams dev;
  int rc = make_dev_params(*params, &dev);
  if (rc != BMPC_OK) return rc;
  if (resolve_path(params->h, params->path) != h->path) h->warm_valid = false;   // the two families keep different state
  h->params = *params; h->dev = dev;
  h->path = resolve_path(params->h, params->path);
  h->rescue_on = resolve_rescue(*params);
  return BMPC_OK;
}

int bmpc_get_params(bmpc_handle h, bmpc_params* out) {
  if (!h || !out) return fail(BMPC_ERR_INVALID, "null argument");
  *out = h->params;
  return BMPC_OK;
}

int bmpc_solve_batch_device(bmpc_handle h, int B, const float* x_fb, const float* foot, const uint8_t* contact,
                            const int32_t* phase, const float* x_cmd, const float* mu, float* controls,
                            float* states, int32_t* iters, float* residuals, int32_t* status, int32_t* nfactor,
                            void* stream) {
  if (!h) return fail(BMPC_ERR_INVALID, "null handle");
  SolveIO io;
  io.in = {x_fb, foot, contact, phase, x_cmd, mu, nullptr, nullptr};
  io.controls = controls; io.states = states; io.iters = iters; io.resid = residuals; io.status = status; io.nfactor = nfactor;
  return solve_device_ordered(h, B, io, stream, h->order);
}

int bmpc_solve_inputs_device(bmpc_handle h, int B, const bmpc_inputs* in, float* controls, float* states, int32_t* iters,
                             float* residuals, int32_t* status, int32_t* nfactor, void* stream) {
  if (!h) return fail(BMPC_ERR_INVALID, "null handle");
  if (!in) return fail(BMPC_ERR_INVALID, "null bmpc_inputs");
  SolveIO io;
  io.in = *in;
  io.controls = controls; io.states = states; io.iters = iters; io.resid = residuals; io.status = status; io.nfactor = nfactor;
  return solve_device_ordered(h, B, io, stream, h->order);
}

int bmpc_host_io(bmpc_handle h, int B, int with_x_cmd, int with_mu, int with_states, bmpc_host_views* out) {
  if (!h || !out) return fail(BMPC_ERR_INVALID, "null argument");
  if (B < 1 || B > h->max_batch) return fail(BMPC_ERR_INVALID, "batch %d outside [1, max_batch=%d]", B, h->max_batch);
  HIP_TRY(hipSetDevice(h->device));
  bmpc_handle_s::IoLayout& L = h->io;
  // inputs | outputs, every array 64-byte aligned, fp64 controls and states; B = 0 (no layout) until the block is there
  L = {packed_layout((size_t)B, (size_t)h->dev.h, (with_x_cmd ? 1u << I_XCMD : 0) | (with_mu ? 1u << I_MU : 0),
                     with_states ? 1u << O_S : 0, 64, 8)};
  h->io_gen = h->io_gen == 0x7fffffff ? 1 : h->io_gen + 1;
  // (the handle's own stream may still read the old block: a re-allocation waits for it)
  if (L.in_bytes > h->io_in.n || L.out_bytes > h->io_out.n) HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(h->io_in.ensure(L.in_bytes));
  HIP_TRY(h->io_out.ensure(L.out_bytes));
  HIP_TRY(h->io_dev.ensure(L.in_bytes));
  L.B = B;
  *out = {};                                    // (an array the layout does not hold: a null view)
  for (int i = 0; i < N_IN; ++i)
    if (L.has_in >> i & 1) set_ptr(out, IN[i].view, h->io_in.p + L.in[i]);
  for (int i = 0; i < N_OUT; ++i)
    if (L.has_out >> i & 1) set_ptr(out, OUT[i].view, h->io_out.p + L.out[i]);
  return BMPC_OK;
}

int bmpc_host_io_generation(bmpc_handle h) {
  if (!h) return fail(BMPC_ERR_INVALID, "null handle");
  return h->io_gen;
}

int bmpc_solve_batch_io(bmpc_handle h, int B) {
  if (!h) return fail(BMPC_ERR_INVALID, "null handle");
  const bmpc_handle_s::IoLayout& L = h->io;
  if (B < 1 || B != L.B) return fail(BMPC_ERR_INVALID, "bmpc_solve_batch_io: batch %d, but the I/O block is laid out for %d (bmpc_host_io)", B, L.B);
  HIP_TRY(hipSetDevice(h->device));
  const size_t n = (size_t)B, H = (size_t)h->dev.h;
  char* din = h->io_dev.p;
  char* o = h->io_out.p;
  // How the results cross PCIe (MI355X, measured in round 5): stores of a kernel into mapped host memory sustain ~8.6 GB/s, the
  // copy engine ~50 GB/s.  A 4096-instance batch returns 3.9 MB of fp64 controls and 4.3 MB of fp64 states in 0.8 ms: the
  // controls (and the per-instance counters) go straight from the kernels' epilogues into the host arrays -- free below that
  // rate --, the states are stored in HBM and follow by copy engine, chunk by chunk on the chunk streams of the host-pointer
  // path, so that only the last chunk's copy (15 % of the states) is exposed.  Everything through the kernels: +0.12 ms.
  const bool states = L.has_out >> O_S & 1;
  const ChunkPlan plan = plan_chunks(h, n, !states);     // (no states: one chunk, everything straight from the kernel)
  if (states) HIP_TRY(h->io_states.ensure(n * OUT[O_S].w.count(H)));
  HIP_TRY(chunks_after_own_stream(h, plan.n));
  int issued = 0;
  for (int c = 0; c < plan.n; ++c) {
    const size_t lo = plan.lo[c], nb = plan.nb[c];
    hipStream_t st = h->cstream[c];
    issued = c + 1;
    if (c == 0) {                               // ONE copy in, for the whole batch
      CHUNK_TRY(hipMemcpyAsync(din, h->io_in.p, L.in_bytes, hipMemcpyHostToDevice, st));
      CHUNK_TRY(hipEventRecord(h->cev_in, st));
    } else {
      CHUNK_TRY(hipStreamWaitEvent(st, h->cev_in, 0));
    }
    // (the last chunk's states go the way of the controls: nothing is left to copy when its kernel ends, and 15 % of the
    //  states on top of the controls stay well below what the kernels' own stores sustain)
    const bool by_copy = states && c < plan.n - 1;
    SolveIO io = packed_io(L, din, o, lo);
    io.controls64 = reinterpret_cast<double*>(o + L.out_at(O_U, lo));
    double* states_host = reinterpret_cast<double*>(o + L.out_at(O_S, lo));
    if (states) io.states64 = by_copy ? h->io_states.p + lo * OUT[O_S].w.count(H) : states_host;
    if (int rc = solve_device_ordered(h, (int)nb, io, st, h->order, plan.events(c)); rc != BMPC_OK) return bail(h, issued, rc);
    if (by_copy) CHUNK_TRY(hipMemcpyAsync(states_host, io.states64, nb * L.stride(OUT[O_S]), hipMemcpyDeviceToHost, st));
    CHUNK_TRY(hipEventRecord(h->cev[c], st));
  }
  for (int c = 0; c < plan.n; ++c) CHUNK_TRY(hipEventSynchronize(h->cev[c]));
#undef CHUNK_TRY
  return BMPC_OK;
}

int bmpc_solve_batch(bmpc_handle h, int B, const float* x_fb, const float* foot, const uint8_t* contact,
                     const int32_t* phase, const float* x_cmd, const float* mu, float* controls, float* states,
                     int32_t* iters, float* residuals, int32_t* status, int32_t* nfactor) {
  const bmpc_inputs in = {x_fb, foot, contact, phase, x_cmd, mu, nullptr, nullptr};
  return solve_host<float>(h, B, in, controls, states, iters, residuals, status, nfactor);
}

int bmpc_solve_batch_f64(bmpc_handle h, int B, const float* x_fb, const float* foot, const uint8_t* contact,
                         const int32_t* phase, const float* x_cmd, const float* mu, double* controls, double* states,
                         int32_t* iters, float* residuals, int32_t* status, int32_t* nfactor) {
  const bmpc_inputs in = {x_fb, foot, contact, phase, x_cmd, mu, nullptr, nullptr};
  return solve_host<double>(h, B, in, controls, states, iters, residuals, status, nfactor);
}

int bmpc_solve_inputs_f64(bmpc_handle h, int B, const bmpc_inputs* in, double* controls, double* states, int32_t* iters,
                          float* residuals, int32_t* status, int32_t* nfactor) {
  if (!h) return fail(BMPC_ERR_INVALID, "null handle");
  if (!in) return fail(BMPC_ERR_INVALID, "null bmpc_inputs");
  return solve_host<double>(h, B, *in, controls, states, iters, residuals, status, nfactor);
}

int bmpc_synchronize(bmpc_handle h) {
  if (!h) return fail(BMPC_ERR_INVALID, "null handle");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (int c = 0; c < bmpc_handle_s::HOST_CHUNKS; ++c)
    if (h->cstream[c]) HIP_TRY(hipStreamSynchronize(h->cstream[c]));
  if (h->timed) HIP_TRY(hipEventSynchronize(h->ev1));     // the last solve launch, whatever stream it was given
  return BMPC_OK;
}

int bmpc_debug_assemble_inputs(bmpc_handle h, int B, const bmpc_inputs* in, double* x_ref, double* foot_ref, double* Gt,
                               double* qt) {
  if (!h) return fail(BMPC_ERR_INVALID, "null handle");
  if (!in) return fail(BMPC_ERR_INVALID, "null bmpc_inputs");
  float dummy = 0;
  if (int rc = check_common(h, B, *in, &dummy); rc <= 0) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t NW = 6 * (size_t)h->dev.h;
  // Gt and qt are formed only where the caller asked for them: Gt alone is n (6h)^2 doubles (1.9 GB at B = 4096, h = 40), and
  // the Gt / qt views exist on the dense family only (h <= 20) -- a caller that wants the references gets them at every horizon
  if ((Gt || qt) && !dense_horizon(h->dev.h))
    return fail(BMPC_ERR_INVALID, "Gt / qt views exist for h <= 20 only (h=%d never forms them); pass NULL for both", h->dev.h);
  // (the references are formed either way; the last row is the controls an assembly launch stores: scratch)
  const OutSlot out[5] = {{x_ref, f64_view(IN[I_XREF]), true}, {foot_ref, f64_view(IN[I_FREF]), true}, {Gt, {NW * NW, 0, 8}},
                          {qt, {NW, 0, 8}}, {nullptr, controls_width(), true}};
  Slices<5> o;
  if (int rc = carve(h, B, out, &o); rc != BMPC_OK) return rc;
  HIP_TRY(hipMemsetAsync(h->host_out.p, 0, o.total, h->stream));
  SolveIO io;
  const float* none;
  if (int rc = stage_inputs(h, B, *in, nullptr, 1, &io.in, &none); rc != BMPC_OK) return rc;
  io.controls = o.at<float>(4);
  const bmpc::DebugOut dbg = {o.at<double>(0), o.at<double>(1), o.at<double>(2), o.at<double>(3), nullptr, 1};
  if (int rc = launch(h, B, io, dbg, h->stream, nullptr); rc != BMPC_OK) return rc;
  return fetch(h, out, o);
}

int bmpc_debug_assemble(bmpc_handle h, int B, const float* x_fb, const float* foot, const uint8_t* contact,
                        const int32_t* phase, const float* x_cmd, const float* mu, double* x_ref, double* foot_ref,
                        double* Gt, double* qt) {
  const bmpc_inputs in = {x_fb, foot, contact, phase, x_cmd, mu, nullptr, nullptr};
  return bmpc_debug_assemble_inputs(h, B, &in, x_ref, foot_ref, Gt, qt);
}

// ---- the evaluation family (helpers above): evaluation of given controls, the gradient of its cost, the KKT certificate

int bmpc_evaluate_device(bmpc_handle h, int B, const bmpc_inputs* in, const float* controls, const bmpc_eval_out* out, void* stream) {
  return eval_device(EVALUATE, h, B, in, controls, {}, out, slots_of(out), stream);
}

int bmpc_evaluate(bmpc_handle h, int B, const bmpc_inputs* in, const float* controls, const bmpc_eval_out* out) {
  return eval_host(EVALUATE, h, B, in, controls, {}, out, slots_of(out));
}

int bmpc_evaluate_grad_device(bmpc_handle h, int B, const bmpc_inputs* in, const float* controls, const bmpc_grad_out* out, void* stream) {
  return eval_device(EVALUATE_GRAD, h, B, in, controls, {}, out, slots_of(out), stream);
}

int bmpc_evaluate_grad(bmpc_handle h, int B, const bmpc_inputs* in, const float* controls, const bmpc_grad_out* out) {
  return eval_host(EVALUATE_GRAD, h, B, in, controls, {}, out, slots_of(out));
}

int bmpc_certify_device(bmpc_handle h, int B, const bmpc_inputs* in, const float* controls, double act_tol, const bmpc_cert_out* out,
                        void* stream) {
  if (act_tol != act_tol) return fail(BMPC_ERR_INVALID, "act_tol is NaN");
  return eval_device(CERTIFY, h, B, in, controls, {act_tol}, out, slots_of(out), stream);
}

int bmpc_certify(bmpc_handle h, int B, const bmpc_inputs* in, const float* controls, double act_tol, const bmpc_cert_out* out) {
  if (act_tol != act_tol) return fail(BMPC_ERR_INVALID, "act_tol is NaN");
  return eval_host(CERTIFY, h, B, in, controls, {act_tol}, out, slots_of(out));
}

int bmpc_evaluate_samples_device(bmpc_handle h, int B, const bmpc_inputs* in, const float* controls, const bmpc_samples* smp,
                                 const bmpc_samples_out* out, void* stream) {
  if (int rc = check_samples(smp); rc != BMPC_OK) return rc;
  return eval_device(EVALUATE_SAMPLES, h, B, in, controls, {0.0, smp}, out, slots_of(out, smp), stream);
}

int bmpc_evaluate_samples(bmpc_handle h, int B, const bmpc_inputs* in, const float* controls, const bmpc_samples* smp,
                          const bmpc_samples_out* out) {
  if (int rc = check_samples(smp); rc != BMPC_OK) return rc;
  return eval_host(EVALUATE_SAMPLES, h, B, in, controls, {0.0, smp}, out, slots_of(out, smp));
}

static bmpc::LowLevelParams ll_params(const bmpc_params& p) {
  bmpc::LowLevelParams q;
  q.h = p.h; q.dt = p.dt; q.kv = p.kv; q.swing_height = p.swingHeight;
  for (int i = 0; i < 12; ++i) q.x_cmd[i] = p.x_cmd[i];
  for (int i = 0; i < 9; ++i) { q.kp[i] = p.kp[i]; q.kd[i] = p.kd[i]; }
  for (int i = 0; i < 3; ++i) q.hip_offset[i] = p.hip_offset[i];
  return q;
}

int bmpc_foot_position_world_device(bmpc_handle h, int B, const float* x_fb, const float* q, float* pf_w, void* stream) {
  if (int rc = check_batch(h, B); rc <= 0) return rc;
  if (!x_fb || !q || !pf_w) return fail(BMPC_ERR_INVALID, "null pointer");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = pick_stream(h, stream);
  hipLaunchKernelGGL(bmpc::foot_world_kernel, dim3((B + 255) / 256), dim3(256), 0, st, ll_params(h->params), B, x_fb, q, pf_w);
  HIP_TRY(hipGetLastError());
  return BMPC_OK;
}

int bmpc_foot_position_world(bmpc_handle h, int B, const float* x_fb, const float* q, float* pf_w) {
  if (int rc = check_batch(h, B); rc <= 0) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const InSlot in[2] = {{x_fb, IN[I_XFB].w}, {q, W_JOINTS}};
  const OutSlot out[1] = {{pf_w, W_FEET}};
  Slices<2> d; Slices<1> o;
  if (int rc = stage(h, B, in, &d, out, &o); rc != BMPC_OK) return rc;
  // (a null array is an absent row and a null pointer: the twin refuses it)
  const int rc = bmpc_foot_position_world_device(h, B, d.at<float>(0), d.at<float>(1), o.at<float>(0), h->stream);
  return rc != BMPC_OK ? rc : fetch(h, out, o);
}

int bmpc_low_level_control_device(bmpc_handle h, int B, const float* x_fb, const double* t, const float* pf_w,
                                  const float* q, const float* qd, const uint8_t* contact0, const float* u0,
                                  float* tau, void* stream) {
  if (int rc = check_batch(h, B); rc <= 0) return rc;
  if (!x_fb || !t || !pf_w || !q || !qd || !contact0 || !u0 || !tau) return fail(BMPC_ERR_INVALID, "null pointer");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = pick_stream(h, stream);
  hipLaunchKernelGGL(bmpc::lowlevel_kernel, dim3((B + 255) / 256), dim3(256), 0, st, ll_params(h->params), B, x_fb, t,
                     pf_w, q, qd, contact0, u0, tau);
  HIP_TRY(hipGetLastError());
  return BMPC_OK;
}

int bmpc_low_level_control(bmpc_handle h, int B, const float* x_fb, const double* t, const float* pf_w,
                           const float* q, const float* qd, const uint8_t* contact0, const float* u0, float* tau) {
  if (int rc = check_batch(h, B); rc <= 0) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const InSlot in[7] = {{x_fb, IN[I_XFB].w}, {t, W_T}, {pf_w, W_FEET}, {q, W_JOINTS}, {qd, W_JOINTS}, {contact0, W_CONTACT0}, {u0, W_U0}};
  const OutSlot out[1] = {{tau, W_JOINTS}};
  Slices<7> d; Slices<1> o;
  if (int rc = stage(h, B, in, &d, out, &o); rc != BMPC_OK) return rc;
  const int rc = bmpc_low_level_control_device(h, B, d.at<float>(0), d.at<double>(1), d.at<float>(2), d.at<float>(3), d.at<float>(4),
                                             d.at<uint8_t>(5), d.at<float>(6), o.at<float>(0), h->stream);
  return rc != BMPC_OK ? rc : fetch(h, out, o);
}

int bmpc_gait_default(bmpc_gait* g, int half) {
  if (!g) return fail(BMPC_ERR_INVALID, "null gait");
  if (half < 1) return fail(BMPC_ERR_INVALID, "half period must be >= 1");
  g->period = 2 * half;
  g->offset[0] = 0; g->offset[1] = half;      // REF:52-55: leg 1 stands first, leg 2 half a period later
  g->duty[0] = half; g->duty[1] = half;
  return BMPC_OK;
}

static int gait_params(bmpc_handle h, const bmpc_gait* gait, bmpc::GaitParams* G) {
  bmpc_gait g;
  if (gait) g = *gait;
  else bmpc_gait_default(&g, h->params.half);
  if (g.period < 1) return fail(BMPC_ERR_INVALID, "gait period must be >= 1");
  for (int k = 0; k < 2; ++k)
    if (g.duty[k] < 0 || g.duty[k] > g.period) return fail(BMPC_ERR_INVALID, "gait duty must be in [0, period]");
  G->h = h->params.h; G->period = g.period; G->dt = h->params.dt;
  for (int k = 0; k < 2; ++k) { G->offset[k] = g.offset[k]; G->duty[k] = g.duty[k]; }
  return BMPC_OK;
}

int bmpc_contact_sequence_device(bmpc_handle h, int B, const double* t, const bmpc_gait* gait, int32_t* phase,
                                 uint8_t* contact, void* stream) {
  if (int rc = check_batch(h, B); rc <= 0) return rc;
  if (!t) return fail(BMPC_ERR_INVALID, "null pointer");
  bmpc::GaitParams G;
  int rc = gait_params(h, gait, &G);
  if (rc != BMPC_OK) return rc;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = pick_stream(h, stream);
  hipLaunchKernelGGL(bmpc::gait_kernel, dim3((B + 255) / 256), dim3(256), 0, st, G, B, t, phase, contact);
  HIP_TRY(hipGetLastError());
  return BMPC_OK;
}

int bmpc_contact_sequence(bmpc_handle h, int B, const double* t, const bmpc_gait* gait, int32_t* phase, uint8_t* contact) {
  if (int rc = check_batch(h, B); rc <= 0) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const InSlot in[1] = {{t, W_T}};
  const OutSlot out[2] = {{phase, IN[I_PHASE].w, true}, {contact, IN[I_CON].w, true}};     // (both formed, either may be unwanted)
  Slices<1> d; Slices<2> o;
  if (int rc = stage(h, B, in, &d, out, &o); rc != BMPC_OK) return rc;
  const int rc = bmpc_contact_sequence_device(h, B, d.at<double>(0), gait, o.at<int32_t>(0), o.at<uint8_t>(1), h->stream);
  return rc != BMPC_OK ? rc : fetch(h, out, o);
}

int bmpc_set_warm_start(bmpc_handle h, int enable, int shift, double theta) {
  if (!h) return fail(BMPC_ERR_INVALID, "null handle");
  if (shift < 0 || shift >= h->params.h) return fail(BMPC_ERR_INVALID, "shift must be in [0, h)");
  if (!(theta >= 0.0 && theta <= 1.0)) return fail(BMPC_ERR_INVALID, "theta must be in [0, 1]");
  h->warm_on = enable != 0;
  h->warm_shift = shift;
  h->warm_theta = (float)theta;
  if (!h->warm_on) h->warm_valid = false;
  return BMPC_OK;
}

int bmpc_reset_warm_start(bmpc_handle h) {
  if (!h) return fail(BMPC_ERR_INVALID, "null handle");
  h->warm_valid = false;
  return BMPC_OK;
}

// period s of a trajectory array of `per_period` elements a period (null: not recorded)
extern "C++" template <typename T>
static T* period_slice(T* traj, int s, size_t per_period) { return traj ? traj + (size_t)s * per_period : nullptr; }

// The closed loop bmpc_rollout_device and bmpc_simulate_device share: per period  t -> (phase, contact)  ->  dispatch order (from the
// second period on, where the roll-out orders its own: the instances that iterated longest last period go first)  ->  solve  ->
// `feedback(s, st)`, the launch that closes the loop and records period s -- the only difference between the two entries.  All on
// one stream, no host arithmetic, no synchronisation; the ro_* scratch holds the solve's outputs.
extern "C++" template <typename Feedback>
static int closed_loop(bmpc_handle h, int B, int steps, const float* x_fb, const float* foot, double* t, const bmpc_gait* gait,
                       const float* x_cmd, const float* mu, int32_t* status_any, void* stream, Feedback feedback) {
  HIP_TRY(hipSetDevice(h->device));
  const size_t n = (size_t)B, H = (size_t)h->dev.h;
  HIP_TRY(h->ro_controls.ensure(n * OUT[O_U].w.count(H))); HIP_TRY(h->ro_states.ensure(n * OUT[O_S].w.count(H)));
  HIP_TRY(h->ro_contact.ensure(n * IN[I_CON].w.count(H))); HIP_TRY(h->ro_phase.ensure(n));
  HIP_TRY(h->ro_iters.ensure(n)); HIP_TRY(h->ro_status.ensure(n));
  hipStream_t st = pick_stream(h, stream);
  if (status_any) HIP_TRY(hipMemsetAsync(status_any, 0, n * sizeof(int32_t), st));
  const int32_t* order = h->order;                 // this roll-out's dispatch order (the handle's is left alone)
  const bool own_order = h->longest_first && !order;
  if (own_order) HIP_TRY(h->ro_order.ensure(n));
  SolveIO io;
  io.in = {x_fb, foot, h->ro_contact.p, h->ro_phase.p, x_cmd, mu, nullptr, nullptr};
  io.controls = h->ro_controls.p; io.states = h->ro_states.p; io.iters = h->ro_iters.p; io.status = h->ro_status.p;
  int rc = BMPC_OK;
  for (int s = 0; s < steps && rc == BMPC_OK; ++s) {
    rc = bmpc_contact_sequence_device(h, B, t, gait, h->ro_phase.p, h->ro_contact.p, st);
    if (rc != BMPC_OK) break;
    if (own_order && s > 0) {
      hipLaunchKernelGGL(bmpc::dispatch_order_kernel, dim3(1), dim3(1024), 0, st, B, h->ro_iters.p, h->ro_order.p);
      if (hipGetLastError() != hipSuccess) { rc = fail(BMPC_ERR_HIP, "dispatch-order launch failed"); break; }
      order = h->ro_order.p;
    }
    rc = solve_device_ordered(h, B, io, stream, order);
    if (rc != BMPC_OK) break;
    feedback(s, st);
    if (hipGetLastError() != hipSuccess) rc = fail(BMPC_ERR_HIP, "roll-out launch failed");
  }
  return rc;
}

int bmpc_rollout_device(bmpc_handle h, int B, int steps, float* x_fb, const float* foot, double* t,
                        const bmpc_gait* gait, const float* x_cmd, const float* mu, float* u0_traj, float* x_traj,
                        int32_t* iters_traj, int32_t* status_any, void* stream) {
  if (int rc = check_batch(h, B); rc < 0) return rc;
  if (steps < 0) return fail(BMPC_ERR_INVALID, "steps must be >= 0");
  if (B == 0 || steps == 0) return BMPC_OK;
  if (!x_fb || !foot || !t) return fail(BMPC_ERR_INVALID, "x_fb, foot and t must be non-null");
  const size_t n = (size_t)B;
  // x_fb <- states[:, 0], t += dt
  return closed_loop(h, B, steps, x_fb, foot, t, gait, x_cmd, mu, status_any, stream, [&](int s, hipStream_t st) {
    hipLaunchKernelGGL(bmpc::rollout_feedback_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, (int)h->dev.h, h->params.dt,
                       h->ro_states.p, h->ro_controls.p, h->ro_iters.p, h->ro_status.p, x_fb, t,
                       period_slice(u0_traj, s, n * 12), period_slice(x_traj, s, n * 12), period_slice(iters_traj, s, n), status_any);
  });
}

// ---- the plant and the closed loop on it (bmpc_plant.hip)

int bmpc_plant_default(bmpc_plant* p) {
  if (!p) return fail(BMPC_ERR_INVALID, "null plant");
  p->integrator = BMPC_PLANT_RK4; p->substeps = 4; p->move_feet = 1; p->push_from = 0; p->push_steps = 0;
  return BMPC_OK;
}

// `plant` (null: the default) checked and resolved; host arithmetic only, before a handle or a device is looked at
static int plant_opts(const bmpc_plant* plant, bmpc_plant* out) {
  if (plant) *out = *plant;
  else bmpc_plant_default(out);
  if (out->integrator != BMPC_PLANT_EULER && out->integrator != BMPC_PLANT_RK4)
    return fail(BMPC_ERR_INVALID, "unknown integrator %d", out->integrator);
  if (out->substeps < 1 || out->substeps > bmpc::PLANT_MAX_SUBSTEPS)
    return fail(BMPC_ERR_INVALID, "substeps %d outside [1, %d]", out->substeps, bmpc::PLANT_MAX_SUBSTEPS);
  if (out->push_from < 0 || out->push_steps < 0) return fail(BMPC_ERR_INVALID, "push_from and push_steps must be >= 0");
  return BMPC_OK;
}

static bmpc::PlantParams plant_params(bmpc_handle h) {
  const bmpc_params& p = h->params;
  bmpc::PlantParams q;
  q.h = p.h; q.dt = p.dt; q.kv = p.kv; q.m = p.m; q.g = p.g;
  q.cmd_x = p.x_cmd[3]; q.cmd_y = p.x_cmd[4];
  for (int i = 0; i < 9; ++i) { q.Ib[i] = p.I[i]; q.Ibinv[i] = h->dev.Iinv[i]; }
  return q;
}

// whether a body / an outcome asks for anything: without, the entries run the kernels of the handle's own body
static bool has_body(const bmpc_plant_body* b) { return b && (b->m || b->I || b->g); }
static bool has_outcome(const bmpc_sim_outcome* o) { return o && (o->first_fall || o->max_tilt || o->min_z); }
static bool has_ground_sum(const bmpc_ground_out* o) { return o && (o->first_slip || o->slip_periods || o->unloaded_periods || o->mu_demand); }

// what a ground entry is asked to record without a ground to record it of; host logic only, checked with the plant block
static int ground_opts(const bmpc_plant_ground* ground, const void* u_applied, const void* flags, const bmpc_ground_out* gout) {
  if (gout && !(gout->fz_floor >= 0.0)) return fail(BMPC_ERR_INVALID, "fz_floor must be >= 0 and not NaN");
  if (!ground && (u_applied || flags || gout)) return fail(BMPC_ERR_INVALID, "u_applied, flags and gout need a ground");
  return BMPC_OK;
}

// bmpc_plant_step_device, bmpc_plant_step_body_device and bmpc_plant_step_ground_device: without a ground, `body` null or empty
// launches plant_step_kernel; with a ground (its mu null: the handle's) plant_step_ground_kernel, whatever the body
static int plant_step_device(bmpc_handle h, int B, const bmpc_plant* plant, const bmpc_plant_body* body, const bmpc_plant_ground* ground,
                             const float* x_fb, const float* u0, const float* foot, const uint8_t* contact0, const float* wrench,
                             float* x_next, float* u_applied, uint8_t* flags, void* stream) {
  bmpc_plant o;
  if (int rc = plant_opts(plant, &o); rc != BMPC_OK) return rc;
  if (int rc = ground_opts(ground, u_applied, flags, nullptr); rc != BMPC_OK) return rc;
  if (int rc = check_batch(h, B); rc <= 0) return rc;
  if (!x_fb || !u0 || !foot || !contact0 || !x_next) return fail(BMPC_ERR_INVALID, "x_fb, u0, foot, contact0 and x_next must be non-null");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = pick_stream(h, stream);
  const bmpc::PlantScheme S = bmpc::plant_scheme(h->params.dt, o.integrator, o.substeps);
  const bmpc::PlantBody Bd = has_body(body) ? bmpc::PlantBody{body->m, body->I, body->g} : bmpc::PlantBody{nullptr, nullptr, nullptr};
  if (ground)
    hipLaunchKernelGGL(bmpc::plant_step_ground_kernel, dim3((B + 255) / 256), dim3(256), 0, st, plant_params(h), Bd,
                       bmpc::PlantGround{ground->mu, h->params.mu, u_applied, flags}, S, B, x_fb, u0, foot, contact0, wrench, x_next);
  else if (has_body(body))
    hipLaunchKernelGGL(bmpc::plant_step_body_kernel, dim3((B + 255) / 256), dim3(256), 0, st, plant_params(h), Bd, S, B, x_fb, u0,
                       foot, contact0, wrench, x_next);
  else
    hipLaunchKernelGGL(bmpc::plant_step_kernel, dim3((B + 255) / 256), dim3(256), 0, st, plant_params(h), S, B, x_fb, u0, foot,
                       contact0, wrench, x_next);
  HIP_TRY(hipGetLastError());
  return BMPC_OK;
}

// bmpc_plant_step, bmpc_plant_step_body and bmpc_plant_step_ground
static int plant_step_host(bmpc_handle h, int B, const bmpc_plant* plant, const bmpc_plant_body* body, const bmpc_plant_ground* ground,
                           const float* x_fb, const float* u0, const float* foot, const uint8_t* contact0, const float* wrench,
                           float* x_next, float* u_applied, uint8_t* flags) {
  bmpc_plant o;
  if (int rc = plant_opts(plant, &o); rc != BMPC_OK) return rc;
  if (int rc = ground_opts(ground, u_applied, flags, nullptr); rc != BMPC_OK) return rc;
  if (int rc = check_batch(h, B); rc <= 0) return rc;
  if (!x_fb || !u0 || !foot || !contact0 || !x_next) return fail(BMPC_ERR_INVALID, "x_fb, u0, foot, contact0 and x_next must be non-null");
  HIP_TRY(hipSetDevice(h->device));
  const InSlot in[9] = {{x_fb, IN[I_XFB].w}, {u0, W_U0}, {foot, W_FEET}, {contact0, W_CONTACT0}, {wrench, W_WRENCH},
                        {body ? body->m : nullptr, W_MASS}, {body ? body->I : nullptr, W_INERTIA}, {body ? body->g : nullptr, W_GRAVITY},
                        {ground ? ground->mu : nullptr, W_GROUND_MU}};
  const OutSlot out[3] = {{x_next, IN[I_XFB].w}, {u_applied, W_U0}, {flags, W_FLAGS}};
  Slices<9> d; Slices<3> r;
  if (int rc = stage(h, B, in, &d, out, &r); rc != BMPC_OK) return rc;
  const bmpc_plant_body d_body = {d.at<double>(5), d.at<double>(6), d.at<double>(7)};
  const bmpc_plant_ground d_ground = {d.at<double>(8)};
  const int rc = plant_step_device(h, B, &o, &d_body, ground ? &d_ground : nullptr, d.at<float>(0), d.at<float>(1), d.at<float>(2),
                                 d.at<uint8_t>(3), d.at<float>(4), r.at<float>(0), r.at<float>(1), r.at<uint8_t>(2), h->stream);
  return rc != BMPC_OK ? rc : fetch(h, out, r);
}

int bmpc_plant_step_device(bmpc_handle h, int B, const bmpc_plant* plant, const float* x_fb, const float* u0, const float* foot,
                           const uint8_t* contact0, const float* wrench, float* x_next, void* stream) {
  return plant_step_device(h, B, plant, nullptr, nullptr, x_fb, u0, foot, contact0, wrench, x_next, nullptr, nullptr, stream);
}

int bmpc_plant_step(bmpc_handle h, int B, const bmpc_plant* plant, const float* x_fb, const float* u0, const float* foot,
                    const uint8_t* contact0, const float* wrench, float* x_next) {
  return plant_step_host(h, B, plant, nullptr, nullptr, x_fb, u0, foot, contact0, wrench, x_next, nullptr, nullptr);
}

int bmpc_plant_step_body_device(bmpc_handle h, int B, const bmpc_plant* plant, const bmpc_plant_body* body, const float* x_fb,
                                const float* u0, const float* foot, const uint8_t* contact0, const float* wrench, float* x_next,
                                void* stream) {
  return plant_step_device(h, B, plant, body, nullptr, x_fb, u0, foot, contact0, wrench, x_next, nullptr, nullptr, stream);
}

int bmpc_plant_step_body(bmpc_handle h, int B, const bmpc_plant* plant, const bmpc_plant_body* body, const float* x_fb,
                         const float* u0, const float* foot, const uint8_t* contact0, const float* wrench, float* x_next) {
  return plant_step_host(h, B, plant, body, nullptr, x_fb, u0, foot, contact0, wrench, x_next, nullptr, nullptr);
}

int bmpc_plant_step_ground_device(bmpc_handle h, int B, const bmpc_plant* plant, const bmpc_plant_body* body,
                                  const bmpc_plant_ground* ground, const float* x_fb, const float* u0, const float* foot,
                                  const uint8_t* contact0, const float* wrench, float* x_next, float* u_applied, uint8_t* flags,
                                  void* stream) {
  return plant_step_device(h, B, plant, body, ground, x_fb, u0, foot, contact0, wrench, x_next, u_applied, flags, stream);
}

int bmpc_plant_step_ground(bmpc_handle h, int B, const bmpc_plant* plant, const bmpc_plant_body* body, const bmpc_plant_ground* ground,
                           const float* x_fb, const float* u0, const float* foot, const uint8_t* contact0, const float* wrench,
                           float* x_next, float* u_applied, uint8_t* flags) {
  return plant_step_host(h, B, plant, body, ground, x_fb, u0, foot, contact0, wrench, x_next, u_applied, flags);
}

// bmpc_simulate_device, bmpc_simulate_body_device and bmpc_simulate_ground_device: closed_loop() with the plant's feedback step.
// Without a ground, a body and an outcome that step is simulate_feedback_kernel; without a ground simulate_body_feedback_kernel;
// with one simulate_ground_feedback_kernel, and ground_reduce_kernel in front of it where a reduced array is wanted.  The
// outcome's and the ground's reduced arrays are initialised on the stream (-1, NaN, NaN; -1, 0, 0, NaN; status_any is zeroed by
// closed_loop the same way).
static int simulate(bmpc_handle h, int B, int steps, const bmpc_plant* plant, const bmpc_plant_body* body, const bmpc_plant_ground* ground,
                    float* x_fb, float* foot, double* t, const bmpc_gait* gait, const float* x_cmd, const float* mu, const float* push,
                    float* u0_traj, float* x_traj, float* foot_traj, int32_t* iters_traj, int32_t* status_any,
                    const bmpc_sim_outcome* outcome, const bmpc_ground_out* gout, void* stream) {
  bmpc_plant o;
  if (int rc = plant_opts(plant, &o); rc != BMPC_OK) return rc;
  if (outcome && (outcome->tilt_max != outcome->tilt_max || outcome->z_min != outcome->z_min))
    return fail(BMPC_ERR_INVALID, "outcome thresholds tilt_max and z_min must not be NaN");
  if (int rc = ground_opts(ground, nullptr, nullptr, gout); rc != BMPC_OK) return rc;
  if (int rc = check_batch(h, B); rc < 0) return rc;
  if (steps < 0) return fail(BMPC_ERR_INVALID, "steps must be >= 0");
  if (B == 0 || steps == 0) return BMPC_OK;
  if (!x_fb || !foot || !t) return fail(BMPC_ERR_INVALID, "x_fb, foot and t must be non-null");
  bmpc::GaitParams G;
  if (int rc = gait_params(h, gait, &G); rc != BMPC_OK) return rc;
  const size_t n = (size_t)B;
  const bmpc::PlantParams P = plant_params(h);
  const bmpc::PlantScheme S = bmpc::plant_scheme(h->params.dt, o.integrator, o.substeps);
  const bmpc::PlantGait PG = {G.period, {G.offset[0], G.offset[1]}, {G.duty[0], G.duty[1]}, o.move_feet != 0};
  const bool ext = has_body(body) || has_outcome(outcome);
  const bmpc::PlantBody Bd = has_body(body) ? bmpc::PlantBody{body->m, body->I, body->g} : bmpc::PlantBody{nullptr, nullptr, nullptr};
  bmpc::PlantOutcome O = {0.0, 0.0, nullptr, nullptr, nullptr};
  if (has_outcome(outcome)) {
    O = {outcome->tilt_max, outcome->z_min, outcome->first_fall, outcome->max_tilt, outcome->min_z};
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = pick_stream(h, stream);
    if (O.first_fall) HIP_TRY(hipMemsetAsync(O.first_fall, 0xff, n * sizeof(int32_t), st));               // -1
    if (O.max_tilt) HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(O.max_tilt), 0x7fc00000, n, st));   // NaN
    if (O.min_z) HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(O.min_z), 0x7fc00000, n, st));
  }
  bmpc::PlantGroundSum R = {0.0, nullptr, nullptr, nullptr, nullptr};
  if (has_ground_sum(gout)) {
    R = {gout->fz_floor, gout->first_slip, gout->slip_periods, gout->unloaded_periods, gout->mu_demand};
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = pick_stream(h, stream);
    if (R.first_slip) HIP_TRY(hipMemsetAsync(R.first_slip, 0xff, n * sizeof(int32_t), st));              // -1
    if (R.slip_periods) HIP_TRY(hipMemsetAsync(R.slip_periods, 0, n * 2 * sizeof(int32_t), st));
    if (R.unloaded_periods) HIP_TRY(hipMemsetAsync(R.unloaded_periods, 0, n * 2 * sizeof(int32_t), st));
    if (R.mu_demand) HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(R.mu_demand), 0x7fc00000, n, st));   // NaN
  }
  return closed_loop(h, B, steps, x_fb, foot, t, gait, x_cmd, mu, status_any, stream, [&](int s, hipStream_t st) {
    const bool push_on = push && s >= o.push_from && s - o.push_from < o.push_steps;
    const float* w = push_on ? push : nullptr;
    float *u0_s = period_slice(u0_traj, s, n * 12), *x_s = period_slice(x_traj, s, n * 12), *foot_s = period_slice(foot_traj, s, n * 6);
    int32_t* iters_s = period_slice(iters_traj, s, n);
    if (ground) {
      // (the reduction first: it reads the solve's outputs, which the feedback step leaves alone, and nothing that step writes)
      if (has_ground_sum(gout))
        hipLaunchKernelGGL(bmpc::ground_reduce_kernel, dim3((B + 255) / 256), dim3(256), 0, st, ground->mu, h->params.mu, R, s, B,
                           (int)h->dev.h, h->ro_controls.p, h->ro_contact.p);
      const bmpc::PlantGround Gr = {ground->mu, h->params.mu, period_slice(gout ? gout->u_applied : nullptr, s, n * 12),
                                    period_slice(gout ? gout->flags : nullptr, s, n)};
      hipLaunchKernelGGL(bmpc::simulate_ground_feedback_kernel, dim3((B + 255) / 256), dim3(256), 0, st, P, Bd, O, Gr, s, S, PG, B,
                         h->ro_controls.p, h->ro_contact.p, h->ro_iters.p, h->ro_status.p, w, x_cmd, x_fb, foot, t, u0_s, x_s, foot_s,
                         iters_s, status_any);
    } else if (ext)
      hipLaunchKernelGGL(bmpc::simulate_body_feedback_kernel, dim3((B + 255) / 256), dim3(256), 0, st, P, Bd, O, s, S, PG, B,
                         h->ro_controls.p, h->ro_contact.p, h->ro_iters.p, h->ro_status.p, w, x_cmd, x_fb, foot, t, u0_s, x_s, foot_s,
                         iters_s, status_any);
    else
      hipLaunchKernelGGL(bmpc::simulate_feedback_kernel, dim3((B + 255) / 256), dim3(256), 0, st, P, S, PG, B, h->ro_controls.p,
                         h->ro_contact.p, h->ro_iters.p, h->ro_status.p, w, x_cmd, x_fb, foot, t, u0_s, x_s, foot_s, iters_s,
                         status_any);
  });
}

int bmpc_simulate_device(bmpc_handle h, int B, int steps, const bmpc_plant* plant, float* x_fb, float* foot, double* t,
                         const bmpc_gait* gait, const float* x_cmd, const float* mu, const float* push, float* u0_traj,
                         float* x_traj, float* foot_traj, int32_t* iters_traj, int32_t* status_any, void* stream) {
  return simulate(h, B, steps, plant, nullptr, nullptr, x_fb, foot, t, gait, x_cmd, mu, push, u0_traj, x_traj, foot_traj, iters_traj,
                  status_any, nullptr, nullptr, stream);
}

int bmpc_simulate_body_device(bmpc_handle h, int B, int steps, const bmpc_plant* plant, const bmpc_plant_body* body, float* x_fb,
                              float* foot, double* t, const bmpc_gait* gait, const float* x_cmd, const float* mu, const float* push,
                              float* u0_traj, float* x_traj, float* foot_traj, int32_t* iters_traj, int32_t* status_any,
                              const bmpc_sim_outcome* outcome, void* stream) {
  return simulate(h, B, steps, plant, body, nullptr, x_fb, foot, t, gait, x_cmd, mu, push, u0_traj, x_traj, foot_traj, iters_traj,
                  status_any, outcome, nullptr, stream);
}

int bmpc_simulate_ground_device(bmpc_handle h, int B, int steps, const bmpc_plant* plant, const bmpc_plant_body* body,
                                const bmpc_plant_ground* ground, float* x_fb, float* foot, double* t, const bmpc_gait* gait,
                                const float* x_cmd, const float* mu, const float* push, float* u0_traj, float* x_traj,
                                float* foot_traj, int32_t* iters_traj, int32_t* status_any, const bmpc_sim_outcome* outcome,
                                const bmpc_ground_out* gout, void* stream) {
  return simulate(h, B, steps, plant, body, ground, x_fb, foot, t, gait, x_cmd, mu, push, u0_traj, x_traj, foot_traj, iters_traj,
                  status_any, outcome, gout, stream);
}

// ---- S candidate plans per instance on the plant (bmpc_plant_rollout.hip)

// the outputs of bmpc_rollout_out in its member order: elements per instance (S: per sample) and bytes per element; a null
// descriptor gives all-null slots.  Slots 8 .. 11 need a ground, 12 .. 16 are sample_reduce_kernel's.
constexpr int RO_SCORE = 1, RO_GROUND = 8, RO_REDUCED = 12, N_RO = 17;
static OutSlots<N_RO> rollout_slots(const bmpc_rollout_out* out, const bmpc_rollout_price* price) {
  const bmpc_rollout_out o = out ? *out : bmpc_rollout_out{};
  const size_t S = price && price->S >= 1 && price->S <= bmpc::SAMPLES_MAX ? (size_t)price->S : 1;
  return {{{o.cost, {S, 0, 8}}, {o.score, {S, 0, 8}}, {o.x_end, {12 * S, 0, 4}}, {o.foot_end, {6 * S, 0, 4}}, {o.x_traj, {0, 12 * S, 4}},
           {o.first_fall, {S, 0, 4}}, {o.max_tilt, {S, 0, 4}}, {o.min_z, {S, 0, 4}}, {o.first_slip, {S, 0, 4}},
           {o.slip_periods, {2 * S, 0, 4}}, {o.unloaded_periods, {2 * S, 0, 4}}, {o.mu_demand, {S, 0, 4}}, {o.best, {1, 0, 4}},
           {o.n_valid, {1, 0, 4}}, {o.weights, {S, 0, 8}}, {o.u_mean, {0, 12, 8}}, {o.ess, {1, 0, 8}}}};
}

// What both entries check, in the order of include/bmpc.h: an error code (< 0), BMPC_OK when there is nothing to do, 1 to go on.
static int rollout_check(bmpc_handle h, int B, const float* x_fb, const float* foot, const uint8_t* contact, const float* controls,
                         const bmpc_plant* plant, const bmpc_plant_ground* ground, const bmpc_rollout_price* price,
                         const bmpc_rollout_out* out, const OutSlots<N_RO>& slots, bmpc_plant* o) {
  if (!price) return fail(BMPC_ERR_INVALID, "null bmpc_rollout_price");
  const double w[3] = {price->w_fall, price->w_slip, price->w_unloaded};
  if (int rc = check_sampling("bmpc_rollout_price", (int)price->S, w, 3, "w_fall, w_slip and w_unloaded", price->temperature); rc != BMPC_OK)
    return rc;
  if (price->tilt_max != price->tilt_max || price->z_min != price->z_min)
    return fail(BMPC_ERR_INVALID, "bmpc_rollout_price: thresholds tilt_max and z_min must not be NaN");
  if (!(price->fz_floor >= 0.0)) return fail(BMPC_ERR_INVALID, "fz_floor must be >= 0 and not NaN");
  if (int rc = plant_opts(plant, o); rc != BMPC_OK) return rc;
  if (!ground)
    for (int i = RO_GROUND; i < RO_REDUCED; ++i)
      if (slots.s[i].p) return fail(BMPC_ERR_INVALID, "first_slip, slip_periods, unloaded_periods and mu_demand need a ground");
  if (!h) return fail(BMPC_ERR_INVALID, "null handle");
  if (!x_fb || !foot || !contact || !controls) return fail(BMPC_ERR_INVALID, "x_fb, foot, contact and controls must be non-null");
  if (!out) return fail(BMPC_ERR_INVALID, "null bmpc_rollout_out");
  bool any_out = false;
  for (const OutSlot& s : slots.s) any_out = any_out || s.p;
  if (!any_out) return fail(BMPC_ERR_INVALID, "bmpc_rollout_out: at least one output must be non-null");
  return check_batch(h, B);
}

// The launches, on device-addressable arrays; d: the slots of bmpc_rollout_out in its order.  (The roll-out kernel stores scores
// only where it has an array for them: score scratch is needed only when reducing.)
static int rollout_launch(bmpc_handle h, int B, const float* x_fb, const float* foot, const uint8_t* contact, const float* x_cmd,
                          const float* x_ref, const float* push, const float* controls, const bmpc_plant& o,
                          const bmpc_plant_body* body, const bmpc_plant_ground* ground, const bmpc_rollout_price& price,
                          void* const* d, hipStream_t st) {
  const bmpc_params& p = h->params;
  bmpc::RolloutCost C;
  for (int i = 0; i < 12; ++i) { C.Q[i] = p.Q[i]; C.R[i] = p.R[i]; C.x_cmd[i] = p.x_cmd[i]; }
  const bool bd = has_body(body);
  const bmpc::RolloutIn in = {x_fb, foot, contact, x_cmd, x_ref, push, controls, bd ? body->m : nullptr, bd ? body->I : nullptr,
                              bd ? body->g : nullptr, ground ? ground->mu : nullptr, p.mu, ground ? 1 : 0, o.move_feet != 0 ? 1 : 0,
                              o.push_from, o.push_steps};
  const bmpc::RolloutPrice pr = {price.tilt_max, price.z_min, price.fz_floor, price.w_fall, price.w_slip, price.w_unloaded};
  const size_t blocks = ((size_t)B * (size_t)price.S + bmpc::ROLLOUT_NT - 1) / bmpc::ROLLOUT_NT;       // (at most 2^24: B, S <= 65536)
  return launch_sampled(h, B, (int)price.S, price.temperature, false, (double*)d[RO_SCORE], controls, d + RO_REDUCED, st, [&](double* score) {
    const bmpc::RolloutOut out = {(double*)d[0], score, (float*)d[2], (float*)d[3], (float*)d[4], (int32_t*)d[5], (float*)d[6],
                                  (float*)d[7], (int32_t*)d[8], (int32_t*)d[9], (int32_t*)d[10], (float*)d[11]};
    hipLaunchKernelGGL(bmpc::plant_rollout_samples_kernel, dim3((unsigned)blocks), dim3(bmpc::ROLLOUT_NT), 0, st, plant_params(h),
                       bmpc::plant_scheme(p.dt, o.integrator, o.substeps), C, in, pr, out, B, (int)price.S);
    return (int)BMPC_OK;
  });
}

int bmpc_plant_rollout_samples_device(bmpc_handle h, int B, const float* x_fb, const float* foot, const uint8_t* contact,
                                      const float* x_cmd, const float* x_ref, const float* push, const float* controls,
                                      const bmpc_plant* plant, const bmpc_plant_body* body, const bmpc_plant_ground* ground,
                                      const bmpc_rollout_price* price, const bmpc_rollout_out* out, void* stream) {
  const OutSlots<N_RO> slots = rollout_slots(out, price);
  bmpc_plant o;
  if (int rc = rollout_check(h, B, x_fb, foot, contact, controls, plant, ground, price, out, slots, &o); rc <= 0) return rc;
  HIP_TRY(hipSetDevice(h->device));
  void* d[N_RO];
  for (int i = 0; i < N_RO; ++i) d[i] = slots.s[i].p;
  return rollout_launch(h, B, x_fb, foot, contact, x_cmd, x_ref, push, controls, o, body, ground, *price, d, pick_stream(h, stream));
}

int bmpc_plant_rollout_samples(bmpc_handle h, int B, const float* x_fb, const float* foot, const uint8_t* contact,
                               const float* x_cmd, const float* x_ref, const float* push, const float* controls,
                               const bmpc_plant* plant, const bmpc_plant_body* body, const bmpc_plant_ground* ground,
                               const bmpc_rollout_price* price, const bmpc_rollout_out* out) {
  const OutSlots<N_RO> slots = rollout_slots(out, price);
  bmpc_plant o;
  if (int rc = rollout_check(h, B, x_fb, foot, contact, controls, plant, ground, price, out, slots, &o); rc <= 0) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const InSlot in[11] = {{x_fb, IN[I_XFB].w}, {foot, IN[I_FOOT].w}, {contact, IN[I_CON].w}, {x_cmd, IN[I_XCMD].w}, {x_ref, IN[I_XREF].w},
                         {push, W_WRENCH}, {controls, controls_width((size_t)price->S)}, {body ? body->m : nullptr, W_MASS},
                         {body ? body->I : nullptr, W_INERTIA}, {body ? body->g : nullptr, W_GRAVITY},
                         {ground ? ground->mu : nullptr, W_GROUND_MU}};
  Slices<11> d; Slices<N_RO> r;
  if (int rc = stage(h, B, in, &d, slots.s, &r); rc != BMPC_OK) return rc;
  const bmpc_plant_body d_body = {d.at<double>(7), d.at<double>(8), d.at<double>(9)};
  const bmpc_plant_ground d_ground = {d.at<double>(10)};
  const int rc = rollout_launch(h, B, d.at<float>(0), d.at<float>(1), d.at<uint8_t>(2), d.at<float>(3), d.at<float>(4), d.at<float>(5),
                              d.at<float>(6), o, body ? &d_body : nullptr, ground ? &d_ground : nullptr, *price, r.d, h->stream);
  return rc != BMPC_OK ? rc : fetch(h, slots.s, r);
}

// ---- the gradient of the plant roll-out (bmpc_plant_rollout_grad.hip)

// the outputs of bmpc_rollout_grad_out in its member order; a null descriptor gives all-null slots
constexpr int N_RG = 6;
static OutSlots<N_RG> rollout_grad_slots(const bmpc_rollout_grad_out* out, int S_) {
  const bmpc_rollout_grad_out o = out ? *out : bmpc_rollout_grad_out{};
  const size_t S = S_ >= 1 && S_ <= bmpc::SAMPLES_MAX ? (size_t)S_ : 1;
  return {{{o.cost, {S, 0, 8}}, {o.grad_u, {0, 12 * S, 8}}, {o.grad_x0, {12 * S, 0, 8}}, {o.grad_foot, {6 * S, 0, 8}},
           {o.x_traj, {0, 12 * S, 4}}, {o.first_bad, {S, 0, 4}}}};
}

// What both entries check, in the order of include/bmpc.h: an error code (< 0), BMPC_OK when there is nothing to do, 1 to go on.
static int rollout_grad_check(bmpc_handle h, int B, int S, const float* x_fb, const float* foot, const uint8_t* contact,
                              const float* controls, const bmpc_plant* plant, const bmpc_rollout_grad_out* out,
                              const OutSlots<N_RG>& slots, bmpc_plant* o) {
  if (S < 1 || S > bmpc::SAMPLES_MAX) return fail(BMPC_ERR_INVALID, "S = %d outside [1, %d]", S, bmpc::SAMPLES_MAX);
  if (int rc = plant_opts(plant, o); rc != BMPC_OK) return rc;
  if (!h) return fail(BMPC_ERR_INVALID, "null handle");
  if (!x_fb || !foot || !contact || !controls) return fail(BMPC_ERR_INVALID, "x_fb, foot, contact and controls must be non-null");
  if (!out) return fail(BMPC_ERR_INVALID, "null bmpc_rollout_grad_out");
  bool any_out = false;
  for (const OutSlot& s : slots.s) any_out = any_out || s.p;
  if (!any_out) return fail(BMPC_ERR_INVALID, "bmpc_rollout_grad_out: at least one output must be non-null");
  return check_batch(h, B);
}

// The launch, on device-addressable arrays; d: the slots of bmpc_rollout_grad_out in its order.  The scratch is made large enough
// first: where that fails nothing is launched.
static int rollout_grad_launch(bmpc_handle h, int B, int S, const float* x_fb, const float* foot, const uint8_t* contact,
                               const float* x_cmd, const float* x_ref, const float* push, const float* controls, const bmpc_plant& o,
                               const bmpc_plant_body* body, const bmpc_plant_ground* ground, void* const* d, hipStream_t st) {
  const bmpc_params& p = h->params;
  const size_t plans = (size_t)B * (size_t)S, H = (size_t)h->dev.h;
  const bool grads = d[1] || d[2] || d[3];
  if ((!d[4] && h->rg_states.ensure(plans * H * 12) != hipSuccess) || h->rg_feet.ensure(plans * H * 6) != hipSuccess ||
      (grads && h->rg_sub.ensure(plans * (size_t)o.substeps * 6) != hipSuccess)) {
    (void)hipGetLastError();
    return fail(BMPC_ERR_ALLOC, "out of device memory for the scratch of %zu plans", plans);
  }
  bmpc::RolloutCost C;
  for (int i = 0; i < 12; ++i) { C.Q[i] = p.Q[i]; C.R[i] = p.R[i]; C.x_cmd[i] = p.x_cmd[i]; }
  const bool bd = has_body(body);
  const bmpc::RolloutIn in = {x_fb, foot, contact, x_cmd, x_ref, push, controls, bd ? body->m : nullptr, bd ? body->I : nullptr,
                              bd ? body->g : nullptr, ground ? ground->mu : nullptr, p.mu, ground ? 1 : 0, o.move_feet != 0 ? 1 : 0,
                              o.push_from, o.push_steps};
  const bmpc::RolloutGradOut out = {(double*)d[0], (double*)d[1], (double*)d[2], (double*)d[3], (float*)d[4], (int32_t*)d[5]};
  const bmpc::RolloutGradScratch W = {d[4] ? nullptr : h->rg_states.p, h->rg_feet.p, h->rg_sub.p, plans};
  const size_t blocks = (plans + bmpc::RGRAD_NT - 1) / bmpc::RGRAD_NT;                 // (at most 2^24: B, S <= 65536)
  hipLaunchKernelGGL(bmpc::plant_rollout_grad_kernel, dim3((unsigned)blocks), dim3(bmpc::RGRAD_NT), 0, st, plant_params(h),
                     bmpc::plant_scheme(p.dt, o.integrator, o.substeps), C, in, out, W, B, S);
  HIP_TRY(hipGetLastError());
  return BMPC_OK;
}

int bmpc_plant_rollout_grad_device(bmpc_handle h, int B, int S, const float* x_fb, const float* foot, const uint8_t* contact,
                                   const float* x_cmd, const float* x_ref, const float* push, const float* controls,
                                   const bmpc_plant* plant, const bmpc_plant_body* body, const bmpc_plant_ground* ground,
                                   const bmpc_rollout_grad_out* out, void* stream) {
  const OutSlots<N_RG> slots = rollout_grad_slots(out, S);
  bmpc_plant o;
  if (int rc = rollout_grad_check(h, B, S, x_fb, foot, contact, controls, plant, out, slots, &o); rc <= 0) return rc;
  HIP_TRY(hipSetDevice(h->device));
  void* d[N_RG];
  for (int i = 0; i < N_RG; ++i) d[i] = slots.s[i].p;
  return rollout_grad_launch(h, B, S, x_fb, foot, contact, x_cmd, x_ref, push, controls, o, body, ground, d, pick_stream(h, stream));
}

int bmpc_plant_rollout_grad(bmpc_handle h, int B, int S, const float* x_fb, const float* foot, const uint8_t* contact,
                            const float* x_cmd, const float* x_ref, const float* push, const float* controls,
                            const bmpc_plant* plant, const bmpc_plant_body* body, const bmpc_plant_ground* ground,
                            const bmpc_rollout_grad_out* out) {
  const OutSlots<N_RG> slots = rollout_grad_slots(out, S);
  bmpc_plant o;
  if (int rc = rollout_grad_check(h, B, S, x_fb, foot, contact, controls, plant, out, slots, &o); rc <= 0) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const InSlot in[11] = {{x_fb, IN[I_XFB].w}, {foot, IN[I_FOOT].w}, {contact, IN[I_CON].w}, {x_cmd, IN[I_XCMD].w}, {x_ref, IN[I_XREF].w},
                         {push, W_WRENCH}, {controls, controls_width((size_t)S)}, {body ? body->m : nullptr, W_MASS},
                         {body ? body->I : nullptr, W_INERTIA}, {body ? body->g : nullptr, W_GRAVITY},
                         {ground ? ground->mu : nullptr, W_GROUND_MU}};
  Slices<11> d; Slices<N_RG> r;
  if (int rc = stage(h, B, in, &d, slots.s, &r); rc != BMPC_OK) return rc;
  const bmpc_plant_body d_body = {d.at<double>(7), d.at<double>(8), d.at<double>(9)};
  const bmpc_plant_ground d_ground = {d.at<double>(10)};
  const int rc = rollout_grad_launch(h, B, S, d.at<float>(0), d.at<float>(1), d.at<uint8_t>(2), d.at<float>(3), d.at<float>(4),
                                     d.at<float>(5), d.at<float>(6), o, body ? &d_body : nullptr, ground ? &d_ground : nullptr, r.d,
                                     h->stream);
  return rc != BMPC_OK ? rc : fetch(h, slots.s, r);
}

int bmpc_set_dispatch_order(bmpc_handle h, const int32_t* order_dev, int longest_first_rollouts) {
  if (!h) return fail(BMPC_ERR_INVALID, "null handle");
  h->order = order_dev;
  h->longest_first = longest_first_rollouts != 0;
  return BMPC_OK;
}

int bmpc_debug_set_profile(bmpc_handle h, long long* device_buf) {
  if (!h) return fail(BMPC_ERR_INVALID, "null handle");
  h->prof_dev = device_buf;
  return BMPC_OK;
}

int bmpc_last_kernel_ms(bmpc_handle h, float* ms) {
  if (!h || !ms) return fail(BMPC_ERR_INVALID, "null argument");
  *ms = -1.f;
  if (!h->timed) return BMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipEventSynchronize(h->ev1));
  HIP_TRY(hipEventElapsedTime(ms, h->ev0, h->ev1));
  return BMPC_OK;
}

}  // extern "C"
