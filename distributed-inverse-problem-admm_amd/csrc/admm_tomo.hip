// admm_tomo.hip -- C-ABI implementation (include/admm_tomo.h) for MI355X (gfx950).
//
// Host side of the hot path: uploads the planner's tables (fwd_plan.hpp: geometry
// records and forward plans, plain C++), owns the scratch, and enqueues the x-update /
// consensus sequences.  A bound batch's sequences are recorded once as
// hipGraphs and replayed every ADMM iteration (launch-bound at small N
// otherwise: ~170 kernels per x-update).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/admm_tomo.h"
#include "fwd_plan.hpp"
#include "kernels.hpp"

using namespace admm;

// k_fwdg reads the block table the planner fills as int4
static_assert(sizeof(FgBlock) == sizeof(int4) && alignof(FgBlock) == alignof(int4), "FgBlock must be an int4");

namespace {
thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIPCHK(expr)                                                                          \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess)                                                                     \
      return fail(ADMM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e) + " @" +     \
                                  std::to_string(__LINE__));                                  \
  } while (0)

#define CHECK_LAUNCH() HIPCHK(hipGetLastError())

size_t dsize(int dtype) { return dtype == ADMM_DTYPE_F64 ? 8 : 4; }

// Makes `device` current for the scope of an entry point and restores the caller's device
// on every return path (the operator API is called freely from Python: applying an
// operator that lives on another GPU must not change torch.cuda.current_device()).
struct DeviceGuard {
  int prev = -1;
  hipError_t err = hipSuccess;
  DeviceGuard() = default;  // (nothing to restore until enter())
  explicit DeviceGuard(int device) { enter(device); }
  void enter(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != device) err = hipSetDevice(device);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

#define DEVICE_SCOPE(dev)                                                                     \
  DeviceGuard _dg(dev);                                                                       \
  if (_dg.err != hipSuccess)                                                                  \
  return fail(ADMM_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(_dg.err))

#define RET(expr)                   \
  do {                              \
    int _rc = (expr);               \
    if (_rc != ADMM_OK) return _rc; \
  } while (0)

// The owners below free what they hold when they go (results ignored, as on every teardown
// path): a context member is released with its context, on every return path of its creation too.
struct Buf {  // device memory
  void* p = nullptr;
  size_t bytes = 0;
  Buf() = default;
  Buf(Buf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
  Buf& operator=(Buf&& o) noexcept {
    std::swap(p, o.p);
    std::swap(bytes, o.bytes);
    return *this;
  }
  ~Buf() { (void)release(); }
  hipError_t release() {
    const hipError_t e = p ? hipFree(p) : hipSuccess;
    p = nullptr;
    bytes = 0;
    return e;
  }
  template <typename T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
};

struct Graph {  // a recorded sequence: the graph and its executable
  hipGraph_t g = nullptr;
  hipGraphExec_t x = nullptr;
  Graph() = default;
  Graph(const Graph&) = delete;
  Graph& operator=(const Graph&) = delete;
  ~Graph() { reset(); }
  void reset() {  // both handles go, whatever either destroy returns
    if (x) (void)hipGraphExecDestroy(x);
    if (g) (void)hipGraphDestroy(g);
    x = nullptr;
    g = nullptr;
  }
};

struct Event {  // timing-only event
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
  // no system-scope fence (cache writeback / invalidation) at each record, which would
  // perturb the launches the events bracket
  int create() {
    HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
    return ADMM_OK;
  }
};

int ensure(Buf& b, size_t bytes) {
  if (b.bytes >= bytes && b.p) return ADMM_OK;
  HIPCHK(b.release());
  if (bytes == 0) return ADMM_OK;
  HIPCHK(hipMalloc(&b.p, bytes));
  // hipMemset is enqueued on the null stream, which does not order against non-blocking
  // streams (the capture stream, a caller's torch stream): finish the zero-fill before any
  // kernel can write the buffer (measured: the bind-time D packing on the capture stream
  // was overwritten by its own buffer's zero-fill)
  HIPCHK(hipMemset(b.p, 0, bytes));
  HIPCHK(hipDeviceSynchronize());
  b.bytes = bytes;
  return ADMM_OK;
}

// ensure + copy of a host table (min_bytes: the allocation of an empty table)
int upload(Buf& b, const void* src, size_t bytes, size_t min_bytes = 0) {
  RET(ensure(b, std::max(bytes, min_bytes)));
  if (bytes > 0) HIPCHK(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
  return ADMM_OK;
}
template <typename E>
int upload(Buf& b, const std::vector<E>& v, size_t min_bytes = 0) {
  return upload(b, v.data(), v.size() * sizeof(E), min_bytes);
}
}  // namespace

// error channel shared with the other translation units (masks.hip)
namespace admm_internal {
int fail(int code, const std::string& msg) { return ::fail(code, msg); }
}  // namespace admm_internal

struct admm_ctx {
  DeviceGuard scope;  // entered by the destructor only
  admm_geom g{};
  int dtype = ADMM_DTYPE_F32;
  int device = 0;
  int max_images = 0;
  int npix = 0, mrays = 0;
  Buf fang_b, bang_b, bangc_b;  // the angle records (fwd_plan.hpp GeomTables) on the device
  const FwdAngle* fang() const { return fang_b.as<const FwdAngle>(); }
  const BackAngle* bang() const { return bang_b.as<const BackAngle>(); }
  const BackAngleC* bangc() const { return bangc_b.as<const BackAngleC>(); }
  double Kb = 0.0;  // angle-independent part of the back projector's k_f
  int kbias = 0;    // integer bias making every pixel's k_f positive (k_back)
  int wexp = 0;     // k_back float weights scaled by 2^-wexp (<= 1 for the fma clamp)
  // the group plans (fwd_plan.hpp build_fwd_plans), one of them active: chosen at bind time
  static constexpr int kPlans = kFwdPlans;
  FwdPlan plans[kPlans];
  Buf plan_groups_b[kPlans], plan_rng_b[kPlans];  // their group and ray-range tables on the device
  const FgGroup* plan_groups(int pl) const { return plan_groups_b[pl].as<const FgGroup>(); }
  const FgRange* plan_rng(int pl) const { return plan_rng_b[pl].as<const FgRange>(); }
  int plan_n[kPlans] = {}, plan_blocks[kPlans] = {};  // groups and blocks per node chunk of each plan
  double plan_staged[kPlans] = {};  // touched row pixels staged per node chunk (host model)
  const FgGroup* groups = nullptr;  // angle groups of the grouped forward projector (active plan)
  const FgRange* rng = nullptr;     // its per-block ray ranges
  int n_groups = 0;                 // 0: geometry does not fit the grouped kernel -> k_fwd
  bool mirror_half = false;  // the half geometry of a mirror-mode context (XCD mapping below)
  Buf fg_order;                       // int4 block table of the grouped forward projector
  int fg_nblk = 0, fg_order_nch = 0;
  int fg_cpb = 1;  // (mirror half geometry) virtual chunks per forward block of the bound table
  Stream cap;  // private capture stream

  // explicit-matrix context (admm_ctx_create_matrix): A and A^T as device CSR, values in
  // the sample dtype; the projector launches dispatch to k_csr_fwd / k_back<..., CSR>
  bool csr = false;
  long long nnz = 0;
  Buf f_ptr, f_idx, f_val, t_ptr, t_idx, t_val;

  // operator-API scratch (admm_project_fwd runs the hot grouped kernel on up to 8 images
  // per launch: node-major images packed into the interleaved sample layout)
  Buf op_img, op_imgT, op_sino, op_fpart;
  Buf op_order[kPlans];  // block tables of the forward plans for one node chunk
  int op_nblk[kPlans] = {};
  int op_fpart_key = -1;  // (plan, VB) whose partial slots op_fpart holds (others are zero)

  // batch
  bool bound = false;
  admm_batch b{};
  int vb = 1;  // node interleave width of the sample buffers
  // mirror mode (kernels.hpp k_fwdg MIRROR): the bound batch projects virtual images over the
  // first half of the angles with the half geometry's context `half` (tables and plans)
  bool mm = false;
  // ADMM_BK_STAGING at creation (A/B, tests): "reg" register-staged back windows, "dma1" LDS-DMA
  // windows with one lane block per block, "dma2" two lane blocks per block wherever the lane
  // blocks pair up; default: LDS-DMA, two lane blocks per block where the grid still fills the chip
  int bk_staging = 0;   // 0 default, 1 reg, 2 dma1, 3 dma2
  // ADMM_BK_EPI at creation (A/B, tests): where the LDS-DMA mirror back projectors' float32 H
  // epilogue reads its p stencil: "lds" a tile staged in the window LDS after the taps (the
  // default), "global" per-pixel global loads; the same results bit for bit
  bool bk_epi_lds = true;
  int n_cu = 0;         // compute units of the device
  std::unique_ptr<admm_ctx> half;
  Buf xs, xsT, p, pT, Hp, sino, bI, fpart, r, c, d2, e2;
  Buf dsumS;  // rho D, D = sum_j q_ij, as interleaved samples (BACK_H epilogue)
  // per-ray weights omega of the bound batch (admm_batch_set_ray_weights), packed into the layout
  // of the sinogram scratch they multiply ([chunk][ray][vb], 0 in the lanes without a node)
  Buf wS;
  bool weighted = false;
  Buf x2, p2; // ping-pong partners of x (local rows) and p for the fused TV update
  Buf pring;  // CG direction slots 1 .. K-1 (direction ring; slot 0 = p, slot K = p2)
  Buf ats;    // A^T (A xs - b) of the last update's final x (ADMM_BATCH_KEEP_X)
  // admm_time_forward(in_solve): events around every CG-step forward tap launch of one
  // directly enqueued x-update (null outside that measurement)
  std::vector<Event>* tf_ev = nullptr;
  size_t tf_next = 0;
  int tf_kind = 0;  // what the in-solve events bracket: 0 forward taps, 1 back projector (BACK_H)
  bool ats_valid = false;  // ats matches x_ext's local rows
  // ats was valid until admm_batch_update_ray_weights changed the weights: xs, xsT still hold the last
  // update's x, so admm_batch_refresh_kept can form A^T s again (any other loss of ats clears it)
  bool ats_stale = false;
  Buf partH, partS, partD, partE;
  Buf redH;
  int P_back = 0, P_tile = 0, P_fwd = 0, P_edge = 0;
  Graph upd, upd_reuse, cons;  // the recorded x-update, its KEEP_X reuse start, the consensus

  admm_ctx() = default;
  admm_ctx(const admm_ctx&) = delete;
  admm_ctx& operator=(const admm_ctx&) = delete;
  // The context's device is current while everything it holds is released (the half
  // geometry's context first), then the caller's device comes back: `scope` is the first
  // member, so it is destroyed after every other one.
  ~admm_ctx() {
    scope.enter(device);
    (void)hipDeviceSynchronize();
    half.reset();
  }
};

namespace {

// Node-interleave width of a batch of V nodes: 32-byte sample vectors at most for float64
// (8 float64 nodes = 64 B would need 4 sample planes per tap: the forward loses its
// LDS-DMA staging, the back projector spills at 128 VGPRs; C5s 65.0 vs 63.0 node-updates/s)
int vb_for(int V, int dtype) {
  const int vb = V >= 5 ? 8 : (V >= 3 ? 4 : (V == 2 ? 2 : 1));
  return dtype == ADMM_DTYPE_F64 ? std::min(vb, 4) : vb;
}

// A/B and test knobs of the environment (ADMM_BK_* are read when a context is created, ADMM_FWD_* when
// a batch is bound).  env_choice: the value's first character as a digit in lo..hi; `unset` when the
// variable is unset or empty, `other` for any other value.  env_word: 1 + the index of the word the
// whole value equals, else 0.
int env_choice(const char* name, int lo, int hi, int unset, int other) {
  const char* v = getenv(name);
  if (!v || !v[0]) return unset;
  return (v[0] >= '0' + lo && v[0] <= '0' + hi) ? v[0] - '0' : other;
}
int env_choice(const char* name, int lo, int hi, int fallback) { return env_choice(name, lo, hi, fallback, fallback); }
int env_word(const char* name, std::initializer_list<const char*> words) {
  const char* v = getenv(name);
  int i = 0;
  for (const char* w : words) {
    ++i;
    if (v && std::string(v) == w) return i;
  }
  return 0;
}

void select_fwd_plan(admm_ctx* C, int pl) {
  C->groups = C->plan_groups(pl);
  C->rng = C->plan_rng(pl);
  C->n_groups = C->plan_n[pl];
}

// Block table of plan pl for nch node chunks in launch order (fwd_plan.hpp fwd_block_order), uploaded
int build_fwd_order_into(admm_ctx* C, int pl, int nch, int cus, Buf& buf, int* nblk) {
  const bool mirror_xcd = env_choice("ADMM_FWD_MIRROR_XCD", 0, 0, 1) != 0;  // "0": segment-per-XCD (A/B)
  const std::vector<FgBlock> t = fwd_block_order(C->plans[pl], nch, cus, C->mirror_half, mirror_xcd);
  RET(upload(buf, t));
  *nblk = (int)t.size();
  return ADMM_OK;
}

int build_fwd_order(admm_ctx* C, int pl, int nch, int cus) {
  RET(build_fwd_order_into(C, pl, nch, cus, C->fg_order, &C->fg_nblk));
  C->fg_order_nch = nch;
  return ADMM_OK;
}

// Forward plan for the bound batch (fwd_plan.hpp choose_fwd_plan_index) on this device's
// resident slots.  ADMM_FWD_PLAN=0..5 forces a plan.
// MIRROR / VBR: the instantiation launch_fwdg_taps launches (mirror mode: k_fwdg<T, VBV, true,
// VBR>, whose piece state and second window buffer set its own registers and LDS), so the
// occupancy query prices the kernel that actually runs.
template <typename T, int VB, bool MIRROR = false, int VBR = VB, int CPB = 1>
int pick_fwd_plan(admm_ctx* C, int nch, int* pl_out, int* cus_out, long* slots_out = nullptr) {
  int per_cu = 0, cus = 0;
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_fwdg<T, VB, MIRROR, VBR, CPB>, kFgThreads, 0));
  HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, C->device));
  if (per_cu < 1) return fail(ADMM_E_HIP, "grouped forward projector cannot be resident");
  const long slots = (long)per_cu * std::max(1, cus);
  const int forced = env_choice("ADMM_FWD_PLAN", 0, admm_ctx::kPlans - 1, -1);
  *pl_out = choose_fwd_plan_index(C->plan_blocks, C->plan_n, C->plan_staged, nch, slots, forced);
  *cus_out = cus;
  if (slots_out) *slots_out = slots;
  return ADMM_OK;
}

// Two virtual chunks per forward block (k_fwdg CPB = 2: mirror mode, float32, one lane block per
// real chunk) where the halved block table still fills every resident slot -- C3 and larger on
// one GPU; the 8-node share of the scaling runs keeps one (its halved table would leave slots
// empty).  ADMM_FWD_CPB=1 / 2 forces one / two (A/B and the bitwise tests; 2 needs an even
// chunk count).
template <typename T, int VB, bool MIRROR, int VBR>
constexpr bool fwd_cpb2_ok() {
  return MIRROR && std::is_same<T, float>::value && VB / 2 == VBR && VB == 8;
}

template <typename T, int VB, bool MIRROR = false, int VBR = VB>
int choose_fwd_plan(admm_ctx* C, int V) {
  if (C->plan_n[0] == 0) return ADMM_OK;
  const int nch = (V + VB - 1) / VB;
  C->fg_cpb = 1;
  if constexpr (fwd_cpb2_ok<T, VB, MIRROR, VBR>()) {
    const int force = env_choice("ADMM_FWD_CPB", 1, 2, 0);
    if (nch % 2 == 0 && force != 1) {
      int pl2 = 0, cus2 = 0;
      long slots2 = 0;
      RET((pick_fwd_plan<T, VB, MIRROR, VBR, 2>(C, nch / 2, &pl2, &cus2, &slots2)));
      if (force == 2 || (long)C->plan_blocks[pl2] * (nch / 2) >= slots2) {
        select_fwd_plan(C, pl2);
        RET(build_fwd_order(C, pl2, nch / 2, cus2));
        C->fg_order_nch = nch;
        C->fg_cpb = 2;
        return ADMM_OK;
      }
    }
  }
  int pl = 0, cus = 0;
  RET((pick_fwd_plan<T, VB, MIRROR, VBR>(C, nch, &pl, &cus)));
  select_fwd_plan(C, pl);
  return build_fwd_order(C, pl, nch, env_choice("ADMM_FWD_NATURAL_ORDER", 1, 1, 0) ? 0 : cus);
}

template <typename F>
int with_vb(int vb, F&& f) {
  switch (vb) {
    case 8: return f(std::integral_constant<int, 8>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 2: return f(std::integral_constant<int, 2>{});
    default: return f(std::integral_constant<int, 1>{});
  }
}

// The sample type of a context: f(type_tag<float>) or f(type_tag<double>)
template <typename T>
struct type_tag {
  using type = T;
};
template <typename F>
int with_type(int dtype, F&& f) {
  if (dtype == ADMM_DTYPE_F32) return f(type_tag<float>{});
  return f(type_tag<double>{});
}
// ... and the node-interleave width with it: f(type_tag<T>, integral_constant<int, VB>)
template <typename F>
int with_type_vb(int dtype, int vb, F&& f) {
  return with_type(dtype, [&](auto tt) { return with_vb(vb, [&](auto vbc) { return f(tt, vbc); }); });
}

// Virtual node-interleave width of mirror mode for a real width VBR: twice VBR, at most one
// 32-byte vector (8 float32 / 4 float64 lanes)
template <typename T, int VBR>
constexpr int mirror_vb() {
  return 2 * VBR < 32 / (int)sizeof(T) ? 2 * VBR : 32 / (int)sizeof(T);
}
// Mirror mode applies to the geometry and sample type, never to the batch (so every node runs
// the same arithmetic whatever its batch's size: rank- and batch-invariant results): an even
// number of angles spanning [0, pi) (block_2_load_odl_data.py:51) and a detector symmetric
// about 0 (block_2:52, uniform_partition(-1, 1, N)).  On by default for float32 samples
// (C3: 62 vs 57 us per forward launch at 16 nodes, but a 4-node rank of C4 on 8 GPUs runs
// 9.4 instead of 11.5 ms per iteration: profiles/r4_mirror_ab.txt); float64 (C5: 2 real
// nodes per 16-byte vector) measured slower in both widths, so opt-in there.
// ADMM_FWD_MIRROR=0 / 1 forces it off / on.
bool mirror_eligible(const admm_ctx* C) {
  if (C->csr || C->g.n_angles < 2 || C->g.n_angles % 2 != 0) return false;
  if (!env_choice("ADMM_FWD_MIRROR", 1, 1, C->dtype == ADMM_DTYPE_F32, 0)) return false;
  const double pi = 3.14159265358979323846;
  return std::fabs(C->g.angle_min) <= 1e-15 && std::fabs(C->g.angle_max - pi) <= 1e-12 &&
         std::fabs(C->g.det_min + C->g.det_max) <= 1e-12 * std::fabs(C->g.det_max);
}

// The bound batch's forward plan and its segment-partial buffer, set together: the clipped
// plans (3-5) write only the (segment, ray) partials of rays crossing the segment inside the
// image and k_fwd_combine reads every slot, so whenever the plan (or the batch) changes, every
// slot is zeroed here -- the one place C->fpart's plan is chosen (the operator API's op_fpart
// keeps its own plan key, op_forward_chunk).
int bind_fwd_plan(admm_ctx* C, int V) {
  C->mm = C->n_groups > 0 && mirror_eligible(C);
  // mirror mode keeps the real sample vectors at 16 bytes (4 float32 / 2 float64 nodes): a
  // virtual chunk then stages every byte of the real vectors it reads -- with 32-byte real
  // vectors each virtual chunk read every other 16 bytes and its sibling chunk the rest
  // (C3: 76 vs 58 us per forward launch, profiles/r4_mirror_ab.txt)
  if (C->mm) C->vb = std::min(C->vb, 16 / (int)dsize(C->dtype));
  if (C->mm && !C->half) {
    // the half geometry: the first a/2 angles, bitwise the full geometry's (angle_max - angle_min
    // is halved exactly and so is the angle count: the same step (t + 1/2) pi / a)
    admm_geom hg = C->g;
    hg.n_angles = C->g.n_angles / 2;
    hg.angle_max = C->g.angle_min + 0.5 * (C->g.angle_max - C->g.angle_min);
    admm_ctx* h = nullptr;
    RET(admm_ctx_create(&h, &hg, C->dtype, 1, C->device));  // (tables and plans only)
    C->half.reset(h);
    C->half->mirror_half = true;
    if (C->half->n_groups == 0) C->mm = false;  // (cannot happen: half the angles fit as well)
  }
  RET(with_type_vb(C->dtype, C->vb, [&](auto tt, auto vbc) -> int {
    using T = typename decltype(tt)::type;
    constexpr int VB = decltype(vbc)::value;
    if (!C->mm) return choose_fwd_plan<T, VB>(C, V);
    constexpr int VBV = mirror_vb<T, VB>();
    const int nchv = ((V + VB - 1) / VB) * (2 * VB / VBV);
    return choose_fwd_plan<T, VBV, true, VB>(C->half.get(), nchv * VBV);
  }));
  if (C->n_groups > 0) {
    // (mirror: virtual chunks x half the rays x the virtual width -- the same element count)
    const size_t Vp = (size_t)((V + C->vb - 1) / C->vb) * C->vb;
    RET(ensure(C->fpart, (size_t)kFgSeg * Vp * C->mrays * dsize(C->dtype)));
    HIPCHK(hipMemset(C->fpart.p, 0, C->fpart.bytes));
    HIPCHK(hipDeviceSynchronize());
  }
  return ADMM_OK;
}

// The optional trailing kernel argument of the weighted instantiations (kernels.hpp W...): f(wts) when
// the batch has per-ray weights, else f()
template <typename T, typename F>
void with_weights(const T* wts, F&& f) {
  if (wts)
    f(wts);
  else
    f();
}

// wts: the bound batch's packed per-ray weights (the weighted instantiations) or null
template <typename T, int VB, int MODE>
int launch_fwd(admm_ctx* C, const T* img, const T* imgT, T* sino, const T* b, double* part, int V, hipStream_t s,
               const T* wts = nullptr) {
  if (C->csr) {  // explicit matrix: one thread per sinogram row
    dim3 cg((C->mrays + kBlock - 1) / kBlock, (V + VB - 1) / VB);
    hipLaunchKernelGGL((k_csr_fwd<T, VB, MODE>), cg, dim3(kBlock), 0, s, (const int*)C->f_ptr.p,
                       (const int*)C->f_idx.p, (const T*)C->f_val.p, img, sino, b, part, C->mrays, C->npix, V);
    CHECK_LAUNCH();
    return ADMM_OK;
  }
  dim3 grid((C->g.n_det + kFwdRays - 1) / kFwdRays, C->g.n_angles, (V + VB - 1) / VB);
  with_weights(wts, [&](auto... w) {
    hipLaunchKernelGGL((k_fwd<T, VB, MODE, decltype(w)...>), grid, dim3(kFwdBlock), 0, s, img, imgT, sino, b, part,
                       C->fang(), C->g.N, C->g.n_det, C->g.n_angles, V, w...);
  });
  CHECK_LAUNCH();
  return ADMM_OK;
}

// hot-path forward projection of the bound batch: grouped kernel + fixed-order combine
// the grouped forward projector's tap kernel (all sample taps; segment partials -> fpart): kern over the
// angles, groups and ranges of A (C itself, or in mirror mode its half geometry) and nblk blocks of `order`
template <typename T>
using FwdgKernel = void (*)(const T*, const T*, T*, const FwdAngle*, const FgGroup*, const FgRange*, const int4*, int,
                            int, int, int);
template <typename T>
int launch_fwdg_taps_with(FwdgKernel<T> kern, admm_ctx* C, const admm_ctx* A, const T* img, const T* imgT, T* fpart,
                          const FgGroup* groups, const FgRange* rng, const int4* order, int nblk, int V,
                          hipStream_t s) {
  hipLaunchKernelGGL(kern, dim3(nblk), dim3(kFgThreads), 0, s, img, imgT, fpart, A->fang(), groups, rng, order,
                     C->g.N, C->g.n_det, A->g.n_angles, V);
  CHECK_LAUNCH();
  return ADMM_OK;
}

template <typename T, int VB>
int launch_fwdg_taps(admm_ctx* C, const T* img, const T* imgT, int V, hipStream_t s) {
  if (C->mm) {  // mirror mode: virtual chunks of the half geometry (k_fwdg MIRROR)
    constexpr int VBV = mirror_vb<T, VB>(), MH = VBV / 2;
    const int nchv = ((V + VB - 1) / VB) * (VB / MH);
    const admm_ctx* H = C->half.get();
    if (nchv != H->fg_order_nch) return fail(ADMM_E_STATE, "mirror block table built for another batch size");
    FwdgKernel<T> kern = k_fwdg<T, VBV, true, VB>;
    if constexpr (fwd_cpb2_ok<T, VBV, true, VB>()) {
      if (H->fg_cpb == 2) kern = k_fwdg<T, VBV, true, VB, 2>;  // two virtual chunks per block (the table holds pairs)
    }
    return launch_fwdg_taps_with<T>(kern, C, H, img, imgT, (T*)C->fpart.p, H->groups, H->rng,
                                    (const int4*)H->fg_order.p, H->fg_nblk, nchv * VBV, s);
  }
  const int nch = (V + VB - 1) / VB;
  if (nch != C->fg_order_nch) return fail(ADMM_E_STATE, "forward block table built for another batch size");
  return launch_fwdg_taps_with<T>(k_fwdg<T, VB>, C, C, img, imgT, (T*)C->fpart.p, C->groups, C->rng,
                                  (const int4*)C->fg_order.p, C->fg_nblk, V, s);
}

template <typename T, int VB, int MODE>
int launch_fwd_batch(admm_ctx* C, const T* img, const T* imgT, T* sino, const T* b, double* part, int V,
                     hipStream_t s, bool timed = false) {
  // timed (admm_time_forward in_solve): HIP events right before and after the tap kernel
  Event* ev = nullptr;
  if (timed && C->tf_ev && C->tf_kind == 0 && C->tf_next + 2 <= C->tf_ev->size()) {
    ev = C->tf_ev->data() + C->tf_next;
    C->tf_next += 2;
    HIPCHK(hipEventRecord(ev[0].e, s));
  }
  const T* wts = C->weighted ? (const T*)C->wS.p : nullptr;
  if (C->n_groups == 0) {
    RET((launch_fwd<T, VB, MODE>(C, img, imgT, sino, b, part, V, s, wts)));
    if (ev) HIPCHK(hipEventRecord(ev[1].e, s));
    return ADMM_OK;
  }
  const int nch = (V + VB - 1) / VB;
  RET((launch_fwdg_taps<T, VB>(C, img, imgT, V, s)));
  if (ev) HIPCHK(hipEventRecord(ev[1].e, s));
  if (C->mm) {  // virtual partials -> the real sinogram (both angles of every virtual ray)
    constexpr int VBV = mirror_vb<T, VB>(), MH = VBV / 2;
    const int mh = C->half->mrays;
    // MODE 0: two threads per virtual ray (k_fwd_combine_mirror); MODE 1: one (its block partials)
    const size_t mthreads = (size_t)mh * (MODE == 0 ? 2 : 1);
    dim3 mg((unsigned)((mthreads + kBlock - 1) / kBlock), nch * (VB / MH));
    with_weights(wts, [&](auto... w) {
      hipLaunchKernelGGL((k_fwd_combine_mirror<T, VBV, VB, MODE, decltype(w)...>), mg, dim3(kBlock), 0, s,
                         (const T*)C->fpart.p, sino, b, part, C->half->fang(), C->g.n_det, C->half->g.n_angles, V, w...);
    });
    CHECK_LAUNCH();
    return ADMM_OK;
  }
  dim3 cg((C->mrays + kBlock - 1) / kBlock, nch);
  with_weights(wts, [&](auto... w) {
    hipLaunchKernelGGL((k_fwd_combine<T, VB, MODE, decltype(w)...>), cg, dim3(kBlock), 0, s, (const T*)C->fpart.p, sino, b,
                       part, C->fang(), C->g.n_det, C->g.n_angles, V, w...);
  });
  CHECK_LAUNCH();
  return ADMM_OK;
}

// The back projectors' geometry arguments: the image and detector of C, the angles of A (C
// itself, or in mirror mode its half geometry)
template <typename T>
void back_geom(BackArgs<T>& a, const admm_ctx* C, const admm_ctx* A, int V) {
  a.ang = A->bang();
  a.angc = A->bangc();
  a.K = A->Kb;
  a.kbias = A->kbias;
  a.wexp = A->wexp;
  a.N = C->g.N;
  a.n_det = C->g.n_det;
  a.n_ang = A->g.n_angles;
  a.V = V;
}

template <typename T, int VB, int MODE>
int launch_back(admm_ctx* C, BackArgs<T> a, int V, hipStream_t s) {
  if constexpr (MODE == BACK_H || MODE == BACK_INIT || MODE == BACK_DIAG || MODE == BACK_ATB) {
    if (C->mm) {  // mirror mode: pixel pairs of the upper half, the half geometry's angles
      constexpr int VBV = mirror_vb<T, VB>(), MH = VBV / 2;
      back_geom(a, C, C->half.get(), V);
      const int N = C->g.N, Nh = (N + 1) / 2;
      dim3 grid((N + kBTJ - 1) / kBTJ, (Nh + kBTI - 1) / kBTI, ((V + VB - 1) / VB) * (VB / MH));
      void (*kern)(BackArgs<T>) = k_back_mirror<T, VBV, VB, MODE>;
      if constexpr (back_mirror_dma<T, VBV, MODE>()) {
        // the variants where LDS-DMA is the default (bk_staging: 0 default, 1 reg, 2 dma1, 3 dma2)
        if (C->bk_staging == 1) {
          kern = k_back_mirror_reg<T, VBV, VB, MODE>;
        } else if constexpr (std::is_same<T, float>::value) {
          // two lane blocks per block while half the blocks still give every CU one
          const bool fills = (long)grid.x * grid.y * grid.z >= 2L * C->n_cu;
          if (grid.z % 2 == 0 && (C->bk_staging == 3 || (C->bk_staging == 0 && fills))) {
            kern = C->bk_epi_lds ? k_back_mirror_2<T, VBV, VB> : k_back_mirror_2_gepi<T, VBV, VB>;
            grid.z /= 2;
          } else if (!C->bk_epi_lds) {
            kern = k_back_mirror_gepi<T, VBV, VB, MODE>;
          }
        }
      }
      hipLaunchKernelGGL(kern, grid, dim3(kBkThreads), 0, s, a);
      CHECK_LAUNCH();
      return ADMM_OK;
    }
  }
  back_geom(a, C, C, V);
  const int N = C->g.N;
  constexpr bool kOneImage = MODE == BACK_WSQ || MODE == BACK_WSQW;  // the column norms: no node chunks
  dim3 grid((N + kBTJ - 1) / kBTJ, (N + kBTI - 1) / kBTI, kOneImage ? 1 : (V + VB - 1) / VB);
  if (C->csr) {
    a.csr_ptr = (const int*)C->t_ptr.p;
    a.csr_idx = (const int*)C->t_idx.p;
    a.csr_val = (const T*)C->t_val.p;
    hipLaunchKernelGGL((k_back<T, VB, MODE, true>), grid, dim3(kBkThreads), 0, s, a);
  } else {
    hipLaunchKernelGGL((k_back<T, VB, MODE>), grid, dim3(kBkThreads), 0, s, a);
  }
  CHECK_LAUNCH();
  return ADMM_OK;
}

int back_partitions(admm_ctx* C) {
  const int N = C->g.N;
  const int rows = C->mm ? (N + 1) / 2 : N;  // mirror mode: blocks over the upper half's pixel pairs
  return ((N + kBTJ - 1) / kBTJ) * ((rows + kBTI - 1) / kBTI);
}
dim3 tile_grid(admm_ctx* C, int nchunks, int vb) {
  const int N = C->g.N, ti = kTile / vb;
  return dim3((N + kTile - 1) / kTile, (N + ti - 1) / ti, nchunks);
}

int launch_reduce(const double* part, int rows, int P, double* out, int G, int ostride, int ooff, hipStream_t s) {
  hipLaunchKernelGGL(k_reduce_rows, dim3(rows), dim3(kBlock), 0, s, part, P, out, G, ostride, ooff);
  CHECK_LAUNCH();
  return ADMM_OK;
}

// the edge state the x-update reads (stored z, or z derived from x_prev: ABI 7)
EdgeIn edge_in(const admm_batch& B) {
  EdgeIn E{};
  E.z = B.z;
  E.y = B.y;
  E.yb = B.fusion == ADMM_FUSE_WEIGHTED ? B.y_b : nullptr;
  E.xp = B.x_prev;
  E.ea = B.edge_a;
  E.eb = B.edge_b;
  return E;
}

// k_tv_update of a split-Bregman round: the last round writes d and e; a round after the first
// reads u, and every round but the last of several leaves u (the five forms an x-update reaches)
template <typename T, int VB>
auto tv_kernel(bool last, bool uin, bool uout) {
  if (last) return uin ? k_tv_update<T, VB, true, true, false> : k_tv_update<T, VB, true, false, false>;
  if (uin) return k_tv_update<T, VB, false, true, true>;
  return uout ? k_tv_update<T, VB, false, false, true> : k_tv_update<T, VB, false, false, false>;
}

// --------------------------------------------------------------------------
// the x-update sequence for the bound batch (replaces block_6_admm_loop_ver2.py:81-197)
// --------------------------------------------------------------------------
template <typename T, int VB>
int enqueue_update(admm_ctx* C, hipStream_t s, bool reuse = false, int rounds = 0) {
  const admm_batch& B = C->b;
  const int V = B.V, N = C->g.N;
  const size_t npix = (size_t)N * N;
  const int nch = (V + VB - 1) / VB;
  T* xs = (T*)C->xs.p;
  T* xsT = (T*)C->xsT.p;
  T* p = (T*)C->p.p;
  T* pT = (T*)C->pT.p;
  T* Hp = (T*)C->Hp.p;
  T* sino = (T*)C->sino.p;
  double* r = (double*)C->r.p;
  double* c = (double*)C->c.p;
  double* redH = (double*)C->redH.p;
  const dim3 tg = tile_grid(C, nch, VB);
  const dim3 cgg((N + kTile - 1) / kTile, (N + kCgRows - 1) / kCgRows, nch);
  const dim3 tvg((N + kTvTile - 1) / kTvTile, (N + EwMap<VB>::TI - 1) / EwMap<VB>::TI, nch);  // k_tv_update
  const int Pb = C->P_back;

  // (D as interleaved samples for the CG operator, dsumS, is packed once at bind time)
  if (reuse) {
    // 1-4. one kernel from the previous update's A^T (A xs - b) (ADMM_BATCH_KEEP_X):
    //      c, r = A^T b + rho c + mu K^T(d - e) - H x, p = r (+ transpose)
    hipLaunchKernelGGL((k_start_reuse<T, VB>), cgg, dim3(kBlock), 0, s, (const T*)C->ats.p, B.x_ext, edge_in(B),
                       B.q, B.inc_off, B.inc_edge, B.inc_qslot, B.inc_sign, B.atb, c, B.dsum, B.d, B.e, r, p, pT,
                       B.rho, B.mu, N, V);
    CHECK_LAUNCH();
  } else {
  // 1. neighbour gather: c = sum_j q_ij (z_ij - y_ij,i); xs = (T) x (+ transpose)
  hipLaunchKernelGGL((k_gather<T, VB>), tg, dim3(kBlock), 0, s, B.x_ext, edge_in(B), B.q, B.inc_off, B.inc_edge,
                     B.inc_qslot, B.inc_sign, c, xs, xsT, N, V);
  CHECK_LAUNCH();
  // 2-4. r = A^T b + rho c + mu K^T(d - e) - H x,  p = r,  rr
  RET((launch_fwd_batch<T, VB, 0>(C, xs, xsT, sino, nullptr, nullptr, V, s)));
  {
    BackArgs<T> a{};
    a.sino = sino;
    a.out_t = p;
    a.out_d = r;
    a.pin = xs;
    a.dsum = B.dsum;
    a.atb = B.atb;
    a.cvec = c;
    a.dvar = B.d;
    a.evar = B.e;
    a.rho = B.rho;
    a.lam = B.lam;
    a.mu = B.mu;
    RET((launch_back<T, VB, BACK_INIT>(C, a, V, s)));
  }
  hipLaunchKernelGGL((k_transpose<T, VB>), tg, dim3(kBlock), 0, s, p, pT, N);
  CHECK_LAUNCH();
  }

  const double tau = B.lam / B.mu;
  double* dcur = B.d;
  double* ecur = B.e;
  double* dnxt = (double*)C->d2.p;
  double* enxt = (double*)C->e2.p;
  // Every x step of a round is applied by the TV update that ends it (F = 2: the CG updates
  // leave x alone and write each new direction to its own slot of a ring, p_0 .. p_K); with
  // more CG steps than ring slots only the round's last step is (F = 1).  The TV update reads
  // x and the directions over its tiles' halos while writing them, so x ping-pongs
  // (xcur -> xnxt) and the restart p = r goes to the ring's spare slot.
  const int K = B.cg_iters, Tt = rounds > 0 ? rounds : B.tv_iters;
  const int F = (K <= kMaxCgRing) ? 2 : 1;
  double* xcur = B.x_ext;
  double* xnxt = (double*)C->x2.p;
  std::vector<T*> slot(K + 1, p);
  if (F == 1) slot[1] = (T*)C->p2.p;
  if (F == 2) {
    slot[K] = (T*)C->p2.p;
    for (int k = 1; k < K; ++k) slot[k] = (T*)C->pring.p + (size_t)(k - 1) * nch * npix * VB;
  }
  const size_t rstride = (F == 2) ? (size_t)5 * V : 0;  // redH ring stride (one reduction per step)
  for (int t = 0; t < Tt; ++t) {
    for (int kk = 0; kk < K; ++kk) {
      T* pk = (F == 2) ? slot[kk] : slot[0];
      double* rk = redH + kk * rstride;
      RET((launch_fwd_batch<T, VB, 0>(C, pk, pT, sino, nullptr, nullptr, V, s, true)));
      BackArgs<T> a{};
      a.sino = sino;
      a.out_t = Hp;
      a.part = (double*)C->partH.p;
      a.pin = pk;
      a.r = r;
      a.dsum = B.dsum;
      a.dsum_s = (const T*)C->dsumS.p;
      a.rho = B.rho;
      a.lam = B.lam;
      a.mu = B.mu;
      // (admm_time_back: events right before and after each in-solve back projection)
      Event* bev = nullptr;
      if (C->tf_ev && C->tf_kind == 1 && C->tf_next + 2 <= C->tf_ev->size()) {
        bev = C->tf_ev->data() + C->tf_next;
        C->tf_next += 2;
        HIPCHK(hipEventRecord(bev[0].e, s));
      }
      RET((launch_back<T, VB, BACK_H>(C, a, V, s)));
      if (bev) HIPCHK(hipEventRecord(bev[1].e, s));
      RET(launch_reduce((double*)C->partH.p, 5 * V, Pb, rk, 1, 1, 0, s));
      if (kk + 1 < K) {  // (ring: x is left to the TV update and p_k+1 takes its own slot)
        const auto cg = (F == 2) ? k_cg_update<T, VB, false> : k_cg_update<T, VB, true>;
        hipLaunchKernelGGL(cg, cgg, dim3(kBlock), 0, s, xcur, r, pk, pT, Hp, rk, N, V, (F == 2) ? slot[kk + 1] : pk);
        CHECK_LAUNCH();
      }  // the round's last step: applied by the TV update
    }
    const bool last = (t + 1 == Tt);
    PRing<T> pr{};
    pr.K = (F == 2) ? K : 1;
    for (int k = 0; k < pr.K; ++k) pr.p[k] = slot[k];
    T* pout = last ? xs : (F == 2 ? slot[K] : (F == 1 ? slot[1] : slot[0]));
    T* poutT = last ? xsT : pT;
    // split-Bregman state in/out of this round: d, e (B.d / B.e or the scratch pair) or,
    // between the rounds of the update (Tt > 1), u = Kx + e in ua / ub
    const bool uin = t > 0 && Tt > 1;
    const bool uout = !last && Tt > 1;
    double* ua = (double*)C->d2.p;
    double* ub = (double*)C->e2.p;
    const double* din = uin ? ((t % 2) ? ua : ub) : dcur;
    const double* ein = ecur;  // (not read when uin)
    double* dout = uout ? ((t % 2) ? ub : ua) : (Tt > 1 ? B.d : dnxt);
    double* eout = uout ? nullptr : (Tt > 1 ? B.e : enxt);
    hipLaunchKernelGGL((tv_kernel<T, VB>(last, uin, uout)), tvg, dim3(kTvThreads), 0, s, xcur, din, ein, dout, eout, r,
                       pout, poutT, tau, B.mu, B.tv_kind, N, V, xnxt, pr, Hp, redH);
    CHECK_LAUNCH();
    if (Tt == 1) {  // one round: d, e went to the scratch pair
      std::swap(dcur, dnxt);
      std::swap(ecur, enxt);
    }
    std::swap(xcur, xnxt);
    if (!last) std::swap(slot[0], slot[F == 2 ? K : 1]);
  }
  if (xcur != B.x_ext)  // odd number of fused rounds: x ended in scratch
    HIPCHK(hipMemcpyAsync(B.x_ext, xcur, (size_t)V * npix * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (dcur != B.d) {  // odd number of d / e rounds: state ended in scratch
    HIPCHK(hipMemcpyAsync(B.d, dcur, 2 * V * npix * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(B.e, ecur, 2 * V * npix * sizeof(double), hipMemcpyDeviceToDevice, s));
  }
  // diagnostics epilogue: s = A x - b, ||s||^2, g, TV, quad, image error
  RET((launch_fwd_batch<T, VB, 1>(C, xs, xsT, sino, (const T*)B.b, (double*)C->partS.p, V, s)));
  {
    BackArgs<T> a{};
    a.sino = sino;
    a.part = (double*)C->partD.p;
    a.dsum = B.dsum;
    a.cvec = c;
    a.x = B.x_ext;
    a.phantom = B.phantom;
    a.edges = edge_in(B);
    a.qv = B.q;
    a.inc_off = B.inc_off;
    a.inc_edge = B.inc_edge;
    a.inc_qslot = B.inc_qslot;
    a.inc_sign = B.inc_sign;
    a.rho = B.rho;
    a.lam = B.lam;
    a.mu = B.mu;
    a.tv_kind = B.tv_kind;
    a.evar = B.e;  // the final Bregman variable (copied back from scratch above for odd rounds)
    a.out_t = (B.flags & ADMM_BATCH_KEEP_X) ? (T*)C->ats.p : nullptr;
    RET((launch_back<T, VB, BACK_DIAG>(C, a, V, s)));
  }
  RET(launch_reduce((double*)C->partS.p, V, C->P_fwd, B.node_stats, 1, ADMM_NODE_STATS, ADMM_NODE_STAT_MSE_SINO, s));
  RET(launch_reduce((double*)C->partD.p, 5 * V, Pb, B.node_stats, 5, ADMM_NODE_STATS, ADMM_NODE_STAT_G2, s));
  return ADMM_OK;
}

int enqueue_update_any(admm_ctx* C, hipStream_t s, bool reuse = false, int rounds = 0) {
  return with_type_vb(C->dtype, C->vb, [&](auto tt, auto vbc) {
    return enqueue_update<typename decltype(tt)::type, decltype(vbc)::value>(C, s, reuse, rounds);
  });
}

// rows of the derived consensus' LDS tile (0: more x_ext rows than any tile: direct kernel)
int cons_rows(int n_xext) { return n_xext <= 16 ? 16 : n_xext <= 64 ? 64 : n_xext <= 128 ? 128 : 0; }

// stored-z midpoint consensus of edge slots [e0, e1) (k_consensus<false>: one edge per
// blockIdx.y, 1024 pixels per block; the endpoint rows are read from HBM / L2 per edge -- at C5's
// share, 476 edges over 64 rows, this streamed 48 B per pixel-edge in 14.1 ms against 17.4 ms for
// a pixel-major LDS-tile variant, profiles/AB_LOG.md round 5)
int enqueue_consensus_stored(admm_ctx* C, int e0, int e1, hipStream_t s) {
  const admm_batch& B = C->b;
  if (e1 <= e0) return ADMM_OK;
  const int npix = C->npix;
  dim3 grid((npix + kBlock * 4 - 1) / (kBlock * 4), e1 - e0);
  hipLaunchKernelGGL(k_consensus<false>, grid, dim3(kBlock), 0, s, B.x_ext, B.y, nullptr, B.z, nullptr, B.edge_a,
                     B.edge_b, (double*)C->partE.p, npix, e0);
  CHECK_LAUNCH();
  // rows 3 e0 .. 3 e1 - 1 of the partials -> edge_stats rows e0 .. e1 - 1
  RET(launch_reduce((double*)C->partE.p + (size_t)3 * e0 * C->P_edge, 3 * (e1 - e0), C->P_edge,
                    B.edge_stats + (size_t)3 * e0, 1, 1, 0, s));
  return ADMM_OK;
}

int enqueue_consensus(admm_ctx* C, hipStream_t s) {
  const admm_batch& B = C->b;
  if (B.n_edges == 0) return ADMM_OK;
  const int npix = C->npix;
  if (B.z == nullptr) {  // derived z (midpoint fusion, ABI 7)
    const dim3 g((npix + kConsPix - 1) / kConsPix);
    double* part = (double*)C->partE.p;
    if (const int rows = cons_rows(B.n_xext)) {
      const auto kern = rows == 16 ? k_consensus_derived<16> : rows == 64 ? k_consensus_derived<64> : k_consensus_derived<128>;
      hipLaunchKernelGGL(kern, g, dim3(kBlock), 0, s, B.x_ext, B.x_prev, B.y, B.edge_a, B.edge_b, part, npix, B.n_xext,
                         B.n_edges);
    } else {
      hipLaunchKernelGGL(k_consensus_derived_direct, g, dim3(kBlock), 0, s, B.x_ext, B.x_prev, B.y, B.edge_a,
                         B.edge_b, part, npix, B.n_edges);
      CHECK_LAUNCH();
      const size_t cnt = (size_t)B.n_xext * npix;
      hipLaunchKernelGGL(k_copy_rows, dim3((unsigned)std::min<size_t>((cnt + kBlock - 1) / kBlock, 16384)),
                         dim3(kBlock), 0, s, (const double*)B.x_ext, B.x_prev, cnt);
    }
    CHECK_LAUNCH();
    RET(launch_reduce(part, 3 * B.n_edges, C->P_edge, B.edge_stats, 1, 1, 0, s));
    return ADMM_OK;
  }
  if (B.fusion == ADMM_FUSE_MIDPOINT) return enqueue_consensus_stored(C, 0, B.n_edges, s);
  dim3 grid((npix + kBlock * 4 - 1) / (kBlock * 4), B.n_edges);
  hipLaunchKernelGGL(k_consensus<true>, grid, dim3(kBlock), 0, s, B.x_ext, B.y, B.y_b, B.z, B.w, B.edge_a,
                     B.edge_b, (double*)C->partE.p, npix);
  CHECK_LAUNCH();
  RET(launch_reduce((double*)C->partE.p, 3 * B.n_edges, C->P_edge, B.edge_stats, 1, 1, 0, s));
  return ADMM_OK;
}

void free_graphs(admm_ctx* C) {
  C->upd.reset();
  C->cons.reset();
  C->upd_reuse.reset();
}

template <typename F>
int capture(admm_ctx* C, F&& fn, Graph& out) {
  HIPCHK(hipStreamBeginCapture(C->cap.s, hipStreamCaptureModeThreadLocal));
  int rc = fn(C->cap.s);
  out.reset();
  hipError_t e = hipStreamEndCapture(C->cap.s, &out.g);
  if (rc != ADMM_OK) {
    out.reset();
    return rc;
  }
  if (e != hipSuccess) return fail(ADMM_E_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
  HIPCHK(hipGraphInstantiate(&out.x, out.g, nullptr, nullptr, 0));
  return ADMM_OK;
}

// the bound batch's x-update and consensus sequences, recorded once and replayed every iteration
// (admm_batch_bind; again by admm_batch_set_ray_weights, whose launches differ)
int record_graphs(admm_ctx* C) {
  free_graphs(C);
  auto fu = [&](hipStream_t s) { return enqueue_update_any(C, s); };
  RET(capture(C, fu, C->upd));
  if (C->b.flags & ADMM_BATCH_KEEP_X) {
    auto fr = [&](hipStream_t s) { return enqueue_update_any(C, s, true); };
    RET(capture(C, fr, C->upd_reuse));
  }
  if (C->b.n_edges > 0) {
    auto fc = [&](hipStream_t s) { return enqueue_consensus(C, s); };
    RET(capture(C, fc, C->cons));
  }
  return ADMM_OK;
}

// Operator API forward projection (A @ x of node-major images).  When the geometry has
// angle-group plans this is the hot path's own kernel pair (k_fwdg + k_fwd_combine) on
// up to 8 images per launch: the images are packed into the interleaved sample layout
// (plus the transposed copy case-A angles read), projected, and the interleaved
// sinograms unpacked.  Otherwise (windows too wide for the grouped kernel) k_fwd.
template <typename T, int VB>
int op_forward_chunk(admm_ctx* C, const T* img, T* sino, int nc, hipStream_t s) {
  const int npix = C->npix, m = C->mrays;
  int pl = 0, cus = 0;
  RET((pick_fwd_plan<T, VB>(C, 1, &pl, &cus)));
  if (C->op_nblk[pl] == 0) RET(build_fwd_order_into(C, pl, 1, cus, C->op_order[pl], &C->op_nblk[pl]));
  if (C->op_fpart_key != pl * 16 + VB) {  // slots another plan / width wrote: back to 0
    HIPCHK(hipMemsetAsync(C->op_fpart.p, 0, C->op_fpart.bytes, s));
    C->op_fpart_key = pl * 16 + VB;
  }
  T* xs = (T*)C->op_img.p;
  T* xsT = (T*)C->op_imgT.p;
  T* sI = (T*)C->op_sino.p;
  hipLaunchKernelGGL((k_pack<T, VB>), dim3((npix + 255) / 256, 1), dim3(256), 0, s, img, xs, npix, nc);
  CHECK_LAUNCH();
  hipLaunchKernelGGL((k_transpose<T, VB>), tile_grid(C, 1, VB), dim3(kBlock), 0, s, (const T*)xs, xsT, C->g.N);
  CHECK_LAUNCH();
  RET((launch_fwdg_taps_with<T>(k_fwdg<T, VB>, C, C, xs, xsT, (T*)C->op_fpart.p, C->plan_groups(pl), C->plan_rng(pl),
                                (const int4*)C->op_order[pl].p, C->op_nblk[pl], nc, s)));
  hipLaunchKernelGGL((k_fwd_combine<T, VB, 0>), dim3((m + kBlock - 1) / kBlock, 1), dim3(kBlock), 0, s,
                     (const T*)C->op_fpart.p, sI, (const T*)nullptr, (double*)nullptr, C->fang(), C->g.n_det,
                     C->g.n_angles, nc);
  CHECK_LAUNCH();
  hipLaunchKernelGGL((k_unpack<T, VB>), dim3((m + 255) / 256, 1), dim3(256), 0, s, (const T*)sI, sino, m, nc);
  CHECK_LAUNCH();
  return ADMM_OK;
}

template <typename T>
int op_forward(admm_ctx* C, const T* img, T* sino, int nimg, hipStream_t s) {
  const size_t npix = C->npix, m = C->mrays, ds = sizeof(T);
  const int N = C->g.N;
  if (C->csr) return launch_fwd<T, 1, 0>(C, img, nullptr, sino, nullptr, nullptr, nimg, s);
  if (C->plan_n[0] == 0) {  // no angle-group plan for this geometry: ray-per-thread kernel
    RET(ensure(C->op_imgT, (size_t)nimg * npix * ds));
    hipLaunchKernelGGL((k_transpose<T, 1>), tile_grid(C, nimg, 1), dim3(kBlock), 0, s, img, (T*)C->op_imgT.p, N);
    CHECK_LAUNCH();
    return launch_fwd<T, 1, 0>(C, img, (const T*)C->op_imgT.p, sino, nullptr, nullptr, nimg, s);
  }
  const int step = vb_for(8, C->dtype);  // images per chunk: one sample vector (8 float32 / 4 float64)
  const int cmax = std::min(nimg, step);
  const int vbmax = vb_for(cmax, C->dtype);
  RET(ensure(C->op_img, vbmax * npix * ds));
  RET(ensure(C->op_imgT, vbmax * npix * ds));
  RET(ensure(C->op_sino, vbmax * m * ds));
  RET(ensure(C->op_fpart, (size_t)kFgSeg * vbmax * m * ds));
  for (int v0 = 0; v0 < nimg; v0 += step) {
    const int nc = std::min(step, nimg - v0);
    const T* in = img + (size_t)v0 * npix;
    T* out = sino + (size_t)v0 * m;
    RET(with_vb(vb_for(nc, C->dtype), [&](auto vbc) { return op_forward_chunk<T, decltype(vbc)::value>(C, in, out, nc, s); }));
  }
  return ADMM_OK;
}

}  // namespace

// ============================================================================
// C ABI
// ============================================================================
extern "C" {

int admm_abi_version(void) { return ADMM_ABI_VERSION; }
const char* admm_last_error(void) { return g_err.c_str(); }

int admm_ctx_create(admm_ctx** out, const admm_geom* geom, int dtype, int max_images, int device) {
  if (!out || !geom) return fail(ADMM_E_INVALID, "null argument");
  *out = nullptr;
  const admm_geom g = *geom;
  // validate -> geometry tables -> forward plans (fwd_plan.hpp, host only) -> upload
  if (const char* err = check_geom(g, dtype, max_images)) return fail(ADMM_E_INVALID, err);
  GeomTables T;
  if (const char* err = geom_tables(g, dtype, T)) return fail(ADMM_E_INVALID, err);
  FwdPlans P = build_fwd_plans(g, T.fa);
  DEVICE_SCOPE(device);
  std::unique_ptr<admm_ctx> C(new admm_ctx());
  C->g = g;
  C->dtype = dtype;
  C->device = device;
  C->bk_staging = env_word("ADMM_BK_STAGING", {"reg", "dma1", "dma2"});
  C->bk_epi_lds = env_word("ADMM_BK_EPI", {"global"}) == 0;
  HIPCHK(hipDeviceGetAttribute(&C->n_cu, hipDeviceAttributeMultiprocessorCount, device));
  C->max_images = max_images;
  C->npix = g.N * g.N;
  C->mrays = g.n_angles * g.n_det;
  C->Kb = T.Kb;
  C->kbias = T.kbias;
  C->wexp = T.wexp;
  RET(upload(C->fang_b, T.fa));
  RET(upload(C->bang_b, T.ba));
  RET(upload(C->bangc_b, T.bc));
  if (P.fits) {
    for (int pl = 0; pl < admm_ctx::kPlans; ++pl) {
      FwdPlan& Q = P.plan[pl];
      if (Q.groups.empty()) continue;
      RET(upload(C->plan_groups_b[pl], Q.groups));
      RET(upload(C->plan_rng_b[pl], Q.ranges));
      C->plan_n[pl] = (int)Q.groups.size();
      C->plan_blocks[pl] = (int)Q.blocks.size();
      C->plan_staged[pl] = Q.staged;
      C->plans[pl] = std::move(Q);
    }
    select_fwd_plan(C.get(), 0);  // until a batch is bound
  }
  HIPCHK(hipStreamCreateWithFlags(&C->cap.s, hipStreamNonBlocking));
  *out = C.release();
  return ADMM_OK;
}

int admm_ctx_create_matrix(admm_ctx** out, int N, int m, long long nnz, const long long* indptr,
                           const int* indices, const double* values, int dtype, int max_images, int device) {
  if (!out || !indptr || (nnz > 0 && (!indices || !values))) return fail(ADMM_E_INVALID, "null argument");
  *out = nullptr;
  if (N < 2 || N > 4096 || m < 1) return fail(ADMM_E_INVALID, "bad matrix sizes");
  if (dtype != ADMM_DTYPE_F32 && dtype != ADMM_DTYPE_F64) return fail(ADMM_E_INVALID, "bad dtype");
  if (max_images < 1) return fail(ADMM_E_INVALID, "max_images < 1");
  const size_t npix = (size_t)N * N;
  if (nnz < 0 || nnz >= (1ll << 31)) return fail(ADMM_E_INVALID, "nnz must be < 2^31");
  if ((size_t)max_images * npix * 8 >= (1ull << 31) || (size_t)max_images * m * 8 >= (1ull << 31))
    return fail(ADMM_E_INVALID, "batch too large for 32-bit buffer offsets; split it across contexts");
  if (indptr[0] != 0 || indptr[m] != nnz) return fail(ADMM_E_INVALID, "indptr must run from 0 to nnz");
  for (int r = 0; r < m; ++r)
    if (indptr[r + 1] < indptr[r]) return fail(ADMM_E_INVALID, "indptr not non-decreasing");
  for (long long k = 0; k < nnz; ++k)
    if (indices[k] < 0 || (size_t)indices[k] >= npix) return fail(ADMM_E_INVALID, "column index out of range");
  // A^T by a counting sort over columns; within a column the rows stay ascending
  std::vector<int> tptr(npix + 1, 0), tidx((size_t)nnz);
  std::vector<double> tval((size_t)nnz);
  for (long long k = 0; k < nnz; ++k) ++tptr[(size_t)indices[k] + 1];
  for (size_t c = 0; c < npix; ++c) tptr[c + 1] += tptr[c];
  {
    std::vector<int> fill(tptr.begin(), tptr.end() - 1);
    for (int r = 0; r < m; ++r)
      for (long long k = indptr[r]; k < indptr[r + 1]; ++k) {
        const int q = fill[indices[k]]++;
        tidx[q] = r;
        tval[q] = values[k];
      }
  }
  std::vector<int> fptr(m + 1);
  for (int r = 0; r <= m; ++r) fptr[r] = (int)indptr[r];
  DEVICE_SCOPE(device);
  std::unique_ptr<admm_ctx> C(new admm_ctx());
  // a one-"angle" geometry (n_det = m, L = 1): every m-sized buffer, the fixed-order
  // reductions and the combine/residual kernels keep their shapes
  C->g = admm_geom{};
  C->g.N = N;
  C->g.n_angles = 1;
  C->g.n_det = m;
  C->dtype = dtype;
  C->device = device;
  C->max_images = max_images;
  C->npix = (int)npix;
  C->mrays = m;
  C->csr = true;
  C->nnz = nnz;
  FwdAngle fa{};
  fa.L = 1.0;
  BackAngle ba{};
  BackAngleC bc{};
  // the values in the sample dtype
  auto upv = [&](Buf& b, const std::vector<double>& v) {
    if (dtype == ADMM_DTYPE_F64) return upload(b, v, 16);
    return upload(b, std::vector<float>(v.begin(), v.end()), 16);
  };
  RET(upload(C->f_ptr, fptr, 16));
  RET(upload(C->f_idx, indices, (size_t)nnz * 4, 16));
  RET(upv(C->f_val, std::vector<double>(values, values + nnz)));
  RET(upload(C->t_ptr, tptr, 16));
  RET(upload(C->t_idx, tidx, 16));
  RET(upv(C->t_val, tval));
  RET(upload(C->fang_b, &fa, sizeof(fa)));
  RET(upload(C->bang_b, &ba, sizeof(ba)));
  RET(upload(C->bangc_b, &bc, sizeof(bc)));
  HIPCHK(hipStreamCreateWithFlags(&C->cap.s, hipStreamNonBlocking));
  *out = C.release();
  return ADMM_OK;
}

int admm_ctx_destroy(admm_ctx* C) {
  if (!C) return ADMM_OK;
  delete C;
  return ADMM_OK;
}

int admm_project_fwd(admm_ctx* C, const void* img, void* sino, int nimg, void* stream) {
  if (!C || !img || !sino) return fail(ADMM_E_INVALID, "null argument");
  if (nimg < 1 || nimg > C->max_images) return fail(ADMM_E_INVALID, "nimg out of range");
  hipStream_t s = (hipStream_t)stream;
  DEVICE_SCOPE(C->device);
  return with_type(C->dtype, [&](auto tt) {
    using T = typename decltype(tt)::type;
    return op_forward<T>(C, (const T*)img, (T*)sino, nimg, s);
  });
}

int admm_project_adj(admm_ctx* C, const void* sino, void* img, int nimg, void* stream) {
  if (!C || !img || !sino) return fail(ADMM_E_INVALID, "null argument");
  if (nimg < 1 || nimg > C->max_images) return fail(ADMM_E_INVALID, "nimg out of range");
  DEVICE_SCOPE(C->device);
  hipStream_t s = (hipStream_t)stream;
  return with_type(C->dtype, [&](auto tt) {
    using T = typename decltype(tt)::type;
    BackArgs<T> a{};
    a.sino = (const T*)sino;
    a.out_t = (T*)img;
    return launch_back<T, 1, BACK_PLAIN>(C, a, nimg, s);
  });
}

int admm_column_norms_sq(admm_ctx* C, double* W, void* stream) {
  if (!C || !W) return fail(ADMM_E_INVALID, "null argument");
  DEVICE_SCOPE(C->device);
  hipStream_t s = (hipStream_t)stream;
  return with_type(C->dtype, [&](auto tt) {
    using T = typename decltype(tt)::type;
    BackArgs<T> a{};
    a.out_d = W;
    return launch_back<T, 1, BACK_WSQ>(C, a, 1, s);
  });
}

int admm_column_norms_sq_weighted(admm_ctx* C, const void* w, double* W, void* stream) {
  if (!C || !w || !W) return fail(ADMM_E_INVALID, "null argument");
  if (C->csr)
    return fail(ADMM_E_INVALID, "weighted column norms are not supported for explicit-matrix contexts: scale "
                                "the rows of A by sqrt(omega) instead (exact there)");
  DEVICE_SCOPE(C->device);
  hipStream_t s = (hipStream_t)stream;
  return with_type(C->dtype, [&](auto tt) {
    using T = typename decltype(tt)::type;
    BackArgs<T> a{};
    a.sino = (const T*)w;
    a.out_d = W;
    return launch_back<T, 1, BACK_WSQW>(C, a, 1, s);
  });
}

int admm_tv_grad(admm_ctx* C, const double* x, double* gx, double* gy, int nimg, void* stream) {
  if (!C || !x || !gx || !gy || nimg < 1) return fail(ADMM_E_INVALID, "bad argument");
  DEVICE_SCOPE(C->device);
  const int N = C->g.N;
  hipLaunchKernelGGL(k_tv_grad, dim3((N + 63) / 64, (N + 3) / 4, nimg), dim3(kBlock), 0, (hipStream_t)stream, x,
                     gx, gy, N);
  CHECK_LAUNCH();
  return ADMM_OK;
}

int admm_tv_div(admm_ctx* C, const double* px, const double* py, double* out, int nimg, void* stream) {
  if (!C || !px || !py || !out || nimg < 1) return fail(ADMM_E_INVALID, "bad argument");
  DEVICE_SCOPE(C->device);
  const int N = C->g.N;
  hipLaunchKernelGGL(k_tv_div, dim3((N + 63) / 64, (N + 3) / 4, nimg), dim3(kBlock), 0, (hipStream_t)stream, px,
                     py, out, N);
  CHECK_LAUNCH();
  return ADMM_OK;
}

int admm_batch_bind(admm_ctx* C, const admm_batch* batch) {
  if (!C || !batch) return fail(ADMM_E_INVALID, "null argument");
  const admm_batch& B = *batch;
  if (B.V < 1) return fail(ADMM_E_INVALID, "batch V < 1");
  if (B.n_xext < B.V) return fail(ADMM_E_INVALID, "n_xext < V");
  if (B.tv_iters < 1 || B.cg_iters < 1) return fail(ADMM_E_INVALID, "tv_iters and cg_iters must be >= 1");
  if (B.tv_kind != ADMM_TV_ISO && B.tv_kind != ADMM_TV_ANISO) return fail(ADMM_E_INVALID, "bad tv_kind");
  if (!(B.mu > 0)) return fail(ADMM_E_INVALID, "mu must be > 0");
  if (!B.x_ext || !B.d || !B.e || !B.atb || !B.dsum || !B.b || !B.inc_off || !B.node_stats)
    return fail(ADMM_E_INVALID, "null batch pointer");
  if (B.n_edges > 0 && (!B.y || !B.q || !B.edge_a || !B.edge_b || !B.inc_edge || !B.inc_qslot ||
                        !B.inc_sign || !B.edge_stats))
    return fail(ADMM_E_INVALID, "null edge pointer");
  if (B.n_edges > 0 && !B.z) {
    if (!B.x_prev) return fail(ADMM_E_INVALID, "z == NULL needs x_prev (derived consensus)");
    if (B.fusion != ADMM_FUSE_MIDPOINT) return fail(ADMM_E_INVALID, "derived z needs midpoint fusion");
  }
  if (B.fusion != ADMM_FUSE_MIDPOINT && B.fusion != ADMM_FUSE_WEIGHTED) return fail(ADMM_E_INVALID, "bad fusion");
  if (B.flags & ~ADMM_BATCH_KEEP_X) return fail(ADMM_E_INVALID, "unknown batch flags");
  if (B.fusion == ADMM_FUSE_WEIGHTED && B.n_edges > 0 && (!B.y_b || !B.w))
    return fail(ADMM_E_INVALID, "weighted fusion needs y_b and w");
  if (B.n_edges > 65535) return fail(ADMM_E_INVALID, "more than 65535 edge slots on one device");
  const size_t npix = C->npix, m = C->mrays;
  if ((size_t)B.V * npix * 8 >= (1ull << 31) || (size_t)B.V * m * 8 >= (1ull << 31))
    return fail(ADMM_E_INVALID, "batch too large for 32-bit buffer offsets");
  DEVICE_SCOPE(C->device);
  HIPCHK(hipDeviceSynchronize());
  free_graphs(C);
  C->b = B;
  C->weighted = false;  // a bind drops the per-ray weights (admm_batch_set_ray_weights)
  const int V = B.V;
  C->vb = vb_for(V, C->dtype);
  RET(bind_fwd_plan(C, V));
  const size_t Vp = (size_t)((V + C->vb - 1) / C->vb) * C->vb;  // padded to whole chunks
  const size_t ds = dsize(C->dtype);
  RET(ensure(C->xs, Vp * npix * ds));
  RET(ensure(C->xsT, Vp * npix * ds));
  RET(ensure(C->p, Vp * npix * ds));
  RET(ensure(C->pT, Vp * npix * ds));
  RET(ensure(C->Hp, Vp * npix * ds));
  RET(ensure(C->dsumS, Vp * npix * ds));
  RET(ensure(C->x2, (size_t)V * npix * 8));
  RET(ensure(C->p2, Vp * npix * ds));
  if (B.cg_iters > 1 && B.cg_iters <= kMaxCgRing)
    RET(ensure(C->pring, (size_t)(B.cg_iters - 1) * Vp * npix * ds));
  if (B.flags & ADMM_BATCH_KEEP_X) RET(ensure(C->ats, Vp * npix * ds));
  C->ats_valid = C->ats_stale = false;
  RET(ensure(C->sino, Vp * m * ds));
  RET(ensure(C->bI, Vp * m * ds));
  RET(ensure(C->r, V * npix * 8));
  RET(ensure(C->c, V * npix * 8));
  RET(ensure(C->d2, 2 * V * npix * 8));
  RET(ensure(C->e2, 2 * V * npix * 8));
  C->P_back = back_partitions(C);
  const int N = C->g.N;
  C->P_tile = ((N + kTile - 1) / kTile) * ((N + kTile - 1) / kTile);
  if ((size_t)Vp * npix * ds >= (1ull << 31) || (size_t)Vp * m * ds >= (1ull << 31))
    return fail(ADMM_E_INVALID, "batch too large for 32-bit buffer offsets");
  C->P_fwd = C->mm ? (int)((C->half->mrays + kBlock - 1) / kBlock)
           : (C->n_groups > 0 || C->csr) ? (int)((m + kBlock - 1) / kBlock)
                                         : ((C->g.n_det + kFwdRays - 1) / kFwdRays) * C->g.n_angles;
  // partials per (edge, 1024 pixels) for the stored-z kernels, per (edge, 64-pixel block) for the
  // derived-z ones
  C->P_edge = B.z ? (int)((npix + kBlock * 4 - 1) / (kBlock * 4)) : (int)((npix + kConsPix - 1) / kConsPix);
  RET(ensure(C->partH, (size_t)5 * V * C->P_back * 8));
  RET(ensure(C->partS, (size_t)V * C->P_fwd * 8));
  RET(ensure(C->partD, (size_t)5 * V * C->P_back * 8));
  RET(ensure(C->partE, (size_t)3 * std::max(1, B.n_edges) * C->P_edge * 8));
  RET(ensure(C->redH, (size_t)5 * V * 8 * std::max(1, std::min(B.cg_iters, kMaxCgRing))));
  C->bound = true;
  // rho D, D = sum_j q_ij, as interleaved samples of the sample dtype (the BACK_H epilogue's
  // rho D p term): setup data, packed and scaled once here rather than in every x-update (rho
  // is the bound batch's; a re-bind packs again)
  RET(with_type_vb(C->dtype, C->vb, [&](auto tt, auto vbc) {
    using T = typename decltype(tt)::type;
    constexpr int VB = decltype(vbc)::value;
    const int nch = (V + VB - 1) / VB;
    hipLaunchKernelGGL((k_pack_d<T, VB>), dim3((unsigned)((npix + 255) / 256), nch), dim3(256), 0, C->cap.s, B.dsum,
                       (T*)C->dsumS.p, (int)npix, V, B.rho);
    CHECK_LAUNCH();
    return ADMM_OK;
  }));
  HIPCHK(hipStreamSynchronize(C->cap.s));
  RET(record_graphs(C));
  HIPCHK(hipDeviceSynchronize());
  return ADMM_OK;
}

int admm_batch_set_ray_weights(admm_ctx* C, const void* w, void* stream) {
  if (!C || !C->bound) return fail(ADMM_E_STATE, "no batch bound");
  if (C->csr)
    return fail(ADMM_E_INVALID, "per-ray weights are not supported for explicit-matrix contexts: scale the "
                                "rows of A and b by sqrt(omega) instead (exact there)");
  DEVICE_SCOPE(C->device);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipDeviceSynchronize());
  if (!w && !C->weighted) return ADMM_OK;
  C->weighted = false;
  C->ats_valid = C->ats_stale = false;  // the kept A^T s belongs to the previous weights
  if (w) {
    const int V = C->b.V, m = C->mrays;
    const size_t Vp = (size_t)((V + C->vb - 1) / C->vb) * C->vb;
    RET(ensure(C->wS, Vp * m * dsize(C->dtype)));
    RET(with_type_vb(C->dtype, C->vb, [&](auto tt, auto vbc) {
      using T = typename decltype(tt)::type;
      constexpr int VB = decltype(vbc)::value;
      const dim3 grid((m + 255) / 256, (V + VB - 1) / VB);
      hipLaunchKernelGGL((k_pack<T, VB>), grid, dim3(256), 0, s, (const T*)w, (T*)C->wS.p, m, V);
      CHECK_LAUNCH();
      return ADMM_OK;
    }));
    HIPCHK(hipStreamSynchronize(s));
    C->weighted = true;
  }
  RET(record_graphs(C));
  HIPCHK(hipDeviceSynchronize());
  return ADMM_OK;
}

// New values for the weights of a batch that has some (robust reweighting): the set
// call's k_pack launch into the same wS, on `stream`, and nothing else.  The recorded sequences
// already hold the weighted launches and read wS by its pointer, which does not move: wS is sized by
// V, m and the dtype of the bound batch (ensure() keeps a buffer that is large enough), and a bind,
// the only call that changes those, clears `weighted`, so the next weights come through the set call.
int admm_batch_update_ray_weights(admm_ctx* C, const void* w, void* stream) {
  if (!C || !C->bound) return fail(ADMM_E_STATE, "no batch bound");
  if (C->csr)
    return fail(ADMM_E_INVALID, "per-ray weights are not supported for explicit-matrix contexts: scale the "
                                "rows of A and b by sqrt(omega) instead (exact there)");
  if (!w) return fail(ADMM_E_INVALID, "w is null (admm_batch_set_ray_weights clears the weights)");
  if (!C->weighted) return fail(ADMM_E_STATE, "the batch has no ray weights: admm_batch_set_ray_weights first");
  DEVICE_SCOPE(C->device);
  hipStream_t s = (hipStream_t)stream;
  const int V = C->b.V, m = C->mrays;
  RET(with_type_vb(C->dtype, C->vb, [&](auto tt, auto vbc) {
    using T = typename decltype(tt)::type;
    constexpr int VB = decltype(vbc)::value;
    const dim3 grid((m + 255) / 256, (V + VB - 1) / VB);
    hipLaunchKernelGGL((k_pack<T, VB>), grid, dim3(256), 0, s, (const T*)w, (T*)C->wS.p, m, V);
    CHECK_LAUNCH();
    return ADMM_OK;
  }));
  C->ats_stale = C->ats_stale || C->ats_valid;  // (what admm_batch_refresh_kept may form again)
  C->ats_valid = false;  // the kept A^T s belongs to the previous weights
  return ADMM_OK;
}

// The kept A^T s of a KEEP_X batch formed again under the weights admm_batch_update_ray_weights gave
// it: the update's own epilogue launches -- s = omega (A xs - b) from the kept samples xs of the last
// update's x, then the DIAG back projection into ats -- without the reductions into node_stats (their
// partials land in the update's scratch, which the next update overwrites).  The next update then
// starts from k_start_reuse, as in a run whose weights never change; with unchanged weights the
// launches and their inputs are the epilogue's, so ats is bitwise what the update left.
int admm_batch_refresh_kept(admm_ctx* C, void* stream) {
  if (!C || !C->bound) return fail(ADMM_E_STATE, "no batch bound");
  if (!(C->b.flags & ADMM_BATCH_KEEP_X) || !C->ats_stale)
    return fail(ADMM_E_STATE, "no kept A^T s to refresh: a KEEP_X batch right after admm_batch_update_ray_weights");
  DEVICE_SCOPE(C->device);
  hipStream_t s = (hipStream_t)stream;
  RET(with_type_vb(C->dtype, C->vb, [&](auto tt, auto vbc) {
    using T = typename decltype(tt)::type;
    constexpr int VB = decltype(vbc)::value;
    const admm_batch& B = C->b;
    T* sino = (T*)C->sino.p;
    RET((launch_fwd_batch<T, VB, 1>(C, (T*)C->xs.p, (T*)C->xsT.p, sino, (const T*)B.b, (double*)C->partS.p, B.V, s)));
    BackArgs<T> a{};
    a.sino = sino;
    a.part = (double*)C->partD.p;
    a.dsum = B.dsum;
    a.cvec = (double*)C->c.p;
    a.x = B.x_ext;
    a.phantom = B.phantom;
    a.edges = edge_in(B);
    a.qv = B.q;
    a.inc_off = B.inc_off;
    a.inc_edge = B.inc_edge;
    a.inc_qslot = B.inc_qslot;
    a.inc_sign = B.inc_sign;
    a.rho = B.rho;
    a.lam = B.lam;
    a.mu = B.mu;
    a.tv_kind = B.tv_kind;
    a.evar = B.e;
    a.out_t = (T*)C->ats.p;
    return launch_back<T, VB, BACK_DIAG>(C, a, B.V, s);
  }));
  C->ats_valid = true;
  C->ats_stale = false;
  return ADMM_OK;
}

// rho of the bound batch <- rho (residual balancing): what a bind does with rho and
// nothing else -- rho D packed again by the bind's own launch, the sequences recorded again.  The
// per-ray weights, the forward plan and all scratch stay.
int admm_batch_set_rho(admm_ctx* C, double rho, void* stream) {
  if (!std::isfinite(rho) || !(rho > 0.0)) return fail(ADMM_E_INVALID, "rho must be finite and > 0");
  if (!C || !C->bound) return fail(ADMM_E_STATE, "no batch bound");
  DEVICE_SCOPE(C->device);
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  HIPCHK(hipDeviceSynchronize());
  C->b.rho = rho;
  const int V = C->b.V;
  const size_t npix = C->npix;
  RET(with_type_vb(C->dtype, C->vb, [&](auto tt, auto vbc) {
    using T = typename decltype(tt)::type;
    constexpr int VB = decltype(vbc)::value;
    const int nch = (V + VB - 1) / VB;
    hipLaunchKernelGGL((k_pack_d<T, VB>), dim3((unsigned)((npix + 255) / 256), nch), dim3(256), 0, C->cap.s,
                       C->b.dsum, (T*)C->dsumS.p, (int)npix, V, rho);
    CHECK_LAUNCH();
    return ADMM_OK;
  }));
  HIPCHK(hipStreamSynchronize(C->cap.s));
  C->ats_valid = C->ats_stale = false;  // (one projection more in the next update: the reuse start is not reasoned about)
  RET(record_graphs(C));
  HIPCHK(hipDeviceSynchronize());
  return ADMM_OK;
}

int admm_batch_atb(admm_ctx* C, double* atb_out, void* stream) {
  if (!C || !C->bound) return fail(ADMM_E_STATE, "no batch bound");
  if (!atb_out) return fail(ADMM_E_INVALID, "null atb_out");
  DEVICE_SCOPE(C->device);
  hipStream_t s = (hipStream_t)stream;
  const int V = C->b.V;
  return with_type_vb(C->dtype, C->vb, [&](auto tt, auto vbc) {
    using T = typename decltype(tt)::type;
    constexpr int VB = decltype(vbc)::value;
    const int nch = (V + VB - 1) / VB;
    if (C->weighted)  // A^T (omega b)
      hipLaunchKernelGGL((k_pack_w<T, VB>), dim3((C->mrays + 255) / 256, nch), dim3(256), 0, s, (const T*)C->b.b,
                         (const T*)C->wS.p, (T*)C->bI.p, C->mrays, V);
    else
      hipLaunchKernelGGL((k_pack<T, VB>), dim3((C->mrays + 255) / 256, nch), dim3(256), 0, s, (const T*)C->b.b,
                         (T*)C->bI.p, C->mrays, V);
    CHECK_LAUNCH();
    BackArgs<T> a{};
    a.sino = (const T*)C->bI.p;
    a.out_d = atb_out;
    return launch_back<T, VB, BACK_ATB>(C, a, V, s);
  });
}

int admm_node_update(admm_ctx* C, void* stream) {
  if (!C || !C->bound) return fail(ADMM_E_STATE, "no batch bound");
  DEVICE_SCOPE(C->device);
  hipStream_t s = (hipStream_t)stream;
  const bool keep = (C->b.flags & ADMM_BATCH_KEEP_X) != 0;
  const bool reuse = keep && C->ats_valid;
  int rc = ADMM_OK;
  if (C->upd.x) {
    HIPCHK(hipGraphLaunch(reuse ? C->upd_reuse.x : C->upd.x, s));
  } else {
    rc = enqueue_update_any(C, s, reuse);
  }
  if (rc == ADMM_OK && keep) C->ats_valid = true;  // this update's DIAG left A^T s of its x
  C->ats_stale = false;
  return rc;
}

int admm_node_update_rounds(admm_ctx* C, int tv_iters, void* stream) {
  if (!C || !C->bound) return fail(ADMM_E_STATE, "no batch bound");
  if (tv_iters < 1) return fail(ADMM_E_INVALID, "tv_iters must be >= 1");
  if (tv_iters == C->b.tv_iters) return admm_node_update(C, stream);
  DEVICE_SCOPE(C->device);
  hipStream_t s = (hipStream_t)stream;
  const bool keep = (C->b.flags & ADMM_BATCH_KEEP_X) != 0;
  const bool reuse = keep && C->ats_valid;
  // a round count other than the bound one: enqueued directly (no recorded graph)
  const int rc = enqueue_update_any(C, s, reuse, tv_iters);
  if (rc == ADMM_OK && keep) C->ats_valid = true;
  C->ats_stale = false;
  return rc;
}

int admm_consensus(admm_ctx* C, void* stream) {
  if (!C || !C->bound) return fail(ADMM_E_STATE, "no batch bound");
  DEVICE_SCOPE(C->device);
  hipStream_t s = (hipStream_t)stream;
  if (C->cons.x) {
    HIPCHK(hipGraphLaunch(C->cons.x, s));
    return ADMM_OK;
  }
  return enqueue_consensus(C, s);
}

extern "C++" {
// One x-update enqueued directly (the graph's launch sequence, no graph) with timing-only
// events around every in-solve launch of `kind` (0: the forward tap kernel of each CG step,
// right after the CG / TV update that wrote p and p^T; 1: the back projector of each CG step,
// right after its forward combine), exactly as in every replay; ms = their average duration.
static int time_in_solve(admm_ctx* C, int kind, hipStream_t s, float* ms) {
  return with_type_vb(C->dtype, C->vb, [&](auto tt, auto vbc) -> int {
    using T = typename decltype(tt)::type;
    constexpr int VB = decltype(vbc)::value;
    const int n = C->b.tv_iters * C->b.cg_iters;
    std::vector<Event> ev(2 * n);
    for (Event& e : ev) RET(e.create());
    C->tf_ev = &ev;
    C->tf_next = 0;
    C->tf_kind = kind;
    const bool keep = (C->b.flags & ADMM_BATCH_KEEP_X) != 0;
    int rc = enqueue_update<T, VB>(C, s, keep && C->ats_valid);
    const size_t used = C->tf_next;
    C->tf_ev = nullptr;
    C->tf_kind = 0;
    if (rc == ADMM_OK && keep) C->ats_valid = true;
    if (rc == ADMM_OK && used == 0) rc = fail(ADMM_E_STATE, "no launch was timed");
    if (rc == ADMM_OK) {
      HIPCHK(hipEventSynchronize(ev[used - 1].e));
      float tot = 0.f;
      for (size_t i = 0; i < used; i += 2) {
        float t = 0.f;
        HIPCHK(hipEventElapsedTime(&t, ev[i].e, ev[i + 1].e));
        tot += t;
      }
      *ms = tot / (float)(used / 2);
    }
    return rc;
  });
}

static int time_fwd(admm_ctx* C, int reps, int in_solve, hipStream_t s, float* ms) {
  if (in_solve) return time_in_solve(C, 0, s, ms);
  return with_type_vb(C->dtype, C->vb, [&](auto tt, auto vbc) -> int {
    using T = typename decltype(tt)::type;
    constexpr int VB = decltype(vbc)::value;
    // the forward tap kernel alone, back to back: k_fwdg (every sample tap) when grouped, else k_fwd
    auto one = [&]() -> int {
      if (C->n_groups > 0) return launch_fwdg_taps<T, VB>(C, (T*)C->xs.p, (T*)C->xsT.p, C->b.V, s);
      return launch_fwd<T, VB, 0>(C, (T*)C->xs.p, (T*)C->xsT.p, (T*)C->sino.p, nullptr, nullptr, C->b.V, s,
                                  C->weighted ? (const T*)C->wS.p : nullptr);
    };
    RET(one());
    Event e0, e1;
    RET(e0.create());
    RET(e1.create());
    HIPCHK(hipEventRecord(e0.e, s));
    int rc = ADMM_OK;
    for (int i = 0; i < reps && rc == ADMM_OK; ++i) rc = one();
    HIPCHK(hipEventRecord(e1.e, s));
    HIPCHK(hipEventSynchronize(e1.e));
    HIPCHK(hipEventElapsedTime(ms, e0.e, e1.e));
    return rc;
  });
}
}  // extern "C++"

int admm_time_forward(admm_ctx* C, int reps, int in_solve, void* stream, double* ms_out) {
  if (!C || !C->bound) return fail(ADMM_E_STATE, "no batch bound");
  if (reps < 1 || !ms_out) return fail(ADMM_E_INVALID, "bad argument");
  DEVICE_SCOPE(C->device);
  hipStream_t s = (hipStream_t)stream;
  float ms = 0.f;
  RET(time_fwd(C, reps, in_solve, s, &ms));
  *ms_out = in_solve ? (double)ms : (double)ms / reps;
  return ADMM_OK;
}

int admm_consensus_range(admm_ctx* C, int e0, int e1, int rows, void* stream) {
  if (!C || !C->bound) return fail(ADMM_E_STATE, "no batch bound");
  const admm_batch& B = C->b;
  if (B.z == nullptr || B.fusion != ADMM_FUSE_MIDPOINT)
    return fail(ADMM_E_STATE, "admm_consensus_range needs stored z and midpoint fusion");
  if (e0 < 0 || e1 < e0 || e1 > B.n_edges) return fail(ADMM_E_INVALID, "edge range out of bounds");
  if (rows < 1 || rows > B.n_xext) return fail(ADMM_E_INVALID, "rows out of range");
  DEVICE_SCOPE(C->device);
  return enqueue_consensus_stored(C, e0, e1, (hipStream_t)stream);
}

int admm_time_back(admm_ctx* C, void* stream, double* ms_out) {
  if (!C || !C->bound) return fail(ADMM_E_STATE, "no batch bound");
  if (!ms_out) return fail(ADMM_E_INVALID, "bad argument");
  DEVICE_SCOPE(C->device);
  hipStream_t s = (hipStream_t)stream;
  float ms = 0.f;
  RET(time_in_solve(C, 1, s, &ms));
  *ms_out = (double)ms;
  return ADMM_OK;
}

int admm_batch_info(admm_ctx* C, int* vb, int* mirror) {
  if (!C || !vb || !mirror) return fail(ADMM_E_INVALID, "bad argument");
  if (!C->bound) return fail(ADMM_E_STATE, "no batch bound");
  *vb = C->vb;
  *mirror = C->mm ? 1 : 0;
  return ADMM_OK;
}

int admm_fwd_plan_info(admm_ctx* C, int plan, int* groups, int* blocks, double* staged, int* active) {
  if (!C || plan < 0 || plan >= admm_ctx::kPlans || !groups || !blocks || !staged || !active)
    return fail(ADMM_E_INVALID, "bad argument");
  if (C->mm && C->half) C = C->half.get();  // mirror mode: the half geometry's plans are the bound ones
  *groups = C->plan_n[plan];
  *blocks = C->plan_blocks[plan];
  *staged = C->plan_staged[plan];
  *active = (C->plan_n[plan] > 0 && C->groups == C->plan_groups(plan)) ? 1 : 0;
  return ADMM_OK;
}

}  // extern "C"
