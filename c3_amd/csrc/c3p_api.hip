// C ABI of libc3prop.so (see include/c3prop.h for the contract and the reference
// functions each entry point stands in for).
#include <algorithm>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <vector>
#include <cstdio>
#include <cstdarg>
#include <cstring>
#include <cstdlib>
#include <cctype>
#include <cmath>

#include "../../include/c3prop.h"
#include "c3p_kernels.h"
#include "c3p_ode.h"
#include "c3p_smalld.h"
#include "c3p_smallr.h"
#include "c3p_midd.h"
#include <cxxabi.h>
#include <cstring>

#include "c3p_bigd.h"
#include "c3p_regd.h"
#include <atomic>
#include "c3p_tiled.h"
#include "c3p_signal.h"
#include "c3p_grad.h"
#include "c3p_seq.h"
#include "c3p_seq_vjp.h"
#include "c3p_ode_vjp.h"
#include "c3p_dress.h"
#include "c3p_readout.h"

namespace {

thread_local std::string g_err;
thread_local int g_last_kernel = C3P_KERNEL_NONE;
// launch log of the current API call (c3p_note_launch / c3p_last_kernel_detail)
struct LaunchNote {
  const void* fn;
  const char* file;
  int count;
};
thread_local LaunchNote g_notes[48];
thread_local int g_nnotes = 0;
thread_local std::string g_note_plan;  // a plan parameter the last call reports beside its kernels (c3p_seq_chain_vjp: the checkpoint interval)
thread_local hipStream_t g_call_stream = nullptr;  // stream of the call in flight (capture check on workspace growth)
thread_local bool g_dry = false;  // c3p_reserve: run the planning and size the workspace, launch nothing

// ---- the options table (c3p_kernels.h) ----
const char* const g_opt_names[C3P_OPT_COUNT] = {
#define C3P_OPT_NAME(n) #n,
    C3P_OPTION_LIST(C3P_OPT_NAME)
#undef C3P_OPT_NAME
};
std::atomic<long> g_opt_val[C3P_OPT_COUNT];
std::once_flag g_opt_once;

long parse_opt_value(const char* v) {
  if (!v || !*v) return 1;  // NAME= : a switch that is set
  char* end = nullptr;
  const long x = strtol(v, &end, 10);
  if (end != v && *end == 0) return x;
  if (!strcmp(v, "all")) return 2;
  if (!strcmp(v, "unset") || !strcmp(v, "default")) return -1;
  return 1;
}

void opt_init() {
  for (int i = 0; i < C3P_OPT_COUNT; ++i) {
    std::string env = "C3P_";
    for (const char* c = g_opt_names[i]; *c; ++c) env += (char)toupper((unsigned char)*c);
    const char* v = getenv(env.c_str());  // read ONCE, here
    g_opt_val[i].store(v ? parse_opt_value(v) : -1, std::memory_order_relaxed);
  }
}

int fail(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return -1;
}

#define HIP_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t e__ = (expr);                                                           \
    if (e__ != hipSuccess) return fail("%s failed: %s", #expr, hipGetErrorString(e__)); \
  } while (0)

#define LAUNCH_TRY(expr) \
  do {                   \
    if (!g_dry) HIP_TRY(expr); \
  } while (0)

// Per-device workspace slots, grown lazily, freed by c3p_shutdown().
enum Slot { SL_SEG_A = 0, SL_SEG_B, SL_SCRATCH, SL_CLP, SL_TABLES, SL_COUNTERS, SL_COUNTERS2, SL_IN0, SL_IN1, SL_IN2, SL_IN3, SL_IN4, SL_IN5, SL_IN6, SL_IN7, SL_OUT0, SL_OUT1, SL_OUT2, SL_OUT3, SL_OUT4, SL_OUT5, SL_OUT6, SL_SEG_F, SL_SEQ_FLAG, SL_SEQ_VJP_WS, SL_SEQ_VJP_SLAB, SL_ODE_VJP_WS, SL_LMODEL_PART, SL_LMODEL_OUT, SL_COUNT };

struct DeviceWs {
  std::mutex mu;  // one lock per device: calls on different GPUs of one process do not serialise
  void* ptr[SL_COUNT] = {};
  size_t cap[SL_COUNT] = {};
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool ev_valid = false;
  std::atomic<int> profiling{0};  // per device, like the event pair it arms (c3p_set_profiling acts on the current device)
  std::atomic<long> generation{0};  // bumped whenever a slot is (re)allocated: steady state = constant
  // The workspace (segment products, tables, arrival counters, arena) is ONE set per device and calls are asynchronous:
  // a call on another stream than the previous one first makes its stream wait for the event recorded at the end of that
  // call, so two streams never run kernels on the shared workspace at the same time (calls on one stream are ordered
  // by the stream itself).
  hipEvent_t done = nullptr;
  hipStream_t last_stream = nullptr;
  bool has_last = false;
  // a BLOCKING stream of the library's own: calls made on the legacy default stream (what torch hands over by default)
  // cannot capture graphs; work enqueued here is ordered against the default stream by the legacy-stream rule
  hipStream_t aux = nullptr;
};

std::mutex g_mu;  // guards the table of per-device workspaces only
std::vector<std::unique_ptr<DeviceWs>> g_ws;

DeviceWs* ws_for_current_device() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(g_mu);
  if ((int)g_ws.size() <= dev) g_ws.resize(dev + 1);
  if (!g_ws[dev]) g_ws[dev].reset(new DeviceWs());
  return g_ws[dev].get();
}

// RAII: the current device's workspace, locked for this call and ordered after the previous call's stream
struct WsLock {
  DeviceWs* w = nullptr;
  hipStream_t st = nullptr;
  bool locked = false;
  bool ok = true;
  WsLock(hipStream_t stream, bool order = true) : st(stream) {
    w = ws_for_current_device();
    if (!w) return;
    w->mu.lock();
    locked = true;
    g_call_stream = stream;
    if (order) g_note_plan.clear();
    if (order) g_nnotes = 0;  // a compute call starts a new launch log (c3p_last_kernel_ms looks with order = false)
    // a capturing stream takes no dependency on work outside its graph: the caller orders other streams before the capture
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (stream && hipStreamIsCapturing(stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone) order = false;
    (void)hipGetLastError();
    // The workspace is shared by the calls of a device: a call on ANOTHER stream than the previous one first waits for
    // everything enqueued on that stream so far.  The event is recorded lazily, here, on the previous stream (enqueue order
    // is fixed by the mutex), so the common one-stream caller pays no event per call (a marker packet between every two
    // kernels: ~3 us of a 140 us cfg2 batch).  A previous stream that has been destroyed meanwhile: device-wide sync.
    if (order && w->has_last && w->last_stream != st) {
      if (!w->done) (void)hipEventCreateWithFlags(&w->done, hipEventDisableTiming);
      if (!w->done || hipEventRecord(w->done, w->last_stream) != hipSuccess || hipStreamWaitEvent(st, w->done, 0) != hipSuccess) {
        (void)hipGetLastError();
        if (hipDeviceSynchronize() != hipSuccess) ok = false;
        w->has_last = false;  // everything enqueued so far is done: forget the (possibly destroyed) stream
        w->last_stream = nullptr;
      }
    }
    ordered = order;
  }
  ~WsLock() {
    if (!locked) return;
    if (ordered) {
      w->last_stream = st;
      w->has_last = true;
    }
    w->mu.unlock();
  }
  bool ordered = true;
};

int ws_get(DeviceWs* w, Slot s, size_t bytes, void** out) {
  if (bytes == 0) bytes = 16;
  if (w->cap[s] < bytes) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (g_call_stream && hipStreamIsCapturing(g_call_stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
      return fail("workspace growth during stream capture: run the call once outside the capture, or c3p_reserve() its shape first");
    (void)hipGetLastError();
    ++w->generation;
    if (w->ptr[s]) {
      HIP_TRY(hipDeviceSynchronize());
      HIP_TRY(hipFree(w->ptr[s]));
      w->ptr[s] = nullptr;
      w->cap[s] = 0;
    }
    size_t want = bytes + bytes / 8;
    HIP_TRY(hipMalloc(&w->ptr[s], want));
    w->cap[s] = want;
    // the arrival counters of the fused combine are self-resetting: zero once, at allocation
    if (s == SL_COUNTERS) HIP_TRY(hipMemset(w->ptr[s], 0, want));
  }
  *out = w->ptr[s];
  return 0;
}

// the timing event pair of c3p_last_kernel_ms around a call's main kernel(s); armed by c3p_set_profiling
int record_start(DeviceWs* w, hipStream_t st) {
  if (!w->profiling || g_dry) return 0;
  if (!w->ev0) {
    HIP_TRY(hipEventCreate(&w->ev0));
    HIP_TRY(hipEventCreate(&w->ev1));
  }
  HIP_TRY(hipEventRecord(w->ev0, st));
  return 0;
}
int record_stop(DeviceWs* w, hipStream_t st) {
  if (!w->profiling || g_dry) return 0;
  HIP_TRY(hipEventRecord(w->ev1, st));
  w->ev_valid = true;
  return 0;
}

struct ChainPlan {
  int S, seg_len;
  bool global_scratch;
};

const int kMaxGenericDm = 256;

ChainPlan plan_generic(int B, int N, int Dm) {
  ChainPlan p;
  const size_t lds = c3p_generic_lds_bytes(Dm);
  p.global_scratch = lds > (size_t)(156 * 1024);
  int wg_per_cu = 2;
  if (!p.global_scratch) {
    wg_per_cu = (int)((160 * 1024) / (lds + 3072));
    if (wg_per_cu < 1) wg_per_cu = 1;
    if (wg_per_cu > 8) wg_per_cu = 8;
  }
  const long target = 256L * wg_per_cu * 2;
  long S = (target + B - 1) / B;
  const long smax = N / 8 > 1 ? N / 8 : 1;
  if (S > smax) S = smax;
  if (S < 1) S = 1;
  p.seg_len = (int)((N + S - 1) / S);
  p.S = (N + p.seg_len - 1) / p.seg_len;
  return p;
}

// Runs one chained propagation (all modes) with the generic kernel, including the
// ordered combine of segment products.  All pointers are device pointers.
// `profile` = false keeps the timing event pair (and c3p_last_kernel) on the caller's main kernel.
int run_chain_generic(DeviceWs* w, ChainArgs base, cplx* U_out, hipStream_t st, bool profile = true) {
  const int Dm = base.Dm;
  // GIVEN mode callers may hand over matrices that live in one of the two segment slots (the segment products of the
  // big-D kernels): this launch must not write its own segment products into the buffer it is reading (and ws_get
  // must not re-allocate it), so it starts on the OTHER slot.
  const bool mats_in_a = base.mats && w->ptr[SL_SEG_A] && (const void*)base.mats == w->ptr[SL_SEG_A];
  const Slot first_slot = mats_in_a ? SL_SEG_B : SL_SEG_A;
  if (Dm > kMaxGenericDm) return fail("matrix dimension %d exceeds the generic kernel limit %d", Dm, kMaxGenericDm);
  const size_t msz = (size_t)Dm * Dm * sizeof(cplx);
  ChainPlan p = plan_generic(base.B, base.N, Dm);
  base.ld = Dm | 1;
  base.S = p.S;
  base.seg_len = p.seg_len;
  const double* final_phase = base.fr_phase;
  cplx* seg = U_out;
  if (p.S > 1) {
    void* v;
    if (ws_get(w, first_slot, (size_t)base.B * p.S * msz, &v)) return -1;
    seg = (cplx*)v;
    base.fr_phase = nullptr;
  }
  base.seg_out = seg;
  if (p.global_scratch) {
    base.scratch_stride = (long)7 * base.ld * Dm;
    void* v;
    if (ws_get(w, SL_SCRATCH, (size_t)base.B * p.S * base.scratch_stride * sizeof(cplx), &v)) return -1;
    base.scratch = (cplx*)v;
  }
  g_last_kernel = p.global_scratch ? C3P_KERNEL_GENERIC_GLOBAL : C3P_KERNEL_GENERIC_LDS;
  if (profile && record_start(w, st)) return -1;
  LAUNCH_TRY(c3p_launch_chain_generic(base, p.global_scratch, st));
  if (profile && record_stop(w, st)) return -1;
  // ordered combine of the S segment products: groups of 8 until <= 16 remain
  int count = p.S;
  cplx* cur = seg;
  Slot next_slot = (first_slot == SL_SEG_A) ? SL_SEG_B : SL_SEG_A;
  while (count > 1) {
    ChainArgs c = {};
    c.mode = C3P_MODE_GIVEN;
    c.mats = cur;
    c.B = base.B;
    c.N = count;
    c.D = base.D;
    c.Dm = Dm;
    c.ld = base.ld;
    c.right_order = base.right_order;
    bool global = p.global_scratch;
    if (count <= 16) {
      c.S = 1;
      c.seg_len = count;
      c.seg_out = U_out;
      c.fr_phase = final_phase;
    } else {
      c.seg_len = 8;
      c.S = (count + 7) / 8;
      void* v;
      if (ws_get(w, next_slot, (size_t)base.B * c.S * msz, &v)) return -1;
      c.seg_out = (cplx*)v;
    }
    if (global) {
      c.scratch_stride = (long)7 * c.ld * Dm;
      void* v;
      // the first launch sized SL_SCRATCH for B*S workgroups >= B*c.S
      if (ws_get(w, SL_SCRATCH, (size_t)c.B * c.S * c.scratch_stride * sizeof(cplx), &v)) return -1;
      c.scratch = (cplx*)v;
    }
    LAUNCH_TRY(c3p_launch_chain_generic(c, global, st));
    cur = c.seg_out;
    count = c.S;
    next_slot = (next_slot == SL_SEG_B) ? SL_SEG_A : SL_SEG_B;
    if (c.seg_out == U_out) break;
  }
  return 0;
}

// ---------------------------------------------------------------------------
// Small-D MFMA path (Dm <= C3P_SMALLD_LIMIT): tables -> segment chains -> ordered combine
// ---------------------------------------------------------------------------
const int kSmallDLimit = 12;  // D = 11, 12 spill ~100 registers but still beat the generic kernel

// the no_t18n option as the kernels' argument structs carry it: its value when set to a positive number, else 0
static inline int opt_no_t18n() { return c3p_opt_on(C3P_OPT_no_t18n) ? (int)c3p_opt(C3P_OPT_no_t18n) : 0; }

// Unitary gradients at 41 <= D <= 64: the VALU sweep (c3p_grad.hip, ~D^3 B) against the tiled sweep (c3p_tiled.hip: matrix cores,
// padded to 64-multiples, so D = 48 and D = 64 cost the same there, and ~35 launches per slice whatever B is).  Measured on one
// MI355X, N = 1000 (tools/bench_grad_41_64.py, profiles/r06/grad_41_64.txt; ms VALU / tiled): D = 48: B = 64 112 / 220,
// B = 256 426 / 505; D = 64: B = 64 254 / 224, B = 256 983 / 519.  Rule: tiled when 1.66 B (D / 48)^3 ms (the VALU estimate)
// exceeds max(220, 1.97 B) ms (the tiled one).
static inline bool tiled_unitary_grad(int D, int B) {
  if (D > 64) return true;
  if (D <= 40) return false;
  if (c3p_opt_on(C3P_OPT_tiled_grad)) return true;
  const double r = (double)D / 48.0, valu = 1.66 * B * r * r * r, tiled = std::max(220.0, 1.97 * B);
  return valu > tiled;
}

// Segments per sample of the VALU backward sweeps (c3p_grad.hip, unitary and general form): one workgroup per (sample, segment),
// 4096 of them in flight, and at least eight slices per segment.  valu_grad_segments pins the count (tests), clamped to 1 .. N: an
// empty segment would make grad_seg_kernel write out a buffer it never filled.
static inline long valu_grad_segments(int B, int N) {
  long S = 4096 / B;
  if (S > N / 8) S = N / 8;
  if (c3p_opt(C3P_OPT_valu_grad_segments) > 0) S = std::min<long>(c3p_opt(C3P_OPT_valu_grad_segments), N);
  return S < 1 ? 1 : S;
}

// One piecewise-constant call after staging: device pointers and sizes.  A batch stride of 0 means one operator set shared
// by all samples.  Every runner below takes this record; the sample chunks of the gradient entry points are cut here only.
struct PwcProblem {
  const cplx* h0;
  long h0_bs;
  const cplx* hks;
  long hk_bs;
  const double* signals;  // [B,K,N]
  const cplx* clp;        // Lindblad dissipator [Dm,Dm] or null
  long clp_bs;            // elements between the samples' dissipators (C3P_COL_PER_SAMPLE: Dm*Dm), 0 = shared
  double dt;
  int B, K, N, D, Dm, lindblad;
  const double* fr_phase;  // [B,Dm] or null
  // model record of the small-D unitary tables (c3p_pwc_record_build) or null; only ever set for shared operators, so a chunk keeps it
  const double* record;
  bool per_sample() const { return h0_bs != 0 || hk_bs != 0 || clp_bs != 0; }
  int nsamp() const { return per_sample() ? B : 1; }  // operator sets (tables) of the call
  // the problem of samples [b0, b0 + nb)
  PwcProblem chunk(long b0, int nb) const {
    PwcProblem c = *this;
    c.h0 += b0 * h0_bs;
    c.hks += b0 * hk_bs;
    if (clp) c.clp += b0 * clp_bs;
    c.signals += b0 * K * N;
    if (fr_phase) c.fr_phase += b0 * Dm;
    c.B = nb;
    return c;
  }
};
// the per-sample cotangents and results of a gradient call at sample b0: U_bar [B,Dm,Dm], grad_signals [B,K,N] and the model-operator
// cotangents of the Lindblad path
const cplx* ubar_at(const PwcProblem& P, const cplx* U_bar, long b0) { return U_bar + b0 * (long)P.Dm * P.Dm; }
double* grad_at(const PwcProblem& P, double* grad_signals, long b0) { return grad_signals + b0 * P.K * P.N; }
struct LindModelOut {
  const cplx* col;  // [C,D,D], or [B,C,D,D] col_bs apart
  long col_bs;
  int C;
  cplx *g_h0, *g_hks, *g_col;  // [nb,D,D], [nb,K,D,D], [nb,C,D,D]
  LindModelOut at(const PwcProblem& P, long b0) const {
    const long dd = (long)P.D * P.D;
    return {col + b0 * col_bs, col_bs, C, g_h0 + b0 * dd, g_hks + b0 * P.K * dd, g_col + b0 * C * dd};
  }
};
// Collapse operators of a Lindblad call: [C,D,D], or [B,C,D,D] under C3P_COL_PER_SAMPLE
long col_bstride(int flags, int C, int D) { return (flags & C3P_COL_PER_SAMPLE) ? (long)C * D * D : 0; }
size_t col_elems(int flags, int B, int C, int D) { return (size_t)((flags & C3P_COL_PER_SAMPLE) ? B : 1) * C * D * D; }
// elements of a batched operand as staged from the host: `one` per sample, `stride` apart (0 = shared: one copy)
size_t staged_elems(int B, int64_t stride, size_t one) { return (size_t)(B - 1) * (size_t)stride + one; }

// The table-build arguments of the three kernel families, from the record; a site adds what is its own (tables, conjT, counters).
PrepArgs prep_args(const PwcProblem& P) {
  PrepArgs p = {};
  p.h0 = P.h0;
  p.h0_bstride = P.h0_bs;
  p.hks = P.hks;
  p.hks_bstride = P.hk_bs;
  p.clp = P.clp;
  p.clp_bstride = P.clp_bs;
  p.dt = P.dt;
  p.K = P.K;
  p.Dh = P.D;
  p.lindblad = P.lindblad;
  return p;
}
MidPrepArgs mid_prep_args(const PwcProblem& P, int nig, int wd) {
  MidPrepArgs p = {};
  p.h0 = P.h0;
  p.h0_bstride = P.h0_bs;
  p.hks = P.hks;
  p.hks_bstride = P.hk_bs;
  p.clp = P.clp;
  p.clp_bstride = P.clp_bs;
  p.dt = P.dt;
  p.K = P.K;
  p.Dh = P.D;
  p.Dm = P.Dm;
  p.lindblad = P.lindblad;
  p.rows = 16 * nig;
  p.W = wd;
  return p;
}
RegdPrepArgs regd_prep_args(const PwcProblem& P) {
  RegdPrepArgs p = {};
  p.h0 = P.h0;
  p.h0_bstride = P.h0_bs;
  p.hks = P.hks;
  p.hks_bstride = P.hk_bs;
  p.clp = P.clp;
  p.clp_bstride = P.clp_bs;
  p.dt = P.dt;
  p.K = P.K;
  p.Dh = P.D;
  p.Dm = P.Dm;
  p.lindblad = P.lindblad;
  return p;
}
// What every table-driven chain and sweep launch takes from the record, on S segments.  Nothing else: mode, no_t18, no_t18n and
// no_real are set by some sites and left zero by others.
template <class Args>
void fill_chain(Args& a, const PwcProblem& P, long S) {
  a.tab_per_sample = P.per_sample() ? 1 : 0;
  a.signals = P.signals;
  a.B = P.B;
  a.K = P.K;
  a.N = P.N;
  a.Dm = P.Dm;
  a.S = (int)S;
  a.Lmax = (int)((P.N + S - 1) / S);
}
// The same for supplied per-slice generators X_n = coef hs[b,n] (no tables, no signals, K = 0): the chain kernels and the general
// sweep kernels of both families read them from fields of one name.  `meta`: the hmeta pre-pass (trace shift and norm per matrix).
struct Supplied {
  const cplx* hs;
  long hs_bstride;
  const double* meta;
  double coef_r, coef_i;
  int B, N, Dm;
};
template <class Args>
void fill_supplied(Args& a, const Supplied& X, long S) {
  a.hs = X.hs;
  a.hs_bstride = X.hs_bstride;
  a.meta = X.meta;
  a.coef_r = X.coef_r;
  a.coef_i = X.coef_i;
  a.B = X.B;
  a.N = X.N;
  a.Dm = X.Dm;
  a.S = (int)S;
  a.Lmax = (int)((X.N + S - 1) / S);
}

// ordered combine of `count` matrices per sample (cur: [B,count,Dm,Dm]) into U_out on the supplied-matrix mode of a chain kernel
// (launch: c3p_launch_smalld_chain at Dm <= 12, c3p_launch_midd_chain at 13 <= Dm <= 40)
template <class Args>
int combine_chain(hipError_t (*launch)(const Args&, hipStream_t), DeviceWs* w, const cplx* cur, int B, int count, int Dm, int right_order,
                  const double* fr_phase, cplx* U_out, hipStream_t st) {
  const size_t msz = (size_t)Dm * Dm * sizeof(cplx);
  Slot next_slot = SL_SEG_B;
  while (true) {
    Args c = {};
    c.mode = C3P_MODE_GIVEN;
    c.mats = cur;
    c.B = B;
    c.N = count;
    c.Dm = Dm;
    c.right_order = right_order;
    if (count <= 8) {
      c.S = 1;
      c.seg_out = U_out;
      c.fr_phase = fr_phase;
    } else {
      c.S = (count + 3) / 4;
      void* v;
      if (ws_get(w, next_slot, (size_t)B * c.S * msz, &v)) return -1;
      c.seg_out = (cplx*)v;
    }
    c.Lmax = (count + c.S - 1) / c.S;
    LAUNCH_TRY(launch(c, st));
    if (c.seg_out == U_out) break;
    cur = c.seg_out;
    count = c.S;
    next_slot = (next_slot == SL_SEG_B) ? SL_SEG_A : SL_SEG_B;
  }
  return 0;
}

int pick_segments(int B, int N, int K, int Dm, bool need_mult4, long slots = 8192) {
  // two waves per SIMD (the D = 9 kernel fits 256 registers): 256 CUs x 4 SIMDs x 2 x 4 chains are resident at once.
  // B S chains run in ceil(B S / slots) rounds of N / S slices (+ the table build and plan of the prologue):
  // take the S that minimises rounds x segment length, so that the last round is not a mostly idle tail
  // (B = 300 with the old "fill the machine twice" rule ran a second round at 2 % occupancy).
  if (c3p_opt(C3P_OPT_smalld_segments) > 0) {  // tuning override
    const long S = c3p_opt(C3P_OPT_smalld_segments);
    if (S >= 1 && S <= N && (!need_mult4 || S % 4 == 0)) return (int)S;
  }
  // (the backward sweep runs one wave per SIMD: 4096 slots)
  // the segment's control amplitudes live in LDS: 4 chains x K x Lmax doubles
  const long lds_budget = 20 * 1024 - (long)(c3p_smalld_table_doubles(Dm, K) + 4 * c3p_smalld_img_doubles(Dm)) * 8;
  const long lmax_cap = K > 0 ? lds_budget / (32L * K) : (1L << 30);
  long best = -1;
  double best_cost = 1e300;
  const long smax = N < 4096 ? N : 4096;
  for (long S = 1; S <= smax; ++S) {
    // a multiple of four lets every wave fold its four segments in registers (fused combine)
    if (S > 1 && (S % 4) != 0 && S + 3 <= N) continue;
    if (need_mult4 && (S % 4) != 0) continue;
    if ((N + S - 1) / S > lmax_cap) continue;
    const long rounds = ((long)B * S + slots - 1) / slots;
    const double cost = (double)rounds * (double)((N + S - 1) / S + 8);
    if (cost < best_cost * (1.0 - 1e-9)) {
      best_cost = cost;
      best = S;
    }
  }
  if (best < 0 && need_mult4) {
    const long S = ((std::min<long>(N, 4) + 3) / 4) * 4;
    if (S <= N && (N + S - 1) / S <= lmax_cap) best = S;
  }
  return (int)best;
}

// Lindblad chains of one qubit / qutrit whose Hamiltonians the caller declares Hermitian (C3P_HERMITIAN_H): real arithmetic
// in the Hermitian basis on the small-D tile layout (c3p_smallr.hip).  Real generator tables -> segment products (turned back
// into the reference's vectorisation by the chain that formed them) -> ordered product with the frame phases (the
// supplied-matrix mode of the complex small-D chain kernel).  Returns 1 when not applicable.
// segments of the real Hermitian-basis kernels at Dm = 16 (two qubits; one wavefront = four chains, one wavefront per SIMD:
// 4096 chain slots): the S that minimises rounds x segment length within the LDS of both kernels; -1 = none
int pick_segments_r(int B, int N, int K, int Dm, bool need_mult4, bool with_grad) {
  if (c3p_opt(C3P_OPT_smalld_segments) > 0) {
    const long S = c3p_opt(C3P_OPT_smalld_segments);
    if (S >= 1 && S <= N && (!need_mult4 || S % 4 == 0)) return (int)S;
  }
  long best = -1;
  double best_cost = 1e300;
  const long smax = N < 4096 ? N : 4096;
  for (long S = 1; S <= smax; ++S) {
    if (S > 1 && (S % 4) != 0 && S + 3 <= N) continue;
    if (need_mult4 && (S % 4) != 0) continue;
    const int Lmax = (int)((N + S - 1) / S);
    if (c3p_smallr_lds_bytes(Dm, K, Lmax) > (size_t)60 * 1024) continue;
    if (with_grad && c3p_smallr_grad_lds_bytes(Dm, K, Lmax) > (size_t)60 * 1024) continue;
    const long rounds = ((long)B * S + 4095) / 4096;
    const double cost = (double)rounds * (double)(Lmax + 8);
    if (cost < best_cost * (1.0 - 1e-9)) {
      best_cost = cost;
      best = S;
    }
  }
  return (int)best;
}
int run_pwc_smallr(DeviceWs* w, const PwcProblem& P, cplx* U_out, hipStream_t st) {
  const int B = P.B, K = P.K, N = P.N, Dm = P.Dm;
  const bool per_sample = P.per_sample();
  int S = Dm > 12 ? pick_segments_r(B, N, K, Dm, per_sample, false) : pick_segments(B, N, K, Dm, per_sample);
  if (S < 0) return 1;
  while (S < N && c3p_smallr_lds_bytes(Dm, K, (N + S - 1) / S) > (size_t)60 * 1024) S += per_sample ? 4 : 1;
  if (c3p_smallr_lds_bytes(Dm, K, (N + S - 1) / S) > (size_t)60 * 1024) return 1;
  const int nsamp = P.nsamp();
  const size_t tdoubles = (size_t)nsamp * c3p_smallr_table_doubles(Dm, K);
  const size_t fl_off = (tdoubles * sizeof(double) + 255) & ~(size_t)255;
  void *tv, *sv;
  if (ws_get(w, SL_TABLES, fl_off + (size_t)nsamp * (1 + K) * sizeof(int), &tv)) return -1;
  if (ws_get(w, SL_SEG_A, (size_t)B * S * Dm * Dm * sizeof(cplx), &sv)) return -1;
  double* tabs = (double*)tv;
  int* flags = reinterpret_cast<int*>(static_cast<char*>(tv) + fl_off);
  LAUNCH_TRY(c3p_launch_smallr_prep(regd_prep_args(P), nsamp, tabs, flags, st));
  SmallRArgs a = {};
  a.no_t18n = opt_no_t18n();
  a.tables = tabs;
  fill_chain(a, P, S);
  a.seg_out = (cplx*)sv;
  g_last_kernel = C3P_KERNEL_SMALLD;
  if (record_start(w, st)) return -1;
  LAUNCH_TRY(c3p_launch_smallr_chain(a, st));
  if (record_stop(w, st)) return -1;
  if (Dm > 12) {
    g_last_kernel = C3P_KERNEL_MFMA;
    return combine_chain(c3p_launch_midd_chain, w, (const cplx*)sv, B, S, Dm, 0, P.fr_phase, U_out, st) ? -1 : 0;
  }
  return combine_chain(c3p_launch_smalld_chain, w, (const cplx*)sv, B, S, Dm, 0, P.fr_phase, U_out, st) ? -1 : 0;
}

int run_pwc_smalld(DeviceWs* w, const PwcProblem& P, cplx* U_out, cplx* dUs_out, hipStream_t st) {
  const int B = P.B, K = P.K, N = P.N, Dm = P.Dm;
  const double* fr_phase = P.fr_phase;
  const int S = pick_segments(B, N, K, Dm, P.per_sample());
  if (S < 0) return 1;  // not applicable -> caller falls back to the generic kernel
  const int nsamp = P.nsamp();
  const bool fuse = (S > 1) && (S % 4 == 0) && !c3p_opt_on(C3P_OPT_no_fuse);
  const bool inline_tables = !P.lindblad && !c3p_opt_on(C3P_OPT_prep_kernel);
  int* counters = nullptr;
  if (fuse) {
    void* cv;
    if (ws_get(w, SL_COUNTERS, (size_t)B * sizeof(int), &cv)) return -1;
    counters = (int*)cv;
  }
  SmallArgs a = {};
  a.no_t18n = opt_no_t18n();
  if (inline_tables) {
    // unitary mode: the chain kernel builds its tables itself (no dependent launch in front of it)
    a.inline_tables = 1;
    if (!dUs_out) a.record = P.record;  // (the kernels that keep the slice propagators build inline)
    a.h0 = P.h0;
    a.h0_bstride = P.h0_bs;
    a.hks = P.hks;
    a.hks_bstride = P.hk_bs;
    a.dt = P.dt;
  } else {
    void* v;
    if (ws_get(w, SL_TABLES, (size_t)nsamp * c3p_smalld_table_doubles(Dm, K) * sizeof(double), &v)) return -1;
    PrepArgs p = prep_args(P);
    p.tables = (double*)v;
    LAUNCH_TRY(c3p_launch_smalld_prep(p, Dm, nsamp, st));
    a.tables = (const double*)v;
  }
  fill_chain(a, P, S);
  a.mode = P.lindblad ? C3P_MODE_LINDBLAD : C3P_MODE_UNITARY;
  a.dUs_out = dUs_out;
  if (S == 1) {
    a.seg_out = U_out;
    a.fr_phase = fr_phase;
  } else {
    void* sv;
    if (ws_get(w, SL_SEG_A, (size_t)B * S * Dm * Dm * sizeof(cplx), &sv)) return -1;
    a.seg_out = (cplx*)sv;
    if (fuse) {
      a.fuse = 1;
      a.counters = counters;
      a.final_out = U_out;
      a.fr_phase = fr_phase;
    }
  }
  g_last_kernel = C3P_KERNEL_SMALLD;
  if (record_start(w, st)) return -1;
  LAUNCH_TRY(c3p_launch_smalld_chain(a, st));
  if (record_stop(w, st)) return -1;
  if (S > 1 && !fuse) return combine_chain(c3p_launch_smalld_chain, w, a.seg_out, B, S, Dm, 0, fr_phase, U_out, st);
  return 0;
}

// Gradient on the mid-D MFMA kernels (13 <= D <= 40): tables, forward segment products (chain kernel, no
// combine), the per-sample scan of c3p_grad.hip, then the pair-T18 backward sweep.  1 = not applicable.
int run_vjp_midd(DeviceWs* w, GradArgs& G, hipStream_t st) {
  const int D = G.D, B = G.B, K = G.K, N = G.N;
  int nig, nj, wd;
  if (!c3p_midd_geometry(D, &nig, &nj, &wd) || K > 16) return 1;
  const size_t img_bytes = (size_t)16 * nig * wd * sizeof(double);
  // backward sweep: one workgroup per CU (two for the real-Hamiltonian kernel at D <= 32); two to four rounds
  long target = D <= 32 ? 2048 : 512;  // (D <= 32: four rounds of the two-per-CU sweep; 1024 -> 2048 measured -2 % at cfg3)
  if (c3p_opt(C3P_OPT_grad_target) > 0) target = c3p_opt(C3P_OPT_grad_target);  // tuning override
  long S = (target + B - 1) / B;
  const long smax = N / 8 > 1 ? N / 8 : 1;
  if (S > smax) S = smax;
  if (S < 1) S = 1;
  (void)img_bytes;
  auto lds_need = [&](long s) { return c3p_midd_grad_image_bytes(D) + (size_t)K * ((N + s - 1) / s) * sizeof(double); };
  while (lds_need(S) > (size_t)150 * 1024 && S < N) ++S;
  if (lds_need(S) > (size_t)150 * 1024) return 1;
  const bool per_sample = (G.h0_bstride != 0) || (G.hks_bstride != 0);
  const int nsamp = per_sample ? B : 1;
  void* v;
  if (ws_get(w, SL_TABLES, (size_t)nsamp * c3p_midd_table_doubles(D, K) * sizeof(double), &v)) return -1;
  MidPrepArgs p = {};
  p.h0 = G.h0;
  p.h0_bstride = G.h0_bstride;
  p.hks = G.hks;
  p.hks_bstride = G.hks_bstride;
  p.dt = G.dt;
  p.K = K;
  p.Dh = D;
  p.Dm = D;
  p.rows = 16 * nig;
  p.W = wd;
  p.tables = (double*)v;
  LAUNCH_TRY(c3p_launch_midd_prep(p, nsamp, st));
  const size_t segb = (size_t)B * S * D * D * sizeof(cplx);
  void *sv, *mv;
  if (ws_get(w, SL_SEG_A, segb, &sv)) return -1;
  if (ws_get(w, SL_SEG_B, segb, &mv)) return -1;
  MidArgs a = {};
  a.tables = p.tables;
  a.tab_per_sample = per_sample ? 1 : 0;
  a.signals = G.signals;
  a.B = B;
  a.K = K;
  a.N = N;
  a.Dm = D;
  a.S = (int)S;
  a.Lmax = (int)((N + S - 1) / S);
  a.mode = C3P_MODE_UNITARY;
  a.seg_out = (cplx*)sv;
  LAUNCH_TRY(c3p_launch_midd_chain(a, st));
  G.S = (int)S;
  G.seg = (cplx*)sv;
  G.Mb = (cplx*)mv;
  const bool scan_global = c3p_grad_lds_bytes(D) > 150 * 1024;
  if (scan_global) {
    // the scan keeps four matrices per sample: one small scratch region per workgroup
    G.scratch_stride = ((long)4 * G.ld * D + G.S - 1) / G.S;
    void* gv;
    if (ws_get(w, SL_SCRATCH, (size_t)B * G.S * G.scratch_stride * sizeof(cplx), &gv)) return -1;
    G.scratch = (cplx*)gv;
  }
  LAUNCH_TRY(c3p_launch_grad_scan(G, scan_global, st));
  MidGradArgs g = {};
  g.tables = p.tables;
  g.tab_per_sample = a.tab_per_sample;
  g.signals = G.signals;
  g.Mb = G.Mb;
  g.grad = G.grad;
  g.zout = G.zout;
  g.B = B;
  g.K = K;
  g.N = N;
  g.Dm = D;
  g.S = (int)S;
  g.Lmax = a.Lmax;
  LAUNCH_TRY(c3p_launch_midd_grad(g, st));
  return 0;
}

// Time segments per sample for the workgroup-per-chain kernels.  B S chains run in ceil(B S / slots) rounds of
// `slots` resident workgroups, each N / S slices long (+ a few slices' worth of prologue): take the S that
// minimises rounds x segment length, so that the last round is not a mostly idle tail.
static long pick_segments_rounds(long B, long N, long slots, long smax, long min_len = 100) {
  if (c3p_opt(C3P_OPT_segments) > 0) {  // tuning override
    const long S = c3p_opt(C3P_OPT_segments);
    if (S >= 1 && S <= (N > 1 ? N : 1)) return S;
  }
  long best = 1;
  double best_cost = 1e300;
  if (smax > 96) smax = 96;
  for (long S = 1; S <= smax; ++S) {
    const long rounds = (B * S + slots - 1) / slots;
    const double cost = (double)rounds * (double)((N + S - 1) / S + 4);
    if (cost < best_cost * (1.0 - 1e-9)) {
      best_cost = cost;
      best = S;
    }
  }
  // The workgroups that share a SIMD do not advance at the same rate (the arbiter serves the older wave first), so a
  // round does not end for all of them at once: with MANY more workgroups than slots the SIMDs stay shared until the
  // very end, with one or two rounds the last workgroup of every CU runs a good part of its segment alone.  Measured
  // (cfg5, B = 1024): S = 1 (2 rounds) 6.13e3, S = 4 6.28e3, S = 12 6.33e3 propagators/s; cfg3 (B = 512): 3 -> 12 segments
  // +1 %.  At least 12 rounds, segments of at least min_len slices (100; 400 in the 16-row class, whose slices are short
  // against the per-segment prologue: D = 13 measured 20 % slower with 100).
  if (!c3p_opt_on(C3P_OPT_no_many_rounds)) {
    long want = (12 * slots + B - 1) / B;
    const long cap = N / min_len > 1 ? N / min_len : 1;
    if (want > cap) want = cap;
    if (want > smax) want = smax;
    if (want > best) best = want;
  }
  return best;
}

// Supplied generators on the mid-D MFMA kernel (13 <= D <= 40); see run_xg_smalld.
int run_xg_midd(DeviceWs* w, const cplx* hs, long hs_bstride, double coef_r, double coef_i, int B, int N, int D,
                const double* fr_phase, cplx* U_out, cplx* dUs_out, hipStream_t st) {
  int nig, nj, wd;
  if (!c3p_midd_geometry(D, &nig, &nj, &wd)) return 1;
  const size_t lds0 = c3p_midd_lds_bytes(D, 0, 0);
  int wg_per_cu = (int)((156 * 1024) / (lds0 + 4096));
  if (wg_per_cu > 3) wg_per_cu = 3;
  if (wg_per_cu < 1) wg_per_cu = 1;
  const long smax = N / 8 > 1 ? N / 8 : 1;
  const long S = pick_segments_rounds(B, N, 256L * wg_per_cu, smax, D <= 16 ? 400 : 100);
  void* mv;
  if (ws_get(w, SL_TABLES, (size_t)B * N * 4 * sizeof(double), &mv)) return -1;
  LAUNCH_TRY(c3p_launch_hmeta(hs, hs_bstride, (long)B * N, N, D, coef_r, coef_i, (double*)mv, st));
  MidArgs a = {};
  fill_supplied(a, Supplied{hs, hs_bstride, (const double*)mv, coef_r, coef_i, B, N, D}, S);
  a.mode = C3P_MODE_EXPM;
  a.dUs_out = dUs_out;
  a.no_t18 = c3p_opt_on(C3P_OPT_no_t18) ? 1 : 0;
  a.no_t18n = opt_no_t18n();
  a.no_real = c3p_opt_on(C3P_OPT_no_real) ? 1 : 0;
  if (S == 1) {
    a.seg_out = U_out;
    a.fr_phase = fr_phase;
  } else {
    void* sv;
    if (ws_get(w, SL_SEG_A, (size_t)B * S * D * D * sizeof(cplx), &sv)) return -1;
    a.seg_out = (cplx*)sv;
  }
  g_last_kernel = C3P_KERNEL_MFMA;
  if (record_start(w, st)) return -1;
  LAUNCH_TRY(c3p_launch_midd_chain(a, st));
  if (record_stop(w, st)) return -1;
  if (S > 1) return combine_chain(c3p_launch_midd_chain, w, a.seg_out, B, (int)S, D, 0, fr_phase, U_out, st);
  return 0;
}

// Supplied generators (branch B of pwc: per-slice Hamiltonians, and c3p_expm) on the small-D MFMA kernel:
// X_n = coef * hs[b,n]; the hmeta pre-pass supplies the trace shift and the norm of every matrix.
int run_xg_smalld(DeviceWs* w, const cplx* hs, long hs_bstride, double coef_r, double coef_i, int B, int N, int D,
                  const double* fr_phase, cplx* U_out, cplx* dUs_out, hipStream_t st) {
  const int S = pick_segments(B, N, 0, D, false);
  if (S < 0) return 1;
  void* mv;
  if (ws_get(w, SL_TABLES, (size_t)B * N * 4 * sizeof(double), &mv)) return -1;
  LAUNCH_TRY(c3p_launch_hmeta(hs, hs_bstride, (long)B * N, N, D, coef_r, coef_i, (double*)mv, st));
  SmallArgs a = {};
  a.no_t18n = opt_no_t18n();
  fill_supplied(a, Supplied{hs, hs_bstride, (const double*)mv, coef_r, coef_i, B, N, D}, S);
  a.mode = C3P_MODE_EXPM;
  a.dUs_out = dUs_out;
  const bool fuse = (S > 1) && (S % 4 == 0) && !c3p_opt_on(C3P_OPT_no_fuse);
  if (S == 1) {
    a.seg_out = U_out;
    a.fr_phase = fr_phase;
  } else {
    void* sv;
    if (ws_get(w, SL_SEG_A, (size_t)B * S * D * D * sizeof(cplx), &sv)) return -1;
    a.seg_out = (cplx*)sv;
    if (fuse) {
      void* cv;
      if (ws_get(w, SL_COUNTERS, (size_t)B * sizeof(int), &cv)) return -1;
      a.fuse = 1;
      a.counters = (int*)cv;
      a.final_out = U_out;
      a.fr_phase = fr_phase;
    }
  }
  g_last_kernel = C3P_KERNEL_SMALLD;
  if (record_start(w, st)) return -1;
  LAUNCH_TRY(c3p_launch_smalld_chain(a, st));
  if (record_stop(w, st)) return -1;
  if (S > 1 && !fuse) return combine_chain(c3p_launch_smalld_chain, w, a.seg_out, B, S, D, 0, fr_phase, U_out, st);
  return 0;
}

// Gradient on the small-D MFMA kernels: forward segment products (unfused smalld chain kernel), the
// per-sample scan of c3p_grad.hip, then the pair-T18 backward sweep.  Returns 1 when not applicable.
int run_vjp_smalld(DeviceWs* w, GradArgs& G, hipStream_t st) {
  const int D = G.D, B = G.B, K = G.K, N = G.N;
  const bool per_sample = (G.h0_bstride != 0) || (G.hks_bstride != 0);
  const int S = pick_segments(B, N, K, D, per_sample, c3p_opt(C3P_OPT_grad_slots) > 0 ? c3p_opt(C3P_OPT_grad_slots) : 4096);
  if (S < 0) return 1;
  const int nsamp = per_sample ? B : 1;
  void* v;
  if (ws_get(w, SL_TABLES, (size_t)nsamp * c3p_smalld_table_doubles(D, K) * sizeof(double), &v)) return -1;
  PrepArgs p = {};
  p.h0 = G.h0;
  p.h0_bstride = G.h0_bstride;
  p.hks = G.hks;
  p.hks_bstride = G.hks_bstride;
  p.dt = G.dt;
  p.K = K;
  p.Dh = D;
  p.tables = (double*)v;
  LAUNCH_TRY(c3p_launch_smalld_prep(p, D, nsamp, st));
  const size_t segb = (size_t)B * S * D * D * sizeof(cplx);
  void *sv, *mv;
  if (ws_get(w, SL_SEG_A, segb, &sv)) return -1;
  if (ws_get(w, SL_SEG_B, segb, &mv)) return -1;
  // The backward sweep runs one wave per SIMD (S is chosen for its 4096 chain slots), the forward chain kernel two: the
  // segment products are formed on 2 S segments (twice the waves: 0.24 -> 0.15 ms at cfg2) and multiplied in pairs by one
  // launch of the chain kernel's supplied-matrix mode (grad_fwd_seg2 = 0: one pass on S segments)
  int Sf = S;
  void* fv = sv;
  if (c3p_opt(C3P_OPT_grad_fwd_seg2) != 0 && (long)B * S <= 4096 && 2L * S <= N / 8) {
    Sf = 2 * S;
    if (ws_get(w, SL_SEG_F, 2 * segb, &fv)) return -1;
  }
  SmallArgs a = {};
  a.no_t18n = opt_no_t18n();
  a.tables = p.tables;
  a.tab_per_sample = per_sample ? 1 : 0;
  a.signals = G.signals;
  a.B = B;
  a.K = K;
  a.N = N;
  a.Dm = D;
  a.S = Sf;
  a.Lmax = (N + Sf - 1) / Sf;
  a.mode = C3P_MODE_UNITARY;
  a.seg_out = (cplx*)fv;
  LAUNCH_TRY(c3p_launch_smalld_chain(a, st));
  if (Sf != S) {
    SmallArgs c = {};
    c.mode = C3P_MODE_GIVEN;
    c.mats = (const cplx*)fv;
    c.B = B * S;
    c.N = 2;
    c.Dm = D;
    c.S = 1;
    c.Lmax = 2;
    c.seg_out = (cplx*)sv;
    LAUNCH_TRY(c3p_launch_smalld_chain(c, st));
  }
  a.S = S;
  a.Lmax = (N + S - 1) / S;
  G.S = S;
  G.seg = (cplx*)sv;
  G.Mb = (cplx*)mv;
  LAUNCH_TRY(c3p_launch_grad_scan(G, false, st));
  SmallGradArgs g = {};
  g.tables = p.tables;
  g.tab_per_sample = a.tab_per_sample;
  g.signals = G.signals;
  g.Mb = G.Mb;
  g.grad = G.grad;
  g.zout = G.zout;
  g.B = B;
  g.K = K;
  g.N = N;
  g.Dm = D;
  g.S = S;
  g.Lmax = a.Lmax;
  LAUNCH_TRY(c3p_launch_smalld_grad(g, st));
  return 0;
}

// ---- the general-generator sweep: forward chain kernel (segment products + slice propagators), general scan of c3p_grad.hip
// (prefix at the start, left adjoint at the end of every segment), backward sweep kernel.  What its four users share: ----
// the store between the kernels, one block of Dm x Dm matrices: pre [B,S] | dUs [B,N] (with_dus: the forward chain of this call
// writes the slice propagators here; a taped sweep reads them from the tape) | pstore [B,N]
struct SweepStore {
  cplx *pre, *dUs, *pstore;
};
int get_sweep_store(DeviceWs* w, Slot slot, int B, long S, int N, int Dm, bool with_dus, SweepStore* s) {
  const size_t msz = (size_t)Dm * Dm;
  void* v;
  if (ws_get(w, slot, ((size_t)B * S + (with_dus ? 2 : 1) * (size_t)B * N) * msz * sizeof(cplx), &v)) return -1;
  s->pre = (cplx*)v;
  s->dUs = with_dus ? s->pre + (size_t)B * S * msz : nullptr;
  s->pstore = s->pre + ((size_t)B * S + (with_dus ? (size_t)B * N : 0)) * msz;
  return 0;
}
// the scan's record: segment products in, left adjoints (Mb) and prefixes (pre) out
void fill_general_scan(GradArgs& G, int B, int K, int N, int Dm, long S, cplx* seg, cplx* Mb, cplx* pre, const cplx* Ubar,
                       const double* fr_phase) {
  G.Ubar = Ubar;
  G.fr_phase = fr_phase;
  G.B = B;
  G.K = K;
  G.N = N;
  G.D = Dm;
  G.ld = Dm | 1;
  G.S = (int)S;
  G.seg = seg;
  G.Mb = Mb;
  G.pre = pre;
  G.general = 1;
}
int general_scan(int B, int K, int N, int Dm, long S, cplx* seg, cplx* Mb, cplx* pre, const cplx* Ubar, const double* fr_phase,
                 hipStream_t st) {
  GradArgs G = {};
  fill_general_scan(G, B, K, N, Dm, S, seg, Mb, pre, Ubar, fr_phase);
  LAUNCH_TRY(c3p_launch_grad_scan_general(G, false, st));
  return 0;
}
// segments of the mid-D general sweep (one workgroup per CU: two to four rounds), before the LDS rule of the caller
long midd_grad_segments(int B, int N, int Dm) {
  long S = ((Dm <= 32 ? 1024 : 512) + B - 1) / B;
  const long smax = N / 8 > 1 ? N / 8 : 1;
  if (S > smax) S = smax;
  return S < 1 ? 1 : S;
}

// Lindblad gradient on the small-D MFMA kernels (superoperators up to 12 x 12, D <= 3), general-generator form: slice
// propagators + segment products from the forward chain kernel, the general scan of c3p_grad.hip (prefix at the start, left
// adjoint at the end of every segment), then smalld_grad_general_kernel.  In two halves around a block of memory that holds
// what the forward half leaves for the backward one -- the workspace (c3p_pwc_lindblad_vjp) or a caller-owned tape
// (c3p_pwc_lindblad_taped / _vjp_taped: the forward half also serves U, one chain pass per evaluation instead of two).
struct LindSmallSizes {
  size_t tabs, seg, dus;  // bytes: both table sets, segment products [B,S,Dm,Dm], slice propagators [B,N,Dm,Dm]
  size_t total() const { return tabs + seg + dus; }
};
LindSmallSizes lind_small_sizes(int B, int K, int N, int Dm, int S, int nsamp) {
  const size_t msz = (size_t)Dm * Dm * sizeof(cplx);
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  LindSmallSizes z;
  z.tabs = up(2 * (size_t)nsamp * c3p_smalld_table_doubles(Dm, K) * sizeof(double));
  z.seg = up((size_t)B * S * msz);
  z.dus = up((size_t)B * N * msz);
  return z;
}
struct LindSmallBufs {
  double* tabs;
  cplx *seg, *dus;
};
LindSmallBufs lind_small_carve(void* base, const LindSmallSizes& z) {
  char* p = static_cast<char*>(base);
  LindSmallBufs b;
  b.tabs = reinterpret_cast<double*>(p);
  b.seg = reinterpret_cast<cplx*>(p + z.tabs);
  b.dus = reinterpret_cast<cplx*>(p + z.tabs + z.seg);
  return b;
}
// segments of the small-D Lindblad sweep, -1 when the shape is not served (tables + images beyond the LDS of the backward kernel)
int lind_small_segments(int B, int K, int N, int Dm, bool need_mult4) {
  if (Dm > 12) return -1;
  // (8192 chain slots: the real sweep of c3p_smallr.hip runs two wavefronts per SIMD; for the complex one -- one per SIMD -- two
  // rounds of half-length segments cost what one round did)
  int S = pick_segments(B, N, K, Dm, need_mult4, 8192);
  // (short segments cost more than the cost model of pick_segments knows here: the segment scan is sequential over S and every
  // chain has a prologue -- below 8 slices per segment the 4096-slot choice is the faster one (with the blocked scan of
  // c3p_smallr.hip; 16 before it): B = 64, N = 1000 takes 128 segments of 8, 0.286 -> 0.259 ms per gradient call)
  if (S > 0 && N / S < 8) S = pick_segments(B, N, K, Dm, need_mult4, 4096);
  if (S < 0) return -1;
  // (the backward kernel keeps BOTH table sets in LDS)
  if ((2 * c3p_smalld_table_doubles(Dm, K) + 8 * (size_t)c3p_smalld_mat_doubles(Dm) + 4 * (size_t)K * ((N + S - 1) / S)) * sizeof(double) > 60 * 1024)
    return -1;
  return S;
}
int lind_small_forward(DeviceWs* w, const LindSmallBufs& bf, const PwcProblem& P, int S, bool hermitian, hipStream_t st) {
  const int K = P.K, N = P.N, D = P.D, Dm = P.Dm;
  const int nsamp = P.nsamp();
  const size_t tdoubles = (size_t)nsamp * c3p_smalld_table_doubles(Dm, K);
  PrepArgs p = prep_args(P);
  p.tables = bf.tabs;
  LAUNCH_TRY(c3p_launch_smalld_prep(p, Dm, nsamp, st));
  p.conjT = 1;
  p.tables = bf.tabs + tdoubles;
  LAUNCH_TRY(c3p_launch_smalld_prep(p, Dm, nsamp, st));
  if (hermitian && c3p_smallr_supported(D, Dm, K) && !c3p_opt_on(C3P_OPT_no_smallr) &&
      c3p_smallr_lds_bytes(Dm, K, (N + S - 1) / S) <= (size_t)60 * 1024) {
    // declared Hermitian Hamiltonians (C3P_HERMITIAN_H): segment products and slice propagators from the real kernels of
    // c3p_smallr.hip (the backward sweep reads them in the complex vectorisation: the kernel converts what it stores)
    const size_t rdoubles = (size_t)nsamp * c3p_smallr_table_doubles(Dm, K);
    const size_t fl_off = (rdoubles * sizeof(double) + 255) & ~(size_t)255;
    void* tv;
    if (ws_get(w, SL_TABLES, fl_off + (size_t)nsamp * (1 + K) * sizeof(int), &tv)) return -1;
    LAUNCH_TRY(c3p_launch_smallr_prep(regd_prep_args(P), nsamp, (double*)tv, reinterpret_cast<int*>(static_cast<char*>(tv) + fl_off), st));
    SmallRArgs ra = {};
    ra.no_t18n = opt_no_t18n();
    ra.tables = (const double*)tv;
    fill_chain(ra, P, S);
    ra.seg_out = bf.seg;
    ra.dUs_out = bf.dus;
    LAUNCH_TRY(c3p_launch_smallr_chain(ra, st));
    return 0;
  }
  SmallArgs a = {};
  a.no_t18n = opt_no_t18n();
  a.tables = bf.tabs;
  fill_chain(a, P, S);
  a.mode = C3P_MODE_LINDBLAD;
  a.seg_out = bf.seg;
  a.dUs_out = bf.dus;
  LAUNCH_TRY(c3p_launch_smalld_chain(a, st));
  return 0;
}
// (the backward halves read the sizes, the signals, the frame phases and per_sample() of the record: the operators are in the tables)
int lind_small_backward(DeviceWs* w, const LindSmallBufs& bf, const PwcProblem& P, int S, const cplx* Ubar, double* grad, hipStream_t st) {
  const int B = P.B, K = P.K, N = P.N, Dm = P.Dm;
  const int nsamp = P.nsamp();
  const size_t tdoubles = (size_t)nsamp * c3p_smalld_table_doubles(Dm, K);
  void* mv;
  SweepStore ss;
  if (ws_get(w, SL_SEG_B, (size_t)B * S * Dm * Dm * sizeof(cplx), &mv)) return -1;
  if (get_sweep_store(w, SL_SEG_A, B, S, N, Dm, false, &ss)) return -1;  // (SL_OUT0 stages grad_signals, SL_OUT1 is the untaped block)
  if (general_scan(B, K, N, Dm, S, bf.seg, (cplx*)mv, ss.pre, Ubar, P.fr_phase, st)) return -1;
  SmallGradArgs g = {};
  g.tables = bf.tabs;
  g.tables_h = bf.tabs + tdoubles;
  fill_chain(g, P, S);
  g.Mb = (cplx*)mv;
  g.pre = ss.pre;
  g.dUs = bf.dus;
  g.pstore = ss.pstore;
  g.grad = grad;
  LAUNCH_TRY(c3p_launch_smalld_grad_general(g, st));
  return 0;
}
// The same two halves in REAL arithmetic in the Hermitian basis (declared Hermitian Hamiltonians, C3P_HERMITIAN_H; c3p_smallr.hip):
// real tables of G' and G'^T, real segment products and slice propagators from the forward half; the cotangent in the basis
// (hb_ubar), the real segment scan and the real pair-evaluation sweep in the backward half.  The block is laid out inside
// the memory the complex halves would use (it is smaller in every part).
LindSmallSizes lind_smallr_sizes(int B, int K, int N, int Dm, int S, int nsamp) {  // tables with their flags, real segment products and slice propagators
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  LindSmallSizes z;
  z.tabs = up(2 * (size_t)nsamp * c3p_smallr_table_doubles(Dm, K) * sizeof(double)) + up((size_t)nsamp * (1 + K) * sizeof(int));
  z.seg = up((size_t)B * S * Dm * Dm * sizeof(double));
  z.dus = up((size_t)B * N * Dm * Dm * sizeof(double));
  return z;
}
struct LindSmallRBufs {
  double *tabs, *tabs_t;
  int* flags;
  double *seg, *dus;
};
LindSmallRBufs lind_smallr_carve(void* base, const LindSmallSizes& z, int nsamp, int Dm, int K) {
  char* p = static_cast<char*>(base);
  const size_t td = (size_t)nsamp * c3p_smallr_table_doubles(Dm, K);
  LindSmallRBufs b;
  b.tabs = reinterpret_cast<double*>(p);
  b.tabs_t = b.tabs + td;
  b.flags = reinterpret_cast<int*>(p + ((2 * td * sizeof(double) + 255) & ~(size_t)255));
  b.seg = reinterpret_cast<double*>(p + z.tabs);
  b.dus = reinterpret_cast<double*>(p + z.tabs + z.seg);
  return b;
}
bool lind_smallr_ok(bool hermitian, int D, int Dm, int K, int N, int S) {
  return hermitian && c3p_smallr_supported(D, Dm, K) && !c3p_opt_on(C3P_OPT_no_smallr) &&
         c3p_smallr_lds_bytes(Dm, K, (N + S - 1) / S) <= (size_t)60 * 1024 && c3p_smallr_grad_lds_bytes(Dm, K, (N + S - 1) / S) <= (size_t)60 * 1024;
}
// forward half; seg_complex (workspace, [B,S,Dm,Dm]) receives the segment products in the reference's vectorisation for U.
// Not one function with the Hermitian sub-branch of lind_small_forward, alike as they look: that one builds ONE real table set in
// SL_TABLES (c3p_launch_smallr_prep, a workspace request) beside the two complex sets and stores complex matrices for the complex
// sweep; this one builds the table PAIR in the tape (c3p_launch_smallr_prep_pair, no request) and stores real ones.  Merged, one
// of the two would change its launch log or its workspace requests.
int lind_smallr_forward(const LindSmallRBufs& bf, const PwcProblem& P, int S, cplx* seg_complex, hipStream_t st) {
  LAUNCH_TRY(c3p_launch_smallr_prep_pair(regd_prep_args(P), P.nsamp(), bf.tabs, bf.tabs_t, bf.flags, st));
  SmallRArgs ra = {};
  ra.no_t18n = opt_no_t18n();
  ra.tables = bf.tabs;
  fill_chain(ra, P, S);
  ra.seg_out = seg_complex;
  ra.seg_real = bf.seg;
  ra.dus_real = bf.dus;
  LAUNCH_TRY(c3p_launch_smallr_chain(ra, st));
  return 0;
}
int lind_smallr_backward(DeviceWs* w, const LindSmallRBufs& bf, const PwcProblem& P, int S, const cplx* Ubar, double* grad, hipStream_t st) {
  const int B = P.B, Dm = P.Dm;
  const size_t m8 = (size_t)Dm * Dm * sizeof(double);
  void *uv, *pv, *sv;
  if (ws_get(w, SL_SCRATCH, (size_t)B * m8, &uv)) return -1;
  if (ws_get(w, SL_SEG_A, (size_t)B * S * m8, &pv)) return -1;
  if (ws_get(w, SL_SEG_B, (size_t)B * S * m8, &sv)) return -1;
  LAUNCH_TRY(c3p_launch_hb_ubar(Ubar, P.fr_phase, B, P.D, (double*)uv, st));
  LAUNCH_TRY(c3p_launch_smallr_scan(bf.seg, (const double*)uv, B, S, Dm, (double*)pv, (double*)sv, st));
  SmallRGradArgs g = {};
  g.no_t18n = opt_no_t18n();
  g.tables = bf.tabs;
  g.tables_t = bf.tabs_t;
  fill_chain(g, P, S);
  g.pre = (const double*)pv;
  g.suf = (const double*)sv;
  g.dus = bf.dus;
  g.grad = grad;
  LAUNCH_TRY(c3p_launch_smallr_grad(g, st));
  return 0;
}

// Both halves on the real kernels (declared Hermitian Hamiltonians) on S segments, around `block_bytes` of SL_OUT1: the block of
// the real layout at 16 x 16, the larger block of the complex halves at D <= 3 (one request per shape, Hermitian or not).
int run_vjp_lind_real(DeviceWs* w, const PwcProblem& P, int S, size_t block_bytes, const cplx* Ubar, double* grad, hipStream_t st) {
  const int B = P.B, K = P.K, N = P.N, Dm = P.Dm;
  const int nsamp = P.nsamp();
  void *blk, *sc;
  if (ws_get(w, SL_OUT1, block_bytes, &blk)) return -1;
  if (ws_get(w, SL_OUT2, (size_t)B * S * Dm * Dm * sizeof(cplx), &sc)) return -1;  // (the complex segment products: not needed here)
  const LindSmallRBufs rb = lind_smallr_carve(blk, lind_smallr_sizes(B, K, N, Dm, S, nsamp), nsamp, Dm, K);
  if (lind_smallr_forward(rb, P, S, (cplx*)sc, st)) return -1;
  return lind_smallr_backward(w, rb, P, S, Ubar, grad, st) ? -1 : 0;
}
// two qubits (16 x 16 superoperators), declared Hermitian; 1 = not applicable
int run_vjp_lind_smallr16(DeviceWs* w, const PwcProblem& P, const cplx* Ubar, double* grad, hipStream_t st) {
  const int S = pick_segments_r(P.B, P.N, P.K, P.Dm, P.per_sample(), true);
  if (S < 0 || !lind_smallr_ok(true, P.D, P.Dm, P.K, P.N, S)) return 1;
  return run_vjp_lind_real(w, P, S, lind_smallr_sizes(P.B, P.K, P.N, P.Dm, S, P.nsamp()).total(), Ubar, grad, st);
}

// Returns 1 when not applicable.
int run_vjp_lind_smalld(DeviceWs* w, const PwcProblem& P, const cplx* Ubar, double* grad, bool hermitian, hipStream_t st) {
  const int B = P.B, K = P.K, N = P.N, D = P.D, Dm = P.Dm;
  const int S = lind_small_segments(B, K, N, Dm, P.per_sample());
  if (S < 0) return 1;
  const LindSmallSizes z = lind_small_sizes(B, K, N, Dm, S, P.nsamp());
  if (lind_smallr_ok(hermitian, D, Dm, K, N, S)) return run_vjp_lind_real(w, P, S, z.total(), Ubar, grad, st);
  void* blk;
  if (ws_get(w, SL_OUT1, z.total(), &blk)) return -1;
  const LindSmallBufs bf = lind_small_carve(blk, z);
  if (lind_small_forward(w, bf, P, S, hermitian, st)) return -1;
  return lind_small_backward(w, bf, P, S, Ubar, grad, st) ? -1 : 0;
}

// ---------------------------------------------------------------------------
// Mid-D MFMA path (13 <= Dm <= 40): one 4-wave workgroup per chain, matrices as LDS images
// ---------------------------------------------------------------------------
int run_pwc_midd(DeviceWs* w, const PwcProblem& P, cplx* U_out, cplx* dUs_out, hipStream_t st) {
  const int B = P.B, K = P.K, N = P.N, Dm = P.Dm;
  int nig, nj, wd;
  if (!c3p_midd_geometry(Dm, &nig, &nj, &wd)) return 1;
  // workgroups resident at once are LDS-limited (three images per workgroup); aim at two rounds
  const size_t lds0 = c3p_midd_lds_bytes(Dm, K, 0);
  int wg_per_cu = (int)((156 * 1024) / (lds0 + 4096));
  if (wg_per_cu > 3) wg_per_cu = 3;
  if (wg_per_cu < 1) wg_per_cu = 1;
  const long smax = N / 8 > 1 ? N / 8 : 1;
  const long S = pick_segments_rounds(B, N, 256L * wg_per_cu, smax, Dm <= 16 ? 400 : 100);
  if (lds0 > 158 * 1024) return 1;
  const int nsamp = P.nsamp();
  void* v;
  if (ws_get(w, SL_TABLES, (size_t)nsamp * c3p_midd_table_doubles(Dm, K) * sizeof(double), &v)) return -1;
  MidPrepArgs p = mid_prep_args(P, nig, wd);
  p.tables = (double*)v;
  LAUNCH_TRY(c3p_launch_midd_prep(p, nsamp, st));
  MidArgs a = {};
  a.tables = (const double*)v;
  fill_chain(a, P, S);
  a.mode = P.lindblad ? C3P_MODE_LINDBLAD : C3P_MODE_UNITARY;
  a.dUs_out = dUs_out;
  a.no_t18 = c3p_opt_on(C3P_OPT_no_t18) ? 1 : 0;
  a.no_t18n = opt_no_t18n();
  a.no_real = c3p_opt_on(C3P_OPT_no_real) ? 1 : 0;
  if (S == 1) {
    a.seg_out = U_out;
    a.fr_phase = P.fr_phase;
  } else {
    void* sv;
    if (ws_get(w, SL_SEG_A, (size_t)B * S * Dm * Dm * sizeof(cplx), &sv)) return -1;
    a.seg_out = (cplx*)sv;
  }
  g_last_kernel = C3P_KERNEL_MFMA;
  if (record_start(w, st)) return -1;
  LAUNCH_TRY(c3p_launch_midd_chain(a, st));
  if (record_stop(w, st)) return -1;
  if (S > 1) return combine_chain(c3p_launch_midd_chain, w, a.seg_out, B, (int)S, Dm, 0, P.fr_phase, U_out, st);
  return 0;
}

// Lindblad gradient on the mid-D MFMA kernels (16 x 16, 25 x 25, 36 x 36 superoperators: D = 4, 5, 6), general-generator
// form; see run_vjp_lind_smalld.  Returns 1 when not applicable.
int run_vjp_lind_midd(DeviceWs* w, const PwcProblem& P, const cplx* Ubar, double* grad, hipStream_t st) {
  const int B = P.B, K = P.K, N = P.N, Dm = P.Dm;
  int nig, nj, wd;
  if (!c3p_midd_geometry(Dm, &nig, &nj, &wd) || K > 16) return 1;
  if (!((nig == 2 && nj == 4) || (nig == 4 && nj == 7) || (nig == 5 && nj == 9))) return 1;
  long S = midd_grad_segments(B, N, Dm);
  auto lds_need = [&](long s) { return c3p_midd_grad_image_bytes(Dm) + (size_t)K * ((N + s - 1) / s) * sizeof(double); };
  while (lds_need(S) > (size_t)150 * 1024 && S < N) ++S;
  if (lds_need(S) > (size_t)150 * 1024) return 1;
  const int nsamp = P.nsamp();
  const size_t tdoubles = (size_t)nsamp * c3p_midd_table_doubles(Dm, K);
  void* v;
  if (ws_get(w, SL_TABLES, 2 * tdoubles * sizeof(double), &v)) return -1;
  double* tabs = (double*)v;
  MidPrepArgs p = mid_prep_args(P, nig, wd);
  p.tables = tabs;
  LAUNCH_TRY(c3p_launch_midd_prep(p, nsamp, st));
  p.conjT = 1;
  p.tables = tabs + tdoubles;
  LAUNCH_TRY(c3p_launch_midd_prep(p, nsamp, st));
  const size_t msz = (size_t)Dm * Dm * sizeof(cplx);
  void *sv, *mv;
  SweepStore ss;
  if (ws_get(w, SL_SEG_A, (size_t)B * S * msz, &sv)) return -1;
  if (ws_get(w, SL_SEG_B, (size_t)B * S * msz, &mv)) return -1;
  if (get_sweep_store(w, SL_OUT1, B, S, N, Dm, true, &ss)) return -1;  // (SL_OUT0 stages grad_signals)
  MidArgs a = {};
  a.tables = tabs;
  fill_chain(a, P, S);
  a.mode = C3P_MODE_LINDBLAD;
  a.seg_out = (cplx*)sv;
  a.dUs_out = ss.dUs;
  a.no_t18 = c3p_opt_on(C3P_OPT_no_t18) ? 1 : 0;
  a.no_t18n = opt_no_t18n();
  a.no_real = 1;
  LAUNCH_TRY(c3p_launch_midd_chain(a, st));
  if (general_scan(B, K, N, Dm, S, (cplx*)sv, (cplx*)mv, ss.pre, Ubar, P.fr_phase, st)) return -1;
  MidGradArgs g = {};
  g.tables = tabs;
  g.tables_h = tabs + tdoubles;
  fill_chain(g, P, S);
  g.Mb = (cplx*)mv;
  g.pre = ss.pre;
  g.dUs = ss.dUs;
  g.pstore = ss.pstore;
  g.grad = grad;
  LAUNCH_TRY(c3p_launch_midd_grad_general(g, st));
  return 0;
}

// Gradient for supplied per-slice generators X_n = coef hs[b,n] (branch B of pwc: the result is the cotangent of every X_n) on the
// on-chip general-generator sweeps (D <= 40): hmeta pre-pass, forward chain kernel in its supplied-generator mode (segment
// products + slice propagators), general scan, then the small-D / mid-D sweep kernel in its supplied-generator mode.
// Nothing is assumed about the generators.  Returns 1 when not applicable.
template <class Chain, class Grad>
int xg_general_sweep(DeviceWs* w, hipError_t (*chain)(const Chain&, hipStream_t), hipError_t (*sweep)(const Grad&, hipStream_t), Chain a,
                     Supplied X, long S, const double* fr_phase, const cplx* Ubar, cplx* zout, hipStream_t st) {
  const int B = X.B, N = X.N, D = X.Dm;
  void *mv, *sv, *av;
  SweepStore ss;
  if (ws_get(w, SL_TABLES, (size_t)B * N * 4 * sizeof(double), &mv)) return -1;
  const size_t msz = (size_t)D * D * sizeof(cplx);
  if (ws_get(w, SL_SEG_A, (size_t)B * S * msz, &sv)) return -1;
  if (ws_get(w, SL_SEG_B, (size_t)B * S * msz, &av)) return -1;
  if (get_sweep_store(w, SL_OUT1, B, S, N, D, true, &ss)) return -1;  // (SL_OUT0 stages gen_bar_out)
  LAUNCH_TRY(c3p_launch_hmeta(X.hs, X.hs_bstride, (long)B * N, N, D, X.coef_r, X.coef_i, (double*)mv, st));
  X.meta = (const double*)mv;
  fill_supplied(a, X, S);
  a.mode = C3P_MODE_EXPM;
  a.seg_out = (cplx*)sv;
  a.dUs_out = ss.dUs;
  LAUNCH_TRY(chain(a, st));
  if (general_scan(B, 0, N, D, S, (cplx*)sv, (cplx*)av, ss.pre, Ubar, fr_phase, st)) return -1;
  Grad g = {};
  fill_supplied(g, X, S);
  g.Mb = (cplx*)av;
  g.pre = ss.pre;
  g.dUs = ss.dUs;
  g.pstore = ss.pstore;
  g.zout = zout;
  LAUNCH_TRY(sweep(g, st));
  return 0;
}
int run_vjp_xg_general(DeviceWs* w, const cplx* hs, long hs_bstride, double coef_r, double coef_i, int B, int N, int D,
                       const double* fr_phase, const cplx* Ubar, cplx* zout, hipStream_t st) {
  const Supplied X = {hs, hs_bstride, nullptr, coef_r, coef_i, B, N, D};  // (meta: the sweep's hmeta pre-pass)
  if (D <= kSmallDLimit && c3p_smalld_supported(D)) {
    const int S = pick_segments(B, N, 0, D, false, 4096);
    if (S < 0) return 1;
    SmallArgs a = {};
    a.no_t18n = opt_no_t18n();
    return xg_general_sweep(w, c3p_launch_smalld_chain, c3p_launch_smalld_grad_general, a, X, S, fr_phase, Ubar, zout, st);
  }
  int nig = 0, nj = 0, wd = 0;
  if (!c3p_midd_geometry(D, &nig, &nj, &wd)) return 1;
  if (c3p_midd_grad_image_bytes(D) > (size_t)150 * 1024) return 1;
  MidArgs a = {};
  a.no_t18 = c3p_opt_on(C3P_OPT_no_t18) ? 1 : 0;
  a.no_t18n = opt_no_t18n();
  a.no_real = 1;
  return xg_general_sweep(w, c3p_launch_midd_chain, c3p_launch_midd_grad_general, a, X, midd_grad_segments(B, N, D), fr_phase, Ubar, zout, st);
}

// ---------------------------------------------------------------------------
// Big-D MFMA path (81 x 81 Lindblad superoperators): 8-wave workgroup per chain, global arena
// ---------------------------------------------------------------------------
int run_pwc_bigd(DeviceWs* w, const PwcProblem& P, cplx* U_out, cplx* dUs_out, hipStream_t st) {
  const int B = P.B, K = P.K, N = P.N, D = P.D, Dm = P.Dm;
  const double* fr_phase = P.fr_phase;
  int nig, nj, wd;
  if (!c3p_bigd_geometry(Dm, &nig, &nj, &wd)) return 1;
  long S = (C3P_BIGD_MAX_WGS + B - 1) / B;
  const long smax = N / 8 > 1 ? N / 8 : 1;
  if (S > smax) S = smax;
  if (S < 1) S = 1;
  while (c3p_bigd_lds_bytes(Dm, K, (int)((N + S - 1) / S)) > 150 * 1024 && S < N) ++S;
  if (c3p_bigd_lds_bytes(Dm, K, (int)((N + S - 1) / S)) > 150 * 1024) return 1;
  const int nsamp = P.nsamp();
  void* v;
  if (ws_get(w, SL_TABLES, (size_t)nsamp * c3p_bigd_table_doubles(Dm, K) * sizeof(double), &v)) return -1;
  MidPrepArgs p = mid_prep_args(P, nig, wd);
  p.tile_nig = nig;
  p.tile_nj = nj;
  p.tables = (double*)v;
  LAUNCH_TRY(c3p_launch_midd_prep(p, nsamp, st));
  void* av;
  if (ws_get(w, SL_SCRATCH, c3p_bigd_arena_doubles(Dm) * sizeof(double), &av)) return -1;
  MidArgs a = {};
  a.tables = (const double*)v;
  fill_chain(a, P, S);
  a.mode = P.lindblad ? C3P_MODE_LINDBLAD : C3P_MODE_UNITARY;
  a.dUs_out = dUs_out;
  cplx* seg = U_out;
  if (S > 1) {
    void* sv;
    if (ws_get(w, SL_SEG_A, (size_t)B * S * Dm * Dm * sizeof(cplx), &sv)) return -1;
    seg = (cplx*)sv;
  }
  a.seg_out = seg;
  g_last_kernel = C3P_KERNEL_MFMA;
  if (record_start(w, st)) return -1;
  LAUNCH_TRY(c3p_launch_bigd_chain(a, (double*)av, st));
  if (record_stop(w, st)) return -1;
  if (S == 1 && fr_phase) LAUNCH_TRY(c3p_launch_rowphase(U_out, fr_phase, B, Dm, st));
  if (S > 1) {
    // ordered combine of the few segment products with the generic kernel (GIVEN mode)
    ChainArgs c = {};
    c.mode = C3P_MODE_GIVEN;
    c.mats = seg;
    c.B = B;
    c.N = (int)S;
    c.D = D;
    c.Dm = Dm;
    c.fr_phase = fr_phase;
    const int keep = g_last_kernel;
    const int rc = run_chain_generic(w, c, U_out, st, /*profile=*/false);  // the event pair stays on the main kernel
    g_last_kernel = keep;
    if (rc) return -1;
  }
  return 0;
}

// ---------------------------------------------------------------------------
// Register-resident MFMA path (Dm = 49, 65, 81; the 81 x 81 Lindblad superoperators of cfg4): 4-wave workgroup
// per chain, right operands / accumulators in registers, three-real-product complex arithmetic (c3p_regd.hip)
// ---------------------------------------------------------------------------
int run_pwc_regd(DeviceWs* w, const PwcProblem& P, cplx* U_out, cplx* dUs_out, hipStream_t st) {
  const int B = P.B, K = P.K, N = P.N, D = P.D, Dm = P.Dm, lindblad = P.lindblad;
  const double* fr_phase = P.fr_phase;
  if (!c3p_regd_supported(Dm) || K > 16) return 1;
  const bool per_sample = P.per_sample();
  long S = (C3P_REGD_MAX_WGS + B - 1) / B;
  const long smax = N / 8 > 1 ? N / 8 : 1;
  if (S > smax) S = smax;
  if (S < 1) S = 1;
  const int nsamp = P.nsamp();
  // Lindblad superoperators of Hermitian Hamiltonians: the whole chain in real arithmetic in the Hermitian basis
  // (c3p_regr.hip); the complex kernel keeps the samples whose tables are not real there
  const bool hb = lindblad && c3p_regr_supported(D, Dm) && !c3p_opt_on(C3P_OPT_no_hermitian_basis);
  const size_t ctab = (((size_t)nsamp * c3p_regd_table_doubles(Dm, K) * sizeof(double)) + 255) & ~(size_t)255;
  const size_t rtab = hb ? ((((size_t)nsamp * c3p_regr_table_doubles(Dm, K) * sizeof(double)) + 255) & ~(size_t)255) : 0;
  const size_t ftab = hb ? (size_t)nsamp * (1 + K) * sizeof(int) : 0;
  void* v;
  if (ws_get(w, SL_TABLES, ctab + rtab + ftab, &v)) return -1;
  RegdPrepArgs p = regd_prep_args(P);
  p.tables = (double*)v;
  LAUNCH_TRY(c3p_launch_regd_prep(p, nsamp, st));
  double* rtables = reinterpret_cast<double*>(static_cast<char*>(v) + ctab);
  int* tabflag = reinterpret_cast<int*>(static_cast<char*>(v) + ctab + rtab);
  if (hb) LAUNCH_TRY(c3p_launch_regr_prep(p, nsamp, rtables, tabflag, st));
  void* av;
  if (ws_get(w, SL_SCRATCH, std::max(c3p_regd_arena_bytes(Dm), hb ? c3p_regr_arena_bytes(Dm) : (size_t)0), &av)) return -1;
  MidArgs a = {};
  a.tables = (const double*)v;
  fill_chain(a, P, S);
  a.mode = lindblad ? C3P_MODE_LINDBLAD : C3P_MODE_UNITARY;
  a.dUs_out = dUs_out;
  if (hb) {
    a.hb_tables = rtables;
    a.hb_tabflag = tabflag;
  }
  a.no_t18n = opt_no_t18n();
  cplx* seg = U_out;
  if (S > 1) {
    void* sv;
    if (ws_get(w, SL_SEG_A, (size_t)B * S * Dm * Dm * sizeof(cplx), &sv)) return -1;
    seg = (cplx*)sv;
  }
  a.seg_out = seg;
  g_last_kernel = C3P_KERNEL_MFMA;
  if (record_start(w, st)) return -1;
  if (hb) LAUNCH_TRY(c3p_launch_regr_chain(a, av, st));
  LAUNCH_TRY(c3p_launch_regd_chain(a, av, st));
  if (record_stop(w, st)) return -1;
  if (hb) {
    // back to the reference's vectorisation, in place (real results sit in the second half of their complex slots)
    LAUNCH_TRY(c3p_launch_hb_to_complex(seg, (long)B * S, (int)S, tabflag, per_sample ? 1 : 0, K, D, st));
    if (dUs_out) LAUNCH_TRY(c3p_launch_hb_to_complex(dUs_out, (long)B * N, N, tabflag, per_sample ? 1 : 0, K, D, st));
  }
  if (S == 1 && fr_phase) LAUNCH_TRY(c3p_launch_rowphase(U_out, fr_phase, B, Dm, st));
  if (S > 1) {
    // ordered combine of the few segment products with the generic kernel (GIVEN mode)
    ChainArgs c = {};
    c.mode = C3P_MODE_GIVEN;
    c.mats = seg;
    c.B = B;
    c.N = (int)S;
    c.D = D;
    c.Dm = Dm;
    c.fr_phase = fr_phase;
    const int keep = g_last_kernel;
    const int rc = run_chain_generic(w, c, U_out, st, /*profile=*/false);  // the event pair stays on the main kernel
    g_last_kernel = keep;
    if (rc) return -1;
  }
  return 0;
}

// ---------------------------------------------------------------------------
// Tiled large-matrix path (c3p_tiled.hip): matrices in HBM, one batched MFMA GEMM launch per product
// ---------------------------------------------------------------------------
int run_pwc_tiled(DeviceWs* w, const ChainArgs& a, bool per_slice, cplx* U_out, hipStream_t st) {
  const bool lindblad = a.mode == C3P_MODE_LINDBLAD;
  const bool per_sample = !per_slice && (a.h0_bstride != 0 || a.hks_bstride != 0 || a.clp_bstride != 0);
  const int K = per_slice ? 0 : a.K;
  int Bc = c3p_tiled_chunk(a.Dm, K, a.B, per_sample, (size_t)24 << 30);
  if (c3p_opt(C3P_OPT_tiled_chunk) > 0 && c3p_opt(C3P_OPT_tiled_chunk) < Bc) Bc = (int)c3p_opt(C3P_OPT_tiled_chunk);  // (tests: a second chunk)
  void* v;
  if (ws_get(w, SL_SCRATCH, c3p_tiled_ws_bytes(a.Dm, K, Bc, per_sample), &v)) return -1;
  TiledArgs t = {};
  t.lindblad = lindblad ? 1 : 0;
  t.per_slice = per_slice ? 1 : 0;
  t.h0 = a.h0;
  t.h0_bstride = a.h0_bstride;
  t.hks = a.hks;
  t.hks_bstride = a.hks_bstride;
  t.signals = a.signals;
  t.clp = a.clp;
  t.clp_bstride = a.clp_bstride;
  t.dt = a.dt;
  t.B = a.B;
  t.K = K;
  t.N = a.N;
  t.D = a.D;
  t.Dm = a.Dm;
  t.fr_phase = a.fr_phase;
  t.U_out = U_out;
  t.dUs_out = a.dUs_out;
  g_last_kernel = C3P_KERNEL_MFMA;
  if (g_dry) return 0;  // c3p_reserve: the arena above is all this path owns
  std::string err;
  // many launches per call: the timing pair brackets the whole host-driven slice loop
  if (record_start(w, st)) return -1;
  if (c3p_tiled_run(t, v, Bc, st, err)) return fail("%s", err.c_str());
  if (record_stop(w, st)) return -1;
  return 0;
}

// Tiled backward sweep (c3p_tiled.hip): any matrix dimension, unitary and Lindblad generators
// Budget (bytes) for the per-sample forward intermediates a backward sweep keeps in HBM: 24 GB, or 60 % of what the device
// has free plus what the workspace slot that will hold them already owns (a caching allocator of the host framework may hold
// most of the 288 GB; a smaller part has less) -- the sweeps run in chunks of samples below it.
static size_t grad_store_budget(DeviceWs* w, Slot slot) {
  size_t budget = (size_t)24 << 30;
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) == hipSuccess) {
    const size_t avail = (size_t)(0.6 * (double)fr) + (w ? w->cap[slot] : 0);
    if (avail < budget) budget = avail;
  }
  if (budget < ((size_t)64 << 20)) budget = (size_t)64 << 20;
  return budget;
}
// Samples per chunk of a sweep that keeps `bytes_per_sample` of forward intermediates in SL_OUT1: what fits the budget, at least
// one; the grad_chunk option (C3P_GRAD_CHUNK) overrides it.
static long grad_chunk_samples(DeviceWs* w, size_t bytes_per_sample) {
  long Bc = (long)(grad_store_budget(w, SL_OUT1) / (bytes_per_sample + 1));
  if (c3p_opt(C3P_OPT_grad_chunk) > 0) Bc = c3p_opt(C3P_OPT_grad_chunk);
  return Bc < 1 ? 1 : Bc;
}
// run(b0, nb) on chunks of at most Bc of the B samples, until one does not return 0 (1 = not applicable, -1 = error)
template <class Run>
int in_chunks(long B, long Bc, Run&& run) {
  for (long b0 = 0; b0 < B; b0 += Bc) {
    const int rc = run(b0, (int)(B - b0 < Bc ? B - b0 : Bc));
    if (rc != 0) return rc;
  }
  return 0;
}

// ---------------------------------------------------------------------------
// Lindblad control gradient at D = 7, 8, 9 (49 x 49 .. 81 x 81 superoperators, cfg4) in the Hermitian basis: forward chain
// kernel with the transposed local prefixes kept in HBM, real segment scan, on-chip backward sweep (c3p_regrg.hip).
// The forward half returns 1 when a Hamiltonian is not Hermitian (complex tables in that basis): the caller falls back.
// ---------------------------------------------------------------------------
// D = 7, 8, 9 in their own classes.  D = 6 (36 x 36) zero padded in the 49 class is an A/B switch (regr_grad_d6 = 1): measured
// SLOWER than the complex mid-D general sweep -- 13.4 against 10.3 ms at B = 64, N = 500, 105 against 80 ms at B = 256, N = 1000
// (profiles/r04/grad_lindblad_d6_*.json): (49 / 36)^3 = 2.5x padded work eats the factor of real arithmetic
static bool lind_regr_grad_ok(int D, int Dm) {
  if (c3p_regr_supported(D, Dm)) return true;
  return Dm == D * D && D == 6 && c3p_opt_on(C3P_OPT_regr_grad_d6);
}
struct LindRegrBufs {  // device buffers of one forward pass (the library's workspace, or a caller-owned tape)
  double *tab_f, *tab_t;
  int *flag_f, *flag_t;
  cplx* seg;   // [B,S] complex slots, the real matrix in the second half of each
  double* qT;  // [B,N,Dm,Dm]
};
static long lind_regr_segments(int B, int N) {
  // fill the 256 workgroup slots evenly (rounds of 256 chains), few segments
  long S = 1;
  const long smax = N / 4 > 1 ? N / 4 : 1;
  double best = -1.0;
  for (long s = 1; s <= 32 && s <= smax; ++s) {
    const long chains = (long)B * s, rounds = (chains + C3P_REGD_MAX_WGS - 1) / C3P_REGD_MAX_WGS;
    const double eff = (double)chains / (double)(rounds * C3P_REGD_MAX_WGS) - 0.004 * (double)s;
    if (eff > best + 1e-12) best = eff, S = s;
  }
  if (c3p_opt(C3P_OPT_segments) > 0) S = std::min<long>(c3p_opt(C3P_OPT_segments), smax);
  return S;
}
struct LindRegrSizes {
  size_t tab1, ftab, seg, qT;
  size_t total() const { return 2 * tab1 + 2 * ftab + seg + qT; }
};
static LindRegrSizes lind_regr_sizes(int B, int K, int N, int Dm, long S, int nsamp) {
  auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
  LindRegrSizes z;
  z.tab1 = up((size_t)nsamp * c3p_regr_table_doubles(Dm, K) * sizeof(double));
  z.ftab = up((size_t)nsamp * (1 + K) * sizeof(int));
  z.seg = up((size_t)B * S * Dm * Dm * sizeof(cplx));
  z.qT = up((size_t)B * N * Dm * Dm * sizeof(double));
  return z;
}
static LindRegrBufs lind_regr_carve(void* base, const LindRegrSizes& z) {
  char* c = static_cast<char*>(base);
  LindRegrBufs b;
  b.tab_f = reinterpret_cast<double*>(c);
  b.tab_t = reinterpret_cast<double*>(c + z.tab1);
  b.flag_f = reinterpret_cast<int*>(c + 2 * z.tab1);
  b.flag_t = reinterpret_cast<int*>(c + 2 * z.tab1 + z.ftab);
  b.seg = reinterpret_cast<cplx*>(c + 2 * z.tab1 + 2 * z.ftab);
  b.qT = reinterpret_cast<double*>(c + 2 * z.tab1 + 2 * z.ftab + z.seg);
  return b;
}
// tables of G' and G'^T, Hermiticity flags (read back: one synchronisation per call), forward chain with Q^T
int lind_regr_forward(DeviceWs* w, const LindRegrBufs& bf, const PwcProblem& P, long S, hipStream_t st) {
  const int K = P.K, Dm = P.Dm;
  const int nsamp = P.nsamp();
  const RegdPrepArgs p = regd_prep_args(P);
  LAUNCH_TRY(c3p_launch_regr_prep_t(p, nsamp, bf.tab_f, bf.flag_f, 0, st));
  LAUNCH_TRY(c3p_launch_regr_prep_t(p, nsamp, bf.tab_t, bf.flag_t, 1, st));
  {
    std::vector<int> hf((size_t)nsamp * (1 + K));
    HIP_TRY(hipMemcpyAsync(hf.data(), bf.flag_f, hf.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int f : hf)
      if (!f) return 1;  // a non-Hermitian Hamiltonian: complex generator in the Hermitian basis
  }
  void* av;
  if (ws_get(w, SL_SCRATCH, std::max(c3p_regr_grad_arena_bytes(Dm), c3p_regr_arena_bytes(Dm)), &av)) return -1;
  MidArgs a = {};
  fill_chain(a, P, S);
  a.mode = C3P_MODE_LINDBLAD;
  a.hb_tables = bf.tab_f;
  a.hb_tabflag = bf.flag_f;
  a.hb_qT = bf.qT;
  a.no_t18n = opt_no_t18n();
  a.seg_out = bf.seg;
  LAUNCH_TRY(c3p_launch_regr_chain(a, av, st));
  return 0;
}
// cotangent in the Hermitian basis, segment scan, backward sweep (scratch from the workspace).  `mo` set: the sweep also keeps the
// sums of the generator cotangents per chain, and the reduce kernel writes the model-operator cotangents from them.
int lind_regr_backward(DeviceWs* w, const LindRegrBufs& bf, const PwcProblem& P, long S, const cplx* Ubar, double* grad, hipStream_t st,
                       const LindModelOut* mo = nullptr) {
  const int B = P.B, Dm = P.Dm;
  const size_t msz = (size_t)Dm * Dm;
  void *bv, *av;
  if (ws_get(w, SL_SEG_B, ((size_t)3 * B * S + B) * msz * sizeof(double) + (size_t)B * sizeof(double), &bv)) return -1;
  if (ws_get(w, SL_SCRATCH, std::max(c3p_regr_grad_arena_bytes(Dm), c3p_regr_arena_bytes(Dm)), &av)) return -1;
  double* pre = (double*)bv;
  double* suf = pre + (size_t)B * S * msz;
  double* lam = suf + (size_t)B * S * msz;
  double* ubr = lam + (size_t)B * S * msz;
  double* tau = ubr + (size_t)B * msz;
  LAUNCH_TRY(c3p_launch_hb_ubar(Ubar, P.fr_phase, B, P.D, ubr, st));
  LAUNCH_TRY(c3p_launch_regr_scan(bf.seg, ubr, B, (int)S, Dm, pre, suf, lam, tau, st));
  RegrGradArgs g = {};
  g.tables = bf.tab_f;
  g.tables_t = bf.tab_t;
  g.tab_per_sample = P.per_sample() ? 1 : 0;
  g.signals = P.signals;
  g.qT = bf.qT;
  g.lam = lam;
  g.tau = tau;
  g.grad = grad;
  g.arena = (double*)av;
  g.B = B;
  g.K = P.K;
  g.N = P.N;
  g.Dm = Dm;
  g.S = (int)S;
  g.degree = c3p_opt(C3P_OPT_regr_grad_degree) > 0 ? (int)c3p_opt(C3P_OPT_regr_grad_degree) : 0;
  if (mo) {
    void* mv;
    if (ws_get(w, SL_LMODEL_PART, (size_t)B * S * c3p_regr_model_part_doubles(Dm, P.K) * sizeof(double), &mv)) return -1;
    g.mpart = (double*)mv;
  }
  LAUNCH_TRY(c3p_launch_regr_grad(g, st));
  if (mo)
    LAUNCH_TRY(c3p_launch_regr_model_reduce(g.mpart, tau, P.signals, mo->col, mo->col_bs, mo->C, B, (int)S, P.K, P.N, P.D, P.dt, mo->g_h0, mo->g_hks,
                                            mo->g_col, st));
  return 0;
}
int run_vjp_lind_regr(DeviceWs* w, const PwcProblem& P, const cplx* Ubar, double* grad, hipStream_t st, const LindModelOut* mo = nullptr) {
  const int B = P.B, K = P.K, N = P.N, Dm = P.Dm;
  if (!lind_regr_grad_ok(P.D, Dm) || K > 16 || K < 1) return 1;
  const long S = lind_regr_segments(B, N);
  const LindRegrSizes z = lind_regr_sizes(B, K, N, Dm, S, P.nsamp());
  void *tv, *sv, *qv;
  if (ws_get(w, SL_TABLES, 2 * z.tab1 + 2 * z.ftab, &tv)) return -1;
  if (ws_get(w, SL_SEG_A, z.seg, &sv)) return -1;
  if (ws_get(w, SL_OUT1, z.qT, &qv)) return -1;
  LindRegrBufs bf = lind_regr_carve(tv, z);
  bf.seg = (cplx*)sv;
  bf.qT = (double*)qv;
  const int rc = lind_regr_forward(w, bf, P, S, st);
  if (rc != 0) return rc;
  return lind_regr_backward(w, bf, P, S, Ubar, grad, st, mo);
}

int run_vjp_tiled(DeviceWs* w, const PwcProblem& P, const cplx* U_bar, double* grad, hipStream_t st, bool per_slice = false,
                  cplx* zout = nullptr) {
  const int B = P.B, K = P.K, N = P.N, Dm = P.Dm;
  const bool per_sample = !per_slice && P.per_sample();
  int Bc = c3p_tiled_vjp_chunk(Dm, K, N, B, per_sample, grad_store_budget(w, SL_SCRATCH));
  if (c3p_opt(C3P_OPT_tiled_chunk) > 0 && c3p_opt(C3P_OPT_tiled_chunk) < Bc) Bc = (int)c3p_opt(C3P_OPT_tiled_chunk);  // (tests: a second chunk)
  void* v;
  if (ws_get(w, SL_SCRATCH, c3p_tiled_vjp_ws_bytes(Dm, K, N, Bc, per_sample), &v)) return -1;
  if (g_dry) return 0;
  TiledArgs t = {};
  t.lindblad = P.lindblad;
  t.per_slice = per_slice ? 1 : 0;
  t.h0 = P.h0;
  t.h0_bstride = P.h0_bs;
  t.hks = P.hks;
  t.hks_bstride = P.hk_bs;
  t.signals = P.signals;
  t.clp = P.clp;
  t.clp_bstride = P.clp_bs;
  t.dt = P.dt;
  t.B = B;
  t.K = K;
  t.N = N;
  t.D = P.D;
  t.Dm = Dm;
  t.fr_phase = P.fr_phase;
  // the per-slice launch sequences are replayed as hipGraphs, which the legacy default stream cannot capture
  hipStream_t run = st;
  if (!run) {
    if (!w->aux) HIP_TRY(hipStreamCreate(&w->aux));
    run = w->aux;
  }
  std::string err;
  if (c3p_tiled_vjp_run(t, U_bar, grad, zout, v, Bc, run, err)) return fail("%s", err.c_str());
  return 0;
}

// Host-pointer staging helpers --------------------------------------------------
struct Stage {
  DeviceWs* w;
  hipStream_t st;
  int in_slot = SL_IN0;
  int out_slot = SL_OUT0;
  struct Back {
    void* host;
    void* dev;
    size_t bytes;
  };
  std::vector<Back> backs;
  int in(const void* host, size_t bytes, const void** dev) {
    if (!host || bytes == 0) {
      *dev = nullptr;
      return 0;
    }
    void* d;
    if (in_slot > SL_IN7) return fail("internal: out of input staging slots");
    if (ws_get(w, (Slot)in_slot++, bytes, &d)) return -1;
    HIP_TRY(hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, st));
    *dev = d;
    return 0;
  }
  int out(void* host, size_t bytes, void** dev) {
    if (!host || bytes == 0) {
      *dev = nullptr;
      return 0;
    }
    void* d;
    if (out_slot > SL_OUT6) return fail("internal: out of output staging slots");
    if (ws_get(w, (Slot)out_slot++, bytes, &d)) return -1;
    backs.push_back({host, d, bytes});
    *dev = d;
    return 0;
  }
  int finish() {
    for (auto& b : backs) HIP_TRY(hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
  }
};

// The dissipator(s) of a Lindblad call into SL_CLP: one [Dm,Dm] for the batch, or one per sample under C3P_COL_PER_SAMPLE
// (*bs = elements between them, 0 = shared).
int build_clp(DeviceWs* w, const void* d_col, int C, int D, int B, int flags, const cplx** clp, long* bs, hipStream_t st) {
  const long gsz = (long)D * D * D * D;
  const int nb = (flags & C3P_COL_PER_SAMPLE) ? B : 1;
  void* v;
  if (ws_get(w, SL_CLP, (size_t)nb * gsz * sizeof(cplx), &v)) return -1;
  LAUNCH_TRY(c3p_launch_clp((const cplx*)d_col, C, D, nb, (cplx*)v, st));
  *clp = (const cplx*)v;
  *bs = (flags & C3P_COL_PER_SAMPLE) ? gsz : 0;
  return 0;
}

// One open-system gradient call (c3p_pwc_lindblad_vjp and the two model-cotangent entries) between its argument checks and its
// result: the workspace lock, the staged operands, the dissipator, the problem record and, for the model entries, where the operator
// cotangents go.  open() once, kernel families over the sample chunks, served(kernel) once.
struct LindGradCall {
  std::optional<WsLock> lk;
  DeviceWs* w = nullptr;
  hipStream_t st = nullptr;
  Stage sg{nullptr, nullptr};
  int flags = 0;
  PwcProblem P = {};
  const cplx* ubar = nullptr;  // [B,Dm,Dm]
  double* grad = nullptr;      // [B,K,N]
  LindModelOut mo = {};        // want_model only

  // The checks every entry makes (`own`: the entry's extra ones, in their place), then lock, staging, dissipator and records.
  // 0 = go on, 1 = nothing to do (B = 0), -1 = error.  grad_signals may be NULL for a model entry (the sweep then writes into SL_OUT0).
  template <class Own>
  int open(const char* entry, int bad_flags, bool want_model, Own&& own, const void* h0, int64_t h0_bstride, const void* hks,
           int64_t hks_bstride, const double* signals, const void* col_ops, int C, double dt, int B, int K, int N, int D, int flags_,
           const double* fr_phase, const void* U_bar, double* grad_signals, void* grad_h0, void* grad_hks, void* grad_col_ops, void* stream) {
    if (B < 0 || K <= 0 || N <= 0 || D <= 0 || C <= 0) return fail("bad sizes B=%d K=%d N=%d D=%d C=%d", B, K, N, D, C);
    if (flags_ & bad_flags) return fail("%s: unsupported flag", entry);
    if (own()) return -1;
    if (B == 0) return 1;
    if (!h0 || !hks || !signals || !col_ops || !U_bar || (want_model ? !grad_h0 || !grad_hks || !grad_col_ops : !grad_signals))
      return fail("NULL pointer argument");
    if (h0_bstride < 0 || hks_bstride < 0) return fail("negative batch stride");
    const size_t cs = sizeof(cplx);
    const int Dm = D * D;
    flags = flags_;
    st = (hipStream_t)stream;
    lk.emplace(st);
    w = lk->w;
    if (!w) return fail("no HIP device");
    if (!lk->ok) return fail("hipStreamWaitEvent on the previous call's stream failed");
    sg.w = w, sg.st = st;
    const void *d_h0 = h0, *d_hks = hks, *d_sig = signals, *d_ph = fr_phase, *d_ub = U_bar, *d_col = col_ops;
    void* d_grad = grad_signals;
    cplx *g_h0 = (cplx*)grad_h0, *g_hks = (cplx*)grad_hks, *g_col = (cplx*)grad_col_ops;
    if (flags & C3P_HOST_PTRS) {
      if (sg.in(h0, staged_elems(B, h0_bstride, (size_t)D * D) * cs, &d_h0)) return -1;
      if (sg.in(hks, staged_elems(B, hks_bstride, (size_t)K * D * D) * cs, &d_hks)) return -1;
      if (sg.in(signals, (size_t)B * K * N * sizeof(double), &d_sig)) return -1;
      if (sg.in(col_ops, col_elems(flags, B, C, D) * cs, &d_col)) return -1;
      if (sg.in(U_bar, (size_t)B * Dm * Dm * cs, &d_ub)) return -1;
      if (fr_phase && sg.in(fr_phase, (size_t)B * Dm * sizeof(double), &d_ph)) return -1;
      if (sg.out(grad_signals, (size_t)B * K * N * sizeof(double), &d_grad)) return -1;  // SL_OUT0 (SL_OUT1 is the sweep's store)
      if (want_model) {  // the three operator cotangents are staged in one block of their own
        void* blk;
        const size_t n0 = (size_t)B * D * D, nk = (size_t)B * K * D * D, nc = (size_t)B * C * D * D;
        if (ws_get(w, SL_LMODEL_OUT, (n0 + nk + nc) * cs, &blk)) return -1;
        g_h0 = (cplx*)blk, g_hks = g_h0 + n0, g_col = g_hks + nk;
        sg.backs.push_back({grad_h0, g_h0, n0 * cs});
        sg.backs.push_back({grad_hks, g_hks, nk * cs});
        sg.backs.push_back({grad_col_ops, g_col, nc * cs});
      }
    }
    if (!d_grad) {  // grad_signals not wanted: the sweep still writes it
      if (ws_get(w, SL_OUT0, (size_t)B * K * N * sizeof(double), &d_grad)) return -1;
    }
    const cplx* clp;
    long clp_bs;
    if (build_clp(w, d_col, C, D, B, flags, &clp, &clp_bs, st)) return -1;
    P = {(const cplx*)d_h0, h0_bstride, (const cplx*)d_hks, hks_bstride, (const double*)d_sig, clp, clp_bs, dt, B, K, N, D, Dm, 1, (const double*)d_ph};
    ubar = (const cplx*)d_ub;
    grad = (double*)d_grad;
    if (want_model) mo = {(const cplx*)d_col, col_bstride(flags, C, D), C, g_h0, g_hks, g_col};
    return 0;
  }
  // the switches that take a call off the on-chip sweeps
  bool on_chip() const { return !(flags & C3P_FORCE_GENERIC) && !c3p_opt_on(C3P_OPT_tiled_grad) && !c3p_opt_on(C3P_OPT_valu_grad); }
  // One kernel family over the call, from the start of the timed span: run(chunk, U_bar, grad_signals, b0) on chunks of samples that
  // keep `bytes_per_sample` of forward intermediates below the budget (grad_chunk_samples), until one does not return 0; what that
  // one returned (1 = the family declined: go on to the next, -1 = error), else 0.
  template <class Run>
  int chunks(size_t bytes_per_sample, Run&& run) {
    if (record_start(w, st)) return -1;
    return in_chunks(P.B, grad_chunk_samples(w, bytes_per_sample),
                     [&](long b0, int nb) { return run(P.chunk(b0, nb), ubar_at(P, ubar, b0), grad_at(P, grad, b0), b0); });
  }
  // the same, through to the result of the call where the family served it: 0 / -1, or 1 = declined
  template <class Run>
  int family(size_t bytes_per_sample, int kernel, Run&& run) {
    const int rc = chunks(bytes_per_sample, run);
    return rc == 0 ? served(kernel) : rc;
  }
  // a family served the call: the kernel it reports, the end of the timed span, the staged results back
  int served(int kernel) {
    g_last_kernel = kernel;
    if (record_stop(w, st)) return -1;
    if (flags & C3P_HOST_PTRS) return sg.finish();
    return 0;
  }
};

// The plan of a taped open-system evaluation for (B, K, N, D): kernel family, segment count, tape size.  Host arithmetic on the
// option table as it is now; c3p_pwc_lindblad_tape_bytes reports it, both taped calls check the caller's tape against it.
enum TapeFamily {
  TAPE_NONE = 0,
  TAPE_SMALL,   // D = 2, 3: the small-D kernels; real or complex layout by C3P_HERMITIAN_H (lind_smallr_ok), the complex size
  TAPE_REAL16,  // D = 4: the real Hermitian-basis kernels only (the taped calls then need C3P_HERMITIAN_H)
  TAPE_REGR     // D = 7, 8, 9: the Hermitian-basis kernels of c3p_regr.hip
};
struct LindTapePlan {
  TapeFamily family;
  int segments;
  size_t bytes;
};
LindTapePlan lind_tape_plan(int B, int K, int N, int D) {
  const LindTapePlan none = {TAPE_NONE, 0, 0};
  if (B > 0 && K >= 1 && K <= 8 && N > 0 && D == 4) {
    const int S = c3p_opt_on(C3P_OPT_no_smallr) ? -1 : pick_segments_r(B, N, K, 16, true, true);
    return S > 0 ? LindTapePlan{TAPE_REAL16, S, lind_smallr_sizes(B, K, N, 16, S, B).total()} : none;
  }
  if (B > 0 && K >= 1 && K <= 8 && N > 0 && D >= 2 && D <= 3) {
    // superoperators up to 9 x 9 on the small-D kernels: tables, segment products and the slice propagators (the generator is
    // not anti-Hermitian: the backward sweep cannot recompute prefixes from the adjoint side); per-sample operators need S % 4 = 0
    const int S = lind_small_segments(B, K, N, D * D, true);
    return S > 0 ? LindTapePlan{TAPE_SMALL, S, lind_small_sizes(B, K, N, D * D, S, B).total()} : none;
  }
  if (B <= 0 || K < 1 || N <= 0 || D <= 0 || !c3p_regr_supported(D, D * D) || K > 16) return none;
  const long S = lind_regr_segments(B, N);
  return {TAPE_REGR, (int)S, lind_regr_sizes(B, K, N, D * D, S, B).total()};
}

int pwc_common(int lindblad, const void* h0, int64_t h0_bstride, const void* hks, int64_t hks_bstride,
               const double* signals, const void* col_ops, int C, double dt, int B, int K, int N, int D,
               int flags, const double* fr_phase, void* U_out, void* dUs_out, void* stream, const void* record = nullptr) {
  if (B < 0 || N < 0 || D <= 0 || K < 0) return fail("bad sizes B=%d K=%d N=%d D=%d", B, K, N, D);
  if (!U_out) return fail("U_out is NULL");
  if (B == 0) return 0;
  if (N == 0) return fail("empty time grid (N == 0)");
  if (!h0) return fail("h0 is NULL");
  if (K > 0 && (!hks || !signals)) return fail("K > 0 but hks/signals missing");
  if (lindblad && (!col_ops || C <= 0)) return fail("lindblad propagation needs col_ops");
  if (!lindblad && (flags & C3P_COL_PER_SAMPLE)) return fail("c3p_pwc_unitary: C3P_COL_PER_SAMPLE needs collapse operators (c3p_pwc_lindblad)");
  const bool per_slice = (flags & C3P_PER_SLICE_H) != 0;
  const int Dm = lindblad ? D * D : D;
  const size_t cs = sizeof(cplx);
  hipStream_t st = (hipStream_t)stream;
  WsLock lk(st);
  DeviceWs* w = lk.w;
  if (!w) return fail("no HIP device");
  if (!lk.ok) return fail("hipStreamWaitEvent on the previous call's stream failed");
  Stage sg{w, st};
  const void *d_h0 = h0, *d_hks = hks, *d_sig = signals, *d_col = col_ops, *d_ph = fr_phase;
  void *d_U = U_out, *d_dUs = dUs_out;
  if (flags & C3P_HOST_PTRS) {
    if (sg.in(h0, staged_elems(B, h0_bstride, (size_t)(per_slice ? N : 1) * D * D) * cs, &d_h0)) return -1;
    if (sg.in(hks, K ? staged_elems(B, hks_bstride, (size_t)K * D * D) * cs : 0, &d_hks)) return -1;
    if (sg.in(signals, (size_t)B * K * N * sizeof(double), &d_sig)) return -1;
    if (sg.in(col_ops, lindblad ? col_elems(flags, B, C, D) * cs : 0, &d_col)) return -1;
    if (sg.in(fr_phase, fr_phase ? (size_t)B * Dm * sizeof(double) : 0, &d_ph)) return -1;
    if (sg.out(U_out, (size_t)B * Dm * Dm * cs, &d_U)) return -1;
    if (sg.out(dUs_out, dUs_out ? (size_t)B * N * Dm * Dm * cs : 0, &d_dUs)) return -1;
  }
  ChainArgs a = {};
  a.h0 = (const cplx*)d_h0;
  a.h0_bstride = h0_bstride;
  a.h0_nstride = per_slice ? (long)D * D : 0;
  a.hks = (const cplx*)d_hks;
  a.hks_bstride = hks_bstride;
  a.signals = (const double*)d_sig;
  a.fr_phase = (const double*)d_ph;
  a.dt = dt;
  a.B = B;
  a.K = K;
  a.N = N;
  a.D = D;
  a.Dm = Dm;
  a.mode = lindblad ? C3P_MODE_LINDBLAD : C3P_MODE_UNITARY;
  a.dUs_out = (cplx*)d_dUs;
  if (lindblad && build_clp(w, d_col, C, D, B, flags, &a.clp, &a.clp_bstride, st)) return -1;
  // a model record serves the unitary small-D table route with operators shared by the batch; every other call ignores it
  const bool use_record = record && !lindblad && !per_slice && !(flags & (C3P_FORCE_GENERIC | C3P_HOST_PTRS)) && h0_bstride == 0 &&
                          hks_bstride == 0 && c3p_pwc_record_bytes(D, K) != 0;
  const PwcProblem P = {a.h0, a.h0_bstride, a.hks, a.hks_bstride, a.signals, a.clp, a.clp_bstride, dt, B, K, N, D, Dm, lindblad, a.fr_phase,
                        use_record ? (const double*)record : nullptr};
  bool done = false;
  if (!(flags & C3P_FORCE_GENERIC) && per_slice && !lindblad && K == 0 && D <= kSmallDLimit && c3p_smalld_supported(D)) {
    // branch B (propagation.py:295-308): X_n = -i dt H_n
    const int rc = run_xg_smalld(w, a.h0, a.h0_bstride, 0.0, -dt, B, N, D, a.fr_phase, (cplx*)d_U, a.dUs_out, st);
    if (rc < 0) return -1;
    done = (rc == 0);
  }
  if (!done && !(flags & C3P_FORCE_GENERIC) && per_slice && !lindblad && K == 0 && D >= 13 && D <= 40) {
    const int rc = run_xg_midd(w, a.h0, a.h0_bstride, 0.0, -dt, B, N, D, a.fr_phase, (cplx*)d_U, a.dUs_out, st);
    if (rc < 0) return -1;
    done = (rc == 0);
  }
  if (!done && !(flags & C3P_FORCE_GENERIC) && per_slice && lindblad && K == 0 && Dm <= 40 &&
      (size_t)B * N * Dm * Dm * cs <= ((size_t)16 << 30)) {
    // branch B with model.lindbladian (propagation.py:295-308 into :551-585): the dense superoperator generator of every slice,
    // then the supplied-generator mode of the matrix-core chain kernels with X_n = dt L_n
    void* gv;
    if (ws_get(w, SL_SCRATCH, (size_t)B * N * Dm * Dm * cs, &gv)) return -1;
    LAUNCH_TRY(c3p_launch_lind_slice_generators(a.h0, a.h0_bstride, a.clp, a.clp_bstride, B, N, D, (cplx*)gv, st));
    const long gbs = (long)N * Dm * Dm;
    const int rc = (Dm <= kSmallDLimit && c3p_smalld_supported(Dm))
                       ? run_xg_smalld(w, (const cplx*)gv, gbs, dt, 0.0, B, N, Dm, a.fr_phase, (cplx*)d_U, a.dUs_out, st)
                       : run_xg_midd(w, (const cplx*)gv, gbs, dt, 0.0, B, N, Dm, a.fr_phase, (cplx*)d_U, a.dUs_out, st);
    if (rc < 0) return -1;
    done = (rc == 0);
  }
  if (!done && !(flags & C3P_FORCE_GENERIC) && !per_slice && lindblad && (flags & C3P_HERMITIAN_H) && !a.dUs_out &&
      c3p_smallr_supported(D, Dm, K) && !c3p_opt_on(C3P_OPT_no_smallr)) {
    const int rc = run_pwc_smallr(w, P, (cplx*)d_U, st);
    if (rc < 0) return -1;
    done = (rc == 0);
  }
  if (!done && !(flags & C3P_FORCE_GENERIC) && !per_slice && Dm <= kSmallDLimit && c3p_smalld_supported(Dm) && K <= 8) {
    const int rc = run_pwc_smalld(w, P, (cplx*)d_U, a.dUs_out, st);
    if (rc < 0) return -1;
    done = (rc == 0);
  }
  if (!done && !(flags & C3P_FORCE_GENERIC) && !per_slice && Dm >= 13 && Dm <= 40 && K <= 16) {
    const int rc = run_pwc_midd(w, P, (cplx*)d_U, a.dUs_out, st);
    if (rc < 0) return -1;
    done = (rc == 0);
  }
  if (!done && !(flags & C3P_FORCE_GENERIC) && !per_slice && c3p_regd_supported(Dm) && K <= 16 && !c3p_opt_on(C3P_OPT_no_regd)) {
    const int rc = run_pwc_regd(w, P, (cplx*)d_U, a.dUs_out, st);
    if (rc < 0) return -1;
    done = (rc == 0);
  }
  if (!done && !(flags & C3P_FORCE_GENERIC) && !per_slice && K <= 16) {
    const int rc = run_pwc_bigd(w, P, (cplx*)d_U, a.dUs_out, st);
    if (rc < 0) return -1;
    done = (rc == 0);
  }
  // beyond the on-chip kernels: Dm >= 93, and supplied / per-slice generators at Dm >= 41 (the generic kernel would run
  // those from global scratch at a few percent of the roofline, and stops at Dm = 256)
  if (!done && !(flags & C3P_FORCE_GENERIC) && !c3p_opt_on(C3P_OPT_no_tiled) && (Dm >= 93 || (per_slice && Dm >= 41)) &&
      (per_slice ? K == 0 : true)) {
    if (run_pwc_tiled(w, a, per_slice, (cplx*)d_U, st)) return -1;
    done = true;
  }
  if (!done && run_chain_generic(w, a, (cplx*)d_U, st)) return -1;
  if (flags & C3P_HOST_PTRS) return sg.finish();
  return 0;
}

}  // namespace

long c3p_opt(C3pOption o) {
  std::call_once(g_opt_once, opt_init);
  return g_opt_val[o].load(std::memory_order_relaxed);
}

void c3p_note_launch(const void* host_fn, const char* file) {
  for (int i = 0; i < g_nnotes; ++i)
    if (g_notes[i].fn == host_fn) {
      ++g_notes[i].count;
      return;
    }
  if (g_nnotes < (int)(sizeof(g_notes) / sizeof(g_notes[0]))) g_notes[g_nnotes++] = LaunchNote{host_fn, file, 1};
}

extern "C" {

int c3p_version(void) { return 1; }

int c3p_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

const char* c3p_last_error(void) { return g_err.c_str(); }
int c3p_last_kernel(void) { return g_last_kernel; }

int c3p_last_kernel_detail(char* buf, int cap) {
  std::string out;
  for (int i = 0; i < g_nnotes; ++i) {
    const LaunchNote& n = g_notes[i];
    const char* raw = hipKernelNameRefByPtr(n.fn, nullptr);
    (void)hipGetLastError();
    std::string name = raw ? raw : "?";
    int status = 1;
    char* dm = abi::__cxa_demangle(name.c_str(), nullptr, nullptr, &status);
    if (status == 0 && dm) name = dm;
    free(dm);
    // "void (anonymous namespace)::kernel<...>(Args)" -> "kernel<...>"
    size_t p0 = name.rfind(')');
    if (p0 != std::string::npos) {  // drop the parameter list: the matching '(' of the LAST ')'
      int depth = 0;
      for (size_t q = p0 + 1; q-- > 0;) {
        if (name[q] == ')') ++depth;
        else if (name[q] == '(' && --depth == 0) {
          name.erase(q);
          break;
        }
      }
    }
    const std::string anon = "(anonymous namespace)::";
    for (size_t q; (q = name.find(anon)) != std::string::npos;) name.erase(q, anon.size());
    if (name.rfind("void ", 0) == 0) name.erase(0, 5);
    const char* base = strrchr(n.file, '/');
    if (!out.empty()) out += "; ";
    out += std::string(base ? base + 1 : n.file) + ": " + name;
    if (n.count > 1) out += " x" + std::to_string(n.count);
  }
  if (!g_note_plan.empty()) out += (out.empty() ? "" : "; ") + g_note_plan;
  if (buf && cap > 0) {
    const size_t m = std::min(out.size(), (size_t)cap - 1);
    memcpy(buf, out.data(), m);
    buf[m] = 0;
  }
  return (int)out.size();
}

int c3p_set_option(const char* name, const char* value) {
  if (!name) return fail("c3p_set_option: null name");
  std::call_once(g_opt_once, opt_init);
  for (int i = 0; i < C3P_OPT_COUNT; ++i)
    if (!strcmp(name, g_opt_names[i])) {
      g_opt_val[i].store(value ? parse_opt_value(value) : -1, std::memory_order_relaxed);
      return 0;
    }
  return fail("c3p_set_option: unknown option '%s'", name);
}

long c3p_get_option(const char* name) {
  if (!name) return -2;
  std::call_once(g_opt_once, opt_init);
  for (int i = 0; i < C3P_OPT_COUNT; ++i)
    if (!strcmp(name, g_opt_names[i])) return g_opt_val[i].load(std::memory_order_relaxed);
  return -2;
}

int c3p_set_profiling(int enable) {
  DeviceWs* w = ws_for_current_device();
  if (!w) return fail("no HIP device");
  w->profiling = enable ? 1 : 0;
  return 0;
}

long c3p_workspace_generation(void) {
  DeviceWs* w = ws_for_current_device();
  return w ? w->generation.load() : -1;
}

int c3p_reserve(int lindblad, int B, int K, int N, int D, int C, int flags) {
  if (flags & C3P_HOST_PTRS) return fail("c3p_reserve sizes the device workspace: not for C3P_HOST_PTRS calls");
  // the planning code of the real call with launches switched off: every slot it would touch is allocated at the size
  // it would need, so later calls of this shape (and smaller ones) never allocate, free or synchronise
  static double dummy[4];
  void* p = dummy;  // never dereferenced: device pointers are only handed to kernels
  g_dry = true;
  const int rc = pwc_common(lindblad ? 1 : 0, p, 0, p, 0, (const double*)p, lindblad ? p : nullptr, lindblad ? C : 0, 1.0, B, K, N, D,
                            flags, nullptr, p, nullptr, nullptr);
  g_dry = false;
  return rc;
}

double c3p_last_kernel_ms(void) {
  WsLock lk(nullptr, false);
  DeviceWs* w = lk.w;
  if (!w || !w->ev_valid) return -1.0;
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, w->ev0, w->ev1) != hipSuccess) {
    (void)hipGetLastError();
    return -1.0;
  }
  return (double)ms;
}

void c3p_shutdown(void) {
  std::vector<DeviceWs*> all;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    for (auto& p : g_ws) all.push_back(p.get());
  }
  int cur = 0;
  (void)hipGetDevice(&cur);
  for (size_t d = 0; d < all.size(); ++d) {
    DeviceWs* w = all[d];
    if (!w) continue;
    std::lock_guard<std::mutex> lk(w->mu);
    bool any = w->ev0 != nullptr || w->done != nullptr || w->aux != nullptr;
    for (int s = 0; s < SL_COUNT; ++s) any = any || w->ptr[s];
    if (!any) continue;
    (void)hipSetDevice((int)d);
    (void)hipDeviceSynchronize();
    for (int s = 0; s < SL_COUNT; ++s) {
      if (w->ptr[s]) (void)hipFree(w->ptr[s]);
      w->ptr[s] = nullptr;
      w->cap[s] = 0;
    }
    if (w->ev0) {
      (void)hipEventDestroy(w->ev0);
      (void)hipEventDestroy(w->ev1);
      w->ev0 = w->ev1 = nullptr;
      w->ev_valid = false;
    }
    if (w->done) {
      (void)hipEventDestroy(w->done);
      w->done = nullptr;
    }
    if (w->aux) {
      (void)hipStreamDestroy(w->aux);
      w->aux = nullptr;
    }
  }
  // the remembered stream may be destroyed by the caller after a shutdown: never touch it again
  for (DeviceWs* w : all)
    if (w) {
      std::lock_guard<std::mutex> lk(w->mu);
      w->has_last = false;
      w->last_stream = nullptr;
    }
  (void)hipSetDevice(cur);
}

int c3p_pwc_unitary(const void* h0, int64_t h0_bstride, const void* hks, int64_t hks_bstride,
                    const double* signals, double dt, int B, int K, int N, int D, int flags,
                    const double* fr_phase, void* U_out, void* dUs_out, void* stream) {
  return pwc_common(0, h0, h0_bstride, hks, hks_bstride, signals, nullptr, 0, dt, B, K, N, D, flags,
                    fr_phase, U_out, dUs_out, stream);
}

size_t c3p_pwc_record_bytes(int D, int K) {
  if (D < 2 || D > kSmallDLimit || !c3p_smalld_supported(D) || K < 0 || K > 8) return 0;  // the shapes run_pwc_smalld takes
  return c3p_smalld_record_doubles(D, K) * sizeof(double);
}

int c3p_pwc_record_build(const void* h0, const void* hks, double dt, int K, int D, int flags, void* record, void* stream) {
  if (c3p_pwc_record_bytes(D, K) == 0) return fail("c3p_pwc_record_build: no record is served for D=%d K=%d", D, K);
  if (flags & C3P_HOST_PTRS) return fail("c3p_pwc_record_build: device pointers only");
  if (!h0 || !record) return fail("c3p_pwc_record_build: h0 or record is NULL");
  if (K > 0 && !hks) return fail("K > 0 but hks missing");
  hipStream_t st = (hipStream_t)stream;
  WsLock lk(st);
  if (!lk.w) return fail("no HIP device");
  if (!lk.ok) return fail("hipStreamWaitEvent on the previous call's stream failed");
  SmallArgs a = {};
  a.h0 = (const cplx*)h0;
  a.hks = (const cplx*)hks;
  a.dt = dt;
  a.K = K;
  a.Dm = D;
  g_last_kernel = C3P_KERNEL_SMALLD;
  LAUNCH_TRY(c3p_launch_smalld_record(a, (double*)record, st));
  return 0;
}

int c3p_pwc_unitary_rec(const void* h0, int64_t h0_bstride, const void* hks, int64_t hks_bstride, const double* signals, double dt, int B,
                        int K, int N, int D, int flags, const double* fr_phase, void* U_out, void* dUs_out, const void* record,
                        void* stream) {
  return pwc_common(0, h0, h0_bstride, hks, hks_bstride, signals, nullptr, 0, dt, B, K, N, D, flags, fr_phase, U_out, dUs_out, stream,
                    record);
}

int c3p_pwc_lindblad(const void* h0, int64_t h0_bstride, const void* hks, int64_t hks_bstride,
                     const double* signals, const void* col_ops, int C, double dt, int B, int K,
                     int N, int D, int flags, const double* fr_phase, void* U_out, void* dUs_out,
                     void* stream) {
  return pwc_common(1, h0, h0_bstride, hks, hks_bstride, signals, col_ops, C, dt, B, K, N, D, flags,
                    fr_phase, U_out, dUs_out, stream);
}

int c3p_expm(const void* A, int n, int D, int flags, void* out, void* stream) {
  if (n < 0 || D <= 0) return fail("bad sizes n=%d D=%d", n, D);
  if (n == 0) return 0;
  if (!A || !out) return fail("NULL matrix pointer");
  hipStream_t st = (hipStream_t)stream;
  WsLock lk(st);
  DeviceWs* w = lk.w;
  if (!w) return fail("no HIP device");
  if (!lk.ok) return fail("hipStreamWaitEvent on the previous call's stream failed");
  Stage sg{w, st};
  const void* d_A = A;
  void* d_out = out;
  const size_t bytes = (size_t)n * D * D * sizeof(cplx);
  if (flags & C3P_HOST_PTRS) {
    if (sg.in(A, bytes, &d_A)) return -1;
    if (sg.out(out, bytes, &d_out)) return -1;
  }
  bool done = false;
  if (!(flags & C3P_FORCE_GENERIC) && D <= kSmallDLimit && c3p_smalld_supported(D)) {
    const int rc = run_xg_smalld(w, (const cplx*)d_A, (long)D * D, 1.0, 0.0, n, 1, D, nullptr, (cplx*)d_out, nullptr, st);
    if (rc < 0) return -1;
    done = (rc == 0);
  }
  if (!done && !(flags & C3P_FORCE_GENERIC) && D >= 13 && D <= 40) {
    const int rc = run_xg_midd(w, (const cplx*)d_A, (long)D * D, 1.0, 0.0, n, 1, D, nullptr, (cplx*)d_out, nullptr, st);
    if (rc < 0) return -1;
    done = (rc == 0);
  }
  ChainArgs a = {};
  a.mode = C3P_MODE_EXPM;
  a.mats = (const cplx*)d_A;
  a.B = n;
  a.N = 1;
  a.D = D;
  a.Dm = D;
  if (!done && run_chain_generic(w, a, (cplx*)d_out, st)) return -1;
  if (flags & C3P_HOST_PTRS) return sg.finish();
  return 0;
}

int c3p_matmul_chain(const void* M, int B, int N, int D, int flags, void* out, void* stream) {
  if (B < 0 || N < 0 || D <= 0) return fail("bad sizes B=%d N=%d D=%d", B, N, D);
  if (B == 0) return 0;
  if (N == 0) return fail("empty matrix list (N == 0)");
  if (!M || !out) return fail("NULL matrix pointer");
  hipStream_t st = (hipStream_t)stream;
  WsLock lk(st);
  DeviceWs* w = lk.w;
  if (!w) return fail("no HIP device");
  if (!lk.ok) return fail("hipStreamWaitEvent on the previous call's stream failed");
  Stage sg{w, st};
  const void* d_M = M;
  void* d_out = out;
  if (flags & C3P_HOST_PTRS) {
    if (sg.in(M, (size_t)B * N * D * D * sizeof(cplx), &d_M)) return -1;
    if (sg.out(out, (size_t)B * D * D * sizeof(cplx), &d_out)) return -1;
  }
  ChainArgs a = {};
  a.mode = C3P_MODE_GIVEN;
  a.mats = (const cplx*)d_M;
  a.B = B;
  a.N = N;
  a.D = D;
  a.Dm = D;
  a.right_order = (flags & C3P_ORDER_RIGHT) ? 1 : 0;
  if (!(flags & C3P_FORCE_GENERIC) && D <= kSmallDLimit && c3p_smalld_supported(D)) {
    g_last_kernel = C3P_KERNEL_SMALLD;
    if (combine_chain(c3p_launch_smalld_chain, w, (const cplx*)d_M, B, N, D, a.right_order, nullptr, (cplx*)d_out, st)) return -1;
  } else if (!(flags & C3P_FORCE_GENERIC) && D >= 13 && D <= 40) {
    g_last_kernel = C3P_KERNEL_MFMA;
    if (combine_chain(c3p_launch_midd_chain, w, (const cplx*)d_M, B, N, D, a.right_order, nullptr, (cplx*)d_out, st)) return -1;
  } else if (run_chain_generic(w, a, (cplx*)d_out, st)) {
    return -1;
  }
  if (flags & C3P_HOST_PTRS) return sg.finish();
  return 0;
}

static int kron_common(const void* A, const void* Bm, int n, int Da, int Db, int which, int flags,
                       void* out, void* stream) {
  if (n < 0 || Da <= 0 || Db <= 0) return fail("bad sizes n=%d Da=%d Db=%d", n, Da, Db);
  if (n == 0) return 0;
  if (!A || !out || (which == 0 && !Bm)) return fail("NULL matrix pointer");
  hipStream_t st = (hipStream_t)stream;
  WsLock lk(st);
  DeviceWs* w = lk.w;
  if (!w) return fail("no HIP device");
  if (!lk.ok) return fail("hipStreamWaitEvent on the previous call's stream failed");
  Stage sg{w, st};
  const void *d_A = A, *d_B = Bm;
  void* d_out = out;
  const size_t Dm = (size_t)Da * Db;
  if (flags & C3P_HOST_PTRS) {
    if (sg.in(A, (size_t)n * Da * Da * sizeof(cplx), &d_A)) return -1;
    if (sg.in(which == 0 ? Bm : nullptr, (size_t)n * Db * Db * sizeof(cplx), &d_B)) return -1;
    if (sg.out(out, (size_t)n * Dm * Dm * sizeof(cplx), &d_out)) return -1;
  }
  LAUNCH_TRY(c3p_launch_kron((const cplx*)d_A, (const cplx*)d_B, n, Da, Db, which, (cplx*)d_out, st));
  if (flags & C3P_HOST_PTRS) return sg.finish();
  return 0;
}

int c3p_kron(const void* A, const void* Bm, int n, int Da, int Db, int flags, void* out, void* stream) {
  return kron_common(A, Bm, n, Da, Db, 0, flags, out, stream);
}

int c3p_superop(const void* A, int n, int D, int which, int flags, void* out, void* stream) {
  if (which < 0 || which > 2) return fail("bad superoperator kind %d", which);
  return kron_common(A, nullptr, n, D, D, which + 1, flags, out, stream);
}

}  // extern "C"

// ---- ODE state solvers: one call record (OdeCall), the route as a value (ode_route) and one launch (ode_launch) behind
// c3p_ode_solve, c3p_ode_solve_vjp and c3p_rk4_unitary ------------------------------------------------------------------------
namespace {
// One ODE call between its argument checks and its result: the workspace lock, the staging of host operands, the flags and the
// problem record the kernels take.
struct OdeCall {
  std::optional<WsLock> lk;
  DeviceWs* w = nullptr;
  hipStream_t st = nullptr;
  Stage sg{nullptr, nullptr};
  int flags = 0;
  OdeArgs a = {};

  bool host() const { return flags & C3P_HOST_PTRS; }
  int lock(int flags_, void* stream) {
    flags = flags_;
    st = (hipStream_t)stream;
    lk.emplace(st);
    w = lk->w;
    if (!w) return fail("no HIP device");
    if (!lk->ok) return fail("hipStreamWaitEvent on the previous call's stream failed");
    sg.w = w, sg.st = st;
    return 0;
  }
  // host pointers: the operands every entry takes, in slot order (each pointer becomes its staged copy)
  int stage_h(const void*& h0, const void*& hks, const void*& signals, int B, int K, int N, int D) {
    if (sg.in(h0, (size_t)D * D * sizeof(cplx), &h0)) return -1;
    if (sg.in(hks, (size_t)K * D * D * sizeof(cplx), &hks)) return -1;
    return sg.in(signals, (size_t)B * K * N * sizeof(double), &signals);
  }
  // the fields of the problem record every entry sets; the rest (states, want_all, hs, ...) stay zero for the entry to set
  void fill(const void* h0, const void* hks, const void* signals, const void* col_ops, const void* init, long init_bstride, double dt,
            int B, int K, int N, int D, int M, int C, int solver, int step, int n_steps, int u_stride) {
    a = {};
    a.h0 = (const cplx*)h0;
    a.hks = (const cplx*)hks;
    a.signals = (const double*)signals;
    a.col_ops = (const cplx*)col_ops;
    a.init = (const cplx*)init;
    a.init_bstride = init_bstride;
    a.dt = dt;
    a.B = B, a.K = K, a.N = N, a.D = D, a.M = M, a.C = C;
    a.solver = solver;
    a.step = step;
    a.n_steps = n_steps;
    a.u_stride = u_stride;
  }
  // The two solve entries: the checks they share (`own`: the vjp's extra ones, in their place), lock, staging of the operands they
  // share (SL_IN0 .. SL_IN4), fill.  0 = go on, 1 = nothing to do (B = 0), -1 = error.  The forward entry needs `states`, the vjp
  // `grad_signals` where K > 0.
  template <class Own>
  int open(bool vjp, Own&& own, const void* h0, const void* hks, const void* signals, const void* col_ops, int C, double dt, int B, int K,
           int N, int D, int solver, int step, const void* init, int64_t init_bstride, int flags_, const void* states,
           const void* grad_signals, void* stream) {
    if (B < 0 || N < 0 || D <= 0 || K < 0 || K > 32) return fail("bad sizes B=%d K=%d N=%d D=%d", B, K, N, D);
    if (solver < 0 || solver > 3) return fail("unknown solver id %d", solver);
    if (step < 0 || step > 2) return fail("unknown step function id %d", step);
    if (flags_ & C3P_COL_PER_SAMPLE)
      return fail("%s: C3P_COL_PER_SAMPLE is not served (one col_ops [C,D,D] for the batch)", vjp ? "c3p_ode_solve_vjp" : "c3p_ode_solve");
    if (B == 0) return 1;
    if (own()) return -1;
    if (N < 2) return fail("the ODE solver needs at least two time samples (N=%d)", N);
    if (!h0 || !init || (!vjp && !states)) return fail("NULL pointer argument");
    if (K > 0 && (!hks || !signals || (vjp && !grad_signals))) return fail("K > 0 but hks/signals%s missing", vjp ? "/grad_signals" : "");
    if (step == C3P_STEP_LINDBLAD && (!col_ops || C <= 0)) return fail("lindblad step needs col_ops");
    if (step != C3P_STEP_LINDBLAD) C = 0;
    const int M = (step == C3P_STEP_SCHRODINGER) ? 1 : D;
    if (lock(flags_, stream)) return -1;
    if (host()) {
      const size_t init_elems = init_bstride ? (size_t)(B - 1) * init_bstride + (size_t)D * M : (size_t)D * M;
      if (stage_h(h0, hks, signals, B, K, N, D)) return -1;
      if (sg.in(col_ops, (size_t)C * D * D * sizeof(cplx), &col_ops)) return -1;
      if (sg.in(init, init_elems * sizeof(cplx), &init)) return -1;
    }
    fill(h0, hks, signals, col_ops, init, init_bstride, dt, B, K, N, D, M, C, solver, step, N, 1);
    return 0;
  }
  int finish() { return host() ? sg.finish() : 0; }
};

// The step maps of nseg time segments of every sample, [B, nseg, D, D] in SL_SEG_A: each segment integrates the D columns of the
// identity (SL_CLP).  17 <= D <= 48: on the matrix-core kernel (propagator step: one product per stage), below on the lane rows.
int ode_segment_maps(DeviceWs* w, const OdeArgs& a, int nseg, OdeArgs* maps, hipStream_t st) {
  const int D = a.D;
  void *v_id, *v_maps;
  if (ws_get(w, SL_CLP, (size_t)D * D * sizeof(cplx), &v_id)) return -1;
  if (ws_get(w, SL_SEG_A, (size_t)a.B * nseg * D * D * sizeof(cplx), &v_maps)) return -1;
  HIP_TRY(c3p_launch_ode_identity((cplx*)v_id, D, st));
  OdeArgs& m = *maps = a;
  m.M = D;
  m.init = (const cplx*)v_id;
  m.init_bstride = 0;
  m.want_all = 0;
  m.seg_count = nseg;
  m.seg_len = (a.n_steps + nseg - 1) / nseg;
  m.states = (cplx*)v_maps;
  if (D > 16) {
    m.step = C3P_STEP_PROPAGATOR_ID;
    HIP_TRY(c3p_launch_ode_rhoq(m, st));
  } else {
    HIP_TRY(c3p_launch_ode_row(m, nullptr, st));
  }
  return 0;
}

// Segmented integration of a small batch, final state / propagator only.  The equations are linear, so the interval is cut into
// nseg time segments, the segment maps are multiplied in order by the chain kernel of their size and, for a vector state (M = 1),
// the product is applied to the initial state -- D x the arithmetic on nseg x D x the lanes.  M = D (rk4_unitary): the product is
// the result.
int ode_segmented(DeviceWs* w, const OdeArgs& a, int nseg, hipStream_t st) {
  const int D = a.D, B = a.B;
  void* v_U = a.M == 1 ? nullptr : a.states;
  if (!v_U && ws_get(w, SL_SCRATCH, (size_t)B * D * D * sizeof(cplx), &v_U)) return -1;
  OdeArgs m;
  if (ode_segment_maps(w, a, nseg, &m, st)) return -1;
  if (D > 16 ? combine_chain(c3p_launch_midd_chain, w, m.states, B, nseg, D, 0, nullptr, (cplx*)v_U, st)
             : combine_chain(c3p_launch_smalld_chain, w, m.states, B, nseg, D, 0, nullptr, (cplx*)v_U, st))
    return -1;
  if (a.M == 1) HIP_TRY(c3p_launch_ode_apply((const cplx*)v_U, a.init, a.init_bstride, a.states, B, D, st));
  return 0;
}

// Trajectory (want_all) of a small batch of Schroedinger states in time segments: the segment maps as above, the state at the
// start of every segment from them, then the B x nseg pieces of the trajectory side by side (one time segment per lane row; at
// 17 <= D <= 48 per wavefront of c3p_ode_rowq.hip).
int ode_trajectory_segmented(DeviceWs* w, const OdeArgs& a, int nseg, hipStream_t st) {
  const int D = a.D, B = a.B;
  void* v_st;
  if (ws_get(w, SL_SEG_B, (size_t)B * nseg * D * sizeof(cplx), &v_st)) return -1;
  OdeArgs m;
  if (ode_segment_maps(w, a, nseg, &m, st)) return -1;
  HIP_TRY(c3p_launch_ode_starts(m.states, a.init, a.init_bstride, (cplx*)v_st, B, nseg, D, st));
  OdeArgs t = a;
  t.init = (const cplx*)v_st;
  t.init_bstride = D;
  t.seg_count = nseg;
  t.seg_len = m.seg_len;
  t.seg_traj = 1;
  HIP_TRY(D > 16 ? c3p_launch_ode_rowq(t, st) : c3p_launch_ode_row(t, nullptr, st));
  return 0;
}

// Time segments for few samples at 17 <= D <= 48: one workgroup per (sample, segment) on the matrix-core kernel.  A sample alone
// keeps ONE CU busy for n_steps x ~5 us; S segments spread it over S CUs (the chip has 256), at the price of the ordered product of
// S maps (final state / propagator) or of the second pass over the pieces on the lane rows of c3p_ode_rowq.hip (`trajectory`).
// min_segments: how many segments the change has to offer at least.
int ode_mfma_segments(const OdeArgs& a0, bool trajectory, int min_segments) {
  if (c3p_opt_on(C3P_OPT_ode_no_seg)) return 0;
  if (a0.D < 17 || a0.D > 48 || (a0.want_all != 0) != trajectory || a0.reset_each_step || a0.transpose_out || a0.hs || a0.K > 4 || a0.n_steps < 64)
    return 0;
  int nig, nj, wd;
  if (trajectory ? a0.M != 1 || !c3p_ode_rowq_supported(a0)
                 : !c3p_midd_geometry(a0.D, &nig, &nj, &wd))  // (the ordered product of the maps runs on the mid-D chain kernel: D <= 40)
    return 0;
  OdeArgs a = a0;
  a.step = C3P_STEP_PROPAGATOR_ID;
  a.M = a.D;
  a.want_all = 0;
  a.seg_count = 2;
  if (!c3p_ode_rhoq_supported(a)) return 0;
  long S = 512 / a.B;
  if (S > a.n_steps / 16) S = a.n_steps / 16;
  if (S > 64) S = 64;
  return S >= min_segments ? (int)S : 0;
}

enum OdeRouteId {
  ODE_RT_ROW,        // lane-row kernels (c3p_ode_row.hip): one sample per 16-lane row, state and operator rows in registers
  ODE_RT_ROW_SEG,    // ... final state / propagator of a small batch in time segments (ode_segmented)
  ODE_RT_ROW_TRAJ,   // ... trajectory of a small batch in time segments (ode_trajectory_segmented)
  ODE_RT_ROW_OR_WG,  // lane rows for real operators, workgroup kernel for complex ones: the device decides
  ODE_RT_ROWQ,       // 17 <= D <= 48 vector states: several DPP rows per sample, operators in LDS (c3p_ode_rowq.hip)
  ODE_RT_RHOQ,       // 17 <= D <= 48 matrix states: register tiles + 16x16x4 fp64 MFMA products (c3p_ode_rhoq.hip)
  ODE_RT_MFMA_SEG,   // ... final state / propagator of few samples in time segments
  ODE_RT_MFMA_TRAJ,  // ... trajectory of few Schroedinger states in time segments
  ODE_RT_WG          // one workgroup per sample (c3p_ode.hip)
};
struct OdeRoute {
  OdeRouteId route;
  int nseg;
};

// Which kernel serves the problem: host arithmetic on the record and the option table.  Segments are for vector states (a state, or
// the D columns of rk4_unitary's propagator).  A state that would otherwise run on the lane rows of c3p_ode_rowq.hip pays 1.5x per
// step for becoming a matrix, so it needs four matrix-core segments; the propagator is a matrix already and takes two.  The
// matrix-core and the rowq kernel both take a propagator step (the former wins unless ode_prop_rows is set); for every other step
// at most one of them does (matrix states need M = D, rowq takes vector steps only).
OdeRoute ode_route(const OdeArgs& a) {
  const bool vec = a.step == C3P_STEP_SCHRODINGER || a.step == C3P_STEP_PROPAGATOR_ID;
  OdeRoute r = {ODE_RT_WG, 0};
  if (c3p_ode_row_supported(a)) {
    r.route = ODE_RT_ROW;
    if (vec && (r.nseg = c3p_ode_row_segments(a)) > 0) r.route = ODE_RT_ROW_SEG;
    else if (vec && (r.nseg = c3p_ode_row_traj_segments(a)) > 0) r.route = ODE_RT_ROW_TRAJ;
    // rho-valued states, more than four control lines, no collapse operators, a batch that leaves SIMDs idle on the lane rows
    // (one wave = four samples; measured crossover between 2048 and 16 384 samples, profiles/r04/ode_fallbacks.json): COMPLEX
    // operators run 1.1 - 1.3x faster on the workgroup kernel there, real ones 1.4 - 1.7x faster on the lane rows.
    else if (a.step == C3P_STEP_VON_NEUMANN && a.K > 4 && a.C == 0 && a.B <= 4096 && !c3p_opt_on(C3P_OPT_ode_no_split)) r.route = ODE_RT_ROW_OR_WG;
  } else if (vec && (r.nseg = ode_mfma_segments(a, true, 4)) > 0) {
    r.route = ODE_RT_MFMA_TRAJ;
  } else if (vec && (r.nseg = ode_mfma_segments(a, false, a.M == 1 ? 4 : 2)) > 0) {
    r.route = ODE_RT_MFMA_SEG;
  } else if (c3p_ode_rhoq_supported(a)) {
    r.route = ODE_RT_RHOQ;
  } else if (c3p_ode_rowq_supported(a)) {
    r.route = ODE_RT_ROWQ;
  }
  // (ROW_OR_WG: the host cannot know which of the two did the work -- a distinct id, so that profiles do not book a workgroup-kernel
  // run on the lane rows; MFMA_TRAJ: the pieces, the longer pass, run on the lane rows)
  static const int kernel[] = {C3P_KERNEL_ODE_ROW, C3P_KERNEL_ODE_ROW, C3P_KERNEL_ODE_ROW, C3P_KERNEL_ODE_ROW_OR_WG, C3P_KERNEL_ODE_ROW,
                               C3P_KERNEL_ODE_MFMA, C3P_KERNEL_ODE_MFMA, C3P_KERNEL_ODE_ROW, C3P_KERNEL_ODE_WG};
  g_last_kernel = kernel[r.route];
  return r;
}

// the workgroup kernel's per-sample scratch: LDS up to 150 KiB, beyond it SL_SCRATCH
int ode_wg_scratch(DeviceWs* w, OdeArgs& a, bool* global) {
  const size_t elems = c3p_ode_elems(a.D, a.M, a.C);
  *global = elems * sizeof(cplx) > (size_t)(150 * 1024);
  if (!*global) return 0;
  void* v;
  if (ws_get(w, SL_SCRATCH, (size_t)a.B * elems * sizeof(cplx), &v)) return -1;
  a.scratch = (cplx*)v;
  a.scratch_stride = (long)elems;
  return 0;
}

int ode_launch_pass(OdeCall& c, OdeArgs a, OdeRoute r) {
  DeviceWs* w = c.w;
  hipStream_t st = c.st;
  bool global = false;
  switch (r.route) {
    case ODE_RT_ROW:
    case ODE_RT_ROW_OR_WG: {
      void* aux = nullptr;
      if (a.C > 0 && ws_get(w, SL_TABLES, c3p_ode_row_aux_bytes(a.D, a.C), &aux)) return -1;
      // both kernels look at the operators and one of them leaves at once, as regr_prep_kernel does for the PWC path; the second
      // launch -- B workgroups of 256 threads that leave at once for real operators -- is paid on every such call
      a.complex_to_wg = r.route == ODE_RT_ROW_OR_WG;
      HIP_TRY(c3p_launch_ode_row(a, aux, st));
      if (r.route == ODE_RT_ROW) return 0;
      a.complex_to_wg = 0;
      a.wg_if_complex = 1;
      if (ode_wg_scratch(w, a, &global)) return -1;
      HIP_TRY(c3p_launch_ode(a, global, st));
      return 0;
    }
    case ODE_RT_ROW_SEG:
    case ODE_RT_MFMA_SEG: return ode_segmented(w, a, r.nseg, st);
    case ODE_RT_ROW_TRAJ:
    case ODE_RT_MFMA_TRAJ: return ode_trajectory_segmented(w, a, r.nseg, st);
    case ODE_RT_ROWQ: HIP_TRY(c3p_launch_ode_rowq(a, st)); return 0;
    case ODE_RT_RHOQ: HIP_TRY(c3p_launch_ode_rhoq(a, st)); return 0;
    case ODE_RT_WG:
      if (ode_wg_scratch(w, a, &global)) return -1;
      HIP_TRY(c3p_launch_ode(a, global, st));
      return 0;
  }
  return fail("internal: unknown ODE route %d", (int)r.route);
}

// The launches of a routed call inside the timing event pair.  per_step (rk4_unitary's dUs, [B,n_steps,D,D]): a second pass on the
// same kernel that restarts from the identity after every step and stores the per-step propagators transposed; never segmented.
int ode_launch(OdeCall& c, const OdeArgs& a, OdeRoute r, cplx* per_step = nullptr) {
  if (record_start(c.w, c.st)) return -1;
  if (ode_launch_pass(c, a, r)) return -1;
  if (per_step) {
    OdeArgs p = a;
    p.want_all = 1;
    p.reset_each_step = 1;
    p.transpose_out = 1;
    p.states = per_step;
    const OdeRouteId whole = r.route == ODE_RT_ROW_SEG ? ODE_RT_ROW : r.route == ODE_RT_MFMA_SEG ? ODE_RT_RHOQ : r.route;
    if (ode_launch_pass(c, p, {whole, 0})) return -1;
  }
  return record_stop(c.w, c.st);
}
}  // namespace

extern "C" {

int c3p_ode_solve(const void* h0, const void* hks, const double* signals, const void* col_ops,
                  int C, double dt, int B, int K, int N, int D, int solver, int step,
                  const void* init, int64_t init_bstride, int want_all, int flags, void* states,
                  void* stream) {
  OdeCall c;
  const int rc = c.open(false, [] { return 0; }, h0, hks, signals, col_ops, C, dt, B, K, N, D, solver, step, init, init_bstride, flags,
                        states, nullptr, stream);
  if (rc) return rc < 0 ? -1 : 0;
  OdeArgs& a = c.a;
  const size_t cs = sizeof(cplx);
  void* d_states = states;
  if (c.host() && c.sg.out(states, (size_t)B * (want_all ? N : 1) * D * a.M * cs, &d_states)) return -1;
  a.want_all = want_all ? 1 : 0;
  a.states = (cplx*)d_states;
  if (K > 4 && D <= 16 && step == C3P_STEP_SCHRODINGER && !c3p_opt_on(C3P_OPT_ode_wg)) {
    // more than four control lines, vector states: the lane-row kernels hold the rows of four operators in registers; H is
    // assembled for every sample index first (B N D^2 numbers) and the kernel interpolates it between consecutive samples --
    // the same linear interpolation, taken after the sum instead of before it.  Beyond 8 GB, and for rho-valued states (no
    // faster there), the workgroup kernel takes the call.
    const size_t hb = (size_t)B * N * D * D * cs;
    if (hb <= ((size_t)8 << 30)) {
      void* hv;
      if (ws_get(c.w, SL_SEG_F, hb, &hv)) return -1;
      HIP_TRY(c3p_launch_ode_assemble_hs(a, (cplx*)hv, c.st));
      a.hs = (const cplx*)hv;
      a.hs_bstride = (long)N * D * D;
      a.hs_lerp = 1;
      if (!c3p_ode_row_supported(a)) {  // (stage slots beyond the LDS: the workgroup kernel assembles H itself)
        a.hs = nullptr;
        a.hs_bstride = 0;
        a.hs_lerp = 0;
      }
    }
  }
  if (ode_launch(c, a, ode_route(a))) return -1;
  return c.finish();
}

int c3p_ode_solve_vjp(const void* h0, const void* hks, const double* signals, const void* col_ops, int C, double dt, int B, int K,
                      int N, int D, int solver, int step, const void* init, int64_t init_bstride, const void* states_bar,
                      int bar_all, const void* target, int64_t target_bstride, int flags, double* grad_signals, void* init_bar,
                      double* infid_out, void* final_out, void* stream) {
  OdeCall c;
  const int rc = c.open(true, [&] {
        if ((states_bar != nullptr) == (target != nullptr)) return fail("exactly one of states_bar and target must be given");
        if (target && bar_all) return fail("bar_all needs states_bar");
        if (init_bstride < 0 || target_bstride < 0) return fail("negative stride");
        return 0;
      }, h0, hks, signals, col_ops, C, dt, B, K, N, D, solver, step, init, init_bstride, flags, nullptr, grad_signals, stream);
  if (rc) return rc < 0 ? -1 : 0;
  const int M = c.a.M;
  const size_t cs = sizeof(cplx);
  const void *d_bar = states_bar, *d_tgt = target;
  void *d_grad = grad_signals, *d_ib = init_bar, *d_inf = infid_out, *d_fin = final_out;
  const size_t state_bytes = (size_t)B * D * M * cs;
  if (c.host()) {
    const size_t tgt_elems = target_bstride ? (size_t)(B - 1) * target_bstride + (size_t)D : (size_t)D;
    if (states_bar && c.sg.in(states_bar, state_bytes * (bar_all ? (size_t)N : 1), &d_bar)) return -1;
    if (target && c.sg.in(target, tgt_elems * cs, &d_tgt)) return -1;
    if (c.sg.out(grad_signals, (size_t)B * K * N * sizeof(double), &d_grad)) return -1;
    if (c.sg.out(init_bar, state_bytes, &d_ib)) return -1;
    if (c.sg.out(infid_out, (size_t)B * sizeof(double), &d_inf)) return -1;
    if (c.sg.out(final_out, state_bytes, &d_fin)) return -1;
  }
  const OdeVjpPlan pl = c3p_ode_vjp_plan(B, K, N, D, M, c.a.C, step);
  OdeVjpArgs v = {};
  v.f = c.a;
  v.states_bar = (const cplx*)d_bar;
  v.bar_all = bar_all ? 1 : 0;
  v.target = (const cplx*)d_tgt;
  v.target_bstride = (long)target_bstride;
  v.grad_signals = (double*)d_grad;
  v.init_bar = (cplx*)d_ib;
  v.infid = (double*)d_inf;
  v.final_out = (cplx*)d_fin;
  v.Cint = pl.Cint;
  v.nck = pl.nck;
  v.rows = pl.rows;
  // (the lane-row grid is rounded up to whole wavefronts of four rows: every launched row has its own checkpoints)
  const size_t ws_rows = pl.row ? (size_t)((pl.rows + 3) / 4) * 4 : (size_t)pl.rows;
  const size_t ws_bytes = ws_rows * pl.ws_elems * cs;
  void* ws;
  if (ws_get(c.w, SL_ODE_VJP_WS, ws_bytes, &ws)) return -1;
  v.ws = (cplx*)ws;
  v.ws_stride = (long)pl.ws_elems;
  if (!pl.row && pl.wg_global) {
    void* sc;
    if (ws_get(c.w, SL_SCRATCH, (size_t)pl.rows * pl.wg_elems * cs, &sc)) return -1;
    v.scratch = (cplx*)sc;
    v.scratch_stride = (long)pl.wg_elems;
  }
  g_last_kernel = C3P_KERNEL_ODE_VJP;
  g_note_plan = "checkpoint interval C=" + std::to_string(pl.Cint) + " checkpoints=" + std::to_string(pl.nck) + " workspace=" +
                std::to_string(ws_bytes) + " bytes (cap " + std::to_string((size_t)C3P_ODE_VJP_WS_CAP) + ") rows=" +
                std::to_string(pl.rows);
  if (record_start(c.w, c.st)) return -1;
  HIP_TRY(c3p_launch_ode_vjp(v, pl, c.st));
  if (record_stop(c.w, c.st)) return -1;
  return c.finish();
}

int c3p_rk4_unitary(const void* h0, const void* hks, const double* signals, const void* hs,
                    int64_t hs_bstride, double dt, int B, int K, int Ns, int D, int flags,
                    void* U_out, void* dUs_out, void* stream) {
  if (B < 0 || Ns < 0 || D <= 0 || K < 0 || K > 32) return fail("bad sizes B=%d K=%d Ns=%d D=%d", B, K, Ns, D);
  if (B == 0) return 0;
  if (Ns < 3) return fail("rk4_unitary needs at least three Hamiltonian samples (Ns=%d)", Ns);
  if (!U_out) return fail("U_out is NULL");
  if (!hs && (!h0 || (K > 0 && (!hks || !signals)))) return fail("NULL Hamiltonian input");
  const int n_steps = (Ns - 1) / 2;  // range(0, len(h) - 2, 2), propagation.py:79,251
  const size_t cs = sizeof(cplx);
  OdeCall c;
  if (c.lock(flags, stream)) return -1;
  const void *d_sig = signals, *d_hs = hs;
  void *d_U = U_out, *d_dUs = dUs_out;
  if (c.host()) {
    if (hs) {
      const size_t one = (size_t)Ns * D * D;
      if (c.sg.in(hs, (hs_bstride ? (size_t)(B - 1) * hs_bstride + one : one) * cs, &d_hs)) return -1;
    } else if (c.stage_h(h0, hks, d_sig, B, K, Ns, D)) {
      return -1;
    }
    if (c.sg.out(U_out, (size_t)B * D * D * cs, &d_U)) return -1;
    if (c.sg.out(dUs_out, dUs_out ? (size_t)B * n_steps * D * D * cs : 0, &d_dUs)) return -1;
  }
  // identity initial state, shared by all samples
  void* v_id;
  if (ws_get(c.w, SL_CLP, (size_t)D * D * cs, &v_id)) return -1;
  HIP_TRY(c3p_launch_ode_identity((cplx*)v_id, D, c.st));  // (on the device: no host round trip, capturable)
  c.fill(h0, hks, d_sig, nullptr, v_id, 0, dt, B, hs ? 0 : K, Ns, D, D, 0, C3P_SOLVER_RK4, C3P_STEP_PROPAGATOR_ID, n_steps, 2);
  c.a.hs = (const cplx*)d_hs;
  c.a.hs_bstride = hs_bstride;
  c.a.states = (cplx*)d_U;
  // every column of the propagator is an independent Schroedinger problem (lane rows: B x D vector states; few gates: time
  // segments fill the chip); the per-step propagators come from a second pass
  if (ode_launch(c, c.a, ode_route(c.a), (cplx*)d_dUs)) return -1;
  return c.finish();
}

int c3p_gate_overlap(const void* U, int B, int D, const int32_t* comp_rows, int L, const void* ideal,
                     int flags, void* overlap_out, void* stream) {
  if (B < 0 || D <= 0 || L <= 0 || L > D) return fail("bad sizes B=%d D=%d L=%d", B, D, L);
  if (B == 0) return 0;
  if (!U || !comp_rows || !ideal || !overlap_out) return fail("NULL pointer argument");
  const size_t cs = sizeof(cplx);
  hipStream_t st = (hipStream_t)stream;
  WsLock lk(st);
  DeviceWs* w = lk.w;
  if (!w) return fail("no HIP device");
  if (!lk.ok) return fail("hipStreamWaitEvent on the previous call's stream failed");
  Stage sg{w, st};
  const void *d_U = U, *d_rows = comp_rows, *d_G = ideal;
  void* d_out = overlap_out;
  if (flags & C3P_HOST_PTRS) {
    for (int a = 0; a < L; ++a)
      if (comp_rows[a] < 0 || comp_rows[a] >= D) return fail("comp_rows[%d]=%d outside [0,%d)", a, comp_rows[a], D);
    if (sg.in(U, (size_t)B * D * D * cs, &d_U)) return -1;
    if (sg.in(comp_rows, (size_t)L * sizeof(int32_t), &d_rows)) return -1;
    if (sg.in(ideal, (size_t)L * L * cs, &d_G)) return -1;
    if (sg.out(overlap_out, (size_t)B * cs, &d_out)) return -1;
  }
  LAUNCH_TRY(c3p_launch_overlap((const cplx*)d_U, B, D, (const int*)d_rows, L, (const cplx*)d_G, (cplx*)d_out, st));
  if (flags & C3P_HOST_PTRS) return sg.finish();
  return 0;
}

// The general-generator sweep in three VALU kernels on dense generator tables (c3p_grad.hip, general form), D^2 <= 36, one chunk
// of samples.  `mo` set: the sweep also accumulates the model-operator cotangents, and the reduce kernel writes them.
static int run_vjp_lind_valu(DeviceWs* w, const PwcProblem& P, const cplx* ub, double* grad, const LindModelOut* mo, bool* global_out,
                             hipStream_t st) {
  const size_t cs = sizeof(cplx);
  const int nb = P.B, K = P.K, N = P.N, D = P.D, Dm = P.Dm;
  const long gsz = (long)Dm * Dm;
  const int nt = P.nsamp();
  void* tab;
  if (ws_get(w, SL_TABLES, (size_t)nt * (K + 1) * gsz * cs, &tab)) return -1;
  LAUNCH_TRY(c3p_launch_lind_generators(P.h0, P.h0_bs, P.hks, P.hk_bs, P.clp, P.clp_bs, nt, K, D, (cplx*)tab, st));
  GradArgs A = {};
  A.h0 = (const cplx*)tab;
  A.h0_bstride = nt > 1 ? (long)(K + 1) * gsz : 0;
  A.hks = (const cplx*)tab + gsz;
  A.hks_bstride = A.h0_bstride;
  A.signals = P.signals;
  A.dt = P.dt;
  A.grad = grad;
  const long S = valu_grad_segments(nb, N);
  void *sv, *mv, *v;
  SweepStore ss;
  if (ws_get(w, SL_SEG_A, (size_t)nb * S * gsz * cs, &sv)) return -1;
  if (ws_get(w, SL_SEG_B, (size_t)nb * S * gsz * cs, &mv)) return -1;
  if (get_sweep_store(w, SL_OUT1, nb, S, N, Dm, false, &ss)) return -1;  // (SL_OUT0 stages grad_signals)
  fill_general_scan(A, nb, K, N, Dm, S, (cplx*)sv, (cplx*)mv, ss.pre, ub, P.fr_phase);
  A.pstore = ss.pstore;
  const bool global = c3p_grad_lds_bytes_general(Dm) > 150 * 1024;
  *global_out = global;
  if (global) {
    A.scratch_stride = (long)C3P_GRAD_NMAT_GENERAL * A.ld * Dm;
    if (ws_get(w, SL_SCRATCH, (size_t)nb * A.S * A.scratch_stride * cs, &v)) return -1;
    A.scratch = (cplx*)v;
  }
  if (mo) {
    if (ws_get(w, SL_LMODEL_PART, (size_t)nb * A.S * ((size_t)gsz + (size_t)(K + 1) * Dm) * cs, &v)) return -1;
    A.mpart = (cplx*)v;
    A.Dsys = D;
  }
  LAUNCH_TRY(c3p_launch_grad_seg(A, global, st));
  LAUNCH_TRY(c3p_launch_grad_scan_general(A, global, st));
  if (!mo) {
    LAUNCH_TRY(c3p_launch_grad_bwd_general(A, global, st));
    return 0;
  }
  LAUNCH_TRY(c3p_launch_grad_bwd_general_model(A, global, st));
  LAUNCH_TRY(c3p_launch_lind_model_reduce(A.mpart, mo->col, mo->col_bs, mo->C, nb, A.S, K, D, P.dt, mo->g_h0, mo->g_hks, mo->g_col, st));
  return 0;
}

int c3p_pwc_lindblad_vjp(const void* h0, int64_t h0_bstride, const void* hks, int64_t hks_bstride, const double* signals,
                         const void* col_ops, int C, double dt, int B, int K, int N, int D, int flags, const double* fr_phase,
                         const void* U_bar, double* grad_signals, void* stream) {
  LindGradCall c;
  const int rc0 = c.open("c3p_pwc_lindblad_vjp", C3P_PER_SLICE_H | C3P_ORDER_RIGHT, false, [] { return 0; }, h0, h0_bstride, hks, hks_bstride,
                         signals, col_ops, C, dt, B, K, N, D, flags, fr_phase, U_bar, grad_signals, nullptr, nullptr, nullptr, stream);
  if (rc0) return rc0 < 0 ? -1 : 0;
  DeviceWs* w = c.w;
  hipStream_t st = c.st;
  const int Dm = c.P.Dm;
  // The general-generator sweeps keep the slice propagators and the prefix of every slice: 2 N D^4 complex per sample.  Large
  // batches are processed in chunks of samples that keep that below 24 GB (C3P_GRAD_CHUNK overrides the chunk size).
  const size_t general_store = 2 * (size_t)N * Dm * Dm * sizeof(cplx);
  const bool on_chip = c.on_chip();
  if (Dm <= kSmallDLimit && c3p_smalld_supported(Dm) && K <= 8 && on_chip) {
    // superoperators up to 12 x 12 (D <= 3): the general-generator sweep on the small-D matrix-core kernels
    const int rc = c.family(general_store, C3P_KERNEL_SMALLD, [&](const PwcProblem& Pc, const cplx* ub, double* g, long) {
      return run_vjp_lind_smalld(w, Pc, ub, g, (flags & C3P_HERMITIAN_H) != 0, st);
    });
    if (rc != 1) return rc;
  }
  if (D == 4 && (flags & C3P_HERMITIAN_H) && K <= 8 && on_chip && !c3p_opt_on(C3P_OPT_no_smallr)) {
    // two qubits with declared Hermitian Hamiltonians: the real Hermitian-basis kernels of c3p_smallr.hip, both halves
    const int rc = c.family(general_store, C3P_KERNEL_MFMA,
                            [&](const PwcProblem& Pc, const cplx* ub, double* g, long) { return run_vjp_lind_smallr16(w, Pc, ub, g, st); });
    if (rc != 1) return rc;
  }
  // 49 x 49 .. 81 x 81 superoperators (D = 7, 8, 9; cfg4) and, zero padded in the 49 class, 36 x 36 (D = 6): on-chip backward sweep in
  // the Hermitian basis, real arithmetic; the transposed local prefix of every slice (N D^4 doubles per sample) is kept in HBM:
  // chunks of samples below the budget.  1 = a Hamiltonian is not Hermitian (the caller goes on to the complex sweeps).
  auto try_regr = [&]() -> int {
    return c.family((size_t)N * Dm * Dm * sizeof(double), C3P_KERNEL_MFMA, [&](const PwcProblem& Pc, const cplx* ub, double* g, long b0) {
      const int rc = run_vjp_lind_regr(w, Pc, ub, g, st);
      if (rc == 1 && b0 > 0) return fail("internal: the Hermitian-basis sweep declined a later chunk");
      return rc;
    });
  };
  const bool regr_ok = lind_regr_grad_ok(D, Dm) && on_chip && !c3p_opt_on(C3P_OPT_no_hermitian_basis);
  if (regr_ok && D == 6) {
    const int rc = try_regr();
    if (rc != 1) return rc;
  }
  if (Dm >= 13 && Dm <= 36 && on_chip) {
    // 16 x 16 .. 36 x 36 superoperators (D = 4, 5, 6): the same sweep on the mid-D matrix-core kernels
    const int rc = c.family(general_store, C3P_KERNEL_MFMA,
                            [&](const PwcProblem& Pc, const cplx* ub, double* g, long) { return run_vjp_lind_midd(w, Pc, ub, g, st); });
    if (rc != 1) return rc;
  }
  if (Dm <= 36 && !c3p_opt_on(C3P_OPT_tiled_grad)) {
    // the same sweep in three VALU kernels on dense generator tables (c3p_grad.hip, general form): fallback and second opinion
    bool global = false;
    const int rc = c.chunks(general_store, [&](const PwcProblem& Pc, const cplx* ub, double* g, long) {
      return run_vjp_lind_valu(w, Pc, ub, g, nullptr, &global, st);
    });
    if (rc != 0) return -1;
    return c.served(global ? C3P_KERNEL_GENERIC_GLOBAL : C3P_KERNEL_GENERIC_LDS);
  }
  if (regr_ok && D != 6) {
    const int rc = try_regr();
    if (rc != 1) return rc;
  }
  if (record_start(w, st)) return -1;
  if (run_vjp_tiled(w, c.P, c.ubar, c.grad, st)) return -1;
  return c.served(C3P_KERNEL_MFMA);
}

int c3p_pwc_lindblad_model_vjp(const void* h0, int64_t h0_bstride, const void* hks, int64_t hks_bstride, const double* signals,
                               const void* col_ops, int C, double dt, int B, int K, int N, int D, int flags, const double* fr_phase,
                               const void* U_bar, double* grad_signals, void* grad_h0, void* grad_hks, void* grad_col_ops, void* stream) {
  LindGradCall c;
  auto own = [&]() -> int {
    if (D > 6)
      return fail("c3p_pwc_lindblad_model_vjp: D=%d, the model-operator cotangents of the Lindblad path are served for D <= 6 "
                  "(superoperators up to 36 x 36); c3p_pwc_lindblad_model_vjp_hb serves D = 7, 8, 9 for Hermitian Hamiltonians", D);
    return 0;
  };
  const int rc0 = c.open("c3p_pwc_lindblad_model_vjp", C3P_PER_SLICE_H | C3P_ORDER_RIGHT, true, own, h0, h0_bstride, hks, hks_bstride, signals,
                         col_ops, C, dt, B, K, N, D, flags, fr_phase, U_bar, grad_signals, grad_h0, grad_hks, grad_col_ops, stream);
  if (rc0) return rc0 < 0 ? -1 : 0;
  bool global = false;
  // chunks of samples as in c3p_pwc_lindblad_vjp: the sweep keeps 2 N D^4 complex per sample
  const int rc = c.chunks(2 * (size_t)N * c.P.Dm * c.P.Dm * sizeof(cplx), [&](const PwcProblem& Pc, const cplx* ub, double* g, long b0) {
    const LindModelOut mc = c.mo.at(c.P, b0);
    return run_vjp_lind_valu(c.w, Pc, ub, g, &mc, &global, c.st);
  });
  if (rc != 0) return -1;
  return c.served(global ? C3P_KERNEL_GENERIC_GLOBAL : C3P_KERNEL_GENERIC_LDS);
}

// The model-operator cotangents at D = 7, 8, 9 (and D = 6 under regr_grad_d6) from the Hermitian-basis sweep: the sweep of
// c3p_pwc_lindblad_vjp with the sums of the real generator cotangents kept per chain (c3p_regrg.hip).
int c3p_pwc_lindblad_model_vjp_hb(const void* h0, int64_t h0_bstride, const void* hks, int64_t hks_bstride, const double* signals,
                                  const void* col_ops, int C, double dt, int B, int K, int N, int D, int flags, const double* fr_phase,
                                  const void* U_bar, double* grad_signals, void* grad_h0, void* grad_hks, void* grad_col_ops,
                                  void* stream) {
  LindGradCall c;
  const int Dm = D * D;
  auto own = [&]() -> int {
    if (!lind_regr_grad_ok(D, Dm))
      return fail("c3p_pwc_lindblad_model_vjp_hb: D=%d, the Hermitian-basis sweep serves D = 7, 8, 9 (D = 6 under regr_grad_d6); "
                  "c3p_pwc_lindblad_model_vjp serves D <= 6", D);
    if (K > 16) return fail("c3p_pwc_lindblad_model_vjp_hb: K=%d, the Hermitian-basis sweep serves 1 <= K <= 16", K);
    return 0;
  };
  const int rc0 = c.open("c3p_pwc_lindblad_model_vjp_hb", C3P_PER_SLICE_H | C3P_ORDER_RIGHT | C3P_FORCE_GENERIC, true, own, h0, h0_bstride, hks,
                         hks_bstride, signals, col_ops, C, dt, B, K, N, D, flags, fr_phase, U_bar, grad_signals, grad_h0, grad_hks, grad_col_ops, stream);
  if (rc0) return rc0 < 0 ? -1 : 0;
  // chunks of samples as in c3p_pwc_lindblad_vjp: the transposed prefixes (N D^4 doubles per sample) and the sums of the generator
  // cotangents (S (1 + K) D^4 doubles per sample, S <= 32)
  const size_t per_sample = ((size_t)N + (size_t)32 * (1 + K)) * Dm * Dm * sizeof(double);
  const int rc = c.chunks(per_sample, [&](const PwcProblem& Pc, const cplx* ub, double* g, long b0) {
    const LindModelOut mc = c.mo.at(c.P, b0);
    const int rc = run_vjp_lind_regr(c.w, Pc, ub, g, c.st, &mc);
    if (rc == 1)
      return fail("c3p_pwc_lindblad_model_vjp_hb: h0 / hks must be Hermitian (the generator is not real in the Hermitian basis)");
    return rc;
  });
  if (rc != 0) return -1;
  return c.served(C3P_KERNEL_MFMA);
}

// ---- open-system evaluation from ONE forward pass: a caller-owned tape between c3p_pwc_lindblad_taped and its vjp ----
size_t c3p_pwc_lindblad_tape_bytes(int B, int K, int N, int D, int* segments_out) {
  const LindTapePlan plan = lind_tape_plan(B, K, N, D);
  if (segments_out) *segments_out = plan.segments;
  return plan.bytes;
}

int c3p_pwc_lindblad_taped(const void* h0, int64_t h0_bstride, const void* hks, int64_t hks_bstride, const double* signals,
                           const void* col_ops, int C, double dt, int B, int K, int N, int D, int flags, const double* fr_phase,
                           void* U_out, void* tape, size_t tape_bytes, int segments, void* stream) {
  if (flags & C3P_COL_PER_SAMPLE)
    return fail("c3p_pwc_lindblad_taped: C3P_COL_PER_SAMPLE is not served (one col_ops [C,D,D] for the batch; c3p_pwc_lindblad and "
                "c3p_pwc_lindblad_vjp take it)");
  if (flags & ~C3P_HERMITIAN_H) return fail("c3p_pwc_lindblad_taped takes device pointers and no flags but C3P_HERMITIAN_H");
  if (B <= 0 || K < 1 || K > 16 || N <= 0 || D <= 0) return fail("bad sizes B=%d K=%d N=%d D=%d", B, K, N, D);
  const int Dm = D * D;
  if (!h0 || !hks || !signals || !col_ops || C <= 0 || !U_out || !tape) return fail("NULL pointer argument");
  if (h0_bstride < 0 || hks_bstride < 0) return fail("negative batch stride");
  if (segments < 1 || segments > N) return fail("bad segment count %d", segments);
  if (D > 4 && !c3p_regr_supported(D, Dm)) return fail("the taped Lindblad evaluation serves D = 2, 3, 4 (small-D tile kernels) and D = 7, 8, 9 (Hermitian-basis kernels), got D=%d", D);
  // the segment count is the library's choice (c3p_pwc_lindblad_tape_bytes): the chain, scan and backward kernels are tuned and
  // tested for that range only, and the tape layout follows from it
  const LindTapePlan plan = lind_tape_plan(B, K, N, D);
  if (plan.family == TAPE_NONE || plan.segments != segments)
    return fail("taped Lindblad evaluation: shape not served or segment count %d != %d (c3p_pwc_lindblad_tape_bytes)", segments, plan.segments);
  if (tape_bytes < plan.bytes) return fail("tape too small: %zu bytes, need %zu (c3p_pwc_lindblad_tape_bytes)", tape_bytes, plan.bytes);
  hipStream_t st = (hipStream_t)stream;
  WsLock lk(st);
  DeviceWs* w = lk.w;
  if (!w) return fail("no HIP device");
  if (!lk.ok) return fail("hipStreamWaitEvent on the previous call's stream failed");
  const size_t cs = sizeof(cplx);
  void* clp;
  if (ws_get(w, SL_CLP, (size_t)Dm * Dm * cs, &clp)) return -1;
  LAUNCH_TRY(c3p_launch_clp((const cplx*)col_ops, C, D, 1, (cplx*)clp, st));
  const PwcProblem P = {(const cplx*)h0, h0_bstride, (const cplx*)hks, hks_bstride, signals, (const cplx*)clp, 0, dt, B, K, N, D, Dm, 1, fr_phase};
  if (plan.family != TAPE_REGR) {
    // small-D kernels: the forward half of run_vjp_lind_smalld writes into the tape, U = the ordered product of its segments
    if (lind_smallr_ok((flags & C3P_HERMITIAN_H) != 0, D, Dm, K, N, segments)) {
      // declared Hermitian: the tape holds the REAL tables, segment products and slice propagators (c3p_pwc_lindblad_vjp_taped
      // must be given the same flag); U from the complex copies of the segment products
      const int nsamp = P.nsamp();
      const LindSmallRBufs rb = lind_smallr_carve(tape, lind_smallr_sizes(B, K, N, Dm, segments, nsamp), nsamp, Dm, K);
      void* sc;
      if (ws_get(w, SL_OUT2, (size_t)B * segments * Dm * Dm * cs, &sc)) return -1;
      if (record_start(w, st)) return -1;
      if (lind_smallr_forward(rb, P, segments, (cplx*)sc, st)) return -1;
      if (record_stop(w, st)) return -1;
      g_last_kernel = Dm > 12 ? C3P_KERNEL_MFMA : C3P_KERNEL_SMALLD;
      const int rc = Dm > 12 ? combine_chain(c3p_launch_midd_chain, w, (const cplx*)sc, B, segments, Dm, 0, fr_phase, (cplx*)U_out, st)
                             : combine_chain(c3p_launch_smalld_chain, w, (const cplx*)sc, B, segments, Dm, 0, fr_phase, (cplx*)U_out, st);
      return rc ? -1 : 0;
    }
    if (D == 4) return fail("the taped Lindblad evaluation at D = 4 runs in the Hermitian basis: declare the Hamiltonians Hermitian (C3P_HERMITIAN_H) or use the untaped pair");
    const LindSmallBufs bf = lind_small_carve(tape, lind_small_sizes(B, K, N, Dm, segments, B));
    if (record_start(w, st)) return -1;
    if (lind_small_forward(w, bf, P, segments, (flags & C3P_HERMITIAN_H) != 0, st)) return -1;
    if (record_stop(w, st)) return -1;
    g_last_kernel = C3P_KERNEL_SMALLD;
    if (segments == 1) {
      HIP_TRY(hipMemcpyAsync(U_out, bf.seg, (size_t)B * Dm * Dm * cs, hipMemcpyDeviceToDevice, st));
      if (fr_phase) LAUNCH_TRY(c3p_launch_rowphase((cplx*)U_out, fr_phase, B, Dm, st));
      return 0;
    }
    return combine_chain(c3p_launch_smalld_chain, w, bf.seg, B, segments, Dm, 0, fr_phase, (cplx*)U_out, st) ? -1 : 0;
  }
  const LindRegrBufs bf = lind_regr_carve(tape, lind_regr_sizes(B, K, N, Dm, segments, B));
  if (record_start(w, st)) return -1;
  const int rc = lind_regr_forward(w, bf, P, segments, st);
  if (rc < 0) return -1;
  if (rc == 1) return fail("a Hamiltonian is not Hermitian: its Lindblad generator is complex in the Hermitian basis (use c3p_pwc_lindblad and c3p_pwc_lindblad_vjp)");
  if (record_stop(w, st)) return -1;
  g_last_kernel = C3P_KERNEL_MFMA;
  // U: the segment products back in the reference's vectorisation (a copy: the tape keeps the real ones), ordered combine
  const bool per_sample = P.per_sample();
  const long S = segments;
  cplx* segc = (cplx*)U_out;
  if (S > 1) {
    void* sv;
    if (ws_get(w, SL_SEG_A, (size_t)B * S * Dm * Dm * cs, &sv)) return -1;
    segc = (cplx*)sv;
  }
  HIP_TRY(hipMemcpyAsync(segc, bf.seg, (size_t)B * S * Dm * Dm * cs, hipMemcpyDeviceToDevice, st));
  LAUNCH_TRY(c3p_launch_hb_to_complex(segc, (long)B * S, (int)S, bf.flag_f, per_sample ? 1 : 0, K, D, st));
  if (S == 1 && fr_phase) LAUNCH_TRY(c3p_launch_rowphase((cplx*)U_out, fr_phase, B, Dm, st));
  if (S > 1) {
    ChainArgs c = {};
    c.mode = C3P_MODE_GIVEN;
    c.mats = segc;
    c.B = B;
    c.N = (int)S;
    c.D = D;
    c.Dm = Dm;
    c.fr_phase = fr_phase;
    const int keep = g_last_kernel;
    const int rc2 = run_chain_generic(w, c, (cplx*)U_out, st, /*profile=*/false);
    g_last_kernel = keep;
    if (rc2) return -1;
  }
  return 0;
}

int c3p_pwc_lindblad_vjp_taped(const void* tape, size_t tape_bytes, int segments, int per_sample_operators, const double* signals, int B,
                               int K, int N, int D, int flags, const double* fr_phase, const void* U_bar, double* grad_signals,
                               void* stream) {
  if (flags & C3P_COL_PER_SAMPLE) return fail("c3p_pwc_lindblad_vjp_taped: C3P_COL_PER_SAMPLE is not served (c3p_pwc_lindblad_vjp takes it)");
  if (flags & ~C3P_HERMITIAN_H) return fail("c3p_pwc_lindblad_vjp_taped takes device pointers and no flags but C3P_HERMITIAN_H (as given to c3p_pwc_lindblad_taped)");
  if (B <= 0 || K < 1 || K > 16 || N <= 0 || D <= 0) return fail("bad sizes B=%d K=%d N=%d D=%d", B, K, N, D);
  const int Dm = D * D;
  if (!tape || !signals || !U_bar || !grad_signals) return fail("NULL pointer argument");
  if (segments < 1 || segments > N) return fail("bad segment count %d", segments);
  if (D > 4 && !c3p_regr_supported(D, Dm)) return fail("the taped Lindblad evaluation serves D = 2, 3, 4 and D = 7, 8, 9, got D=%d", D);
  // the plan from the option table as it is NOW: an option that changes the segment count (or the kernel family) between the
  // taped forward call and this one would reinterpret the tape -- refuse what can be detected
  const LindTapePlan plan = lind_tape_plan(B, K, N, D);
  if (plan.family == TAPE_NONE || plan.segments != segments)
    return D <= 4 ? fail("taped Lindblad evaluation: shape not served or segment count %d != %d", segments, plan.segments)
                  : fail("taped Lindblad vjp: segment count %d != %d (c3p_pwc_lindblad_tape_bytes; were library options changed since the forward call?)", segments, plan.segments);
  if (tape_bytes < plan.bytes) return fail("tape too small: %zu bytes, need %zu", tape_bytes, plan.bytes);
  // the operators are in the tape: of them the backward halves read only whether the tables are per sample (a nonzero stride)
  const PwcProblem P = {nullptr, per_sample_operators ? 1 : 0, nullptr, 0, signals, nullptr, 0, 0.0, B, K, N, D, Dm, 1, fr_phase};
  void* tp = const_cast<void*>(tape);
  hipStream_t st = (hipStream_t)stream;
  WsLock lk(st);
  DeviceWs* w = lk.w;
  if (!w) return fail("no HIP device");
  if (!lk.ok) return fail("hipStreamWaitEvent on the previous call's stream failed");
  int rc, kernel;
  if (plan.family == TAPE_REGR) {
    kernel = C3P_KERNEL_MFMA;
    if (record_start(w, st)) return -1;
    rc = lind_regr_backward(w, lind_regr_carve(tp, lind_regr_sizes(B, K, N, Dm, segments, B)), P, segments, (const cplx*)U_bar, grad_signals, st);
  } else if (lind_smallr_ok((flags & C3P_HERMITIAN_H) != 0, D, Dm, K, N, segments)) {
    const int nsamp = P.nsamp();
    kernel = Dm > 12 ? C3P_KERNEL_MFMA : C3P_KERNEL_SMALLD;
    if (record_start(w, st)) return -1;
    rc = lind_smallr_backward(w, lind_smallr_carve(tp, lind_smallr_sizes(B, K, N, Dm, segments, nsamp), nsamp, Dm, K), P, segments, (const cplx*)U_bar,
                              grad_signals, st);
  } else {
    if (D == 4) return fail("the taped Lindblad evaluation at D = 4 needs C3P_HERMITIAN_H, as given to c3p_pwc_lindblad_taped");
    kernel = C3P_KERNEL_SMALLD;
    if (record_start(w, st)) return -1;
    rc = lind_small_backward(w, lind_small_carve(tp, lind_small_sizes(B, K, N, Dm, segments, B)), P, segments, (const cplx*)U_bar, grad_signals, st);
  }
  if (rc || record_stop(w, st)) return -1;
  g_last_kernel = kernel;
  return 0;
}

int c3p_gate_infid(const void* U, int B, int D, const int32_t* comp_rows, int L, const void* ideal, int kind, int flags,
                   double* infid_out, double* sum_out, void* stream) {
  if (B < 0 || D <= 0 || L <= 0 || L > D) return fail("bad sizes B=%d D=%d L=%d", B, D, L);
  if (kind != 0 && kind != 1) return fail("unknown infidelity kind %d (0 = unitary_infid, 1 = average_infid)", kind);
  if (!U || !comp_rows || !ideal || (!infid_out && !sum_out)) return fail("NULL pointer argument");
  hipStream_t st = (hipStream_t)stream;
  WsLock lk(st);
  DeviceWs* w = lk.w;
  if (!w) return fail("no HIP device");
  if (!lk.ok) return fail("hipStreamWaitEvent on the previous call's stream failed");
  const size_t cs = sizeof(cplx);
  Stage sg{w, st};
  const void *d_U = U, *d_rows = comp_rows, *d_G = ideal;
  void *d_inf = infid_out, *d_sum = sum_out;
  if (flags & C3P_HOST_PTRS) {
    for (int a = 0; a < L; ++a)
      if (comp_rows[a] < 0 || comp_rows[a] >= D) return fail("comp_rows[%d]=%d outside [0,%d)", a, comp_rows[a], D);
    if (sg.in(U, (size_t)B * D * D * cs, &d_U)) return -1;
    if (sg.in(comp_rows, (size_t)L * sizeof(int32_t), &d_rows)) return -1;
    if (sg.in(ideal, (size_t)L * L * cs, &d_G)) return -1;
    if (sg.out(infid_out, infid_out ? (size_t)B * sizeof(double) : 0, &d_inf)) return -1;
    if (sg.out(sum_out, sum_out ? 2 * sizeof(double) : 0, &d_sum)) return -1;
  }
  void* part;
  if (ws_get(w, SL_COUNTERS2, 256 * sizeof(double), &part)) return -1;
  if (B == 0) {
    if (d_sum) HIP_TRY(hipMemsetAsync(d_sum, 0, 2 * sizeof(double), st));
  } else {
    LAUNCH_TRY(c3p_launch_infid((const cplx*)d_U, B, D, (const int*)d_rows, L, (const cplx*)d_G, kind, (double*)d_inf,
                                (double*)part, (double*)d_sum, st));
  }
  if (flags & C3P_HOST_PTRS) return sg.finish();
  return 0;
}

int c3p_seq_chain(const void* G, int64_t G_bstride, int n_gates, int M, int P, const int32_t* seqs, int S, int Lmax,
                  const int32_t* lengths, int mode, const void* psi0, int flags, void* out, void* stream) {
  if (P < 0 || S < 0 || n_gates < 0 || Lmax < 0 || M <= 0 || M > C3P_SEQ_MAX_M || G_bstride < 0)
    return fail("bad sizes P=%d S=%d n_gates=%d M=%d Lmax=%d G_bstride=%lld (M <= %d)", P, S, n_gates, M, Lmax,
                (long long)G_bstride, C3P_SEQ_MAX_M);
  if (mode != C3P_SEQ_PRODUCT && mode != C3P_SEQ_STATE && mode != C3P_SEQ_POPULATION)
    return fail("unknown sequence output mode %d (0 = product, 1 = state, 2 = population)", mode);
  if (P > 65535) return fail("P=%d parameter samples: at most 65535 per call", P);
  if (P == 0 || S == 0) return 0;
  if (!lengths || !out) return fail("NULL lengths / output pointer");
  if (mode == C3P_SEQ_STATE && !psi0) return fail("state mode needs psi0");
  if ((flags & C3P_SEQ_PSI0_PER_SAMPLE) && mode != C3P_SEQ_STATE) return fail("C3P_SEQ_PSI0_PER_SAMPLE needs the state mode (C3P_SEQ_STATE)");
  const long psi0_bs = (flags & C3P_SEQ_PSI0_PER_SAMPLE) ? M : 0;
  if (Lmax > 0 && !seqs) return fail("seqs is NULL but Lmax=%d", Lmax);
  if (n_gates > 0 && !G) return fail("gate table is NULL");
  const size_t cs = sizeof(cplx);
  const size_t table = (size_t)n_gates * M * M;
  hipStream_t st = (hipStream_t)stream;
  WsLock lk(st);
  DeviceWs* w = lk.w;
  if (!w) return fail("no HIP device");
  if (!lk.ok) return fail("hipStreamWaitEvent on the previous call's stream failed");
  Stage sg{w, st};
  const void *d_G = G, *d_seqs = seqs, *d_len = lengths, *d_psi = psi0;
  void* d_out = out;
  const size_t out_bytes = mode == C3P_SEQ_PRODUCT ? (size_t)P * S * M * M * cs
                           : mode == C3P_SEQ_STATE ? (size_t)P * S * M * cs
                                                   : (size_t)P * S * sizeof(double);
  if (flags & C3P_HOST_PTRS) {
    // host memory: every length and every index used is checked here, before anything is staged
    for (int s = 0; s < S; ++s) {
      const int L = lengths[s];
      if (L < 0 || L > Lmax) return fail("sequence %d has length %d outside [0, %d]", s, L, Lmax);
      for (int t = 0; t < L; ++t) {
        const int g = seqs[(size_t)s * Lmax + t];
        if (g < 0 || g >= n_gates) return fail("sequence %d, position %d: gate index %d outside [0, %d)", s, t, g, n_gates);
      }
    }
    const size_t g_elems = G_bstride ? (size_t)(P - 1) * G_bstride + table : table;
    if (sg.in(G, g_elems * cs, &d_G)) return -1;
    if (sg.in(seqs, (size_t)S * Lmax * sizeof(int32_t), &d_seqs)) return -1;
    if (sg.in(lengths, (size_t)S * sizeof(int32_t), &d_len)) return -1;
    if (sg.in(mode == C3P_SEQ_STATE ? psi0 : nullptr, (size_t)(psi0_bs ? P : 1) * M * cs, &d_psi)) return -1;
    if (sg.out(out, out_bytes, &d_out)) return -1;
  }
  void* flag;
  if (ws_get(w, SL_SEQ_FLAG, sizeof(int), &flag)) return -1;
  HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int), st));
  SeqArgs a = {};
  a.G = (const cplx*)d_G;
  a.G_bstride = (long)G_bstride;
  a.n_gates = n_gates;
  a.M = M;
  a.P = P;
  a.seqs = (const int*)d_seqs;
  a.lengths = (const int*)d_len;
  a.S = S;
  a.Lmax = Lmax;
  a.mode = mode;
  a.superop = (flags & C3P_SEQ_SUPEROP) ? 1 : 0;
  a.psi0 = (const cplx*)d_psi;
  a.psi0_bstride = psi0_bs;
  a.out = d_out;
  a.bad = (int*)flag;
  g_last_kernel = C3P_KERNEL_SEQ;
  HIP_TRY(c3p_launch_seq(a, st));
  // device memory: the kernel checked every length and index it met; one int comes back (a stream synchronisation)
  int bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st));
  if (flags & C3P_HOST_PTRS) {
    if (sg.finish()) return -1;
  } else {
    HIP_TRY(hipStreamSynchronize(st));
  }
  if (bad) return fail("a sequence has a length outside [0, %d] or a gate index outside [0, %d): its outputs are NaN", Lmax, n_gates);
  return 0;
}

}  // extern "C"

namespace {
// c3p_seq_chain_vjp and c3p_seq_state_vjp: psi0 [M] (psi0_bstride 0) or one per sample; psi0_bar [P,M] or null (state mode only)
int seq_vjp_common(const void* G, int64_t G_bstride, int n_gates, int M, int P, const int32_t* seqs, int S, int Lmax,
                   const int32_t* lengths, int mode, const void* psi0, int64_t psi0_bstride, const void* out_bar, int flags, void* G_bar,
                   void* psi0_bar, void* out, void* stream) {
  if (P < 0 || S < 0 || n_gates < 0 || Lmax < 0 || M <= 0 || M > C3P_SEQ_MAX_M || G_bstride < 0)
    return fail("bad sizes P=%d S=%d n_gates=%d M=%d Lmax=%d G_bstride=%lld (M <= %d)", P, S, n_gates, M, Lmax,
                (long long)G_bstride, C3P_SEQ_MAX_M);
  if (mode != C3P_SEQ_PRODUCT && mode != C3P_SEQ_STATE && mode != C3P_SEQ_POPULATION)
    return fail("unknown sequence output mode %d (0 = product, 1 = state, 2 = population)", mode);
  if (P > 65535) return fail("P=%d parameter samples: at most 65535 per call", P);
  if (psi0_bstride < 0) return fail("negative psi0_bstride");
  if ((psi0_bstride != 0 || psi0_bar) && mode != C3P_SEQ_STATE) return fail("a per-sample psi0 and psi0_bar need the state mode (C3P_SEQ_STATE)");
  if (P == 0) return 0;
  // an empty table (n_gates = 0) still runs the chains: lengths and indices are checked and `out` is written
  if (n_gates > 0 && !G_bar) return fail("G_bar is NULL");
  if (S > 0 && (!lengths || !out_bar)) return fail("NULL lengths / out_bar pointer");
  if (S > 0 && mode == C3P_SEQ_STATE && !psi0) return fail("state mode needs psi0");
  if (S > 0 && Lmax > 0 && !seqs) return fail("seqs is NULL but Lmax=%d", Lmax);
  if (n_gates > 0 && !G) return fail("gate table is NULL");
  const size_t cs = sizeof(cplx);
  const size_t table = (size_t)n_gates * M * M;
  const int shared = G_bstride == 0;
  const size_t gbar_bytes = (shared ? 1 : (size_t)P) * table * cs;
  hipStream_t st = (hipStream_t)stream;
  WsLock lk(st);
  DeviceWs* w = lk.w;
  if (!w) return fail("no HIP device");
  if (!lk.ok) return fail("hipStreamWaitEvent on the previous call's stream failed");
  Stage sg{w, st};
  const void *d_G = G, *d_seqs = seqs, *d_len = lengths, *d_psi = psi0, *d_ob = out_bar;
  void *d_gbar = G_bar, *d_out = out, *d_pbar = psi0_bar;
  const size_t pbar_bytes = psi0_bar ? (size_t)P * M * cs : 0;
  const size_t out_bytes = mode == C3P_SEQ_PRODUCT ? (size_t)P * S * M * M * cs
                           : mode == C3P_SEQ_STATE ? (size_t)P * S * M * cs
                                                   : (size_t)P * S * sizeof(double);
  if (flags & C3P_HOST_PTRS) {
    // host memory: every length and every index used is checked here, before anything is staged
    for (int s = 0; s < S; ++s) {
      const int L = lengths[s];
      if (L < 0 || L > Lmax) return fail("sequence %d has length %d outside [0, %d]", s, L, Lmax);
      for (int t = 0; t < L; ++t) {
        const int g = seqs[(size_t)s * Lmax + t];
        if (g < 0 || g >= n_gates) return fail("sequence %d, position %d: gate index %d outside [0, %d)", s, t, g, n_gates);
      }
    }
    const size_t g_elems = G_bstride ? (size_t)(P - 1) * G_bstride + table : table;
    if (sg.in(G, g_elems * cs, &d_G)) return -1;
    if (S > 0) {
      if (sg.in(seqs, (size_t)S * Lmax * sizeof(int32_t), &d_seqs)) return -1;
      if (sg.in(lengths, (size_t)S * sizeof(int32_t), &d_len)) return -1;
      if (sg.in(mode == C3P_SEQ_STATE ? psi0 : nullptr, ((size_t)(P - 1) * psi0_bstride + M) * cs, &d_psi)) return -1;
      if (sg.in(out_bar, out_bytes, &d_ob)) return -1;
      if (sg.out(out, out ? out_bytes : 0, &d_out)) return -1;
    }
    if (sg.out(G_bar, gbar_bytes, &d_gbar)) return -1;
    if (sg.out(psi0_bar, pbar_bytes, &d_pbar)) return -1;
  }
  g_last_kernel = C3P_KERNEL_SEQ_VJP;
  if (S == 0) {  // no sequence: a zero gradient
    if (gbar_bytes) HIP_TRY(hipMemsetAsync(d_gbar, 0, gbar_bytes, st));
    if (pbar_bytes) HIP_TRY(hipMemsetAsync(d_pbar, 0, pbar_bytes, st));
    if (flags & C3P_HOST_PTRS) return sg.finish();
    return 0;
  }
  const SeqVjpPlan pl = c3p_seq_vjp_plan(n_gates, M, P, S, Lmax, mode, psi0_bar != nullptr);
  void *flag, *ws, *slab;
  if (ws_get(w, SL_SEQ_FLAG, sizeof(int), &flag)) return -1;
  if (ws_get(w, SL_SEQ_VJP_WS, pl.ws_elems * cs, &ws)) return -1;
  if (ws_get(w, SL_SEQ_VJP_SLAB, pl.slab_elems * cs, &slab)) return -1;
  HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int), st));
  SeqVjpArgs a = {};
  a.f.G = (const cplx*)d_G;
  a.f.G_bstride = (long)G_bstride;
  a.f.n_gates = n_gates;
  a.f.M = M;
  a.f.P = P;
  a.f.seqs = (const int*)d_seqs;
  a.f.lengths = (const int*)d_len;
  a.f.S = S;
  a.f.Lmax = Lmax;
  a.f.mode = mode;
  a.f.superop = (flags & C3P_SEQ_SUPEROP) ? 1 : 0;
  a.f.psi0 = (const cplx*)d_psi;
  a.f.psi0_bstride = (long)psi0_bstride;
  a.f.out = d_out;
  a.f.bad = (int*)flag;
  a.out_bar = d_ob;
  a.C = pl.C;
  a.nck = pl.nck;
  a.nblk = pl.nblk;
  a.ws = (cplx*)ws;
  a.slab = (cplx*)slab;
  a.G_bar = (cplx*)d_gbar;
  a.shared = shared;
  a.psi0_bar = (cplx*)d_pbar;
  g_note_plan = "checkpoint interval C=" + std::to_string(pl.C) + " nblk=" + std::to_string(pl.nblk);
  HIP_TRY(c3p_launch_seq_vjp(a, pl, st));
  int bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st));
  if (flags & C3P_HOST_PTRS) {
    if (sg.finish()) return -1;
  } else {
    HIP_TRY(hipStreamSynchronize(st));
  }
  if (bad) return fail("a sequence has a length outside [0, %d] or a gate index outside [0, %d): the gradient is not valid", Lmax, n_gates);
  return 0;
}
}  // namespace

extern "C" {

int c3p_seq_chain_vjp(const void* G, int64_t G_bstride, int n_gates, int M, int P, const int32_t* seqs, int S, int Lmax,
                      const int32_t* lengths, int mode, const void* psi0, const void* out_bar, int flags, void* G_bar, void* out,
                      void* stream) {
  if ((flags & C3P_SEQ_PSI0_PER_SAMPLE) && mode != C3P_SEQ_STATE) return fail("C3P_SEQ_PSI0_PER_SAMPLE needs the state mode (C3P_SEQ_STATE)");
  return seq_vjp_common(G, G_bstride, n_gates, M, P, seqs, S, Lmax, lengths, mode, psi0, (flags & C3P_SEQ_PSI0_PER_SAMPLE) ? M : 0, out_bar,
                        flags, G_bar, nullptr, out, stream);
}

int c3p_seq_state_vjp(const void* G, int64_t G_bstride, int n_gates, int M, int P, const int32_t* seqs, int S, int Lmax,
                      const int32_t* lengths, const void* psi0, int64_t psi0_bstride, const void* out_bar, int flags, void* G_bar,
                      void* psi0_bar, void* out, void* stream) {
  if (!psi0_bar) return fail("c3p_seq_state_vjp: psi0_bar is NULL (c3p_seq_chain_vjp serves calls that do not want it)");
  if (flags & C3P_SEQ_PSI0_PER_SAMPLE) return fail("c3p_seq_state_vjp takes psi0_bstride, not C3P_SEQ_PSI0_PER_SAMPLE");
  return seq_vjp_common(G, G_bstride, n_gates, M, P, seqs, S, Lmax, lengths, C3P_SEQ_STATE, psi0, psi0_bstride, out_bar, flags, G_bar,
                        psi0_bar, out, stream);
}

// fused goal of c3p_pwc_unitary_goal_vjp (device pointers after staging)
struct GoalSpec {
  const int32_t* rows;
  int L;
  const void* ideal;
  int kind;
  double* infid;
  double* gphase;
  void* U_out;
};
static int unitary_vjp_branch_a(const void* h0, int64_t h0_bstride, const void* hks, int64_t hks_bstride, const double* signals,
                                double dt, int B, int K, int N, int D, int flags, const double* fr_phase, const void* U_bar,
                                double* grad_signals, void* gen_bar_out, void* stream, const GoalSpec* goal) {
  if (B < 0 || K <= 0 || N <= 0 || D <= 0) return fail("bad sizes B=%d K=%d N=%d D=%d", B, K, N, D);
  if (D > 64 && gen_bar_out) return fail("gen_bar_out (per-slice generator cotangents) is available for D <= 64, got %d", D);
  if (B == 0) return 0;
  if (!h0 || !hks || !signals || (!U_bar && !goal) || !grad_signals) return fail("NULL pointer argument");
  if (h0_bstride < 0 || hks_bstride < 0) return fail("negative batch stride");
  const size_t cs = sizeof(cplx);
  hipStream_t st = (hipStream_t)stream;
  WsLock lk(st);
  DeviceWs* w = lk.w;
  if (!w) return fail("no HIP device");
  if (!lk.ok) return fail("hipStreamWaitEvent on the previous call's stream failed");
  Stage sg{w, st};
  const void *d_h0 = h0, *d_hks = hks, *d_sig = signals, *d_ph = fr_phase, *d_ub = U_bar;
  void* d_grad = grad_signals;
  void* d_zout = gen_bar_out;
  if (flags & C3P_HOST_PTRS) {
    // the adjoint recurrence M_n = dU_n^H M_{n+1} dU_n needs unitary slices: Hermitian generators
    const cplx* hh[2] = {(const cplx*)h0, (const cplx*)hks};
    const long cnt[2] = {h0_bstride ? (long)B : 1L, (hks_bstride ? (long)B : 1L) * K};
    for (int a = 0; a < 2; ++a)
      for (long m = 0; m < cnt[a]; ++m) {
        const cplx* H = hh[a] + m * D * D;
        double dev = 0.0, mag = 0.0;
        for (int i = 0; i < D; ++i)
          for (int j = 0; j < D; ++j) {
            dev = fmax(dev, hypot(H[i * D + j].x - H[j * D + i].x, H[i * D + j].y + H[j * D + i].y));
            mag = fmax(mag, hypot(H[i * D + j].x, H[i * D + j].y));
          }
        if (dev > 1e-9 * mag) return fail("c3p_pwc_unitary_vjp needs Hermitian Hamiltonians (deviation %.3g)", dev);
      }
    if (sg.in(h0, staged_elems(B, h0_bstride, (size_t)D * D) * cs, &d_h0)) return -1;
    if (sg.in(hks, staged_elems(B, hks_bstride, (size_t)K * D * D) * cs, &d_hks)) return -1;
    if (sg.in(signals, (size_t)B * K * N * sizeof(double), &d_sig)) return -1;
    if (U_bar && sg.in(U_bar, (size_t)B * D * D * cs, &d_ub)) return -1;
    if (fr_phase && sg.in(fr_phase, (size_t)B * D * sizeof(double), &d_ph)) return -1;
    if (sg.out(grad_signals, (size_t)B * K * N * sizeof(double), &d_grad)) return -1;
    if (gen_bar_out && sg.out(gen_bar_out, (size_t)B * N * D * D * cs, &d_zout)) return -1;
  }
  GoalSpec gd = {};
  if (goal) {
    gd = *goal;
    if (flags & C3P_HOST_PTRS) {
      const void* t;
      void* o;
      if (sg.in(goal->rows, (size_t)goal->L * sizeof(int32_t), &t)) return -1;
      gd.rows = (const int32_t*)t;
      if (sg.in(goal->ideal, (size_t)goal->L * goal->L * cs, &t)) return -1;
      gd.ideal = t;
      if (sg.out(goal->infid, (size_t)B * sizeof(double), &o)) return -1;
      gd.infid = (double*)o;
      if (goal->gphase) {
        if (sg.out(goal->gphase, (size_t)B * D * sizeof(double), &o)) return -1;
        gd.gphase = (double*)o;
      }
      if (goal->U_out) {
        if (sg.out(goal->U_out, (size_t)B * D * D * cs, &o)) return -1;
        gd.U_out = o;
      }
    }
  }
  GradArgs A = {};
  if (goal) {
    A.goal_rows = (const int*)gd.rows;
    A.goal_L = gd.L;
    A.goal_ideal = (const cplx*)gd.ideal;
    A.goal_kind = gd.kind;
    A.goal_infid = gd.infid;
    A.goal_gphase = gd.gphase;
    A.goal_U = (cplx*)gd.U_out;
  }
  A.h0 = (const cplx*)d_h0;
  A.h0_bstride = h0_bstride;
  A.hks = (const cplx*)d_hks;
  A.hks_bstride = hks_bstride;
  A.signals = (const double*)d_sig;
  A.fr_phase = (const double*)d_ph;
  A.Ubar = (const cplx*)d_ub;
  A.dt = dt;
  A.B = B;
  A.K = K;
  A.N = N;
  A.D = D;
  A.ld = D | 1;
  A.grad = (double*)d_grad;
  A.zout = (cplx*)d_zout;
  if (record_start(w, st)) return -1;
  bool done = false;
  if (!(flags & C3P_FORCE_GENERIC) && D <= kSmallDLimit && c3p_smalld_supported(D) && K <= 8) {
    const int rc = run_vjp_smalld(w, A, st);
    if (rc < 0) return -1;
    done = (rc == 0);
    if (done) g_last_kernel = C3P_KERNEL_SMALLD;
  }
  if (!done && !(flags & C3P_FORCE_GENERIC) && D >= 13 && D <= 40) {
    const int rc = run_vjp_midd(w, A, st);
    if (rc < 0) return -1;
    done = (rc == 0);
    if (done) g_last_kernel = C3P_KERNEL_MFMA;
  }
  // beyond the on-chip sweeps: forward partials in HBM, one pair evaluation of T18 per slice on the tiled MFMA GEMM.  ~35
  // launches per slice: below a few hundred samples the launches, not the GEMMs, set the time, and the VALU sweep (which
  // stops at D = 64) is faster for 41 <= D <= 64 (profiles/r03/grad_tiled.json: D = 48, B = 64: 151 ms against 545 ms)
  // (the fused goal entry has no tiled form: it stays on the VALU sweep in its whole domain)
  const bool tiled_grad = goal ? false : tiled_unitary_grad(D, B);
  if (!done && !(flags & C3P_FORCE_GENERIC) && tiled_grad && !gen_bar_out) {
    const PwcProblem P = {A.h0, h0_bstride, A.hks, hks_bstride, A.signals, nullptr, 0, dt, B, K, N, D, D, 0, A.fr_phase};
    if (run_vjp_tiled(w, P, A.Ubar, A.grad, st)) return -1;
    done = true;
    g_last_kernel = C3P_KERNEL_MFMA;
  }
  if (!done && D > 64) return fail("the VALU gradient kernels support D <= 64, got %d", D);
  if (!done) {
    A.S = (int)valu_grad_segments(B, N);
    void* v;
    if (ws_get(w, SL_SEG_A, (size_t)B * A.S * D * D * cs, &v)) return -1;
    A.seg = (cplx*)v;
    if (ws_get(w, SL_SEG_B, (size_t)B * A.S * D * D * cs, &v)) return -1;
    A.Mb = (cplx*)v;
    const bool global = c3p_grad_lds_bytes(D) > 150 * 1024;
    if (global) {
      A.scratch_stride = (long)C3P_GRAD_NMAT * A.ld * D;
      if (ws_get(w, SL_SCRATCH, (size_t)B * A.S * A.scratch_stride * cs, &v)) return -1;
      A.scratch = (cplx*)v;
    }
    g_last_kernel = global ? C3P_KERNEL_GENERIC_GLOBAL : C3P_KERNEL_GENERIC_LDS;
    LAUNCH_TRY(c3p_launch_grad_seg(A, global, st));
    LAUNCH_TRY(c3p_launch_grad_scan(A, global, st));
    LAUNCH_TRY(c3p_launch_grad_bwd(A, global, st));
  }
  if (record_stop(w, st)) return -1;
  if (flags & C3P_HOST_PTRS) return sg.finish();
  return 0;
}

int c3p_pwc_unitary_vjp(const void* h0, int64_t h0_bstride, const void* hks, int64_t hks_bstride,
                        const double* signals, double dt, int B, int K, int N, int D, int flags,
                        const double* fr_phase, const void* U_bar, double* grad_signals, void* gen_bar_out,
                        void* stream) {
  if (flags & C3P_ORDER_RIGHT) return fail("c3p_pwc_unitary_vjp: unsupported flag");
  if (flags & C3P_PER_SLICE_H) {
    // branch B of pwc (propagation.py:295-308): the Hamiltonians are handed over per slice, so the result is the cotangent of
    // every slice GENERATOR G_n = -i dt H_n (gen_bar_out) -- what the tape propagates on into model.get_Hamiltonian
    if (B < 0 || N <= 0 || D <= 0) return fail("bad sizes B=%d N=%d D=%d", B, N, D);
    if (B == 0) return 0;
    if (!h0 || !U_bar || !gen_bar_out) return fail("per-slice gradient: h0 (the Hamiltonians), U_bar and gen_bar_out are required");
    const size_t cs = sizeof(cplx);
    hipStream_t st = (hipStream_t)stream;
    WsLock lk(st);
    DeviceWs* w = lk.w;
    if (!w) return fail("no HIP device");
    if (!lk.ok) return fail("hipStreamWaitEvent on the previous call's stream failed");
    Stage sg{w, st};
    const void *d_h = h0, *d_ph = fr_phase, *d_ub = U_bar;
    void* d_z = gen_bar_out;
    if (flags & C3P_HOST_PTRS) {
      if (sg.in(h0, (size_t)(h0_bstride ? B : 1) * N * D * D * cs, &d_h)) return -1;
      if (sg.in(U_bar, (size_t)B * D * D * cs, &d_ub)) return -1;
      if (fr_phase && sg.in(fr_phase, (size_t)B * D * sizeof(double), &d_ph)) return -1;
      if (sg.out(gen_bar_out, (size_t)B * N * D * D * cs, &d_z)) return -1;
    }
    // the slice Hamiltonians as the record's h0: no control operators, no signals (K = 0)
    const PwcProblem P = {(const cplx*)d_h, h0_bstride, nullptr, 0, nullptr, nullptr, 0, dt, B, 0, N, D, D, 0, (const double*)d_ph};
    auto served = [&](int kernel) -> int {  // (this branch has no timed span)
      g_last_kernel = kernel;
      if (flags & C3P_HOST_PTRS) return sg.finish();
      return 0;
    };
    if (D <= 40 && !(flags & C3P_FORCE_GENERIC) && !c3p_opt_on(C3P_OPT_tiled_grad)) {
      // on-chip general-generator sweeps (nothing assumed about the slice Hamiltonians), in chunks of samples that keep the
      // slice propagators + prefixes (2 N D^2 complex per sample) below 24 GB
      const int rc = in_chunks(B, grad_chunk_samples(w, 2 * (size_t)N * D * D * cs), [&](long b0, int nb) {
        const PwcProblem c = P.chunk(b0, nb);
        return run_vjp_xg_general(w, c.h0, h0_bstride, 0.0, -dt, nb, N, D, c.fr_phase, ubar_at(P, (const cplx*)d_ub, b0),
                                  (cplx*)d_z + b0 * (long)N * D * D, st);
      });
      if (rc < 0) return -1;
      if (rc == 0) return served(D <= kSmallDLimit ? C3P_KERNEL_SMALLD : C3P_KERNEL_MFMA);
    }
    if (run_vjp_tiled(w, P, (const cplx*)d_ub, nullptr, st, true, (cplx*)d_z)) return -1;
    return served(C3P_KERNEL_MFMA);
  }
  if (!U_bar) return fail("NULL pointer argument");
  return unitary_vjp_branch_a(h0, h0_bstride, hks, hks_bstride, signals, dt, B, K, N, D, flags, fr_phase, U_bar, grad_signals,
                              gen_bar_out, stream, nullptr);
}

int c3p_pwc_unitary_goal_vjp(const void* h0, int64_t h0_bstride, const void* hks, int64_t hks_bstride, const double* signals,
                             double dt, int B, int K, int N, int D, int flags, const double* fr_phase, const int32_t* comp_rows,
                             int L, const void* ideal, int kind, double* infid_out, double* grad_signals, double* grad_fr_phase,
                             void* U_out, void* stream) {
  if (flags & (C3P_ORDER_RIGHT | C3P_PER_SLICE_H)) return fail("c3p_pwc_unitary_goal_vjp: unsupported flag");
  if (L <= 0 || L > D || L > C3P_GOAL_LMAX) return fail("bad computational subspace size L=%d (D=%d, at most %d)", L, D, C3P_GOAL_LMAX);
  if (kind != 0 && kind != 1) return fail("unknown infidelity kind %d", kind);
  if (!comp_rows || !ideal || !infid_out) return fail("NULL pointer argument");
  if (grad_fr_phase && !fr_phase) return fail("grad_fr_phase needs fr_phase");
  if (D > 64 || (D > 40 && (B >= 384 || c3p_opt_on(C3P_OPT_tiled_grad))))
    return fail("the fused goal runs on the on-chip and VALU backward sweeps (D <= 40, or D <= 64 below 384 samples): use "
                "c3p_pwc_unitary, c3p_gate_overlap and c3p_pwc_unitary_vjp for D=%d B=%d", D, B);
  if (flags & C3P_HOST_PTRS)
    for (int a = 0; a < L; ++a)
      if (comp_rows[a] < 0 || comp_rows[a] >= D) return fail("comp_rows[%d]=%d outside [0,%d)", a, comp_rows[a], D);
  GoalSpec g = {comp_rows, L, ideal, kind, infid_out, grad_fr_phase, U_out};
  return unitary_vjp_branch_a(h0, h0_bstride, hks, hks_bstride, signals, dt, B, K, N, D, flags, fr_phase, nullptr, grad_signals,
                              nullptr, stream, &g);
}

// ---- signal synthesis: one call record (SynthCall) and one function that runs it (synth_run) behind the six entries ----------
// host-pointer checks of a call with a line chain
static int chain_check_host(const int32_t* line_kind, const double* line_params, int B, int K, double sim_res) {
  for (int k = 0; k < K; ++k)
    if (line_kind[k] < 0 || line_kind[k] >= C3P_LINE_NKINDS) return fail("line_kind[%d]=%d is not a C3P_LINE_KIND_* id", k, line_kind[k]);
  for (long a = 0; a < (long)B * K; ++a) {
    const double* lp = line_params + a * C3P_LINE_NPAR;
    const double rt = lp[C3P_LINE_RISE_TIME];
    if (rt > 0.0 && !(std::floor(rt * sim_res) >= 1.0))
      return fail("line_params[%ld,%d]: rise_time=%g gives no Response tap at sim_res=%g (floor(rise_time * sim_res) = 0)",
                  a / K, (int)(a % K), rt, sim_res);
    if (line_kind[a % K] == C3P_LINE_KIND_FLUX && !(lp[C3P_LINE_PHI_0] != 0.0))
      return fail("line_params[%ld,%d]: a flux line needs phi_0 != 0", a / K, (int)(a % K));
  }
  return 0;
}

static int tab_block_len_host(int shape, int M) {
  switch (shape) {
    case C3P_ENVT_PWC:
    case C3P_ENVT_FOURIER_COS:
      return 2 * M;
    case C3P_ENVT_PWC_SHAPE:
    case C3P_ENVT_PWC_SYMMETRIC:
      return M + 2;
    default:
      return 3 * M;  // C3P_ENVT_FOURIER_SIN
  }
}

// host-pointer checks of an entry that takes a coefficient table: shape ids, blocks inside the row and apart from each other,
// the per-shape sizes, the flags a table shape does not take
static int tab_check_host(const double* env_params, const int32_t* env_shapes, const double* env_tab, const int32_t* tab_index, int T,
                          int B, int K, int E, int Na) {
  std::vector<std::pair<long, long>> blocks;  // [begin, end)
  for (int a = 0; a < K * E; ++a) {
    const int sh = env_shapes[a];
    if (sh >= C3P_ENV_NSHAPES && (sh < C3P_ENVT_FIRST || sh >= C3P_ENVT_END))
      return fail("env_shapes[%d]=%d is neither a C3P_ENV_* nor a C3P_ENVT_* id", a, sh);
    if (sh < C3P_ENVT_FIRST) continue;
    const long off = tab_index[2 * a], M = tab_index[2 * a + 1];
    if (off < 0 || M < 1) return fail("tab_index[%d,%d]={%ld,%ld}: a table shape needs an offset >= 0 and M >= 1", a / E, a % E, off, M);
    if (M > T || off + tab_block_len_host(sh, (int)M) > (long)T)
      return fail("tab_index[%d,%d]={%ld,%ld}: the block of %d doubles leaves the row (T=%d)", a / E, a % E, off, M,
                  M > T ? 0 : tab_block_len_host(sh, (int)M), T);
    if (sh == C3P_ENVT_PWC && M != Na) return fail("component [%d,%d]: pwc holds one pair per AWG sample, M=%ld but Na=%d", a / E, a % E, M, Na);
    if ((sh == C3P_ENVT_PWC_SHAPE || sh == C3P_ENVT_PWC_SYMMETRIC) && M < 2)
      return fail("component [%d,%d]: an interpolated shape needs M >= 2 knots, got %ld", a / E, a % E, M);
    blocks.push_back({off, off + tab_block_len_host(sh, (int)M)});
  }
  std::sort(blocks.begin(), blocks.end());
  for (size_t i = 1; i < blocks.size(); ++i)
    if (blocks[i].first < blocks[i - 1].second)
      return fail("tab_index: the blocks [%ld,%ld) and [%ld,%ld) overlap (grad_tab would be ambiguous)", blocks[i - 1].first,
                  blocks[i - 1].second, blocks[i].first, blocks[i].second);
  // the layout stands: what the rows and the table hold
  for (int a = 0; a < K * E; ++a) {
    const int sh = env_shapes[a];
    if (sh < C3P_ENVT_FIRST) continue;
    const long off = tab_index[2 * a];
    for (int b = 0; b < B; ++b) {
      const int fl = (int)env_params[((size_t)b * K * E + a) * C3P_ENV_NPAR + C3P_ENV_FLAGS];
      if (fl & C3P_ENVF_DRAG) return fail("env_params[%d,%d,%d]: C3P_ENVF_DRAG on a table shape is not served", b, a / E, a % E);
      if (sh == C3P_ENVT_PWC && (fl & C3P_ENVF_T_BEFORE))
        return fail("env_params[%d,%d,%d]: C3P_ENVF_T_BEFORE on pwc (the offset would be the array itself)", b, a / E, a % E);
      if (sh == C3P_ENVT_PWC_SHAPE || sh == C3P_ENVT_PWC_SYMMETRIC) {
        const double* blk = env_tab + (size_t)b * T + off;
        if (!(blk[1] > blk[0])) return fail("env_tab[%d]: component [%d,%d] needs t_bin_end > t_bin_start, got %g and %g", b, a / E, a % E, blk[1], blk[0]);
      }
    }
  }
  return 0;
}

// One synthesis call, as its entry states it.  What the entry takes is a property of the entry, not of the arguments: a
// table entry runs the table-aware AWG kernels at T = 0 too, a chain entry refuses a call without lines.
struct SynthCall {
  const double* env_params;   // [B,K,E,C3P_ENV_NPAR]
  const int32_t* env_shapes;  // [K,E]
  const double* carrier;      // [B,K,2]
  struct {
    bool has;  // c3p_synth_tab(_vjp): the C3P_ENVT_* ids are taken
    const double* env_tab;  // [B,T]
    const int32_t* tab_index;  // [K,E,2]
    int T;
  } table;
  struct {
    bool required;  // c3p_synth_chain(_vjp); otherwise the two go together, both NULL: the standard drive line
    const int32_t* line_kind;  // [K]
    const double* line_params;  // [B,K,C3P_LINE_NPAR]
  } lines;
  double t_start, t_end, awg_res, sim_res;
  int B, K, E, flags;
  struct {
    double *awg_iq_out, *signals_out;  // [B,K,2,Na] (optional), [B,K,N]
  } fwd;
  struct {
    bool on;
    const double* grad_signals;  // [B,K,N]
    double *grad_env, *grad_carrier, *grad_line, *grad_tab;  // grad_line with lines, grad_tab with T > 0
  } vjp;
  void* stream;
  // c3p_synth_filt(_vjp) alone set the two groups below
  struct {
    bool has;  // stage buffers between DAC and Mixer, F = 0 included
    const int32_t* filt_kind;   // [K,F]
    const double* filt_params;  // [B,K,F,C3P_FILT_NPAR]
    int F;
    double* grad_filt;  // [B,K,F,C3P_FILT_NPAR]
  } filters;
  struct {
    const double *dc_offset, *xtalk;  // [B,K], [B,K,K], each optional
    double *grad_dc, *grad_xtalk;     // each iff its input
  } post;
};

// host-pointer checks of the stage slots
static int filt_check_host(const int32_t* filt_kind, const double* filt_params, int B, int K, int F, double sim_res) {
  for (int a = 0; a < K * F; ++a)
    if (filt_kind[a] >= C3P_FILT_NKINDS) return fail("filt_kind[%d,%d]=%d is not a C3P_FILT_* id", a / F, a % F, filt_kind[a]);
  for (long r = 0; r < (long)B * K * F; ++r) {
    const int kind = filt_kind[r % ((long)K * F)];
    if (kind < 0) continue;
    const int b = (int)(r / ((long)K * F)), k = (int)(r / F % K), f = (int)(r % F);
    const double tau = filt_params[r * C3P_FILT_NPAR + C3P_FILT_TAU], amp = filt_params[r * C3P_FILT_NPAR + C3P_FILT_AMP];
    if (!std::isfinite(tau) || !std::isfinite(amp))
      return fail("filt_params[%d,%d,%d]={%g,%g} is not finite", b, k, f, tau, amp);
    if (kind != C3P_FILT_SKIN_EFFECT && !(tau > 0.0))
      return fail("filt_params[%d,%d,%d]: a time constant must be positive, got %g", b, k, f, tau);
    if (kind == C3P_FILT_RESPONSE_FFT && !(std::floor(tau * sim_res) >= 1.0))
      return fail("filt_params[%d,%d,%d]: rise_time=%g gives no ResponseFFT tap at sim_res=%g (floor(rise_time * sim_res) = 0)", b, k,
                  f, tau, sim_res);
  }
  return 0;
}

static int synth_run(const SynthCall& c) {
  const int B = c.B, K = c.K, E = c.E, T = c.table.T, flags = c.flags;
  const bool vjp = c.vjp.on;
  if (B < 0 || K <= 0 || E <= 0 || T < 0) return fail("bad sizes B=%d K=%d E=%d T=%d", B, K, E, T);
  const bool filt = c.filters.has;
  const int F = c.filters.F;
  if (F < 0) return fail("bad sizes F=%d", F);
  if (!(c.awg_res > 0.0) || !(c.sim_res > 0.0)) return fail("resolutions must be positive");
  const double span = c.t_end > c.t_start ? c.t_end - c.t_start : c.t_start - c.t_end;
  const int N = (int)(span * c.sim_res), Na = (int)(span * c.awg_res);  // devices.py:72-84
  if (N <= 0 || Na <= 1) return fail("empty time grid: N=%d Na=%d", N, Na);
  if (B == 0) return 0;
  if (!c.env_params || !c.env_shapes || !c.carrier) return fail("NULL pointer argument");
  if (c.table.has && (!c.table.tab_index || (T > 0 && !c.table.env_tab))) return fail("NULL pointer argument");
  if (c.lines.required && (!c.lines.line_kind || !c.lines.line_params)) return fail("NULL pointer argument");
  if ((c.lines.line_kind == nullptr) != (c.lines.line_params == nullptr))
    return fail("line_kind and line_params go together (both NULL: the standard drive line)");
  const bool chain = c.lines.line_kind != nullptr;
  if ((c.filters.filt_kind == nullptr) != (c.filters.filt_params == nullptr)) return fail("filt_kind and filt_params go together");
  if (F > 0 && !c.filters.filt_kind) return fail("NULL pointer argument");
  if (vjp && ((F > 0 && !c.filters.grad_filt) || (c.post.dc_offset && !c.post.grad_dc) || (c.post.xtalk && !c.post.grad_xtalk)))
    return fail("NULL pointer argument");
  if (!vjp && !c.fwd.signals_out) return fail("NULL pointer argument");
  if (vjp && (!c.vjp.grad_signals || !c.vjp.grad_env || !c.vjp.grad_carrier || (chain && !c.vjp.grad_line) || (T > 0 && !c.vjp.grad_tab)))
    return fail("NULL pointer argument");
  if (flags & C3P_HOST_PTRS) {  // every look at host data comes before the workspace lock and any device work
    if (chain && chain_check_host(c.lines.line_kind, c.lines.line_params, B, K, c.sim_res)) return -1;
    if (c.table.has) {
      if (tab_check_host(c.env_params, c.env_shapes, c.table.env_tab, c.table.tab_index, T, B, K, E, Na)) return -1;
    } else {
      for (int a = 0; a < K * E; ++a)
        if (c.env_shapes[a] >= C3P_ENV_NSHAPES) return fail("env_shapes[%d]=%d is not a C3P_ENV_* id", a, c.env_shapes[a]);
    }
    if (F > 0 && filt_check_host(c.filters.filt_kind, c.filters.filt_params, B, K, F, c.sim_res)) return -1;
  }
  hipStream_t st = (hipStream_t)c.stream;
  WsLock lk(st);
  DeviceWs* w = lk.w;
  if (!w) return fail("no HIP device");
  if (!lk.ok) return fail("hipStreamWaitEvent on the previous call's stream failed");
  Stage sg{w, st};
  const void *d_env = c.env_params, *d_shape = c.env_shapes, *d_tab = c.table.env_tab, *d_tidx = c.table.tab_index, *d_car = c.carrier,
             *d_kind = c.lines.line_kind, *d_line = c.lines.line_params, *d_gs = c.vjp.grad_signals;
  void *d_iq = c.fwd.awg_iq_out, *d_sig = c.fwd.signals_out, *d_ge = c.vjp.grad_env, *d_gc = c.vjp.grad_carrier, *d_gl = c.vjp.grad_line, *d_gt = c.vjp.grad_tab;
  void *d_gf = c.filters.grad_filt, *d_gdc = c.post.grad_dc, *d_gxt = c.post.grad_xtalk;
  const size_t lines = (size_t)B * K, awg = lines * 2 * Na;
  if (flags & C3P_HOST_PTRS) {  // a NULL or empty buffer takes no staging slot: each entry keeps the slots it always had
    if (sg.in(c.env_params, lines * E * C3P_ENV_NPAR * sizeof(double), &d_env)) return -1;
    if (sg.in(c.env_shapes, (size_t)K * E * sizeof(int32_t), &d_shape)) return -1;
    if (sg.in(c.table.env_tab, (size_t)B * T * sizeof(double), &d_tab)) return -1;
    if (sg.in(c.table.tab_index, (size_t)K * E * 2 * sizeof(int32_t), &d_tidx)) return -1;
    if (sg.in(c.carrier, lines * 2 * sizeof(double), &d_car)) return -1;
    if (sg.in(c.lines.line_kind, (size_t)K * sizeof(int32_t), &d_kind)) return -1;
    if (sg.in(c.lines.line_params, lines * C3P_LINE_NPAR * sizeof(double), &d_line)) return -1;
    if (vjp) {
      if (sg.in(c.vjp.grad_signals, lines * N * sizeof(double), &d_gs)) return -1;
      if (sg.out(c.vjp.grad_env, lines * E * C3P_ENV_NPAR * sizeof(double), &d_ge)) return -1;
      if (sg.out(c.vjp.grad_carrier, lines * 2 * sizeof(double), &d_gc)) return -1;
      if (chain && sg.out(c.vjp.grad_line, lines * C3P_LINE_NPAR * sizeof(double), &d_gl)) return -1;
      if (sg.out(c.vjp.grad_tab, (size_t)B * T * sizeof(double), &d_gt)) return -1;
      if (F > 0 && sg.out(c.filters.grad_filt, lines * F * C3P_FILT_NPAR * sizeof(double), &d_gf)) return -1;
      if (c.post.dc_offset && sg.out(c.post.grad_dc, lines * sizeof(double), &d_gdc)) return -1;
      if (c.post.xtalk && sg.out(c.post.grad_xtalk, lines * K * sizeof(double), &d_gxt)) return -1;
    } else {
      if (sg.out(c.fwd.signals_out, lines * N * sizeof(double), &d_sig)) return -1;
      if (sg.out(c.fwd.awg_iq_out, awg * sizeof(double), &d_iq)) return -1;
    }
  }
  // scratch: [taps [B,K,tap_stride]] | iq (unless the caller takes it) | vjp: giq | gcar_part (B*K*2*Na each) |
  //          [gcs [B,K,2,N] | part [B,K,tiles,stride]]; the bracketed parts with a line chain only
  const size_t tap_stride = N > 1 ? (size_t)N - 1 : 1, tap_elems = chain ? lines * tap_stride : 0;
  const size_t iq_elems = (!vjp && d_iq) ? 0 : awg;
  const size_t gcs_elems = (chain || filt) && vjp ? lines * 2 * N : 0;
  const size_t part_elems = (chain || filt) && vjp ? lines * c3p_chain_tiles(N) * c3p_chain_part_stride() : 0;
  // c3p_synth_filt appends: h [B,K,F,N] | buf [F+1,B,K,2,N] | pre [B,K,N] (xtalk) | vjp: gbuf [B,K,2,N] | gh [B,K,N] |
  // gpre [B,K,N] (xtalk) | host-pointer calls: the four inputs that have no staging slot left (filt_kind rounded up to doubles)
  const bool xt = c.post.xtalk != nullptr, host = (flags & C3P_HOST_PTRS) != 0;
  const size_t sig = lines * N, h_elems = filt ? sig * F : 0, buf_elems = filt ? 2 * sig * (F + 1) : 0, pre_elems = filt && xt ? sig : 0;
  const size_t gbuf_elems = filt && vjp ? 2 * sig : 0, gh_elems = filt && vjp ? sig : 0, gpre_elems = filt && vjp && xt ? sig : 0;
  const size_t fk_elems = filt && host && F > 0 ? ((size_t)K * F + 1) / 2 : 0, fp_elems = filt && host ? lines * F * C3P_FILT_NPAR : 0;
  const size_t dc_elems = filt && host && c.post.dc_offset ? lines : 0, xt_elems = filt && host && xt ? lines * K : 0;
  const size_t filt_elems = h_elems + buf_elems + pre_elems + gbuf_elems + gh_elems + gpre_elems + fk_elems + fp_elems + dc_elems + xt_elems;
  const size_t scratch = tap_elems + iq_elems + (vjp ? 2 * awg : 0) + gcs_elems + part_elems + filt_elems;
  // A drive call into the caller's I/Q needs no scratch and asks for none: ws_get rounds an empty request up to 16 bytes,
  // which on a fresh device allocates the slot and bumps c3p_workspace_generation.  The table entries have always asked.
  void* v = nullptr;
  if ((scratch || c.table.has) && ws_get(w, SL_SCRATCH, scratch * sizeof(double), &v)) return -1;
  double* p = (double*)v;
  SynthChainArgs C;
  SynthArgs& A = C.S;
  A.env = (const double*)d_env;
  A.shape = (const int*)d_shape;
  A.carrier = (const double*)d_car;
  A.t_start = c.t_start;
  A.t_end = c.t_end;
  A.awg_res = c.awg_res;
  A.sim_res = c.sim_res;
  A.B = B;
  A.K = K;
  A.E = E;
  A.Na = Na;
  A.N = N;
  A.iq = iq_elems ? p + tap_elems : (double*)d_iq;
  A.signals = (double*)d_sig;
  C.kind = (const int*)d_kind;
  C.line = (const double*)d_line;
  C.taps = chain ? p : nullptr;
  C.tap_stride = (long)tap_stride;
  const SynthTabArgs X = {(const double*)d_tab, (const int*)d_tidx, T};
  const SynthTabArgs* Xp = c.table.has ? &X : nullptr;
  SynthFiltArgs Fa = {};
  SynthFiltVjpBufs W = {};
  if (filt) {
    double* q = p + (scratch - filt_elems);
    Fa.F = F;
    Fa.h = q;
    Fa.buf = Fa.h + h_elems;
    Fa.pre = xt ? Fa.buf + buf_elems : nullptr;
    W.gbuf = Fa.buf + buf_elems + pre_elems;
    W.gh = W.gbuf + gbuf_elems;
    W.gpre = gpre_elems ? W.gh + gh_elems : nullptr;
    Fa.fkind = (const int*)c.filters.filt_kind;
    Fa.fpar = c.filters.filt_params;
    Fa.dc = c.post.dc_offset;
    Fa.xtalk = c.post.xtalk;
    if (host) {  // the staging slots are taken: these four travel in the scratch
      double* in = W.gh + gh_elems + gpre_elems;
      if (fk_elems) HIP_TRY(hipMemcpyAsync(in, c.filters.filt_kind, (size_t)K * F * sizeof(int32_t), hipMemcpyHostToDevice, st));
      if (fp_elems) HIP_TRY(hipMemcpyAsync(in + fk_elems, c.filters.filt_params, fp_elems * sizeof(double), hipMemcpyHostToDevice, st));
      if (dc_elems) HIP_TRY(hipMemcpyAsync(in + fk_elems + fp_elems, c.post.dc_offset, dc_elems * sizeof(double), hipMemcpyHostToDevice, st));
      if (xt_elems) HIP_TRY(hipMemcpyAsync(in + fk_elems + fp_elems + dc_elems, c.post.xtalk, xt_elems * sizeof(double), hipMemcpyHostToDevice, st));
      Fa.fkind = fk_elems ? (const int*)in : nullptr;
      Fa.fpar = fp_elems ? in + fk_elems : nullptr;
      Fa.dc = dc_elems ? in + fk_elems + fp_elems : nullptr;
      Fa.xtalk = xt_elems ? in + fk_elems + fp_elems + dc_elems : nullptr;
    }
    W.gfilt = (double*)d_gf;
    W.gdc = (double*)d_gdc;
    W.gxtalk = (double*)d_gxt;
  }
  if (!vjp) {
    if (filt)
      LAUNCH_TRY(c3p_launch_synth_filt(C, X, Fa, st));
    else
      LAUNCH_TRY(c3p_launch_synth(C, Xp, st));
  } else {
    SynthVjpBufs V = {};
    V.giq = A.iq + awg;
    V.gcar_part = V.giq + awg;
    if (chain || filt) {
      V.gcs = V.gcar_part + awg;
      V.part = V.gcs + gcs_elems;
    }
    V.genv = (double*)d_ge;
    V.gcar = (double*)d_gc;
    V.gline = (double*)d_gl;
    V.gtab = (double*)d_gt;
    if (filt)
      LAUNCH_TRY(c3p_launch_synth_filt_vjp(C, X, Fa, (const double*)d_gs, V, W, st));
    else
      LAUNCH_TRY(c3p_launch_synth_vjp(C, Xp, (const double*)d_gs, V, st));
  }
  if (flags & C3P_HOST_PTRS) return sg.finish();
  return 0;
}

// The six entries: {rows}, {table}, {lines}, grid, sizes, {forward outputs}, {vjp input and outputs}, stream.
int c3p_synth_signals(const double* env_params, const int32_t* env_shapes, const double* carrier,
                      double t_start, double t_end, double awg_res, double sim_res, int B, int K,
                      int E, int flags, double* awg_iq_out, double* signals_out, void* stream) {
  return synth_run({env_params, env_shapes, carrier, {}, {}, t_start, t_end, awg_res, sim_res, B, K, E, flags,
                    {awg_iq_out, signals_out}, {}, stream});
}

int c3p_synth_signals_vjp(const double* env_params, const int32_t* env_shapes, const double* carrier,
                          double t_start, double t_end, double awg_res, double sim_res, int B, int K,
                          int E, int flags, const double* grad_signals, double* grad_env, double* grad_carrier,
                          void* stream) {
  return synth_run({env_params, env_shapes, carrier, {}, {}, t_start, t_end, awg_res, sim_res, B, K, E, flags,
                    {}, {true, grad_signals, grad_env, grad_carrier, nullptr, nullptr}, stream});
}

int c3p_synth_chain(const double* env_params, const int32_t* env_shapes, const double* carrier, const int32_t* line_kind,
                    const double* line_params, double t_start, double t_end, double awg_res, double sim_res, int B, int K,
                    int E, int flags, double* awg_iq_out, double* signals_out, void* stream) {
  return synth_run({env_params, env_shapes, carrier, {}, {true, line_kind, line_params}, t_start, t_end, awg_res, sim_res, B, K, E, flags,
                    {awg_iq_out, signals_out}, {}, stream});
}

int c3p_synth_chain_vjp(const double* env_params, const int32_t* env_shapes, const double* carrier, const int32_t* line_kind,
                        const double* line_params, double t_start, double t_end, double awg_res, double sim_res, int B,
                        int K, int E, int flags, const double* grad_signals, double* grad_env, double* grad_carrier,
                        double* grad_line, void* stream) {
  return synth_run({env_params, env_shapes, carrier, {}, {true, line_kind, line_params}, t_start, t_end, awg_res, sim_res, B, K, E, flags,
                    {}, {true, grad_signals, grad_env, grad_carrier, grad_line, nullptr}, stream});
}

int c3p_synth_tab(const double* env_params, const int32_t* env_shapes, const double* env_tab, const int32_t* tab_index, int T,
                  const double* carrier, const int32_t* line_kind, const double* line_params, double t_start, double t_end,
                  double awg_res, double sim_res, int B, int K, int E, int flags, double* awg_iq_out, double* signals_out,
                  void* stream) {
  return synth_run({env_params, env_shapes, carrier, {true, env_tab, tab_index, T}, {false, line_kind, line_params}, t_start, t_end,
                    awg_res, sim_res, B, K, E, flags, {awg_iq_out, signals_out}, {}, stream});
}

int c3p_synth_tab_vjp(const double* env_params, const int32_t* env_shapes, const double* env_tab, const int32_t* tab_index, int T,
                      const double* carrier, const int32_t* line_kind, const double* line_params, double t_start, double t_end,
                      double awg_res, double sim_res, int B, int K, int E, int flags, const double* grad_signals,
                      double* grad_env, double* grad_carrier, double* grad_line, double* grad_tab, void* stream) {
  if (!grad_signals) return fail("NULL pointer argument");
  return synth_run({env_params, env_shapes, carrier, {true, env_tab, tab_index, T}, {false, line_kind, line_params}, t_start, t_end,
                    awg_res, sim_res, B, K, E, flags, {}, {true, grad_signals, grad_env, grad_carrier, grad_line, grad_tab}, stream});
}

int c3p_synth_filt(const double* env_params, const int32_t* env_shapes, const double* env_tab, const int32_t* tab_index, int T,
                   const double* carrier, const int32_t* line_kind, const double* line_params, const int32_t* filt_kind,
                   const double* filt_params, int F, const double* dc_offset, const double* xtalk, double t_start, double t_end,
                   double awg_res, double sim_res, int B, int K, int E, int flags, double* awg_iq_out, double* signals_out,
                   void* stream) {
  return synth_run({env_params, env_shapes, carrier, {true, env_tab, tab_index, T}, {false, line_kind, line_params}, t_start, t_end,
                    awg_res, sim_res, B, K, E, flags, {awg_iq_out, signals_out}, {}, stream, {true, filt_kind, filt_params, F, nullptr},
                    {dc_offset, xtalk, nullptr, nullptr}});
}

int c3p_synth_filt_vjp(const double* env_params, const int32_t* env_shapes, const double* env_tab, const int32_t* tab_index, int T,
                       const double* carrier, const int32_t* line_kind, const double* line_params, const int32_t* filt_kind,
                       const double* filt_params, int F, const double* dc_offset, const double* xtalk, double t_start,
                       double t_end, double awg_res, double sim_res, int B, int K, int E, int flags, const double* grad_signals,
                       double* grad_env, double* grad_carrier, double* grad_line, double* grad_tab, double* grad_filt,
                       double* grad_dc, double* grad_xtalk, void* stream) {
  if (!grad_signals) return fail("NULL pointer argument");
  return synth_run({env_params, env_shapes, carrier, {true, env_tab, tab_index, T}, {false, line_kind, line_params}, t_start, t_end,
                    awg_res, sim_res, B, K, E, flags, {}, {true, grad_signals, grad_env, grad_carrier, grad_line, grad_tab}, stream,
                    {true, filt_kind, filt_params, F, grad_filt}, {dc_offset, xtalk, grad_dc, grad_xtalk}});
}

int c3p_dress(const void* H, const void* ops, int64_t ops_bstride, int P, int M, int D, int flags, double* eig_out, void* T_out,
              void* h0_out, void* ops_out, int32_t* status_out, void* stream) {
  if (P < 0 || M < 0 || ops_bstride < 0) return fail("bad sizes P=%d M=%d ops_bstride=%lld", P, M, (long long)ops_bstride);
  if (D < 2 || D > C3P_DRESS_MAX_D) return fail("c3p_dress serves 2 <= D <= %d, got D=%d", C3P_DRESS_MAX_D, D);
  if (P == 0) return 0;
  if (!H) return fail("NULL drift Hamiltonian");
  if (M > 0 && ops_out && !ops) return fail("ops is NULL but M=%d", M);
  const size_t cs = sizeof(cplx), dd = (size_t)D * D;
  if (ops_bstride != 0 && (size_t)ops_bstride < (size_t)M * dd) return fail("ops_bstride=%lld is smaller than one operator list (%zu)", (long long)ops_bstride, M * dd);
  hipStream_t st = (hipStream_t)stream;
  WsLock lk(st);
  DeviceWs* w = lk.w;
  if (!w) return fail("no HIP device");
  if (!lk.ok) return fail("hipStreamWaitEvent on the previous call's stream failed");
  Stage sg{w, st};
  const void *d_H = H, *d_ops = ops;
  void *d_eig = eig_out, *d_T = T_out, *d_h0 = h0_out, *d_oo = ops_out, *d_st = status_out;
  if (flags & C3P_HOST_PTRS) {
    if (sg.in(H, (size_t)P * dd * cs, &d_H)) return -1;
    if (sg.in(M > 0 ? ops : nullptr, ((size_t)(P - 1) * ops_bstride + (size_t)M * dd) * cs, &d_ops)) return -1;
    if (sg.out(eig_out, (size_t)P * D * sizeof(double), &d_eig)) return -1;
    if (sg.out(T_out, (size_t)P * dd * cs, &d_T)) return -1;
    if (sg.out(h0_out, (size_t)P * dd * cs, &d_h0)) return -1;
    if (sg.out(ops_out, (size_t)P * M * dd * cs, &d_oo)) return -1;
    if (sg.out(status_out, (size_t)P * sizeof(int32_t), &d_st)) return -1;
  }
  DressArgs a = {};
  a.H = (const cplx*)d_H;
  a.ops = (const cplx*)d_ops;
  a.ops_bstride = (long)ops_bstride;
  a.P = P;
  a.M = M;
  a.D = D;
  a.eig = (double*)d_eig;
  a.T = (cplx*)d_T;
  a.h0 = (cplx*)d_h0;
  a.ops_out = M > 0 ? (cplx*)d_oo : nullptr;
  a.status = (int*)d_st;
  g_last_kernel = C3P_KERNEL_DRESS;
  HIP_TRY(c3p_launch_dress(a, st));
  if (flags & C3P_HOST_PTRS) return sg.finish();
  return 0;
}

int c3p_dress_vjp(const void* T, const double* eig, const void* ops, int64_t ops_bstride, int P, int M, int D, int flags,
                  const double* eig_bar, const void* h0_bar, const void* ops_bar, const void* T_bar, void* H_bar_out,
                  void* ops_bare_bar_out, int32_t* status_out, void* stream) {
  if (P < 0 || M < 0 || ops_bstride < 0) return fail("bad sizes P=%d M=%d ops_bstride=%lld", P, M, (long long)ops_bstride);
  if (D < 2 || D > C3P_DRESS_MAX_D) return fail("c3p_dress_vjp serves 2 <= D <= %d, got D=%d", C3P_DRESS_MAX_D, D);
  if (P == 0) return 0;
  if (!T || !eig) return fail("NULL transform / eigenvalues (the results of c3p_dress)");
  if (M > 0 && ops_bar && !ops) return fail("ops is NULL but M=%d cotangents are given", M);
  const size_t cs = sizeof(cplx), dd = (size_t)D * D;
  if (ops_bstride != 0 && (size_t)ops_bstride < (size_t)M * dd) return fail("ops_bstride=%lld is smaller than one operator list (%zu)", (long long)ops_bstride, M * dd);
  const bool have_ops = M > 0 && ops_bar;
  hipStream_t st = (hipStream_t)stream;
  WsLock lk(st);
  DeviceWs* w = lk.w;
  if (!w) return fail("no HIP device");
  if (!lk.ok) return fail("hipStreamWaitEvent on the previous call's stream failed");
  Stage sg{w, st};
  const void *d_T = T, *d_eig = eig, *d_ops = ops, *d_eb = eig_bar, *d_hb = h0_bar, *d_ob = ops_bar, *d_tb = T_bar;
  void *d_H = H_bar_out, *d_ab = ops_bare_bar_out, *d_st = status_out;
  const size_t abar_bytes = have_ops ? (ops_bstride ? (size_t)P : 1) * M * dd * cs : 0;
  if (flags & C3P_HOST_PTRS) {
    if (sg.in(T, (size_t)P * dd * cs, &d_T)) return -1;
    if (sg.in(eig, (size_t)P * D * sizeof(double), &d_eig)) return -1;
    if (sg.in(have_ops ? ops : nullptr, ((size_t)(P - 1) * ops_bstride + (size_t)M * dd) * cs, &d_ops)) return -1;
    if (sg.in(eig_bar, (size_t)P * D * sizeof(double), &d_eb)) return -1;
    if (sg.in(h0_bar, (size_t)P * dd * cs, &d_hb)) return -1;
    if (sg.in(have_ops ? ops_bar : nullptr, (size_t)P * M * dd * cs, &d_ob)) return -1;
    if (sg.in(T_bar, (size_t)P * dd * cs, &d_tb)) return -1;
    if (sg.out(H_bar_out, (size_t)P * dd * cs, &d_H)) return -1;
    if (sg.out(ops_bare_bar_out, abar_bytes, &d_ab)) return -1;
    if (sg.out(status_out, (size_t)P * sizeof(int32_t), &d_st)) return -1;
  }
  DressVjpArgs a = {};
  a.T = (const cplx*)d_T;
  a.eig = (const double*)d_eig;
  a.ops = (const cplx*)d_ops;
  a.ops_bstride = (long)ops_bstride;
  a.P = P;
  a.M = have_ops ? M : 0;
  a.D = D;
  a.eig_bar = (const double*)d_eb;
  a.h0_bar = (const cplx*)d_hb;
  a.ops_bar = have_ops ? (const cplx*)d_ob : nullptr;
  a.T_bar = (const cplx*)d_tb;
  a.H_bar = (cplx*)d_H;
  a.ops_bare_bar = have_ops ? (cplx*)d_ab : nullptr;
  a.status = (int*)d_st;
  g_last_kernel = C3P_KERNEL_DRESS_VJP;
  HIP_TRY(c3p_launch_dress_vjp(a, st));
  if (flags & C3P_HOST_PTRS) return sg.finish();
  return 0;
}

// c3p_readout_goal (goal_weights, x_bar_out, ... null, vjp false) and c3p_readout_goal_vjp: checks, staging, workspace, launches.
static int readout_common(bool vjp, const void* x, int P, int S, int M, int D, const double* conf, int64_t conf_bstride, int R,
                          const double* label_w, const double* rescale, int64_t rescale_bstride, const double* meas,
                          const double* stds, const double* shots, int estimator, const double* goal_weights, int flags,
                          double* sim_out, double* sim_raw_out, double* goals_out, void* x_bar_out, double* conf_bar_out,
                          double* rescale_bar_out, double* pop_bar_out, void* stream) {
  const char* entry = vjp ? "c3p_readout_goal_vjp" : "c3p_readout_goal";
  if (P < 0 || S < 0 || conf_bstride < 0) return fail("%s: bad sizes P=%d S=%d conf_bstride=%lld", entry, P, S, (long long)conf_bstride);
  if (D < 2 || D > C3P_READOUT_MAX_D) return fail("%s serves 2 <= D <= %d, got D=%d", entry, C3P_READOUT_MAX_D, D);
  if (M != D && M != D * D) return fail("%s: M=%d is neither D=%d (kets) nor D^2=%d (density vectors)", entry, M, D, D * D);
  if (R < 1) return fail("%s: R=%d, the read-out needs at least one row", entry, R);
  if (R > C3P_READOUT_MAX_D) return fail("%s serves R <= %d, got R=%d", entry, C3P_READOUT_MAX_D, R);
  if (!conf && R != D) return fail("%s: without a confusion matrix R must be D=%d, got R=%d", entry, D, R);
  if (estimator < C3P_EST_G_LL_PRIME || estimator > C3P_EST_RMS_SIM_STDS_DIST) return fail("%s: unknown estimator id %d", entry, estimator);
  if (!sim_out || !goals_out) return fail("%s: NULL sim_out / goals_out", entry);
  if (vjp && !x_bar_out) return fail("%s: NULL x_bar_out", entry);
  const size_t rd = (size_t)R * D;
  if (conf && conf_bstride != 0 && (size_t)conf_bstride < rd) return fail("%s: conf_bstride=%lld is smaller than one confusion matrix (%zu)", entry, (long long)conf_bstride, rd);
  if (rescale && rescale_bstride != 0 && rescale_bstride != 2) return fail("%s: rescale_bstride=%lld, expected 0 (shared) or 2", entry, (long long)rescale_bstride);
  if (P == 0 || S == 0) return 0;
  if (!x || !meas || !shots) return fail("%s: NULL x / meas / shots", entry);
  if (estimator == C3P_EST_RMS_EXP_STDS_DIST && !stds) return fail("%s: rms_exp_stds_dist reads stds, which is NULL", entry);
  if (vjp && !goal_weights) return fail("%s: NULL goal_weights", entry);
  const int V = label_w ? 1 : R;
  const size_t ds = sizeof(double), cs = sizeof(cplx);
  const size_t nx = (size_t)P * S * M, nv = (size_t)P * S * V, npop = (size_t)P * S * D;
  hipStream_t st = (hipStream_t)stream;
  WsLock lk(st);
  DeviceWs* w = lk.w;
  if (!w) return fail("no HIP device");
  if (!lk.ok) return fail("hipStreamWaitEvent on the previous call's stream failed");
  Stage sg{w, st};
  const void *d_x = x, *d_conf = conf, *d_lw = label_w, *d_rs = rescale, *d_meas = meas, *d_stds = stds, *d_shots = shots, *d_gw = goal_weights;
  void *d_sim = sim_out, *d_raw = sim_raw_out, *d_goals = goals_out, *d_xb = x_bar_out, *d_cb = conf_bar_out, *d_rb = rescale_bar_out, *d_pb = pop_bar_out;
  if (flags & C3P_HOST_PTRS) {
    if (sg.in(x, nx * cs, &d_x)) return -1;
    if (sg.in(conf, ((size_t)(P - 1) * conf_bstride + rd) * ds, &d_conf)) return -1;
    if (sg.in(label_w, (size_t)R * ds, &d_lw)) return -1;
    if (sg.in(rescale, ((size_t)(P - 1) * rescale_bstride + 2) * ds, &d_rs)) return -1;
    if (sg.in(meas, nv * ds, &d_meas)) return -1;
    if (sg.in(stds, nv * ds, &d_stds)) return -1;
    if (sg.in(shots, nv * ds, &d_shots)) return -1;
    if (sg.in(goal_weights, (size_t)P * ds, &d_gw)) return -1;
    if (sg.out(sim_out, nv * ds, &d_sim)) return -1;
    if (sg.out(sim_raw_out, nv * ds, &d_raw)) return -1;
    if (sg.out(goals_out, (size_t)P * ds, &d_goals)) return -1;
    if (sg.out(x_bar_out, nx * cs, &d_xb)) return -1;
    if (sg.out(conf_bar_out, (size_t)P * rd * ds, &d_cb)) return -1;
    if (sg.out(rescale_bar_out, (size_t)P * 2 * ds, &d_rb)) return -1;
    if (sg.out(pop_bar_out, npop * ds, &d_pb)) return -1;
  }
  // workspace: the summands; for the reverse pass also sim_bar, v_bar, the populations and (not given by the caller) sim_raw
  const bool own_raw = vjp && !d_raw;
  const size_t wsd = nv + (vjp ? 2 * nv + npop + (own_raw ? nv : 0) : 0);
  void* v;
  if (ws_get(w, SL_SCRATCH, wsd * ds, &v)) return -1;
  double* ws = (double*)v;
  ReadoutArgs a = {};
  a.x = (const cplx*)d_x;
  a.P = P;
  a.S = S;
  a.M = M;
  a.D = D;
  a.R = R;
  a.V = V;
  a.density = M != D;
  a.conf = (const double*)d_conf;
  a.conf_bstride = (long)conf_bstride;
  a.label_w = (const double*)d_lw;
  a.rescale = (const double*)d_rs;
  a.rescale_bstride = (long)rescale_bstride;
  a.meas = (const double*)d_meas;
  a.stds = (const double*)d_stds;
  a.shots = (const double*)d_shots;
  a.estimator = estimator;
  a.sim = (double*)d_sim;
  a.sim_raw = (double*)d_raw;
  a.goals = (double*)d_goals;
  a.terms = ws;
  if (vjp) {
    a.sim_bar = ws + nv;
    a.v_bar = ws + 2 * nv;
    a.pop = ws + 3 * nv;
    if (own_raw) a.sim_raw = ws + 3 * nv + npop;
    a.goal_weights = (const double*)d_gw;
    a.x_bar = (cplx*)d_xb;
    a.conf_bar = (double*)d_cb;
    a.rescale_bar = (double*)d_rb;
    a.pop_bar = (double*)d_pb;
  }
  g_last_kernel = vjp ? C3P_KERNEL_READOUT_VJP : C3P_KERNEL_READOUT;
  HIP_TRY(vjp ? c3p_launch_readout_vjp(a, st) : c3p_launch_readout(a, st));
  if (flags & C3P_HOST_PTRS) return sg.finish();
  return 0;
}

int c3p_readout_goal(const void* x, int P, int S, int M, int D, const double* conf, int64_t conf_bstride, int R,
                     const double* label_w, const double* rescale, int64_t rescale_bstride, const double* meas,
                     const double* stds, const double* shots, int estimator, int flags, double* sim_out, double* sim_raw_out,
                     double* goals_out, void* stream) {
  return readout_common(false, x, P, S, M, D, conf, conf_bstride, R, label_w, rescale, rescale_bstride, meas, stds, shots, estimator,
                        nullptr, flags, sim_out, sim_raw_out, goals_out, nullptr, nullptr, nullptr, nullptr, stream);
}

int c3p_readout_goal_vjp(const void* x, int P, int S, int M, int D, const double* conf, int64_t conf_bstride, int R,
                         const double* label_w, const double* rescale, int64_t rescale_bstride, const double* meas,
                         const double* stds, const double* shots, int estimator, const double* goal_weights, int flags,
                         double* sim_out, double* sim_raw_out, double* goals_out, void* x_bar_out, double* conf_bar_out,
                         double* rescale_bar_out, double* pop_bar_out, void* stream) {
  return readout_common(true, x, P, S, M, D, conf, conf_bstride, R, label_w, rescale, rescale_bstride, meas, stds, shots, estimator,
                        goal_weights, flags, sim_out, sim_raw_out, goals_out, x_bar_out, conf_bar_out, rescale_bar_out, pop_bar_out, stream);
}

}  // extern "C"
