// Read-out epilogue of model learning on the device: from the sequence states x [P,S,M] to the simulated
// values and the goal of every parameter set, and back from the goal weights to the cotangents of x and of the read-out
// parameters.  Experiment.process (c3/experiment.py:355-407), ConfusionMatrix.confuse and MeasurementRescale.rescale
// (c3/libraries/tasks.py:107-129,161-178), estimators of c3/libraries/estimators.py.  fp64 throughout.
//
// Work split.  The per-sequence arithmetic is element-wise: a workgroup of the two element kernels serves SEQ_BLOCK sequences
// of one set, populations and confused values in LDS.  Everything that is SUMMED over the sequences of a set -- the goal, the
// cotangents of the confusion matrix and of (scale, offset) -- is summed by kernels of their own from values the element
// kernels leave in the workspace, every output by one thread or one workgroup in an order that S, V, R and D fix: no
// atomics, nothing depends on P or on where a set sits in the batch.
#include "c3p_readout.h"

namespace {

constexpr int SB = C3P_READOUT_SEQ_BLOCK;
constexpr int NT = C3P_READOUT_THREADS;

// r = m - s, v = s (1 - s), var = v / shots, q = r^2 / var.  The summand t of every estimator and dt / ds.
struct Term {
  double t, dt;
};

__device__ __forceinline__ Term estimator_term(int est, double m, double s, double e, double sh) {
  // Straight-line: every estimator's pair is a select over the shared quantities (the estimator is uniform over the launch).
  // The values an estimator does not use may be inf / nan (e.g. rms_dist with s outside (0,1)); they are not selected.
  const double r = m - s;
  const double z = r / e;
  const double v = s * (1.0 - s);
  const double var = v / sh;
  const double q = r * r / var;
  const double slope = (1.0 - 2.0 * s) / v;          // var' / var
  const double dq = -(2.0 * r / var + q * slope);     // d/ds [r^2 / var]
  Term o;
  o.t = q;  // C3P_EST_RMS_SIM_STDS_DIST
  o.dt = dq;
  if (est == C3P_EST_G_LL_PRIME) {
    o.t = (q - 1.0) * 0.5;
    o.dt = 0.5 * dq;
  }
  if (est == C3P_EST_NEG_LOGLKH_GAUSS) {
    // -log N(m; s, sqrt(var)) = q / 2 + log(var) / 2 + log(2 pi) / 2
    o.t = 0.5 * q + 0.5 * log(var) + 0.9189385332046727;
    o.dt = 0.5 * dq + 0.5 * slope;
  }
  if (est == C3P_EST_NEG_LOGLKH_GAUSS_NORM || est == C3P_EST_NEG_LOGLKH_GAUSS_NORM_SUM) {
    o.t = 0.5 * q;
    o.dt = 0.5 * dq;
  }
  if (est == C3P_EST_RMS_DIST) {
    o.t = r * r;
    o.dt = -2.0 * r;
  }
  if (est == C3P_EST_RMS_EXP_STDS_DIST) {
    o.t = z * z;
    o.dt = -2.0 * z / e;
  }
  return o;
}

// goal = f(sum of the n summands), and d goal / d (summand)
__device__ __forceinline__ double estimator_goal(int est, double sum, double n) {
  if (est == C3P_EST_NEG_LOGLKH_GAUSS_NORM_SUM) return sum;
  if (est >= C3P_EST_RMS_DIST) return sqrt(sum / n);
  return sum / n;
}
__device__ __forceinline__ double estimator_factor(int est, double goal, double n) {
  if (est == C3P_EST_NEG_LOGLKH_GAUSS_NORM_SUM) return 1.0;
  if (est >= C3P_EST_RMS_DIST) return 1.0 / (2.0 * goal * n);
  return 1.0 / n;
}

// Sum of the workgroup's NT partials in LDS, as a tree of fixed shape; the result in red[0].
__device__ __forceinline__ void block_tree_sum(double* red, int tid) {
  __syncthreads();
  for (int h = NT / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
}

// Populations of the workgroup's `ns` sequences (from s0 of set p) into LDS pop[ns][D], and the confused values c[ns][R].
__device__ __forceinline__ void block_populations(const ReadoutArgs& a, long p, int s0, int ns, double* pop, double* c, int tid) {
  const int D = a.D, R = a.R;
  const cplx* x = a.x + ((long)p * a.S + s0) * a.M;
  for (int i = tid; i < ns * D; i += NT) {
    const int s = i / D, n = i - s * D;
    double v;
    if (a.density) {
      v = x[(long)s * a.M + (long)n * (D + 1)].x;
    } else {
      const cplx z = x[(long)s * a.M + n];
      v = z.x * z.x + z.y * z.y;
    }
    pop[i] = v;
    if (a.pop) a.pop[((long)p * a.S + s0) * D + i] = v;
  }
  __syncthreads();
  const double* cm = a.conf ? a.conf + p * a.conf_bstride : nullptr;
  for (int i = tid; i < ns * R; i += NT) {
    const int s = i / R, r = i - s * R;
    double acc;
    if (cm) {
      acc = 0.0;
      for (int n = 0; n < D; ++n) acc = fma(cm[r * D + n], pop[s * D + n], acc);
    } else {
      acc = pop[s * D + r];
    }
    c[i] = acc;
  }
  __syncthreads();
}

// Forward element kernel: grid = P * ceil(S / SB) workgroups.  Writes sim, sim_raw, the estimator's summands and (reverse pass) pop.
__global__ __launch_bounds__(NT) void readout_values_kernel(ReadoutArgs a) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x;
  const int nblk = (a.S + SB - 1) / SB;
  const long p = blockIdx.x / nblk;
  const int s0 = (int)(blockIdx.x - p * nblk) * SB;
  const int ns = min(SB, a.S - s0);
  double* pop = lds;
  double* c = lds + SB * a.D;
  block_populations(a, p, s0, ns, pop, c, tid);
  const int R = a.R, V = a.V;
  double scale = 1.0, offset = 0.0;
  if (a.rescale) {
    scale = a.rescale[p * a.rescale_bstride];
    offset = a.rescale[p * a.rescale_bstride + 1];
  }
  for (int i = tid; i < ns * V; i += NT) {
    double v;
    if (a.label_w) {
      v = 0.0;
      for (int r = 0; r < R; ++r) v = fma(a.label_w[r], c[i * R + r], v);
    } else {
      v = c[i];
    }
    const double sim = a.rescale ? fma(scale, v, offset) : v;
    const long o = ((long)p * a.S + s0) * V + i;
    a.sim[o] = sim;
    if (a.sim_raw) a.sim_raw[o] = v;
    a.terms[o] = estimator_term(a.estimator, a.meas[o], sim, a.stds ? a.stds[o] : 1.0, a.shots[o]).t;
  }
}

// goals[p] from the S V summands of set p: thread t adds the values t, t + NT, ... in order, then a fixed tree.  grid = P.
__global__ __launch_bounds__(NT) void readout_goal_kernel(ReadoutArgs a) {
  __shared__ double red[NT];
  const int tid = threadIdx.x;
  const long p = blockIdx.x;
  const long n = (long)a.S * a.V;
  const double* t = a.terms + p * n;
  double acc = 0.0;
  for (long i = tid; i < n; i += NT) acc += t[i];
  red[tid] = acc;
  block_tree_sum(red, tid);
  if (tid == 0) a.goals[p] = estimator_goal(a.estimator, red[0], (double)n);
}

// Reverse element kernel, after the goals are known: sim_bar and v_bar into the workspace, pop_bar, and every entry of x_bar.
__global__ __launch_bounds__(NT) void readout_vjp_kernel(ReadoutArgs a) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x;
  const int nblk = (a.S + SB - 1) / SB;
  const long p = blockIdx.x / nblk;
  const int s0 = (int)(blockIdx.x - p * nblk) * SB;
  const int ns = min(SB, a.S - s0);
  const int D = a.D, R = a.R, V = a.V, M = a.M;
  double* pb = lds;           // pop_bar[ns][D]
  double* cb = lds + SB * D;  // c_bar[ns][R]
  const double scale = a.rescale ? a.rescale[p * a.rescale_bstride] : 1.0;
  const double f = a.goal_weights[p] * estimator_factor(a.estimator, a.goals[p], (double)a.S * V);
  for (int i = tid; i < ns * V; i += NT) {
    const long o = ((long)p * a.S + s0) * V + i;
    const double sb = f * estimator_term(a.estimator, a.meas[o], a.sim[o], a.stds ? a.stds[o] : 1.0, a.shots[o]).dt;
    const double vb = a.rescale ? sb * scale : sb;
    a.sim_bar[o] = sb;
    a.v_bar[o] = vb;
    if (a.label_w) {
      for (int r = 0; r < R; ++r) cb[i * R + r] = a.label_w[r] * vb;
    } else {
      cb[i] = vb;
    }
  }
  __syncthreads();
  const double* cm = a.conf ? a.conf + p * a.conf_bstride : nullptr;
  for (int i = tid; i < ns * D; i += NT) {
    const int s = i / D, n = i - s * D;
    double acc;
    if (cm) {
      acc = 0.0;
      for (int r = 0; r < R; ++r) acc = fma(cm[r * D + n], cb[s * R + r], acc);
    } else {
      acc = cb[s * R + n];
    }
    pb[i] = acc;
    if (a.pop_bar) a.pop_bar[((long)p * a.S + s0) * D + i] = acc;
  }
  __syncthreads();
  const long base = ((long)p * a.S + s0) * M;
  const long tot = (long)ns * M;
  if (a.density) {
    for (long i = tid; i < tot; i += NT) {
      const int s = (int)(i / M), e = (int)(i - (long)s * M);
      const int n = e / (D + 1);
      a.x_bar[base + i] = (e - n * (D + 1) == 0) ? cmake(pb[s * D + n], 0.0) : cmake(0.0, 0.0);
    }
  } else {
    for (long i = tid; i < tot; i += NT) {
      const cplx z = a.x[base + i];
      const double g = 2.0 * pb[i];  // (M == D: the same index)
      a.x_bar[base + i] = cmake(g * z.x, g * z.y);
    }
  }
}

// conf_bar[p,r,n] = sum_s c_bar[p,s,r] pop[p,s,n]: one thread per (r, n), the sequences in order.  grid = P * ceil(R D / NT).
__global__ __launch_bounds__(NT) void readout_conf_bar_kernel(ReadoutArgs a) {
  const int RD = a.R * a.D;
  const int ntile = (RD + NT - 1) / NT;
  const long p = blockIdx.x / ntile;
  const int i = (int)(blockIdx.x - p * ntile) * NT + threadIdx.x;
  if (i >= RD) return;
  const int r = i / a.D, n = i - r * a.D;
  const double* pop = a.pop + p * a.S * a.D + n;
  const double* vb = a.v_bar + p * a.S * a.V;
  double acc = 0.0;
  if (a.label_w) {
    const double w = a.label_w[r];
    for (int s = 0; s < a.S; ++s) acc = fma(w * vb[s], pop[(long)s * a.D], acc);
  } else {
    for (int s = 0; s < a.S; ++s) acc = fma(vb[(long)s * a.V + r], pop[(long)s * a.D], acc);
  }
  a.conf_bar[p * RD + i] = acc;
}

// rescale_bar[p] = (sum sim_bar v, sum sim_bar) over the S V values of set p, summed as the goal is.  grid = P.
__global__ __launch_bounds__(NT) void readout_rescale_bar_kernel(ReadoutArgs a) {
  __shared__ double red[NT];
  const int tid = threadIdx.x;
  const long p = blockIdx.x;
  const long n = (long)a.S * a.V;
  const double* sb = a.sim_bar + p * n;
  const double* v = a.sim_raw + p * n;
  double as = 0.0, ao = 0.0;
  for (long i = tid; i < n; i += NT) {
    as = fma(sb[i], v[i], as);
    ao += sb[i];
  }
  red[tid] = as;
  block_tree_sum(red, tid);
  const double scale_bar = red[0];
  __syncthreads();
  red[tid] = ao;
  block_tree_sum(red, tid);
  if (tid == 0) {
    a.rescale_bar[2 * p] = scale_bar;
    a.rescale_bar[2 * p + 1] = red[0];
  }
}

inline size_t element_lds(const ReadoutArgs& a) { return (size_t)SB * (a.D + a.R) * sizeof(double); }
inline unsigned element_grid(const ReadoutArgs& a) { return (unsigned)((long)a.P * ((a.S + SB - 1) / SB)); }

}  // namespace

hipError_t c3p_launch_readout(const ReadoutArgs& a, hipStream_t st) {
  C3P_LAUNCH(readout_values_kernel, dim3(element_grid(a)), dim3(NT), element_lds(a), st, a);
  C3P_LAUNCH(readout_goal_kernel, dim3(a.P), dim3(NT), 0, st, a);
  return hipGetLastError();
}

hipError_t c3p_launch_readout_vjp(const ReadoutArgs& a, hipStream_t st) {
  C3P_LAUNCH(readout_values_kernel, dim3(element_grid(a)), dim3(NT), element_lds(a), st, a);
  C3P_LAUNCH(readout_goal_kernel, dim3(a.P), dim3(NT), 0, st, a);
  C3P_LAUNCH(readout_vjp_kernel, dim3(element_grid(a)), dim3(NT), element_lds(a), st, a);
  if (a.conf_bar) {
    const long ntile = ((long)a.R * a.D + NT - 1) / NT;
    C3P_LAUNCH(readout_conf_bar_kernel, dim3((unsigned)(a.P * ntile)), dim3(NT), 0, st, a);
  }
  if (a.rescale_bar) C3P_LAUNCH(readout_rescale_bar_kernel, dim3(a.P), dim3(NT), 0, st, a);
  return hipGetLastError();
}
