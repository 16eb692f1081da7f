// Control-signal synthesis for the standard drive line
//   LO + AWG -> DigitalToAnalog -> Mixer -> VoltsToHertz
// (reference: c3/signal/gates.py:341-370 get_awg_signal, c3/signal/pulse.py:88-180 envelopes/mask/DRAG,
//  c3/generator/devices.py:72-122 create_ts, :306-351 DAC, :914-939 Mixer, :1073-1130 LO, :203-221 V->Hz).
// A batch is described by B x K x E envelope-parameter rows instead of B x K x N samples; the samples
// are produced in HBM where the propagator kernels read them.  Two launches: the AWG-resolution I/Q
// (a few hundred samples per line), then upsampling + mixing, one thread per output sample (HBM-bound,
// 8 B written per sample, nothing re-read from HBM: the I/Q rows stay in L2).
// Envelope shapes whose parameters are an array of coefficients (c3/libraries/envelopes.py:31-68,104-125,142-191: pwc, pwc_shape,
// pwc_symmetric, fourier_sin, fourier_cos) read a coefficient table beside the rows: the <true> instantiations of awg_iq_kernel and awg_bwd_kernel, and tab_bwd_kernel.
#include <hip/hip_runtime.h>

#include "c3p_common.h"
#include "c3p_signal.h"

namespace {

// numpy.linspace(start, stop, num)[j]: j * step + start with separate roundings, last sample = stop
__device__ __forceinline__ double linspace_at(double start, double stop, int num, int j) {
  if (num <= 1) return start;
  if (j == num - 1) return stop;
  const double step = __ddiv_rn(__dsub_rn(stop, start), (double)(num - 1));
  return __dadd_rn(__dmul_rn((double)j, step), start);
}

__device__ __forceinline__ double sigmoid(double x) { return 1.0 / (1.0 + exp(-x)); }

struct EnvP {
  double amp, xy, fo, delta, t_final, sigma, t_up, t_down, risefall, delay;
  int use_t_before, drag;
};

__device__ __forceinline__ EnvP load_env(const double* p) {
  EnvP e;
  e.amp = p[C3P_ENV_AMP];
  e.xy = p[C3P_ENV_XY_ANGLE];
  e.fo = p[C3P_ENV_FREQ_OFFSET];
  e.delta = p[C3P_ENV_DELTA];
  e.t_final = p[C3P_ENV_T_FINAL];
  e.sigma = p[C3P_ENV_SIGMA];
  e.t_up = p[C3P_ENV_T_UP];
  e.t_down = p[C3P_ENV_T_DOWN];
  e.risefall = p[C3P_ENV_RISEFALL];
  e.delay = p[C3P_ENV_DELAY];
  const int fl = (int)p[C3P_ENV_FLAGS];
  e.use_t_before = fl & C3P_ENVF_T_BEFORE;
  e.drag = fl & C3P_ENVF_DRAG;
  return e;
}

// (TAB on the closed-form helpers only keeps the two kernel families apart: the instantiation the existing entries launch is
// compiled as it was before the table shapes came)
template <bool TAB>
__device__ double shape_val(int shape, double t, const EnvP& p) {
  switch (shape) {
    case C3P_ENV_RECT:
      return 1.0;
    case C3P_ENV_GAUSSIAN_NONORM: {
      const double u = t - p.t_final / 2;
      return exp(-(u * u) / (2 * p.sigma * p.sigma));
    }
    case C3P_ENV_FLATTOP:
    case C3P_ENV_FLATTOP_RISEFALL: {
      const double rf = p.risefall;
      const double tu = shape == C3P_ENV_FLATTOP ? p.t_up : rf;
      const double td = shape == C3P_ENV_FLATTOP ? p.t_down : p.t_final - rf;
      return (1 + erf((t - tu) / rf)) / 2 * (1 + erf((-t + td) / rf)) / 2;
    }
    case C3P_ENV_COSINE:
      return 0.5 * (1 - cos(2 * M_PI * t / p.t_final));
    case C3P_ENV_GAUSSIAN_SIGMA:
    case C3P_ENV_GAUSSIAN: {
      const double T = p.t_final;
      const double sg = shape == C3P_ENV_GAUSSIAN_SIGMA ? p.sigma : T / 6;
      const double u = t - T / 2;
      const double offset = exp(-(T * T) / (8 * sg * sg));
      const double norm = sqrt(2 * M_PI * sg * sg) * erf(T / (sqrt(8.0) * sg)) - T * offset;
      return (exp(-(u * u) / (2 * sg * sg)) - offset) / norm;
    }
    case C3P_ENV_TRAPEZOID: {
      const double w = p.risefall * 2.5;
      double env = 1.0;
      if (t <= w) env = t / w;
      if (t >= p.t_final - w) env = (p.t_final - t) / w;
      return env;
    }
    default:
      return 0.0;
  }
}

template <bool TAB>
__device__ double shape_der(int shape, double t, const EnvP& p) {
  switch (shape) {
    case C3P_ENV_GAUSSIAN_NONORM:
      return -(t - p.t_final / 2) / (p.sigma * p.sigma) * shape_val<TAB>(shape, t, p);
    case C3P_ENV_FLATTOP:
    case C3P_ENV_FLATTOP_RISEFALL: {
      const double rf = p.risefall;
      const double tu = shape == C3P_ENV_FLATTOP ? p.t_up : rf;
      const double td = shape == C3P_ENV_FLATTOP ? p.t_down : p.t_final - rf;
      const double u = (t - tu) / rf, d = (-t + td) / rf;
      const double c = 2 / sqrt(M_PI) / rf;
      return (c * exp(-u * u) * (1 + erf(d)) - (1 + erf(u)) * c * exp(-d * d)) / 4;
    }
    case C3P_ENV_COSINE: {
      const double w = 2 * M_PI / p.t_final;
      return 0.5 * w * sin(w * t);
    }
    case C3P_ENV_GAUSSIAN_SIGMA:
    case C3P_ENV_GAUSSIAN: {
      const double T = p.t_final;
      const double sg = shape == C3P_ENV_GAUSSIAN_SIGMA ? p.sigma : T / 6;
      const double u = t - T / 2;
      const double offset = exp(-(T * T) / (8 * sg * sg));
      const double norm = sqrt(2 * M_PI * sg * sg) * erf(T / (sqrt(8.0) * sg)) - T * offset;
      return -u / (sg * sg) * exp(-(u * u) / (2 * sg * sg)) / norm;
    }
    case C3P_ENV_TRAPEZOID: {
      const double w = p.risefall * 2.5;
      double d = 0.0;
      if (t <= w) d = 1.0 / w;
      if (t >= p.t_final - w) d = -1.0 / w;
      return d;
    }
    default:
      return 0.0;
  }
}

__device__ __forceinline__ double mask_val(double ts_off, double dt, double tf_) {
  return sigmoid((ts_off / dt + 0.001) * 1e6) * sigmoid((0.999 * tf_ - ts_off) / dt * 1e6);
}

struct EnvEval {
  double er;       // real envelope (mask * (shape - offset))
  double ei_unit;  // imaginary DRAG part per unit delta: -dt * d env/dt (0 unless C3P_ENVF_DRAG)
  double ts_off;   // time relative to the component's start
};

// envelope of component `p` at AWG sample j (pulse.py:88-180)
template <bool TAB>
__device__ EnvEval env_eval(const SynthArgs& A, int shape, const EnvP& p, int j, double a0, double a1) {
  const double t = linspace_at(a0, a1, A.Na, j);
  const double t_first = linspace_at(a0, a1, A.Na, 0), t_second = linspace_at(a0, a1, A.Na, A.Na > 1 ? 1 : 0);
  const double t0 = A.t_start + p.delay;
  const double ts_off = t - t0, off0 = t_first - t0, off1 = t_second - t0;
  const double dt = off1 - off0;
  const double tf_ = p.t_final;  // window = t_final of the component (gates.py:293-297)
  const double m = mask_val(ts_off, dt, tf_);
  const double t_before = 2 * off0 - off1;
  const double offset = p.use_t_before ? shape_val<TAB>(shape, t_before, p) : 0.0;
  EnvEval r;
  r.ts_off = ts_off;
  r.er = m * (shape_val<TAB>(shape, ts_off, p) - offset);
  r.ei_unit = 0.0;
  if (p.drag) {
    double denv = m * shape_der<TAB>(shape, ts_off, p);
    if (p.use_t_before && j < 2) {
      double msum = 0.0;
      for (int i = 0; i < A.Na; ++i) msum += mask_val(linspace_at(a0, a1, A.Na, i) - t0, dt, tf_);
      const double doff = shape_der<TAB>(shape, t_before, p) * msum;
      denv += (j == 0) ? -2 * doff : doff;
    }
    r.ei_unit = -denv * dt;
  }
  return r;
}

// ---- envelopes whose parameters are an array of coefficients (C3P_ENVT_*; envelopes.py:31-68,104-125,142-191) ----------------
// A component's block lies at tab_index[k,e] = {offset, M} in its sample's row of env_tab.  Device-pointer calls cannot look at
// the index table, so a block that does not lie inside the row contributes nothing (and receives no cotangent).
__device__ __forceinline__ int tab_block_len(int shape, int M) {
  switch (shape) {
    case C3P_ENVT_PWC:
    case C3P_ENVT_FOURIER_COS:
      return 2 * M;
    case C3P_ENVT_PWC_SHAPE:
    case C3P_ENVT_PWC_SYMMETRIC:
      return M + 2;
    case C3P_ENVT_FOURIER_SIN:
      return 3 * M;
    default:
      return 0;
  }
}
__device__ __forceinline__ bool tab_block(const SynthTabArgs& X, int ke, int shape, int* off, int* M) {
  const int o = X.tidx[2 * ke], m = X.tidx[2 * ke + 1];
  *off = o;
  *M = m;
  if (o < 0 || m < 1 || m > X.T) return false;
  return (long)o + tab_block_len(shape, m) <= (long)X.T;
}

// tfp.math.interp_regular_1d_grid(t, x0, x1, y[0..M-1], fill_value_below=0, fill_value_above=0) as the pair of knots and the
// weight of the upper one: value = (1 - w) y[lo] + w y[lo + 1]; false outside [x0, x1]
__device__ __forceinline__ bool interp_cell(double t, double x0, double x1, int M, int* lo, double* w) {
  if (!(t >= x0 && t <= x1) || M < 2) return false;
  double xi = (t - x0) / (x1 - x0) * (double)(M - 1);
  xi = xi < 0.0 ? 0.0 : (xi > (double)(M - 1) ? (double)(M - 1) : xi);
  int l = (int)floor(xi);
  l = l > M - 2 ? M - 2 : l;
  *lo = l;
  *w = xi - (double)l;
  return true;
}
__device__ __forceinline__ double mirror_time(int shape, double t, double t_final) {
  return (shape == C3P_ENVT_PWC_SYMMETRIC && t > t_final / 2) ? t_final - t : t;
}
// weight of knot m in the interpolated shapes' value at time t
__device__ __forceinline__ double hat_weight(int shape, double t, double t_final, double x0, double x1, int M, int m) {
  int lo;
  double w;
  if (!interp_cell(mirror_time(shape, t, t_final), x0, x1, M, &lo, &w)) return 0.0;
  return (lo == m ? 1.0 - w : 0.0) + (lo + 1 == m ? w : 0.0);
}

// real shape value of the four real table shapes at time t (blk = the component's block, M its length)
__device__ double tab_shape_val(int shape, double t, double t_final, const double* blk, int M) {
  switch (shape) {
    case C3P_ENVT_PWC_SHAPE:
    case C3P_ENVT_PWC_SYMMETRIC: {
      int lo;
      double w;
      if (!interp_cell(mirror_time(shape, t, t_final), blk[0], blk[1], M, &lo, &w)) return 0.0;
      return (1.0 - w) * blk[2 + lo] + w * blk[2 + lo + 1];
    }
    case C3P_ENVT_FOURIER_SIN: {
      double s = 0.0;
      for (int m = 0; m < M; ++m) s += blk[m] * sin(blk[M + m] * t + blk[2 * M + m]);
      return s;
    }
    case C3P_ENVT_FOURIER_COS: {
      double s = 0.0;
      for (int m = 0; m < M; ++m) s += blk[m] * cos(blk[M + m] * t);
      return s;
    }
    default:
      return 0.0;
  }
}

struct TabTimes {
  double ts_off, dt, t_before, mask;
};
__device__ __forceinline__ TabTimes tab_times(const SynthArgs& A, const EnvP& p, int j, double a0, double a1) {
  const double t0 = A.t_start + p.delay;
  const double off0 = linspace_at(a0, a1, A.Na, 0) - t0, off1 = linspace_at(a0, a1, A.Na, A.Na > 1 ? 1 : 0) - t0;
  TabTimes r;
  r.ts_off = linspace_at(a0, a1, A.Na, j) - t0;
  r.dt = off1 - off0;
  r.t_before = 2 * off0 - off1;
  r.mask = mask_val(r.ts_off, r.dt, p.t_final);
  return r;
}

// complex envelope mask * (s(t) - [T_BEFORE] s(t_before)) of a table component at AWG sample j; pwc takes no offset, no table
// shape a DRAG term
__device__ void tab_env_eval(const SynthArgs& A, int shape, const EnvP& p, const double* blk, int M, int j, double a0, double a1,
                             double* er, double* ei, double* ts_off) {
  const TabTimes tt = tab_times(A, p, j, a0, a1);
  *ts_off = tt.ts_off;
  if (shape == C3P_ENVT_PWC) {
    const bool in = j < M;
    *er = in ? tt.mask * blk[j] : 0.0;
    *ei = in ? tt.mask * blk[M + j] : 0.0;
    return;
  }
  const double offset = p.use_t_before ? tab_shape_val(shape, tt.t_before, p.t_final, blk, M) : 0.0;
  *er = tt.mask * (tab_shape_val(shape, tt.ts_off, p.t_final, blk, M) - offset);
  *ei = 0.0;
}

// one thread per AWG sample (b, k, j); TAB: components with a C3P_ENVT_* id read their block of the coefficient table
// (X is not read without TAB; the body stands in the kernel itself: handed on through an inlined helper, the argument record
// costs the closed-form instantiation registers)
template <bool TAB>
__global__ void __launch_bounds__(TAB ? 128 : 1024) awg_iq_kernel(SynthArgs A, SynthTabArgs X) {
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)A.B * A.K * A.Na;
  if (gid >= total) return;
  const int j = (int)(gid % A.Na);
  const long bk = gid / A.Na;
  const int k = (int)(bk % A.K);
  const double dta = 1.0 / A.awg_res;
  const double a0 = A.t_start + dta / 2, a1 = A.t_end - dta / 2;
  double re = 0.0, im = 0.0;
  for (int e = 0; e < A.E; ++e) {
    const int shape = A.shape[k * A.E + e];
    if (shape < 0) continue;
    const EnvP p = load_env(A.env + (bk * A.E + e) * C3P_ENV_NPAR);
    if constexpr (TAB) {
      if (shape >= C3P_ENVT_FIRST) {
        int off, M;
        if (!tab_block(X, k * A.E + e, shape, &off, &M)) continue;
        double er, ei, ts_off;
        tab_env_eval(A, shape, p, X.tab + (bk / A.K) * (long)X.T + off, M, j, a0, a1, &er, &ei, &ts_off);
        double sn, cs;
        sincos(p.xy - p.fo * ts_off, &sn, &cs);
        re += p.amp * (er * cs - ei * sn);
        im += p.amp * (er * sn + ei * cs);
        continue;
      }
    }
    const EnvEval v = env_eval<TAB>(A, shape, p, j, a0, a1);
    const double er = v.er, ei = v.ei_unit * p.delta;
    double sn, cs;
    sincos(p.xy - p.fo * v.ts_off, &sn, &cs);
    re += p.amp * (er * cs - ei * sn);
    im += p.amp * (er * sn + ei * cs);
  }
  double* iq = A.iq + bk * 2 * A.Na;
  iq[j] = re;
  iq[A.Na + j] = im;
}

__device__ __forceinline__ int dac_src(int n, int Na, int N) {
  int src = (int)floor(((double)n + 0.5) * ((double)Na / (double)N));
  return src < Na - 1 ? src : Na - 1;
}

// ---- vector-Jacobian product: d loss/d signals -> d loss/d (amp, xy_angle, freq_offset, delta, carrier) ----
// step 1, one WAVEFRONT per AWG sample: its lanes take the simulation samples it feeds (sim_res / awg_res of them: 50 at the
// reference's resolutions -- one thread per AWG sample walked them one double-precision sincos after the other, 23 us for 1 280
// threads), fold them back onto I and Q with a fixed-order butterfly sum
__device__ __forceinline__ double wave_sum_b(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__global__ void __launch_bounds__(64) mix_bwd_kernel(SynthArgs A, const double* gsig, double* giq, double* gcar_part) {
  const long gid = blockIdx.x;  // (b, k, j)
  const int lane = threadIdx.x;
  const int j = (int)(gid % A.Na);
  const long bk = gid / A.Na;
  const double dts = 1.0 / A.sim_res;
  const double s0 = A.t_start + dts / 2, s1 = A.t_end - dts / 2;
  int n = (int)ceil((double)j * ((double)A.N / (double)A.Na) - 0.5);
  n = n < 0 ? 0 : (n > A.N ? A.N : n);
  while (n > 0 && dac_src(n - 1, A.Na, A.N) >= j) --n;
  while (n < A.N && dac_src(n, A.Na, A.N) < j) ++n;
  const double w = A.carrier[bk * 2 + 0], v2hz = A.carrier[bk * 2 + 1];
  const double* iq = A.iq + bk * 2 * A.Na;
  const double I = iq[j], Q = iq[A.Na + j];
  const double* g = gsig + bk * A.N;
  double gI = 0.0, gQ = 0.0, gw = 0.0, gv = 0.0;
  // the samples fed by j are contiguous from n on; every wavefront pass takes 64 of them
  for (int base = n; base < A.N && dac_src(base, A.Na, A.N) == j; base += 64) {
    const int m = base + lane;
    if (m < A.N && dac_src(m, A.Na, A.N) == j) {
      const double t = linspace_at(s0, s1, A.N, m);
      double sn, cs;
      sincos(w * t, &sn, &cs);
      const double gn = g[m];
      gI = fma(gn * v2hz, cs, gI);
      gQ = fma(gn * v2hz, sn, gQ);
      gw = fma(gn * v2hz * t, cs * Q - sn * I, gw);
      gv = fma(gn, cs * I + sn * Q, gv);
    }
  }
  gI = wave_sum_b(gI);
  gQ = wave_sum_b(gQ);
  gw = wave_sum_b(gw);
  gv = wave_sum_b(gv);
  if (lane == 0) {
    giq[bk * 2 * A.Na + j] = gI;
    giq[bk * 2 * A.Na + A.Na + j] = gQ;
    gcar_part[(bk * A.Na + j) * 2 + 0] = gw;
    gcar_part[(bk * A.Na + j) * 2 + 1] = gv;
  }
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// step 2, one wavefront per drive line (b, k): reduce over the AWG samples.  The sums hold for a complex envelope er + i ei
// (the DRAG term, or a pwc table component's quadrature row).
template <bool TAB>
__global__ void __launch_bounds__(64) awg_bwd_kernel(SynthArgs A, SynthTabArgs X, const double* giq, const double* gcar_part, double* genv,
                                                     double* gcar) {
  const long bk = blockIdx.x;
  const int k = (int)(bk % A.K);
  const int lane = threadIdx.x;
  const double dta = 1.0 / A.awg_res;
  const double a0 = A.t_start + dta / 2, a1 = A.t_end - dta / 2;
  const double* gI = giq + bk * 2 * A.Na;
  const double* gQ = gI + A.Na;
  double gw = 0.0, gv = 0.0;
  for (int j = lane; j < A.Na; j += 64) {
    gw += gcar_part[(bk * A.Na + j) * 2 + 0];
    gv += gcar_part[(bk * A.Na + j) * 2 + 1];
  }
  gw = wave_sum(gw);
  gv = wave_sum(gv);
  if (lane == 0) {
    gcar[bk * 2 + 0] = gw;
    gcar[bk * 2 + 1] = gv;
  }
  for (int e = 0; e < A.E; ++e) {
    double* out = genv + (bk * A.E + e) * C3P_ENV_NPAR;
    if (lane < C3P_ENV_NPAR) out[lane] = 0.0;
    const int shape = A.shape[k * A.E + e];
    if (shape < 0) continue;
    const EnvP p = load_env(A.env + (bk * A.E + e) * C3P_ENV_NPAR);
    bool tab = false;
    const double* blk = nullptr;
    int M = 0;
    if constexpr (TAB) {
      if (shape >= C3P_ENVT_FIRST) {
        int off;
        if (!tab_block(X, k * A.E + e, shape, &off, &M)) continue;
        blk = X.tab + (bk / A.K) * (long)X.T + off;
        tab = true;
      }
    }
    double g_amp = 0.0, g_xy = 0.0, g_fo = 0.0, g_delta = 0.0;
    for (int j = lane; j < A.Na; j += 64) {
      double er, ei, ei_unit, ts_off;
      if (TAB && tab) {
        tab_env_eval(A, shape, p, blk, M, j, a0, a1, &er, &ei, &ts_off);
        ei_unit = 0.0;
      } else {
        const EnvEval v = env_eval<TAB>(A, shape, p, j, a0, a1);
        er = v.er;
        ei_unit = v.ei_unit;
        ei = v.ei_unit * p.delta;
        ts_off = v.ts_off;
      }
      double sn, cs;
      sincos(p.xy - p.fo * ts_off, &sn, &cs);
      const double ur = er * cs - ei * sn, ui = er * sn + ei * cs;  // env e^{i phase}
      const double zr = p.amp * ur, zi = p.amp * ui;
      const double a = gI[j], b = gQ[j];
      g_amp += a * ur + b * ui;
      g_xy += -a * zi + b * zr;
      g_fo += ts_off * (a * zi - b * zr);
      // d z / d delta = amp * i ei_unit e^{i phase}
      g_delta += p.amp * ei_unit * (-a * sn + b * cs);
    }
    g_amp = wave_sum(g_amp);
    g_xy = wave_sum(g_xy);
    g_fo = wave_sum(g_fo);
    g_delta = wave_sum(g_delta);
    if (lane == 0) {
      out[C3P_ENV_AMP] = g_amp;
      out[C3P_ENV_XY_ANGLE] = g_xy;
      out[C3P_ENV_FREQ_OFFSET] = g_fo;
      out[C3P_ENV_DELTA] = g_delta;
    }
  }
}
// ---- cotangents of the coefficient table, gathered from giq: grad_tab [B,T] ---------------------------------------------------
// With g_j = gI_j + i gQ_j and c_j = amp g_j exp(-i phase_j):  d L / d theta = sum_j mask_j (Re c_j Re d(s_j - s_before)/d theta +
// Im c_j Im d(...)/d theta).  Every double of the row is written by exactly one lane: one finds the block its double lies in
// (none: 0; the two t_bin slots: 0, they are not differentiated).  pwc is element-wise; a knot of the interpolated shapes sums
// the AWG samples in the support of its hat, j ascending (two stretches for pwc_symmetric, and all samples for the at most two
// knots that weigh t_before); a Fourier coefficient (b, k, e, m) takes a wavefront of its own, lanes over j, then the butterfly.
// No atomics: repeated calls return the same bits.
__device__ __forceinline__ void tab_cj(const SynthArgs& A, const EnvP& p, const double* gI, int j, double a0, double a1, TabTimes* tt,
                                       double* cr, double* ci) {
  *tt = tab_times(A, p, j, a0, a1);
  double sn, cs;
  sincos(p.xy - p.fo * tt->ts_off, &sn, &cs);
  const double a = gI[j], b = gI[A.Na + j];
  *cr = tt->mask * p.amp * (a * cs + b * sn);
  *ci = tt->mask * p.amp * (b * cs - a * sn);
}

// AWG samples whose time lies in [lo, hi] (a sample of margin on both sides; the weight decides), inside [0, Na - 1]
__device__ __forceinline__ void sample_range(double lo, double hi, double off0, double dt, int Na, int* ja, int* jb) {
  double a = floor((lo - off0) / dt) - 1.0, b = ceil((hi - off0) / dt) + 1.0;
  a = a > 0.0 ? a : 0.0;  // (a NaN bound leaves the whole range)
  b = b < (double)(Na - 1) ? b : (double)(Na - 1);
  *ja = a <= (double)(Na - 1) ? (int)a : Na;
  *jb = b >= 0.0 ? (int)b : -1;
}

// the table component whose block holds double t of a row: false if none does
__device__ __forceinline__ bool tab_find(const SynthArgs& A, const SynthTabArgs& X, int t, int* ke, int* shape, int* off, int* M) {
  for (int q = 0; q < A.K * A.E; ++q) {
    const int sh = A.shape[q];
    if (sh < C3P_ENVT_FIRST || !tab_block(X, q, sh, off, M)) continue;
    if (t >= *off && t < *off + tab_block_len(sh, *M)) {
      *ke = q;
      *shape = sh;
      return true;
    }
  }
  return false;
}

// blocks [0, tiles) of a sample: 64 consecutive doubles of its row, one per lane (the Fourier blocks are left to the blocks
// below); blocks [tiles, tiles + T): one wavefront per double t, at work where t is amps[m] of a Fourier component
__global__ void __launch_bounds__(64) tab_bwd_kernel(SynthArgs A, SynthTabArgs X, const double* giq, double* gtab, int tiles) {
  const int lane = threadIdx.x;
  const int per_b = tiles + X.T;
  const long b = blockIdx.x / per_b;
  const int part = (int)(blockIdx.x % per_b);
  const double dta = 1.0 / A.awg_res;
  const double a0 = A.t_start + dta / 2, a1 = A.t_end - dta / 2;
  double* grow = gtab + b * (long)X.T;
  int ke = -1, shape = -1, off = 0, M = 0;
  if (part >= tiles) {
    // Fourier coefficient m (wave-uniform): amps[m], freqs[m] and phases[m] from one pass, lanes over j, then the butterfly
    const int t = part - tiles;
    if (!tab_find(A, X, t, &ke, &shape, &off, &M)) return;
    const bool fsin = shape == C3P_ENVT_FOURIER_SIN;
    const int m = t - off;
    if ((!fsin && shape != C3P_ENVT_FOURIER_COS) || m >= M) return;
    const long bk = b * A.K + ke / A.E;
    const EnvP p = load_env(A.env + (b * A.K * A.E + ke) * C3P_ENV_NPAR);
    const double* gI = giq + bk * 2 * A.Na;
    const double* blk = X.tab + b * (long)X.T + off;
    const double am = blk[m], fr = blk[M + m], ph = fsin ? blk[2 * M + m] : 0.0;
    double g_a = 0.0, g_f = 0.0, g_p = 0.0;
    for (int j = lane; j < A.Na; j += 64) {
      TabTimes tt;
      double cr, ci, sn, cs, sb = 0.0, cb = 0.0;
      tab_cj(A, p, gI, j, a0, a1, &tt, &cr, &ci);
      const double tb = p.use_t_before ? tt.t_before : 0.0;
      sincos(fr * tt.ts_off + ph, &sn, &cs);
      if (p.use_t_before) sincos(fr * tb + ph, &sb, &cb);
      if (fsin) {  // d/d amps = sin, d/d freqs = amps t cos, d/d phases = amps cos, each minus its value at t_before
        g_a += cr * (sn - sb);
        g_f += cr * (am * tt.ts_off * cs - am * tb * cb);
        g_p += cr * (am * cs - am * cb);
      } else {  // d/d amps = cos, d/d freqs = -amps t sin
        g_a += cr * (cs - cb);
        g_f += cr * (am * tb * sb - am * tt.ts_off * sn);
      }
    }
    g_a = wave_sum(g_a);
    g_f = wave_sum(g_f);
    g_p = wave_sum(g_p);
    if (lane == 0) {
      grow[off + m] = g_a;
      grow[off + M + m] = g_f;
      if (fsin) grow[off + 2 * M + m] = g_p;
    }
    return;
  }
  const int t = part * 64 + lane;
  if (t >= X.T) return;
  const bool found = tab_find(A, X, t, &ke, &shape, &off, &M);
  if (found && (shape == C3P_ENVT_FOURIER_SIN || shape == C3P_ENVT_FOURIER_COS)) return;
  double out = 0.0;
  if (found) {
    const long bk = b * A.K + ke / A.E;
    const EnvP p = load_env(A.env + (b * A.K * A.E + ke) * C3P_ENV_NPAR);
    const double* gI = giq + bk * 2 * A.Na;
    const int rel = t - off;
    TabTimes tt;
    double cr, ci;
    if (shape == C3P_ENVT_PWC) {
      const int j = rel < M ? rel : rel - M;
      if (j < A.Na) {
        tab_cj(A, p, gI, j, a0, a1, &tt, &cr, &ci);
        out = rel < M ? cr : ci;
      }
    } else if (rel >= 2) {
      const int m = rel - 2;
      const double* blk = X.tab + b * (long)X.T + off;
      const double x0 = blk[0], x1 = blk[1], tf_ = p.t_final;
      tt = tab_times(A, p, 0, a0, a1);
      const double off0 = tt.ts_off, dt = tt.dt;
      const double wb = p.use_t_before ? hat_weight(shape, tt.t_before, tf_, x0, x1, M, m) : 0.0;
      if (wb != 0.0) {
        // this knot weighs the offset every sample carries
        for (int j = 0; j < A.Na; ++j) {
          tab_cj(A, p, gI, j, a0, a1, &tt, &cr, &ci);
          out += cr * (hat_weight(shape, tt.ts_off, tf_, x0, x1, M, m) - wb);
        }
      } else {
        const double h = (x1 - x0) / (double)(M - 1);
        const double lo = x0 + (double)(m - 1) * h, hi = x0 + (double)(m + 1) * h;
        int ja, jb, jc = A.Na, jd = -1;
        sample_range(lo, hi, off0, dt, A.Na, &ja, &jb);
        if (shape == C3P_ENVT_PWC_SYMMETRIC) sample_range(tf_ - hi, tf_ - lo, off0, dt, A.Na, &jc, &jd);
        if (jc < ja) {  // the earlier stretch first
          int s = ja;
          ja = jc;
          jc = s;
          s = jb;
          jb = jd;
          jd = s;
        }
        for (int j = ja; j <= jb; ++j) {
          tab_cj(A, p, gI, j, a0, a1, &tt, &cr, &ci);
          out += cr * hat_weight(shape, tt.ts_off, tf_, x0, x1, M, m);
        }
        for (int j = jc > jb ? jc : jb + 1; j <= jd; ++j) {
          tab_cj(A, p, gI, j, a0, a1, &tt, &cr, &ci);
          out += cr * hat_weight(shape, tt.ts_off, tf_, x0, x1, M, m);
        }
      }
    }
  }
  grow[t] = out;
}

// one thread per simulation sample (b, k, n): nearest-neighbour upsampling, IQ mixing, V -> Hz
__global__ void mix_kernel(SynthArgs A) {
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)A.B * A.K * A.N;
  if (gid >= total) return;
  const int n = (int)(gid % A.N);
  const long bk = gid / A.N;
  const double dts = 1.0 / A.sim_res;
  const double t = linspace_at(A.t_start + dts / 2, A.t_end - dts / 2, A.N, n);
  const int src = dac_src(n, A.Na, A.N);
  const double* iq = A.iq + bk * 2 * A.Na;
  const double w = A.carrier[bk * 2 + 0], v2hz = A.carrier[bk * 2 + 1];
  double sn, cs;
  sincos(w * t, &sn, &cs);
  A.signals[gid] = (cs * iq[src] + sn * iq[A.Na + src]) * v2hz;
}

}  // namespace

namespace {
// the AWG-resolution I/Q: the table-aware instantiation only where a coefficient table travels with the rows
void launch_awg_iq(const SynthArgs& A, const SynthTabArgs* X, long ta, hipStream_t st) {
  if (X)
    C3P_LAUNCH(awg_iq_kernel<true>, dim3((unsigned)((ta + 127) / 128)), dim3(128), 0, st, A, *X);
  else
    C3P_LAUNCH(awg_iq_kernel<false>, dim3((unsigned)((ta + 127) / 128)), dim3(128), 0, st, A, SynthTabArgs{});
}
// giq -> genv, gcar (and, with a table, gtab)
void launch_awg_bwd(const SynthArgs& A, const SynthTabArgs* X, const double* giq, const double* gcar_part, double* genv, double* gcar,
                    double* gtab, hipStream_t st) {
  const unsigned lines = (unsigned)(A.B * A.K);
  if (!X) {
    C3P_LAUNCH(awg_bwd_kernel<false>, dim3(lines), dim3(64), 0, st, A, SynthTabArgs{}, giq, gcar_part, genv, gcar);
    return;
  }
  C3P_LAUNCH(awg_bwd_kernel<true>, dim3(lines), dim3(64), 0, st, A, *X, giq, gcar_part, genv, gcar);
  const int tiles = (X->T + 63) / 64;
  if (tiles > 0) C3P_LAUNCH(tab_bwd_kernel, dim3((unsigned)((long)A.B * (tiles + X->T))), dim3(64), 0, st, A, *X, giq, gtab, tiles);
}
}  // namespace

// ---- the device chain of a flux line: AWG -> DAC -> Response -> Mixer -> VoltsToHertz | FluxTuning --------------------------
// (reference: c3/generator/devices.py:585-642 Response, c3/utils/tf_utils.py:476-518 tf_convolve_legacy, devices.py:457-525
//  FluxTuning).  The reference's zero-padded FFT product with its [M-1 : N+M-1] window is the causal FIR with one sample of
//  delay, y[n] = sum_{m < min(M, n)} h[m] x[n-1-m]; it is evaluated here in that form, m ascending.  x, the upsampled AWG
//  I/Q, exists only in LDS: a block reads the AWG-resolution rows (L2) and keeps the stretch of x its tile's taps reach.
namespace {

constexpr int CH_TN = 256;  // samples per tile = threads per block
constexpr int CH_TC = 256;  // taps per LDS chunk (one tap loaded per thread)
constexpr int CH_NP = 7;    // partial sums per tile: LO frequency, V->Hz, phi_0, phi, omega_0, anhar, d
constexpr int CH_PS = 8;    // their stride

// M = floor(rise_time * sim_res) of the one double product (devices.py:614); 0 = no Response stage
__device__ __forceinline__ int chain_tap_count(double rise_time, double sim_res) {
  if (!(rise_time > 0.0)) return 0;
  const double m = floor(__dmul_rn(rise_time, sim_res));
  return m < 1073741824.0 ? (int)m : 1073741824;
}

// tap m of the rise function before normalisation (devices.py:615-627)
__device__ __forceinline__ double rise_fun(double rt, double sim_res, int M, int m) {
  const double cen = (rt + 1.0 / sim_res) / 2, sg = rt / 4;
  const double u = linspace_at(0.0, rt, M, m) - cen, v = -1.0 - cen;
  return exp(-(u * u) / (2 * sg * sg)) - exp(-(v * v) / (2 * sg * sg));
}

// one wavefront per line (b, k): all M terms summed in a fixed order (lane-strided, then the butterfly), the first
// min(M, N - 1) normalised taps stored -- a later tap multiplies samples before the first one
__global__ void __launch_bounds__(64) chain_taps_kernel(SynthChainArgs C) {
  const long bk = blockIdx.x;
  const int lane = threadIdx.x;
  const double rt = C.line[bk * C3P_LINE_NPAR + C3P_LINE_RISE_TIME];
  const int M = chain_tap_count(rt, C.S.sim_res);
  if (M == 0) return;
  double s = 0.0;
  for (int m = lane; m < M; m += 64) s += rise_fun(rt, C.S.sim_res, M, m);
  s = wave_sum(s);
  const int Mt = M < C.S.N - 1 ? M : C.S.N - 1;
  double* h = C.taps + bk * C.tap_stride;
  for (int m = lane; m < Mt; m += 64) h[m] = rise_fun(rt, C.S.sim_res, M, m) / s;
}

// I, Q the mixer reads at sample n0 + threadIdx.x of line bk; every thread of the block calls it (Mt is block-uniform)
__device__ __forceinline__ void chain_fir_tile(const SynthChainArgs& C, long bk, int n0, int Mt, double* s_h, double* s_xi,
                                               double* s_xq, double& I, double& Q) {
  const int i = threadIdx.x, n = n0 + i, Na = C.S.Na, N = C.S.N;
  const double* iq = C.S.iq + bk * 2 * Na;
  I = 0.0;
  Q = 0.0;
  if (Mt == 0) {
    if (n < N) {
      const int src = dac_src(n, Na, N);
      I = iq[src];
      Q = iq[Na + src];
    }
    return;
  }
  const double* h = C.taps + bk * C.tap_stride;
  // taps from n0 + CH_TN - 1 on reach before sample 0 for the whole tile
  const int Mtile = Mt < n0 + CH_TN - 1 ? Mt : n0 + CH_TN - 1;
  double aI = 0.0, aQ = 0.0;
  for (int c0 = 0; c0 < Mtile; c0 += CH_TC) {
    __syncthreads();
    const int nc = Mtile - c0 < CH_TC ? Mtile - c0 : CH_TC;
    if (i < nc) s_h[i] = h[c0 + i];
    const int base = n0 - c0 - CH_TC;  // sample index of s_x[0]
    for (int p = i; p < CH_TN + CH_TC - 1; p += CH_TN) {
      const int idx = base + p;
      double xi = 0.0, xq = 0.0;
      if (idx >= 0 && idx < N) {
        const int src = dac_src(idx, Na, N);
        xi = iq[src];
        xq = iq[Na + src];
      }
      s_xi[p] = xi;
      s_xq[p] = xq;
    }
    __syncthreads();
    const int off = i + CH_TC - 1;  // x[n - 1 - (c0 + mm)] = s_x[off - mm]
    for (int mm = 0; mm < nc; ++mm) {
      const double hh = s_h[mm];
      aI = fma(hh, s_xi[off - mm], aI);
      aQ = fma(hh, s_xq[off - mm], aQ);
    }
  }
  I = aI;
  Q = aQ;
}

struct FluxP {
  double phi0, phi, w0, anhar, d;
};
__device__ __forceinline__ FluxP load_flux(const double* lp) {
  return FluxP{lp[C3P_LINE_PHI_0], lp[C3P_LINE_PHI], lp[C3P_LINE_OMEGA_0], lp[C3P_LINE_ANHAR], lp[C3P_LINE_D]};
}
// f = (cos^2 u + d^2 sin^2 u)^(1/4), u = pi x / phi_0 (devices.py:481-495; d = 0: the branch without d), with df/du, df/dd
struct FluxV {
  double f, du, dd, u;
};
__device__ __forceinline__ FluxV flux_parts(double x, const FluxP& p) {
  FluxV r;
  r.u = M_PI * x / p.phi0;
  double s, c;
  sincos(r.u, &s, &c);
  r.f = sqrt(sqrt(c * c + p.d * p.d * (s * s)));
  const double q34 = 0.5 / (r.f * r.f * r.f);
  r.du = q34 * s * c * (p.d * p.d - 1.0);
  r.dd = q34 * p.d * s * s;
  return r;
}
// FluxTuning.get_freq (devices.py:497-502)
__device__ __forceinline__ double flux_freq(double x, const FluxP& p) { return (p.w0 - p.anhar) * flux_parts(x, p).f + p.anhar; }

// one block per tile of CH_TN consecutive samples of one line: DAC -> Response -> Mixer -> V->Hz | FluxTuning
__global__ void __launch_bounds__(CH_TN) chain_fwd_kernel(SynthChainArgs C, int nt) {
  __shared__ double s_h[CH_TC], s_xi[CH_TN + CH_TC - 1], s_xq[CH_TN + CH_TC - 1];
  const SynthArgs& A = C.S;
  const long bk = blockIdx.x / nt;
  const int n0 = (int)(blockIdx.x % nt) * CH_TN, n = n0 + threadIdx.x;
  const int k = (int)(bk % A.K);
  const double* lp = C.line + bk * C3P_LINE_NPAR;
  int Mt = chain_tap_count(lp[C3P_LINE_RISE_TIME], A.sim_res);
  Mt = Mt < A.N - 1 ? Mt : A.N - 1;
  double I, Q;
  chain_fir_tile(C, bk, n0, Mt, s_h, s_xi, s_xq, I, Q);
  if (n >= A.N) return;
  const double dts = 1.0 / A.sim_res;
  const double t = linspace_at(A.t_start + dts / 2, A.t_end - dts / 2, A.N, n);
  const double w = A.carrier[bk * 2 + 0], v2hz = A.carrier[bk * 2 + 1];
  double sn, cs;
  sincos(w * t, &sn, &cs);
  double out;
  if (C.kind[k] == C3P_LINE_KIND_FLUX) {
    const FluxP p = load_flux(lp);
    out = flux_freq(p.phi + (cs * I + sn * Q), p) - flux_freq(p.phi, p);
  } else {
    out = (cs * I + sn * Q) * v2hz;
  }
  A.signals[bk * A.N + n] = out;
}

// backward step 1, same tiling: mixed[n] again, the cotangent of the mixer output times cos / sin (gcs [B,K,2,N]) and the
// tile's partial sums for the LO frequency, V->Hz and the five line parameters (part [B,K,nt,CH_PS]); wavefront butterfly,
// then the four wavefronts in order
__global__ void __launch_bounds__(CH_TN) chain_bwd_sample_kernel(SynthChainArgs C, int nt, const double* gsig, double* gcs, double* part) {
  __shared__ double s_h[CH_TC], s_xi[CH_TN + CH_TC - 1], s_xq[CH_TN + CH_TC - 1];
  __shared__ double s_red[CH_TN / 64][CH_PS];
  const SynthArgs& A = C.S;
  const long bk = blockIdx.x / nt;
  const int n0 = (int)(blockIdx.x % nt) * CH_TN, n = n0 + threadIdx.x;
  const int k = (int)(bk % A.K);
  const double* lp = C.line + bk * C3P_LINE_NPAR;
  int Mt = chain_tap_count(lp[C3P_LINE_RISE_TIME], A.sim_res);
  Mt = Mt < A.N - 1 ? Mt : A.N - 1;
  double I, Q;
  chain_fir_tile(C, bk, n0, Mt, s_h, s_xi, s_xq, I, Q);
  double v[CH_NP];
  for (int q = 0; q < CH_NP; ++q) v[q] = 0.0;
  if (n < A.N) {
    const double dts = 1.0 / A.sim_res;
    const double t = linspace_at(A.t_start + dts / 2, A.t_end - dts / 2, A.N, n);
    const double w = A.carrier[bk * 2 + 0], v2hz = A.carrier[bk * 2 + 1];
    double sn, cs;
    sincos(w * t, &sn, &cs);
    const double mixed = cs * I + sn * Q;
    const double g = gsig[bk * A.N + n];
    double gm;
    if (C.kind[k] == C3P_LINE_KIND_FLUX) {
      const FluxP p = load_flux(lp);
      const FluxV f1 = flux_parts(p.phi + mixed, p), f0 = flux_parts(p.phi, p);
      const double a = p.w0 - p.anhar, kk = M_PI / p.phi0;
      gm = g * a * f1.du * kk;
      v[2] = g * a * (f0.du * f0.u - f1.du * f1.u) / p.phi0;
      v[3] = g * a * kk * (f1.du - f0.du);
      v[4] = g * (f1.f - f0.f);
      v[5] = g * (f0.f - f1.f);
      v[6] = g * a * (f1.dd - f0.dd);
    } else {
      gm = g * v2hz;
      v[1] = g * mixed;
    }
    v[0] = gm * t * (cs * Q - sn * I);
    gcs[(bk * 2 + 0) * A.N + n] = gm * cs;
    gcs[(bk * 2 + 1) * A.N + n] = gm * sn;
  }
  for (int q = 0; q < CH_NP; ++q) v[q] = wave_sum(v[q]);
  if ((threadIdx.x & 63) == 0)
    for (int q = 0; q < CH_NP; ++q) s_red[threadIdx.x >> 6][q] = v[q];
  __syncthreads();
  if (threadIdx.x < CH_NP) {
    double s = s_red[0][threadIdx.x];
    for (int wv = 1; wv < CH_TN / 64; ++wv) s += s_red[wv][threadIdx.x];
    part[(long)blockIdx.x * CH_PS + threadIdx.x] = s;
  }
}

// backward step 2, one wavefront per AWG sample (b, k, j): the transposed FIR over the samples j feeds,
//   gI[j] = sum_{i: src(i) = j} sum_m h[m] gc[i+1+m]   (likewise gQ),
// lanes over i, then the butterfly.  The wavefront of j = 0 also folds the line's tile partials: the carrier pair goes to
// gcar_part[.., 0, :] (zeros for j > 0, so awg_bwd_kernel's sum over j returns it), the line parameters to gline.
__global__ void __launch_bounds__(64) chain_bwd_awg_kernel(SynthChainArgs C, int nt, const double* gcs, const double* part, double* giq,
                                                           double* gcar_part, double* gline) {
  const SynthArgs& A = C.S;
  const long gid = blockIdx.x;
  const int lane = threadIdx.x;
  const int j = (int)(gid % A.Na);
  const long bk = gid / A.Na;
  int n = (int)ceil((double)j * ((double)A.N / (double)A.Na) - 0.5);
  n = n < 0 ? 0 : (n > A.N ? A.N : n);
  while (n > 0 && dac_src(n - 1, A.Na, A.N) >= j) --n;
  while (n < A.N && dac_src(n, A.Na, A.N) < j) ++n;
  int Mt = chain_tap_count(C.line[bk * C3P_LINE_NPAR + C3P_LINE_RISE_TIME], A.sim_res);
  Mt = Mt < A.N - 1 ? Mt : A.N - 1;
  const double* gc = gcs + bk * 2 * A.N;
  const double* gs = gc + A.N;
  const double* h = C.taps + bk * C.tap_stride;
  double gI = 0.0, gQ = 0.0;
  for (int base = n; base < A.N && dac_src(base, A.Na, A.N) == j; base += 64) {
    const int i = base + lane;
    if (i < A.N && dac_src(i, A.Na, A.N) == j) {
      if (Mt == 0) {
        gI += gc[i];
        gQ += gs[i];
      } else {
        const int mmax = Mt < A.N - 1 - i ? Mt : A.N - 1 - i;
        double a = 0.0, b = 0.0;
        for (int m = 0; m < mmax; ++m) {
          a = fma(h[m], gc[i + 1 + m], a);
          b = fma(h[m], gs[i + 1 + m], b);
        }
        gI += a;
        gQ += b;
      }
    }
  }
  gI = wave_sum(gI);
  gQ = wave_sum(gQ);
  if (lane == 0) {
    giq[bk * 2 * A.Na + j] = gI;
    giq[bk * 2 * A.Na + A.Na + j] = gQ;
  }
  double* gp = gcar_part + (bk * A.Na + j) * 2;
  if (j != 0) {
    if (lane < 2) gp[lane] = 0.0;
    return;
  }
  double v[CH_NP];
  for (int q = 0; q < CH_NP; ++q) {
    double s = 0.0;
    for (int tl = lane; tl < nt; tl += 64) s += part[(bk * nt + tl) * CH_PS + q];
    v[q] = wave_sum(s);
  }
  if (lane == 0) {
    gp[0] = v[0];
    gp[1] = v[1];
    double* gl = gline + bk * C3P_LINE_NPAR;
    gl[C3P_LINE_RISE_TIME] = 0.0;  // the tap count is a floor: not differentiated
    gl[C3P_LINE_PHI_0] = v[2];
    gl[C3P_LINE_PHI] = v[3];
    gl[C3P_LINE_OMEGA_0] = v[4];
    gl[C3P_LINE_ANHAR] = v[5];
    gl[C3P_LINE_D] = v[6];
  }
}

}  // namespace

int c3p_chain_tiles(int N) { return (N + CH_TN - 1) / CH_TN; }
int c3p_chain_part_stride() { return CH_PS; }

// ---- the two launchers: C.kind == NULL is the standard drive line, X == NULL a call without a coefficient table --------------
hipError_t c3p_launch_synth(const SynthChainArgs& C, const SynthTabArgs* X, hipStream_t st) {
  const SynthArgs& A = C.S;
  const long lines = (long)A.B * A.K, ta = lines * A.Na, ts = lines * A.N;
  if (ta == 0 || ts == 0) return hipSuccess;
  launch_awg_iq(A, X, ta, st);
  if (C.kind) C3P_LAUNCH(chain_taps_kernel, dim3((unsigned)lines), dim3(64), 0, st, C);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (C.kind) {
    const int nt = c3p_chain_tiles(A.N);
    C3P_LAUNCH(chain_fwd_kernel, dim3((unsigned)(lines * nt)), dim3(CH_TN), 0, st, C, nt);
  } else {
    C3P_LAUNCH(mix_kernel, dim3((unsigned)((ts + 255) / 256)), dim3(256), 0, st, A);
  }
  return hipGetLastError();
}

hipError_t c3p_launch_synth_vjp(const SynthChainArgs& C, const SynthTabArgs* X, const double* gsig, const SynthVjpBufs& V, hipStream_t st) {
  const SynthArgs& A = C.S;
  const long lines = (long)A.B * A.K, ta = lines * A.Na;
  if (ta == 0 || A.N == 0) return hipSuccess;
  launch_awg_iq(A, X, ta, st);
  if (C.kind) {
    const int nt = c3p_chain_tiles(A.N);
    C3P_LAUNCH(chain_taps_kernel, dim3((unsigned)lines), dim3(64), 0, st, C);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    C3P_LAUNCH(chain_bwd_sample_kernel, dim3((unsigned)(lines * nt)), dim3(CH_TN), 0, st, C, nt, gsig, V.gcs, V.part);
    C3P_LAUNCH(chain_bwd_awg_kernel, dim3((unsigned)ta), dim3(64), 0, st, C, nt, (const double*)V.gcs, (const double*)V.part, V.giq,
               V.gcar_part, V.gline);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  } else {
    C3P_LAUNCH(mix_bwd_kernel, dim3((unsigned)ta), dim3(64), 0, st, A, gsig, V.giq, V.gcar_part);
  }
  launch_awg_bwd(A, X, (const double*)V.giq, (const double*)V.gcar_part, V.genv, V.gcar, V.gtab, st);
  return hipGetLastError();
}

// ---- line filters, DC offset and crosstalk (c3p_synth_filt): the stage kernels and their two launchers ------------------------
#include "c3p_signal_filt.inc"
