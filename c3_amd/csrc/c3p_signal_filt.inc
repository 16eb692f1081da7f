// Line filters, DC offset and crosstalk of c3p_synth_filt (included at the end of c3p_signal.hip).
//   AWG -> DAC -> [legacy Response] -> stage 0 .. stage F-1 -> Mixer -> + dc_offset -> VoltsToHertz | FluxTuning -> Crosstalk
// (reference: c3/generator/devices.py:646-701 ResponseFFT, :705-787 StepFuncFilter and its three step responses, :1039-1059
//  DC_Offset, :225-292 Crosstalk, c3/utils/tf_utils.py:439-473 tf_convolve).  Every stage is the causal convolution
//  y[n] = sum_{m <= n} h[m] x[n-m] over N taps: the zero-padded FFT product of tf_convolve, summed directly with m ascending.
// The stages work on materialised [B,K,2,N] buffers: the upsampled DAC output (after the legacy Response, if the line has one)
// is written once, every stage reads its predecessor's buffer.  The vjp recomputes the buffers and walks the stages backwards
// with the same convolution kernel: the input cotangent is the convolution of the reversed cotangent, the tap cotangent
// gh[m] = sum_{n >= m} gyI[n] xI[n-m] + gyQ[n] xQ[n-m] the convolution of the stage input with the reversed cotangent.
namespace {

constexpr int FC_R = 8;                    // consecutive outputs per thread, for I and for Q
constexpr int FC_NT = 128;                 // threads per block
constexpr int FC_TILE = FC_R * FC_NT;      // outputs per block
constexpr int FC_TC = 256;                 // taps per LDS chunk
constexpr int FC_XB = (FC_TILE + FC_TC) / 8;  // 8-sample groups of x a chunk reaches
constexpr int FC_XS = 10;  // doubles a group takes in LDS: lane t reads group t + const as 4 x 16 bytes, and 80 bytes from lane
                           // to lane put 16 lanes on 64 different banks (64 bytes: 4 lanes would share each bank)
constexpr int FL_NP = 8;   // partial sums per sample tile: the seven of the chain (CH_NP) and the DC offset
static_assert(FL_NP == CH_PS, "the tile partials share the chain's stride");
static_assert(FC_TC % 16 == 0 && FC_TILE % 8 == 0, "the tap loop takes two groups of 8 per pass");

struct FiltConv {
  const double* a;  // the operand the thread broadcasts: a + bk * a_ls (+ a_cs for Q; 0: one row for both)
  long a_ls, a_cs;
  const double* x;  // [lines,2,N]: the operand that slides through the registers
  double* y;        // [lines,2,N], or [lines,N] for the tap cotangent
  const int* kind;  // [K,F]
  int K, F, f, N, nt;
  long lines;
  int rev_x, rev_y;  // read x / write y back to front
};

__device__ __forceinline__ void fc_load8(double (&v)[8], const double* s, int group) {
  const double2* p = reinterpret_cast<const double2*>(s + group * FC_XS);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double2 d = p[q];
    v[2 * q] = d.x;
    v[2 * q + 1] = d.y;
  }
}

// eight taps u0 .. u0 + 7 of the chunk onto the thread's eight outputs: output r takes tap u times x[r - u], which lies in
// `hi` (the group of the outputs' own offsets) for r >= u and in `lo` (the group before) otherwise
template <bool GH>
__device__ __forceinline__ void fc_step(const double (*s_a)[FC_TC], int u0, const double (&hiI)[8], const double (&loI)[8],
                                        const double (&hiQ)[8], const double (&loQ)[8], double (&accI)[8], double (&accQ)[8]) {
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const double aI = s_a[0][u0 + u];
    const double aQ = GH ? s_a[1][u0 + u] : aI;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int d = r - u;
      accI[r] = fma(aI, d >= 0 ? hiI[d] : loI[8 + d], accI[r]);
      accQ[r] = fma(aQ, d >= 0 ? hiQ[d] : loQ[8 + d], accQ[r]);
    }
  }
}

// y[i] = sum_{m <= i} a[m] xx[i - m] for I and Q, i in one tile of FC_TILE outputs of one line; xx is x, read back to front
// under rev_x, and y is written back to front under rev_y.  GH: a has a row per channel and the two sums are added (the tap
// cotangent); otherwise one row serves both (a stage's taps).  A thread owns FC_R consecutive outputs and keeps the 2 FC_R - 1
// samples of x its next eight taps reach in registers: one 64-byte LDS read of x per channel and one broadcast read of eight
// taps serve 128 FMAs (1.5 bytes of LDS traffic per FMA).  Tile i has (i + 1) FC_TILE taps of work: the blocks are numbered
// from the last tile down, so the long tiles start first and the short ones fill the tail.
template <bool GH>
__global__ void __launch_bounds__(FC_NT) filt_conv_kernel(FiltConv P) {
  __shared__ double s_a[GH ? 2 : 1][FC_TC];
  __shared__ __attribute__((aligned(16))) double s_x[2][FC_XB * FC_XS];
  const int t = threadIdx.x, N = P.N;
  const long bk = blockIdx.x % P.lines;
  const int n0 = (P.nt - 1 - (int)(blockIdx.x / P.lines)) * FC_TILE, nt0 = n0 + FC_R * t;
  const int kind = P.kind[(int)(bk % P.K) * P.F + P.f];
  const double* x = P.x + bk * 2 * N;
  if (GH) {
    if (kind < C3P_FILT_EXP_IIR || kind >= C3P_FILT_NKINDS) return;  // no differentiated parameter: gh is not read
  } else if (kind < 0 || kind >= C3P_FILT_NKINDS) {  // unused slot: the buffer passes through
    double* y = P.y + bk * 2 * N;
    for (int r = 0; r < FC_R; ++r)
      if (nt0 + r < N) {
        y[nt0 + r] = x[nt0 + r];
        y[N + nt0 + r] = x[N + nt0 + r];
      }
    return;
  }
  const double* a = P.a + bk * P.a_ls;
  double accI[8], accQ[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) accI[r] = accQ[r] = 0.0;
  const int mmax = N < n0 + FC_TILE ? N : n0 + FC_TILE;  // later taps reach before sample 0 for the whole tile
  for (int c0 = 0; c0 < mmax; c0 += FC_TC) {
    __syncthreads();
    for (int u = t; u < FC_TC; u += FC_NT) {
      const int m = c0 + u;
      s_a[0][u] = m < N ? a[m] : 0.0;
      if (GH) s_a[1][u] = m < N ? a[P.a_cs + m] : 0.0;
    }
    const int p0 = n0 - c0 - FC_TC;  // sample index of LDS position 0
    for (int q = t; q < FC_TILE + FC_TC; q += FC_NT) {
      const int p = p0 + q;
      double xi = 0.0, xq = 0.0;
      if (p >= 0 && p < N) {
        const int s = P.rev_x ? N - 1 - p : p;
        xi = x[s];
        xq = x[N + s];
      }
      const int o = (q >> 3) * FC_XS + (q & 7);
      s_x[0][o] = xi;
      s_x[1][o] = xq;
    }
    __syncthreads();
    // a tap beyond the thread's last output multiplies zeros only
    const int ulim = nt0 + FC_R - 1 - c0;
    const int g0 = t + FC_TC / 8;  // the group of the thread's outputs at tap c0
    double hiI[8], hiQ[8], loI[8], loQ[8];
    fc_load8(hiI, s_x[0], g0);
    fc_load8(hiQ, s_x[1], g0);
    for (int u0 = 0; u0 < FC_TC && u0 <= ulim; u0 += 16) {
      const int g = g0 - (u0 >> 3);
      fc_load8(loI, s_x[0], g - 1);
      fc_load8(loQ, s_x[1], g - 1);
      fc_step<GH>(s_a, u0, hiI, loI, hiQ, loQ, accI, accQ);
      fc_load8(hiI, s_x[0], g - 2);
      fc_load8(hiQ, s_x[1], g - 2);
      fc_step<GH>(s_a, u0 + 8, loI, hiI, loQ, hiQ, accI, accQ);
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int i = nt0 + r;
    if (i >= N) continue;
    const int pos = P.rev_y ? N - 1 - i : i;
    if (GH) {
      P.y[bk * N + pos] = accI[r] + accQ[r];
    } else {
      P.y[bk * 2 * N + pos] = accI[r];
      P.y[bk * 2 * N + N + pos] = accQ[r];
    }
  }
}

#ifdef C3P_FILT_PLAIN
// A/B baseline, not part of the regular build (tools/ab_build.sh plain c3p_signal.hip -DC3P_FILT_PLAIN; measured in
// profiles/r24/README.md): the tile loop of chain_fir_tile carried to N taps, without its sample of delay -- one output pair
// per thread, two LDS doubles read for every two FMAs.  Forward stages only.
__global__ void __launch_bounds__(CH_TN) filt_conv_plain_kernel(FiltConv P) {
  __shared__ double s_h[CH_TC], s_xi[CH_TN + CH_TC - 1], s_xq[CH_TN + CH_TC - 1];
  const int i = threadIdx.x, N = P.N;
  const long bk = blockIdx.x % P.lines;
  const int n0 = (P.nt - 1 - (int)(blockIdx.x / P.lines)) * CH_TN, n = n0 + i;
  const int kind = P.kind[(int)(bk % P.K) * P.F + P.f];
  const double* x = P.x + bk * 2 * N;
  double* y = P.y + bk * 2 * N;
  if (kind < 0 || kind >= C3P_FILT_NKINDS) {
    if (n < N) {
      y[n] = x[n];
      y[N + n] = x[N + n];
    }
    return;
  }
  const double* h = P.a + bk * P.a_ls;
  const int Mtile = N < n0 + CH_TN ? N : n0 + CH_TN;
  double aI = 0.0, aQ = 0.0;
  for (int c0 = 0; c0 < Mtile; c0 += CH_TC) {
    __syncthreads();
    const int nc = Mtile - c0 < CH_TC ? Mtile - c0 : CH_TC;
    if (i < nc) s_h[i] = h[c0 + i];
    const int base = n0 - c0 - (CH_TC - 1);  // sample index of s_x[0]
    for (int p = i; p < CH_TN + CH_TC - 1; p += CH_TN) {
      const int idx = base + p;
      const bool in = idx >= 0 && idx < N;
      s_xi[p] = in ? x[idx] : 0.0;
      s_xq[p] = in ? x[N + idx] : 0.0;
    }
    __syncthreads();
    const int off = i + CH_TC - 1;  // x[n - (c0 + mm)] = s_x[off - mm]
    for (int mm = 0; mm < nc; ++mm) {
      const double hh = s_h[mm];
      aI = fma(hh, s_xi[off - mm], aI);
      aQ = fma(hh, s_xq[off - mm], aQ);
    }
  }
  if (n < N) {
    y[n] = aI;
    y[N + n] = aQ;
  }
}
#endif

// the signal's own centred grid (devices.py:86-122): absolute time, as StepFuncFilter.process reads it
__device__ __forceinline__ double filt_ts(const SynthArgs& A, int m) {
  const double dts = 1.0 / A.sim_res;
  return linspace_at(A.t_start + dts / 2, A.t_end - dts / 2, A.N, m);
}

// step response of the three StepFuncFilter kinds (devices.py:747-751, :767-769, :785-787)
__device__ __forceinline__ double filt_step(int kind, double t, double tau, double amp) {
  switch (kind) {
    case C3P_FILT_EXP_IIR:
      return 1.0 + amp * exp(-t / tau);
    case C3P_FILT_HIGHPASS_EXP:
      return exp(-t / tau);
    default:  // C3P_FILT_SKIN_EFFECT, tau = alpha
      return erfc(tau / 21.0 / sqrt(fabs(t)));
  }
}
// its derivatives by the TAU and the AMP slot
__device__ __forceinline__ void filt_step_der(int kind, double t, double tau, double amp, double* d_tau, double* d_amp) {
  *d_amp = 0.0;
  if (kind == C3P_FILT_SKIN_EFFECT) {
    const double q = 21.0 * sqrt(fabs(t)), z = tau / q;
    *d_tau = t != 0.0 ? -2.0 / sqrt(M_PI) * exp(-z * z) / q : 0.0;
    return;
  }
  const double e = exp(-t / tau);
  *d_tau = (kind == C3P_FILT_EXP_IIR ? amp : 1.0) * e * t / (tau * tau);
  if (kind == C3P_FILT_EXP_IIR) *d_amp = e;
}

// tap m of ResponseFFT before normalisation (devices.py:675-688): the centre takes - 1/sim_res where the legacy stage takes +
__device__ __forceinline__ double rise_fun_fft(double rt, double sim_res, int M, int m) {
  const double cen = (rt - 1.0 / sim_res) / 2, sg = rt / 4;
  const double u = linspace_at(0.0, rt, M, m) - cen, v = -1.0 - cen;
  return exp(-(u * u) / (2 * sg * sg)) - exp(-(v * v) / (2 * sg * sg));
}

// one block per (b, k, stage): h[0..N).  ResponseFFT: every wavefront sums all M terms in the order of chain_taps_kernel
// (lane-strided, then the butterfly), so each holds the same normaliser.
__global__ void __launch_bounds__(256) filt_taps_kernel(SynthArgs A, SynthFiltArgs Fa) {
  const long bkf = blockIdx.x;
  const long bk = bkf / Fa.F;
  const int f = (int)(bkf % Fa.F), k = (int)(bk % A.K);
  const int kind = Fa.fkind[k * Fa.F + f];
  if (kind < 0 || kind >= C3P_FILT_NKINDS) return;
  const double tau = Fa.fpar[bkf * C3P_FILT_NPAR + C3P_FILT_TAU], amp = Fa.fpar[bkf * C3P_FILT_NPAR + C3P_FILT_AMP];
  double* h = Fa.h + bkf * A.N;
  if (kind == C3P_FILT_RESPONSE_FFT) {
    const int M = chain_tap_count(tau, A.sim_res), lane = threadIdx.x & 63;
    double s = 0.0;
    for (int m = lane; m < M; m += 64) s += rise_fun_fft(tau, A.sim_res, M, m);
    s = wave_sum(s);
    for (int m = threadIdx.x; m < A.N; m += 256) h[m] = m < M ? rise_fun_fft(tau, A.sim_res, M, m) / s : 0.0;
    return;
  }
  for (int m = threadIdx.x; m < A.N; m += 256) {
    const double s1 = filt_step(kind, filt_ts(A, m), tau, amp);
    h[m] = m > 0 ? s1 - filt_step(kind, filt_ts(A, m - 1), tau, amp) : s1;
  }
}

// the four wavefronts of a 256-thread block in order, after the butterfly in each
__device__ __forceinline__ double filt_block_sum(double v, double* s_red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// one block per line (b, k): d loss / d {TAU, AMP} of stage f = sum_m gh[m] d h[m] / d theta, thread-strided, then folded
__global__ void __launch_bounds__(256) filt_par_kernel(SynthArgs A, SynthFiltArgs Fa, int f, const double* gh, double* gfilt) {
  __shared__ double s_red[4];
  const long bk = blockIdx.x;
  const long bkf = bk * Fa.F + f;
  const int kind = Fa.fkind[(int)(bk % A.K) * Fa.F + f];
  double g_tau = 0.0, g_amp = 0.0;
  if (kind >= C3P_FILT_EXP_IIR && kind < C3P_FILT_NKINDS) {  // block-uniform
    const double tau = Fa.fpar[bkf * C3P_FILT_NPAR + C3P_FILT_TAU], amp = Fa.fpar[bkf * C3P_FILT_NPAR + C3P_FILT_AMP];
    const double* g = gh + bk * A.N;
    for (int m = threadIdx.x; m < A.N; m += 256) {
      double t1, a1, t0 = 0.0, a0 = 0.0;
      filt_step_der(kind, filt_ts(A, m), tau, amp, &t1, &a1);
      if (m > 0) filt_step_der(kind, filt_ts(A, m - 1), tau, amp, &t0, &a0);
      g_tau = fma(g[m], t1 - t0, g_tau);
      g_amp = fma(g[m], a1 - a0, g_amp);
    }
    g_tau = filt_block_sum(g_tau, s_red);
    g_amp = filt_block_sum(g_amp, s_red);
  }
  if (threadIdx.x == 0) {
    gfilt[bkf * C3P_FILT_NPAR + C3P_FILT_TAU] = g_tau;
    gfilt[bkf * C3P_FILT_NPAR + C3P_FILT_AMP] = g_amp;
  }
}

// the chain's Mt of a line; no lines: no legacy stage
__device__ __forceinline__ int filt_legacy_taps(const SynthChainArgs& C, long bk) {
  if (!C.line) return 0;
  const int Mt = chain_tap_count(C.line[bk * C3P_LINE_NPAR + C3P_LINE_RISE_TIME], C.S.sim_res);
  return Mt < C.S.N - 1 ? Mt : C.S.N - 1;
}

// stage buffer 0: DAC (and the legacy Response) as chain_fwd_kernel forms the mixer's input, one block per CH_TN samples
__global__ void __launch_bounds__(CH_TN) filt_up_kernel(SynthChainArgs C, int nt, double* buf) {
  __shared__ double s_h[CH_TC], s_xi[CH_TN + CH_TC - 1], s_xq[CH_TN + CH_TC - 1];
  const long bk = blockIdx.x / nt;
  const int n = (int)(blockIdx.x % nt) * CH_TN + threadIdx.x;
  double I, Q;
  chain_fir_tile(C, bk, n - threadIdx.x, filt_legacy_taps(C, bk), s_h, s_xi, s_xq, I, Q);
  if (n >= C.S.N) return;
  buf[bk * 2 * C.S.N + n] = I;
  buf[bk * 2 * C.S.N + C.S.N + n] = Q;
}

// one thread per sample (b, k, n): Mixer, + dc_offset, VoltsToHertz | FluxTuning, written as mix_kernel and chain_fwd_kernel
// write them
__global__ void filt_mix_kernel(SynthChainArgs C, const double* buf, const double* dc, double* out) {
  const SynthArgs& A = C.S;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)A.B * A.K * A.N) return;
  const int n = (int)(gid % A.N);
  const long bk = gid / A.N;
  const double I = buf[bk * 2 * A.N + n], Q = buf[bk * 2 * A.N + A.N + n];
  const double dts = 1.0 / A.sim_res;
  const double t = linspace_at(A.t_start + dts / 2, A.t_end - dts / 2, A.N, n);
  const double w = A.carrier[bk * 2 + 0], v2hz = A.carrier[bk * 2 + 1];
  double sn, cs;
  sincos(w * t, &sn, &cs);
  double mixed = cs * I + sn * Q;
  if (dc) mixed += dc[bk];
  double r;
  if (C.kind && C.kind[bk % A.K] == C3P_LINE_KIND_FLUX) {
    const FluxP p = load_flux(C.line + bk * C3P_LINE_NPAR);
    r = flux_freq(p.phi + mixed, p) - flux_freq(p.phi, p);
  } else {
    r = mixed * v2hz;
  }
  out[gid] = r;
}

// Crosstalk and its two adjoints over [B,K,N], j (or k) ascending
__global__ void xtalk_fwd_kernel(SynthArgs A, const double* xt, const double* pre, double* out) {
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)A.B * A.K * A.N) return;
  const int n = (int)(gid % A.N);
  const long bk = gid / A.N, b = bk / A.K;
  double s = 0.0;
  for (int j = 0; j < A.K; ++j) s = fma(xt[bk * A.K + j], pre[(b * A.K + j) * A.N + n], s);
  out[gid] = s;
}
__global__ void xtalk_bwd_sig_kernel(SynthArgs A, const double* xt, const double* gsig, double* gpre) {
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)A.B * A.K * A.N) return;
  const int n = (int)(gid % A.N);
  const long bj = gid / A.N, b = bj / A.K;
  const int j = (int)(bj % A.K);
  double s = 0.0;
  for (int k = 0; k < A.K; ++k) s = fma(xt[(b * A.K + k) * A.K + j], gsig[(b * A.K + k) * A.N + n], s);
  gpre[gid] = s;
}
// one block per entry (b, k, j): sum_n gsig[b,k,n] pre[b,j,n]
__global__ void __launch_bounds__(256) xtalk_bwd_mat_kernel(SynthArgs A, const double* gsig, const double* pre, double* gxt) {
  __shared__ double s_red[4];
  const long bkj = blockIdx.x;
  const long bk = bkj / A.K, b = bk / A.K;
  const int j = (int)(bkj % A.K);
  const double* g = gsig + bk * A.N;
  const double* s = pre + (b * A.K + j) * A.N;
  double v = 0.0;
  for (int n = threadIdx.x; n < A.N; n += 256) v = fma(g[n], s[n], v);
  v = filt_block_sum(v, s_red);
  if (threadIdx.x == 0) gxt[bkj] = v;
}

// backward step 1, chain_bwd_sample_kernel over the last stage buffer: the cotangent of the mixer's input pair (gcs [B,K,2,N])
// and the tile's partial sums: LO frequency, V->Hz, the five line parameters, the DC offset
__global__ void __launch_bounds__(CH_TN) filt_bwd_sample_kernel(SynthChainArgs C, int nt, const double* buf, const double* dc,
                                                                const double* gsig, double* gcs, double* part) {
  __shared__ double s_red[CH_TN / 64][FL_NP];
  const SynthArgs& A = C.S;
  const long bk = blockIdx.x / nt;
  const int n = (int)(blockIdx.x % nt) * CH_TN + threadIdx.x;
  double v[FL_NP];
  for (int q = 0; q < FL_NP; ++q) v[q] = 0.0;
  if (n < A.N) {
    const double I = buf[bk * 2 * A.N + n], Q = buf[bk * 2 * A.N + A.N + n];
    const double dts = 1.0 / A.sim_res;
    const double t = linspace_at(A.t_start + dts / 2, A.t_end - dts / 2, A.N, n);
    const double w = A.carrier[bk * 2 + 0], v2hz = A.carrier[bk * 2 + 1];
    double sn, cs;
    sincos(w * t, &sn, &cs);
    double mixed = cs * I + sn * Q;
    if (dc) mixed += dc[bk];
    const double g = gsig[bk * A.N + n];
    double gm;
    if (C.kind && C.kind[bk % A.K] == C3P_LINE_KIND_FLUX) {
      const FluxP p = load_flux(C.line + bk * C3P_LINE_NPAR);
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
    v[7] = gm;
    gcs[(bk * 2 + 0) * A.N + n] = gm * cs;
    gcs[(bk * 2 + 1) * A.N + n] = gm * sn;
  }
  for (int q = 0; q < FL_NP; ++q) v[q] = wave_sum(v[q]);
  if ((threadIdx.x & 63) == 0)
    for (int q = 0; q < FL_NP; ++q) s_red[threadIdx.x >> 6][q] = v[q];
  __syncthreads();
  if (threadIdx.x < FL_NP) {
    double s = s_red[0][threadIdx.x];
    for (int wv = 1; wv < CH_TN / 64; ++wv) s += s_red[wv][threadIdx.x];
    part[(long)blockIdx.x * FL_NP + threadIdx.x] = s;
  }
}

// backward step 3, chain_bwd_awg_kernel over the cotangent of stage buffer 0: the transposed legacy FIR and DAC onto giq; the
// wavefront of j = 0 folds the tile partials into gcar_part, gline (with lines) and gdc (with an offset)
__global__ void __launch_bounds__(64) filt_bwd_awg_kernel(SynthChainArgs C, int nt, const double* gcs, const double* part, double* giq,
                                                          double* gcar_part, double* gline, double* gdc) {
  const SynthArgs& A = C.S;
  const long gid = blockIdx.x;
  const int lane = threadIdx.x;
  const int j = (int)(gid % A.Na);
  const long bk = gid / A.Na;
  int n = (int)ceil((double)j * ((double)A.N / (double)A.Na) - 0.5);
  n = n < 0 ? 0 : (n > A.N ? A.N : n);
  while (n > 0 && dac_src(n - 1, A.Na, A.N) >= j) --n;
  while (n < A.N && dac_src(n, A.Na, A.N) < j) ++n;
  const int Mt = filt_legacy_taps(C, bk);
  const double* gc = gcs + bk * 2 * A.N;
  const double* gs = gc + A.N;
  const double* h = Mt ? C.taps + bk * C.tap_stride : nullptr;
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
  double v[FL_NP];
  for (int q = 0; q < FL_NP; ++q) {
    double s = 0.0;
    for (int tl = lane; tl < nt; tl += 64) s += part[(bk * nt + tl) * FL_NP + q];
    v[q] = wave_sum(s);
  }
  if (lane == 0) {
    gp[0] = v[0];
    gp[1] = v[1];
    if (gline) {
      double* gl = gline + bk * C3P_LINE_NPAR;
      gl[C3P_LINE_RISE_TIME] = 0.0;  // the tap count is a floor: not differentiated
      gl[C3P_LINE_PHI_0] = v[2];
      gl[C3P_LINE_PHI] = v[3];
      gl[C3P_LINE_OMEGA_0] = v[4];
      gl[C3P_LINE_ANHAR] = v[5];
      gl[C3P_LINE_D] = v[6];
    }
    if (gdc) gdc[bk] = v[7];
  }
}

int filt_conv_tiles(int N) { return (N + FC_TILE - 1) / FC_TILE; }

// the recomputed forward up to the last stage buffer: AWG I/Q, the legacy taps, the stages' taps, buffer 0, the stages
void launch_filt_stages(const SynthChainArgs& C, const SynthTabArgs& X, const SynthFiltArgs& Fa, hipStream_t st) {
  const SynthArgs& A = C.S;
  const long lines = (long)A.B * A.K, bufsz = lines * 2 * A.N;
  launch_awg_iq(A, &X, lines * A.Na, st);
  if (C.kind) C3P_LAUNCH(chain_taps_kernel, dim3((unsigned)lines), dim3(64), 0, st, C);
  if (Fa.F > 0) C3P_LAUNCH(filt_taps_kernel, dim3((unsigned)(lines * Fa.F)), dim3(256), 0, st, A, Fa);
  const int nt = c3p_chain_tiles(A.N), ct = filt_conv_tiles(A.N);
  C3P_LAUNCH(filt_up_kernel, dim3((unsigned)(lines * nt)), dim3(CH_TN), 0, st, C, nt, Fa.buf);
  for (int f = 0; f < Fa.F; ++f) {
    const FiltConv P = {Fa.h + (long)f * A.N, (long)Fa.F * A.N, 0, Fa.buf + f * bufsz, Fa.buf + (f + 1) * bufsz, Fa.fkind, A.K, Fa.F, f, A.N, ct, lines, 0, 0};
#ifdef C3P_FILT_PLAIN
    FiltConv Q = P;
    Q.nt = nt;
    C3P_LAUNCH(filt_conv_plain_kernel, dim3((unsigned)(lines * nt)), dim3(CH_TN), 0, st, Q);
#else
    C3P_LAUNCH(filt_conv_kernel<false>, dim3((unsigned)(lines * ct)), dim3(FC_NT), 0, st, P);
#endif
  }
}

}  // namespace

hipError_t c3p_launch_synth_filt(const SynthChainArgs& C, const SynthTabArgs& X, const SynthFiltArgs& Fa, hipStream_t st) {
  const SynthArgs& A = C.S;
  const long lines = (long)A.B * A.K, ts = lines * A.N;
  if (lines * A.Na == 0 || ts == 0) return hipSuccess;
  launch_filt_stages(C, X, Fa, st);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const unsigned grid = (unsigned)((ts + 255) / 256);
  const double* last = Fa.buf + Fa.F * lines * 2 * A.N;
  C3P_LAUNCH(filt_mix_kernel, dim3(grid), dim3(256), 0, st, C, last, Fa.dc, Fa.xtalk ? Fa.pre : A.signals);
  if (Fa.xtalk) C3P_LAUNCH(xtalk_fwd_kernel, dim3(grid), dim3(256), 0, st, A, Fa.xtalk, (const double*)Fa.pre, A.signals);
  return hipGetLastError();
}

hipError_t c3p_launch_synth_filt_vjp(const SynthChainArgs& C, const SynthTabArgs& X, const SynthFiltArgs& Fa, const double* gsig,
                                     const SynthVjpBufs& V, const SynthFiltVjpBufs& W, hipStream_t st) {
  const SynthArgs& A = C.S;
  const long lines = (long)A.B * A.K, ta = lines * A.Na, ts = lines * A.N, bufsz = lines * 2 * A.N;
  if (ta == 0 || ts == 0) return hipSuccess;
  launch_filt_stages(C, X, Fa, st);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const unsigned grid = (unsigned)((ts + 255) / 256);
  const double* last = Fa.buf + Fa.F * bufsz;
  const double* g = gsig;
  if (Fa.xtalk) {
    C3P_LAUNCH(filt_mix_kernel, dim3(grid), dim3(256), 0, st, C, last, Fa.dc, Fa.pre);
    C3P_LAUNCH(xtalk_bwd_mat_kernel, dim3((unsigned)(lines * A.K)), dim3(256), 0, st, A, gsig, (const double*)Fa.pre, W.gxtalk);
    C3P_LAUNCH(xtalk_bwd_sig_kernel, dim3(grid), dim3(256), 0, st, A, Fa.xtalk, gsig, W.gpre);
    g = W.gpre;
  }
  const int nt = c3p_chain_tiles(A.N), ct = filt_conv_tiles(A.N);
  double* gy = V.gcs;
  double* gx = W.gbuf;
  C3P_LAUNCH(filt_bwd_sample_kernel, dim3((unsigned)(lines * nt)), dim3(CH_TN), 0, st, C, nt, last, Fa.dc, g, gy, V.part);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  for (int f = Fa.F - 1; f >= 0; --f) {
    const double* xin = Fa.buf + f * bufsz;
    const FiltConv Pg = {xin, 2L * A.N, (long)A.N, gy, W.gh, Fa.fkind, A.K, Fa.F, f, A.N, ct, lines, 1, 1};
    C3P_LAUNCH(filt_conv_kernel<true>, dim3((unsigned)(lines * ct)), dim3(FC_NT), 0, st, Pg);
    C3P_LAUNCH(filt_par_kernel, dim3((unsigned)lines), dim3(256), 0, st, A, Fa, f, (const double*)W.gh, W.gfilt);
    const FiltConv Px = {Fa.h + (long)f * A.N, (long)Fa.F * A.N, 0, gy, gx, Fa.fkind, A.K, Fa.F, f, A.N, ct, lines, 1, 1};
    C3P_LAUNCH(filt_conv_kernel<false>, dim3((unsigned)(lines * ct)), dim3(FC_NT), 0, st, Px);
    double* s = gy;
    gy = gx;
    gx = s;
  }
  C3P_LAUNCH(filt_bwd_awg_kernel, dim3((unsigned)ta), dim3(64), 0, st, C, nt, (const double*)gy, (const double*)V.part, V.giq, V.gcar_part,
             V.gline, W.gdc);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  launch_awg_bwd(A, &X, (const double*)V.giq, (const double*)V.gcar_part, V.genv, V.gcar, V.gtab, st);
  return hipGetLastError();
}
