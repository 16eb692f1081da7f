// Discrete adjoint of the ODE state solvers: gradients of a state cotangent with respect to the control signals and the
// initial state, exact for the arithmetic the forward kernels do (c3p_ode.hip, c3p_ode_row.hip).
//
// Stands in for the tape of goal_run_ode / goal_run_ode_only_final (c3/optimizers/optimalcontrol.py:230-292, differentiated
// by c3/optimizers/optimizer.py:206-216) through compute_states / compute_final_state with an RK solver
// (c3/libraries/propagation.py:687-752, tableaux :755-883, step functions :886-904) and interpolate_signal
// (c3/utils/tf_utils.py:521-559); the state-transfer goal is tf_ketket_fid / tf_dmket_fid (tf_utils.py:320-327).
//
// One step is y_{n+1} = y_n + sum_s b_s k_s, k_s = dt F(H(t_s))[y_n + sum_{j<s} a_sj k_j].  Given ybar_{n+1}:
//   kbar_s = b_s ybar_{n+1};  for s = S-1 .. 0:  zbar = dt F^+(H(t_s))[kbar_s],  cbar_k(t_s) += Re<kbar_s, dt dF/dc_k[y_s]>,
//   ybar_n += zbar,  kbar_j += a_sj zbar (j < s);  the interpolation weights (1 - tau, tau) carry cbar to the two samples.
// Adjoints are taken under Re tr(a^+ b); nothing is assumed Hermitian.
//
// States are never integrated backwards (lossy and Lindblad maps are not undone by their adjoints): the kernel first runs
// the forward pass and keeps checkpoints y_0, y_C, y_2C, ... in global memory, then walks the segments from the last to the
// first, recomputes the <= C states of a segment from its checkpoint and the stages of every step, and sweeps.
//
//  * ode_vjp_row_kernel: Schroedinger step, D <= 16, K <= 4 (the class of ode_vec_kernel).  One sample per 16-lane DPP row,
//    lane i owns row i of h0 (registers) and of every hk (registers, or one LDS copy per wavefront for the large shapes)
//    and element i of y, ybar, k_s, kbar_s.  H y, hk y and H^+ kbar are
//    row_newbcast FMAs (c3p_ode_dpp.inc).  H^+ needs the rows of the adjoint operators: the HERM instance (operators
//    Hermitian, detected on the device; both instances are launched and one leaves) uses the rows it has, the general one
//    (a lossy h0) reads the conjugated columns from memory.  Segment states live in LDS; the per-lane partial sums of cbar are kept
//    for the four samples a step can touch and reduced over the row once per step, when a sample has received its last
//    contribution -- one owner per gradient element, fixed order, no atomics.
//  * ode_vjp_wg_kernel: one workgroup per sample, everything else the forward solver serves (rho-valued steps, D > 16,
//    K up to 32); matrices in LDS or global scratch like ode_kernel.  Correctness first.
#include <type_traits>
#include <utility>

#include "c3p_common.h"
#include "c3p_kernels.h"
#include "c3p_ode.h"
#include "c3p_ode_tab.h"
#include "c3p_ode_dpp.inc"
#include "c3p_ode_vjp.h"

#ifndef C3P_ODE_VJP_PART
#define C3P_ODE_VJP_PART 0  // one translation unit with everything
#endif

extern __shared__ __attribute__((aligned(16))) unsigned char c3p_ode_vjp_smem[];

namespace {

__constant__ OdeTableau c3p_vjp_tab[4] = C3P_ODE_TABLEAUX;

__host__ __device__ constexpr OdeTableau vtab(int solver) {
  constexpr OdeTableau t[4] = C3P_ODE_TABLEAUX;
  return t[solver];
}

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// sum over the 16 lanes of a DPP row, the same value (same order of additions) in every lane
__device__ __forceinline__ double row_sum(double v) {
  v += __shfl_xor(v, 1, 16);
  v += __shfl_xor(v, 2, 16);
  v += __shfl_xor(v, 4, 16);
  v += __shfl_xor(v, 8, 16);
  return v;
}

// a value the compiler cannot see through: LDS addresses formed from it are loaded where they are used (the hk rows in LDS
// are loop invariant, and hoisting their loads out of the step loop would put them back into registers -- and spill them)
__device__ __forceinline__ int opaque(int x) {
  asm volatile("" : "+v"(x));
  return x;
}
// ---------------------------------------------------------------------------------------------------------------
// lane-row kernel
// ---------------------------------------------------------------------------------------------------------------
// hk rows in registers while (1 + KT) DP rows fit beside the stage values; above that they live in LDS, ONE copy for the
// four rows of the wavefront (all samples share the operators), and a stage reads the row it multiplies with
__host__ __device__ constexpr bool hk_in_lds(int DP, int KT) { return DP * KT >= 24; }

template <int DP, int KT, int SOLVER, bool HERM>
__global__ void __launch_bounds__(64) ode_vjp_row_kernel(OdeVjpArgs V) {
  using P = OdeDpp<DP>;
  constexpr int S = vtab(SOLVER).stages;
  constexpr bool HKL = hk_in_lds(DP, KT);
  constexpr int KR = HKL ? 1 : KT, DR = HKL ? 1 : DP;
  const OdeArgs& A = V.f;
  const int lane = threadIdx.x, r = lane >> 4, i = lane & 15;
  const int D = A.D, K = A.K, N = A.N, Cint = V.Cint, SW = Cint + 2;
  const bool row = i < D;
  const double dt = A.dt;

  // LDS: segment states [4][Cint][16] cplx | staged signals [4][KT][Cint + 2] | (HKL) hk rows [KT DP][16] cplx
  cplx* segst = reinterpret_cast<cplx*>(c3p_ode_vjp_smem) + (long)r * Cint * 16;
  double* sig0 = reinterpret_cast<double*>(reinterpret_cast<cplx*>(c3p_ode_vjp_smem) + (long)4 * Cint * 16);
  double* sigl = sig0 + r * KT * SW;
  cplx* hkl = reinterpret_cast<cplx*>(sig0 + 4 * KT * SW);

  // rows of the operators (zero padded; lanes i >= D hold zero rows), Hermiticity seen from this lane's row and column
  double h0r[DP], h0i[DP], hkr[KR][DR], hki[KR][DR];
  bool herm = true;
#pragma unroll
  for (int j = 0; j < DP; ++j) {
    cplx z = cmake(0, 0), zt = cmake(0, 0);
    if (row && j < D) z = A.h0[i * D + j], zt = A.h0[j * D + i];
    h0r[j] = z.x;
    h0i[j] = z.y;
    herm = herm && z.x == zt.x && z.y == -zt.y;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      cplx y = cmake(0, 0), yt = cmake(0, 0);
      if (row && j < D && k < K) y = A.hks[((long)k * D + i) * D + j], yt = A.hks[((long)k * D + j) * D + i];
      if constexpr (HKL) {
        if (r == 0) hkl[(k * DP + j) * 16 + i] = y;
      } else {
        hkr[k][j] = y.x;
        hki[k][j] = y.y;
      }
      herm = herm && y.x == yt.x && y.y == -yt.y;
    }
  }
  if ((__all(herm) != 0) != HERM) return;  // wave-uniform: every row of the grid sees the same operators
  __syncthreads();

  const int v0 = blockIdx.x * 4 + r;
  const int R = V.rows;
  const int nwalk = (A.B + R - 1) / R;
  cplx* ck = V.ws + (long)v0 * V.ws_stride;  // checkpoints [nck][D] of this launched row

  double Hr[DP], Hi[DP];  // row i of H(t), or of H(t)^+ in the sweep
  double kr[S], ki[S];

#pragma unroll 1
  for (int it = 0; it < nwalk; ++it) {
    int b = v0 + it * R;
    const bool live = v0 < R && b < A.B;
    if (!live) b = A.B - 1;
    const double* sg = A.signals + (long)b * K * N;
    int base = 0;

    auto stage_signals = [&](int n0) {
      __syncthreads();
      base = n0 < N - 2 ? n0 : N - 2;
      for (int t = i; t < SW; t += 16) {
        int idx = base + t;
        if (idx > N - 1) idx = N - 1;
#pragma unroll
        for (int k = 0; k < KT; ++k) sigl[k * SW + t] = (k < K) ? sg[(long)k * N + idx] : 0.0;
      }
      __syncthreads();
    };
    // control amplitudes at u = n + theta: linear interpolation, linear extrapolation past the last sample
    auto amplitudes = [&](double theta, int n, double (&c)[KT]) {
      const double u = (double)n + theta;
      int lo = (int)floor(u);
      if (lo > N - 2) lo = N - 2;
      if (lo < 0) lo = 0;
      const double f = u - (double)lo;
      const double* sp = sigl + (lo - base);
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        const double y0 = sp[k * SW], y1 = sp[k * SW + 1];
        c[k] = fma(f, y1 - y0, y0);
      }
    };
    // row i of H(t) = h0 + sum_k c_k hk
    auto assemble = [&](double theta, int n) {
      double c[KT];
      amplitudes(theta, n, c);
      const cplx* hp = hkl + opaque(i);
#pragma unroll
      for (int j = 0; j < DP; ++j) {
        double hr = h0r[j], hi = h0i[j];
#pragma unroll
        for (int k = 0; k < KT; ++k) {
          if constexpr (HKL) {
            const cplx x = hp[(k * DP + j) * 16];
            hr = fma(c[k], x.x, hr);
            hi = fma(c[k], x.y, hi);
          } else {
            hr = fma(c[k], hkr[k][j], hr);
            hi = fma(c[k], hki[k][j], hi);
          }
        }
        Hr[j] = hr;
        Hi[j] = hi;
        // (a few rows in flight at a time: left alone, the scheduler requests all KT DP of them before the first FMA)
        if constexpr (HKL)
          if (j % 4 == 3) __builtin_amdgcn_sched_barrier(0);
      }
    };
    // row i of H(t)^+: the same rows when the operators are Hermitian, else column i of the operators, conjugated (read
    // from memory: the operators are a few kilobytes that every wavefront of the grid reads, i.e. cache resident)
    auto assemble_adj = [&](double theta, int n) {
      if constexpr (HERM) {
        assemble(theta, n);
      } else {
        double c[KT];
        amplitudes(theta, n, c);
        const int ci = opaque(i);  // (loop-invariant loads: requested here, not kept in registers across the sweep)
#pragma unroll
        for (int j = 0; j < DP; ++j) {
          cplx g = cmake(0, 0);
          if (row && j < D) {
            g = A.h0[j * D + ci];
#pragma unroll
            for (int k = 0; k < KT; ++k)
              if (k < K) {
                const cplx x = A.hks[((long)k * D + j) * D + ci];
                g.x = fma(c[k], x.x, g.x);
                g.y = fma(c[k], x.y, g.y);
              }
          }
          Hr[j] = g.x;
          Hi[j] = -g.y;
        }
      }
    };
    // the stages k_s of step n from the state (pr, pi), as ode_vec_kernel computes them
    auto stages_fwd = [&](double pr, double pi, int n) {
      static_for<0, S>([&](auto sc) {
        constexpr int s = decltype(sc)::value;
        // (stage by stage: the assemblies depend on n alone, and a scheduler free to start them all at once -- it has 512
        // registers to fill -- ends with the rows of every stage node live together and spills)
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (s == 0) {
          assemble(vtab(SOLVER).node[0], n);
        } else if constexpr (vtab(SOLVER).node[s] != vtab(SOLVER).node[s - 1]) {
          assemble(vtab(SOLVER).node[s], n);
        }
        double yr = pr, yi = pi;
        static_for<0, s>([&](auto jc) {
          constexpr int j = decltype(jc)::value;
          constexpr double a = vtab(SOLVER).a[s][j];
          if constexpr (a != 0.0) {
            yr = fma(a, kr[j], yr);
            yi = fma(a, ki[j], yi);
          }
        });
        double w[4] = {0.0, 0.0, 0.0, 0.0};
        P::matvec_c(w, yr, yi, Hr, Hi);
        kr[s] = dt * (w[1] + w[3]);  // -i dt (wr + i wi)
        ki[s] = -dt * (w[0] + w[2]);
      });
    };

    double pr = 0.0, pi = 0.0;
    if (row) {
      const cplx z = A.init[(long)b * A.init_bstride + i];
      pr = z.x;
      pi = z.y;
    }
    double br = 0.0, bi = 0.0;  // ybar
    double acc[KT][4];          // per-lane partial sums of grad_signals[n - 1 .. n + 2] of the current step n
#pragma unroll
    for (int k = 0; k < KT; ++k) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0.0;
    double* gs = V.grad_signals + (long)b * K * N;

    // passes 0 .. nck-1: the forward pass, segment by segment, with a checkpoint at every segment start;
    // passes nck .. 2 nck-1: segments from the last to the first -- recompute the segment's states, then sweep it
#pragma unroll 1
    for (int pass = 0; pass < 2 * V.nck; ++pass) {
      const bool fwd = pass < V.nck;
      const int seg = fwd ? pass : 2 * V.nck - 1 - pass;
      const int n0 = seg * Cint, n1 = n0 + Cint < N ? n0 + Cint : N;
      if (fwd) {
        if (row) ck[(long)seg * D + i] = cmake(pr, pi);
      } else {
        cplx z0 = cmake(0, 0);
        if (row) z0 = ck[(long)seg * D + i];
        pr = z0.x;
        pi = z0.y;
      }
      stage_signals(n0);
#pragma unroll 1
      for (int n = n0; n < n1; ++n) {
        segst[(n - n0) * 16 + i] = cmake(pr, pi);
        if (fwd || n + 1 < n1) {
          stages_fwd(pr, pi, n);
          double qr = pr, qi = pi;
          static_for<0, S>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            constexpr double bj = vtab(SOLVER).b[j];
            if constexpr (bj != 0.0) {
              qr = fma(bj, kr[j], qr);
              qi = fma(bj, ki[j], qi);
            }
          });
          pr = qr;
          pi = qi;
        }
      }
      if (fwd) {
        if (pass == V.nck - 1) {
          if (V.final_out && live && row) V.final_out[(long)b * D + i] = cmake(pr, pi);
          if (V.target) {
            // infid = 1 - |<t|psi_N>| (tf_ketket_fid); psibar = -(z / |z|) t, zero where the overlap is zero
            cplx t = cmake(0, 0);
            if (row) t = V.target[(long)b * V.target_bstride + i];
            const double zr = row_sum(t.x * pr + t.y * pi), zi = row_sum(t.x * pi - t.y * pr);
            const double az = hypot(zr, zi);
            if (V.infid && live && i == 0) V.infid[b] = 1.0 - az;
            if (az > 0.0) {
              const double fr = -zr / az, fi = -zi / az;
              br = fr * t.x - fi * t.y;
              bi = fr * t.y + fi * t.x;
            }
          }
        }
        continue;
      }
#pragma unroll 1
      for (int n = n1 - 1; n >= n0; --n) {
        if (V.states_bar && (V.bar_all || n == N - 1)) {
          cplx z = cmake(0, 0);
          if (row) z = V.states_bar[((long)b * (V.bar_all ? N : 1) + (V.bar_all ? n : 0)) * D + i];
          br += z.x;
          bi += z.y;
        }
        const cplx yn = segst[(n - n0) * 16 + i];
        stages_fwd(yn.x, yn.y, n);
        double qr[S], qi[S];  // kbar_s
        static_for<0, S>([&](auto sc) {
          constexpr int s = decltype(sc)::value;
          qr[s] = vtab(SOLVER).b[s] * br;
          qi[s] = vtab(SOLVER).b[s] * bi;
        });
        static_for<0, S>([&](auto tc) {
          constexpr int s = S - 1 - decltype(tc)::value;
          constexpr double theta = vtab(SOLVER).node[s];
          __builtin_amdgcn_sched_barrier(0);
          if constexpr (s == S - 1) {
            assemble_adj(theta, n);
          } else if constexpr (vtab(SOLVER).node[s] != vtab(SOLVER).node[s + 1]) {
            assemble_adj(theta, n);
          }
          double yr = yn.x, yi = yn.y;
          static_for<0, s>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            constexpr double a = vtab(SOLVER).a[s][j];
            if constexpr (a != 0.0) {
              yr = fma(a, kr[j], yr);
              yi = fma(a, ki[j], yi);
            }
          });
          // interpolation weights of this stage: sample lo gets 1 - tau, lo + 1 gets tau; slot = sample - (n - 1)
          constexpr int d0 = theta >= 1.0 ? 1 : 0;
          int lo = n + d0;
          if (lo > N - 2) lo = N - 2;
          const int d = lo - n;
          const double tau = theta - (double)d;
          double wq[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) wq[q] = (q == d + 1 ? 1.0 - tau : 0.0) + (q == d + 2 ? tau : 0.0);
          // cbar_k = Re<kbar_s, -i dt hk y_s> = dt (qr Im(hk y) - qi Re(hk y)), this lane's term
#pragma unroll
          for (int k = 0; k < KT; ++k) {
            double w[4] = {0.0, 0.0, 0.0, 0.0};
            if constexpr (HKL) {
              // (one row at a time: without the fence the scheduler requests the rows of all control lines at once)
              __builtin_amdgcn_sched_barrier(0);
              double tr[DP], ti[DP];
              const cplx* hp = hkl + opaque(i);
#pragma unroll
              for (int j = 0; j < DP; ++j) {
                const cplx x = hp[(k * DP + j) * 16];
                tr[j] = x.x;
                ti[j] = x.y;
              }
              P::matvec_c(w, yr, yi, tr, ti);
            } else {
              P::matvec_c(w, yr, yi, hkr[k], hki[k]);
            }
            const double p = dt * (qr[s] * (w[1] + w[3]) - qi[s] * (w[0] + w[2]));
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[k][q] = fma(wq[q], p, acc[k][q]);
          }
          // zbar = i dt H^+ kbar_s
          double w[4] = {0.0, 0.0, 0.0, 0.0};
          P::matvec_c(w, qr[s], qi[s], Hr, Hi);
          const double zr = -dt * (w[1] + w[3]), zi = dt * (w[0] + w[2]);
          br += zr;
          bi += zi;
          static_for<0, s>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            constexpr double a = vtab(SOLVER).a[s][j];
            if constexpr (a != 0.0) {
              qr[j] = fma(a, zr, qr[j]);
              qi[j] = fma(a, zi, qi[j]);
            }
          });
        });
        // sample n + 2 has received its last contribution
#pragma unroll
        for (int k = 0; k < KT; ++k) {
          const double s = row_sum(acc[k][3]);
          if (live && i == 0 && k < K && n + 2 < N) gs[(long)k * N + n + 2] = s;
          acc[k][3] = acc[k][2];
          acc[k][2] = acc[k][1];
          acc[k][1] = acc[k][0];
          acc[k][0] = 0.0;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      const double s1 = row_sum(acc[k][3]), s0 = row_sum(acc[k][2]);
      if (live && i == 0 && k < K) {
        gs[(long)k * N + 1] = s1;
        gs[(long)k * N] = s0;
      }
    }
    if (V.init_bar && live && row) V.init_bar[(long)b * D + i] = cmake(br, bi);
  }
}

#if C3P_ODE_VJP_PART != 2
// ---------------------------------------------------------------------------------------------------------------
// workgroup-per-sample kernel
// ---------------------------------------------------------------------------------------------------------------
template <bool GLOBAL>
struct VMem {
  cplx* g;
  __device__ __forceinline__ cplx ld(int off) const {
    if constexpr (GLOBAL)
      return g[off];
    else
      return reinterpret_cast<cplx*>(c3p_ode_vjp_smem)[off];
  }
  __device__ __forceinline__ void st(int off, cplx v) const {
    if constexpr (GLOBAL)
      g[off] = v;
    else
      reinterpret_cast<cplx*>(c3p_ode_vjp_smem)[off] = v;
  }
};

// out (+)= alpha * op(A)[D,D] @ X[D,Mc]; conjT: op(A) = A^+
template <bool G>
__device__ void vmm_left(const VMem<G>& M, int out, int a, int x, int D, int Mc, cplx alpha, bool acc, bool conjT, int tid, int nt) {
  for (int e = tid; e < D * Mc; e += nt) {
    const int i = e / Mc, j = e - i * Mc;
    cplx s = cmake(0, 0);
    for (int k = 0; k < D; ++k) {
      const cplx av = conjT ? cconj(M.ld(a + k * D + i)) : M.ld(a + i * D + k);
      cfma(s, av, M.ld(x + k * Mc + j));
    }
    s = cmul(alpha, s);
    if (acc) s = cadd(s, M.ld(out + e));
    M.st(out + e, s);
  }
  __syncthreads();
}
// out (+)= alpha * X[D,D] @ op(A)[D,D]
template <bool G>
__device__ void vmm_right(const VMem<G>& M, int out, int x, int a, int D, cplx alpha, bool acc, bool conjT, int tid, int nt) {
  for (int e = tid; e < D * D; e += nt) {
    const int i = e / D, j = e - i * D;
    cplx s = cmake(0, 0);
    for (int k = 0; k < D; ++k) {
      const cplx av = conjT ? cconj(M.ld(a + j * D + k)) : M.ld(a + k * D + j);
      cfma(s, M.ld(x + i * D + k), av);
    }
    s = cmul(alpha, s);
    if (acc) s = cadd(s, M.ld(out + e));
    M.st(out + e, s);
  }
  __syncthreads();
}

// sum over the workgroup, fixed order, the same value in every thread
__device__ double block_sum(double v, double* red, int tid, int nt) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < nt / 64; ++w) s += red[w];
  __syncthreads();
  return s;
}

template <bool GLOBAL>
__global__ void __launch_bounds__(256) ode_vjp_wg_kernel(OdeVjpArgs V) {
  const OdeArgs& A = V.f;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int D = A.D, Mc = A.M, K = A.K, N = A.N, Cint = V.Cint;
  const int ssz = D * Mc, hsz = D * D;
  VMem<GLOBAL> M;
  M.g = GLOBAL ? V.scratch + (long)blockIdx.x * V.scratch_stride : nullptr;
  const int oH = 0;
  const int oS = oH + hsz;       // y_n
  const int oY = oS + ssz;       // stage argument
  const int oK = oY + ssz;       // k_1..k_7
  const int oQ = oK + 7 * ssz;   // kbar_1..kbar_7
  const int oB = oQ + 7 * ssz;   // ybar
  const int oZ = oB + ssz;       // zbar
  const int oT = oZ + ssz;       // temp (lindblad)
  const int oC = oT + ssz;       // col ops [C,D,D]
  const int oG = oC + A.C * hsz; // C^+ C per col op
  __shared__ double sigv[32], cb[32], red[4];
  __shared__ double ovl[2];
  const OdeTableau& tb = c3p_vjp_tab[A.solver];
  const double dt = A.dt;
  const bool rho = A.step != C3P_STEP_SCHRODINGER_ID;
  cplx* ck = V.ws + (long)blockIdx.x * V.ws_stride;  // checkpoints [nck][ssz], then segment states [Cint][ssz]
  cplx* segst = ck + (long)V.nck * ssz;

  if (A.step == C3P_STEP_LINDBLAD_ID) {
    for (int e = tid; e < A.C * hsz; e += nt) M.st(oC + e, A.col_ops[e]);
    __syncthreads();
    for (int e = tid; e < A.C * hsz; e += nt) {
      const int c = e / hsz, r = e - c * hsz, i = r / D, j = r - i * D;
      cplx s = cmake(0, 0);
      for (int k = 0; k < D; ++k) cfma(s, cconj(M.ld(oC + c * hsz + k * D + i)), M.ld(oC + c * hsz + k * D + j));
      M.st(oG + e, s);
    }
  }
  __syncthreads();

  for (int b = blockIdx.x; b < A.B; b += gridDim.x) {
    const double* sig = A.signals + (long)b * K * N;
    double* gs = V.grad_signals + (long)b * K * N;
    for (int e = tid; e < K * N; e += nt) gs[e] = 0.0;

    // H(t) at u = n + node -> oH (as ode_kernel assembles it)
    auto assemble = [&](int n, double node) {
      const double u = (double)n + node;
      int lo = (int)floor(u);
      if (lo > N - 2) lo = N - 2;
      if (lo < 0) lo = 0;
      const double f = u - (double)lo;
      if (tid < K) {
        const double* y = sig + (long)tid * N;
        sigv[tid] = fma(f, y[lo + 1] - y[lo], y[lo]);
      }
      __syncthreads();
      for (int e = tid; e < hsz; e += nt) {
        cplx h = A.h0[e];
        for (int k = 0; k < K; ++k) {
          const cplx x = A.hks[(long)k * hsz + e];
          h.x = fma(sigv[k], x.x, h.x);
          h.y = fma(sigv[k], x.y, h.y);
        }
        M.st(oH + e, h);
      }
      __syncthreads();
    };
    auto stage_arg = [&](int s) {
      for (int e = tid; e < ssz; e += nt) {
        cplx y = M.ld(oS + e);
        for (int j = 0; j < s; ++j) {
          const double a = tb.a[s][j];
          if (a != 0.0) {
            const cplx kj = M.ld(oK + j * ssz + e);
            y.x = fma(a, kj.x, y.x);
            y.y = fma(a, kj.y, y.y);
          }
        }
        M.st(oY + e, y);
      }
      __syncthreads();
    };
    // k_s of step n from the state in oS
    auto stages_fwd = [&](int n) {
      for (int s = 0; s < tb.stages; ++s) {
        assemble(n, tb.node[s]);
        stage_arg(s);
        const int ok = oK + s * ssz;
        vmm_left(M, ok, oH, oY, D, Mc, cmake(0.0, -dt), false, false, tid, nt);  // -i dt H y
        if (rho) {
          vmm_right(M, ok, oY, oH, D, cmake(0.0, dt), true, false, tid, nt);  // + i dt y H
          for (int c = 0; c < A.C; ++c) {
            vmm_left(M, oT, oC + c * hsz, oY, D, D, cmake(1.0, 0.0), false, false, tid, nt);          // C y
            vmm_right(M, ok, oT, oC + c * hsz, D, cmake(dt, 0.0), true, true, tid, nt);                // + dt C y C^+
            vmm_left(M, ok, oG + c * hsz, oY, D, D, cmake(-0.5 * dt, 0.0), true, false, tid, nt);      // - dt/2 C^+C y
            vmm_right(M, ok, oY, oG + c * hsz, D, cmake(-0.5 * dt, 0.0), true, false, tid, nt);        // - dt/2 y C^+C
          }
        }
      }
    };
    auto advance = [&]() {
      for (int e = tid; e < ssz; e += nt) {
        cplx y = M.ld(oS + e);
        for (int j = 0; j < tb.stages; ++j) {
          const double bj = tb.b[j];
          if (bj != 0.0) {
            const cplx kj = M.ld(oK + j * ssz + e);
            y.x = fma(bj, kj.x, y.x);
            y.y = fma(bj, kj.y, y.y);
          }
        }
        M.st(oS + e, y);
      }
      __syncthreads();
    };

    // ---- forward pass with checkpoints ----
    const cplx* init = A.init + (long)b * A.init_bstride;
    for (int e = tid; e < ssz; e += nt) M.st(oS + e, init[e]);
    __syncthreads();
    for (int seg = 0; seg < V.nck; ++seg) {
      const int n0 = seg * Cint, n1 = n0 + Cint < N ? n0 + Cint : N;
      for (int e = tid; e < ssz; e += nt) ck[(long)seg * ssz + e] = M.ld(oS + e);
      for (int n = n0; n < n1; ++n) {
        stages_fwd(n);
        advance();
      }
    }
    if (V.final_out)
      for (int e = tid; e < ssz; e += nt) V.final_out[(long)b * ssz + e] = M.ld(oS + e);

    // ---- cotangent of the final state ----
    if (V.target) {
      const cplx* t = V.target + (long)b * V.target_bstride;
      if (tid == 0) {
        if (!rho) {
          // infid = 1 - |<t|psi_N>| (tf_ketket_fid); psibar = -(z / |z|) t
          cplx z = cmake(0, 0);
          for (int i = 0; i < D; ++i) cfma(z, cconj(t[i]), M.ld(oS + i));
          const double az = hypot(z.x, z.y);
          if (V.infid) V.infid[b] = 1.0 - az;
          ovl[0] = az > 0.0 ? -z.x / az : 0.0;
          ovl[1] = az > 0.0 ? -z.y / az : 0.0;
        } else {
          // infid = 1 - sqrt(Re <t|rho_N|t>) (tf_dmket_fid); rhobar = -t t^+ / (2 sqrt(.))
          cplx z = cmake(0, 0);
          for (int i = 0; i < D; ++i) {
            cplx s = cmake(0, 0);
            for (int j = 0; j < D; ++j) cfma(s, M.ld(oS + i * D + j), t[j]);
            cfma(z, cconj(t[i]), s);
          }
          const double f = sqrt(z.x);
          if (V.infid) V.infid[b] = 1.0 - f;
          ovl[0] = z.x > 0.0 ? -0.5 / f : 0.0;
          ovl[1] = 0.0;
        }
      }
      __syncthreads();
      for (int e = tid; e < ssz; e += nt) {
        if (!rho) {
          M.st(oB + e, cmul(cmake(ovl[0], ovl[1]), t[e]));
        } else {
          const int i = e / D, j = e - i * D;
          M.st(oB + e, cscale(cmul(t[i], cconj(t[j])), ovl[0]));
        }
      }
    } else {
      for (int e = tid; e < ssz; e += nt) M.st(oB + e, cmake(0, 0));
    }
    __syncthreads();

    // ---- reverse sweep ----
    for (int seg = V.nck - 1; seg >= 0; --seg) {
      const int n0 = seg * Cint, n1 = n0 + Cint < N ? n0 + Cint : N;
      for (int e = tid; e < ssz; e += nt) M.st(oS + e, ck[(long)seg * ssz + e]);
      __syncthreads();
      for (int n = n0; n < n1; ++n) {
        for (int e = tid; e < ssz; e += nt) segst[(long)(n - n0) * ssz + e] = M.ld(oS + e);
        if (n + 1 < n1) {
          stages_fwd(n);
          advance();
        }
      }
      __syncthreads();
      for (int n = n1 - 1; n >= n0; --n) {
        const bool inject = V.states_bar && (V.bar_all || n == N - 1);
        const cplx* sb = V.states_bar ? V.states_bar + ((long)b * (V.bar_all ? N : 1) + (V.bar_all ? n : 0)) * ssz : nullptr;
        for (int e = tid; e < ssz; e += nt) {
          M.st(oS + e, segst[(long)(n - n0) * ssz + e]);
          if (inject) M.st(oB + e, cadd(M.ld(oB + e), sb[e]));
        }
        __syncthreads();
        stages_fwd(n);
        for (int e = tid; e < ssz; e += nt) {
          const cplx yb = M.ld(oB + e);
          for (int s = 0; s < tb.stages; ++s) M.st(oQ + s * ssz + e, cscale(yb, tb.b[s]));
        }
        __syncthreads();
        for (int s = tb.stages - 1; s >= 0; --s) {
          assemble(n, tb.node[s]);
          stage_arg(s);
          const int ox = oQ + s * ssz;
          // cbar_k = Re<kbar_s, -i dt hk y_s> (vector) or Re<kbar_s, -i dt [hk, y_s]> (rho)
          for (int k = 0; k < K; ++k) {
            const cplx* hk = A.hks + (long)k * hsz;
            double p = 0.0;
            for (int e = tid; e < ssz; e += nt) {
              const int i = e / Mc, c = e - i * Mc;
              cplx el = cmake(0, 0);
              for (int j = 0; j < D; ++j) cfma(el, hk[i * D + j], M.ld(oY + j * Mc + c));
              if (rho)
                for (int j = 0; j < D; ++j) cfma(el, cscale(M.ld(oY + i * D + j), -1.0), hk[j * D + c]);
              const cplx x = M.ld(ox + e);
              p += dt * (x.x * el.y - x.y * el.x);
            }
            const double s_ = block_sum(p, red, tid, nt);
            if (tid == 0) cb[k] = s_;
          }
          __syncthreads();
          if (tid < K) {
            const double u = (double)n + tb.node[s];
            int lo = (int)floor(u);
            if (lo > N - 2) lo = N - 2;
            if (lo < 0) lo = 0;
            const double tau = u - (double)lo;
            double* g = gs + (long)tid * N;  // one owner (this thread) per control line of this sample
            g[lo] += (1.0 - tau) * cb[tid];
            g[lo + 1] += tau * cb[tid];
          }
          // zbar = dt F^+(H)[kbar_s]
          vmm_left(M, oZ, oH, ox, D, Mc, cmake(0.0, dt), false, true, tid, nt);  // i dt H^+ x
          if (rho) {
            vmm_right(M, oZ, ox, oH, D, cmake(0.0, -dt), true, true, tid, nt);  // - i dt x H^+
            for (int c = 0; c < A.C; ++c) {
              vmm_left(M, oT, oC + c * hsz, ox, D, D, cmake(1.0, 0.0), false, true, tid, nt);           // C^+ x
              vmm_right(M, oZ, oT, oC + c * hsz, D, cmake(dt, 0.0), true, false, tid, nt);              // + dt C^+ x C
              vmm_left(M, oZ, oG + c * hsz, ox, D, D, cmake(-0.5 * dt, 0.0), true, false, tid, nt);     // - dt/2 C^+C x
              vmm_right(M, oZ, ox, oG + c * hsz, D, cmake(-0.5 * dt, 0.0), true, false, tid, nt);       // - dt/2 x C^+C
            }
          }
          for (int e = tid; e < ssz; e += nt) {
            const cplx z = M.ld(oZ + e);
            M.st(oB + e, cadd(M.ld(oB + e), z));
            for (int j = 0; j < s; ++j) {
              const double a = tb.a[s][j];
              if (a != 0.0) {
                cplx q = M.ld(oQ + j * ssz + e);
                q.x = fma(a, z.x, q.x);
                q.y = fma(a, z.y, q.y);
                M.st(oQ + j * ssz + e, q);
              }
            }
          }
          __syncthreads();
        }
      }
    }
    if (V.init_bar)
      for (int e = tid; e < ssz; e += nt) V.init_bar[(long)b * ssz + e] = M.ld(oB + e);
    __syncthreads();
  }
}

size_t wg_elems(int D, int M, int C) { return (size_t)D * D + (size_t)19 * D * M + (size_t)2 * C * D * D; }

#endif

int pad_dim(int D) {
  const int dps[] = {2, 3, 4, 6, 9, 12, 16};
  for (int d : dps)
    if (D <= d) return d;
  return 0;
}

size_t row_lds(int DP, int KT, int Cint) {
  size_t n = (size_t)4 * Cint * 16 * sizeof(cplx) + (size_t)4 * KT * (Cint + 2) * sizeof(double);
  if (hk_in_lds(DP, KT)) n += (size_t)KT * DP * 16 * sizeof(cplx);
  return n;
}

template <int DP, int KT, int SOLVER, bool HERM>
hipError_t launch_row4(const OdeVjpArgs& V, dim3 grid, hipStream_t st) {
  const size_t lds = row_lds(DP, KT, V.Cint);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&ode_vjp_row_kernel<DP, KT, SOLVER, HERM>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024);
  if (e != hipSuccess) return e;
  C3P_LAUNCH((ode_vjp_row_kernel<DP, KT, SOLVER, HERM>), grid, dim3(64), lds, st, V);
  return hipGetLastError();
}
template <int DP, int KT, int SOLVER>
hipError_t launch_row3(const OdeVjpArgs& V, dim3 grid, hipStream_t st) {
  // both instances are launched; the device looks at the operators and one of them leaves at once
  hipError_t e = launch_row4<DP, KT, SOLVER, true>(V, grid, st);
  if (e == hipSuccess) e = launch_row4<DP, KT, SOLVER, false>(V, grid, st);
  return e;
}
template <int DP, int KT>
hipError_t launch_row2(const OdeVjpArgs& V, dim3 grid, hipStream_t st) {
  switch (V.f.solver) {
    case 0: return launch_row3<DP, KT, 0>(V, grid, st);
    case 1: return launch_row3<DP, KT, 1>(V, grid, st);
    case 2: return launch_row3<DP, KT, 2>(V, grid, st);
    default: return launch_row3<DP, KT, 3>(V, grid, st);
  }
}
template <int KT>
hipError_t launch_row1(const OdeVjpArgs& V, hipStream_t st) {
  const dim3 grid((unsigned)((V.rows + 3) / 4));
  switch (pad_dim(V.f.D)) {
    case 2: return launch_row2<2, KT>(V, grid, st);
    case 3: return launch_row2<3, KT>(V, grid, st);
    case 4: return launch_row2<4, KT>(V, grid, st);
    case 6: return launch_row2<6, KT>(V, grid, st);
    case 9: return launch_row2<9, KT>(V, grid, st);
    case 12: return launch_row2<12, KT>(V, grid, st);
    default: return launch_row2<16, KT>(V, grid, st);
  }
}

}  // namespace

// The lane-row instances are built as two translation units (C3P_ODE_VJP_PART: 1 = up to two control lines, the
// workgroup kernel and the launcher; 2 = three and four control lines), compiled side by side.
#if C3P_ODE_VJP_PART != 2
hipError_t c3p_launch_ode_vjp_row_k2(const OdeVjpArgs& V, hipStream_t st) { return launch_row1<2>(V, st); }
#endif
#if C3P_ODE_VJP_PART != 1
hipError_t c3p_launch_ode_vjp_row_k4(const OdeVjpArgs& V, hipStream_t st) { return launch_row1<4>(V, st); }
#endif

#if C3P_ODE_VJP_PART != 2
OdeVjpPlan c3p_ode_vjp_plan(int B, int K, int N, int D, int M, int C, int step) {
  OdeVjpPlan p = {};
  p.row = step == C3P_STEP_SCHRODINGER_ID && D <= 16 && K <= 4 && !c3p_opt_on(C3P_OPT_ode_wg);
  int c = 1;
  while (c * c < N) ++c;  // ceil(sqrt(N)): forward + recomputation cost 2 N stage sets, memory N / C + C states
  if (c > C3P_ODE_VJP_MAX_C) c = C3P_ODE_VJP_MAX_C;
  if (c < 1) c = 1;
  p.Cint = c;
  p.nck = (N + c - 1) / c;
  p.ws_elems = p.row ? (size_t)p.nck * D : (size_t)(p.nck + c) * D * M;
  size_t rows = C3P_ODE_VJP_WS_CAP / (p.ws_elems * sizeof(cplx));
  if (rows < 1) rows = 1;
  if (rows > (size_t)B) rows = (size_t)B;
  if (!p.row && rows > 65535 * 16) rows = 65535 * 16;
  p.rows = (int)rows;
  p.wg_elems = wg_elems(D, M, C);
  p.wg_global = p.wg_elems * sizeof(cplx) > (size_t)(150 * 1024);
  return p;
}

hipError_t c3p_launch_ode_vjp(const OdeVjpArgs& V, const OdeVjpPlan& pl, hipStream_t st) {
  if (pl.row) return V.f.K <= 2 ? c3p_launch_ode_vjp_row_k2(V, st) : c3p_launch_ode_vjp_row_k4(V, st);
  int threads = ((V.f.D * V.f.M + 63) / 64) * 64;
  if (threads > 256) threads = 256;
  if (threads < 64) threads = 64;
  if (pl.wg_global) {
    C3P_LAUNCH(ode_vjp_wg_kernel<true>, dim3(pl.rows), dim3(threads), 0, st, V);
  } else {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&ode_vjp_wg_kernel<false>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024);
    if (e != hipSuccess) return e;
    C3P_LAUNCH(ode_vjp_wg_kernel<false>, dim3(pl.rows), dim3(threads), pl.wg_elems * sizeof(cplx), st, V);
  }
  return hipGetLastError();
}
#endif
