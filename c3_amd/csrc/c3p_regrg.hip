// Backward sweep (control gradient) of the Lindblad superoperator chains in the Hermitian basis, REAL arithmetic on the f64
// matrix cores: Dm = D^2 = 49, 64 (in the 65 class), 81 -- the gradient of BASELINE cfg4's path.  The reference tapes
// tf_propagation_lind like every other path (c3/libraries/propagation.py:551-585 under c3/optimizers/optimizer.py:206-216).
//
// In the basis of c3p_regr.hip the chain is a product of real matrices E_n = exp(X_n), X_n = G'_0 + sum_k c_k(n) G'_k.  With the
// time axis cut into S segments, Q_n = E_n ... E_n0 the LOCAL prefix inside a segment (stored transposed by the forward kernel,
// MidArgs.hb_qT) and the left adjoint of a segment's end with the prefix at its start folded in (c3p_launch_regr_scan),
//     Lam_n = (E_{n1-1} ... E_{n+1})^T [R^T U_bar' Pstart^T],        E_bar_n = Lam_n Q_{n-1}^T,        Lam_{n-1} = E_n^T Lam_n,
//     grad[k, n] = < L(X_n)^*[E_bar_n], G'_k > + mu_k <U_bar', U'>,   L(X)^* = L(X^T)   (real matrices),
// nothing is inverted (the slices are not orthogonal: a dissipative chain has no cheap inverse).  Value and Frechet derivative
// of the slice exponential come from ONE forward-mode pair evaluation at A = 2^-s X_n^T in direction dA = 2^-s E_bar_n.
//
// What shapes the evaluation is what a CU can hold: the forward kernel's five tile sets already fill the 512 registers of its
// one wave per SIMD, and the pair evaluation of its T18 polynomial keeps ~13 matrices of 51 KB live.  So the polynomial is a
// Taylor polynomial of degree 2J + 2 in Horner form in A^2, whose left operands are FIXED for the whole slice:
//     H_J = c_2J I + c_2J+1 A + c_2J+2 A2,      H_j = (c_2j I + c_2j+1 A) + A2 H_j+1,
//     dH_j = c_2j+1 dA + dA2 H_j+1 + A2 dH_j+1,  A2 = A A,  dA2 = A dA + dA A,          T = H_0, dT = dH_0,
// then s squarings (T, dT) <- (T T, T dT + dT T).  A2 and dA2 sit in TWO LDS images (106 KB of the 160 KB) for all 3 J Horner
// products, the running pair (H, dH), dA, the right operand and the accumulators are the five register tile sets, A itself is
// re-assembled from the (L2-resident) generator tables wherever a combination needs it, and Lam waits in a per-workgroup
// global tile set (51 KB, written and read once per slice by the same thread).  3 + 3 J + 3 s products for the pair, 2 for
// E_bar and Lam: 29 per slice at cfg4's norm for every degree 8 .. 16 (the degree with the fewest products is chosen per
// segment), against 7 of the forward pass -- and nothing but Q^T (52 KB per slice, read once) comes from HBM.
//
// Product loop, register layout, the (Dm-1)^2 core + one-element border split and the border slots are those of
// c3p_regr.hip (c3p_regr_common.h); the slice is a state machine around ONE copy of the product code.
#include <cstdio>

#include "c3p_common.h"
#include "c3p_grad.h"
#include "c3p_kernels.h"
#include "c3p_regd.h"
#include "c3p_regr_common.h"

extern __shared__ __attribute__((aligned(16))) double c3p_rg_lds[];

namespace {

enum { B_Q = 0, B_LAM, B_DA, B_A, B_A2, B_DA2, B_H, B_DH, B_T, B_I, B_NSLOT };
enum { G_EBAR = 0, G_D2A, G_D2B, G_A2, G_HD1, G_HD2, G_HV, G_SQ1, G_SQ2, G_SQ3, G_LAM };

__device__ const double rg_invfact[24] = {1.0,
                                          1.0,
                                          1.0 / 2,
                                          1.0 / 6,
                                          1.0 / 24,
                                          1.0 / 120,
                                          1.0 / 720,
                                          1.0 / 5040,
                                          1.0 / 40320,
                                          1.0 / 362880,
                                          1.0 / 3628800,
                                          1.0 / 39916800,
                                          1.0 / 479001600,
                                          1.0 / 6227020800.0,
                                          1.0 / 87178291200.0,
                                          1.0 / 1307674368000.0,
                                          1.0 / 20922789888000.0,
                                          1.0 / 355687428096000.0,
                                          1.0 / 6402373705728000.0,
                                          1.0 / 121645100408832000.0,
                                          1.0 / 2432902008176640000.0,
                                          1.0 / 51090942171709440000.0,
                                          1.0 / 1124000727777607680000.0,
                                          1.0 / 25852016738884976640000.0};

template <int NRG>
struct RG {
  using G = RR<NRG>;
  static constexpr int LDS_D = 2 * G::IMG_D + B_NSLOT * G::BS + 8 * G::DMP + RR_KMAX * RR_CH + 16 + 4 * RR_KMAX;
};

// MODEL: the sweep also keeps the generator cotangent Z~_n = e^{mu_n} dT of every slice (d loss = sum_n <Z~_n, dX'_n> for the real
// slice generators X'_n of the tables), summed over the slices of the chain with the weights 1, c_1(n) .. c_K(n): 1 + K tile
// sets with their border slot per chain in A.mpart, in the layout of the tables.  Every element has ONE owner thread, which reads,
// updates and writes it in sweep order: no atomics, no barrier, the same bits on every run, and nothing kept in registers
// across the product loop.  regr_model_reduce_kernel turns the sums into the cotangents of h0, hks and col_ops.
// The sweep is ONE body (c3p_regrg_body.inc) compiled into two kernels: regr_grad_kernel<NRG> keeps its name and its code (the launch
// log and the committed dispatch table name it), regr_grad_model_kernel<NRG> is the MODEL form.
template <int NRG>
__global__ void __launch_bounds__(256, 1) regr_grad_kernel(RegrGradArgs A) {
  constexpr bool MODEL = false;
#include "c3p_regrg_body.inc"
}
template <int NRG>
__global__ void __launch_bounds__(256, 1) regr_grad_model_kernel(RegrGradArgs A) {
  constexpr bool MODEL = true;
#include "c3p_regrg_body.inc"
}

// ---- cotangent in the Hermitian basis, segment scan ------------------------------------------------------------------------
// out[b] = Re(T diag(e^{-i phi_b}) U_bar[b] T^+): real Dm x Dm row-major.  One workgroup per sample.
__global__ void __launch_bounds__(256) hb_ubar_kernel(const cplx* Ubar, const double* fr_phase, int Dh, double* out) {
  const int Dm = Dh * Dh;
  const long bidx = blockIdx.x;
  const cplx* ub = Ubar + bidx * (long)Dm * Dm;
  double* o = out + bidx * (long)Dm * Dm;
  for (int e = threadIdx.x; e < Dm * Dm; e += 256) {
    const int a = e / Dm, c = e - a * Dm;
    int ia[2], ic[2];
    cplx ta[2], tc[2];
    const int na = c3p_hb_row(a, Dh, ia, ta), nc = c3p_hb_row(c, Dh, ic, tc);
    double s = 0.0;
    for (int x = 0; x < na; ++x) {
      cplx ph = cmake(1.0, 0.0);
      if (fr_phase) {
        double sn, cs;
        sincos(fr_phase[bidx * Dm + ia[x]], &sn, &cs);
        ph = cmake(cs, -sn);
      }
      for (int y = 0; y < nc; ++y) {
        const cplx w = cmul(cmul(ta[x], cconj(tc[y])), cmul(ph, ub[(long)ia[x] * Dm + ic[y]]));
        s += w.x;
      }
    }
    o[e] = s;
  }
}

// C = op(A) op(B), real n x n row-major in global memory, staged through LDS (sa, sb: n x n each); all 256 threads
template <bool AT, bool BT>
__device__ void rg_mm(double* C, const double* Am, const double* Bm, int n, double* sa, double* sb) {
  const int tid = threadIdx.x;
  __syncthreads();
  for (int e = tid; e < n * n; e += 256) {
    const int i = e / n, k = e - i * n;
    sa[e] = AT ? Am[(long)k * n + i] : Am[e];
    sb[e] = BT ? Bm[(long)k * n + i] : Bm[e];
  }
  __syncthreads();
  for (int e = tid; e < n * n; e += 256) {
    const int i = e / n, jx = e - i * n;
    double s = 0.0;
    for (int k = 0; k < n; ++k) s = fma(sa[i * n + k], sb[k * n + jx], s);
    C[e] = s;
  }
  __syncthreads();
}

// per sample: pre[j] = S_{j-1} ... S_0 (j >= 1), suf[j] = S_{j+1}^T ... S_{S-1}^T U_bar', tau = <suf[0], S_0>
__global__ void __launch_bounds__(256) regr_scan_seq_kernel(const cplx* seg_slots, const double* ubar, int S, int Dm, double* pre, double* suf,
                                                            double* tau) {
  __shared__ double redt[256];
  const long msz = (long)Dm * Dm;
  const long bidx = blockIdx.x;
  double* sa = c3p_rg_lds;
  double* sb = sa + msz;
  auto segm = [&](int jx) -> const double* { return reinterpret_cast<const double*>(seg_slots + (bidx * S + jx) * msz) + msz; };
  double* pb = pre + bidx * S * msz;
  double* sfx = suf + bidx * S * msz;
  const int tid = threadIdx.x;
  if (S > 1) {
    for (long e = tid; e < msz; e += 256) pb[msz + e] = segm(0)[e];
    for (int jx = 2; jx < S; ++jx) rg_mm<false, false>(pb + jx * msz, segm(jx - 1), pb + (jx - 1) * msz, Dm, sa, sb);
  }
  for (long e = tid; e < msz; e += 256) sfx[(S - 1) * msz + e] = ubar[bidx * msz + e];
  for (int jx = S - 1; jx >= 1; --jx) rg_mm<true, false>(sfx + (jx - 1) * msz, segm(jx), sfx + jx * msz, Dm, sa, sb);
  __syncthreads();
  double part = 0.0;
  for (long e = tid; e < msz; e += 256) part = fma(sfx[e], segm(0)[e], part);
  redt[tid] = part;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < 256; ++i) s += redt[i];
    tau[bidx] = s;
  }
}

// lam[b, j] = suf[b, j] pre[b, j]^T (j = 0: suf[b, 0])
__global__ void __launch_bounds__(256) regr_scan_fold_kernel(const double* pre, const double* suf, int S, int Dm, double* lam) {
  const long msz = (long)Dm * Dm;
  const long m = blockIdx.x;
  const int jx = (int)(m % S);
  if (jx == 0) {
    for (long e = threadIdx.x; e < msz; e += 256) lam[m * msz + e] = suf[m * msz + e];
    return;
  }
  double* sa = c3p_rg_lds;
  rg_mm<false, true>(lam + m * msz, suf + m * msz, pre + m * msz, Dm, sa, sa + msz);
}

// ---- model-operator cotangents from the sums of regr_grad_model_kernel ---------------------------------------------------
// One workgroup per sample.  For k1 = 0 (weight 1) and every control line (weight c_k1(n)):
//   W' = the S segment sums added in ascending segment order, untiled to Dm x Dm row-major (real);
//   the trace shift of the tables: exp(X) = e^mu exp(X - mu 1), mu = tr X / Dm, so the cotangent of X is
//     Z' = Z~ - (tr Z~ / Dm) 1 + (tau / Dm) 1,  tau = <U_bar', U'>  (the term mu_k tau of the signal gradient),
//   applied once to the sums with the weights N (k1 = 0) and sum_n c_k1(n);
//   W = dt T^+ W' T: out of the Hermitian basis (T unitary: <Z', T dX T^+> = Re <T^+ Z' T, dX>); the tables hold dt G, and the
//   cotangents below are those of G;
//   grad_h0 (k1 = 0) or grad_hks[k1 - 1] = tau(W), and for k1 = 0 the adjoint of the dissipator map gives grad_col (c3p_grad.h).
// W' is real, so W is the cotangent restricted to the Hermiticity-preserving generators: grad_h0 / grad_hks come out Hermitian
// (the Hermitian part of the general sweep's), grad_col complete -- the dissipator preserves Hermiticity for every C.
// Fixed owners and order everywhere: the same bits on every run.
__global__ void __launch_bounds__(256) regr_model_reduce_kernel(const double* mpart, const double* tau, const double* signals, const cplx* col,
                                                                long col_bs, int C, int S, int K, int N, int Dh, double dt, cplx* g_h0, cplx* g_hks,
                                                                cplx* g_col) {
  __shared__ double red[256];
  __shared__ double shift_s;
  const int tid = threadIdx.x;
  const long bidx = blockIdx.x;
  const int Dm = Dh * Dh, msz = Dm * Dm;
  const int DP = c3p_regd_class(Dm), NRG = (DP - 1) / 16;
  const int TSET = NRG * NRG * 256, BS = 2 * DP;
  const long PD = (long)TSET + BS;
  cplx* W = reinterpret_cast<cplx*>(c3p_rg_lds);   // [Dm,Dm]
  cplx* R = W + msz;                               // [Dm]
  double* Wr = reinterpret_cast<double*>(R + Dm);  // [Dm,Dm]
  const double* pb = mpart + bidx * S * (1 + K) * PD;
  for (int k1 = 0; k1 <= K; ++k1) {
    for (int e = tid; e < msz; e += 256) {
      const int row = e / Dm, cl = e - row * Dm;
      int te;
      if (row == DP - 1) {
        te = TSET + cl;
      } else if (cl == DP - 1) {
        te = TSET + DP + row;
      } else {
        const int Ig = row >> 4, r16 = row & 15, w = cl / (4 * NRG), rem = cl - w * 4 * NRG;
        const int lane = ((r16 & 3) << 4) + ((r16 >> 2) << 2) + (rem & 3);
        te = (Ig * NRG + (rem >> 2)) * 256 + w * 64 + lane;
      }
      double acc = pb[(long)k1 * PD + te];
      for (int s = 1; s < S; ++s) acc += pb[((long)s * (1 + K) + k1) * PD + te];
      Wr[e] = acc;
    }
    double part = 0.0;
    if (k1 > 0) {
      const double* sk = signals + (bidx * K + (k1 - 1)) * N;
      for (int n = tid; n < N; n += 256) part += sk[n];
    }
    red[tid] = part;
    __syncthreads();
    if (tid == 0) {
      double wsum = (double)N;
      if (k1 > 0) {
        wsum = 0.0;
        for (int i = 0; i < 256; ++i) wsum += red[i];
      }
      double tr = 0.0;
      for (int a = 0; a < Dm; ++a) tr += Wr[a * Dm + a];
      shift_s = (wsum * tau[bidx] - tr) / (double)Dm;
    }
    __syncthreads();
    if (tid < Dm) Wr[tid * Dm + tid] += shift_s;
    __syncthreads();
    for (int e = tid; e < msz; e += 256) {
      const int al = e / Dm, be = e - al * Dm;
      int ia[2], ib[2];
      cplx ta[2], tb[2];
      const int na = c3p_hb_col(al, Dh, ia, ta), nb = c3p_hb_col(be, Dh, ib, tb);
      cplx s = cmake(0.0, 0.0);
      for (int x = 0; x < na; ++x)
        for (int y = 0; y < nb; ++y) {
          const cplx c = cmul(cconj(ta[x]), tb[y]);
          const double v = Wr[ia[x] * Dm + ib[y]];
          s.x = fma(c.x, v, s.x);
          s.y = fma(c.y, v, s.y);
        }
      W[e] = cscale(s, dt);
    }
    __syncthreads();
    cplx* gh = k1 == 0 ? g_h0 + bidx * Dm : g_hks + (bidx * K + (k1 - 1)) * Dm;
    for (int e = tid; e < Dm; e += 256) {
      const int a = e / Dh, c = e - a * Dh;
      gh[e] = c3p_lind_times_i(c3p_lind_tau_sum([&](int row, int cl) { return W[row * Dm + cl]; }, a, c, Dh));
    }
    if (k1 == 0) c3p_lind_dissipator_adjoint(W, R, col + bidx * col_bs, C, Dh, g_col + bidx * C * Dm);
    __syncthreads();
  }
}

template <int NRG, bool MODEL>
hipError_t launch_rg(const RegrGradArgs& A, hipStream_t st) {
  const size_t lds = (size_t)RG<NRG>::LDS_D * sizeof(double);
  const long nchains = (long)A.B * A.S;
  const unsigned grid = (unsigned)(nchains < C3P_REGD_MAX_WGS ? nchains : C3P_REGD_MAX_WGS);
  auto kern = MODEL ? regr_grad_model_kernel<NRG> : regr_grad_kernel<NRG>;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  C3P_LAUNCH(kern, dim3(grid), dim3(256), lds, st, A);
  return hipGetLastError();
}

}  // namespace

size_t c3p_regr_grad_arena_bytes(int Dm) {
  const int n = (c3p_regd_class(Dm) - 1) / 16;
  return (size_t)C3P_REGD_MAX_WGS * n * n * 256 * sizeof(double);
}

hipError_t c3p_launch_regr_grad(const RegrGradArgs& A, hipStream_t st) {
  if (A.K > RR_KMAX || A.K < 1 || !A.tables || !A.tables_t || !A.qT || !A.lam || !A.tau || !A.arena) return hipErrorInvalidValue;
  if (A.degree != 0 && A.degree != 8 && A.degree != 12 && A.degree != 16 && A.degree != 20) return hipErrorInvalidValue;
  const int cls = c3p_regd_class(A.Dm);
  if (A.mpart) {
    if (cls == 49) return launch_rg<3, true>(A, st);
    if (cls == 65) return launch_rg<4, true>(A, st);
    if (cls == 81) return launch_rg<5, true>(A, st);
    return hipErrorInvalidValue;
  }
  if (cls == 49) return launch_rg<3, false>(A, st);
  if (cls == 65) return launch_rg<4, false>(A, st);
  if (cls == 81) return launch_rg<5, false>(A, st);
  return hipErrorInvalidValue;
}

size_t c3p_regr_model_part_doubles(int Dm, int K) {
  const int cls = c3p_regd_class(Dm), n = (cls - 1) / 16;
  return (size_t)(1 + K) * ((size_t)n * n * 256 + 2 * cls);
}

hipError_t c3p_launch_regr_model_reduce(const double* mpart, const double* tau, const double* signals, const cplx* col, long col_bstride, int C,
                                        int B, int S, int K, int N, int Dh, double dt, cplx* g_h0, cplx* g_hks, cplx* g_col, hipStream_t st) {
  const int Dm = Dh * Dh;
  if (!mpart || !tau || !signals || !col || C < 1 || Dm > 81) return hipErrorInvalidValue;
  const size_t lds = ((size_t)2 * (Dm * Dm + Dm) + (size_t)Dm * Dm) * sizeof(double);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(regr_model_reduce_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  C3P_LAUNCH(regr_model_reduce_kernel, dim3((unsigned)B), dim3(256), lds, st, mpart, tau, signals, col, col_bstride, C, S, K, N, Dh, dt,
             g_h0, g_hks, g_col);
  return hipGetLastError();
}

hipError_t c3p_launch_hb_ubar(const cplx* Ubar, const double* fr_phase, int B, int Dh, double* out, hipStream_t st) {
  C3P_LAUNCH(hb_ubar_kernel, dim3((unsigned)B), dim3(256), 0, st, Ubar, fr_phase, Dh, out);
  return hipGetLastError();
}

hipError_t c3p_launch_regr_scan(const cplx* seg_slots, const double* ubar, int B, int S, int Dm, double* pre, double* suf, double* lam,
                                double* tau, hipStream_t st) {
  const size_t lds = (size_t)2 * Dm * Dm * sizeof(double);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(regr_scan_seq_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(regr_scan_fold_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  C3P_LAUNCH(regr_scan_seq_kernel, dim3((unsigned)B), dim3(256), lds, st, seg_slots, ubar, S, Dm, pre, suf, tau);
  C3P_LAUNCH(regr_scan_fold_kernel, dim3((unsigned)(B * S)), dim3(256), lds, st, pre, suf, S, Dm, lam);
  return hipGetLastError();
}
