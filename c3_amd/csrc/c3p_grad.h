// Launcher interface of the control-gradient kernels (c3p_grad.hip).
#pragma once
#include "c3p_common.h"

struct GradArgs {
  const cplx* h0;
  long h0_bstride;  // elements between samples (0 = shared)
  const cplx* hks;
  long hks_bstride;
  const double* signals;   // [B,K,N]
  const double* fr_phase;  // [B,D] or null
  const cplx* Ubar;        // [B,D,D] cotangent of U
  double dt;
  int B, K, N, D, ld;
  int S;  // time segments per sample, balanced: segment s covers [s N / S, (s+1) N / S)
  cplx* seg;     // [B,S,D,D] segment products (no frame rotation)
  cplx* Mb;      // [B,S,D,D] adjoint state at the END of each segment
  double* grad;  // [B,K,N]
  cplx* zout;    // [B,N,D,D] or null: Z_n = dU_n^H L(X_n, M_{n+1}), the cotangent of the generator G_n = -i dt H_n
  cplx* scratch;  // GLOBAL variant: scratch_stride elements per workgroup
  long scratch_stride;
  // general (non-unitary) generators, e.g. Lindblad superoperators: h0 / hks hold G_0 / G_k with X_n = dt (G_0 + sum c_k G_k)
  // (no factor -i), the slices have no cheap inverse, so the sweep keeps the prefix product of every slice in memory
  int general;
  cplx* pre;     // [B,S,D,D] prefix product at the START of each segment        (general only; Mb then holds the LEFT adjoint
  cplx* pstore;  // [B,N,D,D] prefix product in front of every slice              A = S^H FR^H Ubar at the end of each segment)
  // fused goal (c3p_pwc_unitary_goal_vjp): when goal_rows is set the scan kernel, which forms the total product anyway,
  // evaluates the gate infidelity of U = FR P and takes ITS cotangent as Ubar (Ubar above is then not read):
  //   s = tr(G^+ U[rows, rows]),  infid = 1 - |s / L|^2 (kind 0) or 1 - (|s|^2 / L + 1) / (L + 1) (kind 1),  Ubar = c s G on (rows x rows)
  const int* goal_rows;    // [L] computational rows (fidelities.py:154-184 via tf_project_to_comp), L <= C3P_GOAL_LMAX
  const cplx* goal_ideal;  // [L,L]
  int goal_L, goal_kind;
  double* goal_infid;   // [B]
  double* goal_gphase;  // [B,D] or null: d infid / d fr_phase
  cplx* goal_U;         // [B,D,D] or null: the propagators themselves
  // model-operator cotangents of the Lindblad path (c3p_launch_grad_bwd_general_model only)
  cplx* mpart;  // [B,S, D^2 + (K+1) Dsys^2] partial sums of every workgroup: W0, T0, T_1 .. T_K (c3p_grad.hip)
  int Dsys;     // system dimension, D = Dsys^2
};
#define C3P_GOAL_LMAX 64

#define C3P_GRAD_NMAT 19  // matrices a backward workgroup keeps (LDS or scratch)
#define C3P_GRAD_NMAT_GENERAL 20

int c3p_grad_threads(int D);
size_t c3p_grad_lds_bytes(int D);  // LDS variant footprint; > 150 KB => use the GLOBAL variant
hipError_t c3p_launch_grad_seg(const GradArgs& A, bool global_scratch, hipStream_t st);   // segment products
hipError_t c3p_launch_grad_scan(const GradArgs& A, bool global_scratch, hipStream_t st);  // adjoint state at segment ends
hipError_t c3p_launch_grad_bwd(const GradArgs& A, bool global_scratch, hipStream_t st);   // backward sweep, writes grad
// general generators (A.general = 1): same three passes without the unitarity shortcut
size_t c3p_grad_lds_bytes_general(int D);
hipError_t c3p_launch_grad_scan_general(const GradArgs& A, bool global_scratch, hipStream_t st);
hipError_t c3p_launch_grad_bwd_general(const GradArgs& A, bool global_scratch, hipStream_t st);
// the same sweep, which also leaves the partial sums of the model-operator cotangents in A.mpart (D = Dsys^2 <= C3P_MODEL_DM_MAX),
// and the kernel that adds them in segment order and applies the adjoint of the dissipator map: grad_h0 [B,D,D],
// grad_hks [B,K,D,D], grad_col [B,C,D,D] of the system dimension D, col [C,D,D] (col_bstride 0) or [B,C,D,D]
#define C3P_MODEL_DM_MAX 36
#define C3P_MODEL_NW 6  // 36 * 36 elements of W0 on 256 threads
hipError_t c3p_launch_grad_bwd_general_model(const GradArgs& A, bool global_scratch, hipStream_t st);
hipError_t c3p_launch_lind_model_reduce(const cplx* mpart, const cplx* col, long col_bstride, int C, int B, int S, int K, int D, double dt, cplx* g_h0,
                                        cplx* g_hks, cplx* g_col, hipStream_t st);
// dense Lindblad generators [nb][(K+1)][D^2 x D^2]: G_0 = -i (spre(h0) - spost(h0)) + clp, G_k = -i (spre(hk) - spost(hk))
// (propagation.py:551-582); nb = B when an operator stride is non-zero, else 1; clp [Dm,Dm] (clp_bstride 0) or one per sample
// per-slice variant: out[b,n] = -i (spre(hs[b,n]) - spost(hs[b,n])) + clp for every slice Hamiltonian (branch B + lindbladian)
hipError_t c3p_launch_lind_slice_generators(const cplx* hs, long hs_bstride, const cplx* clp, long clp_bstride, int B, int N, int D, cplx* out, hipStream_t st);
hipError_t c3p_launch_lind_generators(const cplx* h0, long h0_bstride, const cplx* hks, long hks_bstride, const cplx* clp,
                                      long clp_bstride, int nb, int K, int D, cplx* out, hipStream_t st);

// ---- the adjoint maps of the Lindblad generator (lind_gen_kernel, clp_kernel), shared by the reduce kernels of the model-operator
// cotangents: lind_model_reduce_kernel (c3p_grad.hip) and regr_model_reduce_kernel (c3p_regrg.hip) ----
// Z: the cotangent of the generator [Ds^2 x Ds^2], row (i,j), column (k,l); z(row, col) loads one element.
// tau(Z)[a,c] = i (sum_j Z[(a,j),(c,j)] - sum_i Z[(i,c),(i,a)]), the adjoint of H -> -i (H (x) 1 - 1 (x) H^T): this returns the
// bracket, c3p_lind_times_i the factor (a caller may scale in between)
template <class Ld>
__device__ __forceinline__ cplx c3p_lind_tau_sum(Ld&& z, int a, int c, int Ds) {
  cplx sum = cmake(0, 0);
  for (int j = 0; j < Ds; ++j) {
    const cplx p = z(a * Ds + j, c * Ds + j);
    const cplx m = z(j * Ds + c, j * Ds + a);
    sum.x += p.x - m.x;
    sum.y += p.y - m.y;
  }
  return sum;
}
__device__ __forceinline__ cplx c3p_lind_times_i(cplx v) { return cmake(-v.y, v.x); }
// The adjoint of the dissipator map  clp = sum_c C (x) C* - 1/2 (C^+C) (x) 1 - 1/2 1 (x) (C^+C)^T  (propagation.py:570-581) applied to
// W [Ds^2 x Ds^2, row-major, LDS], the cotangent of clp.  With d loss = Re sum conj(grad) d(operator), every operator entry an
// independent complex number:
//   R[p,q]      = sum_j W[(p,j),(q,j)] + sum_i W[(i,q),(i,p)]                       (the cotangent of C^+C is -R / 2)
//   grad_C[a,b] = sum_jl W[(a,j),(b,l)] C[j,l] + sum_ik conj(W[(i,a),(k,b)]) C[i,k] - 1/2 (C (R + R^+))[a,b]
// All threads of the workgroup; R: Ds^2 elements of LDS scratch; col [C,Ds,Ds]; g_col: the [C,Ds,Ds] block of this sample.  W is
// complete and visible on entry.
__device__ __forceinline__ void c3p_lind_dissipator_adjoint(const cplx* W, cplx* R, const cplx* col, int C, int Ds, cplx* g_col) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int Dm = Ds * Ds;
  for (int e = tid; e < Dm; e += nt) {
    const int p = e / Ds, q = e - p * Ds;
    cplx r = cmake(0, 0);
    for (int j = 0; j < Ds; ++j) r = cadd(r, cadd(W[(p * Ds + j) * Dm + (q * Ds + j)], W[(j * Ds + q) * Dm + (j * Ds + p)]));
    R[e] = r;
  }
  __syncthreads();
  for (int e = tid; e < C * Dm; e += nt) {
    const int c = e / Dm, ab = e - c * Dm, a = ab / Ds, bb = ab - a * Ds;
    const cplx* Cc = col + (long)c * Dm;
    cplx g = cmake(0, 0);
    for (int j = 0; j < Ds; ++j)
      for (int l = 0; l < Ds; ++l) {
        cfma(g, W[(a * Ds + j) * Dm + (bb * Ds + l)], Cc[j * Ds + l]);
        cfma(g, cconj(W[(j * Ds + a) * Dm + (l * Ds + bb)]), Cc[j * Ds + l]);
      }
    cplx h = cmake(0, 0);
    for (int p = 0; p < Ds; ++p) cfma(h, Cc[a * Ds + p], cadd(R[p * Ds + bb], cconj(R[bb * Ds + p])));
    g.x = fma(-0.5, h.x, g.x);
    g.y = fma(-0.5, h.y, g.y);
    g_col[(long)c * Dm + ab] = g;
  }
}
