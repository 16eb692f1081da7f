// Tiled large-matrix propagator path: U[b] = prod_n exp(X_b[n]) for matrix dimensions beyond what a workgroup can
// keep on chip (Dm >= 93; the 729 x 729 Lindblad superoperator of three qutrits is the reference's own "takes way too
// long" case, test/test_tunable_coupler.py:406-418).  Matrices live in HBM (288 GB: ten 9 MB matrices per sample at
// Dm = 729 is nothing), every product is ONE batched launch of a tiled f64 MFMA GEMM, and the slice loop runs on the
// host: assemble X, T18 (5 products, Bader-Blanes-Casas) + s squarings, chain product.  The reference computes the
// same thing with tf.linalg.expm + tf.matmul (propagation.py:426-440, 551-585; tf_utils.py:144-193).
//
// Layout: every matrix is a HALF IMAGE of the real 2x2 representation, rows 2i / 2i+1 = Re / Im of row i, zero
// padded to [2 DPR][DPC] doubles (DPR = Dm rounded up to 32, DPC to 64) so that no tile needs a bounds check.
// C_h = R(A) B_h is then a plain real GEMM; R(A) (2M x 2K) is expanded from A_h while its panel is staged in LDS
// ([[a,-b],[b,a]] per element), B_h and C_h are used as stored.  64 x 64 output tile per workgroup of four waves,
// each wave 2 x 2 tiles of v_mfma_f64_16x16x4_f64, K panels of 16 double-buffered through registers and LDS.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "c3p_tiled.h"
#include "c3p_kernels.h"

namespace {

typedef double tg_d4 __attribute__((ext_vector_type(4)));

constexpr int TG_BM = 64, TG_BN = 64, TG_KP = 16;
constexpr int TG_SA = 17;  // LDS row stride of the expanded A panel (doubles)
constexpr int TG_SB = 80;  // LDS row stride of the B panel: = 16 mod 32, the two k rows of a half-wave hit disjoint banks
enum { M_X = 0, M_A2, M_A3, M_A6, M_T1, M_T2, M_T3, M_T4, M_U0, M_U1, M_COUNT };

struct TG {
  int Dm, DPR, DPC;
  long MS;  // doubles per matrix
  __host__ __device__ TG(int dm) : Dm(dm), DPR((dm + 31) / 32 * 32), DPC((dm + 63) / 64 * 64), MS(2L * ((dm + 31) / 32 * 32) * ((dm + 63) / 64 * 64)) {}
};

// ---- C = A B (+ Add), batched over blockIdx.z ------------------------------------------------------------------------
// (Add may alias C: every element is read and written by the same thread; C must not alias A or B)
// nptr (optional): the slice index lives in device memory (the per-slice launch sequences of the backward sweep are captured
// once into a hipGraph and replayed): B += (*nptr + noff) * nstride.
__global__ void __launch_bounds__(256) tg_gemm_kernel(const double* A, const double* Bm, const double* Add, double* C, int rows2,
                                                      int DPC, long strideA, long strideB, long strideC, const int* nptr = nullptr,
                                                      int noff = 0, long nstride = 0) {
  __shared__ double As[2][TG_BM * TG_SA];
  __shared__ double Bs[2][TG_KP * TG_SB];
  A += (long)blockIdx.z * strideA;
  Bm += (long)blockIdx.z * strideB;
  if (nptr) Bm += (long)(*nptr + noff) * nstride;
  C += (long)blockIdx.z * strideC;
  if (Add) Add += (long)blockIdx.z * strideC;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int r0 = blockIdx.y * TG_BM, c0 = blockIdx.x * TG_BN;
  // loaders: A_h panel 64 rows x 8 complex columns (2 doubles per thread), B_h panel 16 rows x 64 columns (4 per thread)
  const int a_row = tid >> 2, a_j = (tid & 3) * 2;
  const int b_row = tid >> 4, b_c = (tid & 15) * 4;
  const double* ap = A + (long)(r0 + a_row) * DPC + a_j;
  const double* bp = Bm + (long)b_row * DPC + c0 + b_c;
  const int a_rb = a_row & ~1, a_p = a_row & 1;
  tg_d4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (tg_d4){0.0, 0.0, 0.0, 0.0};
  const int npanel = rows2 / TG_KP;
  // operand panels are fetched TWO iterations ahead (register ring of two): with one panel of look-ahead a small product
  // (12 panels at Dm = 81, a handful of workgroups per CU) ran at one memory round trip per panel
  double2 av[2], bv0[2], bv1[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int pq = q < npanel ? q : 0;
    av[q] = *reinterpret_cast<const double2*>(ap + (long)pq * (TG_KP / 2));
    const double* bn = bp + (long)pq * TG_KP * DPC;
    bv0[q] = *reinterpret_cast<const double2*>(bn);
    bv1[q] = *reinterpret_cast<const double2*>(bn + 2);
  }
  // one panel: stage slot Q (compile-time: a run-time selection between the two register slots would make every iteration
  // wait for BOTH outstanding fetches), refill it with panel pn + 2, multiply
  auto panel = [&](int pn, auto qtag) {
    constexpr int Q = decltype(qtag)::value;
    double* as = As[Q];
    double* bs = Bs[Q];
    const double2 avc = av[Q], b0c = bv0[Q], b1c = bv1[Q];
    // expand R(A): a value of a Re row feeds (row, 2j) and (row + 1, 2j + 1); of an Im row (row - 1, 2j + 1) negated and (row, 2j)
    if (a_p == 0) {
      as[a_rb * TG_SA + 2 * a_j] = avc.x;
      as[(a_rb + 1) * TG_SA + 2 * a_j + 1] = avc.x;
      as[a_rb * TG_SA + 2 * a_j + 2] = avc.y;
      as[(a_rb + 1) * TG_SA + 2 * a_j + 3] = avc.y;
    } else {
      as[a_rb * TG_SA + 2 * a_j + 1] = -avc.x;
      as[(a_rb + 1) * TG_SA + 2 * a_j] = avc.x;
      as[a_rb * TG_SA + 2 * a_j + 3] = -avc.y;
      as[(a_rb + 1) * TG_SA + 2 * a_j + 2] = avc.y;
    }
    bs[b_row * TG_SB + b_c + 0] = b0c.x;
    bs[b_row * TG_SB + b_c + 1] = b0c.y;
    bs[b_row * TG_SB + b_c + 2] = b1c.x;
    bs[b_row * TG_SB + b_c + 3] = b1c.y;
    __syncthreads();  // (double buffered: the next panel writes the other buffer, one barrier per panel)
    if (pn + 2 < npanel) {
      av[Q] = *reinterpret_cast<const double2*>(ap + (long)(pn + 2) * (TG_KP / 2));
      const double* bn = bp + (long)(pn + 2) * TG_KP * DPC;
      bv0[Q] = *reinterpret_cast<const double2*>(bn);
      bv1[Q] = *reinterpret_cast<const double2*>(bn + 2);
    }
#pragma unroll
    for (int ks = 0; ks < TG_KP / 4; ++ks) {
      double af[2], bf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i] = as[(32 * wr + 16 * i + (lane & 15)) * TG_SA + 4 * ks + (lane >> 4)];
#pragma unroll
      for (int j = 0; j < 2; ++j) bf[j] = bs[(4 * ks + (lane >> 4)) * TG_SB + 32 * wc + 16 * j + (lane & 15)];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
  };
  for (int pn = 0; pn < npanel; pn += 2) {
    panel(pn, std::integral_constant<int, 0>{});
    if (pn + 1 < npanel) panel(pn + 1, std::integral_constant<int, 1>{});
  }
  // D layout of 16x16x4: register v of lane l = element (4 v + l / 16, l % 16)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const long e = (long)(r0 + 32 * wr + 16 * i + 4 * v + (lane >> 4)) * DPC + c0 + 32 * wc + 16 * j + (lane & 15);
        C[e] = acc[i][j][v] + (Add ? Add[e] : 0.0);
      }
}

// ---- several independent products in ONE launch, each C = A0 B0 (+ A1 B1) (+ Add) on slots of the per-sample matrix block ----
// The backward sweep is a chain of small GEMMs (a few hundred workgroups, 10 - 15 us each) and at small batches the launches,
// not the arithmetic, set the time: the pair evaluation of T18 has two independent results per dependency level (value and
// derivative), and every derivative is a SUM of two products (product rule).  One task = one result; blockIdx.z = task * nb +
// sample; the K loop runs over the panels of the first pair and then of the second.  Same tile code as tg_gemm_kernel.
struct TgTasks {
  int n;
  int a0[2], b0[2], a1[2], b1[2], add[2], c[2];  // slot indices; a1 < 0: one product; add < 0: none
};

__global__ void __launch_bounds__(256) tg_gemm_tasks_kernel(double* mats, long VS, long MS, TgTasks T, int nb, int rows2, int DPC) {
  __shared__ double As[2][TG_BM * TG_SA];
  __shared__ double Bs[2][TG_KP * TG_SB];
  const int task = blockIdx.z / nb, sample = blockIdx.z - task * nb;
  double* base = mats + (long)sample * VS;
  const bool dual = T.a1[task] >= 0;
  const double* A0 = base + (long)T.a0[task] * MS;
  const double* B0 = base + (long)T.b0[task] * MS;
  const double* A1 = dual ? base + (long)T.a1[task] * MS : A0;
  const double* B1 = dual ? base + (long)T.b1[task] * MS : B0;
  const double* Add = T.add[task] >= 0 ? base + (long)T.add[task] * MS : nullptr;
  double* C = base + (long)T.c[task] * MS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int r0 = blockIdx.y * TG_BM, c0 = blockIdx.x * TG_BN;
  const int a_row = tid >> 2, a_j = (tid & 3) * 2;
  const int b_row = tid >> 4, b_c = (tid & 15) * 4;
  const long aoff = (long)(r0 + a_row) * DPC + a_j, boff = (long)b_row * DPC + c0 + b_c;
  const int a_rb = a_row & ~1, a_p = a_row & 1;
  tg_d4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (tg_d4){0.0, 0.0, 0.0, 0.0};
  const int np1 = rows2 / TG_KP;
  const int npanel = dual ? 2 * np1 : np1;
  auto a_at = [&](int pn) { return (pn < np1 ? A0 : A1) + aoff + (long)(pn < np1 ? pn : pn - np1) * (TG_KP / 2); };
  auto b_at = [&](int pn) { return (pn < np1 ? B0 : B1) + boff + (long)(pn < np1 ? pn : pn - np1) * TG_KP * DPC; };
  double2 av[2], bv0[2], bv1[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int pq = q < npanel ? q : 0;
    av[q] = *reinterpret_cast<const double2*>(a_at(pq));
    const double* bn = b_at(pq);
    bv0[q] = *reinterpret_cast<const double2*>(bn);
    bv1[q] = *reinterpret_cast<const double2*>(bn + 2);
  }
  auto panel = [&](int pn, auto qtag) {
    constexpr int Q = decltype(qtag)::value;
    double* as = As[Q];
    double* bs = Bs[Q];
    const double2 avc = av[Q], b0c = bv0[Q], b1c = bv1[Q];
    if (a_p == 0) {
      as[a_rb * TG_SA + 2 * a_j] = avc.x;
      as[(a_rb + 1) * TG_SA + 2 * a_j + 1] = avc.x;
      as[a_rb * TG_SA + 2 * a_j + 2] = avc.y;
      as[(a_rb + 1) * TG_SA + 2 * a_j + 3] = avc.y;
    } else {
      as[a_rb * TG_SA + 2 * a_j + 1] = -avc.x;
      as[(a_rb + 1) * TG_SA + 2 * a_j] = avc.x;
      as[a_rb * TG_SA + 2 * a_j + 3] = -avc.y;
      as[(a_rb + 1) * TG_SA + 2 * a_j + 2] = avc.y;
    }
    bs[b_row * TG_SB + b_c + 0] = b0c.x;
    bs[b_row * TG_SB + b_c + 1] = b0c.y;
    bs[b_row * TG_SB + b_c + 2] = b1c.x;
    bs[b_row * TG_SB + b_c + 3] = b1c.y;
    __syncthreads();
    if (pn + 2 < npanel) {
      av[Q] = *reinterpret_cast<const double2*>(a_at(pn + 2));
      const double* bn = b_at(pn + 2);
      bv0[Q] = *reinterpret_cast<const double2*>(bn);
      bv1[Q] = *reinterpret_cast<const double2*>(bn + 2);
    }
#pragma unroll
    for (int ks = 0; ks < TG_KP / 4; ++ks) {
      double af[2], bf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i] = as[(32 * wr + 16 * i + (lane & 15)) * TG_SA + 4 * ks + (lane >> 4)];
#pragma unroll
      for (int j = 0; j < 2; ++j) bf[j] = bs[(4 * ks + (lane >> 4)) * TG_SB + 32 * wc + 16 * j + (lane & 15)];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
  };
  for (int pn = 0; pn < npanel; pn += 2) {
    panel(pn, std::integral_constant<int, 0>{});
    if (pn + 1 < npanel) panel(pn + 1, std::integral_constant<int, 1>{});
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const long e = (long)(r0 + 32 * wr + 16 * i + 4 * v + (lane >> 4)) * DPC + c0 + 32 * wc + 16 * j + (lane & 15);
        C[e] = acc[i][j][v] + (Add ? Add[e] : 0.0);
      }
}

// The same with 32 x 32 output tiles (one 16 x 16 MFMA tile per wave): a wave of the 64 x 64 form issues 192 dependent-accumulator
// MFMAs per product at Dm = 81 (5 us whatever the batch); for small batches a quarter of that per wave and four times the
// workgroups is the better split.
constexpr int TG_SB32 = 48;
__global__ void __launch_bounds__(256) tg_gemm_tasks32_kernel(double* mats, long VS, long MS, TgTasks T, int nb, int rows2, int DPC) {
  __shared__ double As[2][32 * TG_SA];
  __shared__ double Bs[2][TG_KP * TG_SB32];
  const int task = blockIdx.z / nb, sample = blockIdx.z - task * nb;
  double* base = mats + (long)sample * VS;
  const bool dual = T.a1[task] >= 0;
  const double* A0 = base + (long)T.a0[task] * MS;
  const double* B0 = base + (long)T.b0[task] * MS;
  const double* A1 = dual ? base + (long)T.a1[task] * MS : A0;
  const double* B1 = dual ? base + (long)T.b1[task] * MS : B0;
  const double* Add = T.add[task] >= 0 ? base + (long)T.add[task] * MS : nullptr;
  double* C = base + (long)T.c[task] * MS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  // loaders: A_h panel 32 rows x 8 complex columns (one double per thread), B_h panel 16 rows x 32 columns (two per thread)
  const int a_row = tid >> 3, a_j = tid & 7;
  const int b_row = tid >> 4, b_c = (tid & 15) * 2;
  const long aoff = (long)(r0 + a_row) * DPC + a_j, boff = (long)b_row * DPC + c0 + b_c;
  const int a_rb = a_row & ~1, a_p = a_row & 1;
  tg_d4 acc = (tg_d4){0.0, 0.0, 0.0, 0.0};
  const int np1 = rows2 / TG_KP;
  const int npanel = dual ? 2 * np1 : np1;
  auto a_at = [&](int pn) { return (pn < np1 ? A0 : A1) + aoff + (long)(pn < np1 ? pn : pn - np1) * (TG_KP / 2); };
  auto b_at = [&](int pn) { return (pn < np1 ? B0 : B1) + boff + (long)(pn < np1 ? pn : pn - np1) * TG_KP * DPC; };
  double av[2];
  double2 bv[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int pq = q < npanel ? q : 0;
    av[q] = *a_at(pq);
    bv[q] = *reinterpret_cast<const double2*>(b_at(pq));
  }
  auto panel = [&](int pn, auto qtag) {
    constexpr int Q = decltype(qtag)::value;
    double* as = As[Q];
    double* bs = Bs[Q];
    const double x = av[Q];
    const double2 bc = bv[Q];
    if (a_p == 0) {
      as[a_rb * TG_SA + 2 * a_j] = x;
      as[(a_rb + 1) * TG_SA + 2 * a_j + 1] = x;
    } else {
      as[a_rb * TG_SA + 2 * a_j + 1] = -x;
      as[(a_rb + 1) * TG_SA + 2 * a_j] = x;
    }
    bs[b_row * TG_SB32 + b_c + 0] = bc.x;
    bs[b_row * TG_SB32 + b_c + 1] = bc.y;
    __syncthreads();
    if (pn + 2 < npanel) {
      av[Q] = *a_at(pn + 2);
      bv[Q] = *reinterpret_cast<const double2*>(b_at(pn + 2));
    }
#pragma unroll
    for (int ks = 0; ks < TG_KP / 4; ++ks) {
      const double af = as[(16 * wr + (lane & 15)) * TG_SA + 4 * ks + (lane >> 4)];
      const double bf = bs[(4 * ks + (lane >> 4)) * TG_SB32 + 16 * wc + (lane & 15)];
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(af, bf, acc, 0, 0, 0);
    }
  };
  for (int pn = 0; pn < npanel; pn += 2) {
    panel(pn, std::integral_constant<int, 0>{});
    if (pn + 1 < npanel) panel(pn + 1, std::integral_constant<int, 1>{});
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const long e = (long)(r0 + 16 * wr + 4 * v + (lane >> 4)) * DPC + c0 + 16 * wc + (lane & 15);
    C[e] = acc[v] + (Add ? Add[e] : 0.0);
  }
}

// ---- generator elements ------------------------------------------------------------------------------------------------
// G = -i dt h (unitary) or the Lindblad generator dt (clp - i (h (x) I - I (x) h^T)) (propagation.py:565-582); with_clp only
// for the drift table / per-slice generators
__device__ __forceinline__ cplx tg_gelem(const cplx* h, const cplx* clp, int lindblad, int Dh, int Dm, double dt, bool with_clp,
                                         int row, int col) {
  if (!lindblad) {
    const cplx x = h[(long)row * Dm + col];
    return cmake(x.y * dt, -x.x * dt);
  }
  const int i = row / Dh, j = row - i * Dh, k = col / Dh, l = col - k * Dh;
  cplx v = with_clp ? clp[(long)row * Dm + col] : cmake(0.0, 0.0);
  if (j == l) {
    const cplx x = h[i * Dh + k];
    v.x += x.y;
    v.y -= x.x;
  }
  if (i == k) {
    const cplx x = h[l * Dh + j];
    v.x -= x.y;
    v.y += x.x;
  }
  return cscale(v, dt);
}

struct TabArgs {
  const cplx* h0;
  long h0_bstride;
  const cplx* hks;
  long hks_bstride;
  const cplx* clp;
  long clp_bstride;
  double dt;
  int K, Dh, Dm, lindblad;
  int b0;          // first sample of the chunk (per-sample tables)
  double* tables;  // [nsamp][1+K][MS]
  double* meta;    // [nsamp][1+K][4] = {mu_r, mu_i, ||G - mu||_1, 0}
};

// the dissipator of table set s (b0 counts samples only when the tables are per sample, as for h0 / hks)
__device__ __forceinline__ const cplx* tg_table_clp(const TabArgs& P, int s) { return P.clp + (long)(P.b0 + s) * P.clp_bstride; }
__device__ __forceinline__ const cplx* tg_table_src(const TabArgs& P, int ti, int s) {
  return ti == 0 ? P.h0 + (long)(P.b0 + s) * P.h0_bstride : P.hks + (long)(P.b0 + s) * P.hks_bstride + (long)(ti - 1) * P.Dh * P.Dh;
}

// one block per (table, sample): trace shift and 1-norm
__global__ void __launch_bounds__(256) tg_meta_kernel(TabArgs P) {
  __shared__ double r1[256], r2[256];
  const int ti = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
  const cplx* h = tg_table_src(P, ti, s);
  const cplx* clp = tg_table_clp(P, s);
  double tr = 0.0, tim = 0.0;
  for (int i = tid; i < P.Dm; i += 256) {
    const cplx v = tg_gelem(h, clp, P.lindblad, P.Dh, P.Dm, P.dt, ti == 0, i, i);
    tr += v.x;
    tim += v.y;
  }
  r1[tid] = tr;
  r2[tid] = tim;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) {
      r1[tid] += r1[tid + o];
      r2[tid] += r2[tid + o];
    }
    __syncthreads();
  }
  const double mur = 0.0, mui = r2[0] / P.Dm;  // imaginary shift only (c3p_smalld.hip: build_tables)
  __syncthreads();
  double cs = 0.0;
  for (int j = tid; j < P.Dm; j += 256) {
    double sum = 0.0;
    for (int i = 0; i < P.Dm; ++i) {
      cplx v = tg_gelem(h, clp, P.lindblad, P.Dh, P.Dm, P.dt, ti == 0, i, j);
      if (i == j) {
        v.x -= mur;
        v.y -= mui;
      }
      sum += hypot(v.x, v.y);
    }
    cs = fmax(cs, sum);
  }
  r1[tid] = cs;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) r1[tid] = fmax(r1[tid], r1[tid + o]);
    __syncthreads();
  }
  if (tid == 0) {
    double* m = P.meta + ((long)s * (1 + P.K) + ti) * 4;
    m[0] = mur;
    m[1] = mui;
    m[2] = r1[0];
    m[3] = 0.0;
  }
}

__global__ void __launch_bounds__(256) tg_table_kernel(TabArgs P, int DPR, int DPC) {
  const int ti = blockIdx.y, s = blockIdx.z;
  const long MS = 2L * DPR * DPC;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= MS) return;
  const int r = (int)(e / DPC), c = (int)(e - (long)r * DPC);
  const int i = r >> 1, p = r & 1;
  double out = 0.0;
  if (i < P.Dm && c < P.Dm) {
    const cplx* h = tg_table_src(P, ti, s);
    cplx g = tg_gelem(h, tg_table_clp(P, s), P.lindblad, P.Dh, P.Dm, P.dt, ti == 0, i, c);
    if (i == c) {
      const double* m = P.meta + ((long)s * (1 + P.K) + ti) * 4;
      g.x -= m[0];
      g.y -= m[1];
    }
    out = p ? g.y : g.x;
  }
  P.tables[((long)s * (1 + P.K) + ti) * MS + e] = out;
}

// max_n,b |c_k|: one block per control line, result as the bit pattern of a non-negative double (atomicMax on u64)
__global__ void __launch_bounds__(256) tg_sigmax_kernel(const double* sig, int B, int K, int N, unsigned long long* out) {
  __shared__ double r1[256];
  const int k = blockIdx.x, tid = threadIdx.x;
  double m = 0.0;
  for (long e = tid; e < (long)B * N; e += 256) {
    const long b = e / N, n = e - b * N;
    m = fmax(m, fabs(sig[(b * K + k) * N + n]));
  }
  r1[tid] = m;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) r1[tid] = fmax(r1[tid], r1[tid + o]);
    __syncthreads();
  }
  if (tid == 0) out[k] = (unsigned long long)__double_as_longlong(r1[0]);
}

// per-slice Hamiltonians: max over matrices of ||H||_1 (out[0]) and ||H||_inf (out[1]); ||clp||_1 with nmat = 1 -> out[0]
__global__ void __launch_bounds__(64) tg_hnorm_kernel(const cplx* hs, long bstride, int N, int D, unsigned long long* out) {
  const long m = blockIdx.x;
  const long b = m / N, n = m - b * N;
  const cplx* h = hs + b * bstride + n * (long)D * D;
  const int tid = threadIdx.x;
  double c1 = 0.0, ci = 0.0;
  for (int j = tid; j < D; j += 64) {
    double sc = 0.0, sr = 0.0;
    for (int i = 0; i < D; ++i) {
      sc += hypot(h[(long)i * D + j].x, h[(long)i * D + j].y);
      sr += hypot(h[(long)j * D + i].x, h[(long)j * D + i].y);
    }
    c1 = fmax(c1, sc);
    ci = fmax(ci, sr);
  }
  for (int o = 32; o >= 1; o >>= 1) {
    c1 = fmax(c1, __shfl_xor(c1, o));
    ci = fmax(ci, __shfl_xor(ci, o));
  }
  if (tid == 0) {
    atomicMax(out + 0, (unsigned long long)__double_as_longlong(c1));
    atomicMax(out + 1, (unsigned long long)__double_as_longlong(ci));
  }
}

struct AsmArgs {
  const double* tables;  // mode A
  const double* meta;
  int tab_per_sample;
  const double* signals;  // [B,K,N]
  int b0, n, K, N;
  // mode B: per-slice Hamiltonians
  const cplx* hs;
  long hs_bstride;
  const cplx* clp;
  long clp_bstride;
  int lindblad, Dh, Dm;
  double dt;
  double scale;
  double* X;     // [Bc][M_COUNT][MS] (slot M_X)
  double* mus;   // [Bc][2] running trace-shift sum
  double* mun;   // [Bc][2] this slice's trace shift
  const int* nptr;  // slots kernel only: slice index from device memory (n = *nptr + noff) when set
  int noff;
  int adjoint;      // slots kernel, per-slice mode: assemble X^H instead of X
};

// X = 2^-s (G0 + sum_k c_k G_k)  (propagation.py:426-439), or 2^-s G(H_n) for per-slice Hamiltonians (:295-308)
__global__ void __launch_bounds__(256) tg_assemble_kernel(AsmArgs P, int DPR, int DPC) {
  const int b = blockIdx.y;
  const long MS = 2L * DPR * DPC;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  double* X = P.X + (long)b * M_COUNT * MS + (long)M_X * MS;
  if (P.hs) {
    if (e < MS) {
      const int r = (int)(e / DPC), c = (int)(e - (long)r * DPC);
      const int i = r >> 1, p = r & 1;
      double out = 0.0;
      if (i < P.Dm && c < P.Dm) {
        const cplx* h = P.hs + (long)(P.b0 + b) * P.hs_bstride + (long)P.n * P.Dh * P.Dh;
        const cplx g = tg_gelem(h, P.clp + (long)(P.b0 + b) * P.clp_bstride, P.lindblad, P.Dh, P.Dm, P.dt, true, i, c);
        out = P.scale * (p ? g.y : g.x);
      }
      X[e] = out;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) P.mun[2 * b] = P.mun[2 * b + 1] = 0.0;
    return;
  }
  const int ts = P.tab_per_sample ? b : 0;
  const double* T = P.tables + (long)ts * (1 + P.K) * MS;
  const double* sg = P.signals + ((long)(P.b0 + b) * P.K) * P.N + P.n;
  if (e < MS) {
    double v = T[e];
    for (int k = 0; k < P.K; ++k) v = fma(sg[(long)k * P.N], T[(long)(k + 1) * MS + e], v);
    X[e] = P.scale * v;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const double* m = P.meta + (long)ts * (1 + P.K) * 4;
    double mr = m[0], mi = m[1];
    for (int k = 0; k < P.K; ++k) {
      mr = fma(sg[(long)k * P.N], m[4 * (k + 1)], mr);
      mi = fma(sg[(long)k * P.N], m[4 * (k + 1) + 1], mi);
    }
    P.mun[2 * b] = mr;
    P.mun[2 * b + 1] = mi;
    P.mus[2 * b] += mr;
    P.mus[2 * b + 1] = c3p_phase_add(P.mus[2 * b + 1], mi);
  }
}

// the same for a sample block of `nslots` matrices (backward sweep); table mode only
__global__ void __launch_bounds__(256) tg_assemble_slots_kernel(AsmArgs P, int nslots, int DPR, int DPC) {
  const int b = blockIdx.y;
  const long MS = 2L * DPR * DPC;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  double* X = P.X + (long)b * nslots * MS;
  const int n = P.nptr ? *P.nptr + P.noff : P.n;
  if (P.hs) {  // per-slice Hamiltonians (branch B): no tables, no trace shift
    if (e < MS) {
      const int r = (int)(e / DPC), c = (int)(e - (long)r * DPC);
      const int i = r >> 1, p = r & 1;
      double out = 0.0;
      if (i < P.Dm && c < P.Dm) {
        const cplx* h = P.hs + (long)(P.b0 + b) * P.hs_bstride + (long)n * P.Dh * P.Dh;
        const cplx* clp = P.clp + (long)(P.b0 + b) * P.clp_bstride;
        const cplx g = P.adjoint ? cconj(tg_gelem(h, clp, P.lindblad, P.Dh, P.Dm, P.dt, true, c, i))
                                 : tg_gelem(h, clp, P.lindblad, P.Dh, P.Dm, P.dt, true, i, c);
        out = P.scale * (p ? g.y : g.x);
      }
      X[e] = out;
    }
    return;
  }
  const int ts = P.tab_per_sample ? b : 0;
  const double* T = P.tables + (long)ts * (1 + P.K) * MS;
  const double* sg = P.signals + ((long)(P.b0 + b) * P.K) * P.N + n;
  if (e < MS) {
    double v = T[e];
    for (int k = 0; k < P.K; ++k) v = fma(sg[(long)k * P.N], T[(long)(k + 1) * MS + e], v);
    X[e] = P.scale * v;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const double* m = P.meta + (long)ts * (1 + P.K) * 4;
    double mr = m[0], mi = m[1];
    for (int k = 0; k < P.K; ++k) {
      mr = fma(sg[(long)k * P.N], m[4 * (k + 1)], mr);
      mi = fma(sg[(long)k * P.N], m[4 * (k + 1) + 1], mi);
    }
    P.mun[2 * b] = mr;
    P.mun[2 * b + 1] = mi;
    P.mus[2 * b] += mr;
    P.mus[2 * b + 1] = c3p_phase_add(P.mus[2 * b + 1], mi);
  }
}

__global__ void tg_count_kernel(int* n, int by) { *n += by; }

// T18 combinations (c3p_common.h): from X, A2, A3, A6 -> T1 = B1, T2 = B5, T3 = B4, T4 = B3, X <- B2
__global__ void __launch_bounds__(256) tg_combo_kernel(double* mats, int Dm, int DPR, int DPC) {
  const int b = blockIdx.y;
  const long MS = 2L * DPR * DPC;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= MS) return;
  double* M = mats + (long)b * M_COUNT * MS;
  const int r = (int)(e / DPC), c = (int)(e - (long)r * DPC);
  const double dg = ((r & 1) == 0 && (r >> 1) == c && c < Dm) ? 1.0 : 0.0;
  const double x = M[M_X * MS + e], a2 = M[M_A2 * MS + e], a3 = M[M_A3 * MS + e], a6 = M[M_A6 * MS + e];
  M[M_T1 * MS + e] = fma(C3P_T18_A31, a3, fma(C3P_T18_A21, a2, C3P_T18_A11 * x));
  M[M_T2 * MS + e] = fma(C3P_T18_B64, a6, fma(C3P_T18_B34, a3, C3P_T18_B24 * a2));
  M[M_T3 * MS + e] = fma(C3P_T18_B63, a6, fma(C3P_T18_B33, a3, fma(C3P_T18_B23, a2, fma(C3P_T18_B13, x, C3P_T18_B03 * dg))));
  M[M_T4 * MS + e] = fma(C3P_T18_B62, a6, fma(C3P_T18_B32, a3, fma(C3P_T18_B22, a2, fma(C3P_T18_B12, x, C3P_T18_B02 * dg))));
  M[M_X * MS + e] = fma(C3P_T18_B61, a6, fma(C3P_T18_B31, a3, fma(C3P_T18_B21, a2, C3P_T18_B11 * x)));
}

// dst = a + b (slots of the same sample)
__global__ void __launch_bounds__(256) tg_add_kernel(double* mats, int sa, int sb, int sd, long MS) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= MS) return;
  double* M = mats + (long)blockIdx.y * M_COUNT * MS;
  M[sd * MS + e] = M[sa * MS + e] + M[sb * MS + e];
}

// out[b][i][j] = e^{mu} e^{i phase_i} (M[2i][j] + i M[2i+1][j]) as interleaved complex [Dm][Dm]
__global__ void __launch_bounds__(256) tg_out_kernel(const double* mats, int slot, const double* mu, const double* phase, cplx* out,
                                                     long out_bstride, int Dm, int DPR, int DPC) {
  const int b = blockIdx.y;
  const long MS = 2L * DPR * DPC;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)Dm * Dm) return;
  const int i = (int)(e / Dm), j = (int)(e - (long)i * Dm);
  const double* M = mats + (long)b * M_COUNT * MS + (long)slot * MS;
  const double re = M[(long)(2 * i) * DPC + j], im = M[(long)(2 * i + 1) * DPC + j];
  double ang = mu ? mu[2 * b + 1] : 0.0;
  if (phase) ang += phase[(long)b * Dm + i];
  double sn, cs;
  sincos(ang, &sn, &cs);
  const double er = mu ? exp(mu[2 * b]) : 1.0;
  out[(long)b * out_bstride + e] = cmake(er * (cs * re - sn * im), er * (cs * im + sn * re));
}


// ---- backward sweep (c3p_tiled_vjp_run) ---------------------------------------------------------------------------------
enum {
  V_Y = 0, V_A2, V_A3, V_A6, V_T1, V_T2, V_T3, V_T4,      // value side of the pair evaluation (slot layout as the forward pass)
  V_V, V_DA2, V_DA3, V_DA6, V_DT1, V_DT2, V_DT3, V_DT4,   // derivative side
  V_P0, V_P1, V_L0, V_L1, V_COUNT
};

// dst = src^H in the half-image layout: dst[2i][j] = src[2j][i], dst[2i+1][j] = -src[2j+1][i]
__global__ void __launch_bounds__(256) tg_adjoint_kernel(const double* src, long sstride, double* dst, long dstride, int Dm, int DPR,
                                                         int DPC, const int* nptr = nullptr, int noff = 0) {
  const long MS = 2L * DPR * DPC;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= MS) return;
  const double* S = src + (long)blockIdx.y * sstride;
  double* Dd = dst + (long)blockIdx.y * dstride + (nptr ? (long)(*nptr + noff) * MS : 0);
  const int r = (int)(e / DPC), c = (int)(e - (long)r * DPC);
  const int i = r >> 1, p = r & 1;
  double v = 0.0;
  if (i < Dm && c < Dm) {
    const double x = S[(long)(2 * c + p) * DPC + i];
    v = p ? -x : x;
  }
  Dd[e] = v;
}

// T18 combinations with explicit slots; the derivative side drops the identity terms
__global__ void __launch_bounds__(256) tg_combo_slots_kernel(double* mats, int nslots, int sx, int s2, int s3, int s6, int t1, int t2,
                                                             int t3, int t4, int with_identity, int Dm, int DPR, int DPC) {
  const int b = blockIdx.y;
  const long MS = 2L * DPR * DPC;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= MS) return;
  double* M = mats + (long)b * nslots * MS;
  const int r = (int)(e / DPC), c = (int)(e - (long)r * DPC);
  const double dg = (with_identity && (r & 1) == 0 && (r >> 1) == c && c < Dm) ? 1.0 : 0.0;
  const double x = M[sx * MS + e], a2 = M[s2 * MS + e], a3 = M[s3 * MS + e], a6 = M[s6 * MS + e];
  M[t1 * MS + e] = fma(C3P_T18_A31, a3, fma(C3P_T18_A21, a2, C3P_T18_A11 * x));
  M[t2 * MS + e] = fma(C3P_T18_B64, a6, fma(C3P_T18_B34, a3, C3P_T18_B24 * a2));
  M[t3 * MS + e] = fma(C3P_T18_B63, a6, fma(C3P_T18_B33, a3, fma(C3P_T18_B23, a2, fma(C3P_T18_B13, x, C3P_T18_B03 * dg))));
  M[t4 * MS + e] = fma(C3P_T18_B62, a6, fma(C3P_T18_B32, a3, fma(C3P_T18_B22, a2, fma(C3P_T18_B12, x, C3P_T18_B02 * dg))));
  M[sx * MS + e] = fma(C3P_T18_B61, a6, fma(C3P_T18_B31, a3, fma(C3P_T18_B21, a2, C3P_T18_B11 * x)));
}

// value and derivative side of the T18 combinations in one launch (backward slices: two launches fewer per slice)
__global__ void __launch_bounds__(256) tg_combo2_slots_kernel(double* mats, int nslots, int sx, int s2, int s3, int s6, int t1, int t2,
                                                              int t3, int t4, int dx, int d2, int d3, int d6, int u1, int u2, int u3,
                                                              int u4, int Dm, int DPR, int DPC) {
  const int b = blockIdx.y;
  const long MS = 2L * DPR * DPC;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= MS) return;
  double* M = mats + (long)b * nslots * MS;
  const int r = (int)(e / DPC), c = (int)(e - (long)r * DPC);
  const double dg = ((r & 1) == 0 && (r >> 1) == c && c < Dm) ? 1.0 : 0.0;
  {
    const double x = M[sx * MS + e], a2 = M[s2 * MS + e], a3 = M[s3 * MS + e], a6 = M[s6 * MS + e];
    M[t1 * MS + e] = fma(C3P_T18_A31, a3, fma(C3P_T18_A21, a2, C3P_T18_A11 * x));
    M[t2 * MS + e] = fma(C3P_T18_B64, a6, fma(C3P_T18_B34, a3, C3P_T18_B24 * a2));
    M[t3 * MS + e] = fma(C3P_T18_B63, a6, fma(C3P_T18_B33, a3, fma(C3P_T18_B23, a2, fma(C3P_T18_B13, x, C3P_T18_B03 * dg))));
    M[t4 * MS + e] = fma(C3P_T18_B62, a6, fma(C3P_T18_B32, a3, fma(C3P_T18_B22, a2, fma(C3P_T18_B12, x, C3P_T18_B02 * dg))));
    M[sx * MS + e] = fma(C3P_T18_B61, a6, fma(C3P_T18_B31, a3, fma(C3P_T18_B21, a2, C3P_T18_B11 * x)));
  }
  {
    const double x = M[dx * MS + e], a2 = M[d2 * MS + e], a3 = M[d3 * MS + e], a6 = M[d6 * MS + e];
    M[u1 * MS + e] = fma(C3P_T18_A31, a3, fma(C3P_T18_A21, a2, C3P_T18_A11 * x));
    M[u2 * MS + e] = fma(C3P_T18_B64, a6, fma(C3P_T18_B34, a3, C3P_T18_B24 * a2));
    M[u3 * MS + e] = fma(C3P_T18_B63, a6, fma(C3P_T18_B33, a3, fma(C3P_T18_B23, a2, C3P_T18_B13 * x)));
    M[u4 * MS + e] = fma(C3P_T18_B62, a6, fma(C3P_T18_B32, a3, fma(C3P_T18_B22, a2, C3P_T18_B12 * x)));
    M[dx * MS + e] = fma(C3P_T18_B61, a6, fma(C3P_T18_B31, a3, fma(C3P_T18_B21, a2, C3P_T18_B11 * x)));
  }
}

__global__ void __launch_bounds__(256) tg_add2_slots_kernel(double* mats, int nslots, int sa, int sb, int sd, int ta, int tb, int td,
                                                            long MS) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= MS) return;
  double* M = mats + (long)blockIdx.y * nslots * MS;
  M[sd * MS + e] = M[sa * MS + e] + M[sb * MS + e];
  M[td * MS + e] = M[ta * MS + e] + M[tb * MS + e];
}

__global__ void __launch_bounds__(256) tg_add_slots_kernel(double* mats, int nslots, int sa, int sb, int sd, long MS) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= MS) return;
  double* M = mats + (long)blockIdx.y * nslots * MS;
  M[sd * MS + e] = M[sa * MS + e] + M[sb * MS + e];
}

// Lambda = conj(e^{M}) diag(e^{-i phase}) U_bar as a half image; tau = <Lambda, P> (complex) for the trace-shift term
__global__ void __launch_bounds__(256) tg_ubar_kernel(const cplx* ubar, const double* mus, const double* phase, const double* P,
                                                      long pstride, double* lam, long lstride, double* tau, int Dm, int DPR, int DPC) {
  __shared__ double r1[256], r2[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long MS = 2L * DPR * DPC;
  double* Lm = lam + (long)b * lstride;
  const double* Pm = P + (long)b * pstride;
  for (long e = tid; e < MS; e += 256) Lm[e] = 0.0;
  __syncthreads();
  const double er = exp(mus[2 * b]), mi = mus[2 * b + 1];
  double tr = 0.0, ti = 0.0;
  for (long e = tid; e < (long)Dm * Dm; e += 256) {
    const int i = (int)(e / Dm), j = (int)(e - (long)i * Dm);
    const double ang = -(mi + (phase ? phase[(long)b * Dm + i] : 0.0));  // conj(e^{M}) e^{-i phase_i}
    double sn, cs;
    sincos(ang, &sn, &cs);
    const cplx u = ubar[(long)b * Dm * Dm + e];
    const double lr = er * (cs * u.x - sn * u.y), li = er * (cs * u.y + sn * u.x);
    Lm[(long)(2 * i) * DPC + j] = lr;
    Lm[(long)(2 * i + 1) * DPC + j] = li;
    const double pr = Pm[(long)(2 * i) * DPC + j], pi = Pm[(long)(2 * i + 1) * DPC + j];
    tr += lr * pr + li * pi;  // conj(lambda) p
    ti += lr * pi - li * pr;
  }
  r1[tid] = tr;
  r2[tid] = ti;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) {
      r1[tid] += r1[tid + o];
      r2[tid] += r2[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    tau[2 * b] = r1[0];
    tau[2 * b + 1] = r2[0];
  }
}

// Z[b][n] = scale Xbar as interleaved complex [Dm][Dm] (per-slice mode: the cotangent of the slice generator)
__global__ void __launch_bounds__(256) tg_genbar_kernel(const double* mats, int nslots, int slot, double scale, cplx* zout, long z_bstride,
                                                        const int* nptr, int noff, int Dm, int DPR, int DPC) {
  const int b = blockIdx.y;
  const long MS = 2L * DPR * DPC;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)Dm * Dm) return;
  const int n = *nptr + noff;
  const int i = (int)(e / Dm), j = (int)(e - (long)i * Dm);
  const double* M = mats + ((long)b * nslots + slot) * MS;
  zout[(long)b * z_bstride + (long)n * Dm * Dm + e] = cmake(scale * M[(long)(2 * i) * DPC + j], scale * M[(long)(2 * i + 1) * DPC + j]);
}

// grad[b][k][n] = scale <Xbar, G_k> + Re(mu_k tau): one block per (k, sample)
__global__ void __launch_bounds__(256) tg_graddot_kernel(const double* mats, int nslots, int slot, const double* tables, const double* meta,
                                                         int tab_per_sample, int K, const double* tau, double scale, double* grad, int b0,
                                                         const int* nptr, int noff, int N, long MS) {
  __shared__ double r1[256];
  const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int n = *nptr + noff;
  const double* X = mats + ((long)b * nslots + slot) * MS;
  const int ts = tab_per_sample ? b : 0;
  const double* G = tables + ((long)ts * (1 + K) + (k + 1)) * MS;
  double acc = 0.0;
  for (long e = tid; e < MS; e += 256) acc = fma(X[e], G[e], acc);
  r1[tid] = acc;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) r1[tid] += r1[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const double* m = meta + ((long)ts * (1 + K) + (k + 1)) * 4;
    grad[((long)(b0 + b) * K + k) * N + n] = scale * r1[0] + (m[0] * tau[2 * b] - m[1] * tau[2 * b + 1]);
  }
}

#define TG_TRY(expr)                                                                  \
  do {                                                                                \
    hipError_t e__ = (expr);                                                          \
    if (e__ != hipSuccess) {                                                          \
      err = std::string(#expr) + " failed: " + hipGetErrorString(e__);                \
      return -1;                                                                      \
    }                                                                                 \
  } while (0)

}  // namespace

size_t c3p_tiled_ws_bytes(int Dm, int K, int Bc, bool per_sample_tables) {
  const TG g(Dm);
  const size_t nt = per_sample_tables ? (size_t)Bc : 1;
  return ((size_t)Bc * M_COUNT * g.MS + nt * (1 + K) * (g.MS + 4) + 4 * (size_t)Bc + 64) * sizeof(double);
}

int c3p_tiled_chunk(int Dm, int K, int B, bool per_sample_tables, size_t budget_bytes) {
  int bc = B;
  while (bc > 1 && c3p_tiled_ws_bytes(Dm, K, bc, per_sample_tables) > budget_bytes) bc = (bc + 1) / 2;
  return bc;
}

int c3p_tiled_run(const TiledArgs& A, void* ws, int Bc, hipStream_t st, std::string& err) {
  const TG g(A.Dm);
  const long MS = g.MS;
  const bool per_sample = !A.per_slice && (A.h0_bstride != 0 || A.hks_bstride != 0 || A.clp_bstride != 0);
  const int K = A.per_slice ? 0 : A.K;
  const size_t nt = per_sample ? (size_t)Bc : 1;
  double* mats = reinterpret_cast<double*>(ws);
  double* tables = mats + (size_t)Bc * M_COUNT * MS;
  double* meta = tables + nt * (1 + K) * MS;
  double* mus = meta + nt * (1 + K) * 4;
  double* mun = mus + 2 * (size_t)Bc;
  unsigned long long* red = reinterpret_cast<unsigned long long*>(mun + 2 * (size_t)Bc);  // 64 words
  const unsigned ebl = (unsigned)((MS + 255) / 256);
  const dim3 ggrid((unsigned)(g.DPC / TG_BN), (unsigned)(2 * g.DPR / TG_BM), 1);

  for (int b0 = 0; b0 < A.B; b0 += Bc) {
    const int nb = A.B - b0 < Bc ? A.B - b0 : Bc;
    const int nts = per_sample ? nb : 1;
    // ---- tables (mode A) and the norm bound that fixes the squaring count ----
    double bound = 0.0;
    TG_TRY(hipMemsetAsync(red, 0, 64 * sizeof(unsigned long long), st));
    TabArgs T = {};
    if (!A.per_slice) {
      T.h0 = A.h0;
      T.h0_bstride = A.h0_bstride;
      T.hks = A.hks;
      T.hks_bstride = A.hks_bstride;
      T.clp = A.clp;
      T.clp_bstride = A.clp_bstride;
      T.dt = A.dt;
      T.K = K;
      T.Dh = A.D;
      T.Dm = A.Dm;
      T.lindblad = A.lindblad;
      T.b0 = per_sample ? b0 : 0;
      T.tables = tables;
      T.meta = meta;
      if (b0 == 0 || per_sample) {
        C3P_LAUNCH(tg_meta_kernel, dim3(1 + K, nts), dim3(256), 0, st, T);
        C3P_LAUNCH(tg_table_kernel, dim3(ebl, 1 + K, nts), dim3(256), 0, st, T, g.DPR, g.DPC);
      }
      if (K > 0)
        C3P_LAUNCH(tg_sigmax_kernel, dim3(K), dim3(256), 0, st, A.signals + (long)b0 * K * A.N, nb, K, A.N, red);
      TG_TRY(hipGetLastError());
      std::vector<double> hm((size_t)nts * (1 + K) * 4);
      std::vector<unsigned long long> hr(64);
      TG_TRY(hipMemcpyAsync(hm.data(), meta, hm.size() * sizeof(double), hipMemcpyDeviceToHost, st));
      TG_TRY(hipMemcpyAsync(hr.data(), red, 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
      TG_TRY(hipStreamSynchronize(st));
      for (int ti = 0; ti <= K; ++ti) {
        double nk = 0.0;
        for (int s = 0; s < nts; ++s) nk = std::max(nk, hm[((size_t)s * (1 + K) + ti) * 4 + 2]);
        double cm = 1.0;
        if (ti > 0) memcpy(&cm, &hr[ti - 1], 8);
        bound += cm * nk;
      }
    } else {
      const long nmat = (long)nb * A.N;
      C3P_LAUNCH(tg_hnorm_kernel, dim3((unsigned)nmat), dim3(64), 0, st, A.h0 + (long)b0 * A.h0_bstride, A.h0_bstride, A.N,
                         A.D, red);
      if (A.lindblad)  // ||clp||_1: the maximum over the chunk's dissipators when they are per sample
        C3P_LAUNCH(tg_hnorm_kernel, dim3(A.clp_bstride ? (unsigned)nb : 1u), dim3(64), 0, st, A.clp + (long)b0 * A.clp_bstride, A.clp_bstride, 1,
                   A.Dm, red + 2);
      TG_TRY(hipGetLastError());
      std::vector<unsigned long long> hr(64);
      TG_TRY(hipMemcpyAsync(hr.data(), red, 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
      TG_TRY(hipStreamSynchronize(st));
      double h1, hi, c1;
      memcpy(&h1, &hr[0], 8);
      memcpy(&hi, &hr[1], 8);
      memcpy(&c1, &hr[2], 8);
      bound = A.lindblad ? A.dt * (h1 + hi + c1) : A.dt * h1;
    }
    int s18 = 0;
    {
      double p = C3P_T18_THETA;
      while (p < bound && s18 < 60) {
        p *= 2.0;
        ++s18;
      }
    }
    TG_TRY(hipMemsetAsync(mus, 0, 4 * (size_t)Bc * sizeof(double), st));
    const dim3 eg(ebl, (unsigned)nb);
    dim3 gg = ggrid;
    gg.z = (unsigned)nb;
    auto M = [&](int slot) -> double* { return mats + (long)slot * MS; };
    auto gemm = [&](int a, int b, int add, int c) {
      C3P_LAUNCH(tg_gemm_kernel, gg, dim3(256), 0, st, M(a), M(b), add >= 0 ? M(add) : nullptr, M(c), 2 * g.DPR, g.DPC,
                         (long)M_COUNT * MS, (long)M_COUNT * MS, (long)M_COUNT * MS);
    };
    int ucur = M_U0;
    for (int n = 0; n < A.N; ++n) {
      AsmArgs P = {};
      P.tables = tables;
      P.meta = meta;
      P.tab_per_sample = per_sample ? 1 : 0;
      P.signals = A.signals;
      P.b0 = b0;
      P.n = n;
      P.K = K;
      P.N = A.N;
      if (A.per_slice) {
        P.hs = A.h0;
        P.hs_bstride = A.h0_bstride;
      }
      P.clp = A.clp;
      P.clp_bstride = A.clp_bstride;
      P.lindblad = A.lindblad;
      P.Dh = A.D;
      P.Dm = A.Dm;
      P.dt = A.dt;
      P.scale = ldexp(1.0, -s18);
      P.X = mats;
      P.mus = mus;
      P.mun = mun;
      C3P_LAUNCH(tg_assemble_kernel, eg, dim3(256), 0, st, P, g.DPR, g.DPC);
      gemm(M_X, M_X, -1, M_A2);
      gemm(M_X, M_A2, -1, M_A3);
      gemm(M_A3, M_A3, -1, M_A6);
      C3P_LAUNCH(tg_combo_kernel, eg, dim3(256), 0, st, mats, A.Dm, g.DPR, g.DPC);
      gemm(M_T1, M_T2, M_T3, M_A2);                                                   // A9 = B1 B5 + B4
      C3P_LAUNCH(tg_add_kernel, eg, dim3(256), 0, st, mats, M_T4, M_A2, M_A3, MS);  // B3 + A9
      gemm(M_A3, M_A2, M_X, M_A6);                                                    // T18 = (B3 + A9) A9 + B2
      int e = M_A6, o = M_T1;
      for (int it = 0; it < s18; ++it) {
        gemm(e, e, -1, o);
        std::swap(e, o);
      }
      if (A.dUs_out)
        C3P_LAUNCH(tg_out_kernel, dim3((unsigned)(((long)A.Dm * A.Dm + 255) / 256), (unsigned)nb), dim3(256), 0, st, mats, e,
                           mun, (const double*)nullptr, A.dUs_out + ((long)b0 * A.N + n) * A.Dm * A.Dm, (long)A.N * A.Dm * A.Dm, A.Dm,
                           g.DPR, g.DPC);
      if (n == 0) {
        // U <- E: a product with the identity would cost a launch too; copy instead
        for (int b = 0; b < nb; ++b)
          TG_TRY(hipMemcpyAsync(mats + ((long)b * M_COUNT + ucur) * MS, mats + ((long)b * M_COUNT + e) * MS, MS * sizeof(double),
                                hipMemcpyDeviceToDevice, st));
      } else {
        const int unew = ucur == M_U0 ? M_U1 : M_U0;
        gemm(e, ucur, -1, unew);
        ucur = unew;
      }
      TG_TRY(hipGetLastError());
    }
    C3P_LAUNCH(tg_out_kernel, dim3((unsigned)(((long)A.Dm * A.Dm + 255) / 256), (unsigned)nb), dim3(256), 0, st, mats, ucur, mus,
                       A.fr_phase ? A.fr_phase + (long)b0 * A.Dm : nullptr, A.U_out + (long)b0 * A.Dm * A.Dm, (long)A.Dm * A.Dm, A.Dm,
                       g.DPR, g.DPC);
    TG_TRY(hipGetLastError());
  }
  return 0;
}

// ---- vector-Jacobian product of the whole tiled path -------------------------------------------------------------------
size_t c3p_tiled_vjp_ws_bytes(int Dm, int K, int N, int Bc, bool per_sample_tables) {
  const TG g(Dm);
  const size_t nt = per_sample_tables ? (size_t)Bc : 1;
  return ((size_t)Bc * V_COUNT * g.MS + (size_t)Bc * (N + 1) * g.MS + 2 * nt * (1 + K) * (g.MS + 4) + 12 * (size_t)Bc + 64) * sizeof(double);
}

int c3p_tiled_vjp_chunk(int Dm, int K, int N, int B, bool per_sample_tables, size_t budget_bytes) {
  int bc = B;
  while (bc > 1 && c3p_tiled_vjp_ws_bytes(Dm, K, N, bc, per_sample_tables) > budget_bytes) bc = (bc + 1) / 2;
  return bc;
}

// Replays `body(pair)` `pairs` times.  With `use_graph` the body is captured ONCE into a hipGraph (it must be identical from
// replay to replay: the slice index lives in device memory) and launched as a graph -- ~35 kernel launches per slice are
// what bounds this sweep at a few hundred samples; otherwise (capture unsupported on this stream, e.g. the legacy default
// stream, or the caller is capturing itself) the launches are issued one by one.
template <typename F>
int tg_replay(hipStream_t st, bool use_graph, int pairs, F&& body, std::string& err) {
  if (pairs <= 0) return 0;
  if (use_graph && pairs >= 2) {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess) {
      body();
      hipError_t e = hipStreamEndCapture(st, &graph);
      if (e == hipSuccess && graph && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess) {
        for (int i = 0; i < pairs; ++i) TG_TRY(hipGraphLaunch(exec, st));
        (void)hipGraphExecDestroy(exec);
        (void)hipGraphDestroy(graph);
        return 0;
      }
      if (graph) (void)hipGraphDestroy(graph);
      (void)hipGetLastError();
      err = "hipGraph capture of the slice sequence failed";
      return -1;  // the captured launches did not run: no silent fallback with a half-advanced counter
    }
    (void)hipGetLastError();
  }
  for (int i = 0; i < pairs; ++i) body();
  TG_TRY(hipGetLastError());
  return 0;
}

int c3p_tiled_vjp_run(const TiledArgs& A, const cplx* U_bar, double* grad, cplx* zout, void* ws, int Bc, hipStream_t st, std::string& err) {
  const TG g(A.Dm);
  const long MS = g.MS;
  const bool per_slice = A.per_slice != 0;  // branch B: h0 = per-slice Hamiltonians, result = generator cotangents (zout)
  const bool per_sample = !per_slice && (A.h0_bstride != 0 || A.hks_bstride != 0 || A.clp_bstride != 0);
  const int K = per_slice ? 0 : A.K, N = A.N;
  const size_t nt = per_sample ? (size_t)Bc : 1;
  double* mats = reinterpret_cast<double*>(ws);
  double* store = mats + (size_t)Bc * V_COUNT * MS;          // [Bc][N + 1][MS]: slot n = B_n^H, adjoints of the forward partial products
  double* tables = store + (size_t)Bc * (N + 1) * MS;        // G_k - mu_k
  double* tables_adj = tables + nt * (1 + K) * MS;           // their adjoints
  double* meta = tables_adj + nt * (1 + K) * MS;
  double* meta_adj = meta + nt * (1 + K) * 4;
  double* mus = meta_adj + nt * (1 + K) * 4;
  double* mun = mus + 2 * (size_t)Bc;
  double* junk = mun + 2 * (size_t)Bc;  // trace-shift outputs of the backward assemblies (unused)
  double* tau = junk + 4 * (size_t)Bc;
  unsigned long long* red = reinterpret_cast<unsigned long long*>(tau + 2 * (size_t)Bc);
  int* nctr = reinterpret_cast<int*>(red + 32);  // slice counter of the replayed launch sequences
  const unsigned ebl = (unsigned)((MS + 255) / 256);
  const dim3 ggrid((unsigned)(g.DPC / TG_BN), (unsigned)(2 * g.DPR / TG_BM), 1);
  const long VS = (long)V_COUNT * MS, SS = (long)(N + 1) * MS;
  // Replaying the slice sequences as hipGraphs is OPT-IN (C3P_TILED_GRAPH=1): measured at cfg4's operators, B = 16 / 64,
  // 501 / 759 ms with graphs against 495 / 754 ms without -- the sweep is bound by the latency of its ~47 dependent small
  // kernels per slice (a 192-deep GEMM on a 96 x 128 half image is 12 K-panels of ~0.8 us each), not by launch overhead.
  // Graphs need a capturable stream: not the legacy default stream, not a stream that is itself being captured.
  bool use_graph = st != nullptr && c3p_opt_on(C3P_OPT_tiled_graph);
  const bool no_batch = c3p_opt_on(C3P_OPT_tiled_no_batch);  // A/B switch: one launch per product in the backward slices
  const long t32e = c3p_opt(C3P_OPT_tiled_tile32);
  if (use_graph) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) use_graph = false;
    (void)hipGetLastError();
  }

  for (int b0 = 0; b0 < A.B; b0 += Bc) {
    const int nb = A.B - b0 < Bc ? A.B - b0 : Bc;
    const int nts = per_sample ? nb : 1;
    TG_TRY(hipMemsetAsync(red, 0, 64 * sizeof(unsigned long long), st));
    double bound = 0.0;
    if (!per_slice) {
      TabArgs T = {};
      T.h0 = A.h0;
      T.h0_bstride = A.h0_bstride;
      T.hks = A.hks;
      T.hks_bstride = A.hks_bstride;
      T.clp = A.clp;
      T.clp_bstride = A.clp_bstride;
      T.dt = A.dt;
      T.K = K;
      T.Dh = A.D;
      T.Dm = A.Dm;
      T.lindblad = A.lindblad;
      T.b0 = per_sample ? b0 : 0;
      T.tables = tables;
      T.meta = meta;
      if (b0 == 0 || per_sample) {
        C3P_LAUNCH(tg_meta_kernel, dim3(1 + K, nts), dim3(256), 0, st, T);
        C3P_LAUNCH(tg_table_kernel, dim3(ebl, 1 + K, nts), dim3(256), 0, st, T, g.DPR, g.DPC);
        C3P_LAUNCH(tg_adjoint_kernel, dim3(ebl, (unsigned)(nts * (1 + K))), dim3(256), 0, st, tables, MS, tables_adj, MS, A.Dm,
                           g.DPR, g.DPC, (const int*)nullptr, 0);
      }
      C3P_LAUNCH(tg_sigmax_kernel, dim3(K), dim3(256), 0, st, A.signals + (long)b0 * K * N, nb, K, N, red);
      TG_TRY(hipGetLastError());
      std::vector<double> hm((size_t)nts * (1 + K) * 4);
      std::vector<unsigned long long> hr(64);
      TG_TRY(hipMemcpyAsync(hm.data(), meta, hm.size() * sizeof(double), hipMemcpyDeviceToHost, st));
      TG_TRY(hipMemcpyAsync(hr.data(), red, 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
      TG_TRY(hipStreamSynchronize(st));
      for (int ti = 0; ti <= K; ++ti) {
        double nk = 0.0;
        for (int sidx = 0; sidx < nts; ++sidx) nk = std::max(nk, hm[((size_t)sidx * (1 + K) + ti) * 4 + 2]);
        double cm = 1.0;
        if (ti > 0) memcpy(&cm, &hr[ti - 1], 8);
        bound += cm * nk;
      }
      TG_TRY(hipMemcpyAsync(meta_adj, meta, nt * (1 + K) * 4 * sizeof(double), hipMemcpyDeviceToDevice, st));
    } else {
      const long nmat = (long)nb * N;
      C3P_LAUNCH(tg_hnorm_kernel, dim3((unsigned)nmat), dim3(64), 0, st, A.h0 + (long)b0 * A.h0_bstride, A.h0_bstride, N, A.D, red);
      if (A.lindblad)  // ||clp||_1: the maximum over the chunk's dissipators when they are per sample
        C3P_LAUNCH(tg_hnorm_kernel, dim3(A.clp_bstride ? (unsigned)nb : 1u), dim3(64), 0, st, A.clp + (long)b0 * A.clp_bstride, A.clp_bstride, 1,
                   A.Dm, red + 2);
      TG_TRY(hipGetLastError());
      std::vector<unsigned long long> hr(64);
      TG_TRY(hipMemcpyAsync(hr.data(), red, 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
      TG_TRY(hipStreamSynchronize(st));
      double h1, hi, c1;
      memcpy(&h1, &hr[0], 8);
      memcpy(&hi, &hr[1], 8);
      memcpy(&c1, &hr[2], 8);
      bound = A.lindblad ? A.dt * (h1 + hi + c1) : A.dt * h1;
    }
    int s18 = 0;
    {
      double p = C3P_T18_THETA;
      while (p < bound && s18 < 60) {
        p *= 2.0;
        ++s18;
      }
    }
    const double scale = ldexp(1.0, -s18);
    TG_TRY(hipMemsetAsync(mus, 0, 2 * (size_t)Bc * sizeof(double), st));
    TG_TRY(hipMemsetAsync(nctr, 0, sizeof(int), st));
    const dim3 eg(ebl, (unsigned)nb);
    dim3 gg = ggrid;
    gg.z = (unsigned)nb;
    // small batches: 32 x 32 output tiles in the backward levels (see tg_gemm_tasks32_kernel); C3P_TILED_TILE32=0/1 overrides
    const bool tile32 = t32e >= 0 ? t32e != 0 : ((long)ggrid.x * ggrid.y * nb * 2 < 1024);
    auto M = [&](int slot) -> double* { return mats + (long)slot * MS; };
    auto gemm = [&](int a, int b, int add, int c) {
      C3P_LAUNCH(tg_gemm_kernel, gg, dim3(256), 0, st, M(a), M(b), add >= 0 ? M(add) : nullptr, M(c), 2 * g.DPR, g.DPC, VS, VS,
                         VS, (const int*)nullptr, 0, 0L);
    };
    // X (or X^H) of slice *nctr + off into slot V_Y
    auto assemble = [&](const double* tabs, const double* mt, int off, double* ms, double* mn) {
      AsmArgs P = {};
      P.tables = tabs;
      P.meta = mt;
      P.tab_per_sample = per_sample ? 1 : 0;
      P.signals = A.signals;
      P.b0 = b0;
      P.K = K;
      P.N = N;
      P.clp = A.clp;
      P.clp_bstride = A.clp_bstride;
      P.lindblad = A.lindblad;
      P.Dh = A.D;
      P.Dm = A.Dm;
      P.dt = A.dt;
      P.scale = scale;
      P.X = mats;  // slot V_Y == 0 of a V_COUNT-slot sample block
      P.mus = ms;
      P.mun = mn;
      P.nptr = nctr;
      P.noff = off;
      if (per_slice) {
        P.hs = A.h0;
        P.hs_bstride = A.h0_bstride;
        P.adjoint = (tabs == tables_adj) ? 1 : 0;
      }
      C3P_LAUNCH(tg_assemble_slots_kernel, eg, dim3(256), 0, st, P, V_COUNT, g.DPR, g.DPC);
    };
    auto copy_slot = [&](int src, int dst) -> int {
      for (int b = 0; b < nb; ++b)
        TG_TRY(hipMemcpyAsync(mats + (long)b * VS + (long)dst * MS, mats + (long)b * VS + (long)src * MS, MS * sizeof(double),
                              hipMemcpyDeviceToDevice, st));
      return 0;
    };
    // value side of T18 + squarings from the generator in slot V_Y; returns the slot of exp (the same for every slice)
    auto t18_value = [&]() -> int {
      gemm(V_Y, V_Y, -1, V_A2);
      gemm(V_Y, V_A2, -1, V_A3);
      gemm(V_A3, V_A3, -1, V_A6);
      C3P_LAUNCH(tg_combo_slots_kernel, eg, dim3(256), 0, st, mats, V_COUNT, V_Y, V_A2, V_A3, V_A6, V_T1, V_T2, V_T3, V_T4, 1,
                         A.Dm, g.DPR, g.DPC);
      gemm(V_T1, V_T2, V_T3, V_A2);
      C3P_LAUNCH(tg_add_slots_kernel, eg, dim3(256), 0, st, mats, V_COUNT, V_T4, V_A2, V_A3, MS);
      gemm(V_A3, V_A2, V_Y, V_A6);
      int e = V_A6, o = V_T1;
      for (int it = 0; it < s18; ++it) {
        gemm(e, e, -1, o);
        std::swap(e, o);
      }
      return e;
    };
    // ---- forward: partial products P_n = E_n ... E_0 (trace-shifted), their adjoints stored (slot n + 1 = B_{n+1}^H) ----
    // one forward slice at counter + off: P_out = E P_in, adjoint -> store[n + 1] (the last one is never read)
    auto fwd_slice = [&](int off, int pin, int pout) {
      assemble(tables, meta, off, mus, mun);
      const int e = t18_value();
      gemm(e, pin, -1, pout);
      C3P_LAUNCH(tg_adjoint_kernel, eg, dim3(256), 0, st, M(pout), VS, store + MS, SS, A.Dm, g.DPR, g.DPC, (const int*)nctr, off);
    };
    int pcur = V_P0;
    {
      // slice 0: P_0 = E_0
      assemble(tables, meta, 0, mus, mun);
      const int e = t18_value();
      if (copy_slot(e, pcur)) return -1;
      if (N > 1)
        C3P_LAUNCH(tg_adjoint_kernel, eg, dim3(256), 0, st, M(pcur), VS, store + MS, SS, A.Dm, g.DPR, g.DPC, (const int*)nctr, 0);
      C3P_LAUNCH(tg_count_kernel, dim3(1), dim3(1), 0, st, nctr, 1);
      TG_TRY(hipGetLastError());
    }
    {
      int rem = N - 1;  // slices 1 .. N-1; the store has N slots (index n + 1 <= N - 1 is guaranteed by skipping the last write below)
      if (rem > 0 && (rem & 1)) {
        const int pn = pcur == V_P0 ? V_P1 : V_P0;
        fwd_slice(0, pcur, pn);
        C3P_LAUNCH(tg_count_kernel, dim3(1), dim3(1), 0, st, nctr, 1);
        pcur = pn;
        --rem;
      }
      const int pa = pcur, pb = pcur == V_P0 ? V_P1 : V_P0;
      if (tg_replay(st, use_graph, rem / 2, [&]() {
            fwd_slice(0, pa, pb);
            fwd_slice(1, pb, pa);
            C3P_LAUNCH(tg_count_kernel, dim3(1), dim3(1), 0, st, nctr, 2);
          }, err))
        return -1;
    }
    // (the counter is now N; the adjoint of P_{N-1} went to store slot N, which is one past the end: the store is sized N + 1)
    // ---- cotangent of the trace-shifted product and the trace-shift term ----
    int lcur = V_L0;
    C3P_LAUNCH(tg_ubar_kernel, dim3((unsigned)nb), dim3(256), 0, st, U_bar + (long)b0 * A.Dm * A.Dm, mus,
                       A.fr_phase ? A.fr_phase + (long)b0 * A.Dm : nullptr, M(pcur), VS, M(lcur), VS, tau, A.Dm, g.DPR, g.DPC);
    C3P_LAUNCH(tg_count_kernel, dim3(1), dim3(1), 0, st, nctr, -1);  // counter = N - 1
    // ---- backward: Ebar_n = Lambda_n B_n^H, Xbar_n = L(X_n^H)[Ebar_n] by the pair evaluation of T18, Lambda_{n-1} = E_n^H Lambda_n ----
    // one backward slice at n = counter + off >= 1
    auto bwd_slice = [&](int off, int lin, int lout, bool first_slice_zero) {
      if (!first_slice_zero)
        C3P_LAUNCH(tg_gemm_kernel, gg, dim3(256), 0, st, M(lin), store, (const double*)nullptr, M(V_V), 2 * g.DPR, g.DPC, VS, SS,
                           VS, (const int*)nctr, off, MS);
      assemble(tables_adj, meta_adj, off, junk, junk + 2 * (size_t)Bc);  // Y = X_n^H (scaled)
      // two results per dependency level (value, derivative), every derivative the sum of two products: one launch per level
      // (C3P_TILED_NO_BATCH=1: one launch per product, the first form of this sweep)
      auto level = [&](int va, int vb, int vadd, int vc, int da0, int db0, int da1, int db1, int dadd, int dc) {
        if (no_batch) {
          gemm(va, vb, vadd, vc);
          gemm(da0, db0, dadd, dc);
          gemm(da1, db1, dc, dc);
          return;
        }
        TgTasks T = {};
        T.n = 2;
        T.a0[0] = va, T.b0[0] = vb, T.a1[0] = -1, T.b1[0] = -1, T.add[0] = vadd, T.c[0] = vc;
        T.a0[1] = da0, T.b0[1] = db0, T.a1[1] = da1, T.b1[1] = db1, T.add[1] = dadd, T.c[1] = dc;
        dim3 g2 = ggrid;
        g2.z = (unsigned)(2 * nb);
        if (tile32) {
          g2.x *= 2;
          g2.y *= 2;
          C3P_LAUNCH(tg_gemm_tasks32_kernel, g2, dim3(256), 0, st, mats, VS, MS, T, nb, 2 * g.DPR, g.DPC);
        } else {
          C3P_LAUNCH(tg_gemm_tasks_kernel, g2, dim3(256), 0, st, mats, VS, MS, T, nb, 2 * g.DPR, g.DPC);
        }
      };
      level(V_Y, V_Y, -1, V_A2, V_V, V_Y, V_Y, V_V, -1, V_DA2);
      level(V_Y, V_A2, -1, V_A3, V_V, V_A2, V_Y, V_DA2, -1, V_DA3);
      level(V_A3, V_A3, -1, V_A6, V_DA3, V_A3, V_A3, V_DA3, -1, V_DA6);
      if (no_batch) {
        C3P_LAUNCH(tg_combo_slots_kernel, eg, dim3(256), 0, st, mats, V_COUNT, V_Y, V_A2, V_A3, V_A6, V_T1, V_T2, V_T3, V_T4, 1,
                           A.Dm, g.DPR, g.DPC);
        C3P_LAUNCH(tg_combo_slots_kernel, eg, dim3(256), 0, st, mats, V_COUNT, V_V, V_DA2, V_DA3, V_DA6, V_DT1, V_DT2, V_DT3,
                           V_DT4, 0, A.Dm, g.DPR, g.DPC);
      } else {
        C3P_LAUNCH(tg_combo2_slots_kernel, eg, dim3(256), 0, st, mats, V_COUNT, V_Y, V_A2, V_A3, V_A6, V_T1, V_T2, V_T3, V_T4,
                           V_V, V_DA2, V_DA3, V_DA6, V_DT1, V_DT2, V_DT3, V_DT4, A.Dm, g.DPR, g.DPC);
      }
      level(V_T1, V_T2, V_T3, V_A2, V_DT1, V_T2, V_T1, V_DT2, V_DT3, V_DA2);  // A9 = B1 B5 + B4; dA9 = dB1 B5 + B1 dB5 + dB4
      if (no_batch) {
        C3P_LAUNCH(tg_add_slots_kernel, eg, dim3(256), 0, st, mats, V_COUNT, V_T4, V_A2, V_A3, MS);     // L = B3 + A9
        C3P_LAUNCH(tg_add_slots_kernel, eg, dim3(256), 0, st, mats, V_COUNT, V_DT4, V_DA2, V_DA3, MS);  // dL
      } else {
        C3P_LAUNCH(tg_add2_slots_kernel, eg, dim3(256), 0, st, mats, V_COUNT, V_T4, V_A2, V_A3, V_DT4, V_DA2, V_DA3, MS);
      }
      level(V_A3, V_A2, V_Y, V_A6, V_DA3, V_A2, V_A3, V_DA2, V_V, V_DA6);  // F = L A9 + B2; dF = dL A9 + L dA9 + dB2
      int e = V_A6, o = V_T1, de = V_DA6, dq = V_DT1;
      for (int it = 0; it < s18; ++it) {
        level(e, e, -1, o, de, e, e, de, -1, dq);
        std::swap(e, o);
        std::swap(de, dq);
      }
      if (per_slice)
        C3P_LAUNCH(tg_genbar_kernel, dim3((unsigned)(((long)A.Dm * A.Dm + 255) / 256), (unsigned)nb), dim3(256), 0, st, mats, V_COUNT,
                           de, scale, zout + (long)b0 * N * A.Dm * A.Dm, (long)N * A.Dm * A.Dm, (const int*)nctr, off, A.Dm, g.DPR, g.DPC);
      else
        C3P_LAUNCH(tg_graddot_kernel, dim3((unsigned)K, (unsigned)nb), dim3(256), 0, st, mats, V_COUNT, de, tables, meta,
                           per_sample ? 1 : 0, K, tau, scale, grad, b0, (const int*)nctr, off, N, MS);
      if (lout >= 0) gemm(e, lin, -1, lout);  // Lambda_{n-1} = E_n^H Lambda_n
    };
    {
      int rem = N - 1;  // slices N-1 .. 1
      if (rem > 0 && (rem & 1)) {
        const int ln = lcur == V_L0 ? V_L1 : V_L0;
        bwd_slice(0, lcur, ln, false);
        C3P_LAUNCH(tg_count_kernel, dim3(1), dim3(1), 0, st, nctr, -1);
        lcur = ln;
        --rem;
      }
      const int la = lcur, lb = lcur == V_L0 ? V_L1 : V_L0;
      if (tg_replay(st, use_graph, rem / 2, [&]() {
            bwd_slice(0, la, lb, false);
            bwd_slice(-1, lb, la, false);
            C3P_LAUNCH(tg_count_kernel, dim3(1), dim3(1), 0, st, nctr, -2);
          }, err))
        return -1;
      // slice 0: B_0 = I, Ebar_0 = Lambda_0 (the counter is 0)
      if (copy_slot(lcur, V_V)) return -1;
      bwd_slice(0, lcur, -1, true);
      TG_TRY(hipGetLastError());
    }
  }
  return 0;
}
