// Dressing of batched models on the device: what Model.update_dressed does before every evaluation
// (c3/model.py:453-534) -- eigendecomposition of the drift Hamiltonian, the reorder-and-phase rule, T^+ A T for every control and
// collapse operator -- for P parameter sets in one launch, and its vector-Jacobian product.  fp64, 2 <= D <= 40.
//
// Forward, dress_jacobi_kernel: one matrix per workgroup (one wave for D <= 16, four above).  Cyclic Jacobi for complex Hermitian
// matrices with a round-robin pair ordering: the floor(D/2) rotations of a step touch disjoint rows and columns, so a step is
//   rotation parameters | barrier | A <- A J, V <- V J | barrier | A <- J^+ A | barrier
// with A and V in LDS.  Every threshold is relative to ||A||_F, sums are reduced in a fixed tree: bitwise reproducible.
// Backward, dress_vjp_kernel: takes T and the eigenvalues of the forward call, solves nothing again.
#include "c3p_dress.h"

namespace {

constexpr int kMaxD = C3P_DRESS_MAX_D;
constexpr int kMaxPairs = kMaxD / 2;
constexpr int kMaxSweeps = 30;

// status bits (include/c3prop.h)
constexpr int kRecovered = 1, kDegenerate = 2, kNotConverged = 4;

template <int NT>
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// pair k of step r of the round-robin tournament of n (even) players: player n-1 stays, the others rotate
__device__ __forceinline__ void rr_pair(int n, int r, int k, int* p, int* q) {
  int a, b;
  if (k == 0) {
    a = n - 1;
    b = r;
  } else {
    a = (r + k) % (n - 1);
    b = (r - k + (n - 1)) % (n - 1);
  }
  *p = a < b ? a : b;
  *q = a < b ? b : a;
}

template <int NT>
__global__ __launch_bounds__(NT) void dress_jacobi_kernel(DressArgs a) {
  extern __shared__ __align__(16) unsigned char dress_lds[];
  __shared__ double red[NT];
  __shared__ int redi[NT];
  __shared__ double rot_c[kMaxPairs], rot_app[kMaxPairs], rot_aqq[kMaxPairs];
  __shared__ cplx rot_s[kMaxPairs];
  __shared__ int rot_p[kMaxPairs], rot_q[kMaxPairs];  // rot_p < 0: no rotation (the bye, or a_pq = 0)
  __shared__ double ev[kMaxD], colmax[kMaxD];
  __shared__ int dest[kMaxD], rowused[kMaxD], colused[kMaxD];
  __shared__ cplx phase[kMaxD];

  const int D = a.D, DD = D * D, tid = threadIdx.x;
  const long set = blockIdx.x;
  cplx* A = reinterpret_cast<cplx*>(dress_lds);
  cplx* V = A + DD;
  const cplx* H = a.H + set * DD;
  int status = 0;

  // the lower triangle, as eigh reads it; V = I
  double nrm2_part = 0.0;
  for (int idx = tid; idx < DD; idx += NT) {
    const int i = idx / D, j = idx % D;
    cplx h;
    if (i > j) h = H[idx];
    else if (i < j) h = cconj(H[j * D + i]);
    else h = cmake(H[idx].x, 0.0);
    A[idx] = h;
    V[idx] = cmake(i == j ? 1.0 : 0.0, 0.0);
    nrm2_part += h.x * h.x + h.y * h.y;
  }
  __syncthreads();
  const double nrm2 = block_sum<NT>(nrm2_part, red);
  const double tol = (double)D * 0x1p-52;
  const double thr2 = tol * tol * nrm2;  // off(A) <= D 2^-52 ||A||_F, squared

  const int n = D + (D & 1), npairs = n / 2;
  for (int sweep = 0;; ++sweep) {
    double off_part = 0.0;
    for (int idx = tid; idx < DD; idx += NT) {
      const cplx h = A[idx];
      if (idx / D != idx % D) off_part += h.x * h.x + h.y * h.y;
    }
    const double off2 = block_sum<NT>(off_part, red);
    if (off2 <= thr2) break;
    if (sweep == kMaxSweeps) {  // (a NaN never compares below the threshold: it ends here)
      status |= kNotConverged;
      break;
    }
    for (int r = 0; r < n - 1; ++r) {
      if (tid < npairs) {
        int p, q;
        rr_pair(n, r, tid, &p, &q);
        rot_p[tid] = -1;
        if (q < D) {
          const cplx b = A[p * D + q];
          const double absb = hypot(b.x, b.y);
          if (absb > 0.0) {  // a_pq = 0 (with a_pp = a_qq or not): no rotation
            const double app = A[p * D + p].x, aqq = A[q * D + q].x;
            const double tau = (aqq - app) / (2.0 * absb);
            // the smaller root of t^2 + 2 tau t - 1 = 0 (|t| <= 1); a huge tau gives t = 0
            const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + hypot(1.0, tau));
            const double c = 1.0 / sqrt(fma(t, t, 1.0));
            const double s = t * c;
            rot_p[tid] = p;
            rot_q[tid] = q;
            rot_c[tid] = c;
            rot_s[tid] = cmake(s * (b.x / absb), s * (b.y / absb));  // sigma = s e^{i arg a_pq}
            rot_app[tid] = app - t * absb;
            rot_aqq[tid] = aqq + t * absb;
          }
        }
      }
      __syncthreads();
      // A <- A J, V <- V J:  col_p' = c col_p - conj(sigma) col_q,  col_q' = sigma col_p + c col_q
      for (int it = tid; it < 2 * D * npairs; it += NT) {
        const int k = it % npairs, row = it / npairs;  // row in [0, 2D): A's rows, then V's
        const int p = rot_p[k];
        if (p < 0) continue;
        const int q = rot_q[k];
        const double c = rot_c[k];
        const cplx s = rot_s[k];
        cplx* Mx = row < D ? A + row * D : V + (row - D) * D;
        const cplx x = Mx[p], y = Mx[q];
        Mx[p] = cmake(c * x.x - (s.x * y.x + s.y * y.y), c * x.y - (s.x * y.y - s.y * y.x));
        Mx[q] = cmake(c * y.x + (s.x * x.x - s.y * x.y), c * y.y + (s.x * x.y + s.y * x.x));
      }
      __syncthreads();
      // A <- J^+ A:  row_p' = c row_p - sigma row_q,  row_q' = conj(sigma) row_p + c row_q; the rotated pair exactly
      for (int it = tid; it < D * npairs; it += NT) {
        const int k = it / D, j = it % D;
        const int p = rot_p[k];
        if (p < 0) continue;
        const int q = rot_q[k];
        const double c = rot_c[k];
        const cplx s = rot_s[k];
        const cplx x = A[p * D + j], y = A[q * D + j];
        cplx xp = cmake(c * x.x - (s.x * y.x - s.y * y.y), c * x.y - (s.x * y.y + s.y * y.x));
        cplx yp = cmake(c * y.x + (s.x * x.x + s.y * x.y), c * y.y + (s.x * x.y - s.y * x.x));
        if (j == p) {
          xp = cmake(rot_app[k], 0.0);
          yp = cmake(0.0, 0.0);
        } else if (j == q) {
          xp = cmake(0.0, 0.0);
          yp = cmake(rot_aqq[k], 0.0);
        }
        A[p * D + j] = xp;
        A[q * D + j] = yp;
      }
      __syncthreads();
    }
  }

  // ---- the frame rule (model.py:453-491): eigenvector j goes to the bare state it overlaps most ----
  if (tid < D) {
    ev[tid] = A[tid * D + tid].x;
    double best = -1.0;
    int arg = 0;
    for (int i = 0; i < D; ++i) {
      const cplx v = V[i * D + tid];
      const double w = v.x * v.x + v.y * v.y;
      if (w > best) {
        best = w;
        arg = i;
      }
    }
    colmax[tid] = best;
    dest[tid] = arg;
    rowused[tid] = 0;
    colused[tid] = 0;
  }
  __syncthreads();
  bool ordered = true;
  for (int j = 0; j < D; ++j) ordered = ordered && (colmax[j] > 0.5);
  if (!ordered) {
    // the greedy recovery (model.py:469-475): D times the global argmax of what is left, first in row-major order on ties
    status |= kRecovered;
    for (int step = 0; step < D; ++step) {
      double best = -1.0;
      int arg = -1;
      for (int idx = tid; idx < DD; idx += NT) {
        if (rowused[idx / D] || colused[idx % D]) continue;
        const cplx v = V[idx];
        const double w = v.x * v.x + v.y * v.y;
        if (w > best) {
          best = w;
          arg = idx;
        }
      }
      red[tid] = best;
      redi[tid] = arg;
      __syncthreads();
      for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) {
          const double w2 = red[tid + s];
          const int i2 = redi[tid + s];
          if (i2 >= 0 && (redi[tid] < 0 || w2 > red[tid] || (w2 == red[tid] && i2 < redi[tid]))) {
            red[tid] = w2;
            redi[tid] = i2;
          }
        }
        __syncthreads();
      }
      if (tid == 0) {
        int i, j;
        if (redi[0] >= 0) {
          i = redi[0] / D;
          j = redi[0] % D;
        } else {  // nothing comparable is left (NaN): the first free row and column, so that dest stays a permutation
          i = j = 0;
          while (rowused[i]) ++i;
          while (colused[j]) ++j;
        }
        dest[j] = i;
        rowused[i] = 1;
        colused[j] = 1;
      }
      __syncthreads();
    }
  }
  // the phase of column j: T[i,i] real and positive (for a real drift: the reference's sign(Re v))
  if (tid < D) {
    const cplx v = V[dest[tid] * D + tid];
    const double av = hypot(v.x, v.y);
    phase[tid] = av > 0.0 ? cmake(v.x / av, -v.y / av) : cmake(1.0, 0.0);
    if (a.eig) a.eig[set * D + dest[tid]] = ev[tid];
  }
  __syncthreads();
  // T into A's tile (A is spent), and out
  for (int idx = tid; idx < DD; idx += NT) {
    const int i = idx / D, j = idx % D, d = dest[j];
    cplx t = cmul(V[idx], phase[j]);
    if (i == d) t.y = 0.0;
    A[i * D + d] = t;
    if (a.h0) a.h0[set * DD + i * D + d] = cmake(i == d ? ev[j] : 0.0, 0.0);
  }
  __syncthreads();
  if (a.T)
    for (int idx = tid; idx < DD; idx += NT) a.T[set * DD + idx] = A[idx];
  if (tid == 0 && a.status) a.status[set] = status;

  // ---- T^+ A_m T for the M operators: B = A_m T into V's tile, then T^+ B ----
  if (a.ops_out) {
    cplx* B = V;
    for (int m = 0; m < a.M; ++m) {
      const cplx* Am = a.ops + set * a.ops_bstride + (long)m * DD;
      cplx* out = a.ops_out + (set * a.M + m) * DD;
      __syncthreads();
      for (int idx = tid; idx < DD; idx += NT) {
        const int i = idx / D, j = idx % D;
        cplx acc = cmake(0.0, 0.0);
        for (int l = 0; l < D; ++l) cfma(acc, Am[i * D + l], A[l * D + j]);
        B[idx] = acc;
      }
      __syncthreads();
      for (int idx = tid; idx < DD; idx += NT) {
        const int i = idx / D, j = idx % D;
        cplx acc = cmake(0.0, 0.0);
        for (int l = 0; l < D; ++l) cfma(acc, cconj(A[l * D + i]), B[l * D + j]);
        out[idx] = acc;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Backward.  With e, T as returned (H T = T diag(e), T_jj real), d L = sum e_bar de + Re sum conj(G_bar_m) dG_m + Re sum conj(T_bar) dT:
//   A_bar_m = T G_bar_m T^+
//   T_bar  += sum_m  A_m T G_bar_m^+ + A_m^+ T G_bar_m
//   W       = T^+ T_bar,   g_j = Im W_jj / T_jj   (the phase gauge),   W'_kj = W_kj - i g_j conj(T_jk),  W'_jj = 0
//   H_bar   = herm( T (W' o F + diag(e_bar)) T^+ ),   F_kj = 1 / (e_j - e_k)
// One set per workgroup; T and one scratch tile in LDS, T_bar in registers (E elements per thread).
// ---------------------------------------------------------------------------------------------------------------------------
template <int NT, int E>
__global__ __launch_bounds__(NT) void dress_vjp_kernel(DressVjpArgs a) {
  extern __shared__ __align__(16) unsigned char dress_lds[];
  __shared__ double es[kMaxD];
  const int D = a.D, DD = D * D, tid = threadIdx.x;
  const long set = blockIdx.x;
  cplx* T = reinterpret_cast<cplx*>(dress_lds);
  cplx* X = T + DD;
  const cplx* Tg = a.T + set * DD;
  for (int idx = tid; idx < DD; idx += NT) T[idx] = Tg[idx];
  if (tid < D) es[tid] = a.eig[set * D + tid];
  cplx acc[E], w[E];
#pragma unroll
  for (int n = 0; n < E; ++n) {
    const int idx = tid + n * NT;
    acc[n] = (a.T_bar && idx < DD) ? a.T_bar[set * DD + idx] : cmake(0.0, 0.0);
  }
  __syncthreads();
  const bool per_set_out = a.ops_bstride != 0;
  if (a.ops_bar) {
    for (int m = 0; m < a.M; ++m) {
      const cplx* G = a.ops_bar + (set * a.M + m) * DD;
      const cplx* Am = a.ops + set * a.ops_bstride + (long)m * DD;
      // X = T G^+
#pragma unroll
      for (int n = 0; n < E; ++n) {
        const int idx = tid + n * NT;
        if (idx < DD) {
          const int i = idx / D, j = idx % D;
          cplx s = cmake(0.0, 0.0);
          for (int l = 0; l < D; ++l) cfma(s, T[i * D + l], cconj(G[j * D + l]));
          X[idx] = s;
        }
      }
      __syncthreads();
      // T_bar += A X
#pragma unroll
      for (int n = 0; n < E; ++n) {
        const int idx = tid + n * NT;
        if (idx < DD) {
          const int i = idx / D, j = idx % D;
          for (int l = 0; l < D; ++l) cfma(acc[n], Am[i * D + l], X[l * D + j]);
        }
      }
      __syncthreads();
      // X = T G
#pragma unroll
      for (int n = 0; n < E; ++n) {
        const int idx = tid + n * NT;
        if (idx < DD) {
          const int i = idx / D, j = idx % D;
          cplx s = cmake(0.0, 0.0);
          for (int l = 0; l < D; ++l) cfma(s, T[i * D + l], G[l * D + j]);
          X[idx] = s;
        }
      }
      __syncthreads();
      // T_bar += A^+ X;  A_bar = X T^+ (per-set operators: written here; shared ones are summed over the sets by dress_vjp_opsum_kernel)
#pragma unroll
      for (int n = 0; n < E; ++n) {
        const int idx = tid + n * NT;
        if (idx < DD) {
          const int i = idx / D, j = idx % D;
          for (int l = 0; l < D; ++l) cfma(acc[n], cconj(Am[l * D + i]), X[l * D + j]);
          if (a.ops_bare_bar && per_set_out) {
            cplx s = cmake(0.0, 0.0);
            for (int l = 0; l < D; ++l) cfma(s, X[i * D + l], cconj(T[j * D + l]));
            a.ops_bare_bar[(set * a.M + m) * DD + idx] = s;
          }
        }
      }
      __syncthreads();
    }
  }
  if (!a.H_bar) {
    if (tid == 0 && a.status) a.status[set] = 0;
    return;
  }
  // W = T^+ T_bar
#pragma unroll
  for (int n = 0; n < E; ++n)
    if (tid + n * NT < DD) X[tid + n * NT] = acc[n];
  __syncthreads();
#pragma unroll
  for (int n = 0; n < E; ++n) {
    const int idx = tid + n * NT;
    if (idx < DD) {
      const int k = idx / D, j = idx % D;
      cplx s = cmake(0.0, 0.0);
      for (int l = 0; l < D; ++l) cfma(s, cconj(T[l * D + k]), X[l * D + j]);
      w[n] = s;
    }
  }
  __syncthreads();
#pragma unroll
  for (int n = 0; n < E; ++n)
    if (tid + n * NT < DD) X[tid + n * NT] = w[n];
  __syncthreads();
  // Z = W' o F + diag(e_bar + Re diag h0_bar); a pair closer than 2^-40 max|e| contributes zero (status bit 2)
  double emax = 0.0;
  for (int j = 0; j < D; ++j) emax = fmax(emax, fabs(es[j]));
  const double gap_min = 0x1p-40 * emax;
  int degenerate = 0;
#pragma unroll
  for (int n = 0; n < E; ++n) {
    const int idx = tid + n * NT;
    if (idx < DD) {
      const int k = idx / D, j = idx % D;
      if (k == j) {
        double z = a.eig_bar ? a.eig_bar[set * D + j] : 0.0;
        if (a.h0_bar) z += a.h0_bar[set * DD + idx].x;
        w[n] = cmake(z, 0.0);
      } else {
        const double de = es[j] - es[k];
        if (!(fabs(de) > gap_min)) {
          degenerate = 1;
          w[n] = cmake(0.0, 0.0);
        } else {
          const double tjj = T[j * D + j].x;
          const double g = tjj != 0.0 ? X[j * D + j].y / tjj : 0.0;
          const cplx t = T[j * D + k];
          const cplx x = X[idx];
          w[n] = cmake((x.x - g * t.y) / de, (x.y - g * t.x) / de);
        }
      }
    }
  }
  degenerate = __syncthreads_or(degenerate);
#pragma unroll
  for (int n = 0; n < E; ++n)
    if (tid + n * NT < DD) X[tid + n * NT] = w[n];
  __syncthreads();
  // Q = T Z
#pragma unroll
  for (int n = 0; n < E; ++n) {
    const int idx = tid + n * NT;
    if (idx < DD) {
      const int i = idx / D, j = idx % D;
      cplx s = cmake(0.0, 0.0);
      for (int l = 0; l < D; ++l) cfma(s, T[i * D + l], X[l * D + j]);
      w[n] = s;
    }
  }
  __syncthreads();
#pragma unroll
  for (int n = 0; n < E; ++n)
    if (tid + n * NT < DD) X[tid + n * NT] = w[n];
  __syncthreads();
  // R = Q T^+
#pragma unroll
  for (int n = 0; n < E; ++n) {
    const int idx = tid + n * NT;
    if (idx < DD) {
      const int i = idx / D, j = idx % D;
      cplx s = cmake(0.0, 0.0);
      for (int l = 0; l < D; ++l) cfma(s, X[i * D + l], cconj(T[j * D + l]));
      w[n] = s;
    }
  }
  __syncthreads();
#pragma unroll
  for (int n = 0; n < E; ++n)
    if (tid + n * NT < DD) X[tid + n * NT] = w[n];
  __syncthreads();
  // H_bar = (R + R^+) / 2
  for (int idx = tid; idx < DD; idx += NT) {
    const int i = idx / D, j = idx % D;
    const cplx r = X[idx], rt = X[j * D + i];
    a.H_bar[set * DD + idx] = cmake(0.5 * (r.x + rt.x), 0.5 * (r.y - rt.y));
  }
  if (tid == 0 && a.status) a.status[set] = degenerate ? kDegenerate : 0;
}

// Shared bare operators: A_bar_m = sum_p T_p G_bar_pm T_p^+, row `blockIdx.x` of operator `blockIdx.y` per workgroup.  Wave w of the
// kOpsumWaves adds the sets p = w, w + kOpsumWaves, ... in order (sixteen waves: the loads of one set are latency, not bandwidth),
// the partial rows are added in wave order: no atomics, no workspace, bitwise reproducible.
constexpr int kOpsumWaves = 16;
__global__ __launch_bounds__(64 * kOpsumWaves) void dress_vjp_opsum_kernel(DressVjpArgs a) {
  __shared__ cplx u[kOpsumWaves][kMaxD];
  __shared__ cplx part[kOpsumWaves][kMaxD];
  const int D = a.D, DD = D * D, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x, m = blockIdx.y;
  cplx acc = cmake(0.0, 0.0);
  for (int p0 = 0; p0 < a.P; p0 += kOpsumWaves) {
    const long p = p0 + wv;
    const bool on = p < a.P && lane < D;
    const cplx* T = a.T + p * DD;
    if (on) {
      const cplx* G = a.ops_bar + (p * a.M + m) * DD;
      cplx s = cmake(0.0, 0.0);
      for (int l = 0; l < D; ++l) cfma(s, T[i * D + l], G[l * D + lane]);
      u[wv][lane] = s;
    }
    __syncthreads();
    if (on)
      for (int k = 0; k < D; ++k) cfma(acc, u[wv][k], cconj(T[lane * D + k]));
    __syncthreads();
  }
  if (lane < D) part[wv][lane] = acc;
  __syncthreads();
  if (wv == 0 && lane < D) {
    cplx s = part[0][lane];
    for (int k = 1; k < kOpsumWaves; ++k) s = cadd(s, part[k][lane]);
    a.ops_bare_bar[(long)m * DD + i * D + lane] = s;
  }
}

}  // namespace

hipError_t c3p_launch_dress(const DressArgs& a, hipStream_t st) {
  const size_t lds = 2 * (size_t)a.D * a.D * sizeof(cplx);
  if (a.D <= C3P_DRESS_WAVE_D)
    C3P_LAUNCH((dress_jacobi_kernel<64>), dim3(a.P), dim3(64), lds, st, a);
  else
    C3P_LAUNCH((dress_jacobi_kernel<256>), dim3(a.P), dim3(256), lds, st, a);
  return hipGetLastError();
}

hipError_t c3p_launch_dress_vjp(const DressVjpArgs& a, hipStream_t st) {
  const size_t lds = 2 * (size_t)a.D * a.D * sizeof(cplx);
  // elements of a [D,D] tile per thread: 16^2 / 64 = 4, 40^2 / 256 = 6.25
  if (a.D <= C3P_DRESS_WAVE_D)
    C3P_LAUNCH((dress_vjp_kernel<64, 4>), dim3(a.P), dim3(64), lds, st, a);
  else
    C3P_LAUNCH((dress_vjp_kernel<256, 7>), dim3(a.P), dim3(256), lds, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (a.ops_bare_bar && a.ops_bar && a.M > 0 && a.ops_bstride == 0) {
    C3P_LAUNCH(dress_vjp_opsum_kernel, dim3(a.D, a.M), dim3(64 * kOpsumWaves), 0, st, a);
    e = hipGetLastError();
  }
  return e;
}
