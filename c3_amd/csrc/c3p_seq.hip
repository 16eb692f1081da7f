// Indexed gate-sequence chains (c3p_seq_chain).
//
// For P parameter samples and S sequences of indices into a gate table G[p] [n_gates, M, M], every chain computes
//   x_L = G[i_{L-1}] ... G[i_1] G[i_0] x_0
// as L matrix-vector products (first gate applied first, as evaluate_sequences / tf_matmul_left).  The three output
// modes are the same chain with different start vectors and epilogues:
//   PRODUCT     x_0 = e_c for every column c: M chains per sequence, column c of U_seq
//   STATE       x_0 = psi0, or psi0[p] of the chain's sample (psi0_bstride != 0)
//   POPULATION  x_0 = e_0, output |x_L[0]|^2 (or |x_L[0]| for a superoperator on vec(|0><0|))
// No factor is ever gathered or copied, and no matrix product is formed in the vector modes: a chain reads its gate
// index, then the gate, from the table.  One launch per call whatever the mix of lengths.
//
// Two kernels:
//   seq_lane_kernel<M>  M <= 9: one lane per chain, the state vector in registers, the sample's gate table staged in LDS
//                       once per 64-lane workgroup (all chains of a workgroup belong to one sample); a table larger than
//                       the LDS budget is read from global memory (L2) instead.
//   seq_wave_kernel     M >= 10: one 64-lane workgroup per chain, the state vector double-buffered in LDS, lane r
//                       computing rows r, r + 64, ...; next index prefetched a step ahead; table in LDS (rows padded to
//                       M + 1 against bank conflicts) when it fits beside the vectors, else from L2
//                       (M = 81: one gate is 105 KB, so every superoperator table of a qutrit-pair / D = 9 system streams).
// Every chain checks its length against [0, Lmax] and every index against [0, n_gates) before it reads anything:
// a bad chain sets a flag the entry point reads back and writes NaN, it never reads out of range.
#include "c3p_seq.h"

namespace {

constexpr size_t kSeqLdsBytes = 64 * 1024;

__device__ __forceinline__ cplx seq_nan() { return cmake(__builtin_nan(""), __builtin_nan("")); }

template <int M, bool LDS>
__global__ __launch_bounds__(64) void seq_lane_kernel(SeqArgs a) {
  extern __shared__ cplx tab[];
  const int p = blockIdx.y;
  const cplx* Gp = a.G + (long)p * a.G_bstride;
  if (LDS) {
    const int tsz = a.n_gates * M * M;
    for (int e = threadIdx.x; e < tsz; e += blockDim.x) tab[e] = Gp[e];
    __syncthreads();
  }
  const cplx* T = LDS ? tab : Gp;
  const int C = a.mode == C3P_SEQ_PRODUCT ? M : 1;
  const long item = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (item >= (long)a.S * C) return;
  const int s = (int)(item / C), col = (int)(item % C);
  const cplx* psi = a.mode == C3P_SEQ_STATE ? a.psi0 + (long)p * a.psi0_bstride : nullptr;
  cplx v[M];
#pragma unroll
  for (int i = 0; i < M; ++i) v[i] = a.mode == C3P_SEQ_STATE ? psi[i] : cmake(i == col ? 1.0 : 0.0, 0.0);
  int len = a.lengths[s];
  bool ok = len >= 0 && len <= a.Lmax;
  if (!ok) len = 0;
  const int* row = a.seqs + (long)s * a.Lmax;
  int g = len > 0 ? row[0] : 0;
  for (int t = 0; t < len; ++t) {
    const int gn = t + 1 < len ? row[t + 1] : 0;  // next index in flight while this step computes
    if ((unsigned)g >= (unsigned)a.n_gates) {
      ok = false;
      break;
    }
    const cplx* Gg = T + g * (M * M);
    cplx w[M];
#pragma unroll
    for (int i = 0; i < M; ++i) {
      cplx acc = cmul(Gg[i * M], v[0]);
#pragma unroll
      for (int j = 1; j < M; ++j) cfma(acc, Gg[i * M + j], v[j]);
      w[i] = acc;
    }
#pragma unroll
    for (int i = 0; i < M; ++i) v[i] = w[i];
    g = gn;
  }
  if (!ok) {
    atomicOr(a.bad, 1);
#pragma unroll
    for (int i = 0; i < M; ++i) v[i] = seq_nan();
  }
  const long ps = (long)p * a.S + s;
  if (a.mode == C3P_SEQ_PRODUCT) {
    cplx* o = (cplx*)a.out + ps * (M * M) + col;
#pragma unroll
    for (int i = 0; i < M; ++i) o[i * M] = v[i];
  } else if (a.mode == C3P_SEQ_STATE) {
    cplx* o = (cplx*)a.out + ps * M;
#pragma unroll
    for (int i = 0; i < M; ++i) o[i] = v[i];
  } else {
    const double q = v[0].x * v[0].x + v[0].y * v[0].y;
    ((double*)a.out)[ps] = a.superop ? sqrt(q) : q;
  }
}

// LDS copy of the table: rows padded to M + 1 complex, so that lanes reading rows r, r + 1, ... at the same column hit
// different banks (unpadded, a power-of-two M puts every lane of a group on the same bank: 16-way at M = 16)
__device__ __forceinline__ int seq_wave_ld(int M, bool lds) { return lds ? M + 1 : M; }

template <bool LDS>
__global__ __launch_bounds__(64) void seq_wave_kernel(SeqArgs a) {
  extern __shared__ cplx sm[];
  const int M = a.M;
  const int ld = seq_wave_ld(M, LDS);
  cplx* vb = sm;             // two state vectors [2][M]
  cplx* tab = sm + 2 * M;    // the sample's gate table (LDS variant), [n_gates][M][ld]
  const int lane = threadIdx.x;
  const int p = blockIdx.y;
  const int C = a.mode == C3P_SEQ_PRODUCT ? M : 1;
  const int s = (int)(blockIdx.x / C), col = (int)(blockIdx.x % C);
  const cplx* Gp = a.G + (long)p * a.G_bstride;
  if (LDS) {
    const int tsz = a.n_gates * M * M;
    for (int e = lane; e < tsz; e += 64) {
      const int gr = e / M, c = e - gr * M;  // gr = gate * M + row
      tab[gr * ld + c] = Gp[e];
    }
  }
  const cplx* T = LDS ? tab : Gp;
  const cplx* psi = a.mode == C3P_SEQ_STATE ? a.psi0 + (long)p * a.psi0_bstride : nullptr;
  for (int i = lane; i < M; i += 64) vb[i] = a.mode == C3P_SEQ_STATE ? psi[i] : cmake(i == col ? 1.0 : 0.0, 0.0);
  __syncthreads();
  int len = a.lengths[s];  // the same for the whole workgroup: every branch below is uniform
  bool ok = len >= 0 && len <= a.Lmax;
  if (!ok) len = 0;
  const int* row = a.seqs + (long)s * a.Lmax;
  int g = len > 0 ? __builtin_amdgcn_readfirstlane(row[0]) : 0;
  int t = 0;
  for (; t < len; ++t) {
    // next index in flight while this step computes (t + 1 < len <= Lmax: inside the row)
    const int gn = t + 1 < len ? __builtin_amdgcn_readfirstlane(row[t + 1]) : 0;
    if ((unsigned)g >= (unsigned)a.n_gates) {
      ok = false;
      break;
    }
    const cplx* Gg = T + (long)g * M * ld;
    const cplx* cur = vb + (t & 1) * M;
    cplx* nxt = vb + ((t + 1) & 1) * M;
    for (int r = lane; r < M; r += 64) {
      const cplx* gr = Gg + (long)r * ld;
      cplx acc = cmake(0.0, 0.0);
      for (int j = 0; j < M; ++j) cfma(acc, gr[j], cur[j]);
      nxt[r] = acc;
    }
    __syncthreads();
    g = gn;
  }
  const cplx* fin = vb + (t & 1) * M;
  if (!ok && lane == 0) atomicOr(a.bad, 1);
  const long ps = (long)p * a.S + s;
  if (a.mode == C3P_SEQ_PRODUCT) {
    cplx* o = (cplx*)a.out + ps * M * M + col;
    for (int r = lane; r < M; r += 64) o[(long)r * M] = ok ? fin[r] : seq_nan();
  } else if (a.mode == C3P_SEQ_STATE) {
    cplx* o = (cplx*)a.out + ps * M;
    for (int r = lane; r < M; r += 64) o[r] = ok ? fin[r] : seq_nan();
  } else if (lane == 0) {
    const double q = fin[0].x * fin[0].x + fin[0].y * fin[0].y;
    ((double*)a.out)[ps] = !ok ? __builtin_nan("") : a.superop ? sqrt(q) : q;
  }
}

size_t table_bytes(int n_gates, int M) { return (size_t)n_gates * M * M * sizeof(cplx); }
// LDS bytes of the wave kernel: two state vectors and the table with rows padded to M + 1
size_t wave_lds_bytes(int n_gates, int M) { return 2 * (size_t)M * sizeof(cplx) + (size_t)n_gates * M * (M + 1) * sizeof(cplx); }

template <int M>
void launch_lane(const SeqArgs& a, bool lds, hipStream_t st) {
  const long items = (long)a.S * (a.mode == C3P_SEQ_PRODUCT ? M : 1);
  const dim3 grid((unsigned)((items + 63) / 64), (unsigned)a.P);
  if (lds)
    C3P_LAUNCH((seq_lane_kernel<M, true>), grid, dim3(64), table_bytes(a.n_gates, M), st, a);
  else
    C3P_LAUNCH((seq_lane_kernel<M, false>), grid, dim3(64), 0, st, a);
}

}  // namespace

bool c3p_seq_table_in_lds(int n_gates, int M) {
  return (M <= 9 ? table_bytes(n_gates, M) : wave_lds_bytes(n_gates, M)) <= kSeqLdsBytes;
}

hipError_t c3p_launch_seq(const SeqArgs& a, hipStream_t st) {
  if (a.P == 0 || a.S == 0) return hipSuccess;
  const bool lds = c3p_seq_table_in_lds(a.n_gates, a.M);
  switch (a.M) {
    case 1: launch_lane<1>(a, lds, st); break;
    case 2: launch_lane<2>(a, lds, st); break;
    case 3: launch_lane<3>(a, lds, st); break;
    case 4: launch_lane<4>(a, lds, st); break;
    case 5: launch_lane<5>(a, lds, st); break;
    case 6: launch_lane<6>(a, lds, st); break;
    case 7: launch_lane<7>(a, lds, st); break;
    case 8: launch_lane<8>(a, lds, st); break;
    case 9: launch_lane<9>(a, lds, st); break;
    default: {
      const long chains = (long)a.S * (a.mode == C3P_SEQ_PRODUCT ? a.M : 1);
      const dim3 grid((unsigned)chains, (unsigned)a.P);
      const size_t vec = 2 * (size_t)a.M * sizeof(cplx);
      if (lds)
        C3P_LAUNCH((seq_wave_kernel<true>), grid, dim3(64), wave_lds_bytes(a.n_gates, a.M), st, a);
      else
        C3P_LAUNCH((seq_wave_kernel<false>), grid, dim3(64), vec, st, a);
    }
  }
  return hipGetLastError();
}
