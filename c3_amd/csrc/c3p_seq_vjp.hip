// Reverse sweep of the indexed gate-sequence chain (c3p_seq_chain_vjp).
//
// The forward chain is c3p_seq_chain's, x_{t+1} = G[i_t] x_t.  With d loss = Re sum conj(Xbar) dX the sweep is
//   Gbar[i_t] += xbar_{t+1} x_t^H,     xbar_t = G[i_t]^H xbar_{t+1},
// started from the cotangent of the chain's output (column c of Ubar, the state's cotangent, or 2 pbar x_L[0] e_0 /
// pbar x_L[0] / |x_L[0]| e_0 for a population).  Nothing assumes G unitary: the states x_t are not recovered by G^H but
// recomputed from checkpoints.  The forward pass keeps every C-th state; the backward pass recomputes one segment of C
// states from its checkpoint, then sweeps that segment backward.  Per chain: ceil(L / C) + C stored states, about 3 L
// matrix-vector products (forward, recompute, adjoint) plus L outer products.
//
// Two kernels, the layouts of c3p_seq.hip:
//   seq_vjp_lane_kernel<M>  M <= 9 and n_gates M^2 <= 64: one lane per chain, vectors in registers, table in LDS; every
//                           lane adds its outer products into its own LDS copy of Gbar (entry-major, lanes on adjacent
//                           16-byte words), with no conflicts and no atomics.  The workgroup sums its 64 copies in a fixed
//                           order into its row of the slab.
//   seq_vjp_wave_kernel     otherwise: one 64-lane workgroup per chain, vectors in LDS, lane r owning rows r, r + 64, ...
//                           of the products and entries e, e + 64, ... of the outer product; the workgroup's Gbar in LDS
//                           when it fits (else in its slab row, each entry owned by one lane), the table in LDS when it
//                           fits beside it.
// A workgroup walks several chains one after another (nblk workgroups per sample), so the checkpoint workspace is per
// lane / per workgroup in flight, not per chain.  A second kernel sums the slab over the workgroups (and, for a shared
// table, over the samples) in a fixed order: two identical calls give identical bits.
// The cotangent of the start vector (state mode, psi0_bar) is what the sweep of a chain ends on, xbar_0.  A lane (lane kernel) or
// the owner of a row (wave kernel) adds the xbar_0 of the chains it walks in the order it walks them; the lane kernel then adds
// its 64 lanes in a butterfly of fixed shape; the workgroup's sum goes to its row behind the G_bar rows of the slab, and the same
// reduce launch adds the nblk rows of a sample in order.  No atomics: the same bits on every run.
// Every pass checks the length and each index before it reads through them; a bad chain raises the flag and adds nothing.
#include "c3p_seq_vjp.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr size_t kVjpLdsBytes = 64 * 1024;          // wave kernel: LDS budget per workgroup (as the forward kernel)
constexpr size_t kVjpWsBytes = size_t(512) << 20;   // checkpoint workspace budget
constexpr size_t kVjpSlabBytes = size_t(256) << 20; // partial-Gbar slab budget

__device__ __forceinline__ cplx vjp_nan() { return cmake(__builtin_nan(""), __builtin_nan("")); }

// cotangent of |x0|^2 (2 pbar x0) or, for a superoperator, of |x0| (pbar x0 / |x0|; 0 where x0 = 0)
__device__ __forceinline__ cplx pop_bar(cplx x0, double pb, int superop) {
  if (!superop) return cscale(x0, 2.0 * pb);
  const double r = sqrt(x0.x * x0.x + x0.y * x0.y);
  return r > 0.0 ? cscale(x0, pb / r) : cmake(0.0, 0.0);
}

template <int M>
__global__ __launch_bounds__(64) void seq_vjp_lane_kernel(SeqVjpArgs a) {
  extern __shared__ cplx sm[];
  const SeqArgs& f = a.f;
  constexpr int MM = M * M;
  const int n = f.n_gates, nMM = n * MM;
  cplx* tab = sm;         // [n][M][M]
  cplx* part = sm + nMM;  // [nMM][64]
  const int lane = threadIdx.x, p = blockIdx.y, blk = blockIdx.x;
  const cplx* Gp = f.G + (long)p * f.G_bstride;
  for (int e = lane; e < nMM; e += 64) tab[e] = Gp[e];
  for (int e = 0; e < nMM; ++e) part[e * 64 + lane] = cmake(0.0, 0.0);
  __syncthreads();
  const int Cm = f.mode == C3P_SEQ_PRODUCT ? M : 1;
  const long items = (long)f.S * Cm;
  const long NQ = (long)f.P * a.nblk * 64;
  const long q = ((long)p * a.nblk + blk) * 64 + lane;
  cplx* ck = a.ws + q;                          // ck[(k M + i) NQ]: coalesced over the lanes
  cplx* sg = a.ws + (long)a.nck * M * NQ + q;  // sg[(u M + i) NQ]
  const int C = a.C;
  const cplx* psi = f.mode == C3P_SEQ_STATE ? f.psi0 + (long)p * f.psi0_bstride : nullptr;
  cplx pbar[M];  // this lane's sum of xbar_0 over its chains
#pragma unroll
  for (int i = 0; i < M; ++i) pbar[i] = cmake(0.0, 0.0);
  for (long item = (long)blk * 64 + lane; item < items; item += (long)a.nblk * 64) {
    const int s = (int)(item / Cm), col = (int)(item % Cm);
    cplx v[M];
#pragma unroll
    for (int i = 0; i < M; ++i) v[i] = f.mode == C3P_SEQ_STATE ? psi[i] : cmake(i == col ? 1.0 : 0.0, 0.0);
    int len = f.lengths[s];
    bool ok = len >= 0 && len <= f.Lmax;
    if (!ok) len = 0;
    const int* row = f.seqs + (long)s * f.Lmax;
    // forward, keeping x_0, x_C, ...
    int g = len > 0 ? row[0] : 0;
    for (int t = 0, u = 0, k = 0; t < len; ++t) {
      const int gn = t + 1 < len ? row[t + 1] : 0;
      if ((unsigned)g >= (unsigned)n) {
        ok = false;
        break;
      }
      if (u == 0) {
#pragma unroll
        for (int i = 0; i < M; ++i) ck[((long)k * M + i) * NQ] = v[i];
        ++k;
      }
      if (++u == C) u = 0;
      const cplx* Gg = tab + g * MM;
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
    const long ps = (long)p * f.S + s;
    if (f.out) {
      if (f.mode == C3P_SEQ_PRODUCT) {
        cplx* o = (cplx*)f.out + ps * MM + col;
#pragma unroll
        for (int i = 0; i < M; ++i) o[i * M] = ok ? v[i] : vjp_nan();
      } else if (f.mode == C3P_SEQ_STATE) {
        cplx* o = (cplx*)f.out + ps * M;
#pragma unroll
        for (int i = 0; i < M; ++i) o[i] = ok ? v[i] : vjp_nan();
      } else {
        const double pq = v[0].x * v[0].x + v[0].y * v[0].y;
        ((double*)f.out)[ps] = !ok ? __builtin_nan("") : f.superop ? sqrt(pq) : pq;
      }
    }
    if (!ok) {
      atomicOr(f.bad, 1);
      continue;
    }
    cplx b[M];
    if (f.mode == C3P_SEQ_PRODUCT) {
      const cplx* ob = (const cplx*)a.out_bar + ps * MM + col;
#pragma unroll
      for (int i = 0; i < M; ++i) b[i] = ob[i * M];
    } else if (f.mode == C3P_SEQ_STATE) {
      const cplx* ob = (const cplx*)a.out_bar + ps * M;
#pragma unroll
      for (int i = 0; i < M; ++i) b[i] = ob[i];
    } else {
#pragma unroll
      for (int i = 0; i < M; ++i) b[i] = cmake(0.0, 0.0);
      b[0] = pop_bar(v[0], ((const double*)a.out_bar)[ps], f.superop);
    }
    // backward, one segment [t0, t1) at a time: recompute its states from the checkpoint, then sweep it
    for (int k = (len + C - 1) / C - 1; k >= 0 && ok; --k) {
      const int t0 = k * C, t1 = min(len, t0 + C);
      cplx x[M];
#pragma unroll
      for (int i = 0; i < M; ++i) x[i] = ck[((long)k * M + i) * NQ];
      for (int t = t0; t < t1; ++t) {
#pragma unroll
        for (int i = 0; i < M; ++i) sg[((long)(t - t0) * M + i) * NQ] = x[i];
        if (t + 1 == t1) break;  // the segment's last state is not needed further
        const int gt = row[t];
        if ((unsigned)gt >= (unsigned)n) {
          ok = false;
          break;
        }
        const cplx* Gg = tab + gt * MM;
        cplx w[M];
#pragma unroll
        for (int i = 0; i < M; ++i) {
          cplx acc = cmul(Gg[i * M], x[0]);
#pragma unroll
          for (int j = 1; j < M; ++j) cfma(acc, Gg[i * M + j], x[j]);
          w[i] = acc;
        }
#pragma unroll
        for (int i = 0; i < M; ++i) x[i] = w[i];
      }
      for (int t = t1 - 1; t >= t0 && ok; --t) {
        const int gt = row[t];
        if ((unsigned)gt >= (unsigned)n) {
          ok = false;
          break;
        }
#pragma unroll
        for (int i = 0; i < M; ++i) x[i] = sg[((long)(t - t0) * M + i) * NQ];
        const cplx* Gg = tab + gt * MM;
        cplx* pg = part + (long)gt * MM * 64 + lane;
#pragma unroll
        for (int i = 0; i < M; ++i)
#pragma unroll
          for (int j = 0; j < M; ++j) {
            cplx acc = pg[(i * M + j) * 64];
            cfma(acc, b[i], cconj(x[j]));
            pg[(i * M + j) * 64] = acc;
          }
        cplx w[M];
#pragma unroll
        for (int j = 0; j < M; ++j) {
          cplx acc = cmul(cconj(Gg[j]), b[0]);
#pragma unroll
          for (int i = 1; i < M; ++i) cfma(acc, cconj(Gg[i * M + j]), b[i]);
          w[j] = acc;
        }
#pragma unroll
        for (int j = 0; j < M; ++j) b[j] = w[j];
      }
    }
    if (!ok) {
      atomicOr(f.bad, 1);
      continue;
    }
#pragma unroll
    for (int i = 0; i < M; ++i) pbar[i] = cadd(pbar[i], b[i]);
  }
  __syncthreads();
  if (a.psi0_bar) {  // (uniform) the 64 lanes' sums, a butterfly of fixed shape: every lane ends with the same total
    cplx* po = a.slab + (long)f.P * a.nblk * nMM + ((long)p * a.nblk + blk) * M;
#pragma unroll
    for (int i = 0; i < M; ++i) {
      double re = pbar[i].x, im = pbar[i].y;
      for (int o = 1; o < 64; o <<= 1) {
        re += __shfl_xor(re, o);
        im += __shfl_xor(im, o);
      }
      if (lane == 0) po[i] = cmake(re, im);
    }
  }
  // the workgroup's sum of its 64 copies; entry e starts at lane copy (e mod 64) (spreads the reads over the banks),
  // always the same order for the same entry
  cplx* out = a.slab + ((long)p * a.nblk + blk) * nMM;
  for (int e = lane; e < nMM; e += 64) {
    cplx acc = cmake(0.0, 0.0);
    for (int l = 0; l < 64; ++l) acc = cadd(acc, part[e * 64 + ((l + e) & 63)]);
    out[e] = acc;
  }
}

template <bool TAB_LDS, bool PART_LDS>
__global__ __launch_bounds__(64) void seq_vjp_wave_kernel(SeqVjpArgs a) {
  extern __shared__ cplx sm[];
  const SeqArgs& f = a.f;
  const int M = f.M, MM = M * M, n = f.n_gates;
  const long nMM = (long)n * MM;
  const int ld = TAB_LDS ? M + 1 : M;  // LDS rows padded against bank conflicts, as seq_wave_kernel
  cplx* xb = sm;                              // [2][M] states
  cplx* bb = sm + 2 * M;                      // [2][M] cotangents
  cplx* part = sm + 4 * M;                    // [n][M][M] (PART_LDS)
  cplx* tab = part + (PART_LDS ? nMM : 0);    // [n][M][ld] (TAB_LDS)
  const int lane = threadIdx.x, p = blockIdx.y, blk = blockIdx.x;
  const long q = (long)p * a.nblk + blk;
  cplx* pgall = PART_LDS ? part : a.slab + q * nMM;
  const cplx* Gp = f.G + (long)p * f.G_bstride;
  if (TAB_LDS)
    for (long e = lane; e < nMM; e += 64) {
      const long gr = e / M, c = e - gr * M;  // gr = gate * M + row
      tab[gr * ld + c] = Gp[e];
    }
  for (long e = lane; e < nMM; e += 64) pgall[e] = cmake(0.0, 0.0);
  // the workgroup's partial psi0_bar lives in its slab row; entry r is owned by the lane that computes row r of every product
  cplx* pbar = a.psi0_bar ? a.slab + (long)f.P * a.nblk * nMM + q * M : nullptr;
  if (pbar)
    for (int r = lane; r < M; r += 64) pbar[r] = cmake(0.0, 0.0);
  const cplx* psi = f.mode == C3P_SEQ_STATE ? f.psi0 + (long)p * f.psi0_bstride : nullptr;
  const cplx* T = TAB_LDS ? tab : Gp;
  cplx* ck = a.ws + q * (long)(a.nck + a.C) * M;  // ck[k M + r], then the segment states sg[u M + r]
  cplx* sg = ck + (long)a.nck * M;
  const int C = a.C;
  const int Cm = f.mode == C3P_SEQ_PRODUCT ? M : 1;
  const long items = (long)f.S * Cm;
  __syncthreads();
  // every branch below depends on the chain's length and indices only: uniform over the workgroup
  for (long item = blk; item < items; item += a.nblk) {
    const int s = (int)(item / Cm), col = (int)(item % Cm);
    int len = f.lengths[s];
    bool ok = len >= 0 && len <= f.Lmax;
    if (!ok) len = 0;
    const int* row = f.seqs + (long)s * f.Lmax;
    for (int r = lane; r < M; r += 64) xb[r] = f.mode == C3P_SEQ_STATE ? psi[r] : cmake(r == col ? 1.0 : 0.0, 0.0);
    __syncthreads();
    int t = 0;
    int g = len > 0 ? __builtin_amdgcn_readfirstlane(row[0]) : 0;
    for (int u = 0, k = 0; t < len; ++t) {
      const int gn = t + 1 < len ? __builtin_amdgcn_readfirstlane(row[t + 1]) : 0;
      if ((unsigned)g >= (unsigned)n) {
        ok = false;
        break;
      }
      const cplx* cur = xb + (t & 1) * M;
      cplx* nxt = xb + ((t + 1) & 1) * M;
      if (u == 0) {
        for (int r = lane; r < M; r += 64) ck[(long)k * M + r] = cur[r];
        ++k;
      }
      if (++u == C) u = 0;
      const cplx* Gg = T + (long)g * M * ld;
      for (int r = lane; r < M; r += 64) {
        const cplx* gr = Gg + (long)r * ld;
        cplx acc = cmake(0.0, 0.0);
        for (int j = 0; j < M; ++j) cfma(acc, gr[j], cur[j]);
        nxt[r] = acc;
      }
      __syncthreads();
      g = gn;
    }
    const cplx* fin = xb + (t & 1) * M;
    const long ps = (long)p * f.S + s;
    if (f.out) {
      if (f.mode == C3P_SEQ_PRODUCT) {
        cplx* o = (cplx*)f.out + ps * MM + col;
        for (int r = lane; r < M; r += 64) o[(long)r * M] = ok ? fin[r] : vjp_nan();
      } else if (f.mode == C3P_SEQ_STATE) {
        cplx* o = (cplx*)f.out + ps * M;
        for (int r = lane; r < M; r += 64) o[r] = ok ? fin[r] : vjp_nan();
      } else if (lane == 0) {
        const double pq = fin[0].x * fin[0].x + fin[0].y * fin[0].y;
        ((double*)f.out)[ps] = !ok ? __builtin_nan("") : f.superop ? sqrt(pq) : pq;
      }
    }
    if (ok) {
      cplx* bL = bb + (len & 1) * M;
      if (f.mode == C3P_SEQ_PRODUCT) {
        const cplx* ob = (const cplx*)a.out_bar + ps * MM + col;
        for (int r = lane; r < M; r += 64) bL[r] = ob[(long)r * M];
      } else if (f.mode == C3P_SEQ_STATE) {
        const cplx* ob = (const cplx*)a.out_bar + ps * M;
        for (int r = lane; r < M; r += 64) bL[r] = ob[r];
      } else {
        const double pb = ((const double*)a.out_bar)[ps];
        for (int r = lane; r < M; r += 64) bL[r] = r == 0 ? pop_bar(fin[0], pb, f.superop) : cmake(0.0, 0.0);
      }
    }
    __syncthreads();
    // xbar_t lives in bb[t & 1], x_t in xb[t & 1]; lane r reads back only the states it wrote itself (rows r, r + 64, ...)
    for (int k = (len + C - 1) / C - 1; k >= 0 && ok; --k) {
      const int t0 = k * C, t1 = min(len, t0 + C);
      for (int r = lane; r < M; r += 64) xb[(t0 & 1) * M + r] = ck[(long)k * M + r];
      __syncthreads();
      for (int tt = t0; tt < t1; ++tt) {
        const cplx* cur = xb + (tt & 1) * M;
        for (int r = lane; r < M; r += 64) sg[(long)(tt - t0) * M + r] = cur[r];
        if (tt + 1 == t1) break;
        const int gt = __builtin_amdgcn_readfirstlane(row[tt]);
        if ((unsigned)gt >= (unsigned)n) {
          ok = false;
          break;
        }
        cplx* nxt = xb + ((tt + 1) & 1) * M;
        const cplx* Gg = T + (long)gt * M * ld;
        for (int r = lane; r < M; r += 64) {
          const cplx* gr = Gg + (long)r * ld;
          cplx acc = cmake(0.0, 0.0);
          for (int j = 0; j < M; ++j) cfma(acc, gr[j], cur[j]);
          nxt[r] = acc;
        }
        __syncthreads();
      }
      if (!ok) break;
      for (int r = lane; r < M; r += 64) xb[((t1 - 1) & 1) * M + r] = sg[(long)(t1 - 1 - t0) * M + r];
      __syncthreads();
      for (int tt = t1 - 1; tt >= t0; --tt) {
        const int gt = __builtin_amdgcn_readfirstlane(row[tt]);
        if ((unsigned)gt >= (unsigned)n) {
          ok = false;
          break;
        }
        const cplx* bn = bb + ((tt + 1) & 1) * M;
        cplx* bt = bb + (tt & 1) * M;
        const cplx* xt = xb + (tt & 1) * M;
        const cplx* Gg = T + (long)gt * M * ld;
        cplx* pg = pgall + (long)gt * MM;
        for (int e = lane; e < MM; e += 64) {
          const int i = e / M, j = e - i * M;
          cplx acc = pg[e];
          cfma(acc, bn[i], cconj(xt[j]));
          pg[e] = acc;
        }
        for (int r = lane; r < M; r += 64) {
          cplx acc = cmake(0.0, 0.0);
          for (int i = 0; i < M; ++i) cfma(acc, cconj(Gg[(long)i * ld + r]), bn[i]);
          bt[r] = acc;
        }
        if (tt > t0)
          for (int r = lane; r < M; r += 64) xb[((tt - 1) & 1) * M + r] = sg[(long)(tt - 1 - t0) * M + r];
        __syncthreads();
      }
    }
    if (!ok && lane == 0) atomicOr(f.bad, 1);
    // xbar_0 is in bb[0 .. M), row r written by this lane (the last step of the sweep, or the load of out_bar when len = 0)
    if (ok && pbar)
      for (int r = lane; r < M; r += 64) pbar[r] = cadd(pbar[r], bb[r]);
    __syncthreads();
  }
  if (PART_LDS) {
    cplx* out = a.slab + q * nMM;
    for (long e = lane; e < nMM; e += 64) out[e] = part[e];
  }
}

// Gbar[po] = sum of the slab rows of sample po (all samples for a shared table), in a fixed order; entries nMM .. nMM + M of
// the grid (psi0_bar set): psi0_bar[po] = sum of the nblk partial rows of sample po, always per sample
__global__ __launch_bounds__(256) void seq_vjp_reduce_kernel(const cplx* slab, int P, int nblk, long nMM, int shared, cplx* G_bar, int M,
                                                             cplx* psi0_bar) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int po = blockIdx.y;
  if (e >= nMM) {
    const long r = e - nMM;
    if (!psi0_bar || r >= M) return;
    const cplx* ps = slab + (long)P * nblk * nMM + (long)po * nblk * M;
    cplx acc = cmake(0.0, 0.0);
    for (int b = 0; b < nblk; ++b) acc = cadd(acc, ps[(long)b * M + r]);
    psi0_bar[(long)po * M + r] = acc;
    return;
  }
  if (shared && po > 0) return;  // (the grid spans the samples only for psi0_bar)
  cplx acc = cmake(0.0, 0.0);
  const int p0 = shared ? 0 : po, p1 = shared ? P : po + 1;
  for (int p = p0; p < p1; ++p)
    for (int b = 0; b < nblk; ++b) acc = cadd(acc, slab[((long)p * nblk + b) * nMM + e]);
  G_bar[(long)po * nMM + e] = acc;
}

template <int M>
hipError_t launch_lane(const SeqVjpArgs& a, const SeqVjpPlan& pl, hipStream_t st) {
  if (pl.lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&seq_vjp_lane_kernel<M>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds);
    if (e != hipSuccess) return e;
  }
  C3P_LAUNCH((seq_vjp_lane_kernel<M>), dim3((unsigned)pl.nblk, (unsigned)a.f.P), dim3(64), pl.lds, st, a);
  return hipGetLastError();
}

}  // namespace

SeqVjpPlan c3p_seq_vjp_plan(int n_gates, int M, int P, int S, int Lmax, int mode, bool want_psi0_bar) {
  SeqVjpPlan pl = {};
  const size_t cs = sizeof(cplx);
  const size_t nMM = (size_t)n_gates * M * M;
  pl.C = Lmax > 0 ? (int)std::ceil(std::sqrt((double)Lmax)) : 1;
  pl.nck = std::max(1, (Lmax + pl.C - 1) / pl.C);
  const long items = (long)S * (mode == C3P_SEQ_PRODUCT ? M : 1);
  const size_t per_unit = (size_t)(pl.nck + pl.C) * M * cs;  // one lane's / one workgroup's checkpoints and segment
  pl.lane = M <= 9 && nMM <= 64;
  long want;
  size_t units_per_wg;
  if (pl.lane) {
    want = (items + 63) / 64;
    units_per_wg = 64;
    pl.lds = nMM * cs * 65;  // table + 64 partial copies
  } else {
    // enough workgroups to fill the chip; beyond that a workgroup walks several chains
    want = std::min<long>(items, std::max<long>(1, (8192 + P - 1) / P));
    units_per_wg = 1;
    const size_t vec = 4 * (size_t)M * cs;
    pl.part_lds = vec + nMM * cs <= kVjpLdsBytes;
    pl.tab_lds = pl.part_lds && vec + nMM * cs + (size_t)n_gates * M * (M + 1) * cs <= kVjpLdsBytes;
    pl.lds = vec + (pl.part_lds ? nMM * cs : 0) + (pl.tab_lds ? (size_t)n_gates * M * (M + 1) * cs : 0);
  }
  const long by_ws = (long)std::max<size_t>(1, kVjpWsBytes / ((size_t)P * units_per_wg * per_unit));
  const long by_slab = (long)std::max<size_t>(1, kVjpSlabBytes / std::max<size_t>(1, (size_t)P * nMM * cs));
  pl.nblk = (int)std::max<long>(1, std::min(std::min(want, by_ws), std::min(by_slab, 65535L)));
  pl.ws_elems = (size_t)P * pl.nblk * units_per_wg * (pl.nck + pl.C) * M;
  pl.slab_elems = (size_t)P * pl.nblk * (nMM + (want_psi0_bar ? (size_t)M : 0));
  return pl;
}

hipError_t c3p_launch_seq_vjp(const SeqVjpArgs& a, const SeqVjpPlan& pl, hipStream_t st) {
  const int P = a.f.P;
  const long nMM = (long)a.f.n_gates * a.f.M * a.f.M;
  if (P == 0) return hipSuccess;  // an empty table still runs the chains (checks, forward output); nothing to reduce
  hipError_t e = hipSuccess;
  if (pl.lane) {
    switch (a.f.M) {
      case 1: e = launch_lane<1>(a, pl, st); break;
      case 2: e = launch_lane<2>(a, pl, st); break;
      case 3: e = launch_lane<3>(a, pl, st); break;
      case 4: e = launch_lane<4>(a, pl, st); break;
      case 5: e = launch_lane<5>(a, pl, st); break;
      case 6: e = launch_lane<6>(a, pl, st); break;
      case 7: e = launch_lane<7>(a, pl, st); break;
      case 8: e = launch_lane<8>(a, pl, st); break;
      case 9: e = launch_lane<9>(a, pl, st); break;  // only an empty table: n_gates M^2 > 64 for any gate at M = 9
      default: return hipErrorInvalidValue;
    }
  } else {
    const dim3 grid((unsigned)pl.nblk, (unsigned)P);
    if (pl.tab_lds)
      C3P_LAUNCH((seq_vjp_wave_kernel<true, true>), grid, dim3(64), pl.lds, st, a);
    else if (pl.part_lds)
      C3P_LAUNCH((seq_vjp_wave_kernel<false, true>), grid, dim3(64), pl.lds, st, a);
    else
      C3P_LAUNCH((seq_vjp_wave_kernel<false, false>), grid, dim3(64), pl.lds, st, a);
    e = hipGetLastError();
  }
  const long nred = nMM + (a.psi0_bar ? a.f.M : 0);
  if (e != hipSuccess || nred == 0) return e;
  const dim3 rgrid((unsigned)((nred + 255) / 256), (unsigned)(a.shared && !a.psi0_bar ? 1 : P));
  C3P_LAUNCH(seq_vjp_reduce_kernel, rgrid, dim3(256), 0, st, a.slab, P, pl.nblk, nMM, a.shared, a.G_bar, a.f.M, a.psi0_bar);
  return hipGetLastError();
}
