// Register-resident propagator chains on the f64 matrix cores for matrix dimensions Dm = 16 n + 1
// (49, 65, 81): the 81 x 81 Lindblad superoperator of two qutrits (BASELINE cfg4,
// c3/libraries/propagation.py:551-585) and its D = 7 sibling.
//
// One workgroup of FOUR wavefronts (one per SIMD, 512 registers each) owns a chain.  A complex Dm x Dm matrix
// is split into a CORE of (Dm-1) x (Dm-1) = 16n x 16n elements and a one-element BORDER (last row, last column).
//   * Core matrices live in REGISTERS: wave w owns the 4n columns [4n w, 4n w + 4n) -- n column blocks of 4 --
//     and all 16n rows, as n x n tiles in the C/D layout of v_mfma_f64_4x4x4_4b_f64 (lane (q,b,p) of tile
//     (Ig,jj) holds row 16 Ig + 4 b + q, column 4 (n w + jj) + p), real and imaginary parts in separate registers.
//   * A product C = L R streams the LEFT operand from one LDS image (complex, row stride Dm + 1, 16 x 4 A fragments by
//     ds_read_b128) and takes the RIGHT operand from the registers of the wave that owns those columns: in the four
//     K-steps of a row group of R, MFMA block b multiplies by block (b - s) mod 4 of the tile -- the tile rotated by s
//     4-lane groups with DPP row_ror moves -- and reads its A fragment at the k of that block.  No global or LDS traffic
//     for the right operand, and the result lands in the layout the next product needs.
//   * Complex products use three real products (P = Lr Rr, Q = Li Ri, R = (Lr + Li)(Rr + Ri); Re C = P - Q,
//     Im C = R - P - Q): 3 n^2 MFMAs per K-step and wave instead of 4 n^2, zero padding (the core is a multiple of
//     the tile in every direction).
//   * The border (last row / column / k = Dm - 1): the last column of C is one more B column on a quarter of the K-steps
//     of each wave, the last row uses the tiles of R block by block (partial sums per wave / per MFMA block, summed
//     through LDS), the k = Dm - 1 term is a rank-1 update on the vector unit; border elements of every live matrix stay
//     in small LDS slots, one element per lane.
//   * exp: T18 (Bader-Blanes-Casas, 5 products) + s squarings + 1 chain product per slice.  Five tile sets per slice
//     visit the per-workgroup global arena (X, A2, B2, B3 and the running product U, each written once and read back once
//     by the thread that wrote it): 1.0 MB per slice instead of the 2.5 MB of the arena kernel in c3p_bigd.hip; the
//     polynomial combinations are formed in registers.
//   * The main loop is ROLLED over the row groups of R (its tiles move up one row per pass): a fifth of the code and a
//     register allocation the compiler solves without spilling the right operand; inside a K-step the source order
//     (three MFMAs, one piece of the next step's operand preparation) is pinned with sched_barrier.
#include <cstdio>
#include <utility>

#include "c3p_common.h"
#include "c3p_kernels.h"
#include "c3p_midd.h"
#include "c3p_regd.h"

extern __shared__ __attribute__((aligned(16))) double c3p_rg_lds[];

namespace {

constexpr int RG_WAVES = 4;
constexpr int RG_THREADS = 64 * RG_WAVES;
constexpr int RG_CH = 32;    // control amplitudes staged per chunk of slices
constexpr int RG_KMAX = 16;  // control lines
// border slots in LDS
enum { S_M0 = 0, S_M1, S_M2, S_M3, S_R0, S_R1, S_U0, S_U1, S_NSLOT };
enum { OP_P1 = 0, OP_P2, OP_P3, OP_P4, OP_EX, OP_CH };
// arena tile sets
enum { AR_X = 0, AR_A2, AR_B2, AR_B3, AR_U, AR_NSET };

template <int NRG>
struct RG {
  static constexpr int DM = 16 * NRG + 1;
  static constexpr int NJ = NRG;         // column blocks per wave
  static constexpr int NKS = 4 * NRG;    // K-steps of the core
  static constexpr int NT = NRG * NJ;    // tiles per wave
  static constexpr int LD = DM + 1;      // image row stride (complex elements), = 2 mod 16
  static constexpr int BS = 2 * DM;      // border slot: row DM-1 (DM elements, corner last), column DM-1 (DM elements, corner last)
  static constexpr int DMP = DM + 1;
  static constexpr int IMG_C = DM * LD;
  static constexpr int TSET_C = NT * RG_THREADS;  // complex elements of a tile set: element (tile, thread) at tile * 256 + thread
  static constexpr int TAB_D = 2 * (TSET_C + BS) + 4;  // doubles per generator table: tile set, border slot, {mu_r, mu_i, norm1, 0}
  static constexpr int LDS_C = IMG_C + S_NSLOT * BS + 8 * DMP;
  static constexpr int LDS_D = 2 * LDS_C + RG_KMAX * RG_CH + 2 * RG_WAVES;
};

template <typename F, int... Is>
__device__ __forceinline__ void rg_static_for_impl(F&& f, std::integer_sequence<int, Is...>) {
  (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void rg_static_for(F&& f) {
  rg_static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// The four 4-lane groups of every 16-lane row rotated by S groups (DPP row_ror: lane l takes lane (l - 4 S) mod 16 of its
// row): MFMA block b then holds what block (b - S) mod 4 held.  A VALU move -- it issues in the shadow of the MFMAs,
// where a ds_swizzle broadcast held up the matrix pipe (measured: 20 swizzles per 75 MFMAs cost 3.8 cycles per MFMA).
template <int S>
__device__ __forceinline__ double rg_rot(double v) {
  if constexpr (S == 0) {
    return v;
  } else {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_mov_dpp(lo, 0x120 + 4 * S, 0xf, 0xf, false);
    hi = __builtin_amdgcn_mov_dpp(hi, 0x120 + 4 * S, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
  }
}

// Global accesses are (uniform base in SGPRs, opaque so the address arithmetic is not hoisted out of the slice loop and
// spilled) + (32-bit per-lane byte offset): global_load/store in the saddr form, one offset register for all tiles.
__device__ __forceinline__ int rg_opq(int v) {
  asm volatile("" : "+s"(v));
  return v;
}
template <typename T>
__device__ __forceinline__ T* rg_ubase(T* p) {
  return p + rg_opq(0);
}
// arena traffic is streamed once per slice (written, read back by the same thread, dead): non-temporal, so that it does not
// push the generator tables (shared by every workgroup, re-read every slice) out of the L2
typedef double rg_v2d __attribute__((ext_vector_type(2)));
__device__ __forceinline__ cplx rg_ld_nt(const cplx* ubase, unsigned voff) {
  const rg_v2d v = __builtin_nontemporal_load(reinterpret_cast<const rg_v2d*>(reinterpret_cast<const char*>(ubase) + voff));
  return cmake(v.x, v.y);
}
__device__ __forceinline__ void rg_st_nt(cplx* ubase, unsigned voff, cplx v) {
  rg_v2d w;
  w.x = v.x;
  w.y = v.y;
  __builtin_nontemporal_store(w, reinterpret_cast<rg_v2d*>(reinterpret_cast<char*>(ubase) + voff));
}
__device__ __forceinline__ cplx rg_ld(const cplx* ubase, unsigned voff) {
  return *reinterpret_cast<const cplx*>(reinterpret_cast<const char*>(ubase) + voff);
}
__device__ __forceinline__ void rg_st(cplx* ubase, unsigned voff, cplx v) {
  *reinterpret_cast<cplx*>(reinterpret_cast<char*>(ubase) + voff) = v;
}

// Workgroup barrier that waits for the LDS traffic only (__syncthreads also drains the vector-memory counter, i.e. stalls
// on the outstanding arena stores; those are only ever read back by the thread that wrote them)
__device__ __forceinline__ void rg_bar() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ double rg_rfl(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_readfirstlane(lo);
  hi = __builtin_amdgcn_readfirstlane(hi);
  return __hiloint2double(hi, lo);
}

template <int NRG, bool DUS>
__global__ void __launch_bounds__(RG_THREADS, 1) regd_chain_kernel(MidArgs A, cplx* arena_base, long long* dbg) {
  using G = RG<NRG>;
  constexpr int DM = G::DM, NJ = G::NJ, LD = G::LD, BS = G::BS, DMP = G::DMP;
  constexpr int TSET = G::TSET_C;
  // lane indices are re-derived from an opaque copy of the thread id at the start of every phase (refresh): otherwise
  // the compiler hoists every address / mask that depends on them out of the slice loop and spills them
  const int tid0 = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);
  int tid = tid0, lane = tid & 63;
  int q = lane >> 4, b = (lane >> 2) & 3, p = lane & 3;
  cplx* img = reinterpret_cast<cplx*>(c3p_rg_lds);
  cplx* brd = img + G::IMG_C;
  cplx* cpart = brd + S_NSLOT * BS;
  cplx* rpart = cpart + 4 * DMP;
  double* sg = reinterpret_cast<double*>(rpart + 4 * DMP);
  double* red = sg + RG_KMAX * RG_CH;
  const int col0 = 4 * NJ * wave;  // first column of this wave
  int rowC = 4 * b + q;            // row of a C/D-layout element inside its row group
  int rowA = 4 * b + p;            // row of an A-fragment element inside its row group
  cplx* arena = arena_base + (long)blockIdx.x * AR_NSET * TSET;
  const int K = A.K;
  unsigned voff = (unsigned)tid * (unsigned)sizeof(cplx);  // this thread's byte offset inside a tile (256 complex)
  auto refresh = [&]() {
    int t_ = tid0;
    asm volatile("" : "+v"(t_));
    tid = t_;
    lane = tid & 63;
    q = lane >> 4, b = (lane >> 2) & 3, p = lane & 3;
    rowC = 4 * b + q;
    rowA = 4 * b + p;
    voff = (unsigned)tid * (unsigned)sizeof(cplx);
  };

#ifdef C3P_REGD_TIMING
  long long tacc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  long long tq = 0;
#define RG_TICK(i)                  \
  {                                 \
    const long long tn = clock64(); \
    tacc[i] += tn - tq;             \
    tq = tn;                        \
  }
#else
#define RG_TICK(i)
#endif
  double Rr[NRG][NJ], Ri[NRG][NJ];                // right operand of the next product
  double aP[NRG][NJ], aQ[NRG][NJ], aR[NRG][NJ];   // accumulators; after a product aP = Re C, aR = Im C

  auto mfma = [](double a, double bb, double c) -> double { return __builtin_amdgcn_mfma_f64_4x4x4f64(a, bb, c, 0, 0, 0); };
  auto zero_acc = [&]() {
#pragma unroll
    for (int Ig = 0; Ig < NRG; ++Ig)
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj) aP[Ig][jj] = aQ[Ig][jj] = aR[Ig][jj] = 0.0;
  };
  // a border element (slot index tid) also sits in the image: row DM-1 or column DM-1
  auto border_to_image = [&](cplx v) {
    if (tid < DM) img[(DM - 1) * LD + tid] = v;
    else if (tid < 2 * DM - 1) img[(tid - DM) * LD + DM - 1] = v;
  };

  // C = (init) + L R: L = the LDS image, R = (Rr, Ri) with borders in slot sr; the accumulators carry the initial
  // value (aP = Re, aQ = 0, aR = Re + Im); border of the initial value in slot si (or si < 0); border of C -> slot sd
  // (by finalize, after the workgroup barrier that publishes the border partials).
  // The borders ride on the matrix cores as well: column DM-1 of C is one more B column (the border column of R, read
  // from its LDS slot) on the K-steps with kk mod 4 == wave -- four partial sums, one per wave; row DM-1 of C uses the
  // tiles of R block by block (A operand = row DM-1 of L in the i = 0 row of every block): four partial sums, one per
  // MFMA block.  The k = DM-1 terms are added by finalize / the rank-1 update of the core.
  cplx cornerA = cmake(0.0, 0.0), cornerR = cmake(0.0, 0.0);
  auto product = [&](int sr, int si, int sd) {
    const cplx* rb = brd + sr * BS;
    // new live ranges for the right operand inside the product (whatever the phases around it did to the old ones)
#pragma unroll
    for (int Ig = 0; Ig < NRG; ++Ig)
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj) {
        asm volatile("" : "+v"(Rr[Ig][jj]));
        asm volatile("" : "+v"(Ri[Ig][jj]));
      }
    double cP[NRG], cQ[NRG], cR[NRG];
    double rP[NJ + 1], rQ[NJ + 1], rR[NJ + 1];
#pragma unroll
    for (int Ig = 0; Ig < NRG; ++Ig) cP[Ig] = cQ[Ig] = cR[Ig] = 0.0;
#pragma unroll
    for (int jj = 0; jj <= NJ; ++jj) rP[jj] = rQ[jj] = rR[jj] = 0.0;
    {
      // One pass of this loop = the four K-steps of one row group of R (its tiles are row 0 of (Rr, Ri); the rows move
      // up at the end of the pass) + that row group's share of row DM-1 of C.  A rolled loop: a fifth of the code, and
      // a register allocation problem the compiler solves without spilling the right operand.
      // K-step s of a pass: MFMA block b multiplies by block (b - s) mod 4 of the tile (the tile rotated by s groups), so
      // its A fragment is taken at the k of that block: every block meets every k of the row group in the four steps.
      const cplx* pa = img + rowA * LD;
      const cplx* pr = img + (DM - 1) * LD + rowC;  // row DM-1 of L at this lane's k
      const cplx* pc = rb + DM;                     // column DM-1 of R
      int ko[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) ko[s] = 4 * ((b - s) & 3) + q;
      cplx aC[NRG], aN[NRG];
      double br[NJ], bi[NJ], bs[NJ];  // B operands of the current K-step (prepared during the previous one)
#pragma unroll
      for (int Ig = 0; Ig < NRG; ++Ig) aC[Ig] = pa[16 * Ig * LD + ko[0]];
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj) {
        br[jj] = Rr[0][jj];
        bi[jj] = Ri[0][jj];
        bs[jj] = br[jj] + bi[jj];
      }
      RG_TICK(10)
#pragma unroll 1
      for (int it = 0; it < NRG; ++it) {
        rg_static_for<4>([&](auto s_) {
          constexpr int sx = decltype(s_)::value;
          constexpr int sn = (sx + 1) & 3, rn = (sx == 3) ? 1 : 0;  // next step: rotation, row of (Rr, Ri)
          // Source order = issue order (sched_barrier pins it): three MFMAs, then one piece of the next step's operand
          // preparation -- an A-fragment load, a tile rotation (two DPP moves) or a sum -- so that the preparation issues
          // in the shadow of the matrix pipe instead of stalling it at the top of the step.
          double as[NRG];
          double brN[NJ], biN[NJ], bsN[NJ];
          rg_static_for<NRG>([&](auto Ig_) {
            constexpr int Ig = decltype(Ig_)::value;
            as[Ig] = aC[Ig].x + aC[Ig].y;
            rg_static_for<NJ>([&](auto jj_) {
              constexpr int jj = decltype(jj_)::value;
              constexpr int u = Ig * NJ + jj;  // preparation slot
              aP[Ig][jj] = mfma(aC[Ig].x, br[jj], aP[Ig][jj]);
              aQ[Ig][jj] = mfma(aC[Ig].y, bi[jj], aQ[Ig][jj]);
              aR[Ig][jj] = mfma(as[Ig], bs[jj], aR[Ig][jj]);
              constexpr int OPS = (4 * NRG + NRG * NJ - 1) / (NRG * NJ);  // preparation pieces per slot (4 NRG in all)
              rg_static_for<OPS>([&](auto o_) {
                constexpr int op = u * OPS + decltype(o_)::value;
                if constexpr (op < NRG) {
                  aN[op] = pa[16 * op * LD + (sx == 3 ? 16 : 0) + ko[sn]];  // (the very last prefetch is unused)
                } else if constexpr (op < NRG + 2 * NJ) {
                  constexpr int j2 = (op - NRG) >> 1;
                  if constexpr (((op - NRG) & 1) == 0) brN[j2] = rg_rot<sn>(Rr[rn][j2]);
                  else biN[j2] = rg_rot<sn>(Ri[rn][j2]);
                } else if constexpr (op < NRG + 3 * NJ) {
                  constexpr int j2 = op - NRG - 2 * NJ;
                  bsN[j2] = brN[j2] + biN[j2];
                }
              });
              __builtin_amdgcn_sched_barrier(0);
            });
          });
          if (sx == wave) {  // this wave's share of column DM-1
            const cplx vb = pc[ko[sx]];
            const double cbr = (p == 0) ? vb.x : 0.0, cbi = (p == 0) ? vb.y : 0.0, cbs = cbr + cbi;
#pragma unroll
            for (int Ig = 0; Ig < NRG; ++Ig) {
              cP[Ig] = mfma(aC[Ig].x, cbr, cP[Ig]);
              cQ[Ig] = mfma(aC[Ig].y, cbi, cQ[Ig]);
              cR[Ig] = mfma(as[Ig], cbs, cR[Ig]);
            }
          }
#pragma unroll
          for (int Ig = 0; Ig < NRG; ++Ig) aC[Ig] = aN[Ig];
#pragma unroll
          for (int jj = 0; jj < NJ; ++jj) {
            br[jj] = brN[jj];
            bi[jj] = biN[jj];
            bs[jj] = bsN[jj];
          }
        });
        // row DM-1 (and, on wave 0, the corner): partial sums over the k of each MFMA block
        {
          const cplx va = pr[0];
          const double ar = (p == 0) ? va.x : 0.0, ai = (p == 0) ? va.y : 0.0, as = ar + ai;
#pragma unroll
          for (int jj = 0; jj < NJ; ++jj) {
            rP[jj] = mfma(ar, Rr[0][jj], rP[jj]);
            rQ[jj] = mfma(ai, Ri[0][jj], rQ[jj]);
            rR[jj] = mfma(as, Rr[0][jj] + Ri[0][jj], rR[jj]);
          }
          if (wave == 0) {
            const cplx vb = rb[DM + 16 * it + rowC];
            const double cbr = (p == 0) ? vb.x : 0.0, cbi = (p == 0) ? vb.y : 0.0;
            rP[NJ] = mfma(ar, cbr, rP[NJ]);
            rQ[NJ] = mfma(ai, cbi, rQ[NJ]);
            rR[NJ] = mfma(as, cbr + cbi, rR[NJ]);
          }
        }
#pragma unroll
        for (int Ig = 0; Ig + 1 < NRG; ++Ig)
#pragma unroll
          for (int jj = 0; jj < NJ; ++jj) {
            Rr[Ig][jj] = Rr[Ig + 1][jj];
            Ri[Ig][jj] = Ri[Ig + 1][jj];
          }
        pa += 16;
        pr += 16;
        pc += 16;
      }
    }
    RG_TICK(0)
    if (q == 0) {
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj)
        rpart[b * DMP + col0 + 4 * jj + p] = cmake(rP[jj] - rQ[jj], rR[jj] - rP[jj] - rQ[jj]);
      if (wave == 0 && p == 0) rpart[b * DMP + DM - 1] = cmake(rP[NJ] - rQ[NJ], rR[NJ] - rP[NJ] - rQ[NJ]);
    }
    if (p == 0) {
#pragma unroll
      for (int Ig = 0; Ig < NRG; ++Ig) cpart[wave * DMP + 16 * Ig + rowC] = cmake(cP[Ig] - cQ[Ig], cR[Ig] - cP[Ig] - cQ[Ig]);
    }
    cornerA = img[(DM - 1) * LD + DM - 1];
    cornerR = rb[BS - 1];
#pragma unroll
    for (int Ig = 0; Ig < NRG; ++Ig)
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj) {
        const double t = aP[Ig][jj] + aQ[Ig][jj];
        aP[Ig][jj] = aP[Ig][jj] - aQ[Ig][jj];
        aR[Ig][jj] = aR[Ig][jj] - t;
      }
    // k = DM-1: rank-1 update of the core
    {
      cplx a80[NRG], b80[NJ];
#pragma unroll
      for (int Ig = 0; Ig < NRG; ++Ig) a80[Ig] = img[(16 * Ig + rowC) * LD + DM - 1];
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj) b80[jj] = rb[col0 + 4 * jj + p];
#pragma unroll
      for (int Ig = 0; Ig < NRG; ++Ig)
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
          aP[Ig][jj] = fma(a80[Ig].x, b80[jj].x, fma(-a80[Ig].y, b80[jj].y, aP[Ig][jj]));
          aR[Ig][jj] = fma(a80[Ig].x, b80[jj].y, fma(a80[Ig].y, b80[jj].x, aR[Ig][jj]));
        }
    }
  };
  // after the barrier: the border of the product, one element per lane (own slot entries only; the corners of L and R
  // were read before the barrier, so nothing here races with the image / slot writes of the phase that follows)
  auto finalize = [&](int sr, int si, int sd) {
    if (tid < BS) {
      double vr, vi;
      cplx f;  // the k = DM-1 factor of the other operand
      if (tid < DM || tid == BS - 1) {
        const int j = tid < DM ? tid : DM - 1;
        const cplx v0 = rpart[j], v1 = rpart[DMP + j], v2 = rpart[2 * DMP + j], v3 = rpart[3 * DMP + j];
        vr = (v0.x + v1.x) + (v2.x + v3.x), vi = (v0.y + v1.y) + (v2.y + v3.y);
        f = brd[sr * BS + tid];
        vr = fma(cornerA.x, f.x, fma(-cornerA.y, f.y, vr));
        vi = fma(cornerA.x, f.y, fma(cornerA.y, f.x, vi));
      } else {
        const int i = tid - DM;
        const cplx v0 = cpart[i], v1 = cpart[DMP + i], v2 = cpart[2 * DMP + i], v3 = cpart[3 * DMP + i];
        vr = (v0.x + v1.x) + (v2.x + v3.x), vi = (v0.y + v1.y) + (v2.y + v3.y);
        f = img[i * LD + DM - 1];
        vr = fma(f.x, cornerR.x, fma(-f.y, cornerR.y, vr));
        vi = fma(f.x, cornerR.y, fma(f.y, cornerR.x, vi));
      }
      if (si >= 0) {
        const cplx ini = brd[si * BS + tid];
        vr += ini.x;
        vi += ini.y;
      }
      brd[sd * BS + tid] = cmake(vr, vi);
    }
  };
  auto image_from_C = [&]() {
#pragma unroll
    for (int Ig = 0; Ig < NRG; ++Ig)
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj) img[(16 * Ig + rowC) * LD + col0 + 4 * jj + p] = cmake(aP[Ig][jj], aR[Ig][jj]);
  };
  auto R_from_C = [&]() {
#pragma unroll
    for (int Ig = 0; Ig < NRG; ++Ig)
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj) {
        Rr[Ig][jj] = aP[Ig][jj];
        Ri[Ig][jj] = aR[Ig][jj];
      }
  };
  auto park_C = [&](int set) {
    cplx* dst = rg_ubase(arena + set * TSET);
#pragma unroll
    for (int Ig = 0; Ig < NRG; ++Ig)
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj) rg_st(dst + (Ig * NJ + jj) * RG_THREADS, voff, cmake(aP[Ig][jj], aR[Ig][jj]));
  };
  // all loads of a tile set are issued before the first use (the scheduler otherwise serialises load -> use -> load
  // to save registers: 25 dependent memory round trips)
  auto load_set = [&](const cplx* base, cplx (&v)[NRG][NJ]) {
    const cplx* src = rg_ubase(base);
#pragma unroll
    for (int Ig = 0; Ig < NRG; ++Ig)
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj) v[Ig][jj] = rg_ld(src + (Ig * NJ + jj) * RG_THREADS, voff);
    __builtin_amdgcn_sched_barrier(0);
  };
  auto unpark_R = [&](int set) {
    cplx v[NRG][NJ];
    load_set(arena + set * TSET, v);
#pragma unroll
    for (int Ig = 0; Ig < NRG; ++Ig)
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj) {
        Rr[Ig][jj] = v[Ig][jj].x;
        Ri[Ig][jj] = v[Ig][jj].y;
      }
  };
  auto park_R = [&](int set) {
    cplx* dst = rg_ubase(arena + set * TSET);
#pragma unroll
    for (int Ig = 0; Ig < NRG; ++Ig)
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj) rg_st(dst + (Ig * NJ + jj) * RG_THREADS, voff, cmake(Rr[Ig][jj], Ri[Ig][jj]));
  };
  // dst[row][col] = f * C, row-major complex DR x DR (f = e^{trace shift}); borders from slot.  DR = A.Dm <= DM is the TRUE
  // dimension: a matrix smaller than the kernel's class runs zero padded (exp of diag(X, 0) = diag(exp X, 1): the padding
  // stays decoupled through every product) and only its DR x DR block is written.
  const int DR = A.Dm;
  auto store_out = [&](cplx* dst_, int slot, double fr, double fi) {
    cplx* dst = rg_ubase(dst_);
#pragma unroll
    for (int Ig = 0; Ig < NRG; ++Ig)
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj) {
        const int row = 16 * Ig + rowC, col = col0 + 4 * jj + p;
        if (row < DR && col < DR)
          dst[(long)row * DR + col] = cmake(fma(fr, aP[Ig][jj], -fi * aR[Ig][jj]), fma(fr, aR[Ig][jj], fi * aP[Ig][jj]));
      }
    if (tid < BS - 1) {
      const cplx v = brd[slot * BS + tid];
      const int row = tid < DM ? DM - 1 : tid - DM, col = tid < DM ? tid : DM - 1;
      if (row < DR && col < DR) dst[(long)row * DR + col] = cmake(fma(fr, v.x, -fi * v.y), fma(fr, v.y, fi * v.x));
    }
  };

  const long nchains = (long)A.B * A.S;
  for (long chain = blockIdx.x; chain < nchains; chain += gridDim.x) {
    const int sample = (int)(chain / A.S);
    // Lindblad chains of Hermitian Hamiltonians run in real arithmetic in the Hermitian basis (c3p_regr.hip)
    if (A.hb_tabflag && c3p_hb_sample_is_real(A.hb_tabflag, A.tab_per_sample ? sample : 0, K)) continue;
    const int seg = (int)(chain - (long)sample * A.S);
    const int n0 = (int)(((long)seg * A.N) / A.S);
    const int n1 = (int)(((long)(seg + 1) * A.N) / A.S);
    const int len = n1 - n0;
    const double* tabs = A.tables + (long)(A.tab_per_sample ? sample : 0) * (1 + K) * G::TAB_D;
    auto meta = [&](int k1) -> const double* { return tabs + (long)k1 * G::TAB_D + 2 * (TSET + BS); };
    __syncthreads();  // the previous chain is done with the LDS
    // plan: squarings from ||G0||_1 + sum_k max_t |c_k(t)| ||G_k||_1 over the segment
    double nrm = meta(0)[2];
    for (int k = 0; k < K; ++k) {
      const double* s = A.signals + ((long)sample * K + k) * A.N + n0;
      double cmax = 0.0;
      for (int t = tid; t < len; t += RG_THREADS) cmax = fmax(cmax, fabs(s[t]));
      for (int o = 32; o >= 1; o >>= 1) cmax = fmax(cmax, __shfl_xor(cmax, o));
      if (lane == 0) red[wave] = cmax;
      __syncthreads();
      cmax = 0.0;
      for (int w = 0; w < RG_WAVES; ++w) cmax = fmax(cmax, red[w]);
      __syncthreads();
      nrm = fma(cmax, meta(k + 1)[2], nrm);
    }
    nrm = rg_rfl(nrm);
    const int ps = __builtin_amdgcn_readfirstlane(c3p_squarings(nrm, C3P_T18_THETA));
    const double scale = ldexp(1.0, -ps);

    double mu_r = 0.0, mu_i = 0.0, mus_r = 0.0, mus_i = 0.0;
    auto stage_signals = [&](int t) {  // slices [t, t + RG_CH) of the segment
      for (int e = tid; e < K * RG_CH; e += RG_THREADS) {
        const int k = e / RG_CH, tt = e - k * RG_CH;
        sg[e] = (t + tt < len) ? A.signals[((long)sample * K + k) * A.N + n0 + t + tt] : 0.0;
      }
    };
    // tiles of X = 2^-s (G0 + sum_k c_k G_k) for slice tt of the staged chunk (tables: L2 resident, shared by all workgroups)
    auto assemble_tiles = [&](int tt, double (&xr)[NRG][NJ], double (&xi)[NRG][NJ]) {
      auto table = [&](int k1) -> const cplx* { return reinterpret_cast<const cplx*>(tabs + (long)k1 * G::TAB_D); };
      auto accumulate = [&](const cplx (&v)[NRG][NJ], int k1) {
        const double w = k1 ? scale * sg[(k1 - 1) * RG_CH + tt] : scale;
#pragma unroll
        for (int Ig = 0; Ig < NRG; ++Ig)
#pragma unroll
          for (int jj = 0; jj < NJ; ++jj) {
            xr[Ig][jj] = k1 ? fma(w, v[Ig][jj].x, xr[Ig][jj]) : w * v[Ig][jj].x;
            xi[Ig][jj] = k1 ? fma(w, v[Ig][jj].y, xi[Ig][jj]) : w * v[Ig][jj].y;
          }
      };
      for (int k1 = 0; k1 <= K; ++k1) {
        cplx v[NRG][NJ];
        load_set(table(k1), v);
        accumulate(v, k1);
      }
    };
    // X: tiles -> (Rr, Ri), borders -> slot M0, everything -> image; trace shift of the slice -> (mu_r, mu_i)
    auto assemble = [&](int tt) {
      const cplx* T0 = reinterpret_cast<const cplx*>(tabs);
      mu_r = meta(0)[0];
      mu_i = meta(0)[1];
      cplx bv = cmake(0.0, 0.0);
      if (tid < BS) {
        bv = T0[TSET + tid];
        bv.x *= scale;
        bv.y *= scale;
      }
      for (int k = 0; k < K; ++k) {
        const cplx* Tk = reinterpret_cast<const cplx*>(tabs + (long)(k + 1) * G::TAB_D);
        const double c = sg[k * RG_CH + tt];
        const double w = scale * c;
        mu_r = fma(c, meta(k + 1)[0], mu_r);
        mu_i = fma(c, meta(k + 1)[1], mu_i);
        if (tid < BS) {
          const cplx v = Tk[TSET + tid];
          bv.x = fma(w, v.x, bv.x);
          bv.y = fma(w, v.y, bv.y);
        }
      }
      if (tid < BS) {
        brd[S_M0 * BS + tid] = bv;
        border_to_image(bv);
      }
      assemble_tiles(tt, Rr, Ri);
#pragma unroll
      for (int Ig = 0; Ig < NRG; ++Ig)
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) img[(16 * Ig + rowC) * LD + col0 + 4 * jj + p] = cmake(Rr[Ig][jj], Ri[Ig][jj]);
      park_R(AR_X);
    };

    int t = 0;
    bool first = true;
    int ucur = S_U0;
    stage_signals(0);
    __syncthreads();
    assemble(0);
    zero_acc();
    int op = OP_P1, sr = S_M0, si = -1, sd = S_M1, sq_left = 0;
    __syncthreads();
#ifdef C3P_REGD_TIMING
    tq = clock64();
#endif
    for (;;) {
      refresh();
      product(sr, si, sd);
      RG_TICK(1)
      rg_bar();  // A: everyone is done with the image; border partials are visible
      RG_TICK(2)
      refresh();
      finalize(sr, si, sd);
      const int op_in = op;
      bool next_slice = false;
      if (op == OP_P1) {  // C = A2: parked, and the right operand of the next product (the image still holds X)
        park_C(AR_A2);
        R_from_C();
        zero_acc();
        op = OP_P2, sr = S_M1, si = -1, sd = S_M2;
      } else if (op == OP_P2) {  // C = A3 = X A2: A3 becomes both operands
        image_from_C();
        if (tid < BS) border_to_image(brd[S_M2 * BS + tid]);
        R_from_C();
        zero_acc();
        op = OP_P3, sr = S_M2, si = -1, sd = S_M3;
      } else if (op == OP_P3) {  // C = A6: the T18 combinations of X, A2 (arena), A3 (image), A6 (C)
        {
          cplx* dst = rg_ubase(arena + AR_B2 * TSET);
          cplx* dst3 = rg_ubase(arena + AR_B3 * TSET);
          cplx a2[NRG][NJ], xx[NRG][NJ];
          load_set(arena + AR_X * TSET, xx);
          load_set(arena + AR_A2 * TSET, a2);
#pragma unroll
          for (int Ig = 0; Ig < NRG; ++Ig)
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj) {
              const double dg = (16 * Ig + rowC == col0 + 4 * jj + p) ? 1.0 : 0.0;
              const double xr = xx[Ig][jj].x, xi = xx[Ig][jj].y, a2r = a2[Ig][jj].x, a2i = a2[Ig][jj].y;
              const cplx a3 = img[(16 * Ig + rowC) * LD + col0 + 4 * jj + p];  // the left operand of A6 = A3 A3
              const double a3r = a3.x, a3i = a3.y, a6r = aP[Ig][jj], a6i = aR[Ig][jj];
              // B1 -> image (left operand of A9 = B1 B5 + B4)
              img[(16 * Ig + rowC) * LD + col0 + 4 * jj + p] =
                  cmake(fma(C3P_T18_A31, a3r, fma(C3P_T18_A21, a2r, C3P_T18_A11 * xr)),
                        fma(C3P_T18_A31, a3i, fma(C3P_T18_A21, a2i, C3P_T18_A11 * xi)));
              // B2 -> arena
              rg_st(dst + (Ig * NJ + jj) * RG_THREADS, voff,
                    cmake(fma(C3P_T18_B61, a6r, fma(C3P_T18_B31, a3r, fma(C3P_T18_B21, a2r, C3P_T18_B11 * xr))),
                          fma(C3P_T18_B61, a6i, fma(C3P_T18_B31, a3i, fma(C3P_T18_B21, a2i, C3P_T18_B11 * xi)))));
              // B3 -> arena
              rg_st(dst3 + (Ig * NJ + jj) * RG_THREADS, voff,
                    cmake(fma(C3P_T18_B62, a6r, fma(C3P_T18_B32, a3r, fma(C3P_T18_B22, a2r, fma(C3P_T18_B12, xr, C3P_T18_B02 * dg)))),
                          fma(C3P_T18_B62, a6i, fma(C3P_T18_B32, a3i, fma(C3P_T18_B22, a2i, C3P_T18_B12 * xi)))));
              // B5 -> right operand
              Rr[Ig][jj] = fma(C3P_T18_B64, a6r, fma(C3P_T18_B34, a3r, C3P_T18_B24 * a2r));
              Ri[Ig][jj] = fma(C3P_T18_B64, a6i, fma(C3P_T18_B34, a3i, C3P_T18_B24 * a2i));
              // B4 -> initial value of the accumulators
              const double b4r = fma(C3P_T18_B63, a6r, fma(C3P_T18_B33, a3r, fma(C3P_T18_B23, a2r, fma(C3P_T18_B13, xr, C3P_T18_B03 * dg))));
              const double b4i = fma(C3P_T18_B63, a6i, fma(C3P_T18_B33, a3i, fma(C3P_T18_B23, a2i, C3P_T18_B13 * xi)));
              aP[Ig][jj] = b4r;
              aQ[Ig][jj] = 0.0;
              aR[Ig][jj] = b4r + b4i;
            }
        }
        if (tid < BS) {
          const double dg = (tid == DM - 1 || tid == BS - 1) ? 1.0 : 0.0;
          const cplx x = brd[S_M0 * BS + tid], a2 = brd[S_M1 * BS + tid], a3 = brd[S_M2 * BS + tid], a6 = brd[S_M3 * BS + tid];
          border_to_image(cmake(fma(C3P_T18_A31, a3.x, fma(C3P_T18_A21, a2.x, C3P_T18_A11 * x.x)),
                                fma(C3P_T18_A31, a3.y, fma(C3P_T18_A21, a2.y, C3P_T18_A11 * x.y))));
          brd[S_M3 * BS + tid] = cmake(fma(C3P_T18_B61, a6.x, fma(C3P_T18_B31, a3.x, fma(C3P_T18_B21, a2.x, C3P_T18_B11 * x.x))),
                                       fma(C3P_T18_B61, a6.y, fma(C3P_T18_B31, a3.y, fma(C3P_T18_B21, a2.y, C3P_T18_B11 * x.y))));
          brd[S_M0 * BS + tid] = cmake(fma(C3P_T18_B62, a6.x, fma(C3P_T18_B32, a3.x, fma(C3P_T18_B22, a2.x, fma(C3P_T18_B12, x.x, C3P_T18_B02 * dg)))),
                                       fma(C3P_T18_B62, a6.y, fma(C3P_T18_B32, a3.y, fma(C3P_T18_B22, a2.y, C3P_T18_B12 * x.y))));
          brd[S_M1 * BS + tid] = cmake(fma(C3P_T18_B64, a6.x, fma(C3P_T18_B34, a3.x, C3P_T18_B24 * a2.x)),
                                       fma(C3P_T18_B64, a6.y, fma(C3P_T18_B34, a3.y, C3P_T18_B24 * a2.y)));
          brd[S_M2 * BS + tid] = cmake(fma(C3P_T18_B63, a6.x, fma(C3P_T18_B33, a3.x, fma(C3P_T18_B23, a2.x, fma(C3P_T18_B13, x.x, C3P_T18_B03 * dg)))),
                                       fma(C3P_T18_B63, a6.y, fma(C3P_T18_B33, a3.y, fma(C3P_T18_B23, a2.y, C3P_T18_B13 * x.y))));
        }
        op = OP_P4, sr = S_M1, si = S_M2, sd = S_R0;
      } else if (op == OP_P4) {  // C = A9: left operand B3 + A9, right operand A9, initial value B2
        {
          cplx v3[NRG][NJ], v2[NRG][NJ];
          load_set(arena + AR_B3 * TSET, v3);
          load_set(arena + AR_B2 * TSET, v2);
#pragma unroll
          for (int Ig = 0; Ig < NRG; ++Ig)
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj)
              img[(16 * Ig + rowC) * LD + col0 + 4 * jj + p] = cmake(v3[Ig][jj].x + aP[Ig][jj], v3[Ig][jj].y + aR[Ig][jj]);
          if (tid < BS) {
            const cplx b3 = brd[S_M0 * BS + tid], a9 = brd[S_R0 * BS + tid];
            border_to_image(cmake(b3.x + a9.x, b3.y + a9.y));
          }
          R_from_C();
#pragma unroll
          for (int Ig = 0; Ig < NRG; ++Ig)
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj) {
              aP[Ig][jj] = v2[Ig][jj].x;
              aQ[Ig][jj] = 0.0;
              aR[Ig][jj] = v2[Ig][jj].x + v2[Ig][jj].y;
            }
        }
        op = OP_EX, sr = S_R0, si = S_M3, sd = S_R1, sq_left = ps;
      } else if (op == OP_EX) {  // C = T18 or one of its squarings
        if (sq_left > 0) {
          image_from_C();
          if (tid < BS) border_to_image(brd[sd * BS + tid]);
          R_from_C();
          zero_acc();
          sr = sd, sd = sd ^ 1, si = -1;
          --sq_left;
        } else {  // C = exp(X - mu)
          if constexpr (DUS) {
            double sn, cs;
            sincos(mu_i, &sn, &cs);
            const double er = exp(mu_r);
            store_out(A.dUs_out + ((long)sample * A.N + n0 + t) * DR * DR, sd, er * cs, er * sn);
          }
          if (first) {
            park_C(AR_U);
            if (tid < BS) brd[S_U0 * BS + tid] = brd[sd * BS + tid];
            ucur = S_U0;
            first = false;
            mus_r = mu_r;
            mus_i = c3p_phase_add(0.0, mu_i);
            next_slice = true;
          } else {  // U <- C U
            image_from_C();
            if (tid < BS) border_to_image(brd[sd * BS + tid]);
            unpark_R(AR_U);
            zero_acc();
            mus_r += mu_r;
            mus_i = c3p_phase_add(mus_i, mu_i);
            op = OP_CH, sr = ucur, si = -1, sd = ucur ^ 1;
          }
        }
      } else {  // OP_CH: C = the running product
        park_C(AR_U);
        ucur ^= 1;
        next_slice = true;
      }
      if (next_slice) {
        ++t;
        if (t == len) break;
        if ((t % RG_CH) == 0) {
          stage_signals(t);
          __syncthreads();
        }
        assemble(t % RG_CH);
        zero_acc();
        op = OP_P1, sr = S_M0, si = -1, sd = S_M1;
      }
      RG_TICK(4 + op_in)
      rg_bar();  // B: image and border slots of this phase are visible
      RG_TICK(3)
    }
#ifdef C3P_REGD_TIMING
    if (blockIdx.x == 0 && tid == 0 && dbg)
      for (int i = 0; i < 12; ++i) dbg[i] = tacc[i];
#endif
    // segment product (the frame-rotation row phases are a separate epilogue)
    double sn, cs;
    sincos(mus_i, &sn, &cs);
    const double er = exp(mus_r);
    store_out(A.seg_out + chain * DR * DR, ucur, er * cs, er * sn);
  }
}

// Generator tables in the kernel's layout: G = -i dt (h - mu) (unitary) or the Lindblad generator pieces
// L0 = dt (clp - i (H0 (x) I - I (x) H0^T)), Lk = -i dt (Hk (x) I - I (x) Hk^T) (propagation.py:565-582), trace shifted.
__global__ void __launch_bounds__(256) regd_prep_kernel(RegdPrepArgs P) {
  __shared__ double redr[256], redi[256];
  __shared__ double mu[2];
  const int tid = threadIdx.x;
  const int ti = blockIdx.x % (1 + P.K);
  const int sample = blockIdx.x / (1 + P.K);
  const int D = P.Dm, Dh = P.Dh;  // true dimension; the tables are laid out for the class dimension DP >= D, zero padded
  const int DP = c3p_regd_class(D);
  const int NRG = (DP - 1) / 16, NJ = NRG;
  const cplx* h = (ti == 0) ? P.h0 + (long)sample * P.h0_bstride : P.hks + (long)sample * P.hks_bstride + (long)(ti - 1) * Dh * Dh;
  auto gelem = [&](int row, int col) -> cplx {
    cplx v;
    if (!P.lindblad) {
      const cplx x = h[row * D + col];
      v = cmake(x.y * P.dt, -x.x * P.dt);
    } else {
      const int i = row / Dh, j = row - i * Dh, k = col / Dh, l = col - k * Dh;
      v = (ti == 0) ? P.clp[(long)sample * P.clp_bstride + (long)row * D + col] : cmake(0, 0);
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
      v = cscale(v, P.dt);
    }
    return v;
  };
  double tr = 0, tim = 0;
  for (int i = tid; i < D; i += 256) {
    const cplx v = gelem(i, i);
    tr += v.x;
    tim += v.y;
  }
  redr[tid] = tr;
  redi[tid] = tim;
  __syncthreads();
  if (tid == 0) {
    double a = 0, bq = 0;
    for (int i = 0; i < 256; ++i) {
      a += redr[i];
      bq += redi[i];
    }
    mu[0] = 0.0;  // imaginary shift only: a real one overflows the shifted product of long, strongly damped segments (c3p_smalld.hip: build_tables)
    mu[1] = bq / D;
  }
  __syncthreads();
  double cs = 0;
  for (int j = tid; j < D; j += 256) {
    double s = 0;
    for (int i = 0; i < D; ++i) {
      cplx v = gelem(i, j);
      if (i == j) {
        v.x -= mu[0];
        v.y -= mu[1];
      }
      s += hypot(v.x, v.y);
    }
    cs = fmax(cs, s);
  }
  __syncthreads();
  redr[tid] = cs;
  __syncthreads();
  const int TSET = NRG * NJ * 256, BS = 2 * DP;
  const long TAB_D = 2L * (TSET + BS) + 4;
  double* out = P.tables + ((long)sample * (1 + P.K) + ti) * TAB_D;
  for (int e = tid; e < TSET + BS; e += 256) {
    int row, col;
    if (e < TSET) {
      const int tile = e >> 8, t = e & 255;
      const int w = t >> 6, l = t & 63;
      const int Ig = tile / NJ, jj = tile - Ig * NJ;
      row = 16 * Ig + 4 * ((l >> 2) & 3) + (l >> 4);
      col = 4 * NJ * w + 4 * jj + (l & 3);
    } else {
      const int eb = e - TSET;
      row = eb < DP ? DP - 1 : eb - DP;
      col = eb < DP ? eb : DP - 1;
    }
    cplx g = cmake(0.0, 0.0);
    if (row < D && col < D) {
      g = gelem(row, col);
      if (row == col) {
        g.x -= mu[0];
        g.y -= mu[1];
      }
    }
    out[2 * e] = g.x;
    out[2 * e + 1] = g.y;
  }
  if (tid == 0) {
    double nrm = 0;
    for (int i = 0; i < 256; ++i) nrm = fmax(nrm, redr[i]);
    double* m = out + 2L * (TSET + BS);
    m[0] = mu[0];
    m[1] = mu[1];
    m[2] = nrm;
    m[3] = 0.0;
  }
}

template <int NRG>
hipError_t launch_r(const MidArgs& A, void* arena, hipStream_t st) {
  const size_t lds = (size_t)RG<NRG>::LDS_D * sizeof(double);
  const long nchains = (long)A.B * A.S;
  const unsigned grid = (unsigned)(nchains < C3P_REGD_MAX_WGS ? nchains : C3P_REGD_MAX_WGS);
  auto go = [&](auto kern) -> hipError_t {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    long long* dbg = nullptr;
#ifdef C3P_REGD_TIMING
    static long long* dbg_dev = nullptr;
    if (!dbg_dev) (void)hipMalloc(&dbg_dev, 12 * sizeof(long long));
    dbg = dbg_dev;
#endif
    C3P_LAUNCH(kern, dim3(grid), dim3(RG_THREADS), lds, st, A, reinterpret_cast<cplx*>(arena), dbg);
#ifdef C3P_REGD_TIMING
    {
      long long h[12];
      (void)hipStreamSynchronize(st);
      (void)hipMemcpy(h, dbg, sizeof h, hipMemcpyDeviceToHost);
      fprintf(stderr, "[regd timing, cycles of wave 0 / block 0, last chain] mfma %lld  borders %lld  barA %lld  barB %lld | post P1 %lld P2 %lld P3 %lld P4 %lld EX %lld CH %lld | product entry %lld\n",
              h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], h[9], h[10]);
    }
#endif
    return hipGetLastError();
  };
  if (A.dUs_out) return go(regd_chain_kernel<NRG, true>);
  return go(regd_chain_kernel<NRG, false>);
}

}  // namespace

// Dm = 49, 65, 81 exactly, or a smaller dimension zero padded into the next class where that beats the arena kernel
// (tests/checks/check_regd_pad.py, B = 256, N = 200: 41..48 -> 49 1.29 - 1.39x, 56..64 -> 65 1.04 - 1.40x (64 = the Lindblad
// superoperators of D = 8), 70..80 -> 81 1.04 - 1.29x; 50..55 and 66..69 are a wash, 0.98 - 1.02x, and stay on the arena
// kernel).  C3P_REGD_PAD=0 switches the padding off, C3P_REGD_PAD=all pads everything in 41..81.
bool c3p_regd_supported(int Dm) {
  if (Dm == 49 || Dm == 65 || Dm == 81) return true;
  const long e = c3p_opt(C3P_OPT_regd_pad);
  if (e == 0) return false;
  if (e == 2) return Dm >= 41 && Dm <= 81;
  return (Dm >= 41 && Dm <= 48) || (Dm >= 56 && Dm <= 64) || (Dm >= 70 && Dm <= 80);
}

size_t c3p_regd_table_doubles(int Dm, int K) {
  if (!c3p_regd_supported(Dm)) return 0;
  const int DP = c3p_regd_class(Dm);
  const int n = (DP - 1) / 16;
  return (size_t)(1 + K) * (2 * ((size_t)n * n * 256 + 2 * DP) + 4);
}

size_t c3p_regd_arena_bytes(int Dm) {
  if (!c3p_regd_supported(Dm)) return 0;
  const int n = (c3p_regd_class(Dm) - 1) / 16;
  return (size_t)C3P_REGD_MAX_WGS * AR_NSET * n * n * 256 * sizeof(cplx);
}

hipError_t c3p_launch_regd_prep(const RegdPrepArgs& P, int nsamp, hipStream_t st) {
  if (!c3p_regd_supported(P.Dm)) return hipErrorInvalidValue;
  C3P_LAUNCH(regd_prep_kernel, dim3((unsigned)(nsamp * (1 + P.K))), dim3(256), 0, st, P);
  return hipGetLastError();
}

hipError_t c3p_launch_regd_chain(const MidArgs& A, void* arena, hipStream_t st) {
  if (A.K > RG_KMAX) return hipErrorInvalidValue;
  switch (c3p_regd_class(A.Dm)) {
    case 49: return launch_r<3>(A, arena, st);
    case 65: return launch_r<4>(A, arena, st);
    case 81: return launch_r<5>(A, arena, st);
    default: return hipErrorInvalidValue;
  }
}
