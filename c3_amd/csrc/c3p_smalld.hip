// Small-D propagator chains on the f64 matrix cores (D <= 12: cfg1 D=3, cfg2 D=9, the
// 9x9 Lindblad superoperator of a qutrit, ...).
//
// Mapping (gfx950): v_mfma_f64_4x4x4_4b_f64 performs FOUR independent 4x4x4 real
// products per instruction at the full fp64 rate (16 cycles; measured 72.8 TFLOP/s,
// tools/ubench_f64.hip).  Block b of the instruction is given to chain b: one
// wavefront owns four independent (sample, time-segment) chains, 16 lanes each, and
// every matrix of a chain lives in registers as 4x4 real blocks.
//
// Complex arithmetic is carried by the real 2x2 representation z=a+ib -> [[a,-b],[b,a]]:
//   R(A) (2D x 2D) times the "half" image Bh = first column of each 2x2 (2D x D)
//   gives Ch = half image of C = A B.  No flop is redundant.
//   * D-layout (MFMA C/D and B operand): register zh[I][J], lane (r=l/16, c=l%4) holds
//       Zh[4I+r][4J+c] = (r even ? Re : Im) Z[2I + r/2][4J + c]
//   * A-layout (MFMA A operand): register ra[I][K], lane (r,c) holds R(A)[4I+c][4K+r].
//     Obtained from the D-layout through a per-chain LDS image (15 ds_write_b64 +
//     25 ds_read_b64 + sign xor for D=9); row stride 4*NJ+1 doubles keeps both the
//     16-lane writes and the 32-lane reads bank-conflict free.
//
// Per slice (reference: propagation.py:426-440 + tf_utils.py:144-193):
//   X = G0 + sum_k c_k(n) G_k           (tables prepared by smalld_prep: G = -i dt (h - tr/D))
//   E = exp(X): Taylor, Paterson-Stockmeyer with q=4 (powers X..X^4, Horner in X^4),
//       degree 4r in {4,8,12,16,20} and s squarings chosen from a 1-norm bound, wave-uniform
//   U <- E U ;  the scalar factors e^{mu_n} are summed and applied once per segment.
#include <type_traits>

#include <cstdlib>
#include "c3p_common.h"
#include "c3p_kernels.h"
#include "c3p_smalld.h"

// Built as two translation units (__graft_entry__.build: -DC3P_SMALLD_PART=1 | 2): everything but the real-Hamiltonian
// backward sweep, and that sweep alone -- it is compiled with -mllvm -amdgpu-mfma-vgpr-form (see smalld_grad_real_kernel).
// Without the macro everything lands in one unit.
#ifdef C3P_SMALLD_PART
#define C3P_SMALLD_HAS(p) (C3P_SMALLD_PART == (p))
#else
#define C3P_SMALLD_HAS(p) 1
#endif

extern __shared__ __attribute__((aligned(16))) double c3p_sd_lds[];

namespace {

template <int D>
struct SD {
  static constexpr int NBI = (D + 1) / 2;  // 4-row blocks of the 2D-row half image
  static constexpr int NJ = (D + 3) / 4;   // 4-column blocks
  static constexpr int W = 4 * NJ + 1;     // LDS row stride in doubles
  static constexpr int MAT = 4 * NBI * W;  // doubles per matrix image
  // per-chain image buffer of the forward kernel: one complex half image.  IMG = 12 (mod 32) doubles keeps the
  // LDS patterns bank-conflict free under the gfx950 rules (ds_read_b64: 32-lane groups on 64 dword banks;
  // ds_write_b64: 16-lane groups on 32): image writes b IMG + r W + c, A-fragment reads b IMG + rho W.
  static constexpr int IMG = ((MAT - 12 + 31) / 32) * 32 + 12;
};

__device__ __forceinline__ double mfma4(double a, double b, double c) {
  return __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ double readfirstlane_f64(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_readfirstlane(lo);
  hi = __builtin_amdgcn_readfirstlane(hi);
  return __hiloint2double(hi, lo);
}

// LDS read that the backend may not pair into ds_read2_b64: a wave64 ds_read_b64 costs 2 LDS cycles
// (256 B/clk), a ds_read2_b64 8 for two (128 B/clk), and the image strides are laid out for the bank
// rule of the single form (32-lane groups, 64 dword banks).  With eight waves per CU the LDS pipe, not
// the matrix cores, was the busiest unit of the real fast path before this.
typedef __attribute__((address_space(3))) const volatile double c3p_lds_cvd;
__device__ __forceinline__ double lds_ld(const double* p) { return *(c3p_lds_cvd*)p; }

__device__ __forceinline__ double flip_sign(double v, unsigned mask_hi) {
  unsigned long long u = __double_as_longlong(v);
  u ^= ((unsigned long long)mask_hi) << 32;
  return __longlong_as_double(u);
}

// Wave-level ordering point for the per-chain LDS images.  The workgroup is a single
// wavefront and the LDS services one wave's instructions in issue order, so no s_barrier
// is needed; the fence only stops the compiler from reordering image writes and reads.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// D-layout registers -> the chain's LDS image (plain half image Zh, row stride W)
template <int D>
__device__ __forceinline__ void write_image(const double (&zh)[SD<D>::NBI][SD<D>::NJ], double* img, int woff) {
  using C = SD<D>;
  wave_sync();
#pragma unroll
  for (int I = 0; I < C::NBI; ++I)
#pragma unroll
    for (int J = 0; J < C::NJ; ++J) img[woff + I * 4 * C::W + J * 4] = zh[I][J];
  wave_sync();
}

// acc += M * B, where the left operand M is read from its LDS image as A-layout fragments
// (one K-column of 4x4 blocks at a time: NBI ds_read_b64 + sign xor per 4*NBI*NJ... MFMAs)
template <int D>
__device__ __forceinline__ void mm_img(const double* img, int roff, unsigned negmask,
                                       const double (&zb)[SD<D>::NBI][SD<D>::NJ],
                                       double (&acc)[SD<D>::NBI][SD<D>::NJ]) {
  using C = SD<D>;
  // software pipelined: the A fragments of step K+1 are in flight while step K's MFMAs issue
  double ra[2][C::NBI];
#pragma unroll
  for (int I = 0; I < C::NBI; ++I) ra[0][I] = flip_sign(lds_ld(img + roff + I * 4 * C::W), negmask);
#pragma unroll
  for (int K = 0; K < C::NBI; ++K) {
    if (K + 1 < C::NBI) {
#pragma unroll
      for (int I = 0; I < C::NBI; ++I) ra[(K + 1) & 1][I] = flip_sign(lds_ld(img + roff + I * 4 * C::W + (K + 1) * 2), negmask);
    }
#pragma unroll
    for (int I = 0; I < C::NBI; ++I)
#pragma unroll
      for (int J = 0; J < C::NJ; ++J) acc[I][J] = mfma4(ra[K & 1][I], zb[K][J], acc[I][J]);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ---- one half-image product dealt over the blocks of the instruction (the fold of the fused tail) ----
// mm_img gives block b of every MFMA to chain b.  Where fewer than four chains have a product to form -- the fold of a wave's four
// segments: two products, then one -- the NBI x NJ output tiles of a product are dealt over the nb = 2 or 4 blocks that would
// otherwise multiply slots nobody reads: ceil(NBI NJ / nb) x NBI instructions per product instead of NBI NJ x NBI (D = 9: 40 and
// 20 instead of 75).  An output tile is still NBI instructions in K order from a zero accumulator on the same operands; the blocks
// of an instruction are independent, so every element has the bits mm_img gives it.
struct SDTile {
  int I, J;
  bool on;  // false: the block idles in this task (it repeats tile (0, 0) and does not write it)
};

template <int D>
constexpr int sd_split_tasks(int nb) {
  return (SD<D>::NBI * SD<D>::NJ + nb - 1) / nb;
}

// The deal (block, task) -> (I, J).  A block stays on one column J where it can, so that its lanes read one column of right-operand
// tiles: every column is cut into runs of `per` rows, one run per block, and the rows left over at the bottom of the columns are
// pooled, column by column, on the blocks behind.  D = 9, nb = 4: columns 0, 1, 2 with rows 0 .. 3 on blocks 0, 1, 2 and row 4 of
// the three columns on block 3; nb = 2: column 0 and rows 0 .. 2 of column 1 | rows 3, 4 of column 1 and column 2.
// Banks of the A-fragment reads (ds_read_b64, 32-lane groups on 64 dword banks, see SD<D>::IMG): a lane reads row 4 I + rho of its
// image, stride W doubles with W odd, and an image has at most 24 rows -- blocks that read ONE image (nb = 4) at different I touch
// different rows and so different banks, at the same I they read the same address: no conflict for any deal.  Two pairs that read
// two images 2 IMG = 24 (mod 32) doubles apart (nb = 2) meet in a bank only where their rows differ by 8, that is I by exactly 2:
// a two-way conflict in some tasks (D = 9: three of eight), which no deal of 15 tiles over two blocks avoids in all tasks and
// which costs one LDS cycle against the 16 of the instruction it feeds.
template <int D>
constexpr SDTile sd_split_deal(int nb, int blk, int task) {
  constexpr int NBI = SD<D>::NBI, NJ = SD<D>::NJ;
  const int per = sd_split_tasks<D>(nb);
  const int full = NBI / per, rem = NBI % per;  // whole runs per column, rows left over per column
  if (blk < NJ * full) return SDTile{(blk % full) * per + task, blk / full, true};
  const int idx = (blk - NJ * full) * per + task;
  if (rem == 0 || idx >= NJ * rem) return SDTile{0, 0, false};
  return SDTile{full * per + idx % rem, idx / rem, true};
}

// every output tile exactly once
template <int D>
constexpr bool sd_split_deal_ok(int nb) {
  constexpr int NBI = SD<D>::NBI, NJ = SD<D>::NJ;
  int seen[NBI][NJ] = {};
  for (int blk = 0; blk < nb; ++blk)
    for (int t = 0; t < sd_split_tasks<D>(nb); ++t) {
      const SDTile s = sd_split_deal<D>(nb, blk, t);
      if (s.I < 0 || s.I >= NBI || s.J < 0 || s.J >= NJ) return false;
      if (s.on) ++seen[s.I][s.J];
    }
  for (int I = 0; I < NBI; ++I)
    for (int J = 0; J < NJ; ++J)
      if (seen[I][J] != 1) return false;
  return true;
}
#define C3P_SD_DEAL_OK(D) static_assert(sd_split_deal_ok<D>(2) && sd_split_deal_ok<D>(4), "split product: every output tile exactly once")
C3P_SD_DEAL_OK(2); C3P_SD_DEAL_OK(3); C3P_SD_DEAL_OK(4); C3P_SD_DEAL_OK(5); C3P_SD_DEAL_OK(6); C3P_SD_DEAL_OK(7);
C3P_SD_DEAL_OK(8); C3P_SD_DEAL_OK(9); C3P_SD_DEAL_OK(10); C3P_SD_DEAL_OK(11); C3P_SD_DEAL_OK(12);
#undef C3P_SD_DEAL_OK
static_assert(sd_split_deal<9>(4, 2, 3).I == 3 && sd_split_deal<9>(4, 2, 3).J == 2 && sd_split_deal<9>(4, 3, 1).I == 4 &&
                  sd_split_deal<9>(4, 3, 1).J == 1 && !sd_split_deal<9>(4, 3, 3).on,
              "D = 9 over four blocks: a column each on blocks 0 .. 2, the last row on block 3");

// The lane's tile (I, J) of task t (blk: the lane's block within its product, 0 .. NB - 1)
template <int D, int NB>
__device__ __forceinline__ void split_tiles(int blk, int (&tI)[sd_split_tasks<D>(NB)], int (&tJ)[sd_split_tasks<D>(NB)],
                                            bool (&on)[sd_split_tasks<D>(NB)]) {
#pragma unroll
  for (int t = 0; t < sd_split_tasks<D>(NB); ++t) {
    int I = sd_split_deal<D>(NB, 0, t).I, J = sd_split_deal<D>(NB, 0, t).J;
    bool o = sd_split_deal<D>(NB, 0, t).on;
#pragma unroll
    for (int q = 1; q < NB; ++q) {
      I = blk == q ? sd_split_deal<D>(NB, q, t).I : I;
      J = blk == q ? sd_split_deal<D>(NB, q, t).J : J;
      o = blk == q ? sd_split_deal<D>(NB, q, t).on : o;
    }
    tI[t] = I;
    tJ[t] = J;
    on[t] = o;
  }
}

// Epilogue of mm_split: called once with the block's finished tiles acc[t] = tile (tI[t], tJ[t]) of the product, in D-layout (the
// Re / Im partner of an element is lane ^ 16 of the same register), between the K loop and the write-back.  WRITE: the tiles go to
// the image afterwards (false: the epilogue has taken them where they belong and the image keeps the right operand).
struct SplitPlain {
  static constexpr bool WRITE = true;
  template <int NT>
  __device__ __forceinline__ void operator()(double (&)[NT], const int (&)[NT], const int (&)[NT], const bool (&)[NT]) const {}
};

// C = A B with the output tiles dealt over NB blocks.  `a`: the left operand's image plus the lane's A-fragment offset (roff of
// mm_img less the chain's image base); `bc`: the right operand's image plus the lane's D-layout offset r W + c.  The product is
// written over the right operand's image, after all reads (two wave_syncs), unless the epilogue takes it elsewhere.  K is the
// outer loop, as in mm_img: the instructions of a step are independent of one another and the A and B reads of step K + 1 are
// in flight under them.
template <int D, int NB, class Epi = SplitPlain>
__device__ __forceinline__ void mm_split(const double* a, double* bc, unsigned negmask, int blk, const Epi& epi = Epi{}) {
  using C = SD<D>;
  constexpr int NT = sd_split_tasks<D>(NB);
  int tI[NT], tJ[NT], aoff[NT], coff[NT], joff[NT];  // A fragments start at I 4 W, the tile itself (right operand, output) at I 4 W + J 4
  bool on[NT];
  split_tiles<D, NB>(blk, tI, tJ, on);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    aoff[t] = tI[t] * 4 * C::W;
    joff[t] = tJ[t] * 4;
    coff[t] = aoff[t] + joff[t];
  }
  double ra[2][NT], rb[2][NT], acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    ra[0][t] = flip_sign(lds_ld(a + aoff[t]), negmask);
    rb[0][t] = lds_ld(bc + joff[t]);
    acc[t] = 0.0;
  }
#pragma unroll
  for (int K = 0; K < C::NBI; ++K) {
    if (K + 1 < C::NBI) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        ra[(K + 1) & 1][t] = flip_sign(lds_ld(a + aoff[t] + (K + 1) * 2), negmask);
        rb[(K + 1) & 1][t] = lds_ld(bc + (K + 1) * 4 * C::W + joff[t]);
      }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = mfma4(ra[K & 1][t], rb[K & 1][t], acc[t]);
    __builtin_amdgcn_sched_barrier(0);
  }
  epi(acc, tI, tJ, on);
  if constexpr (Epi::WRITE) {
    wave_sync();
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (on[t]) bc[coff[t]] = acc[t];
    wave_sync();
  }
}

struct LanePos {
  int r, b, c;
  int idx16;  // position among the chain's 16 lanes
};

// out = c1 X + c2 A2 + c3 A3 (+ c0 on the diagonal)
template <int D>
__device__ __forceinline__ void poly_block(double (&out)[SD<D>::NBI][SD<D>::NJ], double c0, double c1,
                                           double c2, double c3, const double (&X)[SD<D>::NBI][SD<D>::NJ],
                                           const double (&A2)[SD<D>::NBI][SD<D>::NJ],
                                           const double (&A3)[SD<D>::NBI][SD<D>::NJ], int ddelta,
                                           int rhalf) {
  using C = SD<D>;
#pragma unroll
  for (int I = 0; I < C::NBI; ++I)
#pragma unroll
    for (int J = 0; J < C::NJ; ++J) {
      double v = c1 * X[I][J];
      v = fma(c2, A2[I][J], v);
      v = fma(c3, A3[I][J], v);
      // diagonal: row 2I + r/2 (real part, r even) == column 4J + c, inside the D x D matrix
      if (2 * I - 4 * J >= -1 && 2 * I - 4 * J <= 3) {
        const bool on = (ddelta == 4 * J - 2 * I) && (2 * I + rhalf < D);
        v += on ? c0 : 0.0;
      }
      out[I][J] = v;
    }
}

// out = cx X + c2 A2 + c3 A3 + c6 A6 (+ c0 on the diagonal) (+ add)
template <int D>
__device__ __forceinline__ void lincomb6(double (&out)[SD<D>::NBI][SD<D>::NJ], double c0, double cx, double c2,
                                         double c3, double c6, const double (&X)[SD<D>::NBI][SD<D>::NJ],
                                         const double (&A2)[SD<D>::NBI][SD<D>::NJ],
                                         const double (&A3)[SD<D>::NBI][SD<D>::NJ],
                                         const double (&A6)[SD<D>::NBI][SD<D>::NJ], int ddelta, int rhalf) {
  using C = SD<D>;
#pragma unroll
  for (int I = 0; I < C::NBI; ++I)
#pragma unroll
    for (int J = 0; J < C::NJ; ++J) {
      double v = cx * X[I][J];
      v = fma(c2, A2[I][J], v);
      v = fma(c3, A3[I][J], v);
      if (c6 != 0.0) v = fma(c6, A6[I][J], v);
      if (c0 != 0.0 && 2 * I - 4 * J >= -1 && 2 * I - 4 * J <= 3) {
        const bool on = (ddelta == 4 * J - 2 * I) && (2 * I + rhalf < D);
        v += on ? c0 : 0.0;
      }
      out[I][J] = v;
    }
}

// ---------------------------------------------------------------------------------------------
// Real-Hamiltonian fast path.  When h0 and every hk are real (lab-frame transmon models in the dressed
// basis are: model.py:453-534 dresses with the real eigenvectors of a real symmetric matrix),
// X = -i Y with Y = dt (H - tr H / D) real symmetric and
//     exp(X) = cos Y - i sin Y,   cos Y = p_c(W),  sin Y = Y p_s(W),  W = Y^2,
// with p_c, p_s the Chebyshev-economised polynomials of c3p_common.h (degree 8 in W, radius C3P_MM8_THETA = 1.85; the core +
// border form takes the degree-6 pair below C3P_MM6_THETA).  Everything up to the chain product is REAL
// D x D arithmetic: 7 real products (27 MFMAs each at D = 9) instead of 5 complex ones (75 each).
// Real matrices live in registers as NB x NB tiles of 4x4 (lane (r,c) of the chain's block holds
// M[4I+r][4J+c]); the left operand is read from a row-major LDS image (A layout: M[4I+c][4K+r]).
// ---------------------------------------------------------------------------------------------
template <int D>
struct RD {
  static constexpr int NB = (D + 3) / 4;
};

// Every matrix of the real path is a polynomial in the real SYMMETRIC Y, hence symmetric: products only
// compute the tiles on and above the diagonal (6 of 9 at D = 9) and sym_fill mirrors them.
// lane (r, c) of tile (I, J) holds M[4I + r][4J + c]; its mirror element M[4J + c][4I + r] is held by lane
// (c, r) of tile (J, I): one in-chain lane swap per lower tile (ds_bpermute).
// Only the tile rows a product reads as operands need their lower tiles: operand tiles are za[K][.] / zb[K][.] with
// K < KM, and with the rank-1 tail (D = 1 mod 4) the last row of tiles is never an operand -- at D = 9 ONE lower tile,
// (1,0), instead of three.  FULL mirrors everything (matrices that leave the symmetric stage: dU output, U <- E).
template <int D>
struct SymTail;
template <int D, bool FULL = false>
__device__ __forceinline__ void sym_fill(double (&m)[RD<D>::NB][RD<D>::NB], int swap_lane);

// The left operand of every real product is SYMMETRIC, and for a symmetric M the A-layout fragment of tile
// (I, K) -- lane (r, c) <- M[4I + c][4K + r] -- equals M[4K + r][4I + c], the D-layout register of tile (K, I)
// the same lane already holds: the real stage needs NO LDS image, no fragment loads, no round trips.
//   acc[I][J] += sum_K A(I,K) B(K,J) = sum_K mfma(Areg[K][I], Breg[K][J])     (tiles J >= I, mirrored afterwards)
// broadcast of the quad's lane 0 (column c = 0 of a tile) to its four lanes: DPP quad_perm [0,0,0,0], no LDS
__device__ __forceinline__ double quad_bcast0(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_mov_dpp(lo, 0x00, 0xf, 0xf, true);
  hi = __builtin_amdgcn_mov_dpp(hi, 0x00, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}

// When D = 1 (mod 4) the last K-step of a product carries ONE valid k (k = D-1; D = 9: a third of the MFMAs doing
// a quarter of their work).  It is applied as a rank-1 update on the vector unit instead:
//   acc(I,J) += a_I (x) b_J,   a_I[lane (r,c)] = A[4I+r][D-1]   (tile (I,NB-1), column 0, quad broadcast)
//                              b_J[lane (r,c)] = B[D-1][4J+c] = B[4J+c][D-1]   (tile (J,NB-1) of the lane (c,0))
// Both vectors come from tiles on or above the diagonal, i.e. they do not wait for the mirror.
template <int D>
struct SymTail {
  static constexpr bool ON = (D % 4 == 1) && (RD<D>::NB > 1);
  static constexpr int KM = ON ? RD<D>::NB - 1 : RD<D>::NB;
};

// first tile column of row I among the tiles kept for a symmetric matrix (operand rows in full, else upper tiles)
template <int D>
__device__ __forceinline__ constexpr int sym_j0(int I) {
  return I >= SymTail<D>::KM ? I : 0;
}
template <int D, bool FULL>
__device__ __forceinline__ void sym_fill(double (&m)[RD<D>::NB][RD<D>::NB], int swap_lane) {
  constexpr int NB = RD<D>::NB;
  constexpr int ROWS = FULL ? NB : SymTail<D>::KM;
#pragma unroll
  for (int I = 1; I < ROWS; ++I)
#pragma unroll
    for (int J = 0; J < I; ++J) m[I][J] = __shfl(m[J][I], swap_lane);
}
// the lower tiles sym_fill<D, false> left out
template <int D>
__device__ __forceinline__ void sym_fill_rest(double (&m)[RD<D>::NB][RD<D>::NB], int swap_lane) {
  constexpr int NB = RD<D>::NB;
#pragma unroll
  for (int I = SymTail<D>::KM; I < NB; ++I)
#pragma unroll
    for (int J = 0; J < I; ++J) m[I][J] = __shfl(m[J][I], swap_lane);
}

template <int D>
__device__ __forceinline__ void mm_sym(const double (&za)[RD<D>::NB][RD<D>::NB], const double (&zb)[RD<D>::NB][RD<D>::NB],
                                       double (&acc)[RD<D>::NB][RD<D>::NB], int tail_lane) {
  constexpr int NB = RD<D>::NB;
#pragma unroll
  for (int K = 0; K < SymTail<D>::KM; ++K)
#pragma unroll
    for (int I = 0; I < NB; ++I)
#pragma unroll
      for (int J = I; J < NB; ++J) acc[I][J] = mfma4(za[K][I], zb[K][J], acc[I][J]);
  if constexpr (SymTail<D>::ON) {
    double av[NB], bv[NB];
#pragma unroll
    for (int I = 0; I < NB; ++I) {
      av[I] = quad_bcast0(za[I][NB - 1]);
      bv[I] = __shfl(zb[I][NB - 1], tail_lane);
    }
#pragma unroll
    for (int I = 0; I < NB; ++I)
#pragma unroll
      for (int J = I; J < NB; ++J) acc[I][J] = fma(av[I], bv[J], acc[I][J]);
  }
}
template <int D>
__device__ __forceinline__ void mm_sym2(const double (&za)[RD<D>::NB][RD<D>::NB], const double (&zb1)[RD<D>::NB][RD<D>::NB],
                                        double (&acc1)[RD<D>::NB][RD<D>::NB], const double (&zb2)[RD<D>::NB][RD<D>::NB],
                                        double (&acc2)[RD<D>::NB][RD<D>::NB], int tail_lane) {
  constexpr int NB = RD<D>::NB;
#pragma unroll
  for (int K = 0; K < SymTail<D>::KM; ++K)
#pragma unroll
    for (int I = 0; I < NB; ++I)
#pragma unroll
      for (int J = I; J < NB; ++J) {
        acc1[I][J] = mfma4(za[K][I], zb1[K][J], acc1[I][J]);
        acc2[I][J] = mfma4(za[K][I], zb2[K][J], acc2[I][J]);
      }
  if constexpr (SymTail<D>::ON) {
    double av[NB], bv1[NB], bv2[NB];
#pragma unroll
    for (int I = 0; I < NB; ++I) {
      av[I] = quad_bcast0(za[I][NB - 1]);
      bv1[I] = __shfl(zb1[I][NB - 1], tail_lane);
      bv2[I] = __shfl(zb2[I][NB - 1], tail_lane);
    }
#pragma unroll
    for (int I = 0; I < NB; ++I)
#pragma unroll
      for (int J = I; J < NB; ++J) {
        acc1[I][J] = fma(av[I], bv1[J], acc1[I][J]);
        acc2[I][J] = fma(av[I], bv2[J], acc2[I][J]);
      }
  }
}

// acc += A B for a SYMMETRIC left operand A (A fragments = registers, as in mm_sym) and a general right operand
// B (all tiles): the chain product of the real path, E U with E = C - iS split into real blocks.
// The single-k tail takes the row D-1 of B from the lanes r = 0 (broadcast over r by one lane swap).
template <int D>
__device__ __forceinline__ void mm_symA(const double (&za)[RD<D>::NB][RD<D>::NB], const double (&zb)[RD<D>::NB][RD<D>::NB],
                                        double (&acc)[RD<D>::NB][RD<D>::NB], int row0_lane, double asign) {
  constexpr int NB = RD<D>::NB;
#pragma unroll
  for (int K = 0; K < SymTail<D>::KM; ++K)
#pragma unroll
    for (int I = 0; I < NB; ++I)
#pragma unroll
      for (int J = 0; J < NB; ++J) acc[I][J] = mfma4(za[K][I], zb[K][J], acc[I][J]);
  if constexpr (SymTail<D>::ON) {
    double av[NB], bv[NB];
#pragma unroll
    for (int I = 0; I < NB; ++I) {
      av[I] = asign * quad_bcast0(za[I][NB - 1]);
      bv[I] = __shfl(zb[NB - 1][I], row0_lane);
    }
#pragma unroll
    for (int I = 0; I < NB; ++I)
#pragma unroll
      for (int J = 0; J < NB; ++J) acc[I][J] = fma(av[I], bv[J], acc[I][J]);
  }
}

// acc (ALL tiles) += A B for symmetric A and B (operand tiles filled): the full product whose mirror gives
// A B + B A (backward sweep).  The single-k tail takes column D-1 of both from their last tile column.
template <int D>
__device__ __forceinline__ void mm_symfull(const double (&za)[RD<D>::NB][RD<D>::NB], const double (&zb)[RD<D>::NB][RD<D>::NB],
                                           double (&acc)[RD<D>::NB][RD<D>::NB], int tail_lane) {
  constexpr int NB = RD<D>::NB;
#pragma unroll
  for (int K = 0; K < SymTail<D>::KM; ++K)
#pragma unroll
    for (int I = 0; I < NB; ++I)
#pragma unroll
      for (int J = 0; J < NB; ++J) acc[I][J] = mfma4(za[K][I], zb[K][J], acc[I][J]);
  if constexpr (SymTail<D>::ON) {
    double av[NB], bv[NB];
#pragma unroll
    for (int I = 0; I < NB; ++I) {
      av[I] = quad_bcast0(za[I][NB - 1]);
      bv[I] = __shfl(zb[I][NB - 1], tail_lane);
    }
#pragma unroll
    for (int I = 0; I < NB; ++I)
#pragma unroll
      for (int J = 0; J < NB; ++J) acc[I][J] = fma(av[I], bv[J], acc[I][J]);
  }
}

// out = c0 I + c1 W + c2 W2 (+ c3 W3); UPPER: tiles J >= I only (accumulators of a symmetric product, mirrored
// afterwards); otherwise the tiles a product reads as operands (rows I < KM in full, upper tiles of the other rows)
template <int D, bool WITH3, bool UPPER = false>
__device__ __forceinline__ void rcomb(double (&out)[RD<D>::NB][RD<D>::NB], double c0, double c1, double c2, double c3,
                                      const double (&W1)[RD<D>::NB][RD<D>::NB], const double (&W2)[RD<D>::NB][RD<D>::NB],
                                      const double (&W3)[RD<D>::NB][RD<D>::NB], const LanePos& lp) {
  constexpr int NB = RD<D>::NB;
#pragma unroll
  for (int I = 0; I < NB; ++I)
#pragma unroll
    for (int J = (UPPER || I >= SymTail<D>::KM) ? I : 0; J < NB; ++J) {
      double v = c1 * W1[I][J];
      v = fma(c2, W2[I][J], v);
      if constexpr (WITH3) v = fma(c3, W3[I][J], v);
      if (I == J) v += (lp.r == lp.c && 4 * I + lp.r < D) ? c0 : 0.0;
      out[I][J] = v;
    }
}


// ---------------------------------------------------------------------------------------------
// "Core + border" form of the real path for D = 4 NC + 1 (D = 9: the 8 + 1 split).  A 9 x 9 matrix in
// 12 x 12 tiles spends 6 of the 12 MFMAs of a symmetric product (10 of the 18 of a chain product) on the tiles of its last
// row and column, which carry 4, 4 and 1 of 16 elements.  Here the (D-1) x (D-1) core tiles exactly (NC x NC tiles, no padding
// at all) and the last row / column / corner are carried separately, per chain, in the lanes of its MFMA block:
//   symmetric matrix (SMat): core tiles (upper, lower mirrored for operands), the border column twice -- vr[I] = M[4I+r][D-1]
//     (replicated over c) and vc[J] = M[4J+c][D-1] (replicated over r) --, the corner s (all 16 lanes);
//   general matrix (GMat, the chain state): core and row border rc[J] = M[D-1][4J+c] of the real and of the imaginary part; the column
//     border and the corner of the complex state as ONE packed register each (GBorder).
// Border of a product: column = core x vector on the vector unit (one FMA per tile and lane + a quad reduction by DPP),
// its c form by one lane swap; corner = dot product (quad reduction); the ROW border of a chain product is a vector-matrix
// product whose sum runs over the r lanes (16 apart: no DPP reach) -- it stayed on the matrix cores as ONE A tile per K-step
// whose only row is the border (4 MFMAs instead of the 10 of the padded tiles).  (Since then every border sum is a reduction over r
// by a matrix instruction against a tile of ones: mm_s8 and chain_step8 below.)  Measured in isolation
// (tools/ubench_sym9.hip, profiles/r04/ubench_sym9.txt): a dependent symmetric product 284 ns against 315 ns per wave at two
// waves per SIMD.
// ---------------------------------------------------------------------------------------------
template <int NC>
struct SMat {
  double m[NC][NC];
  double vr[NC], vc[NC];
  double s;
};
template <int NC>
struct GMat {
  double m[NC][NC];
  double rc[NC];
};
// Column border and corner of the chain state U = Ur + i Ui, PACKED: Re and Im dealt over the quad index c of the lane, one register
// holding {Re, Im, -Re, -Im} in the lanes c = 0 .. 3 (chain_step8 below)
template <int NC>
struct GBorder {
  double Pc[NC];  // lane (r, c): {Ur, Ui, -Ur, -Ui}[4K+r][D-1] for c = 0 .. 3
  double Ps;      // lane (r, c): {Ur, Ui, -Ur, -Ui}[D-1][D-1], replicated over r
};
// the packed value of a lane from the real and imaginary parts it holds
__device__ __forceinline__ double border_pack(double re, double im, int c) {
  const double v = (c & 1) ? im : re;
  return (c & 2) ? -v : v;
}
// quad rotation, lane c reads lane (c + 1) mod 4 of its quad: {Re, Im, -Re, -Im} -> {Im, -Re, -Im, Re}, -i times the packed vector.
// DPP quad_perm [1,2,3,0], no sign flips and no LDS
__device__ __forceinline__ double quad_rot1(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_mov_dpp(lo, 0x39, 0xf, 0xf, true);
  hi = __builtin_amdgcn_mov_dpp(hi, 0x39, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}

template <int NC>
__device__ __forceinline__ void s8_zero(SMat<NC>& a) {
#pragma unroll
  for (int I = 0; I < NC; ++I) {
#pragma unroll
    for (int J = 0; J < NC; ++J) a.m[I][J] = 0.0;
    a.vr[I] = a.vc[I] = 0.0;
  }
  a.s = 0.0;
}

// Border sums on the matrix cores.  On gfx950 a wave's vector instructions and the fp64 matrix instructions of its
// SIMD do not overlap (tools/ubench_coissue.hip: 8 MFMAs + 32 v_mov_dpp take the SUM of their issue times), a quad reduction of a
// double costs four v_mov_b32_dpp + two v_add_f64 = ~29 cycles, one v_mfma_f64_4x4x4_4b 16.7 -- and the instruction contracts over
// the lane's r index for free.  So the partial products of a border are formed with the sum index ON r (for a symmetric left
// operand: its transposed tile, the register the lane holds anyway, times the r form of the vector) and reduced by ONE matrix
// instruction against a tile of ones: A = partials, B = 1 -> D[i][j] = sum_r t(r, c = i), i.e. the r form of the result in every lane,
// with the rest of the border update (a.vr b.s + c.vr) riding in as the accumulator.
// C += A B for symmetric commuting A, B (upper core tiles, vr, s of C; s8_finish completes the operand form of C)
template <int NC>
__device__ __forceinline__ void mm_s8(const SMat<NC>& a, const SMat<NC>& b, SMat<NC>& c) {
  // (the rank-1 term of the border goes into the accumulators BEFORE the matrix instructions: a vector instruction that reads a
  // matrix result waits for the whole instruction, ~45 cycles; the other way round costs two wait states)
#pragma unroll
  for (int I = 0; I < NC; ++I)
#pragma unroll
    for (int J = I; J < NC; ++J) c.m[I][J] = fma(a.vr[I], b.vc[J], c.m[I][J]);
#pragma unroll
  for (int K = 0; K < NC; ++K)
#pragma unroll
    for (int I = 0; I < NC; ++I)
#pragma unroll
      for (int J = I; J < NC; ++J) c.m[I][J] = mfma4(a.m[K][I], b.m[K][J], c.m[I][J]);
  double t[NC], cs = 0.0;
#pragma unroll
  for (int I = 0; I < NC; ++I) {
    t[I] = 0.0;
#pragma unroll
    for (int K = 0; K < NC; ++K) t[I] = fma(a.m[K][I], b.vr[K], t[I]);  // lane (r, c): A[4I+c][4K+r] b[4K+r]
    cs = fma(a.vr[I], b.vr[I], cs);
  }
#pragma unroll
  for (int I = 0; I < NC; ++I) c.vr[I] = mfma4(t[I], 1.0, fma(a.vr[I], b.s, c.vr[I]));
  c.s = mfma4(cs, 1.0, fma(a.s, b.s, c.s));
}
// two products with one left operand, interleaved (C1 += A B1, C2 += A B2)
template <int NC>
__device__ __forceinline__ void mm_s8x2(const SMat<NC>& a, const SMat<NC>& b1, SMat<NC>& c1, const SMat<NC>& b2, SMat<NC>& c2) {
#pragma unroll
  for (int I = 0; I < NC; ++I)
#pragma unroll
    for (int J = I; J < NC; ++J) {
      c1.m[I][J] = fma(a.vr[I], b1.vc[J], c1.m[I][J]);
      c2.m[I][J] = fma(a.vr[I], b2.vc[J], c2.m[I][J]);
    }
#pragma unroll
  for (int K = 0; K < NC; ++K)
#pragma unroll
    for (int I = 0; I < NC; ++I)
#pragma unroll
      for (int J = I; J < NC; ++J) {
        c1.m[I][J] = mfma4(a.m[K][I], b1.m[K][J], c1.m[I][J]);
        c2.m[I][J] = mfma4(a.m[K][I], b2.m[K][J], c2.m[I][J]);
      }
  double t1[NC], t2[NC], cs1 = 0.0, cs2 = 0.0;
#pragma unroll
  for (int I = 0; I < NC; ++I) {
    t1[I] = t2[I] = 0.0;
#pragma unroll
    for (int K = 0; K < NC; ++K) {
      t1[I] = fma(a.m[K][I], b1.vr[K], t1[I]);
      t2[I] = fma(a.m[K][I], b2.vr[K], t2[I]);
    }
    cs1 = fma(a.vr[I], b1.vr[I], cs1);
    cs2 = fma(a.vr[I], b2.vr[I], cs2);
  }
#pragma unroll
  for (int I = 0; I < NC; ++I) {
    c1.vr[I] = mfma4(t1[I], 1.0, fma(a.vr[I], b1.s, c1.vr[I]));
    c2.vr[I] = mfma4(t2[I], 1.0, fma(a.vr[I], b2.s, c2.vr[I]));
  }
  c1.s = mfma4(cs1, 1.0, fma(a.s, b1.s, c1.s));
  c2.s = mfma4(cs2, 1.0, fma(a.s, b2.s, c2.s));
}
// operand form of a product: lower core tiles by the in-chain lane swap, the c form of the border column
template <int NC>
__device__ __forceinline__ void s8_finish(SMat<NC>& a, int swap_lane, int tail_lane) {
#pragma unroll
  for (int I = 1; I < NC; ++I)
#pragma unroll
    for (int J = 0; J < I; ++J) a.m[I][J] = __shfl(a.m[J][I], swap_lane);
#pragma unroll
  for (int J = 0; J < NC; ++J) a.vc[J] = __shfl(a.vr[J], tail_lane);
}
// LEFT-operand form of a product (core tiles complete, vr, s): the lower core tiles alone -- a symmetric left operand is read
// through its tiles, its r-form border and its corner only (mm_s8, chain_step8), the c form is a right operand's business
template <int NC>
__device__ __forceinline__ void s8_finish_lower(SMat<NC>& a, int swap_lane) {
#pragma unroll
  for (int I = 1; I < NC; ++I)
#pragma unroll
    for (int J = 0; J < I; ++J) a.m[I][J] = __shfl(a.m[J][I], swap_lane);
}
template <int NC>
__device__ __forceinline__ void s8_finish_vc(SMat<NC>& a, int tail_lane) {
#pragma unroll
  for (int J = 0; J < NC; ++J) a.vc[J] = __shfl(a.vr[J], tail_lane);
}
// two products with one RIGHT operand, interleaved (C1 += A1 B, C2 += A2 B): A1, A2 in left-operand form
template <int NC>
__device__ __forceinline__ void mm_s8x2r(const SMat<NC>& a1, const SMat<NC>& a2, const SMat<NC>& b, SMat<NC>& c1, SMat<NC>& c2) {
#pragma unroll
  for (int I = 0; I < NC; ++I)
#pragma unroll
    for (int J = I; J < NC; ++J) {
      c1.m[I][J] = fma(a1.vr[I], b.vc[J], c1.m[I][J]);
      c2.m[I][J] = fma(a2.vr[I], b.vc[J], c2.m[I][J]);
    }
#pragma unroll
  for (int K = 0; K < NC; ++K)
#pragma unroll
    for (int I = 0; I < NC; ++I)
#pragma unroll
      for (int J = I; J < NC; ++J) {
        c1.m[I][J] = mfma4(a1.m[K][I], b.m[K][J], c1.m[I][J]);
        c2.m[I][J] = mfma4(a2.m[K][I], b.m[K][J], c2.m[I][J]);
      }
  double t1[NC], t2[NC], cs1 = 0.0, cs2 = 0.0;
#pragma unroll
  for (int I = 0; I < NC; ++I) {
    t1[I] = t2[I] = 0.0;
#pragma unroll
    for (int K = 0; K < NC; ++K) {
      t1[I] = fma(a1.m[K][I], b.vr[K], t1[I]);
      t2[I] = fma(a2.m[K][I], b.vr[K], t2[I]);
    }
    cs1 = fma(a1.vr[I], b.vr[I], cs1);
    cs2 = fma(a2.vr[I], b.vr[I], cs2);
  }
#pragma unroll
  for (int I = 0; I < NC; ++I) {
    c1.vr[I] = mfma4(t1[I], 1.0, fma(a1.vr[I], b.s, c1.vr[I]));
    c2.vr[I] = mfma4(t2[I], 1.0, fma(a2.vr[I], b.s, c2.vr[I]));
  }
  c1.s = mfma4(cs1, 1.0, fma(a1.s, b.s, c1.s));
  c2.s = mfma4(cs2, 1.0, fma(a2.s, b.s, c2.s));
}
// out = c0 I + c1 W1 + c2 W2 (+ c3 W3), every part (operands are complete: the combination is too); ACCUM: only what a
// product accumulates into (upper core tiles, vr, s) -- the initial value of an accumulation that s8_finish completes later
template <int NC, bool WITH3, bool ACCUM = false>
__device__ __forceinline__ void s8_comb(SMat<NC>& out, double c0, double c1, double c2, double c3, const SMat<NC>& W1, const SMat<NC>& W2,
                                        const SMat<NC>& W3, const LanePos& lp) {
  // (the c0 I term rides in as the addend of the first multiply-add: no separate add on the diagonal tiles and the corner)
  auto lc = [&](double x1, double x2, double x3, double add) {
    double v = fma(c1, x1, add);
    v = fma(c2, x2, v);
    if constexpr (WITH3) v = fma(c3, x3, v);
    return v;
  };
  const double dg = (lp.r == lp.c) ? c0 : 0.0;
#pragma unroll
  for (int I = 0; I < NC; ++I) {
#pragma unroll
    for (int J = ACCUM ? I : 0; J < NC; ++J) out.m[I][J] = lc(W1.m[I][J], W2.m[I][J], W3.m[I][J], I == J ? dg : 0.0);
    out.vr[I] = lc(W1.vr[I], W2.vr[I], W3.vr[I], 0.0);
    if constexpr (!ACCUM) out.vc[I] = lc(W1.vc[I], W2.vc[I], W3.vc[I], 0.0);
  }
  out.s = lc(W1.s, W2.s, W3.s, c0);
}


// chain step in real blocks for the core + border form: (Ur + i Ui) <- (C - i S)(Ur + i Ui), C and S symmetric (left-operand form:
// core tiles complete, vr, s).
// Core (the NC x NC tiles, on the matrix cores): three real products, T1 = C Ur, T2 = S Ui, T3 = (C - S)(Ur + Ui), Re = T1 + T2,
// Im = T3 - T1 + T2.  The rank-1 term of the border (column of the left operand times row of the state) is the initial value of the
// three accumulators, in the same 3M form.
// Row border: 3M saves a product on the matrix cores only -- on the vector unit add, mul and fma cost the same, so the row border uses
// the direct form Re = C Ur + S Ui, Im = C Ui - S Ur as fma chains.  No lane swaps, no DPP reductions: the sum index is on r (the r-form
// border vr of the symmetric left operand is also its border row) and ONE matrix instruction against a tile of ones reduces it, the
// k = D-1 term riding in as the accumulator: A = 1, B = partials -> D[i][j] = sum_r t(r, c = j), the c form replicated over r (rc).
// Column border and corner: the packed registers of GBorder ARE a right-operand tile whose four columns are {u, -i u, -u, i u} read as
// real pairs, and the quad rotation Q of a packed register P is -i P.  So column c of C P + S Q is {C ur + S ui, C ui - S ur, -, -} =
// {Re', Im', -Re', -Im'}, the packed form again:
//   Pc'[I] = sum_K mfma(C.m[K][I], Pc[K]) + mfma(S.m[K][I], Qc[K])    accumulator C.vr[I] Ps + S.vr[I] Qs (the k = D-1 term)
//   Ps'    = mfma(1, sum_K C.vr[K] Pc[K] + S.vr[K] Qc[K], C.s Ps + S.s Qs)   (ones as A: column sums, replicated over r)
// The state stays packed from slice to slice; only the rotations are formed per step, at the head of the step.
// Every right-hand side reads the old state; every vector operation that feeds a matrix instruction is issued before the first one
// (a vector instruction that reads a matrix result waits ~45 cycles, the other way round costs two wait states).
template <int NC>
__device__ __forceinline__ void chain_step8(const SMat<NC>& Cc, const SMat<NC>& Sc, GMat<NC>& Ur, GMat<NC>& Ui, GBorder<NC>& Ub) {
  double Qc[NC];
#pragma unroll
  for (int K = 0; K < NC; ++K) Qc[K] = quad_rot1(Ub.Pc[K]);
  const double Qs = quad_rot1(Ub.Ps);
  double Dm[NC][NC], Us[NC][NC], T1[NC][NC], T2[NC][NC], T3[NC][NC];
#pragma unroll
  for (int I = 0; I < NC; ++I)
#pragma unroll
    for (int J = 0; J < NC; ++J) {
      Dm[I][J] = Cc.m[I][J] - Sc.m[I][J];
      Us[I][J] = Ur.m[I][J] + Ui.m[I][J];
    }
  {
    double dv[NC], us[NC];
#pragma unroll
    for (int I = 0; I < NC; ++I) {
      dv[I] = Cc.vr[I] - Sc.vr[I];
      us[I] = Ur.rc[I] + Ui.rc[I];
    }
#pragma unroll
    for (int I = 0; I < NC; ++I)
#pragma unroll
      for (int J = 0; J < NC; ++J) {
        T1[I][J] = Cc.vr[I] * Ur.rc[J];
        T2[I][J] = Sc.vr[I] * Ui.rc[J];
        T3[I][J] = dv[I] * us[J];
      }
  }
  // row border, lane (r, c): sum_K M[D-1][4K+r] U[4K+r][4J+c]; accumulator M[D-1][D-1] U[D-1][4J+c]
  double tr[NC], ti[NC], ar[NC], ai[NC];
#pragma unroll
  for (int J = 0; J < NC; ++J) {
    tr[J] = Cc.vr[0] * Ur.m[0][J];
    ti[J] = Cc.vr[0] * Ui.m[0][J];
#pragma unroll
    for (int K = 1; K < NC; ++K) {
      tr[J] = fma(Cc.vr[K], Ur.m[K][J], tr[J]);
      ti[J] = fma(Cc.vr[K], Ui.m[K][J], ti[J]);
    }
#pragma unroll
    for (int K = 0; K < NC; ++K) {
      tr[J] = fma(Sc.vr[K], Ui.m[K][J], tr[J]);
      ti[J] = fma(-Sc.vr[K], Ur.m[K][J], ti[J]);
    }
    ar[J] = fma(Sc.s, Ui.rc[J], Cc.s * Ur.rc[J]);
    ai[J] = fma(-Sc.s, Ur.rc[J], Cc.s * Ui.rc[J]);
  }
  // column border, packed: the k = D-1 term M[4I+r][D-1] U[D-1][D-1] as the accumulator of the tile products below
  // corner, lane (r, c): sum_K M[D-1][4K+r] U[4K+r][D-1] of column c; accumulator M[D-1][D-1] U[D-1][D-1]
  double Pn[NC];
#pragma unroll
  for (int I = 0; I < NC; ++I) Pn[I] = fma(Sc.vr[I], Qs, Cc.vr[I] * Ub.Ps);
  double ts = Cc.vr[0] * Ub.Pc[0];
#pragma unroll
  for (int K = 1; K < NC; ++K) ts = fma(Cc.vr[K], Ub.Pc[K], ts);
#pragma unroll
  for (int K = 0; K < NC; ++K) ts = fma(Sc.vr[K], Qc[K], ts);
  const double es = fma(Sc.s, Qs, Cc.s * Ub.Ps);
  // the matrix instructions: core and column border, then the border reductions straight into the state
#pragma unroll
  for (int K = 0; K < NC; ++K)
#pragma unroll
    for (int I = 0; I < NC; ++I) {
      Pn[I] = mfma4(Cc.m[K][I], Ub.Pc[K], Pn[I]);
#pragma unroll
      for (int J = 0; J < NC; ++J) {
        T1[I][J] = mfma4(Cc.m[K][I], Ur.m[K][J], T1[I][J]);
        T2[I][J] = mfma4(Sc.m[K][I], Ui.m[K][J], T2[I][J]);
        T3[I][J] = mfma4(Dm[K][I], Us[K][J], T3[I][J]);
      }
      Pn[I] = mfma4(Sc.m[K][I], Qc[K], Pn[I]);
    }
#pragma unroll
  for (int I = 0; I < NC; ++I) {
    Ur.rc[I] = mfma4(1.0, tr[I], ar[I]);
    Ui.rc[I] = mfma4(1.0, ti[I], ai[I]);
  }
  Ub.Ps = mfma4(1.0, ts, es);
#pragma unroll
  for (int I = 0; I < NC; ++I) Ub.Pc[I] = Pn[I];
#pragma unroll
  for (int I = 0; I < NC; ++I)
#pragma unroll
    for (int J = 0; J < NC; ++J) {
      Ur.m[I][J] = T1[I][J] + T2[I][J];
      Ui.m[I][J] = (T3[I][J] - T1[I][J]) + T2[I][J];
    }
}

// q = 4 plan: degree 4r, s squarings, from a bound on ||X||_1
__device__ __forceinline__ void plan_q4(double nrm, int& r, int& s) {
  // Taylor backward-error bounds for unit roundoff 2^-52 (theta_m of Al-Mohy & Higham scaled by 2^(1/m))
  const double th[5] = {4.0e-4, 5.45e-2, 3.18e-1, 8.16e-1, 1.49};
  int best_r = 5, best_s = 0, best_cost = 1 << 30;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    int si = c3p_squarings(nrm, th[i]);
    const int cost = i + si;
    if (cost < best_cost || (cost == best_cost && si <= best_s)) {
      best_cost = cost;
      best_r = i + 1;
      best_s = si;
    }
  }
  r = best_r;
  s = best_s;
}

// Write a D-layout matrix times the complex scalar (sr + i si), with optional row phases,
// to a plain complex [D][D] array.
// cos / sin of the row phases of the lane's rows (store_plain takes them instead of evaluating sincos in the store)
template <int D>
__device__ __forceinline__ void row_phase_factors(const double* row_phase, const LanePos& lp, double (&pc)[SD<D>::NBI],
                                                  double (&ps)[SD<D>::NBI]) {
#pragma unroll
  for (int I = 0; I < SD<D>::NBI; ++I) {
    const int row = 2 * I + (lp.r >> 1);
    pc[I] = 1.0, ps[I] = 0.0;
    if (row_phase != nullptr && row < D) sincos(row_phase[row], &ps[I], &pc[I]);
  }
}

// out = zh with the lane's rows times the complex factors pr[I] + i pi[I], in D-layout.  r even: mine = Re, other = Im; r odd:
// mine = Im, other = Re -- the partner's halves come from lane ^ 16, all exchanges in flight together (behind the predicated
// stores of store_plain each one was a round trip of its own: 15 in a row in the final store of cfg2).
template <int D>
__device__ __forceinline__ void scale_rows(const double (&zh)[SD<D>::NBI][SD<D>::NJ], const double (&pr)[SD<D>::NBI],
                                           const double (&pi)[SD<D>::NBI], const LanePos& lp,
                                           double (&out)[SD<D>::NBI][SD<D>::NJ]) {
  using C = SD<D>;
  double oth[C::NBI][C::NJ];
#pragma unroll
  for (int I = 0; I < C::NBI; ++I)
#pragma unroll
    for (int J = 0; J < C::NJ; ++J) oth[I][J] = __shfl_xor(zh[I][J], 16);
#pragma unroll
  for (int I = 0; I < C::NBI; ++I)
#pragma unroll
    for (int J = 0; J < C::NJ; ++J)
      out[I][J] = (lp.r & 1) ? fma(pr[I], zh[I][J], pi[I] * oth[I][J]) : fma(pr[I], zh[I][J], -pi[I] * oth[I][J]);
}

// ---- scale_rows and store_plain on the tiles of a dealt product (epilogues of mm_split<D, 4>) ----
// The block that formed a tile holds it whole: every element gets the exchange and the fma that scale_rows gives it, on the same
// operands, without the trip through the image that hands the product to one block in register order.
__device__ __forceinline__ double scale_elem(double mine, double oth, double pr, double pi, int r) {
  return (r & 1) ? fma(pr, mine, pi * oth) : fma(pr, mine, -pi * oth);
}

// the product times one complex factor pr + i pi, written to the image (scale_rows with the same factor in every row)
struct SplitScale {
  static constexpr bool WRITE = true;
  double pr, pi;
  int r;
  template <int NT>
  __device__ __forceinline__ void operator()(double (&acc)[NT], const int (&)[NT], const int (&)[NT], const bool (&)[NT]) const {
    double oth[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) oth[t] = __shfl_xor(acc[t], 16);
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = scale_elem(acc[t], oth[t], pr, pi, r);
  }
};

// cos / sin of the row phases of the rows of the lane's dealt tiles (row_phase_factors for SplitStore)
template <int D>
__device__ __forceinline__ void dealt_row_phase_factors(const double* row_phase, const LanePos& lp, double (&pc)[sd_split_tasks<D>(4)],
                                                        double (&ps)[sd_split_tasks<D>(4)]) {
  constexpr int NT = sd_split_tasks<D>(4);
  int tI[NT], tJ[NT];
  bool on[NT];
  split_tiles<D, 4>(lp.b, tI, tJ, on);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int row = 2 * tI[t] + (lp.r >> 1);
    pc[t] = 1.0, ps[t] = 0.0;
    if (row_phase != nullptr && on[t] && row < D) sincos(row_phase[row], &ps[t], &pc[t]);
  }
}

// the product with its rows times their phases, stored as a plain complex [D][D] array and not written to the image
// (store_plain with sr = 1, si = 0 and the factors of dealt_row_phase_factors)
template <int D>
struct SplitStore {
  static constexpr bool WRITE = false;
  double* dst;
  const double (&pc)[sd_split_tasks<D>(4)];
  const double (&ps)[sd_split_tasks<D>(4)];
  int r, c;
  template <int NT>
  __device__ __forceinline__ void operator()(double (&acc)[NT], const int (&tI)[NT], const int (&tJ)[NT], const bool (&on)[NT]) const {
    constexpr double sr = 1.0, si = 0.0;
    double oth[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) oth[t] = __shfl_xor(acc[t], 16);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int row = 2 * tI[t] + (r >> 1), col = 4 * tJ[t] + c;
      const double pr = sr * pc[t] - si * ps[t], pi = sr * ps[t] + si * pc[t];
      if (on[t] && row < D && col < D) dst[(row * D + col) * 2 + (r & 1)] = scale_elem(acc[t], oth[t], pr, pi, r);
    }
  }
};

// SplitStore over the deal of four blocks: every double of the [D][D] complex result is stored by exactly one (block, task, lane)
// and the index of every store lies inside the result
template <int D>
constexpr bool sd_split_store_ok() {
  int seen[D * D * 2] = {};
  for (int blk = 0; blk < 4; ++blk)
    for (int t = 0; t < sd_split_tasks<D>(4); ++t)
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
          const SDTile s = sd_split_deal<D>(4, blk, t);
          const int row = 2 * s.I + (r >> 1), col = 4 * s.J + c;
          if (!(s.on && row < D && col < D)) continue;
          const int idx = (row * D + col) * 2 + (r & 1);
          if (idx < 0 || idx >= D * D * 2) return false;
          ++seen[idx];
        }
  for (int i = 0; i < D * D * 2; ++i)
    if (seen[i] != 1) return false;
  return true;
}
static_assert(sd_split_store_ok<5>() && sd_split_store_ok<6>() && sd_split_store_ok<7>() && sd_split_store_ok<8>() && sd_split_store_ok<9>(),
              "dealt store: every element of the result exactly once, nothing outside it");

template <int D, bool WRITE_THROUGH = false>
__device__ __forceinline__ void store_plain(const double (&zh)[SD<D>::NBI][SD<D>::NJ], double* dst,
                                            double sr, double si, const double* row_phase,
                                            const LanePos& lp, bool active, const double* pre_c = nullptr,
                                            const double* pre_s = nullptr) {
  using C = SD<D>;
  double pr[C::NBI], pi[C::NBI];
#pragma unroll
  for (int I = 0; I < C::NBI; ++I) {
    const int row = 2 * I + (lp.r >> 1);
    pr[I] = sr, pi[I] = si;
    if (pre_c != nullptr) {
      pr[I] = sr * pre_c[I] - si * pre_s[I];
      pi[I] = sr * pre_s[I] + si * pre_c[I];
    } else if (row_phase != nullptr && row < D) {
      double sn, cs;
      sincos(row_phase[row], &sn, &cs);
      pr[I] = sr * cs - si * sn;
      pi[I] = sr * sn + si * cs;
    }
  }
  double outv[C::NBI][C::NJ];
  scale_rows<D>(zh, pr, pi, lp, outv);
#pragma unroll
  for (int I = 0; I < C::NBI; ++I) {
    const int row = 2 * I + (lp.r >> 1);
#pragma unroll
    for (int J = 0; J < C::NJ; ++J) {
      const int col = 4 * J + lp.c;
      if (active && row < D && col < D) {
        double* p = dst + (row * D + col) * 2 + (lp.r & 1);
        if constexpr (WRITE_THROUGH) {
          // sc1 (write-through) store: visible to other CUs/XCDs without a release fence
          __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(outv[I][J]),
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
          *p = outv[I][J];
        }
      }
    }
  }
}

// Cross-lane steps of the prologue's reductions on the register path (no LDS round trip, ~50 cycles each on a cold CU):
// DPP inside a row of 16 lanes, v_permlane16_swap / v_permlane32_swap across rows.  All 64 lanes are active at every call.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xf, 0xf, true);
  hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_XOR3 = 0x1B;                // quad_perm [1,0,3,2], [2,3,0,1], [3,2,1,0]
constexpr int DPP_HALF_MIRROR = 0x141;                                          // row_half_mirror: lane i of eight reads 7 - i
constexpr int DPP_ROR1 = 0x121, DPP_ROR2 = 0x122, DPP_ROR4 = 0x124, DPP_ROR8 = 0x128;  // row_ror (row_ror:8 is lane ^ 8)
// (a, b) = (v of the lane with bit 4 clear, v of the lane with bit 4 set) of the pair {lane, lane ^ 16}, in both lanes
__device__ __forceinline__ void pair_xor16(double v, double& a, double& b) {
  const unsigned lo = __double2loint(v), hi = __double2hiint(v);
  const auto rl = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  const auto rh = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  a = __hiloint2double(rh[0], rl[0]);
  b = __hiloint2double(rh[1], rl[1]);
}
// the same for the pair {lane, lane ^ 32}
__device__ __forceinline__ void pair_xor32(double v, double& a, double& b) {
  const unsigned lo = __double2loint(v), hi = __double2hiint(v);
  const auto rl = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  const auto rh = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  a = __hiloint2double(rh[0], rl[0]);
  b = __hiloint2double(rh[1], rl[1]);
}
// max over {lane, lane ^ 16, lane ^ 32, lane ^ 48}
__device__ __forceinline__ double rows_max(double v) {
  double a, b;
  pair_xor16(v, a, b);
  v = fmax(a, b);
  pair_xor32(v, a, b);
  return fmax(a, b);
}
// v_lane + v_{lane ^ o} for o = 32, 16, 8, 4, 2, 1 in this order: the association of the former __shfl_xor loop (an addition
// commutes, so both lanes of a pair hold the same bits after every step -- which is what lets row_ror:4 stand for lane ^ 4:
// behind the step o = 8 the lanes i ^ 4 and i ^ 12, one of which it reads, are equal)
__device__ __forceinline__ double wave_sum64(double v) {
  double a, b;
  pair_xor32(v, a, b);
  v = a + b;
  pair_xor16(v, a, b);
  v = a + b;
  v += dpp_f64<DPP_ROR8>(v);
  v += dpp_f64<DPP_ROR4>(v);
  v += dpp_f64<DPP_XOR2>(v);
  v += dpp_f64<DPP_XOR1>(v);
  return v;
}
// the maxima of N values over the wave as ONE latency chain: the steps of the N reductions side by side (a maximum is exact
// and free of order)
template <int N>
__device__ __forceinline__ void wave_max64(double (&v)[N]) {
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = fmax(v[n], dpp_f64<DPP_ROR1>(v[n]));
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = fmax(v[n], dpp_f64<DPP_ROR2>(v[n]));
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = fmax(v[n], dpp_f64<DPP_ROR4>(v[n]));
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = fmax(v[n], dpp_f64<DPP_ROR8>(v[n]));
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = rows_max(v[n]);
}
// max over the 16 lanes of a chain (lane bits 0, 1, 4, 5)
__device__ __forceinline__ double chain_max16(double v) {
  v = fmax(v, dpp_f64<DPP_XOR1>(v));
  v = fmax(v, dpp_f64<DPP_XOR2>(v));
  return rows_max(v);
}

// Column sums of |G|, the block the segment's norm bound is formed from (c3p_sd_segment_norm below): SD_CSW doubles per table,
// cs_k[j] = sum_i |G_k[i][j]| in slot j < D and zeros behind.  The sums are taken from the half-image table in LDS, in this one
// place and in one order, so that every kernel and every table mode (built in the kernel, copied from the prep kernel's buffer)
// forms the same bits from the same table.  Plain sqrt(a^2 + b^2) on unrolled, independent LDS reads (round 6: the elements
// are dt x Hamiltonian entries, no overflow to guard, and the table build sits on the critical path of every workgroup's prologue).
constexpr int SD_CSW = 16;  // = the lanes of a chain: lane idx16 = j takes column j (D <= 12)

template <int D>
__device__ __forceinline__ double sd_colsum(const double* g, int j) {
  constexpr int W = SD<D>::W;
  double cs = 0.0;
  if (j < D) {
    double ar[D], ai[D];
#pragma unroll
    for (int i = 0; i < D; ++i) ar[i] = g[(2 * i) * W + j], ai[i] = g[(2 * i + 1) * W + j];
#pragma unroll
    for (int i = 0; i < D; ++i) cs += sqrt(fma(ar[i], ar[i], ai[i] * ai[i]));
  }
  return cs;
}

// the block of tables that are already in LDS (copied from global memory; the grad kernels): table first + step q goes to
// lanes 16 q .. 16 q + 15 of the wave, four tables per pass.  The caller synchronises before (tables) and behind (block).
template <int D>
__device__ __forceinline__ void sd_colsums(const double* tab, int K, double* csb, int lane, int first = 0, int step = 1) {
  constexpr int MAT = SD<D>::MAT;
  for (int t0 = first; t0 <= K; t0 += 4 * step) {
    const int ti = t0 + (lane >> 4) * step;
    if (ti <= K) csb[ti * SD_CSW + (lane & 15)] = sd_colsum<D>(tab + ti * (MAT + 4), lane & 15);
  }
}

// Segment-wide bound on ||X(t)||_1, X(t) = G_0 + sum_k c_k(t) G_k, for one chain (16 lanes, lane idx16 = column):
//   ||X(t)||_1 = max_j sum_i |X_ij(t)|  <=  max_j ( cs_0[j] + sum_k max_t |c_k(t)| cs_k[j] ),
// never larger than the sum of norms ||G_0||_1 + sum_k max_t |c_k| ||G_k||_1 (max_j (a_j + b_j) <= max a + max b), which lets
// every table's widest column meet in one column it does not have.  One fma chain per column in the order of the tables, then
// the maximum over the chain's lanes: every kernel that decides on this bound gets the same bits.  `maxk(k)` is the chain's
// max_t |c_k(t)| on the segment, uniform over the chain's lanes.
// the lane's column of the bound; the chain kernel takes the maximum over its lanes on the register path
template <class F>
__device__ __forceinline__ double c3p_sd_segment_col(const double* csb, int K, int idx16, F&& maxk) {
  double v = csb[idx16];
  for (int k = 0; k < K; ++k) v = fma(maxk(k), csb[(k + 1) * SD_CSW + idx16], v);
  return v;
}
template <class F>
__device__ __forceinline__ double c3p_sd_segment_norm(const double* csb, int K, int idx16, F&& maxk) {
  double v = c3p_sd_segment_col(csb, K, idx16, maxk);
  v = fmax(v, __shfl_xor(v, 1));
  v = fmax(v, __shfl_xor(v, 2));
  v = fmax(v, __shfl_xor(v, 16));
  v = fmax(v, __shfl_xor(v, 32));
  return v;
}

// The wave builds its own tables in LDS (unitary mode): G = -i dt (h - tr h / D) as half images plus
// {Re mu, Im mu, ||G||_1, max |Re G|} -- what smalld_prep_kernel writes, without a dependent launch in
// front of the chain kernel (~12 us of a 250 us batch).
// `under_loads()` is work of the caller that needs no table: it runs once, behind the issue of the first table's loads (the
// kernel's cold global accesses) or, in a wave that builds no table, at once.
template <int D, class F>
__device__ __forceinline__ void build_tables(const SmallArgs& A, int sample, double* tab, double* csb, int lane, int first, int step,
                                             F&& under_loads) {
  // the elements are rounded as products first, the diagonal's shift is a second rounding: a fused -x dt - mu gives other tables
#pragma clang fp contract(off)
  using C = SD<D>;
  constexpr int MAT = C::MAT, W = C::W;
  constexpr int NE = (D * D + 63) / 64;
  if (first > A.K) under_loads();
  for (int ti = first; ti <= A.K; ti += step) {  // (a workgroup of several waves deals the tables to its waves)
    double* out = tab + ti * (MAT + 4);
    const cplx* h = (ti == 0) ? A.h0 + (long)sample * A.h0_bstride
                              : A.hks + (long)sample * A.hks_bstride + (long)(ti - 1) * D * D;
    // every load of the table is in flight before the first is waited for: the address is clamped and the value selected
    // behind the load (a load under `e < D * D` put a branch and a wait between the two of D = 9, both cold misses)
    cplx x[NE];
#pragma unroll
    for (int q = 0; q < NE; ++q) x[q] = h[min(lane + 64 * q, D * D - 1)];
    if (ti == first) under_loads();
    for (int e = lane; e < MAT; e += 64) out[e] = 0.0;
    double gr[NE], gi[NE];
    double tim = 0.0;
#pragma unroll
    for (int q = 0; q < NE; ++q) {
      const int e = lane + 64 * q;
      const bool in = e < D * D;
      gr[q] = in ? x[q].y * A.dt : 0.0;  // -i dt h
      gi[q] = in ? -x[q].x * A.dt : 0.0;
      if (in && e / D == e % D) tim += gi[q];
    }
    // (round 6) the shift is IMAGINARY only: a real shift (lossy Hamiltonians) makes the shifted chain product grow like
    // e^{|Re mu| n} while e^{sum mu} underflows -- inf * 0 over a long segment (tools/fuzz_r06.py found it on the Lindblad tables)
    const double mur = 0.0, mui = wave_sum64(tim) / D;
    wave_sync();
    double remax = 0.0;
#pragma unroll
    for (int q = 0; q < NE; ++q) {
      const int e = lane + 64 * q;
      if (e < D * D) {
        const int i = e / D, j = e - i * D;
        if (i == j) {
          gr[q] -= mur;
          gi[q] -= mui;
        }
        out[(2 * i) * W + j] = gr[q];
        out[(2 * i + 1) * W + j] = gi[q];
        remax = fmax(remax, fabs(gr[q]));
      }
    }
    // column sums of |G|: kept for the segment's bound, their maximum is the 1-norm
    wave_sync();
    const double cs = sd_colsum<D>(out, lane);
    if (lane < SD_CSW) csb[ti * SD_CSW + lane] = cs;
    // the real fast path also needs Y = -Im G symmetric (Hermitian input).  Dressed operators V^T H V are
    // symmetric only to rounding (measured 5e-16 relative), so asymmetry below 1e-14 ||G|| counts as none;
    // anything larger is folded into the flag and sends the sample to the complex path.
    double asym = 0.0, rsk = 0.0;
#pragma unroll
    for (int q = 0; q < NE; ++q) {
      const int e = lane + 64 * q;
      if (e < D * D) {
        const int i = e / D, j = e - i * D;
        asym = fmax(asym, fabs(gi[q] - out[(2 * j + 1) * W + i]));
        rsk = fmax(rsk, fabs(gr[q] + out[(2 * j) * W + i]));  // G + G^H = 0 <=> Hermitian Hamiltonian (diagonal: 2 Re G_ii)
      }
    }
    // the four maxima come down together.  The asymmetry joins the maximum of |Re G| behind the reduction: it is uniform, and
    // max_lanes fmax(x_lane, a) = fmax(max_lanes x_lane, a)
    double red[4] = {cs, asym, rsk, remax};
    wave_max64(red);
    const double nrm = red[0];
    asym = red[1], rsk = red[2], remax = red[3];
    if (asym > 1e-14 * nrm) remax = fmax(remax, asym);
    // (round 6) NEGATIVE: complex but skew-Hermitian to rounding -- a normal generator: T18 with the economised parameters
    if (remax > 0.0 && fmax(asym, rsk) <= 1e-14 * nrm) remax = -remax;
    if (lane == 0) {
      out[MAT + 0] = mur;
      out[MAT + 1] = mui;
      out[MAT + 2] = nrm;
      out[MAT + 3] = remax;
    }
  }
  wave_sync();
}

// XG: the generators are supplied per slice (branch B of pwc, propagation.py:295-308, and c3p_expm):
// X_n = coef * hs[b,n] - mu_n with (mu_n, ||X_n - mu_n||_1) from the hmeta pre-pass; no tables, no signals.
// MW (table modes, fused combine): ONE WORKGROUP PER SAMPLE, S / 4 waves of four chains each (cfg2: 8 waves = two per SIMD
// of one CU).  The tables are built once per workgroup and the waves' partial products meet in LDS behind a barrier,
// instead of once per wave and through global memory behind a ticket: the fixed cost of a cfg2 batch (29 us of 149:
// combine 12, table build 4, launch and prologue 13) is what this mode attacks.
template <int D, bool GIVEN, bool DUS, bool XG = false, bool MW = false, bool SPLIT = false>
__global__ void __launch_bounds__((MW ? 512 : 64), 2) smalld_chain_kernel(SmallArgs A) {
  using C = SD<D>;
  constexpr int NBI = C::NBI, NJ = C::NJ, W = C::W, MAT = C::MAT, IMG = C::IMG;
  const int lane = MW ? (threadIdx.x & 63) : threadIdx.x;
  const int wv = MW ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : 0;
  const int nwv = MW ? (int)(blockDim.x >> 6) : 1;
#ifdef C3P_SD_TIMING
  long long tk0 = wall_clock64(), tk1 = 0, tk2 = 0, tk3 = 0, tk4 = 0, tk5 = 0, tk6 = 0, tk7 = 0, tk8 = 0, tk9 = 0, tkl = 0, tka = 0, tkb = 0, tkc = 0;
#define SD_TICK(v) v = wall_clock64()
#else
#define SD_TICK(v)
#endif
  LanePos lp;
  lp.r = lane >> 4;
  lp.b = (lane >> 2) & 3;
  lp.c = lane & 3;
  lp.idx16 = lp.r * 4 + lp.c;
  const int K = A.K;
  double* tab = c3p_sd_lds;  // (1+K) images + scalars (table modes only; shared by the waves of a workgroup)
  // (core + border real loop: one more row per chain, the weight of the drift table -- see the per-segment weights below)
  const int SG = ((K + ((SPLIT && K > 0) ? 1 : 0)) * A.Lmax) | 1;
  double* img = tab + ((GIVEN || XG) ? 0 : (1 + K) * (MAT + 4)) + wv * (4 * IMG + 4 * SG);  // this wave's 4 chain images
  double* sg = img + 4 * IMG;  // 4 chains x K x Lmax signals, odd chain stride (bank spread)
  // column sums of the tables, a block of its own (the table records and every offset into them stay).  Workgroup per sample:
  // behind the waves' images.  One wave: in the wave's images, which nothing touches before the slice loop (the bound is taken in
  // the prologue) -- a launch of this mode fills the LDS of a CU with eight workgroups at the segment length pick_segments allows,
  // and must not grow; behind the images only where the block does not fit in them (D = 2, 3 with more than ten tables)
  double* csb = (!MW && (1 + K) * SD_CSW <= 4 * IMG) ? img : tab + (1 + K) * (MAT + 4) + nwv * (4 * IMG + 4 * SG);

  // XCD-aware block order: workgroups are dealt round-robin to the 8 XCDs, each with its own L2.  Logical block
  // (bid % 8) * (nb / 8) + bid / 8 keeps consecutive logical blocks -- the waves of one sample, which exchange their
  // segment partials in the fused combine -- on ONE XCD.
  // Workgroup per sample: the workgroup IS the sample (the launch has B workgroups of S / 4 waves, so every chain is valid) and
  // the wave holds four consecutive segments -- no division stands in front of the kernel's first, cold loads.  S is 8, 16 or
  // 32 there (launch_chain_t), so the quotients by S and by S / 2 below are shifts of the same 64-bit products.
  long cc;
  int sample, seg, n0, n1;
  bool valid;
  const int sshift = 31 - __clz(A.S);  // (MW) S = 1 << sshift
  if constexpr (MW) {
    valid = true;
    sample = blockIdx.x;
    seg = 4 * wv + lp.b;
    cc = (long)sample * A.S + seg;
    n0 = (int)(((long)seg * A.N) >> sshift);
    n1 = (int)(((long)(seg + 1) * A.N) >> sshift);
  } else {
    long lblock = blockIdx.x;
    if ((gridDim.x & 7) == 0) lblock = (long)(blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    const long chain = lblock * 4 + lp.b;
    const long nchains = (long)A.B * A.S;
    valid = chain < nchains;
    cc = valid ? chain : nchains - 1;
    sample = (int)(cc / A.S);
    seg = (int)(cc - (long)sample * A.S);
    n0 = (int)(((long)seg * A.N) / A.S);
    n1 = (int)(((long)(seg + 1) * A.N) / A.S);
  }
  int len, tmax;
  // uneven segments (MW): the first S / 2 chains (waves 0 .. 3, the older wave of each SIMD) take `seg_long` slices each, the
  // others share the rest; the wave iterates over the longest of its four chains
  auto split_segments = [&](int seg_long) {
    if (MW && seg_long > 0) {
      const int h = A.S >> 1;
      const long rest = (long)A.N - (long)h * seg_long;
      n0 = seg < h ? seg * seg_long : h * seg_long + (int)(((long)(seg - h) * rest) >> (sshift - 1));
      n1 = seg + 1 <= h ? (seg + 1) * seg_long : h * seg_long + (int)(((long)(seg + 1 - h) * rest) >> (sshift - 1));
    }
    len = n1 - n0;
    tmax = A.Lmax;
    if (MW && seg_long > 0) {
      // (the four chains of a wave are the lanes i, i + 4, i + 8, i + 12 of a row)
      int m = len;
      m = max(m, __builtin_amdgcn_mov_dpp(m, DPP_ROR4, 0xf, 0xf, true));
      m = max(m, __builtin_amdgcn_mov_dpp(m, DPP_ROR8, 0xf, 0xf, true));
      tmax = __builtin_amdgcn_readfirstlane(m);
    }
  };
  split_segments(A.seg_long);

  // per-lane LDS offsets (doubles)
  const int woff = lp.b * IMG + lp.r * W + lp.c;
  const int roff = lp.b * IMG + (2 * (lp.c >> 1) + ((lp.c ^ lp.r) & 1)) * W + (lp.r >> 1);
  const unsigned negmask = (((lp.c & 1) == 0) && ((lp.r & 1) == 1)) ? 0x80000000u : 0u;
  const int toff = lp.r * W + lp.c;  // table read offset (D-layout)
  const int ddelta = (lp.r & 1) ? 1000 : ((lp.r >> 1) - lp.c);
  const int rhalf = lp.r >> 1;

  double U[NBI][NJ];
  double mus_r = 0.0, mus_i = 0.0;
  bool img_holds_U = false;      // the chains' images hold U (the real loops leave it there on their way back to the half-image layout)

  if constexpr (GIVEN) {
    // ---- ordered product of supplied matrices ----
    const double* base = reinterpret_cast<const double*>(A.mats) + ((long)sample * A.N + n0) * D * D * 2;
    for (int t = 0; t < tmax; ++t) {
      const bool act = valid && t < len;
      double P[NBI][NJ];
      const double* src = base + (long)(act ? t : 0) * D * D * 2;
#pragma unroll
      for (int I = 0; I < NBI; ++I)
#pragma unroll
        for (int J = 0; J < NJ; ++J) {
          const int row = 2 * I + (lp.r >> 1), col = 4 * J + lp.c;
          P[I][J] = (act && row < D && col < D) ? src[(row * D + col) * 2 + (lp.r & 1)] : 0.0;
        }
      if (t == 0) {
#pragma unroll
        for (int I = 0; I < NBI; ++I)
#pragma unroll
          for (int J = 0; J < NJ; ++J) U[I][J] = P[I][J];
      } else {
        double acc[NBI][NJ];
#pragma unroll
        for (int I = 0; I < NBI; ++I)
#pragma unroll
          for (int J = 0; J < NJ; ++J) acc[I][J] = 0.0;
        if (A.right_order) {
          write_image<D>(U, img, woff);
          mm_img<D>(img, roff, negmask, P, acc);
        } else {
          write_image<D>(P, img, woff);
          mm_img<D>(img, roff, negmask, U, acc);
        }
#pragma unroll
        for (int I = 0; I < NBI; ++I)
#pragma unroll
          for (int J = 0; J < NJ; ++J) U[I][J] = act ? acc[I][J] : U[I][J];
      }
    }
  } else {
    // ---- prologue: tables and this segment's control amplitudes into LDS ----
    // all four chains of a wave share the sample when tables are per sample (S % 4 == 0)
    double nrm = 0.0;
    bool realH = false, normalG = false;  // (supplied generators: neither)
    if constexpr (XG) {
      const double* mt = A.meta + ((long)sample * A.N + n0) * 4;
      for (int t = lp.idx16; t < A.Lmax; t += 16)
        if (valid && t < len) nrm = fmax(nrm, mt[(long)t * 4 + 2]);
      nrm = fmax(nrm, __shfl_xor(nrm, 1));
      nrm = fmax(nrm, __shfl_xor(nrm, 2));
      nrm = fmax(nrm, __shfl_xor(nrm, 16));
      nrm = fmax(nrm, __shfl_xor(nrm, 32));
      nrm = fmax(nrm, __shfl_xor(nrm, 4));
      nrm = fmax(nrm, __shfl_xor(nrm, 8));
    } else {
    // (MW: table k is built by wave k mod nwv; the barrier comes after the waves have fetched their control amplitudes)
    // The waves that build a table issue the loads of their control amplitudes FIRST (K <= 2, segments up to 48 slices: six
    // registers) -- both are the kernel's first, cold, global accesses and were serialised (4.0 + 1.0 us on wave 0 at cfg2)
    constexpr int PF_K = 2, PF_T = 3;
    const bool prefetch = MW && A.inline_tables && K <= PF_K && A.Lmax <= 16 * PF_T;
    double pre[PF_K][PF_T];
    if (prefetch) {
#pragma unroll
      for (int k = 0; k < PF_K; ++k)
#pragma unroll
        for (int i = 0; i < PF_T; ++i) {
          const int t = lp.idx16 + 16 * i;
          const double* sk = A.signals + ((long)sample * K + (k < K ? k : 0)) * A.N + n0;
          pre[k][i] = (k < K && valid && t < len) ? sk[t] : 0.0;
        }
    }
    // segment-wide bound on ||X||_1, column by column (c3p_sd_segment_col)  -> one plan per segment
    // (MW: the amplitudes are fetched, and the chains' max_t |c_k(t)| taken, while the tables are on their way: they need no
    // table.  The maxima of up to PF_K control lines wait in registers; beyond that they are read back from LDS)
    double cm[PF_K];
#pragma unroll
    for (int k = 0; k < PF_K; ++k) cm[k] = 0.0;
    const bool cm_regs = MW && K <= PF_K;
    auto seg_max = [&](int k, bool from_lds) {
      const double* s = A.signals + ((long)sample * K + k) * A.N + n0;
      double cmax = 0.0;
      for (int t = lp.idx16; t < A.Lmax; t += 16) {
        double v;
        if (from_lds) {
          v = sg[lp.b * SG + k * A.Lmax + t];
        } else {
          v = (valid && t < len) ? s[t] : 0.0;
          sg[lp.b * SG + k * A.Lmax + t] = v;
        }
        cmax = fmax(cmax, fabs(v));
      }
      return chain_max16(cmax);
    };
    auto keep_max = [&](int k, double m) {
#pragma unroll
      for (int q = 0; q < PF_K; ++q)
        if (k == q) cm[q] = m;
    };
    // (MW) the segment's amplitudes into the wave's LDS rows, their maxima into cm
    auto fetch_amplitudes = [&]() {
      if (prefetch) {
#pragma unroll
        for (int k = 0; k < PF_K; ++k) {
          double m = 0.0;
#pragma unroll
          for (int i = 0; i < PF_T; ++i) {
            const int t = lp.idx16 + 16 * i;
            if (k < K && t < A.Lmax) sg[lp.b * SG + k * A.Lmax + t] = pre[k][i];
            m = fmax(m, fabs(pre[k][i]));  // (zero past the segment's end)
          }
          cm[k] = chain_max16(m);
        }
      } else {
        for (int k = 0; k < K; ++k) keep_max(k, seg_max(k, false));
      }
    };
    if (A.record != nullptr) {
      // The model record (smalld_record_kernel): the block build_tables leaves in LDS, formed once per model -- the tables with
      // their four trailing words, then the column sums.  Every thread of the workgroup takes its share.  The first RU loads of a
      // thread are issued together and stand directly behind the amplitude prefetch (all of them cold): nothing is waited for in
      // between, and the amplitudes, issued first, are stored while the record is still on its way.
      constexpr int RU = MW ? 2 : 8;
      const int T = (1 + K) * (MAT + 4), R = T + (1 + K) * SD_CSW;
      const int tid = MW ? (int)threadIdx.x : lane, rstep = 64 * nwv;
      auto put = [&](int e, double v) {
        if (e < T)
          tab[e] = v;
        else if (e < R)
          csb[e - T] = v;
      };
      double rv[RU];
#pragma unroll
      for (int q = 0; q < RU; ++q) rv[q] = A.record[min(tid + q * rstep, R - 1)];
      if constexpr (MW) fetch_amplitudes();
#pragma unroll
      for (int q = 0; q < RU; ++q) put(tid + q * rstep, rv[q]);
      for (int e0 = tid + RU * rstep; e0 < R; e0 += RU * rstep) {  // (more than RU x the workgroup's threads: K > 2 or one wave)
#pragma unroll
        for (int q = 0; q < RU; ++q) rv[q] = A.record[min(e0 + q * rstep, R - 1)];
#pragma unroll
        for (int q = 0; q < RU; ++q) put(e0 + q * rstep, rv[q]);
      }
    } else if (A.inline_tables) {
      build_tables<D>(A, __builtin_amdgcn_readfirstlane(sample), tab, csb, lane, wv, nwv, [&]() {
        if constexpr (MW) fetch_amplitudes();
      });
    } else {
      const double* gt0 = A.tables + (long)(A.tab_per_sample ? sample : 0) * (1 + K) * (MAT + 4);
      for (int e = (MW ? (int)threadIdx.x : lane); e < (1 + K) * (MAT + 4); e += 64 * nwv) tab[e] = gt0[e];
      if constexpr (MW) fetch_amplitudes();
      // tables of the prep kernel: their column sums are formed here, from the copy in LDS and dealt to the waves as a table
      // build is (the barriers below publish the block)
      __syncthreads();
      sd_colsums<D>(tab, K, csb, lane, wv, nwv);
    }
    SD_TICK(tk8);  // `tables`: this wave's share of the tables and column sums is in LDS -- built here, or copied from the model record
    SD_TICK(tk9);
    __syncthreads();  // the tables and their column sums are in place
    // The flags of the K + 1 tables, read ONCE and without an early exit (the reads of the first PF_K + 1 are independent):
    // every table purely imaginary (flag 0: real Hamiltonians) -> real fast path; every table skew-Hermitian to rounding (flag
    // <= 0; negative: complex skew-Hermitian) -> the schemes for normal generators
    bool all_real = true, all_normal = true;
    {
      double f[PF_K + 1];
#pragma unroll
      for (int q = 0; q <= PF_K; ++q) f[q] = tab[min(q, K) * (MAT + 4) + MAT + 3];
#pragma unroll
      for (int q = 0; q <= PF_K; ++q) all_real = all_real & (f[q] == 0.0), all_normal = all_normal & (f[q] <= 0.0);
      for (int k = PF_K + 1; k <= K; ++k) {
        const double fk = tab[k * (MAT + 4) + MAT + 3];
        all_real = all_real & (fk == 0.0), all_normal = all_normal & (fk <= 0.0);
      }
    }
    realH = __builtin_amdgcn_readfirstlane((int)((A.mode == C3P_MODE_UNITARY) && all_real)) != 0;
    normalG = (A.mode == C3P_MODE_UNITARY) && !(A.no_t18n & 1) && all_normal;
    if constexpr (MW) {
      // a sample on the COMPLEX loop has its own split (the two waves of a SIMD finish together at a different ratio there): the
      // table flags are known only now, so its waves fetch their amplitudes a second time (~1 us of a 285 us kernel)
      if (A.seg_long_c > 0 && A.seg_long_c != A.seg_long && !realH) {
        wave_sync();
        split_segments(A.seg_long_c);
        for (int k = 0; k < K; ++k) keep_max(k, seg_max(k, false));
        wave_sync();
      }
    }
    {
      double col[1] = {c3p_sd_segment_col(csb, K, lp.idx16, [&](int k) {
        static_assert(PF_K == 2, "the select below reads cm[0] and cm[1]");
        if (cm_regs) return k == 0 ? cm[0] : cm[1];
        return seg_max(k, MW);
      })};
      wave_max64(col);  // over the columns of a chain and over the wave's four chains
      nrm = col[0];
    }
    }
    nrm = readfirstlane_f64(nrm);
    // plan of the complex loop (not evaluated on the real path: its threshold loops cost ~0.5 us of a workgroup's prologue).
    // (round 6) Hermitian Hamiltonians -- every table flagged skew-Hermitian -- take the schemes for normal generators
    MfmaPlan plan = {0, 0, 0};
    int t18n = 0;
    if (!realH) {
      t18n = __builtin_amdgcn_readfirstlane((int)normalG);
      plan = c3p_pick_plan_mfma(nrm, t18n ? C3P_T18N_THETA : C3P_T18_THETA, t18n != 0 && !(A.no_t18n & 2));
    }
    const int pr = __builtin_amdgcn_readfirstlane(plan.r);
    const int ps = __builtin_amdgcn_readfirstlane(plan.s);
    const int t18 = __builtin_amdgcn_readfirstlane(plan.t18);
    const double scale = ldexp(1.0, -ps);
    // Behind the barrier above a wave reads the tables and the column sums, which nothing writes again, and reads and writes its
    // own images and amplitude rows.  Workgroup per sample: no second barrier (the next is the one in front of the final fold).
    // One wave: the column sums stand in the wave's images, and this one keeps the loop's image writes behind their reads.
    if constexpr (!MW) __syncthreads();
    SD_TICK(tk1);

    if (realH) {
      constexpr int NB = RD<D>::NB;
      typedef double RMat[NB][NB];
      // Both loops below evaluate the economised cos / sin pairs of c3p_common.h (Y is real symmetric, so the polynomial error on
      // [0, theta^2] IS the matrix error), scaled against the radius of the degree-8 pair.
      const int ps_r = __builtin_amdgcn_readfirstlane(c3p_squarings(nrm, C3P_MM8_THETA));
      const double rscale = ldexp(1.0, -ps_r);
      const int swap_lane = 16 * lp.c + 4 * lp.b + lp.r;  // (r, c) <-> (c, r) inside the chain's block
      const int tail_lane = 16 * lp.c + 4 * lp.b;         // lane (c, 0): source of the rank-1 tail's row vector
      const int row0_lane = 4 * lp.b + lp.c;               // lane (0, c): row D-1 of a general right operand
      RMat Ur, Ui;  // the chain state in real blocks
      int yo[NB];        // Im rows of the half-image tables hold -Y
      double ymask[NB];
#pragma unroll
      for (int I = 0; I < NB; ++I) {
        const bool ok = 4 * I + lp.r < D;
        yo[I] = (2 * (ok ? 4 * I + lp.r : 0) + 1) * W + lp.c;
        ymask[I] = ok ? 1.0 : 0.0;
      }
      if constexpr (SPLIT) {
        // ---- core + border form (D = 4 NC + 1; see SMat / GMat above): the same polynomial evaluation and chain step ----
        static_assert(!SPLIT || (D % 4 == 1 && D > 4 && !DUS), "core + border form: D = 5, 9 without slice output");
        constexpr int NC = (D - 1) / 4;
        typedef SMat<NC> SM;
        GMat<NC> Gr, Gi;  // the chain state: core and row border in real blocks,
        GBorder<NC> Gb;   // column border and corner packed
        int so[NC], sro[NC], sco[NC];
#pragma unroll
        for (int I = 0; I < NC; ++I) {
          so[I] = (2 * (4 * I + lp.r) + 1) * W + lp.c;
          sro[I] = (2 * (4 * I + lp.r) + 1) * W + (D - 1);
          sco[I] = (2 * (4 * I + lp.c) + 1) * W + (D - 1);
        }
        constexpr int sso = (2 * (D - 1) + 1) * W + (D - 1);
        // A scaled norm below C3P_MM6_THETA (cfg2: 0.81) takes the degree-6 pair: W, W^2, W^3, ONE paired Horner step in W^3,
        // sin = (sin Y / Y) Y -- 6 products at dependency depth 5; above it the degree-8 pair with W^4 (7 products).  The form is
        // chosen per segment OUTSIDE the slice loop (the loop is instantiated twice) so that neither form's registers burden the
        // other's schedule.
        const bool deg6 = __builtin_amdgcn_readfirstlane((int)(nrm * rscale <= C3P_MM6_THETA)) != 0;
        // Per-segment weights: the amplitudes of the segment are rewritten ONCE as a_k(t) = -rscale c_k(t), with one more row
        // a_0(t) = -rscale on the segment's slices and 0 on the padded slots of a wave's shorter chains (Y = 0, E = I), so that a
        // slice is Y = a_0 T_0 + sum_k a_k T_k: one multiply and K multiply-adds per value, no factors and no masks in the loop.
        // The trace shift of the segment, sum_n mu_i(n) = len mu_0 + sum_k mu_k sum_t c_k(t) (mu_r = 0 for every table of a real
        // Hamiltonian: build_tables), needs the amplitudes alone and is formed here as well, reduced as the loops reduce it.
        {
          double ph = 0.0;
          for (int k = 0; k < K; ++k) {
            const double mk = tab[(k + 1) * (MAT + 4) + MAT + 1];
            for (int t = lp.idx16; t < A.Lmax; t += 16) {
              const double c0 = sg[lp.b * SG + k * A.Lmax + t];  // zero past the segment's end
              ph = c3p_phase_add(ph, c0 * mk);
              sg[lp.b * SG + k * A.Lmax + t] = -rscale * c0;
            }
          }
          if (K > 0)
            for (int t = lp.idx16; t < A.Lmax; t += 16) sg[lp.b * SG + K * A.Lmax + t] = (valid && t < len) ? -rscale : 0.0;
          // (lane ^ 1, 2, 16, 32 in this order on the register path: c3p_phase_add depends on acc + inc alone, so it commutes and
          // both lanes of a pair form the same bits)
          double pa, pb;
          ph = c3p_phase_add(ph, dpp_f64<DPP_XOR1>(ph));
          ph = c3p_phase_add(ph, dpp_f64<DPP_XOR2>(ph));
          pair_xor16(ph, pa, pb);
          ph = c3p_phase_add(pa, pb);
          pair_xor32(ph, pa, pb);
          ph = c3p_phase_add(pa, pb);
          mus_i = c3p_phase_add(ph, (double)(valid ? len : 0) * c3p_phase_add(0.0, tab[MAT + 1]));
          wave_sync();
        }
        // The slots t < tfast are real slices of all four chains of the wave (the chains of a wave differ by at most one slice, so
        // at most the last slot is padding for some of them)
        int tfast = valid ? len : 0;
        tfast = min(tfast, __builtin_amdgcn_mov_dpp(tfast, DPP_ROR4, 0xf, 0xf, true));
        tfast = min(tfast, __builtin_amdgcn_mov_dpp(tfast, DPP_ROR8, 0xf, 0xf, true));
        tfast = min(__builtin_amdgcn_readfirstlane(tfast), tmax);
        // One slice: E = cos Y - i sin Y as Cm = cos Y and acc = sin Y, both in left-operand form.
        //   WEIGHTED: Y = a_0 T_0 + sum_k a_k T_k with the a_0 row (a padded slot gives Y = 0, E = I).  Otherwise the slot is a real
        //     slice of a segment without squarings: rscale = 1, so a_0 T_0 = -T_0 exactly and the drift is the negated addend of the
        //     first multiply-add -- no a_0, no multiplies.
        //   SQ: the ps_r squarings follow.  vc: fetch the c-form borders of Cm and acc, which only the squarings and the first slice
        //     of a segment read (a constant at every call but the run-time-K one).
        auto slice_exp = [&](int t, auto deg6_tag, auto k_tag, auto weighted_tag, auto sq_tag, bool vc, SM& Cm, SM& acc) {
          constexpr bool DEG6 = decltype(deg6_tag)::value;  // true = the degree-6 pair, false = the degree-8 pair
          constexpr int KC = decltype(k_tag)::value;        // K at compile time (0 .. 2); -1 = the run-time loop over the tables
          constexpr bool WEIGHTED = decltype(weighted_tag)::value, SQ = decltype(sq_tag)::value;
          static_assert(WEIGHTED || (KC >= 0 && !SQ), "the unweighted drift is the form of compile-time K without squarings");
          const double* ap = sg + lp.b * SG;
          SM Y;
          if constexpr (WEIGHTED) {
            // (K = 0 has no amplitude rows: the drift weight comes from the slot's mask)
            const double a0 = (KC == 0 || (KC < 0 && K == 0)) ? ((valid && t < len) ? -rscale : 0.0) : ap[K * A.Lmax + t];
#pragma unroll
            for (int I = 0; I < NC; ++I) {
#pragma unroll
              for (int J = 0; J < NC; ++J) Y.m[I][J] = a0 * lds_ld(tab + so[I] + J * 4);
              Y.vr[I] = a0 * lds_ld(tab + sro[I]);
              Y.vc[I] = a0 * lds_ld(tab + sco[I]);
            }
            Y.s = a0 * lds_ld(tab + sso);
          } else if constexpr (KC == 0) {
#pragma unroll
            for (int I = 0; I < NC; ++I) {
#pragma unroll
              for (int J = 0; J < NC; ++J) Y.m[I][J] = -lds_ld(tab + so[I] + J * 4);
              Y.vr[I] = -lds_ld(tab + sro[I]);
              Y.vc[I] = -lds_ld(tab + sco[I]);
            }
            Y.s = -lds_ld(tab + sso);
          } else {
            const double a1 = ap[t];
            const double* t1 = tab + (MAT + 4);
#pragma unroll
            for (int I = 0; I < NC; ++I) {
#pragma unroll
              for (int J = 0; J < NC; ++J) Y.m[I][J] = fma(a1, lds_ld(t1 + so[I] + J * 4), -lds_ld(tab + so[I] + J * 4));
              Y.vr[I] = fma(a1, lds_ld(t1 + sro[I]), -lds_ld(tab + sro[I]));
              Y.vc[I] = fma(a1, lds_ld(t1 + sco[I]), -lds_ld(tab + sco[I]));
            }
            Y.s = fma(a1, lds_ld(t1 + sso), -lds_ld(tab + sso));
          }
          auto add_table = [&](int k) {
            const double ak = ap[k * A.Lmax + t];
            const double* tk = tab + (k + 1) * (MAT + 4);
#pragma unroll
            for (int I = 0; I < NC; ++I) {
#pragma unroll
              for (int J = 0; J < NC; ++J) Y.m[I][J] = fma(ak, lds_ld(tk + so[I] + J * 4), Y.m[I][J]);
              Y.vr[I] = fma(ak, lds_ld(tk + sro[I]), Y.vr[I]);
              Y.vc[I] = fma(ak, lds_ld(tk + sco[I]), Y.vc[I]);
            }
            Y.s = fma(ak, lds_ld(tk + sso), Y.s);
          };
          if constexpr (KC >= 0) {
#pragma unroll
            for (int k = WEIGHTED ? 0 : 1; k < KC; ++k) add_table(k);
          } else {
            for (int k = 0; k < K; ++k) add_table(k);
          }
          SM W1, W2, W3, Sp, acs;
          s8_zero(W1), s8_zero(W2), s8_zero(W3);
          mm_s8(Y, Y, W1);  // W = Y^2
          s8_finish(W1, swap_lane, tail_lane);
          mm_s8(W1, W1, W2);  // W^2
          s8_finish(W2, swap_lane, tail_lane);
          // The Horner factors are the LEFT operands of the paired product (everything commutes): they are combined on the 6
          // registers a product accumulates into (upper core tiles, r-form border, corner) and completed by ONE lane swap each;
          // the shared right operand (W^3 / W^4) is completed in full; a power that is never a product operand is not completed.
          if constexpr (DEG6) {
            // degree 6: cos = (c0 + c1 W + c2 W^2) + W^3 (c3 + c4 W + c5 W^2 + c6 W^3)
            mm_s8(W1, W2, W3);
            s8_finish(W3, swap_lane, tail_lane);
            s8_comb<NC, true, true>(acc, c3p_mm6_cos[3], c3p_mm6_cos[4], c3p_mm6_cos[5], c3p_mm6_cos[6], W1, W2, W3, lp);
            s8_comb<NC, true, true>(acs, c3p_mm6_sinc[3], c3p_mm6_sinc[4], c3p_mm6_sinc[5], c3p_mm6_sinc[6], W1, W2, W3, lp);
            s8_finish_lower(acc, swap_lane);
            s8_finish_lower(acs, swap_lane);
            s8_comb<NC, false, true>(Cm, c3p_mm6_cos[0], c3p_mm6_cos[1], c3p_mm6_cos[2], 0.0, W1, W2, W3, lp);
            s8_comb<NC, false, true>(Sp, c3p_mm6_sinc[0], c3p_mm6_sinc[1], c3p_mm6_sinc[2], 0.0, W1, W2, W3, lp);
            mm_s8x2r(acc, acs, W3, Cm, Sp);  // Cm = cos Y, Sp = sin(Y) / Y
          } else {
            // degree 8: cos = (c0 + c1 W + c2 W^2 + c3 W^3) + W^4 (c4 + c5 W + c6 W^2 + c7 W^3 + c8 W^4); W^3 is not a product operand
            SM W4;
            s8_zero(W4);
            mm_s8(W1, W2, W3);
            mm_s8(W2, W2, W4);
            s8_finish(W4, swap_lane, tail_lane);
            s8_comb<NC, true, true>(acc, c3p_mm8_cos[4], c3p_mm8_cos[5], c3p_mm8_cos[6], c3p_mm8_cos[7], W1, W2, W3, lp);
            s8_comb<NC, true, true>(acs, c3p_mm8_sinc[4], c3p_mm8_sinc[5], c3p_mm8_sinc[6], c3p_mm8_sinc[7], W1, W2, W3, lp);
#pragma unroll
            for (int I = 0; I < NC; ++I) {
#pragma unroll
              for (int J = I; J < NC; ++J) {
                acc.m[I][J] = fma(c3p_mm8_cos[8], W4.m[I][J], acc.m[I][J]);
                acs.m[I][J] = fma(c3p_mm8_sinc[8], W4.m[I][J], acs.m[I][J]);
              }
              acc.vr[I] = fma(c3p_mm8_cos[8], W4.vr[I], acc.vr[I]);
              acs.vr[I] = fma(c3p_mm8_sinc[8], W4.vr[I], acs.vr[I]);
            }
            acc.s = fma(c3p_mm8_cos[8], W4.s, acc.s);
            acs.s = fma(c3p_mm8_sinc[8], W4.s, acs.s);
            s8_finish_lower(acc, swap_lane);
            s8_finish_lower(acs, swap_lane);
            s8_comb<NC, true, true>(Cm, c3p_mm8_cos[0], c3p_mm8_cos[1], c3p_mm8_cos[2], c3p_mm8_cos[3], W1, W2, W3, lp);
            s8_comb<NC, true, true>(Sp, c3p_mm8_sinc[0], c3p_mm8_sinc[1], c3p_mm8_sinc[2], c3p_mm8_sinc[3], W1, W2, W3, lp);
            mm_s8x2r(acc, acs, W4, Cm, Sp);  // Cm = cos Y, Sp = sin(Y) / Y
          }
          // cos Y, sin Y / Y and sin Y are LEFT operands from here on (sin Y = (sin Y / Y) Y, the chain step): lower tiles only;
          // their c-form borders are only fetched for the squarings and the first slice of a segment
          s8_finish_lower(Cm, swap_lane);
          s8_finish_lower(Sp, swap_lane);
          s8_zero(acc);
          mm_s8(Sp, Y, acc);  // acc = sin Y
          s8_finish_lower(acc, swap_lane);
          if (vc) {
            s8_finish_vc(Cm, tail_lane);
            s8_finish_vc(acc, tail_lane);
          }
          // squarings: cos 2Y = (C - S)(C + S), sin 2Y = 2 S C
          if constexpr (SQ) {
            for (int it = 0; it < ps_r; ++it) {
              SM Dm, Sm, C2, SC;
#pragma unroll
              for (int I = 0; I < NC; ++I) {
#pragma unroll
                for (int J = 0; J < NC; ++J) {
                  Dm.m[I][J] = Cm.m[I][J] - acc.m[I][J];
                  Sm.m[I][J] = Cm.m[I][J] + acc.m[I][J];
                }
                Dm.vr[I] = Cm.vr[I] - acc.vr[I];
                Sm.vr[I] = Cm.vr[I] + acc.vr[I];
                Dm.vc[I] = Cm.vc[I] - acc.vc[I];
                Sm.vc[I] = Cm.vc[I] + acc.vc[I];
              }
              Dm.s = Cm.s - acc.s;
              Sm.s = Cm.s + acc.s;
              s8_zero(C2), s8_zero(SC);
              mm_s8(Dm, Sm, C2);
              mm_s8(acc, Cm, SC);
#pragma unroll
              for (int I = 0; I < NC; ++I) {
#pragma unroll
                for (int J = I; J < NC; ++J) {
                  Cm.m[I][J] = C2.m[I][J];
                  acc.m[I][J] = 2.0 * SC.m[I][J];
                }
                Cm.vr[I] = C2.vr[I];
                acc.vr[I] = 2.0 * SC.vr[I];
              }
              Cm.s = C2.s;
              acc.s = 2.0 * SC.s;
              s8_finish(Cm, swap_lane, tail_lane);
              s8_finish(acc, swap_lane, tail_lane);
            }
          }
        };
        // The slices t0 .. t1 - 1 of a segment whose first slice is in the state: exponential + chain step, one basic block per slice
        auto step_loop = [&](int t0, int t1, auto deg6_tag, auto k_tag, auto weighted_tag, auto sq_tag, bool vc) {
          for (int t = t0; t < t1; ++t) {
            SM Cm, acc;
            slice_exp(t, deg6_tag, k_tag, weighted_tag, sq_tag, vc, Cm, acc);
            chain_step8(Cm, acc, Gr, Gi, Gb);
          }
        };
        // All choices are made per segment OUTSIDE the slice loop.  The first slice is peeled: U <- E = C - i S, the one place a
        // segment without squarings needs the c-form borders; it goes through the weighted run-time-K form (once per segment, and a
        // single copy per degree).  Then, with compile-time K = 0 .. 2:
        //   ps_r == 0: the slots that are real for the whole wave in the unweighted form without squarings; a padded last slot is
        //              left to the weighted run-time-K loop (a_0 = 0 where the chain has ended);
        //   ps_r > 0:  the weighted form with its squarings.
        // K > 2 keeps the weighted run-time loop over the tables for either (one copy per degree, zero trips otherwise).
        auto split_loop_k = [&](auto deg6_tag) {
          constexpr std::true_type yes{};
          constexpr std::false_type no{};
          constexpr std::integral_constant<int, -1> krt{};
          {
            SM Cm, acc;
            slice_exp(0, deg6_tag, krt, yes, yes, true, Cm, acc);
#pragma unroll
            for (int I = 0; I < NC; ++I) {
#pragma unroll
              for (int J = 0; J < NC; ++J) {
                Gr.m[I][J] = Cm.m[I][J];
                Gi.m[I][J] = -acc.m[I][J];
              }
              Gr.rc[I] = Cm.vc[I];
              Gi.rc[I] = -acc.vc[I];
              Gb.Pc[I] = border_pack(Cm.vr[I], -acc.vr[I], lp.c);
            }
            Gb.Ps = border_pack(Cm.s, -acc.s, lp.c);
          }
          int t0 = 1;  // first slot left to the run-time-K loop
          auto split_loop = [&](auto k_tag) {
            if (ps_r == 0) {
              step_loop(1, tfast, deg6_tag, k_tag, no, no, false);
              t0 = max(tfast, 1);
            } else {
              step_loop(1, tmax, deg6_tag, k_tag, yes, yes, true);
              t0 = tmax;
            }
          };
          if (K == 2)
            split_loop(std::integral_constant<int, 2>{});
          else if (K == 1)
            split_loop(std::integral_constant<int, 1>{});
          else if (K == 0)
            split_loop(std::integral_constant<int, 0>{});
          step_loop(t0, tmax, deg6_tag, krt, yes, yes, ps_r > 0);
        };
        if (deg6)
          split_loop_k(std::true_type{});
        else
          split_loop_k(std::false_type{});
        SD_TICK(tkl);
        // back to the complex half-image layout of the epilogue (once per segment, through the chain's image, which stays behind
        // as the left operand of the fold's first product).  Only the padding is zeroed: rows 2 D, 2 D + 1 and columns D .. 4 NJ - 1.
        wave_sync();
        if (lp.idx16 < 4 * NJ) img[lp.b * IMG + 2 * D * W + lp.idx16] = img[lp.b * IMG + (2 * D + 1) * W + lp.idx16] = 0.0;
        for (int e = lp.idx16; e < 2 * D * (4 * NJ - D); e += 16) img[lp.b * IMG + (e / (4 * NJ - D)) * W + D + e % (4 * NJ - D)] = 0.0;
#pragma unroll
        for (int I = 0; I < NC; ++I) {
          const int i = 4 * I + lp.r;
#pragma unroll
          for (int J = 0; J < NC; ++J) {
            img[lp.b * IMG + (2 * i) * W + 4 * J + lp.c] = Gr.m[I][J];
            img[lp.b * IMG + (2 * i + 1) * W + 4 * J + lp.c] = Gi.m[I][J];
          }
          // (packed column border: the lanes c = 0 and c = 1 hold Re and Im)
          if (lp.c < 2) img[lp.b * IMG + (2 * i + lp.c) * W + D - 1] = Gb.Pc[I];
          if (lp.r == 0) {
            img[lp.b * IMG + (2 * (D - 1)) * W + 4 * I + lp.c] = Gr.rc[I];
            img[lp.b * IMG + (2 * (D - 1) + 1) * W + 4 * I + lp.c] = Gi.rc[I];
          }
        }
        if (lp.r == 0 && lp.c < 2) img[lp.b * IMG + (2 * (D - 1) + lp.c) * W + D - 1] = Gb.Ps;
        wave_sync();
#pragma unroll
        for (int I = 0; I < NBI; ++I)
#pragma unroll
          for (int J = 0; J < NJ; ++J) U[I][J] = img[woff + I * 4 * W + J * 4];
        wave_sync();
        img_holds_U = true;
      } else {
      for (int t = 0; t < tmax; ++t) {
        // (Two waves share a SIMD and the arbiter serves the OLDER one first: wave w finishes its segment at ~64 % of the
        // kernel time and wave w + 4 then runs alone -- wall_clock64 probes, -DC3P_SD_TIMING.  Alternating s_setprio per
        // slice makes them finish together and changes nothing in the total: measured, not kept.)
        const bool act = valid && t < len;
        const double sc = act ? rscale : 0.0;
        const double muw = act ? 1.0 : 0.0;
        double mu_r = muw * tab[MAT + 0], mu_i = muw * tab[MAT + 1];
        // ---- Y = scale dt (H - tr H / D) = -Im(G0 + sum_k c_k G_k) ----
        // (rows past the table are clamped to a valid row and masked: no exec-mask branches around LDS loads)
        RMat Y;
#pragma unroll
        for (int I = 0; I < NB; ++I) {
          const double f = -sc * ymask[I];
#pragma unroll
          for (int J = 0; J < NB; ++J) Y[I][J] = f * lds_ld(tab + yo[I] + J * 4);
        }
        for (int k = 0; k < K; ++k) {
          const double c0 = sg[lp.b * SG + k * A.Lmax + t];
          const double ck = sc * c0;
          const double* tk = tab + (k + 1) * (MAT + 4);
          mu_r = fma(c0, tk[MAT + 0], mu_r);
          mu_i = fma(c0, tk[MAT + 1], mu_i);
#pragma unroll
          for (int I = 0; I < NB; ++I) {
            const double f = -ck * ymask[I];
#pragma unroll
            for (int J = 0; J < NB; ++J) Y[I][J] = fma(f, lds_ld(tk + yo[I] + J * 4), Y[I][J]);
          }
        }
        RMat W1, W2, W3, Cm, Sp, acc, acs;
#pragma unroll
        for (int I = 0; I < NB; ++I)
#pragma unroll
          for (int J = 0; J < NB; ++J) W1[I][J] = W2[I][J] = W3[I][J] = 0.0;
        mm_sym<D>(Y, Y, W1, tail_lane);  // W = Y^2
        sym_fill<D>(W1, swap_lane);
        mm_sym<D>(W1, W1, W2, tail_lane);  // W^2
        sym_fill<D>(W2, swap_lane);
        // the degree-8 pair (c3p_mm8_cos / c3p_mm8_sinc), Paterson-Stockmeyer with q = 4: W^3 = W W^2 and W^4 = W^2 W^2 are
        // independent, then ONE paired Horner step  P = B0 + W^4 (B1 + c8 W^4): 7 products, dependency depth 5
        // (Y^2, W^2, {W^3, W^4}, {cos, sin/Y}, sin)
        RMat W4;
#pragma unroll
        for (int I = 0; I < NB; ++I)
#pragma unroll
          for (int J = 0; J < NB; ++J) W4[I][J] = 0.0;
        mm_sym<D>(W1, W2, W3, tail_lane);
        mm_sym<D>(W2, W2, W4, tail_lane);
        sym_fill<D>(W3, swap_lane);
        sym_fill<D>(W4, swap_lane);
        rcomb<D, true>(acc, c3p_mm8_cos[4], c3p_mm8_cos[5], c3p_mm8_cos[6], c3p_mm8_cos[7], W1, W2, W3, lp);
        rcomb<D, true>(acs, c3p_mm8_sinc[4], c3p_mm8_sinc[5], c3p_mm8_sinc[6], c3p_mm8_sinc[7], W1, W2, W3, lp);
#pragma unroll
        for (int I = 0; I < NB; ++I)
#pragma unroll
          for (int J = sym_j0<D>(I); J < NB; ++J) {
            acc[I][J] = fma(c3p_mm8_cos[8], W4[I][J], acc[I][J]);
            acs[I][J] = fma(c3p_mm8_sinc[8], W4[I][J], acs[I][J]);
          }
        rcomb<D, true, true>(Cm, c3p_mm8_cos[0], c3p_mm8_cos[1], c3p_mm8_cos[2], c3p_mm8_cos[3], W1, W2, W3, lp);
        rcomb<D, true, true>(Sp, c3p_mm8_sinc[0], c3p_mm8_sinc[1], c3p_mm8_sinc[2], c3p_mm8_sinc[3], W1, W2, W3, lp);
        mm_sym2<D>(W4, acc, Cm, acs, Sp, tail_lane);  // Cm = cos Y, Sp = sin(Y) / Y
        sym_fill<D>(Cm, swap_lane);
        sym_fill<D>(Sp, swap_lane);
#pragma unroll
        for (int I = 0; I < NB; ++I)
#pragma unroll
          for (int J = 0; J < NB; ++J) acc[I][J] = 0.0;
        mm_sym<D>(Y, Sp, acc, tail_lane);  // acc = sin Y
        sym_fill<D>(acc, swap_lane);
        // ---- E = cos Y - i sin Y (Cm, acc) ; squarings in real form.  C and S are polynomials in Y and commute:
        //      cos 2Y = C^2 - S^2 = (C - S)(C + S) (ONE product, symmetric result), sin 2Y = 2 S C ----
        for (int it = 0; it < ps_r; ++it) {
          RMat Dm, Sm, C2, SC;
#pragma unroll
          for (int I = 0; I < NB; ++I)
#pragma unroll
            for (int J = sym_j0<D>(I); J < NB; ++J) {
              Dm[I][J] = Cm[I][J] - acc[I][J];
              Sm[I][J] = Cm[I][J] + acc[I][J];
              C2[I][J] = SC[I][J] = 0.0;
            }
          mm_sym<D>(Dm, Sm, C2, tail_lane);
          mm_sym<D>(acc, Cm, SC, tail_lane);
#pragma unroll
          for (int I = 0; I < NB; ++I)
#pragma unroll
            for (int J = I; J < NB; ++J) {
              Cm[I][J] = C2[I][J];
              acc[I][J] = 2.0 * SC[I][J];
            }
          sym_fill<D>(Cm, swap_lane);
          sym_fill<D>(acc, swap_lane);
        }
        if (DUS || t == 0) {  // the whole matrices leave the symmetric stage: dU output / U <- E
          sym_fill_rest<D>(Cm, swap_lane);
          sym_fill_rest<D>(acc, swap_lane);
        }
        if constexpr (DUS) {
          // dU = e^{mu} (C - iS)
          double sn, cs;
          sincos(mu_i, &sn, &cs);
          const double er = exp(mu_r);
          const double pr = er * cs, pi = er * sn;
          double* dst = reinterpret_cast<double*>(A.dUs_out) + ((long)sample * A.N + n0 + (act ? t : 0)) * D * D * 2;
#pragma unroll
          for (int I = 0; I < NB; ++I)
#pragma unroll
            for (int J = 0; J < NB; ++J) {
              const int i = 4 * I + lp.r, j = 4 * J + lp.c;
              if (act && i < D && j < D) {
                dst[(i * D + j) * 2 + 0] = fma(pr, Cm[I][J], pi * acc[I][J]);
                dst[(i * D + j) * 2 + 1] = fma(pi, Cm[I][J], -pr * acc[I][J]);
              }
            }
        }
        // ---- chain in real blocks (no LDS): Ur' = C Ur + S Ui,  Ui' = C Ui - S Ur ----
        if (t == 0) {
#pragma unroll
          for (int I = 0; I < NB; ++I)
#pragma unroll
            for (int J = 0; J < NB; ++J) {
              Ur[I][J] = Cm[I][J];
              Ui[I][J] = -acc[I][J];
            }
          mus_r = mu_r;
          mus_i = c3p_phase_add(0.0, mu_i);
        } else {
          // (C - iS)(Ur + i Ui) with three real products: T1 = C Ur, T2 = S Ui, T3 = (C - S)(Ur + Ui);
          // Re = T1 + T2, Im = T3 - T1 + T2  (C - S is symmetric: its A fragments are registers, as for C and S)
          RMat Dm, Us, T1, T2, T3;
#pragma unroll
          for (int I = 0; I < NB; ++I)
#pragma unroll
            for (int J = 0; J < NB; ++J) {
              if (J >= sym_j0<D>(I)) Dm[I][J] = Cm[I][J] - acc[I][J];
              Us[I][J] = Ur[I][J] + Ui[I][J];
              T1[I][J] = T2[I][J] = T3[I][J] = 0.0;
            }
          mm_symA<D>(Cm, Ur, T1, row0_lane, 1.0);
          mm_symA<D>(acc, Ui, T2, row0_lane, 1.0);
          mm_symA<D>(Dm, Us, T3, row0_lane, 1.0);
#pragma unroll
          for (int I = 0; I < NB; ++I)
#pragma unroll
            for (int J = 0; J < NB; ++J) {
              Ur[I][J] = T1[I][J] + T2[I][J];
              Ui[I][J] = (T3[I][J] - T1[I][J]) + T2[I][J];
            }
          mus_r += mu_r;
          mus_i = c3p_phase_add(mus_i, mu_i);
        }
      }
      // back to the complex half-image layout of the epilogue (once per segment, through the chain's image)
      wave_sync();
#pragma unroll
      for (int I = 0; I < NB; ++I)
#pragma unroll
        for (int J = 0; J < NB; ++J) {
          const int i = 4 * I + lp.r, j = 4 * J + lp.c;
          if (2 * i + 1 < 4 * NBI) {
            img[lp.b * IMG + (2 * i) * W + j] = Ur[I][J];
            img[lp.b * IMG + (2 * i + 1) * W + j] = Ui[I][J];
          }
        }
      wave_sync();
#pragma unroll
      for (int I = 0; I < NBI; ++I)
#pragma unroll
        for (int J = 0; J < NJ; ++J) U[I][J] = img[woff + I * 4 * W + J * 4];
      wave_sync();
      img_holds_U = true;
      }  // !SPLIT
    } else {
    // the slice loop is instantiated per plan (T18 / Paterson-Stockmeyer) with the branch outside, as on the real path
    // (the 20 parameters as wave-uniform values loaded ONCE: read through the table inside the slice loop they were re-fetched per slice)
    const double* tc = c3p_t18_tab[t18n];
    const double t18_a11 = tc[C3P_I_A11];
    const double t18_a21 = tc[C3P_I_A21];
    const double t18_a31 = tc[C3P_I_A31];
    const double t18_b02 = tc[C3P_I_B02];
    const double t18_b03 = tc[C3P_I_B03];
    const double t18_b11 = tc[C3P_I_B11];
    const double t18_b12 = tc[C3P_I_B12];
    const double t18_b13 = tc[C3P_I_B13];
    const double t18_b21 = tc[C3P_I_B21];
    const double t18_b22 = tc[C3P_I_B22];
    const double t18_b23 = tc[C3P_I_B23];
    const double t18_b24 = tc[C3P_I_B24];
    const double t18_b31 = tc[C3P_I_B31];
    const double t18_b32 = tc[C3P_I_B32];
    const double t18_b33 = tc[C3P_I_B33];
    const double t18_b34 = tc[C3P_I_B34];
    const double t18_b61 = tc[C3P_I_B61];
    const double t18_b62 = tc[C3P_I_B62];
    const double t18_b63 = tc[C3P_I_B63];
    const double t18_b64 = tc[C3P_I_B64];
    auto complex_loop = [&](auto t18_tag) {
    constexpr int VARIANT = decltype(t18_tag)::value;  // 0 Paterson-Stockmeyer, 1 T18, 2 the four-product scheme (normal generators)
    constexpr bool T18 = VARIANT == 1;
    for (int t = 0; t < tmax; ++t) {
      const bool act = valid && t < len;
      // ---- X = scale (G0 + sum_k c_k G_k) in D-layout; trace shift mu ----
      // chains past their segment end (lengths differ by at most one slice) take X = 0, E = I
      double sc = act ? scale : 0.0;
      const double muw = act ? 1.0 : 0.0;
      double mu_r, mu_i;
      double X[NBI][NJ];
      int my_s = ps;  // squarings of THIS chain's matrix (supplied generators only)
      if constexpr (XG) {
        const long m = (long)sample * A.N + n0 + (act ? t : 0);
        // The polynomial and the loop count `ps` are the wave's (largest norm of its four chains); scaling and squaring are
        // the chain's own: a matrix of small norm next to a large one must not be scaled down further and squared more often
        // than its norm asks for -- every squaring doubles the rounding error of exp(X) = 1 + small (2^ps u instead of u).
        // my_s = the smallest count that brings this matrix inside the scaled norm the wave's plan was made for.
        {
          const double lim = nrm * scale;
          double scaled = A.meta[m * 4 + 2] * scale;
          while (my_s > 0 && 2.0 * scaled <= lim) {
            scaled *= 2.0;
            --my_s;
          }
          sc = act ? ldexp(1.0, -my_s) : 0.0;
        }
        mu_r = muw * A.meta[m * 4 + 0];
        mu_i = muw * A.meta[m * 4 + 1];
        const double2* src = reinterpret_cast<const double2*>(A.hs) + (long)sample * A.hs_bstride + (long)(n0 + (act ? t : 0)) * D * D;
        const double mine = (lp.r & 1) ? mu_i : mu_r;
#pragma unroll
        for (int I = 0; I < NBI; ++I)
#pragma unroll
          for (int J = 0; J < NJ; ++J) {
            const int row = 2 * I + (lp.r >> 1), col = 4 * J + lp.c;
            const bool in = row < D && col < D;
            const double2 h = src[in ? row * D + col : 0];
            double v = (lp.r & 1) ? fma(A.coef_r, h.y, A.coef_i * h.x) : fma(A.coef_r, h.x, -A.coef_i * h.y);
            v -= (row == col) ? mine : 0.0;
            X[I][J] = in ? sc * v : 0.0;
          }
      } else {
      mu_r = muw * tab[MAT + 0];
      mu_i = muw * tab[MAT + 1];
#pragma unroll
      for (int I = 0; I < NBI; ++I)
#pragma unroll
        for (int J = 0; J < NJ; ++J) X[I][J] = sc * tab[toff + I * 4 * W + J * 4];
      for (int k = 0; k < K; ++k) {
        const double c0 = sg[lp.b * SG + k * A.Lmax + t];
        const double ck = sc * c0;
        const double* tk = tab + (k + 1) * (MAT + 4);
        mu_r = fma(c0, tk[MAT + 0], mu_r);  // c0 = 0 for inactive slices (sg is zero padded)
        mu_i = fma(c0, tk[MAT + 1], mu_i);
#pragma unroll
        for (int I = 0; I < NBI; ++I)
#pragma unroll
          for (int J = 0; J < NJ; ++J) X[I][J] = fma(ck, tk[toff + I * 4 * W + J * 4], X[I][J]);
      }
      }
      write_image<D>(X, img, woff);
      // ---- powers with the left operand X (read from its image) ----
      double A2[NBI][NJ], A3[NBI][NJ], P[NBI][NJ];
#pragma unroll
      for (int I = 0; I < NBI; ++I)
#pragma unroll
        for (int J = 0; J < NJ; ++J) A2[I][J] = A3[I][J] = 0.0;
      mm_img<D>(img, roff, negmask, X, A2);
      if constexpr (VARIANT == 2) {
        // ---- four products (c3p_common.h, c3p_e4n): A2 above; y0 = A2 (e0 A2 + e1 X);
        //      y1 = (y0 + e2 A2 + e3 X)(y0 + e4 A2) + e5 y0 + e6 A2;
        //      P = (y1 + e7 A2 + e8 X)(y1 + e9 y0 + e10 X) + e11 y1 + e12 y0 + e13 A2 + e14 X + e15 I ----
        // (A3 holds y0)
        // (element loops with exactly the terms of each combination: 15 vector operations per element and slice)
        double y1[NBI][NJ];
        {
          double R[NBI][NJ];
#pragma unroll
          for (int I = 0; I < NBI; ++I)
#pragma unroll
            for (int J = 0; J < NJ; ++J) R[I][J] = fma(c3p_e4n[0], A2[I][J], c3p_e4n[1] * X[I][J]);
          write_image<D>(A2, img, woff);
          mm_img<D>(img, roff, negmask, R, A3);
        }
        {
          double L[NBI][NJ], R[NBI][NJ];
#pragma unroll
          for (int I = 0; I < NBI; ++I)
#pragma unroll
            for (int J = 0; J < NJ; ++J) L[I][J] = fma(c3p_e4n[2], A2[I][J], fma(c3p_e4n[3], X[I][J], A3[I][J]));
          write_image<D>(L, img, woff);
#pragma unroll
          for (int I = 0; I < NBI; ++I)
#pragma unroll
            for (int J = 0; J < NJ; ++J) {
              R[I][J] = fma(c3p_e4n[4], A2[I][J], A3[I][J]);
              y1[I][J] = fma(c3p_e4n[5], A3[I][J], c3p_e4n[6] * A2[I][J]);
            }
          mm_img<D>(img, roff, negmask, R, y1);
        }
        {
          double L[NBI][NJ], R[NBI][NJ];
#pragma unroll
          for (int I = 0; I < NBI; ++I)
#pragma unroll
            for (int J = 0; J < NJ; ++J) L[I][J] = fma(c3p_e4n[7], A2[I][J], fma(c3p_e4n[8], X[I][J], y1[I][J]));
          write_image<D>(L, img, woff);
#pragma unroll
          for (int I = 0; I < NBI; ++I)
#pragma unroll
            for (int J = 0; J < NJ; ++J) {
              R[I][J] = fma(c3p_e4n[9], A3[I][J], fma(c3p_e4n[10], X[I][J], y1[I][J]));
              double v = fma(c3p_e4n[11], y1[I][J], c3p_e4n[12] * A3[I][J]);
              v = fma(c3p_e4n[13], A2[I][J], v);
              v = fma(c3p_e4n[14], X[I][J], v);
              if (2 * I - 4 * J >= -1 && 2 * I - 4 * J <= 3) {  // the real diagonal of the half image: + e15 I  (as lincomb6)
                const bool on = (ddelta == 4 * J - 2 * I) && (2 * I + rhalf < D);
                v += on ? c3p_e4n[15] : 0.0;
              }
              P[I][J] = v;
            }
          mm_img<D>(img, roff, negmask, R, P);
        }
      } else {
      mm_img<D>(img, roff, negmask, A2, A3);
      if constexpr (T18) {
        // ---- T18 (Bader-Blanes-Casas): 5 products in total ----
        double A6[NBI][NJ];
#pragma unroll
        for (int I = 0; I < NBI; ++I)
#pragma unroll
          for (int J = 0; J < NJ; ++J) A6[I][J] = 0.0;
        write_image<D>(A3, img, woff);
        mm_img<D>(img, roff, negmask, A3, A6);
        double acc[NBI][NJ];
        {
          double B1[NBI][NJ], B5[NBI][NJ];
          lincomb6<D>(B1, 0.0, t18_a11, t18_a21, t18_a31, 0.0, X, A2, A3, A6, ddelta, rhalf);
          write_image<D>(B1, img, woff);
          lincomb6<D>(B5, 0.0, 0.0, t18_b24, t18_b34, t18_b64, X, A2, A3, A6, ddelta, rhalf);
          lincomb6<D>(acc, t18_b03, t18_b13, t18_b23, t18_b33, t18_b63, X, A2, A3, A6, ddelta, rhalf);
          mm_img<D>(img, roff, negmask, B5, acc);  // acc = A9 = B1 B5 + B4
        }
        {
          double L[NBI][NJ];
          lincomb6<D>(L, t18_b02, t18_b12, t18_b22, t18_b32, t18_b62, X, A2, A3, A6, ddelta, rhalf);
#pragma unroll
          for (int I = 0; I < NBI; ++I)
#pragma unroll
            for (int J = 0; J < NJ; ++J) L[I][J] += acc[I][J];
          write_image<D>(L, img, woff);
        }
        lincomb6<D>(P, 0.0, t18_b11, t18_b21, t18_b31, t18_b61, X, A2, A3, A6, ddelta, rhalf);
        mm_img<D>(img, roff, negmask, acc, P);  // P = B2 + (B3 + A9) A9
      } else {
        {
          double A4[NBI][NJ];
  #pragma unroll
          for (int I = 0; I < NBI; ++I)
  #pragma unroll
            for (int J = 0; J < NJ; ++J) A4[I][J] = 0.0;
          mm_img<D>(img, roff, negmask, A3, A4);
          // ---- Horner in X^4: P = c_m X^4 + B_{r-1};  P = X^4 P + B_j ----
          const int j = pr - 1;
          poly_block<D>(P, c3p_inv_fact[4 * j], c3p_inv_fact[4 * j + 1], c3p_inv_fact[4 * j + 2],
                        c3p_inv_fact[4 * j + 3], X, A2, A3, ddelta, rhalf);
          const double cm = c3p_inv_fact[4 * pr];
  #pragma unroll
          for (int I = 0; I < NBI; ++I)
  #pragma unroll
            for (int J = 0; J < NJ; ++J) P[I][J] = fma(cm, A4[I][J], P[I][J]);
          if (pr > 1) write_image<D>(A4, img, woff);
        }
        for (int j = pr - 2; j >= 0; --j) {
          double acc[NBI][NJ];
          poly_block<D>(acc, c3p_inv_fact[4 * j], c3p_inv_fact[4 * j + 1], c3p_inv_fact[4 * j + 2],
                        c3p_inv_fact[4 * j + 3], X, A2, A3, ddelta, rhalf);
          mm_img<D>(img, roff, negmask, P, acc);
  #pragma unroll
          for (int I = 0; I < NBI; ++I)
  #pragma unroll
            for (int J = 0; J < NJ; ++J) P[I][J] = acc[I][J];
        }
      }
      }  // VARIANT != 2
      // ---- squarings ----
      for (int it = 0; it < ps; ++it) {
        write_image<D>(P, img, woff);
        double acc[NBI][NJ];
#pragma unroll
        for (int I = 0; I < NBI; ++I)
#pragma unroll
          for (int J = 0; J < NJ; ++J) acc[I][J] = 0.0;
        mm_img<D>(img, roff, negmask, P, acc);
        const bool sq = !XG || it < my_s;  // (XG: a chain that needs fewer squarings than the wave keeps its result)
#pragma unroll
        for (int I = 0; I < NBI; ++I)
#pragma unroll
          for (int J = 0; J < NJ; ++J) P[I][J] = sq ? acc[I][J] : P[I][J];
      }
      // ---- partial propagator write-out ----
      if constexpr (DUS) {
        double sn, cs;
        sincos(mu_i, &sn, &cs);
        const double er = exp(mu_r);
        double* dst = reinterpret_cast<double*>(A.dUs_out) + ((long)sample * A.N + n0 + (act ? t : 0)) * D * D * 2;
        store_plain<D>(P, dst, er * cs, er * sn, nullptr, lp, act);
      }
      // ---- chain ----
      if (t == 0) {
#pragma unroll
        for (int I = 0; I < NBI; ++I)
#pragma unroll
          for (int J = 0; J < NJ; ++J) U[I][J] = P[I][J];
        mus_r = mu_r;
        mus_i = c3p_phase_add(0.0, mu_i);
      } else {
        write_image<D>(P, img, woff);
        double acc[NBI][NJ];
#pragma unroll
        for (int I = 0; I < NBI; ++I)
#pragma unroll
          for (int J = 0; J < NJ; ++J) acc[I][J] = 0.0;
        mm_img<D>(img, roff, negmask, U, acc);
#pragma unroll
        for (int I = 0; I < NBI; ++I)
#pragma unroll
          for (int J = 0; J < NJ; ++J) U[I][J] = acc[I][J];
        mus_r += mu_r;
        mus_i = c3p_phase_add(mus_i, mu_i);
      }
    }
    };
    if (t18 == 2)
      complex_loop(std::integral_constant<int, 2>{});
    else if (t18)
      complex_loop(std::integral_constant<int, 1>{});
    else
      complex_loop(std::integral_constant<int, 0>{});
    }  // complex path
  }
  // ---- segment result ----
  SD_TICK(tk2);
#ifdef C3P_SD_TIMING
  if (tkl == 0) tkl = tk2;
#endif
  if constexpr (!GIVEN) {
    if (A.fuse) {
      // (1) fold the wave's four consecutive segments: W = U3 U2 U1 U0 (later segment on the left)
      // (lane ^ 4 is row_half_mirror of quad_perm [3,2,1,0] -- 7 - (i ^ 3) = i ^ 4 inside eight lanes --, lane ^ 8 is row_ror:8: the
      // association of the sums is the one of the shuffles they replace)
      double tr = mus_r, ti = mus_i;
      tr += dpp_f64<DPP_HALF_MIRROR>(dpp_f64<DPP_XOR3>(tr));
      tr += dpp_f64<DPP_ROR8>(tr);
      ti = c3p_phase_add(ti, dpp_f64<DPP_HALF_MIRROR>(dpp_f64<DPP_XOR3>(ti)));
      ti = c3p_phase_add(ti, dpp_f64<DPP_ROR8>(ti));
      const int rrest = roff - lp.b * IMG;
      double V[NBI][NJ], Wt[NBI][NJ];
      // Wt (slot 0) = M3 M2 M1 M0 of the four slots' matrices; `in_image`: the chains' images hold M already
      // (where the fold is dealt the product does not come back to registers: it goes to image 0 times the wave's factor, see below)
      // Only two of the four slots have a first product to form and one the second.  The workgroup-per-sample instances of
      // D = 5 .. 9 deal each product's output tiles over the blocks of the slots that have none (mm_split: D = 9, 40 + 20 matrix
      // instructions instead of 75 + 75); every element has the bits of the other form, which the remaining instances keep, so the
      // two modes stay bit for bit equal at equal segments.  Not dealt, by the resource figures (profiles/r10):
      //  * up to D = 4 a product has one or two tiles -- a deal saves at most two instructions a product, less than the trip
      //    through the image that returns the result to slot 0's registers;
      //  * D = 10 .. 12 -- the deal's per-lane offsets cost these instances registers they do not have (VGPR spills 328 -> 597 at
      //    D = 11, 565 -> 668 at D = 12 in this mode);
      //  * the one-wave instances -- the last arriver inlines the fold a second time, and every one of D = 9 .. 12 took more
      //    scratch with the deal (124 -> 136 B/lane at D = 9, 340 -> 428 at D = 12).
      constexpr bool FOLD_SPLIT = MW && NBI * NJ > 2 && D <= 9;
      // the wave's factor e^{tr + i ti} = er (cs + i sn)
      double sn, cs, er = 1.0;
      auto wave_factor = [&]() {
        sincos(ti, &sn, &cs);
        // (Hermitian Hamiltonians: the trace shifts are imaginary, tr = 0 exactly -- skip the double-precision exp of the fold)
        if (__ballot(tr != 0.0) != 0) er = exp(tr);
      };
      auto fold_slots = [&](const double (&M)[NBI][NJ], bool in_image) {
        if (!in_image) write_image<D>(M, img, woff);
        if constexpr (FOLD_SPLIT) {
          const int wrest = woff - lp.b * IMG;
          // block pairs {0, 1} and {2, 3}: M1 M0 over image 0, M3 M2 over image 2
          mm_split<D, 2>(img + ((lp.b & 2) + 1) * IMG + rrest, img + (lp.b & 2) * IMG + wrest, negmask, lp.b & 1);
          SD_TICK(tkc);
          // (here the factor is what the second product's epilogue needs, and its latency lies under the LDS traffic of the products)
          wave_factor();
          SD_TICK(tkb);
          // all four blocks: (M3 M2)(M1 M0) over image 0, every tile scaled by the wave's factor where it was formed: image 0 is the
          // wave's partial as the tree of (3) reads it, written once (tr and ti are the same in every lane of the wave)
          mm_split<D, 4>(img + 2 * IMG + rrest, img + wrest, negmask, lp.b, SplitScale{er * cs, er * sn, lp.r});
        } else {
          const int roff1 = ((lp.b + 1) & 3) * IMG + rrest;  // A fragments of the NEXT chain's image
          const int roff2 = ((lp.b + 2) & 3) * IMG + rrest;
#pragma unroll
          for (int I = 0; I < NBI; ++I)
#pragma unroll
            for (int J = 0; J < NJ; ++J) V[I][J] = Wt[I][J] = 0.0;
          mm_img<D>(img, roff1, negmask, M, V);  // slots 0, 2: M_{b+1} M_b
          write_image<D>(V, img, woff);
          mm_img<D>(img, roff2, negmask, V, Wt);  // slot 0: (M3 M2)(M1 M0)
        }
      };
      fold_slots(U, img_holds_U);
      SD_TICK(tka);
      const int nW = A.S >> 2;
      const int wq = seg >> 2;
      const double* ph = A.fr_phase ? A.fr_phase + (long)sample * D : nullptr;
      double* dst = reinterpret_cast<double*>(A.final_out) + (long)sample * D * D * 2;
      const int lo = (lp.b * nW) >> 2, hi = ((lp.b + 1) * nW) >> 2;
      const int cnt = hi - lo;
      const int cmax = (nW + 3) >> 2;
      // (where the fold is not dealt the phase factors stay behind it: in front of it they shorten nothing that can be measured,
      // profiles/r16)
      if constexpr (!FOLD_SPLIT) {
        wave_factor();
        SD_TICK(tkb);
      }
      if constexpr (MW) {
        // (2) the waves of the sample are the waves of this workgroup and their partials are folded behind a barrier (by wave 0; by
        // the tree of (3) where the fold is dealt).  A partial
        // is handed over in the layout its consumer reads: scaled by the wave's e^{tr + i ti} in registers (scale_rows, the
        // arithmetic of store_plain: with equal segments this mode is bit for bit the one-wave mode, tests/test_gpu_round2.py) and
        // written as the image of the wave's chain 0 (the wave's other three images take the unused slots of Wt), from which wave 0
        // reads right operands in register order and streams left operands as they are.  Where the fold is dealt, the second product
        // of fold_slots has done both in its epilogue.
        if constexpr (!FOLD_SPLIT) {
          double pr[NBI], pi[NBI];
#pragma unroll
          for (int I = 0; I < NBI; ++I) pr[I] = er * cs, pi[I] = er * sn;
          scale_rows<D>(Wt, pr, pi, lp, V);
          write_image<D>(V, img, woff);
        }
        SD_TICK(tk3);
        // (wave 0 -- the older wave of its SIMD, through its loop first -- evaluates the row phases of the final store
        // while it waits for the others: five double-precision sincos, 1.5 us otherwise spent after the barrier; where the fold is
        // dealt, those of the rows of the lane's tiles of the last product, one per task)
        double phc[NBI], phs[NBI], dphc[sd_split_tasks<D>(4)], dphs[sd_split_tasks<D>(4)];
        if (wv == 0) {
          if constexpr (FOLD_SPLIT)
            dealt_row_phase_factors<D>(ph, lp, dphc, dphs);
          else
            row_phase_factors<D>(ph, lp, phc, phs);
        }
        __syncthreads();
#ifdef C3P_SD_TIMING
        if (blockIdx.x == 7 && lane == 0) {
          if constexpr (FOLD_SPLIT)
            printf("sd wave %d: slices %d, prologue to the table barrier %lld, behind it %lld, loop ends at %lld (100 MHz ticks after the wave's start); "
                   "layout %lld product 1 %lld phase %lld product 2 with scale and store %lld\n", wv, tmax, tk9 - tk0, tk1 - tk9, tkl - tk0, tk2 - tkl, tkc - tk2, tkb - tkc, tk3 - tkb);
          else
            printf("sd wave %d: slices %d, prologue to the table barrier %lld, behind it %lld, loop ends at %lld (100 MHz ticks after the wave's start); "
                   "layout %lld products %lld phase %lld partial store %lld\n", wv, tmax, tk9 - tk0, tk1 - tk9, tkl - tk0, tk2 - tkl, tka - tk2, tkb - tka, tk3 - tkb);
        }
#endif
        const int pstride = 4 * IMG + 4 * SG;  // partial p is image 0 of wave p
        if constexpr (FOLD_SPLIT) {
          // (3) the tree ((P7 P6)(P5 P4))((P3 P2)(P1 P0)) over the waves, a workgroup barrier between its levels: at stride st = 1,
          // 2, 4 wave q < nW / (2 st) forms P_{(2q+1) st} P_{2q st} over the right operand's image, all four blocks of the wave on
          // the one product (mm_split<D, 4>: one product per SIMD at the first level, where wave 0 alone formed the four of them
          // block by block, and the pair products of the second on two waves).  An output tile is the NBI instructions in K order
          // from a zero accumulator on the same operands that the other form gives it (nW = 2: its products with the identity
          // slots return their operand).  A stage's images are written by one wave each and read by no other wave of the stage;
          // the barrier orders them before the next stage's reads.  Every wave passes every barrier and returns behind the last.
          const int wrest = woff - lp.b * IMG;
          double* const p0 = img - wv * pstride;
          // The last level (st = nW / 2, wave 0 alone) has no consumer in LDS: every block scales the tiles it formed by their rows'
          // frame phases and stores them to the result (SplitStore: the arithmetic of store_plain), and the image is not written.
          SD_TICK(tk5);
          auto level_barrier = [&](int st) {
            if (st > 1) {
              __syncthreads();
#ifdef C3P_SD_TIMING
              if (st == 2) tk6 = wall_clock64();
#endif
            }
          };
          int st = 1;
          for (; 2 * st < nW; st <<= 1) {
            level_barrier(st);
            if (2 * st * wv < nW) mm_split<D, 4>(p0 + (2 * wv + 1) * st * pstride + rrest, p0 + 2 * wv * st * pstride + wrest, negmask, lp.b);
          }
          level_barrier(st);
          if (wv != 0) return;
          SD_TICK(tk7);
          mm_split<D, 4>(p0 + st * pstride + rrest, p0 + wrest, negmask, lp.b, SplitStore<D>{dst, dphc, dphs, lp.r, lp.c});
#ifdef C3P_SD_TIMING
          SD_TICK(tk4);
          if (tk6 == 0) tk6 = tk7;
          if (blockIdx.x == 0 && threadIdx.x == 0)
            printf("sd timing (100 MHz ticks): tables (%s) %lld signals %lld prologue %lld loop %lld fold4+store %lld barrier %lld level1 %lld level2 %lld last product with store %lld total %lld\n", A.record ? "record in LDS" : "built in LDS", tk8 - tk0, tk9 - tk8, tk1 - tk0, tk2 - tk1, tk3 - tk2, tk5 - tk3, tk6 - tk5, tk7 - tk6, tk4 - tk7, tk4 - tk0);
#endif
          return;
        }
        if (wv != 0) return;
        SD_TICK(tk5);
        // slot b takes a contiguous quarter of the nW partials (none: the identity)
        const int woff0 = woff - lp.b * IMG;
#pragma unroll
        for (int I = 0; I < NBI; ++I)
#pragma unroll
          for (int J = 0; J < NJ; ++J) {
            const int row = 2 * I + (lp.r >> 1), col = 4 * J + lp.c;
            const double idv = (row < D && row == col && (lp.r & 1) == 0) ? 1.0 : 0.0;
            U[I][J] = cnt > 0 ? img[lo * pstride + woff0 + I * 4 * W + J * 4] : idv;
          }
        for (int t = 1; t < cmax; ++t) {
          const bool act = t < cnt;
          double acc[NBI][NJ];
#pragma unroll
          for (int I = 0; I < NBI; ++I)
#pragma unroll
            for (int J = 0; J < NJ; ++J) acc[I][J] = 0.0;
          mm_img<D>(img, (act ? lo + t : 0) * pstride + rrest, negmask, U, acc);
#pragma unroll
          for (int I = 0; I < NBI; ++I)
#pragma unroll
            for (int J = 0; J < NJ; ++J) U[I][J] = act ? acc[I][J] : U[I][J];
        }
        SD_TICK(tk6);
        fold_slots(U, false);
        SD_TICK(tk7);
        store_plain<D>(Wt, dst, 1.0, 0.0, ph, lp, lp.b == 0, phc, phs);
#ifdef C3P_SD_TIMING
        SD_TICK(tk4);
        if (blockIdx.x == 0 && threadIdx.x == 0)
          printf("sd timing (100 MHz ticks): tables (%s) %lld signals %lld prologue %lld loop %lld fold4+store %lld barrier %lld level1 %lld fold2 %lld store %lld total %lld\n", A.record ? "record in LDS" : "built in LDS", tk8 - tk0, tk9 - tk8, tk1 - tk0, tk2 - tk1, tk3 - tk2, tk5 - tk3, tk6 - tk5, tk7 - tk6, tk4 - tk7, tk4 - tk0);
#endif
        return;
      }
      // one-wave workgroups: the partials meet in global memory behind a ticket, as plain complex arrays
      if (nW == 1) {
        store_plain<D>(Wt, dst, er * cs, er * sn, ph, lp, valid && lp.b == 0);
        return;
      }
      {
        double* pdst = reinterpret_cast<double*>(A.seg_out) + ((long)sample * nW + wq) * D * D * 2;
        store_plain<D, true>(Wt, pdst, er * cs, er * sn, nullptr, lp, valid && lp.b == 0);
      }
      // (2) publish and arrive (cdna guide G16, form R1: write-through payload, drain, relaxed ticket)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      int old = 0;
      if (lane == 0)
        old = __hip_atomic_fetch_add(A.counters + sample, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      old = __builtin_amdgcn_readfirstlane(old);
      if (old != nW - 1) return;
      if (lane == 0) A.counters[sample] = 0;  // self-resetting: the next launch finds it zero
      // (3) last arriver of this sample: fold the nW partials (slot b takes a contiguous quarter)
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      const double* base = reinterpret_cast<const double*>(A.seg_out) + ((long)sample * nW + lo) * D * D * 2;
      // the next partial of the slot is always in flight while the current product runs, and the first two are
      // fetched together: ONE cross-CU memory round trip for S <= 32
      double Pn[NBI][NJ];
      auto fetch = [&](double (&P)[NBI][NJ], int t) {
        const bool act = t < cnt;
        const double* src = base + (long)(act ? t : 0) * D * D * 2;
#pragma unroll
        for (int I = 0; I < NBI; ++I)
#pragma unroll
          for (int J = 0; J < NJ; ++J) {
            const int row = 2 * I + (lp.r >> 1), col = 4 * J + lp.c;
            const bool in = row < D && col < D;
            const double idv = (in && row == col && (lp.r & 1) == 0) ? 1.0 : 0.0;  // identity when idle
            P[I][J] = (act && in) ? src[(row * D + col) * 2 + (lp.r & 1)] : idv;
          }
      };
      fetch(U, 0);
      if (cmax > 1) fetch(Pn, 1);
      for (int t = 1; t < cmax; ++t) {
        double P[NBI][NJ];
#pragma unroll
        for (int I = 0; I < NBI; ++I)
#pragma unroll
          for (int J = 0; J < NJ; ++J) P[I][J] = Pn[I][J];
        if (t + 1 < cmax) fetch(Pn, t + 1);
        {
          double acc[NBI][NJ];
#pragma unroll
          for (int I = 0; I < NBI; ++I)
#pragma unroll
            for (int J = 0; J < NJ; ++J) acc[I][J] = 0.0;
          write_image<D>(P, img, woff);
          mm_img<D>(img, roff, negmask, U, acc);
#pragma unroll
          for (int I = 0; I < NBI; ++I)
#pragma unroll
            for (int J = 0; J < NJ; ++J) U[I][J] = acc[I][J];
        }
      }
      fold_slots(U, false);
      store_plain<D>(Wt, dst, 1.0, 0.0, ph, lp, lp.b == 0);
      return;
    }
  }
  double sn, cs;
  sincos(mus_i, &sn, &cs);
  const double er = exp(mus_r);
  double* dst = reinterpret_cast<double*>(A.seg_out) + (long)cc * D * D * 2;
  const double* ph = A.fr_phase ? A.fr_phase + (long)sample * D : nullptr;
  store_plain<D>(U, dst, er * cs, er * sn, ph, lp, valid);
}

// Table preparation: one block per (sample, table index).  G = fac * h (unitary: fac = -i dt)
// or the Lindblad generator (table 0 carries the dissipator).  Output image: Zh layout,
// zero padded, followed by {Re mu, Im mu, ||G - mu||_1, 0}.
template <int D>
__global__ void __launch_bounds__(64) smalld_prep_kernel(PrepArgs P) {
  using C = SD<D>;
  constexpr int MAT = C::MAT, W = C::W;
  __shared__ double g[D * D * 2];
  __shared__ double colsum[D];
  __shared__ double mu[2];
  const int tid = threadIdx.x;
  const int ti = blockIdx.x % (1 + P.K);
  const int sample = blockIdx.x / (1 + P.K);
  if (P.counters != nullptr && blockIdx.x == 0)
    for (int e = tid; e < P.ncounters; e += 64) P.counters[e] = 0;
  const int Dh = P.Dh;  // Hilbert dimension of the inputs (D for unitary, sqrt(D) for Lindblad)
  const cplx* h = (ti == 0) ? P.h0 + (long)sample * P.h0_bstride
                            : P.hks + (long)sample * P.hks_bstride + (long)(ti - 1) * Dh * Dh;
  for (int e = tid; e < D * D; e += 64) {
    const int row = e / D, col = e - row * D;
    cplx v;
    if (!P.lindblad) {
      const cplx x = h[e];
      v = cmake(x.y * P.dt, -x.x * P.dt);  // -i dt h
    } else {
      const int i = row / Dh, j = row - i * Dh, k = col / Dh, l = col - k * Dh;
      v = (ti == 0) ? P.clp[(long)sample * P.clp_bstride + e] : cmake(0, 0);
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
    const int eo = P.conjT ? col * D + row : e;  // G^H: element (col, row) = conj(G[row][col])
    g[2 * eo] = v.x;
    g[2 * eo + 1] = P.conjT ? -v.y : v.y;
  }
  __syncthreads();
  if (tid == 0) {
    double tr = 0, ti2 = 0;
    for (int i = 0; i < D; ++i) {
      tr += g[2 * (i * D + i)];
      ti2 += g[2 * (i * D + i) + 1];
    }
    mu[0] = 0.0;  // imaginary shift only (see build_tables)
    mu[1] = ti2 / D;
  }
  __syncthreads();
  if (tid < D) {
    g[2 * (tid * D + tid)] -= mu[0];
    g[2 * (tid * D + tid) + 1] -= mu[1];
  }
  __syncthreads();
  if (tid < D) {
    double s = 0;
    for (int i = 0; i < D; ++i) s += hypot(g[2 * (i * D + tid)], g[2 * (i * D + tid) + 1]);
    colsum[tid] = s;
  }
  __syncthreads();
  double* out = P.tables + ((long)sample * (1 + P.K) + ti) * (MAT + 4);
  for (int e = tid; e < MAT; e += 64) {
    const int rho = e / W, col = e - rho * W;
    const int i = rho >> 1, p = rho & 1;
    out[e] = (i < D && col < D) ? g[2 * (i * D + col) + p] : 0.0;
  }
  if (tid == 0) {
    double nrm = 0;
    for (int j = 0; j < D; ++j) nrm = fmax(nrm, colsum[j]);
    out[MAT + 0] = mu[0];
    out[MAT + 1] = mu[1];
    out[MAT + 2] = nrm;
    // 0 exactly when the Hamiltonian is real (the generator is purely imaginary): selects the real fast path
    double remax = 0, asym = 0, rsk = 0;  // real AND symmetric (to rounding: see build_tables)
    for (int e = 0; e < D * D; ++e) {
      const int i = e / D, j = e - i * D;
      remax = fmax(remax, fabs(g[2 * e]));
      asym = fmax(asym, fabs(g[2 * e + 1] - g[2 * (j * D + i) + 1]));
      rsk = fmax(rsk, fabs(g[2 * e] + g[2 * (j * D + i)]));
    }
    if (asym > 1e-14 * nrm) remax = fmax(remax, asym);
    if (remax > 0.0 && fmax(asym, rsk) <= 1e-14 * nrm) remax = -remax;  // skew-Hermitian: see build_tables
    out[MAT + 3] = P.lindblad ? 1.0 : remax;
  }
}

template <int D>
hipError_t launch_chain_t(const SmallArgs& A, hipStream_t st) {
  using C = SD<D>;
  const long nchains = (long)A.B * A.S;
  const unsigned grid = (unsigned)((nchains + 3) / 4);
  size_t lds = 0;
  // the tables' column sums (SD_CSW doubles per table) of the one-wave kernels live in the wave's images; behind them where they do not fit
  const size_t cs_tail1 = (1 + A.K) * SD_CSW <= 4 * C::IMG ? 0 : (size_t)(1 + A.K) * SD_CSW;
  if (A.mode == C3P_MODE_GIVEN || A.mode == C3P_MODE_EXPM)
    lds = (size_t)(4 * C::IMG) * sizeof(double);
  else
    lds = (size_t)((1 + A.K) * (C::MAT + 4) + 4 * C::IMG + 4 * ((A.K * A.Lmax) | 1) + cs_tail1) * sizeof(double);
  // the core + border real loop (D = 5, 9) keeps one more amplitude row per chain: the weights of the drift table
  const bool split81 = (D == 9 || D == 5) && !c3p_opt_on(C3P_OPT_no_split81);
  const int krows = A.K + ((split81 && A.K > 0) ? 1 : 0);
  if (lds > 60 * 1024) return hipErrorInvalidValue;
  if (A.mode == C3P_MODE_EXPM) {
    if (A.dUs_out)
      C3P_LAUNCH((smalld_chain_kernel<D, false, true, true>), dim3(grid), dim3(64), lds, st, A);
    else
      C3P_LAUNCH((smalld_chain_kernel<D, false, false, true>), dim3(grid), dim3(64), lds, st, A);
  } else if (A.mode == C3P_MODE_GIVEN)
    C3P_LAUNCH((smalld_chain_kernel<D, true, false>), dim3(grid), dim3(64), lds, st, A);
  else if (A.dUs_out)
    C3P_LAUNCH((smalld_chain_kernel<D, false, true>), dim3(grid), dim3(64), lds, st, A);
  else {
    // one workgroup per sample (MW) when the S / 4 waves of a sample fit a CU together with enough other samples for all
    // B workgroups to be resident at once (8 waves per CU at two per SIMD): B = 256, S = 32 -> 256 workgroups of 8 waves
    const int nW = A.S >> 2;
    const size_t wstride = (size_t)(4 * C::IMG + 4 * ((krows * A.Lmax) | 1));
    // (the last term held the waves' partial products as plain arrays; they now stay in the waves' images, and the tables' column
    // sums -- SD_CSW doubles per table -- stand at its start.  It keeps its former size in both sizes below on purpose wherever
    // the column sums fit in it (all but D = 2, 3 with several tables): it counts toward the gates that choose this mode and its
    // split, and no shape is to change path here)
    const size_t tail_mw = std::max((size_t)nW * D * D * 2, (size_t)(1 + A.K) * SD_CSW);
    const size_t lds_mw = (size_t)((1 + A.K) * (C::MAT + 4) + nW * wstride + tail_mw) * sizeof(double);
    const bool mw = A.fuse && (A.S & 3) == 0 && (nW == 2 || nW == 4 || nW == 8) && (long)A.B * nW <= 2048 &&
                    lds_mw * (8 / nW) <= (size_t)156 * 1024 && !c3p_opt_on(C3P_OPT_no_mw);
    if (mw) {
      // Two waves share a SIMD (nW = 8) and the arbiter serves the older one first: with equal segments wave w leaves its
      // loop at 64 % of the kernel time and wave w + 4 runs the rest alone, at the (slower) one-wave rate.  Give the older
      // waves the longer segments so that both finish together: measured optimum near 2 : 1 (C3P_MW_SKEW = long share of
      // a pair's slices in per mille, default 640; 500 = equal segments).
      SmallArgs A2 = A;
      if (nW == 8 && A.N >= 4 * A.S) {
        // (measured optimum 640 with the padded tiles, 660 with the core + border form of D = 5, 9, 700 with its border sums on the
        // matrix cores -- round 6: tools/sweep_split81.py, profiles/r06/sweep_skew.txt; one slice of the long segments moves the
        // two waves of a SIMD by 7 us against each other, so the optimum is sharp)
        // (the complex loop of the same kernel keeps 640: profiles/r06/sweep_skew_complex.txt -- its samples re-split on the device)
        // (D = 9 with the column-wise norm bound -- no workgroup of cfg2 on the seven-product loop any more: 704, long segments of
        // 44 slices instead of 43, 0.6 us faster than 700 in every run of profiles/r09/sweep_skew.json; D = 5 was not re-swept)
        // (re-swept on the loop with the no-squaring body and the packed column border: D = 9 736, long segments of 46 slices, the
        // fastest of 688 .. 736 in every round; D = 5 716, the fastest of 684 .. 716 -- profiles/r14/sweep_skew.json)
        int skew = ((D == 9 || D == 5) && !c3p_opt_on(C3P_OPT_no_split81)) ? (D == 9 ? 736 : 716) : 640, skew_c = 640;
        if (c3p_opt(C3P_OPT_mw_skew) >= 0) skew = skew_c = (int)c3p_opt(C3P_OPT_mw_skew);
        if (skew > 500 && skew < 900) {
          const int h = A.S / 2;
          int lmax = 0;
          auto split = [&](int per_mille) {
            int La = (int)(((long)A.N * per_mille) / (500L * A.S));  // = per_mille / 1000 of the 2 N / S slices of a pair of chains
            if (La < 1) La = 1;
            if ((long)h * La > A.N - h) La = (A.N - h) / h;  // at least one slice for every short chain
            const long rest = (long)A.N - (long)h * La;
            const int Lb = (int)((rest + h - 1) / h);
            lmax = std::max(lmax, std::max(La, Lb));
            return La;
          };
          A2.seg_long = split(skew);
          A2.seg_long_c = (skew_c > 500 && skew_c < 900 && skew_c != skew) ? split(skew_c) : 0;
          A2.Lmax = lmax;
        }
      }
      const size_t wstride2 = (size_t)(4 * C::IMG + 4 * ((krows * A2.Lmax) | 1));
      const size_t lds_mw2 = (size_t)((1 + A2.K) * (C::MAT + 4) + nW * wstride2 + tail_mw) * sizeof(double);
      if (lds_mw2 > (size_t)156 * 1024) A2 = A;  // (the longer segments need more LDS for their control amplitudes)
      const size_t lds_use = A2.seg_long > 0 ? lds_mw2 : lds_mw;
      auto kern = smalld_chain_kernel<D, false, false, false, true>;
      if constexpr (D == 9 || D == 5) {
        // core + border form of the real path (8 + 1 split at D = 9): no_split81 = 1 keeps the padded 12 x 12 tiles
        if (!c3p_opt_on(C3P_OPT_no_split81)) kern = smalld_chain_kernel<D, false, false, false, true, true>;
      }
      if (lds_use > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_use);
        if (e != hipSuccess) return e;
      }
      C3P_LAUNCH(kern, dim3((unsigned)A.B), dim3(64 * nW), lds_use, st, A2);
    } else {
      auto kern1 = smalld_chain_kernel<D, false, false>;
      if constexpr (D == 9 || D == 5) {
        if (!c3p_opt_on(C3P_OPT_no_split81)) kern1 = smalld_chain_kernel<D, false, false, false, false, true>;
      }
      const size_t lds1 = (size_t)((1 + A.K) * (C::MAT + 4) + 4 * C::IMG + 4 * ((krows * A.Lmax) | 1) + cs_tail1) * sizeof(double);
      if (lds1 > 60 * 1024) return hipErrorInvalidValue;
      C3P_LAUNCH(kern1, dim3(grid), dim3(64), lds1, st, A);
    }
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Backward sweep of the control gradient (method in c3p_grad.hip) on the matrix cores.
// Same mapping as the forward kernel (chain = MFMA block), but ONE wave per SIMD: the pair evaluation
// of T18 keeps ~13 matrices live (X, X^2, X^3, X^6 and their derivatives, accumulators), which fits
// the 512-register budget of a single-wave SIMD and not the 256 of two.  Two LDS images (value and
// derivative left operands); per slice 18 + 3s products:
//   (T, dT) = pair-T18(X~, M) ; Z = T^H dT ; grad[k] = <Z, G_k> ; M <- T^H (M T).
// ---------------------------------------------------------------------------------------------
template <int D>
__device__ __forceinline__ void write_image_H(const double (&zh)[SD<D>::NBI][SD<D>::NJ], double* img, const LanePos& lp) {
  using C = SD<D>;
  wave_sync();
#pragma unroll
  for (int I = 0; I < C::NBI; ++I)
#pragma unroll
    for (int J = 0; J < C::NJ; ++J) {
      // lane holds (r even ? Re : Im) Z[i][j], i = 2I + r/2, j = 4J + c; Y = Z^H: Yh[2j + p][i] = p ? -Im Z[i][j] : Re Z[i][j]
      const int trow = 2 * (4 * J + lp.c) + (lp.r & 1), tcol = 2 * I + (lp.r >> 1);
      const double v = (lp.r & 1) ? -zh[I][J] : zh[I][J];
      if (trow < 4 * C::NBI) img[lp.b * C::MAT + trow * C::W + tcol] = v;
    }
  wave_sync();
}

template <int D>
__device__ __forceinline__ void mat_zero(double (&m)[SD<D>::NBI][SD<D>::NJ]) {
#pragma unroll
  for (int I = 0; I < SD<D>::NBI; ++I)
#pragma unroll
    for (int J = 0; J < SD<D>::NJ; ++J) m[I][J] = 0.0;
}

// squarings of the real-Hamiltonian backward sweep (smalld_grad_real_kernel below): the economised degree-8 cos / sin pair of
// c3p_common.h (radius C3P_MM8_THETA)
constexpr int SDG_MAXS = 3;

template <int D>
__global__ void __launch_bounds__(64, 1) smalld_grad_kernel(SmallGradArgs A) {
  using C = SD<D>;
  constexpr int NBI = C::NBI, NJ = C::NJ, W = C::W, MAT = C::MAT;
  typedef double Mat[NBI][NJ];
  const int lane = threadIdx.x;
  LanePos lp;
  lp.r = lane >> 4;
  lp.b = (lane >> 2) & 3;
  lp.c = lane & 3;
  lp.idx16 = lp.r * 4 + lp.c;
  const int K = A.K;
  double* tab = c3p_sd_lds;
  double* img0 = tab + (1 + K) * (MAT + 4);
  double* img1 = img0 + 4 * MAT;
  double* sg = img1 + 4 * MAT;

  const long chain = (long)blockIdx.x * 4 + lp.b;
  const long nchains = (long)A.B * A.S;
  const bool valid = chain < nchains;
  const long cc = valid ? chain : nchains - 1;
  const int sample = (int)(cc / A.S);
  const int seg = (int)(cc - (long)sample * A.S);
  const int n0 = (int)(((long)seg * A.N) / A.S);
  const int n1 = (int)(((long)(seg + 1) * A.N) / A.S);
  const int len = n1 - n0;

  const int woff = lp.b * MAT + lp.r * W + lp.c;
  const int roff = lp.b * MAT + (2 * (lp.c >> 1) + ((lp.c ^ lp.r) & 1)) * W + (lp.r >> 1);
  const unsigned negmask = (((lp.c & 1) == 0) && ((lp.r & 1) == 1)) ? 0x80000000u : 0u;
  const int toff = lp.r * W + lp.c;
  const int ddelta = (lp.r & 1) ? 1000 : ((lp.r >> 1) - lp.c);
  const int rhalf = lp.r >> 1;

  const double* gt0 = A.tables + (long)(A.tab_per_sample ? sample : 0) * (1 + K) * (MAT + 4);
  for (int e = lane; e < (1 + K) * (MAT + 4); e += 64) tab[e] = gt0[e];
  __syncthreads();
  double nrm = tab[MAT + 2];
  for (int k = 0; k < K; ++k) {
    const double* s = A.signals + ((long)sample * K + k) * A.N + n0;
    double cmax = 0.0;
    for (int t = lp.idx16; t < A.Lmax; t += 16) {
      const double v = (valid && t < len) ? s[t] : 0.0;
      sg[(lp.b * K + k) * A.Lmax + t] = v;
      cmax = fmax(cmax, fabs(v));
    }
    cmax = fmax(cmax, __shfl_xor(cmax, 1));
    cmax = fmax(cmax, __shfl_xor(cmax, 2));
    cmax = fmax(cmax, __shfl_xor(cmax, 16));
    cmax = fmax(cmax, __shfl_xor(cmax, 32));
    nrm = fma(cmax, tab[(k + 1) * (MAT + 4) + MAT + 2], nrm);
  }
  nrm = fmax(nrm, __shfl_xor(nrm, 4));
  nrm = fmax(nrm, __shfl_xor(nrm, 8));
  nrm = readfirstlane_f64(nrm);
  int ps = c3p_squarings(nrm, C3P_T18_THETA);
  ps = __builtin_amdgcn_readfirstlane(ps);
  if (A.skip_real) {  // the real-Hamiltonian sweep has taken this wave's chains (same tables, same norm bound: same decision)
    bool realH = true;
    for (int k = 0; k <= K; ++k) realH = realH && (tab[k * (MAT + 4) + MAT + 3] == 0.0);
    // its bound is the column-wise one (c3p_sd_segment_norm), formed here as it forms it; the plan of this kernel's own sweep
    // stays on the sum of norms above
    double* csb = sg + 4 * K * A.Lmax;
    sd_colsums<D>(tab, K, csb, lane);
    __syncthreads();
    double nrm_r = c3p_sd_segment_norm(csb, K, lp.idx16, [&](int k) {
      double cmax = 0.0;
      for (int t = lp.idx16; t < A.Lmax; t += 16) cmax = fmax(cmax, fabs(sg[(lp.b * K + k) * A.Lmax + t]));
      cmax = fmax(cmax, __shfl_xor(cmax, 1));
      cmax = fmax(cmax, __shfl_xor(cmax, 2));
      cmax = fmax(cmax, __shfl_xor(cmax, 16));
      cmax = fmax(cmax, __shfl_xor(cmax, 32));
      return cmax;
    });
    nrm_r = fmax(nrm_r, __shfl_xor(nrm_r, 4));
    nrm_r = fmax(nrm_r, __shfl_xor(nrm_r, 8));
    nrm_r = readfirstlane_f64(nrm_r);
    if (__builtin_amdgcn_readfirstlane((int)realH) != 0 && __builtin_amdgcn_readfirstlane(c3p_squarings(nrm_r, C3P_MM8_THETA)) <= SDG_MAXS)
      return;
  }
  const double scale = ldexp(1.0, -ps);
  __syncthreads();

  // adjoint state at the end of this segment, D-layout
  Mat M;
  {
    const double* src = reinterpret_cast<const double*>(A.Mb) + cc * D * D * 2;
#pragma unroll
    for (int I = 0; I < NBI; ++I)
#pragma unroll
      for (int J = 0; J < NJ; ++J) {
        const int row = 2 * I + (lp.r >> 1), col = 4 * J + lp.c;
        M[I][J] = (valid && row < D && col < D) ? src[(row * D + col) * 2 + (lp.r & 1)] : 0.0;
      }
  }

  for (int t = A.Lmax - 1; t >= 0; --t) {
    const bool act = valid && t < len;
    const double sc = act ? scale : 0.0;
    Mat X, dX;
#pragma unroll
    for (int I = 0; I < NBI; ++I)
#pragma unroll
      for (int J = 0; J < NJ; ++J) {
        X[I][J] = sc * tab[toff + I * 4 * W + J * 4];
        dX[I][J] = scale * M[I][J];
      }
    for (int k = 0; k < K; ++k) {
      const double ck = sc * sg[(lp.b * K + k) * A.Lmax + t];
      const double* tk = tab + (k + 1) * (MAT + 4);
#pragma unroll
      for (int I = 0; I < NBI; ++I)
#pragma unroll
        for (int J = 0; J < NJ; ++J) X[I][J] = fma(ck, tk[toff + I * 4 * W + J * 4], X[I][J]);
    }
    write_image<D>(X, img0, woff);
    write_image<D>(dX, img1, woff);
    Mat A2, dA2, A3, dA3, A6, dA6;
    mat_zero<D>(A2), mat_zero<D>(dA2), mat_zero<D>(A3), mat_zero<D>(dA3), mat_zero<D>(A6), mat_zero<D>(dA6);
    mm_img<D>(img0, roff, negmask, X, A2);
    mm_img<D>(img0, roff, negmask, dX, dA2);
    mm_img<D>(img1, roff, negmask, X, dA2);
    mm_img<D>(img0, roff, negmask, A2, A3);
    mm_img<D>(img0, roff, negmask, dA2, dA3);
    mm_img<D>(img1, roff, negmask, A2, dA3);
    write_image<D>(A3, img0, woff);
    write_image<D>(dA3, img1, woff);
    mm_img<D>(img0, roff, negmask, A3, A6);
    mm_img<D>(img0, roff, negmask, dA3, dA6);
    mm_img<D>(img1, roff, negmask, A3, dA6);
    Mat A9, dA9;
    {
      Mat B1, dB1;
      lincomb6<D>(B1, 0.0, C3P_T18_A11, C3P_T18_A21, C3P_T18_A31, 0.0, X, A2, A3, A6, ddelta, rhalf);
      lincomb6<D>(dB1, 0.0, C3P_T18_A11, C3P_T18_A21, C3P_T18_A31, 0.0, dX, dA2, dA3, dA6, ddelta, rhalf);
      write_image<D>(B1, img0, woff);
      write_image<D>(dB1, img1, woff);
    }
    {
      Mat B5, dB5;
      lincomb6<D>(B5, 0.0, 0.0, C3P_T18_B24, C3P_T18_B34, C3P_T18_B64, X, A2, A3, A6, ddelta, rhalf);
      lincomb6<D>(dB5, 0.0, 0.0, C3P_T18_B24, C3P_T18_B34, C3P_T18_B64, dX, dA2, dA3, dA6, ddelta, rhalf);
      lincomb6<D>(A9, C3P_T18_B03, C3P_T18_B13, C3P_T18_B23, C3P_T18_B33, C3P_T18_B63, X, A2, A3, A6, ddelta, rhalf);
      lincomb6<D>(dA9, 0.0, C3P_T18_B13, C3P_T18_B23, C3P_T18_B33, C3P_T18_B63, dX, dA2, dA3, dA6, ddelta, rhalf);
      mm_img<D>(img0, roff, negmask, B5, A9);
      mm_img<D>(img0, roff, negmask, dB5, dA9);
      mm_img<D>(img1, roff, negmask, B5, dA9);
    }
    Mat T, dT;
    {
      Mat L, dL;
      lincomb6<D>(L, C3P_T18_B02, C3P_T18_B12, C3P_T18_B22, C3P_T18_B32, C3P_T18_B62, X, A2, A3, A6, ddelta, rhalf);
      lincomb6<D>(dL, 0.0, C3P_T18_B12, C3P_T18_B22, C3P_T18_B32, C3P_T18_B62, dX, dA2, dA3, dA6, ddelta, rhalf);
#pragma unroll
      for (int I = 0; I < NBI; ++I)
#pragma unroll
        for (int J = 0; J < NJ; ++J) {
          L[I][J] += A9[I][J];
          dL[I][J] += dA9[I][J];
        }
      write_image<D>(L, img0, woff);
      write_image<D>(dL, img1, woff);
    }
    lincomb6<D>(T, 0.0, C3P_T18_B11, C3P_T18_B21, C3P_T18_B31, C3P_T18_B61, X, A2, A3, A6, ddelta, rhalf);
    lincomb6<D>(dT, 0.0, C3P_T18_B11, C3P_T18_B21, C3P_T18_B31, C3P_T18_B61, dX, dA2, dA3, dA6, ddelta, rhalf);
    mm_img<D>(img0, roff, negmask, A9, T);
    mm_img<D>(img0, roff, negmask, dA9, dT);
    mm_img<D>(img1, roff, negmask, A9, dT);
    for (int it = 0; it < ps; ++it) {
      write_image<D>(T, img0, woff);
      write_image<D>(dT, img1, woff);
      Mat T2, dT2;
      mat_zero<D>(T2), mat_zero<D>(dT2);
      mm_img<D>(img0, roff, negmask, T, T2);
      mm_img<D>(img0, roff, negmask, dT, dT2);
      mm_img<D>(img1, roff, negmask, T, dT2);
#pragma unroll
      for (int I = 0; I < NBI; ++I)
#pragma unroll
        for (int J = 0; J < NJ; ++J) {
          T[I][J] = T2[I][J];
          dT[I][J] = dT2[I][J];
        }
    }
    // ---- Z = T^H dT, grad[k] = Re<Z, G_k> = sum Zh.G~h + Re(mu_k conj(tr Z)) ----
    write_image_H<D>(T, img0, lp);
    write_image<D>(M, img1, woff);
    {
      Mat Z;
      mat_zero<D>(Z);
      mm_img<D>(img0, roff, negmask, dT, Z);
      if (A.zout != nullptr) {  // per-slice cotangent of the generator G_n = -i dt H_n
        double* dst = reinterpret_cast<double*>(A.zout) + ((long)sample * A.N + n0 + (act ? t : 0)) * D * D * 2;
        store_plain<D>(Z, dst, 1.0, 0.0, nullptr, lp, act);
      }
      double trr = 0.0, tri = 0.0;
#pragma unroll
      for (int I = 0; I < NBI; ++I)
#pragma unroll
        for (int J = 0; J < NJ; ++J)
          if (2 * I - 4 * J >= -1 && 2 * I - 4 * J <= 3) {
            const bool on = (((lp.r >> 1) - lp.c) == 4 * J - 2 * I) && (2 * I + rhalf < D);
            const double v = on ? Z[I][J] : 0.0;
            if (lp.r & 1)
              tri += v;
            else
              trr += v;
          }
      for (int k = 0; k < K; ++k) {
        const double* tk = tab + (k + 1) * (MAT + 4);
        double part = fma(tk[MAT + 0], trr, tk[MAT + 1] * tri);
#pragma unroll
        for (int I = 0; I < NBI; ++I)
#pragma unroll
          for (int J = 0; J < NJ; ++J) part = fma(Z[I][J], tk[toff + I * 4 * W + J * 4], part);
        part += __shfl_xor(part, 1);
        part += __shfl_xor(part, 2);
        part += __shfl_xor(part, 16);
        part += __shfl_xor(part, 32);
        if (act && lp.idx16 == 0) A.grad[((long)sample * K + k) * A.N + n0 + t] = part;
      }
    }
    // ---- M <- T^H (M T) ----
    {
      Mat V;
      mat_zero<D>(V);
      mm_img<D>(img1, roff, negmask, T, V);
      mat_zero<D>(M);
      mm_img<D>(img0, roff, negmask, V, M);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Backward sweep for GENERAL generators (Lindblad superoperators up to 12 x 12, i.e. D <= 3): the slices are not unitary, so
// the adjoint state cannot be carried as M_n = dU_n^H M_{n+1} dU_n.  Method of c3p_grad.hip (general form):
//   grad[k,n] = Re <L(X_n^H; M_n), G_k>,  M_n = A_n P_n^H,  P_n = dU_{n-1} .. dU_0 (prefix),  A_n = S_n^H FR^H Ubar (left adjoint).
// Per chain: a forward walk over the segment, P <- dU_n P with the slice propagators of the forward pass (one product per
// slice), every P_n stored; then backwards, ONE pair evaluation of T18 per slice at Y = X_n^H (tables of G^H): the value
// exp(Y) = dU_n^H advances A, the derivative L(Y; M_n) is the generator's cotangent.  The trace shifts do not cancel here: A and
// the derivative carry them as ONE complex scalar per chain, applied to the complex inner product <dT, G_k> at the end.
// ---------------------------------------------------------------------------------------------
template <int D, bool XG = false>
__global__ void __launch_bounds__(64, 1) smalld_grad_general_kernel(SmallGradArgs A) {
  using C = SD<D>;
  constexpr int NBI = C::NBI, NJ = C::NJ, W = C::W, MAT = C::MAT;
  typedef double Mat[NBI][NJ];
  const int lane = threadIdx.x;
  LanePos lp;
  lp.r = lane >> 4;
  lp.b = (lane >> 2) & 3;
  lp.c = lane & 3;
  lp.idx16 = lp.r * 4 + lp.c;
  const int K = XG ? 0 : A.K;
  double* tab = c3p_sd_lds;                 // G tables: inner products
  double* tabh = tab + (1 + K) * (MAT + 4);  // G^H tables: the matrix that is exponentiated
  double* img0 = tabh + (1 + K) * (MAT + 4);
  double* img1 = img0 + 4 * MAT;
  double* sg = img1 + 4 * MAT;

  const long chain = (long)blockIdx.x * 4 + lp.b;
  const long nchains = (long)A.B * A.S;
  const bool valid = chain < nchains;
  const long cc = valid ? chain : nchains - 1;
  const int sample = (int)(cc / A.S);
  const int seg = (int)(cc - (long)sample * A.S);
  const int n0 = (int)(((long)seg * A.N) / A.S);
  const int n1 = (int)(((long)(seg + 1) * A.N) / A.S);
  const int len = n1 - n0;

  const int woff = lp.b * MAT + lp.r * W + lp.c;
  const int roff = lp.b * MAT + (2 * (lp.c >> 1) + ((lp.c ^ lp.r) & 1)) * W + (lp.r >> 1);
  const unsigned negmask = (((lp.c & 1) == 0) && ((lp.r & 1) == 1)) ? 0x80000000u : 0u;
  const int toff = lp.r * W + lp.c;
  const int poff = (lp.r ^ 1) * W + lp.c;  // the same element's other part (Re <-> Im) in a table
  const int ddelta = (lp.r & 1) ? 1000 : ((lp.r >> 1) - lp.c);
  const int rhalf = lp.r >> 1;

  const long tsz = (long)(1 + K) * (MAT + 4);
  double nrm = 0.0;
  if constexpr (XG) {
    // supplied generators: the matrix exponentiated is X_n^H, whose 1-norm is the row-sum norm of X_n (slot 3 of the hmeta pass)
    const double* mt = A.meta + ((long)sample * A.N + n0) * 4;
    for (int t = lp.idx16; t < A.Lmax; t += 16)
      if (valid && t < len) nrm = fmax(nrm, mt[(long)t * 4 + 3]);
    nrm = fmax(nrm, __shfl_xor(nrm, 1));
    nrm = fmax(nrm, __shfl_xor(nrm, 2));
    nrm = fmax(nrm, __shfl_xor(nrm, 16));
    nrm = fmax(nrm, __shfl_xor(nrm, 32));
  } else {
    const double* gt0 = A.tables + (long)(A.tab_per_sample ? sample : 0) * tsz;
    const double* gh0 = A.tables_h + (long)(A.tab_per_sample ? sample : 0) * tsz;
    for (int e = lane; e < (int)tsz; e += 64) {
      tab[e] = gt0[e];
      tabh[e] = gh0[e];
    }
    __syncthreads();
    nrm = tabh[MAT + 2];
  }
  for (int k = 0; k < K; ++k) {
    const double* s = A.signals + ((long)sample * K + k) * A.N + n0;
    double cmax = 0.0;
    for (int t = lp.idx16; t < A.Lmax; t += 16) {
      const double v = (valid && t < len) ? s[t] : 0.0;
      sg[(lp.b * K + k) * A.Lmax + t] = v;
      cmax = fmax(cmax, fabs(v));
    }
    cmax = fmax(cmax, __shfl_xor(cmax, 1));
    cmax = fmax(cmax, __shfl_xor(cmax, 2));
    cmax = fmax(cmax, __shfl_xor(cmax, 16));
    cmax = fmax(cmax, __shfl_xor(cmax, 32));
    nrm = fma(cmax, tabh[(k + 1) * (MAT + 4) + MAT + 2], nrm);
  }
  nrm = fmax(nrm, __shfl_xor(nrm, 4));
  nrm = fmax(nrm, __shfl_xor(nrm, 8));
  nrm = readfirstlane_f64(nrm);
  int ps = c3p_squarings(nrm, C3P_T18_THETA);
  ps = __builtin_amdgcn_readfirstlane(ps);
  const double scale = ldexp(1.0, -ps);
  __syncthreads();

  // element (row, col), part r & 1 of a plain complex matrix in global memory -> D layout (TR: its conjugate transpose)
  auto load_plain = [&](Mat& m, const cplx* srcc, bool on, bool TR) {
    const double* src = reinterpret_cast<const double*>(srcc);
#pragma unroll
    for (int I = 0; I < NBI; ++I)
#pragma unroll
      for (int J = 0; J < NJ; ++J) {
        const int row = 2 * I + (lp.r >> 1), col = 4 * J + lp.c;
        double v = 0.0;
        if (on && row < D && col < D) {
          v = TR ? src[(col * D + row) * 2 + (lp.r & 1)] : src[(row * D + col) * 2 + (lp.r & 1)];
          if (TR && (lp.r & 1)) v = -v;
        }
        m[I][J] = v;
      }
  };
  auto set_identity = [&](Mat& m) {
#pragma unroll
    for (int I = 0; I < NBI; ++I)
#pragma unroll
      for (int J = 0; J < NJ; ++J) {
        const int row = 2 * I + (lp.r >> 1), col = 4 * J + lp.c;
        m[I][J] = (!(lp.r & 1) && row == col && row < D) ? 1.0 : 0.0;
      }
  };

  // ---- forward: the prefix in front of every slice of the segment ----
  cplx* pst = A.pstore + ((long)sample * A.N + n0) * D * D;
  {
    Mat P;
    load_plain(P, A.pre + cc * D * D, valid, false);
    const cplx* du = A.dUs + ((long)sample * A.N + n0) * D * D;
    for (int t = 0; t < A.Lmax; ++t) {
      const bool act = valid && t < len;
      store_plain<D>(P, reinterpret_cast<double*>(pst + (long)(act ? t : 0) * D * D), 1.0, 0.0, nullptr, lp, act);
      if (t + 1 == A.Lmax) break;
      Mat E, V;
      if (__builtin_amdgcn_readfirstlane((int)__any(act)) == 0) continue;
      load_plain(E, du + (long)(act ? t : 0) * D * D, act, false);
      if (!act) set_identity(E);
      write_image<D>(E, img0, woff);
      mat_zero<D>(V);
      mm_img<D>(img0, roff, negmask, P, V);
#pragma unroll
      for (int I = 0; I < NBI; ++I)
#pragma unroll
        for (int J = 0; J < NJ; ++J) P[I][J] = V[I][J];
    }
  }
  __threadfence_block();

  // ---- backward ----
  Mat Aa;  // left adjoint, WITHOUT the trace shifts of the slices behind it: they accumulate in (ams_r, ams_i)
  load_plain(Aa, A.Mb + cc * D * D, valid, false);
  double ams_r = 0.0, ams_i = 0.0;
  for (int t = A.Lmax - 1; t >= 0; --t) {
    const bool act = valid && t < len;
    const double sc = act ? scale : 0.0;
    Mat X, dX;
    {
      Mat PH, Mn;
      load_plain(PH, pst + (long)(act ? t : 0) * D * D, act, true);
      write_image<D>(Aa, img0, woff);
      mat_zero<D>(Mn);
      mm_img<D>(img0, roff, negmask, PH, Mn);  // M_n = A P_n^H
#pragma unroll
      for (int I = 0; I < NBI; ++I)
#pragma unroll
        for (int J = 0; J < NJ; ++J) dX[I][J] = scale * Mn[I][J];
    }
    double mu_r = 0.0, mu_i = 0.0;  // trace shift of Y = X_n^H
    if constexpr (XG) {
      // Y = conj(coef) hs[b,n]^H - conj(mu_n): element (row, col) = conj(coef hs[col][row])
      const long m = (long)sample * A.N + n0 + (act ? t : 0);
      mu_r = act ? A.meta[m * 4 + 0] : 0.0;
      mu_i = act ? -A.meta[m * 4 + 1] : 0.0;
      const double2* src = reinterpret_cast<const double2*>(A.hs) + (long)sample * A.hs_bstride + (long)(n0 + (act ? t : 0)) * D * D;
      const double mine = (lp.r & 1) ? mu_i : mu_r;
#pragma unroll
      for (int I = 0; I < NBI; ++I)
#pragma unroll
        for (int J = 0; J < NJ; ++J) {
          const int row = 2 * I + (lp.r >> 1), col = 4 * J + lp.c;
          const bool in = row < D && col < D;
          const double2 h = src[in ? col * D + row : 0];
          // coef h = (cr hx - ci hy) + i (cr hy + ci hx); conjugated for the transpose
          double v = (lp.r & 1) ? -fma(A.coef_r, h.y, A.coef_i * h.x) : fma(A.coef_r, h.x, -A.coef_i * h.y);
          v -= (row == col) ? mine : 0.0;
          X[I][J] = in ? sc * v : 0.0;
        }
    } else {
    mu_r = act ? tabh[MAT + 0] : 0.0;
    mu_i = act ? tabh[MAT + 1] : 0.0;
#pragma unroll
    for (int I = 0; I < NBI; ++I)
#pragma unroll
      for (int J = 0; J < NJ; ++J) X[I][J] = sc * tabh[toff + I * 4 * W + J * 4];
    }
    for (int k = 0; k < K; ++k) {
      const double c0 = sg[(lp.b * K + k) * A.Lmax + t];  // zero for inactive slices
      const double ck = sc * c0;
      const double* tk = tabh + (k + 1) * (MAT + 4);
      mu_r = fma(c0, tk[MAT + 0], mu_r);
      mu_i = fma(c0, tk[MAT + 1], mu_i);
#pragma unroll
      for (int I = 0; I < NBI; ++I)
#pragma unroll
        for (int J = 0; J < NJ; ++J) X[I][J] = fma(ck, tk[toff + I * 4 * W + J * 4], X[I][J]);
    }
    write_image<D>(X, img0, woff);
    write_image<D>(dX, img1, woff);
    Mat A2, dA2, A3, dA3, A6, dA6;
    mat_zero<D>(A2), mat_zero<D>(dA2), mat_zero<D>(A3), mat_zero<D>(dA3), mat_zero<D>(A6), mat_zero<D>(dA6);
    mm_img<D>(img0, roff, negmask, X, A2);
    mm_img<D>(img0, roff, negmask, dX, dA2);
    mm_img<D>(img1, roff, negmask, X, dA2);
    mm_img<D>(img0, roff, negmask, A2, A3);
    mm_img<D>(img0, roff, negmask, dA2, dA3);
    mm_img<D>(img1, roff, negmask, A2, dA3);
    write_image<D>(A3, img0, woff);
    write_image<D>(dA3, img1, woff);
    mm_img<D>(img0, roff, negmask, A3, A6);
    mm_img<D>(img0, roff, negmask, dA3, dA6);
    mm_img<D>(img1, roff, negmask, A3, dA6);
    Mat A9, dA9;
    {
      Mat B1, dB1;
      lincomb6<D>(B1, 0.0, C3P_T18_A11, C3P_T18_A21, C3P_T18_A31, 0.0, X, A2, A3, A6, ddelta, rhalf);
      lincomb6<D>(dB1, 0.0, C3P_T18_A11, C3P_T18_A21, C3P_T18_A31, 0.0, dX, dA2, dA3, dA6, ddelta, rhalf);
      write_image<D>(B1, img0, woff);
      write_image<D>(dB1, img1, woff);
    }
    {
      Mat B5, dB5;
      lincomb6<D>(B5, 0.0, 0.0, C3P_T18_B24, C3P_T18_B34, C3P_T18_B64, X, A2, A3, A6, ddelta, rhalf);
      lincomb6<D>(dB5, 0.0, 0.0, C3P_T18_B24, C3P_T18_B34, C3P_T18_B64, dX, dA2, dA3, dA6, ddelta, rhalf);
      lincomb6<D>(A9, C3P_T18_B03, C3P_T18_B13, C3P_T18_B23, C3P_T18_B33, C3P_T18_B63, X, A2, A3, A6, ddelta, rhalf);
      lincomb6<D>(dA9, 0.0, C3P_T18_B13, C3P_T18_B23, C3P_T18_B33, C3P_T18_B63, dX, dA2, dA3, dA6, ddelta, rhalf);
      mm_img<D>(img0, roff, negmask, B5, A9);
      mm_img<D>(img0, roff, negmask, dB5, dA9);
      mm_img<D>(img1, roff, negmask, B5, dA9);
    }
    Mat T, dT;
    {
      Mat L, dL;
      lincomb6<D>(L, C3P_T18_B02, C3P_T18_B12, C3P_T18_B22, C3P_T18_B32, C3P_T18_B62, X, A2, A3, A6, ddelta, rhalf);
      lincomb6<D>(dL, 0.0, C3P_T18_B12, C3P_T18_B22, C3P_T18_B32, C3P_T18_B62, dX, dA2, dA3, dA6, ddelta, rhalf);
#pragma unroll
      for (int I = 0; I < NBI; ++I)
#pragma unroll
        for (int J = 0; J < NJ; ++J) {
          L[I][J] += A9[I][J];
          dL[I][J] += dA9[I][J];
        }
      write_image<D>(L, img0, woff);
      write_image<D>(dL, img1, woff);
    }
    lincomb6<D>(T, 0.0, C3P_T18_B11, C3P_T18_B21, C3P_T18_B31, C3P_T18_B61, X, A2, A3, A6, ddelta, rhalf);
    lincomb6<D>(dT, 0.0, C3P_T18_B11, C3P_T18_B21, C3P_T18_B31, C3P_T18_B61, dX, dA2, dA3, dA6, ddelta, rhalf);
    mm_img<D>(img0, roff, negmask, A9, T);
    mm_img<D>(img0, roff, negmask, dA9, dT);
    mm_img<D>(img1, roff, negmask, A9, dT);
    for (int it = 0; it < ps; ++it) {
      write_image<D>(T, img0, woff);
      write_image<D>(dT, img1, woff);
      Mat T2, dT2;
      mat_zero<D>(T2), mat_zero<D>(dT2);
      mm_img<D>(img0, roff, negmask, T, T2);
      mm_img<D>(img0, roff, negmask, dT, dT2);
      mm_img<D>(img1, roff, negmask, T, dT2);
#pragma unroll
      for (int I = 0; I < NBI; ++I)
#pragma unroll
        for (int J = 0; J < NJ; ++J) {
          T[I][J] = T2[I][J];
          dT[I][J] = dT2[I][J];
        }
    }
    // ---- grad[k] = Re <e^{ams + mu} dT, G_k> = Re( conj(e^{ams + mu}) <dT, G_k> ), complex inner product <Z, G> = sum conj(Z) G ----
    {
      double sn, cs;
      sincos(ams_i + mu_i, &sn, &cs);
      const double er = exp(ams_r + mu_r);
      const double pr = er * cs, pi = er * sn;
      if (A.zout != nullptr) {  // Z_n = e^{shift} dT: the cotangent of the generator X_n
        double* dst = reinterpret_cast<double*>(A.zout) + ((long)sample * A.N + n0 + (act ? t : 0)) * D * D * 2;
        store_plain<D>(dT, dst, pr, pi, nullptr, lp, act);
      }
      double trr = 0.0, tri = 0.0;
#pragma unroll
      for (int I = 0; I < NBI; ++I)
#pragma unroll
        for (int J = 0; J < NJ; ++J)
          if (2 * I - 4 * J >= -1 && 2 * I - 4 * J <= 3) {
            const bool on = (((lp.r >> 1) - lp.c) == 4 * J - 2 * I) && (2 * I + rhalf < D);
            const double v = on ? dT[I][J] : 0.0;
            if (lp.r & 1)
              tri += v;
            else
              trr += v;
          }
      for (int k = 0; k < K; ++k) {
        const double* tk = tab + (k + 1) * (MAT + 4);
        // trace part: conj(tr Z) mu_k
        double re = fma(tk[MAT + 0], trr, tk[MAT + 1] * tri);
        double im = fma(tk[MAT + 1], trr, -tk[MAT + 0] * tri);
#pragma unroll
        for (int I = 0; I < NBI; ++I)
#pragma unroll
          for (int J = 0; J < NJ; ++J) {
            const double z = dT[I][J];
            re = fma(z, tk[toff + I * 4 * W + J * 4], re);
            const double go = tk[poff + I * 4 * W + J * 4];  // r even: Im G of my element; r odd: Re G
            im = (lp.r & 1) ? fma(-z, go, im) : fma(z, go, im);
          }
        double part = fma(pr, re, pi * im);
        part += __shfl_xor(part, 1);
        part += __shfl_xor(part, 2);
        part += __shfl_xor(part, 16);
        part += __shfl_xor(part, 32);
        if (act && lp.idx16 == 0) A.grad[((long)sample * K + k) * A.N + n0 + t] = part;
      }
    }
    // ---- A <- dU_n^H A = e^{mu} T A ----
    {
      Mat V;
      write_image<D>(T, img0, woff);
      mat_zero<D>(V);
      mm_img<D>(img0, roff, negmask, Aa, V);
#pragma unroll
      for (int I = 0; I < NBI; ++I)
#pragma unroll
        for (int J = 0; J < NJ; ++J) Aa[I][J] = V[I][J];
      ams_r += mu_r;
      ams_i = c3p_phase_add(ams_i, mu_i);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Backward sweep for REAL Hamiltonians (the case of every dressed lab-frame transmon model): reverse mode through the
// real cos / sin evaluation of the forward kernel instead of the forward-mode pair evaluation of complex T18 above.
// With X = -iY (Y real symmetric), dU = C - iS, and the adjoint state carried TRANSPOSED, N = M^T:
//   R = dU N = (M dU)^T  ->  the cotangents of C and S are REAL and may be symmetrised:  C_bar = sym Re R, S_bar = -sym Im R;
//   every adjoint of the symmetric stage is a symmetrised product of symmetric matrices, 2 sym(A_bar B) = A_bar B + B A_bar
//   (two upper-triangle products whose left operands come from registers, as in the forward kernel);
//   grad[k, n] = scale <Y_bar, Y_k> + Re(mu_k conj(tr N));   N <- R conj(dU)  (the only product with a general LEFT operand:
//   R goes through a real LDS image).
// ~600 MFMAs per slice at D = 9 against ~1500 of the complex pair evaluation.  The economised degree-6 cos / sin pair while the
// segment's bound stays within C3P_MM6_THETA (no squaring), otherwise the degree-8 pair (radius C3P_MM8_THETA) with up to SDG_MAXS
// squarings; samples that are not real, or need more squarings, are left to the complex kernel (same norm bound, same decision).
// ---------------------------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(64, 1) smalld_grad_real_kernel(SmallGradArgs A) {
  using C = SD<D>;
  constexpr int W = C::W, MAT = C::MAT;
  constexpr int NB = RD<D>::NB, WR = 4 * NB + 1, RIMG = 4 * NB * WR;
  typedef double RMat[NB][NB];
  const int lane = threadIdx.x;
  LanePos lp;
  lp.r = lane >> 4;
  lp.b = (lane >> 2) & 3;
  lp.c = lane & 3;
  lp.idx16 = lp.r * 4 + lp.c;
  const int K = A.K;
  double* tab = c3p_sd_lds;
  double* rimg = tab + (1 + K) * (MAT + 4);  // per chain: Re R, Im R as real row-major images (row stride WR)
  double* sg = rimg + 4 * 2 * RIMG;
  double* csb = sg + 4 * K * A.Lmax;  // column sums of the tables (the segment's norm bound)

  const long chain = (long)blockIdx.x * 4 + lp.b;
  const long nchains = (long)A.B * A.S;
  const bool valid = chain < nchains;
  const long cc = valid ? chain : nchains - 1;
  const int sample = (int)(cc / A.S);
  const int seg = (int)(cc - (long)sample * A.S);
  const int n0 = (int)(((long)seg * A.N) / A.S);
  const int n1 = (int)(((long)(seg + 1) * A.N) / A.S);
  const int len = n1 - n0;

  const double* gt0 = A.tables + (long)(A.tab_per_sample ? sample : 0) * (1 + K) * (MAT + 4);
  for (int e = lane; e < (1 + K) * (MAT + 4); e += 64) tab[e] = gt0[e];
  __syncthreads();
  // the forward kernel's bound (column by column: c3p_sd_segment_norm), from the same tables
  sd_colsums<D>(tab, K, csb, lane);
  __syncthreads();
  double nrm = c3p_sd_segment_norm(csb, K, lp.idx16, [&](int k) {
    const double* s = A.signals + ((long)sample * K + k) * A.N + n0;
    double cmax = 0.0;
    for (int t = lp.idx16; t < A.Lmax; t += 16) {
      const double v = (valid && t < len) ? s[t] : 0.0;
      sg[(lp.b * K + k) * A.Lmax + t] = v;
      cmax = fmax(cmax, fabs(v));
    }
    cmax = fmax(cmax, __shfl_xor(cmax, 1));
    cmax = fmax(cmax, __shfl_xor(cmax, 2));
    cmax = fmax(cmax, __shfl_xor(cmax, 16));
    cmax = fmax(cmax, __shfl_xor(cmax, 32));
    return cmax;
  });
  nrm = fmax(nrm, __shfl_xor(nrm, 4));
  nrm = fmax(nrm, __shfl_xor(nrm, 8));
  nrm = readfirstlane_f64(nrm);
  bool realH = true;
  for (int k = 0; k <= K; ++k) realH = realH && (tab[k * (MAT + 4) + MAT + 3] == 0.0);
  // (without per-sample tables the four chains of a wave may belong to different samples, but then all samples share
  // the tables; with per-sample tables S % 4 == 0 and the wave has one sample)
  const int ps = __builtin_amdgcn_readfirstlane(c3p_squarings(nrm, C3P_MM8_THETA));
  if (!(__builtin_amdgcn_readfirstlane((int)realH) != 0) || ps > SDG_MAXS) return;
  const double scale = ldexp(1.0, -ps);
  __syncthreads();

  const int swap_lane = 16 * lp.c + 4 * lp.b + lp.r;
  const int tail_lane = 16 * lp.c + 4 * lp.b;
  const int row0_lane = 4 * lp.b + lp.c;
  int yo[NB];
  double ymask[NB];
#pragma unroll
  for (int I = 0; I < NB; ++I) {
    const bool ok = 4 * I + lp.r < D;
    yo[I] = (2 * (ok ? 4 * I + lp.r : 0) + 1) * W + lp.c;
    ymask[I] = ok ? 1.0 : 0.0;
  }
  auto zero = [&](RMat& m) {
#pragma unroll
    for (int I = 0; I < NB; ++I)
#pragma unroll
      for (int J = 0; J < NB; ++J) m[I][J] = 0.0;
  };
  // acc (all tiles) += A B for symmetric A, B (operand tiles filled)
  auto prod = [&](const RMat& Am, const RMat& Bm, RMat& acc) { mm_symfull<D>(Am, Bm, acc, tail_lane); };
  // out = f (P + P^T) on the tiles a product reads as operands (rows I < KM in full, upper tiles of the others): element
  // (4J + c, 4I + r) of P sits in lane (c, r) of tile (J, I).  One round of lane swaps, no separate mirror fill.
  auto mirror = [&](const RMat& P, double f, RMat& out) {
#pragma unroll
    for (int I = 0; I < NB; ++I)
#pragma unroll
      for (int J = sym_j0<D>(I); J < NB; ++J) out[I][J] = f * (P[I][J] + __shfl(P[J][I], swap_lane));
  };

  // N = M^T at the end of this segment
  RMat Nr, Ni;
  {
    const double* src = reinterpret_cast<const double*>(A.Mb) + cc * D * D * 2;
#pragma unroll
    for (int I = 0; I < NB; ++I)
#pragma unroll
      for (int J = 0; J < NB; ++J) {
        const int row = 4 * I + lp.r, col = 4 * J + lp.c;
        const bool ok = valid && row < D && col < D;
        Nr[I][J] = ok ? src[(col * D + row) * 2 + 0] : 0.0;
        Ni[I][J] = ok ? src[(col * D + row) * 2 + 1] : 0.0;
      }
  }

  // Two instances of the slice loop, the branch outside (as in the forward kernel): MM6 = the economised degree-6 pair (scaled norm
  // <= 0.83: cfg2) -- Horner step in W^3, no W^4: one forward product and one adjoint product less per slice; otherwise the
  // degree-8 pair with W^4 (theta = 1.85).
  const bool small_var = __builtin_amdgcn_readfirstlane((int)(nrm * scale <= C3P_MM6_THETA)) != 0;
  auto sweep = [&](auto mm6_tag) {
  constexpr bool MM6 = decltype(mm6_tag)::value;
  for (int t = A.Lmax - 1; t >= 0; --t) {
    const bool act = valid && t < len;
    const double sc = act ? scale : 0.0;
    // ---- forward: Y, W = Y^2, ..., cos Y, sin Y (as in smalld_chain_kernel) ----
    RMat Y;
#pragma unroll
    for (int I = 0; I < NB; ++I) {
      const double f = -sc * ymask[I];
#pragma unroll
      for (int J = sym_j0<D>(I); J < NB; ++J) Y[I][J] = f * lds_ld(tab + yo[I] + J * 4);
    }
    for (int k = 0; k < K; ++k) {
      const double ck = sc * sg[(lp.b * K + k) * A.Lmax + t];
      const double* tk = tab + (k + 1) * (MAT + 4);
#pragma unroll
      for (int I = 0; I < NB; ++I) {
        const double f = -ck * ymask[I];
#pragma unroll
        for (int J = sym_j0<D>(I); J < NB; ++J) Y[I][J] = fma(f, lds_ld(tk + yo[I] + J * 4), Y[I][J]);
      }
    }
    RMat W1, W2, W3, W4, acc, acs, Cm, Sp, S0;
    zero(W1), zero(W2), zero(W3), zero(W4), zero(S0);
    mm_sym<D>(Y, Y, W1, tail_lane);
    sym_fill<D>(W1, swap_lane);
    mm_sym<D>(W1, W1, W2, tail_lane);
    sym_fill<D>(W2, swap_lane);
    mm_sym<D>(W1, W2, W3, tail_lane);
    if constexpr (!MM6) mm_sym<D>(W2, W2, W4, tail_lane);
    sym_fill<D>(W3, swap_lane);
    if constexpr (MM6) {
      // cos = (c0 + c1 W + c2 W^2) + W^3 (c3 + c4 W + c5 W^2 + c6 W^3)
      rcomb<D, true>(acc, c3p_mm6_cos[3], c3p_mm6_cos[4], c3p_mm6_cos[5], c3p_mm6_cos[6], W1, W2, W3, lp);
      rcomb<D, true>(acs, c3p_mm6_sinc[3], c3p_mm6_sinc[4], c3p_mm6_sinc[5], c3p_mm6_sinc[6], W1, W2, W3, lp);
      rcomb<D, false, true>(Cm, c3p_mm6_cos[0], c3p_mm6_cos[1], c3p_mm6_cos[2], 0.0, W1, W2, W3, lp);
      rcomb<D, false, true>(Sp, c3p_mm6_sinc[0], c3p_mm6_sinc[1], c3p_mm6_sinc[2], 0.0, W1, W2, W3, lp);
      mm_sym2<D>(W3, acc, Cm, acs, Sp, tail_lane);
    } else {
      sym_fill<D>(W4, swap_lane);
      rcomb<D, true>(acc, c3p_mm8_cos[4], c3p_mm8_cos[5], c3p_mm8_cos[6], c3p_mm8_cos[7], W1, W2, W3, lp);
      rcomb<D, true>(acs, c3p_mm8_sinc[4], c3p_mm8_sinc[5], c3p_mm8_sinc[6], c3p_mm8_sinc[7], W1, W2, W3, lp);
#pragma unroll
      for (int I = 0; I < NB; ++I)
#pragma unroll
        for (int J = sym_j0<D>(I); J < NB; ++J) {
          acc[I][J] = fma(c3p_mm8_cos[8], W4[I][J], acc[I][J]);
          acs[I][J] = fma(c3p_mm8_sinc[8], W4[I][J], acs[I][J]);
        }
      rcomb<D, true, true>(Cm, c3p_mm8_cos[0], c3p_mm8_cos[1], c3p_mm8_cos[2], c3p_mm8_cos[3], W1, W2, W3, lp);
      rcomb<D, true, true>(Sp, c3p_mm8_sinc[0], c3p_mm8_sinc[1], c3p_mm8_sinc[2], c3p_mm8_sinc[3], W1, W2, W3, lp);
      mm_sym2<D>(W4, acc, Cm, acs, Sp, tail_lane);
    }
    sym_fill<D>(Cm, swap_lane);
    sym_fill<D>(Sp, swap_lane);
    mm_sym<D>(Y, Sp, S0, tail_lane);
    sym_fill<D>(S0, swap_lane);
    // squarings, every level kept for the way back: C' = (C - S)(C + S), S' = 2 S C
    RMat Cl[SDG_MAXS], Sl[SDG_MAXS], Cf, Sf;
#pragma unroll
    for (int I = 0; I < NB; ++I)
#pragma unroll
      for (int J = sym_j0<D>(I); J < NB; ++J) {
        Cf[I][J] = Cm[I][J];
        Sf[I][J] = S0[I][J];
      }
#pragma unroll
    for (int j = 0; j < SDG_MAXS; ++j)
      if (j < ps) {
        RMat Dm, Sm, C2, SC;
#pragma unroll
        for (int I = 0; I < NB; ++I)
#pragma unroll
          for (int J = sym_j0<D>(I); J < NB; ++J) {
            Cl[j][I][J] = Cf[I][J];
            Sl[j][I][J] = Sf[I][J];
            Dm[I][J] = Cf[I][J] - Sf[I][J];
            Sm[I][J] = Cf[I][J] + Sf[I][J];
            C2[I][J] = SC[I][J] = 0.0;
          }
        mm_sym<D>(Dm, Sm, C2, tail_lane);
        mm_sym<D>(Sf, Cf, SC, tail_lane);
#pragma unroll
        for (int I = 0; I < NB; ++I)
#pragma unroll
          for (int J = I; J < NB; ++J) {
            Cf[I][J] = C2[I][J];
            Sf[I][J] = 2.0 * SC[I][J];
          }
        sym_fill<D>(Cf, swap_lane);
        sym_fill<D>(Sf, swap_lane);
      }
    sym_fill_rest<D>(Cf, swap_lane);  // the whole matrices: right operands of the update of N
    sym_fill_rest<D>(Sf, swap_lane);
    // ---- R = dU N = (C - iS)(Nr + i Ni) with three real products ----
    RMat Rr, Ri;
    {
      RMat Ps, Nd, P1, P2, P3;
#pragma unroll
      for (int I = 0; I < NB; ++I)
#pragma unroll
        for (int J = 0; J < NB; ++J) {
          if (J >= sym_j0<D>(I)) Ps[I][J] = Cf[I][J] + Sf[I][J];
          Nd[I][J] = Ni[I][J] - Nr[I][J];
          P1[I][J] = P2[I][J] = P3[I][J] = 0.0;
        }
      mm_symA<D>(Cf, Nr, P1, row0_lane, 1.0);
      mm_symA<D>(Sf, Ni, P2, row0_lane, 1.0);
      mm_symA<D>(Ps, Nd, P3, row0_lane, 1.0);
#pragma unroll
      for (int I = 0; I < NB; ++I)
#pragma unroll
        for (int J = 0; J < NB; ++J) {
          Rr[I][J] = P1[I][J] + P2[I][J];
          Ri[I][J] = (P3[I][J] + P1[I][J]) - P2[I][J];
        }
    }
    // tr N (= tr M): the trace-shift part of the gradient
    double trr = 0.0, tri = 0.0;
#pragma unroll
    for (int I = 0; I < NB; ++I) {
      const bool on = (lp.r == lp.c) && (4 * I + lp.r < D);
      trr += on ? Nr[I][I] : 0.0;
      tri += on ? Ni[I][I] : 0.0;
    }
    // the images of R for the update of N (written now, read at the end of the slice)
    wave_sync();
#pragma unroll
    for (int I = 0; I < NB; ++I)
#pragma unroll
      for (int J = 0; J < NB; ++J) {
        rimg[(lp.b * 2 + 0) * RIMG + (4 * I + lp.r) * WR + 4 * J + lp.c] = Rr[I][J];
        rimg[(lp.b * 2 + 1) * RIMG + (4 * I + lp.r) * WR + 4 * J + lp.c] = Ri[I][J];
      }
    wave_sync();
    // ---- cotangents of cos / sin: C_bar = sym Re R, S_bar = -sym Im R (upper tiles, then the operand tiles) ----
    RMat Cb, Sb;
    mirror(Rr, 0.5, Cb);
    mirror(Ri, -0.5, Sb);
    // Every cotangent below is A_bar B + B A_bar = P + P^T with ONE full product P = A_bar B (18 MFMAs + a 9-FMA tail
    // at D = 9) and the mirror by lane swaps -- against two upper-triangle products (24 + 12); products that feed the same
    // cotangent are summed (in the accumulators, or by one FMA per element) BEFORE the mirror.
    // ---- back through the squarings: C_bar = {C_bar', C} + {S_bar', S},  S_bar = {S_bar', C} - {C_bar', S} ----
#pragma unroll
    for (int j = SDG_MAXS - 1; j >= 0; --j)
      if (j < ps) {
        RMat Pc, Ps, Pt;
        zero(Pc), zero(Ps), zero(Pt);
        prod(Cb, Cl[j], Pc);
        prod(Sb, Sl[j], Pc);
        prod(Sb, Cl[j], Ps);
        prod(Cb, Sl[j], Pt);
#pragma unroll
        for (int I = 0; I < NB; ++I)
#pragma unroll
          for (int J = 0; J < NB; ++J) Ps[I][J] -= Pt[I][J];
        mirror(Pc, 1.0, Cb);
        mirror(Ps, 1.0, Sb);
      }
    // ---- back through S = Y Sp, Cm = Cm0 + W4 acc, Sp = Sp0 + W4 acs and the powers ----
    RMat Yb2, Spb, W4b, accb, acsb;
    {
      RMat Pa, Pb;
      zero(Pa), zero(Pb);
      prod(Sb, Sp, Pa);
      prod(Sb, Y, Pb);
      mirror(Pa, 1.0, Yb2);  // 2 x sym(S_bar Sp)
      mirror(Pb, 0.5, Spb);  // sym(S_bar Y)
    }
    {
      RMat Pw, Pd, Pf;
      zero(Pw), zero(Pd), zero(Pf);
      prod(Cb, acc, Pw);
      prod(Spb, acs, Pw);
      prod(Cb, MM6 ? W3 : W4, Pd);
      prod(Spb, MM6 ? W3 : W4, Pf);
      mirror(Pw, 0.5, W4b);   // sym(C_bar acc) + sym(Sp_bar acs): the cotangent of the Horner power (W^3 in the degree-6 variant)
      mirror(Pd, 0.5, accb);  // sym(W4 C_bar)
      mirror(Pf, 0.5, acsb);  // sym(W4 Sp_bar)
    }
    RMat W1b, W2b, W3b;
#pragma unroll
    for (int I = 0; I < NB; ++I)
#pragma unroll
      for (int J = sym_j0<D>(I); J < NB; ++J) {
        const double ab = accb[I][J], sb = acsb[I][J], cb = Cb[I][J], pb = Spb[I][J];
        if constexpr (MM6) {
          W1b[I][J] = c3p_mm6_cos[1] * cb + c3p_mm6_sinc[1] * pb + c3p_mm6_cos[4] * ab + c3p_mm6_sinc[4] * sb;
          W2b[I][J] = c3p_mm6_cos[2] * cb + c3p_mm6_sinc[2] * pb + c3p_mm6_cos[5] * ab + c3p_mm6_sinc[5] * sb;
          W3b[I][J] = W4b[I][J] + c3p_mm6_cos[6] * ab + c3p_mm6_sinc[6] * sb;  // (W4b holds the Horner power's cotangent)
        } else {
          W1b[I][J] = c3p_mm8_cos[1] * cb + c3p_mm8_sinc[1] * pb + c3p_mm8_cos[5] * ab + c3p_mm8_sinc[5] * sb;
          W2b[I][J] = c3p_mm8_cos[2] * cb + c3p_mm8_sinc[2] * pb + c3p_mm8_cos[6] * ab + c3p_mm8_sinc[6] * sb;
          W3b[I][J] = c3p_mm8_cos[3] * cb + c3p_mm8_sinc[3] * pb + c3p_mm8_cos[7] * ab + c3p_mm8_sinc[7] * sb;
          W4b[I][J] = W4b[I][J] + c3p_mm8_cos[8] * ab + c3p_mm8_sinc[8] * sb;
        }
      }
    {
      // W4 = W2^2, W3 = W W2:  W2_bar += {W4_bar, W2} + sym(W3_bar W),  W_bar += sym(W3_bar W2)   (degree 6: no W4)
      RMat Pi, Pg, Ph, q, h;
      zero(Pi), zero(Pg), zero(Ph);
      if constexpr (!MM6) prod(W4b, W2, Pi);
      prod(W3b, W1, Pg);
      prod(W3b, W2, Ph);
#pragma unroll
      for (int I = 0; I < NB; ++I)
#pragma unroll
        for (int J = 0; J < NB; ++J) Pi[I][J] = fma(0.5, Pg[I][J], Pi[I][J]);
      mirror(Pi, 1.0, q);
      mirror(Ph, 0.5, h);
#pragma unroll
      for (int I = 0; I < NB; ++I)
#pragma unroll
        for (int J = sym_j0<D>(I); J < NB; ++J) {
          W2b[I][J] += q[I][J];
          W1b[I][J] += h[I][J];
        }
    }
    {
      RMat Pj, q;  // W2 = W^2:  W_bar += {W2_bar, W}
      zero(Pj);
      prod(W2b, W1, Pj);
      mirror(Pj, 1.0, q);
#pragma unroll
      for (int I = 0; I < NB; ++I)
#pragma unroll
        for (int J = sym_j0<D>(I); J < NB; ++J) W1b[I][J] += q[I][J];
    }
    RMat Yb;
    {
      RMat Pk;  // W = Y^2:  Y_bar = sym(S_bar Sp) + {W_bar, Y}
      zero(Pk);
      prod(W1b, Y, Pk);
      mirror(Pk, 1.0, Yb);
#pragma unroll
      for (int I = 0; I < NB; ++I)
#pragma unroll
        for (int J = I; J < NB; ++J) Yb[I][J] = fma(0.5, Yb2[I][J], Yb[I][J]);
    }
    // ---- grad[k] = scale <Y_bar, Y_k> (full-matrix inner product of symmetric matrices) + Re(mu_k conj(tr N)) ----
    for (int k = 0; k < K; ++k) {
      const double* tk = tab + (k + 1) * (MAT + 4);
      double part = 0.0;
#pragma unroll
      for (int I = 0; I < NB; ++I)
#pragma unroll
        for (int J = I; J < NB; ++J) {
          const double yk = -ymask[I] * lds_ld(tk + yo[I] + J * 4);
          part = fma((I == J ? sc : 2.0 * sc) * Yb[I][J], yk, part);
        }
      part = fma(tk[MAT + 0], trr, fma(tk[MAT + 1], tri, part));
      part += __shfl_xor(part, 1);
      part += __shfl_xor(part, 2);
      part += __shfl_xor(part, 16);
      part += __shfl_xor(part, 32);
      if (act && lp.idx16 == 0) A.grad[((long)sample * K + k) * A.N + n0 + t] = part;
    }
    // ---- N <- R conj(dU) = (Rr + i Ri)(C + iS): general left operand from its LDS image, three real products ----
    {
      RMat Ps, Q1, Q2, Q3;
#pragma unroll
      for (int I = 0; I < NB; ++I)
#pragma unroll
        for (int J = 0; J < NB; ++J) {
          Ps[I][J] = Cf[I][J] + Sf[I][J];
          Q1[I][J] = Q2[I][J] = Q3[I][J] = 0.0;
        }
      const double* ir = rimg + (lp.b * 2 + 0) * RIMG;
      const double* ii = rimg + (lp.b * 2 + 1) * RIMG;
#pragma unroll
      for (int Kk = 0; Kk < NB; ++Kk)
#pragma unroll
        for (int I = 0; I < NB; ++I) {
          const double fr = lds_ld(ir + (4 * I + lp.c) * WR + 4 * Kk + lp.r);  // A layout: lane (r, c) <- R[4I + c][4K + r]
          const double fi = lds_ld(ii + (4 * I + lp.c) * WR + 4 * Kk + lp.r);
          const double fs = fr + fi;
#pragma unroll
          for (int J = 0; J < NB; ++J) {
            Q1[I][J] = mfma4(fr, Cf[Kk][J], Q1[I][J]);
            Q2[I][J] = mfma4(fi, Sf[Kk][J], Q2[I][J]);
            Q3[I][J] = mfma4(fs, Ps[Kk][J], Q3[I][J]);
          }
        }
#pragma unroll
      for (int I = 0; I < NB; ++I)
#pragma unroll
        for (int J = 0; J < NB; ++J) {
          Nr[I][J] = Q1[I][J] - Q2[I][J];
          Ni[I][J] = (Q3[I][J] - Q1[I][J]) - Q2[I][J];
        }
    }
  }
  };
  if (small_var)
    sweep(std::true_type{});
  else
    sweep(std::false_type{});
}

template <int D>
hipError_t launch_grad_real_t(const SmallGradArgs& A, hipStream_t st) {
  using C = SD<D>;
  constexpr int NB = RD<D>::NB, RIMG = 4 * NB * (4 * NB + 1);
  const long nchains = (long)A.B * A.S;
  const unsigned grid = (unsigned)((nchains + 3) / 4);
  const size_t lds = (size_t)((1 + A.K) * (C::MAT + 4 + SD_CSW) + 8 * RIMG + 4 * A.K * A.Lmax) * sizeof(double);
  if (lds > 60 * 1024) return hipErrorInvalidValue;
  C3P_LAUNCH(smalld_grad_real_kernel<D>, dim3(grid), dim3(64), lds, st, A);
  return hipGetLastError();
}

template <int D>
hipError_t launch_grad_t(const SmallGradArgs& A, hipStream_t st) {
  using C = SD<D>;
  const long nchains = (long)A.B * A.S;
  const unsigned grid = (unsigned)((nchains + 3) / 4);
  const size_t lds = (size_t)((1 + A.K) * (C::MAT + 4 + SD_CSW) + 8 * C::MAT + 4 * A.K * A.Lmax) * sizeof(double);
  if (lds > 60 * 1024) return hipErrorInvalidValue;
  C3P_LAUNCH(smalld_grad_kernel<D>, dim3(grid), dim3(64), lds, st, A);
  return hipGetLastError();
}

template <int D>
hipError_t launch_grad_general_t(const SmallGradArgs& A, hipStream_t st) {
  using C = SD<D>;
  const long nchains = (long)A.B * A.S;
  const unsigned grid = (unsigned)((nchains + 3) / 4);
  const size_t lds = (size_t)(2 * (1 + A.K) * (C::MAT + 4) + 8 * C::MAT + 4 * A.K * A.Lmax) * sizeof(double);
  if (lds > 60 * 1024) return hipErrorInvalidValue;
  if (A.hs != nullptr)
    C3P_LAUNCH((smalld_grad_general_kernel<D, true>), dim3(grid), dim3(64), lds, st, A);
  else
    C3P_LAUNCH((smalld_grad_general_kernel<D, false>), dim3(grid), dim3(64), lds, st, A);
  return hipGetLastError();
}

template <int D>
hipError_t launch_prep_t(const PrepArgs& P, int nsamp, hipStream_t st) {
  C3P_LAUNCH(smalld_prep_kernel<D>, dim3((unsigned)(nsamp * (1 + P.K))), dim3(64), 0, st, P);
  return hipGetLastError();
}

// The model record: one workgroup forms the block that the chain kernel's inline build leaves behind its table barrier -- the same
// build_tables, table k by wave k mod 8, in this translation unit -- and copies it out of LDS as it stands: (1 + K) tables of
// MAT + 4 doubles, then (1 + K) x SD_CSW column sums.  A chain launch that is handed the record copies it back (A.record).
template <int D>
__global__ void __launch_bounds__(512) smalld_record_kernel(SmallArgs A, double* record) {
  constexpr int MAT = SD<D>::MAT;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwv = (int)(blockDim.x >> 6);
  const int T = (1 + A.K) * (MAT + 4), R = T + (1 + A.K) * SD_CSW;
  double* tab = c3p_sd_lds;
  double* csb = tab + T;
  build_tables<D>(A, 0, tab, csb, lane, wv, nwv, []() {});
  __syncthreads();
  for (int e = threadIdx.x; e < R; e += blockDim.x) record[e] = tab[e];
}

template <int D>
hipError_t launch_record_t(const SmallArgs& A, double* record, hipStream_t st) {
  const size_t lds = (size_t)(1 + A.K) * (SD<D>::MAT + 4 + SD_CSW) * sizeof(double);
  if (lds > 60 * 1024) return hipErrorInvalidValue;
  C3P_LAUNCH(smalld_record_kernel<D>, dim3(1), dim3(512), lds, st, A, record);
  return hipGetLastError();
}

}  // namespace

#define SD_DISPATCH(FN, ...)                                   \
  switch (Dm) {                                                \
    case 2: return FN<2>(__VA_ARGS__);                         \
    case 3: return FN<3>(__VA_ARGS__);                         \
    case 4: return FN<4>(__VA_ARGS__);                         \
    case 5: return FN<5>(__VA_ARGS__);                         \
    case 6: return FN<6>(__VA_ARGS__);                         \
    case 7: return FN<7>(__VA_ARGS__);                         \
    case 8: return FN<8>(__VA_ARGS__);                         \
    case 9: return FN<9>(__VA_ARGS__);                         \
    case 10: return FN<10>(__VA_ARGS__);                       \
    case 11: return FN<11>(__VA_ARGS__);                       \
    case 12: return FN<12>(__VA_ARGS__);                       \
    default: return hipErrorInvalidValue;                      \
  }

#if C3P_SMALLD_HAS(2)
hipError_t c3p_launch_smalld_grad_real(const SmallGradArgs& A, hipStream_t st) {
  const int Dm = A.Dm;
  SD_DISPATCH(launch_grad_real_t, A, st)
}
#endif

#if C3P_SMALLD_HAS(1)
int c3p_smalld_mat_doubles(int Dm) {
  const int NBI = (Dm + 1) / 2, NJ = (Dm + 3) / 4;
  return 4 * NBI * (4 * NJ + 1);
}

int c3p_smalld_img_doubles(int Dm) {
  const int NBI = (Dm + 1) / 2, NJ = (Dm + 3) / 4;
  const int mat = 4 * NBI * (4 * NJ + 1);
  return ((mat - 12 + 31) / 32) * 32 + 12;
}

size_t c3p_smalld_table_doubles(int Dm, int K) { return (size_t)(1 + K) * (c3p_smalld_mat_doubles(Dm) + 4); }

bool c3p_smalld_supported(int Dm) { return Dm >= 2 && Dm <= C3P_SMALLD_MAX; }

size_t c3p_smalld_record_doubles(int Dm, int K) { return c3p_smalld_table_doubles(Dm, K) + (size_t)(1 + K) * SD_CSW; }

hipError_t c3p_launch_smalld_record(const SmallArgs& A, double* record, hipStream_t st) {
  const int Dm = A.Dm;
  SD_DISPATCH(launch_record_t, A, record, st)
}

hipError_t c3p_launch_smalld_chain(const SmallArgs& A, hipStream_t st) {
  const int Dm = A.Dm;
  SD_DISPATCH(launch_chain_t, A, st)
}

hipError_t c3p_launch_smalld_grad(const SmallGradArgs& A_, hipStream_t st) {
  const int Dm = A_.Dm;
  SmallGradArgs A = A_;
  A.skip_real = 0;
  // real Hamiltonians first (reverse mode through the cos / sin evaluation), then the general sweep for the rest; the
  // per-slice generator cotangents (zout) only exist in the general sweep
  if (A.zout == nullptr && !c3p_opt_on(C3P_OPT_no_real_grad)) {
    const hipError_t e = c3p_launch_smalld_grad_real(A, st);
    if (e != hipSuccess) return e;
    A.skip_real = 1;
  }
  SD_DISPATCH(launch_grad_t, A, st)
}

hipError_t c3p_launch_smalld_grad_general(const SmallGradArgs& A, hipStream_t st) {
  const int Dm = A.Dm;
  SD_DISPATCH(launch_grad_general_t, A, st)
}

hipError_t c3p_launch_smalld_prep(const PrepArgs& P, int Dm, int nsamp, hipStream_t st) {
  SD_DISPATCH(launch_prep_t, P, nsamp, st)
}
#endif
