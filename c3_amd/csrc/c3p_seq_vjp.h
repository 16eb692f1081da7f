// Launcher interface of the reverse sweep of the indexed gate-sequence chain (c3p_seq_vjp.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "c3p_seq.h"

struct SeqVjpArgs {
  SeqArgs f;            // the forward chain; f.out is the optional forward output (NULL: not written)
  const void* out_bar;  // cotangent of the forward output: c128 [P,S,M,M] / c128 [P,S,M] / f64 [P,S]
  int C;                // checkpoint interval: x_0, x_C, x_2C, ... are kept, each segment recomputed from its checkpoint
  int nck;              // checkpoints per chain, ceil(Lmax / C) (at least 1)
  int nblk;             // workgroups per sample; workgroup b walks the chains b, b + nblk (x 64 lanes), ...
  cplx* ws;             // checkpoints and segment states, per lane (lane kernel) or per workgroup (wave kernel)
  cplx* slab;           // [P, nblk, n_gates, M, M] partial G_bar of every workgroup, then [P, nblk, M] partial psi0_bar (psi0_bar set)
  cplx* G_bar;          // [P, n_gates, M, M], or [n_gates, M, M] summed over the samples (shared table)
  int shared;           // G_bstride == 0
  cplx* psi0_bar;       // [P, M] or null (mode STATE): the sum over the sample's chains of the adjoint vector at the chain's start
};

struct SeqVjpPlan {
  bool lane;      // lane per chain (M <= 9, n_gates M^2 <= 64) or workgroup per chain
  bool tab_lds;   // wave kernel: gate table staged in LDS
  bool part_lds;  // wave kernel: partial G_bar in LDS (else in the workgroup's slab row, read-modify-write from L2)
  int C, nck, nblk;
  size_t lds, ws_elems, slab_elems;  // LDS bytes per workgroup; workspace / slab sizes in complex elements
};

// want_psi0_bar: the slab also holds one partial start-vector cotangent [M] per workgroup
SeqVjpPlan c3p_seq_vjp_plan(int n_gates, int M, int P, int S, int Lmax, int mode, bool want_psi0_bar = false);
hipError_t c3p_launch_seq_vjp(const SeqVjpArgs& a, const SeqVjpPlan& pl, hipStream_t st);
