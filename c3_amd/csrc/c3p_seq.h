// Launcher interface of the indexed gate-sequence chain (c3p_seq.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/c3prop.h"
#include "c3p_common.h"

// largest M served (the wave kernel keeps two state vectors of M complex in LDS)
#define C3P_SEQ_MAX_M 256

struct SeqArgs {
  const cplx* G;     // [P or 1, n_gates, M, M] (sample stride G_bstride elements, 0 = shared)
  long G_bstride;
  int n_gates, M, P;
  const int* seqs;     // [S, Lmax] gate indices, first gate applied first
  const int* lengths;  // [S]
  int S, Lmax;
  int mode;            // C3P_SEQ_PRODUCT / _STATE / _POPULATION
  int superop;         // population = |x_0| (vectorised density matrix) instead of |x_0|^2
  const cplx* psi0;    // [M], or [P,M] psi0_bstride elements apart (mode STATE)
  long psi0_bstride;   // 0 = one start vector for every sample
  void* out;           // c128 [P,S,M,M] / c128 [P,S,M] / f64 [P,S]
  int* bad;            // set to 1 by any chain with a negative / too long length or an out-of-range gate index
};

// whether the gate table of one sample is staged in LDS (otherwise it is read from global memory / L2)
bool c3p_seq_table_in_lds(int n_gates, int M);
hipError_t c3p_launch_seq(const SeqArgs& a, hipStream_t st);
