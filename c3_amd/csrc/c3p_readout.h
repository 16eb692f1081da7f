// Launcher interface of the read-out epilogue and its vector-Jacobian product (c3p_readout.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/c3prop.h"
#include "c3p_common.h"

// sequences of one set that a workgroup of the two element-wise kernels serves (c3_amd/readout.py: SEQ_BLOCK)
#define C3P_READOUT_SEQ_BLOCK 32
// threads of every read-out kernel; the per-set sums stride over their values with this step (readout.py: REDUCE_THREADS)
#define C3P_READOUT_THREADS 256
// largest dimension served: populations and confused values of one workgroup live in LDS, SEQ_BLOCK (D + R) doubles
#define C3P_READOUT_MAX_D 81

struct ReadoutArgs {
  const cplx* x;         // [P,S,M] sequence states
  int P, S, M, D, R, V;  // V = 1 with label weights, else R
  int density;           // M == D^2: populations are Re x[n (D + 1)]
  const double* conf;    // [R,D] (conf_bstride 0) or [P,R,D]; null = identity (R == D)
  long conf_bstride;
  const double* label_w;  // [R] or null
  const double* rescale;  // (scale, offset): [2] (rescale_bstride 0) or [P,2]; null = none
  long rescale_bstride;
  const double *meas, *stds, *shots;  // [P,S,V]
  int estimator;
  double* sim;      // [P,S,V]
  double* sim_raw;  // [P,S,V] value before the rescale: caller's buffer or workspace (the reverse pass reads it), or null
  double* goals;    // [P]
  double* terms;    // [P,S,V] workspace: the estimator's summands
  double* pop;      // [P,S,D] workspace (reverse pass: conf_bar reads it), or null
  // reverse pass only
  const double* goal_weights;  // [P]
  cplx* x_bar;                 // [P,S,M]
  double* v_bar;               // [P,S,V] workspace: cotangent of the value before the rescale
  double* sim_bar;             // [P,S,V] workspace: cotangent of sim
  double* conf_bar;            // [P,R,D] or null
  double* rescale_bar;         // [P,2] or null
  double* pop_bar;             // [P,S,D] or null
};

hipError_t c3p_launch_readout(const ReadoutArgs& a, hipStream_t st);
hipError_t c3p_launch_readout_vjp(const ReadoutArgs& a, hipStream_t st);
