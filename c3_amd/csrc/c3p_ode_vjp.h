// Launcher interface of the discrete adjoint of the ODE state solvers (c3p_ode_vjp.hip).
#pragma once
#include "c3p_common.h"
#include "c3p_ode.h"

#define C3P_ODE_VJP_MAX_C 32                       // checkpoint interval cap: the segment states of a 16-lane row stay in LDS
#define C3P_ODE_VJP_WS_CAP ((size_t)1 << 30)       // workspace cap (bytes): above it a row / workgroup walks several samples

struct OdeVjpArgs {
  OdeArgs f;               // the forward problem (operators, signals, init, dt, sizes, solver, step); f.states is unused
  const cplx* states_bar;  // [B,D,M] or (bar_all) [B,N,D,M]; NULL in target mode
  int bar_all;
  const cplx* target;      // [D] or [B,D] (target_bstride); NULL in cotangent mode
  long target_bstride;
  double* grad_signals;    // [B,K,N]
  cplx* init_bar;          // [B,D,M] or NULL
  double* infid;           // [B] or NULL (target mode)
  cplx* final_out;         // [B,D,M] or NULL
  cplx* ws;                // workspace: per launched row / workgroup ws_stride elements
  long ws_stride;
  int Cint, nck;           // checkpoint interval and number of checkpoints, nck = ceil(N / Cint)
  int rows;                // launched rows / workgroups; each walks samples b = v, v + rows, ...
  cplx* scratch;           // workgroup kernel: working matrices when they do not fit the LDS
  long scratch_stride;
};

struct OdeVjpPlan {
  bool row;          // lane-row kernel (Schroedinger step, D <= 16, K <= 4), else the workgroup-per-sample kernel
  int Cint, nck, rows;
  size_t ws_elems;   // per launched row / workgroup
  size_t wg_elems;   // workgroup kernel: working-set elements (LDS or global scratch)
  bool wg_global;
};

OdeVjpPlan c3p_ode_vjp_plan(int B, int K, int N, int D, int M, int C, int step);
hipError_t c3p_launch_ode_vjp(const OdeVjpArgs& V, const OdeVjpPlan& pl, hipStream_t st);
// lane-row instances for K <= 2 and for K = 3, 4 (two translation units of c3p_ode_vjp.hip)
hipError_t c3p_launch_ode_vjp_row_k2(const OdeVjpArgs& V, hipStream_t st);
hipError_t c3p_launch_ode_vjp_row_k4(const OdeVjpArgs& V, hipStream_t st);
