// Launcher interface of the batched dressing step and its vector-Jacobian product (c3p_dress.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/c3prop.h"
#include "c3p_common.h"

// largest dimension served: A and V of the Jacobi solve are two [D,D] complex tiles in LDS (51 KB at D = 40)
#define C3P_DRESS_MAX_D 40
// D <= this: one wave per matrix; above: four
#define C3P_DRESS_WAVE_D 16

struct DressArgs {
  const cplx* H;     // [P,D,D] bare drift Hamiltonians (the lower triangle is read)
  const cplx* ops;   // [M,D,D] (ops_bstride 0) or [P,M,D,D]; null with M = 0
  long ops_bstride;  // elements between the operator lists of two sets
  int P, M, D;
  double* eig;   // [P,D] reordered eigenvalues, or null
  cplx* T;       // [P,D,D], or null
  cplx* h0;      // [P,D,D] = diag(eig), or null
  cplx* ops_out; // [P,M,D,D] = T^+ A_m T, or null
  int* status;   // [P], or null
};

struct DressVjpArgs {
  const cplx* T;      // [P,D,D] as returned by the forward call
  const double* eig;  // [P,D]
  const cplx* ops;    // bare operators, as in the forward call
  long ops_bstride;
  int P, M, D;
  const double* eig_bar;  // [P,D] or null
  const cplx* h0_bar;     // [P,D,D] or null (Re diag is read)
  const cplx* ops_bar;    // [P,M,D,D] cotangents of the dressed operators, or null
  const cplx* T_bar;      // [P,D,D] or null
  cplx* H_bar;            // [P,D,D] or null
  cplx* ops_bare_bar;     // [P,M,D,D] (per-set operators) or [M,D,D] (shared: summed over the sets), or null
  int* status;            // [P] or null
};

hipError_t c3p_launch_dress(const DressArgs& a, hipStream_t st);
hipError_t c3p_launch_dress_vjp(const DressVjpArgs& a, hipStream_t st);
