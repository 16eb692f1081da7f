// Launcher interface of the signal-synthesis kernels (c3p_signal.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/c3prop.h"

struct SynthArgs {
  const double* env;      // [B,K,E,C3P_ENV_NPAR]
  const int* shape;       // [K,E], < 0 = slot unused
  const double* carrier;  // [B,K,2]: LO angular frequency, V->Hz factor
  double t_start, t_end, awg_res, sim_res;
  int B, K, E, Na, N;
  double* iq;       // [B,K,2,Na] AWG-resolution inphase / quadrature
  double* signals;  // [B,K,N]
};

// The coefficient table of the C3P_ENVT_* shapes (c3p_synth_tab): components with such an id read their block of it.
struct SynthTabArgs {
  const double* tab;  // [B,T]
  const int* tidx;    // [K,E,2]: {offset into the row, M}
  int T;
};

hipError_t c3p_launch_synth(const SynthArgs& A, hipStream_t st);
hipError_t c3p_launch_synth_tab(const SynthArgs& A, const SynthTabArgs& X, hipStream_t st);
// d loss/d signals [B,K,N] -> d loss/d env_params [B,K,E,NPAR] (amp, xy_angle, freq_offset, delta slots) and
// d loss/d carrier [B,K,2]; giq [B,K,2,Na] and gcar_part [B,K,Na,2] are scratch, A.iq is recomputed.
hipError_t c3p_launch_synth_vjp(const SynthArgs& A, const double* gsig, double* giq, double* gcar_part, double* genv,
                                double* gcar, hipStream_t st);
// the same with a coefficient table, and gtab [B,T]: d loss/d env_tab (0 outside the blocks and in the t_bin slots)
hipError_t c3p_launch_synth_tab_vjp(const SynthArgs& A, const SynthTabArgs& X, const double* gsig, double* giq, double* gcar_part,
                                    double* genv, double* gcar, double* gtab, hipStream_t st);

// The device chain behind a line: AWG -> DAC -> Response -> Mixer -> VoltsToHertz (kind 0) or FluxTuning (kind 1).
struct SynthChainArgs {
  SynthArgs S;
  const int* kind;     // [K] C3P_LINE_KIND_*
  const double* line;  // [B,K,C3P_LINE_NPAR]
  double* taps;        // [B,K,tap_stride] scratch: the normalised Response taps, tap_stride >= N - 1
  long tap_stride;
};
int c3p_chain_tiles(int N);       // sample tiles per line
int c3p_chain_part_stride(void);  // doubles per tile in `part`
hipError_t c3p_launch_chain(const SynthChainArgs& C, hipStream_t st);
hipError_t c3p_launch_chain_tab(const SynthChainArgs& C, const SynthTabArgs& X, hipStream_t st);
// scratch: gcs [B,K,2,N], part [B,K,c3p_chain_tiles(N),c3p_chain_part_stride()], giq [B,K,2,Na], gcar_part [B,K,Na,2];
// outputs genv [B,K,E,NPAR], gcar [B,K,2], gline [B,K,C3P_LINE_NPAR]
hipError_t c3p_launch_chain_vjp(const SynthChainArgs& C, const double* gsig, double* gcs, double* part, double* giq, double* gcar_part,
                                double* genv, double* gcar, double* gline, hipStream_t st);
hipError_t c3p_launch_chain_tab_vjp(const SynthChainArgs& C, const SynthTabArgs& X, const double* gsig, double* gcs, double* part,
                                    double* giq, double* gcar_part, double* genv, double* gcar, double* gline, double* gtab,
                                    hipStream_t st);
