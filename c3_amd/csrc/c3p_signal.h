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

// Scratch and outputs of the vector-Jacobian product.  gcs, part and gline belong to a line chain and stay NULL without
// one; gtab goes with a coefficient table.  The I/Q rows are recomputed into C.S.iq.
struct SynthVjpBufs {
  double* giq;        // [B,K,2,Na] scratch
  double* gcar_part;  // [B,K,Na,2] scratch
  double* gcs;        // [B,K,2,N] scratch
  double* part;       // [B,K,c3p_chain_tiles(N),c3p_chain_part_stride()] scratch
  double* genv;       // [B,K,E,NPAR]: the amp, xy_angle, freq_offset, delta slots
  double* gcar;       // [B,K,2]
  double* gline;      // [B,K,C3P_LINE_NPAR]
  double* gtab;       // [B,T]: 0 outside the blocks and in the t_bin slots
};

// Line filters, DC offset and crosstalk (c3p_synth_filt): F stage slots per line between DAC (and the legacy Response) and
// Mixer, each a causal convolution over a materialised [B,K,2,N] buffer.
struct SynthFiltArgs {
  const int* fkind;     // [K,F] C3P_FILT_*, < 0 = unused slot
  const double* fpar;   // [B,K,F,C3P_FILT_NPAR]
  int F;
  const double* dc;     // [B,K] or NULL
  const double* xtalk;  // [B,K,K] or NULL
  double* h;            // [B,K,F,N] scratch: every stage's impulse response
  double* buf;          // [F+1,B,K,2,N] scratch: the upsampled DAC (and legacy Response) output, then every stage's output
  double* pre;          // [B,K,N] scratch: the signals before the crosstalk (with xtalk only)
};
struct SynthFiltVjpBufs {
  double* gbuf;    // [B,K,2,N] scratch: the second cotangent buffer (V.gcs is the first)
  double* gh;      // [B,K,N] scratch: d loss / d h of the stage at hand
  double* gpre;    // [B,K,N] scratch: the cotangent before the crosstalk (with xtalk only)
  double* gfilt;   // [B,K,F,C3P_FILT_NPAR]
  double* gdc;     // [B,K] (with dc only)
  double* gxtalk;  // [B,K,K] (with xtalk only)
};
// C.kind == NULL: drive lines without a legacy Response.  V.gcs and V.part are needed whether lines travel or not.
hipError_t c3p_launch_synth_filt(const SynthChainArgs& C, const SynthTabArgs& X, const SynthFiltArgs& Fa, hipStream_t st);
hipError_t c3p_launch_synth_filt_vjp(const SynthChainArgs& C, const SynthTabArgs& X, const SynthFiltArgs& Fa, const double* gsig,
                                     const SynthVjpBufs& V, const SynthFiltVjpBufs& W, hipStream_t st);

// C.kind == NULL: the standard drive line (AWG -> DAC -> Mixer -> VoltsToHertz), only C.S is read.  X == NULL: no
// coefficient table travels with the rows, and the table-free instantiations of the AWG kernels run.
hipError_t c3p_launch_synth(const SynthChainArgs& C, const SynthTabArgs* X, hipStream_t st);
// d loss/d signals gsig [B,K,N] -> V
hipError_t c3p_launch_synth_vjp(const SynthChainArgs& C, const SynthTabArgs* X, const double* gsig, const SynthVjpBufs& V, hipStream_t st);
