/* c3prop.h -- C ABI of libc3prop.so, the MI355X (gfx950) implementation of
 * C3's piecewise-constant propagator hot path.
 *
 * The reference (q-optimize/c3) is pure Python/TensorFlow: it has no FFI for
 * this path.  The boundary it exposes is the Python plugin slot
 * `Experiment.set_prop_method(callable)` (c3/experiment.py:76-91) whose callable
 * is invoked as `propagation(model, gen, instr, folding_stack, batch_size)`
 * (c3/experiment.py:472-478).  The numerical inner boundary that this library
 * replaces is
 *
 *     dUs = tf_batch_propagate(h0, hks, signals, dt, batch_size, col_ops, lindbladian)
 *                                               (c3/libraries/propagation.py:460-515)
 *     U   = tf_matmul_n(dUs, folding_stack)     (c3/utils/tf_utils.py:144-163)
 *
 * plus the ODE state solver `ode_solver` (c3/libraries/propagation.py:687-752).
 * Each entry point below cites the reference function it stands in for.
 * `INTEGRATION.md` shows the ctypes binding a C3 maintainer would add.
 *
 * Conventions
 *  - complex128 = interleaved (re, im) doubles, C (row-major) order -- numpy /
 *    TensorFlow layout.  Pointers are typed `const void*` / `void*` for those.
 *  - All pointers are DEVICE pointers unless C3P_HOST_PTRS is set in `flags`,
 *    in which case the library stages inputs/outputs through its own device
 *    buffers (synchronous).
 *  - `stream` is a hipStream_t (NULL = the default stream).  Device-pointer
 *    calls are asynchronous with respect to the host.
 *  - Return value 0 = success; negative = error, message via c3p_last_error()
 *    (thread-local).  The Python wrapper re-raises `Exception("C3:Error: ...")`
 *    like the reference (c3/experiment.py:465-468).
 *  - The caller owns every buffer it passes.  The library owns only a lazily
 *    grown per-device workspace, released by c3p_shutdown().
 *  - Thread-safe.  The workspace is ONE set per device, guarded by a per-device
 *    mutex at enqueue time (different devices do not serialise each other).  Calls
 *    on one stream are ordered by the stream; a call on ANOTHER stream of the same
 *    device first makes its stream wait (hipStreamWaitEvent) for an event recorded,
 *    at that moment, on the stream of the previous call (a one-stream caller pays no
 *    event per call), so two streams never run kernels on the shared workspace at
 *    once -- results are correct from any number of streams, but calls on one
 *    device do not overlap each other.
 */
#ifndef C3PROP_H
#define C3PROP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the entry points declared here are exported */
#pragma GCC visibility push(default)

/* flags */
#define C3P_HOST_PTRS 0x1     /* all data pointers are host memory                    */
#define C3P_PER_SLICE_H 0x2   /* h0 is [N,D,D] (or [B,N,D,D] with h0_bstride): branch B
                                 of pwc, use_control_fields=False (propagation.py:295-308) */
#define C3P_ORDER_RIGHT 0x4   /* c3p_matmul_chain: elems[0]@...@elems[N-1] (tf_matmul_right) */
#define C3P_FORCE_GENERIC 0x8 /* use the generic LDS kernel even where a specialised one exists */
#define C3P_SEQ_SUPEROP 0x20  /* c3p_seq_chain, population mode: the table holds superoperators, population = |x[0]| */
#define C3P_HERMITIAN_H 0x10  /* c3p_pwc_lindblad: the caller DECLARES h0 and every hk Hermitian (the library does not check
                                 device memory).  The Lindblad generator is then real in a basis of Hermitian matrices and the
                                 chain of one qubit / qutrit or two qubits (D = 2, 3, 4) runs in real arithmetic (c3p_smallr.hip); other shapes
                                 ignore the flag (D = 7, 8, 9 detect the case on the device).  Declared wrongly: wrong results.
                                 The reference makes no such distinction (propagation.py:551-585): c3_amd/propagation.py sets
                                 the flag after checking the arrays. */

#define C3P_COL_PER_SAMPLE 0x40 /* Lindblad PWC entries: col_ops is [B,C,D,D], sample b uses col_ops[b] (one dissipator and one
                                 table set per sample, as with a per-sample h0).  Honoured by c3p_pwc_lindblad (every route,
                                 C3P_PER_SLICE_H and dUs_out included), c3p_pwc_lindblad_vjp, c3p_pwc_lindblad_model_vjp and
                                 _model_vjp_hb (grad_col_ops[b] is then the cotangent of col_ops[b]) and c3p_reserve; an error
                                 in c3p_pwc_unitary, c3p_pwc_lindblad_taped / _vjp_taped and c3p_ode_solve / _vjp. */

/* kernels selected (returned by c3p_last_kernel, for tests/bench reporting) */
#define C3P_KERNEL_NONE 0
#define C3P_KERNEL_GENERIC_LDS 1
#define C3P_KERNEL_GENERIC_GLOBAL 2
#define C3P_KERNEL_SMALLD 3
#define C3P_KERNEL_MFMA 4
#define C3P_KERNEL_ODE_WG 5  /* workgroup-per-sample ODE kernel (c3p_ode.hip)            */
#define C3P_KERNEL_ODE_ROW 6 /* lane-row ODE kernels (c3p_ode_row.hip, c3p_ode_rowq.hip)  */
#define C3P_KERNEL_ODE_MFMA 7 /* matrix-core rho-valued ODE kernel, 17 <= D <= 48 (c3p_ode_rhoq.hip) */
#define C3P_KERNEL_ODE_ROW_OR_WG 8 /* both launched; the DEVICE picks: real operators -> lane rows, complex -> workgroup kernel */
#define C3P_KERNEL_SEQ 9 /* indexed gate-sequence chains (c3p_seq.hip)                          */
#define C3P_KERNEL_SEQ_VJP 10 /* reverse sweep of the indexed gate-sequence chains (c3p_seq_vjp.hip)  */
#define C3P_KERNEL_ODE_VJP 11 /* discrete adjoint of the ODE state solvers (c3p_ode_vjp.hip)           */
#define C3P_KERNEL_DRESS 12 /* batched dressing: Jacobi eigensolver, frame rule, T^+ A T (c3p_dress.hip) */
#define C3P_KERNEL_DRESS_VJP 13 /* vector-Jacobian product of the dressing step (c3p_dress.hip)         */
#define C3P_KERNEL_READOUT 14 /* read-out epilogue: populations, confusion, rescale, estimator (c3p_readout.hip) */
#define C3P_KERNEL_READOUT_VJP 15 /* its vector-Jacobian product (c3p_readout.hip)                              */

/* ODE solver / step ids (propagation.py:27-32 solver_slicing; :886-904 steps) */
#define C3P_SOLVER_RK4 0
#define C3P_SOLVER_RK38 1
#define C3P_SOLVER_RK5 2
#define C3P_SOLVER_TSIT5 3
#define C3P_STEP_SCHRODINGER 0
#define C3P_STEP_VON_NEUMANN 1
#define C3P_STEP_LINDBLAD 2

/* Tuning / diagnostic options: one process-wide table of integers (kernel selection switches, segment counts; the list
 * with one line per option is C3P_OPTION_LIST in c3_amd/csrc/c3p_kernels.h).  `value` is a decimal integer, "all" (= 2)
 * or NULL / "unset" (back to the default, -1).  The table is initialised ONCE, at the first use, from environment
 * variables of the same names in upper case with the prefix C3P_ (C3P_NO_REGD=1 python ...): later changes of the
 * environment are not seen -- use this call.  Thread-safe (atomic loads / stores); a call in flight on another thread
 * sees either value.  No reference counterpart (the reference has no kernel selection).  Unknown name: -1 and
 * c3p_last_error(); c3p_get_option returns -2 for an unknown name, -1 for an option that is not set. */
int c3p_set_option(const char* name, const char* value);
long c3p_get_option(const char* name);

int c3p_version(void);
int c3p_device_count(void);
const char* c3p_last_error(void);
int c3p_last_kernel(void);
/* The kernels the most recent compute call of this thread launched, as "file: kernel<template arguments> xCOUNT; ..." in
 * launch order (names resolved from the host function pointers: what ran, not what was planned).  Writes at most cap - 1
 * characters + NUL into buf (may be NULL) and returns the full length.  Diagnostic: INTEGRATION.md's dispatch table is
 * generated from it (tools/dispatch_table.py).  No reference counterpart. */
int c3p_last_kernel_detail(char* buf, int cap);
/* Device time (ms) of the main kernel(s) of the most recent call that records
 * it -- the c3p_pwc_* entries and their gradients, and c3p_ode_solve,
 * c3p_ode_solve_vjp and c3p_rk4_unitary on every route -- measured with
 * hipEvents on the stream it was launched on; valid after that stream has
 * been synchronised.  An entry that does not record leaves the previous
 * call's time in place.  Only recorded when profiling was enabled with
 * c3p_set_profiling(1).  Returns < 0 if nothing was recorded. */
int c3p_set_profiling(int enable); /* per device: acts on the current device's workspace */
double c3p_last_kernel_ms(void);
void c3p_shutdown(void);

/* Workspace management.  The library owns one workspace per device (segment products, generator tables, arenas), grown
 * lazily by the first call that needs more -- which synchronises the device, frees and allocates (not legal inside a
 * stream capture, and a latency cliff in a serving loop).  c3p_reserve sizes it for one call shape ahead of time
 * (arguments as c3p_pwc_unitary / c3p_pwc_lindblad; device-pointer calls only): afterwards calls of that shape, or of
 * any shape that needs no more, neither allocate nor synchronise, and ONE c3p_pwc_* call can be captured into a hipGraph
 * (a call whose workspace would have to grow during a capture fails with an error instead).
 * c3p_workspace_generation counts (re)allocations of the current device's workspace: constant = steady state.
 * Reference analogue: none (TensorFlow owns its allocator; nothing on this path is retained between calls). */
int c3p_reserve(int lindblad, int B, int K, int N, int D, int C, int flags);
long c3p_workspace_generation(void);

/* U[b] = diag(exp(i fr_phase[b])) * prod_n exp(-i (h0 + sum_k signals[b,k,n] hks[k]) dt)
 *
 * Replaces, for B independent parameter samples at once:
 *   tf_propagation_vectorized (propagation.py:426-440) via tf_batch_propagate (:460-515),
 *   tf_matmul_n (tf_utils.py:144-193) / tf_matmul_left (:120-129),
 *   and the frame-rotation left-multiply of compute_propagators (experiment.py:482-509).
 *
 *   h0       c128 [D,D]; with C3P_PER_SLICE_H: [N,D,D]; element stride between samples
 *            h0_bstride (0 = shared by all samples)
 *   hks      c128 [K,D,D] (ignored when K == 0); stride between samples hks_bstride (0 = shared)
 *   signals  f64  [B,K,N]  real control amplitudes (propagation.py:293 casts them to c128)
 *   fr_phase f64  [B,D] or NULL
 *   U_out    c128 [B,D,D]
 *   dUs_out  c128 [B,N,D,D] or NULL (partial propagators, experiment.py:523-533)
 */
int c3p_pwc_unitary(const void* h0, int64_t h0_bstride, const void* hks, int64_t hks_bstride,
                    const double* signals, double dt, int B, int K, int N, int D, int flags,
                    const double* fr_phase, void* U_out, void* dUs_out, void* stream);

/* The same call with a prebuilt model record.  An optimiser or model-learning loop calls the propagator thousands of times with
 * one model (h0, hks, dt) and new control amplitudes; at 2 <= D <= 12 every workgroup of the chain kernel otherwise rebuilds the
 * generator tables of that model in each launch.  A record is that block, built once, bit for bit what the kernel builds:
 *   c3p_pwc_record_bytes  size of the record for (D, K), or 0 where no record is served (D outside 2 .. 12, K > 8)
 *   c3p_pwc_record_build  one launch on `stream` into `record` (device memory of the caller, c3p_pwc_record_bytes(D, K) bytes);
 *                         h0 c128 [D,D], hks c128 [K,D,D], device pointers, operators shared by the batch
 *   c3p_pwc_unitary_rec   c3p_pwc_unitary with `record`.  The record is used by the unitary table route with shared operators
 *                         (both batch strides 0, no C3P_PER_SLICE_H, no C3P_FORCE_GENERIC, no C3P_HOST_PTRS, dUs_out NULL,
 *                         prep_kernel option off); a NULL record or any other call takes the route of c3p_pwc_unitary exactly.
 * The call trusts the record: it must have been built from the h0, hks, dt and K it is passed with (rebuild it after changing
 * them in place).  The library keeps no table of records and keys nothing by device address; the run allocates nothing and
 * launches nothing but what c3p_pwc_unitary launches.  Reference analogue: none. */
size_t c3p_pwc_record_bytes(int D, int K);
int c3p_pwc_record_build(const void* h0, const void* hks, double dt, int K, int D, int flags, void* record, void* stream);
int c3p_pwc_unitary_rec(const void* h0, int64_t h0_bstride, const void* hks, int64_t hks_bstride,
                        const double* signals, double dt, int B, int K, int N, int D, int flags,
                        const double* fr_phase, void* U_out, void* dUs_out, const void* record, void* stream);

/* Lindblad superoperator propagator (propagation.py:551-585):
 *   L[n] = -i (H[n] (x) I - I (x) H[n]^T) + sum_c [ (C(x)I)(I(x)C^T)^+ - 1/2 (C(x)I)^+(C(x)I) - 1/2 (I(x)C^T)(I(x)C^T)^+ ]
 *   U[b] = diag(exp(i fr_phase[b])) * prod_n exp(L[n] dt),   matrices are [D*D, D*D]
 *   col_ops  c128 [C,D,D]
 *   fr_phase f64 [B,D*D] or NULL (phases of tf_super(FR), experiment.py:499-503)
 *   U_out    c128 [B,D*D,D*D];  dUs_out c128 [B,N,D*D,D*D] or NULL
 */
int c3p_pwc_lindblad(const void* h0, int64_t h0_bstride, const void* hks, int64_t hks_bstride,
                     const double* signals, const void* col_ops, int C, double dt, int B, int K,
                     int N, int D, int flags, const double* fr_phase, void* U_out, void* dUs_out,
                     void* stream);

/* out[i] = expm(A[i]) for a batch of n [D,D] matrices: the tf.linalg.expm call sites
 * (propagation.py:378,422,440,456,584). */
int c3p_expm(const void* A, int n, int D, int flags, void* out, void* stream);

/* Ordered product of a list: out[b] = M[b,N-1] @ ... @ M[b,1] @ M[b,0]
 * (tf_matmul_n tf_utils.py:144-163 and tf_matmul_left :120-129; with C3P_ORDER_RIGHT
 * tf_matmul_right :132-141).  M is c128 [B,N,D,D]. */
int c3p_matmul_chain(const void* M, int B, int N, int D, int flags, void* out, void* stream);

/* Superoperator builders (tf_utils.py:257-289) on a batch of n [D,D] matrices:
 *   which = 0: spre(A) = A (x) I;  1: spost(A) = I (x) A^T;  2: super(A) = spre(A) spost(A^+) = A (x) conj(A)
 *   out c128 [n, D*D, D*D] */
int c3p_superop(const void* A, int n, int D, int which, int flags, void* out, void* stream);
/* out[i] = kron(A[i], B[i]);  A [n,Da,Da], B [n,Db,Db], out [n,Da*Db,Da*Db] (tf_kron, tf_utils.py:257-267) */
int c3p_kron(const void* A, const void* Bm, int n, int Da, int Db, int flags, void* out, void* stream);

/* ODE state solver (propagation.py:687-752 + model.py:641-697 + tf_utils.py:521-559):
 * integrates B independent samples with N RK steps each.
 *   solver   C3P_SOLVER_*;  step C3P_STEP_* (LINDBLAD needs col_ops, C > 0)
 *   ts0, dt  first sample time and spacing of the (uniform) signal grid
 *   init     c128 [B, D, M] with M = 1 (state vector, SCHRODINGER) or M = D (density matrix);
 *            init_bstride = 0 shares one initial state
 *   states   c128 [B,N,D,M] if want_all else [B,D,M]
 */
int c3p_ode_solve(const void* h0, const void* hks, const double* signals, const void* col_ops,
                  int C, double dt, int B, int K, int N, int D, int solver, int step,
                  const void* init, int64_t init_bstride, int want_all, int flags, void* states,
                  void* stream);

/* Discrete adjoint of c3p_ode_solve: gradients with respect to the control signals and the initial state, exact for the
 * arithmetic the forward kernels do.  Stands in for the tape over goal_run_ode / goal_run_ode_only_final
 * (c3/optimizers/optimalcontrol.py:230-292, differentiated by c3/optimizers/optimizer.py:206-216) with the state fidelity
 * state_transfer_from_states (c3/libraries/fidelities.py:793-816).
 *   h0 .. init_bstride, flags   as for c3p_ode_solve (device pointers, or host pointers with C3P_HOST_PTRS)
 *   states_bar   c128 [B,D,M] cotangent of the final state, or with bar_all c128 [B,N,D,M]: the cotangent of every
 *                trajectory state, injected at its step boundary
 *   target       c128 [D] (target_bstride = 0) or [B,D] (target_bstride = D): the call forms the state-transfer goal from
 *                the final state of its own forward pass and starts the sweep from its cotangent --
 *                M = 1: infid[b] = 1 - |<t|psi_N>| (tf_ketket_fid, tf_utils.py:325-327), psibar = -(z / |z|) t;
 *                M = D: infid[b] = 1 - sqrt(Re <t|rho_N|t>) (tf_dmket_fid, tf_utils.py:320-322); zero where the overlap is zero.
 *                Exactly one of states_bar / target is non-NULL.
 *   grad_signals f64 [B,K,N]   (every element written by one owner in a fixed order: two calls are bitwise equal)
 *   init_bar     c128 [B,D,M] or NULL: the cotangent of the initial state (consecutive gates chain through it)
 *   infid_out    f64 [B] or NULL (target mode);  final_out  c128 [B,D,M] or NULL: the final state of the forward pass
 * The forward pass of the call keeps checkpoints every C steps in a workspace slot of its own (capped at 1 GiB: above it
 * a row / workgroup walks several samples); c3p_last_kernel_detail reports "checkpoint interval C=..." and the size. */
int c3p_ode_solve_vjp(const void* h0, const void* hks, const double* signals, const void* col_ops, int C, double dt, int B,
                      int K, int N, int D, int solver, int step, const void* init, int64_t init_bstride,
                      const void* states_bar, int bar_all, const void* target, int64_t target_bstride, int flags,
                      double* grad_signals, void* init_bar, double* infid_out, void* final_out, void* stream);

/* RK4 "unitary" provider (propagation.py:71-101,221-255: rk4_unitary, gen_u_rk4, gen_dus_rk4,
 * gen_du_rk4, rk4_step; Hamiltonians from get_hs_of_t_ts :104-204 at prop_res = 2):
 * every RK4 step consumes three consecutive Hamiltonian samples h[2j], h[2j+1], h[2j+2].
 *   signals  f64 [B,K,Ns] on the doubled-resolution grid (branch A), or
 *   hs       c128 [Ns,D,D] / [B,Ns,D,D] per-sample Hamiltonians (branch B; hs_bstride 0 = shared)
 *   dt       the full RK step (ts[prop_res] - ts[0])
 *   U_out    c128 [B,D,D]: columns are the propagated basis vectors (gen_u_rk4 :246-255)
 *   dUs_out  c128 [B,(Ns-1)/2,D,D] or NULL: per-step maps with propagated basis vectors as ROWS,
 *            exactly as gen_du_rk4 (:85-92) stacks them
 */
int c3p_rk4_unitary(const void* h0, const void* hks, const double* signals, const void* hs,
                    int64_t hs_bstride, double dt, int B, int K, int Ns, int D, int flags,
                    void* U_out, void* dUs_out, void* stream);

/* Gradient of the propagators with respect to the control samples.  The reference obtains
 * it by taping the goal function (c3/optimizers/optimizer.py:206-216, optimalcontrol.py:219-226); the
 * taped path is c3p_pwc_unitary's (propagation.py:426-440, tf_utils.py:144-193, experiment.py:482-509).
 * Vector-Jacobian product: with d loss = Re sum_ij conj(U_bar[b,i,j]) dU[b,i,j],
 *   grad_signals[b,k,n] = d loss / d signals[b,k,n]      (exact: Frechet derivative of every slice)
 *   U_bar c128 [B,D,D]; grad_signals f64 [B,K,N]; other arguments as c3p_pwc_unitary (branch A only,
 *   Hermitian h0 / hks: the adjoint sweep uses the unitarity of the slices; checked for host pointers).
 *   gen_bar_out c128 [B,N,D,D] or NULL (D <= 64): Z[b,n], the cotangent of the slice generator G_n = -i dt H_n
 *   (d loss = Re sum conj(Z) dG); the gradient w.r.t. MODEL parameters follows by contraction, e.g.
 *   d loss / d h0 = i dt sum_n Z[b,n] (what ModelLearning differentiates, c3/optimizers/modellearning.py:300-341).
 * With C3P_PER_SLICE_H (branch B of pwc, propagation.py:295-308): h0 = the per-slice Hamiltonians [N,D,D] (h0_bstride 0) or
 *   [B,N,D,D], hks / signals / grad_signals NULL, K = 0, and gen_bar_out [B,N,D,D] (required) receives the cotangent of every
 *   slice generator G_n = -i dt H_n, i.e. d loss / d H_n = i dt Z[b,n]: what the tape hands back to model.get_Hamiltonian.
 *   Any dimension: on-chip general-generator sweeps up to D = 40 (nothing assumed about the Hamiltonians), the tiled
 *   backward sweep above.
 */
int c3p_pwc_unitary_vjp(const void* h0, int64_t h0_bstride, const void* hks, int64_t hks_bstride,
                        const double* signals, double dt, int B, int K, int N, int D, int flags,
                        const double* fr_phase, const void* U_bar, double* grad_signals, void* gen_bar_out,
                        void* stream);

/* One optimiser evaluation of a closed-system gate goal, fused: the goal AND its gradient w.r.t. the control samples from ONE
 * pass over the chains.  The reference evaluates goal_run = fid_func(compute_propagators()) (c3/optimizers/optimalcontrol.py:
 * 200-228) under a GradientTape (c3/optimizers/optimizer.py:206-216); the three-call form here is c3p_pwc_unitary ->
 * c3p_gate_overlap (+ the cotangent, element-wise) -> c3p_pwc_unitary_vjp, whose third call recomputes the segment products of
 * the first.  This entry forms them once: the per-sample scan of the backward pass, which multiplies the segment products
 * anyway, evaluates infid[b] of U = FR P and takes its cotangent
 *   U_bar[b] = c s G on (comp_rows x comp_rows),  s = tr(G^+ U[rows,rows]),  c = -2/L^2 (kind 0, unitary_infid fidelities.py:
 *   154-184) or -2/(L(L+1)) (kind 1, average_infid :290-313)
 * as the start of the adjoint sweep.  Arguments as c3p_pwc_unitary_vjp (branch A only, Hermitian h0 / hks) and c3p_gate_infid:
 *   infid_out f64 [B]; grad_signals f64 [B,K,N] = d infid[b] / d signals[b,k,n];
 *   grad_fr_phase f64 [B,D] or NULL = d infid[b] / d fr_phase[b,i] (needs fr_phase); U_out c128 [B,D,D] or NULL.
 * On the on-chip and VALU backward sweeps (D <= 40, or D <= 64 below 384 samples); other shapes: error, use the three calls. */
int c3p_pwc_unitary_goal_vjp(const void* h0, int64_t h0_bstride, const void* hks, int64_t hks_bstride,
                             const double* signals, double dt, int B, int K, int N, int D, int flags,
                             const double* fr_phase, const int32_t* comp_rows, int L, const void* ideal, int kind,
                             double* infid_out, double* grad_signals, double* grad_fr_phase, void* U_out, void* stream);

/* The same vector-Jacobian product through the LINDBLAD path (c3p_pwc_lindblad; the reference tapes
 * tf_propagation_lind just as well, c3/libraries/propagation.py:551-585 under c3/optimizers/optimizer.py:206-216):
 *   U_bar c128 [B,D^2,D^2] (d loss = Re sum conj(U_bar) dU of the superoperators), grad_signals f64 [B,K,N],
 *   fr_phase f64 [B,D^2] or NULL (the row phases c3p_pwc_lindblad applies).
 * The slices are not unitary, so the adjoint state cannot be propagated backwards through inverses: the forward partial
 * products are kept in HBM (N matrices of D^4 complex per sample, processed in chunks of samples that fit 24 GB) and the
 * backward sweep evaluates value and Frechet derivative of every slice's exponential together on the tiled MFMA GEMM
 * (c3p_tiled.hip).  c3p_pwc_unitary_vjp uses the same sweep above D = 40 (any dimension; gen_bar_out up to D = 64: above 40 on the VALU sweep).
 * D = 7, 8, 9 (49 x 49 .. 81 x 81 superoperators, Hermitian Hamiltonians): the whole evaluation in REAL arithmetic in the Hermitian
 * basis -- forward chain kernel keeping the transposed local prefix of every slice, real segment scan, on-chip backward sweep
 * (c3p_regrg.hip); the call synchronises the stream once (it reads back whether every Hamiltonian is Hermitian: a complex
 * generator in that basis falls back to the tiled sweep).
 * D <= 6 (superoperators up to 36 x 36): three kernels per call instead of ~35 launches per slice -- segment products, a scan
 * that leaves prefix and left adjoint at the segment boundaries, and a sweep that stores the prefix of every slice of its
 * segment and evaluates the pair at X_n^H on the way back (general-generator form on the matrix cores: c3p_smalld.hip for
 * D <= 3, c3p_midd.hip for D = 4 .. 6; c3p_grad.hip is the VALU fallback; C3P_TILED_GRAD=1 selects the tiled sweep). */
int c3p_pwc_lindblad_vjp(const void* h0, int64_t h0_bstride, const void* hks, int64_t hks_bstride,
                         const double* signals, const void* col_ops, int C, double dt, int B, int K, int N, int D,
                         int flags, const double* fr_phase, const void* U_bar, double* grad_signals, void* stream);

/* The Lindblad vector-Jacobian product WITH the cotangents of the model operators, for open-system model learning (T1, T2* and
 * temperature enter through col_ops only; the reference tapes tf_propagation_lind, c3/libraries/propagation.py:551-585, under
 * c3/optimizers/optimizer.py:206-216).  Arguments and C3P_HOST_PTRS staging as c3p_pwc_lindblad_vjp, and
 *   grad_signals f64 [B,K,N] or NULL (not wanted); the same arithmetic as c3p_pwc_lindblad_vjp on the VALU sweep (bitwise equal);
 *   grad_h0 c128 [B,D,D], grad_hks c128 [B,K,D,D], grad_col_ops c128 [B,C,D,D]: PER SAMPLE (operators shared by the batch: the
 *     caller sums over b, as with grad_h0 of c3p_pwc_unitary_vjp's gen_bar_out), d loss = Re sum conj(grad) d(operator), every
 *     operator entry an independent complex number, nothing assumed Hermitian (the dissipator is not holomorphic in col_ops).
 * The backward sweep of c3p_grad.hip (general-generator form, VALU) keeps the generator cotangent Z_n of every slice, contracts
 * it to D x D per slice (the adjoint of H -> -i (H (x) 1 - 1 (x) H^T)) and adds up sum_n Z_n for the dissipator; a second kernel
 * adds the segment partials in segment order (bitwise reproducible) and applies the adjoint of the dissipator map.
 * Served for D <= 6 (superoperators up to 36 x 36); a larger D is an error, never a fallback (D = 7, 8, 9 with Hermitian
 * Hamiltonians: c3p_pwc_lindblad_model_vjp_hb below). */
int c3p_pwc_lindblad_model_vjp(const void* h0, int64_t h0_bstride, const void* hks, int64_t hks_bstride, const double* signals,
                               const void* col_ops, int C, double dt, int B, int K, int N, int D, int flags,
                               const double* fr_phase, const void* U_bar, double* grad_signals, void* grad_h0, void* grad_hks,
                               void* grad_col_ops, void* stream);

/* The same cotangents at D = 7, 8, 9 (49 x 49 .. 81 x 81 superoperators; two coupled qutrits, cfg4) from the Hermitian-basis sweep
 * of c3p_pwc_lindblad_vjp (c3p_regrg.hip), arguments and C3P_HOST_PTRS staging as c3p_pwc_lindblad_model_vjp.  At the end of every
 * slice the sweep holds the REAL generator cotangent of that slice in registers; it is summed over the slices of every chain with
 * the weights 1, c_1(n) .. c_K(n) (one owner thread per element, sweep order, no atomics), and a second kernel adds the segments in
 * ascending order, leaves the Hermitian basis and applies the adjoints of H -> -i (H (x) 1 - 1 (x) H^T) and of the dissipator map.
 *   Shapes: D = 7, 8, 9 (D = 6 under the regr_grad_d6 option), 1 <= K <= 16; any other D is an error that names
 *     c3p_pwc_lindblad_model_vjp.
 *   h0 / hks must be Hermitian: the call reads the flags of the table build back (one synchronisation of the stream, as the control
 *     sweep does); a non-Hermitian Hamiltonian is an error ("... must be Hermitian"), never a fallback.
 *   grad_col_ops c128 [B,C,D,D] is the FULL cotangent, every entry an independent complex number: the dissipator preserves
 *     Hermiticity for every C, so nothing is lost in the real basis.
 *   grad_h0 c128 [B,D,D], grad_hks c128 [B,K,D,D] are HERMITIAN matrices: the Hermitian part (g + g^+) / 2 of what the general sweep
 *     returns.  A real generator only sees Hermitian perturbations of H; Re sum conj(grad) dH is exact for every Hermitian dH.
 *   grad_signals f64 [B,K,N] or NULL: bitwise what c3p_pwc_lindblad_vjp returns on the Hermitian-basis sweep under the same options
 *     (same segment count).
 *   All outputs are per sample and bitwise reproducible, and bitwise independent of the sample chunks (grad_chunk) at a fixed
 *     segment count.  The per-sample budget of a chunk counts the partial sums, S (1 + K) D^4 doubles, beside the N D^4 doubles of
 *     transposed prefixes.  c3p_last_kernel reports C3P_KERNEL_MFMA.
 * Not served: D >= 10, non-Hermitian Hamiltonians at D = 7 .. 9, the caller-owned tape (c3p_pwc_lindblad_vjp_taped). */
int c3p_pwc_lindblad_model_vjp_hb(const void* h0, int64_t h0_bstride, const void* hks, int64_t hks_bstride, const double* signals,
                                  const void* col_ops, int C, double dt, int B, int K, int N, int D, int flags,
                                  const double* fr_phase, const void* U_bar, double* grad_signals, void* grad_h0, void* grad_hks,
                                  void* grad_col_ops, void* stream);

/* Open-system optimiser evaluation from ONE forward pass (D = 7, 8, 9: 49 x 49 .. 81 x 81 superoperators, Hermitian Hamiltonians;
 * D = 2, 3: 4 x 4 / 9 x 9 superoperators on the small-D kernels, any Hamiltonian, up to 8 control lines -- there the tape holds
 * the generator tables, the segment products and the slice propagators; D = 4 (two qubits) with C3P_HERMITIAN_H in `flags` of
 * BOTH calls: the real Hermitian-basis kernels -- the flag selects the layout of the tape at D = 2, 3 as well).
 * c3p_pwc_lindblad followed by c3p_pwc_lindblad_vjp computes the chain twice (the second time with the per-slice prefixes the
 * backward sweep reads).  Here the forward call records what the backward pass needs -- the generator tables in the Hermitian
 * basis, the real segment products, the transposed local prefix of every slice -- on a TAPE the caller owns (device memory, as
 * the reference's GradientTape keeps the forward intermediates of tf_propagation_lind, c3/libraries/propagation.py:551-585 under
 * c3/optimizers/optimizer.py:206-216), and the vector-Jacobian product runs from the tape: no second forward pass, nothing of
 * the evaluation lives in the library's shared workspace between the two calls.
 *   c3p_pwc_lindblad_tape_bytes: bytes of the tape for a shape (0: shape not served) and the segment count it is laid out for
 *     (pass it to both calls unchanged: both calls recompute it and fail on a mismatch, for every D.  The layout of the tape
 *     also follows from the library's option table -- c3p_set_option must not be called between the taped forward call and
 *     its vjp; a change that alters the segment count is refused by the vjp call);
 *   c3p_pwc_lindblad_taped: arguments and U_out as c3p_pwc_lindblad (device pointers, flags = 0, no dUs_out);
 *   c3p_pwc_lindblad_vjp_taped: U_bar, fr_phase, grad_signals as c3p_pwc_lindblad_vjp; signals = the ones the tape was recorded
 *     with; per_sample_operators = whether h0 / hks had a batch stride.
 * At D = 7, 8, 9 a non-Hermitian Hamiltonian is an error of the taped forward call (use the untaped pair). */
size_t c3p_pwc_lindblad_tape_bytes(int B, int K, int N, int D, int* segments_out);
int c3p_pwc_lindblad_taped(const void* h0, int64_t h0_bstride, const void* hks, int64_t hks_bstride, const double* signals,
                           const void* col_ops, int C, double dt, int B, int K, int N, int D, int flags, const double* fr_phase,
                           void* U_out, void* tape, size_t tape_bytes, int segments, void* stream);
int c3p_pwc_lindblad_vjp_taped(const void* tape, size_t tape_bytes, int segments, int per_sample_operators, const double* signals,
                               int B, int K, int N, int D, int flags, const double* fr_phase, const void* U_bar,
                               double* grad_signals, void* stream);

/* Control-signal synthesis for the standard drive line LO + AWG -> DAC -> Mixer -> VoltsToHertz
 * (Instruction.get_awg_signal c3/signal/gates.py:341-370, Envelope/EnvelopeDrag
 * c3/signal/pulse.py:88-180, Device.create_ts c3/generator/devices.py:72-122, DigitalToAnalog :306-351,
 * Mixer :914-939, LO :1073-1130 noiseless branch, VoltsToHertz :203-221, envelope shapes
 * c3/libraries/envelopes.py:26,195,201,228,254,374,401,421,470).  A batch is described by B x K x E envelope
 * parameter rows instead of B x K x N samples:
 *   signals[b,k,n] = v2hz * (cos(w t_n) I(t_n) + sin(w t_n) Q(t_n)),
 *   I + iQ = nearest-neighbour upsampling of sum_e amp_e env_e(t - t0_e) exp(i (xy_e - fo_e (t - t0_e)))
 *   sampled on the AWG grid, env_e = mask * (shape - shape(t_before)) [+ i DRAG term].
 *   env_params  f64 [B,K,E,C3P_ENV_NPAR]   rows laid out by the C3P_ENV_* slots below
 *   env_shapes  int32 [K,E]                C3P_ENV_* shape ids, negative = unused slot
 *   carrier     f64 [B,K,2]                {LO angular frequency [rad/s], V_to_Hz factor}
 *   N = (int)(|t_end - t_start| * sim_res), Na = (int)(|t_end - t_start| * awg_res)
 *   awg_iq_out  f64 [B,K,2,Na] or NULL     AWG-resolution inphase, quadrature
 *   signals_out f64 [B,K,N]                what c3p_pwc_* take as `signals`
 */
#define C3P_ENV_NO_DRIVE 0
#define C3P_ENV_RECT 1
#define C3P_ENV_GAUSSIAN_NONORM 2
#define C3P_ENV_FLATTOP 3
#define C3P_ENV_FLATTOP_RISEFALL 4
#define C3P_ENV_COSINE 5
#define C3P_ENV_GAUSSIAN_SIGMA 6 /* envelopes.py:374-398 */
#define C3P_ENV_GAUSSIAN 7       /* envelopes.py:401-418: sigma = t_final / 6 */
#define C3P_ENV_TRAPEZOID 8      /* envelopes.py:201-225 */
#define C3P_ENV_NSHAPES 9

#define C3P_ENV_AMP 0
#define C3P_ENV_XY_ANGLE 1
#define C3P_ENV_FREQ_OFFSET 2
#define C3P_ENV_DELTA 3
#define C3P_ENV_T_FINAL 4
#define C3P_ENV_SIGMA 5
#define C3P_ENV_T_UP 6
#define C3P_ENV_T_DOWN 7
#define C3P_ENV_RISEFALL 8
#define C3P_ENV_DELAY 9
#define C3P_ENV_FLAGS 10 /* C3P_ENVF_* bits stored as a double */
#define C3P_ENV_NPAR 12
#define C3P_ENVF_T_BEFORE 1 /* Envelope(use_t_before=True) */
#define C3P_ENVF_DRAG 2     /* EnvelopeDrag: imag = -delta * dt * d env/dt */

int c3p_synth_signals(const double* env_params, const int32_t* env_shapes, const double* carrier,
                      double t_start, double t_end, double awg_res, double sim_res, int B, int K,
                      int E, int flags, double* awg_iq_out, double* signals_out, void* stream);

/* Vector-Jacobian product of c3p_synth_signals for the commonly optimised pulse parameters (the same
 * GradientTape of optimizers/optimizer.py:206-216 covers Instruction.get_awg_signal gates.py:341-370):
 *   grad_signals f64 [B,K,N]             d loss / d signals (e.g. from c3p_pwc_unitary_vjp)
 *   grad_env     f64 [B,K,E,C3P_ENV_NPAR] d loss / d {amp, xy_angle, freq_offset, delta} in their slots,
 *                                        0 in every other slot (times, sigma, flags are not differentiated)
 *   grad_carrier f64 [B,K,2]             d loss / d {LO angular frequency, V_to_Hz}
 */
int c3p_synth_signals_vjp(const double* env_params, const int32_t* env_shapes, const double* carrier,
                          double t_start, double t_end, double awg_res, double sim_res, int B, int K,
                          int E, int flags, const double* grad_signals, double* grad_env, double* grad_carrier,
                          void* stream);

/* Signal synthesis through the device chain of a flux line (the reference's tunable-coupler generator,
 * test/test_tunable_coupler.py:159-218): AWG -> DAC -> Response -> Mixer -> VoltsToHertz | FluxTuning.  The arguments of
 * c3p_synth_signals plus, per line,
 *   line_kind   int32 [K]                    C3P_LINE_KIND_DRIVE: values = V_to_Hz * mixed (devices.py:203-221)
 *                                            C3P_LINE_KIND_FLUX:  values = F(phi + mixed) - F(phi) (devices.py:457-525),
 *                                            F(x) = (omega_0 - anhar) (cos^2(pi x/phi_0) + d^2 sin^2(pi x/phi_0))^(1/4) + anhar
 *                                            (d = 0: the reference's branch without d); the V_to_Hz slot of `carrier` is ignored
 *   line_params f64 [B,K,C3P_LINE_NPAR]      rows laid out by the C3P_LINE_* slots below
 * Response (devices.py:585-642, tf_utils.py:476-518), applied to the upsampled inphase and quadrature when rise_time > 0:
 *   M = floor(rise_time * sim_res) taps h = r / sum r, r_m = exp(-(t_m - cen)^2 / 2 sigma^2) - exp(-(-1 - cen)^2 / 2 sigma^2),
 *   t = linspace(0, rise_time, M), cen = (rise_time + 1/sim_res) / 2, sigma = rise_time / 4,
 *   y[n] = sum_{m < min(M, n)} h[m] x[n-1-m]  (the reference's zero-padded FFT product and window; y[0] = 0).
 * rise_time <= 0: no Response stage.  rise_time > 0 with M = 0 is an error on host-pointer calls (device-pointer calls
 * cannot look: they run such a line without the stage).  With every kind C3P_LINE_KIND_DRIVE and no rise_time the result
 * equals c3p_synth_signals'.
 */
#define C3P_LINE_KIND_DRIVE 0
#define C3P_LINE_KIND_FLUX 1
#define C3P_LINE_NKINDS 2

#define C3P_LINE_RISE_TIME 0
#define C3P_LINE_PHI_0 1
#define C3P_LINE_PHI 2
#define C3P_LINE_OMEGA_0 3
#define C3P_LINE_ANHAR 4
#define C3P_LINE_D 5
#define C3P_LINE_NPAR 6

int c3p_synth_chain(const double* env_params, const int32_t* env_shapes, const double* carrier, const int32_t* line_kind,
                    const double* line_params, double t_start, double t_end, double awg_res, double sim_res, int B, int K,
                    int E, int flags, double* awg_iq_out, double* signals_out, void* stream);

/* Vector-Jacobian product of c3p_synth_chain: grad_env and grad_carrier as c3p_synth_signals_vjp (d/d V_to_Hz = 0 on a
 * flux line), and
 *   grad_line f64 [B,K,C3P_LINE_NPAR]   d loss / d {phi_0, phi, omega_0, anhar, d} in their slots (0 on a drive line);
 *                                       the rise_time slot is 0: the tap count is a floor, rise_time is not differentiated.
 * Every sum runs in a fixed order: repeated calls return the same bits.
 */
int c3p_synth_chain_vjp(const double* env_params, const int32_t* env_shapes, const double* carrier, const int32_t* line_kind,
                        const double* line_params, double t_start, double t_end, double awg_res, double sim_res, int B,
                        int K, int E, int flags, const double* grad_signals, double* grad_env, double* grad_carrier,
                        double* grad_line, void* stream);

/* Sampled and Fourier pulse envelopes: the parametrisations whose parameters are an array of coefficients
 * (c3/libraries/envelopes.py:31-34 pwc, :37-68 pwc_shape, :104-125 pwc_symmetric, :142-168 fourier_sin, :171-191 fourier_cos).
 * c3p_synth_tab takes the arguments of c3p_synth_chain plus a coefficient table that travels with the envelope rows:
 *   env_shapes int32 [K,E]      C3P_ENV_* ids as before, or a C3P_ENVT_* id below for a component that reads the table
 *   env_tab    f64 [B,T]        one flat row of T doubles per sample, holding every table component's block
 *   tab_index  int32 [K,E,2]    {offset of the block in the row, M} per component, {-1, 0} for a component without a table
 *   line_kind, line_params      may both be NULL: the standard drive line, exactly as c3p_synth_signals
 * A component contributes amp * env * exp(i (xy_angle - freq_offset tau)) to the AWG-resolution I + iQ (gates.py:341-370),
 * tau = t_awg - (t_start + delay), env = mask * (s(tau) - [C3P_ENVF_T_BEFORE] s(tau_before)) (pulse.py:98-141), with s per shape
 * from the component's block:
 *   C3P_ENVT_PWC            inphase[M], quadrature[M]          s_j = inphase[j] + i quadrature[j], one pair per AWG sample: M = Na
 *   C3P_ENVT_PWC_SHAPE      t_bin_start, t_bin_end, inphase[M]  linear interpolation of inphase on the regular grid of M >= 2 knots
 *                                                              from t_bin_start to t_bin_end (both included), 0 outside
 *                                                              (tfp.math.interp_regular_1d_grid, fill values 0)
 *   C3P_ENVT_PWC_SYMMETRIC  as C3P_ENVT_PWC_SHAPE              evaluated at tau > t_final / 2 ? t_final - tau : tau (the row's
 *                                                              C3P_ENV_T_FINAL slot)
 *   C3P_ENVT_FOURIER_SIN    amps[M], freqs[M], phases[M]       s = sum_m amps[m] sin(freqs[m] tau + phases[m])
 *   C3P_ENVT_FOURIER_COS    amps[M], freqs[M]                  s = sum_m amps[m] cos(freqs[m] tau)
 * The other slots of such a component's parameter row (amp, xy_angle, freq_offset, t_final, delay, flags) mean what they
 * mean for the closed-form shapes.  Refused on host-pointer calls: a block that leaves the row, blocks that overlap, M != Na
 * for pwc, M < 2 or t_bin_end <= t_bin_start for the interpolated shapes, C3P_ENVF_DRAG on a table shape, C3P_ENVF_T_BEFORE
 * on pwc (the reference's offset would be the array itself).  Device-pointer calls do not synchronise and cannot look: a block
 * that leaves the row contributes nothing, and those two flags are ignored where they are refused.  c3p_synth_signals and
 * c3p_synth_chain keep refusing C3P_ENVT_* ids.
 */
#define C3P_ENVT_PWC 16
#define C3P_ENVT_PWC_SHAPE 17
#define C3P_ENVT_PWC_SYMMETRIC 18
#define C3P_ENVT_FOURIER_SIN 19
#define C3P_ENVT_FOURIER_COS 20
#define C3P_ENVT_FIRST 16 /* table shape ids are C3P_ENVT_FIRST .. C3P_ENVT_END - 1 */
#define C3P_ENVT_END 21

int c3p_synth_tab(const double* env_params, const int32_t* env_shapes, const double* env_tab, const int32_t* tab_index, int T,
                  const double* carrier, const int32_t* line_kind, const double* line_params, double t_start, double t_end,
                  double awg_res, double sim_res, int B, int K, int E, int flags, double* awg_iq_out, double* signals_out,
                  void* stream);

/* Vector-Jacobian product of c3p_synth_tab: grad_env, grad_carrier and grad_line (NULL with line_kind NULL) as
 * c3p_synth_chain_vjp -- the amp, xy_angle and freq_offset slots hold for the table shapes too -- and
 *   grad_tab f64 [B,T]   d loss / d env_tab in the layout of env_tab: every coefficient (inphase, quadrature, amps, freqs,
 *                        phases).  t_bin_start and t_bin_end are not differentiated: their slots, and every double that
 *                        belongs to no block, are written as 0.
 * Every sum runs in a fixed order without atomics: repeated calls return the same bits.
 */
int c3p_synth_tab_vjp(const double* env_params, const int32_t* env_shapes, const double* env_tab, const int32_t* tab_index, int T,
                      const double* carrier, const int32_t* line_kind, const double* line_params, double t_start, double t_end,
                      double awg_res, double sim_res, int B, int K, int E, int flags, const double* grad_signals,
                      double* grad_env, double* grad_carrier, double* grad_line, double* grad_tab, void* stream);

/* Line filters, DC offset and crosstalk: c3p_synth_tab with distortion stages between DAC and Mixer, an offset between Mixer
 * and VoltsToHertz | FluxTuning, and a mixing matrix over the finished lines.  The arguments of c3p_synth_tab (table and line
 * arguments may be NULL as there) plus
 *   filt_kind    int32 [K,F]                  C3P_FILT_* id per stage slot, negative = unused slot; shared by the batch
 *   filt_params  f64 [B,K,F,C3P_FILT_NPAR]    {C3P_FILT_TAU, C3P_FILT_AMP} per slot
 *   F            stage slots per line; 0 allowed (then both pointers may be NULL)
 *   dc_offset    f64 [B,K] or NULL            DC_Offset (devices.py:1039-1059): added to the mixer output
 *   xtalk        f64 [B,K,K] or NULL          Crosstalk (devices.py:225-292): out[b,k,:] = sum_j xtalk[b,k,j] s[b,j,:]
 * Chain per line, the stages acting on the I and Q pair: AWG -> DAC -> legacy Response (rise_time slot > 0) -> stage 0 ..
 * stage F-1 -> Mixer -> + dc_offset -> VoltsToHertz | FluxTuning; then the crosstalk over all lines.
 * Every stage is the causal convolution y[n] = sum_{m=0..n} h[m] x[n-m] (tf_convolve, tf_utils.py:439-473: zero-padded, no
 * wrap-around, no delay), summed directly with m ascending.  With ts[m] the signal's own centred grid (absolute time, as
 * StepFuncFilter.process reads it, devices.py:719-731):
 *   C3P_FILT_RESPONSE_FFT   ResponseFFT (devices.py:646-701): M = floor(TAU * sim_res) taps, h = r / sum r,
 *                           r[m] = exp(-(lin[m] - cen)^2 / (2 sg^2)) - exp(-(-1 - cen)^2 / (2 sg^2)), lin = linspace(0, TAU, M),
 *                           cen = (TAU - 1/sim_res) / 2, sg = TAU / 4; h[m] = 0 for m >= M
 *   C3P_FILT_EXP_IIR        ExponentialIIR (:735-751):       s(t) = 1 + AMP exp(-t / TAU)
 *   C3P_FILT_HIGHPASS_EXP   HighpassExponential (:755-769):  s(t) = exp(-t / TAU)
 *   C3P_FILT_SKIN_EFFECT    SkinEffectResponse (:773-787):   s(t) = erfc(TAU / 21 / sqrt|t|), the TAU slot holding alpha
 * and for the three step responses h[0] = s(ts[0]), h[m] = s(ts[m]) - s(ts[m-1]).
 * Refused on host-pointer calls: an unknown kind, TAU <= 0 or non-finite (kinds 0-2), M = 0 (kind 0), a non-finite alpha or
 * AMP, filt_kind without filt_params or the reverse.  Device-pointer calls do not synchronise: an unknown kind runs as an
 * unused slot.
 */
#define C3P_FILT_RESPONSE_FFT 0
#define C3P_FILT_EXP_IIR 1
#define C3P_FILT_HIGHPASS_EXP 2
#define C3P_FILT_SKIN_EFFECT 3
#define C3P_FILT_NKINDS 4

#define C3P_FILT_TAU 0
#define C3P_FILT_AMP 1
#define C3P_FILT_NPAR 2

int c3p_synth_filt(const double* env_params, const int32_t* env_shapes, const double* env_tab, const int32_t* tab_index, int T,
                   const double* carrier, const int32_t* line_kind, const double* line_params, const int32_t* filt_kind,
                   const double* filt_params, int F, const double* dc_offset, const double* xtalk, double t_start, double t_end,
                   double awg_res, double sim_res, int B, int K, int E, int flags, double* awg_iq_out, double* signals_out,
                   void* stream);

/* Vector-Jacobian product of c3p_synth_filt: the outputs of c3p_synth_tab_vjp, taken through the stages, plus
 *   grad_filt  f64 [B,K,F,C3P_FILT_NPAR]  TAU and AMP of EXP_IIR, TAU of HIGHPASS_EXP, alpha of SKIN_EFFECT; 0 in every other
 *                                         slot (RESPONSE_FFT's tap count is a floor) and in unused slots
 *   grad_dc    f64 [B,K]                  iff dc_offset
 *   grad_xtalk f64 [B,K,K]                iff xtalk
 * Every sum runs in a fixed order without atomics: repeated calls return the same bits.
 */
int c3p_synth_filt_vjp(const double* env_params, const int32_t* env_shapes, const double* env_tab, const int32_t* tab_index, int T,
                       const double* carrier, const int32_t* line_kind, const double* line_params, const int32_t* filt_kind,
                       const double* filt_params, int F, const double* dc_offset, const double* xtalk, double t_start,
                       double t_end, double awg_res, double sim_res, int B, int K, int E, int flags, const double* grad_signals,
                       double* grad_env, double* grad_carrier, double* grad_line, double* grad_tab, double* grad_filt,
                       double* grad_dc, double* grad_xtalk, void* stream);

/* Fidelity epilogue: overlap[b] = tr(P^T U[b] P G^+), the number behind
 * unitary_infid = 1 - |overlap/L|^2 (c3/libraries/fidelities.py:154-184, tf_unitary_overlap
 * c3/utils/tf_utils.py:330-366) and average_infid = 1 - (|overlap|^2/L + 1)/(L + 1)
 * (fidelities.py:290-313, tf_average_fidelity tf_utils.py:380-401).  The projector of
 * tf_project_to_comp (tf_utils.py:428-436, qt_utils.py:178-193) is a 0/1 selection, passed
 * as the L row indices `comp_rows` of the computational states in the full space.
 *   U c128 [B,D,D]; comp_rows int32 [L]; ideal c128 [L,L]; overlap_out c128 [B]
 */
int c3p_gate_overlap(const void* U, int B, int D, const int32_t* comp_rows, int L, const void* ideal,
                     int flags, void* overlap_out, void* stream);

/* The goal itself, fused: infid[b] = unitary_infid (kind 0: 1 - |overlap / L|^2, fidelities.py:154-184)
 * or average_infid (kind 1: 1 - (|overlap|^2 / L + 1) / (L + 1), fidelities.py:290-313) of every propagator and their sum
 * over the batch -- B scalars (or two) leave the device instead of B matrices, and a batch sharded over GPUs exchanges
 * ONE all-reduce of sum_out instead of an all-gather of U (the mean over noise / parameter instances is what
 * OptimalControlRobust.goal_run_with_grad forms, c3/optimizers/optimalcontrol_robust.py:49-70).
 *   infid_out f64 [B] or NULL; sum_out f64 [2] = {sum_b infid[b], B} or NULL (deterministic summation order)
 */
int c3p_gate_infid(const void* U, int B, int D, const int32_t* comp_rows, int L, const void* ideal, int kind,
                   int flags, double* infid_out, double* sum_out, void* stream);

/* Gate sequences evaluated by index (evaluate_sequences, c3/libraries/propagation.py:588-627, as used by RB, ORBIT and
 * epc_analytical, c3/libraries/fidelities.py:437-591,754-791): for every parameter sample p and sequence s
 *   U_seq[p,s] = G[p, i_{L-1}] ... G[p, i_1] G[p, i_0]        (first gate applied first, as tf_matmul_left)
 * without gathering the factors: every chain reads its indices and then the gates from the table.  One launch per call.
 *   G        c128 [P, n_gates, M, M]; element stride between samples G_bstride (0 = one table shared by every sample).
 *            M = D for unitaries, D^2 for superoperators; 1 <= M <= 256 (M <= 9: one lane per chain, table in LDS)
 *   seqs     int32 [S, Lmax] gate indices (row s uses its first lengths[s] entries); lengths int32 [S], 0 = identity.
 *            Shared by all P samples.
 *   mode     C3P_SEQ_PRODUCT:    out c128 [P,S,M,M] = U_seq
 *            C3P_SEQ_STATE:      out c128 [P,S,M]   = U_seq psi0, psi0 c128 [M]; with C3P_SEQ_PSI0_PER_SAMPLE in flags psi0 is
 *                                c128 [P,M] and sample p starts from psi0[p] (the flag is an error in the other modes)
 *            C3P_SEQ_POPULATION: out f64  [P,S]     = |(U_seq e_0)[0]|^2, or with C3P_SEQ_SUPEROP in flags |(U_seq e_0)[0]|
 *                                (the Lindblad population of vec(|0><0|), fidelities.py:460-470)
 *            The state and population modes are matrix-vector chains: no matrix product is formed.
 * A negative length, a length above Lmax or an index outside [0, n_gates) is an error (never a fault): checked on the
 * host for C3P_HOST_PTRS, otherwise by the kernel, which writes NaN for that sequence and raises a flag the call reads
 * back -- so every call synchronises its stream once (not capturable into a graph). */
#define C3P_SEQ_PRODUCT 0
#define C3P_SEQ_STATE 1
#define C3P_SEQ_POPULATION 2
#define C3P_SEQ_PSI0_PER_SAMPLE 0x80 /* c3p_seq_chain, c3p_seq_chain_vjp, state mode: psi0 is [P,M], one start vector per sample */
int c3p_seq_chain(const void* G, int64_t G_bstride, int n_gates, int M, int P, const int32_t* seqs, int S, int Lmax,
                  const int32_t* lengths, int mode, const void* psi0, int flags, void* out, void* stream);

/* Vector-Jacobian product of c3p_seq_chain w.r.t. the gate table: the reverse sweep of the same chains
 * (x_{t+1} = G[i_t] x_t, first gate applied first), with d loss = Re sum conj(Xbar) dX as c3p_pwc_unitary_vjp.
 * Arguments, flags (C3P_HOST_PTRS, C3P_SEQ_SUPEROP) and validation as c3p_seq_chain, plus
 *   out_bar  the cotangent of what c3p_seq_chain returns in `mode`:
 *            C3P_SEQ_PRODUCT:    c128 [P,S,M,M] (column c = the cotangent of the chain started at e_c)
 *            C3P_SEQ_STATE:      c128 [P,S,M]
 *            C3P_SEQ_POPULATION: f64  [P,S]; the chain's cotangent is 2 pbar x_L[0] e_0, or with C3P_SEQ_SUPEROP
 *                                pbar x_L[0] / |x_L[0]| e_0 (0 where x_L[0] = 0)
 *   G_bar    c128 [P,n_gates,M,M]: Gbar[i_t] += xbar_{t+1} x_t^H over every sequence and position,
 *            xbar_t = G[i_t]^H xbar_{t+1}.  G_bstride == 0 (shared table): [n_gates,M,M] summed over the samples.
 *   out      NULL, or the forward output of `mode` (as c3p_seq_chain), from the same pass.
 * No unitarity is assumed: the states are recomputed from checkpoints kept every C ~ sqrt(Lmax) steps (the kernel and C
 * are reported by c3p_last_kernel_detail).  Workspace O(P S (Lmax / C + C) M) at most, from the library's workspace.
 * Bitwise reproducible: partial sums per workgroup, reduced in a fixed order (no float atomics).  Two launches per call
 * whatever the lengths; a bad length or index is an error as in c3p_seq_chain (the stream is synchronised once). */
int c3p_seq_chain_vjp(const void* G, int64_t G_bstride, int n_gates, int M, int P, const int32_t* seqs, int S, int Lmax,
                      const int32_t* lengths, int mode, const void* psi0, const void* out_bar, int flags, void* G_bar,
                      void* out, void* stream);

/* c3p_seq_chain_vjp in C3P_SEQ_STATE mode with the cotangent of the start vector as one more result.
 *   psi0         c128 [M] (psi0_bstride 0: shared) or one per sample, psi0_bstride elements apart ([P,M]: M)
 *   psi0_bar     c128 [P,M]: psi0_bar[p] = sum_s G[p,i_0]^H ... G[p,i_{L-1}]^H out_bar[p,s], the vector the reverse sweep of
 *                every chain ends on; a sequence of length 0 contributes out_bar[p,s] itself.  Always per sample, also for
 *                a shared psi0 (the caller sums over p, as with grad_h0).
 *   G_bar, out   as c3p_seq_chain_vjp.
 * The sum over the sequences follows G_bar's rule: one partial per workgroup, added by the reduce launch in a fixed order --
 * bitwise reproducible, still two launches per call.  C3P_SEQ_PSI0_PER_SAMPLE is not taken here (psi0_bstride says it). */
int c3p_seq_state_vjp(const void* G, int64_t G_bstride, int n_gates, int M, int P, const int32_t* seqs, int S, int Lmax,
                      const int32_t* lengths, const void* psi0, int64_t psi0_bstride, const void* out_bar, int flags, void* G_bar,
                      void* psi0_bar, void* out, void* stream);

/* Dressing of P models in one launch: Model.update_dressed (c3/model.py:453-534) -- the eigendecomposition of the drift
 * Hamiltonian, the reorder rule of reorder_frame (ordered=True) and T^+ A T for every control and collapse operator.
 *   H        c128 [P,D,D] bare drift Hamiltonians, Hermitian (the lower triangle is read, as eigh does); 2 <= D <= 40
 *   ops      c128 [M,D,D] (ops_bstride 0: one list for every set) or [P,M,D,D] (ops_bstride = elements between two lists);
 *            control Hamiltonians and collapse operators in one list, not necessarily Hermitian; M = 0: none
 *   eig_out  f64  [P,D]   the eigenvalues in the reordered frame (the reference's `eigenframe`)
 *   T_out    c128 [P,D,D] the transform: column i is the eigenvector that overlaps bare state i most (every column's largest
 *            |v|^2 above 0.5), else the reference's greedy assignment (status bit 1); its phase makes T[i,i] real and positive --
 *            for a real symmetric H this is the reference's sign(Re v) rule, for a complex one it defines what the reference
 *            leaves to LAPACK's phase convention
 *   h0_out   c128 [P,D,D] diag(eig_out) exactly (the reference's T^+ H T differs from it by rounding noise eps ||H||)
 *   ops_out  c128 [P,M,D,D] T_p^+ A_m T_p
 *   status_out int32 [P]: bit 1 = reordered by the greedy branch, 4 = the solver did not converge in 30 sweeps (e.g. NaN input;
 *            the outputs of that set are not valid)
 * Any output may be NULL.  Cyclic Jacobi, converged at off(A) <= D 2^-52 ||A||_F: every threshold is relative, results are
 * bitwise reproducible.  One launch, no workspace. */
int c3p_dress(const void* H, const void* ops, int64_t ops_bstride, int P, int M, int D, int flags, double* eig_out, void* T_out,
              void* h0_out, void* ops_out, int32_t* status_out, void* stream);

/* Vector-Jacobian product of c3p_dress (d loss = Re sum conj(Xbar) dX): from T and eig AS RETURNED by it (nothing is solved
 * again) and the cotangents
 *   eig_bar  f64  [P,D] or NULL;   h0_bar c128 [P,D,D] or NULL (h0 = diag(eig): Re diag(h0_bar) adds to eig_bar)
 *   ops_bar  c128 [P,M,D,D] or NULL: cotangents of the dressed operators;   T_bar c128 [P,D,D] or NULL
 * returns
 *   H_bar_out         c128 [P,D,D]: the gradient on the Hermitian H (a Hermitian matrix)
 *   ops_bare_bar_out  c128 [P,M,D,D] = T Gbar_m T^+ for per-set operators; [M,D,D], summed over the sets in a fixed order, for
 *                     shared ones (ops_bstride 0)
 *   status_out        int32 [P]: bit 2 = a pair of eigenvalues closer than 2^-40 max|e| was met; it contributes zero (the
 *                     reference's gradient is infinite there)
 * Outputs may be NULL.  The permutation and the greedy branch are locally constant and contribute nothing. */
int c3p_dress_vjp(const void* T, const double* eig, const void* ops, int64_t ops_bstride, int P, int M, int D, int flags,
                  const double* eig_bar, const void* h0_bar, const void* ops_bar, const void* T_bar, void* H_bar_out,
                  void* ops_bare_bar_out, int32_t* status_out, void* stream);

/* Read-out epilogue of model learning: from the sequence states to the goals of P parameter sets in one call --
 * Experiment.process (c3/experiment.py:355-407) with ConfusionMatrix.confuse and MeasurementRescale.rescale
 * (c3/libraries/tasks.py:107-129,161-178), then an estimator of c3/libraries/estimators.py over the values of every set.
 *   x        c128 [P,S,M] sequence states, as c3p_seq_chain returns them in state mode; M == D: kets, populations |x_n|^2;
 *            M == D^2: density vectors, populations Re x[n (D + 1)].  2 <= D <= 81.
 *   conf     f64  [R,D] (conf_bstride 0: one confusion matrix for every set) or [P,R,D] (conf_bstride = elements between
 *            two of them); NULL: identity, R must be D.  c = conf pop.
 *   label_w  f64  [R] or NULL: with it ONE value per sequence, v = sum_r label_w[r] c_r (V = 1; label_w[r] is how often label r
 *            was listed); without it every c_r is a value (V = R).
 *   rescale  f64  (scale, offset): [2] (rescale_bstride 0) or [P,2] (rescale_bstride 2); NULL: none.  sim = scale v + offset.
 *   meas, stds, shots   f64 [P,S,V]: measured values, their standard deviations, shot counts (stds may be NULL unless the
 *            estimator reads it: C3P_EST_RMS_EXP_STDS)
 *   estimator  one of C3P_EST_*
 *   sim_out     f64 [P,S,V];  sim_raw_out f64 [P,S,V] or NULL: v before the rescale (populations_no_rescale)
 *   goals_out   f64 [P]
 * sim outside (0,1) gives the inf / nan of the reference's arithmetic.  The sum over the S V values of a set runs in a fixed
 * order that depends on S and V alone: the same call returns the same bits, and set p gives the same bits alone as inside a
 * batch.  Two launches; the estimator's summands go through the workspace. */
#define C3P_EST_G_LL_PRIME 0           /* mean(((m - s)^2 / (s (1 - s) / shots) - 1) / 2)                     */
#define C3P_EST_NEG_LOGLKH_GAUSS 1     /* -mean(log N(m; s, sqrt(s (1 - s) / shots)))                          */
#define C3P_EST_NEG_LOGLKH_GAUSS_NORM 2 /* -mean(log N(m; ..) - log N(s; ..)) = mean((m - s)^2 / (2 var))      */
#define C3P_EST_NEG_LOGLKH_GAUSS_NORM_SUM 3 /* the same, summed                                               */
#define C3P_EST_RMS_DIST 4             /* sqrt(mean((m - s)^2))                                                */
#define C3P_EST_RMS_EXP_STDS_DIST 5    /* sqrt(mean(((m - s) / stds)^2))                                       */
#define C3P_EST_RMS_SIM_STDS_DIST 6    /* sqrt(mean((m - s)^2 / (s (1 - s) / shots)))                          */
int c3p_readout_goal(const void* x, int P, int S, int M, int D, const double* conf, int64_t conf_bstride, int R,
                     const double* label_w, const double* rescale, int64_t rescale_bstride, const double* meas,
                     const double* stds, const double* shots, int estimator, int flags, double* sim_out, double* sim_raw_out,
                     double* goals_out, void* stream);

/* c3p_readout_goal and the vector-Jacobian product of  sum_p goal_weights[p] goals[p]  (goal_weights f64 [P]: the w_p / sum w
 * of dv_g_LL_prime).  Inputs as c3p_readout_goal; sim_out, sim_raw_out and goals_out are written with the same bits, and
 *   x_bar_out        c128 [P,S,M], every entry written: the cotangent c3p_seq_chain_vjp reads (d loss = Re sum conj(x_bar) dx),
 *                    2 pop_bar x for kets, pop_bar on the entries n (D + 1) and zero elsewhere for density vectors
 *   conf_bar_out     f64 [P,R,D] or NULL;  rescale_bar_out f64 [P,2] (scale, offset) or NULL: always per set, also for a
 *                    shared read-out (the caller sums over p, as with grad_h0)
 *   pop_bar_out      f64 [P,S,D] or NULL
 * The sums over the sequences run in a fixed order without atomics.  Four or five launches. */
int c3p_readout_goal_vjp(const void* x, int P, int S, int M, int D, const double* conf, int64_t conf_bstride, int R,
                         const double* label_w, const double* rescale, int64_t rescale_bstride, const double* meas,
                         const double* stds, const double* shots, int estimator, const double* goal_weights, int flags,
                         double* sim_out, double* sim_raw_out, double* goals_out, void* x_bar_out, double* conf_bar_out,
                         double* rescale_bar_out, double* pop_bar_out, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* C3PROP_H */
