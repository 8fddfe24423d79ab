/*
 * dqmc.h -- C ABI of libdqmc_hip.so, the MI355X (gfx950) local-energy / MCMC evaluator.
 *
 * The reference (deepqmc/deepqmc) has no FFI boundary: its hot path is a set of Python
 * callables.  Each entry point below replaces one of them; the
 * reference-side binding a maintainer would add is the ctypes stub in INTEGRATION.md.
 *
 *   dqmc_wf_eval        <- ansatz.apply(params, phys_conf) -> Psi(sign, log)
 *                          reference src/deepqmc/types.py:107-150,
 *                          wf/nn_wave_function.py:127-173 (vmapped over walkers at
 *                          sampling/electron_samplers.py:76-81)
 *   dqmc_local_energy   <- hamil.local_energy(ansatz)(rng, params, phys_conf)
 *                          hamil.py:156-184, vmapped over walkers at loss/energy.py:50-57
 *   dqmc_mcmc_steps     <- DecorrSampler.sample / MetropolisSampler.sample
 *                          sampling/electron_samplers.py:140-163,347-357
 *   dqmc_langevin_*     <- LangevinSampler._update / .sample, sampling/electron_samplers.py:176-232
 *   dqmc_exchange_step  <- OppositeSpinExchangeSampler.sample's exchange branch, electron_samplers.py:235-330
 *   dqmc_energy_stats   <- EnergyMonitor's mean/std/min/max, observable.py:474-479
 *                          (per-rank partial record; ranks merge them after one all-gather)
 *   dqmc_set_weights    <- a new `params` tree after an optimiser step
 *   dqmc_log_psi_vjp    <- jax.vjp of vmap(ansatz.apply)(., r).log with a cotangent per walker
 *                          (loss/loss_function.py:59-75): the parameter gradient of the energy loss
 *   dqmc_log_psi_jacobian <- the per-walker rows of that Jacobian (natural-gradient / KFAC preconditioners)
 *   dqmc_log_psi_kfac   <- the loss gradient plus the KFAC Kronecker factors of every linear layer
 *   dqmc_log_psi_grad_coords <- jax.grad of ansatz.apply(.).log with respect to r and R (force.py make_grad_log_wf,
 *                          make_grad_nuc_log_wf), vmapped over walkers
 *   dqmc_hf_force       <- the Hellmann-Feynman force estimators of force.py (nuclear_force, evaluate_hf_force_bare,
 *                          evaluate_hf_force_ac_zvq / _zvzbq / _zb), per walker
 *   dqmc_ecp_force      <- evaluate_hf_force_bare / _ac_zb for a Hamiltonian with a Gaussian-type ECP (force.py:286-299 with
 *                          hamil.pot.grad_nonloc_potential, ecp/gaussian_type_ecp.py:257-330, ecp/ecp_force_utils.py)
 *   dqmc_oscillator_strength <- OscillatorStrengthMonitor.compute_observable, observable.py:556-605
 *   dqmc_fd_displace / dqmc_fd_force <- the displacements and the quotient of evaluate_finite_difference_force, force.py:550-606
 *
 * Conventions: plain pointers and sizes only.  Unless marked "host", every pointer is a
 * DEVICE pointer.  Walker-major contiguous layouts: r[B][N][3], R[n_nuc][3].  `real` is
 * float (dtype 0) or double (dtype 1), fixed per context.  Every function returns 0 on
 * success or a negative DQMC_E_* code and never throws; dqmc_last_error() gives a message.
 * A context is bound to one device (every entry point makes it the calling thread's current device) and is
 * not thread-safe; use one context per GPU.
 * All work is enqueued on the stream given at creation (0 = the null stream); functions
 * that return host values synchronise that stream.
 */
#ifndef DQMC_H
#define DQMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DQMC_OK 0
#define DQMC_E_ARG (-1)     /* invalid argument / malformed program */
#define DQMC_E_HIP (-2)     /* a HIP runtime call failed */
#define DQMC_E_NOMEM (-3)
#define DQMC_E_UNSUPPORTED (-4)

/* ---- the layer program ------------------------------------------------------------
 * The wave function is handed over as a flat list of ops acting on per-walker
 * activation buffers.  Activation buffer b has `rows` rows per walker and `width`
 * features per row (width % 4 == 0, zero padded); in memory it is
 * real[B][rows][TP][width], TP = number of forward-Laplacian lanes: lane 0 = value,
 * lanes 1..3N = d/dr_c, lane 3N+1 = Laplacian, further lanes zero padding.  TP = 1 for
 * value-only evaluation (dqmc_wf_eval, MCMC); TP = round_up(3N+2, 16) for the local
 * energy.  Weight offsets index the `real` weight buffer, table offsets the int32 table. */

typedef struct dqmc_buf {
  int32_t rows;
  int32_t width;
} dqmc_buf;

enum dqmc_op_kind {
  /* i: [0]=dst buf [1]=log_rescale [2]=use_spin. Electron-nucleus input features
   * (gnn/electron_gnn.py:596-625): row i = [|d|,dx,dy,dz] per nucleus (+ spin). */
  DQMC_OP_FEAT_EN = 1,
  /* i: [0]=dst buf [1]=table offset of (recv,send) int pairs [2]=n_edge_rows
   * [3]=log_rescale.  Edge features of d = r_recv - r_send (gnn/graph.py:23-31, gnn/edge_features.py:21-123);
   * send >= 0: an electron, send < 0: nucleus -1 - send (the 'ne' edges, d = r_recv - R). */
  DQMC_OP_FEAT_EE = 2,
  /* Forward-Laplacian linear layer y = act(concat(pieces) W + b) (+ residual).
   * i: [0]=n_pieces, then per piece p (p<4) at [1+4p..]: src buf, r0, K (unpadded
   * width used), bcast (1: every dst row of a walker reads src row r0);
   * [17]=dst buf [18]=dst r0 [19]=dst col0 [20]=nrows (per walker) [21]=Nout
   * [22]=W offset [23]=bias offset or -1 [24]=act (0 none, 1 tanh, 2 silu, 3 shifted softplus hkext.py:13-19,
   * 4 the multiplicative backflow activation 1 + 2 tanh(x/4) of wf/nn_wave_function.py:17)
   * [25]=residual buf or -1 [26]=residual r0 [27]=normalize (1: out = (res + y)/sqrt(2),
   * 0: out = res + y; hkext.py:130-137).  W is row-major [sum_p pad4(K_p)][pad4(Nout)]. */
  DQMC_OP_LINEAR = 3,
  /* i: [0]=src buf [1]=dst buf (rows = 2) [2]=n_up.  Mean over up / down electrons
   * (gnn/update_features.py:86-102). */
  DQMC_OP_SPIN_MEAN = 4,
  /* i: [0]=edge buf (we) [1]=node buf (hx; rows = electrons, or nuclei for 'ne' edges) [2]=dst buf [3]=dst col0
   * [4]=table offset of int [N][S][2] (edge row, sender; row -1 = none; sender < 0 = nucleus -1 - sender = row of hx)
   * [5]=S [6]=width.
   * out[i] = sum_s we[row(i,s)] * hx[send(i,s)] (gnn/graph.py:226-335). */
  DQMC_OP_CONV = 5,
  /* i: as CONV with [1]=divisor instead of a node buf.  out[i] = sum_s e[row(i,s)] / divisor
   * (EdgeSum with normalize, gnn/update_features.py:109-159). */
  DQMC_OP_EDGE_SUM = 6,
  /* i: [0]=src buf [1]=dst buf (rows = 1).  Sum over all rows (Jastrow sum_first,
   * wf/omni.py:35-40). */
  DQMC_OP_ROW_SUM = 7,
  /* i: [0]=backflow buf ([N][pad4(K*N)], column k*N+mu) [1]=dst buf (rows=K,
   * width=pad4(N*N), column i*N+mu) [2..5]=weight offsets of pi_up, pi_down, zetas_up,
   * zetas_down ([K*N][n_nuc*n_env]) [6]=n_env envelopes per nucleus (0 = 1).  Slater matrix
   * entries A = envelope * backflow (wf/env.py:57-75, wf/nn_wave_function.py:135-147;
   * n_env = 3 with pi = 1: the SimplifiedNucleusDependentEnvelopes of env.py:110-226). */
  DQMC_OP_ORBITALS = 8,
  /* i: [0]=orbital buf.  sign/log|det| of the K matrices and their forward-Laplacian
   * lanes, kept in double inside the context (wf/nn_wave_function.py:36-39).  At most 64 electrons (4 x 4
   * tiles of the float64 MFMA determinant kernel, one wave of rows for the pivot search; the kernels of 45 .. 64
   * electrons use up to 99 KB of LDS, which creation requests: DQMC_E_HIP if the device refuses); programs with more
   * are rejected at creation (DQMC_E_ARG).  The forward-Laplacian pass runs with TP = round_up(3 N + 2, 16) lanes,
   * every multiple of 16 up to 208; nothing is padded beyond that. */
  DQMC_OP_SLOGDET = 9,
  /* i: [0]=jastrow buf or -1 [1]=conf_coeff weight offset or -1 (SumPool) [2]=cusp kind
   * (0 none,1 deepqmc,2 psiformer) [3]=weight offset of {same_alpha, anti_alpha}.
   * f: [0]=same_scale [1]=anti_scale.  CI sum + cusps + Jastrow
   * (wf/nn_wave_function.py:152-171); in Laplacian mode also the potentials and E_loc
   * (hamil.py:160-182, physics.py:105-133). */
  DQMC_OP_FINAL = 10,
  /* Multi-head self attention over the electrons of a walker, forward-Laplacian form
   * (hk.MultiHeadAttention called at gnn/update_features.py:273-278).
   * i: [0]=q buf [1]=k buf [2]=v buf [3]=dst buf [4]=heads [5]=head_dim
   * [6]=n_const extra key/value rows that do not depend on the electrons (the nuclear tokens of
   * CombinedNodeAttention with elec_to_nuc = false, update_features.py:385-451; they come first
   * in the key order) [7],[8]=weight offsets of their keys / values ([n_const][heads*head_dim]). */
  DQMC_OP_ATTENTION = 11,
  /* i: [0]=dst buf [1]=weight offset of real[rows][width].  Rows that do not depend on the electron positions
   * (hk.Embed electron / nuclear embeddings, gnn/electron_gnn.py:497-503,596-625): value lane = the table,
   * derivative lanes zero. */
  DQMC_OP_CONST = 12
};

typedef struct dqmc_op {
  int32_t kind;
  int32_t i[28];
  float f[4];
} dqmc_op;

typedef struct dqmc_system {
  int32_t n_up, n_down, n_nuc, n_det;
  int32_t dtype;        /* 0 = float32, 1 = float64 */
  int32_t reserved;
  double norm_eps;      /* eps under the safe norm, utils.py:79-85 (finfo(dtype).eps) */
  double e_nuc;         /* unused (kept for layout): the nuclear repulsion is recomputed from the R of every call,
                           physics.py:112-116 */
} dqmc_system;

typedef struct dqmc_ctx dqmc_ctx;

/* Create a context on `device`.  charges: host double[n_nuc].  weights: host double[]
 * (converted to `real` on upload).  itable: host int32[].  stream: a hipStream_t (or 0). */
int dqmc_create(dqmc_ctx** out, int device, void* stream, const dqmc_system* sys,
                const double* charges_host, const dqmc_buf* bufs_host, int n_bufs,
                const dqmc_op* ops_host, int n_ops, const double* weights_host,
                size_t n_weights, const int32_t* itable_host, size_t n_itable);
void dqmc_destroy(dqmc_ctx* ctx);
const char* dqmc_last_error(void);

/* Replace the weight buffer (same length as at creation).  host double[]. */
int dqmc_set_weights(dqmc_ctx* ctx, const double* weights_host, size_t n_weights);

/* ---- Device-resident optimiser step ----
 * The parameters live in a device vector theta (double[n_params], the order of Program.grad_leaves) that the caller owns.
 * After dqmc_set_param_map, every call below only enqueues kernels on the context's stream: none synchronises it or touches
 * host memory once its arguments are validated, and none invalidates a captured forward-Laplacian graph ("pass_graph") --
 * a capture records pointers and shape-derived arguments, never weight values, and no buffer moves.  (dqmc_set_weights
 * keeps dropping the graphs, as before.)  All pointers are device pointers unless marked host.
 *
 * dqmc_set_param_map: src_host int32[n_weights], the parameter element each flat weight entry (dqmc_set_weights layout) is a
 * copy of, -1 for a constant or padding (Program.grad_src).  Builds the device tables of the re-packers; a setup call (it
 * synchronises).  DQMC_E_ARG for n_weights other than the context's or an entry outside [-1, n_params). */
int dqmc_set_param_map(dqmc_ctx* ctx, const int32_t* src_host, size_t n_weights, size_t n_params);
/* ---- The nuclear-token stream on the device (TransPsiformer; option "nuclear_reverse") ----
 * The nuclear tokens of an ansatz with DQMC_OP_ATTENTION constant rows attend to each other only: their stream (nuclei embedding,
 * per layer token attention + MLP, the envelope head) depends on theta and on the geometry, not on the electrons, and reaches
 * the layer program as constants of the weight buffer (the key / value rows of every ATTENTION op, the zeta tables of the
 * simplified envelopes).  dqmc_set_weights receives them folded on the host.  With a stream registered the library evaluates
 * the same fold on the device, in float64 whatever the context's precision, and owns its transpose:
 *   dqmc_weights_from_params  also folds theta -> derived vector, scatters it into the constant entries (rounded to the context's
 *                             precision; the double copy and the float64 twin get the doubles), then re-packs as before
 *   dqmc_grad_to_params       also gathers the adjoints of the derived vector from the constant entries of grad_w (ascending
 *                             entry order) and ADDS the stream's parameter gradients into grad_theta
 * Invariant: constants and the activations the transpose reads are always written together by the same fold; after a
 * dqmc_set_weights (host fold) dqmc_grad_to_params answers DQMC_E_ARG until the next dqmc_weights_from_params.
 *
 * The derived vector: per layer K_nuc then V_nuc [n_nuc][dim]; then, with n_env > 0, zetas up and zetas down [n_nuc][n_det][n_env].
 * lin: the stream's linear layers y = act(x w + b) as offsets into theta (w [n_in][n_out] row-major, b -1: none; act 0 none,
 * 1 tanh, 2 silu), in the order: edge MLP (n_edge_lin; input 4 + n_nuc features), embed MLP (n_embed_lin), per layer query, key,
 * value, linear, then the MLP (n_mlp_lin; the output projection and the MLP carry the residuals of nuclear_stream.fold), and with
 * n_env > 0 the GLU readouts W_up, V_up, W_down, V_down; zbias_up / zbias_down: offsets of zetas_bias_* [n_nuc][n_det][n_env].
 * sc_row / sc_col: CSR over the derived elements of the weight entries that are copies of each (entries the parameter map marks
 * -1).  theta: the current parameters (the call folds them once, so that constants and activations agree from the start).
 * All pointers are host memory.  A setup call: it synchronises and allocates everything the stream will ever need; it needs
 * dqmc_set_param_map first.  DQMC_E_ARG for tables that are inconsistent with the program or out of range. */
typedef struct dqmc_nuc_linear {
  int64_t w, b;
  int32_t n_in, n_out, act, reserved;
} dqmc_nuc_linear;
typedef struct dqmc_nuc_stream {
  int32_t n_nuc, n_layers, heads, dim, n_det, n_env;
  int32_t n_edge_lin, n_embed_lin, n_mlp_lin, n_lin;
  const dqmc_nuc_linear* lin;
  int64_t zbias_up, zbias_down;
  const int32_t* nuc_types;   /* [n_nuc] atom type of every nucleus (column of the one-hot edge feature) */
  const double* R;            /* [n_nuc][3] the geometry the context was compiled for */
  int64_t n_derived;
  const int64_t* sc_row;      /* [n_derived + 1] */
  const int32_t* sc_col;
  const double* theta;        /* [n_params] */
} dqmc_nuc_stream;
int dqmc_set_nuclear_stream(dqmc_ctx* ctx, const dqmc_nuc_stream* desc_host);
/* w[j] = theta[src[j]] where src[j] >= 0; the other entries keep the value of creation / the last dqmc_set_weights.  From
 * those doubles everything dqmc_set_weights refreshes is refreshed in place on the device -- the weights in the context's
 * precision, the float64 twin's (a twin created later starts from the current values), the weight tape of a generated
 * sub-step kernel, the packed planes of the fused kernel with their bf16 three-way split -- bit-identical to what
 * dqmc_set_weights produces from the same doubles.  DQMC_E_ARG before a map is set. */
int dqmc_weights_from_params(dqmc_ctx* ctx, const double* theta);
/* The transpose of the packing: grad_theta[e] = sum over j with src[j] == e of grad_w[j] (double[n_weights], what
 * dqmc_log_psi_vjp writes), in ascending j.  No atomics: identical calls give bit-identical results. */
int dqmc_grad_to_params(dqmc_ctx* ctx, const double* grad_w, double* grad_theta);
/* The per-walker form of dqmc_grad_to_params.  jac: real[B][ld_jac] as dqmc_log_psi_jacobian wrote it for B walkers, with the
 * logpsi / sign of that call (all device memory, the context's precision).  Row b of jac_theta (real[B][ld_theta], ld_theta >=
 * n_params; columns beyond n_params are left alone) receives the transpose of the packing applied to row b of jac: element e is
 * the sum of jac[b][j] over the entries j with src[j] == e, in ascending j, in the context's precision.  Rows of walkers with
 * sign 0 or a non-finite log|psi| are zero.  Works for every program with a parameter map.  With a nuclear stream (option
 * "nuclear_params" 1, else DQMC_E_UNSUPPORTED) each walker's partials of the derived vector are gathered from its row (ascending
 * entry order), taken back through the stream for all walkers of a chunk at once (float64, the chunk's arenas come from the
 * gradient workspace under "ws_budget_mb") and the stream's parameter partials -- dW = X^T dZ and db = colsum dZ of every linear
 * layer on the float64 MFMA, the walker's adjoint of the zeta tables for zetas_bias_* -- are ADDED to the row.  A walker's row
 * does not depend on the other walkers; identical calls are bit-identical.  DQMC_E_ARG while the stream's activations are older
 * than the weights (as dqmc_grad_to_params), DQMC_E_UNSUPPORTED, launching nothing, if a stream layer does not fit the LDS (its
 * 16 x n_out weight panel, or 16 x rows of its transposed input). */
int dqmc_jacobian_to_params(dqmc_ctx* ctx, const void* jac, size_t ld_jac, int B, const void* logpsi, const int32_t* sign,
                            void* jac_theta, size_t ld_theta);
/* optax.adam over the flat vectors, in place: with t the 1-based count of this step,
 *   mu = b1 mu + (1 - b1) g, nu = b2 nu + (1 - b2) g^2, theta += -lr (mu / (1 - b1^t)) / (sqrt(nu / (1 - b2^t)) + eps),
 * followed by dqmc_weights_from_params(theta).  n must be the map's n_params.  norms3: double[3] or NULL, receives the
 * 2-norms of theta before the step, of g and of the update from a fixed-order reduction. */
int dqmc_adam_step(dqmc_ctx* ctx, double* theta, double* mu, double* nu, const double* grad_theta, size_t n, double lr,
                   double b1, double b2, double eps, int64_t t, double* norms3);
/* theta += scale * delta (both double[n_params]), then dqmc_weights_from_params(theta): the entry point for directions
 * formed elsewhere on the device (natural gradient).  norms3 as above: theta before the step, delta, scale * delta. */
int dqmc_apply_update(dqmc_ctx* ctx, double* theta, const double* delta, double scale, double* norms3);
/* ---- KFAC preconditioner on the flat device vectors ----
 * The join between dqmc_log_psi_kfac and the device-resident optimiser step: the direction
 *   A_hat = sum_l A_l / (n_v R_mod),  G_hat = sum_l G_l / n_v      (per module, scattered through the row / column maps)
 *   F <- ema F_old + (1 - ema) F_new                               (first != 0: F_new)
 *   pi = sqrt((tr A_hat / dim A_hat) / (tr G_hat / dim G_hat))
 *   delta[W; b] = (A_hat + pi sqrt(damping) I)^-1 [g_W; g_b] (G_hat + sqrt(damping) / pi I)^-1
 *   diagonal elements:  F_ii = sum_b o_bi^2 / n_v (same EMA),  delta_i = g_i / (F_ii + damping)
 * is formed in float64 (also in a float32 context) by fixed-order reductions and a blocked Cholesky factorisation (panel
 * width DQMC_KFAC_PANEL) with triangular solves; there are no atomics and identical calls are bit-identical.  A factor that is
 * not positive definite (it can only be so when it is not finite) turns that module's part of delta into NaN.
 *
 * dqmc_set_kfac_map: host tables that say where a module's factors, gradient and diagonal partials live (a setup call: it
 * synchronises and allocates the workspace of the later calls; it needs dqmc_set_param_map first).
 *   mod   int64[n_modules][8]: n_in, n_out, has_bias, R (rows per walker of its ops), first element of w ([n_in][n_out]
 *         row-major) in theta, of b ([n_out], -1 without a bias), its first op in `op`, its number of ops
 *   op    int64[n_ops][6]: offsets of A_l and G_l in the factor buffer, d_A, d_G (dqmc_kfac_layout), the first entry in `maps`
 *         of its row map (d_A entries: the row of the module's A, the bias row being n_in, or -1 for padding) and of its column
 *         map (d_G entries: the column of the module's G or -1); every map is a permutation onto the module's rows / columns
 *   diag_pos  int64[n_diag] the parameter elements outside the modules; diag_row int64[n_diag + 1], diag_col: CSR of the
 *         rest columns that hold an element's copies (they are summed in the order given: ascending)
 * DQMC_E_ARG for tables that are inconsistent with each other, with the factor layout or with the parameter map (every
 * parameter element has to be covered exactly once); DQMC_E_UNSUPPORTED where dqmc_log_psi_kfac is.
 * dqmc_kfac_state_size: the doubles of the caller-owned state: per module A_hat (d x d, d = n_in + has_bias) then G_hat
 * (n_out x n_out), row-major, in the order of `mod`; then F of the diagonal elements, in the order of diag_pos.
 * dqmc_kfac_direction: all pointers are device memory.  grad_theta double[n_params] (dqmc_grad_to_params); factors, rest,
 * logpsi, sign exactly as dqmc_log_psi_kfac wrote them for B walkers (rest and logpsi in the context's precision; n_v is
 * counted from sign and logpsi on the device); state as above, read unless first != 0, and written; damping > 0;
 * delta double[n_params] and dot[1] = <delta, grad_theta> are written.
 * With a nuclear stream (option "nuclear_params"): the parameter elements of the stream that no module covers -- w / b of its
 * linear layers, zetas_bias_* -- are listed in diag_pos with an EMPTY CSR row (they have no copy in the weight buffer);
 * dqmc_set_kfac_map recognises them from the stream descriptor (an empty row anywhere else, or a row with columns there, is
 * DQMC_E_ARG) and allocates the arenas of the stream's batched backward.  dqmc_kfac_direction forms their o_bi from the rest rows
 * (the constant rows' and zeta tables' partials) through the stream, F_ii = sum_b o_bi^2 / n_v without ever storing a per-walker
 * row, with the same EMA, and delta_i = g_i / (F_ii + damping).  Kronecker factors of the stream's own layers are not formed.
 * dqmc_kfac_apply: theta += -lr coeff delta with coeff = min(1, sqrt(norm_constraint / (lr^2 dot[0]))) -- the norm
 * constraint of kfac_jax with momentum 0; coeff = 1 when norm_constraint <= 0 or dot[0] <= 0 -- evaluated on the device,
 * then dqmc_weights_from_params(theta).  norms4: double[4] or NULL = the 2-norms of theta before the step, of delta and of
 * the update, and lr^2 dot[0].
 * dqmc_kfac_direction and dqmc_kfac_apply only enqueue kernels on the context's stream: no synchronisation, no host memory
 * traffic, no allocation, and captured forward-Laplacian graphs stay valid. */
#define DQMC_KFAC_PANEL 32
typedef struct dqmc_kfac_map {
  int n_modules;
  const int64_t* mod;
  int n_ops;
  const int64_t* op;
  size_t n_maps;
  const int32_t* maps;
  size_t n_diag;
  const int64_t* diag_pos;
  const int64_t* diag_row;
  const int64_t* diag_col;
} dqmc_kfac_map;
int dqmc_set_kfac_map(dqmc_ctx* ctx, const dqmc_kfac_map* map_host);
int dqmc_kfac_state_size(dqmc_ctx* ctx, size_t* n_doubles);
int dqmc_kfac_direction(dqmc_ctx* ctx, const double* grad_theta, const double* factors, const void* rest, const void* logpsi,
                        const int32_t* sign, int B, double* state, int first, double ema, double damping, double* delta, double* dot);
int dqmc_kfac_apply(dqmc_ctx* ctx, double* theta, const double* delta, const double* dot, double lr, double norm_constraint,
                    double* norms4);
/* Test access to the weight buffers.  which: 0 = the flat weights in the context's precision, 1 = the weight tape of the
 * generated sub-step kernel, 2 = the packed planes of the fused kernel, 3 = the flat weights of the float64 twin, 4 = the
 * double copy of the flat weights a float32 context keeps once a parameter map is set.
 * out_host NULL: returns the size of the buffer in bytes (> 0).  Otherwise `bytes` must be exactly that size (DQMC_E_ARG);
 * DQMC_E_UNSUPPORTED when the context has no such buffer.  Synchronises the stream. */
int dqmc_debug_read_weights(dqmc_ctx* ctx, int which, void* out_host, size_t bytes);
/* Timing aid (tools/nuclear_coords_time.py): on the largest linear layer of the nuclear stream's token rows, B walkers, the
 * batched input-adjoint kernel of option "nuclear_coords" against the reverse pass's float64 LINEAR backward restricted to dX,
 * alternated `reps` times after a warm-up round.  ms2: the two median times in ms (device events); shape3: {B n_nuc, n_in,
 * n_out}.  Uses the gradient workspace; synchronises the stream.  DQMC_E_ARG without a folded stream. */
int dqmc_debug_nuc_dx_time(dqmc_ctx* ctx, int B, int reps, double* ms2, int* shape3);
/* out2 (host) = {captures, replays} of the context's forward-Laplacian graphs since its creation. */
int dqmc_graph_counters(dqmc_ctx* ctx, int64_t* out2);

/* ---- Loss assembly of multi-state training: between the value passes and dqmc_log_psi_vjp ----
 * All buffers are device memory of the caller, double (masks: uint8, 0 or 1).  The calls run on the context's stream, allocate
 * nothing, copy nothing to the host and do not synchronise; any context serves (it supplies the stream and nothing else).
 * Every sum has a fixed order: identical calls give bit-identical results.  One molecule, one process. */

/* Wave-function ratios from log-shifted values.  log_psi, sign, ratio: double[S][S][B], element [i][j][b] = psi_i on sample b
 * of state j.  With mean_i the mean of log_psi[i] over all S B samples:
 *   ratio[i][j][b] = sign[i][j][b] sign[j][j][b] exp((log_psi[i][j][b] - mean_i) - (log_psi[j][j][b] - mean_j)). */
int dqmc_psi_ratio(dqmc_ctx* ctx, const double* log_psi, const double* sign, int S, int B, double* ratio);

#define DQMC_CLIP_CENTER_MEAN 0
#define DQMC_CLIP_CENTER_MEDIAN 1       /* exact; even B: the mean of the two middle values */
#define DQMC_CLIP_SCALE_MEAN_ABS_DEV 0  /* mean_b |x - centre| */
#define DQMC_CLIP_SCALE_MEDIAN_ABS_DEV 1 /* median_b |x - centre|, exact */
/* Per row of x[n_rows][B] (any B >= 1), with the row's own centre and scale:
 *   x_clip = min(max(x, centre - clip_width scale), centre + clip_width scale),  mask = |x - centre| < exclude_width,
 *   row_stats[row] = {centre, scale, (1/B) sum_b w[row][b] x_clip[row][b], number of mask bits set}.
 * w: double[n_rows][B] or NULL (all ones).  A row with a non-finite element gets NaN for centre, scale, every clipped value
 * and the weighted mean; the call returns as for any other input.  x_clip must not alias x. */
int dqmc_clip_rows(dqmc_ctx* ctx, const double* x, const double* w, int n_rows, int B, int center, int scale, double clip_width,
                   double exclude_width, double* x_clip, uint8_t* mask, double* row_stats);

#define DQMC_SPIN_NONE 0
#define DQMC_SPIN_SQUARED 1
#define DQMC_SPIN_RAISING 2
/* What dqmc_loss_cotangents reads.  Hats are clipped values, m masks, w the sample weights, *_stats the row_stats of
 * dqmc_clip_rows called WITH the weights (entry 2 is the weighted mean, entry 3 the mask count). */
typedef struct dqmc_loss_terms {
  int S, B;
  const double* w;           /* [S][B] or NULL (all ones) */
  const double* e_clip;      /* [S][B] clipped local energies */
  const uint8_t* e_mask;     /* [S][B] */
  const double* e_stats;     /* [S][4] */
  double alpha;
  const double* r_clip;      /* [S][S][B] clipped ratios, or NULL: no overlap term */
  const uint8_t* r_mask;     /* [S][S][B] */
  const double* r_stats;     /* [S*S][4] */
  const double* scale;       /* [S][S] */
  const int32_t* rank;       /* [S] device: position of every state in the ordering */
  int spin_kind;             /* DQMC_SPIN_* */
  double lambda;
  const double* spin;        /* [n_states][B]: squared kind: the spin contributions; raising kind: the CLIPPED contributions */
  const uint8_t* spin_mask;  /* [n_states][B], raising kind */
  const double* spin_stats;  /* [n_states][4], raising kind */
  const int32_t* states_host;/* [n_states] HOST: the distinct states the spin rows belong to */
  int n_states;
} dqmc_loss_terms;
/* The cotangent of log|psi_s| on state s's own samples, c[S][B]: the whole loss gradient of state s is
 * dqmc_log_psi_vjp with cot = c[s] (the raising kind adds a direct term, below).
 *   energy:   c_sb  = m_sb w_sb (E^_sb - mean_b(E^_s w_s)) / sum_{s,b} m_sb
 *   overlap:  c_jb += alpha sum_{i: rank(i) < rank(j)} 2 x_ji scale_ij m_ijb (rho^_ijb - x_ij) w_jb / sum_b m_ijb,
 *             x_ij = mean_b(w_jb rho^_ijb)
 *   squared:  c_sb += lambda m_sb w_sb (s_sb - mean_b(s_s w_s)) / sum_{s in states, b} m_sb       (m: the energy mask)
 *   raising:  c_sb += lambda m_sb mu_s w_sb 2 (L^_sb - mu_s) / n,  mu_s = mean_b(L^_s w_s), n = sum_{s in states, b} m_sb
 *             (m: the mask of the clipped L), and k[q][b] = lambda m_sb mu_s w_sb / n for s = states[q]: the weights of the
 *             direct term sum_b k_sb dL_sb/dtheta.  k: double[n_states][B], may be NULL.
 *             Row q of spin / spin_mask / spin_stats belongs to state states[q]. */
int dqmc_loss_cotangents(dqmc_ctx* ctx, const dqmc_loss_terms* terms, double* c, double* k);

/* ---- Observables of the training loop (reference observable.py, force.py evaluate_finite_difference_force) ----
 * As the loss assembly: the calls run on the context's stream, copy nothing to the host and do not synchronise; every sum has
 * a fixed order and there are no atomics, so identical calls give bit-identical results.  One molecule, one process. */

/* Oscillator strengths between S electronic states (OscillatorStrengthMonitor, observable.py:556-605).
 *   r: real[S][B][N][3], the walkers of every state;  psi_ratio: double[S][S][B] as dqmc_psi_ratio writes it;  e_loc: real[S][B].
 *   os_mean, os_err: double[S][S];  cd_mean, cd_err: double[S][S][3].
 * First launch, one workgroup per ordered pair (i, j), means and population standard deviations over b (the mean, then in a
 * second pass the squared deviations from it):
 *   d[j][b][c]     = -sum_n r[j][b][n][c]                       (formed on the fly, the electrons added in ascending order)
 *   cd[i][j][b][c] = d[j][b][c] psi_ratio[i][j][b]   ->  cd_mean[i][j][c], cd_std[i][j][c]
 *   E[i], std_E[i] = those of e_loc[i]                          (the workgroups (i, i))
 * Second launch, one workgroup, IEEE double with every operation rounded on its own, as written:
 *   err_E[i]   = std_E[i] / sqrt(B)
 *   ex[i][j]   = E[j] - E[i]
 *   ex_err     = sqrt(err_E[i]^2 + err_E[j]^2)
 *   cd_err     = cd_std / sqrt(B)
 *   rel        = cd_err / cd_mean
 *   ds_vec[i][j][c] = cd_mean[i][j][c] cd_mean[j][i][c]
 *   ds_err_vec = |ds_vec| sqrt(rel[i][j][c]^2 + rel[j][i][c]^2)
 *   ds         = sum_c ds_vec
 *   ds_err     = sqrt(sum_c ds_err_vec^2)
 *   os_mean    = (2/3) ex ds
 *   os_err     = (2/3) |os_mean| sqrt((ex_err / ex)^2 + (ds_err / ds)^2)
 * The diagonal is not special-cased: os_mean[i][i] = 0 and os_err[i][i] = NaN, as in the reference.  1 <= S <= 32.  The context
 * keeps the moments between the launches in a scratch of 2 S + 3 S^2 doubles, allocated by the first call (dqmc_debug_read -5). */
int dqmc_oscillator_strength(dqmc_ctx* ctx, const void* r, const double* psi_ratio, const void* e_loc, int S, int B, double* os_mean,
                             double* os_err, double* cd_mean, double* cd_err);

/* The finite-difference force (force.py:550-606), per walker b, with the reference's signs.  D = 3 n_nuc displacements
 * d = 3 n0 + j0 (nucleus n0, Cartesian component j0) of step h:
 *   R_d = R - h e_(n0, j0)
 *   w[b][n][e] = exp(-|R_n - r_be|) / sum_n' exp(-|R_n' - r_be|)          (double, whatever the context's dtype)
 *   r_d[b][e][j0] = r[b][e][j0] + h w[b][n0][e]                            (the other components unchanged)
 *   F[b][n0][j0] = exp(2 (log|psi|(r_d, R_d) - log|psi|(r, R))) (E_loc(r_d, R_d) - e_loc[b]) / h
 * dqmc_fd_displace writes all D displaced copies in one launch: r_out real[D][B][N][3], R_out real[D][n_nuc][3] (each value
 * computed in double and rounded once to real); they must not alias r and R.  Between the two calls the caller evaluates
 * log|psi| (dqmc_wf_eval) and E_loc (dqmc_local_energy) at every (r_d, R_d).
 * dqmc_fd_force: log_d, e_d real[D][B]; log_0, e_0 real[B]; F double[B][n_nuc][3], the quotient formed in double.  h != 0. */
int dqmc_fd_displace(dqmc_ctx* ctx, const void* r, const void* R, int B, double h, void* r_out, void* R_out);
int dqmc_fd_force(dqmc_ctx* ctx, const void* log_d, const void* log_0, const void* e_d, const void* e_0, int B, double h, double* F);

/* psi for B walkers.  r: real[B][N][3], R: real[n_nuc][3]; out logpsi: real[B],
 * sign: int32[B] (values -1, 0, +1; bit-exact item of the parity contract). */
int dqmc_wf_eval(dqmc_ctx* ctx, const void* r, const void* R, int B, void* logpsi, int32_t* sign);

/* Local energy for B walkers.  e_loc: real[B]; stats: real[6][B] in the order V_el, E_kin,
 * V_loc, V_nl, lap, quantum_force (hamil.py:173-180), may be NULL; grad: real[B][3N]
 * (d log|psi| / dr, the quantum force), may be NULL; logpsi/sign may be NULL. */
int dqmc_local_energy(dqmc_ctx* ctx, const void* r, const void* R, int B, void* e_loc,
                      void* stats, void* grad, void* logpsi, int32_t* sign);

/* sign, log|psi| and grad log|psi| (real[B][3N]) from the forward-Laplacian pass alone -- no potentials, no
 * non-local ECP quadrature: what jax.value_and_grad(psi) hands the reference's LangevinSampler
 * (sampling/electron_samplers.py:193-201).  logpsi / sign may be NULL. */
int dqmc_psi_grad(dqmc_ctx* ctx, const void* r, const void* R, int B, void* logpsi, int32_t* sign, void* grad);

/* Sum over walkers of cot[b] * d log|psi(r_b)| / d w, for every entry w of the flat weight buffer (same layout and
 * length as dqmc_set_weights).  cot: real[B] device, NULL = all ones.  grad: device double[n_weights], overwritten.
 * logpsi / sign: optional, as dqmc_wf_eval.  Walkers with sign 0 or a non-finite log|psi| contribute nothing.
 * Entries that are constants or padding receive whatever their position accumulates (padding rows / columns of the
 * linear layers: exact zeros); mapping the flat gradient back onto the parameters is the caller's (Program.unflatten_grad).
 * Per walker chunk ("ws_budget_mb", adjoint buffers included) a value pass op by op, then the ops in reverse; the
 * walker sums run in a fixed order, so two identical calls give bit-identical results.
 * DQMC_E_UNSUPPORTED for programs with ATTENTION ops (Psiformer, TransPsiformer) unless option "attention_reverse" is 1
 * (dqmc_set_option); with it, only ATTENTION ops with constant key / value rows (n_const > 0, the TransPsiformer's nuclear
 * tokens) stay refused.  The same gate holds for every entry point that runs this reverse pass.
 * Option "nuclear_reverse" 1 (it needs dqmc_set_nuclear_stream; values other than 0 / 1 and a missing stream: DQMC_E_ARG) admits
 * the constant rows in the calls that sum partials over the walkers -- dqmc_log_psi_vjp, dqmc_orbitals_vjp,
 * dqmc_pretrain_loss_grad: grad then also carries the walker-summed gradient of the constant key / value rows and of the
 * folded zeta tables, which dqmc_grad_to_params takes back through the nuclear stream.  The per-walker calls
 * (dqmc_log_psi_jacobian, dqmc_log_psi_kfac, dqmc_log_psi_grad_coords, dqmc_ecp_force, dqmc_set_kfac_map) keep answering
 * DQMC_E_UNSUPPORTED for such programs: the stream is shared by all walkers and has no per-walker partials.
 * Option "nuclear_coords" 1 (it needs a registered stream AND "nuclear_reverse" 1; anything else, and values other than 0 / 1:
 * DQMC_E_ARG) admits dqmc_log_psi_grad_coords as well: it needs the stream's per-walker ADJOINTS only, which a backward of the
 * stream batched over the walkers provides (see there).  The other four keep refusing with the same text.  Off (the default)
 * nothing changes.
 * Option "nuclear_params" 1 (the same conditions and errors; independent of "nuclear_coords") admits dqmc_log_psi_jacobian,
 * dqmc_log_psi_kfac and dqmc_set_kfac_map: the Jacobian and KFAC modes then write each walker's partials of the constant key /
 * value rows and of the zeta tables into those entries' own jac resp. rest columns, dqmc_jacobian_to_params takes a Jacobian's
 * rows back through the stream per walker, and dqmc_kfac_direction treats the stream's own parameters as diagonal elements (see
 * there).  dqmc_ecp_force keeps refusing, and dqmc_log_psi_grad_coords does unless "nuclear_coords" is on as well.  Off (the
 * default) nothing changes. */
int dqmc_log_psi_vjp(dqmc_ctx* ctx, const void* r, const void* R, int B, const void* cot,
                     double* grad, void* logpsi, int32_t* sign);

/* Per-walker parameter Jacobian of log|psi|: row b = d log|psi(r_b)| / d w for every entry w of the flat weight buffer
 * (the layout of dqmc_set_weights), B rows -- the per-walker rows O_b of natural-gradient / stochastic-reconfiguration and
 * KFAC preconditioners.
 *   jac: real[B][ld_jac], ld_jac >= n_weights; columns >= n_weights are not touched.  logpsi / sign: optional outputs.
 * Same conventions as dqmc_log_psi_vjp: walkers with sign 0 or a non-finite log|psi| get an all-zero row; constant and
 * padding entries get what their position accumulates (padding of linear layers: exact zeros); walker chunks per
 * "ws_budget_mb" (dqmc_last_chunks); no atomics, so identical calls are bit-identical, and a chunked call equals an
 * unchunked one bit for bit.  DQMC_E_UNSUPPORTED for ATTENTION programs without
 * option "attention_reverse" and for N > 64, as dqmc_log_psi_vjp. */
int dqmc_log_psi_jacobian(dqmc_ctx* ctx, const void* r, const void* R, int B, void* jac, size_t ld_jac,
                          void* logpsi, int32_t* sign);

/* KFAC Kronecker factors from the reverse pass.  A walker is valid when its sign is nonzero and its log|psi| is finite;
 * every sum below runs over the valid walkers only.  For each DQMC_OP_LINEAR op l, in program order, with nrows_l rows
 * per walker, pieces p of K_p inputs, ldw = pad4(nout):
 *   x~[b][r]  the op's input row of walker b, row r: the pieces concatenated in packed-weight row order, piece p taking
 *             pad4(K_p) entries (zeros past K_p; a broadcast piece gives walker b's one row to every r), then a 1 if the
 *             op has a bias;  d_A = sum_p pad4(K_p) + has_bias.
 *   dZ1[b][r] d log|psi(r_b)| / d Z[b][r] over the ldw pre-activation columns (padding columns 0): the adjoint of a unit
 *             cotangent.
 *   A_l = sum_b sum_r x~ x~^T   double[d_A][d_A], row-major; A_l[d_A-1][d_A-1] = n_valid * nrows_l when has_bias.
 *   G_l = sum_b sum_r dZ1 dZ1^T double[ldw][ldw], row-major.
 * Padding rows and columns of both are exact zeros.
 * Layout of `factors`: A_0, G_0, A_1, G_1, ... contiguous in program order (A_l at the sum of d_A^2 + ldw^2 over the ops
 * before l).  "Rest" entries: the flat weight entries (dqmc_set_weights layout) that lie in no LINEAR op's W block
 * (sum_p pad4(K_p) x ldw at its weight offset) or bias block (ldw at its bias offset), in ascending order: envelopes,
 * cusp alphas, conf_coeff, CONST tables, padding.
 *   dqmc_kfac_layout: host outputs, each may be NULL: the number of LINEAR ops, the doubles of `factors`, the rest entries.
 *   dqmc_log_psi_kfac arguments:
 *     cot     real[B] or NULL (ones);  grad double[n_weights]: sum_b cot[b] d log|psi_b| / d w, as dqmc_log_psi_vjp;
 *     factors double[n_factor_doubles];  rest real[B][n_rest] or NULL: rest[b][j] = d log|psi(r_b)| / d w of rest entry j
 *     (the values dqmc_log_psi_jacobian writes into those columns; invalid walkers get zeros);  logpsi / sign optional.
 * One value pass and one reverse pass (unit cotangent) per walker chunk ("ws_budget_mb", dqmc_last_chunks); the cotangent
 * weights the walker sums of grad.  No atomics: identical calls are bit-identical; with cot == NULL grad equals
 * dqmc_log_psi_vjp's bit for bit.  DQMC_E_UNSUPPORTED for ATTENTION programs without
 * option "attention_reverse" and for N > 64, as dqmc_log_psi_vjp. */
int dqmc_kfac_layout(dqmc_ctx* ctx, int* n_linear, size_t* n_factor_doubles, size_t* n_rest);
int dqmc_log_psi_kfac(dqmc_ctx* ctx, const void* r, const void* R, int B, const void* cot, double* grad, double* factors,
                      void* rest, void* logpsi, int32_t* sign);

/* Per walker b: grad_r[b] = d log|psi(r_b)| / d r (real[B][N][3]) and grad_R[b] = d log|psi(r_b)| / d R
 * (real[B][n_nuc][3]); either may be NULL, not both.  logpsi / sign optional, as dqmc_wf_eval.
 * The reverse pass of dqmc_log_psi_vjp (value pass op by op, then the ops in reverse, per "ws_budget_mb" walker chunk) with
 * no weight gradients: the adjoints of the feature, envelope and cusp inputs are carried into the coordinates.  Sums over
 * the electrons and nuclei run in a fixed order (no atomics): identical calls are bit-identical, and a chunked call equals
 * an unchunked one bit for bit.  Walkers with sign 0 or a non-finite log|psi| get zero rows.  By translation invariance
 * sum_a grad_R[b][a] = -sum_i grad_r[b][i].  DQMC_E_UNSUPPORTED for ATTENTION programs without
 * option "attention_reverse" and for N > 64, as dqmc_log_psi_vjp.
 * Programs with a nuclear stream (constant key / value rows) run with option "nuclear_coords" 1.  grad_R then is the sum of two
 * parts: the electron stream's, differentiated at the R of the call as for every program, and the nuclear stream's -- each
 * walker's partials of the constant key / value rows and of the zeta tables, summed over the copies of every derived element,
 * taken back through the stream per walker (float64 in both precisions, adjoints only, a number of launches that does not depend
 * on B) and through the edge features into R.  The stream's part is differentiated at the REGISTERED geometry
 * (dqmc_nuc_stream.R), whatever R the call passes: the constants the program reads were folded there.  (Through
 * NeuralNetworkWaveFunction the two coincide: one context per geometry.)  A call with grad_R == NULL never runs the stream's
 * backward; one with grad_R refuses with DQMC_E_ARG while the stream's activations are older than the weights (dqmc_set_weights
 * since the last dqmc_weights_from_params), as dqmc_grad_to_params does, and with DQMC_E_UNSUPPORTED, launching nothing, if a
 * stream layer's weight panel (16 columns x n_out doubles) does not fit the 160 KB of LDS.  The stream's part of a walker's
 * row is summed in a fixed order that does not depend on the other walkers of the chunk. */
int dqmc_log_psi_grad_coords(dqmc_ctx* ctx, const void* r, const void* R, int B, void* grad_r, void* grad_R,
                             void* logpsi, int32_t* sign);

/* Hellmann-Feynman force estimators (reference force.py), per walker b and nucleus I, Cartesian:
 * force: device double[B][n_nuc][3], overwritten.  Z_I = the charges given to dqmc_create.  With d = r_i - R_I,
 * rho = |d|, u = d / rho, g_i = grad_r[b][i], F_nuc,I = sum_{J != I} Z_I Z_J (R_I - R_J) / |R_I - R_J|^3:
 *   DQMC_FORCE_NUCLEAR   F_nuc                                                       (nuclear_force)
 *   DQMC_FORCE_BARE      F_nuc + Z_I sum_i d / rho^3                                 (evaluate_hf_force_bare, all-electron)
 *   DQMC_FORCE_AC_ZVQ    F_nuc + Z_I sum_i (g_i - (u . g_i) u) / rho                 (evaluate_hf_force_ac_zvq)
 *   DQMC_FORCE_AC_ZVZBQ  AC_ZVQ - 2 (e_loc[b] - energy) Z_I sum_i u                  (evaluate_hf_force_ac_zvzbq)
 *   DQMC_FORCE_AC_ZB     BARE - 2 (e_loc[b] - energy) grad_R[b][I]                   (evaluate_hf_force_ac_zb)
 *   DQMC_FORCE_AC_ZVQZB  AC_ZVQ - 2 (e_loc[b] - energy) grad_R[b][I]                 (AC_ZVQ with the ZB term of AC_ZB)
 * r: real[B][N][3], R: real[n_nuc][3]; grad_r: real[B][N][3] (d log|psi| / d r, e.g. from dqmc_psi_grad), needed by the
 * ZVQ family; grad_R: real[B][n_nuc][3] (dqmc_log_psi_grad_coords), needed by AC_ZB and AC_ZVQZB; e_loc: real[B], needed by
 * the estimators with a ZB term; each may be NULL where it is not needed.  energy: the batch energy E.  Sums in double. */
enum dqmc_force_estimator {
  DQMC_FORCE_NUCLEAR = 0,
  DQMC_FORCE_BARE = 1,
  DQMC_FORCE_AC_ZVQ = 2,
  DQMC_FORCE_AC_ZVZBQ = 3,
  DQMC_FORCE_AC_ZB = 4,
  DQMC_FORCE_AC_ZVQZB = 5
};
int dqmc_hf_force(dqmc_ctx* ctx, int estimator, const void* r, const void* R, int B, const void* grad_r, const void* grad_R,
                  const void* e_loc, double energy, double* force);

/* Hellmann-Feynman force of a Hamiltonian with a Gaussian-type ECP (dqmc_set_ecp), per walker b and nucleus I, Cartesian:
 *     F_I = F_nuc,I(Z) - dV_loc/dR_I - G_I,      Z = the (valence) charges given to dqmc_create.
 * V_loc = sum_i sum_I f_I(rho), f_I = -Z_I / rho + the local r^-1, r^0, r^1 Gaussians of nucleus I (d = r_i - R_I, rho = |d|):
 *     dV_loc/dR_I = -sum_i f_I'(rho) d / rho.
 * G is the gradient of the non-local term.  For a nucleus I = nl_nuc[j] with a non-local channel, electron i and quadrature
 * vertex q (x_q = R_I + rho w_q, w_q = Rz(phi) Ry(theta) Rz(phi_rand) p_q: the vertices of dqmc_local_energy):
 *     ratio_q       = s_q s_0 exp(log_q - log_0)
 *     dratio_q/dR_K = ratio_q ( gR_q[K] - gR_0[K] + [K == I] J_q^T gr_q[i] )
 *     J_q = dx_q/dR_I = 1 - [ w_q dhat^T + rho (d_theta w_q)(grad_d theta)^T + rho (d_phi w_q)(grad_d phi)^T ]
 *     grad_d theta = (cos(theta) dhat - e_z) / (rho sin(theta)),   grad_d phi = (-d_y, d_x, 0) / (d_x^2 + d_y^2)
 *     v_l(rho) = sum_t beta_lt e^{-alpha_lt rho^2},   dv_l/dR_I = -2 (R_I - r_i) sum_t alpha_lt beta_lt e^{-alpha_lt rho^2}
 *     G_K += sum_i sum_l (2l+1)/12 [ [K == I] dv_l/dR_I sum_q P_l(cos theta_q) ratio_q + v_l sum_q P_l(cos theta_q) dratio_q/dR_K ]
 * gr_q / gR_q: d log|psi| / dr, / dR at the configuration with electron i at x_q, gR_0 the same at the walker itself, all from
 * one coordinate reverse pass (dqmc_log_psi_grad_coords) per walker chunk of "ecp_max_cfg" quadrature configurations, in the
 * context's dtype; the assembly is double.  all_rows 0: only K == I is kept (the reference's wf_ratio_grad[:, nucleus_index]);
 * all_rows 1: every K, the full dV_nl/dR.  The row of nucleus nl_nuc[j] is stored at row nl_nuc[j] (the reference stores it
 * at row j, which is right only when every nucleus has a non-local channel).  On the axis d || e_z, J_q is singular, as the
 * reference's autograd is.
 *   estimator: DQMC_FORCE_BARE, or DQMC_FORCE_AC_ZB = BARE - 2 (e_loc[b] - energy) gR_0[b][I] (e_loc: real[B], else may be
 *              NULL); anything else DQMC_E_ARG.
 *   force: device double[B][n_nuc][3].  parts: NULL or device double[2][B][n_nuc][3]: parts[0] = F_nuc - dV_loc/dR,
 *          parts[1] = -G (BARE: force = parts[0] + parts[1]).
 *   The rotation is the one set by the preceding dqmc_ecp_rotation: the same seed or angles give the vertices of the
 *   dqmc_local_energy call.
 * DQMC_E_ARG when no Gaussian ECP is set or a pseudo-Hamiltonian is; DQMC_E_UNSUPPORTED for ATTENTION programs without option
 * "attention_reverse" and for N > 64, as dqmc_log_psi_grad_coords.  An ECP with local terms only is valid: parts[1] is zero
 * and no reverse pass runs unless AC_ZB needs gR_0.  A walker with sign 0 or a non-finite log|psi| gets NaN rows in parts[1] and force; a quadrature configuration
 * with sign 0 or a non-finite log|psi| contributes ratio 0.  Fixed-order sums, no atomics: identical calls are bit-identical,
 * and a chunked call equals an unchunked one bit for bit.  dqmc_last_chunks[0] afterwards: the walker chunks of the call. */
int dqmc_ecp_force(dqmc_ctx* ctx, int estimator, int all_rows, const void* r, const void* R, int B, const void* e_loc,
                   double energy, double* force, double* parts);

/* ---- SCF-orbital pretraining (reference pretrain/pretraining.py, pretraining_target.py, gto.py) ----
 * Slater matrices are real[B][K][N][N], K = n_det: rows electrons (up first), columns orbitals.
 *
 * dqmc_set_pretrain_target uploads the (MC-)SCF target once per context; every array is a host pointer.
 *   shells: n_shells contracted Cartesian GTO shells, one contraction each: shell_atom (index of the nucleus it sits on),
 *           shell_l (0 .. 3), shell_n_prim, and coeffs / zetas: the primitives of all shells, concatenated in shell order.
 *           Shell s owns (l+1)(l+2)/2 atomic orbitals in the order (lx, ly, l - lx - ly), lx = l..0, ly = l-lx..0;
 *           n_ao must equal their sum.
 *   mo_coeffs: double[n_ao][n_mo];  confs: int32[n_conf][N] orbital indices < n_mo (the first n_up entries the up orbitals,
 *           then the down ones);  conf_coeffs: double[n_conf].
 *   A malformed table (l > 3, atom out of range, wrong n_ao, orbital index out of range) returns DQMC_E_ARG before any HIP call.
 * dqmc_pretrain_target: target real[B][n_conf][N][N] on the device,
 *   phi = anorm x^lx y^ly z^lz sum_p coeff_p rnorm_p exp(-|zeta_p d^2|), d = r_i - R_atom (the R of this call; plain squared
 *   distance), anorm = 1 / sqrt(prod (2 l_i - 1)!!), rnorm_p = (2 zeta_p / pi)^(3/4) (4 zeta_p)^(l/2);
 *   target[b][c][i][mu] = (phi(r_i) . mo_coeffs[:, confs[c][mu]]) |c_c|^(1/N) (sign(c_c) for mu = 0).
 *   Arithmetic in the context's dtype.
 * dqmc_orbitals: orb real[B][K][N][N], the Slater matrices of the value pass, run op by op per "ws_budget_mb" walker chunk.
 *   DQMC_E_UNSUPPORTED unless the program stores full [N][N] matrices.
 * dqmc_orbitals_vjp: grad (device double[n_weights], overwritten) = sum_{b,k,i,mu} cot[b][k][i][mu] d A[b][k][i][mu] / d w for
 *   every entry w of the flat weight buffer (layout of dqmc_set_weights); cot real[B][K][N][N]; orb: optional output as
 *   dqmc_orbitals.  The reverse pass of dqmc_log_psi_vjp with the cotangent entering at the Slater matrices: the
 *   determinants, the CI sum and every op from which no path leads to the matrices (the Jastrow factor) are skipped and
 *   their entries are exact zeros.  No walker is left out (orbitals are finite wherever the walker is).  Fixed-order
 *   sums: identical calls are bit-identical, chunked and unchunked calls differ in the last bits.
 *   DQMC_E_UNSUPPORTED for ATTENTION programs without option "attention_reverse", as dqmc_log_psi_vjp; any number of electrons.
 * dqmc_pretrain_loss_grad: value pass -> target -> loss and its cotangent -> reverse pass, all on the device:
 *   per_sample_loss[b] (device double[B]) = mean_{k, i < n_up, mu} (A - T)^2 + mean_{k, i >= n_up, mu} (A - T)^2, with
 *   T[k] = target configuration k mod n_conf, its [:n_up, :n_up] and [n_up:, n_up:] blocks, zeros elsewhere;
 *   grad = d (sum_b per_sample_loss[b] / n_total) / d w.  n_total: the walker count the means of the caller's loss run
 *   over.  The down term is omitted when n_down == 0.  DQMC_E_ARG before a target is set. */
int dqmc_set_pretrain_target(dqmc_ctx* ctx, int n_shells, const int32_t* shell_atom, const int32_t* shell_l,
                             const int32_t* shell_n_prim, const double* coeffs, const double* zetas, int n_ao, int n_mo,
                             const double* mo_coeffs, int n_conf, const int32_t* confs, const double* conf_coeffs);
int dqmc_pretrain_target(dqmc_ctx* ctx, const void* r, const void* R, int B, void* target);
int dqmc_orbitals(dqmc_ctx* ctx, const void* r, const void* R, int B, void* orb);
int dqmc_orbitals_vjp(dqmc_ctx* ctx, const void* r, const void* R, int B, const void* cot, double* grad, void* orb);
int dqmc_pretrain_loss_grad(dqmc_ctx* ctx, const void* r, const void* R, int B, double n_total, double* grad,
                            double* per_sample_loss);

/* Gaussian-type effective core potential (reference ecp/gaussian_type_ecp.py:32-93 table layout,
 * :127-159 local part, :161-255 non-local part; replaces GaussianTypeECP.__init__'s pyscf lookup by
 * caller-supplied tables).  The `charges_host` given to dqmc_create must then be the valence charges
 * (ns_valence) and dqmc_system.e_nuc the repulsion of those.
 *   loc_host: double[n_nuc][3][2][n_terms_loc] -- terms r^-1, r^0, r^1; [.,term,0,.] exponents alpha,
 *             [.,term,1,.] coefficients beta; zero padded (all-zero = no ECP on that nucleus); may be NULL.
 *   nl_host:  double[n_nuc][n_l][2][n_terms_nl] -- channel l: V_l(r) = sum_k beta_lk exp(-alpha_lk r^2);
 *             nuclei whose block is all zero have no non-local part; may be NULL.
 * Afterwards dqmc_local_energy adds the local terms to V_loc and V_nl (12-point icosahedron quadrature,
 * 12 N n_ecp value-only psi evaluations per walker) to E_loc and stats[3]. */
int dqmc_set_ecp(dqmc_ctx* ctx, int n_terms_loc, const double* loc_host, int n_l, int n_terms_nl,
                 const double* nl_host);
/* Random rotation of the quadrature about the electron-nucleus axis for the following
 * dqmc_local_energy calls (ecp_utils.py:55: uniform in [0, pi/5) per (nucleus, electron); the reference
 * keys it by fold_in(fold_in(rng, j), i)).  phi: device real[B][n_ecp_nl][N] angles, or NULL to draw them
 * from Philox4x32-10 keyed by (seed, nucleus, walker, electron). */
int dqmc_ecp_rotation(dqmc_ctx* ctx, uint64_t seed, const void* phi);

/* Pseudo-Hamiltonian (reference ecp/pseudo_hamiltonian.py: PseudoHamiltonian.local_potential :173-190,
 * compute_coefficients_of_differential_operators :192-234, kinetic_term :236-278; replaces load_PH_functions'
 * XML lookup :73-112 by caller-supplied tables).  `charges_host` of dqmc_create must be the valence charges.
 *   rv_loc_host, rv_l2_host: double[n_nuc][n_grid] -- r*V_loc(r) (+ Z_eff) and r*V_L2(r) on the regular grid
 *             linspace(0, r_max, n_grid) (what parse_xml :32-70 returns; linear interpolation, zero beyond r_max);
 *   mask_host: int32[n_nuc], non-zero = this nucleus carries a PH (rows of the others are ignored).
 * An all-zero mask or n_grid == 0 switches the PH off.  Afterwards dqmc_local_energy evaluates
 *   E_kin = sum_i b(r_i).grad_i log|psi| - sum_i tr(A(r_i) Hess_ii) - |Q^T grad|^2,   A = Q Q^T (3x3 per electron),
 * by seeding the forward-Laplacian lanes with the columns of the Cholesky factors Q (the reference's coordinate
 * change r = Q v with Q held fixed), adds sum rV_loc(rho)/rho to V_loc, and reports in stats[4], stats[5] and
 * `grad` the transformed Laplacian, |grad_v|^2 and grad_v = Q^T grad_r (what the reference's kinetic_term returns).
 * dqmc_psi_grad and the Langevin entry points keep the plain gradient.  Not combinable with a non-local dqmc_set_ecp. */
int dqmc_set_pseudo_hamiltonian(dqmc_ctx* ctx, int n_grid, double r_max, const double* rv_loc_host,
                                const double* rv_l2_host, const int32_t* mask_host);

/* n_sub Metropolis sub-steps, in place on the sampler state
 * (sampling/electron_samplers.py:102-138,347-357).
 *   r real[B][N][3], logpsi real[B], sign int32[B], age int32[B], tau real[1] (device).
 *   max_age < 0: off.  target_acceptance <= 0: tau not adapted.
 *   noise: real[n_sub][B][N][3] standard normals and unif: real[n_sub][B] in [0,1), or
 *   both NULL to draw them on the device from Philox4x32-10 keyed by (seed, sub-step).
 *   accept_out: uint8[n_sub][B] accept decisions or NULL.
 *   stats7_host: host double[7] = acceptance, tau, age mean, age max, log|psi| mean,
 *   log|psi| std, mean e-e distance of the LAST sub-step (electron_samplers.py:154-163),
 *   or NULL (then the call does not synchronise). */
int dqmc_mcmc_steps(dqmc_ctx* ctx, void* r, void* logpsi, int32_t* sign, int32_t* age,
                    void* tau, const void* R, int B, int n_sub, int max_age,
                    double target_acceptance, uint64_t seed, const void* noise,
                    const void* unif, uint8_t* accept_out, double* stats7_host);

/* Metropolis-adjusted Langevin sampler (reference sampling/electron_samplers.py:176-232; drift cleaning
 * sampling/sampling_utils.py:72-101).  The sampler state additionally carries the cleaned drift force real[B][N][3].
 * mol_charges_host: host double[n_nuc], the FULL nuclear charges (mol.charges; the crossover parameter of the
 * drift cleaning uses them even under an ECP).
 *   dqmc_langevin_update <- LangevinSampler._update: log|psi|, sign and the drift of the CURRENT positions, cleaned
 *                           with the step size `tau` (device real[1]) of the previous iteration.
 *   dqmc_langevin_steps  <- n_sub x LangevinSampler.sample, in place: r' = r + tau F + sqrt(tau) xi, forward-Laplacian
 *                           pass for psi' and its gradient (no ECP quadrature), Green's-function ratio in the acceptance,
 *                           age override and step-size adaptation as dqmc_mcmc_steps.  noise / unif / accept_out /
 *                           stats7_host as there. */
int dqmc_langevin_update(dqmc_ctx* ctx, const void* r, const void* R, const double* mol_charges_host, int B, const void* tau,
                         void* logpsi, int32_t* sign, void* force);
int dqmc_langevin_steps(dqmc_ctx* ctx, void* r, void* logpsi, int32_t* sign, int32_t* age, void* force, void* tau, const void* R,
                        const double* mol_charges_host, int B, int n_sub, int max_age, double target_acceptance, uint64_t seed,
                        const void* noise, const void* unif, uint8_t* accept_out, double* stats7_host);
/* One opposite-spin exchange step (sampling/electron_samplers.py:235-330): per walker the positions of spin-up electron
 * up_idx[b] and spin-down electron n_up + down_idx[b] (device int32[B] each) are swapped, psi re-evaluated (value path),
 * accepted with 2 (log|psi'| - log|psi|) > log unif[b]; no age override, step size untouched (:312-313).  stats7_host
 * (may be NULL): the sampler statistics after the step, [0] = acceptance of this step. */
int dqmc_exchange_step(dqmc_ctx* ctx, void* r, void* logpsi, int32_t* sign, int32_t* age, const void* tau, const void* R, int B,
                       const int32_t* up_idx, const int32_t* down_idx, const void* unif, uint8_t* accept_out, double* stats7_host);

/* Per-rank partial record of the energy reduction: host double[7] =
 * {n, sum_w, sum_wE, sum_E, M2 (sum of squared deviations from this rank's mean), min,
 * max}.  w may be NULL (all ones).  Ranks all-gather the 56-byte records (RCCL) and
 * merge them with dqmc_merge_energy_stats. */
int dqmc_energy_stats(dqmc_ctx* ctx, const void* e_loc, const void* w, int B, double* out7_host);
/* The whole cross-GPU energy reduction in one call: this rank's record, ONE ncclAllGather of the 56-byte records over
 * the caller's RCCL communicator (`rccl_comm` = an ncclComm_t of `n_ranks` ranks; the call is enqueued on the context's
 * stream), Chan merge -> host double[5] as dqmc_merge_energy_stats.  Replaces the reference's five pmean / pmin / pmax
 * calls (parallel.py:175-225).  librccl.so is loaded at the first call; DQMC_E_UNSUPPORTED if it is absent. */
int dqmc_energy_stats_allgather(dqmc_ctx* ctx, void* rccl_comm, int n_ranks, const void* e_loc, const void* w, int B,
                                double* out5_host);
/* Chan merge of n_ranks records -> host double[5] = mean, std (population), min, max,
 * weighted mean.  Pure host arithmetic. */
int dqmc_merge_energy_stats(const double* records_host, int n_ranks, double* out5_host);

/* Debug / test access: copy activation buffer `buf` of the last evaluation (layout
 * real[B][rows][TP][width]) to host as double[].  n must equal B*rows*TP*width.
 * buf = -1: log|det| lanes double[B][K][TP]; buf = -2: det signs as double[B][K]; buf = -4: the psi-weighted
 * conditioning record of the Slater matrices, double[B] (Laplacian-mode evaluations); buf = -5: the moments of the last
 * dqmc_oscillator_strength call, double[2 S + 3 S^2] = E[S], std_E[S], cd_std[S][S][3] (needs no evaluation). */
int dqmc_debug_read(dqmc_ctx* ctx, int buf, double* out_host, size_t n);
/* Lanes (TP) used by the last evaluation. */
int dqmc_debug_lanes(dqmc_ctx* ctx);
/* Walkers the last dqmc_local_energy / dqmc_psi_grad call re-evaluated in float64 (float32 contexts: the local
 * energy near a node of psi is a difference of huge numbers, E_kin = -(lap + |grad|^2)/2 with both terms ~ 1/psi^2;
 * walkers whose error predictor score = (|lap| + |grad|^2) / max(1, |E_loc|) x max(1, sum_k |p_k| kappa_k) -- node
 * cancellation times the conditioning record of the Slater matrices that carry psi -- exceeds "refine_thresh", or whose
 * E_loc is not finite, are run again by a float64 twin of the context and their E_loc / stats / grad / log|psi| / sign
 * replaced.  The threshold calibrates itself: on the first and then every "refine_probe"-th call a strided sample of
 * <= "refine_sample" (256) further walkers is evaluated in float64 too.  Measured on the MI355X, the float32 error of a
 * walker is m x score x (an exponentially distributed factor): the sample gives the scale m, and the threshold is the largest
 * one for which the expected share of float32-kept walkers beyond the tolerance "refine_target_e7" x 1e-7 (default 1e-5
 * relative) -- the mean of exp(-tol / (m score_i)) over the kept walkers of the probed batch -- stays below
 * "refine_miss_e9" x 1e-9 (default 1e-8).  A batch with more than
 * "refine_direct_pct" (60 %) of its walkers above the threshold is evaluated in float64 whole, and so are the next
 * "refine_direct_calls" (15) calls -- a stay that doubles with every float32 look that confirms the mode, at most
 * "refine_direct_backoff" times --;
 * the context returns to the mixed mode only when a float32 pass then finds fewer than "refine_direct_exit_pct" (45 %)
 * above it -- hysteresis: one calibration draw near a single line used to flip the mode from run to run). */
int dqmc_last_refined(dqmc_ctx* ctx);
/* State of the refinement after the last local-energy call: out4 = {mode ("refine": 0 / 1 / 2; 0 in a float64
 * context), current score threshold, measured float32 error per unit of score (0 before the first probe), calls
 * that will still go to the direct float64 pass because most walkers were flagged}. */
int dqmc_refine_info(dqmc_ctx* ctx, double* out4);
/* Walker chunks of the last dqmc_local_energy call: out2 = {chunks of the context's own forward-Laplacian pass (0: it did
 * not run one, e.g. the whole batch went to float64), chunks of the largest pass of its float64 twin}.  An evaluation
 * whose activations exceed "ws_budget_mb" is split into chunks inside the library (the reference has no such limit to
 * replace: its vmap over the electron batch, loss/energy.py:50-57, simply needs the memory). */
int dqmc_last_chunks(dqmc_ctx* ctx, int* out2);
/* Running counts since the context was created: out4 = {dqmc_local_energy / dqmc_psi_grad calls, of them calls evaluated in
 * float64 whole ("direct" mode or "refine" 2), calibration probe calls, walkers re-evaluated in float64 (sum of
 * dqmc_last_refined)} -- what a caller needs to say which mode its steps actually ran in (bench.py: config.refine_engaged). */
int dqmc_refine_counters(dqmc_ctx* ctx, int64_t* out4);
/* Which kernel dqmc_mcmc_steps launches per Metropolis sub-step (sampling/electron_samplers.py:102-138): writes the name of the
 * PLAN-SPECIALISED kernel bound to this context's program (deepqmc_amd/csrc/gen/, generated by deepqmc_amd/codegen from the
 * layer program and matched by a hash of its structure; option "fused_spec" 0 switches it off) into name_out[n] and returns
 * 1; returns 0 with an empty string when the program runs on the descriptor-driven kernel or the one-launch-per-op path. */
int dqmc_substep_kernel(dqmc_ctx* ctx, char* name_out, size_t n);
/* The error-predictor scores (see dqmc_last_refined) of the first n walkers of the context's last float32 forward-Laplacian
 * pass, copied to the host: together with the threshold of dqmc_refine_info they say which walkers kept their float32
 * result.  DQMC_E_UNSUPPORTED if the last call ran no such pass (float64 context, "refine" 0 / 2, direct mode). */
int dqmc_refine_scores(dqmc_ctx* ctx, double* out, int n);
/* Non-local ECP term of a float32 context (replaces nonloc_potential, ecp/gaussian_type_ecp.py:161-255, for a whole
 * batch): with "refine" 1 the 12-point quadrature of every (walker, ECP nucleus, electron) triple runs in the precision its
 * weight w = max_l (2l+1)|V_l(|r_i - R_a|)| calls for -- float64 psi ratios above "ecp_heavy_e6" (default 10000 = 1e-2 Ha),
 * float32 below, none below "ecp_skip_e12" (default 100 = 1e-10 Ha: the contribution is below that times the mean ratio).
 * The bound is per walker: psi(r) of every walker is evaluated by both value paths first, and where the float32
 * log|psi(r)| is off by more than "ecp_dlog_floor_e6" (default 30 = 3e-5: half the median float32 error of these networks) the
 * walker's float64 bound tightens in proportion -- near a node psi(r), the denominator of all its ratios, is what float32
 * cannot resolve; a sign mismatch sends all its kept pairs to float64 (0: weights alone decide).  Without a float64 twin
 * (DQMC_E_UNSUPPORTED for this program) every kept pair runs in float32.
 * "ecp_mixed" 0 restores whole-walker float64 quadrature for flagged walkers only.  out3 = triples of the last call
 * {float32, float64, dropped}. */
int dqmc_ecp_counts(dqmc_ctx* ctx, int64_t* out3);
/* Tuning / debugging switches.  "fused" (default 1): evaluate value-only psi (dqmc_wf_eval,
 * MCMC) with the single LDS-resident kernel instead of one launch per op where that is the faster path
 * (N <= 4, or fewer than 1024 walkers; 2 = always, 0 = never, which also keeps every
 * activation buffer readable by dqmc_debug_read); "fused_substep" (1): fold propose / determinants /
 * accept of a Metropolis sub-step into that kernel when N <= 4; "fused_wt": walkers per workgroup tile (0 = automatic);
 * "fused_sched" (3: list scheduling under an LDS budget, 2: as late as possible, 1: full dependency
 * levels, 0: program order); "fused_occ": register budget as workgroups per CU (0 = from the LDS size);
 * "fused_lds_kb", "fused_sched_kb": LDS budgets; "fused_dbg": clock stamps readable through
 * dqmc_debug_read(buf = -3); "fused_print": plan summary on stderr; "ecp_max_cfg": quadrature walkers
 * per value-mode batch of the non-local ECP term; "ws_budget_mb": activation workspace per evaluation
 * (larger batches are split into walker chunks); "lane_compact" (1): 8-lane storage of the edge stream;
 * "attention_mfma", "slogdet_mfma" (1: MFMA kernels where profitable, 2: wherever supported, 0: never);
 * "fused_lean" (1): straight-line unit body for layers with one input piece and K <= 32; "fused_wg_per_cu" (4): LDS share a
 * tile is planned for;
 * "fused_prio" (1): the co-resident tiles of a CU take turns at the highest issue priority, level by level, instead of the
 * hardware's oldest-wave-first order (2: unit by unit, 0: off); "fused_bf" (float32 contexts; 1: the float32 layers of the
 * fused kernel whose pieces are whole octets wide run on the bf16 matrix pipe -- operands split into three bf16 pieces,
 * six v_mfma_f32_16x16x32_bf16 per 16 x 16 x 32 block, float32-class results; 2: only the layers deep enough to pay by
 * the stricter rule; 0: v_mfma_f32_16x16x4_f32 everywhere); "linear_bf" (2): the same split with nine
 * products for the per-op linear kernel -- 2: the Laplacian tiles of the 48-lane groups (11-15 electrons), where it is
 * faster, and of the 16-lane groups (up to 4 electrons), where it costs the same and rounds less often (fewer walkers reach the
 * float64 pass); 1: every layer deep enough (measured slower elsewhere); 0: never; "dual_stream" (1): edge stream of the Laplacian pass on a
 * companion HIP stream; options prefixed "twin." go to the float64 refinement twin;
 * "pass_graph" (1): a forward-Laplacian pass that fits one workspace chunk is captured into a hipGraph on its second call
 * with the same buffers and batch size and replayed afterwards (one hipGraphLaunch instead of ~40 launches and their
 * cross-stream events; contexts without a non-local ECP / pseudo-Hamiltonian, timing off); the float64 twin's batch is
 * rounded up to a multiple of 64 walkers so that a few graphs serve every call; a context whose captures outnumber its
 * replays (callers passing fresh buffers every time) returns to eager launches; 0: always eager;
 * "refine" (float32 contexts; 1: float64 re-evaluation of ill-conditioned walkers, 2: the whole local-energy pass in
 * float64 while sampling stays float32, 0: off), "refine_thresh" (200 until the first probe): score above which mode 1
 * refines a walker, "refine_probe" (32): calls between self-calibration probes (0: keep refine_thresh as set), "refine_sample"
 * (256; 64 until round 4): walkers of the calibration sample, "refine_direct_pct" (60) / "refine_direct_exit_pct" (45): share
 * of a batch above the threshold at which the context enters / leaves the whole-batch float64 mode, "refine_direct_calls" (15): calls it
 * stays there before a float32 pass looks again, "refine_direct_backoff" (4): every look that confirms the mode doubles the stay, at
 * most this many times (15, 30, ... 240 calls),
 * "refine_target_e7" (100): relative tolerance the float32-kept walkers are to meet, in units of 1e-7; "refine_miss_e9" (10):
 * accepted share of kept walkers beyond it, in units of 1e-9 (1e-8 costs LiH / PauliNet ~16 % and N2 / FermiNet ~12 % of their
 * walkers in float64 and leaves the largest float32 error of a 82 k-evaluation trajectory at 5e-6; 100 = 1e-7: ~13 % / ~9 %,
 * largest error 7.6e-6 / 1.01e-5; the 90th-percentile rule of rounds 3-4 refined 5 % and left ~30 of 82 k evaluations beyond
 * the tolerance).
 * "linear_bf", "linear_bkx" act on the calling context only;
 * "linear_f64_split" (float64 contexts, 1): layers over 96- / 128-lane groups with a PAIR of waves per group (two waves per
 * SIMD instead of one); "attention_split" (float64 contexts, 1): eight-wave attention kernel, a pair of waves per query row
 * block; "attention_ncb" (-1: kernel instance per number of key tiles in float32, four-tile instance in float64);
 * "mlp_fuse" (1): row-wise two-layer MLPs in one launch where the chained kernel has an instance;
 * "no_twin" (0; set before the first local-energy call): never create the float64 twin, i.e. plain
 * float32 everywhere, as for a program without a float64 kernel set; "ecp_mixed" (1),
 * "ecp_heavy_e6" (10000), "ecp_skip_e12" (100), "ecp_dlog_floor_e6" (30): mixed-precision non-local ECP quadrature
 * (dqmc_ecp_counts); passes of fewer than 64 walkers are never captured into graphs.
 * Removed in round 5 (each had been measured slower than the default or neutral on the MI355X and was never on; DESIGN.md
 * section 4 keeps the numbers): "refine_defer" + dqmc_refine_finish, "refine_ahead", "mlp_dual", "fused_chain",
 * "fused_stagger", "linear_bf" 3 and its host-split weight planes, "linear_bkx_big", "linear_bkx_val", "linear_f64_nr1".
 * Removed later: "tail_f64" (float64 tail of a float32 forward-Laplacian pass), measured slower than the default and never on.
 * Unknown names return DQMC_E_ARG. */
int dqmc_set_option(dqmc_ctx* ctx, const char* name, int value);

/* Per-kernel timing (HIP events on the context's stream).  enable != 0 starts recording
 * every launch; dqmc_timing_get returns total ms / launch count / algorithmic flops of the
 * kernel class `name` ("linear", "slogdet", ...) accumulated since the last reset. */
int dqmc_timing_enable(dqmc_ctx* ctx, int enable);
int dqmc_timing_reset(dqmc_ctx* ctx);
int dqmc_timing_get(dqmc_ctx* ctx, const char* name, double* ms, int64_t* launches, double* flops);
/* The flops the launches of kernel class `name` actually multiplied, beside dqmc_timing_get's ALGORITHMIC count (the dense
 * T = 3N + 2 lanes of SURVEY.md section 8d, which `roofline.achieved` is priced with): edge rows carry 8 pair-compact lanes,
 * per-walker (broadcast) pieces are multiplied once per walker, lanes are padded to TP and widths to multiples of 4.
 * executed / time / peak is the matrix-pipe utilisation; algorithmic / time / peak is the roofline fraction -- for
 * N2 / FermiNet the two differ by ~2x. */
int dqmc_timing_get_executed(dqmc_ctx* ctx, const char* name, double* flops_executed);
int dqmc_timing_names(dqmc_ctx* ctx, char* out, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* DQMC_H */
