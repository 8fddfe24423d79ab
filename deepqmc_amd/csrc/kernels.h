// kernels.h -- host-callable launchers of the gfx950 kernels (explicitly instantiated for
// float and double in the .hip files).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dqmc.h"
#include "common.h"

namespace dqmc {

// ---- kernels_graph.hip ----
template <typename real>
void launch_feat_en(hipStream_t st, const real* r, const real* R, real* x, int B, int n_nuc, int n_up, int width,
                    LaneInfo li, double eps, int log_rescale, int use_spin, const double* phq = nullptr);
template <typename real>
void launch_feat_ee(hipStream_t st, const real* r, const real* R, const int32_t* pairs, real* e, int B, int n_rows, LaneInfo li,
                    double eps, int log_rescale, int compact, const double* phq = nullptr);
template <typename real>
void launch_const_rows(hipStream_t st, const real* tab, real* x, int B, int rows, int width, LaneInfo li);
template <typename real>
void launch_spin_mean(hipStream_t st, const real* x, real* m, int B, int n_up, int width, LaneInfo li);
template <typename real>
void launch_row_sum(hipStream_t st, const real* x, real* s, int B, int rows, int width, LaneInfo li);
template <typename real>
void launch_conv(hipStream_t st, const real* we, int we_rows, int we_width, const real* hx, int hx_rows, int hx_width, real* out,
                 int out_width, int col0, const int32_t* tab, int S, int W, int B, LaneInfo li, int compact);
template <typename real>
void launch_edge_sum(hipStream_t st, const real* e, int e_rows, int e_width, real* out, int out_width, int col0,
                     const int32_t* tab, int S, int W, double scale, int B, LaneInfo li, int compact);
template <typename real>
void launch_zero_cols(hipStream_t st, real* x, long rows, int width, int c0, int c1);     // x[rows][width], columns [c0, c1) = 0

// ---- kernel_linear.hip ----
// One concat piece of the A operand: logical row (b, rr, t) reads
// src[((b*rpw + r0 + (bcast ? 0 : rr))*TP + t)*ld + k], k < K (K % 4 == 0, zero padded).
template <typename real> struct LinPiece {
  const real* src;
  int ld, rpw, r0, K, bcast;
  int w_row;          // first row of this piece's block in W
};
template <typename real> struct LinArgs {
  int n_pieces;
  LinPiece<real> piece[4];
  const real* W;      // [sum K][ldw]
  int ldw;            // pad4(Nout)
  const real* bias;   // [ldw] or nullptr (value lane only)
  real* dst;
  int ld_dst, rpw_dst, r0_dst, col0_dst;
  const real* pre;    // per-walker addend to the pre-activation, real[B][TP][ld_pre], or nullptr: the product of the
  int ld_pre;         //   per-walker (broadcast) pieces, computed once per walker by a separate launch
  const real* res;    // residual input or nullptr: out = (res + y) * res_scale
  int ld_res, rpw_res, r0_res;
  real res_scale;
  int act;            // 0 none, 1 tanh, 2 silu
  int nrows;          // rows per walker in this segment
  int B;
  int T, TP;
  // chained second layer (launch_linear_chain): Y = act2(H W2 + bias2) with H = act(X W + bias) kept on chip;
  // dst / res / col0_dst then describe Y
  const real* W2;     // [ldw][ldw2]
  int ldw2;           // pad4(Nout of the second layer)
  const real* bias2;
  int act2;
  // kernel-selection switches of the calling context (dqmc_set_option "linear_bf" / "linear_bkx" / "linear_f64_split";
  // read on the host by launch_linear only): per launch, so that contexts -- a float32 engine and its float64 twin,
  // contexts of other threads -- do not steer each other and a captured pass keeps what its own context chose
  int cfg_bf, cfg_bkx, cfg_f64_split;
};
template <typename real> void launch_linear(hipStream_t st, const LinArgs<real>& a);
template <typename real> void launch_linear_chain(hipStream_t st, const LinArgs<real>& a);
bool linear_chain_supported(int TP, int ldw_hidden, int ldw_out);
constexpr int LINEAR_BF_DEFAULT = 2, LINEAR_BKX_DEFAULT = 3;      // (kernel_linear.hip: what the values select)

// ---- kernel_fused2.hip: LDS-resident value-only psi evaluation, descriptor driven ----
struct FusedBuf {
  int off;        // LDS offset in elements (LDS-resident buffers)
  int stride;     // LDS row stride in elements (width + 2)
  int rows;       // rows per walker
  int width;
  int is_global;  // 1: lives in the HBM workspace (read by later kernels)
  long goff;      // byte offset of the buffer in the workspace
};
// One entry of a wave's work list; built on the host (engine.hip: build_fused2_plan), read through scalar loads.
// quads of k-steps per B-operand group of the fused kernel (kernel_fused2.hip: BSet); lean units hold at most one group
// (float: three slots per column block, which are also the three bf16 planes of a K = 32 chunk of a bf16 unit)
template <typename real> struct FusedGroup { static constexpr int P = sizeof(real) == 4 ? 3 : 2; };
struct FDesc {
  int32_t kind;         // 0 end of list, 1 linear unit, 2 workgroup barrier, 3 structured op (all waves), 4 wave-local LDS fence, 5 lean linear unit (one piece, at most FusedGroup::P quads of k-steps, LDS destination), 6 / 7 linear unit / lean unit on the bf16 matrix pipe (float only; a_ks = octets of k, a_nq = chunks of 32 k, qstride = Vec4 per chunk)
  int32_t op;           // scheduled op index (FusedArgs::ops)
  int32_t ma;           // row blocks of the unit (1..4); column blocks are always 2
  int32_t n_pieces;
  int32_t row0;         // first tile row m = row*WT + wl of the unit
  int32_t rtot;         // rows of the segment in the tile (WT * nrows)
  int32_t col0;         // first output column of the unit
  int32_t ldw;          // padded output width of the layer
  int32_t a_base[4];    // LDS offset of segment row m = 0 of concat piece p
  int32_t a_stride[4];
  int32_t a_ks[4];      // k-steps (pad4(K)/4)
  int32_t a_nq[4];      // quads of 4 k-steps
  int32_t bcast;        // bit p: piece p is one row per walker (row index m & (WT-1))
  int32_t w_off;        // Vec4 index of (quad 0, first column block of the unit, lane 0) in the packed weights
  int32_t w_cb1;        // Vec4 distance to the second column block (0: none, re-read the first)
  int32_t qstride;      // Vec4 per quad of k-steps
  int32_t bias_off;     // into the plain weight buffer, or -1
  int32_t dst_base;     // LDS offset of (segment row 0, col0_dst); HBM destination: buffer index
  int32_t dst_stride;
  int32_t res_base;     // LDS offset of (residual segment row 0, col0_dst), or -1
  int32_t res_stride;
  int32_t flags;        // bits 0-1 activation, bit 2 scale by 1/sqrt(2), bit 3 destination in HBM, bit 4 no partial row/column block
  int32_t g_r0, g_col0; // HBM destination: first row / column
  // first weight group of the wave's NEXT unit (of this unit itself when it is the last): the unit requests it before its
  // own epilogue without touching that unit's descriptor (a dependent scalar load = one more ~250-cycle round trip)
  int32_t nx_w_off, nx_cb1, nx_qstride, nx_nq;
};
static_assert(sizeof(FDesc) == 160, "FDesc is 40 dwords");
// Metropolis sub-step folded into the fused kernel (N <= 4): propose r' = r + tau xi in the prologue, the K
// Slater determinants, the CI sum / cusp / Jastrow and the accept step in the tail -- one launch per sub-step
// instead of seven (electron_samplers.py:102-138).  enabled = 0: plain psi evaluation.
struct FusedMc {
  int enabled;
  const void* noise;      // real[B][N][3]
  const void* unif;       // real[B]
  void* r;                // real[B][N][3] sampler state, updated in place
  void* logpsi;           // real[B]
  int32_t* sign;          // [B]
  int32_t* age;           // [B]
  // Step size without a launch of its own: sub-step s reads the step size and the acceptance count of sub-step
  // s-1 (tau_ring[(s+1)&1], counters[(s+2)%3]), every workgroup derives the same tau_s
  // (electron_samplers.py:121-126), workgroup 0 records it in tau_ring[s&1] and clears counters[(s+1)%3];
  // accepts of this sub-step go to counters[s%3].  k_tau_finalize after the last sub-step writes the caller's tau.
  const void* tau_in;     // real[1]: the caller's step size (used by sub-step 0)
  void* tau_ring;         // real[2]
  int32_t* counters;      // int[3], all zero between calls
  int s;                  // sub-step index within this call
  double target;          // target acceptance (<= 0: no adaptation)
  uint8_t* accept_out;    // [B] or nullptr
  int max_age;
  int orb_op;             // scheduled index of the ORBITALS op (backflow buffer, envelope tables)
  int mat_off;            // LDS offset (reals) of WT*K*N*N free elements for the Slater matrices (dead activations)
  int jas_width;          // > 0: a Jastrow value per walker arrives through the scratch area
  int cc_off, al_off, cusp_kind;
  double same_scale, anti_scale;
};
template <typename real> struct Fused2Args {
  const FDesc* descs;       // device: the four wave lists, concatenated
  const int32_t* wave_begin; // device int[8]: first descriptor of each wave, then the first kind-1 descriptor of each wave (-1: none)
  const ::dqmc_op* ops;     // device: the scheduled ops (structured ops read their fields from here)
  const FusedBuf* fbufs;    // device: LDS offset / stride (tile layout [row][WT]) or HBM offset per buffer
  const real* w;
  const real* wpk;
  const int32_t* itable;
  char* ws;
  const real* r;
  const real* R;
  int B, WT, wt_shift, n_up, n_nuc, K;
  int scratch_off;          // LDS offset (in reals) of the per-tile scratch: positions, Jastrow, log|det|, det signs
  int it_off, n_it;         // LDS byte offset and length of the staged int table
  int ma1;                  // every unit is one row block high: launch the specialised kernel
  int prio_mode;            // 0: hardware default (oldest wave first); 1/2: issue priority rotates among the co-resident workgroups per level / per unit
  int stagger_div;          // workgroups per dispatch wave (the co-resident tiles of a CU are blockIdx / stagger_div apart)
  FusedMc mc;
  long long* prof;          // optional clock stamps of workgroup 0: [wave][256]
  long long* prof_wg;       // optional constant-rate (100 MHz) stamps of EVERY workgroup: [n_blocks][2] start, end
  LaneInfo li;
  double eps;
};
// bytes of that scratch area: r tile [WT][N][3], Jastrow [WT][4], log|det| double[WT][K], sign int[WT][K], CI shift double[WT],
// then the staged int table (n_it ints, 16-byte aligned)
__host__ __device__ inline int fused2_scratch_core(int WT, int N, int K, int real_size) {
  return ((WT * (N * 3 + 4) * real_size + 15) / 16 * 16) + WT * K * 12 + WT * 8;
}
__host__ __device__ inline int fused2_scratch_bytes(int WT, int N, int K, int real_size, int n_it = 0) {
  return (fused2_scratch_core(WT, N, K, real_size) + 15) / 16 * 16 + (4 * n_it + 15) / 16 * 16;
}
template <typename real> void launch_fused2_value(hipStream_t st, const Fused2Args<real>& a, int n_blocks, size_t lds_bytes, int occ);
template <typename real> int fused2_set_lds_limit(size_t lds_bytes);
template <typename real> int slogdet_set_lds_limit();       // kernels_head.hip: the Laplacian-mode determinant kernels of 45..64 electrons
template <typename real> int slogdet_bwd_set_lds_limit();   // kernels_grad.inl: k_slogdet_bwd past 44 electrons

// ---- kernel_attention.hip ----
// returns 0, or -1 if the (N, head_dim) tile set does not fit the 160 KiB LDS, -2 on a HIP error
template <typename real>
int launch_attention(hipStream_t st, const real* q, const real* k, const real* v, real* out, int width, int H, int hd,
                     int B, LaneInfo li, int n_const, const real* k_const, const real* v_const);
template <typename real> size_t attention_lds_bytes(int N, int hd, int n_const);
// kernels_attention_bwd.inl: the reverse pass's backward of the op (TP = 1); dq, dk, dv are added into.  n_const > 0: the
// constant key / value rows kc, vc [n_const][H * hd] come first in the key order as in the forward, and their per-walker
// partials are WRITTEN to cpart [B][2][n_const][H * hd] (dKc then dVc).  n_const == 0: kc, vc, cpart are not read.
// Returns 0, or -1 if the shape is not supported (LDS tile set, N * hd or n_const * hd per thread), -2 on a HIP error
template <typename real>
int launch_attention_bwd(hipStream_t st, const real* q, const real* k, const real* v, const real* dout, real* dq, real* dk, real* dv,
                         int width, int H, int hd, int B, int N, int n_const, const real* kc, const real* vc, real* cpart);
template <typename real> size_t attention_bwd_lds_bytes(int N, int hd, int n_const);

// ---- kernels_nuc.inl (included by kernel_attention.hip): the nuclear-token stream of the TransPsiformer in float64 ----
// (engine_nuc.inl says what is chained how; activation codes as DQMC_OP_LINEAR: 0 none, 1 tanh, 2 silu)
void launch_nuc_edge_feat(hipStream_t st, const double* R, const int32_t* types, double eps, double* F, int n);
// Z = X W + b, Y = act(Z) (+ res); Z == Y where act is 0
void launch_nuc_linear(hipStream_t st, const double* X, const double* W, const double* b, double* Z, double* Y, const double* res, int rows,
                       int n_in, int n_out, int act);
// dZ = dY act'(Z) (act 0: dY itself, dZ unused); gW += X^T dZ, gb += column sums (gb may be nullptr); dX += dZ W^T (dX may be nullptr)
void launch_nuc_linear_bwd(hipStream_t st, const double* X, const double* W, const double* Z, const double* dY, double* dZ, double* dX,
                           double* gW, double* gb, int rows, int n_in, int n_out, int act);
void launch_nuc_sender_sum(hipStream_t st, const double* in, double* out, int n, int w);
void launch_nuc_sender_sum_bwd(hipStream_t st, const double* dout, double* din, int n, int w);
void launch_nuc_add(hipStream_t st, double* a, const double* b, long n);
void launch_nuc_attention(hipStream_t st, const double* q, const double* k, const double* v, double* P, double* o, int n, int H, int hd);
void launch_nuc_attention_bwd(hipStream_t st, const double* q, const double* k, const double* v, const double* P, const double* dO, double* dS,
                              double* dq, double* dk, double* dv, int n, int H, int hd);
void launch_nuc_layernorm(hipStream_t st, const double* h, double* ln, double* rstd, int n, int D);
void launch_nuc_layernorm_bwd(hipStream_t st, const double* ln, const double* rstd, const double* dln, double* dh, int n, int D);
void launch_nuc_glu(hipStream_t st, const double* zw, const double* zv, const double* bias, double* zeta, long n);
void launch_nuc_glu_bwd(hipStream_t st, const double* zw, const double* zv, const double* dzeta, double* dzw, double* dzv, double* gbias,
                        long n);
template <typename real>
void launch_nuc_scatter(hipStream_t st, const double* derived, const int32_t* row, const int32_t* col, real* w, double* w64, long n);
// The stream's backward batched over walkers (option "nuclear_coords"; engine_nuc.inl: nuc_fold_coords): adjoints only.  Walker b's
// adjoint arena is G + b * A, laid out like nuc_adj; pointers to adjoints point into walker 0's arena, activations are shared.
// G[b][e] += walker b's partials src[b * stride + (col - w0)] over the copies of derived element e in [w0, w0 + len); e in [e_lo, e_hi)
template <typename T>
void launch_nucb_gather(hipStream_t st, const T* src, long stride, long w0, long len, const int32_t* row, const int32_t* col, long e_lo,
                        long e_hi, double* G, long A, int B);
void launch_nucb_add(hipStream_t st, double* a, const double* c, long n, long A, int B);
void launch_nucb_glu_bwd(hipStream_t st, const double* zw, const double* zv, const double* dzeta, double* dzw, double* dzv, long n, long A,
                         int B);
void launch_nucb_layernorm_bwd(hipStream_t st, const double* ln, const double* rstd, const double* dln, double* dh, int n, int D, long A,
                               int B);
void launch_nucb_sender_sum_bwd(hipStream_t st, const double* dout, double* din, int n, int w, long A, int B);
size_t nucb_attention_bwd_lds_bytes(int n);
void launch_nucb_attention_bwd(hipStream_t st, const double* q, const double* k, const double* v, const double* P, const double* dO,
                               double* dq, double* dk, double* dv, int n, int H, int hd, long A, int B);
// table[z[j] + e] = act'(acts[z[j] + e]), e < n[j], for `count` activated layers (shared by the walkers: once per call)
void launch_nucb_dact(hipStream_t st, const double* acts, double* table, const int* act, const long* z, const long* n, int count);
// dX[m][i] += sum_o dY[m][o] dA[rr][o] W[i][o], i < k_cols <= n_in, rows m = (b, rr < rows), on the float64 MFMA with the W panel
// in the LDS; dA = act'(Z) of the layer (launch_nucb_dact) or nullptr (no activation); with dA, writes dZ = dY act'(Z).
// nucb_dx_col_tiles: 16-column tiles per workgroup, 0 if no panel fits the LDS (launch_nucb_dx then returns -1 without
// launching; -2 on a HIP error)
int nucb_dx_col_tiles(int k_cols, int n_out);
size_t nucb_dx_lds_bytes(int ct, int n_out);
int launch_nucb_dx(hipStream_t st, const double* dY, const double* dA, const double* W, double* dZ, double* dX, int rows, int B, int n_in,
                   int n_out, int k_cols, long A);
// the edge features' adjoint dF [B][n n][4 + n] carried into R and added into grad_R [B][n][3] (rows of invalid walkers are kept)
template <typename real>
void launch_nucb_edge_feat_bwd(hipStream_t st, const double* R, double eps, const double* dF, int n, long A, const real* lp, const int32_t* sg,
                               real* grad_R, int B);

// Option "nuclear_params" (engine_nuc.inl: nuc_fold_rows): per-walker parameter partials of one stream layer on the float64 MFMA,
// dW_b = X^T dZ_b (X [rows][n_in] shared, dZ_b [rows][n_out] at dZ + b * A) and db_b = colsum dZ_b (b_off -1: no bias).  The
// X^T tile of a workgroup lives in the LDS: -1, launching nothing, when 16 x pad4(rows) doubles exceed it (nucb_dw_fits); -2 on
// a HIP error.  store: ADDS walker b's partials to row b of out [B][ld] at w_off / b_off (theta order).  sqsum: F[w_off + e] +=
// sum_b dW_b[e]^2 (F over theta), the walkers in NUCB_DW_SLICES contiguous slices whose sums meet in ascending order through
// part (nucb_dw_part_doubles doubles); no per-walker rows, no atomics.
constexpr int NUCB_DW_SLICES = 8;
bool nucb_dw_fits(int rows);
size_t nucb_dw_lds_bytes(int rows);
size_t nucb_dw_part_doubles(int n_in, int n_out);
template <typename real>
int launch_nucb_dw_store(hipStream_t st, const double* X, const double* dZ, long A, int rows, int n_in, int n_out, int B, real* out, long ld,
                         long w_off, long b_off);
int launch_nucb_dw_sqsum(hipStream_t st, const double* X, const double* dZ, long A, int rows, int n_in, int n_out, int B, double* F,
                         long w_off, long b_off, double* part);
// the zeta tables' bias: walker b's partial is its adjoint of the table (dzeta + b * A, n entries)
template <typename real>
void launch_nucb_zbias_store(hipStream_t st, const double* dzeta, long A, long n, int B, real* out, long ld, long off);
void launch_nucb_zbias_sqsum(hipStream_t st, const double* dzeta, long A, long n, int B, double* F, long off);
// jt[b][p] = sum of jac[b][col] over the copies of parameter element p (CSR row / col, ascending), zero rows for invalid walkers
template <typename real>
void launch_jac_to_params(hipStream_t st, const real* jac, long ld_jac, const int32_t* row, const int32_t* col, const real* lp,
                          const int32_t* sg, real* jt, long ld_t, long n_params, int B);

// ---- kernel_attention_mfma.hip: contractions on MFMA, float32 and float64 (head_dim % 16 == 0, <= 64 queries / keys) ----
template <typename real> size_t attention_mfma_lds_bytes(int N, int hd, int n_const);
template <typename real> bool attention_mfma_supported(int N, int hd, int n_const);
bool attention_mfma_profitable(int N);
// split variant: eight waves, a pair per query row block (kernel_attention_mfma.hip); returns -1 when the shape is not supported
template <typename real> size_t attention_mfma_split_lds_bytes(int N, int hd, int n_const);
template <typename real>
int launch_attention_mfma_split(hipStream_t st, const real* q, const real* k, const real* v, real* out, int width, int H, int hd, int B,
                                LaneInfo li, int n_const, const real* k_const, const real* v_const);
template <typename real>
int launch_attention_mfma(hipStream_t st, const real* q, const real* k, const real* v, real* out, int width, int H,
                          int hd, int B, LaneInfo li, int n_const, const real* k_const, const real* v_const,
                          int exact_tiles = 1);      // 0: the instance for four key tiles whatever their number (option "attention_ncb")

// ---- kernels_head.hip ----
template <typename real>
void launch_orbitals(hipStream_t st, const real* r, const real* R, const real* bf, int bf_width, real* orb,
                     int orb_width, const real* pi_up, const real* pi_dn, const real* ze_up, const real* ze_dn, int B,
                     int n_up, int n_nuc, int n_env, int K, LaneInfo li, double eps, const double* phq = nullptr);
template <typename real>
void launch_slogdet(hipStream_t st, const real* orb, int orb_width, double* logdet, int32_t* sign_k, int B, int K,
                    LaneInfo li, int use_mfma, double* cond = nullptr);
struct FinalArgs {
  const void* r;          // real[B][N][3]
  const void* R;          // real[n_nuc][3]
  const double* charges;  // device double[n_nuc] (valence charges Z_eff when an ECP is set)
  const double* ecp_loc;  // device double[n_nuc][3][2][ecp_nt] local ECP terms, or nullptr
  int ecp_nt;
  const double* logdet;   // [B][K][TP]
  const int32_t* sign_k;  // [B][K]
  const void* jastrow;    // real[B][1][TP][jas_width] or nullptr
  int jas_width;
  const void* conf_coeff; // real[K] or nullptr
  const void* alphas;     // real[2]
  int cusp_kind;
  double same_scale, anti_scale;
  double eps;
  int B, n_up, n_nuc, K;
  LaneInfo li;
  // outputs (any may be nullptr)
  void* logpsi;   // real[B]
  int32_t* sign;  // [B]
  void* e_loc;    // real[B]
  void* stats;    // real[6][stats_ld], this call's walkers at columns 0..B-1
  long stats_ld;  // leading dimension of stats (the caller's total batch when evaluating a chunk)
  void* grad;     // real[B][3N]
  // float64 refinement (float32 build): the float32 error of E_loc is predicted by
  //   score = (|lap| + |grad|^2) / max(1, |E_loc|)  x  max(1, sum_k |p_k| kappa_k)
  // -- the cancellation in E_kin = -(lap + |grad|^2)/2 (both terms ~ 1/psi^2 near a node) times the conditioning record
  // of the Slater matrices that carry psi (kernels_head.hip, above k_slogdet).  Walkers with score > refine_thresh or a
  // non-finite E_loc are appended to flag_idx (global walker index b_offset + b); nullptr: no flagging.
  // score_out [B_total] (indexed like flag_idx) and kappa_out [B] (this chunk) receive the two records.
  int32_t* flag_count;
  int32_t* flag_idx;
  double refine_thresh;
  const double* thresh_dev;  // when set: the threshold is read from here (a replayed hipGraph of the pass follows re-calibrations)
  int b_offset;
  const double* cond;     // [B][K] conditioning record of the determinant kernels, or nullptr
  double* score_out;
  double* kappa_out;
  // pseudo-Hamiltonian (ecp/pseudo_hamiltonian.py): per-(walker, electron) factors [B][N][PH_STRIDE] the derivative
  // lanes were seeded with (and the electron's share of the local PH potential); nullptr = ordinary kinetic energy
  const double* phq;
};
template <typename real> void launch_final(hipStream_t st, const FinalArgs& a);

// ---- kernels_ecp.hip ----
struct EcpArgs {
  const void* r;           // real[B][N][3], all walkers
  const void* R;           // real[n_nuc][3]
  const int32_t* nl_nuc;   // device [n_nl]: nuclei with a non-local part
  const double* nl;        // device [n_nl][L][2][n_t]: exponents ([.,l,0,.]) and coefficients ([.,l,1,.])
  const void* phi;         // real[B][n_nl][N] rotation angles, or nullptr: Philox(seed)
  // float64 twin evaluating a gathered subset of a float32 context's walkers: walker b of this call is walker
  // walker_idx[b] of the caller's batch (rotation angles -- explicit or Philox -- are keyed by THAT index), and the
  // explicit angles are the caller's float array
  const int32_t* walker_idx;
  int phi_f32;
  uint64_t seed;
  int B, N, n_nl, L, n_t;
  int b0, nb;              // walker chunk of this launch
};
// mixed-precision quadrature of a float32 context (kernels_ecp.hip)
struct EcpMixArgs {
  const float* r;          // float[B][N][3], all walkers of the caller
  const float* R;          // float[n_nuc][3]
  const int32_t* nl_nuc;
  const double* nl;
  const float* phi;        // float[B][n_nl][N] rotation angles, or nullptr: Philox(seed)
  uint64_t seed;
  int B, N, n_nl, L, n_t;
  int b0, nb;              // walker chunk of this launch
  double w_heavy, w_skip;  // class bounds on w = max_l (2l+1) |V_l(r_ia)|
  // Measured float32 error of log|psi(r)| of the chunk's own walkers (both value paths evaluate them before the pairs are
  // classified): l32 / l64 [nb] and their signs, or nullptr.  psi(r) is the denominator of every ratio of a walker, and near
  // a node it is the quantity float32 cannot resolve (while the ratios themselves grow like 1 / psi(r)): the float64 bound
  // of a walker's pairs tightens in proportion, w x max(1, |l32 - l64| / dlog_floor) > w_heavy; a sign mismatch sends
  // every kept pair of the walker to float64.
  const float* l32; const double* l64; const int32_t* s32; const int32_t* s64;
  double dlog_floor;
};
void launch_ecp_classify(hipStream_t st, const EcpMixArgs& a, int32_t* cls, int32_t* list_l, int32_t* list_h, int32_t* counts);
template <typename real_out> void launch_ecp_points_list(hipStream_t st, const EcpMixArgs& a, const int32_t* list, int n_list, real_out* rq);
void launch_ecp_reduce_mixed(hipStream_t st, const EcpMixArgs& a, const int32_t* cls, const float* lq32, const int32_t* sq32,
                             const double* lq64, const int32_t* sq64, float* e_loc, float* stats);
template <typename real> void launch_ecp_points(hipStream_t st, const EcpArgs& a, real* rq);
template <typename real>
void launch_ecp_reduce(hipStream_t st, const EcpArgs& a, const real* logq, const int32_t* signq, const real* log0,
                       const int32_t* sign0, real* e_loc, real* stats, real* v_nl_out);
// Hellmann-Feynman force of a Gaussian-type ECP Hamiltonian (dqmc_ecp_force).  Configurations of a walker chunk: [0, nb) the
// walkers themselves, then 11 per (walker, non-local nucleus j, electron i) triple t = (bl n_nl + j) N + i (vertices 1 .. 11;
// vertex 0 is the electron itself).  lq / sq / gr / gR: log|psi|, sign, d log|psi| / dr [n_cfg][N][3] and / dR [n_cfg][n_nuc][3]
// of those configurations (the Coords reverse pass); gj: double[nb][n_nl][n_nuc][3], nucleus j's part of the non-local gradient.
constexpr int ECPF_NQ = 11;      // configurations per (walker, nucleus, electron) triple: vertices 1 .. 11
template <typename real> void launch_ecp_force_points(hipStream_t st, const EcpArgs& a, real* rq);
template <typename real>
void launch_ecp_force_reduce(hipStream_t st, const EcpArgs& a, int n_nuc, int all_rows, const real* lq, const int32_t* sq, const real* gr,
                             const real* gR, double* gj);
// force[b][K] = part0 + part1 (+ the zero-bias term when e_loc is given); part0 = F_nuc - dV_loc/dR, part1 = -sum_j gj (0 when
// gj is nullptr); lq / sq / gR: the chunk's own walkers, or nullptr when no reverse pass has run; part0 / part1 may be nullptr.
template <typename real>
void launch_ecp_force_local(hipStream_t st, const EcpArgs& a, int n_nuc, const double* Z, const double* loc, int nt_loc, const double* gj,
                            const real* lq, const int32_t* sq, const real* gR, const real* e_loc, double energy, double* force,
                            double* part0, double* part1);
template <typename real>
void launch_ph_coeffs(hipStream_t st, const real* r, const real* R, const int32_t* ph_nuc, int n_ph, const double* rv_loc,
                      const double* rv_l2, int n_grid, double r_max, int B, int N, double* phq);

// ---- kernels_mcmc.hip ----
template <typename real>
void launch_rng(hipStream_t st, real* noise, long n_noise, real* unif, long n_unif, uint64_t seed, uint64_t stream_id);
template <typename real>
void launch_propose(hipStream_t st, const real* r, const real* noise, const real* tau, real* r_prop, long n);
template <typename real>
void launch_accept(hipStream_t st, real* r, real* logpsi, int32_t* sign, int32_t* age, const real* r_prop,
                   const real* logpsi_prop, const int32_t* sign_prop, const real* unif, int max_age, int B, int N,
                   int32_t* n_accept, uint8_t* accept_out);
template <typename real>
void launch_tau_update(hipStream_t st, real* tau, int32_t* n_accept, int B, double target, double* acc_out);
template <typename real>
void launch_tau_finalize(hipStream_t st, real* tau, const real* tau_ring, int32_t* counters, int s_last, int B, double target,
                         double* acc_out);
template <typename real>
void launch_sampler_stats(hipStream_t st, const real* r, const real* logpsi, const int32_t* age, const real* tau,
                          const double* acc, int B, int N, double eps, double* stats7);
template <typename real>
void launch_energy_stats(hipStream_t st, const real* e_loc, const real* w, int B, double* out7);
template <typename real>
void launch_clean_force(hipStream_t st, const real* grad, const real* r, const real* R, const double* Z, const real* tau, int B,
                        int N, int n_nuc, real* force);
template <typename real>
void launch_langevin_propose(hipStream_t st, const real* r, const real* force, const real* noise, const real* tau, real* r_prop, long n);
template <typename real>
void launch_langevin_accept(hipStream_t st, real* r, real* logpsi, int32_t* sign, int32_t* age, real* force, const real* r_prop,
                            const real* lp_prop, const int32_t* sign_prop, const real* force_prop, const real* unif, const real* tau,
                            int max_age, int B, int N, int32_t* n_accept, uint8_t* accept_out);
template <typename real>
void launch_exchange_propose(hipStream_t st, const real* r, const int32_t* up_idx, const int32_t* down_idx, int n_up, int B, int N,
                             real* r_prop);
void launch_read_accept(hipStream_t st, int32_t* n_accept, int B, double* acc_out);
void launch_refine_gather(hipStream_t st, const float* r, const float* R, const int32_t* idx, const int32_t* count, int n, int n3,
                          int nR3, double* r64, double* R64);
void launch_refine_scatter(hipStream_t st, const int32_t* idx, const int32_t* count, int n, int n_scatter, const double* score,
                           double thresh, int n3, const double* e64, const double* st64,
                           const double* g64, const double* lp64, const int32_t* sg64, float* e_loc, float* stats,
                           long stats_ld, float* grad, float* logpsi, int32_t* sign);

// ---- kernels_grad.inl (included by kernel_linear.hip): reverse pass of the value-only program (dqmc_log_psi_vjp) ----
template <typename real> struct LinBwdPiece {
  const real* X;      // the piece's source buffer (forward activations)
  real* dX;           // its adjoint (same layout), or nullptr
  int ld, rpw, r0, K, bcast;   // K: unpadded width
  int w_row;          // first row of the piece's block in W
};
template <typename real> struct LinBwdArgs {
  int n_pieces;
  LinBwdPiece<real> piece[4];
  const real* W;      // [sum pad4(K)][ldw]
  int ldw, nout, nrows, B, act;
  const real* Z;      // recomputed pre-activations real[B][nrows][ldw]
  real* dZ;           // scratch of the same shape
  real* dZs;          // scratch real[B][ldw] (broadcast pieces)
  const real* dY;     // adjoint of the destination buffer
  int ld_dst, rpw_dst, r0_dst, col0_dst;
  real* dres;         // adjoint of the residual input, or nullptr
  int ld_res, rpw_res, r0_res;
  real res_scale;
  double* dW;         // gradient of W (double, flat weight layout), accumulated; nullptr (with dbias nullptr): dX only
  double* dbias;      // gradient of the bias, or nullptr
  double* part;       // split-K scratch: grad_dw_part_doubles of the largest block
  const double* wt;   // per-walker weights of the weight-gradient sums (dqmc_log_psi_kfac), or nullptr: unweighted
};
// Split-K of the weight-gradient GEMMs: about GRAD_DW_WAVES waves (16 x 16 tiles x splits) per launch, at most GRAD_DW_MAX_SPLIT
// splits (the fixed-order second pass reads every split of an entry serially) and at least 64 rows per split
constexpr long GRAD_DW_WAVES = 4096, GRAD_DW_MAX_SPLIT = 64;
inline long grad_dw_splits(int kt, int nt, long M) {
  const long tiles = (long)kt * nt;
  long s = (GRAD_DW_WAVES + tiles - 1) / tiles;
  if (s > GRAD_DW_MAX_SPLIT) s = GRAD_DW_MAX_SPLIT;
  const long cap = (M + 63) / 64;
  if (s > cap) s = cap;
  return s < 1 ? 1 : s;
}
// doubles of split partials a block of kt x nt tiles needs at most (any M)
inline size_t grad_dw_part_doubles(int kt, int nt) {
  const long tiles = (long)kt * nt;
  long s = (GRAD_DW_WAVES + tiles - 1) / tiles;
  if (s > GRAD_DW_MAX_SPLIT) s = GRAD_DW_MAX_SPLIT;
  return (size_t)s * tiles * 256;
}
template <typename real> void launch_linear_bwd(hipStream_t st, const LinBwdArgs<real>& a);
// out[m] += sum_c in[c * stride + m] (c < count, m < n_out), fixed summation order; with wt, term c is in[..] * wt[c]
// (exactly 0 where wt[c] == 0)
template <typename real>
void launch_colsum(hipStream_t st, const real* in, long count, long stride, int n_out, double* out, const double* wt = nullptr);
void launch_colsum_f64(hipStream_t st, const double* in, long count, long stride, int n_out, double* out, const double* wt = nullptr);
template <typename real> void launch_spin_mean_bwd(hipStream_t st, real* dx, const real* dm, int B, int N, int n_up, int width);
template <typename real> void launch_row_sum_bwd(hipStream_t st, real* dx, const real* ds, int B, int rows, int width);
// edge-row adjoint of CONV (hx given) / EDGE_SUM (hx == nullptr, factor `scale`) through rtab[row][Sr][2] = (receiver, sender)
template <typename real>
void launch_edge_rows_bwd(hipStream_t st, real* dwe, int we_rows, int we_w, const real* hx, int hx_rows, int hx_w, const real* dout,
                          int out_w, int col0, const int32_t* rtab, int Sr, int W, int B, int N, double scale);
// sender adjoint of CONV through stab[sender row][Ss][2] = (receiver, edge row)
template <typename real>
void launch_conv_send_bwd(hipStream_t st, real* dhx, int hx_rows, int hx_w, const real* we, int we_rows, int we_w, const real* dout,
                          int out_w, int col0, const int32_t* stab, int Ss, int W, int B, int N);
template <typename real> struct FinalBwdArgs {
  const real* r;
  const double* logdet;   // [B][K] (TP = 1)
  const int32_t* sign_k;
  const real* cc;         // conf_coeff [K] or nullptr
  const real* alphas;     // [2]
  int cusp_kind;
  double same_scale, anti_scale, eps;
  const real* logpsi;
  const int32_t* sign;
  const real* cot;        // [B] or nullptr (ones)
  real* djas;             // adjoint of the Jastrow buffer or nullptr
  int jas_ld;
  double* dL;             // out [B][K]: cot * p_k
  double* pw;             // out [B][K + 2]: per-walker gradient of conf_coeff and of {same_alpha, anti_alpha}
  int B, N, n_up, K;
};
template <typename real> void launch_final_bwd(hipStream_t st, const FinalBwdArgs<real>& a);
constexpr int GRAD_GJ_NMAX = 64;      // largest N of the Gauss-Jordan inverse of k_slogdet_bwd (as the forward slogdet)
template <typename real> void launch_slogdet_bwd(hipStream_t st, const real* orb, int orb_w, const double* dL, real* dorb, int B, int K, int N);
// pw: per-walker partials double[B][4][K*N][n_nuc*n_env] of the pi_up / pi_down / zeta_up / zeta_down tables, or nullptr (the
// backflow adjoint alone)
template <typename real>
void launch_orbitals_bwd(hipStream_t st, const real* r, const real* R, const real* bf, int bf_w, real* dbf, const real* dorb, int orb_w,
                         const real* pi_up, const real* pi_dn, const real* ze_up, const real* ze_dn, double* pw, int B, int N, int n_up,
                         int n_env, int n_nuc, int K, double eps);

// ---- kernels_jac.inl (included by kernel_linear.hip): per-walker parameter Jacobian (dqmc_log_psi_jacobian) ----
// LINEAR weight blocks are formed per walker in tiles of at most JAC_TILE entries (LDS staged), JAC_MAX_COLS columns wide
constexpr int JAC_TILE = 4096, JAC_MAX_COLS = 1024;
template <typename real> struct JacOut {
  real* J;              // row b of walker b of the chunk, ld entries apart
  long ld;
  const real* lp;       // log|psi| and sign of the chunk's walkers: sign 0 or a non-finite log|psi| gives zeros
  const int32_t* sg;
  int accum;            // 1: add into J (rows zeroed first), 0: plain stores (no weight block is shared between ops)
  int vec;              // 1: J and ld allow 16-byte stores
};
// the LINEAR reverse pass with the weight gradient per walker: k_lin_dz and k_lin_dx as launch_linear_bwd, the weight block of
// every piece at column w_col + w_row * ldw and the bias at bias_col (< 0: none); a.dW, a.dbias and a.part are not used
template <typename real> void launch_linear_jac(hipStream_t st, const LinBwdArgs<real>& a, const JacOut<real>& o, long w_col, long bias_col);
// J[b][col + m] = (real) src[b * stride + m], m < n (added with o.accum)
template <typename T, typename real> void launch_jac_scatter(hipStream_t st, const T* src, long stride, int n, int B, const JacOut<real>& o, long col);
// J[b][cols[m]] = 0, m < n (cols == nullptr: columns 0 .. n-1)
template <typename real> void launch_jac_zero(hipStream_t st, real* J, long ld_jac, const int32_t* cols, int n, int B);

// ---- kernels_kfac.inl (included by kernel_linear.hip): KFAC Kronecker factors (dqmc_log_psi_kfac) ----
// Gram products: super-tiles of GRAM_TI x GRAM_TJ 16 x 16 tiles (one tile row per wave), LDS row blocks of GRAM_RB_MAX rows
// (float; half as many for double), about GRAM_WGS workgroups per launch
constexpr int GRAM_TI = 4, GRAM_TJ = 8, GRAM_RB_MAX = 64;
constexpr long GRAM_WGS = 512;
template <typename real> struct GramPiece {
  const real* X;      // rows X[(b * rpw + r0 + (bcast ? 0 : rr)) * ld + kk], kk < K
  int ld, rpw, r0, K, Kp, bcast;   // Kp = pad4(K) columns of y, zeros past K
  int col0;           // first column of y
};
template <typename real> struct GramArgs {
  int n_pieces;
  GramPiece<real> piece[4];
  int bias_col;       // column of the constant 1, or -1
  int D;              // columns of y
  int nrows;          // rows per walker
  long M;             // B * nrows
  const double* ok;   // per walker: 0 = contributes nothing
};
struct GramPlan { int nt, T, RB; long groups, S, m_per; };
GramPlan gram_plan(int D, long M, int real_bytes);
size_t gram_part_doubles(int D);
// A += sum over the valid walkers' rows of x~ x~^T (x~: the pieces of a, zero padded to pad4(K), then 1 if has_bias) and
// G += sum dZ dZ^T over the ldw columns of a.dZ; part: gram_part_doubles of the larger of the two
template <typename real>
void launch_kfac_factors(hipStream_t st, const LinBwdArgs<real>& a, int has_bias, const double* ok, double* A, double* G, double* part);
// w[b] = cot[b] (cot == nullptr: 1) and w[B + b] = 1 for valid walkers, 0 and 0 otherwise
template <typename real> void launch_kfac_weights(hipStream_t st, const real* lp, const int32_t* sg, const real* cot, double* w, int B);

// ---- kernels_coords.inl (included by kernel_linear.hip): coordinate reverse pass (dqmc_log_psi_grad_coords), force estimators ----
// Slots: double[B][n_slots][3], d log|psi| / d d of one difference d = r_p - r_q each; `slot` points at the first slot of the op's
// range.  FEAT_EN / ORBITALS: slot i * n_nuc + a (d = r_i - R_a); FEAT_EE: slot `row`; cusps: the pair (i < j, row-major), d = r_i - r_j.
template <typename real>
void launch_feat_en_coords(hipStream_t st, const real* r, const real* R, const real* dx, int width, int B, int N, int n_nuc, double eps,
                           int log_rescale, double* slot, int n_slots);
template <typename real>
void launch_feat_ee_coords(hipStream_t st, const real* r, const real* R, const int32_t* pairs, const real* de, int n_rows, int B, int N,
                           double eps, int log_rescale, double* slot, int n_slots);
template <typename real>
void launch_orbitals_coords(hipStream_t st, const real* r, const real* R, const real* bf, int bf_w, const real* dorb, int orb_w,
                            const real* pi_up, const real* pi_dn, const real* ze_up, const real* ze_dn, int B, int N, int n_up, int n_env,
                            int n_nuc, int K, double eps, double* slot, int n_slots);
template <typename real>
void launch_cusp_coords(hipStream_t st, const real* r, const real* alphas, int cusp_kind, double same_scale, double anti_scale,
                        double eps, int B, int N, int n_up, double* slot, int n_slots);
// grad_r[b][i] / grad_R[b][a] (either may be nullptr) = sum over tab[particle][S][2] = (slot, +1 / -1), slot -1 = end of the list
template <typename real>
void launch_coords_gather(hipStream_t st, const double* slot, int n_slots, const int32_t* tab, int S, const real* lp, const int32_t* sg,
                          int B, int N, int n_nuc, real* grad_r, real* grad_R);
template <typename real>
void launch_hf_force(hipStream_t st, int est, const real* r, const real* R, const double* Z, const real* gr, const real* gR,
                     const real* e_loc, double energy, int B, int N, int n_nuc, double* force);

// ---- kernels_pretrain.inl (included by kernel_linear.hip): SCF-orbital pretraining (dqmc_pretrain_target, dqmc_orbitals_vjp, ...) ----
constexpr int PT_AO_CAP = 4096;       // atomic-orbital values (electrons of one tile x n_ao) k_pretrain_target keeps in LDS
constexpr int PT_SHELL_INTS = 5;      // per shell: atom, l, first primitive, primitives, first AO
constexpr int PT_LMAX = 3;
// target: real[B][n_conf][N][N]; shells int32 [n_shell][PT_SHELL_INTS], prims real [.][2] = (coeff x rnorm, zeta), mo real [n_ao][n_mo],
// confs int32 [n_conf][N], fac real [n_conf][2] = (|c|^(1/N), sign c); n_ao <= PT_AO_CAP
template <typename real>
void launch_pretrain_target(hipStream_t st, const real* r, const real* R, const int32_t* shells, const real* prims, const real* mo,
                            const int32_t* confs, const real* fac, real* target, int B, int N, int n_shell, int n_ao, int n_mo,
                            int n_conf);
// dst[row][e] = src[row][e], e < NN, for `rows` rows of leading dimensions dst_ld / src_ld
template <typename real>
void launch_orbitals_copy(hipStream_t st, const real* src, long src_ld, real* dst, long dst_ld, int NN, long rows);
// loss[b] (double) and the cotangent dorb of the ORBITALS buffer orb (both [B][K][orb_w]) against the tiled, block-diagonal target
template <typename real>
void launch_pretrain_loss(hipStream_t st, const real* orb, int orb_w, const real* target, real* dorb, double* loss, int B, int N,
                          int n_up, int K, int n_conf, double n_total);

// ---- kernels_optim.inl (included by kernel_linear.hip): device-resident optimiser step (dqmc_weights_from_params, dqmc_adam_step, ...) ----
// One destination word of a packed weight buffer (the tape of a generated sub-step kernel, the planes of the fused kernel) as
// a function of the flat weights w: plane < 0: the word is w[src0] * scale in `real` (src0 < 0: zero); plane 0..2: a 32-bit
// word of two bf16 numbers, piece `plane` of the three-way split of (float)w[src0] * scale (low half) and of w[src1] (high).
// The tables are written by the host packers themselves (spec_registry.hip: spec_tape_sources, engine_fused_plan.inl).
struct PackSrc { int32_t src0, src1; float scale; int32_t plane; };
constexpr int OPT_BLOCK = 256;        // threads per workgroup of the optimiser kernels
constexpr int OPT_MAX_BLOCKS = 1024;  // workgroups of an optimiser launch at most = partial sums of a norm
// w[j] = (real)theta[src[j]] and w64[j] = theta[src[j]] (w64 may be nullptr) where src[j] >= 0; other entries are left alone
template <typename real>
void launch_weights_from_params(hipStream_t st, const double* theta, const int32_t* src, real* w, double* w64, long n);
// out[q] (real, or 32-bit words for real = float) per tab[q] from the flat weights w, n words
template <typename real>
void launch_pack_words(hipStream_t st, const PackSrc* tab, const real* w, real* out, long n);
template <> void launch_pack_words<float>(hipStream_t st, const PackSrc* tab, const float* w, float* out, long n);
template <> void launch_pack_words<double>(hipStream_t st, const PackSrc* tab, const double* w, double* out, long n);
// grad_theta[e] = sum of grad_w[col[k]], k in [row[e], row[e + 1]), in that order
void launch_grad_to_params(hipStream_t st, const double* grad_w, const int32_t* row, const int32_t* col, double* grad_theta, long n_params);
// optax.adam with bias corrections c1 = 1 - b1^t, c2 = 1 - b2^t, in place on theta, mu, nu.  part: double[3][OPT_MAX_BLOCKS]
// scratch and norms3: double[3] = 2-norms of theta (before the step), g and the update, or both nullptr.
void launch_adam(hipStream_t st, double* theta, double* mu, double* nu, const double* g, long n, double lr, double b1, double b2,
                 double eps, double c1, double c2, double* part, double* norms3);
// theta += scale * delta; norms3 = 2-norms of theta (before), delta and scale * delta
void launch_apply_update(hipStream_t st, double* theta, const double* delta, double scale, long n, double* part, double* norms3);

// ---- kernels_kfacopt.inl (included by kernel_linear.hip): the KFAC preconditioner on flat device vectors (dqmc_kfac_direction, dqmc_kfac_apply) ----
constexpr int KF_NB = 32;     // panel width of the blocked Cholesky factorisation and of the blocked triangular solves
constexpr int KF_ROWS = 64;   // rows behind a panel per workgroup (one thread each)
constexpr int KF_RB = 16;     // right-hand sides per workgroup of a triangular solve
// One Kronecker module: A_hat (da x da, bias = last row) and G_hat (dg x dg) at a_st / g_st of the state (and of the two
// workspaces M, L, which share the state's layout); its block [W; b] at w_pos (n_in x dg, row-major) and b_pos (-1: none) of a
// parameter-ordered vector; its ops are op[op0 .. op1).
struct KfMod { long a_st, g_st, w_pos, b_pos; int da, dg, n_in, R, op0, op1; };
// One LINEAR op: A_l (d_a x d_a) and G_l (d_g x d_g) at a_off / g_off of the factor buffer; inv[inv_row + i] is the row of A_l
// that holds row i of the module's A, inv[inv_col + j] the column of G_l that holds column j of its G.
struct KfOp { long a_off, g_off; int d_a, d_g, inv_row, inv_col; };
struct KfMat { long ws; int n, pad; };       // a matrix of the factorisation list (sorted by n, descending): offset in M / L
struct KfTables {
  const KfMod* mod; const KfOp* op; const int32_t* inv;
  const long* mat_start;      // [2 n_mod + 1] first state element of A_0, G_0, A_1, ...; the last entry = n_mat_elems
  const KfMat* mats;          // [2 n_mod]
  const long* diag_pos;       // [n_diag] parameter element of every diagonal entry
  const long* diag_row;       // [n_diag + 1] CSR over diag_col
  const long* diag_col;       // rest columns that hold the copies of an element, ascending
  int n_mod;
  long n_diag, n_mat_elems;
};
struct KfacDirArgs {
  KfTables t;
  const double* g; const double* factors; const void* rest; long n_rest; const void* logpsi; const int32_t* sign; int B;
  double* state; int first; double ema, damping;
  double* delta; double* dot;
  double* M; double* L;       // [n_mat_elems] each
  double* scal;               // [1 + n_mod]: n_v, pi per module
  double* part;               // [3][OPT_MAX_BLOCKS]
  long n_params;
  int max_n, max_da, max_dg, n_panels;
  const int* active;          // host, [n_panels + 1]: matrices that have panel k (a prefix of mats)
  const double* nuc_F;        // [n_params] or nullptr: sum_b o_bi^2 of the diagonal entries with an empty CSR row (the nuclear stream's)
};
// delta must already hold a copy of g; `real` is the type of rest and logpsi
template <typename real> void launch_kfac_direction(hipStream_t st, const KfacDirArgs& a);
// theta += -lr min(1, sqrt(norm_constraint / (lr^2 dot))) delta; norms4 (or nullptr) = |theta before|, |delta|, |update|, lr^2 dot
void launch_kfac_apply(hipStream_t st, double* theta, const double* delta, const double* dot, double lr, double norm_constraint, long n,
                       double* part, double* norms4);

// ---- kernels_loss.inl (included by kernel_linear.hip): loss assembly of multi-state training (dqmc_psi_ratio, dqmc_clip_rows, dqmc_loss_cotangents) ----
constexpr int LOSS_BLOCK = 256;          // threads per workgroup = bins of a radix-select pass; one workgroup per row
constexpr int LOSS_MAX_STATES = 32;      // electronic states of a batch at most
enum { LOSS_CENTER_MEAN = 0, LOSS_CENTER_MEDIAN = 1 };
enum { LOSS_SCALE_MEAN_ABS_DEV = 0, LOSS_SCALE_MEDIAN_ABS_DEV = 1 };
enum { LOSS_SPIN_NONE = 0, LOSS_SPIN_SQUARED = 1, LOSS_SPIN_RAISING = 2 };
// arguments of dqmc_loss_cotangents (device pointers; r_clip == nullptr: no overlap term)
struct LossCotArgs {
  int S;
  long B;
  const double* w;                 // [S][B] or nullptr (all ones)
  const double* e_clip; const uint8_t* e_mask; const double* e_stats;       // [S][B], [S][B], [S][4]
  double alpha;
  const double* r_clip; const uint8_t* r_mask; const double* r_stats;       // [S][S][B], [S][S][B], [S*S][4]
  const double* scale; const int32_t* rank;                                 // [S][S], [S]
  int spin_kind;
  double lambda;
  const double* spin; const uint8_t* spin_mask; const double* spin_stats;   // [n_states][B]; raising: clipped rows, mask, [n_states][4]
  int n_states;
  int32_t states[LOSS_MAX_STATES];
  double* c;                       // [S][B]
  double* k;                       // [n_states][B] or nullptr (raising: the direct weights)
};
// ratio[i][j][b] = sign_ij sign_jj exp((log_ij - mean_i) - (log_jj - mean_j)); lg, sg, ratio: [S][S][B]
void launch_psi_ratio(hipStream_t st, const double* lg, const double* sg, int S, long B, double* ratio);
// per row of x[n_rows][B]: clip to centre +- clip_width x scale, mask = |x - centre| < exclude_width, row_stats[row][4]
void launch_clip_rows(hipStream_t st, const double* x, const double* w, int n_rows, long B, int center_kind, int scale_kind,
                      double clip_width, double exclude_width, double* x_clip, uint8_t* mask, double* row_stats);
void launch_loss_cotangents(hipStream_t st, const LossCotArgs& a);

// ---- kernels_observable.inl (included by kernels_ecp.hip): observables of the training loop (dqmc_oscillator_strength, dqmc_fd_displace, dqmc_fd_force) ----
// r: real[S][B][N][3], ratio: double[S][S][B], e_loc: real[S][B]; mom: double[2 S + 3 S^2] scratch = E mean, E std, cd std;
// os_mean, os_err: double[S][S]; cd_mean, cd_err: double[S][S][3].  Two launches.
template <typename real>
void launch_oscillator_strength(hipStream_t st, const real* r, const double* ratio, const real* e_loc, int S, long B, int N, double* mom,
                                double* os_mean, double* os_err, double* cd_mean, double* cd_err);
// r_out: real[3 n_nuc][B][N][3], R_out: real[3 n_nuc][n_nuc][3]: the displaced copies of the finite-difference force, one launch
template <typename real>
void launch_fd_displace(hipStream_t st, const real* r, const real* R, long B, int N, int n_nuc, double h, real* r_out, real* R_out);
// F: double[B][D] from log_d, e_d: real[D][B] and log_0, e_0: real[B]
template <typename real>
void launch_fd_force(hipStream_t st, const real* log_d, const real* log_0, const real* e_d, const real* e_0, long B, int D, double h,
                     double* F);

}  // namespace dqmc
