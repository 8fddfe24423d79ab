// op_view.h -- the slot layout of dqmc_op { kind, i[28], f[4] }, once: index constants per op kind (host and device code) and
// host views with named accessors.  The documentation of every slot is the comment of its op kind in include/dqmc.h; this
// header mirrors it and nothing else numbers the slots.  Views hold a reference and decode on access: constructing one costs
// nothing and allocates nothing.
#pragma once

#include "../../include/dqmc.h"

namespace dqmc {

constexpr int OP_N_SLOTS = 28, OP_N_FSLOTS = 4;      // lengths of dqmc_op::i and dqmc_op::f

enum FeatEnSlot { FEN_DST = 0, FEN_LOG_RESCALE = 1, FEN_USE_SPIN = 2 };
enum FeatEeSlot { FEE_DST = 0, FEE_TABLE = 1, FEE_N_ROWS = 2, FEE_LOG_RESCALE = 3 };
enum LinearSlot {
  LIN_N_PIECES = 0,
  LIN_PIECE0 = 1, LIN_PIECE_STRIDE = 4, LIN_MAX_PIECES = 4,      // piece p at [LIN_PIECE0 + LIN_PIECE_STRIDE * p + ...]:
  LIN_P_SRC = 0, LIN_P_R0 = 1, LIN_P_K = 2, LIN_P_BCAST = 3,
  LIN_DST = 17, LIN_DST_R0 = 18, LIN_DST_COL0 = 19, LIN_NROWS = 20, LIN_NOUT = 21, LIN_W = 22, LIN_BIAS = 23, LIN_ACT = 24,
  LIN_RES = 25, LIN_RES_R0 = 26, LIN_RES_NORM = 27
};
enum SpinMeanSlot { SPM_SRC = 0, SPM_DST = 1, SPM_N_UP = 2 };
enum ConvSlot { CNV_EDGE = 0, CNV_NODE = 1, CNV_DST = 2, CNV_DST_COL0 = 3, CNV_TABLE = 4, CNV_S = 5, CNV_WIDTH = 6 };
enum EdgeSumSlot { ESUM_DIVISOR = CNV_NODE };        // every other slot as CONV
enum RowSumSlot { RSUM_SRC = 0, RSUM_DST = 1 };
enum OrbitalsSlot { ORB_SRC = 0, ORB_DST = 1, ORB_PI_UP = 2, ORB_PI_DOWN = 3, ORB_ZETA_UP = 4, ORB_ZETA_DOWN = 5, ORB_N_ENV = 6 };
enum SlogdetSlot { SLD_SRC = 0 };
enum FinalSlot { FIN_JASTROW = 0, FIN_CONF_COEFF = 1, FIN_CUSP_KIND = 2, FIN_ALPHAS = 3 };
enum FinalFSlot { FIN_F_SAME_SCALE = 0, FIN_F_ANTI_SCALE = 1 };
enum AttentionSlot { ATT_Q = 0, ATT_K = 1, ATT_V = 2, ATT_DST = 3, ATT_HEADS = 4, ATT_HEAD_DIM = 5, ATT_N_CONST = 6, ATT_CONST_K = 7, ATT_CONST_V = 8 };
enum ConstSlot { CST_DST = 0, CST_TABLE = 1 };

static_assert(LIN_PIECE0 + LIN_PIECE_STRIDE * LIN_MAX_PIECES == LIN_DST && LIN_RES_NORM + 1 == OP_N_SLOTS, "LINEAR fills the op");
static_assert(sizeof(dqmc_op) == 4 * (1 + OP_N_SLOTS + OP_N_FSLOTS), "dqmc_op layout");

inline int pad4(int n) { return (n + 3) / 4 * 4; }

// ---- host views ----
struct OpView {
  const dqmc_op& op;
  explicit OpView(const dqmc_op& o) : op(o) {}
  int at(int slot) const { return op.i[slot]; }
};
struct FeatEnOp : OpView {
  using OpView::OpView;
  int dst() const { return at(FEN_DST); }
  int log_rescale() const { return at(FEN_LOG_RESCALE); }
  int use_spin() const { return at(FEN_USE_SPIN); }
};
struct FeatEeOp : OpView {
  using OpView::OpView;
  int dst() const { return at(FEE_DST); }
  int table() const { return at(FEE_TABLE); }         // (recv, send) pairs in the int table
  int n_rows() const { return at(FEE_N_ROWS); }
  int log_rescale() const { return at(FEE_LOG_RESCALE); }
};
struct LinearOp : OpView {
  using OpView::OpView;
  int n_pieces() const { return at(LIN_N_PIECES); }
  int src(int p) const { return at(LIN_PIECE0 + LIN_PIECE_STRIDE * p + LIN_P_SRC); }
  int r0(int p) const { return at(LIN_PIECE0 + LIN_PIECE_STRIDE * p + LIN_P_R0); }
  int K(int p) const { return at(LIN_PIECE0 + LIN_PIECE_STRIDE * p + LIN_P_K); }          // unpadded
  int bcast(int p) const { return at(LIN_PIECE0 + LIN_PIECE_STRIDE * p + LIN_P_BCAST); }
  int dst() const { return at(LIN_DST); }
  int dst_r0() const { return at(LIN_DST_R0); }
  int dst_col0() const { return at(LIN_DST_COL0); }
  int nrows() const { return at(LIN_NROWS); }
  int nout() const { return at(LIN_NOUT); }
  int w() const { return at(LIN_W); }
  int bias() const { return at(LIN_BIAS); }
  int act() const { return at(LIN_ACT); }
  int res() const { return at(LIN_RES); }
  int res_r0() const { return at(LIN_RES_R0); }
  bool res_norm() const { return at(LIN_RES_NORM) != 0; }
  bool has_bias() const { return bias() >= 0; }
  bool has_residual() const { return res() >= 0; }
  template <typename real> real res_scale() const { return res_norm() ? (real)0.70710678118654752440 : (real)1; }
  int ldw() const { return pad4(nout()); }                // row length of W and of the bias
  int w_rows() const { int n = 0; for (int p = 0; p < n_pieces(); ++p) n += pad4(K(p)); return n; }      // rows of W
  int k_total() const { int n = 0; for (int p = 0; p < n_pieces(); ++p) n += K(p); return n; }
  int n_bcast() const { int n = 0; for (int p = 0; p < n_pieces(); ++p) n += bcast(p) ? 1 : 0; return n; }
  double flops_per_walker() const { return 2.0 * nrows() * (double)k_total() * nout(); }                // value lane, unpadded
  long kfac_dim_a() const { return (long)w_rows() + (has_bias() ? 1 : 0); }     // sides of the KFAC factors A_l, G_l (dqmc_log_psi_kfac)
  long kfac_dim_g() const { return ldw(); }
};
struct SpinMeanOp : OpView {
  using OpView::OpView;
  int src() const { return at(SPM_SRC); }
  int dst() const { return at(SPM_DST); }
  int n_up() const { return at(SPM_N_UP); }
};
struct EdgeOp : OpView {                // what CONV and EDGE_SUM share
  using OpView::OpView;
  int edge() const { return at(CNV_EDGE); }
  int dst() const { return at(CNV_DST); }
  int dst_col0() const { return at(CNV_DST_COL0); }
  int table() const { return at(CNV_TABLE); }         // int [N][S][2]: (edge row, sender)
  int S() const { return at(CNV_S); }
  int width() const { return at(CNV_WIDTH); }
};
struct ConvOp : EdgeOp {
  using EdgeOp::EdgeOp;
  int node() const { return at(CNV_NODE); }
};
struct EdgeSumOp : EdgeOp {
  using EdgeOp::EdgeOp;
  int divisor() const { return at(ESUM_DIVISOR); }
  double scale() const { return 1.0 / (double)(divisor() > 0 ? divisor() : 1); }
};
struct RowSumOp : OpView {
  using OpView::OpView;
  int src() const { return at(RSUM_SRC); }
  int dst() const { return at(RSUM_DST); }
};
struct OrbitalsOp : OpView {
  using OpView::OpView;
  int src() const { return at(ORB_SRC); }             // backflow buffer
  int dst() const { return at(ORB_DST); }
  int w(int t) const { return at(ORB_PI_UP + t); }    // weight offsets of pi_up, pi_down, zetas_up, zetas_down (t < 4)
  int n_env_slot() const { return at(ORB_N_ENV); }
  int n_env() const { return n_env_slot() > 0 ? n_env_slot() : 1; }
};
struct SlogdetOp : OpView {
  using OpView::OpView;
  int src() const { return at(SLD_SRC); }
};
struct FinalOp : OpView {
  using OpView::OpView;
  int jastrow() const { return at(FIN_JASTROW); }
  bool has_jastrow() const { return jastrow() >= 0; }
  int conf_coeff() const { return at(FIN_CONF_COEFF); }
  bool has_conf_coeff() const { return conf_coeff() >= 0; }
  int cusp_kind() const { return at(FIN_CUSP_KIND); }
  int alphas() const { return at(FIN_ALPHAS); }
  float same_scale() const { return op.f[FIN_F_SAME_SCALE]; }
  float anti_scale() const { return op.f[FIN_F_ANTI_SCALE]; }
};
struct AttentionOp : OpView {
  using OpView::OpView;
  int buf(int q) const { return at(ATT_Q + q); }      // q, k, v, dst (q < 4)
  int q() const { return at(ATT_Q); }
  int k() const { return at(ATT_K); }
  int v() const { return at(ATT_V); }
  int dst() const { return at(ATT_DST); }
  int heads() const { return at(ATT_HEADS); }
  int head_dim() const { return at(ATT_HEAD_DIM); }
  int n_const() const { return at(ATT_N_CONST); }
  int const_k() const { return at(ATT_CONST_K); }
  int const_v() const { return at(ATT_CONST_V); }
};
struct ConstOp : OpView {
  using OpView::OpView;
  int dst() const { return at(CST_DST); }
  int table() const { return at(CST_TABLE); }         // real[rows][width] in the weight buffer
};

// Every view of one op side by side, for code that switches on op.kind: `const OpViews v(op);` once, then
// `case DQMC_OP_CONV: ... v.conv.edge()`.  Only the view of the op's own kind means anything.
struct OpViews {
  FeatEnOp feat_en; FeatEeOp feat_ee; LinearOp lin; SpinMeanOp spin_mean; ConvOp conv; EdgeSumOp edge_sum; RowSumOp row_sum;
  OrbitalsOp orb; SlogdetOp slogdet; FinalOp fin; AttentionOp att; ConstOp cst;
  explicit OpViews(const dqmc_op& o)
      : feat_en(o), feat_ee(o), lin(o), spin_mean(o), conv(o), edge_sum(o), row_sum(o), orb(o), slogdet(o), fin(o), att(o), cst(o) {}
};

}  // namespace dqmc
