// engine.hip -- the C ABI of include/dqmc.h: context, layer-program executor, MCMC driver,
// per-kernel timing.  Host code only; every arithmetic step is one of the kernels in
// kernel_linear.hip / kernels_graph.hip / kernels_head.hip / kernels_mcmc.hip.
// This file: DevBuf, the one type that owns device memory here (every allocation of a context is a DevBuf member and is
// released by it), Slab, the one way a scratch DevBuf<char> is carved into aligned typed slices, PassOpts, what a pass is asked
// to do beyond its outputs, the context base, the state of Engine<real> (members, options' storage, captured-graph bookkeeping),
// and the extern "C" entry points.  The member functions live in engine_*.inl by concern -- program analyses
// (engine_program.inl), planner of the LDS-resident kernel (engine_fused_plan.inl), pass runner (engine_pass.inl),
// float64 refinement (engine_refine.inl; its host-only policy -- threshold calibration, direct-mode hysteresis -- in
// refine_policy.h), ECP / pseudo-Hamiltonian (engine_ecp.inl), samplers (engine_mcmc.inl), the reverse
// pass (engine_grad.inl, engine_reverse.inl) and the plans and entry points of its modes (engine_jac.inl, engine_kfac.inl;
// engine_coords.inl, with the force estimators; engine_ecp_force.inl, the ECP force), SCF-orbital pretraining (engine_pretrain.inl), the device-resident optimiser
// step (engine_optim.inl), the KFAC preconditioner on its vectors (engine_kfacopt.inl), the loss assembly (engine_loss.inl),
// the observables of the training loop (engine_observable.inl) -- and
// are included inside the struct body: one translation unit, as before.  The slot layout of dqmc_op lives in op_view.h: all of
// the above read an op through its named views, never by slot number.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <algorithm>
#include <vector>

#include "../../include/dqmc.h"
#include "kernels.h"
#include "op_view.h"
#include "refine_policy.h"
#include "spec_device.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                                                   \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess)                                                                               \
      return fail(DQMC_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_) + " (" + __FILE__ +   \
                                  ":" + std::to_string(__LINE__) + ")");                                \
  } while (0)

using dqmc::pad4;

struct TimingRec {
  double ms = 0;
  int64_t launches = 0;
  double flops = 0;       // algorithmic: the dense-T count of SURVEY.md section 8d (what `roofline.achieved` is priced with)
  double executed = 0;    // what the launches actually multiply: 8 compact lanes on edge rows, per-walker pieces once per walker,
                          // lanes padded to TP, widths padded to 4 (matrix-pipe utilisation = this / time / peak)
};

// One device allocation and its capacity in elements, released with its owner.  Converts to T*, so argument structs, launches
// and pointer arithmetic read as with a raw pointer, and `if (!buf)` asks whether it holds anything.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { reset(); }
  operator T*() const { return p; }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
  }
  hipError_t alloc(size_t n) {      // into the empty buffer; p and cap change on success only
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, sizeof(T) * n);
    if (e == hipSuccess) { p = static_cast<T*>(q); cap = n; }
    return e;
  }
  // exactly n elements in a fresh block (a table that a setup call replaces; the caller has synchronised what may read the old one)
  int assign(size_t n) {
    reset();
    HIP_TRY(alloc(n));
    return DQMC_OK;
  }
  int upload(const T* host, size_t n) {      // assign + blocking copy
    const int rc = assign(n);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(p, host, sizeof(T) * n, hipMemcpyHostToDevice));
    return DQMC_OK;
  }
  // at least n elements, grow-only and exact: a call that fits performs no allocation and keeps the pointer; one that does not
  // drains `st` (a kernel in flight may read the old block), and a failed growth leaves (nullptr, 0), never a stale capacity.
  // With `what` the failure is DQMC_E_NOMEM "<what> of <bytes> bytes: ...", without it the DQMC_E_HIP of HIP_TRY.
  int reserve(size_t n, hipStream_t st, const char* what = nullptr) {
    if (n <= cap) return DQMC_OK;
    if (p) { HIP_TRY(hipStreamSynchronize(st)); reset(); }
    if (!what) HIP_TRY(alloc(n));
    else if (const hipError_t e = alloc(n); e != hipSuccess)
      return fail(DQMC_E_NOMEM, std::string(what) + " of " + std::to_string(sizeof(T) * n) + " bytes: " + hipGetErrorString(e));
    return DQMC_OK;
  }
};

// The layout of one scratch slab (a DevBuf<char>): take<T>(n) the slices in order -- each starts 256-byte aligned --, reserve
// `bytes` once, then slice.in(slab) is the slice's typed pointer.
struct Slab {
  template <typename T> struct Slice {
    size_t off;
    T* in(char* slab) const { return reinterpret_cast<T*>(slab + off); }
  };
  size_t bytes = 0;
  size_t take_bytes(size_t n) { const size_t o = bytes; bytes += (n + 255) / 256 * 256; return o; }
  template <typename T> Slice<T> take(size_t n) { return {take_bytes(sizeof(T) * n)}; }
};

// What a forward-Laplacian pass is asked to do beyond its outputs (lap_refined -> pass_own -> run -> run_graphed / run_chunk,
// local_energy_ecp).  The default is the plain pass of a caller that knows nothing of the refinement.
struct PassOpts {
  bool flag = false;         // k_final scores every walker and lists those above refine_thresh in d_flag (part of a captured graph's key)
  bool skip_ph = false;      // a float64 twin serving a plain-gradient call (psi_grad / Langevin): no pseudo-Hamiltonian seeding
  bool skip_nl = false;      // ... and no non-local ECP quadrature; also a call whose quadrature follows in ecp_mixed
  const int32_t* walker_idx = nullptr;   // twin serving a float32 context: global walker index per walker (EcpArgs::walker_idx)
  bool phi_f32 = false;      // ... whose rotation angles (ecp_phi) are float32
};

}  // namespace

struct dqmc_ctx {
  virtual ~dqmc_ctx() = default;
  virtual int set_weights(const double* w, size_t n) = 0;
  virtual int wf_eval(const void* r, const void* R, int B, void* logpsi, int32_t* sign) = 0;
  virtual int local_energy(const void* r, const void* R, int B, void* e_loc, void* stats, void* grad, void* logpsi,
                           int32_t* sign) = 0;
  virtual int psi_grad(const void* r, const void* R, int B, void* logpsi, int32_t* sign, void* grad) = 0;
  virtual int log_psi_vjp(const void* r, const void* R, int B, const void* cot, double* grad, void* logpsi, int32_t* sign) = 0;
  virtual int log_psi_jacobian(const void* r, const void* R, int B, void* jac, size_t ld_jac, void* logpsi, int32_t* sign) = 0;
  virtual int kfac_layout(int* n_linear, size_t* n_factor_doubles, size_t* n_rest) = 0;
  virtual int log_psi_grad_coords(const void* r, const void* R, int B, void* grad_r, void* grad_R, void* logpsi, int32_t* sign) = 0;
  virtual int hf_force(int est, const void* r, const void* R, int B, const void* grad_r, const void* grad_R, const void* e_loc,
                       double energy, double* force) = 0;
  virtual int ecp_force(int est, int all_rows, const void* r, const void* R, int B, const void* e_loc, double energy, double* force,
                        double* parts) = 0;
  virtual int log_psi_kfac(const void* r, const void* R, int B, const void* cot, double* grad, double* factors, void* rest,
                           void* logpsi, int32_t* sign) = 0;
  virtual int set_pretrain_target(int n_shells, const int32_t* atom, const int32_t* l, const int32_t* n_prim, const double* coeffs,
                                  const double* zetas, int n_ao, int n_mo, const double* mo_coeffs, int n_conf, const int32_t* confs,
                                  const double* conf_coeffs) = 0;
  virtual int pretrain_target(const void* r, const void* R, int B, void* target) = 0;
  virtual int orbitals(const void* r, const void* R, int B, void* orb) = 0;
  virtual int orbitals_vjp(const void* r, const void* R, int B, const void* cot, double* grad, void* orb) = 0;
  virtual int pretrain_loss_grad(const void* r, const void* R, int B, double n_total, double* grad, double* per_sample_loss) = 0;
  virtual int set_param_map(const int32_t* src, size_t n, size_t n_params) = 0;
  virtual int set_nuclear_stream(const dqmc_nuc_stream* d) = 0;
  virtual int weights_from_params(const double* theta) = 0;
  virtual int load_weights_device(const double* w64) = 0;
  virtual int grad_to_params(const double* grad_w, double* grad_theta) = 0;
  virtual int jacobian_to_params(const void* jac, size_t ld_jac, int B, const void* logpsi, const int32_t* sign, void* jac_theta,
                                 size_t ld_theta) = 0;
  virtual int adam_step(double* theta, double* mu, double* nu, const double* g, size_t n, double lr, double b1, double b2, double eps,
                        int64_t t, double* norms3) = 0;
  virtual int apply_update(double* theta, const double* delta, double scale, double* norms3) = 0;
  virtual int set_kfac_map(const dqmc_kfac_map* m) = 0;
  virtual int kfac_state_size(size_t* n_doubles) = 0;
  virtual int kfac_direction(const double* g, const double* factors, const void* rest, const void* logpsi, const int32_t* sign, int B,
                             double* state, int first, double ema, double damping, double* delta, double* dot) = 0;
  virtual int kfac_apply(double* theta, const double* delta, const double* dot, double lr, double norm_constraint, double* norms4) = 0;
  virtual int debug_read_weights(int which, void* out, size_t bytes) = 0;
  virtual int debug_nuc_dx_time(int B, int reps, double* ms2, int* shape3) = 0;
  virtual void graph_counters(int64_t* out2) = 0;
  virtual int psi_ratio(const double* lg, const double* sg, int S, long B, double* ratio) = 0;
  virtual int clip_rows(const double* x, const double* w, int n_rows, long B, int center, int scale, double clip_width,
                        double exclude_width, double* x_clip, uint8_t* mask, double* row_stats) = 0;
  virtual int loss_cotangents(const dqmc_loss_terms* t, double* c, double* k) = 0;
  virtual int oscillator_strength(const void* r, const double* ratio, const void* e_loc, int S, long B, double* os_mean, double* os_err,
                                  double* cd_mean, double* cd_err) = 0;
  virtual int fd_displace(const void* r, const void* R, long B, double h, void* r_out, void* R_out) = 0;
  virtual int fd_force(const void* log_d, const void* log_0, const void* e_d, const void* e_0, long B, double h, double* F) = 0;
  virtual int mcmc(void* r, void* logpsi, int32_t* sign, int32_t* age, void* tau, const void* R, int B, int n_sub,
                   int max_age, double target, uint64_t seed, const void* noise, const void* unif, uint8_t* accept_out,
                   double* stats7) = 0;
  virtual int langevin_update(const void* r, const void* R, const double* mol_charges, int B, const void* tau, void* logpsi,
                              int32_t* sign, void* force) = 0;
  virtual int langevin(void* r, void* logpsi, int32_t* sign, int32_t* age, void* force, void* tau, const void* R,
                       const double* mol_charges, int B, int n_sub, int max_age, double target, uint64_t seed, const void* noise,
                       const void* unif, uint8_t* accept_out, double* stats7) = 0;
  virtual int exchange(void* r, void* logpsi, int32_t* sign, int32_t* age, const void* tau, const void* R, int B,
                       const int32_t* up_idx, const int32_t* down_idx, const void* unif, uint8_t* accept_out, double* stats7) = 0;
  virtual int set_ecp(int n_t_loc, const double* loc, int n_l, int n_t_nl, const double* nl) = 0;
  virtual int ecp_rotation(uint64_t seed, const void* phi) = 0;
  virtual int set_ph(int n_grid, double r_max, const double* rv_loc, const double* rv_l2, const int32_t* mask) = 0;
  virtual int energy_stats(const void* e, const void* w, int B, double* out7) = 0;
  virtual int energy_stats_dev(const void* e, const void* w, int B, double** rec_dev) = 0;
  virtual int debug_read(int buf, double* out, size_t n) = 0;
  virtual int option(const char* name, int value) = 0;
  virtual int refine_scores(double* out, int n) { (void)out; (void)n; return DQMC_E_UNSUPPORTED; }
  virtual int substep_kernel(char* name_out, size_t n) { (void)n; name_out[0] = 0; return 0; }
  int64_t refine_counters[4] = {0, 0, 0, 0};   // local-energy / psi_grad calls; of them whole-batch float64; probe calls; walkers refined (sum)
  virtual dqmc_ctx* twin_ctx() { return nullptr; }
                                                         // (the float64 refinement twin of a float32 context, once it exists)
  int last_TP = 0;
  int last_refined = 0;     // walkers re-evaluated in float64 by the last local-energy / psi_grad call
  double refine_info[4] = {0, 0, 0, 0};   // {mode, score threshold, measured error per unit of score, direct float64 calls left}
  int64_t ecp_last_counts[3] = {0, 0, 0};   // (nucleus, electron) pairs of the last mixed-precision quadrature: float32, float64, dropped
  int last_chunks[2] = {0, 0};   // walker chunks of the last Laplacian-mode evaluation: this context's own pass, its float64 twin's (max over its passes)
  int device = 0;           // every entry point makes this the calling thread's current device
  DevBuf<double> d_gather;      // all-gathered energy records (dqmc_energy_stats_allgather)
  // timing
  bool timing = false;
  std::map<std::string, TimingRec> trec;
  struct Pending { std::string name; hipEvent_t a, b; double flops, executed; };
  std::vector<Pending> pending;
  std::vector<hipEvent_t> ev_pool;
  hipStream_t st = nullptr;

  hipEvent_t get_event() {
    if (!ev_pool.empty()) { hipEvent_t e = ev_pool.back(); ev_pool.pop_back(); return e; }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
  }
  hipStream_t t_stream = nullptr;      // stream of the launch being timed (the context's, or its edge-stream companion)
  void t_begin(const char* name, double flops, hipStream_t s = nullptr, double executed = -1.0) {
    if (!timing) return;
    t_stream = s ? s : st;
    Pending p{name, get_event(), get_event(), flops, executed < 0 ? flops : executed};
    (void)hipEventRecord(p.a, t_stream);
    pending.push_back(p);
  }
  void t_end() {
    if (!timing) return;
    (void)hipEventRecord(pending.back().b, t_stream);
  }
  void t_collect() {
    if (pending.empty()) return;
    (void)hipStreamSynchronize(st);
    for (auto& p : pending) {
      float ms = 0;
      (void)hipEventElapsedTime(&ms, p.a, p.b);
      auto& r = trec[p.name];
      r.ms += ms; r.launches += 1; r.flops += p.flops; r.executed += p.executed;
      ev_pool.push_back(p.a); ev_pool.push_back(p.b);
    }
    pending.clear();
  }
};

namespace {

template <typename real>
struct Engine : dqmc_ctx {
  dqmc_system sys{};
  int N = 0;
  std::vector<dqmc_buf> bufs;
  std::vector<dqmc_op> ops;
  std::vector<double> charges_h;
  size_t n_weights = 0, n_itable = 0;
  std::vector<int32_t> h_itable;
  DevBuf<real> d_w;
  DevBuf<int32_t> d_it;
  DevBuf<double> d_charges;
  // workspace
  DevBuf<char> d_ws;
  std::vector<size_t> buf_off;  // byte offsets for the current (B, TP)
  size_t off_logdet = 0, off_signk = 0, off_z = 0, off_cond = 0, off_kappa = 0;
  int split_bcast = 1;           // option "split_bcast": per-walker pieces of a linear layer multiplied once per walker
  int last_B = 0;
  // mcmc scratch
  DevBuf<char> d_mc;
  DevBuf<int32_t> d_nacc;
  DevBuf<double> d_tau_ring;    // holds real[2]: step sizes of the last two one-launch sub-steps
  DevBuf<double> d_acc;        // [1] acceptance, then [7] stats, then [7] energy record
  std::vector<real> wtmp;
  // fused value-only plan
  int fused_enabled = 1;      // 0 off, 1 where it is the faster value path (fused_pays), 2 always
  int fused_n_ops = 0, fused_wt_req = 0, fused_dbg = 0, fused_sched_mode = 3, fused_occ_req = 0;
  std::vector<int> f_order, f_level;   // fused schedule: op index and dependency level per slot
  DevBuf<dqmc_op> d_ops;
  DevBuf<int32_t> d_wpk_off;      // per scheduled op: {packed-weight offset, barrier-after flag}
  DevBuf<real> d_wpk;            // cap counts reals
  DevBuf<long long> d_prof;
  // pair-compact edge buffers (common.h: PAIR_LANES): which buffers carry 8 lanes in Laplacian mode, and the
  // (receiver, sender) of each of their rows (for the lane maps of debug_read)
  size_t ws_budget = (size_t)32 << 30;   // activation workspace per evaluation chunk (option "ws_budget_mb"); several contexts
                                         // (electronic states, float64 twins) share the 288 GB of one GPU
  bool lane_compact = true;
  int attention_mfma = 1;      // 1: where profitable (N > 16), 2: wherever supported, 0: never
  int attention_ncb = -1;      // 1: kernel instance for the exact number of key tiles, 0: the four-tile instance, -1: exact in float32 only (measured)
  int attention_split = -1;    // float64 contexts: eight-wave variant (a pair of waves per query row block) for Laplacian passes (1 / -1), 0: never
  int slogdet_mfma = 1;        // 1: where profitable (N > 16), 2: from N > 8 on, 0: never
  int attention_reverse = 0;   // 1: the reverse pass runs through ATTENTION ops (engine_grad.inl: attention_refused), 0: it refuses them
  std::vector<char> compact;
  std::vector<int> pad_end;    // per op: the CONV / EDGE_SUM op that also zeroes its destination's columns up to pad_end (0: none)
  // two-layer row-wise MLPs run as ONE launch (kernel_linear.hip: CHAIN): mlp_child[k] = op index of the second layer
  // of the LINEAR op k, or -1; mlp_skip[k]: op k is such a second layer (executed with its parent)
  std::vector<int> mlp_child;
  std::vector<char> mlp_skip;
  int mlp_fuse = 1;
  int linear_bf = dqmc::LINEAR_BF_DEFAULT, linear_bkx = dqmc::LINEAR_BKX_DEFAULT, linear_f64_split = 1;   // LinArgs::cfg_*
  std::vector<std::vector<int>> pair_rs;   // per compact buffer: [2*row] = recv, [2*row+1] = send
  // descriptor-driven fused kernel (kernel_fused2.hip): the default when its plan exists
  int fused2_WT = 0, fused2_shift = 0, fused_sched_wt = 4, fused_substep = 1;
  size_t fused_sched_budget = 36 * 1024;   // bytes live per level the list scheduler (mode 3) aims for
  size_t fused2_lds_quarter = 160 * 1024 / 4;   // LDS per workgroup for 4 (option "fused_wg_per_cu": 5) workgroups per CU
  size_t fused2_lds = 0, fused2_lds_budget = 80 * 1024;
  std::vector<dqmc::FusedBuf> fbufs2_h;
  bool fused2_ma1 = false;       // every unit of the plan has ma == 1
  bool fbufs2_uploaded = false;
  // Laplacian pass on two HIP streams: the two-particle (edge) stream does not depend on the node stream (reference
  // gnn/electron_gnn.py:160-276: edges are updated from edges), its launches are HBM bound while the node layers are
  // MFMA bound, so they run on a companion stream and the node stream waits (event) only where a convolution or an
  // edge sum consumes an edge buffer.  Option "dual_stream" (1).
  int dual_stream = 1;
  // Laplacian pass of the small systems: its ~40 kernels are latency bound one by one (2-3 TB/s, 40 % of the MFMA peak at
  // best), and a layer's node-MLP + convolution of one edge type, that of the other, and the spin means + their product
  // are three INDEPENDENT branches that meet in the g layer.  Option "multi_stream" (1): those branches run on up to two
  // more HIP streams (op_sid, analyse_streams), ordered by events per produced buffer.
  int multi_stream = 1;
  std::vector<int> op_sid;             // stream slot per op: 0 main, 1 edge stream, 2 / 3 node branches
  hipStream_t st_extra[2] = {nullptr, nullptr};
  std::vector<hipEvent_t> ms_events;   // event pool of one pass
  hipStream_t st2 = nullptr;
  std::vector<hipEvent_t> buf_ev;      // per buffer: last write on the companion stream (nullptr: none pending)
  hipEvent_t ev_fork = nullptr;
  int fused_stagger_div = 256;   // workgroups per dispatch wave (= CUs): workgroup b is the (b / 256)-th placed on its CU
  int fused_prio = 1;            // option "fused_prio": issue priority rotates among the tiles that share a CU (1: per level, 2: per unit, 0: off)
  int fused_lean = 1;            // option "fused_lean": lean unit body for small layers
  int fused_bf = 1;              // option "fused_bf": float32 layers of the value path on the bf16 matrix pipe (three-piece split, six products; float engines only)
  std::vector<char> op_bf;       // per scheduled op: packed in the bf16 plane layout
  std::vector<std::vector<dqmc::FDesc>> plan_lists;   // the four wave lists (kept for "fused_print")
  // plan-specialised sub-step kernel (csrc/gen/*.hip, spec_device.h): found by the hash of the program; its weight tape
  const dqmc::SpecKernel* spec_k = nullptr;
  DevBuf<uint32_t> d_tape;
  int fused_spec = 1;            // option "fused_spec": 0 = always the descriptor-driven kernel
  DevBuf<dqmc::FDesc> d_descs;
  DevBuf<int32_t> d_wave_begin;
  DevBuf<dqmc::FusedBuf> d_fbufs2;
  // effective core potential (dqmc_set_ecp): local terms for k_final, non-local channels per nucleus
  DevBuf<double> d_ecp_loc, d_ecp_nl;
  DevBuf<int32_t> d_ecp_nuc;
  int ecp_nt_loc = 0, ecp_n_nl = 0, ecp_L = 0, ecp_nt_nl = 0;
  uint64_t ecp_seed = 0;
  const void* ecp_phi = nullptr;
  std::vector<double> ecp_nl_h;       // host copy of the non-local tables for the float64 twin
  int ecp_nl_L_h = 0, ecp_nl_nt_h = 0;
  DevBuf<char> d_ecp;           // quadrature walkers + their psi + psi of the walkers themselves
  // mixed-precision quadrature of a float32 context (ecp_mixed): "ecp_mixed" 1 (default) with "refine" 1; a triple whose
  // weight w = max_l (2l+1)|V_l| exceeds ecp_w_heavy ("ecp_heavy_e6", in 1e-6 Ha) gets float64 psi ratios, one below
  // ecp_w_skip ("ecp_skip_e12", in 1e-12 Ha) is dropped
  int ecp_mixed_on = 1;
  double ecp_w_heavy = 1e-2, ecp_w_skip = 1e-10;
  // float32 error of log|psi(r)| up to which a walker counts as ordinary ("ecp_dlog_floor_e6", in 1e-6; 0: weights alone
  // decide, the round-4 rule): beyond it the walker's float64 bound tightens in proportion (kernels.h: EcpMixArgs::l32).
  // 3e-5 = half the median float32 error of log|psi| of these networks (6e-5).  Sweep on the MI355X (tools/ecp_sweep_b.py,
  // profiles/r05_ecp_threshold_sweep.txt), largest E_loc error of 256 set-B / 32 set-A walkers and time per call:
  // weights alone 1.2e-5 (one walker beyond the tolerance) / 1.7e-6; floor 1e-4: 9.8e-6 / 1.7e-6 at + 0.6 %; floor 3e-5:
  // 3.5e-6 / 5.9e-7 at + 3 % -- the same as tightening "ecp_heavy_e6" to 3e-3 at + 6 %.
  double ecp_dlog_floor = 3e-5;
  DevBuf<char> d_ecpm;
  size_t ecp_max_cfg = 1 << 16; // quadrature walkers per value-mode batch
  // float64 refinement (float32 build): walkers flagged by k_final as ill conditioned (near a node of psi the kinetic
  // energy is a difference of huge numbers and float32 round-off is amplified by the CI cancellation) are
  // re-evaluated by a float64 twin of this context and their results replace the float32 ones
  int refine = 1;
  // Flag rule: score > refine_thresh (kernels.h: FinalArgs).  The threshold is SELF-CALIBRATED: every refine_probe-th
  // local-energy call (and the first) a strided sample of <= refine_sample (256) walkers is evaluated by the float64 twin
  // as well.  What the MI355X shows (round 5: 82 k evaluations each along the bench trajectories of LiH / PauliNet and
  // N2 / FermiNet, 5 k of benzene / Psiformer; tools/calib_data.py, profiles/r05_calibration_model.txt): the float32 error
  // of a walker is  err = m x score x xi  with xi EXPONENTIALLY distributed -- every quantile of err / score is the same in
  // every score bin (p50 : p90 : p99 : p99.9 = ln 2 : ln 10 : ln 100 : ln 1000), m = 1.3e-8 (LiH), 0.8e-8 (N2, benzene),
  // 5.6e-8 (LiH / Psiformer).  A walker kept in float32 at score s therefore misses the tolerance with probability
  // exp(-tol / (m s)), and a score threshold can promise a RATE of misses, not their absence.  The probe measures m on
  // its sample (robustly: the larger of median / ln 2 and 90th percentile / ln 10) and sets the largest threshold for
  // which the expected share of kept walkers beyond refine_target (the tolerance, 1e-5) -- the mean of
  // exp(-tol / (m s_i)) over the kept walkers of the probed batch -- stays below refine_miss (1e-8).  (1e-7 until the linear kernels got their fresh
  // per-chunk accumulators, kernel_linear.hip: the typical error fell to 0.65-0.70 of what it was, the rare outliers whose error is
  // made elsewhere did not, and relative to the smaller m they reach further: 3 of 19 k N2 walkers at scores 100-400 beyond
  // 10 m s where the old kernels had none -- one of them at 1.008e-5 under the threshold of the 1e-7 rule.  1e-8 keeps the
  // largest float32 error of both 82 k-evaluation trajectories at 5e-6.)  Rounds 3-4 used threshold = 7e-6 / (90th percentile of err / score): along the same
  // trajectories that left 27-32 of 82 k evaluations beyond 1e-5 (max 2.2e-5).  Deep / ill-conditioned systems
  // (Psiformer, a random-init TransPsiformer) end up with most walkers above the threshold and fall into the direct
  // float64 pass by themselves.  refine_probe = 0 freezes the threshold at the option's value.
  double refine_thresh = 200.0;
  double refine_target = 1e-5;      // "refine_target_e7" (100): the relative tolerance the kept walkers are to meet
  double refine_miss = 1e-8;        // "refine_miss_e9" (10): accepted share of kept walkers beyond it
  int refine_probe = 32;
  int refine_sample = 256;       // walkers of the calibration sample (option "refine_sample"; 64 until round 4 -- six seeds on benzene
                                 // then drew thresholds that flagged 36-50 % of the batch)
  dqmc::DirectMode direct;       // whole-batch float64 ("direct") mode: lines, stay, back-off and their state (refine_policy.h)

  int twin_full_budget = 1;      // the twin's activation workspace may be as large as this context's (option "twin_full_budget")
  // option "pass_graph" (1): a forward-Laplacian pass that fits one workspace chunk is captured ONCE per (buffers, batch
  // size) into a hipGraph -- its ~40 launches, and the event records / waits that spread them over four streams -- and
  // replayed with one hipGraphLaunch per call.  The pass is launch-bound at the batch sizes it is used for (LiH, 4096
  // walkers: 140 us of a 1.7 ms float32 pass are gaps between kernels, 206 of the 690 us of the float64 twin's pass over
  // ~190 walkers: profiles/r03_eloc_pass_timeline.txt).  The first pass at a batch size runs eagerly (workspace, streams,
  // events, kernel attributes get created), the second one is captured on a stream of the context's own (the caller's
  // may be the legacy default stream, which cannot be captured) fenced by two events.  Everything a kernel of the pass
  // receives by value is a function of the key; what is not (the score threshold) is read from device memory.
  int pass_graph = 1;
  bool graph_broken = false;
  hipStream_t st_g = nullptr;
  hipEvent_t ev_g0 = nullptr, ev_g1 = nullptr;
  struct PassGraph { const void* p[7]; int B; bool flag; const void* ws; const void* flagp; uint64_t epoch, used; void* exec; };
  std::vector<PassGraph> pgraphs;
  uint64_t graph_epoch = 0, graph_clock = 0, graph_captures = 0, graph_hits = 0;
  std::vector<int> graph_warm;          // batch sizes that have run eagerly
  DevBuf<double> d_thresh;              // device copy of refine_thresh (read by k_final: graphs must not bake it in)
  double thresh_uploaded = -1.0;
  bool graphs_active() const {
    return pass_graph && !graph_broken && !timing && !fused_dbg && ph_n == 0 && ecp_n_nl == 0;
  }
  // ... and only passes that are launch-bound: up to 2 GiB of activations per pass (LiH / PauliNet: 4096 walkers in
  // float32, the twin's few hundred in float64).  The passes of the larger systems run for milliseconds per kernel: a
  // replay gains nothing there, and rounding the twin's batch up would cost real work (benzene, 87 flagged walkers -> 128:
  // 266 -> 338 ms per step when it was tried)
  bool graph_fits(int B) const {
    const int TP = (3 * N + 2 + 15) / 16 * 16;
    // (batches below 64 walkers -- the twin's are multiples of 64 -- stay eager: probes, test and debugging calls; a capture
    // costs milliseconds and such calls rarely repeat)
    return graphs_active() && B >= 64 && (double)ws_bytes_per_walker(TP) * (double)B <= 2147483648.0;
  }
  void drop_graphs() {
    if (st_g && !pgraphs.empty()) (void)hipStreamSynchronize(st_g);      // (a replay may still be running)
    for (auto& g : pgraphs) if (g.exec) (void)hipGraphExecDestroy((hipGraphExec_t)g.exec);
    pgraphs.clear();
  }
  int calls_since_probe = -1;    // -1: never probed
  double probe_c = 0.0;          // last measured scale m of the float32 error per unit of score (0: none yet)
  std::vector<std::pair<std::string, int>> twin_opts;
  std::vector<double> w64_h, ecp_loc_h;
  int ecp_loc_nt_h = 0;
  // pseudo-Hamiltonian (dqmc_set_pseudo_hamiltonian): radial tables of the PH nuclei, compacted
  DevBuf<double> d_ph_loc, d_ph_l2;
  DevBuf<int32_t> d_ph_nuc;
  int ph_n = 0, ph_grid = 0;
  double ph_rmax = 0.0;
  size_t off_phq = 0;
  std::vector<double> ph_loc_h, ph_l2_h;      // host copies for the float64 twin
  std::vector<int32_t> ph_mask_h;
  Engine<double>* twin = nullptr;
  dqmc_ctx* twin_ctx() override { return twin; }
  int no_twin = 0;        // option "no_twin" 1: this float32 context never creates its float64 twin -- ensure_twin answers like a program
                          // without a float64 kernel set (DQMC_E_UNSUPPORTED): plain float32 everywhere (refinement off by itself,
                          // float32 ECP quadrature)
  DevBuf<int32_t> d_flag;        // [0] = count, [1..] = walker indices
  DevBuf<double> d_score;        // [B] error predictor of the last flagged pass
  DevBuf<char> d_ref;

  ~Engine() override {      // what is not memory, before the members release theirs
    delete twin;
    drop_graphs();
    if (st_g) (void)hipStreamDestroy(st_g);
    if (ev_g0) (void)hipEventDestroy(ev_g0);
    if (ev_g1) (void)hipEventDestroy(ev_g1);
    if (st2) (void)hipStreamDestroy(st2);
    for (auto x : st_extra) if (x) (void)hipStreamDestroy(x);
    for (auto e : ms_events) if (e) (void)hipEventDestroy(e);
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    for (auto e : buf_ev) if (e) (void)hipEventDestroy(e);
    for (auto e : ev_pool) (void)hipEventDestroy(e);
  }

  int init(const dqmc_system* s, const double* charges, const dqmc_buf* b, int nb, const dqmc_op* o, int no,
           const double* w, size_t nw, const int32_t* it, size_t nit) {
    sys = *s;
    N = sys.n_up + sys.n_down;
    if (N < 1 || sys.n_nuc < 1 || sys.n_det < 1) return fail(DQMC_E_ARG, "bad system sizes");
    bufs.assign(b, b + nb);
    ops.assign(o, o + no);
    charges_h.assign(charges, charges + sys.n_nuc);
    for (auto& bb : bufs)
      if (bb.rows < 1 || bb.width < 4 || bb.width % 4) return fail(DQMC_E_ARG, "buffer width must be a positive multiple of 4");
    n_weights = nw; n_itable = nit;
    int rc;
    if ((rc = d_w.assign(nw ? nw : 1)) || (rc = d_it.assign(nit ? nit : 1)) || (rc = d_charges.assign(sys.n_nuc)) ||
        (rc = d_nacc.assign(4)) || (rc = d_tau_ring.assign(2)) || (rc = d_acc.assign(16)))
      return rc;
    HIP_TRY(hipMemsetAsync(d_nacc, 0, sizeof(int32_t) * 4, st));
    HIP_TRY(hipMemcpyAsync(d_charges, charges, sizeof(double) * sys.n_nuc, hipMemcpyHostToDevice, st));
    if (nit) HIP_TRY(hipMemcpyAsync(d_it, it, sizeof(int32_t) * nit, hipMemcpyHostToDevice, st));
    h_itable.assign(it, it + nit);
    HIP_TRY(hipStreamSynchronize(st));
    rc = validate();
    if (rc) return rc;
    // the determinant kernels of 45 .. 64 electrons use more LDS than the 64 KB a kernel gets unasked
    if (N > 44 && (dqmc::slogdet_set_lds_limit<real>() != 0 || dqmc::slogdet_bwd_set_lds_limit<real>() != 0))
      return fail(DQMC_E_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed for the determinant kernels of more than 44 electrons");
    analyse_lanes();
    analyse_chains();
    rc = analyse_pad_columns();
    if (rc) return rc;
    analyse_streams();
    if (sizeof(real) == 4) spec_k = dqmc::find_spec_kernel(program_hash());
    rc = set_weights(w, nw);
    if (rc) return rc;
    return build_fused_plan();
  }

  // ---- the rest of the engine, by concern (member functions; textual includes inside the struct body) ----
#include "engine_program.inl"
#include "engine_fused_plan.inl"
#include "engine_pass.inl"
#include "engine_refine.inl"
#include "engine_ecp.inl"
#include "engine_mcmc.inl"
#include "engine_grad.inl"
#include "engine_reverse.inl"
#include "engine_jac.inl"
#include "engine_kfac.inl"
#include "engine_coords.inl"
#include "engine_ecp_force.inl"
#include "engine_pretrain.inl"
#include "engine_optim.inl"
#include "engine_nuc.inl"
#include "engine_kfacopt.inl"
#include "engine_loss.inl"
#include "engine_observable.inl"
};

}  // namespace

extern "C" {

const char* dqmc_last_error(void) { return g_err.c_str(); }

int dqmc_create(dqmc_ctx** out, int device, void* stream, const dqmc_system* sys, const double* charges_host,
                const dqmc_buf* bufs_host, int n_bufs, const dqmc_op* ops_host, int n_ops, const double* weights_host,
                size_t n_weights, const int32_t* itable_host, size_t n_itable) {
  if (!out || !sys || !charges_host || !bufs_host || !ops_host || !weights_host || n_bufs < 1 || n_ops < 1)
    return fail(DQMC_E_ARG, "null argument");
  *out = nullptr;
  HIP_TRY(hipSetDevice(device));
  dqmc_ctx* ctx = nullptr;
  int rc;
  if (sys->dtype == 0) {
    auto* e = new Engine<float>();
    e->st = (hipStream_t)stream; e->device = device;
    rc = e->init(sys, charges_host, bufs_host, n_bufs, ops_host, n_ops, weights_host, n_weights, itable_host, n_itable);
    ctx = e;
  } else if (sys->dtype == 1) {
    auto* e = new Engine<double>();
    e->st = (hipStream_t)stream; e->device = device;
    rc = e->init(sys, charges_host, bufs_host, n_bufs, ops_host, n_ops, weights_host, n_weights, itable_host, n_itable);
    ctx = e;
  } else {
    return fail(DQMC_E_ARG, "dtype must be 0 (float32) or 1 (float64)");
  }
  if (rc) { delete ctx; return rc; }
  *out = ctx;
  return DQMC_OK;
}

void dqmc_destroy(dqmc_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  delete ctx;
}

int dqmc_set_weights(dqmc_ctx* ctx, const double* w, size_t n) {
  if (!ctx || !w) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->set_weights(w, n);
}
int dqmc_wf_eval(dqmc_ctx* ctx, const void* r, const void* R, int B, void* logpsi, int32_t* sign) {
  if (!ctx || !r || !R || !logpsi || !sign) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->wf_eval(r, R, B, logpsi, sign);
}
int dqmc_local_energy(dqmc_ctx* ctx, const void* r, const void* R, int B, void* e_loc, void* stats, void* grad,
                      void* logpsi, int32_t* sign) {
  if (!ctx || !r || !R || !e_loc) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->local_energy(r, R, B, e_loc, stats, grad, logpsi, sign);
}
int dqmc_psi_grad(dqmc_ctx* ctx, const void* r, const void* R, int B, void* logpsi, int32_t* sign, void* grad) {
  if (!ctx || !r || !R || !grad) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->psi_grad(r, R, B, logpsi, sign, grad);
}
int dqmc_log_psi_vjp(dqmc_ctx* ctx, const void* r, const void* R, int B, const void* cot, double* grad, void* logpsi,
                     int32_t* sign) {
  if (!ctx || !r || !R || !grad) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->log_psi_vjp(r, R, B, cot, grad, logpsi, sign);
}
int dqmc_log_psi_jacobian(dqmc_ctx* ctx, const void* r, const void* R, int B, void* jac, size_t ld_jac, void* logpsi,
                          int32_t* sign) {
  if (!ctx || !r || !R || !jac) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->log_psi_jacobian(r, R, B, jac, ld_jac, logpsi, sign);
}
int dqmc_kfac_layout(dqmc_ctx* ctx, int* n_linear, size_t* n_factor_doubles, size_t* n_rest) {
  if (!ctx) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->kfac_layout(n_linear, n_factor_doubles, n_rest);
}
int dqmc_log_psi_kfac(dqmc_ctx* ctx, const void* r, const void* R, int B, const void* cot, double* grad, double* factors, void* rest,
                      void* logpsi, int32_t* sign) {
  if (!ctx || !r || !R || !grad || !factors) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->log_psi_kfac(r, R, B, cot, grad, factors, rest, logpsi, sign);
}
int dqmc_log_psi_grad_coords(dqmc_ctx* ctx, const void* r, const void* R, int B, void* grad_r, void* grad_R, void* logpsi,
                             int32_t* sign) {
  if (!ctx || !r || !R) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->log_psi_grad_coords(r, R, B, grad_r, grad_R, logpsi, sign);
}
int dqmc_hf_force(dqmc_ctx* ctx, int estimator, const void* r, const void* R, int B, const void* grad_r, const void* grad_R,
                  const void* e_loc, double energy, double* force) {
  if (!ctx || !r || !R || !force) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->hf_force(estimator, r, R, B, grad_r, grad_R, e_loc, energy, force);
}
int dqmc_ecp_force(dqmc_ctx* ctx, int estimator, int all_rows, const void* r, const void* R, int B, const void* e_loc, double energy,
                   double* force, double* parts) {
  if (!ctx || !r || !R || !force) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->ecp_force(estimator, all_rows, r, R, B, e_loc, energy, force, parts);
}
int dqmc_set_pretrain_target(dqmc_ctx* ctx, int n_shells, const int32_t* shell_atom, const int32_t* shell_l, const int32_t* shell_n_prim,
                             const double* coeffs, const double* zetas, int n_ao, int n_mo, const double* mo_coeffs, int n_conf,
                             const int32_t* confs, const double* conf_coeffs) {
  if (!ctx || !shell_atom || !shell_l || !shell_n_prim || !coeffs || !zetas || !mo_coeffs || !confs || !conf_coeffs)
    return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->set_pretrain_target(n_shells, shell_atom, shell_l, shell_n_prim, coeffs, zetas, n_ao, n_mo, mo_coeffs, n_conf, confs,
                                  conf_coeffs);
}
int dqmc_pretrain_target(dqmc_ctx* ctx, const void* r, const void* R, int B, void* target) {
  if (!ctx || !r || !R || !target) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->pretrain_target(r, R, B, target);
}
int dqmc_orbitals(dqmc_ctx* ctx, const void* r, const void* R, int B, void* orb) {
  if (!ctx || !r || !R || !orb) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->orbitals(r, R, B, orb);
}
int dqmc_orbitals_vjp(dqmc_ctx* ctx, const void* r, const void* R, int B, const void* cot, double* grad, void* orb) {
  if (!ctx || !r || !R || !cot || !grad) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->orbitals_vjp(r, R, B, cot, grad, orb);
}
int dqmc_pretrain_loss_grad(dqmc_ctx* ctx, const void* r, const void* R, int B, double n_total, double* grad, double* per_sample_loss) {
  if (!ctx || !r || !R || !grad || !per_sample_loss) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->pretrain_loss_grad(r, R, B, n_total, grad, per_sample_loss);
}
int dqmc_set_param_map(dqmc_ctx* ctx, const int32_t* src_host, size_t n_weights, size_t n_params) {
  if (!ctx || !src_host) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->set_param_map(src_host, n_weights, n_params);
}
int dqmc_set_nuclear_stream(dqmc_ctx* ctx, const dqmc_nuc_stream* desc_host) {
  if (!ctx || !desc_host) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->set_nuclear_stream(desc_host);
}
int dqmc_weights_from_params(dqmc_ctx* ctx, const double* theta) {
  if (!ctx || !theta) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->weights_from_params(theta);
}
int dqmc_grad_to_params(dqmc_ctx* ctx, const double* grad_w, double* grad_theta) {
  if (!ctx || !grad_w || !grad_theta) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->grad_to_params(grad_w, grad_theta);
}
int dqmc_jacobian_to_params(dqmc_ctx* ctx, const void* jac, size_t ld_jac, int B, const void* logpsi, const int32_t* sign, void* jac_theta,
                            size_t ld_theta) {
  if (!ctx || !jac || !logpsi || !sign || !jac_theta) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->jacobian_to_params(jac, ld_jac, B, logpsi, sign, jac_theta, ld_theta);
}
int dqmc_adam_step(dqmc_ctx* ctx, double* theta, double* mu, double* nu, const double* grad_theta, size_t n, double lr, double b1,
                   double b2, double eps, int64_t t, double* norms3) {
  if (!ctx || !theta || !mu || !nu || !grad_theta) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->adam_step(theta, mu, nu, grad_theta, n, lr, b1, b2, eps, t, norms3);
}
int dqmc_apply_update(dqmc_ctx* ctx, double* theta, const double* delta, double scale, double* norms3) {
  if (!ctx || !theta || !delta) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->apply_update(theta, delta, scale, norms3);
}
int dqmc_set_kfac_map(dqmc_ctx* ctx, const dqmc_kfac_map* map_host) {
  if (!ctx || !map_host) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->set_kfac_map(map_host);
}
int dqmc_kfac_state_size(dqmc_ctx* ctx, size_t* n_doubles) {
  if (!ctx || !n_doubles) return fail(DQMC_E_ARG, "null argument");
  return ctx->kfac_state_size(n_doubles);
}
int dqmc_kfac_direction(dqmc_ctx* ctx, const double* grad_theta, const double* factors, const void* rest, const void* logpsi,
                        const int32_t* sign, int B, double* state, int first, double ema, double damping, double* delta, double* dot) {
  if (!ctx || !grad_theta || !factors || !logpsi || !sign || !state || !delta || !dot) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->kfac_direction(grad_theta, factors, rest, logpsi, sign, B, state, first, ema, damping, delta, dot);
}
int dqmc_kfac_apply(dqmc_ctx* ctx, double* theta, const double* delta, const double* dot, double lr, double norm_constraint,
                    double* norms4) {
  if (!ctx || !theta || !delta || !dot) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->kfac_apply(theta, delta, dot, lr, norm_constraint, norms4);
}
int dqmc_debug_read_weights(dqmc_ctx* ctx, int which, void* out_host, size_t bytes) {
  if (!ctx) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->debug_read_weights(which, out_host, bytes);
}
int dqmc_debug_nuc_dx_time(dqmc_ctx* ctx, int B, int reps, double* ms2, int* shape3) {
  if (!ctx || !ms2 || !shape3) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->debug_nuc_dx_time(B, reps, ms2, shape3);
}
int dqmc_graph_counters(dqmc_ctx* ctx, int64_t* out2) {
  if (!ctx || !out2) return fail(DQMC_E_ARG, "null argument");
  ctx->graph_counters(out2);
  return DQMC_OK;
}
int dqmc_psi_ratio(dqmc_ctx* ctx, const double* log_psi, const double* sign, int S, int B, double* ratio) {
  if (!ctx || !log_psi || !sign || !ratio) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->psi_ratio(log_psi, sign, S, B, ratio);
}
int dqmc_clip_rows(dqmc_ctx* ctx, const double* x, const double* w, int n_rows, int B, int center, int scale, double clip_width,
                   double exclude_width, double* x_clip, uint8_t* mask, double* row_stats) {
  if (!ctx || !x || !x_clip || !mask || !row_stats) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->clip_rows(x, w, n_rows, B, center, scale, clip_width, exclude_width, x_clip, mask, row_stats);
}
int dqmc_loss_cotangents(dqmc_ctx* ctx, const dqmc_loss_terms* terms, double* c, double* k) {
  if (!ctx || !terms || !c) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->loss_cotangents(terms, c, k);
}
int dqmc_oscillator_strength(dqmc_ctx* ctx, const void* r, const double* psi_ratio, const void* e_loc, int S, int B, double* os_mean,
                             double* os_err, double* cd_mean, double* cd_err) {
  if (!ctx || !r || !psi_ratio || !e_loc || !os_mean || !os_err || !cd_mean || !cd_err) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->oscillator_strength(r, psi_ratio, e_loc, S, B, os_mean, os_err, cd_mean, cd_err);
}
int dqmc_fd_displace(dqmc_ctx* ctx, const void* r, const void* R, int B, double h, void* r_out, void* R_out) {
  if (!ctx || !r || !R || !r_out || !R_out) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->fd_displace(r, R, B, h, r_out, R_out);
}
int dqmc_fd_force(dqmc_ctx* ctx, const void* log_d, const void* log_0, const void* e_d, const void* e_0, int B, double h, double* F) {
  if (!ctx || !log_d || !log_0 || !e_d || !e_0 || !F) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->fd_force(log_d, log_0, e_d, e_0, B, h, F);
}
int dqmc_mcmc_steps(dqmc_ctx* ctx, void* r, void* logpsi, int32_t* sign, int32_t* age, void* tau, const void* R,
                    int B, int n_sub, int max_age, double target_acceptance, uint64_t seed, const void* noise,
                    const void* unif, uint8_t* accept_out, double* stats7_host) {
  if (!ctx || !r || !logpsi || !sign || !age || !tau || !R) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->mcmc(r, logpsi, sign, age, tau, R, B, n_sub, max_age, target_acceptance, seed, noise, unif, accept_out,
                   stats7_host);
}
int dqmc_langevin_update(dqmc_ctx* ctx, const void* r, const void* R, const double* mol_charges_host, int B, const void* tau,
                         void* logpsi, int32_t* sign, void* force) {
  if (!ctx || !r || !R || !mol_charges_host || !tau || !force) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->langevin_update(r, R, mol_charges_host, B, tau, logpsi, sign, force);
}
int dqmc_langevin_steps(dqmc_ctx* ctx, void* r, void* logpsi, int32_t* sign, int32_t* age, void* force, void* tau, const void* R,
                        const double* mol_charges_host, int B, int n_sub, int max_age, double target_acceptance, uint64_t seed,
                        const void* noise, const void* unif, uint8_t* accept_out, double* stats7_host) {
  if (!ctx || !r || !logpsi || !sign || !age || !force || !tau || !R || !mol_charges_host) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->langevin(r, logpsi, sign, age, force, tau, R, mol_charges_host, B, n_sub, max_age, target_acceptance, seed, noise, unif,
                       accept_out, stats7_host);
}
int dqmc_exchange_step(dqmc_ctx* ctx, void* r, void* logpsi, int32_t* sign, int32_t* age, const void* tau, const void* R, int B,
                       const int32_t* up_idx, const int32_t* down_idx, const void* unif, uint8_t* accept_out, double* stats7_host) {
  if (!ctx || !r || !logpsi || !sign || !age || !tau || !R || !up_idx || !down_idx || !unif) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->exchange(r, logpsi, sign, age, tau, R, B, up_idx, down_idx, unif, accept_out, stats7_host);
}
int dqmc_set_ecp(dqmc_ctx* ctx, int n_terms_loc, const double* loc_host, int n_l, int n_terms_nl, const double* nl_host) {
  if (!ctx) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->set_ecp(n_terms_loc, loc_host, n_l, n_terms_nl, nl_host);
}
int dqmc_set_pseudo_hamiltonian(dqmc_ctx* ctx, int n_grid, double r_max, const double* rv_loc_host, const double* rv_l2_host,
                                const int32_t* mask_host) {
  if (!ctx) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->set_ph(n_grid, r_max, rv_loc_host, rv_l2_host, mask_host);
}
int dqmc_ecp_rotation(dqmc_ctx* ctx, uint64_t seed, const void* phi) {
  if (!ctx) return fail(DQMC_E_ARG, "null argument");
  return ctx->ecp_rotation(seed, phi);
}
int dqmc_energy_stats(dqmc_ctx* ctx, const void* e_loc, const void* w, int B, double* out7_host) {
  if (!ctx || !e_loc || !out7_host) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->energy_stats(e_loc, w, B, out7_host);
}

// The ONE collective of a VMC step inside the library: per-rank record -> ncclAllGather over the caller's RCCL
// communicator on the context's stream -> Chan merge.  librccl is resolved at the first call (dlopen), so the
// library itself carries no link-time dependency on it.
int dqmc_energy_stats_allgather(dqmc_ctx* ctx, void* rccl_comm, int n_ranks, const void* e_loc, const void* w, int B,
                                double* out5_host) {
  if (!ctx || !rccl_comm || !e_loc || !out5_host || n_ranks < 1 || n_ranks > 4096) return fail(DQMC_E_ARG, "null / bad argument");
  HIP_TRY(hipSetDevice(ctx->device));
  typedef int (*allgather_fn)(const void*, void*, size_t, int, void*, hipStream_t);
  static allgather_fn nccl_all_gather = nullptr;
  if (!nccl_all_gather) {
    void* h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return fail(DQMC_E_UNSUPPORTED, std::string("librccl.so not found: ") + dlerror());
    nccl_all_gather = (allgather_fn)dlsym(h, "ncclAllGather");
    if (!nccl_all_gather) return fail(DQMC_E_UNSUPPORTED, "ncclAllGather not found in librccl.so");
  }
  double* rec = nullptr;
  int rc = ctx->energy_stats_dev(e_loc, w, B, &rec);
  if (rc) return rc;
  rc = ctx->d_gather.reserve((size_t)n_ranks * 7, ctx->st);
  if (rc) return rc;
  const int nrc = nccl_all_gather(rec, ctx->d_gather, 7, /* ncclFloat64 */ 8, rccl_comm, ctx->st);
  if (nrc != 0) return fail(DQMC_E_HIP, "ncclAllGather failed with code " + std::to_string(nrc));
  std::vector<double> host((size_t)n_ranks * 7);
  HIP_TRY(hipMemcpyAsync(host.data(), ctx->d_gather, sizeof(double) * host.size(), hipMemcpyDeviceToHost, ctx->st));
  HIP_TRY(hipStreamSynchronize(ctx->st));
  return dqmc_merge_energy_stats(host.data(), n_ranks, out5_host);
}

int dqmc_merge_energy_stats(const double* rec, int n_ranks, double* out5) {
  if (!rec || !out5 || n_ranks < 1) return fail(DQMC_E_ARG, "null argument");
  // Chan et al. pairwise merge of (n, mean, M2); min/max/weighted sums are plain reductions.
  double n = 0, mean = 0, m2 = 0, sw = 0, swe = 0, mn = INFINITY, mx = -INFINITY;
  for (int k = 0; k < n_ranks; ++k) {
    const double* r = rec + 7 * k;
    const double nb = r[0], mb = r[3] / r[0];
    const double d = mb - mean, nt = n + nb;
    m2 += r[4] + d * d * n * nb / nt;
    mean += d * nb / nt;
    n = nt;
    sw += r[1]; swe += r[2];
    mn = std::fmin(mn, r[5]); mx = std::fmax(mx, r[6]);
  }
  out5[0] = mean; out5[1] = std::sqrt(m2 / n); out5[2] = mn; out5[3] = mx; out5[4] = swe / sw;
  return DQMC_OK;
}

int dqmc_debug_read(dqmc_ctx* ctx, int buf, double* out, size_t n) {
  if (!ctx || !out) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->debug_read(buf, out, n);
}
int dqmc_debug_lanes(dqmc_ctx* ctx) { return ctx ? ctx->last_TP : 0; }
int dqmc_last_refined(dqmc_ctx* ctx) { return ctx ? ctx->last_refined : 0; }
int dqmc_ecp_counts(dqmc_ctx* ctx, int64_t* out3) {
  if (!ctx || !out3) return DQMC_E_ARG;
  for (int k = 0; k < 3; ++k) out3[k] = ctx->ecp_last_counts[k];
  return DQMC_OK;
}
int dqmc_last_chunks(dqmc_ctx* ctx, int* out2) {
  if (!ctx || !out2) return DQMC_E_ARG;
  out2[0] = ctx->last_chunks[0]; out2[1] = ctx->last_chunks[1];
  return DQMC_OK;
}
int dqmc_refine_info(dqmc_ctx* ctx, double* out4) {
  if (!ctx || !out4) return fail(DQMC_E_ARG, "null argument");
  for (int k = 0; k < 4; ++k) out4[k] = ctx->refine_info[k];
  return DQMC_OK;
}
int dqmc_substep_kernel(dqmc_ctx* ctx, char* name_out, size_t n) {
  if (!ctx || !name_out || n < 1) return fail(DQMC_E_ARG, "null argument");
  return ctx->substep_kernel(name_out, n);
}
int dqmc_refine_counters(dqmc_ctx* ctx, int64_t* out4) {
  if (!ctx || !out4) return fail(DQMC_E_ARG, "null argument");
  for (int k = 0; k < 4; ++k) out4[k] = ctx->refine_counters[k];
  return DQMC_OK;
}
int dqmc_refine_scores(dqmc_ctx* ctx, double* out, int n) {
  if (!ctx || !out || n < 1) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->refine_scores(out, n);
}
int dqmc_set_option(dqmc_ctx* ctx, const char* name, int value) {
  if (!ctx || !name) return fail(DQMC_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return ctx->option(name, value);
}

// Per-launch HIP-event timing.  The records of a float32 context's float64 refinement twin are reported under the same
// names with the prefix "f64." ("f64.linear", "f64.attention", ...).
int dqmc_timing_enable(dqmc_ctx* ctx, int enable) {
  if (!ctx) return fail(DQMC_E_ARG, "null argument");
  ctx->t_collect();
  ctx->timing = enable != 0;
  if (dqmc_ctx* t = ctx->twin_ctx()) { t->t_collect(); t->timing = enable != 0; }
  return DQMC_OK;
}
int dqmc_timing_reset(dqmc_ctx* ctx) {
  if (!ctx) return fail(DQMC_E_ARG, "null argument");
  ctx->t_collect();
  ctx->trec.clear();
  if (dqmc_ctx* t = ctx->twin_ctx()) { t->t_collect(); t->trec.clear(); }
  return DQMC_OK;
}
int dqmc_timing_get(dqmc_ctx* ctx, const char* name, double* ms, int64_t* launches, double* flops) {
  if (!ctx || !name) return fail(DQMC_E_ARG, "null argument");
  if (!std::strncmp(name, "f64.", 4)) {
    dqmc_ctx* t = ctx->twin_ctx();
    if (t) return dqmc_timing_get(t, name + 4, ms, launches, flops);
    if (ms) *ms = 0; if (launches) *launches = 0; if (flops) *flops = 0;
    return DQMC_OK;
  }
  ctx->t_collect();
  auto it = ctx->trec.find(name);
  TimingRec r = it == ctx->trec.end() ? TimingRec{} : it->second;
  if (ms) *ms = r.ms;
  if (launches) *launches = r.launches;
  if (flops) *flops = r.flops;
  return DQMC_OK;
}
int dqmc_timing_get_executed(dqmc_ctx* ctx, const char* name, double* flops_executed) {
  if (!ctx || !name || !flops_executed) return fail(DQMC_E_ARG, "null argument");
  if (!std::strncmp(name, "f64.", 4)) {
    dqmc_ctx* t = ctx->twin_ctx();
    if (t) return dqmc_timing_get_executed(t, name + 4, flops_executed);
    *flops_executed = 0;
    return DQMC_OK;
  }
  ctx->t_collect();
  auto it = ctx->trec.find(name);
  *flops_executed = it == ctx->trec.end() ? 0.0 : it->second.executed;
  return DQMC_OK;
}
int dqmc_timing_names(dqmc_ctx* ctx, char* out, size_t n) {
  if (!ctx || !out || n == 0) return fail(DQMC_E_ARG, "null argument");
  ctx->t_collect();
  std::string s;
  for (auto& kv : ctx->trec) { if (!s.empty()) s += ","; s += kv.first; }
  if (dqmc_ctx* t = ctx->twin_ctx()) {
    t->t_collect();
    for (auto& kv : t->trec) { if (!s.empty()) s += ","; s += "f64." + kv.first; }
  }
  std::snprintf(out, n, "%s", s.c_str());
  return DQMC_OK;
}

}  // extern "C"
