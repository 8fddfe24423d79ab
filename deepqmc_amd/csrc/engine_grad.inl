// engine_grad.inl -- member functions of Engine<real>, included INSIDE the struct body by engine.hip: what every mode of the
// reverse pass (engine_reverse.inl) needs beside the value pass -- the adjoint workspace and its sizes, the gather tables of
// CONV and EDGE_SUM -- and the entry point of the plain mode, the parameter gradient of log|psi| contracted with a cotangent
// per walker (dqmc_log_psi_vjp).

  DevBuf<char> g_ws;             // the adjoint workspace, addressed by byte offset
  DevBuf<int32_t> g_tab;
  std::vector<int> g_tab_of;     // per op: {rows table offset, Sr, senders table offset, Ss} into g_tab (CONV, EDGE_SUM)

  // The one refusal of every entry point that needs the reverse pass: a program with an ATTENTION op is refused unless option
  // "attention_reverse" is on, and whatever the option when an ATTENTION op has constant key / value rows (the nuclear tokens
  // of the TransPsiformer are folded on the host from parameters and R: their adjoints have nowhere to go).
  // With option "nuclear_reverse" and a registered nuclear stream (engine_nuc.inl) the constant rows are admitted by the calls
  // that sum their partials over the walkers (per_walker false: the Vjp and Orbs modes).  With option "nuclear_coords" as well
  // the Coords mode is admitted (coords true: it needs per-walker ADJOINTS of the stream only, nuc_fold_coords).  Every other
  // mode would need the stream's parameter partials per walker and keeps refusing, as do dqmc_set_kfac_map and dqmc_ecp_force.
  // With option "nuclear_params" the Jac and Kfac modes, dqmc_set_kfac_map and dqmc_jacobian_to_params are admitted (params true:
  // the stream's parameter partials per walker, nuc_fold_rows); dqmc_ecp_force keeps refusing.
  // 0: runs, 1: no reverse pass for ATTENTION ops, 2: nuclear tokens, per-walker mode.
  int attention_refusal(bool per_walker, bool coords = false, bool params = false) const {
    for (const auto& o : ops)
      if (o.kind == DQMC_OP_ATTENTION) {
        if (!attention_reverse) return 1;
        if (dqmc::AttentionOp(o).n_const() > 0) {
          if (!nuclear_reverse || !nuc_set) return 1;
          if (per_walker && !(coords && nuclear_coords) && !(params && nuclear_params)) return 2;
        }
      }
    return 0;
  }
  bool attention_refused(bool per_walker = true, bool coords = false, bool params = false) const {
    return attention_refusal(per_walker, coords, params) != 0;
  }
  std::string attention_refusal_text(bool per_walker, bool coords = false, bool params = false) const {
    return attention_refusal(per_walker, coords, params) == 2
               ? "the nuclear-token stream has no per-walker partials (all walkers share it: one nuclear backward per walker); only "
                 "log_psi_vjp, orbitals_vjp and pretrain_loss_grad run with nuclear tokens"
               : "no reverse pass for ATTENTION ops";
  }
  // the Coords mode carries the stream's part into grad_R: constant rows, option "nuclear_coords", grad_R requested
  bool nuc_coords_active(bool want_R) const { return want_R && nuclear_coords && nuclear_reverse && nuc_set && grad_att_const() > 0; }
  size_t grad_att_const() const {      // largest n_const * heads * head_dim of an ATTENTION op
    size_t m = 0;
    for (const auto& o : ops)
      if (o.kind == DQMC_OP_ATTENTION) { const dqmc::AttentionOp a(o); m = std::max(m, (size_t)a.n_const() * a.heads() * a.head_dim()); }
    return m;
  }
  // what the reverse pass reads and writes of an op: op_io, which leaves ATTENTION out because the forward planners that
  // call it never reach one
  static void rev_op_io(const dqmc_op& op, std::vector<int>& rd, std::vector<int>& wr) {
    op_io(op, rd, wr);
    if (op.kind == DQMC_OP_ATTENTION) {
      const dqmc::AttentionOp a(op);
      for (int q = 0; q < 3; ++q) rd.push_back(a.buf(q));
      wr.push_back(a.dst());
    }
  }
  size_t grad_zrow() const {     // largest nrows * ldw of a LINEAR op
    size_t z = 4;
    for (const auto& o : ops)
      if (o.kind == DQMC_OP_LINEAR) z = std::max(z, (size_t)dqmc::LinearOp(o).nrows() * dqmc::LinearOp(o).ldw());
    return z;
  }
  size_t grad_orb_partials() const {   // doubles per walker of the ORBITALS table partials
    for (const auto& o : ops)
      if (o.kind == DQMC_OP_ORBITALS) return (size_t)4 * sys.n_det * N * sys.n_nuc * dqmc::OrbitalsOp(o).n_env();
    return 0;
  }
  // adjoint workspace bytes per walker (beside the value pass's ws_bytes_per_walker(1))
  size_t grad_bytes_per_walker() const {
    size_t b = 0;
    for (const auto& bb : bufs) b += sizeof(real) * (size_t)bb.rows * bb.width;
    b += sizeof(real) * (2 * grad_zrow() + max_ldw());                      // Z, dZ, dZs
    b += sizeof(double) * (grad_orb_partials() + 2 * (size_t)sys.n_det + 2);   // table partials, dL, conf_coeff / alpha partials
    b += sizeof(real) + sizeof(int32_t);                                        // log|psi|, sign when the caller passes none
    b += sizeof(real) * 2 * grad_att_const();                                   // dKc, dVc partials of the constant rows
    return b;
  }
  size_t grad_part_bytes() const {
    size_t m = 0;
    for (const auto& o : ops)
      if (o.kind == DQMC_OP_LINEAR) {
        const dqmc::LinearOp l(o);
        const int nt = (l.ldw() + 15) / 16;
        m = std::max(m, dqmc::grad_dw_part_doubles(1, nt));             // bias
        for (int p = 0; p < l.n_pieces(); ++p) m = std::max(m, dqmc::grad_dw_part_doubles((l.K(p) + 15) / 16, nt));
      }
    return sizeof(double) * m;
  }

  int grad_ws_reserve(size_t bytes) { return g_ws.reserve(bytes, st, "gradient workspace"); }

  // receiver / sender gather tables of the CONV and EDGE_SUM ops (the transposes of their (edge row, sender) lists)
  int grad_tables() {
    if (g_tab) return DQMC_OK;
    std::vector<int32_t> t;
    g_tab_of.assign(4 * ops.size(), 0);
    for (size_t k = 0; k < ops.size(); ++k) {
      const dqmc_op& o = ops[k];
      if (o.kind != DQMC_OP_CONV && o.kind != DQMC_OP_EDGE_SUM) continue;
      const dqmc::ConvOp e(o);        // (EDGE_SUM: the slots it shares with CONV)
      const int S = e.S(), e_rows = bufs[e.edge()].rows;
      const int s_rows = o.kind == DQMC_OP_CONV ? bufs[e.node()].rows : 1;
      std::vector<std::vector<std::pair<int, int>>> rl(e_rows), sl(s_rows);
      for (int rc = 0; rc < N; ++rc)
        for (int s = 0; s < S; ++s) {
          const int row = h_itable[e.table() + 2 * (rc * S + s)], snd = h_itable[e.table() + 2 * (rc * S + s) + 1];
          if (row < 0) continue;
          rl[row].push_back({rc, snd});
          if (o.kind == DQMC_OP_CONV) sl[snd >= 0 ? snd : -1 - snd].push_back({rc, row});
        }
      auto emit = [&](const std::vector<std::vector<std::pair<int, int>>>& l, int& off, int& w) {
        w = 1;
        for (const auto& v : l) w = std::max(w, (int)v.size());
        off = (int)t.size();
        for (const auto& v : l)
          for (int e = 0; e < w; ++e) {
            t.push_back(e < (int)v.size() ? v[e].first : -1);
            t.push_back(e < (int)v.size() ? v[e].second : -1);
          }
      };
      emit(rl, g_tab_of[4 * k], g_tab_of[4 * k + 1]);
      emit(sl, g_tab_of[4 * k + 2], g_tab_of[4 * k + 3]);
    }
    if (t.empty()) t.push_back(-1);
    return g_tab.upload(t.data(), t.size());
  }

  int log_psi_vjp(const void* r, const void* R, int B, const void* cot, double* grad, void* logpsi, int32_t* sign) override {
    HIP_TRY(hipMemsetAsync(grad, 0, sizeof(double) * n_weights, st));
    RevReq q{Rev::Vjp};
    q.logpsi = (real*)logpsi; q.sign = sign; q.cot = (const real*)cot; q.grad = grad;
    return reverse_pass((const real*)r, (const real*)R, B, q);
  }
