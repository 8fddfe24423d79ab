// engine_jac.inl -- member functions of Engine<real>, included INSIDE the struct body by engine.hip: the per-walker parameter
// Jacobian of log|psi| (dqmc_log_psi_jacobian), the reverse pass of engine_reverse.inl in its Jac mode.
//
// Here: which weight entries each op's reverse pass writes, and the plan made from it.  Entries no op writes (constants the
// ops do not read back, padding of the buffer) are zeroed first.  If two ops ever wrote the same entries, every row would
// be zeroed first and the ops would add in op order instead.

  DevBuf<int32_t> g_jac_cols;    // the columns of J no op writes
  int g_jac_ncols = 0;
  bool jac_accum = false;        // some weight entry is written by more than one op
  bool jac_planned = false;

  // f(offset, count, is_linear) for every block of weight entries whose partials op o's reverse pass forms
  template <class F> void for_each_weight_block(const dqmc_op& o, F&& f) const {
    const dqmc::OpViews v(o);
    switch (o.kind) {
      case DQMC_OP_LINEAR:
        f((long)v.lin.w(), (long)v.lin.w_rows() * v.lin.ldw(), true);
        if (v.lin.has_bias()) f((long)v.lin.bias(), (long)v.lin.ldw(), true);
        break;
      case DQMC_OP_CONST: f((long)v.cst.table(), (long)bufs[v.cst.dst()].rows * bufs[v.cst.dst()].width, false); break;
      case DQMC_OP_ORBITALS:
        for (int t = 0; t < 4; ++t) f((long)v.orb.w(t), (long)sys.n_det * N * sys.n_nuc * v.orb.n_env(), false);
        break;
      case DQMC_OP_FINAL:
        if (v.fin.has_conf_coeff()) f((long)v.fin.conf_coeff(), (long)sys.n_det, false);
        f((long)v.fin.alphas(), 2L, false);
        break;
      default: break;
    }
  }

  int jac_plan() {
    if (jac_planned) return DQMC_OK;
    std::vector<uint8_t> cover(n_weights, 0);
    for (const auto& o : ops)
      for_each_weight_block(o, [&](long off, long n, bool) {
        for (long j = off; j < off + n; ++j) {
          if (cover[j]) jac_accum = true;
          cover[j] = 1;
        }
      });
    std::vector<int32_t> cols;
    if (!jac_accum)
      for (size_t j = 0; j < n_weights; ++j) if (!cover[j]) cols.push_back((int32_t)j);
    g_jac_ncols = jac_accum ? (int)n_weights : (int)cols.size();
    if (!cols.empty()) { const int rc = g_jac_cols.upload(cols.data(), cols.size()); if (rc) return rc; }
    jac_planned = true;
    return DQMC_OK;
  }

  void jac_zero_rows(real* jac, size_t ld_jac, int B) {
    dqmc::launch_jac_zero<real>(st, jac, (long)ld_jac, jac_accum ? nullptr : g_jac_cols.p, g_jac_ncols, B);
  }

  int log_psi_jacobian(const void* r, const void* R, int B, void* jac, size_t ld_jac, void* logpsi, int32_t* sign) override {
    if (ld_jac < n_weights) return fail(DQMC_E_ARG, "ld_jac must be at least n_weights");
    { const int rc = jac_plan(); if (rc) return rc; }
    RevReq q{Rev::Jac};
    q.logpsi = (real*)logpsi; q.sign = sign; q.jac = (real*)jac; q.ld_jac = ld_jac;
    return reverse_pass((const real*)r, (const real*)R, B, q);
  }
