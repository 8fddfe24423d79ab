// engine_coords.inl -- member functions of Engine<real>, included INSIDE the struct body by engine.hip: d log|psi| / d r and
// d log|psi| / d R per walker (dqmc_log_psi_grad_coords) and the Hellmann-Feynman force estimators (dqmc_hf_force).
//
// The coordinate gradients are the Coords mode of the reverse pass (engine_reverse.inl).  The ops that read the coordinates
// (FEAT_EN, FEAT_EE, ORBITALS, the cusps of FINAL) turn their adjoints into one 3-vector per coordinate difference they read
// ("slots", kernels_coords.inl); one gather per particle then sums them in the fixed order of c_tab, which is built here.

  DevBuf<int32_t> c_tab;         // [N + n_nuc][c_S][2]: (slot, +1 / -1) per particle, slot -1 = end of the list
  std::vector<int> c_slot0;      // per op: first slot of its range, -1: none
  int c_n_slots = 0, c_S = 1;
  bool c_tab_built = false;

  int coord_tables() {
    if (c_tab_built) return DQMC_OK;
    const int n_nuc = sys.n_nuc, P = N + n_nuc;
    std::vector<std::vector<std::pair<int, int>>> l(P);
    c_slot0.assign(ops.size(), -1);
    int ns = 0;
    auto elec_nuc = [&]() {      // slot i * n_nuc + a: d = r_i - R_a
      for (int i = 0; i < N; ++i)
        for (int a = 0; a < n_nuc; ++a) { l[i].push_back({ns + i * n_nuc + a, 1}); l[N + a].push_back({ns + i * n_nuc + a, -1}); }
      ns += N * n_nuc;
    };
    for (size_t k = 0; k < ops.size(); ++k) {
      const dqmc::OpViews v(ops[k]);
      switch (ops[k].kind) {
        case DQMC_OP_FEAT_EN: case DQMC_OP_ORBITALS:
          c_slot0[k] = ns;
          elec_nuc();
          break;
        case DQMC_OP_FEAT_EE:
          c_slot0[k] = ns;
          for (int row = 0; row < v.feat_ee.n_rows(); ++row) {
            const int rc = h_itable[v.feat_ee.table() + 2 * row], sd = h_itable[v.feat_ee.table() + 2 * row + 1];
            if (rc == sd) continue;                    // a self edge: d = 0 whatever the coordinates
            l[rc].push_back({ns + row, 1});
            l[sd >= 0 ? sd : N - 1 - sd].push_back({ns + row, -1});
          }
          ns += v.feat_ee.n_rows();
          break;
        case DQMC_OP_FINAL:
          if (!v.fin.cusp_kind()) break;
          c_slot0[k] = ns;
          for (int a = 0, p = 0; a < N; ++a)
            for (int b = a + 1; b < N; ++b, ++p) { l[a].push_back({ns + p, 1}); l[b].push_back({ns + p, -1}); }
          ns += N * (N - 1) / 2;
          break;
        default: break;
      }
    }
    c_S = 1;
    for (const auto& v : l) c_S = std::max(c_S, (int)v.size());
    std::vector<int32_t> t((size_t)P * c_S * 2, -1);
    for (int p = 0; p < P; ++p)
      for (size_t e = 0; e < l[p].size(); ++e) { t[((size_t)p * c_S + e) * 2] = l[p][e].first; t[((size_t)p * c_S + e) * 2 + 1] = l[p][e].second; }
    { const int rc = c_tab.upload(t.data(), t.size()); if (rc) return rc; }
    c_n_slots = std::max(ns, 1);
    c_tab_built = true;
    return DQMC_OK;
  }

  int log_psi_grad_coords(const void* r, const void* R, int B, void* grad_r, void* grad_R, void* logpsi, int32_t* sign) override {
    if (!grad_r && !grad_R) return fail(DQMC_E_ARG, "log_psi_grad_coords: grad_r and grad_R are both NULL");
    { const int rc = coord_tables(); if (rc) return rc; }
    RevReq q{Rev::Coords};
    q.logpsi = (real*)logpsi; q.sign = sign; q.grad_r = (real*)grad_r; q.grad_R = (real*)grad_R;
    return reverse_pass((const real*)r, (const real*)R, B, q);
  }

  int hf_force(int est, const void* r, const void* R, int B, const void* grad_r, const void* grad_R, const void* e_loc, double energy,
               double* force) override {
    if (B < 1) return fail(DQMC_E_ARG, "B must be positive");
    if (est < DQMC_FORCE_NUCLEAR || est > DQMC_FORCE_AC_ZVQZB) return fail(DQMC_E_ARG, "hf_force: unknown estimator " + std::to_string(est));
    const bool zvq = est == DQMC_FORCE_AC_ZVQ || est == DQMC_FORCE_AC_ZVZBQ || est == DQMC_FORCE_AC_ZVQZB;
    const bool zb = est == DQMC_FORCE_AC_ZVZBQ || est == DQMC_FORCE_AC_ZB || est == DQMC_FORCE_AC_ZVQZB;
    const bool nuc = est == DQMC_FORCE_AC_ZB || est == DQMC_FORCE_AC_ZVQZB;
    if ((zvq && !grad_r) || (nuc && !grad_R) || (zb && !e_loc))
      return fail(DQMC_E_ARG, "hf_force: estimator " + std::to_string(est) + " needs " + (zvq && !grad_r ? "grad_r" : nuc && !grad_R ? "grad_R" : "e_loc"));
    dqmc::launch_hf_force<real>(st, est, (const real*)r, (const real*)R, d_charges, (const real*)grad_r, (const real*)grad_R,
                                (const real*)e_loc, energy, B, N, sys.n_nuc, force);
    HIP_TRY(hipGetLastError());
    return DQMC_OK;
  }
