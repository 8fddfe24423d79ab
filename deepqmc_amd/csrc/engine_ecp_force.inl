// engine_ecp_force.inl -- member functions of Engine<real>, included INSIDE the struct body by engine.hip: the per-walker
// Hellmann-Feynman force of a Gaussian-type ECP Hamiltonian (dqmc_ecp_force),
//     F_I = F_nuc,I(Z) - dV_loc/dR_I - G_I,      G = gradient of the non-local term (kernels_ecp.hip).
//
// Per walker chunk (sized by ecp_max_cfg as local_energy_ecp and ecp_mixed size theirs): k_ecp_force_points writes the chunk's
// own walkers followed by 11 quadrature configurations per (walker, non-local nucleus, electron) triple; one Coords reverse
// pass over that batch gives log|psi|, sign, d log|psi| / dr and d log|psi| / dR of numerators and denominator in one
// arithmetic; k_ecp_force_reduce folds them into the non-local gradient per (walker, non-local nucleus); k_ecp_force_local adds
// the nuclear and local-term gradient and writes force and parts.  The assembly is double whatever the context's dtype.

  DevBuf<char> d_ecpf;           // configurations of a chunk, their log|psi|, sign and coordinate gradients, per-nucleus partial gradients
  bool ecp_is_set = false;       // dqmc_set_ecp has succeeded (a table of zeros is a Gaussian ECP all the same)

  int ecp_force(int est, int all_rows, const void* r_, const void* R_, int B, const void* e_loc_, double energy, double* force,
                double* parts) override {
    if (B < 1) return fail(DQMC_E_ARG, "B must be positive");
    if (est != DQMC_FORCE_BARE && est != DQMC_FORCE_AC_ZB)
      return fail(DQMC_E_ARG, "ecp_force: estimator " + std::to_string(est) + " (DQMC_FORCE_BARE or DQMC_FORCE_AC_ZB)");
    if (ph_n) return fail(DQMC_E_ARG, "ecp_force: a pseudo-Hamiltonian is set; only Gaussian-type ECPs have a force");
    if (!ecp_is_set) return fail(DQMC_E_ARG, "ecp_force: no Gaussian-type ECP is set (all-electron contexts: dqmc_hf_force)");
    const bool zb = est == DQMC_FORCE_AC_ZB;
    if (zb && !e_loc_) return fail(DQMC_E_ARG, "ecp_force: estimator " + std::to_string(est) + " needs e_loc");
    const real* r = (const real*)r_; const real* R = (const real*)R_;
    const real* e_loc = zb ? (const real*)e_loc_ : nullptr;
    const int n_nuc = sys.n_nuc, n_nl = ecp_n_nl;
    const size_t nB3 = (size_t)B * n_nuc * 3;
    double* part0 = parts; double* part1 = parts ? parts + nB3 : nullptr;
    const double* loc = ecp_nt_loc ? (const double*)d_ecp_loc : nullptr;
    dqmc::EcpArgs a{};
    a.r = r; a.R = R; a.nl_nuc = d_ecp_nuc; a.nl = d_ecp_nl; a.phi = ecp_phi; a.seed = ecp_seed;
    a.walker_idx = nullptr; a.phi_f32 = 0;
    a.B = B; a.N = N; a.n_nl = n_nl; a.L = ecp_L; a.n_t = ecp_nt_nl;
    if (n_nl == 0 && !zb) {      // local terms only: no psi enters
      a.b0 = 0; a.nb = B;
      t_begin("ecp_force", 0);
      dqmc::launch_ecp_force_local<real>(st, a, n_nuc, d_charges, loc, ecp_nt_loc, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0,
                                         force, part0, part1);
      t_end();
      last_chunks[0] = 1;
      HIP_TRY(hipGetLastError());
      return DQMC_OK;
    }
    if (attention_refused()) return fail(DQMC_E_UNSUPPORTED, "ecp_force: " + attention_refusal_text(true));
    if (N > dqmc::GRAD_GJ_NMAX) return fail(DQMC_E_UNSUPPORTED, "ecp_force: more than 64 electrons");
    { const int rc = coord_tables(); if (rc) return rc; }
    const size_t per_walker = (size_t)n_nl * N * 12;
    int nbw = per_walker ? (int)(ecp_max_cfg / per_walker) : (int)std::min<size_t>(ecp_max_cfg, (size_t)B);
    nbw = nbw < 1 ? 1 : (nbw > B ? B : nbw);
    const size_t cfg_pw = 1 + (size_t)n_nl * N * dqmc::ECPF_NQ, n_cfg = (size_t)nbw * cfg_pw;
    Slab slab;
    const auto o_rq = slab.take<real>(n_cfg * N * 3), o_lq = slab.take<real>(n_cfg);
    const auto o_sq = slab.take<int32_t>(n_cfg);
    const auto o_gr = slab.take<real>(n_nl ? n_cfg * N * 3 : 0), o_gR = slab.take<real>(n_cfg * n_nuc * 3);
    const auto o_gj = slab.take<double>((size_t)nbw * n_nl * n_nuc * 3);
    int rc = d_ecpf.reserve(slab.bytes, st, "ECP force scratch");
    if (rc) return rc;
    real *rq = o_rq.in(d_ecpf), *lq = o_lq.in(d_ecpf), *gr = n_nl ? o_gr.in(d_ecpf) : nullptr, *gR = o_gR.in(d_ecpf);
    int32_t* sq = o_sq.in(d_ecpf);
    double* gj = n_nl ? o_gj.in(d_ecpf) : nullptr;
    int n_chunks = 0;
    for (int b0 = 0; b0 < B; b0 += nbw, ++n_chunks) {
      a.b0 = b0; a.nb = (B - b0) < nbw ? (B - b0) : nbw;
      t_begin("ecp_force", 0);
      dqmc::launch_ecp_force_points<real>(st, a, rq);
      t_end();
      RevReq q{Rev::Coords};
      q.logpsi = lq; q.sign = sq; q.grad_r = gr; q.grad_R = gR;
      rc = reverse_pass(rq, R, (int)((size_t)a.nb * cfg_pw), q);
      if (rc) return rc;
      t_begin("ecp_force", 0);
      if (n_nl) dqmc::launch_ecp_force_reduce<real>(st, a, n_nuc, all_rows ? 1 : 0, lq, sq, gr, gR, gj);
      dqmc::launch_ecp_force_local<real>(st, a, n_nuc, d_charges, loc, ecp_nt_loc, gj, lq, sq, gR, e_loc, energy, force, part0, part1);
      t_end();
    }
    last_chunks[0] = n_chunks;      // (walker chunks of this call; each ran its own reverse pass)
    HIP_TRY(hipGetLastError());
    return DQMC_OK;
  }
