// engine_pretrain.inl -- member functions of Engine<real>, included INSIDE the struct body by engine.hip: SCF-orbital
// pretraining.  The target table (dqmc_set_pretrain_target, dqmc_pretrain_target), the Slater matrices of the value pass on
// the device (dqmc_orbitals), and the two entry points of the Orbs mode of the reverse pass (engine_reverse.inl): the VJP of
// the Slater matrices with a given cotangent (dqmc_orbitals_vjp) and the fused loss + gradient step (dqmc_pretrain_loss_grad).

  DevBuf<int32_t> pt_shells, pt_confs;      // device tables of the target (kernels.h: launch_pretrain_target)
  DevBuf<real> pt_prims, pt_mo, pt_fac;
  int pt_n_shell = 0, pt_n_ao = 0, pt_n_mo = 0, pt_n_conf = 0;
  std::vector<char> orb_live;    // per op: a path leads from it to the ORBITALS destination buffer
  int orb_op = -1;               // the ORBITALS op
  bool orb_tab_built = false;

  size_t pt_target_bytes_per_walker() const { return sizeof(real) * (size_t)pt_n_conf * N * N; }

  // Liveness sweep of the Orbs mode: walking the ops backwards from the ORBITALS op, an op is live when it writes a buffer a
  // live op reads.  The Jastrow MLP, its ROW_SUM, SLOGDET and FINAL are not.
  int orb_tables() {
    if (orb_tab_built) return DQMC_OK;
    orb_op = -1;
    for (size_t k = 0; k < ops.size(); ++k) if (ops[k].kind == DQMC_OP_ORBITALS) orb_op = (int)k;
    if (orb_op < 0) return fail(DQMC_E_UNSUPPORTED, "orbitals: the program has no ORBITALS op");
    const dqmc_buf& ob = bufs[dqmc::OrbitalsOp(ops[orb_op]).dst()];
    if (ob.rows != sys.n_det || ob.width != pad4(N * N))
      return fail(DQMC_E_UNSUPPORTED, "orbitals: full-determinant programs only ([n_det][N x N] Slater matrices)");
    orb_live.assign(ops.size(), 0);
    std::vector<char> live_buf(bufs.size(), 0);
    std::vector<int> rd, wr;
    for (size_t k = (size_t)orb_op + 1; k-- > 0;) {
      rev_op_io(ops[k], rd, wr);
      bool live = (int)k == orb_op;
      for (int b : wr) live = live || live_buf[b];
      if (!live) continue;
      orb_live[k] = 1;
      for (int b : rd) live_buf[b] = 1;
    }
    orb_tab_built = true;
    return DQMC_OK;
  }

  int set_pretrain_target(int n_shells, const int32_t* atom, const int32_t* l, const int32_t* n_prim, const double* coeffs,
                          const double* zetas, int n_ao, int n_mo, const double* mo_coeffs, int n_conf, const int32_t* confs,
                          const double* conf_coeffs) override {
    // everything is checked before the first HIP call
    if (n_shells < 1 || n_ao < 1 || n_mo < 1 || n_conf < 1) return fail(DQMC_E_ARG, "set_pretrain_target: sizes must be positive");
    std::vector<int32_t> sh((size_t)n_shells * dqmc::PT_SHELL_INTS);
    std::vector<real> pr;
    int ao = 0, np = 0;
    for (int s = 0; s < n_shells; ++s) {
      if (l[s] < 0 || l[s] > dqmc::PT_LMAX)
        return fail(DQMC_E_ARG, "set_pretrain_target: shell " + std::to_string(s) + " has l = " + std::to_string(l[s]) + " (0 .. 3 supported)");
      if (atom[s] < 0 || atom[s] >= sys.n_nuc)
        return fail(DQMC_E_ARG, "set_pretrain_target: shell " + std::to_string(s) + " sits on atom " + std::to_string(atom[s]));
      if (n_prim[s] < 1) return fail(DQMC_E_ARG, "set_pretrain_target: shell " + std::to_string(s) + " has no primitives");
      int32_t* e = &sh[(size_t)s * dqmc::PT_SHELL_INTS];
      e[0] = atom[s]; e[1] = l[s]; e[2] = np; e[3] = n_prim[s]; e[4] = ao;
      for (int p = 0; p < n_prim[s]; ++p) {
        const double z = zetas[np + p];
        // rnorm = (2 zeta / pi)^(3/4) (4 zeta)^(l/2), folded into the contraction coefficient
        pr.push_back((real)(coeffs[np + p] * std::pow(2 * z / M_PI, 0.75) * std::pow(4 * z, 0.5 * l[s])));
        pr.push_back((real)z);
      }
      np += n_prim[s];
      ao += (l[s] + 1) * (l[s] + 2) / 2;
    }
    if (ao != n_ao)
      return fail(DQMC_E_ARG, "set_pretrain_target: the shells hold " + std::to_string(ao) + " Cartesian orbitals, n_ao = " + std::to_string(n_ao));
    if (n_ao > dqmc::PT_AO_CAP) return fail(DQMC_E_ARG, "set_pretrain_target: more than " + std::to_string(dqmc::PT_AO_CAP) + " atomic orbitals");
    for (long k = 0; k < (long)n_conf * N; ++k)
      if (confs[k] < 0 || confs[k] >= n_mo)
        return fail(DQMC_E_ARG, "set_pretrain_target: orbital index " + std::to_string(confs[k]) + " with n_mo = " + std::to_string(n_mo));
    std::vector<real> mo((size_t)n_ao * n_mo), fac((size_t)2 * n_conf);
    for (size_t k = 0; k < mo.size(); ++k) mo[k] = (real)mo_coeffs[k];
    for (int c = 0; c < n_conf; ++c) {      // the CI coefficient goes into the orbitals of its determinant: |c|^(1/N) each, the sign into column 0
      fac[2 * c] = (real)std::pow(std::fabs(conf_coeffs[c]), 1.0 / N);
      fac[2 * c + 1] = (real)(conf_coeffs[c] > 0 ? 1 : conf_coeffs[c] < 0 ? -1 : 0);
    }
    HIP_TRY(hipStreamSynchronize(st));      // (a call that reads the old tables may still run)
    int rc = pt_shells.upload(sh.data(), sh.size());      // (none of the five is empty: the sizes were checked above)
    if (!rc) rc = pt_prims.upload(pr.data(), pr.size());
    if (!rc) rc = pt_mo.upload(mo.data(), mo.size());
    if (!rc) rc = pt_confs.upload(confs, (size_t)n_conf * N);
    if (!rc) rc = pt_fac.upload(fac.data(), fac.size());
    if (rc) return rc;
    pt_n_shell = n_shells; pt_n_ao = n_ao; pt_n_mo = n_mo; pt_n_conf = n_conf;
    return DQMC_OK;
  }

  void pt_launch_target(const real* r, const real* R, int B, real* target) {
    dqmc::launch_pretrain_target<real>(st, r, R, pt_shells, pt_prims, pt_mo,
                                       pt_confs, pt_fac, target, B, N, pt_n_shell, pt_n_ao, pt_n_mo,
                                       pt_n_conf);
  }

  int pretrain_target(const void* r, const void* R, int B, void* target) override {
    if (!pt_n_conf) return fail(DQMC_E_ARG, "pretrain_target: no target set (dqmc_set_pretrain_target)");
    if (B < 1) return fail(DQMC_E_ARG, "B must be positive");
    pt_launch_target((const real*)r, (const real*)R, B, (real*)target);
    HIP_TRY(hipGetLastError());
    return DQMC_OK;
  }

  // the value pass op by op, per walker chunk, and the ORBITALS destination buffer copied out
  int orbitals(const void* r_, const void* R, int B, void* orb_) override {
    const real* r = (const real*)r_;
    real* orb = (real*)orb_;
    if (B < 1) return fail(DQMC_E_ARG, "B must be positive");
    { const int rc = orb_tables(); if (rc) return rc; }
    const size_t per = ws_bytes_per_walker(1) + sizeof(real) + sizeof(int32_t);
    long chunk = (long)(ws_budget / per);
    if (chunk < 1) chunk = 1;
    if (chunk > B) chunk = B;
    last_chunks[0] = (int)((B + chunk - 1) / chunk);
    Slab slab;                                   // log|psi| of a chunk, then (unpadded) its signs
    const auto o_lp = slab.take<real>((size_t)chunk);
    const Slab::Slice<int32_t> o_sg{slab.bytes};
    { const int rc = grad_ws_reserve(slab.bytes + sizeof(int32_t) * (size_t)chunk); if (rc) return rc; }
    const UnfusedForward unfused(*this);
    const int ob = dqmc::OrbitalsOp(ops[orb_op]).dst(), NN = N * N;
    for (int b0 = 0; b0 < B; b0 += (int)chunk) {
      const int nb = (B - b0) < chunk ? (B - b0) : (int)chunk;
      const int rc = run_chunk(r + (size_t)b0 * N * 3, (const real*)R, nb, false, o_lp.in(g_ws), o_sg.in(g_ws), nullptr, nullptr, nb, nullptr, 0);
      if (rc) return rc;
      dqmc::launch_orbitals_copy<real>(st, bptr(ob), bufs[ob].width, orb + (size_t)b0 * sys.n_det * NN, NN, NN, (long)nb * sys.n_det);
    }
    HIP_TRY(hipGetLastError());
    return DQMC_OK;
  }

  int orbitals_vjp(const void* r, const void* R, int B, const void* cot, double* grad, void* orb) override {
    HIP_TRY(hipMemsetAsync(grad, 0, sizeof(double) * n_weights, st));
    RevReq q{Rev::Orbs};
    q.cot_orb = (const real*)cot; q.grad = grad; q.orb = (real*)orb;
    return reverse_pass((const real*)r, (const real*)R, B, q);
  }

  int pretrain_loss_grad(const void* r, const void* R, int B, double n_total, double* grad, double* per_sample_loss) override {
    if (attention_refused(false)) return fail(DQMC_E_UNSUPPORTED, "pretrain_loss_grad: no reverse pass for ATTENTION ops");
    if (!pt_n_conf) return fail(DQMC_E_ARG, "pretrain_loss_grad: no target set (dqmc_set_pretrain_target)");
    if (!(n_total >= 1)) return fail(DQMC_E_ARG, "pretrain_loss_grad: n_total must be at least 1");
    HIP_TRY(hipMemsetAsync(grad, 0, sizeof(double) * n_weights, st));
    RevReq q{Rev::Orbs};
    q.grad = grad; q.ps_loss = per_sample_loss; q.n_total = n_total;
    return reverse_pass((const real*)r, (const real*)R, B, q);
  }
