// engine_kfac.inl -- member functions of Engine<real>, included INSIDE the struct body by engine.hip: KFAC Kronecker factors
// of the LINEAR ops from the reverse pass (dqmc_log_psi_kfac).
//
// One value pass and one reverse pass per walker chunk (grad_chunk with a KfacChunk).  The reverse pass is linear in the
// cotangent and the cotangent enters only at FINAL, so it runs with a unit cotangent: every pre-activation adjoint is then the
// dZ1 of G, and the cotangent is applied as a per-walker weight where parameter partials are summed over the walkers (the
// split-K k_lin_dw and the colsums of CONST, ORBITALS and FINAL).  After each LINEAR backward has formed dZ, the factor
// kernels (kernels_kfac.inl) add A_l and G_l of the chunk; the per-walker partials of the entries no LINEAR op owns go to
// the compact `rest` block through the Jacobian's scatter.
//
// Layout (include/dqmc.h): LINEAR op l in program order owns A_l (d_A x d_A, d_A = sum_p pad4(K_p) + has_bias) followed by
// G_l (ldw x ldw, ldw = pad4(nout)), both row-major double; rest column j is the j-th weight entry, ascending, that lies in
// no LINEAR op's W or bias block.

  std::vector<size_t> k_fac_off;      // per op: offset of A_l in `factors` (LINEAR ops)
  size_t k_fac_total = 0;
  int k_n_linear = 0;
  std::vector<long> k_rest_pos;       // per weight entry: its rest column, -1 when a LINEAR op owns it
  size_t k_n_rest = 0;
  GradDev k_rest_zero;                // rest columns no op writes (int32, device)
  int k_rest_nzero = 0;
  bool k_planned = false;

  static long kfac_dim_a(const dqmc_op& o) {
    long d = o.i[23] >= 0 ? 1 : 0;
    for (int p = 0; p < o.i[0]; ++p) d += pad4(o.i[3 + 4 * p]);
    return d;
  }
  static long kfac_dim_g(const dqmc_op& o) { return pad4(o.i[21]); }
  size_t kfac_part_bytes() const {
    size_t m = 0;
    for (const auto& o : ops)
      if (o.kind == DQMC_OP_LINEAR)
        m = std::max(m, std::max(dqmc::gram_part_doubles((int)kfac_dim_a(o)), dqmc::gram_part_doubles((int)kfac_dim_g(o))));
    return sizeof(double) * m;
  }

  int kfac_plan() {
    if (k_planned) return DQMC_OK;
    { const int rc = jac_plan(); if (rc) return rc; }
    k_fac_off.assign(ops.size(), 0);
    std::vector<uint8_t> owned(n_weights, 0), written(n_weights, 0);
    auto mark = [&](std::vector<uint8_t>& v, long off, long n) { for (long j = off; j < off + n; ++j) v[j] = 1; };
    k_fac_total = 0;
    k_n_linear = 0;
    for (size_t k = 0; k < ops.size(); ++k) {
      const dqmc_op& o = ops[k];
      const int32_t* i = o.i;
      switch (o.kind) {
        case DQMC_OP_LINEAR: {
          const long da = kfac_dim_a(o), dg = kfac_dim_g(o);
          k_fac_off[k] = k_fac_total;
          k_fac_total += (size_t)(da * da + dg * dg);
          ++k_n_linear;
          mark(owned, i[22], (da - (i[23] >= 0 ? 1 : 0)) * dg);
          if (i[23] >= 0) mark(owned, i[23], dg);
          break;
        }
        case DQMC_OP_CONST: mark(written, i[1], (long)bufs[i[0]].rows * bufs[i[0]].width); break;
        case DQMC_OP_ORBITALS: {
          const long ne = (long)sys.n_det * N * sys.n_nuc * (i[6] > 0 ? i[6] : 1);
          for (int q = 0; q < 4; ++q) mark(written, i[2 + q], ne);
          break;
        }
        case DQMC_OP_FINAL:
          if (i[1] >= 0) mark(written, i[1], sys.n_det);
          mark(written, i[3], 2);
          break;
        default: break;
      }
    }
    k_rest_pos.assign(n_weights, -1);
    std::vector<int32_t> zero;
    k_n_rest = 0;
    for (size_t j = 0; j < n_weights; ++j) {
      if (owned[j]) continue;
      if (!written[j] || jac_accum) zero.push_back((int32_t)k_n_rest);
      k_rest_pos[j] = (long)k_n_rest++;
    }
    k_rest_nzero = (int)zero.size();
    if (!zero.empty()) {
      HIP_TRY(hipMalloc(&k_rest_zero.p, sizeof(int32_t) * zero.size()));
      HIP_TRY(hipMemcpy(k_rest_zero.p, zero.data(), sizeof(int32_t) * zero.size(), hipMemcpyHostToDevice));
    }
    k_planned = true;
    return DQMC_OK;
  }

  void kfac_zero_rest(real* rest, int B) {
    dqmc::launch_jac_zero<real>(st, rest, (long)k_n_rest, (const int32_t*)k_rest_zero.p, k_rest_nzero, B);
  }

  int kfac_layout(int* n_linear, size_t* n_factor_doubles, size_t* n_rest) override {
    { const int rc = kfac_plan(); if (rc) return rc; }
    if (n_linear) *n_linear = k_n_linear;
    if (n_factor_doubles) *n_factor_doubles = k_fac_total;
    if (n_rest) *n_rest = k_n_rest;
    return DQMC_OK;
  }

  int log_psi_kfac(const void* r_, const void* R_, int B, const void* cot_, double* grad, double* factors, void* rest_, void* logpsi_,
                   int32_t* sign) override {
    if (B < 1) return fail(DQMC_E_ARG, "B must be positive");
    if (has_attention()) return fail(DQMC_E_UNSUPPORTED, "log_psi_kfac: no reverse pass for ATTENTION ops");
    if (N > dqmc::GRAD_GJ_NMAX) return fail(DQMC_E_UNSUPPORTED, "log_psi_kfac: more than 44 electrons");
    const real* r = (const real*)r_;
    const real* R = (const real*)R_;
    const real* cot = (const real*)cot_;
    real* rest = (real*)rest_;
    real* logpsi = (real*)logpsi_;
    { const int rc = grad_tables(); if (rc) return rc; }
    { const int rc = kfac_plan(); if (rc) return rc; }
    const size_t per = ws_bytes_per_walker(1) + grad_bytes_per_walker() + 2 * sizeof(double);
    const size_t fixed = grad_part_bytes() + kfac_part_bytes();
    long chunk = per ? (long)((ws_budget > fixed ? ws_budget - fixed : 0) / per) : B;
    if (chunk < 1) chunk = 1;
    last_chunks[0] = chunk >= B ? 1 : (int)((B + chunk - 1) / chunk);
    HIP_TRY(hipMemsetAsync(grad, 0, sizeof(double) * n_weights, st));
    if (k_fac_total) HIP_TRY(hipMemsetAsync(factors, 0, sizeof(double) * k_fac_total, st));
    // the value pass op by op with every activation in memory, as dqmc_log_psi_vjp
    const int fused_saved = fused_enabled;
    std::vector<int> child_saved;
    child_saved.swap(mlp_child);
    mlp_child.assign(ops.size(), -1);
    fused_enabled = 0;
    int rc = DQMC_OK;
    for (int b0 = 0; b0 < B && !rc; b0 += (int)chunk) {
      const int nb = (B - b0) < chunk ? (B - b0) : (int)chunk;
      const KfacChunk kf{cot ? cot + b0 : nullptr, factors, rest ? rest + (size_t)b0 * k_n_rest : nullptr};
      rc = grad_chunk(r + (size_t)b0 * N * 3, R, nb, nullptr, grad, logpsi ? logpsi + b0 : nullptr, sign ? sign + b0 : nullptr, nullptr,
                      0, &kf);
    }
    fused_enabled = fused_saved;
    mlp_child.swap(child_saved);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return DQMC_OK;
  }
