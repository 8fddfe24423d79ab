// engine_kfac.inl -- member functions of Engine<real>, included INSIDE the struct body by engine.hip: KFAC Kronecker factors
// of the LINEAR ops from the reverse pass (dqmc_log_psi_kfac).
//
// One value pass and one reverse pass per walker chunk, the Kfac mode of engine_reverse.inl.  The reverse pass is linear in
// the cotangent and the cotangent enters only at FINAL, so it runs with a unit cotangent: every pre-activation adjoint is then
// the dZ1 of G, and the cotangent is applied as a per-walker weight where parameter partials are summed over the walkers (the
// split-K k_lin_dw and the colsums of CONST, ORBITALS and FINAL).  Here: the layout of the factors and of the compact `rest`
// block, which the per-walker partials of the entries no LINEAR op owns reach through the Jacobian's scatter.
//
// Layout (include/dqmc.h): LINEAR op l in program order owns A_l (d_A x d_A, d_A = sum_p pad4(K_p) + has_bias) followed by
// G_l (ldw x ldw, ldw = pad4(nout)), both row-major double; rest column j is the j-th weight entry, ascending, that lies in
// no LINEAR op's W or bias block.

  std::vector<size_t> k_fac_off;      // per op: offset of A_l in `factors` (LINEAR ops)
  size_t k_fac_total = 0;
  int k_n_linear = 0;
  std::vector<long> k_rest_pos;       // per weight entry: its rest column, -1 when a LINEAR op owns it
  size_t k_n_rest = 0;
  DevBuf<int32_t> k_rest_zero;        // rest columns no op writes
  int k_rest_nzero = 0;
  bool k_planned = false;

  size_t kfac_part_bytes() const {
    size_t m = 0;
    for (const auto& o : ops)
      if (o.kind == DQMC_OP_LINEAR)
        m = std::max(m, std::max(dqmc::gram_part_doubles((int)dqmc::LinearOp(o).kfac_dim_a()), dqmc::gram_part_doubles((int)dqmc::LinearOp(o).kfac_dim_g())));
    return sizeof(double) * m;
  }

  int kfac_plan() {
    if (k_planned) return DQMC_OK;
    { const int rc = jac_plan(); if (rc) return rc; }
    k_fac_off.assign(ops.size(), 0);
    std::vector<uint8_t> owned(n_weights, 0), written(n_weights, 0);
    k_fac_total = 0;
    k_n_linear = 0;
    for (size_t k = 0; k < ops.size(); ++k) {
      if (ops[k].kind == DQMC_OP_LINEAR) {
        const long da = dqmc::LinearOp(ops[k]).kfac_dim_a(), dg = dqmc::LinearOp(ops[k]).kfac_dim_g();
        k_fac_off[k] = k_fac_total;
        k_fac_total += (size_t)(da * da + dg * dg);
        ++k_n_linear;
      }
      for_each_weight_block(ops[k], [&](long off, long n, bool linear) {
        for (long j = off; j < off + n; ++j) (linear ? owned : written)[j] = 1;
      });
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
    if (!zero.empty()) { const int rc = k_rest_zero.upload(zero.data(), zero.size()); if (rc) return rc; }
    k_planned = true;
    return DQMC_OK;
  }

  void kfac_zero_rest(real* rest, int B) {
    dqmc::launch_jac_zero<real>(st, rest, (long)k_n_rest, k_rest_zero, k_rest_nzero, B);
  }

  int kfac_layout(int* n_linear, size_t* n_factor_doubles, size_t* n_rest) override {
    { const int rc = kfac_plan(); if (rc) return rc; }
    if (n_linear) *n_linear = k_n_linear;
    if (n_factor_doubles) *n_factor_doubles = k_fac_total;
    if (n_rest) *n_rest = k_n_rest;
    return DQMC_OK;
  }

  int log_psi_kfac(const void* r, const void* R, int B, const void* cot, double* grad, double* factors, void* rest, void* logpsi,
                   int32_t* sign) override {
    { const int rc = kfac_plan(); if (rc) return rc; }
    HIP_TRY(hipMemsetAsync(grad, 0, sizeof(double) * n_weights, st));
    if (k_fac_total) HIP_TRY(hipMemsetAsync(factors, 0, sizeof(double) * k_fac_total, st));
    RevReq q{Rev::Kfac};
    q.logpsi = (real*)logpsi; q.sign = sign; q.cot = (const real*)cot; q.grad = grad; q.factors = factors; q.rest = (real*)rest;
    return reverse_pass((const real*)r, (const real*)R, B, q);
  }
