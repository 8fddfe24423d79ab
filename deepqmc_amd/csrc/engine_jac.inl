// engine_jac.inl -- member functions of Engine<real>, included INSIDE the struct body by engine.hip: the per-walker parameter
// Jacobian of log|psi| (dqmc_log_psi_jacobian).
//
// The reverse pass of engine_grad.inl with a cotangent of 1 per walker, where every op with parameters writes walker b's
// partials into row b of J instead of summing them over the walkers: LINEAR forms its weight blocks per walker
// (kernels_jac.inl, no split-K reduction), CONST / ORBITALS / FINAL copy their per-walker partials.  Entries no op writes
// (constants the ops do not read back, padding of the buffer) are zeroed first.  If two ops ever wrote the same entries,
// every row would be zeroed first and the ops would add in op order instead.

  GradDev g_jac_cols;            // the columns of J no op writes (int32, device)
  int g_jac_ncols = 0;
  bool jac_accum = false;        // some weight entry is written by more than one op
  bool jac_planned = false;

  int jac_plan() {
    if (jac_planned) return DQMC_OK;
    std::vector<uint8_t> cover(n_weights, 0);
    auto mark = [&](long off, long n) {
      for (long j = off; j < off + n; ++j) {
        if (cover[j]) jac_accum = true;
        cover[j] = 1;
      }
    };
    for (const auto& o : ops) {
      const int32_t* i = o.i;
      switch (o.kind) {
        case DQMC_OP_LINEAR: {
          const long ldw = pad4(i[21]);
          long w_row = 0;
          for (int p = 0; p < i[0]; ++p) w_row += pad4(i[3 + 4 * p]);
          mark(i[22], w_row * ldw);
          if (i[23] >= 0) mark(i[23], ldw);
          break;
        }
        case DQMC_OP_CONST: mark(i[1], (long)bufs[i[0]].rows * bufs[i[0]].width); break;
        case DQMC_OP_ORBITALS: {
          const long ne = (long)sys.n_det * N * sys.n_nuc * (i[6] > 0 ? i[6] : 1);
          for (int q = 0; q < 4; ++q) mark(i[2 + q], ne);
          break;
        }
        case DQMC_OP_FINAL:
          if (i[1] >= 0) mark(i[1], sys.n_det);
          mark(i[3], 2);
          break;
        default: break;
      }
    }
    std::vector<int32_t> cols;
    if (!jac_accum)
      for (size_t j = 0; j < n_weights; ++j) if (!cover[j]) cols.push_back((int32_t)j);
    g_jac_ncols = jac_accum ? (int)n_weights : (int)cols.size();
    if (!cols.empty()) {
      HIP_TRY(hipMalloc(&g_jac_cols.p, sizeof(int32_t) * cols.size()));
      HIP_TRY(hipMemcpy(g_jac_cols.p, cols.data(), sizeof(int32_t) * cols.size(), hipMemcpyHostToDevice));
    }
    jac_planned = true;
    return DQMC_OK;
  }

  void jac_zero_rows(real* jac, size_t ld_jac, int B) {
    dqmc::launch_jac_zero<real>(st, jac, (long)ld_jac, jac_accum ? nullptr : (const int32_t*)g_jac_cols.p, g_jac_ncols, B);
  }

  int log_psi_jacobian(const void* r_, const void* R_, int B, void* jac_, size_t ld_jac, void* logpsi_, int32_t* sign) override {
    if (B < 1) return fail(DQMC_E_ARG, "B must be positive");
    if (ld_jac < n_weights) return fail(DQMC_E_ARG, "ld_jac must be at least n_weights");
    if (has_attention()) return fail(DQMC_E_UNSUPPORTED, "log_psi_jacobian: no reverse pass for ATTENTION ops");
    if (N > dqmc::GRAD_GJ_NMAX) return fail(DQMC_E_UNSUPPORTED, "log_psi_jacobian: more than 44 electrons");
    const real* r = (const real*)r_;
    const real* R = (const real*)R_;
    real* jac = (real*)jac_;
    real* logpsi = (real*)logpsi_;
    { const int rc = grad_tables(); if (rc) return rc; }
    { const int rc = jac_plan(); if (rc) return rc; }
    const size_t per = ws_bytes_per_walker(1) + grad_bytes_per_walker();
    long chunk = per ? (long)((ws_budget > grad_part_bytes() ? ws_budget - grad_part_bytes() : 0) / per) : B;
    if (chunk < 1) chunk = 1;
    last_chunks[0] = chunk >= B ? 1 : (int)((B + chunk - 1) / chunk);
    // the value pass op by op with every activation in memory, as dqmc_log_psi_vjp
    const int fused_saved = fused_enabled;
    std::vector<int> child_saved;
    child_saved.swap(mlp_child);
    mlp_child.assign(ops.size(), -1);
    fused_enabled = 0;
    int rc = DQMC_OK;
    for (int b0 = 0; b0 < B && !rc; b0 += (int)chunk) {
      const int nb = (B - b0) < chunk ? (B - b0) : (int)chunk;
      rc = grad_chunk(r + (size_t)b0 * N * 3, R, nb, nullptr, nullptr, logpsi ? logpsi + b0 : nullptr, sign ? sign + b0 : nullptr,
                      jac + (size_t)b0 * ld_jac, ld_jac);
    }
    fused_enabled = fused_saved;
    mlp_child.swap(child_saved);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return DQMC_OK;
  }
