// engine_grad.inl -- member functions of Engine<real>, included INSIDE the struct body by engine.hip: the parameter
// gradient of log|psi| contracted with a cotangent per walker (dqmc_log_psi_vjp).
//
// Per walker chunk: the per-op value pass (TP = 1, no fused kernel, no chained MLPs, so that every activation buffer the
// reverse pass reads is in memory), then the ops in reverse with adjoint buffers of the same shapes.  LINEAR recomputes its
// pre-activation Z = X W + b with the forward kernel (act = none) instead of storing it in the forward: the value pass
// stays the one dqmc_wf_eval runs, and one extra GEMM per layer costs less than the other two (dX, dW) each.  Weight
// gradients accumulate across chunks in double through fixed-order reductions (kernels_grad.inl).

  struct GradDev {               // device allocation released with the context
    void* p = nullptr;
    ~GradDev() { if (p) (void)hipFree(p); }
  };
  // dqmc_log_psi_kfac's additions to one chunk of the reverse pass (engine_kfac.inl)
  struct KfacChunk {
    const real* cot;             // the chunk's cotangents, or nullptr (ones)
    double* factors;             // A_l, G_l of every LINEAR op, accumulated
    real* rest;                  // [B][n_rest] partials of the entries no LINEAR op owns, or nullptr
  };
  // dqmc_log_psi_grad_coords's outputs for one chunk (engine_coords.inl); either may be nullptr
  struct CoordChunk {
    real* grad_r;                // [B][N][3]
    real* grad_R;                // [B][n_nuc][3]
  };
  GradDev g_ws, g_tab;
  size_t g_ws_bytes = 0;
  std::vector<int> g_tab_of;     // per op: {rows table offset, Sr, senders table offset, Ss} into g_tab (CONV, EDGE_SUM)
  bool g_tab_built = false;

  bool has_attention() const {
    for (const auto& o : ops) if (o.kind == DQMC_OP_ATTENTION) return true;
    return false;
  }
  size_t grad_zrow() const {     // largest nrows * ldw of a LINEAR op
    size_t z = 4;
    for (const auto& o : ops)
      if (o.kind == DQMC_OP_LINEAR && (size_t)o.i[20] * pad4(o.i[21]) > z) z = (size_t)o.i[20] * pad4(o.i[21]);
    return z;
  }
  size_t grad_max_ldw() const {
    size_t m = 4;
    for (const auto& o : ops) if (o.kind == DQMC_OP_LINEAR && (size_t)pad4(o.i[21]) > m) m = (size_t)pad4(o.i[21]);
    return m;
  }
  size_t grad_orb_partials() const {   // doubles per walker of the ORBITALS table partials
    for (const auto& o : ops)
      if (o.kind == DQMC_OP_ORBITALS) return (size_t)4 * sys.n_det * N * sys.n_nuc * (o.i[6] > 0 ? o.i[6] : 1);
    return 0;
  }
  // adjoint workspace bytes per walker (beside the value pass's ws_bytes_per_walker(1))
  size_t grad_bytes_per_walker() const {
    size_t b = 0;
    for (const auto& bb : bufs) b += sizeof(real) * (size_t)bb.rows * bb.width;
    b += sizeof(real) * (2 * grad_zrow() + grad_max_ldw());                      // Z, dZ, dZs
    b += sizeof(double) * (grad_orb_partials() + 2 * (size_t)sys.n_det + 2);   // table partials, dL, conf_coeff / alpha partials
    b += sizeof(real) + sizeof(int32_t);                                        // log|psi|, sign when the caller passes none
    return b;
  }
  size_t grad_part_bytes() const {
    size_t m = 0;
    for (const auto& o : ops)
      if (o.kind == DQMC_OP_LINEAR) {
        const int nt = (pad4(o.i[21]) + 15) / 16;
        m = std::max(m, dqmc::grad_dw_part_doubles(1, nt));             // bias
        for (int p = 0; p < o.i[0]; ++p) m = std::max(m, dqmc::grad_dw_part_doubles((o.i[3 + 4 * p] + 15) / 16, nt));
      }
    return sizeof(double) * m;
  }

  // receiver / sender gather tables of the CONV and EDGE_SUM ops (the transposes of their (edge row, sender) lists)
  int grad_tables() {
    if (g_tab_built) return DQMC_OK;
    std::vector<int32_t> t;
    g_tab_of.assign(4 * ops.size(), 0);
    for (size_t k = 0; k < ops.size(); ++k) {
      const dqmc_op& o = ops[k];
      if (o.kind != DQMC_OP_CONV && o.kind != DQMC_OP_EDGE_SUM) continue;
      const int32_t* i = o.i;
      const int S = i[5], e_rows = bufs[i[0]].rows;
      const int s_rows = o.kind == DQMC_OP_CONV ? bufs[i[1]].rows : 1;
      std::vector<std::vector<std::pair<int, int>>> rl(e_rows), sl(s_rows);
      for (int rc = 0; rc < N; ++rc)
        for (int s = 0; s < S; ++s) {
          const int row = h_itable[i[4] + 2 * (rc * S + s)], snd = h_itable[i[4] + 2 * (rc * S + s) + 1];
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
    HIP_TRY(hipMalloc(&g_tab.p, sizeof(int32_t) * t.size()));
    HIP_TRY(hipMemcpy(g_tab.p, t.data(), sizeof(int32_t) * t.size(), hipMemcpyHostToDevice));
    g_tab_built = true;
    return DQMC_OK;
  }

  int log_psi_vjp(const void* r_, const void* R_, int B, const void* cot_, double* grad, void* logpsi_, int32_t* sign) override {
    if (B < 1) return fail(DQMC_E_ARG, "B must be positive");
    if (has_attention()) return fail(DQMC_E_UNSUPPORTED, "log_psi_vjp: no reverse pass for ATTENTION ops");
    if (N > dqmc::GRAD_GJ_NMAX) return fail(DQMC_E_UNSUPPORTED, "log_psi_vjp: more than 44 electrons");
    const real* r = (const real*)r_;
    const real* R = (const real*)R_;
    const real* cot = (const real*)cot_;
    real* logpsi = (real*)logpsi_;
    { const int rc = grad_tables(); if (rc) return rc; }
    const size_t per = ws_bytes_per_walker(1) + grad_bytes_per_walker();
    long chunk = per ? (long)((ws_budget > grad_part_bytes() ? ws_budget - grad_part_bytes() : 0) / per) : B;
    if (chunk < 1) chunk = 1;
    last_chunks[0] = chunk >= B ? 1 : (int)((B + chunk - 1) / chunk);
    HIP_TRY(hipMemsetAsync(grad, 0, sizeof(double) * n_weights, st));
    // the value pass op by op with every activation in memory: no fused kernel, no chained MLPs
    const int fused_saved = fused_enabled;
    std::vector<int> child_saved;
    child_saved.swap(mlp_child);
    mlp_child.assign(ops.size(), -1);
    fused_enabled = 0;
    int rc = DQMC_OK;
    for (int b0 = 0; b0 < B && !rc; b0 += (int)chunk) {
      const int nb = (B - b0) < chunk ? (B - b0) : (int)chunk;
      rc = grad_chunk(r + (size_t)b0 * N * 3, R, nb, cot ? cot + b0 : nullptr, grad, logpsi ? logpsi + b0 : nullptr,
                      sign ? sign + b0 : nullptr, nullptr, 0);
    }
    fused_enabled = fused_saved;
    mlp_child.swap(child_saved);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return DQMC_OK;
  }

  // jac == nullptr: accumulate sum_b cot[b] (...) into grad (dqmc_log_psi_vjp).  Otherwise (dqmc_log_psi_jacobian, cot == nullptr,
  // grad unused) row b of jac[B][ld_jac] receives walker b's parameter partials (engine_jac.inl).
  // kf != nullptr (dqmc_log_psi_kfac, cot == nullptr, jac == nullptr): the adjoints are those of a unit cotangent; kf->cot
  // weights the walker sums of grad, and the KFAC factors and rest partials are formed on the way (engine_kfac.inl).
  // cc != nullptr (dqmc_log_psi_grad_coords, cot, grad, jac and kf all nullptr): no parameter gradients; the adjoints are carried
  // into the coordinates instead (engine_coords.inl).
  int grad_chunk(const real* r, const real* R, int B, const real* cot, double* grad, real* logpsi, int32_t* sign, real* jac,
                 size_t ld_jac, const KfacChunk* kf = nullptr, const CoordChunk* cc = nullptr) {
    // adjoint workspace of this chunk
    std::vector<size_t> adj(bufs.size());
    size_t off = 0;
    auto bump = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    for (size_t k = 0; k < bufs.size(); ++k) adj[k] = bump(sizeof(real) * (size_t)B * bufs[k].rows * bufs[k].width);
    const size_t adj_end = off;
    const size_t o_z = bump(sizeof(real) * (size_t)B * grad_zrow()), o_dz = bump(sizeof(real) * (size_t)B * grad_zrow());
    const size_t o_dzs = bump(sizeof(real) * (size_t)B * grad_max_ldw());
    const size_t o_orb = bump(sizeof(double) * (size_t)B * (!cc && grad_orb_partials() ? grad_orb_partials() : 1));
    const size_t o_dl = bump(sizeof(double) * (size_t)B * sys.n_det), o_pw = bump(sizeof(double) * (size_t)B * (sys.n_det + 2));
    const size_t o_lp = bump(sizeof(real) * (size_t)B), o_sg = bump(sizeof(int32_t) * (size_t)B);
    const size_t o_part = bump(cc ? 0 : grad_part_bytes());
    const size_t o_kw = bump(kf ? sizeof(double) * 2 * (size_t)B : 0), o_kpart = bump(kf ? kfac_part_bytes() : 0);
    const size_t o_slot = bump(cc ? sizeof(double) * 3 * (size_t)B * c_n_slots : 0);
    if (off > g_ws_bytes) {
      if (g_ws.p) { HIP_TRY(hipStreamSynchronize(st)); HIP_TRY(hipFree(g_ws.p)); g_ws.p = nullptr; g_ws_bytes = 0; }
      const hipError_t e = hipMalloc(&g_ws.p, off);
      if (e != hipSuccess) return fail(DQMC_E_NOMEM, "gradient workspace of " + std::to_string(off) + " bytes: " + hipGetErrorString(e));
      g_ws_bytes = off;
    }
    char* gw = (char*)g_ws.p;
    auto A = [&](int b) { return reinterpret_cast<real*>(gw + adj[b]); };
    real* lp = logpsi ? logpsi : reinterpret_cast<real*>(gw + o_lp);
    int32_t* sg = sign ? sign : reinterpret_cast<int32_t*>(gw + o_sg);
    { const int rc = run_chunk(r, R, B, false, lp, sg, nullptr, nullptr, B, nullptr, 0); if (rc) return rc; }
    HIP_TRY(hipMemsetAsync(gw, 0, adj_end, st));
    const dqmc::JacOut<real> jo{jac, (long)ld_jac, lp, sg, jac_accum ? 1 : 0,
                                (ld_jac % 4 == 0 && (reinterpret_cast<uintptr_t>(jac) & 15) == 0) ? 1 : 0};
    if (jac) jac_zero_rows(jac, ld_jac, B);
    // kfac: per-walker weights of the walker sums (cot, 0 for invalid walkers) and validity flags of the factors
    double* kw = kf ? reinterpret_cast<double*>(gw + o_kw) : nullptr;
    const dqmc::JacOut<real> ko{kf ? kf->rest : nullptr, (long)k_n_rest, lp, sg, jac_accum ? 1 : 0, 0};
    if (kf) {
      dqmc::launch_kfac_weights<real>(st, lp, sg, kf->cot, kw, B);
      if (kf->rest) kfac_zero_rest(kf->rest, B);
    }
    const int32_t* gt = (const int32_t*)g_tab.p;
    double* dL = reinterpret_cast<double*>(gw + o_dl);
    double* slot = cc ? reinterpret_cast<double*>(gw + o_slot) : nullptr;     // coordinate-difference adjoints (kernels_coords.inl)
    for (size_t opi = ops.size(); opi-- > 0;) {
      const dqmc_op& op = ops[opi];
      const int32_t* i = op.i;
      switch (op.kind) {
        case DQMC_OP_FEAT_EN:      // leaves: no parameters; only the coordinate mode carries their adjoints on
          if (cc)
            dqmc::launch_feat_en_coords<real>(st, r, R, A(i[0]), bufs[i[0]].width, B, N, sys.n_nuc, sys.norm_eps, i[1],
                                              slot + 3 * (size_t)c_slot0[opi], c_n_slots);
          break;
        case DQMC_OP_FEAT_EE:
          if (cc)
            dqmc::launch_feat_ee_coords<real>(st, r, R, d_it + i[1], A(i[0]), i[2], B, N, sys.norm_eps, i[3],
                                              slot + 3 * (size_t)c_slot0[opi], c_n_slots);
          break;
        case DQMC_OP_LINEAR: {
          // Z = X W + b with the forward kernel (no activation, no residual)
          dqmc::LinArgs<real> f{};
          f.cfg_bf = linear_bf; f.cfg_bkx = linear_bkx; f.cfg_f64_split = linear_f64_split;
          f.n_pieces = i[0];
          dqmc::LinBwdArgs<real> a{};
          a.n_pieces = i[0];
          int w_row = 0;
          for (int p = 0; p < i[0]; ++p) {
            const int sb = i[1 + 4 * p];
            f.piece[p].src = bptr(sb);
            f.piece[p].ld = bufs[sb].width; f.piece[p].rpw = bufs[sb].rows; f.piece[p].r0 = i[2 + 4 * p];
            f.piece[p].K = pad4(i[3 + 4 * p]); f.piece[p].bcast = i[4 + 4 * p]; f.piece[p].w_row = w_row;
            a.piece[p].X = bptr(sb); a.piece[p].dX = A(sb);
            a.piece[p].ld = bufs[sb].width; a.piece[p].rpw = bufs[sb].rows; a.piece[p].r0 = i[2 + 4 * p];
            a.piece[p].K = i[3 + 4 * p]; a.piece[p].bcast = i[4 + 4 * p]; a.piece[p].w_row = w_row;
            w_row += pad4(i[3 + 4 * p]);
          }
          real* Z = reinterpret_cast<real*>(gw + o_z);
          f.W = d_w + i[22]; f.ldw = pad4(i[21]); f.bias = i[23] >= 0 ? d_w + i[23] : nullptr;
          f.dst = Z; f.ld_dst = f.ldw; f.rpw_dst = i[20]; f.r0_dst = 0; f.col0_dst = 0;
          f.act = 0; f.nrows = i[20]; f.B = B; f.T = 1; f.TP = 1;
          t_begin(cc ? "linear_dx" : jac ? "linear_jac" : "linear_bwd", (cc ? 4.0 : 6.0) * B * i[20] * (double)w_row * f.ldw);     // Z recompute, dX, dW
          dqmc::launch_linear<real>(st, f);
          a.W = f.W; a.ldw = f.ldw; a.nout = i[21]; a.nrows = i[20]; a.B = B; a.act = i[24];
          a.Z = Z; a.dZ = reinterpret_cast<real*>(gw + o_dz); a.dZs = reinterpret_cast<real*>(gw + o_dzs);
          a.dY = A(i[17]); a.ld_dst = bufs[i[17]].width; a.rpw_dst = bufs[i[17]].rows; a.r0_dst = i[18]; a.col0_dst = i[19];
          if (i[25] >= 0) { a.dres = A(i[25]); a.ld_res = bufs[i[25]].width; a.rpw_res = bufs[i[25]].rows; a.r0_res = i[26]; }
          a.res_scale = i[27] ? (real)0.70710678118654752440 : (real)1;
          a.dW = cc ? nullptr : grad + i[22]; a.dbias = !cc && i[23] >= 0 ? grad + i[23] : nullptr;
          a.part = reinterpret_cast<double*>(gw + o_part);
          a.wt = kw;
          if (jac) dqmc::launch_linear_jac<real>(st, a, jo, i[22], i[23]);
          else dqmc::launch_linear_bwd<real>(st, a);
          if (kf) {
            double* fA = kf->factors + k_fac_off[opi];
            dqmc::launch_kfac_factors<real>(st, a, i[23] >= 0, kw + B, fA, fA + kfac_dim_a(op) * kfac_dim_a(op),
                                            reinterpret_cast<double*>(gw + o_kpart));
          }
          t_end();
          break;
        }
        case DQMC_OP_SPIN_MEAN:
          dqmc::launch_spin_mean_bwd<real>(st, A(i[0]), A(i[1]), B, N, i[2], bufs[i[0]].width);
          break;
        case DQMC_OP_ROW_SUM:
          dqmc::launch_row_sum_bwd<real>(st, A(i[0]), A(i[1]), B, bufs[i[0]].rows, bufs[i[0]].width);
          break;
        case DQMC_OP_CONV: {
          const int* t = &g_tab_of[4 * opi];
          dqmc::launch_edge_rows_bwd<real>(st, A(i[0]), bufs[i[0]].rows, bufs[i[0]].width, bptr(i[1]), bufs[i[1]].rows, bufs[i[1]].width,
                                           A(i[2]), bufs[i[2]].width, i[3], gt + t[0], t[1], i[6], B, N, 1.0);
          dqmc::launch_conv_send_bwd<real>(st, A(i[1]), bufs[i[1]].rows, bufs[i[1]].width, bptr(i[0]), bufs[i[0]].rows, bufs[i[0]].width,
                                           A(i[2]), bufs[i[2]].width, i[3], gt + t[2], t[3], i[6], B, N);
          break;
        }
        case DQMC_OP_EDGE_SUM: {
          const int* t = &g_tab_of[4 * opi];
          dqmc::launch_edge_rows_bwd<real>(st, A(i[0]), bufs[i[0]].rows, bufs[i[0]].width, nullptr, 1, 4, A(i[2]), bufs[i[2]].width, i[3],
                                           gt + t[0], t[1], i[6], B, N, 1.0 / (double)(i[1] > 0 ? i[1] : 1));
          break;
        }
        case DQMC_OP_CONST:
          if (cc) break;
          if (jac) {
            dqmc::launch_jac_scatter<real, real>(st, A(i[0]), (long)bufs[i[0]].rows * bufs[i[0]].width, bufs[i[0]].rows * bufs[i[0]].width,
                                                 B, jo, i[1]);
            break;
          }
          if (kf && kf->rest)
            dqmc::launch_jac_scatter<real, real>(st, A(i[0]), (long)bufs[i[0]].rows * bufs[i[0]].width, bufs[i[0]].rows * bufs[i[0]].width,
                                                 B, ko, k_rest_pos[i[1]]);
          dqmc::launch_colsum<real>(st, A(i[0]), B, (long)bufs[i[0]].rows * bufs[i[0]].width, bufs[i[0]].rows * bufs[i[0]].width, grad + i[1],
                                    kw);
          break;
        case DQMC_OP_ORBITALS: {
          const int n_env = i[6] > 0 ? i[6] : 1, KN = sys.n_det * N, L = sys.n_nuc * n_env;
          double* pw = reinterpret_cast<double*>(gw + o_orb);
          t_begin("orbitals_bwd", 0);
          dqmc::launch_orbitals_bwd<real>(st, r, R, bptr(i[0]), bufs[i[0]].width, A(i[0]), A(i[1]), bufs[i[1]].width, d_w + i[2], d_w + i[3],
                                          d_w + i[4], d_w + i[5], cc ? nullptr : pw, B, N, sys.n_up, n_env, sys.n_nuc, sys.n_det,
                                          sys.norm_eps);
          if (cc) {
            dqmc::launch_orbitals_coords<real>(st, r, R, bptr(i[0]), bufs[i[0]].width, A(i[1]), bufs[i[1]].width, d_w + i[2], d_w + i[3],
                                               d_w + i[4], d_w + i[5], B, N, sys.n_up, n_env, sys.n_nuc, sys.n_det, sys.norm_eps,
                                               slot + 3 * (size_t)c_slot0[opi], c_n_slots);
            t_end();
            break;
          }
          for (int q = 0; q < 4; ++q) {
            if (jac) { dqmc::launch_jac_scatter<double, real>(st, pw + (size_t)q * KN * L, 4L * KN * L, KN * L, B, jo, i[2 + q]); continue; }
            if (kf && kf->rest) dqmc::launch_jac_scatter<double, real>(st, pw + (size_t)q * KN * L, 4L * KN * L, KN * L, B, ko, k_rest_pos[i[2 + q]]);
            dqmc::launch_colsum_f64(st, pw + (size_t)q * KN * L, B, 4L * KN * L, KN * L, grad + i[2 + q], kw);
          }
          t_end();
          break;
        }
        case DQMC_OP_SLOGDET:
          t_begin("slogdet_bwd", 0);
          dqmc::launch_slogdet_bwd<real>(st, bptr(i[0]), bufs[i[0]].width, dL, A(i[0]), B, sys.n_det, N);
          t_end();
          break;
        case DQMC_OP_FINAL: {
          dqmc::FinalBwdArgs<real> a{};
          a.r = r;
          a.logdet = reinterpret_cast<double*>(d_ws + off_logdet);
          a.sign_k = reinterpret_cast<int32_t*>(d_ws + off_signk);
          a.cc = i[1] >= 0 ? d_w + i[1] : nullptr;
          a.alphas = d_w + i[3];
          a.cusp_kind = i[2]; a.same_scale = op.f[0]; a.anti_scale = op.f[1]; a.eps = sys.norm_eps;
          a.logpsi = lp; a.sign = sg; a.cot = cot;
          a.djas = i[0] >= 0 ? A(i[0]) : nullptr;
          a.jas_ld = i[0] >= 0 ? bufs[i[0]].rows * bufs[i[0]].width : 0;
          a.dL = dL;
          a.pw = reinterpret_cast<double*>(gw + o_pw);
          a.B = B; a.N = N; a.n_up = sys.n_up; a.K = sys.n_det;
          dqmc::launch_final_bwd<real>(st, a);
          if (cc) {
            if (i[2])
              dqmc::launch_cusp_coords<real>(st, r, d_w + i[3], i[2], op.f[0], op.f[1], sys.norm_eps, B, N, sys.n_up,
                                             slot + 3 * (size_t)c_slot0[opi], c_n_slots);
            break;
          }
          if (jac) {
            if (i[1] >= 0) dqmc::launch_jac_scatter<double, real>(st, a.pw, sys.n_det + 2, sys.n_det, B, jo, i[1]);
            dqmc::launch_jac_scatter<double, real>(st, a.pw + sys.n_det, sys.n_det + 2, 2, B, jo, i[3]);
            break;
          }
          if (kf && kf->rest) {
            if (i[1] >= 0) dqmc::launch_jac_scatter<double, real>(st, a.pw, sys.n_det + 2, sys.n_det, B, ko, k_rest_pos[i[1]]);
            dqmc::launch_jac_scatter<double, real>(st, a.pw + sys.n_det, sys.n_det + 2, 2, B, ko, k_rest_pos[i[3]]);
          }
          if (i[1] >= 0) dqmc::launch_colsum_f64(st, a.pw, B, sys.n_det + 2, sys.n_det, grad + i[1], kw);
          dqmc::launch_colsum_f64(st, a.pw + sys.n_det, B, sys.n_det + 2, 2, grad + i[3], kw);
          break;
        }
        default:
          return fail(DQMC_E_UNSUPPORTED, "log_psi_vjp: op kind " + std::to_string(op.kind));
      }
    }
    if (cc)
      dqmc::launch_coords_gather<real>(st, slot, c_n_slots, (const int32_t*)c_tab.p, c_S, lp, sg, B, N, sys.n_nuc, cc->grad_r, cc->grad_R);
    HIP_TRY(hipGetLastError());
    return DQMC_OK;
  }
