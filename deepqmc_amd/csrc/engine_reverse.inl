// engine_reverse.inl -- member functions of Engine<real>, included INSIDE the struct body by engine.hip: the reverse pass of
// log|psi| that dqmc_log_psi_vjp, dqmc_log_psi_jacobian, dqmc_log_psi_kfac and dqmc_log_psi_grad_coords share, and of the
// Slater matrices themselves (dqmc_orbitals_vjp, dqmc_pretrain_loss_grad).  A request
// (RevReq) names one of five modes and that mode's outputs; reverse_pass() checks it, sizes the walker chunks and runs
// grad_chunk() on each.
//
// Per walker chunk: the per-op value pass (TP = 1, no fused kernel, no chained MLPs, so that every activation buffer the
// reverse pass reads is in memory), then the ops in reverse with adjoint buffers of the same shapes.  LINEAR recomputes its
// pre-activation Z = X W + b with the forward kernel (act = none) instead of storing it in the forward: the value pass
// stays the one dqmc_wf_eval runs, and one extra GEMM per layer costs less than the other two (dX, dW) each.  Weight
// gradients accumulate across chunks in double through fixed-order reductions (kernels_grad.inl).
//
// What the modes make of an op's per-walker parameter partials:
//   Vjp     sum_b cot[b] (...) into grad (the cotangent enters at FINAL).
//   Jac     unit cotangent; row b of jac[B][ld_jac] receives walker b's partials: LINEAR forms its weight blocks per walker
//           (kernels_jac.inl, no split-K reduction), CONST / ORBITALS / FINAL copy theirs (engine_jac.inl), and so does ATTENTION
//           for its constant key / value rows (option "nuclear_params"; in Kfac they are rest columns).
//   Kfac    unit cotangent, so every pre-activation adjoint is the dZ1 of G; cot is applied as a per-walker weight where
//           partials are summed over the walkers into grad.  After each LINEAR backward has formed dZ, the factor kernels
//           (kernels_kfac.inl) add A_l and G_l; partials of the entries no LINEAR op owns go to `rest` (engine_kfac.inl).
//   Coords  no parameter partials: LINEAR forms dX only, CONST is skipped, and the ops that read the coordinates carry their
//           adjoints into r and R (engine_coords.inl).
//   Orbs    as Vjp, but the cotangent enters at the ORBITALS destination buffer (given, or formed from the pretraining target
//           by the loss kernel): SLOGDET, FINAL and every op from which no path leads to that buffer are skipped
//           (engine_pretrain.inl: orb_tables), their gradient entries stay exact zeros.  No invalid-walker rule.

  enum class Rev { Vjp, Jac, Kfac, Coords, Orbs };
  static const char* rev_name(Rev m) {
    switch (m) {
      case Rev::Vjp: return "log_psi_vjp";
      case Rev::Jac: return "log_psi_jacobian";
      case Rev::Kfac: return "log_psi_kfac";
      case Rev::Orbs: return "orbitals_vjp";
      default: return "log_psi_grad_coords";
    }
  }
  // what one call (and, moved to walker b0 by at(), one chunk) asks of the reverse pass; only the fields of `mode` are read
  struct RevReq {
    Rev mode;
    real* logpsi = nullptr;      // [B], optional in every mode
    int32_t* sign = nullptr;     // [B], optional in every mode
    const real* cot = nullptr;   // Vjp, Kfac: [B] cotangents, or nullptr (ones)
    double* grad = nullptr;      // Vjp, Kfac: [n_weights], accumulated
    real* jac = nullptr;         // Jac: [B][ld_jac]
    size_t ld_jac = 0;
    double* factors = nullptr;   // Kfac: A_l, G_l of every LINEAR op, accumulated
    real* rest = nullptr;        // Kfac: [B][n_rest] partials of the entries no LINEAR op owns, or nullptr
    real* grad_r = nullptr;      // Coords: [B][N][3], or nullptr
    real* grad_R = nullptr;      // Coords: [B][n_nuc][3], or nullptr
    const real* cot_orb = nullptr;   // Orbs: [B][K][N][N] cotangent of the Slater matrices; nullptr: formed from the pretraining target
    real* orb = nullptr;         // Orbs: [B][K][N][N] Slater matrices of the value pass, or nullptr
    double* ps_loss = nullptr;   // Orbs without cot_orb: [B] per-walker pretraining loss
    double n_total = 1;          // Orbs without cot_orb: walkers the means of the loss run over
    template <class T> static T* adv(T* p, size_t n) { return p ? p + n : nullptr; }
    RevReq at(size_t b0, int N, int n_nuc, size_t n_rest, size_t n_orb) const {   // the same request for the chunk that starts at walker b0
      RevReq c = *this;
      c.logpsi = adv(logpsi, b0); c.sign = adv(sign, b0); c.cot = adv(cot, b0);
      c.jac = adv(jac, b0 * ld_jac); c.rest = adv(rest, b0 * n_rest);
      c.grad_r = adv(grad_r, b0 * N * 3); c.grad_R = adv(grad_R, b0 * n_nuc * 3);
      c.cot_orb = adv(cot_orb, b0 * n_orb); c.orb = adv(orb, b0 * n_orb); c.ps_loss = adv(ps_loss, b0);
      return c;
    }
  };

  // For its lifetime the value pass runs op by op with every activation in memory: no fused kernel, no chained MLPs.
  struct UnfusedForward {
    Engine& e;
    const int fused_saved;
    std::vector<int> child_saved;
    explicit UnfusedForward(Engine& e_) : e(e_), fused_saved(e_.fused_enabled) {
      child_saved.swap(e.mlp_child);
      e.mlp_child.assign(e.ops.size(), -1);
      e.fused_enabled = 0;
    }
    ~UnfusedForward() { e.fused_enabled = fused_saved; e.mlp_child.swap(child_saved); }
    UnfusedForward(const UnfusedForward&) = delete;
    UnfusedForward& operator=(const UnfusedForward&) = delete;
  };

  // Walkers per chunk under ws_budget: the workspace of grad_chunk per walker, and the part that does not grow with the chunk.
  // The modes differ on purpose (Coords reserves nothing for the split-K partials it never allocates).  Chunk boundaries fix
  // the order in which chunks add into grad and factors, so a change here moves results in the last bits.
  // nuc: the Coords mode also carries the nuclear stream's part into grad_R (nuc_coords_active): one adjoint arena per walker
  // (the table partials pw are part of grad_bytes_per_walker in every mode).
  long rev_chunk_len(Rev mode, int B, bool nuc = false) const {
    size_t per = ws_bytes_per_walker(1) + grad_bytes_per_walker(), fixed = 0;
    switch (mode) {
      case Rev::Vjp: case Rev::Jac: fixed = grad_part_bytes(); break;
      case Rev::Kfac: per += 2 * sizeof(double); fixed = grad_part_bytes() + kfac_part_bytes(); break;
      case Rev::Coords: per += sizeof(double) * (3 * (size_t)c_n_slots + (nuc ? nuc_arena : 0)); fixed = nuc ? sizeof(double) * nuc_arena : 0; break;
      case Rev::Orbs: per += pt_target_bytes_per_walker(); fixed = grad_part_bytes(); break;
    }
    const long chunk = per ? (long)((ws_budget > fixed ? ws_budget - fixed : 0) / per) : B;
    return chunk < 1 ? 1 : chunk;
  }

  // The caller has run its mode's plan (jac_plan, kfac_plan, coord_tables) and zeroed the accumulators it passes.
  int reverse_pass(const real* r, const real* R, int B, const RevReq& q) {
    const std::string name = rev_name(q.mode);
    if (B < 1) return fail(DQMC_E_ARG, "B must be positive");
    const bool per_walker = q.mode != Rev::Vjp && q.mode != Rev::Orbs;
    const bool coords = q.mode == Rev::Coords;
    const bool params = q.mode == Rev::Jac || q.mode == Rev::Kfac;      // (option "nuclear_params": the constant rows' and zeta tables'
    if (attention_refused(per_walker, coords, params))                  // partials go to their own jac / rest columns, per walker)
      return fail(DQMC_E_UNSUPPORTED, name + ": " + attention_refusal_text(per_walker, coords, params));
    const bool nuc = coords && nuc_coords_active(q.grad_R != nullptr);
    if (nuc && !nuc_fresh)
      return fail(DQMC_E_ARG, name + ": the nuclear stream's activations are older than the weights (dqmc_set_weights since the last "
                                     "dqmc_weights_from_params)");
    if (nuc && !nuc_coords_fits()) return fail(DQMC_E_UNSUPPORTED, name + ": a nuclear-stream layer's weight panel exceeds the LDS");
    if (q.mode != Rev::Orbs && N > dqmc::GRAD_GJ_NMAX) return fail(DQMC_E_UNSUPPORTED, name + ": more than 64 electrons");   // (Orbs forms no inverse)
    { const int rc = grad_tables(); if (rc) return rc; }
    if (q.mode == Rev::Orbs) { const int rc = orb_tables(); if (rc) return rc; }
    const long chunk = rev_chunk_len(q.mode, B, nuc);
    last_chunks[0] = chunk >= B ? 1 : (int)((B + chunk - 1) / chunk);
    const UnfusedForward unfused(*this);
    for (int b0 = 0; b0 < B; b0 += (int)chunk) {
      const int nb = (B - b0) < chunk ? (B - b0) : (int)chunk;
      const int rc = grad_chunk(r + (size_t)b0 * N * 3, R, nb, q.at(b0, N, sys.n_nuc, k_n_rest, (size_t)sys.n_det * N * N));
      if (rc) return rc;
    }
    HIP_TRY(hipGetLastError());
    return DQMC_OK;
  }

  int grad_chunk(const real* r, const real* R, int B, const RevReq& q) {
    const bool jac = q.mode == Rev::Jac, kfac = q.mode == Rev::Kfac, coords = q.mode == Rev::Coords, orbs = q.mode == Rev::Orbs;
    const bool nuc = coords && nuc_coords_active(q.grad_R != nullptr);      // the stream's part of grad_R (engine_nuc.inl: nuc_fold_coords)
    // adjoint workspace of this chunk
    std::vector<size_t> adj(bufs.size());
    Slab slab;
    for (size_t k = 0; k < bufs.size(); ++k) adj[k] = slab.take_bytes(sizeof(real) * (size_t)B * bufs[k].rows * bufs[k].width);
    const size_t adj_end = slab.bytes;
    const size_t o_z = slab.take_bytes(sizeof(real) * (size_t)B * grad_zrow()), o_dz = slab.take_bytes(sizeof(real) * (size_t)B * grad_zrow());
    const size_t o_dzs = slab.take_bytes(sizeof(real) * (size_t)B * max_ldw());
    const size_t o_orb = slab.take_bytes(sizeof(double) * (size_t)B * ((!coords || nuc) && grad_orb_partials() ? grad_orb_partials() : 1));
    const size_t o_dl = slab.take_bytes(sizeof(double) * (size_t)B * sys.n_det), o_pw = slab.take_bytes(sizeof(double) * (size_t)B * (sys.n_det + 2));
    const size_t o_lp = slab.take_bytes(sizeof(real) * (size_t)B), o_sg = slab.take_bytes(sizeof(int32_t) * (size_t)B);
    const size_t o_part = slab.take_bytes(coords ? 0 : grad_part_bytes());
    const size_t o_kw = slab.take_bytes(kfac ? sizeof(double) * 2 * (size_t)B : 0), o_kpart = slab.take_bytes(kfac ? kfac_part_bytes() : 0);
    const size_t o_slot = slab.take_bytes(coords ? sizeof(double) * 3 * (size_t)B * c_n_slots : 0);
    const size_t o_tgt = slab.take_bytes(orbs && !q.cot_orb ? (size_t)B * pt_target_bytes_per_walker() : 0);
    const size_t o_cpart = slab.take_bytes(sizeof(real) * (size_t)B * 2 * grad_att_const());      // (nuclear tokens: [B][2][n_const][H * hd])
    const size_t o_nuc = slab.take_bytes(nuc ? sizeof(double) * (size_t)B * nuc_arena : 0);      // [B][nuc_arena] adjoint arenas
    const size_t o_nucT = slab.take_bytes(nuc ? sizeof(double) * nuc_arena : 0);                 // act'(Z) of the stream's layers
    { const int rc = grad_ws_reserve(slab.bytes); if (rc) return rc; }
    char* gw = g_ws;
    double* nucG = nuc ? reinterpret_cast<double*>(gw + o_nuc) : nullptr;
    if (nuc) HIP_TRY(hipMemsetAsync(nucG, 0, sizeof(double) * (size_t)B * nuc_arena, st));
    auto A = [&](int b) { return reinterpret_cast<real*>(gw + adj[b]); };
    real* lp = q.logpsi ? q.logpsi : reinterpret_cast<real*>(gw + o_lp);
    int32_t* sg = q.sign ? q.sign : reinterpret_cast<int32_t*>(gw + o_sg);
    { const int rc = run_chunk(r, R, B, false, lp, sg, nullptr, nullptr, B, nullptr, 0); if (rc) return rc; }
    HIP_TRY(hipMemsetAsync(gw, 0, adj_end, st));
    if (orbs) {      // the cotangent enters at the ORBITALS destination buffer
      const int ob = dqmc::OrbitalsOp(ops[orb_op]).dst(), NN = N * N;
      const long rows = (long)B * sys.n_det;
      if (q.orb) dqmc::launch_orbitals_copy<real>(st, bptr(ob), bufs[ob].width, q.orb, NN, NN, rows);
      if (q.cot_orb) dqmc::launch_orbitals_copy<real>(st, q.cot_orb, NN, A(ob), bufs[ob].width, NN, rows);
      else {
        real* tgt = reinterpret_cast<real*>(gw + o_tgt);
        t_begin("pretrain_target", 0);
        pt_launch_target(r, R, B, tgt);
        t_end();
        t_begin("pretrain_loss", 0);
        dqmc::launch_pretrain_loss<real>(st, bptr(ob), bufs[ob].width, tgt, A(ob), q.ps_loss, B, N, sys.n_up, sys.n_det, pt_n_conf, q.n_total);
        t_end();
      }
    }
    // where per-walker partials go: rows of J (Jac), rows of rest (Kfac)
    const dqmc::JacOut<real> jo{q.jac, (long)q.ld_jac, lp, sg, jac_accum ? 1 : 0,
                                (q.ld_jac % 4 == 0 && (reinterpret_cast<uintptr_t>(q.jac) & 15) == 0) ? 1 : 0};
    const dqmc::JacOut<real> ko{q.rest, (long)k_n_rest, lp, sg, jac_accum ? 1 : 0, 0};
    if (jac) jac_zero_rows(q.jac, q.ld_jac, B);
    // Kfac: per-walker weights of the walker sums (cot, 0 for invalid walkers) and validity flags of the factors
    double* kw = kfac ? reinterpret_cast<double*>(gw + o_kw) : nullptr;
    if (kfac) {
      dqmc::launch_kfac_weights<real>(st, lp, sg, q.cot, kw, B);
      if (q.rest) kfac_zero_rest(q.rest, B);
    }
    // an op's per-walker parameter partials src[b * stride + m], m < n, of the weight entries w_off + m
    auto emit_partials = [&](const auto* src, long stride, int n, long w_off) {
      using T = std::remove_cv_t<std::remove_pointer_t<decltype(src)>>;
      switch (q.mode) {
        case Rev::Coords:      // no parameter partials; the nuclear stream's outputs keep theirs per walker
          if (nuc) nuc_gather_partials(src, stride, (long)n, w_off, nucG, B);
          return;
        case Rev::Jac: dqmc::launch_jac_scatter<T, real>(st, src, stride, n, B, jo, w_off); return;
        case Rev::Kfac:
          if (q.rest) dqmc::launch_jac_scatter<T, real>(st, src, stride, n, B, ko, k_rest_pos[w_off]);
          [[fallthrough]];
        case Rev::Vjp: case Rev::Orbs:
          if constexpr (std::is_same_v<T, real>) dqmc::launch_colsum<real>(st, src, B, stride, n, q.grad + w_off, kw);
          else dqmc::launch_colsum_f64(st, src, B, stride, n, q.grad + w_off, kw);
      }
    };
    const int32_t* gt = g_tab;
    double* dL = reinterpret_cast<double*>(gw + o_dl);
    double* slot = coords ? reinterpret_cast<double*>(gw + o_slot) : nullptr;   // coordinate-difference adjoints (kernels_coords.inl)
    for (size_t opi = ops.size(); opi-- > 0;) {
      const dqmc_op& op = ops[opi];
      const dqmc::OpViews v(op);
      if (orbs && !orb_live[opi]) continue;
      switch (op.kind) {
        case DQMC_OP_FEAT_EN:      // leaves: no parameters; only the coordinate mode carries their adjoints on
          if (coords)
            dqmc::launch_feat_en_coords<real>(st, r, R, A(v.feat_en.dst()), bufs[v.feat_en.dst()].width, B, N, sys.n_nuc, sys.norm_eps,
                                              v.feat_en.log_rescale(), slot + 3 * (size_t)c_slot0[opi], c_n_slots);
          break;
        case DQMC_OP_FEAT_EE:
          if (coords)
            dqmc::launch_feat_ee_coords<real>(st, r, R, d_it + v.feat_ee.table(), A(v.feat_ee.dst()), v.feat_ee.n_rows(), B, N, sys.norm_eps,
                                              v.feat_ee.log_rescale(), slot + 3 * (size_t)c_slot0[opi], c_n_slots);
          break;
        case DQMC_OP_LINEAR: {
          const dqmc::LinearOp& l = v.lin;
          // Z = X W + b with the forward kernel (no activation, no residual)
          dqmc::LinArgs<real> f{};
          f.cfg_bf = linear_bf; f.cfg_bkx = linear_bkx; f.cfg_f64_split = linear_f64_split;
          dqmc::LinBwdArgs<real> a{};
          f.n_pieces = a.n_pieces = l.n_pieces();
          lin_pieces(l, f.piece, true, [&](dqmc::LinPiece<real>& pc, int b) { pc.src = bptr(b); });
          lin_pieces(l, a.piece, false, [&](dqmc::LinBwdPiece<real>& pc, int b) { pc.X = bptr(b); pc.dX = A(b); });
          real* Z = reinterpret_cast<real*>(gw + o_z);
          f.W = d_w + l.w(); f.ldw = l.ldw(); f.bias = l.has_bias() ? d_w + l.bias() : nullptr;
          f.dst = Z; f.ld_dst = f.ldw; f.rpw_dst = l.nrows(); f.r0_dst = 0; f.col0_dst = 0;
          f.act = 0; f.nrows = l.nrows(); f.B = B; f.T = 1; f.TP = 1;
          t_begin(coords ? "linear_dx" : jac ? "linear_jac" : "linear_bwd", (coords ? 4.0 : 6.0) * B * l.nrows() * (double)l.w_rows() * f.ldw);     // Z recompute, dX, dW
          dqmc::launch_linear<real>(st, f);
          a.W = f.W; a.ldw = f.ldw; a.nout = l.nout(); a.nrows = l.nrows(); a.B = B; a.act = l.act();
          a.Z = Z; a.dZ = reinterpret_cast<real*>(gw + o_dz); a.dZs = reinterpret_cast<real*>(gw + o_dzs);
          lin_dst_res(l, a, a.dY, a.dres, A);
          if (!coords && !jac) { a.dW = q.grad + l.w(); a.dbias = l.has_bias() ? q.grad + l.bias() : nullptr; }   // else dX only
          a.part = reinterpret_cast<double*>(gw + o_part);
          a.wt = kw;
          if (jac) dqmc::launch_linear_jac<real>(st, a, jo, l.w(), l.bias());
          else dqmc::launch_linear_bwd<real>(st, a);
          if (kfac) {
            double* fA = q.factors + k_fac_off[opi];
            dqmc::launch_kfac_factors<real>(st, a, l.has_bias(), kw + B, fA, fA + l.kfac_dim_a() * l.kfac_dim_a(), reinterpret_cast<double*>(gw + o_kpart));
          }
          t_end();
          break;
        }
        case DQMC_OP_SPIN_MEAN:
          dqmc::launch_spin_mean_bwd<real>(st, A(v.spin_mean.src()), A(v.spin_mean.dst()), B, N, v.spin_mean.n_up(), bufs[v.spin_mean.src()].width);
          break;
        case DQMC_OP_ROW_SUM:
          dqmc::launch_row_sum_bwd<real>(st, A(v.row_sum.src()), A(v.row_sum.dst()), B, bufs[v.row_sum.src()].rows, bufs[v.row_sum.src()].width);
          break;
        case DQMC_OP_CONV: {
          const int* t = &g_tab_of[4 * opi];
          const dqmc::ConvOp& c = v.conv;
          const dqmc_buf &eb = bufs[c.edge()], &nb = bufs[c.node()];
          dqmc::launch_edge_rows_bwd<real>(st, A(c.edge()), eb.rows, eb.width, bptr(c.node()), nb.rows, nb.width, A(c.dst()), bufs[c.dst()].width,
                                           c.dst_col0(), gt + t[0], t[1], c.width(), B, N, 1.0);
          dqmc::launch_conv_send_bwd<real>(st, A(c.node()), nb.rows, nb.width, bptr(c.edge()), eb.rows, eb.width, A(c.dst()), bufs[c.dst()].width,
                                           c.dst_col0(), gt + t[2], t[3], c.width(), B, N);
          break;
        }
        case DQMC_OP_EDGE_SUM: {
          const int* t = &g_tab_of[4 * opi];
          const dqmc::EdgeSumOp& e = v.edge_sum;
          dqmc::launch_edge_rows_bwd<real>(st, A(e.edge()), bufs[e.edge()].rows, bufs[e.edge()].width, nullptr, 1, 4, A(e.dst()), bufs[e.dst()].width,
                                           e.dst_col0(), gt + t[0], t[1], e.width(), B, N, e.scale());
          break;
        }
        case DQMC_OP_ATTENTION: {    // dq, dk, dv are added into the adjoint buffers, the same in every mode; constant key / value
          const dqmc::AttentionOp& at = v.att;      // rows (Vjp, Orbs only) are weight entries: per-walker partials, summed below
          for (int x = 0; x < 4; ++x)
            for (int y = x + 1; y < 4; ++y)
              if (at.buf(x) == at.buf(y)) return fail(DQMC_E_UNSUPPORTED, std::string(rev_name(q.mode)) + ": ATTENTION op with shared q / k / v / dst buffers");
          t_begin("attention_bwd", 2.0 * B * at.heads() * (double)N * N * at.head_dim() * 5.0);
          const int nc = at.n_const(), HD = at.heads() * at.head_dim();
          real* cpart = reinterpret_cast<real*>(gw + o_cpart);
          const int rc2 = dqmc::launch_attention_bwd<real>(st, bptr(at.q()), bptr(at.k()), bptr(at.v()), A(at.dst()), A(at.q()), A(at.k()), A(at.v()),
                                                           bufs[at.q()].width, at.heads(), at.head_dim(), B, N, nc, nc ? d_w + at.const_k() : nullptr,
                                                           nc ? d_w + at.const_v() : nullptr, nc ? cpart : nullptr);
          if (rc2 == 0 && nc) {
            emit_partials((const real*)cpart, 2L * nc * HD, nc * HD, at.const_k());
            emit_partials((const real*)cpart + (size_t)nc * HD, 2L * nc * HD, nc * HD, at.const_v());
          }
          t_end();
          if (rc2 == -1) return fail(DQMC_E_UNSUPPORTED, std::string(rev_name(q.mode)) + ": attention backward tile set (N, head_dim) exceeds the LDS or the register tile");
          if (rc2) return fail(DQMC_E_HIP, "attention backward launch failed");
          break;
        }
        case DQMC_OP_CONST: {
          const dqmc_buf& cb = bufs[v.cst.dst()];
          emit_partials((const real*)A(v.cst.dst()), (long)cb.rows * cb.width, cb.rows * cb.width, v.cst.table());
          break;
        }
        case DQMC_OP_ORBITALS: {
          const dqmc::OrbitalsOp& o = v.orb;
          const int n_env = o.n_env(), KN = sys.n_det * N, L = sys.n_nuc * n_env;
          double* pw = reinterpret_cast<double*>(gw + o_orb);
          t_begin("orbitals_bwd", 0);
          dqmc::launch_orbitals_bwd<real>(st, r, R, bptr(o.src()), bufs[o.src()].width, A(o.src()), A(o.dst()), bufs[o.dst()].width, d_w + o.w(0),
                                          d_w + o.w(1), d_w + o.w(2), d_w + o.w(3), coords && !nuc ? nullptr : pw, B, N, sys.n_up, n_env, sys.n_nuc, sys.n_det,
                                          sys.norm_eps);
          if (coords)
            dqmc::launch_orbitals_coords<real>(st, r, R, bptr(o.src()), bufs[o.src()].width, A(o.dst()), bufs[o.dst()].width, d_w + o.w(0),
                                               d_w + o.w(1), d_w + o.w(2), d_w + o.w(3), B, N, sys.n_up, n_env, sys.n_nuc, sys.n_det, sys.norm_eps,
                                               slot + 3 * (size_t)c_slot0[opi], c_n_slots);
          for (int t = 0; t < 4; ++t) emit_partials((const double*)pw + (size_t)t * KN * L, 4L * KN * L, KN * L, o.w(t));
          t_end();
          break;
        }
        case DQMC_OP_SLOGDET:
          t_begin("slogdet_bwd", 0);
          dqmc::launch_slogdet_bwd<real>(st, bptr(v.slogdet.src()), bufs[v.slogdet.src()].width, dL, A(v.slogdet.src()), B, sys.n_det, N);
          t_end();
          break;
        case DQMC_OP_FINAL: {
          const dqmc::FinalOp& fin = v.fin;
          dqmc::FinalBwdArgs<real> a{};
          a.r = r;
          a.logdet = reinterpret_cast<double*>(d_ws + off_logdet);
          a.sign_k = reinterpret_cast<int32_t*>(d_ws + off_signk);
          a.cc = fin.has_conf_coeff() ? d_w + fin.conf_coeff() : nullptr;
          a.alphas = d_w + fin.alphas();
          a.cusp_kind = fin.cusp_kind(); a.same_scale = fin.same_scale(); a.anti_scale = fin.anti_scale(); a.eps = sys.norm_eps;
          a.logpsi = lp; a.sign = sg;
          a.cot = q.mode == Rev::Vjp ? q.cot : nullptr;      // every other mode runs a unit cotangent
          a.djas = fin.has_jastrow() ? A(fin.jastrow()) : nullptr;
          a.jas_ld = fin.has_jastrow() ? bufs[fin.jastrow()].rows * bufs[fin.jastrow()].width : 0;
          a.dL = dL;
          a.pw = reinterpret_cast<double*>(gw + o_pw);
          a.B = B; a.N = N; a.n_up = sys.n_up; a.K = sys.n_det;
          dqmc::launch_final_bwd<real>(st, a);
          if (coords && fin.cusp_kind())
            dqmc::launch_cusp_coords<real>(st, r, d_w + fin.alphas(), fin.cusp_kind(), fin.same_scale(), fin.anti_scale(), sys.norm_eps, B, N, sys.n_up,
                                           slot + 3 * (size_t)c_slot0[opi], c_n_slots);
          if (fin.has_conf_coeff()) emit_partials((const double*)a.pw, sys.n_det + 2, sys.n_det, fin.conf_coeff());
          emit_partials((const double*)a.pw + sys.n_det, sys.n_det + 2, 2, fin.alphas());
          break;
        }
        default:
          return fail(DQMC_E_UNSUPPORTED, std::string(rev_name(q.mode)) + ": op kind " + std::to_string(op.kind));
      }
    }
    if (coords)
      dqmc::launch_coords_gather<real>(st, slot, c_n_slots, c_tab, c_S, lp, sg, B, N, sys.n_nuc, q.grad_r, q.grad_R);
    if (nuc) {
      t_begin("nuc_coords", 0);
      const int rc = nuc_fold_coords(nucG, reinterpret_cast<double*>(gw + o_nucT), B, lp, sg, q.grad_R);
      t_end();
      if (rc) return rc;
    }
    HIP_TRY(hipGetLastError());
    return DQMC_OK;
  }
