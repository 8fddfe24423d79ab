// engine_nuc.inl -- member functions of Engine<real>, included INSIDE the struct body by engine.hip: the nuclear-token stream of
// the TransPsiformer on the device (dqmc_set_nuclear_stream, option "nuclear_reverse"; kernels_nuc.inl).
//
// The electron-independent stream (deepqmc_amd/nuclear_stream.py: nuclei embedding, per layer the token attention and MLP,
// the envelope head) is a function of theta and of the geometry the context was compiled for.  What the layer program reads of
// it are CONSTANTS of the weight buffer: the key / value rows of every ATTENTION op and the zeta tables of the simplified
// envelopes.  nuc_fold(theta) evaluates the stream in float64 (in a float32 context too) and writes
//   the derived vector   per layer K_nuc, V_nuc [n_nuc][D], then zetas up and down [n_nuc][K][n_env]   (the head of nuc_act)
//   every activation the backward needs                                                                  (the rest of nuc_act)
// and nuc_fold_vjp(grad_theta) is its transpose: from the adjoints of the derived vector (the head of nuc_adj) back through the
// envelope head, the layers in reverse -- layer l's K / V adjoints enter at that layer's key / value projections -- the embed
// MLP, the sender sum and the edge MLP, ADDING parameter gradients into grad_theta.  No adjoint of R.  Everything runs on the
// context's stream in a fixed order without atomics, allocates nothing and never waits for the host.
// With option "nuclear_coords" nuc_fold_coords runs the same chain once more for the Coords mode of the reverse pass: batched
// over the walkers of a chunk, adjoints only, and one step further, through the edge features into R (the end of this file).
//
// INVARIANT: constants and activations are always written together, by the same fold (weights_from_params: fold, scatter into
// d_w / d_w64, re-pack), and the fold keeps its own copy of the theta it ran on (the backward reads the weights from it).
// dqmc_set_weights writes constants folded on the host and therefore marks the activations stale: dqmc_grad_to_params refuses
// until the next dqmc_weights_from_params.

  struct NucLin { long w, b; int n_in, n_out, act; size_t z, y; };   // theta offsets (b -1: none); nuc_act offsets of Z and Y (act 0: the same)
  int nuclear_reverse = 0;       // option: the reverse pass admits constant key / value rows in the Vjp and Orbs modes
  int nuclear_coords = 0;        // option: the Coords mode admits them too and carries the stream's part of d log|psi| / dR (nuc_fold_coords)
  int nuclear_params = 0;        // option: the Jac and Kfac modes admit them, and the stream's parameter partials exist per walker (nuc_fold_rows)
  bool nuc_set = false, nuc_fresh = false;
  std::map<std::pair<long, long>, std::pair<long, long>> nuc_range_of;      // weight range -> derived elements with a copy in it
  int nuc_n = 0, nuc_L = 0, nuc_H = 0, nuc_D = 0, nuc_K = 0, nuc_ne = 0, nuc_n_edge = 0, nuc_n_embed = 0, nuc_n_mlp = 0;
  long nuc_zbias[2] = {-1, -1};
  std::vector<NucLin> nuc_lin;
  size_t nuc_n_derived = 0, nuc_arena = 0, nuc_o_F = 0, nuc_o_esum = 0, nuc_o_ln = 0, nuc_o_rstd = 0;
  std::vector<size_t> nuc_o_P, nuc_o_o;       // per layer: softmax weights [H][n][n] (adjoint: dS), attention output [n][D]
  DevBuf<double> d_nuc_act, d_nuc_adj, d_nuc_theta, d_nuc_R;
  DevBuf<int32_t> d_nuc_row, d_nuc_col, d_nuc_types;
  // host copy of the descriptor for a twin created later
  std::vector<dqmc_nuc_linear> nuc_lin_h;
  std::vector<int32_t> nuc_types_h, nuc_col_h;
  std::vector<int64_t> nuc_row_h;
  std::vector<double> nuc_R_h, nuc_theta_h;
  dqmc_nuc_stream nuc_desc_h{};

  size_t nuc_zeta_off(int spin) const { return (size_t)2 * nuc_L * nuc_n * nuc_D + (size_t)spin * nuc_n * nuc_K * nuc_ne; }
  int nuc_lin_layer0() const { return nuc_n_edge + nuc_n_embed; }
  int nuc_lin_head0() const { return nuc_lin_layer0() + nuc_L * (4 + nuc_n_mlp); }

  int set_nuclear_stream(const dqmc_nuc_stream* d) override {
    if (!d_pm_src) return fail(DQMC_E_ARG, "dqmc_set_nuclear_stream: no parameter map set (dqmc_set_param_map)");
    auto bad = [&](const std::string& m) { return fail(DQMC_E_ARG, "dqmc_set_nuclear_stream: " + m); };
    if (!d->lin || !d->nuc_types || !d->R || !d->sc_row || !d->sc_col || !d->theta) return bad("null table");
    const int n = d->n_nuc, L = d->n_layers, H = d->heads, D = d->dim, K = d->n_det, ne = d->n_env;
    if (n != sys.n_nuc || n < 1 || n > 64) return bad("n_nuc must be the context's and at most 64");
    if (L < 1 || H < 1 || D < 1 || D % H || K != sys.n_det || ne < 0) return bad("bad n_layers / heads / dim / n_det / n_env");
    if (d->n_edge_lin < 1 || d->n_embed_lin < 1 || d->n_mlp_lin < 1) return bad("every MLP needs a layer");
    const int n_lin = d->n_edge_lin + d->n_embed_lin + L * (4 + d->n_mlp_lin) + (ne ? 4 : 0);
    if (d->n_lin != n_lin) return bad("n_lin does not match the layer counts");
    int n_att = 0;
    for (const auto& o : ops)
      if (o.kind == DQMC_OP_ATTENTION) {
        const dqmc::AttentionOp a(o);
        if (a.n_const() != n || a.heads() != H || a.heads() * a.head_dim() != D) return bad("an ATTENTION op has other constant rows, heads or width");
        ++n_att;
      }
    if (n_att != L) return bad("n_layers differs from the number of ATTENTION ops");
    const long np = (long)pm_n_params;
    const long nz = (long)K * ne;
    // the chain of widths
    auto want = [&](int k, int n_in, int n_out) {
      const dqmc_nuc_linear& l = d->lin[k];
      return l.n_in == n_in && (n_out < 0 || l.n_out == n_out) && l.n_in >= 1 && l.n_out >= 1 && l.act >= 0 && l.act <= 2 && l.w >= 0 &&
             l.w + (long)l.n_in * l.n_out <= np && (l.b == -1 || (l.b >= 0 && l.b + l.n_out <= np));
    };
    int k = 0, width = 4 + n;
    for (int e = 0; e < d->n_edge_lin; ++e, ++k) { if (!want(k, width, -1)) return bad("edge MLP layer " + std::to_string(e)); width = d->lin[k].n_out; }
    for (int e = 0; e < d->n_embed_lin; ++e, ++k) { if (!want(k, width, e == d->n_embed_lin - 1 ? D : -1)) return bad("embed MLP layer " + std::to_string(e)); width = d->lin[k].n_out; }
    for (int l = 0; l < L; ++l) {
      for (int p = 0; p < 4; ++p, ++k) if (!want(k, D, D) || d->lin[k].act != 0) return bad("attention projection of layer " + std::to_string(l));
      width = D;
      for (int e = 0; e < d->n_mlp_lin; ++e, ++k) { if (!want(k, width, e == d->n_mlp_lin - 1 ? D : -1)) return bad("MLP of layer " + std::to_string(l)); width = d->lin[k].n_out; }
    }
    if (ne) {
      for (int p = 0; p < 4; ++p, ++k) if (!want(k, D, (int)nz) || d->lin[k].act != 0) return bad("readout of the envelope head");
      for (int s = 0; s < 2; ++s) { const long zb = s ? d->zbias_down : d->zbias_up; if (zb < 0 || zb + (long)n * nz > np) return bad("zetas_bias offset"); }
    }
    for (int t = 0; t < n; ++t) if (d->nuc_types[t] < 0 || d->nuc_types[t] >= n) return bad("atom type out of range");
    const size_t n_derived = (size_t)2 * L * n * D + (ne ? (size_t)2 * n * nz : 0);
    if ((size_t)d->n_derived != n_derived) return bad("n_derived differs from the stream's outputs");
    if (d->sc_row[0] != 0) return bad("scatter rows must start at 0");
    for (size_t e = 0; e < n_derived; ++e) if (d->sc_row[e + 1] < d->sc_row[e]) return bad("scatter rows must ascend");
    const int64_t n_col = d->sc_row[n_derived];
    if (n_col > (int64_t)INT32_MAX) return bad("too many scatter entries");
    for (int64_t c = 0; c < n_col; ++c) {
      if (d->sc_col[c] < 0 || (size_t)d->sc_col[c] >= n_weights) return bad("scatter entry beyond the weight buffer");
      if (pm_src_h[d->sc_col[c]] != -1) return bad("scatter entry is a copy of a parameter in the map");
    }
    HIP_TRY(hipStreamSynchronize(st));      // (a setup call)
    // host copy (a twin created later registers the same stream)
    nuc_lin_h.assign(d->lin, d->lin + n_lin);
    nuc_types_h.assign(d->nuc_types, d->nuc_types + n);
    nuc_R_h.assign(d->R, d->R + 3 * n);
    nuc_row_h.assign(d->sc_row, d->sc_row + n_derived + 1);
    nuc_col_h.assign(d->sc_col, d->sc_col + n_col);
    nuc_theta_h.assign(d->theta, d->theta + np);
    nuc_desc_h = *d;
    nuc_n = n; nuc_L = L; nuc_H = H; nuc_D = D; nuc_K = K; nuc_ne = ne;
    nuc_n_edge = d->n_edge_lin; nuc_n_embed = d->n_embed_lin; nuc_n_mlp = d->n_mlp_lin;
    nuc_zbias[0] = d->zbias_up; nuc_zbias[1] = d->zbias_down;
    nuc_n_derived = n_derived;
    nuc_range_of.clear();
    // the arena: derived vector first, then the activations
    size_t at = n_derived;
    auto take = [&](size_t m) { const size_t o = at; at += m; return o; };
    nuc_o_F = take((size_t)n * n * (4 + n));
    nuc_lin.assign(n_lin, NucLin{});
    for (int q = 0; q < n_lin; ++q) {
      const dqmc_nuc_linear& l = d->lin[q];
      NucLin& m = nuc_lin[q];
      m.w = l.w; m.b = l.b; m.n_in = l.n_in; m.n_out = l.n_out; m.act = l.act;
      const size_t rows = q < nuc_n_edge ? (size_t)n * n : (size_t)n;
      const int rel = q - nuc_lin_layer0();
      const int p = (rel >= 0 && q < nuc_lin_head0()) ? rel % (4 + nuc_n_mlp) : -1, lay = p >= 0 ? rel / (4 + nuc_n_mlp) : -1;
      if (p == 1 || p == 2) m.y = m.z = ((size_t)2 * lay + (p - 1)) * n * D;      // key, value: rows of the derived vector
      else { m.y = take(rows * l.n_out); m.z = l.act ? take(rows * l.n_out) : m.y; }
    }
    nuc_o_esum = take((size_t)n * nuc_lin[nuc_n_edge - 1].n_out);
    nuc_o_P.resize(L); nuc_o_o.resize(L);
    for (int l = 0; l < L; ++l) { nuc_o_P[l] = take((size_t)H * n * n); nuc_o_o[l] = take((size_t)n * D); }
    nuc_o_ln = take((size_t)n * D);
    nuc_o_rstd = take(n);
    nuc_arena = at;
    d_nuc_act.reset(); d_nuc_adj.reset(); d_nuc_theta.reset(); d_nuc_R.reset(); d_nuc_row.reset(); d_nuc_col.reset(); d_nuc_types.reset();
    std::vector<int32_t> row32(nuc_row_h.begin(), nuc_row_h.end());
    if (nuc_col_h.empty()) nuc_col_h.push_back(0);
    int rc = d_nuc_act.assign(nuc_arena);
    if (!rc) rc = d_nuc_adj.assign(nuc_arena);
    if (!rc) rc = d_nuc_theta.upload(nuc_theta_h.data(), nuc_theta_h.size());
    if (!rc) rc = d_nuc_R.upload(nuc_R_h.data(), nuc_R_h.size());
    if (!rc) rc = d_nuc_types.upload(nuc_types_h.data(), nuc_types_h.size());
    if (!rc) rc = d_nuc_row.upload(row32.data(), row32.size());
    if (!rc) rc = d_nuc_col.upload(nuc_col_h.data(), nuc_col_h.size());
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(d_nuc_act, 0, sizeof(double) * nuc_arena, st));
    dqmc::launch_nuc_edge_feat(st, d_nuc_R, d_nuc_types, sys.norm_eps, d_nuc_act + nuc_o_F, n);      // (of R and eps alone: once)
    nuc_set = true;
    // constants and activations from one fold, from now on
    nuc_fold_and_scatter(d_nuc_theta);
    repack_from_dw();
    dev_ahead = true;
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipGetLastError());
    if (twin) return twin->set_nuclear_stream(nuc_host_desc());
    return DQMC_OK;
  }
  const dqmc_nuc_stream* nuc_host_desc() {
    nuc_desc_h.lin = nuc_lin_h.data(); nuc_desc_h.nuc_types = nuc_types_h.data(); nuc_desc_h.R = nuc_R_h.data();
    nuc_desc_h.sc_row = nuc_row_h.data(); nuc_desc_h.sc_col = nuc_col_h.data(); nuc_desc_h.theta = nuc_theta_h.data();
    return &nuc_desc_h;
  }

  void nuc_run_linear(const NucLin& m, const double* X, int rows, const double* res) {
    double* a = d_nuc_act;
    const double* th = d_nuc_theta;
    dqmc::launch_nuc_linear(st, X, th + m.w, m.b >= 0 ? th + m.b : nullptr, a + m.z, a + m.y, res, rows, m.n_in, m.n_out, m.act);
  }
  // theta -> derived vector and activations (nuclear_stream.fold)
  void nuc_fold(const double* theta) {
    if (theta != d_nuc_theta.p) (void)hipMemcpyAsync(d_nuc_theta, theta, sizeof(double) * pm_n_params, hipMemcpyDeviceToDevice, st);
    double* a = d_nuc_act;
    const int n = nuc_n, D = nuc_D;
    const double* X = a + nuc_o_F;
    int q = 0;
    for (int e = 0; e < nuc_n_edge; ++e, ++q) { nuc_run_linear(nuc_lin[q], X, n * n, nullptr); X = a + nuc_lin[q].y; }
    dqmc::launch_nuc_sender_sum(st, X, a + nuc_o_esum, n, nuc_lin[q - 1].n_out);
    X = a + nuc_o_esum;
    for (int e = 0; e < nuc_n_embed; ++e, ++q) { nuc_run_linear(nuc_lin[q], X, n, nullptr); X = a + nuc_lin[q].y; }
    const double* h = X;
    for (int l = 0; l < nuc_L; ++l) {
      for (int p = 0; p < 3; ++p) nuc_run_linear(nuc_lin[q + p], h, n, nullptr);
      dqmc::launch_nuc_attention(st, a + nuc_lin[q].y, a + nuc_lin[q + 1].y, a + nuc_lin[q + 2].y, a + nuc_o_P[l], a + nuc_o_o[l], n, nuc_H, D / nuc_H);
      nuc_run_linear(nuc_lin[q + 3], a + nuc_o_o[l], n, h);
      const double* att = a + nuc_lin[q + 3].y;
      q += 4;
      X = att;
      for (int e = 0; e < nuc_n_mlp; ++e, ++q) { nuc_run_linear(nuc_lin[q], X, n, e == nuc_n_mlp - 1 ? att : nullptr); X = a + nuc_lin[q].y; }
      h = X;
    }
    if (nuc_ne) {
      dqmc::launch_nuc_layernorm(st, h, a + nuc_o_ln, a + nuc_o_rstd, n, D);
      for (int s = 0; s < 2; ++s, q += 2) {
        nuc_run_linear(nuc_lin[q], a + nuc_o_ln, n, nullptr);
        nuc_run_linear(nuc_lin[q + 1], a + nuc_o_ln, n, nullptr);
        dqmc::launch_nuc_glu(st, a + nuc_lin[q].y, a + nuc_lin[q + 1].y, d_nuc_theta + nuc_zbias[s], a + nuc_zeta_off(s), (long)n * nuc_K * nuc_ne);
      }
    }
    nuc_fresh = true;
  }
  void nuc_fold_and_scatter(const double* theta) {
    nuc_fold(theta);
    dqmc::launch_nuc_scatter<real>(st, d_nuc_act, d_nuc_row, d_nuc_col, d_w, sizeof(real) == 4 ? d_w64.p : nullptr, (long)nuc_n_derived);
  }

  void nuc_linear_bwd(const NucLin& m, size_t x_off, bool x_adj, int rows, long res_off, double* grad_theta) {
    double *a = d_nuc_act, *g = d_nuc_adj;
    if (res_off >= 0) dqmc::launch_nuc_add(st, g + res_off, g + m.y, (long)rows * m.n_out);
    dqmc::launch_nuc_linear_bwd(st, a + x_off, d_nuc_theta + m.w, a + m.z, g + m.y, g + m.z, x_adj ? g + x_off : nullptr, grad_theta + m.w,
                                m.b >= 0 ? grad_theta + m.b : nullptr, rows, m.n_in, m.n_out, m.act);
  }
  // The transpose of nuc_fold at the activations of the last fold.  The head of nuc_adj holds the adjoints of the derived
  // vector (grad_to_params gathers them); the rest is zeroed here and every kernel adds into it.
  void nuc_fold_vjp(double* grad_theta) {
    double *a = d_nuc_act, *g = d_nuc_adj;
    const int n = nuc_n, D = nuc_D;
    (void)hipMemsetAsync(g + nuc_n_derived, 0, sizeof(double) * (nuc_arena - nuc_n_derived), st);
    // where the stream's h of every layer lives: h_0 = the embed MLP's output, h_{l+1} = the last MLP layer's output of layer l
    std::vector<size_t> h_off(nuc_L + 1);
    h_off[0] = nuc_lin[nuc_lin_layer0() - 1].y;
    for (int l = 0; l < nuc_L; ++l) h_off[l + 1] = nuc_lin[nuc_lin_layer0() + (l + 1) * (4 + nuc_n_mlp) - 1].y;
    if (nuc_ne) {
      int q = nuc_lin_head0();
      for (int s = 0; s < 2; ++s, q += 2) {
        dqmc::launch_nuc_glu_bwd(st, a + nuc_lin[q].y, a + nuc_lin[q + 1].y, g + nuc_zeta_off(s), g + nuc_lin[q].y, g + nuc_lin[q + 1].y,
                                 grad_theta + nuc_zbias[s], (long)n * nuc_K * nuc_ne);
        nuc_linear_bwd(nuc_lin[q], nuc_o_ln, true, n, -1, grad_theta);
        nuc_linear_bwd(nuc_lin[q + 1], nuc_o_ln, true, n, -1, grad_theta);
      }
      dqmc::launch_nuc_layernorm_bwd(st, a + nuc_o_ln, a + nuc_o_rstd, g + nuc_o_ln, g + h_off[nuc_L], n, D);
    }
    for (int l = nuc_L; l-- > 0;) {
      const int q0 = nuc_lin_layer0() + l * (4 + nuc_n_mlp);
      const size_t att = nuc_lin[q0 + 3].y;
      for (int e = nuc_n_mlp; e-- > 0;)
        nuc_linear_bwd(nuc_lin[q0 + 4 + e], e ? nuc_lin[q0 + 4 + e - 1].y : att, true, n, e == nuc_n_mlp - 1 ? (long)att : -1, grad_theta);
      nuc_linear_bwd(nuc_lin[q0 + 3], nuc_o_o[l], true, n, (long)h_off[l], grad_theta);
      dqmc::launch_nuc_attention_bwd(st, a + nuc_lin[q0].y, a + nuc_lin[q0 + 1].y, a + nuc_lin[q0 + 2].y, a + nuc_o_P[l], g + nuc_o_o[l],
                                     g + nuc_o_P[l], g + nuc_lin[q0].y, g + nuc_lin[q0 + 1].y, g + nuc_lin[q0 + 2].y, n, nuc_H, D / nuc_H);
      for (int p = 0; p < 3; ++p) nuc_linear_bwd(nuc_lin[q0 + p], h_off[l], true, n, -1, grad_theta);
    }
    for (int e = nuc_n_embed; e-- > 0;) {
      const int q = nuc_n_edge + e;
      nuc_linear_bwd(nuc_lin[q], e ? nuc_lin[q - 1].y : nuc_o_esum, true, n, -1, grad_theta);
    }
    dqmc::launch_nuc_sender_sum_bwd(st, g + nuc_o_esum, g + nuc_lin[nuc_n_edge - 1].y, n, nuc_lin[nuc_n_edge - 1].n_out);
    for (int e = nuc_n_edge; e-- > 0;)
      nuc_linear_bwd(nuc_lin[e], e ? nuc_lin[e - 1].y : nuc_o_F, e > 0, n * n, -1, grad_theta);      // (the features have no adjoint: no dR)
  }

  // ---- option "nuclear_coords": the same transpose per walker, adjoints only, carried one step further into R ----
  // The Coords mode of the reverse pass (engine_reverse.inl) keeps the per-walker partials of the constant key / value rows and
  // of the zeta tables instead of dropping them: nuc_gather_partials sums each walker's partials over the copies of a derived
  // element into the head of that walker's adjoint arena G + b * nuc_arena (double, chunk workspace, zeroed by the caller; laid
  // out like nuc_adj, so nuc_lin[q].z / .y address walker b's dZ / dY of stream layer q for the lifetime of the chunk).
  // nuc_fold_coords then runs nuc_fold_vjp's chain on all arenas at once -- no parameter gradient, the number of launches does
  // not depend on B -- and adds the edge features' adjoint into grad_R at the registered geometry d_nuc_R.

  // derived elements [lo, hi) that have a copy among the weight entries [w0, w0 + len) (host tables; kept per range)
  std::pair<long, long> nuc_derived_range(long w0, long len) {
    const auto key = std::make_pair(w0, len);
    const auto it = nuc_range_of.find(key);
    if (it != nuc_range_of.end()) return it->second;
    long lo = (long)nuc_n_derived, hi = 0;
    for (long e = 0; e < (long)nuc_n_derived; ++e)
      for (int64_t k = nuc_row_h[e]; k < nuc_row_h[e + 1]; ++k)
        if (nuc_col_h[k] >= w0 && nuc_col_h[k] < w0 + len) { lo = std::min(lo, e); hi = std::max(hi, e + 1); }
    if (hi < lo) lo = hi = 0;
    return nuc_range_of[key] = std::make_pair(lo, hi);
  }
  // src[b * stride + m], m < len: walker b's partials of the weight entries w0 + m
  template <class T> void nuc_gather_partials(const T* src, long stride, long len, long w0, double* G, int B) {
    const auto range = nuc_derived_range(w0, len);
    dqmc::launch_nucb_gather<T>(st, src, stride, w0, len, d_nuc_row, d_nuc_col, range.first, range.second, G, (long)nuc_arena, B);
  }
  // every linear layer's W panel must fit the LDS of k_nucb_dx, the token attention's dS tile that of k_nucb_attention_bwd
  bool nuc_coords_fits() const {
    for (size_t q = 0; q < nuc_lin.size(); ++q)
      if (!dqmc::nucb_dx_col_tiles(q == 0 ? 4 : nuc_lin[q].n_in, nuc_lin[q].n_out)) return false;
    return dqmc::nucb_attention_bwd_lds_bytes(nuc_n) <= (size_t)160 * 1024;
  }
  int nuc_coords_linear(double* G, const double* T, int B, const NucLin& m, size_t x_off, int rows, long res_off, int k_cols) {
    const long A = (long)nuc_arena;
    if (res_off >= 0) dqmc::launch_nucb_add(st, G + res_off, G + m.y, (long)rows * m.n_out, A, B);
    return dqmc::launch_nucb_dx(st, G + m.y, m.act ? T + m.z : nullptr, d_nuc_theta + m.w, G + m.z, G + x_off, rows, B, m.n_in, m.n_out,
                                k_cols, A);
  }
  // T[nuc_lin[q].z ..] = act'(Z) of every activated layer q (T: nuc_arena doubles, shared by the walkers)
  void nuc_dact_table(double* T) {
    std::vector<int> act;
    std::vector<long> z, cnt;
    for (size_t q = 0; q < nuc_lin.size(); ++q)
      if (nuc_lin[q].act) {
        act.push_back(nuc_lin[q].act); z.push_back((long)nuc_lin[q].z);
        cnt.push_back(((int)q < nuc_n_edge ? (long)nuc_n * nuc_n : (long)nuc_n) * nuc_lin[q].n_out);
      }
    dqmc::launch_nucb_dact(st, d_nuc_act, T, act.data(), z.data(), cnt.data(), (int)act.size());
  }
  // The batched adjoint chain both per-walker routes share: from the adjoints of the derived vector (the head of every arena)
  // down to the edge features' adjoint at G + nuc_o_F.  Afterwards walker b's arena holds the pre-activation adjoint dZ of every
  // linear layer q at nuc_lin[q].z.  G: the walkers' adjoint arenas, T: nuc_arena doubles of scratch; x_of (or nullptr)
  // receives, per layer, the offset of its input X in nuc_act.  0, -1 (a weight panel exceeds the LDS) or -2 (HIP error).
  int nuc_fold_adjoints(double* G, double* T, int B, std::vector<size_t>* x_of) {
    const double* a = d_nuc_act;
    const int n = nuc_n, D = nuc_D;
    const long A = (long)nuc_arena;
    int rc = 0;
    nuc_dact_table(T);
    if (x_of) x_of->assign(nuc_lin.size(), 0);
    auto lin = [&](const NucLin& m, size_t x_off, int rows, long res_off, int k_cols) {
      if (x_of) (*x_of)[&m - nuc_lin.data()] = x_off;
      if (!rc) rc = nuc_coords_linear(G, T, B, m, x_off, rows, res_off, k_cols);
    };
    std::vector<size_t> h_off(nuc_L + 1);
    h_off[0] = nuc_lin[nuc_lin_layer0() - 1].y;
    for (int l = 0; l < nuc_L; ++l) h_off[l + 1] = nuc_lin[nuc_lin_layer0() + (l + 1) * (4 + nuc_n_mlp) - 1].y;
    if (nuc_ne) {
      int q = nuc_lin_head0();
      for (int s = 0; s < 2; ++s, q += 2) {
        dqmc::launch_nucb_glu_bwd(st, a + nuc_lin[q].y, a + nuc_lin[q + 1].y, G + nuc_zeta_off(s), G + nuc_lin[q].y, G + nuc_lin[q + 1].y,
                                  (long)n * nuc_K * nuc_ne, A, B);
        lin(nuc_lin[q], nuc_o_ln, n, -1, D);
        lin(nuc_lin[q + 1], nuc_o_ln, n, -1, D);
      }
      dqmc::launch_nucb_layernorm_bwd(st, a + nuc_o_ln, a + nuc_o_rstd, G + nuc_o_ln, G + h_off[nuc_L], n, D, A, B);
    }
    for (int l = nuc_L; l-- > 0;) {
      const int q0 = nuc_lin_layer0() + l * (4 + nuc_n_mlp);
      const size_t att = nuc_lin[q0 + 3].y;
      for (int e = nuc_n_mlp; e-- > 0;)
        lin(nuc_lin[q0 + 4 + e], e ? nuc_lin[q0 + 4 + e - 1].y : att, n, e == nuc_n_mlp - 1 ? (long)att : -1, nuc_lin[q0 + 4 + e].n_in);
      lin(nuc_lin[q0 + 3], nuc_o_o[l], n, (long)h_off[l], D);
      dqmc::launch_nucb_attention_bwd(st, a + nuc_lin[q0].y, a + nuc_lin[q0 + 1].y, a + nuc_lin[q0 + 2].y, a + nuc_o_P[l], G + nuc_o_o[l],
                                      G + nuc_lin[q0].y, G + nuc_lin[q0 + 1].y, G + nuc_lin[q0 + 2].y, n, nuc_H, D / nuc_H, A, B);
      for (int p = 0; p < 3; ++p) lin(nuc_lin[q0 + p], h_off[l], n, -1, D);
    }
    for (int e = nuc_n_embed; e-- > 0;) {
      const int q = nuc_n_edge + e;
      lin(nuc_lin[q], e ? nuc_lin[q - 1].y : nuc_o_esum, n, -1, nuc_lin[q].n_in);
    }
    dqmc::launch_nucb_sender_sum_bwd(st, G + nuc_o_esum, G + nuc_lin[nuc_n_edge - 1].y, n, nuc_lin[nuc_n_edge - 1].n_out, A, B);
    for (int e = nuc_n_edge; e-- > 0;)      // (of the features only the four columns of d carry an adjoint)
      lin(nuc_lin[e], e ? nuc_lin[e - 1].y : nuc_o_F, n * n, -1, e ? nuc_lin[e].n_in : 4);
    return rc;
  }
  // the chain, then through the edge features into R.  lp, sg [B]: rows of walkers with sign 0 or a non-finite log|psi| stay as
  // they are (zero)
  int nuc_fold_coords(double* G, double* T, int B, const real* lp, const int32_t* sg, real* grad_R) {
    const int rc = nuc_fold_adjoints(G, T, B, nullptr);
    if (rc) return rc == -1 ? fail(DQMC_E_UNSUPPORTED, "log_psi_grad_coords: a stream layer's weight panel exceeds the LDS")
                            : fail(DQMC_E_HIP, "nuclear-stream backward launch failed");
    dqmc::launch_nucb_edge_feat_bwd<real>(st, d_nuc_R, sys.norm_eps, G + nuc_o_F, nuc_n, (long)nuc_arena, lp, sg, grad_R, B);
    return DQMC_OK;
  }

  // ---- option "nuclear_params": the stream's parameter partials per walker ----
  // The stream's only parameters are the w / b of its linear layers and the two zetas_bias tables.  With dZ_q[b] from the chain
  // above and the shared activations X_q of the last fold, walker b's partials are dW_q[b] = X_q^T dZ_q[b], db_q[b] = colsum
  // dZ_q[b] (k_nucb_dw) and its adjoint of the zeta tables.  nuc_fold_rows gathers each walker's partials of the derived
  // elements from rows `src` (Jacobian rows over the weight buffer, or `rest` rows through the column table `col`), runs the
  // chain and then either ADDS the partials to the rows of out [B][ld] in theta order (store) or adds the sum of their squares
  // over the walkers into F [n_params] (sqF; `part`: the slice sums of the widest layer), in chunks of at most `cap` walkers
  // whose arenas are G (then T: nuc_arena doubles).  only: per theta element, 1 where sqF is wanted (host, or nullptr: all);
  // a layer is all or nothing.
  bool nuc_params_fits() const {
    if (!nuc_coords_fits()) return false;
    for (size_t q = 0; q < nuc_lin.size(); ++q)
      if (!dqmc::nucb_dw_fits((int)q < nuc_n_edge ? nuc_n * nuc_n : nuc_n)) return false;
    return true;
  }
  size_t nuc_params_part_doubles() const {
    size_t m = 1;
    for (const auto& l : nuc_lin) m = std::max(m, dqmc::nucb_dw_part_doubles(l.n_in, l.n_out));
    return m;
  }
  int nuc_params_check(const std::string& name) {
    if (!nuc_fresh)
      return fail(DQMC_E_ARG, name + ": the nuclear stream's activations are older than the weights (dqmc_set_weights since the last "
                                     "dqmc_weights_from_params)");
    if (!nuc_params_fits()) return fail(DQMC_E_UNSUPPORTED, name + ": a nuclear-stream layer exceeds the LDS");
    return DQMC_OK;
  }
  template <class T>
  int nuc_fold_rows(const std::string& name, const T* src, long stride, long len, const int32_t* col, int B, double* G, double* Tb, long cap,
                    real* out, long ld, double* sqF, double* part, const std::vector<uint8_t>* skip_lin) {
    { const int rc = nuc_params_check(name); if (rc) return rc; }
    const long A = (long)nuc_arena;
    std::vector<size_t> x_of;
    for (long b0 = 0; b0 < B; b0 += cap) {
      const int nb = (int)std::min<long>(cap, B - b0);
      HIP_TRY(hipMemsetAsync(G, 0, sizeof(double) * (size_t)nb * nuc_arena, st));
      dqmc::launch_nucb_gather<T>(st, src + b0 * stride, stride, 0, len, d_nuc_row, col, 0, (long)nuc_n_derived, G, A, nb);
      t_begin("nuc_rows_chain", 0);
      int rc = nuc_fold_adjoints(G, Tb, nb, &x_of);
      t_end();
      real* o = out ? out + b0 * ld : nullptr;
      t_begin("nucb_dw", 0);
      for (size_t q = 0; q < nuc_lin.size() && !rc; ++q) {
        if (skip_lin && (*skip_lin)[q]) continue;
        const NucLin& m = nuc_lin[q];
        const int rows = (int)q < nuc_n_edge ? nuc_n * nuc_n : nuc_n;
        if (out) rc = dqmc::launch_nucb_dw_store<real>(st, d_nuc_act + x_of[q], G + m.z, A, rows, m.n_in, m.n_out, nb, o, ld, m.w, m.b);
        else rc = dqmc::launch_nucb_dw_sqsum(st, d_nuc_act + x_of[q], G + m.z, A, rows, m.n_in, m.n_out, nb, sqF, m.w, m.b, part);
      }
      t_end();
      if (rc) return rc == -1 ? fail(DQMC_E_UNSUPPORTED, name + ": a nuclear-stream layer exceeds the LDS")
                              : fail(DQMC_E_HIP, "nuclear-stream backward launch failed");
      if (nuc_ne)
        for (int s = 0; s < 2; ++s) {
          const long nz = (long)nuc_n * nuc_K * nuc_ne;
          if (out) dqmc::launch_nucb_zbias_store<real>(st, G + nuc_zeta_off(s), A, nz, nb, o, ld, nuc_zbias[s]);
          else dqmc::launch_nucb_zbias_sqsum(st, G + nuc_zeta_off(s), A, nz, nb, sqF, nuc_zbias[s]);
        }
    }
    HIP_TRY(hipGetLastError());
    return DQMC_OK;
  }
  // dqmc_jacobian_to_params: the per-walker form of grad_to_params.  The arenas come from the gradient workspace under ws_budget.
  int jacobian_to_params(const void* jac, size_t ld_jac, int B, const void* logpsi, const int32_t* sign, void* jac_theta,
                         size_t ld_theta) override {
    const std::string name = "dqmc_jacobian_to_params";
    if (!d_pm_src) return fail(DQMC_E_ARG, "no parameter map set (dqmc_set_param_map)");
    if (B < 1) return fail(DQMC_E_ARG, name + ": B must be positive");
    if (ld_jac < n_weights) return fail(DQMC_E_ARG, name + ": ld_jac must be at least n_weights");
    if (ld_theta < pm_n_params) return fail(DQMC_E_ARG, name + ": ld_theta must be at least n_params");
    const bool nuc = nuc_set && grad_att_const() > 0;
    if (nuc && !nuclear_params)
      return fail(DQMC_E_UNSUPPORTED, name + ": " + attention_refusal_text(true));
    if (nuc) { const int rc = nuc_params_check(name); if (rc) return rc; }
    dqmc::launch_jac_to_params<real>(st, (const real*)jac, (long)ld_jac, d_pm_row, d_pm_col, (const real*)logpsi, sign, (real*)jac_theta,
                                     (long)ld_theta, (long)pm_n_params, B);
    last_chunks[0] = 1;
    if (nuc) {
      const size_t arena = sizeof(double) * nuc_arena;
      long cap = (long)((ws_budget > arena ? ws_budget - arena : 0) / arena);
      cap = cap < 1 ? 1 : cap > B ? B : cap;
      { const int rc = grad_ws_reserve(arena * ((size_t)cap + 1)); if (rc) return rc; }
      double* G = reinterpret_cast<double*>(g_ws.p);
      last_chunks[0] = (int)((B + cap - 1) / cap);
      const int rc = nuc_fold_rows<real>(name, (const real*)jac, (long)ld_jac, (long)n_weights, d_nuc_col, B, G, G + (size_t)cap * nuc_arena, cap,
                                         (real*)jac_theta, (long)ld_theta, nullptr, nullptr, nullptr);
      if (rc) return rc;
    }
    HIP_TRY(hipGetLastError());
    return DQMC_OK;
  }

  // dqmc_debug_nuc_dx_time (tools/nuclear_coords_time.py): the batched dX kernel against launch_linear_bwd<double> (dX only:
  // k_lin_dz, k_lin_dx) on the largest linear layer of the stream's token rows, B walkers, the layer's own weights and
  // pre-activations.  The two alternate `reps` times after a warm-up round; ms2 = their median times, shape3 = {B n, n_in, n_out}.
  int debug_nuc_dx_time(int B, int reps, double* ms2, int* shape3) override {
    if (!nuc_set || !nuc_fresh) return fail(DQMC_E_ARG, "dqmc_debug_nuc_dx_time: no folded nuclear stream");
    if (B < 1 || reps < 1) return fail(DQMC_E_ARG, "dqmc_debug_nuc_dx_time: B and reps must be positive");
    int best = nuc_lin_layer0();
    for (int q = best; q < nuc_lin_head0(); ++q) {
      const long sz = (long)nuc_lin[q].n_in * nuc_lin[q].n_out, sb = (long)nuc_lin[best].n_in * nuc_lin[best].n_out;
      if (sz > sb || (sz == sb && nuc_lin[q].act && !nuc_lin[best].act)) best = q;
    }
    const NucLin& m = nuc_lin[best];
    if (m.n_out % 4) return fail(DQMC_E_UNSUPPORTED, "dqmc_debug_nuc_dx_time: the reference kernel needs n_out % 4 == 0");
    const int n = nuc_n;
    const size_t ny = (size_t)B * n * m.n_out, nx = (size_t)B * n * m.n_in;
    const size_t A = (size_t)n * std::max(m.n_in, m.n_out);      // the walker stride of the batched kernel's three buffers
    { const int rc = grad_ws_reserve(sizeof(double) * (3 * ny + nx + 3 * (size_t)B * A + (size_t)n * m.n_out)); if (rc) return rc; }
    double* Y = reinterpret_cast<double*>(g_ws.p);
    double *Zb = Y + ny, *dZ = Zb + ny, *X2 = dZ + ny, *Y1 = X2 + nx, *dZ1 = Y1 + (size_t)B * A, *X1 = dZ1 + (size_t)B * A, *T1 = X1 + (size_t)B * A;
    for (int b = 0; b < B; ++b) {      // dY of both and the reference's per-walker Z: the layer's pre-activations
      const size_t bytes = sizeof(double) * n * m.n_out;
      HIP_TRY(hipMemcpyAsync(Y + (size_t)b * n * m.n_out, d_nuc_act + m.z, bytes, hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemcpyAsync(Zb + (size_t)b * n * m.n_out, d_nuc_act + m.z, bytes, hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemcpyAsync(Y1 + (size_t)b * A, d_nuc_act + m.z, bytes, hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(hipMemsetAsync(X2, 0, sizeof(double) * nx, st));
    HIP_TRY(hipMemsetAsync(X1, 0, sizeof(double) * B * A, st));
    dqmc::LinBwdArgs<double> a{};
    a.n_pieces = 1;
    a.piece[0].X = nullptr; a.piece[0].dX = X2; a.piece[0].ld = m.n_in; a.piece[0].rpw = n; a.piece[0].r0 = 0; a.piece[0].K = m.n_in;
    a.piece[0].bcast = 0; a.piece[0].w_row = 0;
    a.W = d_nuc_theta + m.w; a.ldw = m.n_out; a.nout = m.n_out; a.nrows = n; a.B = B; a.act = m.act;
    a.Z = Zb; a.dZ = dZ; a.dZs = nullptr; a.dY = Y; a.ld_dst = m.n_out; a.rpw_dst = n; a.r0_dst = 0; a.col0_dst = 0;
    const long zero = 0, tn = (long)n * m.n_out;
    std::vector<hipEvent_t> ev(3 * (size_t)(reps + 1));
    for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
    int rc = 0;
    for (int k = 0; k <= reps && !rc; ++k) {
      (void)hipEventRecord(ev[3 * k], st);
      if (m.act) dqmc::launch_nucb_dact(st, d_nuc_act + m.z, T1, &m.act, &zero, &tn, 1);      // (per call, not per layer: timed all the same)
      rc = dqmc::launch_nucb_dx(st, Y1, m.act ? T1 : nullptr, d_nuc_theta + m.w, dZ1, X1, n, B, m.n_in, m.n_out, m.n_in, (long)A);
      (void)hipEventRecord(ev[3 * k + 1], st);
      dqmc::launch_linear_bwd<double>(st, a);
      (void)hipEventRecord(ev[3 * k + 2], st);
    }
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<double> t1, t2;
    for (int k = 1; k <= reps; ++k) {      // (round 0 is the warm-up)
      float x = 0, y = 0;
      (void)hipEventElapsedTime(&x, ev[3 * k], ev[3 * k + 1]);
      (void)hipEventElapsedTime(&y, ev[3 * k + 1], ev[3 * k + 2]);
      t1.push_back(x); t2.push_back(y);
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    if (rc) return fail(DQMC_E_UNSUPPORTED, "dqmc_debug_nuc_dx_time: the layer's weight panel exceeds the LDS");
    std::sort(t1.begin(), t1.end()); std::sort(t2.begin(), t2.end());
    ms2[0] = t1[t1.size() / 2]; ms2[1] = t2[t2.size() / 2];
    shape3[0] = B * n; shape3[1] = m.n_in; shape3[2] = m.n_out;
    HIP_TRY(hipGetLastError());
    return DQMC_OK;
  }
