// engine_kfacopt.inl -- member functions of Engine<real>, included INSIDE the struct body by engine.hip: the KFAC
// preconditioner on the flat device vectors (dqmc_set_kfac_map, dqmc_kfac_state_size, dqmc_kfac_direction, dqmc_kfac_apply).
//
// dqmc_set_kfac_map checks the host tables against the factor layout of engine_kfac.inl and the parameter map of
// engine_optim.inl, inverts the row / column maps (the assembly kernel gathers, it never scatters), sorts the 2 n_mod matrices
// by dimension for the lockstep panel sequence of kernels_kfacopt.inl and reserves everything a direction needs: the device
// tables, the two matrix workspaces M (damped factors, updated in place) and L (their Cholesky factors), the scalars (n_v,
// pi per module).  Nothing here depends on the batch size, so dqmc_kfac_direction and dqmc_kfac_apply never allocate: they
// validate their arguments and enqueue kernels on the stream.  graph_epoch is not touched.
//
// The state's matrix part, M and L share one layout: A_hat then G_hat of every module in table order (mat_start).  Keeping the
// factors L in a buffer of their own, laid out like the state, is what lets a later inverse_update_period > 1 reuse them.

  DevBuf<char> kf_tab;                  // one allocation: every device table of KfTables
  DevBuf<double> kf_M, kf_L;            // [n_mat_elems] each
  DevBuf<double> kf_scal;               // [1 + n_mod]
  dqmc::KfTables kf_t{};
  std::vector<int> kf_active;           // [n_panels + 1] matrices with a panel k (prefix of the sorted list)
  int kf_max_n = 0, kf_max_da = 0, kf_max_dg = 0, kf_panels = 0;
  size_t kf_state = 0;
  bool kf_set = false;
  // option "nuclear_params": the stream's own parameters as diagonal elements (their o_bi through nuc_fold_rows, square-summed)
  bool kf_nuc = false;
  std::vector<uint8_t> kf_nuc_skip;     // per stream layer: 1 = a module covers it (no diagonal treatment)
  DevBuf<double> kf_nucG, kf_nucF, kf_nucPart;      // [kf_nuc_cap + 1] arenas, F over theta, the slice sums of k_nucb_dw
  DevBuf<int32_t> kf_nuc_col;           // d_nuc_col as rest columns
  long kf_nuc_cap = 0;

  // The stream's elements among the diagonal entries: a stream layer (zetas_bias table) no module covers must consist of entries
  // with an empty CSR row, and an empty row must belong to one.  Reserves what dqmc_kfac_direction needs of the stream.
  int set_kfac_map_nuc(const dqmc_kfac_map* hm, const std::vector<uint8_t>& in_module) {
    auto bad = [&](const std::string& what) { return fail(DQMC_E_ARG, "dqmc_set_kfac_map: " + what); };
    const long np = (long)pm_n_params, nd = (long)hm->n_diag;
    std::vector<uint8_t> stream((size_t)np, 0);
    kf_nuc_skip.assign(nuc_lin.size(), 0);
    auto claim = [&](long off, long n, bool& any_mod, bool& any_diag) {
      for (long e = off; e < off + n; ++e) { (in_module[e] ? any_mod : any_diag) = true; if (!in_module[e]) stream[e] = 1; }
    };
    bool some = false;
    for (size_t q = 0; q < nuc_lin.size(); ++q) {
      bool any_mod = false, any_diag = false;
      claim(nuc_lin[q].w, (long)nuc_lin[q].n_in * nuc_lin[q].n_out, any_mod, any_diag);
      if (nuc_lin[q].b >= 0) claim(nuc_lin[q].b, nuc_lin[q].n_out, any_mod, any_diag);
      if (any_mod && any_diag) return bad("a nuclear-stream layer is covered partly by a module, partly by diagonal entries");
      kf_nuc_skip[q] = any_mod ? 1 : 0;
      some = some || any_diag;
    }
    if (nuc_ne)
      for (int sp = 0; sp < 2; ++sp) {
        bool any_mod = false, any_diag = false;
        claim(nuc_zbias[sp], (long)nuc_n * nuc_K * nuc_ne, any_mod, any_diag);
        if (any_mod) return bad("a module covers zetas_bias entries");
        some = true;
      }
    for (long e = 0; e < nd; ++e) {
      const bool empty = hm->diag_row[e + 1] == hm->diag_row[e];
      if (stream[hm->diag_pos[e]] && !empty) return bad("a diagonal entry of the nuclear stream lists rest columns (its partials come through the stream)");
      if (!stream[hm->diag_pos[e]] && empty) return bad("a diagonal entry without rest columns is no parameter of the nuclear stream");
    }
    kf_nuc = some;
    if (!some) return DQMC_OK;
    std::vector<int32_t> col(nuc_col_h.size());
    for (size_t k = 0; k < col.size(); ++k) col[k] = (size_t)nuc_col_h[k] < n_weights ? (int32_t)k_rest_pos[nuc_col_h[k]] : -1;
    const size_t arena = sizeof(double) * nuc_arena;
    kf_nuc_cap = (long)std::min<size_t>(1024, std::max<size_t>(1, ((size_t)256 << 20) / arena));
    int rc = kf_nuc_col.upload(col.data(), col.size());
    if (!rc) rc = kf_nucG.assign(((size_t)kf_nuc_cap + 1) * nuc_arena);
    if (!rc) rc = kf_nucF.assign((size_t)np);
    if (!rc) rc = kf_nucPart.assign(nuc_params_part_doubles());
    return rc;
  }

  int set_kfac_map(const dqmc_kfac_map* hm) override {
    if (attention_refused(true, false, true)) return fail(DQMC_E_UNSUPPORTED, "dqmc_set_kfac_map: " + attention_refusal_text(true, false, true));
    if (N > dqmc::GRAD_GJ_NMAX) return fail(DQMC_E_UNSUPPORTED, "dqmc_set_kfac_map: more than 64 electrons");
    if (!d_pm_src) return fail(DQMC_E_ARG, "no parameter map set (dqmc_set_param_map)");
    { const int rc = kfac_plan(); if (rc) return rc; }
    const int nm = hm->n_modules, no = hm->n_ops;
    if (nm < 0 || no < 0 || (nm > 0 && (!hm->mod || !hm->op || !hm->maps)) || (hm->n_diag > 0 && (!hm->diag_pos || !hm->diag_row || !hm->diag_col)))
      return fail(DQMC_E_ARG, "dqmc_set_kfac_map: missing table");
    auto bad = [&](const std::string& what) { return fail(DQMC_E_ARG, "dqmc_set_kfac_map: " + what); };
    // the LINEAR ops of the context by the offset of their A_l
    std::map<long, std::pair<long, long>> lin;      // a_off -> (d_a, d_g)
    for (size_t k = 0; k < ops.size(); ++k)
      if (ops[k].kind == DQMC_OP_LINEAR) lin[(long)k_fac_off[k]] = {dqmc::LinearOp(ops[k]).kfac_dim_a(), dqmc::LinearOp(ops[k]).kfac_dim_g()};
    const long np = (long)pm_n_params;
    std::vector<uint8_t> covered((size_t)np, 0);
    std::vector<dqmc::KfMod> mods((size_t)nm);
    std::vector<dqmc::KfOp> kops((size_t)no);
    std::vector<int32_t> inv;
    std::vector<long> mat_start((size_t)2 * nm + 1, 0);
    std::vector<uint8_t> op_used((size_t)no, 0);
    long off = 0;
    kf_max_n = kf_max_da = kf_max_dg = 0;
    for (int m = 0; m < nm; ++m) {
      const int64_t* r = hm->mod + 8 * (size_t)m;
      const long n_in = r[0], n_out = r[1], hb = r[2], R = r[3], w_pos = r[4], b_pos = r[5], o0 = r[6], on = r[7];
      if (n_in < 1 || n_out < 1 || (hb != 0 && hb != 1) || R < 1 || on < 1 || o0 < 0 || o0 + on > no || n_in >= INT32_MAX / 2 || n_out >= INT32_MAX / 2)
        return bad("module " + std::to_string(m) + ": bad sizes");
      if (w_pos < 0 || w_pos + n_in * n_out > np || (hb ? (b_pos < 0 || b_pos + n_out > np) : b_pos != -1))
        return bad("module " + std::to_string(m) + ": parameter positions out of range");
      for (long e = w_pos; e < w_pos + n_in * n_out; ++e) if (covered[e]++) return bad("parameter element covered twice");
      if (hb) for (long e = b_pos; e < b_pos + n_out; ++e) if (covered[e]++) return bad("parameter element covered twice");
      const long da = n_in + hb, dg = n_out;
      dqmc::KfMod& M = mods[m];
      M.a_st = off; M.g_st = off + da * da; M.w_pos = w_pos; M.b_pos = b_pos;
      M.da = (int)da; M.dg = (int)dg; M.n_in = (int)n_in; M.R = (int)R; M.op0 = (int)o0; M.op1 = (int)(o0 + on);
      mat_start[2 * m] = M.a_st; mat_start[2 * m + 1] = M.g_st;
      off = M.g_st + dg * dg;
      kf_max_da = std::max(kf_max_da, (int)da); kf_max_dg = std::max(kf_max_dg, (int)dg);
      for (long q = o0; q < o0 + on; ++q) {
        if (op_used[q]++) return bad("op listed by two modules");
        const int64_t* o = hm->op + 6 * (size_t)q;
        const auto it = lin.find((long)o[0]);
        if (it == lin.end() || it->second.first != o[2] || it->second.second != o[3] || o[1] != o[0] + o[2] * o[2])
          return bad("op " + std::to_string(q) + " is not a LINEAR op of the factor layout (dqmc_kfac_layout)");
        if (o[4] < 0 || o[5] < 0 || (size_t)(o[4] + o[2]) > hm->n_maps || (size_t)(o[5] + o[3]) > hm->n_maps) return bad("op map out of range");
        dqmc::KfOp& K = kops[q];
        K.a_off = o[0]; K.g_off = o[1]; K.d_a = (int)o[2]; K.d_g = (int)o[3];
        for (int side = 0; side < 2; ++side) {      // invert: module row / column -> the op's
          const long d_op = side ? o[3] : o[2], d_mod = side ? dg : da;
          const int32_t* fw = hm->maps + (side ? o[5] : o[4]);
          const size_t base = inv.size();
          inv.resize(base + (size_t)d_mod, -1);
          for (long k = 0; k < d_op; ++k) {
            if (fw[k] < -1 || fw[k] >= d_mod) return bad("op map entry out of range");
            if (fw[k] < 0) continue;
            if (inv[base + fw[k]] >= 0) return bad("op map is not a permutation");
            inv[base + fw[k]] = (int32_t)k;
          }
          for (long i = 0; i < d_mod; ++i) if (inv[base + i] < 0) return bad("op map does not cover the module");
          if (base > (size_t)INT32_MAX) return bad("tables too large");
          (side ? K.inv_col : K.inv_row) = (int)base;
        }
      }
    }
    for (int q = 0; q < no; ++q) if (!op_used[q]) return bad("op belongs to no module");
    mat_start[2 * nm] = off;
    const long n_mat = off, nd = (long)hm->n_diag;
    const std::vector<uint8_t> in_module(covered);
    for (long e = 0; e < nd; ++e) {
      const long pos = hm->diag_pos[e], c0 = hm->diag_row[e], c1 = hm->diag_row[e + 1];
      if (pos < 0 || pos >= np || covered[pos]++) return bad("diagonal element out of range or covered twice");
      if (c0 < 0 || c1 < c0 || (e == 0 && c0 != 0)) return bad("diagonal CSR offsets are not ascending");
      for (long c = c0; c < c1; ++c)
        if (hm->diag_col[c] < 0 || (size_t)hm->diag_col[c] >= k_n_rest || (c > c0 && hm->diag_col[c] <= hm->diag_col[c - 1]))
          return bad("rest column out of range or not ascending");
    }
    for (long e = 0; e < np; ++e) if (!covered[e]) return bad("parameter element " + std::to_string(e) + " is covered by no module and no diagonal entry");
    // factorisation list: by dimension, descending (ties: table order)
    std::vector<dqmc::KfMat> mats((size_t)2 * nm);
    for (int q = 0; q < 2 * nm; ++q) { mats[q].ws = mat_start[q]; mats[q].n = (q & 1) ? mods[q >> 1].dg : mods[q >> 1].da; mats[q].pad = 0; }
    std::stable_sort(mats.begin(), mats.end(), [](const dqmc::KfMat& a, const dqmc::KfMat& b) { return a.n > b.n; });
    kf_max_n = nm ? mats[0].n : 0;
    kf_panels = (kf_max_n + dqmc::KF_NB - 1) / dqmc::KF_NB;
    kf_active.assign((size_t)kf_panels + 1, 0);
    for (int k = 0; k <= kf_panels; ++k)
      for (const auto& mt : mats) if (mt.n > k * dqmc::KF_NB) ++kf_active[k];
    // one device allocation for the tables
    HIP_TRY(hipStreamSynchronize(st));
    kf_set = false;
    kf_nuc = false;
    if (nuc_set && grad_att_const() > 0) { const int rc = set_kfac_map_nuc(hm, in_module); if (rc) return rc; }
    const size_t n_cols = nd ? (size_t)hm->diag_row[nd] : 0;
    auto up8 = [](size_t b) { return (b + 15) / 16 * 16; };
    size_t o_mod = 0, o_op = o_mod + up8(sizeof(dqmc::KfMod) * mods.size()), o_inv = o_op + up8(sizeof(dqmc::KfOp) * kops.size()),
           o_ms = o_inv + up8(sizeof(int32_t) * inv.size()), o_mats = o_ms + up8(sizeof(long) * mat_start.size()),
           o_dp = o_mats + up8(sizeof(dqmc::KfMat) * mats.size()), o_dr = o_dp + up8(sizeof(long) * (size_t)nd),
           o_dc = o_dr + up8(sizeof(long) * (size_t)(nd + 1)), total = o_dc + up8(sizeof(long) * n_cols);
    std::vector<char> blob(total ? total : 16, 0);
    auto put = [&](size_t o, const void* src, size_t bytes) { if (bytes) memcpy(blob.data() + o, src, bytes); };
    put(o_mod, mods.data(), sizeof(dqmc::KfMod) * mods.size());
    put(o_op, kops.data(), sizeof(dqmc::KfOp) * kops.size());
    put(o_inv, inv.data(), sizeof(int32_t) * inv.size());
    put(o_ms, mat_start.data(), sizeof(long) * mat_start.size());
    put(o_mats, mats.data(), sizeof(dqmc::KfMat) * mats.size());
    static_assert(sizeof(long) == sizeof(int64_t), "the host tables are copied as they are");
    put(o_dp, hm->diag_pos, sizeof(long) * (size_t)nd);
    if (nd) put(o_dr, hm->diag_row, sizeof(long) * (size_t)(nd + 1));
    put(o_dc, hm->diag_col, sizeof(long) * n_cols);
    int rc = kf_tab.upload(blob.data(), blob.size());
    if (!rc) rc = kf_M.assign((size_t)(n_mat ? n_mat : 1));
    if (!rc) rc = kf_L.assign((size_t)(n_mat ? n_mat : 1));
    if (!rc) rc = kf_scal.assign((size_t)(1 + nm));
    if (rc) return rc;
    char* base = kf_tab;
    kf_t.mod = (const dqmc::KfMod*)(base + o_mod); kf_t.op = (const dqmc::KfOp*)(base + o_op); kf_t.inv = (const int32_t*)(base + o_inv);
    kf_t.mat_start = (const long*)(base + o_ms); kf_t.mats = (const dqmc::KfMat*)(base + o_mats);
    kf_t.diag_pos = (const long*)(base + o_dp); kf_t.diag_row = (const long*)(base + o_dr); kf_t.diag_col = (const long*)(base + o_dc);
    kf_t.n_mod = nm; kf_t.n_diag = nd; kf_t.n_mat_elems = n_mat;
    kf_state = (size_t)(n_mat + nd);
    kf_set = true;
    return DQMC_OK;
  }

  int kfac_state_size(size_t* n_doubles) override {
    if (!kf_set) return fail(DQMC_E_ARG, "no KFAC map set (dqmc_set_kfac_map)");
    *n_doubles = kf_state;
    return DQMC_OK;
  }

  int kfac_direction(const double* g, const double* factors, const void* rest, const void* logpsi, const int32_t* sign, int B,
                     double* state, int first, double ema, double damping, double* delta, double* dot) override {
    if (!kf_set) return fail(DQMC_E_ARG, "no KFAC map set (dqmc_set_kfac_map)");
    if (B < 1) return fail(DQMC_E_ARG, "dqmc_kfac_direction: B must be positive");
    if (!(damping > 0)) return fail(DQMC_E_ARG, "dqmc_kfac_direction: damping must be positive");
    if (!(ema >= 0 && ema <= 1)) return fail(DQMC_E_ARG, "dqmc_kfac_direction: ema must lie in [0, 1]");
    if (kf_t.n_diag > 0 && !rest) return fail(DQMC_E_ARG, "dqmc_kfac_direction: the diagonal elements need `rest`");
    if (kf_nuc) {      // sum_b o_bi^2 of the stream's own parameters, from the rest rows through the stream
      HIP_TRY(hipMemsetAsync(kf_nucF, 0, sizeof(double) * pm_n_params, st));
      const int rc = nuc_fold_rows<real>("dqmc_kfac_direction", (const real*)rest, (long)k_n_rest, (long)k_n_rest, kf_nuc_col, B, kf_nucG,
                                         kf_nucG + (size_t)kf_nuc_cap * nuc_arena, kf_nuc_cap, nullptr, 0, kf_nucF, kf_nucPart, &kf_nuc_skip);
      if (rc) return rc;
    }
    HIP_TRY(hipMemcpyAsync(delta, g, sizeof(double) * pm_n_params, hipMemcpyDeviceToDevice, st));
    dqmc::KfacDirArgs a{};
    a.nuc_F = kf_nuc ? kf_nucF.p : nullptr;
    a.t = kf_t;
    a.g = g; a.factors = factors; a.rest = rest; a.n_rest = (long)k_n_rest; a.logpsi = logpsi; a.sign = sign; a.B = B;
    a.state = state; a.first = first ? 1 : 0; a.ema = ema; a.damping = damping;
    a.delta = delta; a.dot = dot;
    a.M = kf_M; a.L = kf_L; a.scal = kf_scal; a.part = d_opt_part;
    a.n_params = (long)pm_n_params;
    a.max_n = kf_max_n; a.max_da = kf_max_da; a.max_dg = kf_max_dg; a.n_panels = kf_panels;
    a.active = kf_active.data();
    dqmc::launch_kfac_direction<real>(st, a);
    return DQMC_OK;
  }

  int kfac_apply(double* theta, const double* delta, const double* dot, double lr, double norm_constraint, double* norms4) override {
    if (!d_pm_src) return fail(DQMC_E_ARG, "no parameter map set (dqmc_set_param_map)");
    dqmc::launch_kfac_apply(st, theta, delta, dot, lr, norm_constraint, (long)pm_n_params, d_opt_part, norms4);
    return weights_from_params(theta);
  }
