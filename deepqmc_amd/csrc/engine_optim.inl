// engine_optim.inl -- member functions of Engine<real>, included INSIDE the struct body by engine.hip: the device-resident
// optimiser step (dqmc_set_param_map, dqmc_weights_from_params, dqmc_grad_to_params, dqmc_adam_step, dqmc_apply_update) and
// the test access to the weight buffers (dqmc_debug_read_weights, dqmc_graph_counters).
//
// A parameter vector theta (double, Program.grad_leaves order) lives in the caller's device memory.  The map src[j] says which
// element of it flat weight j is a copy of.  A device update writes d_w (and, in a float32 context, the double copy d_w64 a
// later twin starts from) from theta and re-packs the tape of the generated sub-step kernel and the planes of the fused
// kernel from d_w with one table-driven kernel each (kernels_optim.inl).  The tables are written by the host packers'
// own layout walks (spec_registry.hip: spec_tape_sources; engine_fused_plan.inl: walk_fused_weights), so a device re-pack
// is bit-identical to dqmc_set_weights from the same doubles.
//
// Captured forward-Laplacian graphs survive a device update: what a capture records is pointers (d_w, the workspace, the
// caller's buffers) and by-value arguments that are functions of the program, the options and the batch size -- never of a
// weight VALUE.  No buffer is reallocated here (d_w, d_wpk and d_tape keep their sizes), op_bf is decided from the shapes
// alone, and the refinement threshold is read from device memory.  graph_epoch therefore stays as it is.
//
// With a nuclear stream registered (engine_nuc.inl) a device update also folds the stream from theta and scatters the derived
// constants into d_w / d_w64 before the re-pack, and dqmc_grad_to_params ends with the stream's transpose.

  DevBuf<int32_t> d_pm_src;             // [n_weights] parameter element of every flat weight entry, -1: none
  DevBuf<int32_t> d_pm_row;             // [n_params + 1] transpose of the map, CSR: entries of element e are d_pm_col[row[e] .. row[e + 1])
  DevBuf<int32_t> d_pm_col;             // ascending within an element
  size_t pm_n_params = 0;
  std::vector<int32_t> pm_src_h;
  DevBuf<double> d_w64;                 // float32 contexts: the weights in double (what w64_h is to dqmc_set_weights)
  DevBuf<dqmc::PackSrc> d_tape_src;     // [tape words]
  DevBuf<dqmc::PackSrc> d_wpk_src;      // [wpk_len]
  size_t wpk_len = 0;
  std::vector<int32_t> tab_words;       // what the table of d_wpk_src was built for
  std::vector<char> tab_op_bf;
  DevBuf<double> d_opt_part;            // [3][OPT_MAX_BLOCKS] partial sums of the norms
  bool dev_ahead = false;               // the device weights are newer than wtmp / w64_h

  int set_param_map(const int32_t* src, size_t n, size_t n_params) override {
    if (n != n_weights) return fail(DQMC_E_ARG, "parameter map length differs from the weight buffer's");
    if (n_params < 1 || n_params > (size_t)INT32_MAX) return fail(DQMC_E_ARG, "bad number of parameters");
    for (size_t j = 0; j < n; ++j)
      if (src[j] < -1 || (src[j] >= 0 && (size_t)src[j] >= n_params))
        return fail(DQMC_E_ARG, "parameter map entry " + std::to_string(j) + " = " + std::to_string(src[j]) + " is out of range");
    HIP_TRY(hipStreamSynchronize(st));      // (a setup call: the tables below replace ones a running kernel may read)
    pm_src_h.assign(src, src + n);
    pm_n_params = n_params;
    std::vector<int32_t> row(n_params + 1, 0), col;
    for (size_t j = 0; j < n; ++j) if (src[j] >= 0) ++row[src[j] + 1];
    for (size_t e = 0; e < n_params; ++e) row[e + 1] += row[e];
    col.resize((size_t)row[n_params] ? (size_t)row[n_params] : 1);
    {
      std::vector<int32_t> at(row.begin(), row.end() - 1);
      for (size_t j = 0; j < n; ++j) if (src[j] >= 0) col[at[src[j]]++] = (int32_t)j;      // ascending j within an element
    }
    d_pm_src.reset(); d_pm_row.reset(); d_pm_col.reset();
    int rc = d_pm_src.assign(n ? n : 1);
    if (!rc) rc = d_pm_row.upload(row.data(), row.size());
    if (!rc) rc = d_pm_col.upload(col.data(), col.size());
    if (!rc) rc = d_opt_part.reserve((size_t)3 * dqmc::OPT_MAX_BLOCKS, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(d_pm_src, src, sizeof(int32_t) * n, hipMemcpyHostToDevice));
    if (sizeof(real) == 4 && !d_w64) {
      rc = d_w64.assign(n ? n : 1);
      if (rc) return rc;
      HIP_TRY(hipMemcpy(d_w64, w64_h.data(), sizeof(double) * n, hipMemcpyHostToDevice));
    }
    if constexpr (sizeof(real) == 4) {
      if (spec_k && d_tape && !d_tape_src) {
        std::vector<dqmc::PackSrc> tab((size_t)spec_k->tape_bytes / 4);
        dqmc::spec_tape_sources(*spec_k, tab.data());
        for (const auto& t : tab)
          if (t.src0 >= (long)n || t.src1 >= (long)n) return fail(DQMC_E_ARG, "weight tape refers to an entry beyond the weight buffer");
        rc = d_tape_src.upload(tab.data(), tab.size());
        if (rc) return rc;
      }
    }
    if (fused_n_ops > 0) { tab_words.clear(); rc = upload_fused_sources(); if (rc) return rc; }
    if (twin) return twin->set_param_map(src, n, n_params);
    return DQMC_OK;
  }

  // the table of d_wpk for the current plan (op_bf and the offsets of pack_fused_weights); kept while the plan stays
  int upload_fused_sources() {
    std::vector<int32_t> words;
    std::vector<dqmc::PackSrc> tab;
    walk_fused_weights(
        words, [&](long s0, long s1, int pl) { tab.push_back(dqmc::PackSrc{(int32_t)s0, (int32_t)s1, 1.0f, pl}); },
        [&](long s) { tab.push_back(dqmc::PackSrc{(int32_t)s, -1, 1.0f, -1}); });
    if (words == tab_words && op_bf == tab_op_bf && d_wpk_src) return DQMC_OK;
    for (const auto& t : tab)
      if (t.src0 >= (long)n_weights || t.src1 >= (long)n_weights) return fail(DQMC_E_ARG, "packed weights refer to an entry beyond the weight buffer");
    HIP_TRY(hipStreamSynchronize(st));
    { const int rc = d_wpk_src.reserve(tab.size(), st); if (rc) return rc; }
    if (!tab.empty()) HIP_TRY(hipMemcpy(d_wpk_src, tab.data(), sizeof(dqmc::PackSrc) * tab.size(), hipMemcpyHostToDevice));
    wpk_len = tab.size();
    tab_words = words; tab_op_bf = op_bf;
    return DQMC_OK;
  }
  // pack_fused_weights of a context whose host copy of the weights is stale (an option rebuilt the plan after a device update)
  int repack_fused_on_device() {
    tab_words.clear();
    int rc = upload_fused_sources();
    if (!rc) rc = d_wpk.reserve(wpk_len, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(d_wpk_off, tab_words.data(), sizeof(int32_t) * tab_words.size(), hipMemcpyHostToDevice));
    if (wpk_len) dqmc::launch_pack_words<real>(st, d_wpk_src, d_w, d_wpk, (long)wpk_len);
    HIP_TRY(hipStreamSynchronize(st));
    return DQMC_OK;
  }

  // tape and planes from d_w, in place, on the stream
  void repack_from_dw() {
    if constexpr (sizeof(real) == 4) {
      if (d_tape_src) dqmc::launch_pack_words<float>(st, d_tape_src, d_w, reinterpret_cast<float*>(d_tape.p), (long)spec_k->tape_bytes / 4);
    }
    if (fused_n_ops > 0 && wpk_len) dqmc::launch_pack_words<real>(st, d_wpk_src, d_w, d_wpk, (long)wpk_len);
  }

  int weights_from_params(const double* theta) override {
    if (!d_pm_src) return fail(DQMC_E_ARG, "no parameter map set (dqmc_set_param_map)");
    dqmc::launch_weights_from_params<real>(st, theta, d_pm_src, d_w, d_w64, (long)n_weights);
    if (nuc_set) nuc_fold_and_scatter(theta);      // (engine_nuc.inl: the constants of the nuclear stream, before the re-pack reads them)
    repack_from_dw();
    dev_ahead = true;
    if (twin) return twin->weights_from_params(theta);
    return DQMC_OK;
  }
  // a twin created after device updates: its host-side start (w64_h) is stale, the double copy on the device is not
  int load_weights_device(const double* w64) override {
    if constexpr (sizeof(real) == 8) {
      HIP_TRY(hipMemcpyAsync(d_w, w64, sizeof(double) * n_weights, hipMemcpyDeviceToDevice, st));
      repack_from_dw();
      dev_ahead = true;
      return DQMC_OK;
    }
    (void)w64;
    return fail(DQMC_E_UNSUPPORTED, "float64 contexts only");
  }
  int seed_twin_from_device() {
    if (!twin || !d_pm_src) return DQMC_OK;
    int rc = twin->set_param_map(pm_src_h.data(), pm_src_h.size(), pm_n_params);
    if (!rc && nuc_set) rc = twin->set_nuclear_stream(nuc_host_desc());
    if (!rc && dev_ahead) rc = twin->load_weights_device(d_w64);
    return rc;
  }

  int grad_to_params(const double* grad_w, double* grad_theta) override {
    if (!d_pm_src) return fail(DQMC_E_ARG, "no parameter map set (dqmc_set_param_map)");
    if (nuc_set && !nuc_fresh)
      return fail(DQMC_E_ARG, "dqmc_grad_to_params: the nuclear stream's activations are older than the weights (dqmc_set_weights since the "
                              "last dqmc_weights_from_params)");
    dqmc::launch_grad_to_params(st, grad_w, d_pm_row, d_pm_col, grad_theta, (long)pm_n_params);
    if (nuc_set) {      // the adjoints of the derived vector from the constant entries (ascending), then the stream's transpose
      dqmc::launch_grad_to_params(st, grad_w, d_nuc_row, d_nuc_col, d_nuc_adj, (long)nuc_n_derived);
      nuc_fold_vjp(grad_theta);
    }
    return DQMC_OK;
  }
  int adam_step(double* theta, double* mu, double* nu, const double* g, size_t n, double lr, double b1, double b2, double eps, int64_t t,
                double* norms3) override {
    if (!d_pm_src) return fail(DQMC_E_ARG, "no parameter map set (dqmc_set_param_map)");
    if (n != pm_n_params) return fail(DQMC_E_ARG, "parameter vector length differs from the map's n_params");
    if (t < 1) return fail(DQMC_E_ARG, "the Adam count t starts at 1");
    const double c1 = 1.0 - std::pow(b1, (double)t), c2 = 1.0 - std::pow(b2, (double)t);
    dqmc::launch_adam(st, theta, mu, nu, g, (long)n, lr, b1, b2, eps, c1, c2, d_opt_part, norms3);
    return weights_from_params(theta);
  }
  int apply_update(double* theta, const double* delta, double scale, double* norms3) override {
    if (!d_pm_src) return fail(DQMC_E_ARG, "no parameter map set (dqmc_set_param_map)");
    dqmc::launch_apply_update(st, theta, delta, scale, (long)pm_n_params, d_opt_part, norms3);
    return weights_from_params(theta);
  }

  // out == nullptr: the size of the buffer in bytes is the (positive) return value
  int debug_read_weights(int which, void* out, size_t bytes) override {
    const void* p = nullptr;
    size_t have = 0;
    if (which == 3) {
      if (!twin) return fail(DQMC_E_UNSUPPORTED, "this context has no float64 twin");
      return twin->debug_read_weights(0, out, bytes);
    }
    if (which == 0) { p = d_w; have = sizeof(real) * n_weights; }
    else if (which == 1) { if (d_tape && spec_k) { p = d_tape; have = (size_t)spec_k->tape_bytes; } }
    else if (which == 2) { if (d_wpk && fused_n_ops > 0) { p = d_wpk; have = sizeof(real) * wpk_len; } }
    else if (which == 4) { if (d_w64) { p = d_w64; have = sizeof(double) * n_weights; } }
    else return fail(DQMC_E_ARG, "which must be 0 (weights), 1 (tape), 2 (fused planes), 3 (the twin's weights) or 4 (the double copy)");
    if (!p) return fail(DQMC_E_UNSUPPORTED, "this context has no such buffer");
    if (!out) return (int)have;
    if (bytes != have) return fail(DQMC_E_ARG, "buffer of " + std::to_string(bytes) + " bytes for " + std::to_string(have));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(out, p, have, hipMemcpyDeviceToHost));
    return DQMC_OK;
  }
  void graph_counters(int64_t* out2) override { out2[0] = (int64_t)graph_captures; out2[1] = (int64_t)graph_hits; }
